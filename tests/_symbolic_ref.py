"""A plain-Python statement of what xwb_xw_symbolic (include/xwb.h) reports for ONE oracle world: the [3, S, S] planes KIND,
ICON, NAME of the squares of its newest frame, put together from pieces the oracle already exports -- grid(), entities(),
agent_xy(), agent_yaw(), agent_masking() (window origin and shadow flags of XMap::image_masking) and the palette's type and name
tables.  It shares no code with xworld_amd/; tests/test_symbolic_ref.py pins it to the oracle's own pixels, tests/
test_gpu_symbolic.py compares the kernel with it.

The quarter turn (xmap.cpp:196-200): the r x r window is turned with cv::getRotationMatrix2D(centre, 90 + yaw degrees) and
cv::warpAffine.  OpenCV's positive angle turns the picture counter-clockwise on the screen, so with k = (90 + yaw) / 90 quarter
turns, written out per cell (row i, column j of the turned frame <- row, column of the window):
    yaw   0  (facing +x, right)  k = 1    [i][j] <- [j][r - 1 - i]
    yaw  90  (facing +y, down)   k = 2    [i][j] <- [r - 1 - i][r - 1 - j]
    yaw 180  (facing -x, left)   k = 3    [i][j] <- [r - 1 - j][i]
    yaw 270  (facing -y, up)     k = 0    [i][j] <- [i][j]
(the pixel-exact warp puts the turned picture one pixel line off for k = 1, 2, 3: a square of the frame is one window cell's
image apart from that line).  The window is placed so that the agent stands in its last row / column along the heading, in the
middle across it: after the turn that is the bottom-centre square."""
import math

import numpy as np

EMPTY, GOAL, BLOCK, AGENT, DARK = 0, 1, 2, 3, 4
KIND, ICON, NAME = 0, 1, 2
CHARS = ".G#A "


def facing(yaw):
    """XItem::get_item_facing_dir, xitem.cpp:65-78: 0 right, 1 down, 2 left, 3 up"""
    eps = 1e-4
    if abs(yaw) < eps:
        return 0
    if abs(yaw - math.pi / 2) < eps:
        return 1
    if abs(yaw - math.pi) < eps:
        return 2
    return 3


def map_planes(world, pal):
    """[3, D, D] of the whole map, indexed [plane][y][x]: what full observation shows"""
    d = world.cfg.max_dim
    out = np.full((3, d, d), -1, np.int16)
    out[KIND] = EMPTY
    for etype, x, y, icon, _name, _serial in world.entities():             # stack order: the last item of a cell is the visible one
        out[KIND, y, x] = etype + 1
        out[ICON, y, x] = icon
        out[NAME, y, x] = pal.name_arr[icon]
        assert pal.type_arr[icon] == etype
    grid = world.grid()
    assert np.array_equal(out[ICON].astype(np.int32) + 1, grid), "entities() and grid() disagree"
    return out


def unturn(facing_dir, r, i, j):
    """(window row, window column) behind square [i][j] of the turned frame -- the table of the module docstring"""
    if facing_dir == 0:
        return j, r - 1 - i
    if facing_dir == 1:
        return r - 1 - i, r - 1 - j
    if facing_dir == 2:
        return r - 1 - j, i
    return i, j


def expected(world, pal, detail=False):
    """The [3, S, S] int16 observation of `world`.  detail=True: also a bool [S, S] array, True where the square lies inside the
    map (a DARK square inside the map is a wall's shadow, one outside is the black padding)."""
    planes = map_planes(world, pal)
    r = world.cfg.visible_radius
    d = world.cfg.max_dim
    if r == 0:
        return (planes, np.ones((d, d), bool)) if detail else planes
    x_st, y_st, shadow = world.agent_masking()
    if world.cfg.no_wall_shadow:                                            # xmap.cpp:170: if (FLAGS_wall_shadow)
        shadow = np.zeros_like(shadow)
    fd = facing(world.agent_yaw())
    out = np.full((3, r, r), -1, np.int16)
    inside = np.zeros((r, r), bool)
    for i in range(r):
        for j in range(r):
            wy, wx = unturn(fd, r, i, j)
            gx, gy = x_st - r + wx, y_st - r + wy                           # the window on the map padded by r cells
            inside[i, j] = 0 <= gx < d and 0 <= gy < d
            if inside[i, j] and not shadow[wy, wx]:
                out[:, i, j] = planes[:, gy, gx]
            else:
                out[KIND, i, j] = DARK
    return (out, inside) if detail else out


def show(kind_plane):
    """the KIND plane as lines of characters: '.' empty, 'G', '#', 'A', ' ' dark"""
    return ["".join(CHARS[int(v)] for v in row) for row in np.asarray(kind_plane)]
