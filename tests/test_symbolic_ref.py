"""The symbolic-observation checker (tests/_symbolic_ref.py) against the oracle's own pixels, without a GPU: every 64-pixel
square of XMap::to_image -- agent_view() in egocentric mode, canvas_from_grid under full observation -- must look like what the
checker says the square shows.  Then the host side of the verb: declarations, exports, Python argument checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import _symbolic_ref as S
from test_view_expected import canvas_from_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS, STEPS = 120, 2                                      # seeded worlds per case; each looked at after its reset and after each step

# cv::warpAffine turns about (S/2, S/2) in pixel-INDEX coordinates, so an index v that is mirrored lands on S - v, not on
# S - 1 - v: the mirrored axes of the turned picture sit one pixel further down / right than np.rot90 puts them.  Rows are
# mirrored for k = 1, 2 quarter turns (facing right, down), columns for k = 2, 3 (facing down, left).
SHIFT = {0: (1, 0), 1: (1, 1), 2: (0, 1), 3: (0, 0)}        # facing dir -> (rows, columns)


def _turned_icon_interior(icon, fd):
    """what the interior [2:62, 2:62] of a frame square shows of a 64 x 64 item image, the agent facing fd"""
    t = np.rot90(icon, (fd + 1) % 4)
    dy, dx = SHIFT[fd]
    return t[2 - dy:62 - dy, 2 - dx:62 - dx]


def _check_squares(view, exp, pal, fd, where):
    """the rule of the issue, square by square; returns nothing, asserts"""
    s = exp.shape[1]
    assert view.shape == (64 * s, 64 * s, 3)
    for i in range(s):
        for j in range(s):
            sq = view[64 * i + 2:64 * i + 62, 64 * j + 2:64 * j + 62]
            kind, icon = int(exp[S.KIND, i, j]), int(exp[S.ICON, i, j])
            assert (int(sq.max()) == 0) == (kind == S.DARK), (where, i, j, kind)
            assert (int(sq.min()) == 255) == (kind == S.EMPTY), (where, i, j, kind)
            is_block_image = False
            for b in np.nonzero(pal.type_arr == 1)[0]:
                if np.array_equal(sq, _turned_icon_interior(pal.icons64[b], fd)):
                    is_block_image = True
                    assert kind == S.BLOCK and icon == b, (where, i, j, kind, icon, int(b))
            assert is_block_image == (kind == S.BLOCK), (where, i, j, kind)
            if kind in (S.EMPTY, S.DARK):
                assert icon == -1 and int(exp[S.NAME, i, j]) == -1
            else:
                assert pal.type_arr[icon] + 1 == kind and int(exp[S.NAME, i, j]) == pal.name_arr[icon]


@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "no_wall_shadow"])
@pytest.mark.parametrize("r", [1, 3, 5, 7])
def test_checker_against_the_oracles_egocentric_pixels(oracle, r, shadow):
    pal = oracle.Palette(oracle.NAV_SUBTREES)
    w = oracle.XWorld(pal, map_kind=0, max_dim=7, dim=7, num_goals=4, num_blocks=16, color=1, visible_radius=r,
                      no_wall_shadow=0 if shadow else 1, tasks=["XWorld3DNavTarget"], seed=77)
    met = {"shadow": 0, "outside": 0, S.EMPTY: 0, S.GOAL: 0, S.BLOCK: 0, S.AGENT: 0}
    headings = set()
    looked = 0
    for e in range(WORLDS):
        w.reset_game(e, 0)
        for s in range(STEPS + 1):
            exp, inside = S.expected(w, pal, detail=True)
            fd = S.facing(w.agent_yaw())
            headings.add(fd)
            assert exp.shape == (3, r, r) and exp.dtype == np.int16
            _check_squares(w.agent_view(), exp, pal, fd, (r, shadow, e, s))
            assert exp[S.KIND, r - 1, r // 2] == S.AGENT and int((exp[S.KIND] == S.AGENT).sum()) == 1   # bottom centre, nowhere else
            dark = exp[S.KIND] == S.DARK
            assert not (dark & inside).any() or shadow
            met["shadow"] += int((dark & inside).sum())
            met["outside"] += int((dark & ~inside).sum())
            assert not (~dark & ~inside).any()
            for k in (S.EMPTY, S.GOAL, S.BLOCK, S.AGENT):
                met[k] += int((exp[S.KIND] == k).sum())
            looked += 1
            if w.game_over():
                break
            w.take_actions(oracle.policy_action(5, e, s, w.num_actions()))
    assert headings == {0, 1, 2, 3} and looked > WORLDS
    if r >= 3 and shadow:
        assert all(v > 0 for v in met.values()), met
    if not shadow:
        assert met["shadow"] == 0


def _masking(is_block, ax, ay, fd, r):
    """XMap::image_masking (xmap.cpp:273-362) a second time, from the map alone: the window's origin on the map padded by r cells
    and shadow[window row][window column].  The agent stands in the window's last line along its heading, in the middle across
    it.  A ray runs from the agent to either side: what lies beyond a block on it starts its scan line in the dark; every scan
    line then runs away from the agent along the heading, and what lies beyond a block on it is dark."""
    ahead = {0: (1, 0), 1: (0, 1), 2: (-1, 0), 3: (0, -1)}[fd]
    across = (abs(ahead[1]), abs(ahead[0]))
    h = r // 2
    cx, cy = ax + r + ahead[0] * h, ay + r + ahead[1] * h                   # the window's centre cell, padded coordinates
    x_st, y_st = cx - h, cy - h
    lit = [True] * r                                                        # per scan line: it starts in the light
    for side in (-1, 1):
        blocked = False
        for k in range(1, h + 1):
            if blocked:
                lit[h + side * k] = False
            blocked = blocked or is_block(ax + side * k * across[0], ay + side * k * across[1])
    shadow = np.zeros((r, r), np.uint8)
    for t in range(r):
        blocked = not lit[t]
        for j in range(r):
            gx = ax + (t - h) * across[0] + j * ahead[0]
            gy = ay + (t - h) * across[1] + j * ahead[1]
            shadow[gy + r - y_st, gx + r - x_st] = blocked
            blocked = blocked or is_block(gx, gy)
    return x_st, y_st, shadow


@pytest.mark.parametrize("r", [13, 15])
def test_checker_and_masking_at_sixteen_cells(oracle, r):
    """16 x 16 maps at r = 13 and 15, where the oracle's egocentric render is the r = 3 code run further (unpinned by the
    reference): 36 views square by square against the checker, and the oracle's window and wall shadows against _masking above,
    which shares nothing with it but the map.  tests/test_gpu_ego_sizes.py rests on both at these sizes."""
    pal = oracle.Palette(oracle.NAV_SUBTREES)
    w = oracle.XWorld(pal, map_kind=0, max_dim=16, dim=16, num_goals=4, num_blocks=60, color=1, visible_radius=r,
                      tasks=["XWorld3DNavTarget"], seed=77)
    met = {"shadow": 0, "outside": 0, S.EMPTY: 0, S.GOAL: 0, S.BLOCK: 0, S.AGENT: 0}
    headings = set()
    for e in range(12):
        w.reset_game(e, 0)
        for s in range(STEPS + 1):
            exp, inside = S.expected(w, pal, detail=True)
            fd = S.facing(w.agent_yaw())
            headings.add(fd)
            planes = S.map_planes(w, pal)
            ax, ay = w.agent_xy()
            x_st, y_st, shadow = _masking(lambda x, y: 0 <= x < 16 and 0 <= y < 16 and planes[S.KIND, y, x] == S.BLOCK, ax, ay, fd, r)
            ox, oy, oshadow = w.agent_masking()
            assert (x_st, y_st) == (ox, oy) and np.array_equal(shadow, oshadow), (r, e, s, fd)
            _check_squares(w.agent_view(), exp, pal, fd, (r, e, s))
            assert exp[S.KIND, r - 1, r // 2] == S.AGENT and int((exp[S.KIND] == S.AGENT).sum()) == 1
            dark = exp[S.KIND] == S.DARK
            met["shadow"] += int((dark & inside).sum())
            met["outside"] += int((dark & ~inside).sum())
            for k in (S.EMPTY, S.GOAL, S.BLOCK, S.AGENT):
                met[k] += int((exp[S.KIND] == k).sum())
            w.take_actions(oracle.policy_action(5, e, s, w.num_actions()))
    assert headings == {0, 1, 2, 3} and all(v > 0 for v in met.values()), (headings, met)


@pytest.mark.parametrize("key", ["nav7", "nav8_dim5", "walls7"])
def test_checker_against_the_oracles_full_observation_pixels(oracle, key):
    from test_view_expected import FULL
    sub, cfg = FULL[key]
    pal = oracle.Palette(getattr(oracle, sub))
    w = oracle.XWorld(pal, color=1, seed=77, **cfg)
    d = cfg["max_dim"]
    met = {S.EMPTY: 0, S.GOAL: 0, S.BLOCK: 0, S.AGENT: 0}
    for e in range(WORLDS):
        w.reset_game(e, 0)
        for s in range(STEPS + 1):
            exp = S.expected(w, pal)
            assert exp.shape == (3, d, d) and not (exp[S.KIND] == S.DARK).any()
            _check_squares(canvas_from_grid(w.grid(), pal.icons64), exp, pal, 3, (key, e, s))
            ax, ay = w.agent_xy()
            assert exp[S.KIND, ay, ax] == S.AGENT and int((exp[S.KIND] == S.AGENT).sum()) == 1
            for k in met:
                met[k] += int((exp[S.KIND] == k).sum())
            if w.game_over():
                break
            w.take_actions(oracle.policy_action(5, e, s, w.num_actions()))
    assert all(v > 0 for v in met.values()), met
    if key == "nav8_dim5":                                  # the brick padding around the 5 x 5 map: blocks
        assert (exp[S.KIND, 0] == S.BLOCK).all() and (exp[S.KIND, :, 0] == S.BLOCK).all()


def test_unturn_is_the_counter_clockwise_quarter_turn():
    """the hand-written table of _symbolic_ref.unturn is np.rot90 by (facing + 1) quarter turns"""
    r = 5
    window = np.arange(r * r).reshape(r, r)
    for fd in range(4):
        turned = np.array([[window[S.unturn(fd, r, i, j)] for j in range(r)] for i in range(r)])
        assert np.array_equal(turned, np.rot90(window, (fd + 1) % 4)), fd
    assert S.show([[0, 1, 2], [3, 4, 0]]) == [".G#", "A ."]


def test_symbolic_verbs_are_declared_and_exported():
    """include/xwb.h declares both verbs and the enums, xworld_amd.lib binds them, the built library exports them under XWB_1"""
    from xworld_amd import batched, build, lib
    with open(os.path.join(ROOT, "include", "xwb.h")) as f:
        header = f.read()
    assert "int xwb_xw_symbolic_dims(const xwb_sim *sim, size_t *planes, size_t *rows, size_t *cols);" in header
    assert "int xwb_xw_symbolic(xwb_sim *sim, int16_t *out_dev, size_t out_bytes, void *stream);" in header
    assert "enum { XWB_SYM_EMPTY = 0, XWB_SYM_GOAL = 1, XWB_SYM_BLOCK = 2, XWB_SYM_AGENT = 3, XWB_SYM_DARK = 4 };" in header
    assert "enum { XWB_SYM_PLANE_KIND = 0, XWB_SYM_PLANE_ICON = 1, XWB_SYM_PLANE_NAME = 2, XWB_SYM_PLANES = 3 };" in header
    assert re.search(r"#define XWB_ABI_VERSION\s+%d\b" % lib.XWB_ABI_VERSION, header)
    for name in ("xwb_xw_symbolic", "xwb_xw_symbolic_dims"):
        assert name in lib.EXPORTED_SYMBOLS
    assert (batched.SYM_EMPTY, batched.SYM_GOAL, batched.SYM_BLOCK, batched.SYM_AGENT, batched.SYM_DARK) == (0, 1, 2, 3, 4)
    assert (batched.SYM_PLANE_KIND, batched.SYM_PLANE_ICON, batched.SYM_PLANE_NAME, batched.SYM_PLANES) == (0, 1, 2, 3)
    assert (S.EMPTY, S.GOAL, S.BLOCK, S.AGENT, S.DARK) == (0, 1, 2, 3, 4)
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    node = {line.split()[-1].split("@")[0]: line.split()[-1].split("@")[-1] for line in out.splitlines() if line.strip()}
    for name in ("xwb_xw_symbolic", "xwb_xw_symbolic_dims"):
        assert node.get(name) == "XWB_1", (name, node.get(name))


def test_python_checks_out_before_it_touches_the_library():
    """BatchedSimulator.symbolic refuses a wrong `out` without a library call (the object below has no handle at all)"""
    import torch
    from xworld_amd.batched import BatchedSimulator
    sim = object.__new__(BatchedSimulator)
    sim.h = None
    sim.L = None
    sim.num_envs, sim.device, sim._sym_dims = 8, 0, (3, 7, 7)
    for bad in (torch.zeros((8, 3, 7, 8), dtype=torch.int16), torch.zeros((8, 3, 7, 7), dtype=torch.int32),
                torch.zeros((7, 3, 7, 7), dtype=torch.int16), torch.zeros((8, 3, 7, 7), dtype=torch.int16), np.zeros((8, 3, 7, 7), np.int16)):
        with pytest.raises(ValueError):
            sim.symbolic(out=bad)
