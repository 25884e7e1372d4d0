"""Expected values for the native-resolution views (xwb_xw_render_view, BatchedSimulator.render_view) and their pin to the
oracle: a view pushed through XWorldSimulator's resize(s) is the frame.  The helpers are what tests/test_gpu_view.py compares
the HIP kernels with; the tests here check the helpers themselves against the oracle alone, where no GPU is needed, and the
host side of the new verb (declarations, Python argument checks)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def canvas_from_grid(grid, icons64):
    """XMap::to_image(agent, false, 0), xmap.cpp:125-146: a white [64 D, 64 D, 3] canvas with icons64[code - 1] copied into every
    non-empty cell.  grid: [D, D] (or flat) cell codes, icon + 1, 0 = empty, target bit stripped."""
    g = np.asarray(grid)
    d = int(round(np.sqrt(g.size)))
    g = g.reshape(d, d)
    canvas = np.full((64 * d, 64 * d, 3), 255, np.uint8)
    for y in range(d):
        for x in range(d):
            if g[y, x]:
                canvas[64 * y:64 * (y + 1), 64 * x:64 * (x + 1)] = icons64[int(g[y, x]) - 1]
    return canvas


def _resize(oracle, a, out_px):
    a = np.ascontiguousarray(a)
    o = np.zeros((out_px, out_px, 3), np.uint8)
    oracle.lib().orc_cv_resize_linear_8u(a.ctypes.data_as(oracle.u8p), a.shape[0], a.shape[1], 3, o.ctypes.data_as(oracle.u8p), out_px, out_px)
    return o


def frame_from_view(oracle, view, world_px, out_px, color):
    """What XWorldSimulator::get_screen makes of a view: get_screen_rgb's resize of an egocentric view to the world's pixel size
    (64 * max_dim; a full-observation view has that size already), down_sample_image's resize to out_px, optional BGR2GRAY,
    planar output [c, out_px, out_px] (xworld_simulator.cpp:287-307, 508-545)."""
    a = np.ascontiguousarray(view)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[0] == a.shape[1] and a.shape[2] == 3
    if a.shape[0] != world_px:
        a = _resize(oracle, a, world_px)
    o = _resize(oracle, a, out_px)
    if not color:
        g = np.zeros((out_px, out_px), np.uint8)
        oracle.lib().orc_cv_bgr2gray_8u(o.ctypes.data_as(oracle.u8p), out_px * out_px, g.ctypes.data_as(oracle.u8p))
        return g[None]
    return np.ascontiguousarray(o.transpose(2, 0, 1))


FULL = {  # key: (subtrees attribute, oracle cfg)
    "nav7": ("NAV_SUBTREES", dict(map_kind=0, max_dim=7, dim=7, num_goals=4, num_blocks=16, tasks=["XWorld3DNavTarget"])),
    "nav8": ("NAV_SUBTREES", dict(map_kind=0, max_dim=8, dim=8, num_goals=4, num_blocks=16, tasks=["XWorld3DNavTarget"])),
    "nav8_dim5": ("NAV_SUBTREES", dict(map_kind=0, max_dim=8, dim=5, num_goals=2, num_blocks=6, tasks=["XWorld3DNavTarget"])),
    "walls7": ("WALLS_SUBTREES", dict(map_kind=1, max_dim=7, dim=7, num_goals=12, num_blocks=12, tasks=["XWorldNavTarget", "XWorldNavNear"])),
}


@pytest.mark.parametrize("color", [0, 1])
@pytest.mark.parametrize("key", list(FULL))
def test_canvas_through_the_resize_is_the_oracle_frame(oracle, key, color):
    sub, cfg = FULL[key]
    pal = oracle.Palette(getattr(oracle, sub))
    w = oracle.XWorld(pal, color=color, **cfg)
    frames = 0
    for e in range(6):
        w.reset_game(e, 0)
        for s in range(12):
            h = w.dims[0]
            got = frame_from_view(oracle, canvas_from_grid(w.grid(), pal.icons64), 64 * cfg["max_dim"], h, color)
            assert np.array_equal(got, w.screen()), (key, color, e, s)
            frames += 1
            w.take_actions(oracle.policy_action(1, e, s, w.num_actions()))
            if w.game_over():
                break
    assert frames >= 6


@pytest.mark.parametrize("color", [0, 1])
@pytest.mark.parametrize("r,md,blocks", [(1, 7, 6), (3, 7, 6), (5, 8, 6), (7, 7, 6), (9, 11, 30)])
def test_agent_view_through_the_resizes_is_the_oracle_frame(oracle, r, md, blocks, color):
    pal = oracle.Palette(oracle.NAV_SUBTREES)
    w = oracle.XWorld(pal, map_kind=0, max_dim=md, dim=md, num_goals=4, num_blocks=blocks, color=color, visible_radius=r,
                      tasks=["XWorld3DNavTarget"])
    assert w.dims[0] == r * (84 // r)
    frames = 0
    for e in range(4):
        w.reset_game(e, 0)
        for s in range(8):
            v = w.agent_view()
            assert v.shape == (64 * r, 64 * r, 3)
            got = frame_from_view(oracle, v, 64 * md, w.dims[0], color)
            assert np.array_equal(got, w.screen()), (r, md, color, e, s)
            frames += 1
            w.take_actions(oracle.policy_action(1, e, s, w.num_actions()))
            if w.game_over():
                break
    assert frames >= 4


def test_view_verb_is_declared_and_python_checks_arguments_first():
    """include/xwb.h declares, and xworld_amd.lib lists, both names; BatchedSimulator.render_view refuses a wrong `out` and a host
    index outside the batch before it touches the library (the object below has no library handle at all)."""
    import torch
    from xworld_amd import lib
    from xworld_amd.batched import BatchedSimulator
    header = open(os.path.join(ROOT, "include", "xwb.h")).read()
    declared = set(re.findall(r"\b(xwb_[a-z0-9_]+)\s*\(", header))
    for name in ("xwb_xw_view_dims", "xwb_xw_render_view"):
        assert name in declared and name in lib.EXPORTED_SYMBOLS, name
    sim = object.__new__(BatchedSimulator)
    sim.h = None                      # (close() / __del__ then have nothing to destroy)
    sim.L = None                      # any library call would raise AttributeError, not the errors expected below
    sim.num_envs, sim.device, sim._view_hwc = 8, 0, (448, 448, 3)
    for bad in ([0, 8], [-1], torch.tensor([3, 9]), 9, -1):
        with pytest.raises(IndexError):
            sim.render_view(bad)
    with pytest.raises(ValueError):
        sim.render_view(2, out=torch.zeros((2, 448, 448, 4), dtype=torch.uint8))          # shape
    with pytest.raises(ValueError):
        sim.render_view(2, out=torch.zeros((2, 448, 448, 3), dtype=torch.int8))           # dtype
    with pytest.raises(ValueError):
        sim.render_view([1, 2, 3], out=torch.zeros((2, 448, 448, 3), dtype=torch.uint8))  # one view short
    with pytest.raises(ValueError):
        sim.render_view(2, out=torch.zeros((2, 448, 448, 3), dtype=torch.uint8))          # not on the batch's device
