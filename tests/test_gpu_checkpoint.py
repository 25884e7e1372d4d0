"""Checkpoint / resume (xwb_save_state / xwb_load_state): a batch resumed from a blob continues bit for bit."""
import os

import numpy as np
import pytest

from _blob import _blob_layout, _walk

pytestmark = pytest.mark.gpu

CONF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xworld_amd", "confs")
NAV = {"xwd_conf_path": os.path.join(CONF, "navigation2d.json"), "task_mode": "lang_acquisition", "max_dim": 7, "num_blocks": 16}
CASES = [
    ("simple_game", {"array_size": 16, "context": 2}),
    ("simple_race", {"track_width": 20.0, "track_length": 100.0, "track_radius": 30.0, "random": True}),
    ("xworld", dict(NAV, color=True, context=2)),
    ("xworld", dict(NAV, visible_radius=3, color=True)),
    ("xworld", {"xwd_conf_path": os.path.join(CONF, "walls.json"), "task_group": "XWorldNav", "task_mode": "one_channel", "max_steps": 50}),
]


def _run(sim, steps, autoreset):
    import torch
    out = []
    for t in range(steps):
        if autoreset:
            sim.step_autoreset()
        else:
            sim.reset_done()
            sim.step()
        out.append((sim.reward.clone(), sim.game_over_codes.clone(), sim.obs.clone(), sim.num_steps.clone()))
        # num_steps is a state array: xwb_reset_done may start the next episode of a finished env on its internal queue before
        # reads queued on this stream have run (include/xwb.h; outputs are ordered -- tests/test_gpu_stream_order.py)
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("game,opts", CASES, ids=lambda v: v if isinstance(v, str) else ("ego" if v.get("visible_radius") else str(len(v))))
@pytest.mark.parametrize("autoreset", [False, True])
def test_resume_is_bit_exact(game, opts, autoreset):
    import torch
    assert torch.cuda.is_available()
    from xworld_amd.batched import BatchedSimulator
    n = 1024
    a = BatchedSimulator(game, opts, num_envs=n, seed=5, policy_seed=9)
    _run(a, 40, autoreset)
    blob = a.save_state(include_obs=True)
    ref = _run(a, 25, autoreset)
    b = BatchedSimulator(game, opts, num_envs=n, seed=5, policy_seed=9)      # a fresh batch resumes from the blob
    b.load_state(blob)
    got = _run(b, 25, autoreset)
    for t, (x, y) in enumerate(zip(ref, got)):
        for u, v in zip(x, y):
            assert torch.equal(u, v), t
    a.load_state(blob)                                                        # and the original rewinds
    got = _run(a, 25, autoreset)
    assert all(torch.equal(u, v) for x, y in zip(ref, got) for u, v in zip(x, y))
    a.close()
    b.close()


def test_resume_without_obs_and_config_check():
    import torch
    from xworld_amd.batched import BatchedSimulator
    from xworld_amd.lib import XwbError
    opts = dict(NAV, color=True)
    a = BatchedSimulator("xworld", opts, num_envs=512, seed=1)
    _run(a, 30, False)
    small = a.save_state(include_obs=False)
    full = a.save_state(include_obs=True)
    assert small.size < full.size // 50
    ref = _run(a, 10, False)
    b = BatchedSimulator("xworld", opts, num_envs=512, seed=1)
    b.load_state(small)                                                       # context 1: frames re-rendered from the state
    got = _run(b, 10, False)
    assert all(torch.equal(u, v) for x, y in zip(ref, got) for u, v in zip(x, y))
    c = BatchedSimulator("xworld", opts, num_envs=512, seed=2)                # another seed: another configuration
    with pytest.raises(XwbError):
        c.load_state(small)
    with pytest.raises(XwbError):
        c.load_state(small[:100])
    for s in (a, b, c):
        s.close()


def _same(torch, a, b, where):
    torch.cuda.synchronize()
    for key in ("obs", "reward", "game_over_codes", "num_steps", "episode", "grid"):
        assert torch.equal(getattr(a, key), getattr(b, key)), (where, key)


def test_load_between_fused_step_and_reset_done():
    """A blob saved between a one-launch step and its reset_done, loaded right away: the reset_done that follows must not wait
    for the step's hand-over (nothing of that step is pending after a load), and the batch goes on as one on the classic path."""
    import torch
    from xworld_amd.batched import BatchedSimulator
    n = 1024
    a = BatchedSimulator("xworld", dict(NAV, color=True), num_envs=n, seed=3, policy_seed=4)
    b = BatchedSimulator("xworld", dict(NAV, color=True, debug=["no_fused", "no_pregen"]), num_envs=n, seed=3, policy_seed=4)
    for s in (a, b):
        s.reset()
        for _ in range(6):
            s.step()
            s.reset_done()
        s.step()
    assert a.step_path()["path"] == "lazy_fused" and b.step_path()["path"] == "classic"
    for s in (a, b):
        s.load_state(s.save_state())
        s.reset_done()
        assert s.check_errors() == 0                                          # (a poisoned batch raises here)
    assert a.step_path()["path"] == "lazy_fused"
    _same(torch, a, b, "after reset_done")
    for t in range(8):
        for s in (a, b):
            s.step()
            s.reset_done()
        _same(torch, a, b, t)
    assert a.check_errors() == b.check_errors() == 0
    a.close()
    b.close()


def test_refused_load_leaves_the_batch_alone():
    """A truncated blob is refused, and the batch that refused it keeps stepping exactly as a twin that never saw it."""
    import torch
    from xworld_amd.batched import BatchedSimulator
    from xworld_amd.lib import XwbError
    n = 1024
    a, b = (BatchedSimulator("xworld", dict(NAV, color=True), num_envs=n, seed=8, policy_seed=2) for _ in range(2))
    for s in (a, b):
        s.reset()
        for _ in range(5):
            s.step()
            s.reset_done()
        s.step()                                                              # (the done list rotation is mid-way)
    blob = a.save_state()
    with pytest.raises(XwbError):
        a.load_state(blob[:blob.size - 100])
    for t in range(10):
        for s in (a, b):
            s.reset_done()
            s.step()
        _same(torch, a, b, t)
    assert a.check_errors() == b.check_errors() == 0
    a.close()
    b.close()


TWO_GROUPS = {"xwd_conf_path": os.path.join(CONF, "nav_two_groups.json"), "max_steps": 50, "max_dim": 7, "num_blocks": 16}
LAYOUTS = {
    "simple_game": ("simple_game", {"array_size": 16, "context": 2}, dict(simple_game=True), 2 * 16),
    "simple_race": ("simple_race", {"track_width": 20.0, "track_length": 100.0, "track_radius": 30.0}, dict(simple_race=True), 4 * 4),
    "xworld_full": ("xworld", dict(NAV, color=True, context=2), dict(cells=49), 2 * 3 * 84 * 84),
    "xworld_ego": ("xworld", dict(NAV, visible_radius=3, color=True), dict(cells=49, ego=True), 3 * 84 * 84),
    "xworld_two_groups": ("xworld", TWO_GROUPS, dict(cells=49, groups=2, exclusive=True), 84 * 84),   # one_channel, exclusive: the defaults
}


@pytest.mark.parametrize("case", sorted(LAYOUTS))
def test_blob_layout_is_version_4(case):
    """The blob's array sequence, written out here and not taken from the library: a header of 56 bytes, then a uint64 length in
    front of each array, with and without frames."""
    from xworld_amd.batched import BatchedSimulator
    game, opts, shape, frames = LAYOUTS[case]
    n = 3
    sim = BatchedSimulator(game, opts, num_envs=n, seed=2)
    if game == "xworld":
        assert sim.cfg.max_dim == 7 and sim.cfg.curriculum == 0 and sim.cfg.rng_mode == 0
    sim.step()
    for include_obs in (False, True):
        n_arrays, lengths = _walk(sim.save_state(include_obs=include_obs))
        want = _blob_layout(n, frames if include_obs else None, **shape)
        print(case, include_obs, lengths)
        assert lengths == want and n_arrays == len(want)
    sim.close()
