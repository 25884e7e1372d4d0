"""xwb_copy_envs / BatchedSimulator.copy_envs on the device: a clone is its source and follows it, nothing else moves, the expert
agrees with what the forks find, template levels scatter into another batch, pack_grids still describes the frames, refusals
and bad indices, stream order.  Every rollout steps with explicit actions drawn from a seeded generator."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from test_gpu_view import FrameCheck
from test_gpu_xworld import _grid_from_entities, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "xworld_amd", "confs")
NAV2D = os.path.join(CONF, "navigation2d.json")
NAV_TARGET = os.path.join(CONF, "nav_target.json")
GOLD_DIR = os.path.join(ROOT, "tests", "golden")
ERR_ARG, ERR_STATE = -1, -3                                                    # include/xwb.h
SKIP, SUCCESS = -1, 4                                                          # XWB_ACTION_SKIP, XWB_SUCCESS
WIN_REWARD = np.float32(-0.01 + 1.0)                                           # time penalty + the success reward, as the step adds them

DIM5 = dict(dim=5, num_goals=2, num_blocks=6)
RACE = {"track_type": "straight", "track_width": 20.0, "track_length": 100.0, "track_radius": 30.0}
# name -> (game, options, ego render path or None)
CASES = {
    "full_dim5": ("xworld", dict(DIM5, color=True), None),
    "full_dim5_f32_ctx2": ("xworld", dict(DIM5, obs_format="float32", context=2), None),
    "curriculum": ("xworld", dict(curriculum=0.1), None),
    "ego_r3": ("xworld", dict(visible_radius=3, color=True), "span"),
    "ego_r5": ("xworld", dict(visible_radius=5), "span"),
    "ego_r9_nav11": ("xworld", dict(max_dim=11, num_blocks=30, visible_radius=9), "per_env"),
    "simple_game": ("simple_game", {"array_size": 8}, None),
    "simple_race_minstd": ("simple_race", dict(RACE, random=True, rng="minstd", simulator_seed=7), None),
}


def _make(game, opts, n, seed=21, policy_seed=5, conf=NAV2D):
    from xworld_amd.batched import BatchedSimulator
    o = dict(opts)
    if game == "xworld":
        o = dict({"xwd_conf_path": conf, "task_mode": "lang_acquisition"}, **o)
    return BatchedSimulator(game, o, num_envs=n, seed=seed, policy_seed=policy_seed)


def _actions(torch, gen, sim, mirror=None):
    """one random action per env from the seeded generator; mirror = (dst, src) index tensors: the clones take their sources'"""
    a = torch.randint(0, sim.num_actions, (sim.num_envs,), generator=gen, dtype=torch.int32).cuda()
    if mirror is not None:
        a[mirror[0]] = a[mirror[1]]
    return a


def _state_fields(st):
    return {name: getattr(st, name) for name, _ in st._fields_}


def _error_code(excinfo):
    return int(str(excinfo.value).split("xwb error ")[1].split(":")[0])


@pytest.mark.parametrize("case", list(CASES))
def test_a_clone_is_its_source(case):
    """Test 1: 30 steps of step / reset_done, the lower half forked into the upper half; every clone equals its source in state,
    grid, frames, results, view, symbolic observation and expert answer, speaks the slot's own wording, and then follows its
    source under identical actions: until the source's first game-over (XWorld2D), for all 40 steps and across resets (the
    simple games: SimpleGame draws nothing, SimpleRace's engine was forked with the env)."""
    torch = _torch()
    game, opts, ego_path = CASES[case]
    n, half = 128, 64
    sim = _make(game, opts, n)
    xw = game == "xworld"
    if ego_path:
        assert sim.ego_render_path == ego_path
    gen = torch.Generator().manual_seed(1234)
    for _ in range(30):
        sim.step(_actions(torch, gen, sim))
        sim.reset_done()
    src = torch.arange(half, dtype=torch.int32).cuda()
    dst = src + half
    assert sim.copy_envs(dst, src) is sim
    lo, hi = slice(0, half), slice(half, n)
    for name in ("reward", "game_over_codes", "num_steps", "success", "obs", "episode"):
        t = getattr(sim, name)
        assert torch.equal(t[hi], t[lo]), name
    for i in range(half):
        assert _state_fields(sim.env_state(half + i)) == _state_fields(sim.env_state(i)), i
        assert np.array_equal(sim.env_obs(half + i), sim.env_obs(i)), i
        if xw:
            assert np.array_equal(sim.env_grid(half + i, raw=True), sim.env_grid(i, raw=True)), i
            assert sim.sentence(half + i) == sim.sentence_c(half + i), i
    if xw:
        assert torch.equal(sim.render_view(dst), sim.render_view(src))
        sym = sim.symbolic()
        assert torch.equal(sym[hi], sym[lo])
        act, dist = sim.expert()
        assert torch.equal(act[hi], act[lo]) and torch.equal(dist[hi], dist[lo])
    tracking = torch.ones(half, dtype=torch.bool, device="cuda")
    compared = 0
    for t in range(40):
        sim.step(_actions(torch, gen, sim, (dst.long(), src.long())))
        for name in ("reward", "game_over_codes", "success", "obs"):
            v = getattr(sim, name)
            assert torch.equal(v[hi][tracking], v[lo][tracking]), (t, name)
        compared += int(tracking.sum())
        if xw:                                                                 # the clone's next episode is the slot's own
            tracking &= sim.game_over_codes[lo] == 0
        sim.reset_done()
    print("%s: %d clone-steps compared, %d of %d sources still in their first episode" % (case, compared, int(tracking.sum()), half))
    if xw:
        assert compared >= half
    else:
        assert compared == 40 * half and torch.equal(sim.obs[hi], sim.obs[lo]) and int(sim.episode.max()) > 0
    assert sim.check_errors() == 0
    sim.close()


@pytest.mark.parametrize("autoreset", [False, True], ids=["default_loop", "step_autoreset"])
def test_nothing_else_moved(autoreset):
    """Test 2: twin batches run the same verbs, one forks 8 envs at step 10: every other env has the same rewards, codes and
    frames in both for 60 steps, resets included; the fork made the live pre-generated episodes stale exactly once."""
    torch = _torch()
    n = 128
    a, b = (_make("xworld", dict(color=True), n) for _ in range(2))
    dst, src = list(range(100, 108)), list(range(3, 11))
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[dst] = False
    gen = torch.Generator().manual_seed(99)
    resets = 0
    for t in range(60):
        acts = _actions(torch, gen, a)
        for sim in (a, b):
            if autoreset:
                sim.step_autoreset(acts)
            else:
                sim.step(acts)
        for name in ("reward", "game_over_codes", "obs"):
            assert torch.equal(getattr(a, name)[keep], getattr(b, name)[keep]), (t, name)
        resets += int((a.game_over_codes != 0).sum())
        for sim in (a, b):
            sim.reset_done()
        assert torch.equal(a.obs[keep], b.obs[keep]), t
        if t == 10:
            before = (a.step_path(), b.step_path())
            assert before[0]["path"] == ("pregen" if autoreset else "lazy") and before[0] == before[1]
            b.copy_envs(dst, src)
            assert torch.equal(b.obs[dst], b.obs[src]) and torch.equal(a.obs[keep], b.obs[keep])
            assert b.step_path()["shadow_breaks"] == before[1]["shadow_breaks"] + 1
    assert resets > 0
    assert b.step_path()["shadow_breaks"] == a.step_path()["shadow_breaks"] + 1
    assert a.check_errors() == 0 and b.check_errors() == 0
    a.close()
    b.close()


def _lookahead_module():
    spec = importlib.util.spec_from_file_location("lookahead_example", os.path.join(ROOT, "examples", "lookahead.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("radius", [0, 3], ids=["full", "ego_r3"])
def test_forks_against_the_expert(radius):
    """Test 3: roots 0 .. R - 1, root i's child for action a at R + A i + a.  With the expert's (k, a*) at the roots: after the fork
    and one step the a* child has dist k - 1 and no child a smaller one (k >= 2), or carries the success reward and code (k = 1);
    examples/lookahead.py picks a* or an action as good.  Eight rounds, the roots advancing along the expert's path in between."""
    torch = _torch()
    look = _lookahead_module()
    r = 32
    sim = _make("xworld", dict(color=True, visible_radius=radius) if radius else dict(color=True), r * 7, seed=8)
    a = sim.num_actions
    assert a == (6 if radius else 4)
    kids = torch.arange(r * a, dtype=torch.int32).cuda()
    child, parent = kids + r, kids // a
    near = far = 0
    for rnd in range(8):
        act, dist = (x[:r].clone() for x in sim.expert())
        best = look.lookahead(sim, r)
        sim.copy_envs(child, parent)
        acts = torch.full((sim.num_envs,), SKIP, dtype=torch.int32, device="cuda")
        acts[r:r + r * a] = kids % a
        sim.step(acts)
        cd = sim.expert()[1][r:r + r * a].view(r, a).cpu().numpy()
        codes = sim.game_over_codes[r:r + r * a].view(r, a).cpu().numpy()
        rew = sim.reward[r:r + r * a].view(r, a).cpu().numpy()
        sim.reset_done()
        k, astar, pick = dist.cpu().numpy(), act.cpu().numpy(), best.cpu().numpy()
        for i in range(r):
            if k[i] < 1:
                continue
            if k[i] == 1:
                near += 1
                assert codes[i, astar[i]] == SUCCESS and rew[i, astar[i]] == WIN_REWARD, (rnd, i)
                assert codes[i, pick[i]] == SUCCESS, (rnd, i)
            else:
                far += 1
                live = cd[i][cd[i] > 0]
                assert cd[i, astar[i]] == k[i] - 1 and live.min() == k[i] - 1, (rnd, i, k[i], cd[i])
                assert not (codes[i] & SUCCESS).any() and cd[i, pick[i]] == k[i] - 1, (rnd, i)
        step = torch.full((sim.num_envs,), SKIP, dtype=torch.int32, device="cuda")
        step[:r] = act
        sim.step(step)
        sim.reset_done()
    assert near > 0 and far > 0, (near, far)
    assert sim.check_errors() == 0
    sim.close()


def test_template_scatter(oracle):
    """Test 4: eight replayed reference maps in a template batch, scattered over a 64-env batch with another seed (keep_rng)."""
    torch = _torch()
    with open(os.path.join(GOLD_DIR, "maps_nav.json")) as f:
        maps = json.load(f)[:8]
    opts = dict(color=True)
    template = _make("xworld", opts, 8, seed=1, conf=NAV_TARGET)
    for e, m in enumerate(maps):
        agent = [x for x in m["entities"] if x[0] == 2][0]
        goal = [x for x in m["entities"] if x[0] == 0][0]                      # the target: every goal named like the map's first one
        template.load_map(e, _grid_from_entities(m["entities"], 8), agent[1], agent[2], int(template.palette.icon_name[goal[3]]))
    work = _make("xworld", opts, 64, seed=2, policy_seed=77, conf=NAV_TARGET)
    episode = work.episode.clone()
    blob = template.save_state()
    assert work.copy_envs(range(64), [i % 8 for i in range(64)], source=template, keep_rng=True) is work
    assert np.array_equal(template.save_state(), blob)
    assert torch.equal(work.episode, episode)
    tdist = template.expert()[1].clone()
    dist0 = work.expert()[1].clone()
    for e in range(64):
        assert np.array_equal(work.env_grid(e, raw=True), template.env_grid(e % 8, raw=True)), e
        assert np.array_equal(work.env_obs(e), template.env_obs(e % 8)), e
        assert work.env_target_cells(e) == template.env_target_cells(e % 8) != [], e
        assert int(dist0[e]) == int(tdist[e % 8]), e
    # under the expert an env with a path finishes on its dist-th step; afterwards every frame is still its view, resized
    can_win = dist0 > 0
    assert bool(can_win.any())
    finished = torch.zeros(64, dtype=torch.bool, device="cuda")
    for _ in range(int(dist0.max())):
        work.step(work.expert(no_path=SKIP)[0])                                # (an env without a path sits the step out)
        finished |= work.game_over_codes != 0
        work.reset_done()
    assert torch.equal(finished, can_win)
    assert bool((work.episode[finished] > episode[finished]).all()) and torch.equal(work.episode[~finished], episode[~finished])
    FrameCheck(oracle, work, True).check(work.render_view(), "after the resets")
    assert work.check_errors() == 0 and template.check_errors() == 0
    work.close()
    template.close()


def test_pack_grids_still_describes_the_frames():
    """Test 5: after a fork, pack_grids -> render_grids of the whole batch is obs (context 1)."""
    torch = _torch()
    n = 96
    sim = _make("xworld", dict(DIM5, color=True), n)
    gen = torch.Generator().manual_seed(5)
    for _ in range(12):
        sim.step(_actions(torch, gen, sim))
        sim.reset_done()
    sim.copy_envs(range(48, 96), range(48))
    d = sim.cfg.max_dim
    grids = torch.empty((n, d * d), dtype=torch.int16, device="cuda")
    out = torch.empty_like(sim.obs)
    sim.pack_grids(grids)
    sim.render_grids(grids, None, out)
    assert torch.equal(out, sim.obs) and torch.equal(grids[48:], grids[:48])
    assert sim.check_errors() == 0
    sim.close()


def test_refusals_and_bad_indices():
    """Test 6."""
    torch = _torch()
    from xworld_amd import lib
    n = 64
    sim = _make("xworld", {}, n)
    gen = torch.Generator().manual_seed(3)
    sim.step(_actions(torch, gen, sim))
    blob = sim.save_state()
    with pytest.raises(lib.XwbError) as ei:                                    # between step and reset_done
        sim.copy_envs([1], [0])
    assert _error_code(ei) == ERR_STATE and np.array_equal(sim.save_state(), blob)
    sim.reset_done()
    for game, opts in (("xworld", dict(dim=5, num_goals=2, num_blocks=6)), ("xworld", dict(visible_radius=3)), ("simple_game", {"array_size": 8})):
        other = _make(game, opts, 16)
        with pytest.raises(lib.XwbError) as ei:
            sim.copy_envs([1], [0], source=other)
        assert _error_code(ei) == ERR_ARG, (game, opts)
        other.close()
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = C.c_void_p(one.data_ptr())
    assert sim.L.xwb_copy_envs(sim.h, ptr, sim.h, ptr, -1, 0, None) == ERR_ARG
    assert sim.L.xwb_copy_envs(sim.h, ptr, sim.h, ptr, 1, 2, None) == ERR_ARG
    assert sim.L.xwb_copy_envs(sim.h, None, sim.h, ptr, 1, 0, None) == ERR_ARG
    assert sim.L.xwb_copy_envs(None, ptr, sim.h, ptr, 1, 0, None) == ERR_ARG
    # n = 0 launches nothing: the state and the step paths' bookkeeping stay as they are
    blob, breaks = sim.save_state(), sim.step_path()["shadow_breaks"]
    assert sim.copy_envs([], []) is sim
    assert np.array_equal(sim.save_state(), blob) and sim.step_path()["shadow_breaks"] == breaks
    # -1 and num_envs in the lists: those pairs are skipped, the others copied, the errors counted
    obs = sim.obs.clone()
    assert sim.check_errors() == 0
    sim.copy_envs([40, -1, 41, 42], [1, 2, 3, n])
    assert sim.check_errors() == 2
    assert torch.equal(sim.obs[40], obs[1]) and torch.equal(sim.obs[41], obs[3]) and torch.equal(sim.obs[42], obs[42])
    rest = [e for e in range(n) if e not in (40, 41)]
    assert torch.equal(sim.obs[rest], obs[rest])
    assert np.array_equal(sim.env_grid(41, raw=True), sim.env_grid(3, raw=True))
    assert sim.check_errors() == 0
    sim.close()


def test_stream_order():
    """Test 7: steps, a fork and more steps on a probed non-default stream give the default-stream run's results."""
    torch = _torch()
    n = 128
    a, b = (_make("xworld", dict(color=True), n) for _ in range(2))
    s = torch.cuda.Stream()
    assert b.queue_sync_mode(s)[0] in ("events", "epochs")
    gen = torch.Generator().manual_seed(17)
    acts = [_actions(torch, gen, a) for _ in range(24)]
    dst = torch.arange(64, 128, dtype=torch.int32).cuda()
    src = torch.arange(0, 64, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    for sim, st in ((a, None), (b, s)):
        for t in range(24):
            sim.step(acts[t], stream=st)
            sim.reset_done(stream=st)
            if t == 11:
                sim.copy_envs(dst, src, stream=st)
    s.synchronize()
    torch.cuda.synchronize()
    for name in ("reward", "game_over_codes", "obs", "episode", "num_steps"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.grid, b.grid)
    assert a.check_errors() == 0 and b.check_errors(stream=s) == 0
    a.close()
    b.close()
