"""Checkpoint / resume over the stateful modes: every array xwb_save_state lists has to come back, and the verbs after a load
have to use it.  300 envs everywhere (two entries of the per-workgroup reset counts, five wavefronts, the last one ragged),
40 loop iterations before the save and 25 after; everything is compared after EVERY iteration, and the final blobs --
tests/_blob.py canonical(): apart from the done list's order -- catch any state array no getter exposes.

(a) test_resume_matrix: eleven configurations x three loops, library against library, each with an assertion that the state
    it is there for was live.  The loops: "reset_step" = `reset_done; step`, the blob saved between the reset_done and the step
    of an iteration (no step open); "autoreset" = step_autoreset; "open_step" = `step; reset_done`, the blob saved between the
    two, and the comparison after each of the two verbs.  Where a case departs from the plain recipe: the egocentric r = 9 case
    has a 9 x 9 map (visible_radius is clamped to max_dim, and r = 7 draws on the span path); the curriculum batch runs 260
    iterations before its 40 (PRELUDE); sg_minstd and race_minstd cannot show that their engines moved -- SimpleGame never draws,
    and a SimpleRace with a fixed start never does -- so they show that the engines are distinct per env and come back bit-equal.
(b) test_resumed_batch_against_the_oracle: the resumed batch against rows 40..64 of an oracle rollout that was never
    interrupted: rewards and codes of all 300 envs, frames of the first 64 (the r = 9 case: 20 iterations before the save and 12
    after, ORACLE_STEPS).  Configurations WITHOUT a whole-run oracle rollout, library against library in (a) only:
    race_random_minstd (race_rollout draws its start positions from the counter-based stream, not from per-env minstd engines).
    float32 frames go back to pixels (x 255, rounded) before the checksum.
(c) test_load_without_frames: a blob without frames, loaded into a batch that shows foreign frames.
(d) test_done_list_order_is_unobservable: the blob of an open step loaded as it is, with the list reversed and shuffled.
(e) test_seeded_run_reproduces_itself: canonical blobs of two runs of one configuration in one process.
(f) test_load_across_paths: blobs exchanged between the default kernel sequence and its classic / per-env twin."""
import functools
import os

import numpy as np
import pytest

from _blob import canonical, parse, permute_done_list

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "xworld_amd", "confs")
NAV = os.path.join(CONF, "navigation2d.json")
T3 = ["XWorld3DNavTarget", "XWorld3DNavTargetNear", "XWorld3DNavTargetBetween", "XWorld3DNavTargetDirection", "XWorld3DNavTargetAvoid"]
T2 = ["XWorldNavTarget", "XWorldNavNear", "XWorldNavColorTarget", "XWorldNavBetween"]
N, WARM, POST = 300, 40, 25
SPREAD = [0, 1, 63, 64, 127, 255, 256, 299]                       # envs whose sentence and env_state are compared: wavefront and workgroup edges
RACE = {"track_width": 20.0, "track_length": 100.0, "track_radius": 30.0}
NAV7 = {"xwd_conf_path": NAV, "task_mode": "lang_acquisition", "max_dim": 7, "num_blocks": 16, "max_steps": 30}
NAV7_OR = dict(map_kind=0, max_dim=7, dim=7, num_goals=4, num_blocks=16, max_steps=30, tasks=[0, 1, 2, 3, 4])

# name: game, options, (seed, policy_seed), the blob's shape (tests/_blob.py), the oracle's configuration (None: no whole-run
# rollout), what shows that the case's state was live.  max_steps = 30 ends every episode that lasts: envs finish between
# the save at 40 and the end at 65 whatever the policy does.
CONFIGS = {
    "sg_minstd": ("simple_game", {"array_size": 16, "rng": "minstd", "simulator_seed": 7}, (5, 9),
                  dict(simple_game=True, minstd=True), {}, ("idle_engines",)),
    "race_minstd": ("simple_race", dict(RACE, max_steps=30, rng="minstd", simulator_seed=7), (5, 9),
                    dict(simple_race=True, minstd=True), dict(max_steps=30), ("idle_engines",)),
    "race_random_minstd": ("simple_race", dict(RACE, max_steps=30, random=True, rng="minstd", simulator_seed=7, thread_base=3), (5, 9),
                           dict(simple_race=True, minstd=True), None, ("engines",)),
    "xw_minstd_weighted": ("xworld", dict(NAV7, task_weights=[1, 2, 3, 4, 5], rng="minstd", simulator_seed=2, thread_base=5), (9, 3),
                           dict(cells=49, minstd=True), dict(NAV7_OR, task_weights=[1, 2, 3, 4, 5], simulator_seed=2, thread_base=5),
                           ("engines",)),
    "xw_float32_ctx2": ("xworld", dict(NAV7, color=True, obs_format="float32", context=2), (21, 4),
                        dict(cells=49), dict(NAV7_OR, color=1, context=2), ()),
    "xw_gray_walls": ("xworld", {"xwd_conf_path": os.path.join(CONF, "walls.json"), "map": "XWorldWalls", "task_group": "XWorldNav",
                                 "task_mode": "one_channel", "max_steps": 30, "color": False}, (31, 6),
                      dict(cells=49), dict(map_kind=1, max_dim=7, dim=7, num_goals=12, num_blocks=12, max_steps=30, task_mode=1,
                                           tasks=T2, walls=True), ()),
    "xw_two_groups": ("xworld", {"xwd_conf_path": NAV, "task_mode": "lang_acquisition", "max_dim": 8, "color": True, "max_steps": 30,
                                 "tasks": T3, "tasks2": T2}, (44, 4),
                      dict(cells=64, groups=2), dict(map_kind=0, max_dim=8, dim=8, num_goals=4, num_blocks=16, max_steps=30, color=1,
                                                     tasks=T3, tasks2=T2), ()),
    "xw_exclusive": ("xworld", {"xwd_conf_path": os.path.join(CONF, "nav_two_groups.json"), "max_steps": 30, "max_dim": 7, "num_blocks": 16},
                     (33, 9), dict(cells=49, groups=2, exclusive=True),
                     dict(map_kind=0, max_dim=7, dim=7, num_goals=4, num_blocks=16, max_steps=30, task_mode=1, tasks=T3, tasks2=T2,
                          task_weights2=[2, 1, 3, 1], task_groups_exclusive=1, group_weights=[1, 0.5]), ("grp_order",)),
    "xw_curriculum": ("xworld", {"xwd_conf_path": NAV, "task_mode": "lang_acquisition", "tasks": T3[:1], "curriculum": 0.1,
                                 "start_level": 2, "max_steps": 3}, (11, 6),
                      dict(cells=64, curriculum=True), dict(map_kind=0, max_dim=8, dim=8, num_goals=4, num_blocks=16, max_steps=3,
                                                            tasks=T3[:1], curriculum=0.1, start_level=2), ("levels",)),
    # (a 9 x 9 map: the library clamps visible_radius to max_dim, and r = 7 draws on the span path)
    "xw_ego9": ("xworld", dict(NAV7, max_dim=9, num_blocks=20, color=True, visible_radius=9), (17, 3),
                dict(cells=81, ego=True), dict(NAV7_OR, max_dim=9, dim=9, num_blocks=20, color=1, visible_radius=9), ("per_env",)),
    "xw_ego3_two_groups": ("xworld", dict(NAV7, color=True, visible_radius=3, tasks=T3, tasks2=T2), (21, 8),
                           dict(cells=49, groups=2, ego=True), dict(NAV7_OR, color=1, visible_radius=3, tasks=T3, tasks2=T2), ("span",)),
    # further configurations of (c) .. (f)
    "sg_ctx2": ("simple_game", {"array_size": 16, "context": 2}, (5, 9), dict(simple_game=True), {}, ()),
    "race_ctx3": ("simple_race", dict(RACE, max_steps=30, random=True, context=3), (5, 9), dict(simple_race=True), None, ()),
    "xw_full_ctx2": ("xworld", dict(NAV7, color=True, context=2), (21, 4), dict(cells=49), dict(NAV7_OR, color=1, context=2), ()),
    "xw_ego3": ("xworld", dict(NAV7, color=True, visible_radius=3), (17, 3), dict(cells=49, ego=True),
                dict(NAV7_OR, color=1, visible_radius=3), ("span",)),
    "xw_default": ("xworld", dict(NAV7, color=True), (3, 4), dict(cells=49), dict(NAV7_OR, color=1), ()),
}
MATRIX = ["sg_minstd", "race_minstd", "race_random_minstd", "xw_minstd_weighted", "xw_float32_ctx2", "xw_gray_walls", "xw_two_groups",
          "xw_exclusive", "xw_curriculum", "xw_ego9", "xw_ego3_two_groups"]
WITH_ORACLE = [k for k in MATRIX if CONFIGS[k][4] is not None]
# A curriculum level is checked every 100th reset of an env, so no level can change within 40 iterations of a fresh batch: the
# source batch of this configuration first runs PRELUDE iterations of `step; reset_done` in one xwb_run call.  With max_steps = 3
# the oracle shows levels 2 and 3 side by side from step 300 to 500 (one level only at 200, levels 2 to 4 at 600).
PRELUDE = {"xw_curriculum": 260}
# (b) holds the frames of the first 64 envs against the oracle's renderer, which takes 7 ms (r = 3) to 25 ms (r = 9 on a 9 x 9 map)
# for an egocentric frame on one core: the 64 envs are rendered in chunks on a thread pool, and the r = 9 case runs fewer
# iterations on either side of the save (the wave of time-outs at step 30 falls after it).
ORACLE_STEPS = {"xw_ego9": (20, 12)}                    # (iterations before the save, after it); default (WARM, POST)
CK_ENVS, CK_CHUNK, CK_THREADS = 64, 4, 16


def _make(name, debug=None, warm=False, **over):
    """a batch of configuration `name`; warm: the one that will save runs the configuration's prelude first"""
    import torch
    assert torch.cuda.is_available()
    from xworld_amd.batched import BatchedSimulator
    game, opts, (seed, policy_seed), _, _, _ = CONFIGS[name]
    opts = dict(opts, **over)
    if debug:
        opts["debug"] = list(debug)
    sim = BatchedSimulator(game, opts, num_envs=N, seed=seed, policy_seed=policy_seed)
    if warm and PRELUDE.get(name):
        sim.run(PRELUDE[name])
    return sim


@functools.lru_cache(maxsize=None)
def _oracle_rollout(name, steps=WARM + POST, max_steps=None, render=CK_ENVS):
    """(rewards, codes, frame checksums of the first `render` envs or None) of `steps` iterations of `reset_done; step` after the
    configuration's prelude, computed once.  An env's rollout is a function of its global id alone, so the rendered envs are
    split into chunks of CK_CHUNK (env_gid0 = first env of the chunk) that run side by side: the oracle call holds no lock."""
    import _oracle as O
    from concurrent.futures import ThreadPoolExecutor
    skip = PRELUDE.get(name, 0)
    steps += skip
    game, _, (seed, policy_seed), _, oc, _ = CONFIGS[name]
    if game == "simple_game":
        r = O.sg_rollout(N, 16, steps, policy_seed=policy_seed)
        return r.rewards, r.codes, r.obs_ck[:, :render]
    if game == "simple_race":                                 # (random = false: no draw is ever made, whatever engine the batch has)
        r = O.race_rollout(N, O.race_cfg(**oc), seed=seed, steps=steps, policy_seed=policy_seed)
        return r.rewards, r.codes, r.obs_ck[:, :render]
    oc = dict(oc)
    if max_steps is not None:
        oc["max_steps"] = max_steps
    pal = O.Palette(O.WALLS_SUBTREES if oc.pop("walls", False) else O.NAV_SUBTREES)
    cfg = O.xw_cfg(seed=seed, **oc)
    full = O.xw_rollout(N, cfg, pal, steps, policy_seed=policy_seed)
    if not render:
        return full.rewards[skip:], full.codes[skip:], None
    assert render % CK_CHUNK == 0

    def chunk(g0):
        r = O.xw_rollout(CK_CHUNK, cfg, pal, steps, policy_seed=policy_seed, env_gid0=g0, render=True)
        same = r.rewards.view(np.uint32) == full.rewards[:, g0:g0 + CK_CHUNK].view(np.uint32)
        assert same.all() and np.array_equal(r.codes, full.codes[:, g0:g0 + CK_CHUNK]), g0      # the chunk is those envs' rollout
        return r.obs_ck
    with ThreadPoolExecutor(CK_THREADS) as pool:
        ck = np.concatenate(list(pool.map(chunk, range(0, render, CK_CHUNK))), axis=1)
    return full.rewards[skip:], full.codes[skip:], ck[skip:]


KEYS = ("reward", "game_over_codes", "num_steps", "episode", "success", "actions")


def _snap(sim, obs=True):
    """clones of everything a caller can read of a batch, after the queues have drained (num_steps is a state array: a
    reset_done may run ahead of reads queued on the caller's stream, include/xwb.h)"""
    import torch
    torch.cuda.synchronize()
    out = {k: getattr(sim, k).clone() for k in KEYS}
    if obs:
        out["obs"] = sim.obs.clone()
    if sim.name == "xworld":
        out["grid"] = sim.grid.clone()
    if sim.cfg.rng_mode == 1:
        out["minstd_state"] = sim.minstd_state.clone()
    return out


def _first_diff(x, y):
    import torch
    bad = torch.nonzero((x != y).reshape(x.shape[0], -1).any(1)).flatten()
    return int(bad[0]), int(bad.numel())


def _assert_same(want, got, where, skip=()):
    """the first differing array and env are the evidence: they go into the message"""
    import torch
    for k in want:
        if k in skip:
            continue
        x, y = want[k], got[k]
        if x.dtype.is_floating_point:                         # floats by their bits
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        if not torch.equal(x, y):
            e, cnt = _first_diff(x, y)
            raise AssertionError("%s: %s differs, first at env %d (%d envs): %s != %s" % (
                where, k, e, cnt, want[k][e].flatten()[:8].tolist(), got[k][e].flatten()[:8].tolist()))


def _blob_diff(x, y, shape):
    """None, or which named array of two blobs differs first and at which env"""
    if np.array_equal(x, y):
        return None
    px, py = parse(x, **shape), parse(y, **shape)
    if px["header"] != py["header"]:
        return "header: %s != %s" % (px["header"], py["header"])
    for k in px:
        if k != "header" and px[k].tobytes() != py[k].tobytes():
            a, b = px[k].reshape(px[k].shape[0], -1), py[k].reshape(py[k].shape[0], -1)
            rows = np.nonzero((a.view(np.uint8) != b.view(np.uint8)).any(1))[0]
            return "blob array %s differs, first at row %d (%d rows): %s != %s" % (k, rows[0], rows.size, a[rows[0]][:8], b[rows[0]][:8])
    return "blobs differ outside the arrays"


def _end_state(sim, shape):
    """what is compared once, at the end of a run"""
    out = {"errors": sim.check_errors(), "blob": canonical(sim.save_state(include_obs=True), **shape)}
    if sim.name == "xworld":
        out["perf"] = sim.task_performance()
        out["sentences"] = [sim.sentence(e) for e in SPREAD]
    out["env_state"] = [tuple(getattr(st, f[0]) for f in st._fields_) for st in (sim.env_state(e) for e in SPREAD)]
    return out


def _assert_same_end(want, got, shape, where):
    d = _blob_diff(want["blob"], got["blob"], shape)
    for k in want:
        if k != "blob":
            assert want[k] == got[k], (where, k, want[k], got[k])
    assert d is None, (where, d)
    assert want["errors"] == 0


VERBS = {"R": lambda s: s.reset_done(), "S": lambda s: s.step(), "A": lambda s: s.step_autoreset()}
# loop: (verbs before the save, verbs after it, after which of those the batch is recorded)
LOOPS = {
    "reset_step": ("RS" * WARM + "R", "S" + "RS" * (POST - 1), "S"),
    "autoreset": ("A" * WARM, "A" * POST, "A"),
    "open_step": ("SR" * WARM + "S", "R" + "SR" * (POST - 1), "SR"),
}


def _play(sim, verbs, record=""):
    out = []
    for v in verbs:
        VERBS[v](sim)
        if v in record:
            out.append(_snap(sim))
    return out


def _check_live(name, live, blob, shape, rec, sim, start):
    """each case shows that the state it is there for was in use"""
    import torch
    p = parse(blob, **shape)
    finished = sum(int((r["game_over_codes"] != 0).sum()) for r in rec)
    assert finished > 0, "no env finished in the %d iterations after the load" % POST
    if sim.name == "xworld":
        assert p["episode"].max() > 0, "no env had been reset before the save"
    if "engines" in live:
        assert not torch.equal(start["minstd_state"], rec[-1]["minstd_state"]), "the engines did not move after the save"
        assert len(np.unique(p["minstd"])) > N // 2
    if "idle_engines" in live:
        # SimpleGame never draws and a SimpleRace with a fixed start never does either (kernels_simple.hip race_reset), so no seed
        # can make these engines move: they are distinct per env, and what comes back is what the blob holds
        assert len(np.unique(p["minstd"])) == N
        assert np.array_equal(rec[-1]["minstd_state"].cpu().numpy().view(np.uint32), p["minstd"])
    if "grp_order" in live:
        assert len(np.unique(p["grp_order"])) >= 2, "grp_order is constant over the envs at the save"
    if "levels" in live:
        assert len(np.unique(p["cur_level"])) >= 2, "one curriculum level only: %s" % np.unique(p["cur_level"])
        assert p["cur_usage"].any() and len(np.unique(p["cur_counter"])) >= 2
    if "per_env" in live:
        assert sim.ego_render_path == "per_env"
    if "span" in live:
        assert sim.ego_render_path == "span"
    if shape.get("ego"):
        assert np.isfinite(p["goal_warps"]).all() and len(np.unique(p["heading"])) == 4
    if shape.get("groups") == 2:
        assert p["task_state2"].any() and len(np.unique(p["task_steps2"])) > 1


@pytest.mark.parametrize("loop", sorted(LOOPS))
@pytest.mark.parametrize("name", MATRIX)
def test_resume_matrix(name, loop):
    """(a): batch `a` runs on from the save and keeps a record, a fresh batch resumes from the blob, then `a` rewinds."""
    shape, live = CONFIGS[name][3], CONFIGS[name][5]
    before, after, record = LOOPS[loop]
    a = _make(name, warm=True)
    _play(a, before)
    blob = a.save_state(include_obs=True)
    start = _snap(a)
    if loop == "open_step" and a.name == "xworld":
        assert parse(blob, **shape)["header"]["list_valid"] & 1      # the blob carries the step's done list
    ref = _play(a, after, record)
    end = _end_state(a, shape)
    _check_live(name, live, blob, shape, ref, a, start)
    b = _make(name)
    for who, sim in (("fresh batch", b), ("rewound batch", a)):
        sim.load_state(blob)
        _assert_same(start, _snap(sim), "%s right after the load" % who)
        got = _play(sim, after, record)
        for t, (x, y) in enumerate(zip(ref, got)):
            _assert_same(x, y, "%s, record %d after the load" % (who, t))
        _assert_same_end(end, _end_state(sim, shape), shape, who)
    a.close()
    b.close()


def _obs_ck(sim, k):
    """orc_obs_checksum of the first k envs' frames; float32 frames are pixel * (1 / 255): back to the pixel first"""
    import _oracle as O
    import torch
    obs = sim.obs[:k]
    if sim.name == "xworld" and sim.obs_is_float:
        obs = torch.round(obs * 255.0).to(torch.uint8)
    return O.obs_checksum_np(obs.contiguous().cpu().numpy().reshape(k, -1).view(np.uint8))


@pytest.mark.parametrize("name", WITH_ORACLE)
def test_resumed_batch_against_the_oracle(oracle, name):
    """(b): an independent reference.  The oracle's 65 steps are never interrupted; batch `a` runs 40 and saves, a fresh batch
    loads and runs steps 40 .. 64: reward bits, codes and the frame the policy sees (first 64 envs) of every one of them.  A
    state word that save drops and load re-derives the same wrong way on both sides of test_resume_matrix fails here."""
    warm, post = ORACLE_STEPS.get(name, (WARM, POST))
    rewards, codes, obs_ck = _oracle_rollout(name, warm + post)

    def run(sim, t0, t1):
        for t in range(t0, t1):
            sim.reset_done()
            ck = _obs_ck(sim, CK_ENVS)
            bad = np.nonzero(ck != obs_ck[t])[0]
            assert bad.size == 0, "step %d: the frame of env %d (%d envs) is not the oracle's" % (t, bad[0], bad.size)
            sim.step()
            r = sim.reward.cpu().numpy().view(np.uint32)
            bad = np.nonzero(r != rewards[t].view(np.uint32))[0]
            assert bad.size == 0, "step %d: reward of env %d (%d envs): %r, oracle %r" % (
                t, bad[0], bad.size, r[bad[0]].view(np.float32), rewards[t][bad[0]])
            c = sim.game_over_codes.cpu().numpy()
            bad = np.nonzero(c != codes[t])[0]
            assert bad.size == 0, "step %d: code of env %d (%d envs): %d, oracle %d" % (t, bad[0], bad.size, c[bad[0]], codes[t][bad[0]])

    assert (codes[warm:] != 0).any() and (codes[:warm] != 0).any()          # envs finish on both sides of the save
    a = _make(name, warm=True)
    run(a, 0, warm)
    blob = a.save_state(include_obs=True)
    a.close()
    b = _make(name)
    b.load_state(blob)
    run(b, warm, warm + post)
    assert b.check_errors() == 0
    b.close()


def _foreign_actions(sim, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, sim.num_actions, (N,), generator=g, dtype=torch.int32).cuda()


@pytest.mark.parametrize("name", ["sg_minstd", "sg_ctx2", "race_ctx3", "xw_full_ctx2", "xw_float32_ctx2", "xw_ego3", "xw_curriculum"])
def test_load_without_frames(name):
    """(c): include/xwb.h -- without include_obs "the frames are re-rendered from the state on load and the older context frames
    start black" -- for every game, checked right after the load and before any verb.  The receiving batch has run 7 steps of
    its own under other actions (a blob only loads into a batch of the same configuration, policy_seed included, so the other
    rollout comes from explicit actions), so what it shows before the load is visibly not the source's."""
    import torch
    shape = CONFIGS[name][3]
    a = _make(name, warm=True)
    _play(a, "RS" * WARM)                                      # (the step is open: finished envs show their terminal frames)
    ctx = a.cfg.context
    small, full = a.save_state(include_obs=False), a.save_state(include_obs=True)
    assert "obs" not in parse(small, **shape) and small.size < full.size
    want = _snap(a)
    b = _make(name)
    for t in range(7):
        b.reset_done()
        b.step(_foreign_actions(b, 100 + t))
    torch.cuda.synchronize()
    per = a.obs.shape[1] // ctx                                # channels of one frame
    assert int((b.obs[:, -per:] != a.obs[:, -per:]).reshape(N, -1).any(1).sum()) > N // 2     # foreign frames ...
    if ctx > 1:
        assert bool(b.obs[:, :-per].any())                     # ... in the older ring slots too
    b.load_state(small)
    got = _snap(b)
    _assert_same({"newest frame": want["obs"][:, -per:]}, {"newest frame": got["obs"][:, -per:]}, "right after the load")
    if ctx > 1:
        assert not bool(got["obs"][:, :-per].any()), "an older context frame is not black after the load"
    _assert_same(want, got, "right after the load", skip=("obs",))
    if a.name == "xworld":
        _assert_same({"render_view": a.render_view(), "symbolic": a.symbolic()}, {"render_view": b.render_view(), "symbolic": b.symbolic()},
                     "right after the load")
    for t in range(10):
        for s in (a, b):
            s.reset_done()
            s.step()
        _assert_same(_snap(a), _snap(b), "iteration %d after the load" % t, skip=("obs",) if t < ctx - 1 else ())
        d = _blob_diff(canonical(a.save_state(False), **shape), canonical(b.save_state(False), **shape), shape)
        assert d is None, (t, d)
    _assert_same_end(_end_state(a, shape), _end_state(b, shape), shape, "after 10 iterations")
    a.close()
    b.close()


LIST_STEP = 11        # the step whose finished envs the saved list holds: max_steps = 6 times the second wave out at step index 11
LIST_CASES = {"default": ("xw_default", None, "lazy_fused"), "classic": ("xw_default", ("no_fused", "no_pregen"), "classic"),
              "ego3_span": ("xw_ego3", None, "ego_span"), "ego9_per_env": ("xw_ego9", None, "ego_per_env")}


@pytest.mark.parametrize("case", sorted(LIST_CASES))
def test_done_list_order_is_unobservable(oracle, case):
    """(d): wavefronts append to the done list with atomics, so its order is not a function of the seed.  The blob of an open
    step is loaded as it is, with the first done_count entries reversed (into the batch that saved it) and shuffled: the
    reset_done that consumes the list, and everything after it, must not tell them apart."""
    name, debug, path = LIST_CASES[case]
    shape = CONFIGS[name][3]
    _, codes, _ = _oracle_rollout(name, LIST_STEP + 1, max_steps=6, render=0)
    n_done = int((codes[LIST_STEP] != 0).sum())
    assert n_done >= 8                                         # a condition on the input, from the oracle alone
    a = _make(name, debug, max_steps=6)
    _play(a, "RS" * (LIST_STEP + 1))
    assert a.done_count() == n_done and a.step_path()["path"] == path
    blob = a.save_state(include_obs=True)
    p = parse(blob, **shape)
    assert p["header"]["list_valid"] & 1 and p["done_count"][0] == n_done
    assert sorted(p["done_list"][:n_done].tolist()) == np.nonzero(codes[LIST_STEP])[0].tolist()
    rng = np.random.default_rng(12)
    perms = {"as saved": np.arange(n_done), "reversed": np.arange(n_done)[::-1], "shuffled": rng.permutation(n_done)}
    sims = {"as saved": _make(name, debug, max_steps=6), "reversed": a, "shuffled": _make(name, debug, max_steps=6)}
    for k, s in sims.items():
        s.load_state(permute_done_list(blob, perms[k], **shape))
    for i, v in enumerate("R" + "SR" * 10):
        for s in sims.values():
            VERBS[v](s)
        want = _snap(sims["as saved"])
        for k in ("reversed", "shuffled"):
            _assert_same(want, _snap(sims[k]), "%s list, verb %d (%s)" % (k, i, v))
    end = _end_state(sims["as saved"], shape)
    for k in ("reversed", "shuffled"):
        _assert_same_end(end, _end_state(sims[k], shape), shape, k)
    for s in sims.values():
        s.close()


@pytest.mark.parametrize("name", ["xw_default", "xw_ego3", "race_random_minstd"])
def test_seeded_run_reproduces_itself(name):
    """(e): one configuration created and run twice in one process, 40 x (step(actions); reset_done) under seeded explicit
    actions: the canonical blobs, frames included, are equal.  (The raw blobs may differ in the done list's order.)"""
    shape = CONFIGS[name][3]
    blobs = []
    for run in range(2):
        s = _make(name)
        for t in range(WARM):
            s.step(_foreign_actions(s, 500 + t))
            s.reset_done()
        assert s.check_errors() == 0
        blobs.append(canonical(s.save_state(include_obs=True), **shape))
        s.close()
    p = parse(blobs[0], **shape)
    assert p["episode"].max() > 1                              # (envs did finish)
    d = _blob_diff(blobs[0], blobs[1], shape)
    assert d is None, d


PATH_CASES = {"full": ("xw_default", ("no_fused", "no_pregen"), "lazy_fused", "classic"),
              "ego3": ("xw_ego3", ("ego_no_span",), "ego_span", "ego_per_env")}


@pytest.mark.parametrize("open_step", [False, True], ids=["closed", "open"])
@pytest.mark.parametrize("to_default", [False, True], ids=["default_to_twin", "twin_to_default"])
@pytest.mark.parametrize("case", sorted(PATH_CASES))
def test_load_across_paths(case, to_default, open_step):
    """(f): the configuration hash leaves the debug switches out, so a blob of the default kernel sequence loads into a batch
    held on the classic one (egocentric: the span path and the per-env render) and the reverse.  The batch that saved runs on
    uninterrupted, the receiving batch of the other kind loads, and a third, uninterrupted batch of the receiving kind runs beside
    them: all three are equal after every verb, and the default path is taken up again after the load."""
    name, twin, path_default, path_twin = PATH_CASES[case]
    shape = CONFIGS[name][3]
    dbg = {True: None, False: twin}
    src, dst, beside = _make(name, dbg[not to_default]), _make(name, dbg[to_default]), _make(name, dbg[to_default])
    warm = "SR" * WARM + ("S" if open_step else "")
    for s in (src, beside):
        _play(s, warm)
    assert src.step_path()["path"] == (path_twin if to_default else path_default)
    dst.load_state(src.save_state(include_obs=True))
    want = _snap(src)
    _assert_same(want, _snap(dst), "right after the load")
    _assert_same(want, _snap(beside), "uninterrupted batches of the two kinds at the save")
    paths = set()
    for i, v in enumerate(("R" if open_step else "") + "SR" * 12):
        for s in (src, dst, beside):
            VERBS[v](s)
        want = _snap(src)
        _assert_same(want, _snap(dst), "loaded batch, verb %d (%s)" % (i, v))
        _assert_same(want, _snap(beside), "uninterrupted batch, verb %d (%s)" % (i, v))
        if v == "S":
            paths.add(dst.step_path()["path"])
    assert (path_default if to_default else path_twin) in paths, paths
    if not to_default:
        assert paths == {path_twin}
    end = _end_state(src, shape)
    _assert_same_end(end, _end_state(dst, shape), shape, "loaded batch")
    _assert_same_end(end, _end_state(beside, shape), shape, "uninterrupted batch")
    for s in (src, dst, beside):
        s.close()
