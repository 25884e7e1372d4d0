"""The shortest-path expert on the GPU (xwb_xw_expert, BatchedSimulator.expert): dist, action and the whole field of every env
exactly equal to the plain-Python checker (tests/_expert_ref.py, pinned on the CPU by tests/test_expert_ref.py) fed from the
oracle's state; expert-driven rollouts against the oracle; the curriculum climbed; reads only; stream order; refusals."""
import os

import numpy as np
import pytest

import _expert_cases as cases
import _expert_ref as ref

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _na(name):
    return 6 if cases.CASES[name][0].get("visible_radius") else 4


class Oracles:
    """one oracle object per env, stepped with the batch"""

    def __init__(self, oracle, name, n):
        self.oracle, self.name, self.n = oracle, name, n
        self.pal = cases.palette(oracle, name)
        cfg = cases.make_oracle_cfg(name)
        self.two = name in cases.TWO_GROUPS
        self.w = [oracle.XWorld(self.pal, render=False, **cfg) for _ in range(n)]
        self.episode = np.zeros(n, int)
        for e, w in enumerate(self.w):
            w.reset_game(cases.GID0 + e, 0)

    def reset_done(self):
        for e, w in enumerate(self.w):
            if w.game_over() != 0:
                self.episode[e] += 1
                w.reset_game(cases.GID0 + e, int(self.episode[e]))

    def step(self, actions):
        r = np.zeros(self.n, np.float32)
        code = np.zeros(self.n, np.uint8)
        for e, w in enumerate(self.w):
            r[e] = w.take_actions(int(actions[e]))
            code[e] = w.game_over()
        return r, code

    def event3d(self, e):
        return self.w[e].group_state(0)[3] if self.two else self.w[e].event()

    def performance(self):
        """successes, failures, success_steps of the XWorld3DNav* tasks, summed over the env objects' own tallies"""
        import ctypes as C
        fn = self.oracle.lib().orc_xw_get_performance
        tot = np.zeros(3, np.int64)
        for w in self.w:
            arr = ((C.c_int64 * 4) * 9)()
            fn(C.c_void_p(w.h) if isinstance(w.h, int) else w.h, arr)
            tot += np.array([[arr[k][i] for i in range(3)] for k in range(5)]).sum(0)
        return tot.tolist()

    def steps3d(self, e):
        return self.w[e].group_state(0)[2] if self.two else self.w[e].steps_in_task()

    def state(self, e):
        return ref.state_from_oracle(self.w[e], self.pal, two_groups=self.two)


def _compare(sim, orc, where, no_path=0, sample_env_getters=True):
    torch = _torch()
    a, d, f = sim.expert(field=True, no_path=no_path)
    torch.cuda.synchronize()
    a, d, f = a.cpu().numpy(), d.cpu().numpy(), f.cpu().numpy()
    types = np.asarray(sim.palette.icon_type)
    finite = 0
    for e in range(orc.n):
        st = orc.state(e)
        wd, firsts, wf = ref.solve(st, want_field=True)
        assert d[e] == wd, (where, e, d[e], wd)
        assert a[e] == (firsts[0] if firsts else no_path), (where, e, a[e], firsts)
        assert np.array_equal(f[e], wf), (where, e, np.nonzero(f[e] != wf))
        finite += wd != ref.NO_PATH
        if sample_env_getters and e % (orc.n // 64) == 0 and st.active:
            st2 = ref.state_from_env(sim, e, types)                  # the two sides agree on the state itself
            assert ref.solve(st2) == (wd, firsts), (where, e)
    return finite


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_exact_against_the_checker(oracle, name):
    _torch()
    n = 1024
    sim = cases.make_sim(name, n)
    orc = Oracles(oracle, name, n)
    finite = _compare(sim, orc, "reset")
    if name != "curriculum":                 # (the bar tests/test_expert_ref.py holds the same first episodes to; level 0 is not held to it)
        assert 2 * finite >= n, finite
    t = 0
    for upto in (1, 5, 40):
        while t < upto:
            sim.step()
            orc.step([oracle.policy_action(5, cases.GID0 + e, t, _na(name)) for e in range(n)])
            t += 1
            if t == upto and upto == 5:
                # between step and reset_done: finished envs answer -1, no_path_action, an all-0xFFFF field
                done = sim.game_over_codes.cpu().numpy() != 0
                _compare(sim, orc, "finished", no_path=-1, sample_env_getters=False)
                a, d, f = (x.cpu().numpy() for x in sim.expert(field=True, no_path=-1))
                assert (d[done] == -1).all() and (a[done] == -1).all() and (f[done] == 0xFFFF).all()
            sim.reset_done()
            orc.reset_done()
        _compare(sim, orc, "after %d" % upto, no_path=3)
    assert sim.check_errors() == 0
    sim.close()


def _expert_rollout(oracle, name, n, iters, autoreset=False):
    """expert -> step(actions) -> reset_done (or step_autoreset) beside one oracle object per env driven by the same actions:
    reward bits and codes of every env-step; an episode that began with dist = d records correct_goal on its d-th step and not
    before; the batch's task_performance equals the oracle objects' own tallies."""
    _torch()
    sim = cases.make_sim(name, n)
    orc = Oracles(oracle, name, n)
    start_dist = np.full(n, -2)              # dist at the episode's first step; -2: not taken yet, -3: its win has been seen
    k_in_episode = np.zeros(n, int)
    wins = 0
    for it in range(iters):
        a, d = sim.expert()
        ah, dh = a.cpu().numpy(), d.cpu().numpy()
        fresh = start_dist == -2
        start_dist[fresh] = dh[fresh]
        if autoreset:
            sim.step_autoreset(a)
        else:
            sim.step(a)
        r, code = orc.step(ah)
        assert np.array_equal(sim.reward.cpu().numpy().view(np.uint32), r.view(np.uint32)), it
        assert np.array_equal(sim.game_over_codes.cpu().numpy(), code), it
        k_in_episode += 1
        for e in np.nonzero(start_dist > 0)[0]:
            won = orc.event3d(e) == 1
            assert won == (k_in_episode[e] == start_dist[e]), (it, e, k_in_episode[e], start_dist[e])
            if won:
                wins += 1
                start_dist[e] = -3
        over = code != 0
        start_dist[over] = -2
        k_in_episode[over] = 0
        if not autoreset:
            sim.reset_done()
        orc.reset_done()
    if name != "curriculum":
        assert 2 * wins >= n                 # at least half of the FIRST episodes have a path (tests/test_expert_ref.py); each is won
    perf, _ = sim.task_performance()
    got = [sum(v[i] for k, v in perf.items() if k.startswith("XWorld3D")) for i in range(3)]
    assert got == orc.performance(), (got, orc.performance())
    assert sim.check_errors() == 0
    sim.close()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_expert_rollout_against_the_oracle(oracle, name):
    _expert_rollout(oracle, name, 1024, 240)


def test_expert_rollout_autoreset(oracle):
    _expert_rollout(oracle, "nav8_five", 1024, 240, autoreset=True)


def test_full_size_c4_expert(oracle):
    """32 768 envs, 7 x 7, the five tasks: rewards and codes of every env for 24 expert-driven steps against the oracle."""
    _torch()
    n = 32768
    sim = cases.make_sim("nav8_five", n, max_dim=7, num_blocks=16)
    pal = cases.palette(oracle, "nav8_five")
    cfg = cases.make_oracle_cfg("nav8_five")
    cfg.update(max_dim=7, dim=7)
    ws = [oracle.XWorld(pal, render=False, **cfg) for _ in range(n)]
    ep = np.zeros(n, int)
    for e, w in enumerate(ws):
        w.reset_game(cases.GID0 + e, 0)
    for it in range(24):
        a, _ = sim.expert()
        ah = a.cpu().numpy()
        sim.step(a)
        rew, codes = sim.reward.cpu().numpy(), sim.game_over_codes.cpu().numpy()
        for e, w in enumerate(ws):
            r = w.take_actions(int(ah[e]))
            assert np.float32(r).view(np.uint32) == rew[e].view(np.uint32) and w.game_over() == codes[e], (it, e)
            if codes[e]:
                ep[e] += 1
                w.reset_game(cases.GID0 + e, int(ep[e]))
        sim.reset_done()
    assert (ep > 0).sum() > n // 3
    sim.close()


def test_curriculum_is_climbed(oracle):
    """32 envs at curriculum 0.1 under the expert: rewards and codes of every step, level and check counter after EVERY reset
    (each reset runs the level check) equal the oracle's; every env reaches level >= 2 (about 5 s on an MI355X box)."""
    _torch()
    n, iters = 32, cases.CURRICULUM_ITERS
    sim = cases.make_sim("curriculum", n)
    orc = Oracles(oracle, "curriculum", n)
    for it in range(iters):
        a, _ = sim.expert()
        ah = a.cpu().numpy()
        sim.step(a)
        r, code = orc.step(ah)
        assert np.array_equal(sim.reward.cpu().numpy().view(np.uint32), r.view(np.uint32)), it
        assert np.array_equal(sim.game_over_codes.cpu().numpy(), code), it
        sim.reset_done()
        orc.reset_done()
        for e in np.nonzero(code)[0]:
            st = sim.env_state(int(e))
            assert (st.xw_level, st.xw_check_counter) == orc.w[e].curriculum_state(), (it, e)
    assert min(sim.env_state(e).xw_level for e in range(n)) >= 2
    sim.close()


@pytest.mark.parametrize("mode", ["lazy_fused", "autoreset", "ego"])
def test_reads_only(mode):
    torch = _torch()
    name = "ego3" if mode == "ego" else "nav8_five"
    n = 1024
    a, b = cases.make_sim(name, n), cases.make_sim(name, n)
    for it in range(60):
        b.expert(field=True)
        if mode == "autoreset":
            a.step_autoreset(); b.step_autoreset()
        else:
            a.step(); b.step()
        b.expert(field=True)
        assert torch.equal(a.reward, b.reward) and torch.equal(a.game_over_codes, b.game_over_codes), it
        assert torch.equal(a.obs, b.obs), it
        assert a.step_path() == b.step_path(), it
        if mode != "autoreset":
            a.reset_done(); b.reset_done()
            b.expert(field=True)
            assert torch.equal(a.obs, b.obs), it
    if mode == "lazy_fused":
        assert b.step_path()["path"] == "lazy_fused"
    assert a.check_errors() == 0 and b.check_errors() == 0
    a.close(); b.close()


def test_stream_order():
    """step; reset_done; expert; step(actions) queued on a caller stream without any host synchronisation in between gives what
    the same sequence gives with a device synchronisation after every call."""
    torch = _torch()
    n, iters = 4096, 30
    b, c = cases.make_sim("nav8_five", n), cases.make_sim("nav8_five", n)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b.step(stream=st)
        for _ in range(iters):
            b.reset_done(stream=st)
            acts, _ = b.expert(stream=st)
            b.step(acts, stream=st)
    st.synchronize()
    c.step()
    torch.cuda.synchronize()
    for _ in range(iters):
        c.reset_done()
        torch.cuda.synchronize()
        acts, _ = c.expert()
        torch.cuda.synchronize()
        c.step(acts)
        torch.cuda.synchronize()
    assert torch.equal(b.reward, c.reward) and torch.equal(b.game_over_codes, c.game_over_codes) and torch.equal(b.obs, c.obs)
    assert b.task_performance() == c.task_performance()
    for s in (b, c):
        assert s.check_errors() == 0
        s.close()


def test_refusals():
    torch = _torch()
    import ctypes as C
    from xworld_amd.batched import BatchedSimulator
    from xworld_amd.lib import XwbError
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    for game, opts in (("simple_game", {"array_size": 8}), ("simple_race", {"track_width": 20.0, "track_length": 100.0, "track_radius": 30.0})):
        sim = BatchedSimulator(game, opts, num_envs=8)
        rc = sim.L.xwb_xw_expert(sim.h, C.c_void_p(buf.data_ptr()), None, None, 0, None)
        assert rc == -1 and b"xworld" in sim.L.xwb_last_error()
        sim.close()
    sim = BatchedSimulator("xworld", {"xwd_conf_path": os.path.join(cases.CONF, "walls.json")}, num_envs=8)
    with pytest.raises(XwbError, match="2-D-native"):
        sim.expert()
    sim.close()
    for extra in ({}, {"task_mode": "one_channel", "task_groups_exclusive": True, "max_steps": 45}):     # the 3-D group second
        sim = BatchedSimulator("xworld", dict({"xwd_conf_path": cases.NAV2D, "task_mode": "lang_acquisition", "max_dim": 7,
                                               "num_blocks": 6, "tasks": cases.T2, "tasks2": cases.T3}, **extra), num_envs=8)
        with pytest.raises(XwbError, match="SECOND group"):
            sim.expert()
        sim.close()
    sim = cases.make_sim("nav7_one", 8)
    rc = sim.L.xwb_xw_expert(sim.h, None, None, None, 0, None)
    assert rc == -1 and b"both NULL" in sim.L.xwb_last_error()
    _, d = sim.expert(no_path=-1)                                    # then dist alone into the caller's buffer
    assert sim.L.xwb_xw_expert(sim.h, None, C.c_void_p(buf.data_ptr()), None, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:8], d)
    assert sim.expert_field_dims == (1, 49)
    sim.close()
