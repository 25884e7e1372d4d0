"""xwb_xw_evaluate_plans / BatchedSimulator.evaluate_plans on the GPU: every plan of every env against the oracle (steps, code,
last, return bits at two gammas; the cases and seeds of tests/_plans_cases.py, whose coverage tests/test_plans_host.py holds),
against the batch's own forks stepped by the real kernels, "it reads only", agreement with the expert, the edges and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import _expert_cases as ec
import _plans_cases as pc

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _dev(torch, a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _play_prefix(torch, sim, name):
    """the case's prefix with step + reset_done; the test's own record of episode counters and actions since the last reset"""
    rec = pc.Record()
    rep = pc.CASES[name]["act_rep"]
    for acts in pc.prefix_actions(name):
        sim.step(_dev(torch, acts, torch.int32), act_rep=rep)
        rec.add(acts, sim.game_over_codes.cpu().numpy())
        sim.reset_done()
    return rec


def _same_bytes(a, b):
    """equal shapes and equal bytes (float returns compared as bits; slices need not be contiguous)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_every_plan_against_the_oracle(oracle, name):
    torch = _torch()
    c = pc.CASES[name]
    want_rec, steps, codes, last, rewards = pc.expected(name)
    need = pc.required(name)
    assert need <= pc.coverage(name), need - pc.coverage(name)        # the coverage condition (seeds: tests/test_plans_host.py)
    sim = pc.make_sim(name)
    rec = _play_prefix(torch, sim, name)
    assert np.array_equal(rec.episode, want_rec.episode) and rec.since == want_rec.since
    assert np.array_equal(sim.episode.cpu().numpy(), rec.episode)
    plans = _dev(torch, pc.plans(name), torch.int8)
    for gamma in pc.GAMMAS:
        ret, st, cd, la = (t.cpu().numpy() for t in sim.evaluate_plans(plans, gamma=gamma, act_rep=c["act_rep"], last=True))
        print(name, "gamma", gamma, "steps differ", int((st != steps).sum()), "codes differ", int((cd != codes).sum()),
              "last differ", int((la != last).sum()))
        want = np.array([[pc.returns_f32(rewards[e][k], gamma) for k in range(pc.K)] for e in range(pc.N)], np.float32)
        print(name, "gamma", gamma, "returns differ", int((_bits(ret) != _bits(want)).sum()))
        assert np.array_equal(st, steps), np.argwhere(st != steps)[:5]
        assert np.array_equal(cd, codes), np.argwhere(cd != codes)[:5]
        assert np.array_equal(la, last), np.argwhere(la != last)[:5]
        assert np.array_equal(_bits(ret), _bits(want)), np.argwhere(_bits(ret) != _bits(want))[:5]
    assert sim.check_errors() == 0
    sim.close()


# ------------------------------------------------------------------ 2. against the batch's own forks
@pytest.mark.parametrize("radius", [0, 5])
def test_against_forks_stepped_by_the_step_kernels(radius):
    torch = _torch()
    from xworld_amd.batched import BatchedSimulator
    R, K, H, gamma = 64, 5, 8, 0.9
    opts = {"xwd_conf_path": ec.NAV2D, "task_mode": "lang_acquisition", "tasks": ec.T3, "max_dim": 7, "num_blocks": 12}
    if radius:
        opts["visible_radius"] = radius
    sim = BatchedSimulator("xworld", opts, num_envs=R * (K + 1), seed=3, policy_seed=9)
    na = sim.num_actions
    rng = np.random.RandomState(7 + radius)
    for _ in range(4):                                         # leave the first step of the episodes
        sim.step(_dev(torch, rng.randint(0, na, sim.num_envs), torch.int32))
        sim.reset_done()
    plans_h = np.where(rng.rand(R, K, H) < 0.5, 0 if radius else 1, rng.randint(0, na, (R, K, H))).astype(np.int8)
    roots = torch.arange(R, dtype=torch.int32, device="cuda")
    ret, st, cd = (t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, plans_h, torch.int8), gamma=gamma, envs=roots))
    # the fork route: child slot R + r * K + k takes plan k of root r
    sim.copy_envs(torch.arange(R, R * (K + 1), dtype=torch.int32, device="cuda"),
                  torch.arange(R, dtype=torch.int32, device="cuda").repeat_interleave(K))
    rewards = [[[] for _ in range(K)] for _ in range(R)]
    f_steps, f_code = np.zeros((R, K), int), np.zeros((R, K), int)
    live = np.ones((R, K), bool)
    for t in range(H):
        acts = np.full(sim.num_envs, pc.SKIP, np.int32)
        acts[R:] = np.where(live, plans_h[:, :, t], pc.SKIP).reshape(-1)
        sim.step(_dev(torch, acts, torch.int32))
        rw = sim.reward.cpu().numpy()[R:].reshape(R, K)
        co = sim.game_over_codes.cpu().numpy()[R:].reshape(R, K)
        for r, k in np.argwhere(live):
            rewards[r][k].append(rw[r, k])
            f_steps[r, k] += 1
            if co[r, k]:
                f_code[r, k] = co[r, k]
                live[r, k] = False
        sim.reset_done()
    want = np.array([[pc.returns_f32(rewards[r][k], gamma) for k in range(K)] for r in range(R)], np.float32)
    assert (f_code != 0).sum() > R * K // 20 and live.sum() > R * K // 20     # both kinds of plans took part
    assert np.array_equal(st, f_steps), np.argwhere(st != f_steps)[:5]
    assert np.array_equal(cd, f_code), np.argwhere(cd != f_code)[:5]
    assert np.array_equal(_bits(ret), _bits(want)), np.argwhere(_bits(ret) != _bits(want))[:5]
    assert sim.check_errors() == 0
    sim.close()


# ------------------------------------------------------------------ 3. it reads only
def _call(torch, sim, plans):
    sim.evaluate_plans(plans, gamma=0.9, last=True)


@pytest.mark.parametrize("name", ["dim5_five_tasks", "ego3"])
def test_state_blob_and_step_path_unchanged(name):
    torch = _torch()
    sim = pc.make_sim(name)
    _play_prefix(torch, sim, name)
    plans = _dev(torch, pc.plans(name), torch.int8)
    for where in ("after reset_done", "between step and reset_done"):
        if where.startswith("between"):
            sim.step(_dev(torch, pc.prefix_actions(name)[0], torch.int32))
        blob, path = sim.save_state(include_obs=True), sim.step_path()
        _call(torch, sim, plans)
        torch.cuda.synchronize()
        assert np.array_equal(sim.save_state(include_obs=True), blob), where
        assert sim.step_path() == path, where
    sim.close()


@pytest.mark.parametrize("case", ["default_loop", "ego"])
def test_rollout_is_the_same_with_calls_in_between(case):
    torch = _torch()
    from xworld_amd.batched import BatchedSimulator
    opts = {"xwd_conf_path": ec.NAV2D, "task_mode": "lang_acquisition", "max_dim": 7, "num_blocks": 16, "color": True}
    n = 1024 + 37
    if case == "ego":
        opts.update(visible_radius=3)
        n = 256 + 5
    a = BatchedSimulator("xworld", opts, num_envs=n, seed=11, policy_seed=5)
    b = BatchedSimulator("xworld", opts, num_envs=n, seed=11, policy_seed=5)
    plans = torch.randint(0, a.num_actions, (n, 3, 5), dtype=torch.int8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    a.reset(); b.reset()
    _call(torch, a, plans)
    paths = set()
    for t in range(20):
        a.step(); b.step()
        _call(torch, a, plans)
        paths.add(a.step_path()["path"])
        assert a.step_path() == b.step_path(), t
        assert torch.equal(a.reward, b.reward) and torch.equal(a.game_over_codes, b.game_over_codes) and torch.equal(a.obs, b.obs), t
        a.reset_done(); b.reset_done()
        _call(torch, a, plans)
        assert torch.equal(a.obs, b.obs) and torch.equal(a.grid, b.grid) and torch.equal(a.episode, b.episode), t
    if case == "default_loop":
        assert "lazy_fused" in paths, paths                    # the one-launch step of the default loop took part
    # (the blob of ONE batch before and after a call: test_state_blob_and_step_path_unchanged; two batches' blobs also hold their
    # done lists, which the step kernel's wavefronts append in whatever order they run)
    assert torch.equal(a.num_steps, b.num_steps) and torch.equal(a.success, b.success) and torch.equal(a.actions, b.actions)
    assert a.task_performance() == b.task_performance()
    assert a.check_errors() == 0
    a.close(); b.close()


# ------------------------------------------------------------------ 4. agreement with the expert
@pytest.mark.parametrize("name", ["nav8_five", "ego3"])
def test_single_actions_agree_with_the_expert(name):
    torch = _torch()
    n = 512
    sim = ec.make_sim(name, n)
    na = sim.num_actions
    for _ in range(3):
        sim.step()
        sim.reset_done()
    plans = torch.arange(na, dtype=torch.int8, device="cuda").reshape(1, na, 1).repeat(n, 1, 1).contiguous()
    ret, st, cd = (t.cpu().numpy() for t in sim.evaluate_plans(plans))
    act, dist = (t.cpu().numpy() for t in sim.expert())
    wins = (cd & pc.SUCCESS) != 0
    assert (st == 1).all()
    assert np.array_equal(wins.any(axis=1), dist == 1)
    assert (dist == 1).sum() > 0
    for e in np.nonzero(dist == 1)[0]:
        assert wins[e, act[e]] and not wins[e, :act[e]].any(), e          # the expert's is the lowest winning id
    assert np.array_equal(_bits(ret[wins]), _bits(np.full(wins.sum(), np.float32(-0.01 + 1.0))))
    sim.close()


# ------------------------------------------------------------------ 5. edges
def test_edges():
    torch = _torch()
    name = "dim5_five_tasks"
    sim = pc.make_sim(name)
    _play_prefix(torch, sim, name)
    p_h = pc.plans(name)
    plans = _dev(torch, p_h, torch.int8)
    full = [t.cpu().numpy().copy() for t in sim.evaluate_plans(plans, gamma=0.5, last=True)]

    # a subset with repeats, and an index outside the batch
    idx = np.array([5, 0, 5, 47, pc.N, -1, 17], np.int32)
    rows = np.clip(idx, 0, pc.N - 1)
    sub = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, p_h[rows], torch.int8), gamma=0.5, last=True, envs=_dev(torch, idx, torch.int32))]
    ok = (idx >= 0) & (idx < pc.N)
    # (row i holds the plans of env rows[i]: the answers are those of that env)
    for got, want in zip(sub, full):
        assert _same_bytes(got[ok], want[rows[ok]])
    r, s, c, l = sub
    assert (s[~ok] == -1).all() and (r[~ok] == 0).all() and (c[~ok] == 0).all() and (l[~ok] == -1).all()
    assert sim.check_errors() == 2                             # one per bad index, not per plan

    # XWB_ACTION_SKIP pads a ragged plan: steps = the prefix length (or the earlier end), everything else that of the truncated plan
    for cut in (0, 3, 7):
        padded = p_h.copy()
        padded[:, :, cut:] = pc.SKIP
        got = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, padded, torch.int8), gamma=0.5, last=True)]
        if cut:
            trunc = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, np.ascontiguousarray(p_h[:, :, :cut]), torch.int8), gamma=0.5, last=True)]
            for g, w in zip(got, trunc):
                assert _same_bytes(g, w), cut
            assert np.array_equal(got[1], np.minimum(full[1], cut))
        else:
            st0 = sim.env_state(3)
            assert (got[1] == 0).all() and (got[0] == 0).all() and (got[2] == 0).all()
            assert got[3][3, 0] == st0.xw_agent_y * sim.cfg.max_dim + st0.xw_agent_x
    assert sim.check_errors() == 0

    # an illegal id ends the plan and is counted once per plan that reaches it
    bad = p_h.copy()
    bad[:, :, 4] = 4                                           # full observation: ids 0 .. 3
    bad[:, 0, 2] = -7
    got = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, bad, torch.int8), gamma=0.5, last=True)]
    lim = np.full((pc.N, pc.K), 4)
    lim[:, 0] = 2
    assert np.array_equal(got[1], np.minimum(full[1], lim))
    assert sim.check_errors() == int((full[1] > lim).sum())   # (a plan that ended before the bad id never sees it)

    # K = 1, K = 70 (more plans than lanes), H = 1; byte-wide, 4-byte and 16-byte plan pieces
    rng = np.random.RandomState(5)
    big = rng.randint(0, 4, (pc.N, 70, 16)).astype(np.int8)
    big[:, :pc.K, :pc.H] = p_h
    big[:, :pc.K, pc.H:] = pc.SKIP
    g70 = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, big, torch.int8), gamma=0.5, last=True)]
    for g, w in zip(g70, full):
        assert _same_bytes(g[:, :pc.K], w)
    for k in (0, 63, 64, 69):                                  # every plan of the 70 equals the same plan evaluated alone (K = 1)
        one = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, big[:, k:k + 1], torch.int8), gamma=0.5, last=True)]
        for g, w in zip(one, g70):
            assert _same_bytes(g[:, 0], w[:, k]), k
    for width in (12, 7):                                      # 4-byte pieces; single bytes (also at an odd buffer offset)
        cutp = np.ascontiguousarray(big[:, :, :width])
        g = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, cutp, torch.int8), gamma=0.5, last=True)]
        w16 = big.copy()
        w16[:, :, width:] = pc.SKIP
        w = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, w16, torch.int8), gamma=0.5, last=True)]
        for x, y in zip(g, w):
            assert _same_bytes(x, y), width
    h1 = [t.cpu().numpy() for t in sim.evaluate_plans(_dev(torch, np.ascontiguousarray(p_h[:, :, :1]), torch.int8), gamma=0.5, last=True)]
    assert (h1[1] == 1).all()

    # outputs one at a time, the rest NULL
    for j in range(4):
        out = [None] * 4
        out[j] = torch.zeros((pc.N, pc.K), dtype=(torch.float32, torch.int32, torch.uint8, torch.int32)[j], device="cuda")
        res = sim.evaluate_plans(plans, gamma=0.5, last=True, out=out)
        assert [x is None for x in res] == [i != j for i in range(4)]
        assert _same_bytes(res[j].cpu().numpy(), full[j]), j
    # the method's own tensors are reused between calls
    assert sim.evaluate_plans(plans)[0].data_ptr() == sim.evaluate_plans(plans)[0].data_ptr()

    # between step and reset_done a finished env reports steps 0 with its code and its node; the others are evaluated
    ends = np.nonzero((full[2] != 0) & (full[1] == 1))
    assert len(ends[0]) > 0                                    # plans that end the episode with their first action
    acts = np.full(pc.N, 1, np.int32)
    acts[ends[0]] = p_h[ends[0], ends[1], 0]
    sim.step(_dev(torch, acts, torch.int32))
    codes = sim.game_over_codes.cpu().numpy()
    done = codes != 0
    assert done[ends[0]].all() and not done.all()
    r, s, c, l = (t.cpu().numpy() for t in sim.evaluate_plans(plans, gamma=0.5, last=True))
    assert (s[done] == 0).all() and (r[done] == 0).all() and np.array_equal(c[done], np.repeat(codes[done][:, None], pc.K, 1))
    e = int(ends[0][0])
    st = sim.env_state(e)
    assert (l[e] == st.xw_agent_y * sim.cfg.max_dim + st.xw_agent_x).all()
    assert (s[~done] >= 1).all()
    sim.reset_done()
    assert (sim.evaluate_plans(plans)[1].cpu().numpy() >= 1).all()
    sim.close()


# ------------------------------------------------------------------ 6. refusals
def _raw(sim, torch, **kw):
    """the C ABI itself, with valid arguments unless overridden"""
    from xworld_amd import lib
    n = sim.num_envs
    keep = dict(plans=torch.zeros((n, 2, 3), dtype=torch.int8, device="cuda"), ret=torch.zeros((n, 2), device="cuda"),
                steps=torch.zeros((n, 2), dtype=torch.int32, device="cuda"), code=torch.zeros((n, 2), dtype=torch.uint8, device="cuda"),
                last=torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
    a = dict(envs=None, n=n, plans=keep["plans"].data_ptr(), n_plans=2, horizon=3, act_rep=1, gamma=1.0, ret=keep["ret"].data_ptr(),
             steps=keep["steps"].data_ptr(), code=keep["code"].data_ptr(), last=keep["last"].data_ptr())
    a.update(kw)
    rc = lib.load().xwb_xw_evaluate_plans(sim.h, a["envs"], a["n"], a["plans"], a["n_plans"], a["horizon"], a["act_rep"], a["gamma"],
                                          a["ret"], a["steps"], a["code"], a["last"], None)
    torch.cuda.synchronize()
    return rc, keep


def test_refusals():
    torch = _torch()
    from xworld_amd import lib
    from xworld_amd.batched import BatchedSimulator
    ERR_ARG = -1
    conf = os.path.join(ec.CONF, "nav_two_groups.json")
    refused = [BatchedSimulator("simple_game", {"array_size": 8}, num_envs=16),
               BatchedSimulator("xworld", {"xwd_conf_path": conf, "task_mode": "lang_acquisition"}, num_envs=16),
               BatchedSimulator("xworld", {"xwd_conf_path": os.path.join(ec.CONF, "walls.json"), "task_mode": "one_channel", "max_steps": 30}, num_envs=16)]
    assert refused[1].cfg.n_tasks2 > 0
    for sim in refused:
        blob = sim.save_state()
        rc, keep = _raw(sim, torch)
        assert rc == ERR_ARG, sim.name
        assert all(int(t.abs().sum()) == 0 for k, t in keep.items() if k != "plans")        # nothing launched
        assert np.array_equal(sim.save_state(), blob) and sim.check_errors() == 0
        with pytest.raises(lib.XwbError):
            sim.evaluate_plans(torch.zeros((16, 2, 3), dtype=torch.int8, device="cuda"))
        sim.close()
    sim = pc.make_sim("dim5_five_tasks")
    blob = sim.save_state()
    assert _raw(sim, torch)[0] == 0
    for kw in (dict(plans=None), dict(n_plans=0), dict(horizon=0), dict(act_rep=0), dict(ret=None, steps=None, code=None, last=None),
               dict(gamma=float("nan")), dict(gamma=float("inf")),
               dict(envs=torch.zeros(4, dtype=torch.int32, device="cuda").data_ptr(), n=-1)):
        rc, keep = _raw(sim, torch, **kw)
        assert rc == ERR_ARG, kw
        assert b"" != lib.load().xwb_last_error()
        assert all(int(t.abs().sum()) == 0 for k, t in keep.items() if k != "plans"), kw
    assert np.array_equal(sim.save_state(), blob) and sim.check_errors() == 0
    # NULL env list: n is ignored
    rc, keep = _raw(sim, torch, n=-5)
    assert rc == 0 and (keep["steps"].cpu().numpy() >= 1).all()
    sim.close()
