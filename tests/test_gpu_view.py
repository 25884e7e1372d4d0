"""Native-resolution views on the device (xwb_xw_render_view / BatchedSimulator.render_view) against the oracle's own
XMap::to_image (orc_xw_get_grid + the icon atlas under full observation, orc_xw_agent_view in egocentric mode), against the
frames the batch already draws (a view pushed through the oracle's resizes IS the env's newest frame) and against the one
rendered frame the reference holds (tests/golden/xworld2d_doc.png) -- byte for byte everywhere.  Expected values come from
tests/test_view_expected.py, which pins them to the oracle without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import test_gpu_ego as E
import test_gpu_xworld as X
from test_gpu_xworld import _torch
from test_oracle_tasks import KINDS
from test_view_expected import canvas_from_grid, frame_from_view

pytestmark = pytest.mark.gpu

ERR_ARG = -1                                                                   # include/xwb.h XWB_ERR_ARG

CONF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xworld_amd", "confs")


def _newest(sim):
    """the newest frame of every env, uint8 [n, c, h, w] (float32 batches: checked to be frame * float32(1 / 255) exactly)"""
    c = sim.screen_dims[2]
    obs = sim.obs[:, -c:].cpu().numpy()
    if sim.obs_is_float:
        u8 = np.rint(obs * 255.0).astype(np.uint8)
        assert np.array_equal(u8.astype(np.float32) * np.float32(1 / 255.0), obs)
        return u8
    return obs


class FrameCheck:
    """view -> frame for every env of a batch at every point of a rollout.  A view that has not changed since the last point
    (compared on the device) keeps the frame computed from it then; the frame is compared with the CURRENT obs either way."""

    def __init__(self, oracle, sim, color):
        self.oracle, self.sim, self.color = oracle, sim, color
        self.prev = None
        self.frames = [None] * sim.num_envs
        self.world_px = 64 * sim.cfg.max_dim
        self.checked = 0

    def check(self, views, where, zero_ok=()):
        """views: the device tensor of all envs.  zero_ok: envs whose slot is documented as zero-filled (none on any path today)."""
        sim = self.sim
        n = sim.num_envs
        if self.prev is None:
            changed = np.ones(n, bool)
        else:
            changed = (views != self.prev).reshape(n, -1).any(dim=1).cpu().numpy()
        self.prev = views.clone()
        idx = np.nonzero(changed)[0]
        if len(idx):
            host = views[_torch().from_numpy(idx).to(views.device)].cpu().numpy()
            for k, e in enumerate(idx):
                self.frames[e] = frame_from_view(self.oracle, host[k], self.world_px, sim.screen_dims[0], self.color)
        obs = _newest(sim)
        for e in range(n):
            assert e not in zero_ok
            assert np.array_equal(self.frames[e], obs[e]), (where, e, int((self.frames[e] != obs[e]).sum()))
            self.checked += 1


def _canvases(torch, grids, icons64):
    """canvas_from_grid for a whole batch, on the device: grids int [n, D, D] -> [n, 64 D, 64 D, 3]"""
    n, d, _ = grids.shape
    atlas = torch.cat([torch.full((1, 64, 64, 3), 255, dtype=torch.uint8), torch.from_numpy(icons64)]).cuda()
    c = atlas[torch.from_numpy(grids.astype(np.int64)).cuda()]                     # [n, D, D, 64, 64, 3]
    return c.permute(0, 1, 3, 2, 4, 5).reshape(n, 64 * d, 64 * d, 3)


FULL_CASES = [(k, c, {}) for k in ("nav7", "nav8", "nav8_dim5", "walls7") for c in (False, True)]
EXTRA_CASES = [("nav7", True, dict(context=2)), ("nav8", False, dict(obs_format="float32"))]


@pytest.mark.parametrize("key,color,extra", FULL_CASES + EXTRA_CASES)
def test_full_observation_views_against_oracle_and_frames(oracle, key, color, extra):
    """Tests 1 and 2 of the feature on one rollout: 256 envs in lock-step with per-env oracle worlds under the built-in policy,
    the default loop (step, reset_done), views after the reset, after every step and after every reset_done.  Every env's view
    equals canvas_from_grid(oracle grid) -- after a step a finished env shows the oracle's state BEFORE its reset_game -- and
    every env's view pushed through the resize is the env's newest frame."""
    torch = _torch()
    n, steps = 256, 40
    sim, pal, cfg = X._make(oracle, key, n, seed=31, policy_seed=9, color=color, **extra)
    d = cfg["max_dim"]
    assert sim.view_dims == (64 * d, 64 * d, 3)
    envs = [oracle.XWorld(pal, render=False, **cfg) for _ in range(n)]
    ep = [0] * n
    for e, w in enumerate(envs):
        w.reset_game(e, 0)
    fc = FrameCheck(oracle, sim, color)
    resets = 0

    def point(where):
        views = sim.render_view()
        assert views.shape == (n, 64 * d, 64 * d, 3) and views.dtype == torch.uint8
        grids = np.stack([w.grid().reshape(d, d) for w in envs])
        exp = _canvases(torch, grids, pal.icons64)
        bad = (views != exp).reshape(n, -1).any(dim=1)
        assert not bool(bad.any()), (where, "envs", torch.nonzero(bad).flatten().tolist()[:8])
        for e in (0, n // 2, n - 1):                                               # the device gather is the CPU helper
            assert np.array_equal(exp[e].cpu().numpy(), canvas_from_grid(grids[e], pal.icons64))
        fc.check(views, where)

    point("reset")
    for t in range(steps):
        sim.step()
        acts = sim.actions.cpu().numpy()
        codes = sim.game_over_codes.cpu().numpy()
        for e, w in enumerate(envs):
            w.take_actions(int(acts[e]))
            assert w.game_over() == codes[e], (t, e)
        point(("step", t))
        sim.reset_done()
        for e, w in enumerate(envs):
            if codes[e]:
                ep[e] += 1
                resets += 1
                w.reset_game(e, ep[e])
        point(("reset_done", t))
    assert resets > 0 and sim.check_errors() == 0
    assert fc.checked == n * (2 * steps + 1)
    sim.close()


def _load_host_poses(oracle, sim, pal, cfg, n):
    """as test_ego_frames_with_host_poses: the oracle's maps and goal poses go into the product through the host"""
    envs = []
    for e in range(n):
        w = oracle.XWorld(pal, render=True, **cfg)
        w.reset_game(e, 0)
        envs.append(w)
        g = w.grid().astype(np.uint16)
        ax, ay = w.agent_xy()
        g[w.target_cells() != 0] |= 0x8000
        sim.load_map(e, g, ax, ay, dim=cfg["dim"], task=KINDS[0], target=w.target_name())
        sim.set_agent_dir(e, E._facing(w.agent_yaw()))
        for i, ent in enumerate(w.entities()):
            if ent[0] == 0:
                sim.set_goal_pose(e, ent[1], ent[2], *w.get_pose(i))
        sim.refresh_obs(e)
    return envs


@pytest.mark.parametrize("key,r,color,shadow", [("nav7", 1, True, True), ("nav7", 3, True, True), ("nav8", 3, False, False),
                                                ("nav8", 5, False, True), ("nav7", 7, True, True), ("nav11", 9, True, True)])
def test_ego_views_with_host_poses(oracle, key, r, color, shadow):
    """Test 3 (a) and (c): 48 envs, 14 random action steps; view[e] == the oracle's agent_view() at every step, and the view pushed
    through the two resizes is the env's frame (every env, finished ones included: the library holds their state until a reset)."""
    torch = _torch()
    n, steps = 48, 14
    opts = {} if shadow else dict(wall_shadow=False)
    sim, pal, cfg = E._make(oracle, key, n, r, tasks=[KINDS[0]], seed=5, color=color, **opts)
    if not shadow:
        cfg["no_wall_shadow"] = 1
    envs = _load_host_poses(oracle, sim, pal, cfg, n)
    assert sim.view_dims == (64 * r, 64 * r, 3)
    fc = FrameCheck(oracle, sim, color)
    rng = np.random.default_rng(1)
    for t in range(steps + 1):
        views = sim.render_view()
        host = views.cpu().numpy()
        for e, w in enumerate(envs):
            exp = w.agent_view()
            assert np.array_equal(host[e], exp), (t, e, int((host[e] != exp).sum()))
        fc.check(views, t)
        acts = rng.integers(0, 6, n).astype(np.int32)
        sim.step(torch.from_numpy(acts).cuda())
        for e, w in enumerate(envs):
            w.take_actions(int(acts[e]))
    assert sim.check_errors() == 0
    sim.close()


@pytest.mark.parametrize("key,r", [("nav7", 3), ("nav8", 5)])
def test_ego_views_device_poses_rollout(oracle, trig, key, r):
    """Test 3 (b) and (c): poses drawn by the reset kernel, 128 envs x 64 steps of the default loop with resets, against the libm
    oracle and the xwb_trig one; differing envs / bytes are counted over the whole run, the gate is 0.  After a step a finished env
    is compared with the oracle's world before its reset_game -- heading, goal images and map are still the library's."""
    _torch()
    n, steps = 128, 64
    sim, pal, cfg = E._make(oracle, key, n, r, seed=29, policy_seed=6, color=True)
    envs = [oracle.XWorld(pal, render=True, **cfg) for _ in range(n)]
    ep = [0] * n
    for e, w in enumerate(envs):
        w.reset_game(e, 0)
    fc = FrameCheck(oracle, sim, True)
    bad_views = bad_bytes = resets = finished_compared = 0

    oview = [None] * n                                      # the oracle's views, redrawn for the worlds that moved since the last point

    def point(where, codes=None, moved=None):
        nonlocal bad_views, bad_bytes, finished_compared
        views = sim.render_view()
        host = views.cpu().numpy()
        for e, w in enumerate(envs):
            if moved is None or e in moved:
                oview[e] = w.agent_view()
            dlt = int((host[e] != oview[e]).sum())
            bad_views += dlt > 0
            bad_bytes += dlt
            if codes is not None and codes[e]:
                finished_compared += 1
        fc.check(views, where)

    point("reset")
    for t in range(steps):
        sim.step()
        acts = sim.actions.cpu().numpy()
        codes = sim.game_over_codes.cpu().numpy()
        for e, w in enumerate(envs):
            w.take_actions(int(acts[e]))
            assert w.game_over() == codes[e], (t, e)
        point(("step", t), codes)
        sim.reset_done()
        for e, w in enumerate(envs):
            if codes[e]:
                ep[e] += 1
                resets += 1
                w.reset_game(e, ep[e])
        point(("reset_done", t), moved=set(np.nonzero(codes)[0].tolist()))
    total = n * (2 * steps + 1)
    print("trig=%s %s r=%d: %d of %d views differ (%d bytes); %d resets" % (trig, key, r, bad_views, total, bad_bytes, resets))
    assert sim.check_errors() == 0
    sim.close()
    assert resets > 8 and finished_compared == resets
    assert bad_views == 0, "trig=%s: %d of %d views differ (%d bytes)" % (trig, bad_views, total, bad_bytes)


def test_ego_autoreset_views_are_the_frames(oracle):
    """xwb_step_autoreset on an egocentric batch: the finished envs already show their next episode, in the frame and in the view."""
    _torch()
    sim, pal, cfg = E._make(oracle, "nav7", 96, 3, seed=3, policy_seed=2, color=False, max_steps=9)
    fc = FrameCheck(oracle, sim, False)
    done = 0
    for t in range(24):
        sim.step_autoreset()
        done += int((sim.game_over_codes != 0).sum())
        fc.check(sim.render_view(), t)
    assert done > 0 and sim.check_errors() == 0
    sim.close()


@pytest.mark.parametrize("dim,agent", [(5, (2, 4)), (8, (3, 6))])
def test_view_equals_the_reference_image(oracle, dim, agent):
    """Test 4: the map of the reference's rendered frame (tests/golden/xworld2d_doc.png) loaded as tests/test_gpu_doc_image.py
    does; the kernels' view equals the reference's own 319 pixel lines with 0 differing bytes, no resize in between.  The PNG
    lacks the view's last line: that one is compared with the oracle's agent_view()."""
    _torch()
    from xworld_amd.batched import BatchedSimulator
    from test_oracle_doc_image import R, doc_view, doc_world
    sim = BatchedSimulator("xworld", {"xwd_conf_path": os.path.join(CONF, "nav_target.json"), "max_dim": dim, "dim": dim,
                                      "task_mode": "lang_acquisition", "tasks": ["XWorld3DNavTarget"],
                                      "visible_radius": R, "color": True, "num_goals": 3, "num_blocks": 4}, num_envs=4)
    w, ents, poses = doc_world(oracle, dim, agent, color=1)
    g = np.zeros((dim, dim), np.uint16)
    for t, x, y, icon, name, serial in ents:
        g[y, x] = icon + 1
    g[w.target_cells() != 0] |= 0x8000
    for e in (1, 3):
        sim.load_map(e, g, agent[0], agent[1], dim=dim, task="XWorld3DNavTarget", target=w.target_name())
        sim.set_agent_dir(e, 3)
        for (t, x, y, icon, name, serial), (yaw, scale, offset) in zip(ents, poses):
            if t == 0:
                sim.set_goal_pose(e, x, y, yaw, scale, offset)
        sim.refresh_obs(e)
    views = sim.render_view([1, 3]).cpu().numpy()
    ref, full = doc_view(), w.agent_view()
    assert views.shape == (2, 64 * R, 64 * R, 3) and ref.shape == (64 * R - 1, 64 * R, 3)
    for k in range(2):
        assert int((views[k, :319] != ref).sum()) == 0
        assert np.array_equal(views[k, 319], full[319])
    sim.close()


def test_selection_and_errors(oracle):
    """Test 5: index lists, the zero slot of an index outside the batch, XWB_ERR_ARG cases, out= reuse, a stream of the caller's."""
    torch = _torch()
    from xworld_amd import lib
    from xworld_amd.batched import BatchedSimulator
    n = 24
    for sim in (X._make(oracle, "nav7", n, seed=4, color=False)[0], E._make(oracle, "nav7", n, 3, seed=4)[0]):
        for _ in range(3):
            sim.step()
        allv = sim.render_view()
        h, w, c = sim.view_dims
        assert allv.shape == (n, h, w, 3)
        assert torch.equal(sim.render_view(5), allv[:5])
        pick = [7, 7, 23, 0, 3, 3, 1]
        assert torch.equal(sim.render_view(pick), allv[pick])                                     # host list, repeats
        rev = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")
        assert torch.equal(sim.render_view(rev), allv.flip(0))                                    # device list, reversed
        assert torch.equal(sim.render_view(torch.tensor([2, 2, 9], dtype=torch.int32)), allv[[2, 2, 9]])   # CPU tensor
        assert sim.render_view([]).shape == (0, h, w, 3) and sim.render_view(0).shape == (0, h, w, 3)
        with pytest.raises(IndexError):
            sim.render_view([0, n])
        # an index outside the batch in a DEVICE list: a zero slot, the others drawn, no error counted
        odd = torch.tensor([1, n, -1, 2 ** 30, 5], dtype=torch.int32, device="cuda")
        got = sim.render_view(odd)
        assert torch.equal(got[0], allv[1]) and torch.equal(got[4], allv[5])
        assert int(got[1:4].max()) == 0 and int(allv[1].max()) > 0
        assert sim.check_errors() == 0
        # out= reuse: the same storage comes back
        buf = torch.full((3, h, w, 3), 7, dtype=torch.uint8, device="cuda")
        back = sim.render_view([4, 5, 6], out=buf)
        assert back.data_ptr() == buf.data_ptr() and torch.equal(buf, allv[4:7])
        with pytest.raises(ValueError):
            sim.render_view(2, out=buf)
        # the C ABI's own refusals: nothing is launched, the buffer stays as it was
        buf.fill_(9)
        torch.cuda.synchronize()
        per = h * w * 3
        rv = sim.L.xwb_xw_render_view
        assert rv(sim.h, None, 3, C.c_void_p(buf.data_ptr()), 3 * per - 1, None) == ERR_ARG            # one byte short
        assert rv(sim.h, None, n + 1, C.c_void_p(buf.data_ptr()), (n + 1) * per, None) == ERR_ARG    # n > num_envs
        assert rv(sim.h, None, -1, C.c_void_p(buf.data_ptr()), 3 * per, None) == ERR_ARG
        assert rv(sim.h, None, 0, None, 0, None) == 0                                                         # a no-op
        torch.cuda.synchronize()
        assert int(buf.min()) == 9 and int(buf.max()) == 9
        # a stream of the caller's (BatchedSimulator._stream probes it on first use)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            on_st = sim.render_view(stream=st)
        st.synchronize()
        assert torch.equal(on_st, allv)
        assert sim.check_errors() == 0
        sim.close()
    sg = BatchedSimulator("simple_game", {"array_size": 8}, num_envs=8)
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    assert sg.L.xwb_xw_render_view(sg.h, None, 1, C.c_void_p(buf.data_ptr()), 1024, None) == ERR_ARG
    hh = C.c_size_t()
    assert sg.L.xwb_xw_view_dims(sg.h, C.byref(hh), None, None) == ERR_ARG
    with pytest.raises(lib.XwbError):
        sg.render_view()
    sg.close()


def _rollout(sim, steps, autoreset, look):
    """rewards, codes, obs and step paths of `steps` iterations of the loop; look: render_view(16) after every verb"""
    torch = _torch()
    rec = []
    peek = lambda: sim.render_view(16) if look else None
    peek()
    for t in range(steps):
        if autoreset:
            sim.step_autoreset()
        else:
            sim.step()
        path = sim.step_path()["path"]
        peek()
        rec.append((sim.reward.clone(), sim.game_over_codes.clone(), sim.obs.clone(), path))
        if not autoreset:
            sim.reset_done()
            peek()
            rec.append((sim.obs.clone(),))
    torch.cuda.synchronize()
    return rec


@pytest.mark.parametrize("kind", ["default", "autoreset", "ego"])
def test_views_change_nothing(oracle, kind):
    """Test 6: the same rollout twice from the same seeds, once with render_view(16) after every verb: rewards, codes and obs are
    identical step for step and xwb_step_path reports the same path on the same steps (xworld7 defaults: the fused one)."""
    torch = _torch()
    recs = []
    for look in (False, True):
        if kind == "ego":
            sim = E._make(oracle, "nav7", 1024, 3, seed=8, policy_seed=3)[0]
            steps = 20
        else:
            sim = X._make(oracle, "nav7", 1024, seed=8, policy_seed=3)[0]
            steps = 60
        recs.append(_rollout(sim, steps, kind == "autoreset", look))
        assert sim.check_errors() == 0
        sim.close()
    a, b = recs
    assert len(a) == len(b)
    finished = 0
    for i, (ra, rb) in enumerate(zip(a, b)):
        for xa, xb in zip(ra, rb):
            if isinstance(xa, torch.Tensor):
                assert torch.equal(xa, xb), (kind, i)
            else:
                assert xa == xb, (kind, i, xa, xb)
        if len(ra) > 1:
            finished += int((ra[1] != 0).sum())
    assert finished > 0
    if kind == "default":
        fused = [r[3] == "lazy_fused" for r in b if len(r) > 1]
        assert sum(fused) >= len(fused) - 2, fused                                 # (every step but the first ones)
