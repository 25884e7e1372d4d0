"""The egocentric mode past the sizes tests/test_gpu_ego.py runs: maps of 12 to 16 cells (more than 192 cells: the fourth grid
cell per lane of the one-workgroup-per-env render), radii 13 and 15 (78 and 75 pixel edges), up to 16 goals (goals next to
goals, slots 4-15, the goal-cell cache's limit num_goals * r * r <= 512 that decides between the two renders) and a goal in
cell 255 of a 16 x 16 map, whose index reads like goal_cells' "no goal".  Everything is bit-exact against the CPU oracle through
the C ABI; symbolic observations against tests/_symbolic_ref.py.

The oracle's egocentric render is pinned to the reference at r = 3 only (tests/golden/tasks_ego.json, the doc image); at these
sizes it is the same code run further: every stage compared here is `unpinned_by_reference` beyond r = 3.  tests/
test_symbolic_ref.py states window and shadows a second time, in plain Python, at 16 cells and r = 13 / 15."""
import numpy as np
import pytest

import _symbolic_ref as S
from test_gpu_ego import _facing
from test_gpu_view import FrameCheck
from test_gpu_xworld import NAV, _torch
from test_oracle_tasks import KINDS

pytestmark = pytest.mark.gpu


def _nav(max_dim, goals, blocks):
    return ({"max_dim": max_dim, "num_goals": goals, "num_blocks": blocks},
            dict(map_kind=0, max_dim=max_dim, dim=max_dim, num_goals=goals, num_blocks=blocks))


# key: (options for the product, oracle cfg) -- XWorldNav maps, dim = max_dim
SIZES = {
    "nav12": _nav(12, 4, 30), "nav13": _nav(13, 4, 40), "nav15": _nav(15, 4, 50), "nav16": _nav(16, 4, 60),
    "nav16_g12": _nav(16, 12, 60),
    "nav7_g16": _nav(7, 16, 8), "nav8_g16": _nav(8, 16, 16), "nav7_g10": _nav(7, 10, 8), "nav7_g11": _nav(7, 11, 8),
}


def _make(oracle, key, n, r, tasks=KINDS, seed=0xC0FFEE, policy_seed=0x5EED, **opts):
    from xworld_amd.batched import BatchedSimulator
    popts, ocfg = SIZES[key]
    o = {"xwd_conf_path": NAV, "task_mode": "lang_acquisition", "tasks": list(tasks), "visible_radius": r}
    o.update(popts)
    o.update(opts)
    sim = BatchedSimulator("xworld", o, num_envs=n, seed=seed, policy_seed=policy_seed)
    assert (sim.cfg.max_dim, sim.cfg.num_goals, sim.cfg.visible_radius) == (ocfg["max_dim"], ocfg["num_goals"], r)
    pal = oracle.Palette(oracle.NAV_SUBTREES)
    cfg = dict(ocfg)
    cfg.update(seed=seed, tasks=list(tasks), visible_radius=r, color=int(bool(opts.get("color", False))),
               context=int(opts.get("context", 1)), max_steps=int(opts.get("max_steps", 0)))
    return sim, pal, cfg


def _load_world(sim, e, w, cfg):
    """an oracle world into env e through the host: map, heading, the goals' poses"""
    g = w.grid().astype(np.uint16)
    ax, ay = w.agent_xy()
    g[w.target_cells() != 0] |= 0x8000
    sim.load_map(e, g, ax, ay, dim=cfg["dim"], task=KINDS[0], target=w.target_name())
    sim.set_agent_dir(e, _facing(w.agent_yaw()))
    for i, ent in enumerate(w.entities()):
        if ent[0] == 0:
            sim.set_goal_pose(e, ent[1], ent[2], *w.get_pose(i))
    sim.refresh_obs(e)


def _highest_cell_shown(w):
    """the largest index y * max_dim + x of a map cell the world's view shows (inside the map, not behind a wall): the oracle alone"""
    r, d = w.cfg.visible_radius, w.cfg.max_dim
    x_st, y_st, shadow = w.agent_masking()
    best = -1
    for wy in range(r):
        for wx in range(r):
            gx, gy = x_st - r + wx, y_st - r + wy
            if 0 <= gx < d and 0 <= gy < d and not shadow[wy, wx]:
                best = max(best, gy * d + gx)
    return best


def _frames(sim):
    """the batch's frames as the oracle's state_screen() states them: uint8; a float32 batch holds frame * float32(1 / 255)"""
    obs = sim.obs.cpu().numpy()
    if not sim.obs_is_float:
        return obs
    u8 = np.rint(obs * 255.0).astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32) * np.float32(1 / 255.0), obs), "float32 frames are not uint8 * (1 / 255)"
    return u8


HOST_POSE_CASES = [
    # key, r, colour, context, float32, path
    ("nav12", 3, True, 1, False, "span"), ("nav13", 5, False, 2, False, "span"), ("nav15", 7, True, 1, False, "span"),
    ("nav16", 3, False, 2, False, "span"), ("nav12", 11, True, 2, False, "per_env"), ("nav13", 13, False, 1, False, "per_env"),
    ("nav16", 13, True, 2, False, "per_env"), ("nav15", 15, True, 1, True, "per_env"), ("nav16", 15, False, 1, False, "per_env"),
]


@pytest.mark.parametrize("key,r,color,context,f32,path", HOST_POSE_CASES, ids=["%s_r%d" % c[:2] for c in HOST_POSE_CASES])
def test_large_maps_frames_with_host_poses(oracle, key, r, color, context, f32, path):
    """(a) Maps of 12, 13, 15 and 16 cells from the oracle's generator, loaded with the goal poses set through the host; every
    frame of every env against state_screen() after each of a few random first-person actions.  The case must take the render it
    is meant for, and on the maps that have them (15 and 16 cells) some compared frame must show a cell with index >= 192 --
    said by the oracle's window and shadows alone.  unpinned_by_reference beyond r = 3."""
    torch = _torch()
    n, steps = (8, 6) if r >= 9 else (12, 8)                   # 56 / 108 oracle frames
    extra = dict(obs_format="float32") if f32 else {}
    sim, pal, cfg = _make(oracle, key, n, r, tasks=[KINDS[0]], seed=5, color=color, context=context, **extra)
    assert sim.ego_render_path == path
    envs = []
    for e in range(n):
        w = oracle.XWorld(pal, render=True, **cfg)
        w.reset_game(e, 0)
        envs.append(w)
        _load_world(sim, e, w, cfg)
    rng = np.random.default_rng(1)
    highest = -1
    for t in range(steps + 1):
        obs = _frames(sim)
        for e, w in enumerate(envs):
            exp = w.state_screen()
            assert np.array_equal(obs[e], exp), (t, e, int((obs[e] != exp).sum()))
            highest = max(highest, _highest_cell_shown(w))
        acts = rng.integers(0, 6, n).astype(np.int32)
        sim.step(torch.from_numpy(acts).cuda())
        for e, w in enumerate(envs):
            w.take_actions(int(acts[e]))
    assert sim.check_errors() == 0
    sim.close()
    if cfg["max_dim"] ** 2 > 192:
        assert highest >= 192, highest


@pytest.mark.parametrize("r,context,path", [(5, 2, "span"), (13, 1, "per_env")])
def test_sixteen_cell_maps_through_the_verbs(oracle, r, context, path):
    """(b) 16 x 16 maps with poses drawn by the reset kernel, a ragged batch (77 envs) and episodes of 3 steps: step + reset_done,
    then step_autoreset.  Reward bits and game-over codes of every env against oracle.xw_rollout, the frames of a handful of envs
    -- the terminal frame, the first frame of the next episode, the shifted ring -- against per-env oracle worlds.
    unpinned_by_reference beyond r = 3."""
    _torch()
    n, plain, auto = 77, 5, 3
    sim, pal, cfg = _make(oracle, "nav16", n, r, seed=19, policy_seed=4, color=True, context=context, max_steps=3)
    assert sim.ego_render_path == path
    ref = oracle.xw_rollout(n, oracle.xw_cfg(**cfg), pal, plain + auto, policy_seed=4)
    watch = [0, 63, 64, n - 1]
    worlds = {e: oracle.XWorld(pal, render=True, **cfg) for e in watch}
    ep = dict.fromkeys(watch, 0)
    for e, w in worlds.items():
        w.reset_game(e, 0)

    def frames(where):
        obs = sim.obs.cpu().numpy()
        for e, w in worlds.items():
            exp = w.state_screen()
            assert np.array_equal(obs[e], exp), (where, e, int((obs[e] != exp).sum()))

    def restart(codes):
        for e, w in worlds.items():
            if codes[e]:
                ep[e] += 1
                w.reset_game(e, ep[e])

    frames("reset")
    resets = 0
    for t in range(plain + auto):
        if t < plain:
            sim.step()
        else:
            sim.step_autoreset()
        assert np.array_equal(sim.reward.cpu().numpy().view(np.uint32), ref.rewards[t].view(np.uint32)), t
        codes = sim.game_over_codes.cpu().numpy()
        assert np.array_equal(codes, ref.codes[t]), t
        acts = sim.actions.cpu().numpy()
        for e, w in worlds.items():
            w.take_actions(int(acts[e]))
        if t + 1 < plain + auto:                                                   # (the rollout restarts an env before its next step)
            resets += int((codes != 0).sum())
        if t < plain:
            frames(("step", t))                                                    # terminal frames included
            sim.reset_done()
        restart(codes)
        frames(("reset_done" if t < plain else "step_autoreset", t))
    assert resets == ref.stats.resets and resets >= n
    assert min(ep.values()) > 0
    assert sim.check_errors() == 0
    sim.close()


MANY_GOALS = [("nav7_g16", 3, "span"), ("nav8_g16", 5, "span"), ("nav7_g10", 7, "span"), ("nav7_g11", 7, "per_env")]
MANY_IDS = ["16_goals_r3", "16_goals_r5", "10_goals_r7", "11_goals_r7"]


def _goals_touch(w):
    """two goals of the world in edge-adjacent cells"""
    cells = {(x, y) for t, x, y, *_ in w.entities() if t == 0}
    return any((x + 1, y) in cells or (x, y + 1) in cells for x, y in cells)


@pytest.mark.parametrize("key,r,path", MANY_GOALS, ids=MANY_IDS)
def test_many_goals_frames_against_oracle(oracle, key, r, path):
    """(c) 10, 11 and 16 goals: border lines that blend two goals' images, crossing pixels among goals, goal slots 4-15, miss
    lists of n * min(num_goals, r * r) entries.  The goal-cell cache -- and with it the span path -- exists while
    num_goals * r * r <= 512: at r = 7, 10 goals draw on the span path and 11 on the one-workgroup-per-env kernel.  Poses from the
    reset kernel, episodes of 6 steps; at least half of the envs start with two goals in edge-adjacent cells (the oracle's
    entities say so).  unpinned_by_reference beyond r = 3."""
    _torch()
    n, steps, shown = 64, 8, 16
    sim, pal, cfg = _make(oracle, key, n, r, seed=13, policy_seed=7, color=True, max_steps=6)
    assert sim.ego_render_path == path
    assert (cfg["num_goals"] * r * r <= 512) == (path == "span")
    probe = oracle.XWorld(pal, render=False, **cfg)
    touching = 0
    for e in range(n):
        probe.reset_game(e, 0)
        touching += _goals_touch(probe)
    assert touching >= n // 2, touching
    worlds = [oracle.XWorld(pal, render=True, **cfg) for _ in range(shown)]
    ep = [0] * shown
    for e, w in enumerate(worlds):
        w.reset_game(e, 0)
    assert sum(_goals_touch(w) for w in worlds) >= shown // 2

    def frames(where):
        obs = sim.obs.cpu().numpy()
        for e, w in enumerate(worlds):
            exp = w.state_screen()
            assert np.array_equal(obs[e], exp), (where, e, int((obs[e] != exp).sum()))

    frames("reset")
    resets = 0
    for t in range(steps):
        auto = t % 3 == 2
        if auto:
            sim.step_autoreset()
        else:
            sim.step()
        acts = sim.actions.cpu().numpy()
        codes = sim.game_over_codes.cpu().numpy()
        for e, w in enumerate(worlds):
            w.take_actions(int(acts[e]))
            assert w.game_over() == codes[e], (t, e)
        if not auto:
            frames(("step", t))
            sim.reset_done()
        for e, w in enumerate(worlds):
            if codes[e]:
                ep[e] += 1
                resets += 1
                w.reset_game(e, ep[e])
        frames(("after resets", t))
    assert resets >= shown and sim.check_errors() == 0
    sim.close()


@pytest.mark.parametrize("key,r,path", MANY_GOALS, ids=MANY_IDS)
def test_many_goals_span_path_equals_per_env_path(oracle, key, r, path):
    """(c) the verbs of test_ego_span_path_equals_per_env_path with 10, 11 and 16 goals: the configuration's own render against
    the one-workgroup-per-env kernel on a ragged batch, through step + reset_done, step_autoreset and a masked reset.  With 11
    goals at r = 7 both batches take the per-env kernel -- the configuration falls off the span path -- and must still agree."""
    torch = _torch()
    n = 203
    a, _, _ = _make(oracle, key, n, r, seed=11, policy_seed=3, color=True, context=2, max_steps=9)
    b, _, _ = _make(oracle, key, n, r, seed=11, policy_seed=3, color=True, context=2, max_steps=9, debug=["ego_no_span"])
    assert a.ego_render_path == path and b.ego_render_path == "per_env"
    for sim in (a, b):
        sim.reset()
    assert torch.equal(a.obs, b.obs)
    mask = (torch.arange(n, device="cuda") % 7 == 3)
    resets = 0
    for t in range(30):
        for sim in (a, b):
            if t % 3 == 2:
                sim.step_autoreset()
            else:
                sim.step()
        assert torch.equal(a.obs, b.obs), ("terminal / stepped frames", t)
        resets += int((a.game_over_codes != 0).sum())
        for sim in (a, b):
            if t % 3 != 2:
                sim.reset_done()
            if t == 20:
                sim.reset_masked(mask)
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.game_over_codes, b.game_over_codes), t
    assert resets > n
    a.close()
    b.close()


@pytest.mark.parametrize("key,r", [("nav13", 13), ("nav16_g12", 15)])
def test_views_and_symbolic_at_the_largest_radii(oracle, key, r):
    """(d) render_view against the oracle's agent_view(), symbolic against tests/_symbolic_ref.py, and the view pushed through the
    two resizes against the frame (tests/test_gpu_view.py's FrameCheck): 169 and 225 view cells, 12 goals on the 16-cell map.
    unpinned_by_reference beyond r = 3."""
    torch = _torch()
    n, steps = 8, 4
    sim, pal, cfg = _make(oracle, key, n, r, tasks=[KINDS[0]], seed=5, color=True)
    assert sim.ego_render_path == "per_env" and sim.view_dims == (64 * r, 64 * r, 3) and sim.symbolic_dims == (3, r, r)
    envs = []
    for e in range(n):
        w = oracle.XWorld(pal, render=True, **cfg)
        w.reset_game(e, 0)
        envs.append(w)
        _load_world(sim, e, w, cfg)
    fc = FrameCheck(oracle, sim, True)
    rng = np.random.default_rng(3)
    goals_seen = 0
    for t in range(steps + 1):
        views = sim.render_view()
        host = views.cpu().numpy()
        sym = sim.symbolic().cpu().numpy()
        for e, w in enumerate(envs):
            exp = w.agent_view()
            assert np.array_equal(host[e], exp), (t, e, int((host[e] != exp).sum()))
            want = S.expected(w, pal)
            assert np.array_equal(sym[e], want), (t, e, S.show(sym[e][S.KIND]), S.show(want[S.KIND]))
            goals_seen += int((want[S.KIND] == S.GOAL).sum())
        fc.check(views, t)
        acts = rng.integers(0, 6, n).astype(np.int32)
        sim.step(torch.from_numpy(acts).cuda())
        for e, w in enumerate(envs):
            w.take_actions(int(acts[e]))
    assert goals_seen > 0 and sim.check_errors() == 0
    sim.close()


CORNER = (15, 15)                                           # cell 15 * 16 + 15 = 255 = 0xff, goal_cells' "no goal"
AGENT = (15, 14)                                            # the cell above it: heading down, the corner is straight ahead
CORNER_CASES = ["goal", "block", "empty", "goal", "goal"]   # per env; the LAST env of the batch holds a goal there


def corner_world(oracle, pal, cfg, e, what):
    """The oracle's map of env e, edited: the agent on AGENT heading down, and on CORNER a goal, a block or nothing.  Loaded back
    into a fresh oracle world (load_map with the staged poses); returns (world, icon of the goal on CORNER or -1)."""
    src = oracle.XWorld(pal, render=False, **cfg)
    src.reset_game(e, 0)
    ents = [list(x) for x in src.entities()]
    poses = [list(src.get_pose(i)) for i in range(len(ents))]

    def at(cell):
        return next((i for i, x in enumerate(ents) if (x[1], x[2]) == cell), None)

    def drop(i):
        del ents[i]
        del poses[i]

    agent = next(i for i, x in enumerate(ents) if x[0] == 2)
    old = (ents[agent][1], ents[agent][2])
    i = at(AGENT)
    if i is not None and i != agent:
        if ents[i][0] == 0:
            ents[i][1], ents[i][2] = old                    # a goal makes room: it moves to the agent's cell
        else:
            drop(i)
            agent = next(k for k, x in enumerate(ents) if x[0] == 2)
    ents[agent][1], ents[agent][2] = AGENT
    poses[agent] = [np.pi / 2, poses[agent][1], poses[agent][2]]
    i = at(CORNER)
    icon = -1
    if what == "goal":
        if i is not None and ents[i][0] != 0:
            drop(i)
            i = None
        if i is None:
            i = next(k for k, x in enumerate(ents) if x[0] == 0)
            ents[i][1], ents[i][2] = CORNER
        icon = ents[i][3]
    elif what == "block":
        if i is None or ents[i][0] != 1:
            if i is not None:
                drop(i)
            i = next(k for k, x in enumerate(ents) if x[0] == 1)
            ents[i][1], ents[i][2] = CORNER
    elif i is not None:
        drop(i)
    assert len({(x[1], x[2]) for x in ents}) == len(ents)
    w = oracle.XWorld(pal, render=True, **cfg)
    w.stage_poses(poses)
    w.load_map([tuple(x) for x in ents], cfg["dim"], target_pick=0, env_gid=e, episode=0)
    assert w.agent_xy() == AGENT and _facing(w.agent_yaw()) == 1
    d = cfg["max_dim"]
    kind = {"goal": 0, "block": 1}.get(what)
    code = int(w.grid()[CORNER[1], CORNER[0]])
    assert (code == 0) if kind is None else (pal.type_arr[code - 1] == kind), (what, code)
    assert CORNER[1] * d + CORNER[0] == 0xff
    return w, icon


@pytest.mark.parametrize("r,path", [(3, "span"), (9, "per_env")])
def test_goal_in_cell_255(oracle, r, path):
    """(e) A 16 x 16 map's last cell has index 255, the byte goal_cells uses for "no goal".  A goal there is a goal like any other:
    its image is warped with its pose, frames, render_view and symbolic show it in its own slot (not slot 15, whose image belongs
    to the next env or lies past the buffer for the last one), set_goal_pose finds it, a move into it along the heading is a
    reached goal, and a checkpoint restores it (xwb_load_state warps the goal images again).  Beside it: a block in that cell and
    nothing in it, where set_goal_pose must refuse.  unpinned_by_reference beyond r = 3."""
    torch = _torch()
    from xworld_amd.lib import XwbError
    n = len(CORNER_CASES)
    sim, pal, cfg = _make(oracle, "nav16", n, r, tasks=[KINDS[0]], seed=37, color=True)
    twin, _, _ = _make(oracle, "nav16", n, r, tasks=[KINDS[0]], seed=37, color=True)
    assert sim.ego_render_path == path
    envs, icons = [], []
    for e, what in enumerate(CORNER_CASES):
        w, icon = corner_world(oracle, pal, cfg, e, what)
        envs.append(w)
        icons.append(icon)
        _load_world(sim, e, w, cfg)
        if what != "goal":
            with pytest.raises(XwbError):
                sim.set_goal_pose(e, CORNER[0], CORNER[1], 0.3, 0.9, 0.05)
    fc = FrameCheck(oracle, sim, True)
    corner_shown = [0] * n

    def look(where, s=sim):
        obs = s.obs.cpu().numpy()
        views = s.render_view()
        host = views.cpu().numpy()
        sym = s.symbolic().cpu().numpy()
        for e, w in enumerate(envs):
            exp = w.state_screen()
            assert np.array_equal(obs[e], exp), (where, "frame", e, CORNER_CASES[e], int((obs[e] != exp).sum()))
            exp = w.agent_view()
            assert np.array_equal(host[e], exp), (where, "view", e, CORNER_CASES[e], int((host[e] != exp).sum()))
            want = S.expected(w, pal)
            assert np.array_equal(sym[e], want), (where, "symbolic", e, S.show(sym[e][S.KIND]), S.show(want[S.KIND]))
            if s is sim and icons[e] >= 0:
                corner_shown[e] += int(((want[S.KIND] == S.GOAL) & (want[S.ICON] == icons[e])).any())
        return views

    fc.check(look("loaded"), "loaded")
    blob = sim.save_state(include_obs=False)
    twin.load_state(blob)                                                          # frames drawn again from the restored state
    look("restored", twin)
    twin.close()
    for t, a in enumerate([4, 4, 4, 4, 5, 4]):                                     # a full turn, then right and back: heading down again
        acts = np.full(n, a, np.int32)
        sim.step(torch.from_numpy(acts).cuda())
        for w in envs:
            w.take_actions(a)
        fc.check(look(("turn", t)), ("turn", t))
    for e in range(n):
        if icons[e] >= 0:                                                          # the goal's icon is unique on the map (XWorldNav: distinct names)
            assert corner_shown[e] == 6, (e, corner_shown[e])               # of 7 looks: the window never holds it while the agent looks up
    sim.step(torch.zeros(n, dtype=torch.int32, device="cuda"))                     # MOVE_FORWARD: into the corner cell
    rew = sim.reward.cpu().numpy()
    codes = sim.game_over_codes.cpu().numpy()
    events = set()
    for e, w in enumerate(envs):
        assert np.float32(w.take_actions(0)) == rew[e] and w.game_over() == codes[e], (e, CORNER_CASES[e])
        st = sim.env_state(e)
        assert st.xw_event == w.event() and st.xw_stage == w.stage(), (e, CORNER_CASES[e])
        assert (st.xw_agent_x, st.xw_agent_y) == w.agent_xy() and st.last_action_success == w.last_action_success()
        assert (w.event() != 0) == (CORNER_CASES[e] == "goal"), (e, w.event())
        assert (w.agent_xy() == CORNER) == (CORNER_CASES[e] == "empty")
        events.add(w.event())
    assert events - {0}, events
    fc.check(look("bumped"), "bumped")
    assert sim.check_errors() == 0
    sim.close()


@pytest.mark.parametrize("r,path", [(3, "span"), (9, "per_env")])
def test_reset_puts_a_goal_in_cell_255(oracle, r, path):
    """(e) The reset kernel itself puts a goal into cell 255: the idle stage of Near / Between / Direction moves two goals onto a
    tile that may end in the last cell, and a moved goal keeps its slot.  With seed 199 the LAST env of a batch of 7 starts under
    XWorld3DNavTargetNear with the goal created third of four on (15, 15) and the agent on (15, 14) -- the oracle's entities say
    so below --, so goal_cells reads [a, b, 0xff, c, 0xff, ...]: a real 0xff with a goal behind it, then the empty ones.  A rule
    that takes "the 0xff after a real slot" for the goal also takes slot 4 and draws an image past the batch's goal images.
    Frames, render_view and symbolic of every env against the oracle at five headings, then the move into the goal: reward,
    event and the terminal frame.  unpinned_by_reference beyond r = 3."""
    torch = _torch()
    n, last = 7, 6
    sim, pal, cfg = _make(oracle, "nav16", n, r, seed=199, color=True)
    assert sim.ego_render_path == path
    envs = [oracle.XWorld(pal, render=True, **cfg) for _ in range(n)]
    for e, w in enumerate(envs):
        w.reset_game(e, 0)
    w = envs[last]
    goals = sorted((x for x in w.entities() if x[0] == 0), key=lambda x: x[5])     # creation order = the device's slots
    slot = [(x[1], x[2]) for x in goals].index(CORNER)
    assert len(goals) == 4 and slot == 2 and w.task_kind() == 1 and w.agent_xy() == AGENT, (goals, w.task_kind(), w.agent_xy())
    icon = goals[slot][3]
    assert [x[3] for x in goals].count(icon) == 1
    fc = FrameCheck(oracle, sim, True)
    corner_shown = 0

    def look(where):
        nonlocal corner_shown
        obs = sim.obs.cpu().numpy()
        views = sim.render_view()
        host = views.cpu().numpy()
        sym = sim.symbolic().cpu().numpy()
        for e, w in enumerate(envs):
            exp = w.state_screen()
            assert np.array_equal(obs[e], exp), (where, "frame", e, int((obs[e] != exp).sum()))
            exp = w.agent_view()
            assert np.array_equal(host[e], exp), (where, "view", e, int((host[e] != exp).sum()))
            want = S.expected(w, pal)
            assert np.array_equal(sym[e], want), (where, "symbolic", e, S.show(sym[e][S.KIND]), S.show(want[S.KIND]))
            if e == last:
                corner_shown += int(((want[S.KIND] == S.GOAL) & (want[S.ICON] == icon)).any())
        fc.check(views, where)

    look("reset")
    for t, a in enumerate([4, 4, 4, 5]):                                           # headings left, down, right, down again
        sim.step(torch.from_numpy(np.full(n, a, np.int32)).cuda())
        for w in envs:
            w.take_actions(a)
        look(("turn", t))
    assert _facing(envs[last].agent_yaw()) == 1 and corner_shown == 4, corner_shown    # (not while the agent looks up, at reset)
    sim.step(torch.zeros(n, dtype=torch.int32, device="cuda"))                     # MOVE_FORWARD: the last env bumps into the goal
    rew = sim.reward.cpu().numpy()
    codes = sim.game_over_codes.cpu().numpy()
    for e, w in enumerate(envs):
        assert np.float32(w.take_actions(0)) == rew[e] and w.game_over() == codes[e], e
        st = sim.env_state(e)
        assert st.xw_event == w.event() and st.xw_stage == w.stage(), e
        assert (st.xw_agent_x, st.xw_agent_y) == w.agent_xy()
    assert envs[last].event() != 0 and envs[last].agent_xy() == AGENT
    look("bumped")
    assert sim.check_errors() == 0
    sim.close()
