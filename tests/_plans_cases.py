"""What the plan-evaluation tests share (tests/test_plans_host.py on the CPU, tests/test_gpu_plans.py on the GPU): the cases,
their seeded prefixes and plan sets, the float32 return recurrence of include/xwb.h, and the oracle's answer for every plan --
computed once per case and process, then only read.

A case = (options of the batch, the oracle's cfg) as in tests/_expert_cases.py, plus how it is driven: PREFIX seeded explicit
actions played with step + reset_done, then K plans of H steps per env.  The oracle's side needs nothing from the GPU: the prefix
is played on one oracle object per env, which yields each env's episode counter and the actions since its last reset; every
(env, plan) is then answered by an object reset to that episode, replayed through those actions and driven through the plan
until its game-over code is set.
"""
import functools

import numpy as np

import _expert_cases as ec

N, K, H = 48, 6, 10
ALIVE, MAX_STEP, DEAD, SUCCESS = 0, 1, 2, 4
SKIP = -1
GAMMAS = (1.0, 0.5)


def _case(conf, popts, ocfg, prefix=6, act_rep=1, seed=1, limit=False, wins=True, **both):
    o, c, _ = ec._case(conf, popts, ocfg, ec.T3, **both)
    return dict(opts=o, cfg=c, prefix=prefix, act_rep=act_rep, seed=seed, limit=limit, wins=wins)


_D5 = ({"dim": 5, "num_goals": 2, "num_blocks": 6}, dict(map_kind=0, max_dim=8, dim=5, num_goals=2, num_blocks=6))
_M5 = ({"max_dim": 5, "num_goals": 2, "num_blocks": 3}, dict(map_kind=0, max_dim=5, dim=5, num_goals=2, num_blocks=3))
_N7 = ({"max_dim": 7, "num_blocks": 16}, dict(map_kind=0, max_dim=7, dim=7, num_goals=4, num_blocks=16))
_N8 = ({}, dict(map_kind=0, max_dim=8, dim=8, num_goals=4, num_blocks=16))
_N16 = ({"max_dim": 16, "num_goals": 12, "num_blocks": 40}, dict(map_kind=0, max_dim=16, dim=16, num_goals=12, num_blocks=40))

# seed: chosen on the CPU (tests/test_plans_host.py asserts the coverage condition for it); limit: a case whose plans must cross
# the task's time limit or max_steps; wins: the game-over code can carry XWB_SUCCESS / XWB_DEAD (lang_acquisition)
CASES = {
    "dim5_five_tasks": _case(ec.NAV2D, *_D5),
    "ego3": _case(ec.NAV2D, *_N7, visible_radius=3),
    "curriculum": _case(ec.NAV2D, *_N8, curriculum=0.1, start_level=3),
    "factor1": _case(ec.NAV2D, *_M5, prefix=20, limit=True, max_steps_factor=1),
    "max_steps12": _case(ec.NAV2D, *_N7, prefix=5, limit=True, max_steps=12),
    "act_rep2": _case(ec.NAV2D, *_N7, act_rep=2),
    # egocentric repeats: a turn is applied on every repeat and the contact of an earlier repeat is kept; the prefix is played by
    # the step kernels with act_rep 2, so every later number depends on the headings they stored
    "ego3_act_rep2": _case(ec.NAV2D, *_N7, act_rep=2, visible_radius=3),
    # outside lang_acquisition the code ignores the task's events: an episode ends on max_steps alone (every env on the same step,
    # so one case cannot hold both plans that cross it and plans that do not: max_steps12 is the case that crosses), and a plan
    # that wins is paid + 1 and goes on.  One group, so exclusive scheduling has nothing to choose
    "one_channel": _case(ec.NAV2D, dict(_N7[0], task_mode="one_channel", task_groups_exclusive=False), dict(_N7[1], task_mode=1),
                         prefix=5, wins=False, max_steps=40),
    "nav16": _case(ec.NAV, *_N16),
}


def num_actions(name):
    return 6 if CASES[name]["opts"].get("visible_radius") else 4


def make_sim(name, n=N, **extra):
    from xworld_amd.batched import BatchedSimulator
    return BatchedSimulator("xworld", dict(CASES[name]["opts"], **extra), num_envs=n, seed=ec.SEED, policy_seed=5, env_gid0=ec.GID0)


@functools.lru_cache(maxsize=None)
def _palette():
    import _oracle
    return _oracle.Palette(_oracle.NAV_SUBTREES)


def make_oracle(oracle, name):
    return oracle.XWorld(_palette(), render=False, **CASES[name]["cfg"])


def prefix_actions(name):
    """[PREFIX][N] seeded uniform action ids"""
    rng = np.random.RandomState(1000 + CASES[name]["seed"])
    return rng.randint(0, num_actions(name), size=(CASES[name]["prefix"], N)).astype(np.int32)


def plans(name):
    """int8 [N][K][H]: every other action is "along the heading" (MOVE_DOWN under full observation, MOVE_FORWARD in egocentric
    mode: the only way to reach a goal, xwb.h "the shortest-path expert"), the rest uniform -- uniform plans seldom bump a goal."""
    rng = np.random.RandomState(2000 + CASES[name]["seed"])
    na = num_actions(name)
    p = rng.randint(0, na, size=(N, K, H))
    ahead = 0 if na == 6 else 1
    return np.where(rng.rand(N, K, H) < 0.5, ahead, p).astype(np.int8)


def returns_f32(rewards, gamma):
    """include/xwb.h, xwb_xw_evaluate_plans: ret = ret + g * r_t; g = g * gamma -- float32, every product and sum rounded on its
    own, in step order."""
    ret, g, gamma = np.float32(0.0), np.float32(1.0), np.float32(gamma)
    for r in rewards:
        ret = np.float32(ret + np.float32(g * np.float32(r)))
        g = np.float32(g * gamma)
    return ret


def heading_of(world, name):
    """the heading part of `last`: the expert field's plane -- 0 under full observation, the facing direction in egocentric mode"""
    if not CASES[name]["opts"].get("visible_radius"):
        return 0
    return int(round(world.agent_yaw() / (np.pi / 2))) & 3


class Record:
    """per env: the episode it is in and the actions it has taken since that episode began"""

    def __init__(self):
        self.episode = np.zeros(N, int)
        self.since = [[] for _ in range(N)]

    def add(self, actions, codes):
        for e in range(N):
            self.since[e].append(int(actions[e]))
            if codes[e]:
                self.episode[e] += 1
                self.since[e] = []


def drive(world, gid, episode, since, plan, act_rep, max_dim, name):
    """(rewards of the executed steps, code, last) of one plan on an oracle object put into the env's state"""
    world.reset_game(gid, int(episode))
    for a in since:
        world.take_actions(a, act_rep)
        assert world.game_over() == 0
    rewards, code = [], 0
    for a in plan:
        if a < 0:
            break
        rewards.append(np.float32(world.take_actions(int(a), act_rep)))
        code = world.game_over()
        if code:
            break
    x, y = world.agent_xy()
    return rewards, code, (heading_of(world, name) << 16) | (y * max_dim + x)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's answer for the case: (record after the prefix, steps [N][K], codes [N][K], last [N][K], rewards [N][K] lists).
    Treat as read-only."""
    import _oracle as oracle
    c = CASES[name]
    rep, md = c["act_rep"], c["cfg"]["max_dim"]
    worlds = [make_oracle(oracle, name) for _ in range(N)]
    rec = Record()
    for e, w in enumerate(worlds):
        w.reset_game(ec.GID0 + e, 0)
    for acts in prefix_actions(name):
        codes = np.zeros(N, int)
        for e, w in enumerate(worlds):
            w.take_actions(int(acts[e]), rep)
            codes[e] = w.game_over()
        rec.add(acts, codes)
        for e, w in enumerate(worlds):
            if codes[e]:
                w.reset_game(ec.GID0 + e, int(rec.episode[e]))
    p = plans(name)
    steps, codes, last = (np.zeros((N, K), int) for _ in range(3))
    rewards = [[None] * K for _ in range(N)]
    for e in range(N):
        w = make_oracle(oracle, name)               # (a curriculum object counts its resets: a fresh one per env keeps its level)
        for k in range(K):
            rewards[e][k], codes[e, k], last[e, k] = drive(w, ec.GID0 + e, rec.episode[e], rec.since[e], p[e, k], rep, md, name)
            steps[e, k] = len(rewards[e][k])
    return rec, steps, codes, last, rewards


def coverage(name):
    """what the case's plans end on: the set the coverage condition is asserted over"""
    _, steps, codes, _, rewards = expected(name)
    out = set()
    for e in range(N):
        for k in range(K):
            c = int(codes[e, k])
            if c == 0 and steps[e, k] == H:
                out.add("alive")
            if c & SUCCESS:
                out.add("success")
            if c & DEAD:
                out.add("dead")
            if c & MAX_STEP:
                out.add("limit")
            if any(r > 0.5 for r in rewards[e][k]):
                out.add("paid")
            if any(r < -0.5 for r in rewards[e][k]):
                out.add("fined")
    return out


def required(name):
    """The coverage condition of a case.  lang_acquisition: a plan ending on XWB_SUCCESS, one on the wrong goal's XWB_DEAD, one
    still alive after H steps, and in the two limit cases one on the time-up / max_steps code.  Outside lang_acquisition the code
    cannot carry the first two: there a plan must have been paid for the right goal and one fined for a wrong one instead."""
    c = CASES[name]
    need = {"alive"} | ({"success", "dead"} if c["wins"] else {"paid", "fined"})
    if c["limit"]:
        need.add("limit")
    return need
