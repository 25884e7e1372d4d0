"""Cases shared by the reference-build tests (tests/test_ref_simple.py), the fixture generator
(tests/golden/make_ref_simple_golden.py) and the GPU fixture tests: flag sets, action scripts, the oracle's run of a case in
the shape tests/_ref.py records the reference's, and the coverage conditions read off a REFERENCE run."""
import base64

import numpy as np

import _ref as R

PI = 3.1415926                     # the reference's own constant (simple_race_simulator.h:39)


# ------------------------------------------------------------------ actions
def policy_actions(oracle, policy_seed, gid, T, n_actions):
    """The oracle's (and the kernels' built-in) policy: action of env `gid` at rollout step t."""
    return [oracle.policy_action(policy_seed, gid, t, n_actions) for t in range(T)]


def n_actions_of(game, flags):
    return 2 if game == R.GAME or not flags.get("race_full_manouver") else 9


# scripted walks, as action INDICES.  Two-action set: index 0 = forward + left turn (4), 1 = forward + right turn (7).
# Full set: index = manoeuvre id, id % 3 = none / forward / backward, id / 3 = none / +PI/10 / -PI/10.
def walk(T, pattern):
    return [pattern[t % len(pattern)] for t in range(T)]


WALKS2 = [[0, 1], [0], [1], [0, 0, 1], [1, 1, 0], [0, 1, 1, 0]]
WALKS9 = [[1], [2], [1, 1, 1, 4, 1, 1, 7], [3, 3, 3, 3, 3, 1], [6, 6, 6, 6, 6, 1], [4], [7], [5], [8], [0, 3, 6, 2],
          [3], [6], [1, 4, 1, 7], [2, 5, 2, 8]]


# ------------------------------------------------------------------ the oracle's run of one case
def oracle_rollout(oracle, game, flags, actions, nth_thread=0):
    """The same loop as ref_api.cpp's xwref_rollout, through oracle/simple_{race,game}.c; returns an _ref.Record."""
    T = len(actions)
    r = R.Record()
    r.actions = np.asarray(actions, np.int32)
    r.rewards = np.zeros(T, np.float32)
    r.codes = np.zeros(T, np.uint8)
    r.num_steps = np.zeros(T, np.int32)
    r.resets = np.zeros(T + 1, np.uint8)
    r.nth_thread = nth_thread
    if game == R.RACE:
        f = dict(R.RACE_DEFAULTS, **flags)
        g = oracle.SimpleRace(track_type=1 if f["track_type"] == "circle" else 0, track_width=f["track_width"],
                              track_length=f["track_length"], track_radius=f["track_radius"],
                              race_full_manouver=int(f["race_full_manouver"]), random=int(f["random"]),
                              difficulty_hard=0 if f["difficulty"] == "easy" else 1, reward_scale=f["reward_scale"],
                              max_steps=f["max_steps"], context=f["context"], simulator_seed=f["simulator_seed"],
                              nth_thread=max(nth_thread, 1))
        r.obs = np.zeros((T + 1, 4 * f["context"]), np.float32)
        r.cars = np.zeros((T + 1, 3), np.float32)
        r.cars_after = np.zeros((T, 3), np.float32)
        r.ctor_car = g.car()
        r.n_actions = g.num_actions()
    else:
        f = dict(dict(context=1, max_steps=0), **flags)
        g = oracle.SimpleGame(f["array_size"], f["max_steps"], f["context"])
        r.obs = np.zeros((T + 1, f["array_size"] * f["context"]), np.uint8)
        r.cars = r.cars_after = r.ctor_car = None
        r.n_actions = 2
    r.obs_after = np.zeros((T,) + r.obs.shape[1:], r.obs.dtype)
    g.reset_game()
    for t in range(T + 1):
        if g.game_over() != 0:
            g.reset_game()
            r.resets[t] = 1
        r.obs[t] = g.state_screen()
        if r.cars is not None:
            r.cars[t] = g.car()
        if t == T:
            break
        r.rewards[t] = np.float32(g.take_actions(int(actions[t])))
        r.codes[t] = g.game_over()
        r.num_steps[t] = g.num_steps()
        r.obs_after[t] = g.state_screen()
        if r.cars is not None:
            r.cars_after[t] = g.car()
    return r


def assert_same(a, b, what=""):
    """Bit patterns of everything two records hold."""
    assert a.n_actions == b.n_actions, what
    for name in ("rewards", "obs", "obs_after", "cars", "cars_after", "ctor_car"):
        x, y = getattr(a, name), getattr(b, name)
        if x is None:
            assert y is None
            continue
        x = x.view(np.uint32) if x.dtype == np.float32 else x
        y = y.view(np.uint32) if y.dtype == np.float32 else y
        bad = np.argwhere(x != y)
        assert bad.size == 0, "%s: %s differs first at %s: %s vs %s" % (what, name, bad[0], x[tuple(bad[0])], y[tuple(bad[0])])
    for name in ("codes", "num_steps", "resets"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)


# ------------------------------------------------------------------ coverage, read off a reference run
MANOEUVRE = {False: [4, 7], True: list(range(9))}
BRANCHES = (["finish_reward", "left_boundary", "right_boundary", "backwards_over_start", "circle_inwards", "circle_outwards",
             "hard_boundary_penalty", "hard_finish_no_penalty", "wrap_above_2pi", "wrap_below_0", "screen_sign_flip",
             "screen_no_sign_flip", "cos_theta_clamp"] + ["manoeuvre_%d" % m for m in range(9)])


def coverage(flags, rec, seen):
    """Counts in `seen` the branches this REFERENCE run of a SimpleRace case visited.  Judged only from what the reference
    returned -- its car after every step, its rewards, codes and screens -- against the track as its constructor lays it
    out (float members; cv::norm in double, narrowed where the source narrows).  The reference's own DEAD code must agree with
    the geometry here at every step, which checks this bookkeeping itself."""
    f = dict(R.RACE_DEFAULTS, **flags)
    f32 = np.float32
    full = bool(f["race_full_manouver"])
    straight = f["track_type"] == "straight"
    hard = f["difficulty"] == "hard"
    w = f32(f["track_width"])
    cx, cy = f32(240), f32(360)
    if straight:
        length = f32(f["track_length"])
        start_y = f32(cy - f32(0.4 * float(length)))
        end_y = f32(cy + f32(0.6 * float(length)))
        left, right = f32(cx - w / f32(2)), f32(cx + w / f32(2))
    else:
        r_in = f32(f["track_radius"])
        r_out = f32(r_in + w)

    def hit(name):
        seen[name] = seen.get(name, 0) + 1

    for t in range(len(rec.actions)):
        m = MANOEUVRE[full][rec.actions[t]]
        hit("manoeuvre_%d" % m)
        a0 = rec.cars[t][2]
        x, y, a1 = rec.cars_after[t]
        turn = (m // 3) % 3
        if turn == 1 and a1 < a0:
            hit("wrap_above_2pi")
        if turn == 2 and a1 > a0:
            hit("wrap_below_0")
        s = rec.obs_after[t][-4:]
        hit("screen_sign_flip" if np.signbit(s[1]) else "screen_no_sign_flip")
        finish = False
        if straight:
            out = []
            if x < left:
                out.append("left_boundary")
            if x > right:
                out.append("right_boundary")
            if y < start_y:
                out.append("backwards_over_start")
            if y > end_y:
                out.append("finish_reward")
                finish = True
            c = float(np.sin(float(a1)))
        else:
            dx, dy = f32(x - cx), f32(y - cy)
            nrm = np.sqrt(float(dx) * float(dx) + float(dy) * float(dy))
            r = f32(nrm)
            out = ["circle_inwards"] if r < r_in else ["circle_outwards"] if r > r_out else []
            tx, ty = f32(float(f32(cy - y)) * (1 / nrm)), f32(float(f32(x - cx)) * (1 / nrm))
            c = float(tx) * float(np.cos(float(a1))) + float(ty) * float(np.sin(float(a1)))
        if abs(c) > 1.0:
            hit("cos_theta_clamp")
        assert bool(rec.codes[t] & 2) == bool(out), (flags, t, out, rec.codes[t], rec.cars_after[t])
        for name in out:
            hit(name)
        if hard and out:
            hit("hard_finish_no_penalty" if finish else "hard_boundary_penalty")
            # the reference's reward shows the rule: the -2 term is there, or at the finish it is not
            speed_bound = 1.0 * abs(f["reward_scale"]) + 1e-6
            r_ref = float(rec.rewards[t])
            want = (2.0 if finish else -2.0) * f["reward_scale"]
            assert abs(r_ref - want) <= speed_bound, (flags, t, r_ref)
    return seen


# ------------------------------------------------------------------ fixtures (tests/golden/ref_simple_{race,game}.json)
def _hex(a):
    """The bytes of an array (little-endian floats) as base64 text."""
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode()


def _unhex(s, dtype, shape):
    return np.frombuffer(base64.b64decode(s), dtype=dtype).reshape(shape).copy()


def record_to_json(rec, policy=None, cars=False):
    """Text form of a record.  obs[t + 1] equals obs_after[t] unless the env was reset in between, so only obs[0] and the
    observations right after a reset are stored; with `cars` (the random-reset cases) also the start states at those points
    and the constructor's."""
    T = len(rec.actions)
    d = {"policy": policy, "nth_thread": int(rec.nth_thread), "n_actions": int(rec.n_actions),
         "actions": "".join(str(int(a)) for a in rec.actions), "rewards": _hex(rec.rewards),
         "codes": "".join(str(int(c)) for c in rec.codes), "resets": "".join(str(int(c)) for c in rec.resets),
         "obs_after": _hex(rec.obs_after), "obs_start": {}, "car_start": {}}
    for t in range(T + 1):
        if t == 0 or rec.resets[t]:
            d["obs_start"][str(t)] = _hex(rec.obs[t])
            if cars:
                d["car_start"][str(t)] = _hex(rec.cars[t])
        else:
            assert np.array_equal(rec.obs[t].view(np.uint8), rec.obs_after[t - 1].view(np.uint8))
    if cars:
        d["ctor_car"] = _hex(rec.ctor_car)
    return d


def record_from_json(d, game):
    r = R.Record()
    T = len(d["actions"])
    r.actions = np.array([int(c) for c in d["actions"]], np.int32)
    r.rewards = _unhex(d["rewards"], np.float32, (T,))
    r.codes = np.array([int(c) for c in d["codes"]], np.uint8)
    r.resets = np.array([int(c) for c in d["resets"]], np.uint8)
    dt = np.float32 if game == R.RACE else np.uint8
    r.obs_after = _unhex(d["obs_after"], dt, (T, -1))
    r.obs = np.zeros((T + 1, r.obs_after.shape[1]), dt)
    for t in range(T + 1):
        r.obs[t] = _unhex(d["obs_start"][str(t)], dt, (-1,)) if str(t) in d["obs_start"] else r.obs_after[t - 1]
    r.cars = {int(t): _unhex(v, np.float32, (3,)) for t, v in d["car_start"].items()}
    r.cars_after = None
    r.ctor_car = _unhex(d["ctor_car"], np.float32, (3,)) if "ctor_car" in d else None
    r.n_actions = d["n_actions"]
    r.nth_thread = d["nth_thread"]
    r.num_steps = None
    return r


def assert_fixture_equals(fix, rec, what=""):
    """A fixture record against a full record of another implementation: every stored bit."""
    for name in ("rewards", "obs", "obs_after"):
        x, y = getattr(fix, name), getattr(rec, name)
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, name)
    assert np.array_equal(fix.codes, rec.codes) and np.array_equal(fix.resets, rec.resets), what
    assert fix.n_actions == rec.n_actions, what
    for t, car in fix.cars.items():
        assert np.array_equal(car.view(np.uint32), rec.cars[t].view(np.uint32)), (what, "start state", t)
    if fix.ctor_car is not None:
        assert np.array_equal(fix.ctor_car.view(np.uint32), rec.ctor_car.view(np.uint32)), (what, "constructor's start state")


FIX_POLICY_SEED = 0x51A9
# (flags, T, scripts): a script is ("policy", gid) -- the oracle's policy stream of env gid, which xwb_step_n replays -- or
# ("walk", pattern).  Short tracks so that finish lines, boundaries and wraps fall inside T steps.
_P2 = [("policy", 0), ("policy", 1)]
_W9 = [[1], [2], [1, 1, 1, 4, 1, 1, 7], [3, 3, 3, 3, 3, 1], [6, 6, 6, 6, 6, 1], [5], [8], [0, 3, 6, 2], [2, 5, 2, 8]]
FIXTURE_RACE = [
    ({}, 30, _P2),
    ({"track_type": "circle"}, 24, _P2),
    ({"track_length": 20.0, "track_width": 8.0}, 24, _P2 + [("walk", [0, 1])]),
    ({"track_length": 20.0, "track_width": 8.0, "difficulty": "hard", "reward_scale": 0.5}, 24, _P2 + [("walk", [0, 1])]),
    ({"track_type": "circle", "track_radius": 12.5, "track_width": 7.5, "difficulty": "hard", "reward_scale": 3.0}, 24, _P2),
    ({"track_length": 16.0, "track_width": 6.0, "race_full_manouver": True, "reward_scale": 3.0}, 20,
     _P2 + [("walk", p) for p in _W9]),
    ({"track_length": 16.0, "track_width": 6.0, "race_full_manouver": True, "difficulty": "hard"}, 20, _P2 + [("walk", [1])]),
    ({"track_type": "circle", "track_radius": 80.0, "track_width": 40.0, "race_full_manouver": True, "reward_scale": 0.5}, 20,
     _P2 + [("walk", [1])]),
    ({"track_length": 400.0, "track_width": 80.0, "context": 3, "max_steps": 9}, 12, _P2),
    ({"track_type": "circle", "race_full_manouver": True, "context": 3}, 12, _P2),
    ({"track_length": 30.0, "track_width": 8.0, "max_steps": 7, "difficulty": "hard"}, 16, _P2),
]
# random = true: (flags, T, envs, first thread): env i of the group runs on the reference's (first thread + i)-th thread and
# takes the policy stream of gid = its thread number - 1
FIXTURE_RACE_RANDOM = [
    ({"random": True, "simulator_seed": 1}, 10, 10, 230),
    ({"random": True, "simulator_seed": 2, "track_type": "circle", "race_full_manouver": True}, 10, 10, 256),
    ({"random": True, "simulator_seed": 77, "race_full_manouver": True, "difficulty": "hard", "track_length": 30.0}, 10, 10, 300),
]
# SimpleGame: (flags, T, number of random scripts); two policy streams and two scripted walks (all left, all right) are
# added to each
FIXTURE_GAME = [
    ({"array_size": 1}, 8, 0), ({"array_size": 2, "context": 2}, 8, 1), ({"array_size": 3, "context": 3}, 12, 1),
    ({"array_size": 6}, 16, 2), ({"array_size": 7, "context": 2}, 16, 1), ({"array_size": 16, "context": 3}, 16, 1),
    ({"array_size": 64}, 34, 0), ({"array_size": 6, "context": 3, "max_steps": 4}, 16, 2),
    ({"array_size": 16, "max_steps": 5}, 16, 1),
]


def fixture_scripts(oracle, game, flags, T, scripts):
    na = n_actions_of(game, flags)
    out = []
    for kind, arg in scripts:
        if kind == "policy":
            out.append((policy_actions(oracle, FIX_POLICY_SEED, arg, T, na), [FIX_POLICY_SEED, arg]))
        else:
            out.append((walk(T, arg), None))
    return out


def game_scripts(oracle, flags, T, n_random, n_policy=0):
    """(actions, policy) pairs: the policy stream of gids 0 .. n_policy - 1 (what xwb_step_n replays), all left, all right,
    and n_random biased coin walks."""
    rng = np.random.default_rng(1000 + flags["array_size"] * 7 + flags.get("context", 1))
    out = [(policy_actions(oracle, FIX_POLICY_SEED, g, T, 2), [FIX_POLICY_SEED, g]) for g in range(n_policy)]
    out += [(walk(T, [0]), None), (walk(T, [1]), None)]
    for k in range(n_random):
        p = (0.35, 0.5, 0.65, 0.5)[k % 4]
        out.append(([int(x) for x in (rng.random(T) < p)], None))
    return out
