"""SimpleRace and SimpleGame: a build of the reference's OWN sources (oracle/_ref/libxwref.so, tests/_ref.py) against the
oracle (oracle/simple_race.c, simple_game.c), on bit patterns only -- reward as uint32, every observation float, the car, the
game-over code, the step count, where each reset happened.  No tolerance anywhere.

The coverage conditions are asserted on what the REFERENCE run did (tests/_ref_cases.py coverage()), so a comparison cannot
pass by never visiting a branch.  That includes `cos_theta`'s clamp (simple_race_simulator.cpp:415-416): the double sum
exceeds 1 in the deterministic sweep, which coverage() sees by repeating get_tangent_vec and the sum on the reference's car with
the source's operand types (after narrowing to float the clamp itself cannot be seen in the screen)."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _ref as R
import _ref_cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# straight (width, length) / circle (width, radius): the defaults, the two doc-image geometries
# (tests/test_oracle_race_doc_images.py: straight 80 x 400, circle width 40 radius 80), and short odd ones
GEOM = {"straight": [dict(), dict(track_width=80.0, track_length=400.0), dict(track_width=8.0, track_length=30.0),
                     dict(track_width=33.3, track_length=55.5)],
        "circle": [dict(), dict(track_width=40.0, track_radius=80.0), dict(track_width=7.5, track_radius=12.5),
                   dict(track_width=33.3, track_radius=47.1)]}


def test_simple_race_reference_equals_oracle_and_visits_every_branch(oracle):
    R.require()
    seen, env_steps, resets, configs = {}, 0, 0, 0
    combos = itertools.product(("straight", "circle"), ("easy", "hard"), (False, True), (1.0, 0.5, 3.0))
    for i, (track, diff, full, scale) in enumerate(combos):
        for j, geom in enumerate(GEOM[track]):
            # max_steps {0, small} and context {1, 3} rotate over the configurations: each pair meets every track / difficulty
            max_steps, context = [(0, 1), (0, 3), (13, 1), (40, 3)][(i + j) % 4]
            flags = dict(geom, track_type=track, difficulty=diff, race_full_manouver=full, reward_scale=scale,
                         max_steps=max_steps, context=context)
            na = K.n_actions_of(R.RACE, flags)
            T = 260
            scripts = [K.policy_actions(oracle, 900 + i, gid, T, na) for gid in range(4)]
            scripts += [K.walk(T, p) for p in (K.WALKS9 if full else K.WALKS2)]
            for k, acts in enumerate(scripts):
                ref = R.rollout(R.RACE, flags, acts)
                orc = K.oracle_rollout(oracle, R.RACE, flags, acts)
                K.assert_same(ref, orc, "%s script %d" % (flags, k))
                K.coverage(flags, ref, seen)
                env_steps += T
                resets += int(ref.resets.sum())
            configs += 1
    print("simple_race: %d configurations, %d env-steps, %d resets; reference visited: %s" % (configs, env_steps, resets,
                                                                                              sorted(seen.items())))
    missing = [b for b in K.BRANCHES if not seen.get(b)]
    assert not missing, missing
    assert resets > 1000


@pytest.mark.parametrize("sim_seed", [1, 2, 77])
def test_simple_race_random_reset_on_reference_threads(oracle, sim_seed):
    """random = true: 64 envs, each on its own thread of the reference, started one after the other, so env e is the
    (e + 1 + base)-th thread the reference's counter sees; the oracle's minstd path with (simulator_seed, nth_thread) must give
    the constructor's start state, the start position / angle of every reset, and the rollouts."""
    L = R.require()
    seen, resets = {}, 0
    for track, full, diff in (("straight", False, "easy"), ("circle", True, "hard"), ("straight", True, "hard"), ("circle", False, "easy")):
        flags = dict(track_type=track, race_full_manouver=full, difficulty=diff, random=True, simulator_seed=sim_seed,
                     track_length=60.0)
        na = K.n_actions_of(R.RACE, flags)
        R.set_flags(R.RACE, flags)
        base = L.xwref_threads()
        for e in range(64):
            acts = K.policy_actions(oracle, 4, e, 120, na)
            ref = R.rollout(R.RACE, flags, acts)
            assert ref.nth_thread == e + 1 + base
            orc = K.oracle_rollout(oracle, R.RACE, flags, acts, nth_thread=ref.nth_thread)
            K.assert_same(ref, orc, "seed %d %s env %d" % (sim_seed, track, e))
            K.coverage(flags, ref, seen)
            resets += int(ref.resets.sum())
        # the single track of the pool is chosen by a draw too (RaceEngine::reset_game): four draws per reset is what the
        # equal start states of every later reset already show
    print("seed %d: %d random resets; reference visited: %s" % (sim_seed, resets, sorted(seen.items())))
    assert resets > 64
    assert seen.get("wrap_above_2pi") and seen.get("wrap_below_0")


def test_simple_game_reference_equals_oracle(oracle):
    R.require()
    env_steps = codes = 0
    for size, context, max_steps in itertools.product((1, 2, 3, 6, 7, 16, 64), (1, 2, 3), (0, 5)):
        flags = dict(array_size=size, context=context, max_steps=max_steps)
        for acts, _ in K.game_scripts(oracle, flags, 3 * size + 20, 4):
            ref = R.rollout(R.GAME, flags, acts)
            orc = K.oracle_rollout(oracle, R.GAME, flags, acts)
            K.assert_same(ref, orc, str(flags))
            env_steps += len(acts)
            codes |= 1 << int(ref.codes.max())
    print("simple_game: %d env-steps" % env_steps)
    assert codes & (1 << 4) and codes & (1 << 1)             # the reference ended games by SUCCESS and by MAX_STEP


def test_handle_api_agrees_with_the_thread_rollout(oracle):
    """The per-call entry points (create, reset_game, take_actions through a StatePacket, game_over, get_screen,
    get_num_actions, the car) give what the threaded rollout recorded."""
    L = R.require()
    flags = dict(track_type="circle", race_full_manouver=True, context=3)
    acts = K.policy_actions(oracle, 11, 0, 50, 9)
    rec = R.rollout(R.RACE, flags, acts)
    R.set_flags(R.RACE, flags)
    h = L.xwref_create(R.RACE)
    assert L.xwref_get_num_actions(h) == 9 and L.xwref_get_lives(h) == 1
    L.xwref_reset_game(h)
    obs, scr, car = np.zeros(12, np.float32), np.zeros(4, np.float32), np.zeros(3, np.float32)
    for t, a in enumerate(acts):
        if L.xwref_game_over(h):
            L.xwref_reset_game(h)
        assert L.xwref_get_state_screen(h, obs.ctypes.data) == 12 and L.xwref_get_screen(h, scr.ctypes.data) == 4
        assert np.array_equal(obs.view(np.uint32), rec.obs[t].view(np.uint32)) and np.array_equal(scr, obs[8:])
        r = np.float32(L.xwref_take_actions(h, a, 1))
        L.xwref_get_car(h, car.ctypes.data_as(R.C.POINTER(R.C.c_float)))
        assert r.view(np.uint32) == rec.rewards[t].view(np.uint32) and L.xwref_game_over(h) == rec.codes[t]
        assert np.array_equal(car.view(np.uint32), rec.cars_after[t].view(np.uint32))
        assert L.xwref_get_num_steps(h) == rec.num_steps[t]
    L.xwref_destroy(h)


def test_a_failed_check_of_the_reference_aborts():
    """The glog stand-in: CHECK_LT(action_id, _legal_actions.size()) must stop the process with its message, not pass."""
    R.require()
    code = ("import sys; sys.path.insert(0, %r); import _ref as R; R.set_flags(R.RACE, {}); L = R.lib(); "
            "h = L.xwref_create(R.RACE); L.xwref_take_actions(h, 2, 1); print('survived')" % os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == -6 and "survived" not in p.stdout
    assert "Check failed: (action_id) < (_legal_actions.size())" in p.stderr


def test_fixtures_regenerate_byte_for_byte(tmp_path):
    R.require()
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, "make_ref_simple_golden.py"), str(tmp_path)])
    for name in ("ref_simple_race.json", "ref_simple_game.json"):
        with open(os.path.join(GOLDEN, name), "rb") as a, open(str(tmp_path / name), "rb") as b:
            assert a.read() == b.read(), name


@pytest.mark.parametrize("name,game", [("ref_simple_race.json", R.RACE), ("ref_simple_game.json", R.GAME)])
def test_fixtures_replay_through_the_oracle(oracle, name, game):
    """Runs without the reference: the recorded results of the reference's programs against the oracle."""
    with open(os.path.join(GOLDEN, name)) as f:
        doc = json.load(f)
    n = 0
    for g in doc["groups"]:
        for k, d in enumerate(g["envs"]):
            fix = K.record_from_json(d, game)
            if d["policy"]:
                assert list(fix.actions) == K.policy_actions(oracle, d["policy"][0], d["policy"][1], g["T"], fix.n_actions)
            orc = K.oracle_rollout(oracle, game, g["flags"], fix.actions, nth_thread=fix.nth_thread)
            K.assert_fixture_equals(fix, orc, "%s env %d" % (g["flags"], k))
            n += g["T"]
    assert n > 0
