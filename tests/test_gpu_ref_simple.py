"""race_kernel / sg_kernel against results recorded from a build of the reference's OWN sources
(tests/golden/ref_simple_race.json, ref_simple_game.json; tests/golden/make_ref_simple_golden.py) -- directly, with the oracle
not in the loop: reward bits, observation bits and game-over codes of every step, through step + reset_done, through
step_autoreset and, where the recorded actions are the built-in policy's, through xwb_step_n.  Each recorded env becomes many
envs of a batch (env e replays record e mod K), at batch sizes that put the records into different lanes and workgroups.
The random-reset records run with rng = "minstd": env e is the reference's (env_gid0 + e + 1)-th thread."""
import json
import os

import numpy as np
import pytest

import _ref as R
import _ref_cases as K

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _groups(name, game):
    with open(os.path.join(GOLDEN, name)) as f:
        doc = json.load(f)
    return [(g["flags"], g["T"], [K.record_from_json(d, game) for d in g["envs"]], [d["policy"] for d in g["envs"]])
            for g in doc["groups"]]


RACE = _groups("ref_simple_race.json", R.RACE)
GAME = _groups("ref_simple_game.json", R.GAME)
RACE_FIXED = [g for g in RACE if not g[0].get("random")]
RACE_RANDOM = [g for g in RACE if g[0].get("random")]


def _opts(game, flags):
    if game == R.GAME:
        return "simple_game", dict(flags)
    f = dict(R.RACE_DEFAULTS, **flags)
    o = {k: f[k] for k in ("track_type", "track_width", "track_length", "track_radius", "race_full_manouver", "random",
                           "difficulty", "reward_scale", "context", "max_steps")}
    if f["random"]:
        o.update(rng="minstd", simulator_seed=f["simulator_seed"], thread_base=0)
    return "simple_race", o


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _replay(game, flags, T, recs, n, mode, e0=0, gid0=0):
    """env e0 + i replays record i mod K for every i that fits (random-reset records: once each, others idle on action 0)."""
    torch = _torch()
    from xworld_amd.batched import BatchedSimulator
    name, opts = _opts(game, flags)
    K_ = len(recs)
    rnd = bool(flags.get("random"))
    which = np.full(n, -1)
    for e in range(e0, n if not rnd else min(n, e0 + K_)):
        which[e] = (e - e0) % K_
    cmp_envs = np.flatnonzero(which >= 0)
    w = which[cmp_envs]
    sim = BatchedSimulator(name, opts, num_envs=n, env_gid0=gid0)
    sim.reset()                                                    # SimulatorInterface::reset_game after the constructor
    width = recs[0].obs.shape[1]

    def obs():
        return _bits(sim.obs.cpu().numpy().reshape(n, width)[cmp_envs])

    def want(field, t):
        return _bits(np.stack([getattr(recs[k], field)[t] for k in w]))

    assert sim.num_actions == recs[0].n_actions
    assert np.array_equal(obs(), want("obs", 0)), "start state"
    for t in range(T):
        acts = np.zeros(n, np.int32)
        acts[cmp_envs] = [recs[k].actions[t] for k in w]
        a = torch.from_numpy(acts).cuda()
        if mode == "step":
            sim.step(a, act_rep=1)
            assert np.array_equal(obs(), want("obs_after", t)), ("obs after step", t)
        else:
            sim.step_autoreset(a, act_rep=1)
        assert np.array_equal(_bits(sim.reward.cpu().numpy()[cmp_envs]), want("rewards", t)), ("reward", t)
        assert np.array_equal(sim.game_over_codes.cpu().numpy()[cmp_envs], want("codes", t)), ("code", t)
        if mode == "step":
            sim.reset_done()
        assert np.array_equal(obs(), want("obs", t + 1)), ("obs before the next step", t)
    assert sim.check_errors() == 0
    sim.close()


@pytest.mark.parametrize("mode", ["step", "autoreset"])
@pytest.mark.parametrize("n", [1, 65, 257, 4099])
@pytest.mark.parametrize("gi", range(len(RACE_FIXED)))
def test_race_kernel_equals_the_reference_records(gi, n, mode):
    flags, T, recs, _ = RACE_FIXED[gi]
    _replay(R.RACE, flags, T, recs, n, mode)


@pytest.mark.parametrize("mode", ["step", "autoreset"])
@pytest.mark.parametrize("n,e0", [(20, 0), (65, 33), (257, 225)])
@pytest.mark.parametrize("gi", range(len(RACE_RANDOM)))
def test_race_kernel_random_reset_equals_the_reference_threads(gi, n, e0, mode):
    """rng = "minstd": the recorded envs ran on threads first .. first + K - 1 of the reference; env e0 + i of the batch is made
    that thread by env_gid0, which puts the records at lane / workgroup offsets 0, 33 and 225."""
    flags, T, recs, _ = RACE_RANDOM[gi]
    gid0 = recs[0].nth_thread - 1 - e0
    assert gid0 >= 0
    _replay(R.RACE, flags, T, recs, n, mode, e0=e0, gid0=gid0)


@pytest.mark.parametrize("mode", ["step", "autoreset"])
@pytest.mark.parametrize("n", [1, 65, 257, 4099])
@pytest.mark.parametrize("gi", range(len(GAME)))
def test_sg_kernel_equals_the_reference_records(gi, n, mode):
    flags, T, recs, _ = GAME[gi]
    _replay(R.GAME, flags, T, recs, n, mode)


STEP_N = [(R.RACE, g) for g in RACE] + [(R.GAME, g) for g in GAME]


@pytest.mark.parametrize("ci", range(len(STEP_N)))
def test_step_n_replays_the_recorded_policy_runs(ci):
    """Records whose actions are the built-in policy's stream of env gid, race_kernel and sg_kernel: xwb_step_n (every step and
    reset inside one launch) must leave the reward, code and observation the reference recorded at the split point and at the
    end."""
    _torch()
    from xworld_amd.batched import BatchedSimulator
    game, (flags, T, recs, pols) = STEP_N[ci]
    idx = [i for i, p in enumerate(pols) if p]
    gids = [pols[i][1] for i in idx]
    if not idx or gids != list(range(gids[0], gids[0] + len(gids))):
        pytest.fail("fixture group %d holds no run of consecutive policy records" % ci)
    name, opts = _opts(game, flags)
    sim = BatchedSimulator(name, opts, num_envs=len(idx), env_gid0=gids[0], policy_seed=pols[idx[0]][0])
    sim.reset()
    done = 0
    for k in (T // 3, T - T // 3):
        sim.step_n(k, act_rep=1)
        done += k
        t = done - 1
        assert np.array_equal(sim.actions.cpu().numpy(), [recs[i].actions[t] for i in idx])
        assert np.array_equal(_bits(sim.reward.cpu().numpy()), _bits(np.array([recs[i].rewards[t] for i in idx], np.float32)))
        assert np.array_equal(sim.game_over_codes.cpu().numpy(), [recs[i].codes[t] for i in idx])
        assert np.array_equal(_bits(sim.obs.cpu().numpy().reshape(len(idx), -1)), _bits(np.stack([recs[i].obs[done] for i in idx])))
    sim.close()


def test_live_reference_against_the_kernel(oracle):
    """Where oracle/_ref/libxwref.so travelled along: 2048 reference objects x 300 steps under the built-in policy against
    race_kernel's step + reset_done, straight and circle.  (`oracle` only supplies the policy's action stream.)"""
    R.require()
    torch = _torch()
    from xworld_amd.batched import BatchedSimulator
    n, T = 2048, 300
    for flags in (dict(track_length=60.0), dict(track_type="circle", race_full_manouver=True, difficulty="hard", reward_scale=0.5)):
        na = K.n_actions_of(R.RACE, flags)
        recs = [R.rollout(R.RACE, flags, K.policy_actions(oracle, 21, e, T, na)) for e in range(n)]
        name, opts = _opts(R.RACE, flags)
        sim = BatchedSimulator(name, opts, num_envs=n, policy_seed=21)
        sim.reset()
        rew, codes, ob = (np.stack([getattr(r, f) for r in recs]) for f in ("rewards", "codes", "obs"))
        for t in range(T):
            assert np.array_equal(_bits(sim.obs.cpu().numpy().reshape(n, 4)), _bits(ob[:, t])), t
            sim.step()
            assert np.array_equal(_bits(sim.reward.cpu().numpy()), _bits(rew[:, t])), t
            assert np.array_equal(sim.game_over_codes.cpu().numpy(), codes[:, t]), t
            sim.reset_done()
        assert int(np.stack([r.resets for r in recs]).sum()) > 0          # the reference's run held resets at all
        sim.close()
