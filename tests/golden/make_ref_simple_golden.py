"""Records tests/golden/ref_simple_race.json and ref_simple_game.json from oracle/_ref/libxwref.so, the build of the
reference's own SimpleRace / SimpleGame sources (`make -C oracle ref`): flags, action lists and, per step, the reward bits,
observation bits and game-over codes the reference's programs returned, plus the start states of the random resets.

    python tests/golden/make_ref_simple_golden.py [out_dir]

Run it in a fresh process: the reference numbers its threads from the start of the process, and the random-reset cases record
which thread each env ran on.  tests/test_ref_simple.py regenerates the files and compares the bytes."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _oracle as O            # noqa: E402  (only its policy function: the action lists)
import _ref as R               # noqa: E402
import _ref_cases as K         # noqa: E402


def dump(path, doc):
    """One line per group."""
    js = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"what":%s,\n"groups":[\n%s\n]}\n' % (js(doc["what"]), ",\n".join(js(g) for g in doc["groups"])))


def main(out_dir):
    L = R.lib()
    assert L.xwref_threads() == 0
    groups = []
    for flags, T, scripts in K.FIXTURE_RACE:
        envs = [K.record_to_json(R.rollout(R.RACE, flags, acts), pol) for acts, pol in K.fixture_scripts(O, R.RACE, flags, T, scripts)]
        groups.append({"flags": flags, "T": T, "envs": envs})
    for flags, T, n, first in K.FIXTURE_RACE_RANDOM:
        R.set_flags(R.RACE, flags)                     # the counter only counts while the seed flag is set
        L.xwref_burn_threads(first - 1 - L.xwref_threads())
        envs = []
        for i in range(n):
            gid = first + i - 1
            rec = R.rollout(R.RACE, flags, K.policy_actions(O, K.FIX_POLICY_SEED, gid, T, K.n_actions_of(R.RACE, flags)))
            assert rec.nth_thread == first + i
            envs.append(K.record_to_json(rec, [K.FIX_POLICY_SEED, gid], cars=True))
        groups.append({"flags": flags, "T": T, "envs": envs})
    dump(os.path.join(out_dir, "ref_simple_race.json"),
         {"what": "results recorded from a build of the reference's own SimpleRace sources (make_ref_simple_golden.py)",
          "groups": groups})
    groups = []
    for flags, T, n in K.FIXTURE_GAME:
        envs = [K.record_to_json(R.rollout(R.GAME, flags, acts), pol) for acts, pol in K.game_scripts(O, flags, T, n, n_policy=2)]
        groups.append({"flags": flags, "T": T, "envs": envs})
    dump(os.path.join(out_dir, "ref_simple_game.json"),
         {"what": "results recorded from a build of the reference's own SimpleGame sources (make_ref_simple_golden.py)",
          "groups": groups})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
