#!/usr/bin/env python3
"""Random-policy rollouts, the shape of the reference's python/examples/test_*.py -- once through the
py_simulator-compatible object (one env, Python dicts), once through the batch API (device tensors).

    python examples/rollout.py [simple_game|simple_race|xworld|xworld_ego] [--frames DIR [--frame-envs K]] [--symbolic]

--frames DIR (xworld, xworld_ego): the batch rollout also writes the first K envs' views of every step (render_view: the
64-pixel-per-cell image behind the observation) as DIR/<game>_env<e>_step<t>.png -- what take_actions(..., show_screen=True)
put into a window.  Views are B,G,R like the reference's cv::Mat; they are flipped to R,G,B for the PNG here.

--symbolic (xworld, xworld_ego): the batch rollout prints env 0's symbolic observation at every step -- the KIND plane of
BatchedSimulator.symbolic() as characters ('.' empty, 'G' goal, '#' block, 'A' agent, ' ' dark) beside the teacher's sentence.
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xworld_amd.batched import BatchedSimulator      # noqa: E402
from xworld_amd.py_simulator import Simulator        # noqa: E402

CONF = os.path.join(ROOT, "xworld_amd", "confs", "navigation2d.json")
OPTS = {
    "simple_game": ("simple_game", {"array_size": 16}),
    "simple_race": ("simple_race", {"track_type": "straight", "track_width": 20.0, "track_length": 100.0, "track_radius": 30.0}),
    "xworld": ("xworld", {"xwd_conf_path": CONF, "task_mode": "lang_acquisition", "color": True}),
    "xworld_ego": ("xworld", {"xwd_conf_path": CONF, "task_mode": "lang_acquisition", "color": True, "visible_radius": 3}),
}


def single_env(name, opts, steps=200):
    """python/examples/test_simple_game.py:15-30 / test_xworld.py:41-60"""
    game = Simulator.create(name, opts)
    game.reset_game()
    n_actions = game.get_num_actions()
    total, episodes = 0.0, 0
    for _ in range(steps):
        if game.game_over() != "alive":
            episodes += 1
            game.reset_game()
        state = game.get_state()                     # {"screen": [floats], ("sentence": str, ...)}
        if "sentence" in state and state["sentence"] != "-" and total == 0.0:
            print("teacher:", state["sentence"])
        total += game.take_actions({"action": random.randrange(n_actions)}, 1, False)
    print("%s: 1 env, %d steps, %d episodes, reward %.2f, screen %s" % (name, steps, episodes, total,
                                                                       game.get_screen_out_dimensions()))


SYM_CHARS = ".G#A "                                   # SYM_EMPTY, SYM_GOAL, SYM_BLOCK, SYM_AGENT, SYM_DARK


def print_symbolic(sim, t):
    """env 0: the KIND plane as characters, the teacher's sentence beside its first line"""
    from xworld_amd.batched import SYM_PLANE_KIND
    kind = sim.symbolic()[0, SYM_PLANE_KIND].cpu().numpy()
    sentence = sim.sentence(0) or "-"
    for i, row in enumerate(kind):
        print("symbolic step %3d  |%s|%s" % (t, "".join(SYM_CHARS[v] for v in row), "  teacher: " + sentence if i == 0 else ""))


def batch(name, opts, num_envs=4096, steps=200, frames=None, frame_envs=4, tag="", policy="random", symbolic=False):
    import torch
    sim = BatchedSimulator(name, opts, num_envs=num_envs)
    symbolic = symbolic and name == "xworld"
    view = None
    if frames and name == "xworld":
        from PIL import Image
        os.makedirs(frames, exist_ok=True)
        k = min(frame_envs, num_envs)
        view = torch.empty((k,) + sim.view_dims, dtype=torch.uint8, device="cuda")     # reused by every step
    total = torch.zeros(num_envs, device="cuda")
    finished = 0
    expert = policy == "expert" and name == "xworld"
    started = no_path = 0                            # expert: episodes begun, and those that began without any winning path
    fresh = torch.ones(num_envs, dtype=torch.bool, device="cuda")
    for t in range(steps):
        if expert:                                   # the shortest path to the task's goal, computed on the device
            actions, dist = sim.expert()
            started += int(fresh.sum())
            no_path += int((fresh & (dist < 0)).sum())
        else:
            actions = torch.randint(0, sim.num_actions, (num_envs,), dtype=torch.int32, device="cuda")
        sim.step(actions)                            # obs / reward / game_over_codes are device tensors (views)
        total += sim.reward
        finished += int((sim.game_over_codes != 0).sum())
        if view is not None:                         # (before the reset: a finished env still shows its last state)
            rgb = sim.render_view(k, out=view).flip(-1).cpu().numpy()                  # B,G,R -> R,G,B
            for e in range(k):
                Image.fromarray(rgb[e]).save(os.path.join(frames, "%s_env%d_step%04d.png" % (tag, e, t)))
        if symbolic:                                 # (before the reset, like the views)
            print_symbolic(sim, t)
        fresh = sim.game_over_codes != 0
        sim.reset_done()                             # `if game_over: reset_game()` for the whole batch
    print("%s: %d envs, %d steps, %d episodes finished, mean reward %.3f, obs %s %s" % (
        name, num_envs, steps, finished, float(total.mean()), tuple(sim.obs.shape), sim.obs.dtype))
    if expert:
        perf, _ = sim.task_performance()
        print("expert policy: %d successes, %d failures; %d of %d episodes (%.1f %%) started without a path" % (
            sum(v[0] for v in perf.values()), sum(v[1] for v in perf.values()), no_path, started, 100.0 * no_path / max(started, 1)))
    sim.close()


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("games", nargs="*", metavar="|".join(OPTS))
    ap.add_argument("--frames", metavar="DIR", help="write the first K envs' views of every step as PNGs (xworld, xworld_ego)")
    ap.add_argument("--frame-envs", type=int, default=4, metavar="K")
    ap.add_argument("--policy", choices=["random", "expert"], default="random",
                    help="expert: xworld batches follow BatchedSimulator.expert (the other games stay random)")
    ap.add_argument("--symbolic", action="store_true", help="print env 0's symbolic observation at every step (xworld, xworld_ego)")
    ap.add_argument("--steps", type=int, default=200, metavar="N", help="steps of each rollout")
    args = ap.parse_args()
    for w in args.games or list(OPTS):
        if w not in OPTS:
            ap.error("unknown game " + w)
        name, opts = OPTS[w]
        single_env(name, dict(opts), steps=args.steps)
        batch(name, dict(opts), steps=args.steps, frames=args.frames, frame_envs=args.frame_envs, tag=w, policy=args.policy,
              symbolic=args.symbolic)
