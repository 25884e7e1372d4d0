#!/usr/bin/env python3
"""One-step look-ahead on the true dynamics, on the device: fork every root env into one child per action inside ONE batch
(copy_envs), step the children with their action while the roots sit the step out, and keep the action whose child is
closest to the goal.

    python examples/lookahead.py [roots] [rounds]

Layout of a batch of R * (1 + A) envs, A = num_actions: roots are envs 0 .. R - 1, root i's child for action a is env
R + A * i + a.  Children are overwritten by every fork; only the roots carry the rollout.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xworld_amd.batched import BatchedSimulator      # noqa: E402

CONF = os.path.join(ROOT, "xworld_amd", "confs", "navigation2d.json")
SKIP, SUCCESS, FAR = -1, 4, 1 << 20                  # XWB_ACTION_SKIP, XWB_SUCCESS; the score of a child that cannot win


def lookahead(sim, roots):
    """The best first action of envs 0 .. roots - 1 by trying every action on a fork: int64 CUDA tensor [roots], the lowest
    action id among equally good ones.  A child's score: 0 if its step won, else the expert's distance to the goal after it
    (FAR for a child that died, timed out or has no path).  The roots are not stepped; the children end reset and live."""
    import torch
    r, a = int(roots), sim.num_actions
    if sim.num_envs < r * (1 + a):
        raise ValueError("%d roots with %d actions need %d envs, the batch has %d" % (r, a, r * (1 + a), sim.num_envs))
    dev = torch.device("cuda", sim.device)
    kids = torch.arange(r * a, dtype=torch.int32, device=dev)
    sim.copy_envs(kids + r, torch.div(kids, a, rounding_mode="floor").to(torch.int32))
    actions = torch.full((sim.num_envs,), SKIP, dtype=torch.int32, device=dev)
    actions[r:r + r * a] = kids % a
    sim.step(actions)
    _, dist = sim.expert()                           # (-1: no path, or the child's episode is over)
    dist = dist[r:r + r * a].to(torch.int64)
    codes = sim.game_over_codes[r:r + r * a].to(torch.int64)
    score = torch.where(dist > 0, dist, torch.full_like(dist, FAR))
    score = torch.where((codes & SUCCESS) != 0, torch.zeros_like(score), score).view(r, a)
    best = score.argmin(dim=1)                       # (ties: the first, i.e. lowest, action)
    sim.reset_done()                                 # finished children start over: every env is live again
    return best


def main():
    import torch
    roots = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    sim = BatchedSimulator("xworld", {"xwd_conf_path": CONF, "task_mode": "lang_acquisition", "color": True}, num_envs=roots * 5)
    wins = agree = 0
    for _ in range(rounds):
        expert = sim.expert()[0][:roots].clone()         # (expert() reuses its tensors: lookahead() calls it again)
        best = lookahead(sim, roots)
        agree += int((best == expert).sum())
        actions = torch.full((sim.num_envs,), SKIP, dtype=torch.int32, device=best.device)
        actions[:roots] = best.to(torch.int32)
        sim.step(actions)
        wins += int(((sim.game_over_codes[:roots] & SUCCESS) != 0).sum())
        sim.reset_done()
    print("%d roots x %d rounds: %d goals reached, look-ahead = expert's action in %d of %d decisions"
          % (roots, rounds, wins, agree, roots * rounds))
    assert sim.check_errors() == 0
    sim.close()


if __name__ == "__main__":
    main()
