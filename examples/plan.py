#!/usr/bin/env python3
"""Random shooting on the true dynamics without a single child slot: every step, K random plans of H actions per env go through
evaluate_plans (one launch, nothing written), and each env takes the first action of its best plan.

    python examples/plan.py [envs] [rounds] [K] [H]

A plan that reaches the goal within H steps is scored by its return (the sooner the better); a plan that dies or runs out of
time scores below everything else; plans still alive after H steps -- all of them, far from the goal -- are told apart by the
expert's distance field at the node where they end, the leaf value of a tree search.  The win rate is printed beside that of
the random policy on a batch of the same envs.  examples/lookahead.py does one-step look-ahead the other way, by forking.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xworld_amd.batched import BatchedSimulator      # noqa: E402

CONF = os.path.join(ROOT, "xworld_amd", "confs", "navigation2d.json")
SUCCESS = 4                                          # XWB_SUCCESS
FAR = 1 << 15                                        # the distance of a node without a path


def shoot(sim, k, h, gen):
    """the first action of each env's best plan among k random ones of length h: int32 CUDA tensor [num_envs]"""
    import torch
    n = sim.num_envs
    plans = torch.randint(0, sim.num_actions, (n, k, h), dtype=torch.int8, device="cuda", generator=gen)
    ret, steps, codes, last = sim.evaluate_plans(plans, gamma=0.95, last=True)
    _, _, field = sim.expert(field=True)             # uint16 [n, headings, cells], 0xFFFF = no path
    flat = field.reshape(n, -1).view(torch.int16).to(torch.int64) & 0xFFFF
    cells = field.shape[2]
    node = (last >> 16).to(torch.int64) * cells + (last & 0xffff).to(torch.int64)
    leaf = torch.gather(flat, 1, node.clamp(min=0))
    leaf = torch.where(leaf == 0xFFFF, torch.full_like(leaf, FAR), leaf)
    won, over = (codes & SUCCESS) != 0, codes != 0
    # one score, higher is better: winners by return, then the live plans by closeness of their last node, then the dead
    score = torch.where(won, 2.0 + ret, torch.where(over, torch.full_like(ret, -1.0), 1.0 / (1.0 + leaf.to(torch.float32))))
    best = score.argmax(dim=1)
    return plans[torch.arange(n, device="cuda"), best, 0].to(torch.int32)


def main():
    import torch
    envs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    h = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    opts = {"xwd_conf_path": CONF, "task_mode": "lang_acquisition", "max_dim": 7, "num_blocks": 16, "color": True}
    sim = BatchedSimulator("xworld", opts, num_envs=envs)
    rnd = BatchedSimulator("xworld", opts, num_envs=envs)
    sim.set_draw(False)                              # nobody looks at the frames here
    rnd.set_draw(False)
    gen = torch.Generator(device="cuda").manual_seed(1)
    wins = ends = rwins = rends = 0
    for _ in range(rounds):
        sim.step(shoot(sim, k, h, gen))
        wins += int(((sim.game_over_codes & SUCCESS) != 0).sum())
        ends += int((sim.game_over_codes != 0).sum())
        sim.reset_done()
        rnd.step()                                   # the built-in random policy
        rwins += int(((rnd.game_over_codes & SUCCESS) != 0).sum())
        rends += int((rnd.game_over_codes != 0).sum())
        rnd.reset_done()
    print("%d envs x %d steps, %d plans of %d steps per decision" % (envs, rounds, k, h))
    print("random shooting: %d episodes ended, %d won (%.1f %%), %.2f wins per 100 env-steps"
          % (ends, wins, 100.0 * wins / max(ends, 1), 100.0 * wins / (envs * rounds)))
    print("random policy:   %d episodes ended, %d won (%.1f %%), %.2f wins per 100 env-steps"
          % (rends, rwins, 100.0 * rwins / max(rends, 1), 100.0 * rwins / (envs * rounds)))
    assert sim.check_errors() == 0
    sim.close()
    rnd.close()


if __name__ == "__main__":
    main()
