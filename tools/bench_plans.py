"""Times xwb_xw_evaluate_plans (BatchedSimulator.evaluate_plans) on one GPU against the fork route, in one process:

  verb   one launch: K plans of H steps for each of N envs, N * K = 32 768 plans, nothing written
  fork   the only route the verbs before it offer: copy_envs of every root into K child slots of a batch of N * (K + 1) envs with
         set_draw(0) (full observation; egocentric batches always draw), then H x (step with the children's actions -- XWB_ACTION_SKIP for the roots and for finished children --,
         the torch ops that mask and accumulate returns, steps and codes, reset_done): 2 H + 1 launches of the library plus the
         torch kernels

for H = 4, 8, 16, under full observation at 7 x 7 and egocentric at r = 3.  Device events around `calls` back-to-back
evaluations after a warm-up, best of `blocks`: when the host enqueues slower than the kernels run the figure is the enqueue rate
(an upper bound of the device time), which is what a caller of either route sees.  The two routes are checked against each other
once per row (steps, codes, return bits) before they are timed.

    python tools/bench_plans.py [--envs 512] [--plans 64] [--calls 20] [--blocks 3]

Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONF = os.path.join(ROOT, "xworld_amd", "confs", "navigation2d.json")
SKIP = -1


def events(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls                  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--plans", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_plans.py needs a GPU")
    from xworld_amd import build, lib
    from xworld_amd.batched import BatchedSimulator
    n, k, gamma = args.envs, args.plans, 0.95
    rows = [("xworld7", {"color": True}), ("xworld7_ego3", {"color": True, "visible_radius": 3})]
    print("evaluate_plans against the fork route (copy_envs + H x (step + torch bookkeeping + reset_done)), %d envs x %d plans = %d plans "
          "(device events, %d calls, best of %d blocks); source %s on %s" % (n, k, n * k, args.calls, args.blocks, build.source_fingerprint(),
                                                                            torch.cuda.get_device_name(0)))
    print("| batch | envs | plans per env | H | evaluate_plans us (<=) | fork route us | fork / verb | library launches of the fork route |")
    print("|---|---|---|---|---|---|---|---|")
    out = []
    for name, opts in rows:
        o = {"xwd_conf_path": CONF, "task_mode": "lang_acquisition", "max_dim": 7, "num_blocks": 16}
        o.update(opts)
        sim = BatchedSimulator("xworld", o, num_envs=n * (k + 1))          # roots 0 .. n - 1, root r's child for plan j: n + r * k + j
        if not sim.cfg.visible_radius:
            sim.set_draw(False)                                # (egocentric frames cannot be switched off: that row's fork route draws them)
        for _ in range(10):                                    # a batch in mid-rollout, every env live
            sim.step()
            sim.reset_done()
        na = sim.num_actions
        roots = torch.arange(n, dtype=torch.int32, device="cuda")
        kids = torch.arange(n, n * (k + 1), dtype=torch.int32, device="cuda")
        parents = roots.repeat_interleave(k).contiguous()
        gen = torch.Generator(device="cuda").manual_seed(3)
        for h in (4, 8, 16):
            plans = torch.randint(0, na, (n, k, h), dtype=torch.int8, device="cuda", generator=gen)
            ret = torch.empty((n, k), dtype=torch.float32, device="cuda")
            steps = torch.empty((n, k), dtype=torch.int32, device="cuda")
            codes = torch.empty((n, k), dtype=torch.uint8, device="cuda")
            verb = lambda: lib.check(sim.L.xwb_xw_evaluate_plans(sim.h, C.c_void_p(roots.data_ptr()), n, C.c_void_p(plans.data_ptr()), k, h, 1,
                                                                 gamma, C.c_void_p(ret.data_ptr()), C.c_void_p(steps.data_ptr()),
                                                                 C.c_void_p(codes.data_ptr()), None, None))
            per_step = plans.reshape(n * k, h).t().contiguous().to(torch.int32)      # [h][n * k]
            acts = torch.full((sim.num_envs,), SKIP, dtype=torch.int32, device="cuda")
            f_ret = torch.empty(n * k, dtype=torch.float32, device="cuda")
            f_steps = torch.empty(n * k, dtype=torch.int32, device="cuda")
            f_codes = torch.empty(n * k, dtype=torch.uint8, device="cuda")
            skip = torch.full((n * k,), SKIP, dtype=torch.int32, device="cuda")

            def fork():
                sim.copy_envs(kids, parents)
                live = torch.ones(n * k, dtype=torch.bool, device="cuda")
                f_ret.zero_(); f_steps.zero_(); f_codes.zero_()
                g = 1.0
                for t in range(h):
                    acts[n:] = torch.where(live, per_step[t], skip)
                    sim.step(acts)
                    f_ret.add_(torch.where(live, sim.reward[n:] * g, torch.zeros_like(f_ret)))
                    f_steps.add_(live.to(torch.int32))
                    ended = live & (sim.game_over_codes[n:] != 0)
                    f_codes.copy_(torch.where(ended, sim.game_over_codes[n:], f_codes))
                    live = live & ~ended
                    g = float(torch.tensor(g, dtype=torch.float32) * torch.tensor(gamma, dtype=torch.float32))
                    sim.reset_done()

            verb()
            fork()
            torch.cuda.synchronize()
            same = bool(torch.equal(steps.reshape(-1), f_steps) and torch.equal(codes.reshape(-1), f_codes)
                        and torch.equal(ret.reshape(-1).view(torch.int32), f_ret.view(torch.int32)))
            us_verb = min(events(torch, verb, args.calls) for _ in range(args.blocks))
            us_fork = min(events(torch, fork, max(2, args.calls // 4)) for _ in range(args.blocks))
            print("| %s | %d | %d | %d | %.1f | %.1f | %.0f | %d |%s" % (name, n, k, h, us_verb, us_fork, us_fork / us_verb, 2 * h + 1,
                                                                        "" if same else " (the two routes DISAGREE)"))
            out.append({"batch": name, "envs": n, "plans": k, "horizon": h, "evaluate_plans_us": us_verb, "fork_route_us": us_fork,
                        "routes_agree": same})
        assert sim.check_errors() == 0
        sim.close()
    print(json.dumps({"bench_plans": out, "source": build.source_fingerprint()}))


if __name__ == "__main__":
    main()
