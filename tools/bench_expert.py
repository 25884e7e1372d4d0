"""Times the shortest-path expert (BatchedSimulator.expert, xwb_xw_expert) on one GPU, in one process:

  (a) device events around `calls` back-to-back xwb_xw_expert calls (straight through ctypes into preallocated tensors), with and
      without the distance field: an UPPER BOUND of the kernel's time -- when the host enqueues slower than the kernel runs, the
      figure is the enqueue rate.  Beside it the step kernel's event average from the library's profile hooks (an event pair
      around every launch: xwb_profile_begin / _end, kernel "step") over the loop of (b).  Kernel durations proper come from a
      trace:  rocprofv3 --kernel-trace --stats -- python tools/bench_expert.py --steps 100 --calls 50 --blocks 1
  (b) env-steps/s of the loop  expert -> step(actions) -> reset_done  against the same loop fed from a pre-drawn ring of action
      tensors (path "lazy" on both sides), the two alternating in blocks, and their ratio.

    python tools/bench_expert.py [--envs 32768] [--steps 400] [--warmup 50] [--calls 200] [--blocks 3]

Rows: the C4 shape (7 x 7, confs/navigation2d.json) and xworld7_ego3.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONF = os.path.join(ROOT, "xworld_amd", "confs", "navigation2d.json")


def events(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls                  # us per call


def loop(torch, sim, steps, ring):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        acts = ring[t % len(ring)] if ring is not None else sim.expert()[0]
        sim.step(acts)
        sim.reset_done()
    torch.cuda.synchronize()
    return sim.num_envs * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_expert.py needs a GPU")
    from xworld_amd import build
    from xworld_amd.batched import BatchedSimulator
    rows = [("C4 7x7", {"max_dim": 7, "num_blocks": 16, "color": True}), ("xworld7_ego3", {"max_dim": 7, "num_blocks": 16, "visible_radius": 3})]
    print("expert launch (device events, %d calls) and expert-driven loop vs pre-drawn actions (%d steps after %d, best of %d blocks); "
          "source %s on %s" % (args.calls, args.steps, args.warmup, args.blocks, build.source_fingerprint(), torch.cuda.get_device_name(0)))
    print("| batch | envs | expert us (<=) | expert + field us (<=) | step kernel us | loop expert steps/s | loop ring steps/s | expert / ring |")
    print("|---|---|---|---|---|---|---|---|")
    out = []
    for name, opts in rows:
        o = {"xwd_conf_path": CONF, "task_mode": "lang_acquisition"}
        o.update(opts)
        sim = BatchedSimulator("xworld", o, num_envs=args.envs)
        na = 6 if opts.get("visible_radius") else 4
        ring = [torch.randint(0, na, (args.envs,), dtype=torch.int32, device="cuda") for _ in range(16)]
        loop(torch, sim, args.warmup, None)
        loop(torch, sim, args.warmup, ring)
        acts, dist, field = sim.expert(field=True)
        pa, pd, pf = (C.c_void_p(x.data_ptr()) for x in (acts, dist, field))
        e_plain = min(events(torch, lambda: sim.L.xwb_xw_expert(sim.h, pa, pd, None, 0, None), args.calls) for _ in range(args.blocks))
        e_field = min(events(torch, lambda: sim.L.xwb_xw_expert(sim.h, pa, pd, pf, 0, None), args.calls) for _ in range(args.blocks))
        le, lr = [], []
        for _ in range(args.blocks):
            le.append(loop(torch, sim, args.steps, None))
            lr.append(loop(torch, sim, args.steps, ring))
        sim.L.xwb_profile_begin(sim.h)
        loop(torch, sim, 100, None)
        us, launches = C.c_double(), C.c_int64()
        sim.L.xwb_profile_end(sim.h, None, b"step", C.byref(us), C.byref(launches))
        sim.L.xwb_profile_stop(sim.h)
        path = sim.step_path()["path"]
        assert sim.check_errors() == 0
        sim.close()
        print("| %s | %d | %.1f | %.1f | %.1f | %.3g | %.3g | %.2f |" % (name, args.envs, e_plain, e_field, us.value, max(le), max(lr), max(le) / max(lr)))
        out.append({"batch": name, "envs": args.envs, "expert_us": e_plain, "expert_field_us": e_field, "step_kernel_us": us.value,
                    "loop_expert_sps": le, "loop_ring_sps": lr, "ratio": max(le) / max(lr), "path": path})
    print(json.dumps({"bench_expert": out, "source": build.source_fingerprint()}))


if __name__ == "__main__":
    main()
