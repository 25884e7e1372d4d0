"""Times the symbolic observation (BatchedSimulator.symbolic, xwb_xw_symbolic) on one GPU, in one process:

  (a) device events around `calls` back-to-back xwb_xw_symbolic calls (straight through ctypes into a preallocated tensor): an
      UPPER BOUND of the kernel's time -- when the host enqueues slower than the kernel runs, the figure is the enqueue rate.
      Beside it the frame render's event average from the library's profile hooks (xwb_profile_begin / _end, kernel "render":
      one event pair around the render of every step) over the loop of (b).  On the egocentric span path that pair spans
      xw_ego_cells_kernel -- the same shadows for the same envs, plus the pixel table entries -- AND the kernels behind it
      (misses, gather): an upper bound of the cells kernel, which the hooks do not time alone.  Kernel against kernel comes from
      a trace:  rocprofv3 --kernel-trace --stats -- python tools/bench_symbolic.py --steps 100 --calls 50 --blocks 1
  (b) env-steps/s of the workload's loop  step -> reset_done  with and without a symbolic() per step, the two alternating in
      blocks, and their ratio.

    python tools/bench_symbolic.py [--envs 32768] [--steps 400] [--warmup 50] [--calls 200] [--blocks 3]

Rows: xworld7 (the C4 shape, 7 x 7, confs/navigation2d.json), xworld7_ego3, xworld8_ego5, xworld7_ego7.  Needs a GPU; there is
no fallback."""
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


def loop(torch, sim, steps, look):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        sim.step()
        if look:
            sim.symbolic()
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
        sys.exit("bench_symbolic.py needs a GPU")
    from xworld_amd import build
    from xworld_amd.batched import BatchedSimulator
    rows = [("xworld7", {"max_dim": 7, "num_blocks": 16, "color": True}),
            ("xworld7_ego3", {"max_dim": 7, "num_blocks": 16, "visible_radius": 3}),
            ("xworld8_ego5", {"max_dim": 8, "visible_radius": 5}),
            ("xworld7_ego7", {"max_dim": 7, "num_blocks": 16, "visible_radius": 7})]
    print("symbolic launch (device events, %d calls) and the step loop with / without a symbolic() per step (%d steps after %d, best of "
          "%d blocks); source %s on %s" % (args.calls, args.steps, args.warmup, args.blocks, build.source_fingerprint(), torch.cuda.get_device_name(0)))
    print("| batch | envs | bytes per env | symbolic us (<=) | frame render us (events) | loop steps/s | loop + symbolic steps/s | with / without | path |")
    print("|---|---|---|---|---|---|---|---|---|")
    out = []
    for name, opts in rows:
        o = {"xwd_conf_path": CONF, "task_mode": "lang_acquisition"}
        o.update(opts)
        sim = BatchedSimulator("xworld", o, num_envs=args.envs)
        loop(torch, sim, args.warmup, False)
        loop(torch, sim, args.warmup, True)
        buf = sim.symbolic()
        ptr, nbytes = C.c_void_p(buf.data_ptr()), buf.numel() * 2
        e_sym = min(events(torch, lambda: sim.L.xwb_xw_symbolic(sim.h, ptr, nbytes, None), args.calls) for _ in range(args.blocks))
        plain, look = [], []
        for _ in range(args.blocks):
            plain.append(loop(torch, sim, args.steps, False))
            look.append(loop(torch, sim, args.steps, True))
        sim.L.xwb_profile_begin(sim.h)
        loop(torch, sim, 100, False)
        us, launches = C.c_double(), C.c_int64()
        sim.L.xwb_profile_end(sim.h, None, b"render", C.byref(us), C.byref(launches))
        sim.L.xwb_profile_stop(sim.h)
        path = sim.step_path()["path"]
        assert sim.check_errors() == 0
        sim.close()
        per_env = nbytes // args.envs
        print("| %s | %d | %d | %.1f | %.1f | %.3g | %.3g | %.3f | %s |" % (name, args.envs, per_env, e_sym, us.value, max(plain), max(look),
                                                                        max(look) / max(plain), path))
        out.append({"batch": name, "envs": args.envs, "bytes_per_env": per_env, "symbolic_us": e_sym, "render_us": us.value,
                    "loop_sps": plain, "loop_symbolic_sps": look, "ratio": max(look) / max(plain), "path": path})
    print(json.dumps({"bench_symbolic": out, "source": build.source_fingerprint()}))


if __name__ == "__main__":
    main()
