"""Times xwb_copy_envs (BatchedSimulator.copy_envs) on one GPU, in one process, for two uses:

  fork     the lower half of a batch forked into its upper half (dst == src, envs / 2 pairs)
  scatter  a 64-env template batch scattered over the whole batch with keep_rng (envs pairs, every source read envs / 64 times)

and next to each, in the same run: a plain device-to-device copy of the same number of bytes (torch `copy_` between two
preallocated uint8 tensors) and the only route without the verb, save_state + load_state of the whole batch through the host.
Device events around `calls` back-to-back calls (straight through ctypes for the verb): when the host enqueues slower than the
kernel runs the figure is the enqueue rate, so it is an upper bound of the kernel's time; the host route is a host clock
around the two synchronous calls.  Bytes per env = the state blob with frames / envs, plus the egocentric goal images -- what a
pair moves, to within the few bytes per env of the blob that are not per-env state.

    python tools/bench_copy_envs.py [--envs 32768] [--calls 50] [--blocks 3] [--host-reps 2]

Rows: xworld8 (8 x 8 colour, confs/navigation2d.json) and xworld8_ego3 (the same map, egocentric r = 3).  Needs a GPU; there is
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_copy_envs.py needs a GPU")
    from xworld_amd import build, lib
    from xworld_amd.batched import BatchedSimulator
    n = args.envs
    rows = [("xworld8", {"color": True}), ("xworld8_ego3", {"color": True, "visible_radius": 3})]
    print("copy_envs against a plain device copy of the same bytes and against save_state + load_state (device events, %d calls, best of "
          "%d blocks; host route: best of %d); source %s on %s" % (args.calls, args.blocks, args.host_reps, build.source_fingerprint(),
                                                                 torch.cuda.get_device_name(0)))
    print("| batch | envs | use | pairs | bytes per env | copy_envs us (<=) | torch copy_ us | copy_envs / copy_ | save + load ms | save + load / copy_envs |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    out = []
    for name, opts in rows:
        o = {"xwd_conf_path": CONF, "task_mode": "lang_acquisition"}
        o.update(opts)
        sim = BatchedSimulator("xworld", o, num_envs=n)
        template = BatchedSimulator("xworld", o, num_envs=64, seed=7)
        for _ in range(20):                                    # a batch in mid-rollout, every env live
            sim.step()
            sim.reset_done()
        nb = C.c_size_t()
        lib.check(sim.L.xwb_state_bytes(sim.h, 1, C.byref(nb)))
        per_env = nb.value // n + (sim.cfg.num_goals * 16384 if sim.cfg.visible_radius else 0)
        idx = torch.arange(n, dtype=torch.int32, device="cuda")
        half = n // 2
        uses = [("fork", sim, idx[half:].contiguous(), idx[:half].contiguous(), 0),
                ("scatter", template, idx, (idx % 64).contiguous(), lib.XWB_COPY_KEEP_RNG)]
        host_ms = []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sim.load_state(sim.save_state())
            host_ms.append((time.perf_counter() - t0) * 1000.0)
        for use, source, dst, src, flags in uses:
            pairs = int(dst.numel())
            call = lambda: lib.check(sim.L.xwb_copy_envs(sim.h, C.c_void_p(dst.data_ptr()), source.h, C.c_void_p(src.data_ptr()), pairs, flags, None))
            call()
            us = min(events(torch, call, args.calls) for _ in range(args.blocks))
            a = torch.empty(pairs * per_env, dtype=torch.uint8, device="cuda")
            b = torch.zeros_like(a)
            a.copy_(b)
            plain = min(events(torch, lambda: a.copy_(b), args.calls) for _ in range(args.blocks))
            del a, b
            print("| %s | %d | %s | %d | %d | %.1f | %.1f | %.2f | %.1f | %.0f |" % (name, n, use, pairs, per_env, us, plain, us / plain, min(host_ms),
                                                                                   min(host_ms) * 1000.0 / us))
            out.append({"batch": name, "envs": n, "use": use, "pairs": pairs, "bytes_per_env": per_env, "copy_envs_us": us, "torch_copy_us": plain,
                        "save_load_ms": host_ms})
        assert sim.check_errors() == 0
        sim.close()
        template.close()
    print(json.dumps({"bench_copy_envs": out, "source": build.source_fingerprint()}))


if __name__ == "__main__":
    main()
