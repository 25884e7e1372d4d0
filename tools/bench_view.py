"""Times BatchedSimulator.render_view (xwb_xw_render_view) of ALL envs of a batch against a memset of the same bytes in the same
process -- the anchor this project uses for its store streams (docs/measurements.md).

    python tools/bench_view.py [--envs-full 1024] [--envs-ego 4096] [--calls 100] [--warmup 10]

Rows: xworld7 and xworld8 under full observation, egocentric r = 3, 5, 7 on the 7 x 7 map.  Each row: device events around
`calls` back-to-back calls after `warmup` calls, for the view and for tensor.zero_() of the same buffer, the two alternating
in blocks so that a drift of the clocks hits both.  Prints bytes per call, microseconds per call, TB/s and view / memset
(the ratio of rates: 1.00 = the view stores as fast as a memset).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONF = os.path.join(ROOT, "xworld_amd", "confs", "nav_target.json")


def timed(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls                  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs-full", type=int, default=1024)
    ap.add_argument("--envs-ego", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3, help="alternating timing blocks per row; the best of each side is reported")
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be >= 50")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_view.py needs a GPU")
    from xworld_amd import build
    from xworld_amd.batched import BatchedSimulator
    rows = [("xworld7 full", {"max_dim": 7, "num_blocks": 16}, args.envs_full), ("xworld8 full", {}, args.envs_full)]
    rows += [("ego r=%d (7x7)" % r, {"max_dim": 7, "num_blocks": 16, "visible_radius": r}, args.envs_ego) for r in (3, 5, 7)]
    print("render_view of all envs vs zero_() of the same bytes; %d calls per block after %d warm-up calls, best of %d blocks; source %s on %s"
          % (args.calls, args.warmup, args.blocks, build.source_fingerprint(), torch.cuda.get_device_name(0)))
    print("| batch | envs | bytes per call | view us | view TB/s | memset us | memset TB/s | view / memset |")
    print("|---|---|---|---|---|---|---|---|")
    out = []
    for name, opts, n in rows:
        o = {"xwd_conf_path": CONF, "task_mode": "lang_acquisition"}
        o.update(opts)
        sim = BatchedSimulator("xworld", o, num_envs=n)
        for _ in range(5):                                       # a state some steps into the episodes
            sim.step()
            sim.reset_done()
        h, w, c = sim.view_dims
        buf = torch.empty((n, h, w, c), dtype=torch.uint8, device="cuda")
        nbytes = buf.numel()
        view = lambda: sim.render_view(out=buf)
        zero = lambda: buf.zero_()
        for _ in range(args.warmup):
            view()
            zero()
        tv, tz = [], []
        for _ in range(args.blocks):
            tv.append(timed(torch, view, args.calls))
            tz.append(timed(torch, zero, args.calls))
        v, z = min(tv), min(tz)
        assert sim.check_errors() == 0
        sim.close()
        print("| %s | %d | %d | %.1f | %.2f | %.1f | %.2f | %.2f |" % (name, n, nbytes, v, nbytes / v / 1e6, z, nbytes / z / 1e6, z / v))
        out.append({"batch": name, "envs": n, "bytes": nbytes, "view_us": v, "memset_us": z, "ratio": z / v, "view_us_blocks": tv, "memset_us_blocks": tz})
        del buf
    print(json.dumps({"bench_view": out, "source": build.source_fingerprint()}))


if __name__ == "__main__":
    main()
