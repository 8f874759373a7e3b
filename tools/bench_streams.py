"""Several live streams on one model (DiffusionDet.open_streams) against as many private models, and the grouped memory update against
single calls.

  python tools/bench_streams.py [--streams 1,2,4,8,16] [--calls 24] [--warm 4] [--repeats 5] [--height 600 --width 1000] [--out FILE]
  python tools/bench_streams.py --only-step 8 --calls 12 --repeats 1      # one size, e.g. under rocprofv3 --kernel-trace --stats

1. Aggregate frames/s of StreamSet.step at N streams of synthetic 1000 x 600 video, against the SAME N items run one after the other through N
   private models' `model(item)` in the same process (N weight copies, N workspaces: what a user of the streaming mode runs today).
   Each repeat restarts every stream's video; the opening call (24 global frames) and `warm` steady calls are outside the timed window,
   which ends in a device synchronise.  The two sides alternate, medians over the repeats, spread = (max - min) / median.
2. ops.update_erase_memory_groups at G = 1 .. 16 for 975 -> 900 rows (the steady call's larger pruning) against G calls of
   ops.update_erase_memory, timed the same way.
Acceptance (printed): at N = 8 / G = 8 the grouped side wins by more than the larger of the two spreads."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.config import get_cfg  # noqa: E402
from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset  # noqa: E402
from diffusionvid_amd.modeling.detector import build_detection_model  # noqa: E402
from diffusionvid_amd.utils import synthetic  # noqa: E402

STREAMING = ["INPUT.INFER_BATCH", 1, "MODEL.VID.MEGA.MAX_OFFSET", 0, "MODEL.VID.MEGA.MIN_OFFSET", 0, "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 1,
             "MODEL.VID.MEGA.KEY_FRAME_LOCATION", 0, "MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST", False]


def summary(values):
    med = statistics.median(values)
    return {"median": med, "min": min(values), "max": max(values), "spread": (max(values) - min(values)) / med, "n": len(values)}


def wins(a, b, higher_is_better):
    """a beats b by more than the larger of the two spreads (absolute, in a's unit)"""
    margin = max(a["spread"] * a["median"], b["spread"] * b["median"])
    return (a["median"] - b["median"] > margin) if higher_is_better else (b["median"] - a["median"] > margin)


def build(cfg):
    model = build_detection_model(cfg).to("cuda").eval()
    model.noise_fn = synthetic.DeviceNoise()
    model.results_on_host = True
    return model


def timed(fn, first, last):
    """seconds of fn(t) for t in [first, last), from an idle device to an idle device"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(first, last):
        fn(t)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_steps(cfg, sizes, calls, warm, repeats, height, width):
    nmax = max(sizes)
    sets = []
    for s in range(nmax):
        ds = SyntheticVIDDataset([calls], cfg, height=height, width=width, device="cuda", video_base=s)
        ds.preload()
        sets.append([ds[i][0] for i in range(calls)])
    shared = build(cfg)
    privates = [build(cfg) for _ in range(nmax)]
    rows = {}
    with torch.no_grad():
        for n in sizes:
            streams = shared.open_streams()

            def grouped(t):
                out = streams.step({s: sets[s][t] for s in range(n)})
                assert len(out) == n

            def serial(t):
                for s in range(n):
                    assert len(privates[s](sets[s][t])) == 1
            rate = {"streams": [], "serial": []}
            for r in range(repeats + 1):          # repeat 0 warms every shape of both sides and is dropped
                order = [("streams", grouped), ("serial", serial)]
                for name, fn in (order if r % 2 == 0 else order[::-1]):
                    for t in range(1 + warm):          # the opening call and the first steady calls: outside the window
                        fn(t)
                    dt = timed(fn, 1 + warm, calls)
                    if r:
                        rate[name].append(n * (calls - 1 - warm) / dt)
            rows[n] = {k: summary(v) for k, v in rate.items()}
            a, b = rows[n]["streams"], rows[n]["serial"]
            print("N %2d  StreamSet.step %8.1f frames/s (spread %4.1f %%)   %d private models %8.1f frames/s (spread %4.1f %%)   x%.2f"
                  % (n, a["median"], a["spread"] * 100, n, b["median"], b["spread"] * 100, a["median"] / b["median"]), flush=True)
            for s in range(n):
                streams.close(s)
    return rows


def bench_update(groups, repeats, iters=40):
    g = torch.Generator().manual_seed(0)
    rows = {}
    for G in groups:
        mem = torch.randn(G, 900, 256, generator=g).cuda()
        new = torch.randn(G, 75, 256, generator=g).cuda()
        singles = [(new[k].contiguous(), mem[k].contiguous()) for k in range(G)]

        def grouped(_):
            ops.update_erase_memory_groups(new, mem, 900)

        def single(_):
            for nw, mm in singles:
                ops.update_erase_memory(nw, mm, 900)
        ms = {"groups": [], "singles": []}
        for r in range(repeats + 1):
            order = [("groups", grouped), ("singles", single)]
            for name, fn in (order if r % 2 == 0 else order[::-1]):
                fn(0)
                dt = timed(fn, 0, iters)
                if r:
                    ms[name].append(dt / iters * 1e3)
        rows[G] = {k: summary(v) for k, v in ms.items()}
        a, b = rows[G]["groups"], rows[G]["singles"]
        print("G %2d  update_erase_memory_groups 975 -> 900: %7.3f ms (spread %4.1f %%)   %d single calls %7.3f ms (spread %4.1f %%)   x%.2f"
              % (G, a["median"], a["spread"] * 100, G, b["median"], b["spread"] * 100, b["median"] / a["median"]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,2,4,8,16")
    ap.add_argument("--groups", default="1,2,4,8,16")
    ap.add_argument("--calls", type=int, default=24, help="calls per video and repeat (the first 1 + warm are not timed)")
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--only-step", type=int, default=0, help="time StreamSet.step at this many streams and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None, help="write the tables as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_streams.py measures on the GPU: no HIP device visible")
    if args.repeats < 1 or args.calls < args.warm + 3:
        raise SystemExit("need --repeats >= 1 and --calls >= --warm + 3")
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), ["DTYPE", args.dtype] + STREAMING, os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.freeze()
    result = {"device": "%s (%s)" % (torch.cuda.get_device_name(0), getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")), "frame": [args.height, args.width], "dtype": args.dtype, "calls": args.calls, "warm": args.warm,
              "repeats": args.repeats}
    print("# %s, %d x %d frames, DTYPE %s, %d repeats of %d timed calls per stream" % (result["device"], args.width, args.height, args.dtype, args.repeats,
                                                                                       args.calls - 1 - args.warm), flush=True)
    if args.only_step:
        n = args.only_step
        ds = [SyntheticVIDDataset([args.calls], cfg, height=args.height, width=args.width, device="cuda", video_base=s) for s in range(n)]
        items = [[d[i][0] for i in range(args.calls)] for d in ds]
        model = build(cfg)
        streams = model.open_streams()
        g = torch.Generator().manual_seed(0)
        for s in range(n):          # full memories from the start: every step is the steady call, no opening call in the trace
            streams.adopt_memory(s, [torch.randn(900, 256, generator=g), torch.randn(150, 256, generator=g)])
        with torch.no_grad():
            dt = timed(lambda t: streams.step({s: items[s][t] for s in range(n)}), 1, args.calls)
        print("N %d: %d steady steps in %.3f s (the first ones warm up)" % (n, args.calls - 1, dt))
        return
    sizes = [int(v) for v in args.streams.split(",") if v]
    result["step"] = bench_steps(cfg, sizes, args.calls, args.warm, args.repeats, args.height, args.width)
    result["update"] = bench_update([int(v) for v in args.groups.split(",") if v], args.repeats)
    if 8 in result["step"]:
        r = result["step"][8]
        result["accept_step_n8"] = wins(r["streams"], r["serial"], True)
        print("acceptance, N = 8: StreamSet.step beats 8 private models by more than the larger spread: %s" % result["accept_step_n8"])
    if 8 in result["update"]:
        r = result["update"][8]
        result["accept_update_g8"] = wins(r["groups"], r["singles"], False)
        print("acceptance, G = 8: the grouped update beats 8 single calls by more than the larger spread: %s" % result["accept_update_g8"])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
