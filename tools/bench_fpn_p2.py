"""Frames/s of the four-level pyramid (MODEL.ROI_HEADS.IN_FEATURES [p2, p3, p4, p5]) on the benchmark's workload -- DiffusionVID R-101,
SAMPLE_STEP 1, one 304-frame video of 1000 x 600 frames padded to 1024 x 608 -- and what the stride-4 level costs in it.

    python tools/bench_fpn_p2.py [--dtype float16|float32] [--levels 4|3] [--frames 304] [--lookahead 38] [--steps 3] [--warmup 2]
                                 [--no-profile] [--csv table.csv] [--json out.json]

Timing: bench.py's loop (engine.lookahead_items over a resident synthetic video, device-side noise, one result copy per group), host
clock between device synchronisations, per step, median and spread.  There is no three-level parent of this configuration to gate
against; `--levels 3` runs the shipped three-level model through the same loop for scale.
Share: one more pass with the library's per-launch events on and sub-batch chains off (dvid_profile_dump, as bench.py's roofline pass),
from whose table come the times of lateral2 (the 1x1 on the stride-4 map: N 256, K 256, M = a launch's frames x H/4 x W/4), output2 (the
3x3 on that map: K 2304) and the RoI gather (the roialign and dynconv_roi launches, whole:
a launch does not split by level)."""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P2_OPTS = ["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"], "MODEL.FPN.IN_FEATURES", ["res2", "res3", "res4", "res5"]]


def run_video(model, ds):
    from diffusionvid_amd.engine import inference as engine
    results = {}
    for idx, (images, _, ids) in engine.lookahead_items(ds, range(len(ds)), model.infer_batch, model.lookahead):
        out = model(images)
        if out:
            results.update({i: o for i, o in zip(ids, out)})
    return results


def level2_table(path, launch_frames, h, w):
    """-> {group: ms} from the per-launch table: lateral2, output2, gather, everything.  launch_frames: the frame counts of the backbone's
    launch sequences (chains off: one launch per layer and sequence) -- a stride-4 layer of n frames has M = n H/4 W/4 rows, which a
    deeper layer reaches only with 4 or 16 times the frames"""
    px4 = (h // 4) * (w // 4)
    rows4 = {n * px4 for n in launch_frames}
    out = {"lateral2": 0.0, "output2": 0.0, "gather": 0.0, "all": 0.0}
    with open(path) as f:
        for r in csv.DictReader(f):
            ms, M, N, K = float(r["ms"]), int(r["M"]), int(r["N"]), int(r["K"])
            out["all"] += ms
            if r["kernel"].startswith(("roialign", "dynconv_roi")):
                out["gather"] += ms
            elif M in rows4 and N == 256 and K == 256:          # (res2's own 1x1 layers have K 64 or N 64)
                out["lateral2"] += ms
            elif M in rows4 and N == 256 and K == 2304:         # (res2's 3x3 has K 576)
                out["output2"] += ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="float16", choices=["float16", "float32"])
    ap.add_argument("--levels", type=int, default=4, choices=[3, 4])
    ap.add_argument("--frames", type=int, default=304)
    ap.add_argument("--lookahead", type=int, default=38)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--csv", default=None, help="keep the per-launch table here")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fpn_p2 needs the GPU: nothing is timed without one")
    from diffusionvid_amd import _lib
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    H, W = 600, 1000
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"),
                  ["DTYPE", args.dtype, "INPUT.LOOKAHEAD_BATCHES", args.lookahead] + (P2_OPTS if args.levels == 4 else []),
                  os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.freeze()
    model = build_detection_model(cfg).to("cuda").eval()
    model.noise_fn = synthetic.DeviceNoise()
    model.results_on_host = True
    ds = SyntheticVIDDataset([args.frames], cfg, height=H, width=W, device="cuda", emit_ref_ahead=False)
    times = []
    with torch.no_grad():
        for _ in range(args.warmup):
            run_video(model, ds)
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = len(run_video(model, ds))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            assert n == args.frames
    fps = [args.frames / t for t in times]
    res = dict(config="R101 x1 %s, %s, %d frames of %dx%d, lookahead %d" % (args.dtype, "p2-p5" if args.levels == 4 else "p3-p5", args.frames, W, H, args.lookahead),
               device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, frames_per_s_median=round(statistics.median(fps), 1),
               frames_per_s_min=round(min(fps), 1), frames_per_s_max=round(max(fps), 1))
    if not args.no_profile:
        lib = _lib.load()
        eng = model._get_engine()
        eng.set_chains(1)
        graphs, model.use_call_graph = model.use_call_graph, False          # per-launch events need kernel-by-kernel launches
        with torch.no_grad():
            run_video(model, ds)          # un-instrumented: the tile tuner sees the chains = 1 shapes first
            torch.cuda.synchronize()
            lib.dvid_profile_enable(1)
            for _ in range(2):          # the second pass is kept (bench.py: the first launch of the first pass is not steady)
                lib.dvid_profile_reset()
                run_video(model, ds)
                torch.cuda.synchronize()
        model.use_call_graph = graphs
        path = args.csv
        if not path:
            fd, path = tempfile.mkstemp(suffix=".csv")
            os.close(fd)
        try:
            _lib.check(lib.dvid_profile_dump(path.encode()), "dvid_profile_dump")
            group = cfg.INPUT.INFER_BATCH * args.lookahead
            launches = {min(group, args.frames - a) for a in range(0, args.frames, group)} | {int(cfg.MODEL.VID.MEGA.GLOBAL.SIZE)}
            t = level2_table(path, launches, 608, 1024)
        finally:
            if not args.csv:
                os.unlink(path)
        lib.dvid_profile_enable(0)
        lib.dvid_profile_reset()
        res["recorded_kernel_ms_per_step"] = round(t["all"], 2)
        for k in ("lateral2", "output2", "gather"):
            res[k + "_ms"] = round(t[k], 3)
            res[k + "_share"] = round(t[k] / t["all"], 4) if t["all"] else None
        res["what"] = "shares of the recorded kernel time of one step, chains off; gather = roialign + dynconv_roi launches over all levels"
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
