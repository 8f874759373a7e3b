"""Time the VID evaluator on a VID-val-shaped synthetic set: the numpy path (vid_eval.do_vid_evaluation, device=None) and the device
path (device=cuda: ops.vid_eval_match, csrc/videval.hip), with one motion range and with four.

    python tools/bench_vid_eval.py [--videos 0] [--dets 300] [--cpu-frames 1000] [--repeats 3] [--warmup 1] [--fps 2476] [--out FILE]

The set: the 555 videos / 176126 frames of `bench.py --workload vidval` (data/samplers.vid_val_shaped_lengths), seeded.  Per frame 1..3
ground-truth boxes of the video's one or two classes, a motion IoU per box, and `--dets` detections in a 1000 x 600 frame: four
jittered copies of every box with detector-like scores and clutter of low score and random label in the other rows.  The annotations
are 1280 x 720, so every prediction is resized (two ratios).
What is timed
  numpy   do_vid_evaluation(device=None) on the FIRST `--cpu-frames` frames only, median of `--repeats` runs, and that time SCALED
          linearly by frames to the whole set -- the per-frame loops are linear in frames, the final sort slightly worse, so the
          scaled figure flatters the numpy path if anything.  It is a scaled figure, not a measurement of the whole set.
  device  the WHOLE set, median of `--repeats` runs after `--warmup`, in parts: pack (engine.pack_predictions + pack_groundtruth on
          the host), copy (host to device with the resize, and the results back), kernel (label range + the matching launch, to the
          device synchronise) and tail (numpy: per-class order, sort by score, cumulative sums, AP, CorLoc); their sum is the total.
On the subset both paths' result.txt texts are compared.  For scale: detecting the whole set at `--fps` frames/s (the README's rate)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("pack", "copy_in", "kernel", "copy_out", "tail")


def make_set(lengths, dets, classes, seed):
    """-> (predictions, ground truths: lists of BoxList, motion IoUs: list of lists)"""
    from diffusionvid_amd.structures.bounding_box import BoxList
    rng = np.random.RandomState(seed)
    F = int(sum(lengths))
    video = np.repeat(np.arange(len(lengths)), lengths)
    pair = rng.randint(1, classes + 1, size=(len(lengths), 2))
    g = rng.randint(1, 4, size=F)
    xy = rng.uniform(0, 900, size=(F, 3, 2)) * (1.0, 0.5)
    gt = np.concatenate((xy, xy + rng.uniform(60, 360, size=(F, 3, 2))), axis=2).astype(np.float32)
    gl = pair[video[:, None], rng.randint(0, 2, size=(F, 3))]
    motion = rng.choice([0.2, 0.5, 0.7, 0.8, 0.9, 0.95, 1.0], size=(F, 3))
    out = np.zeros((F, dets, 6), dtype=np.float32)
    step = 8192
    for a in range(0, F, step):          # in pieces: the temporaries of the whole set would not fit beside it
        b = min(F, a + step)
        n = b - a
        xy = rng.uniform(0, 640, size=(n, dets, 2)) * (1.0, 0.6)
        out[a:b, :, :4] = np.concatenate((xy, xy + rng.uniform(20, 200, size=(n, dets, 2))), axis=2)
        out[a:b, :, 4] = rng.beta(1, 12, size=(n, dets))
        out[a:b, :, 5] = rng.randint(1, classes + 1, size=(n, dets))
        for j in range(min(12, dets)):
            k = j % 3
            has = g[a:b] > k
            box = gt[a:b, k] * np.float32(1000.0 / 1280.0) + rng.uniform(-14, 14, size=(n, 4)) * (1.0 + j // 3)
            out[a:b, j, :4] = np.where(has[:, None], box, out[a:b, j, :4])
            out[a:b, j, 4] = np.where(has, np.clip(rng.normal(0.75 - 0.15 * (j // 3), 0.12, size=n), 0.02, 0.99), out[a:b, j, 4])
            out[a:b, j, 5] = np.where(has, gl[a:b, k], out[a:b, j, 5])
    t = torch.from_numpy(out)
    labels = t[:, :, 5].long()
    gt_t, gl_t = torch.from_numpy(gt), torch.from_numpy(gl.astype(np.int64))
    preds, gts = [], []
    for f in range(F):
        p = BoxList(t[f, :, :4], (1000, 600))
        p.add_field("scores", t[f, :, 4])
        p.add_field("labels", labels[f])
        q = BoxList(gt_t[f, :g[f]], (1280, 720))
        q.add_field("labels", gl_t[f, :g[f]])
        preds.append(p)
        gts.append(q)
    return preds, gts, [motion[f, :g[f]].tolist() for f in range(F)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=0, help="use only the first K videos of the set (0 = all 555)")
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--classes", type=int, default=30)
    ap.add_argument("--cpu-frames", type=int, default=1000, help="the numpy path is timed on the first K frames and scaled")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fps", type=float, default=2476.0, help="detection rate for scale (the README's headline)")
    ap.add_argument("--seed", type=int, default=2015)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vid_eval_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vid_eval needs the GPU: nothing is timed without one")
    from diffusionvid_amd.data.evaluation import vid_eval
    from diffusionvid_amd.data.samplers import vid_val_shaped_lengths
    lengths = vid_val_shaped_lengths()
    if args.videos:
        lengths = lengths[:args.videos]
    t0 = time.perf_counter()
    preds, gts, motion = make_set(lengths, args.dets, args.classes, args.seed)
    F, K = len(preds), min(args.cpu_frames, len(preds))
    lines = ["VID evaluator: %d videos, %d frames, %d detections per frame, %d classes, %d ground-truth boxes (set built in %.1f s)" % (
        len(lengths), F, args.dets, args.classes, sum(len(g) for g in gts), time.perf_counter() - t0),
        "torch %s, %s; the host parts (pack, tail, numpy) run on one thread" % (torch.__version__, torch.cuda.get_device_name(0))]
    print("\n".join(lines), flush=True)
    device = torch.device("cuda")
    whole = vid_eval.GroundTruthList(gts, motion=motion)
    part = vid_eval.GroundTruthList(gts[:K], motion=motion[:K])
    detect_s = F / args.fps
    for ms in (False, True):
        name = "four motion ranges" if ms else "one motion range"
        with tempfile.TemporaryDirectory() as tmp:
            # numpy, on the subset
            cpu = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                vid_eval.do_vid_evaluation(part, preds[:K], tmp, motion_specific=ms)
                cpu.append(time.perf_counter() - t0)
            want = open(os.path.join(tmp, "result.txt"), "rb").read()
            vid_eval.do_vid_evaluation(part, preds[:K], tmp, motion_specific=ms, device=device)
            same = want == open(os.path.join(tmp, "result.txt"), "rb").read()
        cpu_s = statistics.median(cpu)
        # device, on the whole set
        runs = []
        for i in range(args.warmup + args.repeats):
            times = {}
            vid_eval._do_vid_evaluation_device(whole, preds, None, ms, None, None, device, times=times)
            if i >= args.warmup:
                runs.append(times)
            print("  device run %d (%s): %s" % (i, name, " ".join("%s %.2f" % (k, times[k]) for k in STAGES)), flush=True)
        med = {k: statistics.median(r[k] for r in runs) for k in STAGES}
        total = statistics.median(sum(r[k] for k in STAGES) for r in runs)
        block = ["", "%s" % name,
                 "  numpy, MEASURED on the first %d frames: %.3f s (median of %d, min %.3f max %.3f)" % (K, cpu_s, len(cpu), min(cpu), max(cpu)),
                 "  numpy, SCALED by frames to %d frames (not measured): %.1f s" % (F, cpu_s * F / K),
                 "  device, measured on all %d frames, median of %d after %d warm-up: total %.2f s" % (F, len(runs), args.warmup, total),
                 "    pack %.2f s | copy %.2f s (in, with the resize %.2f + out %.2f) | kernel %.2f s | tail %.2f s" % (
                     med["pack"], med["copy_in"] + med["copy_out"], med["copy_in"], med["copy_out"], med["kernel"], med["tail"]),
                 "    spread of the total over the runs: min %.2f max %.2f s" % (min(sum(r[k] for k in STAGES) for r in runs),
                                                                               max(sum(r[k] for k in STAGES) for r in runs)),
                 "  result.txt of both paths on the first %d frames: %s" % (K, "identical" if same else "DIFFERENT"),
                 "  detecting the set at %.0f frames/s takes %.1f s: the device evaluation is %.2fx that (%s), the scaled numpy figure %.2fx" % (
                     args.fps, detect_s, total / detect_s, "target met" if total < detect_s else "target MISSED, largest part: " + max(med, key=med.get),
                     cpu_s * F / K / detect_s)]
        lines += block
        print("\n".join(block), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
