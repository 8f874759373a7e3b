"""Time Seq-NMS (ops.seq_nms_video, csrc/seqnms.hip) on one synthetic video of the benchmark's shape: 304 frames, 300 detections per
frame, 30 classes -- and, on the same input, the plain numpy restatement the tests check it against (tests/_seq_nms_host.py).

    python tools/bench_seq_nms.py [--frames 304] [--dets 300] [--classes 30] [--repeats 20] [--warmup 3] [--fps 2400] [--json out.json]

The video: `--tracks` objects that drift across a 1000 x 600 frame for a random span of frames, each detected in every frame of its
span as one strong box and a few weaker near-duplicates, the remaining rows of a frame filled with clutter of low score; scores as a
detector's, printed as a histogram with the result because the number of rounds -- paths a class removes -- follows from them, and
the step's time is bound by rounds x frames (one sweep over the frames from the last path's root per round).
GPU time: the whole call, host clock around a device synchronise (it uploads its layout and waits, so it is a host-synchronous call),
median and spread over `--repeats` after `--warmup`.  Host time: one run.  For scale, not as a target, the video's detection time at
`--fps` frames/s (take the figure from the current `bench.py --gpus 1` line)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_video(frames, dets, classes, tracks, seed):
    rng = np.random.RandomState(seed)
    W, H = 1000.0, 600.0
    rows = [[] for _ in range(frames)]
    for _ in range(tracks):
        label = 1 + rng.randint(classes)
        f0 = rng.randint(0, max(1, frames - 8))
        f1 = min(frames, f0 + rng.randint(8, frames))
        w, h = rng.uniform(60, 300), rng.uniform(60, 300)
        x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
        vx, vy = rng.uniform(-3, 3), rng.uniform(-2, 2)
        base = rng.uniform(0.3, 0.95)
        for f in range(f0, f1):
            bx, by = np.clip(x + vx * (f - f0), 0, W - w), np.clip(y + vy * (f - f0), 0, H - h)
            s = float(np.clip(base + rng.normal(0, 0.08), 0.02, 0.99))
            rows[f].append((bx, by, bx + w, by + h, s, label))
            for _ in range(rng.randint(1, 4)):
                j = rng.uniform(-0.06, 0.06, 4) * (w, h, w, h)
                rows[f].append((bx + j[0], by + j[1], bx + w + j[2], by + h + j[3], s * rng.uniform(0.2, 0.8), label))
    out = np.zeros((frames, dets, 6), dtype=np.float32)
    for f in range(frames):
        r = rows[f][:dets]
        while len(r) < dets:
            w, h = rng.uniform(20, 200), rng.uniform(20, 200)
            x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
            r.append((x, y, x + w, y + h, float(rng.beta(1, 12)), 1 + rng.randint(classes)))
        a = np.asarray(r, dtype=np.float32)
        out[f] = np.clip(a[rng.permutation(dets)], 0, [W - 1, H - 1, W - 1, H - 1, 1, classes])
    return out, np.full((frames,), dets, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=304)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--classes", type=int, default=30)
    ap.add_argument("--tracks", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fps", type=float, default=2400.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_seq_nms needs the GPU: nothing is timed without one")
    from diffusionvid_amd import ops
    import _seq_nms_host as H
    dets, counts = make_video(args.frames, args.dets, args.classes, args.tracks, args.seed)
    hist, edges = np.histogram(dets[:, :, 4], bins=[0, 0.01, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0])
    d, c = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    for _ in range(args.warmup):
        keep, scores, status = ops.seq_nms_video(d, c, args.classes, return_status=True)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.seq_nms_video(d, c, args.classes)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    res = dict(frames=args.frames, dets=args.dets, classes=args.classes, tracks=args.tracks, repeats=args.repeats,
               score_histogram=dict(edges=[float(e) for e in edges], counts=[int(h) for h in hist]),
               rounds_per_class=status[0].tolist(), rounds_max=int(status.max()), kept=int(keep.sum()), boxes=int(counts.sum()),
               gpu_ms_median=statistics.median(times), gpu_ms_min=min(times), gpu_ms_max=max(times),
               detection_ms_at_fps=args.frames / args.fps * 1e3, fps_for_scale=args.fps)
    res["gpu_over_detection"] = res["gpu_ms_median"] / res["detection_ms_at_fps"]
    if not args.no_host:
        t0 = time.perf_counter()
        hk, hs = H.seq_nms_video(dets, counts, args.classes, progress=lambda c, r: print("host: class", c, "rounds", r, flush=True))
        res["host_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_over_gpu"] = res["host_ms"] / res["gpu_ms_median"]
        res["host_over_detection"] = res["host_ms"] / res["detection_ms_at_fps"]
        res["equals_host"] = bool(np.array_equal(hk, keep.cpu().numpy()) and np.array_equal(hs.view(np.uint32), scores.cpu().numpy().view(np.uint32)))
    print("scores:", " ".join("%g-%g:%d" % (edges[i], edges[i + 1], hist[i]) for i in range(len(hist))))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
