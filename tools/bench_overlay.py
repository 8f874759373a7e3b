"""Device time of ops.overlay_detections per frame, against a Pillow composition of the same frames on the host.  A record, not a gate.

    python tools/bench_overlay.py [--frames 304] [--rows 100] [--seed 0] [--seconds 1.0] [--host-frames 32] [--out profiles/overlay_bench.txt]

Workload: `--frames` frames of 1280 x 720 (uint8 RGB, on the device as the demo holds them), `--rows` detections per frame in a
1000 x 562 model frame of which about a fifth pass the 0.7 threshold, the 30 ImageNet-VID class names, Pillow's built-in bitmap font;
seeded.  Measured with device events around at least `--seconds` of work, after a warm-up pass:
  (a) the launch sequence (two kernels for all frames) per frame;
  (b) the device-to-host copy of the annotated frames into pinned memory, per frame;
  (c) the host side: ImageDraw.rectangle + ImageDraw.text per passing detection on `--host-frames` of the frames (wall clock, one
      thread), with the scores already on the host.
The pictures of (a) and (c) are not the same pixels (Pillow's outline and text placement differ); the work per detection is."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NATIVE_HW, MODEL_WH = (720, 1280), (1000, 562)


def workload(n, rows, seed):
    rng = np.random.RandomState(seed)
    mw, mh = MODEL_WH
    x1, y1 = rng.uniform(0, mw - 40, (n, rows)), rng.uniform(0, mh - 40, (n, rows))
    bw, bh = rng.uniform(20, 0.5 * mw, (n, rows)), rng.uniform(20, 0.5 * mh, (n, rows))
    score = np.where(rng.rand(n, rows) < 0.2, rng.uniform(0.7001, 1.0, (n, rows)), rng.uniform(0.05, 0.7, (n, rows)))
    dets = np.stack([x1, y1, np.minimum(x1 + bw, mw - 1), np.minimum(y1 + bh, mh - 1), score, rng.randint(1, 31, (n, rows))], axis=2).astype(np.float32)
    frames = rng.randint(0, 256, size=(n,) + NATIVE_HW + (3,), dtype=np.uint8)
    return frames, dets


def timed(fn, seconds):
    """device ms per call of fn: events around enough repetitions for `seconds` of work"""
    fn()
    torch.cuda.synchronize()
    reps, total = 1, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        total = a.elapsed_time(b)
        if total >= seconds * 1000.0:
            return total / reps, reps
        reps = max(reps * 2, int(reps * seconds * 1000.0 / max(total, 1e-3)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=304)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--host-frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_overlay needs the GPU: nothing is timed without one")
    from PIL import Image, ImageDraw
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.datasets.vid import VID_CLASSES
    from diffusionvid_amd.engine import demo
    n = args.frames
    frames_np, dets_np = workload(n, args.rows, args.seed)
    passing = float((dets_np[:, :, 4] > np.float32(0.7)).sum()) / n
    source = torch.from_numpy(frames_np).cuda()
    frames = source.clone()
    dets = torch.from_numpy(dets_np).cuda()
    counts = torch.full((n,), args.rows, dtype=torch.int32, device="cuda")
    rw, rh = NATIVE_HW[1] / MODEL_WH[0], NATIVE_HW[0] / MODEL_WH[1]
    ratios = torch.tensor([[rw, rh]] * n, dtype=torch.float64).to(torch.float32).cuda()
    names = torch.from_numpy(demo.name_table(VID_CLASSES)).cuda()
    atlas = torch.from_numpy(demo.glyph_atlas()).cuda()
    draw_ms, draw_reps = timed(lambda: ops.overlay_detections(frames, dets, counts, ratios, names, atlas), args.seconds)
    changed = float((frames != source).any(dim=3).float().mean())
    pinned = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
    copy_ms, copy_reps = timed(lambda: pinned.copy_(frames, non_blocking=True), args.seconds)
    # the host composition
    font = None
    k = min(args.host_frames, n)
    images = [Image.fromarray(frames_np[f]) for f in range(k)]
    t0 = time.perf_counter()
    for f, im in enumerate(images):
        draw = ImageDraw.Draw(im)
        d = dets_np[f]
        keep = np.nonzero(d[:, 4] > np.float32(0.7))[0]
        keep = keep[np.argsort(d[keep, 4], kind="stable")]
        for r in keep:
            x1, y1, x2, y2 = int(d[r, 0] * rw), int(d[r, 1] * rh), int(d[r, 2] * rw), int(d[r, 3] * rh)
            colour = demo.label_colour(int(d[r, 5]))
            draw.rectangle([x1, y1, x2, y2], outline=colour, width=2)
            text = "{}: {:.2f}".format(VID_CLASSES[int(d[r, 5])], float(d[r, 4]))
            box = draw.textbbox((x1 + 1, y1 + 1), text, font=font)
            draw.rectangle([x1, y1, box[2] + 1, box[3] + 1], fill=colour)
            draw.text((x1 + 1, y1 + 1), text, fill=(255, 255, 255), font=font)
    host_ms = (time.perf_counter() - t0) * 1000.0 / k
    lines = [
        "overlay bench: %d frames of %d x %d, %d rows per frame, %.1f passing 0.7 on average, seed %d" % (n, NATIVE_HW[1], NATIVE_HW[0], args.rows, passing, args.seed),
        "device: %s" % torch.cuda.get_device_name(0),
        "(a) ops.overlay_detections, all frames per call: %.4f ms per frame (%.3f ms per call, %d calls timed); %.1f %% of the pixels drawn" % (
            draw_ms / n, draw_ms, draw_reps, 100.0 * changed),
        "(b) device-to-host copy of the annotated frames (pinned): %.4f ms per frame (%.3f ms per call, %d calls timed, %.1f GB/s)" % (
            copy_ms / n, copy_ms, copy_reps, frames.numel() / copy_ms / 1e6),
        "(c) Pillow on the host (ImageDraw.rectangle + text, one thread, %d frames): %.3f ms per frame" % (k, host_ms),
        "(c) / ((a) + (b)) = %.1f" % (host_ms / ((draw_ms + copy_ms) / n)),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
