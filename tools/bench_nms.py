#!/usr/bin/env python
"""The two NMS forms of csrc/postproc.hip on one group of frames: nms_frame_kernel (one workgroup per frame, up to 997 candidates)
through dvid_postproc_topk_nms and the tiled form through dvid_nms_frames_tiled, on the same candidates.  Prints device-event times per
call and per frame; run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_nms.py` for the split into sort / mask / sweep.

  python tools/bench_nms.py [--frames 304] [--shapes 3x300,7x300,4x1024]          (sets x boxes per shape)
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionvid_amd import ops  # noqa: E402


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=304)
    ap.add_argument("--shapes", default="3x300,7x300,4x1024")
    args = ap.parse_args()
    n, C, W, H = args.frames, 30, 1000.0, 600.0
    for shape in args.shapes.split(","):
        S, M = (int(v) for v in shape.split("x"))
        N = S * M
        g = torch.Generator().manual_seed(S * 1000 + M)
        # a trained detector's picture: a dozen objects per frame, the boxes clustered on them, random classes
        ctr = torch.rand(n, 12, 2, generator=g) * torch.tensor([W, H])
        which = torch.randint(0, 12, (S, n, M), generator=g)
        c = ctr[torch.arange(n)[None, :, None], which] + torch.randn(S, n, M, 2, generator=g) * 8
        wh = torch.rand(S, n, M, 2, generator=g) * 120 + 30
        boxes = torch.cat([c - wh / 2, c + wh / 2], dim=-1).cuda()
        logits = (torch.randn(S, n, M, C, generator=g) * 2 - 3).cuda()
        full = lambda: ops.postproc_topk_nms(logits, boxes, W, H)          # noqa: E731
        ob, osc, ol, oc = ops.postproc_topk_nms(logits, boxes, 1e9, 1e9, use_nms=False)          # the candidates, merged; NMS input order is free
        cb, cs, cl = ob.clone(), osc.clone(), ol.clone()
        tiled = lambda: ops.nms_frames_tiled(cb, cs, cl, W, H)          # noqa: E731
        kept = float(tiled()[3].float().mean())
        t_full, t_tiled = timeit(full), timeit(tiled)
        form = "nms_frame_kernel" if N <= 997 else "tiled"
        print(f"{S} x {M} = {N} candidates, {n} frames, kept {kept:.0f} per frame: top-k + NMS ({form}) {t_full:.3f} ms = {1e3 * t_full / n:.2f} us per frame; "
              f"tiled NMS alone {t_tiled:.3f} ms = {1e3 * t_tiled / n:.2f} us per frame; scratch {ops.postproc_scratch_bytes(S, n, M) / 2**20:.1f} MiB")


if __name__ == "__main__":
    main()
