#!/usr/bin/env python
"""What a wide class vocabulary costs, kernel group by kernel group, on one group of frames (bench.py has no class-count switch):

  head      one RCNNHead pass (dvid_rcnn_head, head-only model, float16) at 64 classes with the fused tail (csrc/headtail.hip) and with
            the layer-by-layer tail (option head_tail = 0), and at 80 / 1203 classes, where the layer-by-layer tail is the only one:
            the fused-vs-unfused difference at 64 is what a wider head_tail would win back at 80
  select    the candidate selection: dvid_postproc_topk_nms without NMS at 300 x 30 (topk_select_kernel, the yardstick) against
            dvid_topk_candidates_stream (topk_stream_kernel) at 300 x 30, 300 x 80 and 300 x 1203
  rowmax    dvid_select_topk_features and dvid_ddim_renew_step at 30 classes (one thread per box row) and at 80 / 1203 (one wave per row)

Device-event times per call.  python tools/bench_class_vocab.py [--frames 304] [--head-frames 38]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.utils import synthetic  # noqa: E402


def timeit(fn, iters=10):
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


def head(n, M=300, H=608, W=1024):
    g = torch.Generator().manual_seed(1)
    feats = [ops.nhwc_from_nchw((torch.randn(n, 256, H >> s, W >> s, generator=g) * 0.5).cuda()) for s in (3, 4, 5)]
    xy = torch.rand(n, M, 2, generator=g) * torch.tensor([W - 220.0, H - 220.0])
    boxes = torch.cat([xy, xy + 20.0 + torch.rand(n, M, 2, generator=g) * 200.0], dim=-1).cuda()
    pro = torch.randn(n * M, 256, generator=g).cuda()
    t = torch.full((n,), 499, dtype=torch.long)
    for C, fused in ((64, 1), (64, 0), (80, 1), (1203, 1)):
        sd = synthetic.make_head_state_dict(0, num_classes=C)
        model = ops.Model(sd, res_blocks=(0, 0, 0, 0), num_classes=C)
        model.reserve(n, H, W, M)
        ops.set_option("head_tail", fused)
        try:
            ms = timeit(lambda: model.rcnn_head(1, feats, H, W, boxes, pro, t))
        finally:
            ops.reset_options()
        tail = "fused tail" if fused and C <= 64 else "layer-by-layer tail"
        print(f"head pass, {n} frames x {M} boxes, {C} classes, {tail}: {ms:.3f} ms = {1e3 * ms / n:.1f} us per frame")
        model.close()


def select(n, M=300):
    g = torch.Generator().manual_seed(2)
    boxes = (torch.rand(n, M, 4, generator=g) * 500).cuda()
    for C in (30, 80, 1203):
        logits = (torch.randn(n, M, C, generator=g) * 2 - 3).cuda()
        if C == 30:
            ms = timeit(lambda: ops.postproc_topk_nms(logits, boxes, 1e9, 1e9, use_nms=False))
            print(f"select {M} x {C}, {n} frames: topk_select_kernel + merge without NMS (dvid_postproc_topk_nms) {ms:.3f} ms")
        ms = timeit(lambda: ops.topk_candidates_stream(logits, boxes))
        print(f"select {M} x {C}, {n} frames: topk_stream_kernel {ms:.3f} ms = {1e3 * ms / n:.2f} us per frame, "
              f"{n * M * C * 4 / ms / 1e6:.0f} GB/s of logits per pass")


def rowmax(n, M=300, d=256):
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(n * M, d, generator=g).cuda()
    b4 = [torch.randn(n, M, 4, generator=g).cuda() for _ in range(4)]
    for C in (30, 80, 1203):
        logits = (torch.randn(n, M, C, generator=g) * 2 - 3).cuda()
        t1 = timeit(lambda: ops.select_topk_features(logits, feats, 75, 25))
        t2 = timeit(lambda: ops.ddim_renew_step(logits, b4[0].abs() * 100, b4[1], b4[2], b4[3], (1000.0, 600.0), 2.0, 2.6, 2.4, 0.7, 0.25, 0.66))
        print(f"row maximum {M} x {C}, {n} frames ({'one wave' if C > 64 else 'one thread'} per row): select_topk_features {t1:.3f} ms, "
              f"ddim_renew_step {t2:.3f} ms; logits {n * M * C * 4 / 1e6:.0f} MB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=304)
    ap.add_argument("--head-frames", type=int, default=38, help="frames per head launch (the detector's sub-batches; 304 x 300 x 1203 logits alone are 0.44 GB)")
    args = ap.parse_args()
    head(args.head_frames)
    select(args.frames)
    rowmax(args.frames)


if __name__ == "__main__":
    main()
