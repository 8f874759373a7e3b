"""Time the Swin window-attention kernels on their own: the 12x12 kernels (the 384-pretrained sizes) and, as the yardstick, the
unchanged 7x7 kernels, on Swin-B's four stage maps at the benchmark's frame size (152x256, 76x128, 38x64 and 19x32 tokens with 4, 8,
16 and 32 heads), fp16 and fp32, plain and shifted blocks.

    python tools/bench_swin_window.py [--frames 1] [--repeats 200] [--json out.json]

Each figure is the median over `--repeats` rounds of device-event times; a round times every configuration once, in turn, so a drift
of the machine falls on all of them alike.  Every configuration is launched `--warmup` times first.  Random qkv: the kernels' time does
not depend on the values.  Each token attends 144 keys where it attended 49, so about 144 / 49 = 2.9 times the 7x7 kernel's arithmetic
per token is the expectation the ratio column is read against."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = [(152, 256, 4), (76, 128, 8), (38, 64, 16), (19, 32, 32)]      # Swin-B: tokens H x W, heads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from diffusionvid_amd import ops
    if not torch.cuda.is_available():
        sys.exit("bench_swin_window needs the GPU: nothing is timed without one")
    g = torch.Generator().manual_seed(0)
    runs = []                 # (key, callable)
    for (H, W, heads) in STAGES:
        B, C = args.frames, 32 * heads
        qkv32 = torch.randn(B * H * W, 3 * C, generator=g).cuda()
        qb32 = (0.5 * torch.randn(3 * C, generator=g)).cuda()
        qkv16, qb16 = qkv32.half(), qb32.half()
        for ws in (7, 12):
            relbias = ops.swin_pack_relbias(torch.randn((2 * ws - 1) ** 2, heads, generator=g), window=ws).cuda()
            for dtype, fn, qkv, qb in (("f16", ops.swin_window_attn_f16, qkv16, qb16), ("f32", ops.swin_window_attn_f32, qkv32, qb32)):
                out = torch.empty((B * H * W, C), dtype=qkv.dtype, device="cuda")
                for shift in (0, ws // 2):
                    runs.append(((H, W, heads, dtype, ws, shift),
                                 lambda fn=fn, qkv=qkv, qb=qb, relbias=relbias, B=B, H=H, W=W, heads=heads, shift=shift, out=out, ws=ws:
                                 fn(qkv, qb, relbias, B, H, W, heads, shift, out=out, window=ws)))
    for _, run in runs:
        for _ in range(args.warmup):
            run()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in runs}
    for _ in range(args.repeats):
        marks = []
        for k, run in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            marks.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in marks:
            times[k].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"{args.frames} frame(s), median of {args.repeats} device-event times, microseconds per launch")
    print(f"{'tokens':>9} {'heads':>5} {'type':>4} {'shift':>7} {'7x7':>9} {'12x12':>9} {'ratio':>6}")
    rows = []
    for (H, W, heads) in STAGES:
        for dtype in ("f16", "f32"):
            for shifted in (False, True):
                t7 = med[(H, W, heads, dtype, 7, 3 if shifted else 0)]
                t12 = med[(H, W, heads, dtype, 12, 6 if shifted else 0)]
                print(f"{H:>4}x{W:<4} {heads:>5} {dtype:>4} {'shifted' if shifted else 'plain':>7} {t7:9.1f} {t12:9.1f} {t12 / t7:6.2f}")
                rows.append(dict(H=H, W=W, heads=heads, dtype=dtype, shifted=shifted, us_window7=t7, us_window12=t12, ratio=t12 / t7))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(frames=args.frames, repeats=args.repeats, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
