#!/usr/bin/env python
"""Split JPEG decode against Pillow on the same CPUs in the same run -- a record, not a gate.

Frames: synthetic 1280 x 720, quality 90, 4:2:0 (Pillow's default sampling), the kind bench.py's real_data_feed measurement writes.
Reports, in frames/s:
  pillow_per_cpu         PIL.Image.open(f).convert("RGB") on one thread
  entropy_1_thread       data.jpeg.entropy_decode (parse + Huffman, into a reused buffer) on one thread
  entropy_at_cap         the same in a pool of default_threads() threads (ctypes drops the GIL); and Pillow in the same pool
  upload_reconstruct     data.jpeg.reconstruct alone over already decoded coefficients, in batches
  decode_many            files in memory -> CUDA uint8 frames, end to end, in batches
  python tools/bench_jpeg_decode.py [--files 48] [--passes 4] [--batch 16] [--out profiles/jpeg_decode_bench.txt]"""
import argparse
import io
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(n):
    from PIL import Image
    rng = np.random.RandomState(0)
    out = []
    for i in range(n):
        yy, xx = np.mgrid[0:720, 0:1280]
        img = np.stack([(128 + 100 * np.sin(xx / (37.0 + i) + c) * np.cos(yy / (53.0 + 2 * i))) for c in range(3)], -1)
        img = np.clip(img + rng.randn(720, 1280, 3) * 6, 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=90)
        out.append(buf.getvalue())
    return out


def rate(fn, n_frames, passes):
    fn()          # warm-up
    best = 0.0
    for _ in range(passes):
        t = time.perf_counter()
        fn()
        best = max(best, n_frames / (time.perf_counter() - t))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=48)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from PIL import Image

    from diffusionvid_amd.data import jpeg as J
    blobs = frames(args.files)
    n = len(blobs)
    cap = J.default_threads()
    lines = ["split JPEG decode, %d synthetic 1280x720 q90 4:2:0 frames (%.0f KB each), best of %d passes; thread cap %d"
             % (n, sum(map(len, blobs)) / n / 1e3, args.passes, cap)]

    def pil(b):
        with Image.open(io.BytesIO(b)) as im:
            return np.asarray(im.convert("RGB"))

    info = J.parse(blobs[0])
    local = threading.local()

    def entropy(b):          # into one buffer per thread, as a worker writes into its slot of a ring
        if not hasattr(local, "buf"):
            local.buf = np.empty(info.coef_count, dtype=np.int16)
        return J.entropy_decode(b, out=local.buf).info.coef_count

    r_pil = rate(lambda: [pil(b) for b in blobs], n, args.passes)
    r_ent = rate(lambda: [entropy(b) for b in blobs], n, args.passes)
    lines.append("pillow_per_cpu        %8.1f frames/s" % r_pil)
    lines.append("entropy_1_thread      %8.1f frames/s   (%.2fx Pillow's whole decode)" % (r_ent, r_ent / r_pil))
    with ThreadPoolExecutor(cap) as pool:
        r_pil_cap = rate(lambda: list(pool.map(pil, blobs)), n, args.passes)
        r_ent_cap = rate(lambda: list(pool.map(entropy, blobs)), n, args.passes)
    lines.append("pillow_at_cap         %8.1f frames/s   (%d threads)" % (r_pil_cap, cap))
    lines.append("entropy_at_cap        %8.1f frames/s   (%d threads, %.2fx Pillow in the same pool)" % (r_ent_cap, cap, r_ent_cap / r_pil_cap))
    if torch.cuda.is_available():
        dev = torch.device("cuda:0")
        coefs = [J.entropy_decode(b) for b in blobs]
        batches = [coefs[i:i + args.batch] for i in range(0, n, args.batch)]

        def recon():
            for b in batches:
                J.reconstruct(b, dev)
            torch.cuda.synchronize()

        def many():
            for i in range(0, n, args.batch):
                J.decode_many(blobs[i:i + args.batch], dev)
            torch.cuda.synchronize()

        got = J.reconstruct(coefs[:1], dev)[0].cpu().numpy()
        lines.append("bits: frame 0 %s Pillow's array" % ("EQUALS" if np.array_equal(got, pil(blobs[0])) else "DIFFERS FROM"))
        r_rec = rate(recon, n, args.passes)
        r_many = rate(many, n, args.passes)
        lines.append("upload_reconstruct    %8.1f frames/s   (batches of %d: one pinned copy, one upload, two launches)" % (r_rec, args.batch))
        lines.append("decode_many           %8.1f frames/s   (batches of %d, entropy pool of %d threads; %.2fx Pillow in the same pool)"
                     % (r_many, args.batch, cap, r_many / r_pil_cap))
    else:
        lines.append("no GPU: upload_reconstruct and decode_many not measured")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
