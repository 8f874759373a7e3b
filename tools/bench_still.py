"""Images/s of DiffusionDet.detect_images on still images of mixed sizes -- configs/still_R_101_DiffusionDet_p2.yaml: R-101, p2..p5, 80
classes, 500 proposals, six heads, SAMPLE_STEP 1 -- against the same images detected one per call.

    python tools/bench_still.py [--images 32] [--dtype float16|float32] [--chunk 8] [--steps 5] [--warmup 2] [--repeat 20] [--json out.json]

Images: the synthetic frame generator (white noise, as bench.py) at four aspect ratios -- 4:3, 3:4, 16:9 and 1:1 sources -- at the size the
test transform gives them (shortest edge 800, longest at most 1333), interleaved, resident on the device as un-padded fp32 [3, h, w].
Three ways through the same 32 images, each timed between device synchronisations (host clock; results brought to the host, one copy per
launch sequence; device-side draws); a timed step is `--repeat` passes over the images, so that it lasts about a second; per step, median
and spread:
  mixed    one detect_images call: one canvas for all, the union of both orientations
  grouped  one call per orientation (data/datasets/still.py: orientation_batches): wide and tall images on canvases of their own
  single   one call per image, each on its own canvas
and the share of canvas pixels that is padding for the first two (none is timed separately: the backbone runs over the padding).
Not part of bench.py: the video benchmark's line is the project's yardstick; this one has no parent to be gated against."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOURCES_WH = [(640, 480), (480, 640), (1280, 720), (500, 500)]


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--dtype", default="float16", choices=["float16", "float32"])
    ap.add_argument("--chunk", type=int, default=0, help="images per launch sequence (0: INFER_BATCH * LOOKAHEAD_BATCHES = 8)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=20, help="passes over the images per timed step")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_still needs the GPU: nothing is timed without one")
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data import transforms
    from diffusionvid_amd.data.datasets import still
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg(os.path.join(ROOT, "configs/still_R_101_DiffusionDet_p2.yaml"), ["DTYPE", args.dtype], os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.freeze()
    model = build_detection_model(cfg).to("cuda").eval()
    model.noise_fn = synthetic.DeviceNoise()
    model.results_on_host = True
    model.still_chunk = args.chunk or None
    sizes_wh, images = [], []
    for i in range(args.images):
        oh, ow = transforms.get_size(SOURCES_WH[i % len(SOURCES_WH)], 800, 1333)
        sizes_wh.append((ow, oh))
        images.append(synthetic.synthetic_frame(i, oh, ow).cuda())
    ids = list(range(args.images))
    everything = [ids]
    groups = still.orientation_batches(sizes_wh, args.images)
    # canvases are made once, outside the timed region (a loader's collate function makes them on the host, beside the GPU's work)
    from diffusionvid_amd.structures.image_list import to_image_list
    canvases = {name: [(to_image_list([images[i] for i in b], 32), b) for b in batches]
                for name, batches in (("mixed", everything), ("grouped", groups), ("single", [[i] for i in ids]))}

    def run(name):
        def fn():
            n = 0
            with torch.no_grad():
                for _ in range(args.repeat):
                    for canvas, b in canvases[name]:
                        n += len(model.detect_images(canvas, b))
            assert n == args.images * args.repeat
        return fn

    res = dict(config="R101 p2-p5 x1 %s, 80 classes, 500 proposals, 6 heads; %d images at shortest edge 800 from %s sources, %d per launch sequence"
                      % (args.dtype, args.images, "/".join("%dx%d" % s for s in SOURCES_WH), args.chunk or model.infer_batch * model.lookahead),
               device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, passes_per_step=args.repeat,
               sizes_wh=sorted(set(sizes_wh)), canvases_hw={k: [tuple(c.tensors.shape[-2:]) for c, _ in v][:4] for k, v in canvases.items()},
               padding_share_mixed=round(still.padding_share(sizes_wh, everything), 4),
               padding_share_grouped=round(still.padding_share(sizes_wh, groups), 4),
               padding_share_single=round(still.padding_share(sizes_wh, [[i] for i in ids]), 4))
    for name in ("mixed", "grouped", "single"):
        ips = [args.images * args.repeat / t for t in timed(run(name), args.warmup, args.steps)]
        res["images_per_s_" + name] = dict(median=round(statistics.median(ips), 2), min=round(min(ips), 2), max=round(max(ips), 2))
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
