"""Images/s of DiffusionDet.detect_images_aug (TEST.BBOX_AUG) against the composition the package allowed without it.

    python tools/bench_bbox_aug.py [--images 8] [--dtype float16|float32] [--calls 4] [--rounds 5] [--warmup 1] [--out profiles/bbox_aug_bench.txt]

Workload: configs/still_R_101_DiffusionDet_p2_aug.yaml -- R-101, p2..p5, 80 classes, 500 proposals, six heads, SAMPLE_STEP 1; six views
per image (800 / 640 / 960 on the short side, each with its mirror), 3000 candidates per image into the merging NMS -- on synthetic uint8
images of COCO-like sizes (640 x 480, 640 x 427, 500 x 375, 640 x 360; one orientation, as the orientation sampler batches them), held on
the host as a loader hands them over.  Device events around whole calls, results brought to the host in both:
  (a) detect_images_aug: the views built on the device, one launch sequence per scale group, the merge on the device
  (b) per scale group the views made with Pillow on the host and one detect_images call; the BoxLists mapped with BoxList.transpose /
      resize on the host, padded, and ops.nms_frames_tiled; the cut on the host
(a) and (b) alternate in one process, `--rounds` windows of `--calls` calls each; per window images/s, then median and spread.  Also: the
share of (a) spent building the views and merging, each timed on its own between events, and for the view kernels the bytes they move
(from the shapes) over that time.  Not part of bench.py: that line is the project's yardstick; this one has no parent to be gated against."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOURCES_WH = [(640, 480), (640, 427), (500, 375), (640, 360)]


def event_ms(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--dtype", default="float16", choices=["float16", "float32"])
    ap.add_argument("--calls", type=int, default=4, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bbox_aug needs the GPU: nothing is timed without one")
    from PIL import Image
    from diffusionvid_amd import ops
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data import transforms as T
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.structures.bounding_box import FLIP_LEFT_RIGHT, BoxList
    from diffusionvid_amd.structures.image_list import ImageList
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg(os.path.join(ROOT, "configs/still_R_101_DiffusionDet_p2_aug.yaml"),
                  ["DTYPE", args.dtype, "INPUT.MIN_SIZE_TEST", 800, "INPUT.MAX_SIZE_TEST", 1333], os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.trained_like_scores(synthetic.tame_box_deltas(model.state_dict(), 0.1)))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.DeviceNoise()
    model.results_on_host = True
    n = args.images
    images = []
    for i in range(n):
        w, h = SOURCES_WH[i % len(SOURCES_WH)]
        images.append((synthetic.synthetic_frame(i, h, w, smooth=True).permute(1, 2, 0) * 255).round().to(torch.uint8).numpy())
    ids = list(range(n))
    views = [T.bbox_aug_views(cfg, (im.shape[1], im.shape[0])) for im in images]
    V = len(views[0])
    scales = T.bbox_aug_scales(cfg)
    thr, K = float(cfg.MODEL.ROI_HEADS.NMS), int(cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG)

    def run_a():
        with torch.no_grad():
            return model.detect_images_aug(images, ids)

    def run_b():
        per_view = [[None] * V for _ in range(n)]
        with torch.no_grad():
            for g in range(len(scales)):
                mine = [[(v, view) for v, view in enumerate(vs) if view.group == g] for vs in views]
                PH = -(-max(m[0][1].h for m in mine) // 32) * 32
                PW = -(-max(m[0][1].w for m in mine) // 32) * 32
                canvas = torch.zeros(sum(len(m) for m in mine), 3, PH, PW)
                sizes, where = [], []
                for i, m in enumerate(mine):
                    resized = Image.fromarray(images[i]).resize((m[0][1].w, m[0][1].h), Image.BILINEAR)
                    for v, view in m:
                        im = resized.transpose(Image.FLIP_LEFT_RIGHT) if view.flip else resized
                        canvas[len(where), :, :view.h, :view.w] = torch.from_numpy(np.array(im)).permute(2, 0, 1).to(torch.float32).div(255)
                        sizes.append(torch.Size((view.h, view.w)))
                        where.append((i, v))
                base = g * 2 * n          # consecutive ids per call: one draw launch per kind
                out = model.detect_images(ImageList(canvas, sizes), list(range(base, base + len(where))))
                for (i, v), bl in zip(where, out):
                    per_view[i][v] = bl
            N = max(sum(len(bl) for bl in pv) for pv in per_view)
            boxes, scores = torch.zeros(n, N, 4), torch.full((n, N), torch.finfo(torch.float32).tiny)
            labels, live = torch.ones(n, N, dtype=torch.int32), []
            for i, pv in enumerate(per_view):
                mapped = [(bl.transpose(FLIP_LEFT_RIGHT) if view.flip else bl) for bl, view in zip(pv, views[i])]
                mapped = [m if v == 0 else m.resize((views[i][0].w, views[i][0].h)) for v, m in enumerate(mapped)]
                k = sum(len(m) for m in mapped)
                boxes[i, :k] = torch.cat([m.bbox for m in mapped])
                scores[i, :k] = torch.cat([m.get_field("scores") for m in mapped])
                labels[i, :k] = torch.cat([m.get_field("labels") for m in mapped]).to(torch.int32)
                live.append(k)
            sizes0 = torch.tensor([(vs[0].w, vs[0].h) for vs in views], dtype=torch.float32)
            ob, osc, ol, oc = ops.nms_frames_tiled(boxes.cuda(), scores.cuda(), labels.cuda(), sizes0, None, thr)
            ob, osc, ol, oc = ob.cpu(), osc.cpu(), ol.cpu(), oc.cpu()
            results = []
            for i in range(n):
                m = int(oc[i]) - (N - live[i])
                if 0 < K < m:
                    m = int((osc[i, :m] >= osc[i, K - 1]).sum())
                bl = BoxList(ob[i, :m], (views[i][0].w, views[i][0].h), mode="xyxy")
                bl.add_field("scores", osc[i, :m])
                bl.add_field("labels", ol[i, :m].to(torch.int64))
                results.append(bl)
            return results

    for _ in range(args.warmup):
        ra, rb = run_a(), run_b()
    rates = {"a": [], "b": []}
    for _ in range(args.rounds):
        for name, fn in (("a", run_a), ("b", run_b)):
            rates[name].append(n * args.calls / (event_ms(fn, args.calls) * args.calls / 1000.0))

    # the parts of (a) on their own: the view kernels per scale group and the merge, on buffers of the call's shapes
    srcs = ops.ImageTable([torch.from_numpy(im).cuda() for im in images])
    view_ms, view_bytes, shapes = 0.0, 0, []
    v0 = 0
    for g, (_, _, nv) in enumerate(scales):
        out_hw = [(vs[v0].h, vs[v0].w) for vs in views]
        plan = T.ViewsPlan(srcs.sizes_hw, out_hw).to("cuda")
        PH, PW = -(-plan.max_oh // 32) * 32, -(-plan.max_ow // 32) * 32
        ms = event_ms(lambda: ops.resize_views_u8(srcs, plan, PH, PW, nv == 2), 20)
        nbytes = sum(h * w * 3 + 2 * h * ow * 3 for (h, w), (oh, ow) in zip(srcs.sizes_hw, out_hw)) + n * nv * 3 * PH * PW * 4
        view_ms += ms
        view_bytes += nbytes
        shapes.append("group %d: %d x %d canvas, %d slots, %.3f ms, %.1f MB -> %.0f GB/s" % (g, PH, PW, n * nv, ms, nbytes / 1e6, nbytes / ms / 1e6))
        v0 += nv
    cap = model.num_proposals
    g = torch.Generator().manual_seed(0)
    mb = torch.rand(n * V, cap, 4, generator=g).cuda() * 500
    msc, ml = torch.rand(n * V, cap, generator=g).cuda(), torch.randint(1, 81, (n * V, cap), generator=g).to(torch.int32).cuda()
    mc = torch.full((n * V,), cap, dtype=torch.int32).cuda()
    table = ops.bbox_aug_table(views).cuda()
    sizes0 = ops.FrameSizes(torch.tensor([(vs[0].w, vs[0].h) for vs in views], dtype=torch.float32), "cuda")
    merge_ms = event_ms(lambda: ops.bbox_aug_merge(mb, msc, ml, mc, table, V), 20)
    finish_ms = event_ms(lambda: ops.bbox_aug_finish(*ops.bbox_aug_merge(mb, msc, ml, mc, table, V), sizes0, thr, K), 20) - merge_ms
    call_ms = 1000.0 * n / statistics.median(rates["a"])

    def stat(x):
        return "median %.2f, min %.2f, max %.2f (spread %.1f %%)" % (statistics.median(x), min(x), max(x), 100 * (max(x) - min(x)) / statistics.median(x))
    lines = [
        "TEST.BBOX_AUG: R101 p2-p5 x1 %s, 80 classes, 500 proposals, 6 heads; %d views per image (800, 640, 960, each mirrored), %d candidates per image"
        % (args.dtype, V, V * cap),
        "%d uint8 images per call from %s sources on the host; torch %s, %s" % (n, "/".join("%dx%d" % s for s in SOURCES_WH), torch.__version__, torch.cuda.get_device_name(0)),
        "device events around %d calls per window, %d windows of each, alternating, after %d warm-up call(s); detections on the host in both" % (args.calls, args.rounds, args.warmup),
        "",
        "  (a) detect_images_aug, images/s:                       " + stat(rates["a"]),
        "  (b) Pillow views + detect_images per group + host map, images/s: " + stat(rates["b"]),
        "  (a) / (b) by the medians: %.3f" % (statistics.median(rates["a"]) / statistics.median(rates["b"])),
        "  detections of the last warm-up call: (a) %s, (b) %s" % ([len(r) for r in ra], [len(r) for r in rb]),
        "",
        "  one call of (a) is %.1f ms; on their own, between events (20 repetitions):" % call_ms,
        "    the view kernels of the %d scale groups: %.3f ms = %.2f %% of the call" % (len(scales), view_ms, 100 * view_ms / call_ms),
    ] + ["      " + s for s in shapes] + [
        "      all groups: %.1f MB in %.3f ms = %.0f GB/s (both passes of a group together; launch gaps included)" % (view_bytes / 1e6, view_ms, view_bytes / view_ms / 1e6),
        "    the merge kernel: %.3f ms; the NMS and the cut behind it: %.3f ms; together %.2f %% of the call" % (merge_ms, finish_ms, 100 * (merge_ms + finish_ms) / call_ms),
        "  AP: not measured (no trained weights)",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
