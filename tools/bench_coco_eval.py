"""Time the COCO bbox evaluator on a COCO-val-shaped synthetic set: the numpy path (coco_eval.do_coco_evaluation, device=None) and the
device path (device=cuda: ops.coco_eval_match, csrc/cocoeval.hip).

    python tools/bench_coco_eval.py [--images 5000] [--dets 500] [--cpu-images 250] [--repeats 3] [--warmup 1] [--out FILE]
        [--accumulate {numpy,device,both}] [--accumulate-out FILE]

The set: `--images` images of 640 x 480 (val2017 has 5000), 80 categories, per image 1 .. 14 ground-truth boxes (7.5 on average; val2017
has 7.4) of one to three categories, sides 6 .. 400 pixels drawn log-uniformly so that all three area ranges are met, the annotation's
area 0.5 .. 1 of w * h, 5 % crowd boxes; and `--dets` detections (500 = NUM_PROPOSALS of configs/still_R_101_DiffusionDet_p2.yaml): three
jittered copies of every box with detector-like scores, and clutter of low score and random label in the other rows.  Seeded.
What is timed
  numpy   do_coco_evaluation(device=None) on the FIRST `--cpu-images` images only, median of `--repeats` runs, and that time SCALED
          linearly by images to the whole set -- the matching loops are linear in images, the final sorts slightly worse.  It is a scaled
          figure, not a measurement of the whole set.
  device  the WHOLE set, median of `--repeats` runs after `--warmup`, in parts: pack (pack_detections + pack_groundtruth on the host),
          copy (host to device, and the results back), kernel (the matching launch, to the device synchronise) and tail (numpy:
          accumulate_from_matches and summarize); their sum is the total.
On the subset both paths' coco_eval.txt texts are compared.
--accumulate  numpy (default): the run above.  device: the same run with the accumulation on the device as well
              (accumulate="device", csrc/evalaccum.hip): a lap `accumulate` appears and the tail is summarize alone.  both: ONLY the two
              accumulations side by side on the whole set, packed once, in one run (tools/_accumulate_bench.py): the numpy tail is the
              yardstick of the device tail, and precision, recall, the numbers and the text of the two are compared at full size.  The
              block is appended to `--accumulate-out` (profiles/eval_accumulate_bench.txt)."""
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
W, H, CLASSES = 640, 480, 80


def make_set(images, dets, seed):
    """-> (a COCO annotation dict, {image id: BoxList})"""
    from diffusionvid_amd.structures.bounding_box import BoxList
    rng = np.random.RandomState(seed)
    ann = {"images": [{"id": i + 1, "width": W, "height": H} for i in range(images)],
           "categories": [{"id": c + 1, "name": "c%d" % (c + 1)} for c in range(CLASSES)], "annotations": []}
    preds = {}
    for i in range(images):
        g = int(rng.randint(1, 15))
        cats = rng.randint(1, CLASSES + 1, size=int(rng.randint(1, 4)))
        wh = np.exp(rng.uniform(np.log(6), np.log(400), size=(g, 2)))
        xy = rng.uniform(0, 1, size=(g, 2)) * np.maximum((W, H) - wh, 1)
        gl = cats[rng.randint(0, len(cats), size=g)]
        for k in range(g):
            ann["annotations"].append({"id": len(ann["annotations"]) + 1, "image_id": i + 1, "category_id": int(gl[k]),
                                       "bbox": [float(xy[k, 0]), float(xy[k, 1]), float(wh[k, 0]), float(wh[k, 1])],
                                       "area": float(wh[k, 0] * wh[k, 1] * rng.uniform(0.5, 1.0)), "iscrowd": int(rng.rand() < 0.05)})
        out = np.zeros((dets, 6), dtype=np.float32)
        dxy = rng.uniform(0, 1, size=(dets, 2)) * (W - 40, H - 40)
        out[:, :4] = np.concatenate((dxy, dxy + np.exp(rng.uniform(np.log(6), np.log(300), size=(dets, 2)))), axis=1)
        out[:, 4] = rng.beta(1, 12, size=dets)
        out[:, 5] = rng.randint(1, CLASSES + 1, size=dets)
        for j in range(min(3 * g, dets)):
            k, tier = j % g, j // g
            box = np.concatenate((xy[k], xy[k] + wh[k])) + rng.uniform(-0.08, 0.08, size=4) * (1 + tier) * np.tile(wh[k], 2)
            out[j, :4] = box
            out[j, 4] = np.clip(rng.normal(0.75 - 0.2 * tier, 0.12), 0.02, 0.99)
            out[j, 5] = gl[k]
        t = torch.from_numpy(out)
        bl = BoxList(t[:, :4], (W, H))
        bl.add_field("scores", t[:, 4])
        bl.add_field("labels", t[:, 5].long())
        preds[i + 1] = bl
    return ann, preds


def subset(ann, preds, k):
    ids = set(im["id"] for im in ann["images"][:k])
    part = dict(ann, images=ann["images"][:k], annotations=[a for a in ann["annotations"] if a["image_id"] in ids])
    return part, {i: preds[i] for i in ids}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=500)
    ap.add_argument("--cpu-images", type=int, default=250, help="the numpy path is timed on the first K images and scaled")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2017)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_bench.txt"))
    ap.add_argument("--accumulate", choices=("numpy", "device", "both"), default="numpy")
    ap.add_argument("--accumulate-out", default=os.path.join(ROOT, "profiles", "eval_accumulate_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_coco_eval needs the GPU: nothing is timed without one")
    from diffusionvid_amd.data.evaluation import coco_eval
    t0 = time.perf_counter()
    ann, preds = make_set(args.images, args.dets, args.seed)
    N, K = args.images, min(args.cpu_images, args.images)
    lines = ["COCO evaluator: %d images, %d detections per image, %d categories, %d ground-truth boxes (set built in %.1f s)" % (
        N, args.dets, CLASSES, len(ann["annotations"]), time.perf_counter() - t0),
        "torch %s, %s; the host parts (pack, tail, numpy) run on one thread" % (torch.__version__, torch.cuda.get_device_name(0))]
    print("\n".join(lines), flush=True)
    device = torch.device("cuda")
    whole = coco_eval.CocoAnnotations(ann)
    if args.accumulate == "both":
        from _accumulate_bench import compare
        counts, dets = coco_eval.pack_detections(preds, whole.image_ids)
        packed = (dets, counts) + tuple(coco_eval.pack_groundtruth(whole))
        block = compare(coco_eval, packed, CLASSES, device, args.repeats, args.warmup, lines[0].split(" (set built")[0])
        print("\n".join(block), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.accumulate_out)), exist_ok=True)
        with open(args.accumulate_out, "a") as f:
            f.write("\n".join(lines[-1:] + block) + "\n")
        return
    mode = args.accumulate
    stages = STAGES if mode == "numpy" else STAGES[:3] + ("accumulate",) + STAGES[3:]
    part_ann, part_preds = subset(ann, preds, K)
    part = coco_eval.CocoAnnotations(part_ann)
    with tempfile.TemporaryDirectory() as tmp:
        cpu = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            coco_eval.do_coco_evaluation(part, part_preds, tmp)
            cpu.append(time.perf_counter() - t0)
        want = open(os.path.join(tmp, "coco_eval.txt"), "rb").read()
        coco_eval.do_coco_evaluation(part, part_preds, tmp, device=device, accumulate=mode)
        same = want == open(os.path.join(tmp, "coco_eval.txt"), "rb").read()
    cpu_s = statistics.median(cpu)
    runs, stats = [], None
    for i in range(args.warmup + args.repeats):
        times = {}
        stats = coco_eval.do_coco_evaluation(whole, preds, None, device=device, times=times, accumulate=mode)
        if i >= args.warmup:
            runs.append(times)
        print("  device run %d: %s" % (i, " ".join("%s %.2f" % (k, times[k]) for k in stages)), flush=True)
    med = {k: statistics.median(r[k] for r in runs) for k in stages}
    totals = [sum(r[k] for k in stages) for r in runs]
    total = statistics.median(totals)
    block = ["",
             "  numpy, MEASURED on the first %d images: %.3f s (median of %d, min %.3f max %.3f)" % (K, cpu_s, len(cpu), min(cpu), max(cpu)),
             "  numpy, SCALED by images to %d images (not measured): %.1f s" % (N, cpu_s * N / K),
             "  device, measured on all %d images, median of %d after %d warm-up: total %.2f s" % (N, len(runs), args.warmup, total),
             "    pack %.2f s | copy %.2f s (in %.2f + out %.2f) | kernel %.3f s | tail %.2f s" % (
                 med["pack"], med["copy_in"] + med["copy_out"], med["copy_in"], med["copy_out"], med["kernel"], med["tail"]) +
             (" | accumulate (device) %.3f s" % med["accumulate"] if mode == "device" else ""),
             "    spread of the total over the runs: min %.2f max %.2f s" % (min(totals), max(totals)),
             "  coco_eval.txt of both paths on the first %d images: %s" % (K, "identical" if same else "DIFFERENT"),
             "  the scaled numpy figure is %.1fx the device total; largest device part: %s" % (cpu_s * N / K / total, max(med, key=med.get)),
             "  whole set on the device: " + " ".join("%s %.3f" % kv for kv in stats.items())]
    lines += block
    print("\n".join(block), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
