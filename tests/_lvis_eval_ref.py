"""What the LVIS evaluator's tests share: a second restatement of the federated protocol that works dict by dict and list by list, as
the rules read (plain Python loops, Python floats, sets of labels; none of lvis_eval.py's code and none of its packed arrays), the
hand-worked known-answer cases with their answers, and a generator of random ones.  `Case.packed()` lays a case out as
lvis_eval.pack_groundtruth and engine.pack_predictions would, for the code under test; `matches` lays the restatement's answers out as
ops.lvis_eval_match returns them."""
import bisect

import numpy as np

IOU_THRS = [float(v) for v in np.linspace(.5, .95, 10)]
REC_THRS = [float(v) for v in np.linspace(0, 1, 101)]
AREA_RANGES = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))
MAX_DETS = 300
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf", "AR@300", "ARs@300", "ARm@300", "ARl@300")


def image(rows=(), boxes=(), neg=(), nex=()):
    """rows: [[x1, y1, x2, y2, score, label], ...] (held as float32, as the detector emits them); boxes: [(bbox xywh, area | None, ignore,
    label), ...], area None is w * h; neg, nex: labels"""
    rows = [[float(np.float32(v)) for v in r] for r in rows]
    boxes = [{"bbox": [float(v) for v in b], "area": float(b[2]) * float(b[3]) if area is None else float(area), "ignore": int(ig),
              "label": int(l)} for b, area, ig, l in boxes]
    return {"rows": rows, "boxes": boxes, "neg": [int(l) for l in neg], "nex": [int(l) for l in nex]}


class Case:
    """images: a list of image(...) dicts; frequency: {label: "r" / "c" / "f"} (default: all "f")"""

    def __init__(self, images, num_classes, frequency=None, cap=None):
        self.images, self.num_classes = list(images), int(num_classes)
        self.frequency = {l: "f" for l in range(1, num_classes + 1)} if frequency is None else dict(frequency)
        self.cap = max(1, max((len(im["rows"]) for im in self.images), default=1)) if cap is None else cap

    def packed(self):
        """-> (dets [N, cap, 6] float32, counts [N] int32, gt_boxes [G, 4] float64, gt_areas, gt_ignore uint8, gt_labels int32, gt_starts
        [N + 1] int32, neg_starts, neg_labels, nex_starts, nex_labels int32, frequency [K + 1] str)"""
        N = len(self.images)
        dets, counts = np.zeros((N, self.cap, 6), dtype=np.float32), np.zeros(N, dtype=np.int32)
        boxes, areas, ig, labels, starts, neg, neg_starts, nex, nex_starts = [], [], [], [], [0], [], [0], [], [0]
        for f, im in enumerate(self.images):
            if im["rows"]:
                dets[f, :len(im["rows"])] = np.asarray(im["rows"], dtype=np.float32)
            counts[f] = len(im["rows"])
            for b in im["boxes"]:
                boxes.append(b["bbox"]), areas.append(b["area"]), ig.append(b["ignore"]), labels.append(b["label"])
            starts.append(len(boxes))
            neg += im["neg"]
            nex += im["nex"]
            neg_starts.append(len(neg)), nex_starts.append(len(nex))
        i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1)          # noqa: E731
        return (dets, counts, np.asarray(boxes, dtype=np.float64).reshape(-1, 4), np.asarray(areas, dtype=np.float64).reshape(-1),
                np.asarray(ig, dtype=np.uint8).reshape(-1), i32(labels), i32(starts), i32(neg_starts), i32(neg), i32(nex_starts), i32(nex),
                np.array([""] + [self.frequency[l] for l in range(1, self.num_classes + 1)]))


# ---- the protocol, rule by rule --------------------------------------------------------------------------------------------------------
def compute_iou(d, g):
    """d, g: [x, y, w, h] Python floats; no crowd case"""
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] + g[2] * g[3]
    u = u - i
    return i / u


def label_of(row, num_classes):
    """a row's label, or None when it names none of 0 .. num_classes (such a row is no detection and takes no place among the 300)"""
    return int(row[5]) if 0 <= row[5] <= num_classes else None


def kept_rows(im, num_classes):
    """Per image, before anything else: the 300 rows of highest score across all categories (stable), and of those the rows whose
    category is in the image's positive or negative set -> row numbers in descending score"""
    rows = [r for r in range(len(im["rows"])) if label_of(im["rows"][r], num_classes) is not None]
    rows.sort(key=lambda r: -im["rows"][r][4])          # Python's sort is stable, and -0.0 == 0.0
    rows = rows[:MAX_DETS]
    positive = set(b["label"] for b in im["boxes"])
    return [r for r in rows if label_of(im["rows"][r], num_classes) in positive or label_of(im["rows"][r], num_classes) in set(im["neg"])]


def evaluate_img(im, kept, label, area_rng, num_classes):
    """-> None when the (image, label) pair has neither a kept row nor a box, else a dict: rows (the image's row numbers in order), scores,
    dtm[t][d] (True: matched), dt_ig[t][d], gt_ig[g] in annotation order"""
    rows = [r for r in kept if label_of(im["rows"][r], num_classes) == label]
    gts = [k for k, b in enumerate(im["boxes"]) if b["label"] == label]
    if not rows and not gts:
        return None
    lo, hi = area_rng
    ig_of = {k: bool(im["boxes"][k]["ignore"]) or im["boxes"][k]["area"] < lo or im["boxes"][k]["area"] > hi for k in gts}
    order = [k for k in gts if not ig_of[k]] + [k for k in gts if ig_of[k]]
    boxes = []
    for r in rows:
        x1, y1, x2, y2 = im["rows"][r][:4]
        boxes.append([x1, y1, x2 - x1, y2 - y1])
    not_exhaustive = label in set(im["nex"])
    dtm = [[False] * len(rows) for _ in IOU_THRS]
    dt_ig = [[False] * len(rows) for _ in IOU_THRS]
    for ti, t in enumerate(IOU_THRS):
        taken = set()
        for di, d in enumerate(boxes):
            best = min(t, 1 - 1e-10)
            m = -1
            for k in order:
                if k in taken:
                    continue
                if m >= 0 and not ig_of[m] and ig_of[k]:
                    break
                iou = compute_iou(d, im["boxes"][k]["bbox"])
                if iou < best:
                    continue
                best = iou
                m = k
            if m >= 0:
                dtm[ti][di] = True
                taken.add(m)
                dt_ig[ti][di] = ig_of[m]
            else:
                area = d[2] * d[3]
                dt_ig[ti][di] = area < lo or area > hi or not_exhaustive
    return {"rows": rows, "scores": [im["rows"][r][4] for r in rows], "dtm": dtm, "dt_ig": dt_ig, "gt_ig": [ig_of[k] for k in gts]}


def accumulate(case):
    """-> precision [10, 101, K, 4], recall [10, K, 4]; category k is label k + 1"""
    T, R, K, A = len(IOU_THRS), len(REC_THRS), case.num_classes, len(AREA_RANGES)
    precision, recall = -np.ones((T, R, K, A)), -np.ones((T, K, A))
    kept = [kept_rows(im, K) for im in case.images]
    for k in range(K):
        for a, rng in enumerate(AREA_RANGES):
            per_image = [evaluate_img(im, kept[f], k + 1, rng, K) for f, im in enumerate(case.images)]
            per_image = [e for e in per_image if e is not None]
            scores, cols, num_gt = [], [], 0
            for e in per_image:
                for di in range(len(e["rows"])):
                    scores.append(e["scores"][di])
                    cols.append((e, di))
                num_gt += sum(1 for ig in e["gt_ig"] if not ig)
            if num_gt == 0:
                continue
            order = sorted(range(len(scores)), key=lambda i: -scores[i])
            for ti in range(T):
                tp, fp, tps, fps = 0.0, 0.0, [], []
                for i in order:
                    e, di = cols[i]
                    if not e["dt_ig"][ti][di]:
                        if e["dtm"][ti][di]:
                            tp += 1.0
                        else:
                            fp += 1.0
                    tps.append(tp)
                    fps.append(fp)
                nd = len(tps)
                rc = [tps[i] / num_gt for i in range(nd)]
                pr = [tps[i] / (tps[i] + fps[i] + float(np.spacing(1))) for i in range(nd)]
                recall[ti, k, a] = rc[-1] if nd else 0
                for i in range(nd - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                for ri, r in enumerate(REC_THRS):
                    pi = bisect.bisect_left(rc, r)
                    precision[ti, ri, k, a] = pr[pi] if pi < nd else 0.0
    return precision, recall


def _mean(values):
    values = [float(v) for v in np.asarray(values).reshape(-1) if v > -1]
    return float(np.mean(values)) if values else -1.0


def summarize(precision, recall, case):
    """the thirteen numbers, in STAT_NAMES' order"""
    t50, t75 = IOU_THRS.index(.5), IOU_THRS.index(.75)
    out = [_mean(precision[:, :, :, 0]), _mean(precision[t50, :, :, 0]), _mean(precision[t75, :, :, 0])]
    out += [_mean(precision[:, :, :, a]) for a in (1, 2, 3)]
    for fr in ("r", "c", "f"):
        cats = [l - 1 for l in range(1, case.num_classes + 1) if case.frequency[l] == fr]
        out.append(_mean(precision[:, :, cats, 0]))
    out += [_mean(recall[:, :, a]) for a in (0, 1, 2, 3)]
    return np.array(out)


def evaluate(case):
    precision, recall = accumulate(case)
    return {"precision": precision, "recall": recall, "stats": summarize(precision, recall, case)}


def matches(case):
    """evaluate_img's answers at every row's own place -> (match [4, 10, N, cap] int8, ignore [4, 10, N, cap] int8, rank [N, cap] int32,
    npig [4, num_classes + 1] int32): the arrays of ops.lvis_eval_match.  Labels 0 .. num_classes are evaluated; any other row, a row
    past the image's 300 and a row of a label nobody looked for have rank -1."""
    N, cap = len(case.images), case.cap
    A, T = len(AREA_RANGES), len(IOU_THRS)
    match, ignore = np.zeros((A, T, N, cap), dtype=np.int8), np.zeros((A, T, N, cap), dtype=np.int8)
    rank, npig = np.full((N, cap), -1, dtype=np.int32), np.zeros((A, case.num_classes + 1), dtype=np.int32)
    for f, im in enumerate(case.images):
        kept = kept_rows(im, case.num_classes)
        for label in sorted(set(b["label"] for b in im["boxes"]) | set(label_of(im["rows"][r], case.num_classes) for r in kept)):
            if not 0 <= label <= case.num_classes:
                continue
            for a, rng in enumerate(AREA_RANGES):
                e = evaluate_img(im, kept, label, rng, case.num_classes)
                if e is None:
                    continue
                npig[a, label] += sum(1 for ig in e["gt_ig"] if not ig)
                for di, row in enumerate(e["rows"]):
                    rank[f, row] = di
                    for ti in range(T):
                        match[a, ti, f, row] = e["dtm"][ti][di]
                        ignore[a, ti, f, row] = e["dt_ig"][ti][di]
    return match, ignore, rank, npig


def as_annotations(case, first_id=10):
    """-> (an LVIS annotation dict, {image id: BoxList}) that pack to `case` again: image f gets id first_id + f, label l category id 2 * l"""
    import torch

    from diffusionvid_amd.structures.bounding_box import BoxList
    ann = {"images": [], "annotations": [],
           "categories": [{"id": 2 * l, "name": "c%d" % l, "frequency": case.frequency[l]} for l in range(1, case.num_classes + 1)]}
    preds, k = {}, 0
    for f, im in enumerate(case.images):
        ann["images"].append({"id": first_id + f, "width": 640, "height": 640, "neg_category_ids": [2 * l for l in im["neg"]],
                              "not_exhaustive_category_ids": [2 * l for l in im["nex"]]})
        for b in im["boxes"]:
            k += 1
            a = {"id": k, "image_id": first_id + f, "category_id": 2 * b["label"], "bbox": list(b["bbox"]), "area": b["area"]}
            if b["ignore"]:
                a["ignore"] = 1
            ann["annotations"].append(a)
        rows = np.asarray(im["rows"], dtype=np.float32).reshape(-1, 6)
        if len(rows) == 0 and f % 2:
            continue          # an image without a prediction at all
        bl = BoxList(torch.from_numpy(rows[:, :4].copy()), (640, 640))
        bl.add_field("scores", torch.from_numpy(rows[:, 4].copy()))
        bl.add_field("labels", torch.from_numpy(rows[:, 5].astype(np.int64)))
        preds[first_id + f] = bl
    return ann, preds


# ---- known answers, hand-worked --------------------------------------------------------------------------------------------------------
def _det(x, y, w, h, score, label=1):
    return [x, y, x + w, y + h, score, label]


GT = ([10, 10, 50, 50], None, 0, 1)          # 50 x 50 = 2500 pixels: "medium"
ONE = 1.0          # a precision of "1" is 1 / (1 + np.spacing(1)) in this protocol: the tests compare precisions within 1e-12


def known_cases():
    """name -> (Case, {stat name: value}); every answer is worked out in the comment above its case.  In every case a hit has IoU 1, so
    each category's AP is the same at all ten thresholds."""
    cases = {}
    # Category 2's only box is on image 1, found by a row of score 0.5: tp = [1], fp = [0], AP(2) = 1.  Image 0 has a row of category 2
    # and score 0.9 on nothing, but image 0 was never searched for category 2 (not a category of its boxes, not in its negative list):
    # the row vanishes.  Category 1: one box, one hit: AP(1) = 1.  AP = (1 + 1) / 2 = 1.  The COCO protocol keeps the 0.9 row as a false
    # positive in front of the hit: tp = [0, 1], fp = [1, 1], precision [0, 1/2] -> envelope [1/2, 1/2], AP(2) = 1/2, AP = 3/4.
    two = [image([_det(10, 10, 50, 50, 0.8, 1), _det(300, 300, 50, 50, 0.9, 2)], [GT]),
           image([_det(10, 10, 50, 50, 0.5, 2)], [([10, 10, 50, 50], None, 0, 2)])]
    cases["unlisted_vanishes"] = (Case(two, 2), {"AP": ONE, "AP50": ONE, "APf": ONE, "AR@300": 1.0})
    # The same with category 2 in image 0's negative list: somebody looked and there is none, so the 0.9 row IS a false positive:
    # AP(2) = 1/2 as worked out above, AP = (1 + 1/2) / 2 = 3/4.  Recall is untouched: both boxes are found.
    listed = [dict(two[0], neg=[2]), two[1]]
    cases["negative_counts"] = (Case(listed, 2), {"AP": 0.75, "AP50": 0.75, "AR@300": 1.0})
    # One box of category 1; a row on nothing (0.9) in front of a hit (0.8).  Exhaustive: tp = [0, 1], fp = [1, 1] -> AP = 1/2.
    miss_hit = [_det(300, 300, 50, 50, 0.9), _det(10, 10, 50, 50, 0.8)]
    cases["exhaustive_miss"] = (Case([image(miss_hit, [GT])], 1), {"AP": 0.5, "AR@300": 1.0})
    # The same image with category 1 not exhaustively annotated: the unmatched row may be an instance nobody boxed, so it is ignored:
    # tp = [1], fp = [0], AP = 1.  The matched row counts as ever (match 1, ignore 0).
    cases["not_exhaustive_miss"] = (Case([image(miss_hit, [GT], nex=[1])], 1), {"AP": ONE, "AR@300": 1.0})
    # Three categories, rare, common, common, each with one box on its own image.  1: a hit, AP 1.  2: a miss (0.9) in front of a hit
    # (0.8), AP 1/2.  3: a hit, AP 1.  APr = 1, APc = (1/2 + 1) / 2 = 3/4, no frequent category: APf = -1.  AP = (1 + 1/2 + 1) / 3 = 5/6.
    freq = [image([_det(10, 10, 50, 50, 0.7, 1)], [GT]),
            image([_det(300, 300, 50, 50, 0.9, 2), _det(10, 10, 50, 50, 0.8, 2)], [([10, 10, 50, 50], None, 0, 2)]),
            image([_det(10, 10, 50, 50, 0.6, 3)], [([10, 10, 50, 50], None, 0, 3)])]
    cases["frequency_groups"] = (Case(freq, 3, {1: "r", 2: "c", 3: "c"}), {"AP": 5 / 6, "APr": ONE, "APc": 0.75, "APf": -1.0, "AR@300": 1.0})
    # Two boxes of category 1: the first has `ignore` 1, the second counts (npig = 1).  The row on the ignored box (0.9) matches it and is
    # ignored; the row on the counted box (0.8) is the one true positive: tp = [1], fp = [0], AP = 1, recall 1 / 1.  Were `ignore`
    # overlooked, npig would be 2; were the 0.9 row a false positive, AP would be 1/2.
    flagged = [image([_det(200, 200, 50, 50, 0.9), _det(10, 10, 50, 50, 0.8)], [([200, 200, 50, 50], None, 1, 1), GT])]
    cases["ignore_flag"] = (Case(flagged, 1), {"AP": ONE, "APm": ONE, "APs": -1.0, "AR@300": 1.0})
    return cases


def cut_case(on_box):
    """301 rows of one label on one image, one box.  Rows 0 and 1 share the LOWEST score and rows 2 .. 300 rise above it, so 299 rows come
    first and one place is left: the tie goes to the lower row, row 0 gets place 299 and row 1 falls out.  Row `on_box` (0 or 1) sits on
    the box, every other row on nothing: with 0 the box is found (AR@300 = 1), with 1 it never is (AR@300 = 0), as if row 1 did not exist."""
    rows = [_det(300 + i, 300, 20, 20, 0.001 if i < 2 else 0.01 + 0.001 * i, 1) for i in range(301)]
    rows[on_box] = _det(10, 10, 50, 50, 0.001, 1)
    return Case([image(rows, [GT])], 1)


def long_segment_case(n):
    """n rows of one label on one image in ascending score; the row of lowest score (row 0, last in order) sits on the only box.  For
    n <= 300 it is evaluated at place n - 1 and finds the box: there is no cut at 100 per (image, category)."""
    rows = [_det(10, 10, 50, 50, 0.001, 1)] + [_det(300 + i, 300, 20, 20, 0.01 + 0.001 * i, 1) for i in range(1, n)]
    return Case([image(rows, [GT])], 1)


def random_case(seed, images=None, max_gt=30, max_rows=340, classes=5):
    """seeded images with 0 .. max_rows rows (so some pass the 300) and 0 .. max_gt boxes of `classes` labels, coordinates on a
    quarter-pixel grid (float32 holds them exactly).  About half the rows are copies of a box of the image, shifted by whole pixels or not
    at all, and some boxes are copies of each other, so equal IoUs and all three sizes are met; one box in ten has `ignore`; the negative
    and not-exhaustive lists are random subsets of the labels (a third of the images have empty ones); one row in twenty repeats the
    score of the row before it.  The categories' frequencies cycle r, c, f."""
    rng = np.random.RandomState(seed)
    images = int(rng.randint(1, 7)) if images is None else images
    grid = (rng.permutation(images * max_rows).astype(np.float64) + 1) / (images * max_rows + 1)
    out = []
    for f in range(images):
        g = int(rng.randint(0, max_gt + 1)) if rng.rand() < 0.85 else 0
        gts = []
        for k in range(g):
            side = [8, 24, 40, 80, 120, 200][int(rng.randint(6))]
            w, h = (np.round(rng.uniform(0.5, 1.5, size=2) * side * 4) / 4).tolist()
            x, y = (np.round(rng.uniform(0, 300, size=2) * 4) / 4).tolist()
            if gts and rng.rand() < 0.15:
                x, y, w, h = gts[int(rng.randint(len(gts)))][0]
            area = None if rng.rand() < 0.5 else w * h * float(rng.uniform(0.4, 1.0))
            gts.append(([x, y, w, h], area, int(rng.rand() < 0.1), int(rng.randint(1, classes + 1))))
        n = int(rng.randint(0, max_rows + 1)) if rng.rand() < 0.85 else 0
        rows = []
        for i in range(n):
            if gts and rng.rand() < 0.5:
                (x, y, w, h), _, _, label = gts[int(rng.randint(len(gts)))]
                if rng.rand() < 0.7:
                    dx, dy, dw, dh = rng.randint(-6, 7, size=4).tolist()
                    x, y, w, h = x + dx, y + dy, max(1.0, w + dw), max(1.0, h + dh)
                if rng.rand() < 0.2:
                    label = int(rng.randint(1, classes + 1))
            else:
                side = [8, 24, 40, 80, 120, 200][int(rng.randint(6))]
                w, h = (np.round(rng.uniform(0.5, 1.5, size=2) * side * 4) / 4).tolist()
                x, y = (np.round(rng.uniform(0, 300, size=2) * 4) / 4).tolist()
                label = int(rng.randint(1, classes + 1))
            score = rows[-1][4] if rows and rng.rand() < 0.05 else grid[f * max_rows + i]
            rows.append([x, y, x + w, y + h, score, label])
        lists = rng.rand() >= 1 / 3
        neg = [l for l in range(1, classes + 1) if lists and rng.rand() < 0.4]
        nex = [l for l in range(1, classes + 1) if lists and rng.rand() < 0.3]
        out.append(image(rows, gts, neg, nex))
    return Case(out, classes, {l: "rcf"[(l - 1) % 3] for l in range(1, classes + 1)})
