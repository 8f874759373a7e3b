"""What the COCO evaluator's tests share: a loop-for-loop restatement of the protocol (compute_iou, evaluate_img, accumulate, summarize;
plain Python loops and Python floats, written from the protocol's text and not from the product's vectorised code), the hand-built
known-answer cases and a generator of random ones.  `matches` lays evaluate_img's answers out as ops.coco_eval_match returns them."""
import bisect

import numpy as np

IOU_THRS = [float(v) for v in np.linspace(.5, .95, 10)]
REC_THRS = [float(v) for v in np.linspace(0, 1, 101)]
MAX_DETS = (1, 10, 100)
AREA_RANGES = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))


class Case:
    """dets [N, cap, 6] float32 (xyxy, score, label), counts [N] int32; gt_boxes [G, 4] float64 xywh, gt_areas [G] float64, gt_crowd [G]
    uint8, gt_labels [G] int32, gt_starts [N + 1] int32; num_classes"""

    def __init__(self, dets, counts, gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, num_classes):
        self.dets, self.counts = np.ascontiguousarray(dets, dtype=np.float32), np.ascontiguousarray(counts, dtype=np.int32)
        self.gt_boxes = np.ascontiguousarray(gt_boxes, dtype=np.float64).reshape(-1, 4)
        self.gt_areas, self.gt_crowd = np.ascontiguousarray(gt_areas, dtype=np.float64), np.ascontiguousarray(gt_crowd, dtype=np.uint8)
        self.gt_labels, self.gt_starts = np.ascontiguousarray(gt_labels, dtype=np.int32), np.ascontiguousarray(gt_starts, dtype=np.int32)
        self.num_classes = int(num_classes)

    @property
    def images(self):
        return len(self.counts)

    def gt(self):
        return self.gt_boxes, self.gt_areas, self.gt_crowd, self.gt_labels, self.gt_starts


def pack(images, num_classes, cap=None):
    """images: per image (rows [[x1, y1, x2, y2, score, label], ...], boxes [([x, y, w, h], area | None, crowd, label), ...]); area None is
    w * h -> Case"""
    need = max(1, max((len(p) for p, _ in images), default=1))
    cap = need if cap is None else cap
    dets, counts = np.zeros((len(images), cap, 6), dtype=np.float32), np.zeros(len(images), dtype=np.int32)
    boxes, areas, crowd, labels, starts = [], [], [], [], [0]
    for f, (p, gts) in enumerate(images):
        p = np.asarray(p, dtype=np.float32).reshape(-1, 6)
        dets[f, :len(p)], counts[f] = p, len(p)
        for b, area, c, l in gts:
            boxes.append([float(v) for v in b])
            areas.append(float(b[2]) * float(b[3]) if area is None else float(area))
            crowd.append(int(c))
            labels.append(int(l))
        starts.append(len(boxes))
    return Case(dets, counts, np.asarray(boxes, dtype=np.float64).reshape(-1, 4), areas, crowd, labels, starts, num_classes)


# ---- the protocol, loop for loop -------------------------------------------------------------------------------------------------------
def compute_iou(d, g, crowd):
    """d, g: [x, y, w, h] Python floats"""
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    area_d = d[2] * d[3]
    if crowd:
        u = area_d
    else:
        area_g = g[2] * g[3]
        u = area_d + area_g
        u = u - i
    return i / u


def _rows_of(case, f, label):
    """the image's rows of `label`, stably sorted by descending score, cut at 100"""
    n = int(min(max(case.counts[f], 0), case.dets.shape[1]))
    rows = [r for r in range(n) if float(case.dets[f, r, 5]) == float(label)]
    rows.sort(key=lambda r: -float(case.dets[f, r, 4]))          # Python's sort is stable
    return rows[:MAX_DETS[-1]]


def _xywh(row):
    x1, y1, x2, y2 = (float(v) for v in row[:4])
    return [x1, y1, x2 - x1, y2 - y1]


def evaluate_img(case, f, label, area_rng):
    """-> None when the (image, label) pair has neither a row nor a box, else a dict: rows (the image's row numbers in order), scores,
    dtm[t][d] (True: matched), dt_ig[t][d], gt_ig[g] in annotation order"""
    rows = _rows_of(case, f, label)
    gts = [k for k in range(int(case.gt_starts[f]), int(case.gt_starts[f + 1])) if int(case.gt_labels[k]) == label]
    if not rows and not gts:
        return None
    lo, hi = area_rng
    ig_of = {}
    for k in gts:
        area = float(case.gt_areas[k])
        ig_of[k] = bool(case.gt_crowd[k]) or area < lo or area > hi
    order = [k for k in gts if not ig_of[k]] + [k for k in gts if ig_of[k]]
    boxes = [_xywh(case.dets[f, r]) for r in rows]
    ious = [{k: compute_iou(d, [float(v) for v in case.gt_boxes[k]], bool(case.gt_crowd[k])) for k in gts} for d in boxes]
    dtm =[[False] * len(rows) for _ in IOU_THRS]
    dt_ig = [[False] * len(rows) for _ in IOU_THRS]
    for ti, t in enumerate(IOU_THRS):
        gtm = {k: False for k in gts}
        for di, d in enumerate(boxes):
            best = min(t, 1 - 1e-10)
            m = -1
            for k in order:
                crowd = bool(case.gt_crowd[k])
                if gtm[k] and not crowd:
                    continue
                if m > -1 and not ig_of[m] and ig_of[k]:
                    break
                iou = ious[di][k]
                if iou < best:
                    continue
                best = iou
                m = k
            if m > -1:
                dtm[ti][di] = True
                dt_ig[ti][di] = ig_of[m]
                gtm[m] = True
    for di, d in enumerate(boxes):
        area = d[2] * d[3]
        if area < lo or area > hi:
            for ti in range(len(IOU_THRS)):
                if not dtm[ti][di]:
                    dt_ig[ti][di] = True
    return {"rows": rows, "scores": [float(case.dets[f, r, 4]) for r in rows], "dtm": dtm, "dt_ig": dt_ig, "gt_ig": [ig_of[k] for k in gts]}


def accumulate(case):
    """-> precision [10, 101, K, 4, 3], recall [10, K, 4, 3]; category k is label k + 1"""
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), case.num_classes, len(AREA_RANGES), len(MAX_DETS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        for a, rng in enumerate(AREA_RANGES):
            per_image = [evaluate_img(case, f, k + 1, rng) for f in range(case.images)]
            per_image = [e for e in per_image if e is not None]
            for mi, max_det in enumerate(MAX_DETS):
                scores, cols, npig = [], [], 0
                for e in per_image:
                    for di in range(min(max_det, len(e["rows"]))):
                        scores.append(e["scores"][di])
                        cols.append((e, di))
                    npig += sum(1 for ig in e["gt_ig"] if not ig)
                if npig == 0:
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
                    rc = [tps[i] / npig for i in range(nd)]
                    pr = [tps[i] / (fps[i] + tps[i] + float(np.spacing(1))) for i in range(nd)]
                    recall[ti, k, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, r in enumerate(REC_THRS):
                        pi = bisect.bisect_left(rc, r)
                        precision[ti, ri, k, a, mi] = pr[pi] if pi < nd else 0.0
    return precision, recall


def _mean(values):
    values = [float(v) for v in np.asarray(values).reshape(-1) if v > -1]
    return float(np.mean(values)) if values else -1.0


def summarize(precision, recall):
    """AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl"""
    t50, t75 = IOU_THRS.index(.5), IOU_THRS.index(.75)
    out = [_mean(precision[:, :, :, 0, 2]), _mean(precision[t50, :, :, 0, 2]), _mean(precision[t75, :, :, 0, 2])]
    out += [_mean(precision[:, :, :, a, 2]) for a in (1, 2, 3)]
    out += [_mean(recall[:, :, 0, mi]) for mi in (0, 1, 2)]
    out += [_mean(recall[:, :, a, 2]) for a in (1, 2, 3)]
    return np.array(out)


def evaluate(case):
    precision, recall = accumulate(case)
    return {"precision": precision, "recall": recall, "stats": summarize(precision, recall)}


def matches(case):
    """evaluate_img's answers at every row's own place -> (match [4, 10, N, cap] int8, ignore [4, 10, N, cap] int8, rank [N, cap] int32,
    npig [4, num_classes + 1] int32): the arrays of ops.coco_eval_match.  Labels 0 .. num_classes are evaluated; any other row has rank -1."""
    N, cap = case.dets.shape[:2]
    A, T = len(AREA_RANGES), len(IOU_THRS)
    match, ignore = np.zeros((A, T, N, cap), dtype=np.int8), np.zeros((A, T, N, cap), dtype=np.int8)
    rank, npig = np.full((N, cap), -1, dtype=np.int32), np.zeros((A, case.num_classes + 1), dtype=np.int32)
    for f in range(N):
        for label in range(case.num_classes + 1):
            for a, rng in enumerate(AREA_RANGES):
                e = evaluate_img(case, f, label, rng)
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
    """-> (a COCO annotation dict, {image id: BoxList}) that pack to `case` again: image f gets id first_id + f, label l category id 2 * l"""
    import torch

    from diffusionvid_amd.structures.bounding_box import BoxList
    ann = {"images": [{"id": first_id + f, "width": 640, "height": 640} for f in range(case.images)],
           "categories": [{"id": 2 * l, "name": "c%d" % l} for l in range(1, case.num_classes + 1)], "annotations": []}
    preds = {}
    for f in range(case.images):
        for k in range(int(case.gt_starts[f]), int(case.gt_starts[f + 1])):
            ann["annotations"].append({"id": k + 1, "image_id": first_id + f, "category_id": 2 * int(case.gt_labels[k]),
                                       "bbox": case.gt_boxes[k].tolist(), "area": float(case.gt_areas[k]), "iscrowd": int(case.gt_crowd[k])})
        n = int(case.counts[f])
        if n == 0 and f % 2:
            continue          # an image without a prediction at all
        bl = BoxList(torch.from_numpy(case.dets[f, :n, :4].copy()), (640, 640))
        bl.add_field("scores", torch.from_numpy(case.dets[f, :n, 4].copy()))
        bl.add_field("labels", torch.from_numpy(case.dets[f, :n, 5].astype(np.int64)))
        preds[first_id + f] = bl
    return ann, preds


# ---- known answers (tests/test_coco_eval.py states the arithmetic) ---------------------------------------------------------------------
def _det(x, y, w, h, score, label=1):
    return [x, y, x + w, y + h, score, label]


def known_cases():
    """name -> Case; boxes of 50 x 50 = 2500 pixels are "medium", 10 x 10 "small", 100 x 100 "large" """
    gt = ([10, 10, 50, 50], None, 0, 1)
    cases = {}
    cases["perfect"] = pack([([_det(10, 10, 50, 50, 0.9)], [gt])], 1)
    cases["hit_and_miss"] = pack([([_det(200, 200, 50, 50, 0.9), _det(10, 10, 50, 50, 0.8)], [gt])], 1)
    cases["iou_half"] = pack([([_det(0, 0, 10, 5, 0.9)], [([0, 0, 10, 10], None, 0, 1)])], 1)
    cases["crowd"] = pack([([_det(0, 0, 10, 10, 0.9), _det(10, 10, 10, 10, 0.8), _det(20, 20, 10, 10, 0.7), _det(300, 300, 50, 50, 0.6)],
                            [([0, 0, 100, 100], None, 1, 1), ([300, 300, 50, 50], None, 0, 1)])], 1)
    cases["small_gt"] = pack([([_det(10, 10, 10, 10, 0.9)], [([10, 10, 10, 10], None, 0, 1)])], 1)
    cases["unmatched_outside"] = pack([([_det(10, 10, 50, 50, 0.9), _det(200, 200, 10, 10, 0.95)], [gt])], 1)
    # a 10 x 10 row with IoU exactly 0.5 to its upper and to its lower half; the second row is the lower half itself
    cases["equal_iou"] = pack([([_det(0, 0, 10, 10, 0.9), _det(0, 5, 10, 5, 0.8)],
                                [([0, 0, 10, 5], None, 0, 1), ([0, 5, 10, 5], None, 0, 1)])], 1)
    # the break rule: a 100 x 100 row over a 100 x 78 counted box (IoU 0.78) and an identical crowd box (IoU 1.0), the crowd box annotated first
    cases["break_rule"] = pack([([_det(0, 0, 100, 100, 0.9)], [([0, 0, 100, 100], None, 1, 1), ([0, 0, 100, 78], None, 0, 1)])], 1)
    return cases


def cut_case(n):
    """one label, one image, n rows in ascending score (so the last row is first in order): the row of LOWEST score sits on the box"""
    rows = [_det(10, 10, 50, 50, 0.001, 1)] + [_det(300 + i, 300, 20, 20, 0.01 + 0.001 * i, 1) for i in range(1, n)]
    return pack([(rows, [([10, 10, 50, 50], None, 0, 1)])], 1)


def ar_case():
    """eleven 30 x 30 boxes of one label on one image and twelve rows in descending score: the rows at positions 0, 4, 9 and 10 sit exactly
    on boxes 0, 1, 2 and 3, the others on nothing.  So 1, 3 and 4 of the 11 boxes are found among the first 1, 10 and 100 rows."""
    boxes = [([40.0 * i, 0, 30, 30], None, 0, 1) for i in range(11)]
    rows = []
    for i in range(12):
        on = {0: 0, 4: 1, 9: 2, 10: 3}.get(i)
        rows.append(_det(40.0 * on, 0, 30, 30, 0.9 - 0.01 * i) if on is not None else _det(40.0 * i, 500, 30, 30, 0.9 - 0.01 * i))
    return pack([(rows, boxes)], 1)


def random_case(seed, images=None, max_gt=40, max_rows=130, classes=3):
    """seeded images with 0 .. max_rows rows and 0 .. max_gt boxes of `classes` labels (coordinates on a quarter-pixel grid, so float32 rows
    hold them exactly).  About half the rows are copies of a box of the image, shifted by whole pixels or not at all, and some boxes are
    copies of each other, so equal IoUs, crowd boxes, all three sizes and segments beyond 100 rows are met.  Scores are distinct over the
    whole set (a shuffled grid).  Some annotation areas are a fraction of w * h, as a segmentation's would be."""
    rng = np.random.RandomState(seed)
    images = int(rng.randint(1, 9)) if images is None else images
    grid = (rng.permutation(images * max_rows).astype(np.float64) + 1) / (images * max_rows + 1)
    out = []
    for f in range(images):
        g = int(rng.randint(0, max_gt + 1)) if rng.rand() < 0.85 else 0
        one_label = rng.rand() < 0.4
        gts = []
        for k in range(g):
            side = [8, 24, 40, 80, 120, 200][int(rng.randint(6))]
            w, h = (np.round(rng.uniform(0.5, 1.5, size=2) * side * 4) / 4).tolist()
            x, y = (np.round(rng.uniform(0, 300, size=2) * 4) / 4).tolist()
            if gts and rng.rand() < 0.15:
                x, y, w, h = gts[int(rng.randint(len(gts)))][0]
            label = 1 if one_label else int(rng.randint(1, classes + 1))
            area = None if rng.rand() < 0.5 else w * h * float(rng.uniform(0.4, 1.0))
            gts.append(([x, y, w, h], area, int(rng.rand() < 0.15), label))
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
                label = 1 if one_label else int(rng.randint(1, classes + 1))
            rows.append([x, y, x + w, y + h, grid[f * max_rows + i], label])
        out.append((rows, gts))
    return pack(out, classes)
