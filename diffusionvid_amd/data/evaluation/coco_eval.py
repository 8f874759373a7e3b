"""COCO bbox evaluation (iouType "bbox", useCats 1) of the still-image path: the twelve numbers of the COCO protocol from
engine.inference_images' predictions and a COCO annotation file.  numpy by default; with `device` the matching runs on the GPU
(ops.coco_eval_match, csrc/cocoeval.hip), as vid_eval does for ImageNet VID.

The reference hands this to pycocotools (mega_core/data/datasets/evaluation/coco/coco_eval.py:305-324).  This module states the protocol
itself, from its published definition:

  parameters   IoU thresholds linspace(.5, .95, 10), recall thresholds linspace(0, 1, 101), maxDets (1, 10, 100), area ranges all / small
               (<= 32^2) / medium / large (>= 96^2), both ends inclusive
  boxes        [x, y, w, h] float64; a detection's area is w * h, a ground-truth box's the annotation's `area`; ignore = iscrowd
  IoU          per axis min(dx + dw, gx + gw) - max(dx, gx), <= 0 on either axis: 0; i = w * h; u = area_d for a crowd box, else
               (area_d + area_g) - i with the areas w * h of both boxes; i / u
  matching     per (image, category): detections in descending score (stable), the first 100; per area range the ground truth ordered not
               ignored first; per threshold every detection takes the box of greatest IoU >= min(t, 1 - 1e-10) that no earlier
               detection took (crowd boxes can be taken again), the later box on equal IoU, and does not leave a not ignored match for an
               ignored box; a detection matched to an ignored box, or unmatched with its own area outside the range, does not count
  accumulate   per (category, area range, maxDet M): every image's first M detections, stably sorted by descending score; cumulative true
               and false positives; recall = tp / npig, precision = tp / (fp + tp + eps) made monotone from the back and read at the
               101 recall thresholds
  summarize    means over the entries > -1

Both paths produce (match, ignore, rank, npig) in one layout and share accumulate_from_matches, so their results are equal, not close.
accumulate="device" runs accumulate_arrays as kernels on those arrays (ops.eval_accumulate, csrc/evalaccum.hip): its order of the rows is
total -- label, score descending, image, rank -- and the rest is integer counts and single float64 divisions, so that result is equal too.
Not here: segmentation and keypoint evaluation, proposal recall, evaluation spread over ranks; LVIS' federated protocol is lvis_eval.py."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

from .vid_eval import _Laps

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RANGES = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))
AREA_NAMES = ("all", "small", "medium", "large")
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


class CocoAnnotations:
    """A COCO annotation file (a path or the loaded dict), read with the standard library.  image_ids: ascending; label_of: category id
    -> label 1 .. K by ascending category id; category_of: the inverse (the `label_map` of engine.coco_results); names: label -> name;
    images: id -> its entry; anns_of: image id -> its annotations in file order."""

    def __init__(self, json_file_or_dict):
        data = json_file_or_dict
        if not isinstance(data, dict):
            with open(data) as f:
                data = json.load(f)
        self.images = {int(im["id"]): im for im in data.get("images", ())}
        self.image_ids = sorted(self.images)
        cats = sorted(data.get("categories", ()), key=lambda c: int(c["id"]))
        self.label_of = {int(c["id"]): i + 1 for i, c in enumerate(cats)}
        self.category_of = {l: c for c, l in self.label_of.items()}
        self.names = {self.label_of[int(c["id"])]: c.get("name", str(c["id"])) for c in cats}
        self.num_classes = len(cats)
        self.anns_of = {i: [] for i in self.image_ids}
        for a in data.get("annotations", ()):
            image_id, cat = int(a["image_id"]), int(a["category_id"])
            if image_id not in self.anns_of:
                raise ValueError("annotation %r names image %d, which the file does not list" % (a.get("id"), image_id))
            if cat not in self.label_of:
                raise ValueError("annotation %r names category %d, which the file does not list" % (a.get("id"), cat))
            self.anns_of[image_id].append(a)


def pack_groundtruth(ann, image_ids=None):
    """-> (boxes [G, 4] float64 xywh, areas [G] float64, crowd [G] uint8, labels [G] int32, starts [N + 1] int32): image j of `image_ids`
    (default: all of ann's, ascending) owns rows starts[j] : starts[j + 1], in annotation order.  An annotation without `area` gets w * h."""
    image_ids = ann.image_ids if image_ids is None else list(image_ids)
    n = [len(ann.anns_of[i]) for i in image_ids]
    starts = np.zeros(len(n) + 1, dtype=np.int64)
    np.cumsum(n, out=starts[1:])
    G = int(starts[-1])
    assert G < 2 ** 31, "the ground truth is indexed with int32"
    boxes, areas = np.zeros((G, 4), dtype=np.float64), np.zeros(G, dtype=np.float64)
    crowd, labels = np.zeros(G, dtype=np.uint8), np.zeros(G, dtype=np.int32)
    k = 0
    for i in image_ids:
        for a in ann.anns_of[i]:
            boxes[k] = a["bbox"]
            areas[k] = a["area"] if "area" in a else boxes[k, 2] * boxes[k, 3]
            crowd[k] = 1 if a.get("iscrowd", 0) else 0
            labels[k] = ann.label_of[int(a["category_id"])]
            k += 1
    return boxes, areas, crowd, labels, starts.astype(np.int32)


def pack_detections(predictions, image_ids):
    """{image id: BoxList} -> engine.pack_predictions' (counts [N] int32, dets [N, cap, 6] fp32) over `image_ids`: an image without a
    prediction is an empty row; a prediction for an image that is not listed is an error."""
    from ...engine.inference import pack_predictions
    pos = {i: j for j, i in enumerate(image_ids)}
    for i in sorted(predictions):
        if int(i) not in pos:
            raise ValueError("there is a prediction for image id %d, which the annotations do not list" % int(i))
    ids, counts, dets, _ = pack_predictions(predictions)
    at = torch.tensor([pos[int(i)] for i in ids.tolist()], dtype=torch.int64)
    all_counts = torch.zeros((len(image_ids),), dtype=torch.int32)
    all_dets = torch.zeros((len(image_ids), dets.shape[1], 6), dtype=torch.float32)
    all_counts[at], all_dets[at] = counts, dets
    return all_counts, all_dets


def _np(a, dtype=None):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if dtype is None else a.astype(dtype, copy=False)


def _xywh(rows):
    """xyxy float32 rows -> (x, y, w, h, area) float64, w = x2 - x1 in float64"""
    x, y = rows[:, 0].astype(np.float64), rows[:, 1].astype(np.float64)
    w, h = rows[:, 2].astype(np.float64) - x, rows[:, 3].astype(np.float64) - y
    return x, y, w, h, w * h


def _ious(d, g, crowd):
    """[D, G] float64; d, g: (x, y, w, h) columns"""
    dx, dy, dw, dh = (c[:, None] for c in d)
    gx, gy, gw, gh = (c[None, :] for c in g)
    w = np.minimum(dx + dw, gx + gw) - np.maximum(dx, gx)
    h = np.minimum(dy + dh, gy + gh) - np.maximum(dy, gy)
    i = w * h
    da, ga = dw * dh, gw * gh
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(crowd[None, :], np.broadcast_to(da, i.shape), da + ga - i)
        return np.where((w <= 0) | (h <= 0), 0.0, i / u)


def _match_setup(N, cap, gt_flag, gt_areas, gt_labels, num_classes):
    """what a match_numpy starts from -> (match, ignore, rank, npig, gig_all): the four outputs with no row matched and npig counted, and
    gig_all [A, G] bool: the box is flagged (COCO: crowd, LVIS: ignore) or its area lies outside the range"""
    A, T = len(AREA_RANGES), len(IOU_THRS)
    match, ignore = np.zeros((A, T, N, cap), dtype=np.int8), np.zeros((A, T, N, cap), dtype=np.int8)
    rank = np.full((N, cap), -1, dtype=np.int32)
    npig = np.zeros((A, num_classes + 1), dtype=np.int32)
    gig_all = np.stack([gt_flag | (gt_areas < lo) | (gt_areas > hi) for lo, hi in AREA_RANGES])
    ok = (gt_labels >= 0) & (gt_labels <= num_classes)
    for a in range(A):
        np.add.at(npig[a], gt_labels[ok & ~gig_all[a]], 1)
    return match, ignore, rank, npig, gig_all


def _match_label(match, ignore, f, sel, xywh, g_boxes, gig, crowd, unmatched):
    """The rows `sel` of image f, one label's in descending score, against that label's boxes g_boxes [n_g, 4] with gig [A, n_g]; written
    to match / ignore [:, :, f, sel].  crowd [n_g] bool: the box can be taken again; unmatched [A, n] bool by row of the image: what a row
    that takes no box gets as its ignore."""
    if len(g_boxes) == 0:
        ignore[:, :, f, sel] = unmatched[:, None, sel]
        return
    T, best0 = len(IOU_THRS), np.minimum(IOU_THRS, 1 - 1e-10)
    iou = _ious(tuple(c[sel] for c in xywh), g_boxes.T, crowd)
    for a in range(len(AREA_RANGES)):
        gorder = np.argsort(gig[a], kind="mergesort")
        taken = np.zeros((T, len(g_boxes)), dtype=bool)
        for d, row in enumerate(sel):
            best, m, m_ig = best0.copy(), np.full(T, -1), np.zeros(T, dtype=bool)
            for k in gorder:
                free = ~taken[:, k] | crowd[k]
                if gig[a, k]:
                    free &= ~((m > -1) & ~m_ig)
                take = free & ~(iou[d, k] < best)
                best[take], m[take], m_ig[take] = iou[d, k], k, gig[a, k]
            hit = m > -1
            taken[hit, m[hit]] = True
            match[a, :, f, row] = hit
            ignore[a, :, f, row] = np.where(hit, m_ig, unmatched[a, row])


def match_numpy(dets, counts, gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, num_classes):
    """The matching, in the layout of ops.coco_eval_match: (match [4, 10, N, cap] int8, ignore [4, 10, N, cap] int8, rank [N, cap] int32,
    npig [4, num_classes + 1] int32).  Vectorised over the thresholds; images, labels, area ranges, detections and boxes are loops."""
    dets, counts = _np(dets, np.float32), _np(counts, np.int64)
    gt_boxes, gt_areas, gt_crowd = _np(gt_boxes, np.float64).reshape(-1, 4), _np(gt_areas, np.float64), _np(gt_crowd).astype(bool)
    gt_labels, gt_starts = _np(gt_labels, np.int64), _np(gt_starts, np.int64)
    N, cap = dets.shape[:2]
    top = MAX_DETS[-1]
    match, ignore, rank, npig, gig_all = _match_setup(N, cap, gt_crowd, gt_areas, gt_labels, num_classes)
    for f in range(N):
        n = int(min(max(counts[f], 0), cap))
        if n == 0:
            continue
        rows = dets[f, :n]
        x, y, w, h, area = _xywh(rows)
        lab = np.where((rows[:, 5] >= 0) & (rows[:, 5] <= num_classes), rows[:, 5], -1).astype(np.int64)
        g0, g1 = int(gt_starts[f]), int(gt_starts[f + 1])
        d_out = np.stack([(area < lo) | (area > hi) for lo, hi in AREA_RANGES])          # [A, n]
        for l in np.unique(lab[lab >= 0]):
            idx = np.nonzero(lab == l)[0]
            sel = idx[np.argsort(-rows[idx, 4], kind="mergesort")[:top]]
            rank[f, sel] = np.arange(len(sel))
            gi = g0 + np.nonzero(gt_labels[g0:g1] == l)[0]
            _match_label(match, ignore, f, sel, (x, y, w, h), gt_boxes[gi], gig_all[:, gi], gt_crowd[gi], d_out)
    return match, ignore, rank, npig


def accumulate_from_matches(scores, labels, counts, rank, match, ignore, npig):
    """accumulate + summarize on the matching's arrays: scores / labels / rank [N, cap] (images in ascending id), counts [N], match and
    ignore [4, 10, N, cap], npig [4, K + 1] -> {"precision" [10, 101, K, 4, 3], "recall" [10, K, 4, 3], "stats": the twelve numbers};
    category k is label k + 1.  float64 throughout."""
    precision, recall = accumulate_arrays(scores, labels, counts, rank, match, ignore, npig, MAX_DETS)
    return {"precision": precision, "recall": recall, "stats": summarize(precision, recall)}


def accumulate_arrays(scores, labels, counts, rank, match, ignore, npig, max_dets):
    """accumulate alone, for the protocol's own list of detection limits (lvis_eval has one, 300) -> (precision [10, 101, K, 4, M],
    recall [10, K, 4, M]), M = len(max_dets)"""
    scores, labels, rank = _np(scores), _np(labels, np.int64), _np(rank)
    match, ignore, npig = _np(match), _np(ignore), _np(npig)
    A, T, N, cap = match.shape
    K, R, M = npig.shape[1] - 1, len(REC_THRS), len(max_dets)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    live = (np.arange(cap)[None, :] < _np(counts, np.int64).reshape(-1, 1)) & (rank >= 0)
    fi, ri = np.nonzero(live)
    lab, rk = labels[fi, ri], rank[fi, ri]
    order = np.lexsort((rk, fi, lab))          # by label, then image, then rank
    flat, lab, rk = (fi * cap + ri)[order], lab[order], rk[order]
    bounds = np.searchsorted(lab, np.arange(K + 2))
    # the counted true and false positives of every live row, all (area range, threshold) pairs side by side, in that order: a category
    # is then one contiguous block of columns
    flat_m, flat_i = match.reshape(A * T, -1) != 0, ignore.reshape(A * T, -1) != 0
    tp_all, fp_all = (flat_m & ~flat_i)[:, flat], (~flat_m & ~flat_i)[:, flat]
    s_all = scores.reshape(-1)[flat]
    eps = np.spacing(1)
    for k in range(K):
        b0, b1 = bounds[k + 1], bounds[k + 2]
        counted = np.nonzero(npig[:, k + 1] > 0)[0]
        if len(counted) == 0:
            continue
        n_gt = np.where(npig[:, k + 1] > 0, npig[:, k + 1], 1).astype(np.float64)[:, None, None]
        for mi, max_det in enumerate(max_dets):
            sel = b0 + np.nonzero(rk[b0:b1] < max_det)[0]
            sel = sel[np.argsort(-s_all[sel], kind="mergesort")]
            nd = len(sel)
            if nd == 0:
                recall[:, k, counted, mi], precision[:, :, k, counted, mi] = 0, 0
                continue
            tp = np.cumsum(tp_all[:, sel].astype(np.float64), axis=1).reshape(A, T, nd)
            fp = np.cumsum(fp_all[:, sel].astype(np.float64), axis=1).reshape(A, T, nd)
            rc = tp / n_gt
            pr = tp / (fp + tp + eps)
            pr = np.maximum.accumulate(pr[:, :, ::-1], axis=2)[:, :, ::-1]          # pr[i - 1] = max(pr[i - 1], pr[i]) from the back
            for a in counted:
                recall[:, k, a, mi] = rc[a, :, -1]
                for t in range(T):
                    inds = np.searchsorted(rc[a, t], REC_THRS, side="left")
                    precision[t, :, k, a, mi] = np.where(inds < nd, pr[a, t, np.minimum(inds, nd - 1)], 0.0)
    return precision, recall


ACCUMULATE_MODES = ("numpy", "device")


def check_accumulate(accumulate, device, keyword="accumulate", device_keyword="device"):
    """the evaluators' `accumulate` keyword: "numpy", or "device", which needs a device for the matching as well"""
    if accumulate not in ACCUMULATE_MODES:
        raise ValueError("%s is 'numpy' or 'device', not %r" % (keyword, accumulate))
    if accumulate == "device" and device is None:
        raise ValueError("%s='device' needs %s: the accumulation runs where the matching leaves its arrays" % (keyword, device_keyword))


def accumulate_arrays_device(dets, counts, rank, match, ignore, npig, max_dets):
    """accumulate_arrays as kernels (ops.eval_accumulate, csrc/evalaccum.hip) on the arrays the matching left on the device (dets
    [N, cap, 6] supplies the scores and the labels) -> (precision, recall) on the host, equal to accumulate_arrays' bit for bit"""
    from ... import ops
    precision, recall = ops.eval_accumulate(dets, counts, rank, match, ignore, npig, max_dets, REC_THRS)
    return precision.cpu().numpy(), recall.cpu().numpy()


def _mean(s):
    s = s[s > -1]
    return float(np.mean(s)) if len(s) else -1.0


def summarize(precision, recall):
    """the twelve numbers, in STAT_NAMES' order"""
    t50, t75, last = int(np.where(IOU_THRS == .5)[0][0]), int(np.where(IOU_THRS == .75)[0][0]), len(MAX_DETS) - 1
    stats = [_mean(precision[:, :, :, 0, last]), _mean(precision[t50, :, :, 0, last]), _mean(precision[t75, :, :, 0, last])]
    stats += [_mean(precision[:, :, :, a, last]) for a in (1, 2, 3)]
    stats += [_mean(recall[:, :, 0, mi]) for mi in range(len(MAX_DETS))]
    stats += [_mean(recall[:, :, a, last]) for a in (1, 2, 3)]
    return np.array(stats)


def _tail(dets, counts, rank, match, ignore, npig):
    host = _np(dets[:, :, 4:6])
    return accumulate_from_matches(np.ascontiguousarray(host[:, :, 0]), host[:, :, 1].astype(np.int64), counts, rank, match, ignore, npig)


def evaluate_numpy(dets, counts, gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, num_classes):
    """The whole protocol in numpy on engine.pack_predictions' arrays (dets [N, cap, 6] fp32 xyxy / score / label, counts [N]; images in
    ascending id) and pack_groundtruth's -> accumulate_from_matches' dict."""
    dets = torch.as_tensor(_np(dets, np.float32))
    if dets.shape[1] == 0:          # no detection at all: the ground truth still counts
        dets = dets.new_zeros((dets.shape[0], 1, 6))
    got = match_numpy(dets, counts, gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, num_classes)
    return _tail(dets, counts, got[2], got[0], got[1], got[3])


def _evaluate_on_device(dets, counts, gt, match_op, num_classes, max_dets, summarize, device, times, accumulate):
    """What the evaluate_device of COCO and of LVIS do alike.  gt: the ground truth as (array, numpy dtype) pairs in the order match_op
    (ops.coco_eval_match / ops.lvis_eval_match) takes them; max_dets: the protocol's detection limits; summarize(precision, recall) -> stats"""
    from ... import ops
    dets = torch.as_tensor(dets)
    device = torch.device(device) if device is not None else dets.device
    check_accumulate(accumulate, device)
    lap = _Laps(times, device)
    dets = dets.to(device=device, dtype=torch.float32)
    counts = torch.as_tensor(counts).to(device=device, dtype=torch.int32)
    if dets.shape[1] == 0:
        dets = dets.new_zeros((dets.shape[0], 1, 6))
    gt = [torch.from_numpy(np.ascontiguousarray(_np(a, t))).to(device) for a, t in gt]
    lap("copy_in")
    got = match_op(dets, counts, *gt, num_classes, IOU_THRS, AREA_RANGES)
    lap("kernel")
    if accumulate == "device":
        match, ignore, rank, npig = got
        pr, rc = ops.eval_accumulate(dets, counts, rank, match, ignore, npig, max_dets, REC_THRS)
        lap("accumulate")
        precision, recall = pr.cpu().numpy(), rc.cpu().numpy()
        lap("copy_out")
    else:
        match, ignore, rank, npig = (t.cpu().numpy() for t in got)
        host, counts = dets.cpu(), counts.cpu().numpy()
        lap("copy_out")
        host = _np(host[:, :, 4:6])
        precision, recall = accumulate_arrays(np.ascontiguousarray(host[:, :, 0]), host[:, :, 1].astype(np.int64), counts, rank, match, ignore, npig,
                                              max_dets)
    out = {"precision": precision, "recall": recall, "stats": summarize(precision, recall)}
    lap("tail")
    return out


def evaluate_device(dets, counts, gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, num_classes, device=None, times=None, accumulate="numpy"):
    """evaluate_numpy with the matching as one kernel call on `device` (default: where dets is); the accumulation is the same numpy
    code on the same arrays, so the result is equal.  times: see vid_eval._Laps (copy_in, kernel, copy_out, tail).
    accumulate "device": match, ignore and rank stay on the device, ops.eval_accumulate runs there and only precision and recall
    come back (equal again: csrc/evalaccum.hip); the laps are then copy_in, kernel, accumulate, copy_out, tail (summarize)."""
    from ... import ops
    gt = ((gt_boxes, np.float64), (gt_areas, np.float64), (gt_crowd, np.uint8), (gt_labels, np.int32), (gt_starts, np.int32))
    return _evaluate_on_device(dets, counts, gt, ops.coco_eval_match, num_classes, MAX_DETS, summarize, device, times, accumulate)


def result_string(stats):
    """the twelve lines, in pycocotools' printed wording"""
    def line(ap, iou, area, max_det, value):
        return " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}\n".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area, max_det, value)
    span = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1])
    s, top = list(stats), MAX_DETS[-1]
    text = line(1, span, "all", top, s[0]) + line(1, "0.50", "all", top, s[1]) + line(1, "0.75", "all", top, s[2])
    text += "".join(line(1, span, AREA_NAMES[a], top, s[2 + a]) for a in (1, 2, 3))
    text += "".join(line(0, span, "all", m, s[6 + i]) for i, m in enumerate(MAX_DETS))
    text += "".join(line(0, span, AREA_NAMES[a], top, s[8 + a]) for a in (1, 2, 3))
    return text


def _do_evaluation(protocol, annotations_class, file_name, annotations, predictions, output_folder, device, logger, times, accumulate):
    """What do_coco_evaluation and do_lvis_evaluation do alike.  protocol: the module (this one or lvis_eval) with pack_groundtruth,
    evaluate_numpy, evaluate_device, result_string and STAT_NAMES; the text goes to output_folder/file_name"""
    check_accumulate(accumulate, device)
    ann = annotations if isinstance(annotations, annotations_class) else annotations_class(annotations)
    lap = _Laps(times, torch.device(device) if device is not None else torch.device("cpu"))
    counts, dets = pack_detections(predictions, ann.image_ids)
    live = torch.arange(dets.shape[1])[None, :] < counts[:, None]
    bad = live & ((dets[:, :, 5] < 1) | (dets[:, :, 5] > ann.num_classes))
    if bool(bad.any()):
        f, r = [int(v) for v in torch.nonzero(bad)[0]]
        raise ValueError("image id %d: label %d is outside 1 .. %d" % (ann.image_ids[f], int(dets[f, r, 5]), ann.num_classes))
    gt = protocol.pack_groundtruth(ann)
    lap("pack")
    if device is None:
        res = protocol.evaluate_numpy(dets, counts, *gt, max(1, ann.num_classes))
    else:
        res = protocol.evaluate_device(dets, counts, *gt, max(1, ann.num_classes), device=device, times=times, accumulate=accumulate)
    text = protocol.result_string(res["stats"])
    if logger is not None:
        logger.info("\n" + text)
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
        with open(os.path.join(output_folder, file_name), "w") as fid:
            fid.write(text)
    return OrderedDict(zip(protocol.STAT_NAMES, (float(v) for v in res["stats"])))


def do_coco_evaluation(annotations, predictions, output_folder=None, device=None, logger=None, times=None, accumulate="numpy"):
    """annotations: a CocoAnnotations, a path or a dict; predictions: {image id: BoxList} as engine.inference_images returns them (boxes
    xyxy in the original image's pixels, `scores`, `labels` 1 .. K in CocoAnnotations' order).  Every image of the annotations is
    evaluated, one without a prediction as an image without detections; a prediction for an image the annotations do not list, or a
    label outside 1 .. K, is an error.  -> an ordered dict of the twelve numbers (STAT_NAMES); the text goes to the logger and to
    `output_folder/coco_eval.txt`.  device: a torch.device runs the matching there and writes the same text; None is the numpy path.
    accumulate: "device" runs the accumulation on `device` too (evaluate_device) and writes the same text again."""
    return _do_evaluation(sys.modules[__name__], CocoAnnotations, "coco_eval.txt", annotations, predictions, output_folder, device, logger, times, accumulate)
