"""LVIS bbox evaluation, the federated protocol: the thirteen numbers from engine.inference_images' predictions and an LVIS annotation file.
numpy by default; with `device` the matching runs on the GPU (ops.lvis_eval_match, csrc/lviseval.hip), as coco_eval does for COCO.

LVIS annotates every image for a SUBSET of its 1203 categories, so the COCO protocol on an LVIS file counts every detection of a category
that nobody looked for as a false positive.  This module states the LVIS protocol itself, from its published definition, with neither
`lvis` nor `pycocotools`:

  file         COCO-style JSON; every image carries `neg_category_ids` (looked for, not there) and `not_exhaustive_category_ids` (there,
               but not every instance is boxed); every category carries `frequency` "r" / "c" / "f"; annotations have no `iscrowd` and may
               have `ignore`
  parameters   coco_eval's IoU thresholds, recall thresholds and area ranges; ONE detection limit, 300 per IMAGE
  per image    the 300 rows of highest score over all categories (stable: of equal scores the earlier row; -0 and +0 are one score); of
               those, a row whose category is neither a category of one of the image's annotations (the positive set) nor in
               `neg_category_ids` is dropped: nobody looked.  No further cut per category
  matching     per (image, category, area range): a box is ignored when its `ignore` is set or its area lies outside the range (both ends
               inclusive); boxes ordered not ignored first; rows in descending score (stable); coco_eval's IoU without the crowd case; per
               threshold every row takes the box of greatest IoU >= min(t, 1 - 1e-10) that no earlier row took, the later box on equal
               IoU, and does not leave a not ignored match for an ignored box.  A row matched to an ignored box does not count; an
               unmatched row does not count when its own area lies outside the range OR its category is in the image's
               `not_exhaustive_category_ids`; a matched row in such a category counts as any other
  accumulate   coco_eval.accumulate_arrays with the one limit 300
  summarize    AP AP50 AP75 APs APm APl, AP over the rare / common / frequent categories alone, AR@300 and its three sizes; each the
               mean over the entries > -1, or -1 without any

Both paths produce (match, ignore, rank, npig) in coco_eval's layout and share the accumulation, so their results are equal, not close.
Not here: segmentation masks, the `ignore`-region variants of the protocol, evaluation spread over ranks."""
import json
import sys

import numpy as np
import torch

from . import coco_eval
from .coco_eval import AREA_NAMES, AREA_RANGES, IOU_THRS, REC_THRS, _ious, _mean, _np, _xywh, pack_detections          # noqa: F401

MAX_DETS = 300
FREQUENCIES = ("r", "c", "f")
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf", "AR@300", "ARs@300", "ARm@300", "ARl@300")
LVIS_IMAGE_KEYS = ("neg_category_ids", "not_exhaustive_category_ids")


def is_lvis(data):
    """does this annotation dict speak LVIS: do its images carry `neg_category_ids`"""
    return any("neg_category_ids" in im for im in data.get("images", ()))


class LvisAnnotations(coco_eval.CocoAnnotations):
    """CocoAnnotations of an LVIS file, with neg_of / nex_of: image id -> the labels of its `neg_category_ids` /
    `not_exhaustive_category_ids`, in file order, and frequency_of: label -> "r" / "c" / "f".  An image without one of the two lists, a
    category without `frequency` and a list that names an unknown category are errors that name the image or the category."""

    def __init__(self, json_file_or_dict):
        data = json_file_or_dict
        if not isinstance(data, dict):
            with open(data) as f:
                data = json.load(f)
        super().__init__(data)
        self.frequency_of = {}
        for c in data.get("categories", ()):
            if c.get("frequency") not in FREQUENCIES:
                raise ValueError("category %d has no `frequency` of 'r', 'c' or 'f' (%r): not an LVIS annotation file" % (int(c["id"]), c.get("frequency")))
            self.frequency_of[self.label_of[int(c["id"])]] = c["frequency"]
        self.neg_of, self.nex_of = {}, {}
        for image_id in self.image_ids:
            im = self.images[image_id]
            for key, table in zip(LVIS_IMAGE_KEYS, (self.neg_of, self.nex_of)):
                if not isinstance(im.get(key), (list, tuple)):
                    raise ValueError("image %d has no list `%s`: not an LVIS annotation file" % (image_id, key))
                for cat in im[key]:
                    if int(cat) not in self.label_of:
                        raise ValueError("image %d: `%s` names category %d, which the file does not list" % (image_id, key, int(cat)))
                table[image_id] = [self.label_of[int(cat)] for cat in im[key]]


def _csr(lists):
    starts = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=starts[1:])
    assert int(starts[-1]) < 2 ** 31, "the lists are indexed with int32"
    flat = np.asarray([v for l in lists for v in l], dtype=np.int32).reshape(-1)
    return starts.astype(np.int32), flat


def pack_groundtruth(ann, image_ids=None):
    """-> (boxes [G, 4] float64 xywh, areas [G] float64, ignore [G] uint8, labels [G] int32, starts [N + 1] int32, neg_starts [N + 1] int32,
    neg_labels int32, nex_starts [N + 1] int32, nex_labels int32, frequency [K + 1] of "", "r", "c", "f" by label): coco_eval's layout with
    the annotation's `ignore` where it has the crowd byte, the images' negative and not-exhaustive lists as CSR tables, and every label's
    frequency."""
    image_ids = ann.image_ids if image_ids is None else list(image_ids)
    boxes, areas, _, labels, starts = coco_eval.pack_groundtruth(ann, image_ids)
    flagged = np.asarray([1 if a.get("ignore", 0) else 0 for i in image_ids for a in ann.anns_of[i]], dtype=np.uint8).reshape(-1)
    neg_starts, neg_labels = _csr([ann.neg_of[i] for i in image_ids])
    nex_starts, nex_labels = _csr([ann.nex_of[i] for i in image_ids])
    frequency = np.array([""] + [ann.frequency_of[l] for l in range(1, ann.num_classes + 1)])
    return boxes, areas, flagged, labels, starts, neg_starts, neg_labels, nex_starts, nex_labels, frequency


def _score_key(scores):
    """what the stable descending sorts order by: -0 and +0 are one score"""
    return -(scores.astype(np.float32) + np.float32(0))


def _label_set(labels, num_classes):
    """[num_classes + 1] bool; a label outside 0 .. num_classes is in no set"""
    out = np.zeros(num_classes + 1, dtype=bool)
    out[labels[(labels >= 0) & (labels <= num_classes)]] = True
    return out


def match_numpy(dets, counts, gt_boxes, gt_areas, gt_ignore, gt_labels, gt_starts, neg_starts, neg_labels, nex_starts, nex_labels, num_classes):
    """The matching, in the layout of ops.lvis_eval_match: (match [4, 10, N, cap] int8, ignore [4, 10, N, cap] int8, rank [N, cap] int32,
    npig [4, num_classes + 1] int32).  Vectorised over the thresholds; images, labels, area ranges, detections and boxes are loops."""
    dets, counts = _np(dets, np.float32), _np(counts, np.int64)
    gt_boxes, gt_areas, gt_ignore = _np(gt_boxes, np.float64).reshape(-1, 4), _np(gt_areas, np.float64), _np(gt_ignore).astype(bool)
    gt_labels, gt_starts = _np(gt_labels, np.int64), _np(gt_starts, np.int64)
    neg_starts, neg_labels = _np(neg_starts, np.int64), _np(neg_labels, np.int64)
    nex_starts, nex_labels = _np(nex_starts, np.int64), _np(nex_labels, np.int64)
    N, cap = dets.shape[:2]
    match, ignore, rank, npig, gig_all = coco_eval._match_setup(N, cap, gt_ignore, gt_areas, gt_labels, num_classes)
    for f in range(N):
        n = int(min(max(counts[f], 0), cap))
        if n == 0:
            continue
        rows = dets[f, :n]
        x, y, w, h, area = _xywh(rows)
        lab = np.where((rows[:, 5] >= 0) & (rows[:, 5] <= num_classes), rows[:, 5], -1).astype(np.int64)
        g0, g1 = int(gt_starts[f]), int(gt_starts[f + 1])
        # the image's 300, then the rows somebody looked for
        cand = np.nonzero(lab >= 0)[0]
        cand = cand[np.argsort(_score_key(rows[cand, 4]), kind="mergesort")[:MAX_DETS]]
        listed = _label_set(gt_labels[g0:g1], num_classes) | _label_set(neg_labels[neg_starts[f]:neg_starts[f + 1]], num_classes)
        nex = _label_set(nex_labels[nex_starts[f]:nex_starts[f + 1]], num_classes)
        cand = cand[listed[lab[cand]]]          # still in descending score
        d_out = np.stack([(area < lo) | (area > hi) for lo, hi in AREA_RANGES])          # [A, n]
        for l in np.unique(lab[cand]):
            sel = cand[lab[cand] == l]
            rank[f, sel] = np.arange(len(sel))
            gi = g0 + np.nonzero(gt_labels[g0:g1] == l)[0]
            coco_eval._match_label(match, ignore, f, sel, (x, y, w, h), gt_boxes[gi], gig_all[:, gi], np.zeros(len(gi), dtype=bool), d_out | nex[l])
    return match, ignore, rank, npig


def summarize(precision, recall, frequency):
    """the thirteen numbers, in STAT_NAMES' order; precision [10, 101, K, 4, 1], recall [10, K, 4, 1], frequency [K + 1] by label"""
    t50, t75 = int(np.where(IOU_THRS == .5)[0][0]), int(np.where(IOU_THRS == .75)[0][0])
    frequency = np.asarray(frequency)[1:]
    stats = [_mean(precision[:, :, :, 0, 0]), _mean(precision[t50, :, :, 0, 0]), _mean(precision[t75, :, :, 0, 0])]
    stats += [_mean(precision[:, :, :, a, 0]) for a in (1, 2, 3)]
    stats += [_mean(precision[:, :, np.nonzero(frequency == fr)[0], 0, 0]) for fr in FREQUENCIES]
    stats += [_mean(recall[:, :, a, 0]) for a in (0, 1, 2, 3)]
    return np.array(stats)


def accumulate_from_matches(scores, labels, counts, rank, match, ignore, npig, frequency):
    """coco_eval.accumulate_arrays with the one limit 300 + summarize -> {"precision" [10, 101, K, 4, 1], "recall" [10, K, 4, 1], "stats"}"""
    precision, recall = coco_eval.accumulate_arrays(scores, labels, counts, rank, match, ignore, npig, (MAX_DETS,))
    return {"precision": precision, "recall": recall, "stats": summarize(precision, recall, frequency)}


def _tail(dets, counts, rank, match, ignore, npig, frequency):
    host = _np(dets[:, :, 4:6])
    return accumulate_from_matches(np.ascontiguousarray(host[:, :, 0]), host[:, :, 1].astype(np.int64), counts, rank, match, ignore, npig, frequency)


def _frequency(frequency, num_classes):
    """None: every category is frequent"""
    return np.array([""] + ["f"] * num_classes) if frequency is None else np.asarray(frequency)


def evaluate_numpy(dets, counts, gt_boxes, gt_areas, gt_ignore, gt_labels, gt_starts, neg_starts, neg_labels, nex_starts, nex_labels, frequency,
                   num_classes):
    """The whole protocol in numpy on engine.pack_predictions' arrays (dets [N, cap, 6] fp32 xyxy / score / label, counts [N]; images in
    ascending id) and pack_groundtruth's -> accumulate_from_matches' dict."""
    dets = torch.as_tensor(_np(dets, np.float32))
    if dets.shape[1] == 0:          # no detection at all: the ground truth still counts
        dets = dets.new_zeros((dets.shape[0], 1, 6))
    got = match_numpy(dets, counts, gt_boxes, gt_areas, gt_ignore, gt_labels, gt_starts, neg_starts, neg_labels, nex_starts, nex_labels, num_classes)
    return _tail(dets, counts, got[2], got[0], got[1], got[3], _frequency(frequency, num_classes))


def evaluate_device(dets, counts, gt_boxes, gt_areas, gt_ignore, gt_labels, gt_starts, neg_starts, neg_labels, nex_starts, nex_labels, frequency,
                    num_classes, device=None, times=None, accumulate="numpy"):
    """evaluate_numpy with the matching as one kernel call on `device` (default: where dets is); the accumulation is the same numpy
    code on the same arrays, so the result is equal.  times: see vid_eval._Laps (copy_in, kernel, copy_out, tail).
    accumulate "device": as coco_eval.evaluate_device, with the one limit 300 (laps copy_in, kernel, accumulate, copy_out, tail)."""
    from ... import ops
    gt = ((gt_boxes, np.float64), (gt_areas, np.float64), (gt_ignore, np.uint8), (gt_labels, np.int32), (gt_starts, np.int32),
          (neg_starts, np.int32), (neg_labels, np.int32), (nex_starts, np.int32), (nex_labels, np.int32))
    return coco_eval._evaluate_on_device(dets, counts, gt, ops.lvis_eval_match, num_classes, (MAX_DETS,),
                                         lambda precision, recall: summarize(precision, recall, _frequency(frequency, num_classes)), device, times,
                                         accumulate)


def result_string(stats):
    """the thirteen lines, in the LVIS API's printed wording"""
    def line(ap, iou, area, cats, value):
        return " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} catIds={:>3s}] = {:0.3f}\n".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area, MAX_DETS, cats, value)
    span = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1])
    s = list(stats)
    text = line(1, span, "all", "all", s[0]) + line(1, "0.50", "all", "all", s[1]) + line(1, "0.75", "all", "all", s[2])
    text += "".join(line(1, span, AREA_NAMES[a], "all", s[2 + a]) for a in (1, 2, 3))
    text += "".join(line(1, span, "all", fr, s[6 + i]) for i, fr in enumerate(FREQUENCIES))
    text += "".join(line(0, span, AREA_NAMES[a], "all", s[9 + a]) for a in (0, 1, 2, 3))
    return text


def lvis_results(predictions, label_map=None):
    """engine.coco_results of every image's MAX_DETS rows of highest score (stable), the LVIS result format: image_id, category_id, bbox
    xywh, score"""
    from ...engine.inference import coco_results
    top = {}
    for image_id, bl in predictions.items():
        scores = bl.get_field("scores").detach().cpu().numpy()
        if len(scores) > MAX_DETS:
            keep = np.sort(np.argsort(_score_key(scores), kind="mergesort")[:MAX_DETS])
            bl = bl[torch.from_numpy(keep)]
        top[image_id] = bl
    return coco_results(top, label_map)


def do_lvis_evaluation(annotations, predictions, output_folder=None, device=None, logger=None, times=None, accumulate="numpy"):
    """annotations: an LvisAnnotations, a path or a dict; predictions: {image id: BoxList} as engine.inference_images returns them (boxes
    xyxy in the original image's pixels, `scores`, `labels` 1 .. K in the annotations' order).  Every image of the annotations is
    evaluated, one without a prediction as an image without detections; a prediction for an image the annotations do not list, or a
    label outside 1 .. K, is an error.  -> an ordered dict of the thirteen numbers (STAT_NAMES); the text goes to the logger and to
    `output_folder/lvis_eval.txt`.  device: a torch.device runs the matching there and writes the same text; None is the numpy path.
    accumulate: "device" runs the accumulation on `device` too (evaluate_device) and writes the same text again."""
    return coco_eval._do_evaluation(sys.modules[__name__], LvisAnnotations, "lvis_eval.txt", annotations, predictions, output_folder, device, logger,
                                    times, accumulate)
