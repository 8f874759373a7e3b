"""The COCO bbox evaluator (data/evaluation/coco_eval.py) without a GPU: hand-computed answers, the numpy path against the loop-for-loop
restatement of the protocol in _coco_eval_ref.py (exactly), the cut at 100 rows per (image, category), and the interfaces around it.

A precision of "1" is 1 / (1 + np.spacing(1)) = 1 - 2^-52 in this protocol (the eps in the denominator), so the known answers that involve
a precision are compared within 1e-12; recalls, match flags and the comparison with the restatement are exact."""
import json
import os
import re

import numpy as np
import pytest
import torch

import _coco_eval_ref as C

from diffusionvid_amd.data.evaluation import coco_eval
from diffusionvid_amd.engine import inference as engine
from diffusionvid_amd.structures.bounding_box import BoxList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 1e-12
KNOWN = C.known_cases()


def _eval(case):
    return coco_eval.evaluate_numpy(case.dets, case.counts, *case.gt(), case.num_classes)


def _match(case):
    return coco_eval.match_numpy(case.dets, case.counts, *case.gt(), case.num_classes)


def _stats(case):
    return dict(zip(coco_eval.STAT_NAMES, _eval(case)["stats"]))


def _same(got, want):
    for k in ("precision", "recall", "stats"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


# ---- 1. known answers -------------------------------------------------------------------------------------------------------------------
def test_parameters_are_the_protocols():
    assert coco_eval.IOU_THRS.dtype == np.float64 and coco_eval.IOU_THRS.tolist() == C.IOU_THRS and len(C.IOU_THRS) == 10
    assert coco_eval.IOU_THRS[0] == 0.5 and coco_eval.IOU_THRS[5] == 0.75 and coco_eval.IOU_THRS[-1] == 0.95
    assert coco_eval.REC_THRS.tolist() == C.REC_THRS and len(C.REC_THRS) == 101
    assert coco_eval.MAX_DETS == (1, 10, 100) and coco_eval.AREA_RANGES == ((0, 1e10), (0, 1024), (1024, 9216), (9216, 1e10))


def test_one_perfect_detection():
    """One 50 x 50 box (area 2500: medium) and one row on it with IoU 1.  tp = [1], fp = [0]: recall 1 / 1 = 1, precision 1 / (0 + 1 + eps)
    at every recall threshold and every IoU threshold, so AP = AP50 = AP75 = APm = 1 and AR1 = AR10 = AR100 = ARm = 1.  No small and no
    large box exists (npig = 0 there), so APs, APl, ARs, ARl stay -1."""
    s = _stats(KNOWN["perfect"])
    for k in ("AP", "AP50", "AP75", "APm"):
        assert abs(s[k] - 1.0) <= NEAR, k
    for k in ("AR1", "AR10", "AR100", "ARm"):
        assert s[k] == 1.0, k
    for k in ("APs", "APl", "ARs", "ARl"):
        assert s[k] == -1.0, k


def test_a_hit_behind_a_higher_scored_miss():
    """Rows in score order: a miss (0.9), then a hit with IoU 1 (0.8); one box.  tp = [0, 1], fp = [1, 1], recall = [0, 1], precision =
    [0, 1 / 2]; the envelope from the back makes it [1 / 2, 1 / 2]; recall threshold 0 reads index 0, every other index 1: all 101 samples
    are 1 / 2.  AP50 = 0.5, and the same at every IoU threshold (the IoU is 1): AP = 0.5.  AR1 = 0 (the first row is the miss), AR10 = 1."""
    s = _stats(KNOWN["hit_and_miss"])
    assert abs(s["AP50"] - 0.5) <= NEAR and abs(s["AP"] - 0.5) <= NEAR
    assert s["AR1"] == 0.0 and s["AR10"] == 1.0 and s["AR100"] == 1.0


def test_iou_of_exactly_one_half():
    """[0, 0, 10, 10] against [0, 0, 10, 5]: overlap 10 x 5 = 50, union (50 + 100) - 50 = 100, IoU = 0.5 exactly.  `iou < best` with best =
    0.5 is false, so the row matches at threshold 0.5; at 0.55 and above 0.5 < best skips the box.  AP50 = 1, AP75 = 0, AP = 1 / 10."""
    match, ignore, rank, npig = _match(KNOWN["iou_half"])
    assert match[0, :, 0, 0].tolist() == [1] + [0] * 9 and rank[0, 0] == 0
    s = _stats(KNOWN["iou_half"])
    assert abs(s["AP50"] - 1.0) <= NEAR and s["AP75"] == 0.0 and abs(s["AP"] - 0.1) <= NEAR


def test_a_crowd_box_absorbs_detections():
    """A 100 x 100 crowd box and three 10 x 10 rows inside it: overlap 100, union = the row's own area 100, IoU = 1 -- with the ordinary
    union (100 + 10000) - 100 it would be 0.0099 and all three would be false positives.  Each takes the crowd box (a crowd box can be
    taken again) and is ignored.  The fourth row (lowest score) sits on the one counted box: tp = [1], fp = [0] after dropping the ignored
    rows, AP = AP50 = 1; with three false positives in front the precision would have been 1 / 4."""
    case = KNOWN["crowd"]
    match, ignore, rank, npig = _match(case)
    assert match[0, :, 0, :4].min() == 1 and ignore[0, :, 0, :3].min() == 1 and ignore[0, :, 0, 3].max() == 0
    assert npig[0].tolist() == [0, 1]
    s = _stats(case)
    assert abs(s["AP"] - 1.0) <= NEAR and abs(s["AP50"] - 1.0) <= NEAR and s["AR100"] == 1.0


def test_a_small_box_is_ignored_under_large():
    """A 10 x 10 box (area 100) and a row on it.  Under "large" (9216 .. 1e10) the box is ignored, the row still matches it and inherits
    the flag; under "small" and "all" it counts.  No counted box is large or medium: APl = APm = -1; APs = AP = 1."""
    match, ignore, rank, npig = _match(KNOWN["small_gt"])
    assert match[:, :, 0, 0].min() == 1
    assert ignore[3, :, 0, 0].min() == 1 and ignore[2, :, 0, 0].min() == 1 and ignore[1, :, 0, 0].max() == 0 and ignore[0, :, 0, 0].max() == 0
    assert npig[:, 1].tolist() == [1, 1, 0, 0]
    s = _stats(KNOWN["small_gt"])
    assert s["APl"] == -1.0 and s["APm"] == -1.0 and abs(s["APs"] - 1.0) <= NEAR and abs(s["AP"] - 1.0) <= NEAR


def test_an_unmatched_detection_outside_the_range_is_ignored():
    """A 10 x 10 row on nothing (score 0.95) in front of a hit on a 50 x 50 box (0.9).  Under "all" the first row is a false positive:
    tp = [0, 1], fp = [1, 1], AP = 1 / 2 as in the hit-and-miss case.  Under "medium" its area 100 lies outside 1024 .. 9216 and it is
    unmatched, so it is ignored: tp = [1], fp = [0], APm = 1."""
    match, ignore, rank, npig = _match(KNOWN["unmatched_outside"])
    assert match[:, :, 0, 1].max() == 0
    assert ignore[2, :, 0, 1].min() == 1 and ignore[3, :, 0, 1].min() == 1 and ignore[0, :, 0, 1].max() == 0 and ignore[1, :, 0, 1].max() == 0
    s = _stats(KNOWN["unmatched_outside"])
    assert abs(s["AP"] - 0.5) <= NEAR and abs(s["APm"] - 1.0) <= NEAR


def test_equal_iou_moves_to_the_later_box():
    """[0, 0, 10, 10] has IoU 50 / ((100 + 50) - 50) = 0.5 with its upper half [0, 0, 10, 5] and with its lower half [0, 5, 10, 5].  At
    threshold 0.5 the walk takes the upper half (0.5 >= 0.5), then the lower half (0.5 < 0.5 is false): the later box.  The second row
    IS the lower half: that box is taken, the upper half has IoU 0, so it stays unmatched -- had the first row kept the earlier box, the
    second would have matched with IoU 1.  From 0.55 on the first row matches nothing and the second takes the lower half."""
    match, ignore, rank, npig = _match(KNOWN["equal_iou"])
    assert match[0, 0, 0, :2].tolist() == [1, 0]
    assert all(match[0, t, 0, :2].tolist() == [0, 1] for t in range(1, 10))


# ---- 2. the break rule ------------------------------------------------------------------------------------------------------------------
def test_a_counted_match_does_not_move_to_a_better_ignored_box():
    """A 100 x 100 row, a counted 100 x 78 box (IoU 7800 / ((10000 + 7800) - 7800) = 0.78) and an identical crowd box annotated BEFORE it
    (IoU 10000 / 10000 = 1).  The counted box is walked first; at thresholds 0.5 .. 0.75 it matches and the walk stops at the crowd box
    although its IoU is greater: the row is a true positive.  At 0.8 .. 0.95 the counted box fails, the crowd box matches: the row is
    ignored, and with one counted box and no counted row the precision is 0.  AP = 6 / 10."""
    match, ignore, rank, npig = _match(KNOWN["break_rule"])
    assert match[0, :, 0, 0].tolist() == [1] * 10
    assert ignore[0, :, 0, 0].tolist() == [0] * 6 + [1] * 4
    s = _stats(KNOWN["break_rule"])
    assert abs(s["AP"] - 0.6) <= NEAR and abs(s["AP50"] - 1.0) <= NEAR and abs(s["AP75"] - 1.0) <= NEAR and abs(s["AR100"] - 0.6) <= 1e-15


# ---- 3. the numpy path is the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_cases_equal_the_restatement(name):
    _same(_eval(KNOWN[name]), C.evaluate(KNOWN[name]))
    for g, w in zip(_match(KNOWN[name]), C.matches(KNOWN[name])):
        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_cases_equal_the_restatement(seed):
    case = C.random_case(seed, max_gt=12, max_rows=110)
    for g, w in zip(_match(case), C.matches(case)):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    _same(_eval(case), C.evaluate(case))


# ---- 4. the cut at 100 per (image, category) --------------------------------------------------------------------------------------------
def test_the_101st_row_of_a_label_changes_nothing():
    """101 rows of one label; the one of lowest score sits on the only box.  It is the 101st in order: cut, so the box is never found
    (recall 0), exactly as if the row were not there.  With 100 rows the same row is the 100th and finds the box."""
    with_101 = C.cut_case(101)
    match, ignore, rank, npig = _match(with_101)
    assert rank[0, 0] == -1 and sorted(rank[0, 1:].tolist()) == list(range(100))
    without = C.Case(with_101.dets[:, 1:], [100], *with_101.gt(), 1)
    _same(_eval(with_101), _eval(without))
    assert _stats(with_101)["AR100"] == 0.0
    assert _match(C.cut_case(100))[2][0, 0] == 99 and _stats(C.cut_case(100))["AR100"] == 1.0


def test_recall_at_1_10_and_100_detections():
    """Eleven boxes; the rows at positions 0, 4, 9 and 10 of the score order hit one each (IoU 1, so at every threshold).  Among the first
    1, 10 and 100 rows that is 1, 3 and 4 of the 11 boxes.  (The mean of ten equal recalls may round in its last place: 1e-15.)"""
    s = _stats(C.ar_case())
    assert abs(s["AR1"] - 1 / 11) <= 1e-15 and abs(s["AR10"] - 3 / 11) <= 1e-15 and abs(s["AR100"] - 4 / 11) <= 1e-15
    assert _eval(C.ar_case())["recall"][:, 0, 0, :].tolist() == [[1 / 11, 3 / 11, 4 / 11]] * 10


# ---- 5. interfaces ------------------------------------------------------------------------------------------------------------------------
def _annotations():
    return {"images": [{"id": 7, "width": 640, "height": 480}, {"id": 3, "width": 500, "height": 400}, {"id": 11, "width": 100, "height": 100}],
            "categories": [{"id": 18, "name": "dog"}, {"id": 1, "name": "person"}, {"id": 90, "name": "toothbrush"}],
            "annotations": [{"id": 1, "image_id": 7, "category_id": 18, "bbox": [10, 10, 50, 50], "area": 2000.0, "iscrowd": 0},
                            {"id": 2, "image_id": 3, "category_id": 1, "bbox": [0, 0, 100, 100], "area": 9000.0, "iscrowd": 1},
                            {"id": 3, "image_id": 7, "category_id": 90, "bbox": [5.5, 6.5, 20, 30], "area": 410.0}]}


def _predictions():
    a = BoxList(torch.tensor([[10., 10., 60., 60.], [5.5, 6.5, 25.5, 36.5]]), (640, 480))
    a.add_field("scores", torch.tensor([0.9, 0.8]))
    a.add_field("labels", torch.tensor([2, 3]))
    b = BoxList(torch.tensor([[0., 0., 10., 10.]]), (500, 400))
    b.add_field("scores", torch.tensor([0.7]))
    b.add_field("labels", torch.tensor([1]))
    return {7: a, 3: b}


def test_annotations_load_from_a_file_and_map_categories(tmp_path):
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(_annotations()))
    for source in (str(path), _annotations()):
        ann = coco_eval.CocoAnnotations(source)
        assert ann.image_ids == [3, 7, 11] and ann.num_classes == 3
        assert ann.label_of == {1: 1, 18: 2, 90: 3} and ann.category_of == {1: 1, 2: 18, 3: 90} and ann.names[2] == "dog"
        boxes, areas, crowd, labels, starts = coco_eval.pack_groundtruth(ann)
        assert boxes.dtype == areas.dtype == np.float64 and starts.tolist() == [0, 1, 3, 3]
        assert boxes.tolist() == [[0, 0, 100, 100], [10, 10, 50, 50], [5.5, 6.5, 20, 30]]
        assert areas.tolist() == [9000.0, 2000.0, 410.0] and crowd.tolist() == [1, 0, 0] and labels.tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="image 99"):
        coco_eval.CocoAnnotations(dict(_annotations(), annotations=[{"id": 5, "image_id": 99, "category_id": 1, "bbox": [0, 0, 1, 1]}]))


def test_coco_results_round_trip_through_the_inverse_map():
    ann = coco_eval.CocoAnnotations(_annotations())
    res = engine.coco_results(_predictions(), ann.category_of)
    assert [r["category_id"] for r in res] == [1, 18, 90] and [r["image_id"] for r in res] == [3, 7, 7]
    assert [ann.label_of[r["category_id"]] for r in res] == [1, 2, 3]
    assert res[2]["bbox"] == [5.5, 6.5, 20.0, 30.0]


def test_do_coco_evaluation_scores_and_writes_the_text(tmp_path):
    """Image 7: both rows sit exactly on their boxes (labels 2 and 3): AP 1 for both categories.  Image 3: label 1 has only a crowd box,
    its row is absorbed and the category has no counted box (-1).  Image 11 has neither.  Mean over the two categories: 1."""
    stats = coco_eval.do_coco_evaluation(_annotations(), _predictions(), str(tmp_path))
    assert list(stats) == list(coco_eval.STAT_NAMES)
    assert abs(stats["AP"] - 1.0) <= NEAR and stats["AR100"] == 1.0 and stats["APl"] == -1.0
    lines = (tmp_path / "coco_eval.txt").read_text().splitlines()
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 1.000"
    assert lines[5] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 1.000"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"
    extra = dict(_predictions())
    extra[5] = extra[3]
    with pytest.raises(ValueError, match="image id 5"):
        coco_eval.do_coco_evaluation(_annotations(), extra)
    bad = _predictions()
    bad[3].add_field("labels", torch.tensor([4]))
    with pytest.raises(ValueError, match=r"image id 3: label 4 is outside 1 \.\. 3"):
        coco_eval.do_coco_evaluation(_annotations(), bad)


class _StubModel:
    def detect_images(self, images, image_ids):
        preds = _predictions()
        return [preds[int(i)] for i in image_ids]


def test_inference_images_without_annotations_is_unchanged(tmp_path):
    loader = [(None, [7], [(640, 480)]), (None, [3], [(500, 400)])]
    out = engine.inference_images(_StubModel(), loader, str(tmp_path / "plain"))
    assert isinstance(out, dict) and sorted(out) == [3, 7] and torch.equal(out[7].bbox, _predictions()[7].bbox)
    assert sorted(os.listdir(tmp_path / "plain")) == ["coco_results.json", "predictions.pth"]
    assert [r["category_id"] for r in json.load(open(tmp_path / "plain" / "coco_results.json"))] == [1, 2, 3]


def test_inference_images_with_annotations_returns_the_stats(tmp_path):
    loader = [(None, [7], [(640, 480)]), (None, [3], [(500, 400)])]
    preds, stats = engine.inference_images(_StubModel(), loader, str(tmp_path), annotations=_annotations())
    assert sorted(preds) == [3, 7] and list(stats) == list(coco_eval.STAT_NAMES) and abs(stats["AP"] - 1.0) <= NEAR
    assert [r["category_id"] for r in json.load(open(tmp_path / "coco_results.json"))] == [1, 18, 90]
    assert os.path.exists(tmp_path / "coco_eval.txt")
    ann = dict(_annotations(), images=_annotations()["images"][:1], annotations=_annotations()["annotations"][:1])
    with pytest.raises(ValueError, match="image id 3"):
        engine.inference_images(_StubModel(), loader, annotations=ann)


def test_library_header_and_binding_carry_the_entry():
    from diffusionvid_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    assert "int dvid_coco_eval_match(" in header
    assert int(re.search(r"#define DVID_COCO_EVAL_MAX_GT (\d+)", header).group(1)) == ops.COCO_EVAL_MAX_GT >= 256
    assert int(re.search(r"#define DVID_COCO_EVAL_THRESHOLDS (\d+)", header).group(1)) == ops.COCO_EVAL_THRESHOLDS == len(coco_eval.IOU_THRS)
    assert int(re.search(r"#define DVID_COCO_EVAL_AREAS (\d+)", header).group(1)) == ops.COCO_EVAL_AREAS == len(coco_eval.AREA_RANGES)
    assert int(re.search(r"#define DVID_COCO_EVAL_MAX_DETS (\d+)", header).group(1)) == ops.COCO_EVAL_MAX_DETS == coco_eval.MAX_DETS[-1]
    assert "dvid_coco_eval_match" in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdvid_hip.so is not built")
    lib = _lib.load()
    assert lib.dvid_version() >= 6 and lib.dvid_coco_eval_match.argtypes == _lib.SIGNATURES["dvid_coco_eval_match"][1]
    assert header.split("int dvid_coco_eval_match(")[1].split(");")[0].count(",") + 1 == len(lib.dvid_coco_eval_match.argtypes)
