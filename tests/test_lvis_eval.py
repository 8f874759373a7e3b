"""The LVIS bbox evaluator (data/evaluation/lvis_eval.py, the federated protocol) without a GPU: the numpy path against the list-by-list
restatement in _lvis_eval_ref.py (exactly), hand-worked cases, one per rule (their arithmetic stands beside the cases in
_lvis_eval_ref.py), the COCO evaluator as a yardstick where the two protocols must agree, and the interfaces around it.

A precision of "1" is 1 / (1 + np.spacing(1)) = 1 - 2^-52 in this protocol (the eps in the denominator), so the known answers that involve
a precision are compared within 1e-12; recalls, match flags and the comparison with the restatement are exact."""
import copy
import json
import os
import re

import numpy as np
import pytest
import torch

import _lvis_eval_ref as L

from diffusionvid_amd.data.evaluation import coco_eval, lvis_eval
from diffusionvid_amd.engine import inference as engine
from diffusionvid_amd.structures.bounding_box import BoxList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 1e-12
KNOWN = L.known_cases()


def _eval(case):
    p = case.packed()
    return lvis_eval.evaluate_numpy(*p, case.num_classes)


def _match(case):
    p = case.packed()
    return lvis_eval.match_numpy(*p[:11], case.num_classes)


def _stats(case):
    return dict(zip(lvis_eval.STAT_NAMES, _eval(case)["stats"]))


def _same(got, want):
    """lvis_eval's dict (a trailing axis of one detection limit) against the restatement's"""
    assert got["precision"].shape == want["precision"].shape + (1,) and np.array_equal(got["precision"][..., 0], want["precision"])
    assert got["recall"].shape == want["recall"].shape + (1,) and np.array_equal(got["recall"][..., 0], want["recall"])
    assert got["stats"].shape == (13,) and np.array_equal(got["stats"], want["stats"])


def _same_matches(got, want):
    for name, g, w in zip(("match", "ignore", "rank", "npig"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


# ---- 1. the numpy path is the restatement --------------------------------------------------------------------------------------------------
def test_parameters_are_the_protocols():
    assert lvis_eval.IOU_THRS.tolist() == L.IOU_THRS and lvis_eval.REC_THRS.tolist() == L.REC_THRS
    assert lvis_eval.AREA_RANGES == L.AREA_RANGES and lvis_eval.MAX_DETS == L.MAX_DETS == 300
    assert lvis_eval.STAT_NAMES == L.STAT_NAMES and len(lvis_eval.STAT_NAMES) == 13
    assert lvis_eval.pack_detections is coco_eval.pack_detections


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_cases_equal_the_restatement_and_their_hand_worked_answers(name):
    case, answers = KNOWN[name]
    _same_matches(_match(case), L.matches(case))
    got = _eval(case)
    _same(got, L.evaluate(case))
    s = dict(zip(lvis_eval.STAT_NAMES, got["stats"]))
    for k, v in answers.items():
        assert abs(s[k] - v) <= NEAR, (k, s[k], v)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_random_cases_equal_the_restatement(seed):
    case = L.random_case(seed)
    _same_matches(_match(case), L.matches(case))
    _same(_eval(case), L.evaluate(case))


# ---- 2. one case per rule ------------------------------------------------------------------------------------------------------------------
def _as_coco(case):
    """the case's arrays for coco_eval: no box is crowd"""
    p = case.packed()
    return p[0], p[1], p[2], p[3], np.zeros(len(p[3]), dtype=np.uint8), p[5], p[6]


def test_a_detection_of_a_category_nobody_looked_for_vanishes():
    """unlisted_vanishes: the row of category 2 on image 0 gets rank -1, match 0, ignore 0 and AP is 1; the COCO protocol on the same
    arrays keeps it as a false positive and gives category 2 AP 1/2, AP 3/4.  In the image's negative list it counts here too."""
    case = KNOWN["unlisted_vanishes"][0]
    match, ignore, rank, npig = _match(case)
    assert rank[0].tolist() == [0, -1] and match[:, :, 0, 1].max() == 0 and ignore[:, :, 0, 1].max() == 0
    assert abs(_stats(case)["AP"] - 1.0) <= NEAR
    coco = coco_eval.evaluate_numpy(*_as_coco(case), case.num_classes)
    assert abs(coco["stats"][0] - 0.75) <= NEAR and coco_eval.match_numpy(*_as_coco(case), case.num_classes)[2][0].tolist() == [0, 0]
    listed = KNOWN["negative_counts"][0]
    assert _match(listed)[2][0].tolist() == [0, 0] and abs(_stats(listed)["AP"] - 0.75) <= NEAR


def test_not_exhaustive_ignores_an_unmatched_detection_and_counts_a_matched_one():
    match, ignore, rank, npig = _match(KNOWN["not_exhaustive_miss"][0])
    assert match[0, :, 0, 0].max() == 0 and ignore[:, :, 0, 0].min() == 1          # the miss: ignored under every range and threshold
    assert match[0, :, 0, 1].min() == 1 and ignore[0, :, 0, 1].max() == 0          # the hit: counts
    assert abs(_stats(KNOWN["not_exhaustive_miss"][0])["AP"] - 1.0) <= NEAR
    match, ignore, rank, npig = _match(KNOWN["exhaustive_miss"][0])
    assert ignore[0, :, 0, 0].max() == 0 and abs(_stats(KNOWN["exhaustive_miss"][0])["AP"] - 0.5) <= NEAR


@pytest.mark.parametrize("on_box", [0, 1])
def test_the_301st_detection_of_an_image_falls_out_and_a_tie_keeps_the_lower_row(on_box):
    case = L.cut_case(on_box)
    match, ignore, rank, npig = _match(case)
    assert rank[0, 0] == 299 and rank[0, 1] == -1 and sorted(rank[0, 2:].tolist()) == list(range(299))
    assert match[:, :, 0, 1].max() == 0 and ignore[:, :, 0, 1].max() == 0
    assert _stats(case)["AR@300"] == (1.0 if on_box == 0 else 0.0)
    _same(_eval(case), L.evaluate(case))
    if on_box == 1:          # exactly as if the row were not there
        without = copy.deepcopy(case)
        del without.images[0]["rows"][1]
        a, b = _eval(case), _eval(without)
        assert np.array_equal(a["precision"], b["precision"]) and np.array_equal(a["recall"], b["recall"])


def test_101_rows_of_one_label_are_all_evaluated():
    """the row of lowest score sits on the box: place 100 of its label, which the COCO protocol cuts and this one evaluates"""
    case = L.long_segment_case(101)
    match, ignore, rank, npig = _match(case)
    assert rank[0, 0] == 100 and match[0, :, 0, 0].min() == 1 and sorted(rank[0].tolist()) == list(range(101))
    assert _stats(case)["AR@300"] == 1.0
    assert coco_eval.match_numpy(*_as_coco(case), 1)[2][0, 0] == -1
    _same_matches(_match(case), L.matches(case))


def test_each_frequency_group_sees_only_its_categories():
    case, answers = KNOWN["frequency_groups"]
    s = _stats(case)
    assert abs(s["APr"] - 1.0) <= NEAR and abs(s["APc"] - 0.75) <= NEAR and s["APf"] == -1.0 and abs(s["AP"] - 5 / 6) <= NEAR
    swapped = L.Case(case.images, 3, {1: "f", 2: "r", 3: "f"})
    s = _stats(swapped)
    assert abs(s["APr"] - 0.5) <= NEAR and s["APc"] == -1.0 and abs(s["APf"] - 1.0) <= NEAR


def test_an_annotation_with_ignore_is_ignored():
    case = KNOWN["ignore_flag"][0]
    match, ignore, rank, npig = _match(case)
    assert npig[:, 1].tolist() == [1, 0, 1, 0]
    assert match[0, :, 0, 0].min() == 1 and ignore[0, :, 0, 0].min() == 1          # on the ignored box: matched, does not count
    assert match[0, :, 0, 1].min() == 1 and ignore[0, :, 0, 1].max() == 0
    assert abs(_stats(case)["AP"] - 1.0) <= NEAR


# ---- 3. the yardstick from existing code ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_where_the_protocols_agree_the_coco_evaluator_gives_the_same(seed):
    """Every category in every image's positive-or-negative set, nothing not-exhaustive, nothing ignored, at most 100 rows per image:
    neither protocol's own rules apply, so the matching equals coco_eval's and so do the six numbers both report."""
    case = L.random_case(seed, max_rows=100)
    for im in case.images:
        im["neg"], im["nex"] = list(range(1, case.num_classes + 1)), []
        for b in im["boxes"]:
            b["ignore"] = 0
    assert max(len(im["rows"]) for im in case.images) <= 100
    _same_matches(_match(case), coco_eval.match_numpy(*_as_coco(case), case.num_classes))
    want = coco_eval.evaluate_numpy(*_as_coco(case), case.num_classes)["stats"]
    got = _eval(case)["stats"]
    assert np.array_equal(got[:6], want[:6]) and (want[:3] > 0).all()
    assert got[9] == want[8] and np.array_equal(got[10:], want[9:])          # AR@300 is AR100 here, and its three sizes


# ---- 4. interfaces -------------------------------------------------------------------------------------------------------------------------
def _annotations():
    return {"images": [{"id": 7, "width": 640, "height": 480, "neg_category_ids": [90], "not_exhaustive_category_ids": []},
                       {"id": 3, "width": 500, "height": 400, "neg_category_ids": [], "not_exhaustive_category_ids": [1]}],
            "categories": [{"id": 18, "name": "dog", "frequency": "c"}, {"id": 1, "name": "person", "frequency": "f"},
                           {"id": 90, "name": "toothbrush", "frequency": "r"}],
            "annotations": [{"id": 1, "image_id": 7, "category_id": 18, "bbox": [10, 10, 50, 50], "area": 2000.0},
                            {"id": 2, "image_id": 3, "category_id": 1, "bbox": [0, 0, 100, 100], "area": 9000.0, "ignore": 1}]}


def _coco_annotations():
    ann = _annotations()
    ann["images"] = [{k: v for k, v in im.items() if not k.endswith("category_ids")} for im in ann["images"]]
    return ann


def _predictions():
    a = BoxList(torch.tensor([[10., 10., 60., 60.], [5.5, 6.5, 25.5, 36.5]]), (640, 480))
    a.add_field("scores", torch.tensor([0.9, 0.8]))
    a.add_field("labels", torch.tensor([2, 3]))
    b = BoxList(torch.tensor([[0., 0., 10., 10.]]), (500, 400))
    b.add_field("scores", torch.tensor([0.7]))
    b.add_field("labels", torch.tensor([1]))
    return {7: a, 3: b}


def test_annotations_load_validate_and_pack(tmp_path):
    path = tmp_path / "lvis.json"
    path.write_text(json.dumps(_annotations()))
    for source in (str(path), _annotations()):
        ann = lvis_eval.LvisAnnotations(source)
        assert isinstance(ann, coco_eval.CocoAnnotations) and ann.image_ids == [3, 7] and ann.label_of == {1: 1, 18: 2, 90: 3}
        assert ann.frequency_of == {1: "f", 2: "c", 3: "r"} and ann.neg_of == {3: [], 7: [3]} and ann.nex_of == {3: [1], 7: []}
        boxes, areas, flagged, labels, starts, neg_starts, neg_labels, nex_starts, nex_labels, frequency = lvis_eval.pack_groundtruth(ann)
        assert boxes.tolist() == [[0, 0, 100, 100], [10, 10, 50, 50]] and areas.tolist() == [9000.0, 2000.0]
        assert flagged.dtype == np.uint8 and flagged.tolist() == [1, 0] and labels.tolist() == [1, 2] and starts.tolist() == [0, 1, 2]
        assert (neg_starts.tolist(), neg_labels.tolist(), nex_starts.tolist(), nex_labels.tolist()) == ([0, 0, 1], [3], [0, 1, 1], [1])
        assert neg_starts.dtype == neg_labels.dtype == nex_starts.dtype == nex_labels.dtype == np.int32
        assert frequency.tolist() == ["", "f", "c", "r"]


def test_a_file_that_lacks_an_lvis_key_raises_and_names_the_culprit():
    bad = _annotations()
    del bad["categories"][2]["frequency"]
    with pytest.raises(ValueError, match=r"category 90 has no `frequency`"):
        lvis_eval.LvisAnnotations(bad)
    bad = _annotations()
    del bad["images"][0]["not_exhaustive_category_ids"]
    with pytest.raises(ValueError, match=r"image 7 has no list `not_exhaustive_category_ids`"):
        lvis_eval.LvisAnnotations(bad)
    bad = _annotations()
    del bad["images"][1]["neg_category_ids"]
    with pytest.raises(ValueError, match=r"image 3 has no list `neg_category_ids`"):
        lvis_eval.LvisAnnotations(bad)
    bad = _annotations()
    bad["images"][0]["neg_category_ids"] = [55]
    with pytest.raises(ValueError, match=r"image 7: `neg_category_ids` names category 55"):
        lvis_eval.LvisAnnotations(bad)
    with pytest.raises(ValueError, match=r"category 1 has no `frequency`"):
        lvis_eval.LvisAnnotations(_coco_annotations() | {"categories": [{"id": 1, "name": "person"}], "annotations": []})


def test_do_lvis_evaluation_scores_and_writes_the_text(tmp_path):
    """Image 7: the row of label 2 (dog) sits on its box: AP 1.  The row of label 3 (toothbrush) is on nothing, and toothbrush is in the
    image's negative list, so it is a false positive -- but the category has no box anywhere, so it has no AP.  Image 3: person's only
    box has `ignore`: no counted box, no AP.  One category has numbers, dog (common): AP = APc = 1, APr = APf = -1."""
    stats = lvis_eval.do_lvis_evaluation(_annotations(), _predictions(), str(tmp_path))
    assert list(stats) == list(lvis_eval.STAT_NAMES)
    assert abs(stats["AP"] - 1.0) <= NEAR and abs(stats["APc"] - 1.0) <= NEAR and stats["APr"] == -1.0 and stats["APf"] == -1.0
    assert stats["AR@300"] == 1.0 and stats["ARl@300"] == -1.0
    lines = (tmp_path / "lvis_eval.txt").read_text().splitlines()
    assert len(lines) == 13
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=all] = 1.000"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=300 catIds=all] = 1.000"
    assert lines[2] == " Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=300 catIds=all] = 1.000"
    assert lines[5] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=300 catIds=all] = -1.000"
    assert lines[6] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=  r] = -1.000"
    assert lines[7] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=  c] = 1.000"
    assert lines[8] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=  f] = -1.000"
    assert lines[9] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=all] = 1.000"
    assert lines[12] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=300 catIds=all] = -1.000"
    extra = dict(_predictions())
    extra[5] = extra[3]
    with pytest.raises(ValueError, match="image id 5"):
        lvis_eval.do_lvis_evaluation(_annotations(), extra)
    bad = _predictions()
    bad[3].add_field("labels", torch.tensor([4]))
    with pytest.raises(ValueError, match=r"image id 3: label 4 is outside 1 \.\. 3"):
        lvis_eval.do_lvis_evaluation(_annotations(), bad)


class _StubModel:
    def __init__(self, preds=None):
        self.preds = _predictions() if preds is None else preds

    def detect_images(self, images, image_ids):
        return [self.preds[int(i)] for i in image_ids]


LOADER = [(None, [7], [(640, 480)]), (None, [3], [(500, 400)])]


def test_protocol_none_picks_lvis_for_a_file_with_the_keys_and_coco_for_one_without(tmp_path):
    preds, stats = engine.inference_images(_StubModel(), LOADER, str(tmp_path / "lvis"), annotations=_annotations())
    assert sorted(preds) == [3, 7] and list(stats) == list(lvis_eval.STAT_NAMES) and abs(stats["AP"] - 1.0) <= NEAR
    assert sorted(os.listdir(tmp_path / "lvis")) == ["coco_results.json", "lvis_eval.txt", "lvis_results.json", "predictions.pth"]
    assert [(r["image_id"], r["category_id"]) for r in json.load(open(tmp_path / "lvis" / "lvis_results.json"))] == [(3, 1), (7, 18), (7, 90)]
    preds, stats = engine.inference_images(_StubModel(), LOADER, str(tmp_path / "coco"), annotations=_coco_annotations())
    assert list(stats) == list(coco_eval.STAT_NAMES)
    assert sorted(os.listdir(tmp_path / "coco")) == ["coco_eval.txt", "coco_results.json", "predictions.pth"]
    # the explicit forms: a file with the keys under the COCO protocol, and a file without them under LVIS, which is refused with a name
    _, stats = engine.inference_images(_StubModel(), LOADER, annotations=_annotations(), protocol="coco")
    assert list(stats) == list(coco_eval.STAT_NAMES)
    _, stats = engine.inference_images(_StubModel(), LOADER, annotations=lvis_eval.LvisAnnotations(_annotations()))
    assert list(stats) == list(lvis_eval.STAT_NAMES)
    with pytest.raises(ValueError, match="image 3 has no list `neg_category_ids`"):
        engine.inference_images(_StubModel(), LOADER, annotations=_coco_annotations(), protocol="lvis")
    with pytest.raises(ValueError, match="protocol is 'coco', 'lvis' or None"):
        engine.inference_images(_StubModel(), LOADER, annotations=_annotations(), protocol="voc")


def test_lvis_results_hold_at_most_300_rows_per_image(tmp_path):
    """301 rows on image 7 in ascending score, the two lowest equal: rows 2 .. 300 and, of the tie, one row (row 0) stay"""
    n = 301
    bl = BoxList(torch.tensor([[10., 10., 60., 60.]]).repeat(n, 1), (640, 480))
    bl.add_field("scores", torch.tensor([0.001, 0.001] + [0.01 + 0.001 * i for i in range(2, n)]))
    bl.add_field("labels", torch.full((n,), 2))
    preds = {7: bl, 3: _predictions()[3]}
    engine.inference_images(_StubModel(preds), LOADER, str(tmp_path), annotations=_annotations())
    res = json.load(open(tmp_path / "lvis_results.json"))
    mine = [r for r in res if r["image_id"] == 7]
    assert len(mine) == 300 and len(res) == 301 and set(mine[0]) == {"image_id", "category_id", "bbox", "score"} and mine[0]["bbox"] == [10, 10, 50, 50]
    assert sorted(r["score"] for r in mine)[:2] == pytest.approx([0.001, 0.012]) and len(json.load(open(tmp_path / "coco_results.json"))) == 302


def test_library_header_and_binding_carry_the_entry():
    from diffusionvid_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    assert "int dvid_lvis_eval_match(" in header
    assert int(re.search(r"#define DVID_LVIS_EVAL_MAX_GT (\d+)", header).group(1)) == ops.LVIS_EVAL_MAX_GT
    assert int(re.search(r"#define DVID_LVIS_EVAL_MAX_DETS (\d+)", header).group(1)) == ops.LVIS_EVAL_MAX_DETS == lvis_eval.MAX_DETS == 300
    assert "dvid_lvis_eval_match" in _lib.SIGNATURES and callable(ops.lvis_eval_match)
    assert header.split("int dvid_lvis_eval_match(")[1].split(");")[0].count(",") + 1 == len(_lib.SIGNATURES["dvid_lvis_eval_match"][1]) == 24
    assert "lviseval.hip" in open(os.path.join(ROOT, "diffusionvid_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    assert lib.dvid_version() >= 8 and lib.dvid_lvis_eval_match.argtypes == _lib.SIGNATURES["dvid_lvis_eval_match"][1]


def test_the_lvis_config_parses_and_passes_the_construction_checks():
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    cfg = get_cfg(os.path.join(ROOT, "configs", "still_R_101_DiffusionDet_lvis.yaml"), [], os.path.join(ROOT, "configs", "BASE_RCNN_1gpu.yaml"))
    p2 = get_cfg(os.path.join(ROOT, "configs", "still_R_101_DiffusionDet_p2.yaml"), [], os.path.join(ROOT, "configs", "BASE_RCNN_1gpu.yaml"))
    d = cfg.MODEL.DiffusionDet
    assert d.NUM_CLASSES == 1203 and cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG == 300
    assert (d.NUM_PROPOSALS, d.SAMPLE_STEP, d.NUM_HEADS) == (p2.MODEL.DiffusionDet.NUM_PROPOSALS, p2.MODEL.DiffusionDet.SAMPLE_STEP, p2.MODEL.DiffusionDet.NUM_HEADS)
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    assert model.num_classes == 1203 and model.fpn_levels == (2, 3, 4, 5)
