"""The host side of the device evaluator (vid_eval.pack_groundtruth / resize_packed / prec_rec_from_matches, the binding of
dvid_vid_eval_match) without a GPU: each piece against the CPU evaluator's own code on the same data."""
import os
import re

import numpy as np
import pytest
import torch

import _vid_eval_ref as V

from diffusionvid_amd.data.evaluation import vid_eval
from diffusionvid_amd.structures.bounding_box import BoxList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resize_packed_is_boxlist_resize_bit_for_bit():
    """both branches of BoxList.resize: one common ratio (600 x 1000 -> 300 x 500, and 1.7x) and two ratios (-> 1280 x 720, 333 x 500)"""
    rng = np.random.RandomState(0)
    sizes = [(1000, 600), (1000, 600), (1000, 600), (999, 601), (640, 480), (1000, 600)]
    targets = [(500, 300), (1280, 720), (333, 500), (1280, 720), (1088, 816), (1000, 600)]
    cap = 9
    dets, counts = torch.zeros((len(sizes), cap, 6)), [9, 5, 0, 7, 9, 3]
    want = []
    for f, (size, target) in enumerate(zip(sizes, targets)):
        xy = rng.uniform(0, 400, size=(counts[f], 2))
        box = torch.from_numpy(np.concatenate((xy, xy + rng.uniform(1, 500, size=(counts[f], 2))), axis=1).astype(np.float32))
        dets[f, :counts[f], :4] = box
        dets[f, :counts[f], 4] = torch.rand(counts[f])
        dets[f, :counts[f], 5] = 3.0
        bl = BoxList(box, size)
        rw, rh = (float(n) / float(o) for n, o in zip(target, size))
        assert (rw == rh) == (f in (0, 4, 5))          # the equal-ratio branch and the per-axis branch are both taken
        want.append(bl.resize(target).bbox)
    got = vid_eval.resize_packed(dets, sizes, targets)
    for f in range(len(sizes)):
        assert torch.equal(got[f, :counts[f], :4].view(torch.int32), want[f].view(torch.int32)), f
    assert torch.equal(got[:, :, 4:], dets[:, :, 4:]) and got.data_ptr() != dets.data_ptr()


def test_pack_groundtruth_round_trips_ragged_frames():
    rng = np.random.RandomState(1)
    n = [3, 0, 1, 0, 0, 5, 2]
    gts, motion = [], []
    for k in n:
        bl = BoxList(torch.from_numpy(rng.uniform(0, 300, size=(k, 4)).astype(np.float32)), (500, 400))
        bl.add_field("labels", torch.from_numpy(rng.randint(1, 31, size=k)))
        gts.append(bl)
        motion.append(rng.rand(k).tolist())
    motion[5] = motion[5][:3]          # two entries missing: they count as 0
    boxes, labels, starts, mo = vid_eval.pack_groundtruth(gts, motion)
    assert (boxes.dtype, labels.dtype, starts.dtype, mo.dtype) == (np.float32, np.int32, np.int32, np.float64)
    assert starts.tolist() == [0, 3, 3, 4, 4, 4, 9, 11] and boxes.shape == (11, 4)
    for f, bl in enumerate(gts):
        a, b = starts[f], starts[f + 1]
        assert np.array_equal(boxes[a:b], bl.bbox.numpy().reshape(-1, 4)) and np.array_equal(labels[a:b], bl.get_field("labels").numpy())
        assert mo[a:b].tolist() == (motion[f] + [0.0, 0.0])[:b - a]
    assert vid_eval.pack_groundtruth(gts)[3] is None
    boxes, labels, starts, mo = vid_eval.pack_groundtruth([])
    assert boxes.shape == (0, 4) and starts.tolist() == [0] and len(labels) == 0


@pytest.mark.parametrize("name, ranges", [("g11_vid_eval", None), ("g15_vid_eval_motion", vid_eval.MOTION_RANGES)])
def test_prec_rec_from_matches_gives_the_cpu_evaluators_ap(name, ranges):
    """match / weight / rank / n_pos recorded by the instrumented CPU loop -> the same `ap` arrays as eval_detection_vid, element for
    element, and the reference's recorded ones within the goldens' 1e-12"""
    case, z = V.golden_case(name)
    preds, gts = case.boxlists()
    want = vid_eval.eval_detection_vid(preds, gts, motion_ious=case.motion_lists() if ranges else None)
    match, weight, rank, n_pos = V.cpu_matches(case, ranges or ((0.0, 1.0),), use_motion=bool(ranges))
    scores, labels = case.dets[:, :, 4], case.dets[:, :, 5].astype(np.int64)
    got = []
    for prec, rec in vid_eval.prec_rec_from_matches(scores, labels, case.counts, rank, match, weight, n_pos, case.gt_labels):
        ap = vid_eval.calc_ap(prec, rec)
        got.append({"ap": ap, "map": float(np.nanmean(ap))})
    V.same_ap(got, want)
    if ranges:
        for i, r in enumerate(got):
            np.testing.assert_allclose(r["ap"], z["ap%d" % i], rtol=0, atol=1e-12, equal_nan=True)
    else:
        np.testing.assert_allclose(got[0]["ap"], z["ap"], rtol=0, atol=1e-12, equal_nan=True)
        prec, rec = vid_eval.prec_rec_from_matches(scores, labels, case.counts, rank, match[0], weight[0], n_pos[0], case.gt_labels)
        assert np.array_equal(vid_eval.calc_ap(prec, rec), want["ap"], equal_nan=True)          # the one-range form


def test_prec_rec_from_matches_on_random_frames_with_all_ranges():
    """the same on the seeded 64-frame set of the GPU test: prec and rec themselves, array for array"""
    case = V.random_case(5)
    preds, gts = case.boxlists()
    match, weight, rank, n_pos = V.cpu_matches(case, vid_eval.MOTION_RANGES)
    got = vid_eval.prec_rec_from_matches(case.dets[:, :, 4], case.dets[:, :, 5].astype(np.int64), case.counts, rank, match, weight, n_pos, case.gt_labels)
    for (prec, rec), rng in zip(got, vid_eval.MOTION_RANGES):
        wp, wr = vid_eval.calc_prec_rec(preds, gts, 0.5, case.motion_lists(), rng)
        assert len(prec) == len(wp)
        for a, b in list(zip(prec, wp)) + list(zip(rec, wr)):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b, equal_nan=True))


def test_library_header_and_binding_carry_the_entry():
    from diffusionvid_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    assert "int dvid_vid_eval_match(" in header
    assert int(re.search(r"#define DVID_VID_EVAL_MAX_GT (\d+)", header).group(1)) == ops.VID_EVAL_MAX_GT >= 256
    assert int(re.search(r"#define DVID_VID_EVAL_MAX_RANGES (\d+)", header).group(1)) == ops.VID_EVAL_MAX_RANGES == 4
    assert "dvid_vid_eval_match" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.dvid_version() >= 5 and lib.dvid_vid_eval_match.argtypes == _lib.SIGNATURES["dvid_vid_eval_match"][1]
    assert header.split("int dvid_vid_eval_match(")[1].split(");")[0].count(",") + 1 == len(lib.dvid_vid_eval_match.argtypes)
