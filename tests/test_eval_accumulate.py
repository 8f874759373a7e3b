"""The order argument of the device accumulation (csrc/evalaccum.hip), pinned without a GPU: coco_eval.accumulate_arrays equals a plain
restatement that sorts the live rows ONCE by (label, -score with -0 folded, image, rank) and then counts with integers.  Also the C
ABI's declaration and the `accumulate` keyword's refusals."""
import os
import re

import numpy as np
import pytest
import torch

import _coco_eval_ref as R
import _eval_accumulate_ref as E
import _lvis_eval_ref as L
from diffusionvid_amd.data.evaluation import coco_eval, lvis_eval
from diffusionvid_amd.engine import inference as engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(args, max_dets):
    want = coco_eval.accumulate_arrays(*args, max_dets)
    got = E.accumulate_plain(*args, max_dets)
    for name, g, w in zip(("precision", "recall"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype == np.float64 and np.array_equal(g, w), name
    return want


def _coco_args(case):
    match, ignore, rank, npig = coco_eval.match_numpy(case.dets, case.counts, *case.gt(), case.num_classes)
    return np.ascontiguousarray(case.dets[:, :, 4]), case.dets[:, :, 5].astype(np.int64), case.counts, rank, match, ignore, npig


@pytest.mark.parametrize("name", sorted(R.known_cases()))
def test_known_cases(name):
    _both(_coco_args(R.known_cases()[name]), coco_eval.MAX_DETS)


@pytest.mark.parametrize("case", [R.cut_case(100), R.cut_case(101), R.ar_case()], ids=["cut100", "cut101", "ar"])
def test_cut_and_average_recall_cases(case):
    _both(_coco_args(case), coco_eval.MAX_DETS)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_cases(seed):
    precision, _ = _both(_coco_args(R.random_case(seed, images=3, max_gt=12, max_rows=60)), coco_eval.MAX_DETS)
    assert (precision > 0).any()


def test_an_lvis_case_with_the_one_limit_300():
    case = L.random_case(5, images=3, max_gt=8, max_rows=320)
    p = case.packed()
    match, ignore, rank, npig = lvis_eval.match_numpy(*p[:11], case.num_classes)
    assert rank.max() >= 100
    _both((np.ascontiguousarray(p[0][:, :, 4]), p[0][:, :, 5].astype(np.int64), p[1], rank, match, ignore, npig), (lvis_eval.MAX_DETS,))


def test_synthetic_arrays_with_equal_scores_signed_zeros_and_dead_rows():
    """what the GPU tests feed the kernels: equal scores across images, +0 / -0, rank -1, label 0, uncounted ranges"""
    syn = list(E.synthetic(7, images=6, cap=9, classes=3, scores=[0.25, 0.5, 0.0, -0.0]))
    syn[0][1, :, 5] = 0
    syn[2][2, :3] = -1
    _both(E.numpy_args(*syn), (1, 3, 100))


def test_the_order_of_equal_scores_across_images_is_observable():
    """the reason the order is pinned at all: with equal scores, reversing the images changes the precision"""
    dets, counts, rank, match, ignore, npig = E.synthetic(11, images=7, cap=5, classes=1, scores=[0.25, 0.5], p_ignore=0.0, counts=[5] * 7,
                                                          npig=np.full((4, 2), 9))
    match[:, :, :3], match[:, :, 3:] = 1, 0
    a = coco_eval.accumulate_arrays(*E.numpy_args(dets, counts, rank, match, ignore, npig), (100,))
    b = coco_eval.accumulate_arrays(*E.numpy_args(dets[::-1], counts[::-1], rank[::-1], match[:, :, ::-1], ignore[:, :, ::-1], npig), (100,))
    assert not np.array_equal(a[0], b[0])


def test_library_header_and_binding_carry_the_entry():
    from diffusionvid_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    assert "int dvid_eval_accumulate(" in header and "long long dvid_eval_accumulate_scratch_bytes(int n_images, int cap, int max_dets_count);" in header
    assert int(re.search(r"#define DVID_EVAL_ACCUMULATE_RECALLS (\d+)", header).group(1)) == ops.EVAL_ACCUMULATE_RECALLS == len(coco_eval.REC_THRS)
    assert int(re.search(r"#define DVID_EVAL_ACCUMULATE_MAX_LIMITS (\d+)", header).group(1)) == ops.EVAL_ACCUMULATE_MAX_LIMITS == len(coco_eval.MAX_DETS)
    assert re.search(r"#define DVID_EVAL_ACCUMULATE_MAX_SCRATCH_BYTES \(1ll << 30\)", header) and ops.EVAL_ACCUMULATE_MAX_SCRATCH_BYTES == 1 << 30
    assert "dvid_eval_accumulate" in _lib.SIGNATURES and "dvid_eval_accumulate_scratch_bytes" in _lib.SIGNATURES and callable(ops.eval_accumulate)
    assert header.split("int dvid_eval_accumulate(")[1].split(");")[0].count(",") + 1 == len(_lib.SIGNATURES["dvid_eval_accumulate"][1]) == 20
    assert "evalaccum.hip" in open(os.path.join(ROOT, "diffusionvid_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    assert lib.dvid_version() >= 9 and lib.dvid_eval_accumulate.argtypes == _lib.SIGNATURES["dvid_eval_accumulate"][1]
    # 56 bytes per row and the tables; sizes that are no sizes
    rows = 5000 * 500
    assert 56 * rows < lib.dvid_eval_accumulate_scratch_bytes(5000, 500, 3) < 57 * rows
    assert lib.dvid_eval_accumulate_scratch_bytes(0, 1, 1) > 0 and lib.dvid_eval_accumulate_scratch_bytes(1, 0, 1) == -1
    assert lib.dvid_eval_accumulate_scratch_bytes(1, 1, 4) == -1


class _NoModel:
    def detect_images(self, images, image_ids):
        raise AssertionError("the keywords are checked before the first batch")


def test_accumulate_device_without_a_device_names_both_keywords():
    ann, preds = R.as_annotations(R.known_cases()["perfect"])
    with pytest.raises(ValueError, match=r"accumulate='device' needs device"):
        coco_eval.do_coco_evaluation(ann, preds, accumulate="device")
    lann, lpreds = L.as_annotations(L.random_case(1, images=2, max_gt=3, max_rows=5))
    with pytest.raises(ValueError, match=r"accumulate='device' needs device"):
        lvis_eval.do_lvis_evaluation(lann, lpreds, accumulate="device")
    with pytest.raises(ValueError, match=r"eval_accumulate='device' needs eval_device"):
        engine.inference_images(_NoModel(), [(None, [10], [(640, 640)])], annotations=ann, eval_accumulate="device")


def test_any_other_accumulate_value_is_refused():
    ann, preds = R.as_annotations(R.known_cases()["perfect"])
    with pytest.raises(ValueError, match=r"accumulate is 'numpy' or 'device', not 'torch'"):
        coco_eval.do_coco_evaluation(ann, preds, accumulate="torch")
    lann, lpreds = L.as_annotations(L.random_case(1, images=2, max_gt=3, max_rows=5))
    with pytest.raises(ValueError, match=r"accumulate is 'numpy' or 'device', not None"):
        lvis_eval.do_lvis_evaluation(lann, lpreds, accumulate=None)
    with pytest.raises(ValueError, match=r"eval_accumulate is 'numpy' or 'device', not 'gpu'"):
        engine.inference_images(_NoModel(), [(None, [10], [(640, 640)])], annotations=ann, eval_accumulate="gpu")
    case = R.known_cases()["perfect"]
    with pytest.raises(ValueError, match=r"accumulate is 'numpy' or 'device'"):
        coco_eval.evaluate_device(torch.from_numpy(case.dets), case.counts, *case.gt(), case.num_classes, accumulate="host")


def test_the_default_is_the_numpy_path_and_writes_the_same_numbers(tmp_path):
    ann, preds = R.as_annotations(R.random_case(2, images=2, max_gt=6, max_rows=20))
    assert coco_eval.do_coco_evaluation(ann, preds) == coco_eval.do_coco_evaluation(ann, preds, accumulate="numpy")
