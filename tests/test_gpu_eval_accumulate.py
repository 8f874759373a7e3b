"""The device accumulation of the COCO / LVIS evaluators (ops.eval_accumulate, csrc/evalaccum.hip) against coco_eval.accumulate_arrays on
the same arrays: every comparison is np.array_equal on precision and recall.  The arrays are synthetic (random match, ignore and rank)
except where the real pipeline is run."""
import numpy as np
import pytest
import torch

import _coco_eval_ref as R
import _eval_accumulate_ref as E
import _lvis_eval_ref as L
from diffusionvid_amd.data.evaluation import coco_eval, lvis_eval

pytestmark = pytest.mark.gpu
COCO, LVIS = coco_eval.MAX_DETS, (lvis_eval.MAX_DETS,)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device(syn, max_dets, out=None, rec_thrs=coco_eval.REC_THRS):
    from diffusionvid_amd import ops
    got = ops.eval_accumulate(*(_dev(a) for a in syn), max_dets, rec_thrs, out=out)
    return [g.cpu().numpy() for g in got]


def _check(syn, max_dets):
    want = coco_eval.accumulate_arrays(*E.numpy_args(*syn), max_dets)
    got = _device(syn, max_dets)
    for name, g, w in zip(("precision", "recall"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s differs at %d places, first %s: %r vs %r" % (name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    return want


def _blank(images, cap, classes, npig=1):
    """every row live in category 1 with rank = its row, distinct descending scores over the set, nothing matched, nothing ignored"""
    dets = np.zeros((images, cap, 6), dtype=np.float32)
    dets[:, :, 4] = 1.0 - (np.arange(images * cap, dtype=np.float64).reshape(images, cap) + 1) / (images * cap + 2)
    dets[:, :, 5] = 1
    rank = np.broadcast_to(np.arange(cap, dtype=np.int32), (images, cap)).copy()
    return [dets, np.full(images, cap, dtype=np.int32), rank, np.zeros((4, 10, images, cap), dtype=np.int8), np.zeros((4, 10, images, cap), dtype=np.int8),
            np.full((4, classes + 1), npig, dtype=np.int32)]


# ---- 1. the order ----------------------------------------------------------------------------------------------------------------------
def test_equal_scores_across_images_keep_the_image_order():
    syn = list(E.synthetic(11, images=7, cap=5, classes=1, scores=[0.25, 0.5], p_ignore=0.0, counts=[5] * 7, npig=np.full((4, 2), 9)))
    syn[3][:, :, :3], syn[3][:, :, 3:] = 1, 0          # the first three images hit, the others miss
    back = [syn[0][::-1], syn[1][::-1], syn[2][::-1], syn[3][:, :, ::-1], syn[4][:, :, ::-1], syn[5]]
    a, b = _check(syn, COCO), _check(back, COCO)
    assert not np.array_equal(a[0], b[0]), "the case is blind: the images' order does not show in numpy's precision"


def test_equal_scores_within_an_image_keep_the_rank_order_not_the_row_order():
    syn = list(E.synthetic(12, images=3, cap=40, classes=2, scores=[0.25, 0.5], p_ignore=0.1, counts=[40, 17, 40]))
    assert (np.diff(syn[2][0][syn[0][0, :, 5] == 1]) < 0).any(), "ranks that do not follow the rows"
    _check(syn, COCO)


def test_signed_zero_is_one_score():
    syn = _blank(3, 4, 1, npig=6)
    syn[0][:, :, 4] = np.array([-0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    assert np.signbit(syn[0][:, 0::2, 4]).all() and not np.signbit(syn[0][:, 1::2, 4]).any()
    syn[3][:, :, :, 0::2] = 1          # the true positives sit on the -0.0 rows
    want = _check(syn, COCO)
    moved = [a.copy() for a in syn]
    moved[0][:, 0::2, 4] = -1e-30
    assert not np.array_equal(coco_eval.accumulate_arrays(*E.numpy_args(*moved), COCO)[0], want[0]), "the case is blind to the sign of zero"


# ---- 2. the arithmetic -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gt", [10, 20, 50, 100])
def test_recall_lands_on_the_thresholds(n_gt):
    """tp steps by one up to n_gt, so rc is k / n_gt: some of the 101 thresholds are hit exactly and "left" decides; at the odd IoU
    thresholds every other row is a false positive"""
    syn = _blank(n_gt // 10, 10, 1, npig=n_gt)
    syn[3][:] = 1
    syn[3][:, 1::2, :, 1::2] = 0
    want = _check(syn, COCO)
    assert (want[1][0::2, 0, :, 2] == 1.0).all() and (want[1][1::2, 0, :, 2] == 0.5).all()


def test_the_eps_in_front_of_the_first_counted_row_and_at_one_and_two_counted_rows():
    syn = _blank(1, 8, 3, npig=2)
    syn[0][0, :, 5] = [1, 1, 1, 1, 1, 2, 3, 3]
    syn[2][0] = [0, 1, 2, 3, 4, 0, 0, 1]
    syn[4][:, :, 0, :3] = 1          # category 1: the three rows of highest score are ignored, 0 / (0 + eps) three times
    syn[3][:, :, 0, 3] = 1           # then a true and a false positive
    syn[3][:, 0::2, 0, 5] = 1        # category 2: fp + tp == 1, a hit at the even thresholds
    syn[3][:, :, 0, 6] = 1           # category 3: fp + tp == 2
    syn[3][:, 1::3, 0, 7] = 1
    want = _check(syn, COCO)
    assert want[0][0, 0, 0, 0, 0] == 0.0 and want[0][0, 0, 0, 0, 2] == 1.0 / (1.0 + np.spacing(1))


# ---- 3. empty shapes -------------------------------------------------------------------------------------------------------------------
def test_no_live_row_at_all():
    syn = _blank(3, 4, 2)
    syn[1][:] = 0
    syn[5][:, 2] = 0
    want = _check(syn, COCO)
    assert (want[0][:, :, 0] == 0).all() and (want[0][:, :, 1] == -1).all() and (want[1][:, 0] == 0).all() and (want[1][:, 1] == -1).all()
    syn = _blank(2, 3, 1)
    syn[2][:] = -1
    _check(syn, LVIS)


def test_categories_without_rows_without_counted_boxes_and_counted_in_two_ranges_only():
    syn = list(E.synthetic(21, images=4, cap=12, classes=2))
    syn[0] = np.concatenate((syn[0], syn[0][:, :4]), axis=1)
    syn[0][:, 12:, 5] = 4                                          # label 4 of K = 5: rows, and counted in ranges 0 and 2 only
    syn[2] = np.concatenate((syn[2], np.broadcast_to(np.arange(4, dtype=np.int32), (4, 4))), axis=1)
    syn[3], syn[4] = (np.concatenate((a, a[:, :, :, :4]), axis=3) for a in (syn[3], syn[4]))
    syn[1] = np.array([16, 16, 14, 16], dtype=np.int32)
    syn[5] = np.array([[3, 5, 0, 4, 7, 0], [3, 5, 0, 4, 0, 0], [3, 5, 0, 4, 2, 0], [3, 5, 0, 4, 0, 0]], dtype=np.int32)
    # label 2: rows without counted ground truth in any range -> -1; label 3: counted without rows -> 0; label 5: neither -> -1
    assert (syn[0][:, :12, 5] == 2).any() and (syn[0][:, :, 5] != 3).all()
    want = _check(syn, COCO)
    assert (want[0][:, :, 1] == -1).all() and (want[0][:, :, 2] == 0).all() and (want[0][:, :, 4] == -1).all()
    assert (want[0][:, :, 3, [1, 3]] == -1).all() and (want[0][:, :, 3, [0, 2]] >= 0).all()


def test_counts_zero_one_and_cap_dead_ranks_and_label_zero():
    syn = list(E.synthetic(22, images=6, cap=7, classes=3, counts=[0, 1, 7, 7, 3, 7]))
    syn[2][2, [0, 3]] = -1          # rows the matching dropped
    syn[2][5, :] = -1
    syn[0][3, :, 5] = 0             # label 0: the matching ranks it, the accumulation drops it
    syn[0][4, 1, 5] = 0
    syn[0][2, 6, 5] = 7.0           # a label past K
    _check(syn, COCO)


# ---- 4. maxDets ------------------------------------------------------------------------------------------------------------------------
def test_the_three_coco_limits_with_ranks_on_both_sides_of_each():
    syn = _blank(2, 6, 1, npig=6)
    syn[2][:] = [0, 1, 9, 10, 99, 100]
    syn[3][:, :, :, [1, 3, 4, 5]] = 1
    want = _check(syn, COCO)
    assert want[1][0, 0, 0].tolist() == [0.0, 2.0 / 6.0, 1.0]          # ranks < 1: no hit; < 10: rank 1 twice; < 100: ranks 1, 10, 99 twice


def test_the_one_lvis_limit_with_ranks_299_and_300():
    syn = _blank(2, 3, 1, npig=4)
    syn[2][:] = [298, 299, 300]
    syn[3][:] = 1
    want = _check(syn, LVIS)
    assert want[1].shape == (10, 1, 4, 1) and (want[1] == 1.0).all()


# ---- 5. tile and digit edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("images,cap", [(1, 1), (1, 255), (1, 256), (1, 257), (17, 241)], ids=["1", "255", "256", "257", "4097"])
def test_one_category_blocks_at_the_tile_edges(images, cap):
    """256 rows are a tile of the scan, 4096 a tile of the sort: 4097 = 17 x 241 rows cross both"""
    syn = E.synthetic(30 + cap, images=images, cap=cap, classes=1, counts=[cap] * images, npig=np.full((4, 2), 50))
    assert int((syn[2] >= 0).sum()) == images * cap
    _check(syn, (1, 10, 300))


@pytest.mark.parametrize("total", [1, 255, 257])
def test_live_row_totals_spread_over_images_and_categories(total):
    counts = np.zeros(9, dtype=np.int32)
    counts[[1, 4, 8]] = [total - 2 * (total // 3), total // 3, total // 3]
    syn = E.synthetic(40 + total, images=9, cap=int(counts.max()), classes=5, counts=counts, scores=[0.125, 0.25, 0.5, 0.75] if total == 257 else None)
    assert int((syn[2] >= 0).sum()) == total
    _check(syn, COCO)


@pytest.mark.parametrize("classes,max_dets", [(1280, LVIS), (1, COCO)], ids=["K1280", "K1"])
def test_65537_live_rows(classes, max_dets):
    """2^16 + 1 live rows in seventeen sort tiles: 257 images of 255 rows are 65535, so two of them hold 256 (cap 256); one category of
    65537 rows, or 1280 categories of about 51"""
    syn = E.synthetic(50, images=257, cap=256, classes=classes, counts=[256] + [255] * 255 + [256], p_match=0.3)
    assert int((syn[2] >= 0).sum()) == 65537
    _check(syn, max_dets)


# ---- 6. the real pipeline --------------------------------------------------------------------------------------------------------------
def _same(got, want):
    for k in ("precision", "recall", "stats"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_coco_matching_then_accumulation_on_the_device(seed):
    from diffusionvid_amd import ops
    case = R.random_case(seed)
    want = coco_eval.evaluate_numpy(case.dets, case.counts, *case.gt(), case.num_classes)
    dets, counts = _dev(case.dets), _dev(case.counts)
    match, ignore, rank, npig = ops.coco_eval_match(dets, counts, *(_dev(a) for a in case.gt()), case.num_classes, coco_eval.IOU_THRS, coco_eval.AREA_RANGES)
    precision, recall = coco_eval.accumulate_arrays_device(dets, counts, rank, match, ignore, npig, COCO)
    assert np.array_equal(precision, want["precision"]) and np.array_equal(recall, want["recall"])
    times = {}
    _same(coco_eval.evaluate_device(case.dets, case.counts, *case.gt(), case.num_classes, device="cuda", accumulate="device", times=times), want)
    assert list(times) == ["copy_in", "kernel", "accumulate", "copy_out", "tail"]


@pytest.mark.parametrize("seed", [20, 21])
def test_lvis_matching_then_accumulation_on_the_device(seed):
    case = L.random_case(seed, images=5, max_gt=12)
    p = case.packed()
    times = {}
    _same(lvis_eval.evaluate_device(*p, case.num_classes, device="cuda", accumulate="device", times=times), lvis_eval.evaluate_numpy(*p, case.num_classes))
    assert list(times) == ["copy_in", "kernel", "accumulate", "copy_out", "tail"]


def test_do_coco_evaluation_with_the_device_accumulation_writes_the_same_text(tmp_path):
    ann, preds = R.as_annotations(R.random_case(4))
    host = coco_eval.do_coco_evaluation(ann, preds, str(tmp_path / "host"))
    dev = coco_eval.do_coco_evaluation(ann, preds, str(tmp_path / "dev"), device=torch.device("cuda"), accumulate="device")
    assert list(host.items()) == list(dev.items())
    assert (tmp_path / "dev" / "coco_eval.txt").read_bytes() == (tmp_path / "host" / "coco_eval.txt").read_bytes()


def test_do_lvis_evaluation_with_the_device_accumulation_writes_the_same_text(tmp_path):
    ann, preds = L.as_annotations(L.random_case(22, images=5, max_gt=10, max_rows=320))
    host = lvis_eval.do_lvis_evaluation(ann, preds, str(tmp_path / "host"))
    dev = lvis_eval.do_lvis_evaluation(ann, preds, str(tmp_path / "dev"), device=torch.device("cuda"), accumulate="device")
    assert list(host.items()) == list(dev.items())
    assert (tmp_path / "dev" / "lvis_eval.txt").read_bytes() == (tmp_path / "host" / "lvis_eval.txt").read_bytes()


# ---- 7. repeatability ------------------------------------------------------------------------------------------------------------------
def test_two_launches_give_the_same_bits():
    syn = E.synthetic(60, images=40, cap=130, classes=7, scores=[0.1, 0.2, 0.3, 0.4, 0.5])
    first, second = _device(syn, COCO), _device(syn, COCO)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(message, syn, max_dets=COCO, rec_thrs=coco_eval.REC_THRS):
    from diffusionvid_amd._lib import DvidError
    A, T = syn[3].shape[:2]
    out = (torch.full((T, len(rec_thrs), syn[5].shape[1] - 1, A, len(max_dets)), 77.0, dtype=torch.float64, device="cuda"),
           torch.full((T, syn[5].shape[1] - 1, A, len(max_dets)), 77.0, dtype=torch.float64, device="cuda"))
    with pytest.raises(DvidError, match=message):
        _device(syn, max_dets, out=out, rec_thrs=rec_thrs)
    torch.cuda.synchronize()
    assert bool((out[0] == 77.0).all()) and bool((out[1] == 77.0).all())


def test_the_shape_limits_are_refused_before_anything_is_written():
    syn = _blank(2, 3, 2)
    _refused(r"3 area ranges, 10 IoU thresholds and 101 recall thresholds; the kernels are built for 4, 10 and 101",
             syn[:3] + [syn[3][:3], syn[4][:3], syn[5][:3]])
    _refused(r"4 area ranges, 9 IoU thresholds and 101 recall", syn[:3] + [syn[3][:, :9], syn[4][:, :9], syn[5]])
    _refused(r"4 area ranges, 10 IoU thresholds and 100 recall", syn, rec_thrs=np.linspace(0, 1, 100))
    _refused(r"4 detection limits, 1 \.\. 3 are taken \(DVID_EVAL_ACCUMULATE_MAX_LIMITS\)", syn, max_dets=(1, 10, 100, 300))
    _refused(r"max_dets must be positive and ascending \(entry 1 is 1\)", syn, max_dets=(10, 1, 100))
    _refused(r"max_dets must be positive and ascending \(entry 1 is 10\)", syn, max_dets=(10, 10))
    _refused(r"max_dets must be positive and ascending \(entry 0 is 0\)", syn, max_dets=(0,))
    _refused(r"rec_thrs decreases at entry 100", syn, rec_thrs=list(np.linspace(0, 1, 100)) + [0.5])


def test_the_size_limits_are_refused_before_anything_is_written():
    from diffusionvid_amd import _lib, ops
    from diffusionvid_amd._lib import DvidError, ptr
    _refused(r"4097 rows per image exceed the limit of 4096 \(DVID_NMS_MAX_CANDIDATES\)", _blank(1, 4097, 1), max_dets=LVIS)
    _refused(r"1281 classes exceed the limit of 1280 \(DVID_MAX_CLASSES\)", _blank(1, 2, 1281), max_dets=LVIS)
    # sizes that no test can allocate: the entry refuses them before it reads a pointer
    small = [_dev(a) for a in _blank(1, 1, 1)]
    lim, thr = torch.tensor([300], dtype=torch.int32), torch.from_numpy(coco_eval.REC_THRS.copy())
    out = torch.full((10 * 101 * 4 + 10 * 4,), 77.0, dtype=torch.float64, device="cuda")
    scratch = torch.empty((1 << 16,), dtype=torch.uint8, device="cuda")

    def entry(n_images, cap):
        _lib.call("dvid_eval_accumulate", *(ptr(t) for t in small), n_images, cap, 1, 4, 10, ptr(lim), 1, ptr(thr), 101, ptr(out), ptr(out[4040:]),
                  ptr(scratch), scratch.numel(), _lib.stream_ptr())

    with pytest.raises(DvidError, match=r"1048576 images x 2048 rows are 2147483648 rows, the limit is 2147483647"):
        entry(1 << 20, 2048)
    need = int(_lib.load().dvid_eval_accumulate_scratch_bytes(100000, 300, 1))
    assert need > ops.EVAL_ACCUMULATE_MAX_SCRATCH_BYTES
    with pytest.raises(DvidError, match=r"%d bytes of sort buffers for 30000000 rows \(56 bytes per row\) exceed the limit of 1073741824 "
                                        r"\(DVID_EVAL_ACCUMULATE_MAX_SCRATCH_BYTES\)" % need):
        entry(100000, 300)
    with pytest.raises(DvidError, match=r"the scratch holds 65536 bytes, \d+ are needed"):
        entry(1000, 300)
    torch.cuda.synchronize()
    assert bool((out == 77.0).all())
