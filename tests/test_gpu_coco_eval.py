"""The COCO evaluator's matching on the GPU (ops.coco_eval_match, csrc/cocoeval.hip; coco_eval.evaluate_device) against the loop-for-loop
restatement of the protocol in _coco_eval_ref.py and against the numpy path.  Every comparison is exact: the kernel computes the
protocol's float64 IoU one operation at a time and takes its branches, and the accumulation is the same numpy code on the same arrays,
so a difference is a wrong kernel, not rounding."""
import numpy as np
import pytest
import torch

import _coco_eval_ref as C

from diffusionvid_amd.data.evaluation import coco_eval

pytestmark = pytest.mark.gpu
NAMES = ("match", "ignore", "rank", "npig")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(case, out=None):
    from diffusionvid_amd import ops
    got = ops.coco_eval_match(_dev(case.dets), _dev(case.counts), *(_dev(a) for a in case.gt()), case.num_classes, coco_eval.IOU_THRS,
                              coco_eval.AREA_RANGES, out=out)
    return [o.cpu().numpy() for o in got]


def _check(case):
    """kernel == restatement, at every row's own place; nothing behind counts"""
    got, want = _run(case), C.matches(case)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s differs at %s: %s vs %s" % (name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    live = np.arange(case.dets.shape[1])[None, :] < case.counts[:, None]
    assert (got[2][~live] == -1).all() and (got[0][:, :, ~live] == 0).all() and (got[1][:, :, ~live] == 0).all()
    return got


def _same(got, want):
    for k in ("precision", "recall", "stats"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _numpy_and_device(case):
    args = (case.dets, case.counts) + case.gt() + (case.num_classes,)
    return coco_eval.evaluate_numpy(*args), coco_eval.evaluate_device(*args, device="cuda")


# ---- 1. exact equality with the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.known_cases()))
def test_known_cases(name):
    case = C.known_cases()[name]
    _check(case)
    _same(coco_eval.evaluate_device(case.dets, case.counts, *case.gt(), case.num_classes, device="cuda"), C.evaluate(case))


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_random_cases(seed):
    """1-8 images, 0-40 boxes, 0-130 rows of three labels (so segments pass 100 rows), crowd boxes, equal IoUs"""
    _check(C.random_case(seed))


# ---- 2. boundaries -------------------------------------------------------------------------------------------------------------------------
def _rows(rng, n, labels, x0=0.0):
    xy = np.round(rng.uniform(0, 300, size=(n, 2)) * 4) / 4 + x0
    wh = np.round(rng.uniform(4, 150, size=(n, 2)) * 4) / 4
    score = (rng.permutation(n) + 1.0) / (n + 1)
    return np.concatenate((xy, xy + wh, score[:, None], np.asarray(labels, dtype=np.float64).reshape(n, 1)), axis=1).tolist()


def _boxes(rng, n, labels):
    xy = np.round(rng.uniform(0, 300, size=(n, 2)) * 4) / 4
    wh = np.round(rng.uniform(4, 150, size=(n, 2)) * 4) / 4
    return [(xy[k].tolist() + wh[k].tolist(), None, int(rng.rand() < 0.1), int(labels[k])) for k in range(n)]


def test_counts_of_0_1_and_cap_with_cap_not_a_power_of_two():
    rng = np.random.RandomState(10)
    for cap in (5, 70):          # 70: the sort pads to 128
        gts = _boxes(rng, 6, rng.randint(1, 4, size=6))
        on = [[b[0], b[1], b[0] + b[2], b[1] + b[3], 0.5 + 0.01 * i, l] for i, (b, _, _, l) in enumerate(gts)]          # a row on every box
        images = [([], gts), (_rows(rng, 1, [2]), gts), (_rows(rng, cap, rng.randint(1, 4, size=cap)), gts), (on, gts)]
        case = C.pack(images, 3, cap=max(cap, 6))
        got = _check(case)
        assert (got[2][0] == -1).all() and got[2][1, 0] == 0 and (got[2][2, :cap] >= 0).all()
    # counts beyond cap and below 0 are clamped
    case = C.pack([(_rows(rng, 4, [1, 1, 2, 2]), gts), (_rows(rng, 4, [1, 1, 2, 2]), gts)], 3)
    want = _run(case)
    case.counts[:] = (9, -3)
    got = _run(case)
    assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[0][:, :, 0], want[0][:, :, 0]) and (got[2][1] == -1).all()


def test_images_with_boxes_only_rows_only_and_neither():
    rng = np.random.RandomState(11)
    case = C.pack([([], _boxes(rng, 5, [1, 1, 2, 3, 3])), (_rows(rng, 7, [1, 2, 2, 3, 3, 3, 1]), []), ([], [])], 3)
    got = _check(case)
    assert got[3][0].tolist()[1:] == C.matches(case)[3][0].tolist()[1:] and got[3][0].sum() > 0
    assert (got[0][:, :, 1] == 0).all() and (got[2][1] >= 0).all()
    _same(*_numpy_and_device(case))


def test_labels_out_of_range_belong_to_no_segment():
    rng = np.random.RandomState(12)
    rows = _rows(rng, 8, [1, 4, -1, 2, 1e9, 3, 0, 2])
    gts = _boxes(rng, 3, [1, 2, 3])
    case = C.pack([(rows, gts)], 3)
    got = _check(case)
    assert got[2][0].tolist()[1] == -1 and got[2][0].tolist()[2] == -1 and got[2][0].tolist()[4] == -1 and got[2][0].tolist()[6] == 0
    case.dets[0, 4, 5] = np.nan
    assert _run(case)[2][0, 4] == -1


@pytest.mark.parametrize("n", [100, 101])
def test_a_segment_of_100_and_of_101_rows(n):
    got = _check(C.cut_case(n))
    assert got[2][0, 0] == (99 if n == 100 else -1)
    _same(*_numpy_and_device(C.cut_case(n)))


def test_more_than_64_segments_and_more_tasks_than_threads():
    """70 labels in one image: 70 segments x 40 (area range, threshold) tasks = 2800 > 256 threads; a second image with 7 segments = 280 tasks"""
    rng = np.random.RandomState(13)
    labels = np.repeat(np.arange(1, 71), 2)
    rng.shuffle(labels)
    gl = rng.randint(1, 71, size=30)
    gts = _boxes(rng, 30, gl)
    rows = _rows(rng, 140, labels)
    for i in range(0, 140, 3):          # a third of the rows sit on a box
        b = gts[i % 30][0]
        rows[i][:4] = [b[0], b[1], b[0] + b[2], b[1] + b[3]]
        rows[i][5] = gts[i % 30][3]
    case = C.pack([(rows, gts), (_rows(rng, 21, np.repeat(np.arange(1, 8), 3)), _boxes(rng, 7, np.arange(1, 8)))], 80)
    _check(case)


def test_cap_4096():
    """the largest image: 4096 rows of 8 labels (every segment is cut at 100); one more row per image is refused"""
    from diffusionvid_amd import ops
    from diffusionvid_amd._lib import DvidError
    rng = np.random.RandomState(14)
    gts = _boxes(rng, 12, rng.randint(1, 9, size=12))
    rows = _rows(rng, 4096, rng.randint(1, 9, size=4096))
    for i in range(0, 4096, 5):
        b = gts[i % 12][0]
        rows[i][:4] = [b[0] + i % 3, b[1], b[0] + b[2], b[1] + b[3]]
        rows[i][5] = gts[i % 12][3]
    case = C.pack([(rows, gts), (rows[:33], gts)], 8)
    got = _check(case)
    assert (got[2][0] >= 0).sum() == 800
    big = C.Case(np.zeros((1, 4097, 6)), [0], *C.pack([([], gts)], 8).gt(), 8)
    with pytest.raises(DvidError, match=r"4097 rows per image exceed the limit of 4096 \(DVID_NMS_MAX_CANDIDATES\)"):
        _run(big)
    assert ops.NMS_MAX_CANDIDATES == 4096


def test_the_ground_truth_limit():
    """DVID_COCO_EVAL_MAX_GT boxes in one image are evaluated; one more is refused before anything is written"""
    from diffusionvid_amd import ops
    from diffusionvid_amd._lib import DvidError
    rng = np.random.RandomState(15)
    G = ops.COCO_EVAL_MAX_GT
    gts = _boxes(rng, G + 1, rng.randint(1, 3, size=G + 1))
    rows = _rows(rng, 24, rng.randint(1, 3, size=24))
    for i in range(0, 24, 2):
        b = gts[(37 * i) % G][0]
        rows[i][:4] = [b[0], b[1], b[0] + b[2], b[1] + b[3]]
        rows[i][5] = gts[(37 * i) % G][3]
    got = _check(C.pack([(rows[:3], gts[:2]), (rows, gts[:G])], 2))
    assert got[3][0].sum() > 200
    case = C.pack([(rows[:3], gts[:2]), (rows, gts)], 2)
    out = (torch.full((4, 10, 2, 24), 77, dtype=torch.int8, device="cuda"), torch.full((4, 10, 2, 24), 77, dtype=torch.int8, device="cuda"),
           torch.full((2, 24), 77, dtype=torch.int32, device="cuda"), torch.full((4, 3), 77, dtype=torch.int32, device="cuda"))
    with pytest.raises(DvidError, match=r"image 1 holds %d ground-truth boxes, the limit is %d \(DVID_COCO_EVAL_MAX_GT\)" % (G + 1, G)):
        _run(case, out=out)
    torch.cuda.synchronize()
    assert all(bool((o == 77).all()) for o in out)


# ---- 3. the device path is the numpy path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [20, 21])
def test_evaluate_device_equals_evaluate_numpy(seed):
    case = C.random_case(seed, images=6, max_gt=12, max_rows=110)
    host, dev = _numpy_and_device(case)
    _same(dev, host)
    _same(dev, C.evaluate(case))


def test_do_coco_evaluation_on_the_device_writes_the_same_text(tmp_path):
    case = C.random_case(22, images=5, max_gt=10, max_rows=60)
    ann, preds = C.as_annotations(case)
    host = coco_eval.do_coco_evaluation(ann, preds, str(tmp_path / "host"))
    dev = coco_eval.do_coco_evaluation(ann, preds, str(tmp_path / "dev"), device=torch.device("cuda"))
    assert list(host.items()) == list(dev.items())
    text = (tmp_path / "dev" / "coco_eval.txt").read_text()
    assert text == (tmp_path / "host" / "coco_eval.txt").read_text() and len(text.splitlines()) == 12
    assert np.array_equal(np.array(list(dev.values())), C.evaluate(case)["stats"])


# ---- 4. repeatability ------------------------------------------------------------------------------------------------------------------------
def test_two_launches_give_the_same_bits():
    case = C.random_case(3)
    first, second = _run(case), _run(case)
    for name, a, b in zip(NAMES, first, second):
        assert np.array_equal(a, b), name
