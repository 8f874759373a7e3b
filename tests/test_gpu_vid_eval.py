"""The VID evaluator on the GPU (ops.vid_eval_match, csrc/videval.hip; vid_eval.eval_detection_vid_device) against the CPU evaluator
of this repository on the same data.  The comparison is exact: the kernel computes _iou_vid's float32 bits and takes the loop's
branches, the numpy tail sorts the same arrays in the same order, so a difference is a wrong kernel, not rounding.  match / weight /
rank / n_pos are compared with the instrumented restatement of calc_prec_rec's loop in _vid_eval_ref.py, the AP arrays, CorLoc and
result.txt with eval_detection_vid, corloc_eval_detection_vid and do_vid_evaluation themselves."""
import numpy as np
import pytest
import torch

import _vid_eval_ref as V

from diffusionvid_amd.data.evaluation import vid_eval

pytestmark = pytest.mark.gpu
RANGES4 = vid_eval.MOTION_RANGES


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _run(case, ranges=((0.0, 1.0),), num_classes=30, use_motion=True, empty_w=None, **kw):
    from diffusionvid_amd import ops
    motion = case.motion if use_motion else None
    if empty_w is None:
        empty_w = vid_eval._empty_weights(motion, ranges)
    out = ops.vid_eval_match(_dev(case.dets), _dev(case.counts), _dev(case.gt_boxes), _dev(case.gt_labels), _dev(case.gt_starts), num_classes,
                             motion=_dev(motion), ranges=ranges, empty_w=empty_w, **kw)
    return [o.cpu().numpy() for o in out]


def _same_matches(got, want, case):
    live = np.arange(case.dets.shape[1])[None, :] < case.counts[:, None]
    for name, g, w in zip(("match", "weight", "rank", "n_pos"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s differs at %s: %s vs %s" % (name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert (got[2][~live] == -1).all() and (got[0][:, ~live] == 0).all() and (got[1][:, ~live] == 0).all()


def _check(case, ranges=((0.0, 1.0),), num_classes=30, use_motion=True, stable=False):
    """kernel == instrumented CPU loop; device AP == eval_detection_vid (distinct scores); device CorLoc == corloc_eval_detection_vid"""
    got = _run(case, ranges, num_classes, use_motion)
    want = V.cpu_matches(case, ranges, num_classes=num_classes, stable=stable, use_motion=use_motion)
    _same_matches(got, want, case)
    if stable:
        return got
    preds, gts = case.boxlists()
    motion = case.motion_lists() if use_motion else None
    args = (torch.from_numpy(case.dets), case.counts, case.gt_boxes, case.gt_labels, case.gt_starts)
    dev_ap = vid_eval.eval_detection_vid_device(*args, motion_ious=case.motion if use_motion else None, motion_ranges=ranges, device="cuda",
                                                num_classes=num_classes)
    V.same_ap(dev_ap, vid_eval.eval_detection_vid(preds, gts, motion_ious=motion, motion_ranges=ranges))
    assert vid_eval.corloc_eval_detection_vid_device(*args, device="cuda", num_classes=num_classes) == vid_eval.corloc_eval_detection_vid(preds, gts)
    return got


def _row(box, score, label):
    return list(box) + [score, label]


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------
def test_golden_g11_one_range():
    case, z = V.golden_case("g11_vid_eval")
    _check(case, use_motion=False)
    got = vid_eval.eval_detection_vid_device(_dev(case.dets), case.counts, case.gt_boxes, case.gt_labels, case.gt_starts)
    np.testing.assert_allclose(got["ap"], z["ap"], rtol=0, atol=1e-12, equal_nan=True)
    assert abs(got["map"] - float(z["map"])) < 1e-12


def test_golden_g15_four_ranges():
    case, z = V.golden_case("g15_vid_eval_motion")
    _check(case, RANGES4)
    got = vid_eval.eval_detection_vid_device(_dev(case.dets), case.counts, case.gt_boxes, case.gt_labels, case.gt_starts, motion_ious=case.motion)
    assert len(got) == 4
    for i, r in enumerate(got):
        np.testing.assert_allclose(r["ap"], z["ap%d" % i], rtol=0, atol=1e-12, equal_nan=True)
        assert abs(r["map"] - float(z["map%d" % i])) < 1e-12


# ---- 2. random frames -----------------------------------------------------------------------------------------------------------------
def test_random_frames_all_ranges_corloc_and_result_txt(tmp_path):
    case = V.random_case(5)
    assert case.dets.shape[:2] == (64, 48) and {0.7, 0.9} <= set(case.motion.tolist())
    live = case.dets[:, :, 4][np.arange(48)[None, :] < case.counts[:, None]]
    assert len(np.unique(live)) == len(live)          # distinct scores
    _check(case, RANGES4)
    # do_vid_evaluation: predictions in the 1000 x 600 frame the detector saw, annotations at two sizes (one ratio, two ratios)
    preds, gts = case.boxlists()
    sizes = [(500, 300) if f % 2 else (640, 400) for f in range(case.frames)]
    for f, (p, g) in enumerate(zip(preds, gts)):
        p.size, g.size = (1000, 600), sizes[f]
    ds = vid_eval.GroundTruthList(gts, motion=case.motion_lists())
    texts = []
    for k, dev in enumerate((None, torch.device("cuda"))):
        folder = tmp_path / str(k)
        folder.mkdir()
        res = vid_eval.do_vid_evaluation(ds, preds, str(folder), motion_specific=True, device=dev)
        texts.append(((folder / "result.txt").read_bytes(), res))
    assert texts[0][0] == texts[1][0] and b"motion=  slow" in texts[0][0]
    V.same_ap(texts[1][1], texts[0][1])
    for k, dev in enumerate((None, torch.device("cuda"))):          # and without the motion ranges
        folder = tmp_path / ("plain%d" % k)
        folder.mkdir()
        vid_eval.do_vid_evaluation(ds, preds, str(folder), device=dev)
        texts.append((folder / "result.txt").read_bytes())
    assert texts[2] == texts[3]


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------
GT = [10, 10, 60, 60]


def test_frames_without_detections_without_ground_truth_and_with_neither():
    frames = [([], [GT], [2]), ([_row(GT, 0.9, 2)], np.zeros((0, 4)), []), ([], np.zeros((0, 4)), []), ([_row(GT, 0.8, 2)], [GT], [2])]
    got = _check(V.pack(frames), use_motion=False)
    assert got[0][0, :, 0].tolist() == [0, 0, 0, 1] and got[2][:, 0].tolist() == [-1, 0, -1, 0] and got[3][0, 2] == 2
    assert got[4].tolist() == [-1, 0, -1, 0] and got[5].tolist() == [0, 0, 0, 1]


def test_cap_one():
    frames = [([_row(GT, 0.9, 1)], [GT], [1]), ([_row([200, 200, 260, 260], 0.8, 1)], [GT], [1])]
    case = V.pack(frames)
    assert case.dets.shape[1] == 1
    assert _check(case, use_motion=False)[0].reshape(-1).tolist() == [1, 0]


def test_class_only_in_ground_truth_and_class_only_in_predictions():
    frames = [([_row(GT, 0.9, 3), _row(GT, 0.7, 5)], [GT, GT], [3, 7])]          # 5: predictions only; 7: ground truth only
    got = _check(V.pack(frames, [[0.5, 0.8]]), RANGES4)
    assert got[3][:, 7].tolist() == [1, 0, 1, 0] and got[3][:, 5].tolist() == [0, 0, 0, 0] and got[0][0, 0].tolist() == [1, 0]
    assert got[1][:, 0, 1].tolist() == [0.0, 0.5, 0.5, 0.0]          # no box of label 5: the in-range fraction, 0 where that is 1


def test_iou_exactly_at_the_threshold_matches():
    """[0, 0, 8, 18] against [0, 0, 8, 8]: with both + 1 the areas are 10 x 20 and 10 x 10, the overlap 100: 100 / 200 = 0.5"""
    case = V.pack([([_row([0, 0, 8, 18], 0.9, 1)], [[0, 0, 8, 8]], [1])])
    assert vid_eval._iou_vid(case.dets[0, :1, :4], case.gt_boxes)[0, 0] == np.float32(0.5)
    got = _check(case, use_motion=False)
    assert got[0][0, 0, 0] == 1 and got[5][0] == 0          # >= for the AP, > for CorLoc


def test_identical_boxes_first_ignored_goes_to_the_second():
    frames = [([_row(GT, 0.9, 1), _row(GT, 0.8, 1), _row(GT, 0.7, 1)], [GT, GT], [1, 1])]
    got = _check(V.pack(frames, [[0.95, 0.8]]), ((0.0, 0.9),))          # box 0 is ignored in (0, 0.9)
    assert got[0][0, 0].tolist() == [1, 1, 0] and got[1][0, 0].tolist() == [0.0, 1.0, 0.5]


def test_identical_boxes_neither_ignored_keeps_the_first():
    frames = [([_row(GT, 0.9, 1), _row(GT, 0.8, 1), _row(GT, 0.7, 1)], [GT, GT], [1, 1])]
    got = _check(V.pack(frames, [[0.5, 0.5]]), RANGES4)
    assert got[0][0, 0].tolist() == [1, 1, 0] and got[1][0, 0].tolist() == [0.0, 0.0, 0.0]
    assert got[1][1, 0].tolist() == [0.0, 0.0, 0.0] and got[1][2, 0].tolist() == [1.0, 1.0, 1.0]


def test_unmatched_row_best_overlap_ignored_counted_and_a_draw():
    a, b = [10, 10, 60, 60], [200, 200, 250, 250]
    near_a, near_b, far = [10, 10, 30, 30], [200, 200, 220, 220], [400, 300, 450, 380]
    frames = [([_row(near_a, 0.9, 1), _row(near_b, 0.8, 1), _row(far, 0.7, 1)], [a, b, b], [1, 1, 1])]
    got = _check(V.pack(frames, [[0.95, 0.5, 0.5]]), ((0.0, 0.9),))          # a is ignored, both b are counted
    assert got[0][0, 0].tolist() == [0, 0, 0] and got[1][0, 0].tolist() == [1.0, 0.0, 1.0 / 3.0]


def test_empty_weight_of_one_is_forced_to_zero():
    frames = [([_row(GT, 0.9, 4)], [GT], [2])]          # every motion IoU is inside (0, 1): the in-range fraction is 1
    case = V.pack(frames, [[0.5]])
    assert vid_eval._empty_weights(case.motion, ((0.0, 1.0), (0.7, 0.9))) == [0.0, 0.0]
    case2 = V.pack(frames + [([], [GT], [2])], [[0.5], [0.8]])
    assert vid_eval._empty_weights(case2.motion, ((0.0, 1.0), (0.7, 0.9))) == [0.0, 0.5]
    assert _check(case, ((0.0, 1.0), (0.7, 0.9)))[1][:, 0, 0].tolist() == [0.0, 0.0]
    assert _check(case2, ((0.0, 1.0), (0.7, 0.9)))[1][:, 0, 0].tolist() == [0.0, 0.5]


@pytest.mark.parametrize("labels", [65, 130])
def test_more_labels_in_a_frame_than_a_wave_has_lanes(labels):
    rng = np.random.RandomState(labels)
    rows, gb, gl = [], [], []
    for l in range(1, labels + 1):
        x, y = 12 * (l % 20), 15 * (l // 20)
        box = [x, y, x + 40, y + 50]
        gb.append(box), gl.append(l)
        rows.append(_row(box, 0.0, l))
        rows.append(_row([x + 3, y, x + 43, y + 50], 0.0, l))
    rows = np.array(rows, dtype=np.float32)[rng.permutation(len(rows))]
    rows[:, 4] = rng.permutation(len(rows)) / np.float32(len(rows))
    got = _check(V.pack([(rows, gb, gl), (rows[::-1].copy(), gb[::-1], gl[::-1])], [rng.rand(labels), rng.rand(labels)]), RANGES4, num_classes=labels)
    assert got[0][0].sum() == 2 * labels


def test_one_class_of_200_rows_against_70_boxes():
    rng = np.random.RandomState(7)
    xy = rng.uniform(0, 300, size=(70, 2))
    gb = np.concatenate((xy, xy + rng.uniform(20, 90, size=(70, 2))), axis=1).astype(np.float32)
    gb[40] = gb[3]
    rows = np.zeros((200, 6), dtype=np.float32)
    rows[:, :4] = gb[rng.randint(70, size=200)] + rng.randint(-6, 7, size=(200, 4))
    rows[:, 4], rows[:, 5] = rng.permutation(200) / np.float32(200), 9
    got = _check(V.pack([(rows, gb, np.full(70, 9))], [rng.choice([0.3, 0.7, 0.8, 0.9, 1.0], size=70)]), RANGES4)
    assert 20 < got[0][0].sum() <= 70


def test_num_classes_1280_with_labels_1_and_1280():
    frames = [([_row(GT, 0.9, 1280), _row(GT, 0.8, 1), _row(GT, 0.7, 1280)], [GT, GT], [1, 1280])]
    got = _check(V.pack(frames), num_classes=1280, use_motion=False)
    assert got[0][0, 0].tolist() == [1, 1, 0] and got[3].shape == (1, 1281) and got[3][0, 1] == got[3][0, 1280] == 1


def test_cap_4096_on_two_frames():
    rng = np.random.RandomState(11)
    frames = []
    for f in range(2):
        xy = rng.uniform(0, 400, size=(12, 2))
        gb = np.concatenate((xy, xy + rng.uniform(20, 90, size=(12, 2))), axis=1).astype(np.float32)
        gl = rng.randint(1, 31, size=12)
        n = 4096 if f == 0 else 4095
        k = rng.randint(12, size=n)
        rows = np.zeros((n, 6), dtype=np.float32)
        rows[:, :4] = gb[k] + rng.randint(-8, 9, size=(n, 4))
        rows[:, 4], rows[:, 5] = (rng.permutation(n) + f * 4096) / np.float32(8192), np.where(rng.rand(n) < 0.9, gl[k], rng.randint(1, 31, size=n))
        frames.append((rows, gb, gl))
    case = V.pack(frames, [rng.rand(12), rng.rand(12)])
    assert case.dets.shape[1] == 4096
    _check(case, RANGES4)


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------
def test_equal_scores_go_lower_row_first():
    case = V.random_case(9, frames=24, cap=40, ties=True)
    got = _check(case, RANGES4, stable=True)
    want = V.cpu_matches(case, RANGES4, stable=True)
    scores, labels = case.dets[:, :, 4], case.dets[:, :, 5].astype(np.int64)
    dev = vid_eval.eval_detection_vid_device(_dev(case.dets), case.counts, case.gt_boxes, case.gt_labels, case.gt_starts, motion_ious=case.motion,
                                             num_classes=30)
    host = vid_eval.prec_rec_from_matches(scores, labels, case.counts, want[2], want[0], want[1], want[3], case.gt_labels)
    for d, (prec, rec) in zip(dev, host):
        assert np.array_equal(d["ap"], vid_eval.calc_ap(prec, rec), equal_nan=True)
    # a tie inside one (frame, class): three identical rows on one box -- the lowest row takes it
    frames = [([_row(GT, 0.5, 1), _row(GT, 0.5, 1), _row(GT, 0.5, 1)], [GT], [1])]
    got = _check(V.pack(frames), use_motion=False, stable=True)
    assert got[0][0, 0].tolist() == [1, 0, 0] and got[2][0].tolist() == [0, 1, 2] and got[4][0] == 0


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def _refused(case, pattern, ranges=((0.0, 1.0),), num_classes=30):
    from diffusionvid_amd import _lib
    F, cap, R = case.dets.shape[0], case.dets.shape[1], len(ranges)
    out = (torch.full((R, F, cap), 77, dtype=torch.int8), torch.full((R, F, cap), 77.0, dtype=torch.float64), torch.full((F, cap), 77, dtype=torch.int32),
           torch.full((R, num_classes + 1), 77.0, dtype=torch.float64), torch.full((F,), 77, dtype=torch.int32), torch.full((F,), 77, dtype=torch.int8))
    out = tuple(o.cuda() for o in out)
    with pytest.raises(_lib.DvidError, match=pattern):
        _run(case, ranges, num_classes, use_motion=False, empty_w=[0.0] * R, out=out)
    torch.cuda.synchronize()
    assert all(bool((o == 77).all()) for o in out), "a refused call wrote to its outputs"


def test_refusals_name_the_limit_and_write_nothing():
    rows = np.zeros((4097, 6), dtype=np.float32)
    rows[:, 2:4], rows[:, 4], rows[:, 5] = 10, np.arange(4097) / np.float32(4097), 1
    _refused(V.pack([(rows, [GT], [1])]), r"4097 rows per frame exceed the limit of 4096 \(DVID_NMS_MAX_CANDIDATES\)")
    _refused(V.pack([([_row(GT, 0.9, 31)], [GT], [1])]), r"labels 1 \.\. 31 leave the range 0 \.\. 30")
    _refused(V.pack([([_row(GT, 0.9, 1)], [GT], [31])]), r"labels 1 \.\. 31 leave the range 0 \.\. 30")
    _refused(V.pack([([_row(GT, 0.9, 1)], [GT], [1]), ([_row(GT, 0.9, 1)], [GT] * 257, [1] * 257)]),
             r"frame 1 holds 257 ground-truth boxes, the limit is 256 \(DVID_VID_EVAL_MAX_GT\)")
    _refused(V.pack([([_row(GT, 0.9, 1)], [GT], [1])]), r"5 motion ranges, the limit is 1 \.\. 4 \(DVID_VID_EVAL_MAX_RANGES\)", ranges=((0.0, 1.0),) * 5)
    _refused(V.pack([([_row(GT, 0.9, 1)], [GT], [1])]), r"1281 classes exceed the limit of 1280 \(DVID_MAX_CLASSES\)", num_classes=1281)
    assert _run(V.pack([([_row(GT, 0.9, 1)], [GT] * 256, [1] * 256)]), use_motion=False)[0].reshape(-1).tolist() == [1]          # at the bound


# ---- 6. run to run ------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes():
    case = V.random_case(5)
    a, b = _run(case, RANGES4), _run(case, RANGES4)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
