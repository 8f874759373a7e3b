"""Seq-NMS on the GPU (ops.seq_nms_video, csrc/seqnms.hip) against the reference's own results: tests/golden/seqnms/g19_seq_nms.npz
holds what the reference's seq_nms.py returned on six synthetic videos (tests/golden/make_golden_seqnms.py lists what each is for).
The comparison is exact -- keep equal, scores bit-equal: the kernel computes float32 without contraction and with IEEE division, as
the reference does, so a difference is a wrong kernel, not rounding.

g20_seq_nms_bounds.npz holds the videos that reach the second trip of every loop of the kernel -- more than 256 boxes of a class in a
frame, predecessors and link rows past the first 64-bit word, more than 256 frames, all 30 classes of several videos side by side --
and the tests on it also pin what only a real wave can get wrong: the rounds each class ran, the scratch the kernel reads before it has
written it and the bytes around the size it asked for, the same answer on every run, and independence of how the classes' rows
interleave."""
import numpy as np
import pytest
import torch

from conftest import golden

import _seq_nms_host as H

pytestmark = pytest.mark.gpu
CASES = "abcdef"
CASES20 = ("g", "h", "i0", "i1", "i2")
GUARD = 4096


@pytest.fixture(scope="module")
def g19():
    return golden("seqnms/g19_seq_nms")


@pytest.fixture(scope="module")
def g20():
    return golden("seqnms/g20_seq_nms_bounds")


@pytest.fixture(scope="module")
def rounds(g19, g20):
    """the restatement's rounds per class, [1, 30] per fixture video: what the kernel's status words must equal.  Computed once."""
    return {c: H.seq_nms_rounds(z[c + "_dets"], z[c + "_counts"], 30)[2] for z, cases in ((g19, CASES), (g20, CASES20)) for c in cases}


@pytest.fixture(scope="module")
def busy(g20):
    """case i as ONE call: (dets, counts, video_starts, keep, scores); the rows a narrower video gains are copies of a live row, not zeros"""
    vids = [(g20["i%d_dets" % v], g20["i%d_counts" % v], g20["i%d_keep" % v], g20["i%d_scores" % v]) for v in range(3)]
    cap, frames = max(d.shape[1] for d, _, _, _ in vids), sum(len(c) for _, c, _, _ in vids)
    dets, keep, scores = np.zeros((frames, cap, 6), dtype=np.float32), np.zeros((frames, cap), dtype=np.uint8), np.zeros((frames, cap), dtype=np.float32)
    starts = [0]
    for d, c, k, s in vids:
        a, b = starts[-1], starts[-1] + len(c)
        dets[a:b] = d[0, 0]
        dets[a:b, :d.shape[1]], keep[a:b, :d.shape[1]], scores[a:b, :d.shape[1]] = d, k, s
        starts.append(b)
    return dets, np.concatenate([c for _, c, _, _ in vids]), starts, keep, scores


def _run(dets, counts, num_classes=30, **kw):
    from diffusionvid_amd import ops
    out = ops.seq_nms_video(torch.from_numpy(np.ascontiguousarray(dets)).cuda(), torch.from_numpy(np.ascontiguousarray(counts)).cuda(), num_classes, **kw)
    return [o.cpu().numpy() for o in out]


def _same(got_keep, got_scores, keep, scores):
    assert np.array_equal(got_keep, keep), "keep differs at %s" % (np.argwhere(got_keep != keep)[:5].tolist(),)
    bad = np.argwhere(got_scores.view(np.uint32) != scores.view(np.uint32))
    assert len(bad) == 0, "score bits differ at %s: %s vs %s" % (bad[:5].tolist(), got_scores[tuple(bad[0])], scores[tuple(bad[0])])


@pytest.mark.parametrize("case", CASES)
def test_kernel_reproduces_the_reference_bit_for_bit(g19, rounds, case):
    keep, scores, status = _run(g19[case + "_dets"], g19[case + "_counts"], return_status=True)
    print(case, "rounds per class:", status[0].tolist())
    _same(keep, scores, g19[case + "_keep"], g19[case + "_scores"])
    assert (status >= 0).all() and (status < (1 << 29)).all()
    assert np.array_equal(status, rounds[case]), "rounds per class: %s, the restatement ran %s" % (status[0].tolist(), rounds[case][0].tolist())


@pytest.mark.parametrize("case", CASES20)
def test_kernel_reproduces_the_bounds_bit_for_bit_and_round_for_round(g20, rounds, case):
    keep, scores, status = _run(g20[case + "_dets"], g20[case + "_counts"], return_status=True)
    print(case, "rounds per class:", status[0].tolist())
    _same(keep, scores, g20[case + "_keep"], g20[case + "_scores"])
    assert np.array_equal(status, rounds[case]), "rounds per class: %s, the restatement ran %s" % (status[0].tolist(), rounds[case][0].tolist())


def test_three_busy_videos_in_one_call_equal_their_single_calls(g20, rounds, busy):
    dets, counts, starts, want_keep, want_scores = busy
    keep, scores, status = _run(dets, counts, video_starts=starts, return_status=True)
    _same(keep, scores, want_keep, want_scores)
    assert np.array_equal(status, np.concatenate([rounds["i%d" % v] for v in range(3)]))
    for v in range(3):
        d, c = g20["i%d_dets" % v], g20["i%d_counts" % v]
        k1, s1, st1 = _run(d, c, return_status=True)
        _same(keep[starts[v]:starts[v + 1], :d.shape[1]], scores[starts[v]:starts[v + 1], :d.shape[1]], k1, s1)
        assert np.array_equal(status[v:v + 1], st1)


def _raw(dets, counts, starts, fill, num_classes=30):
    """dvid_seq_nms_video on a scratch of exactly the bytes it asked for, between two guard bands, the whole allocation (and the
    outputs) filled with `fill` beforehand.  Returns (keep, scores, status, the two guard bands after the call)."""
    from diffusionvid_amd import _lib, ops
    lib = _lib.load()
    d, c = torch.from_numpy(np.ascontiguousarray(dets)).cuda(), torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    table = ops.seq_nms_class_counts(d, c, num_classes).contiguous()
    st = torch.tensor(starts, dtype=torch.int32)
    nv, (F, cap) = len(starts) - 1, dets.shape[:2]
    need = int(lib.dvid_seq_nms_scratch_bytes(_lib.ptr(table), _lib.ptr(st), nv, num_classes))
    assert need == H.scratch_bytes(table.numpy(), starts) > 0 and need % 16 == 0
    buf = torch.full((GUARD + need + GUARD,), fill, dtype=torch.uint8, device="cuda")
    mid = buf[GUARD:GUARD + need]
    assert mid.data_ptr() % 16 == 0
    keep = torch.full((F, cap), fill, dtype=torch.uint8, device="cuda")
    scores = torch.full((F, cap * 4), fill, dtype=torch.uint8, device="cuda").view(torch.float32)
    status = torch.full((nv, num_classes), 0x7f if fill else 0, dtype=torch.int32, device="cuda")
    _lib.call("dvid_seq_nms_video", _lib.ptr(d), _lib.ptr(c), _lib.ptr(table), _lib.ptr(st), nv, cap, num_classes, _lib.ptr(keep), _lib.ptr(scores),
              _lib.ptr(status), mid.data_ptr(), need, _lib.stream_ptr())
    torch.cuda.synchronize()
    return keep.cpu().numpy(), scores.cpu().numpy(), status.cpu().numpy(), buf[:GUARD].cpu().numpy(), buf[GUARD + need:].cpu().numpy()


@pytest.mark.parametrize("case", ["h", "i"])
def test_result_is_independent_of_the_scratch_and_stays_inside_it(g20, rounds, busy, case):
    """the scratch is torch.empty in ops.seq_nms_video: whatever it held, the answer is the fixture's, and no byte outside the size the
    library asked for changes"""
    if case == "h":
        dets, counts, starts, want_keep, want_scores, want_rounds = g20["h_dets"], g20["h_counts"], [0, len(g20["h_counts"])], g20["h_keep"], g20["h_scores"], rounds["h"]
    else:
        dets, counts, starts, want_keep, want_scores = busy
        want_rounds = np.concatenate([rounds["i%d" % v] for v in range(3)])
    for fill in (0x00, 0xFF):
        keep, scores, status, front, back = _raw(dets, counts, starts, fill)
        _same(keep, scores, want_keep, want_scores)
        assert np.array_equal(status, want_rounds), fill
        assert (front == fill).all() and (back == fill).all(), "a guard band of the 0x%02x run changed at %s / %s" % (
            fill, np.nonzero(front != fill)[0][:5].tolist(), np.nonzero(back != fill)[0][:5].tolist())


def test_three_runs_give_the_same_bits(g20, busy):
    """a missing barrier shows as a difference between runs before it shows anywhere else"""
    for dets, counts, starts in ((g20["h_dets"], g20["h_counts"], None), busy[:3]):
        first = _run(dets, counts, video_starts=starts, return_status=True)
        for n in (2, 3):
            again = _run(dets, counts, video_starts=starts, return_status=True)
            for name, a, b in zip(("keep", "scores", "status"), first, again):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), "run %d: %s differs from the first run's" % (n, name)


def _reorder(dets, counts, alternate):
    """every frame's rows with the small class (9) first, or the two classes strictly alternating while both last; each class keeps its
    internal order.  Returns (dets, src): the new row r of frame f is the old row src[f, r]."""
    out, src = dets.copy(), np.tile(np.arange(dets.shape[1]), (dets.shape[0], 1))
    for f in range(dets.shape[0]):
        lab = dets[f, :counts[f], 5]
        small, wide = list(np.nonzero(lab == 9)[0]), list(np.nonzero(lab != 9)[0])
        if alternate:
            order = [r for pair in zip(small, wide) for r in pair] + small[len(wide):] + wide[len(small):]
        else:
            order = small + wide
        assert sorted(order) == list(range(counts[f]))
        src[f, :counts[f]] = order
        out[f, :counts[f]] = dets[f, order]
    return out, src


@pytest.mark.parametrize("alternate", [False, True])
def test_row_order_across_classes_does_not_matter(g20, rounds, alternate):
    dets, src = _reorder(g20["h_dets"], g20["h_counts"], alternate)
    assert not np.array_equal(dets, g20["h_dets"])
    keep, scores, status = _run(dets, g20["h_counts"], return_status=True)
    _same(keep, scores, np.take_along_axis(g20["h_keep"], src, 1), np.take_along_axis(g20["h_scores"], src, 1))
    assert np.array_equal(status, rounds["h"])


def test_one_class_and_1280_classes(g20, rounds):
    dets = g20["g_dets"].copy()
    dets[:, :, 5] = 1                                   # every box of the 304 frames in the one class
    want_keep, want_scores, want_rounds = H.seq_nms_rounds(dets, g20["g_counts"], 1)
    keep, scores, status = _run(dets, g20["g_counts"], 1, return_status=True)
    _same(keep, scores, want_keep, want_scores)
    assert status.shape == (1, 1) and np.array_equal(status, want_rounds) and want_rounds[0, 0] > rounds["g"].max()
    keep, scores, status = _run(g20["h_dets"], g20["h_counts"], 1280, return_status=True)
    _same(keep, scores, g20["h_keep"], g20["h_scores"])
    assert status.shape == (1, 1280) and np.array_equal(status[:, :30], rounds["h"]) and not status[0, 30:].any()


def test_two_videos_in_one_call_equal_their_single_calls(g19):
    da, ca, dc, cc = g19["a_dets"], g19["a_counts"], g19["c_dets"], g19["c_counts"]
    cap = max(da.shape[1], dc.shape[1])
    dets = np.zeros((len(ca) + len(cc), cap, 6), dtype=np.float32)
    dets[:len(ca), :da.shape[1]] = da
    dets[len(ca):, :dc.shape[1]] = dc
    keep, scores = _run(dets, np.concatenate([ca, cc]), video_starts=[0, len(ca), len(ca) + len(cc)])
    ka, sa = _run(da, ca)
    kc, sc = _run(dc, cc)
    _same(keep[:len(ca), :da.shape[1]], scores[:len(ca), :da.shape[1]], ka, sa)
    _same(keep[len(ca):, :dc.shape[1]], scores[len(ca):, :dc.shape[1]], kc, sc)
    assert not keep[:len(ca), da.shape[1]:].any() and not keep[len(ca):, dc.shape[1]:].any()


def test_a_1203_class_call_equals_the_30_class_call(g19):
    k30, s30 = _run(g19["a_dets"], g19["a_counts"], 30)
    k, s, status = _run(g19["a_dets"], g19["a_counts"], 1203, return_status=True)
    _same(k, s, k30, s30)
    assert status.shape == (1, 1203) and not status[0, 30:].any()


def test_seq_nms_boxlists_equals_the_host_composition(g19):
    """engine.seq_nms_boxlists on the GPU against the restatement followed by oracle.postproc's class-aware NMS and clip, as sets of (label,
    box, score) per frame"""
    from diffusionvid_amd.engine.inference import seq_nms_boxlists
    from diffusionvid_amd.structures.bounding_box import BoxList
    from oracle import postproc
    dets, counts = g19["a_dets"], g19["a_counts"]
    size = (640, 360)
    bls = []
    for f in range(len(counts)):
        bl = BoxList(torch.from_numpy(dets[f, :counts[f], :4].copy()), size, mode="xyxy")
        bl.add_field("scores", torch.from_numpy(dets[f, :counts[f], 4].copy()))
        bl.add_field("labels", torch.from_numpy(dets[f, :counts[f], 5].astype(np.int64)))
        bls.append(bl)
    out = seq_nms_boxlists(bls, 30, 0.5)
    keep, scores = H.seq_nms_video(dets, counts, 30)
    assert len(out) == len(bls)
    dropped = 0
    for f, bl in enumerate(out):
        rows = np.nonzero(keep[f])[0]
        b, s, lab = dets[f, rows, :4], scores[f, rows], dets[f, rows, 5].astype(np.int64)
        k = postproc.batched_nms(b, s, lab, 0.5)
        dropped += len(rows) - len(k)
        want = {(int(lab[i]),) + tuple(postproc.clip_to_image(b[i:i + 1], size)[0].tolist()) + (float(s[i]),) for i in k}
        got = {(int(x),) + tuple(bb) + (float(sc),) for x, bb, sc in
               zip(bl.get_field("labels").tolist(), bl.bbox.tolist(), bl.get_field("scores").tolist())}
        assert got == want, f
        assert type(bl) is BoxList and bl.size == size and len(bl) == len(k)
    print("the trailing NMS dropped", dropped, "boxes")


def test_over_limit_calls_are_refused_before_any_launch():
    from diffusionvid_amd import _lib, ops
    dets = torch.zeros((2, ops.NMS_MAX_CANDIDATES + 1, 6), device="cuda")
    counts = torch.zeros((2,), dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.DvidError, match=r"code 3: Seq-NMS: 4097 rows per frame x 30 classes exceed the limits of 4096 rows"):
        ops.seq_nms_video(dets, counts, 30)
    with pytest.raises(_lib.DvidError, match=r"code 3: Seq-NMS: 8 rows per frame x 1281 classes exceed"):
        ops.seq_nms_video(dets[:, :8].contiguous(), counts, ops.MAX_CLASSES + 1)
    # the scratch cap: 300 frames x 4096 boxes of one class need 300 x 4096 x 64 link words = 630 MB ... x 2 videos > 1 GiB
    table = torch.zeros((600, 1), dtype=torch.int32)
    table[:] = 4096
    starts = torch.tensor([0, 300, 600], dtype=torch.int32)
    need = _lib.load().dvid_seq_nms_scratch_bytes(_lib.ptr(table), _lib.ptr(starts), 2, 1)
    assert need == H.scratch_bytes(table.numpy(), [0, 300, 600]) > (1 << 30)
    big = torch.zeros((600, 4096, 6), device="cuda")          # buffers of the true size: a refusal that failed would still stay in bounds
    keep = torch.zeros((600, 4096), dtype=torch.uint8, device="cuda")
    scores = torch.zeros((600, 4096), device="cuda")
    status = torch.zeros((2,), dtype=torch.int32, device="cuda")
    rc = _lib.load().dvid_seq_nms_video(_lib.ptr(big), _lib.ptr(torch.zeros((600,), dtype=torch.int32, device="cuda")), _lib.ptr(table),
                                        _lib.ptr(starts), 2, 4096, 1, _lib.ptr(keep), _lib.ptr(scores), _lib.ptr(status), None, 0, None)
    assert rc == 3 and b"exceed the limit of 1073741824" in _lib.load().dvid_last_error()
    torch.cuda.synchronize()
