"""Seq-NMS on the GPU (ops.seq_nms_video, csrc/seqnms.hip) against the reference's own results: tests/golden/seqnms/g19_seq_nms.npz
holds what the reference's seq_nms.py returned on six synthetic videos (tests/golden/make_golden_seqnms.py lists what each is for).
The comparison is exact -- keep equal, scores bit-equal: the kernel computes float32 without contraction and with IEEE division, as
the reference does, so a difference is a wrong kernel, not rounding."""
import numpy as np
import pytest
import torch

from conftest import golden

import _seq_nms_host as H

pytestmark = pytest.mark.gpu
CASES = "abcdef"


@pytest.fixture(scope="module")
def g19():
    return golden("seqnms/g19_seq_nms")


def _run(dets, counts, num_classes=30, **kw):
    from diffusionvid_amd import ops
    out = ops.seq_nms_video(torch.from_numpy(np.ascontiguousarray(dets)).cuda(), torch.from_numpy(np.ascontiguousarray(counts)).cuda(), num_classes, **kw)
    return [o.cpu().numpy() for o in out]


def _same(got_keep, got_scores, keep, scores):
    assert np.array_equal(got_keep, keep), "keep differs at %s" % (np.argwhere(got_keep != keep)[:5].tolist(),)
    bad = np.argwhere(got_scores.view(np.uint32) != scores.view(np.uint32))
    assert len(bad) == 0, "score bits differ at %s: %s vs %s" % (bad[:5].tolist(), got_scores[tuple(bad[0])], scores[tuple(bad[0])])


@pytest.mark.parametrize("case", CASES)
def test_kernel_reproduces_the_reference_bit_for_bit(g19, case):
    keep, scores, status = _run(g19[case + "_dets"], g19[case + "_counts"], return_status=True)
    print(case, "rounds per class:", status[0].tolist())
    _same(keep, scores, g19[case + "_keep"], g19[case + "_scores"])
    assert (status >= 0).all() and (status < (1 << 29)).all()


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
