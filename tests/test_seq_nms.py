"""TEST.SEQ_NMS, host side and reference pin -- no GPU.

tests/golden/seqnms/g19_seq_nms.npz is what the reference's seq_nms.py returned (tests/golden/make_golden_seqnms.py); the restatement in
tests/_seq_nms_host.py must equal it exactly, and stands in for the kernel where the engine is exercised without a GPU.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

import _seq_nms_host as H

G19 = "seqnms/g19_seq_nms"
CASES = "abcdef"


@pytest.mark.skipif(not os.path.isdir("/root/reference/mega_core"), reason="the reference tree is only present in the build container")
def test_fixture_regenerates_bit_identically(tmp_path):
    env = dict(os.environ, DVID_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_seqnms.py")], check=True, env=env, capture_output=True)
    new, old = np.load(tmp_path / "g19_seq_nms.npz"), golden(G19)
    assert sorted(new.files) == sorted(old.files) and len(old.files) == 4 * len(CASES)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k


def test_fixture_holds_the_cases_it_is_for():
    z = golden(G19)
    assert z["a_dets"].shape[0] == 12 and z["b_dets"].shape[0] == 1 and z["c_dets"].shape[0] == 6 and z["f_dets"].shape[0] == 40
    ta = H.class_counts(z["a_dets"], z["a_counts"], 30)
    assert not ta[:, 8].any() and ta[:4, 4].all() and not ta[4:7, 4].any() and ta[7:, 4].all()          # class 9 empty, class 5 absent in the middle
    assert H.class_counts(z["c_dets"], z["c_counts"], 30)[2, 3] >= 130
    live = np.arange(z["f_dets"].shape[1])[None, :] < z["f_counts"][:, None]
    s64 = np.float32(z["f_dets"][:, :, 4][live].astype(np.float64).sum() / 40)
    assert (z["f_scores"][live] != s64).all()          # the float64 sum gives other bits: case f pins the float32 accumulation


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference_exactly(case):
    z = golden(G19)
    keep, scores = H.seq_nms_video(z[case + "_dets"], z[case + "_counts"], 30)
    assert np.array_equal(keep, z[case + "_keep"])
    assert np.array_equal(scores.view(np.uint32), z[case + "_scores"].view(np.uint32))


def test_header_declares_and_library_exports_the_symbols():
    from diffusionvid_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvid_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("dvid_seq_nms_video", "dvid_seq_nms_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.SIGNATURES and getattr(lib, name) is not None


def test_scratch_size_equals_the_formula():
    from diffusionvid_amd import _lib, ops
    lib = _lib.load()
    z = golden(G19)
    # the fixture's largest table, and two videos of unlike length in one call with empty classes, empty frames and a 64-box word edge
    ta = ops.seq_nms_class_counts(torch.from_numpy(z["c_dets"]), torch.from_numpy(z["c_counts"]), 30)
    assert np.array_equal(ta.numpy(), H.class_counts(z["c_dets"], z["c_counts"], 30))
    rng = np.random.RandomState(3)
    tb = rng.randint(0, 4, size=(9, 5)).astype(np.int32) * rng.randint(0, 2, size=(9, 5)).astype(np.int32)
    tb[2, 1], tb[3, 1], tb[4, 1], tb[:, 3] = 64, 65, 129, 0
    for table, starts in ((ta.numpy(), [0, 6]), (tb, [0, 7, 9]), (tb, [0, 1, 9])):
        t, s = torch.from_numpy(np.ascontiguousarray(table)), torch.tensor(starts, dtype=torch.int32)
        got = lib.dvid_seq_nms_scratch_bytes(_lib.ptr(t), _lib.ptr(s), len(starts) - 1, table.shape[1])
        assert got == H.scratch_bytes(table, starts) > 0
    one = torch.tensor([[3, 0], [0, 3]], dtype=torch.int32)          # no class has boxes in two adjacent frames: nothing to do
    assert lib.dvid_seq_nms_scratch_bytes(_lib.ptr(one), _lib.ptr(torch.tensor([0, 2], dtype=torch.int32)), 1, 2) == 0


# ---- the engine, with the restatement and the oracle's NMS injected ----
def _host_nms(boxes, scores, labels, img_w, img_h, iou):
    """ops.nms_frames_tiled's contract on the host: oracle.postproc's class-aware NMS, survivors in score order, clipped"""
    from oracle import postproc
    n, N = scores.shape
    ob, osc, ol = torch.zeros((n, N, 4)), torch.zeros((n, N)), torch.zeros((n, N), dtype=torch.int32)
    oc = torch.zeros((n,), dtype=torch.int32)
    for f in range(n):
        k = postproc.batched_nms(boxes[f].numpy(), scores[f].numpy(), labels[f].numpy(), iou)
        oc[f] = len(k)
        ob[f, :len(k)] = torch.from_numpy(postproc.clip_to_image(boxes[f].numpy()[k], (img_w, img_h)))
        osc[f, :len(k)], ol[f, :len(k)] = scores[f][k], labels[f][k]
    return ob, osc, ol, oc


def _host_seq_nms(dets, counts, num_classes):
    return H.seq_nms_video(dets.numpy(), counts.numpy(), num_classes)


SIZE = (640, 360)


def _boxlists(dets, counts):
    from diffusionvid_amd.structures.bounding_box import BoxList
    out = []
    for f in range(len(counts)):
        bl = BoxList(torch.from_numpy(dets[f, :counts[f], :4].copy()), SIZE, mode="xyxy")
        bl.add_field("scores", torch.from_numpy(dets[f, :counts[f], 4].copy()))
        bl.add_field("labels", torch.from_numpy(dets[f, :counts[f], 5].astype(np.int64)))
        out.append(bl)
    return out


def _equal(a, b):
    return (type(a) is type(b) and a.size == b.size and torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
            and torch.equal(a.get_field("labels"), b.get_field("labels")))


class _Video:
    """two videos (cases a and d) as a dataset of the reference's item protocol; image id = dataset index"""

    def __init__(self, z):
        self.frames = _boxlists(z["a_dets"], z["a_counts"]) + _boxlists(z["d_dets"], z["d_counts"])
        self.seg = [(f, 12) for f in range(12)] + [(f, 5) for f in range(5)]

    def __getitem__(self, idx):
        f, n = self.seg[idx]
        return {"frame_id": f, "seg_len": n, "end_id": n - 1, "frame_category": 0 if f == 0 else 1, "ref_l": [idx], "idx": idx}, None, [idx, idx + 1]


class _Model:
    """returns canned BoxLists; with look-ahead 2 the first call of a group of two also returns the next frame's, whose own call returns nothing"""

    def __init__(self, video, lookahead, seq_nms):
        from diffusionvid_amd.config import get_cfg
        self.video, self.lookahead, self.infer_batch = video, lookahead, 1
        self.cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), ["TEST.SEQ_NMS", seq_nms], os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
        self.seen = []

    def eval(self):
        return self

    def __call__(self, images):
        idx, f, n = images["idx"], images["frame_id"], images["seg_len"]
        self.seen.append(idx)
        if self.lookahead == 1:
            return [self.video.frames[idx]]
        if f % 2 == 1:
            return []
        return [self.video.frames[idx]] + ([self.video.frames[idx + 1]] if f + 1 < n else [])


@pytest.mark.parametrize("lookahead", [1, 2])
def test_compute_on_dataset_replaces_a_video_on_its_last_call(lookahead):
    from diffusionvid_amd.engine import inference as E
    z = golden(G19)
    video = _Video(z)
    fn = functools.partial(E.seq_nms_boxlists, num_classes=30, nms_thresh=0.5, seq_nms_fn=_host_seq_nms, nms_fn=_host_nms)
    calls = []

    def spy(bls):
        calls.append(len(bls))
        return fn(bls)

    cpu = torch.device("cpu")
    plain = E.compute_on_dataset(_Model(video, lookahead, False), video, range(17), cpu)
    assert sorted(plain) == list(range(17)) and all(_equal(plain[i], video.frames[i]) for i in range(17))          # do_seq_nms off: today's output
    # results change only on a video's last call: up to there they are the detector's own
    want = fn(video.frames[:12]) + fn(video.frames[12:])
    for stop, done in ((11, 0), (12, 1), (16, 1), (17, 2)):
        calls.clear()
        got = E.compute_on_dataset(_Model(video, lookahead, True), video, range(stop), cpu, do_seq_nms=True, seq_nms=spy)
        assert calls == [12, 5][:done] and len(got) >= stop
        for i in got:
            finished = (i < 12 and done >= 1) or done == 2
            assert _equal(got[i], want[i] if finished else video.frames[i]), (stop, i)
    assert any(len(want[i]) < len(video.frames[i]) for i in range(17))
    assert any(not torch.equal(want[i].get_field("scores"), video.frames[i].get_field("scores")[:len(want[i])]) for i in range(12))


def test_seq_nms_boxlists_is_restatement_then_class_nms():
    from diffusionvid_amd.engine import inference as E
    from oracle import postproc
    z = golden(G19)
    dets, counts = z["a_dets"], z["a_counts"]
    out = E.seq_nms_boxlists(_boxlists(dets, counts), 30, 0.5, seq_nms_fn=_host_seq_nms, nms_fn=_host_nms)
    keep, scores = H.seq_nms_video(dets, counts, 30)
    for f, bl in enumerate(out):
        rows = np.nonzero(keep[f])[0]
        k = postproc.batched_nms(dets[f, rows, :4], scores[f, rows], dets[f, rows, 5].astype(np.int64), 0.5)
        assert np.array_equal(bl.bbox.numpy(), postproc.clip_to_image(dets[f, rows[k], :4], SIZE))
        assert np.array_equal(bl.get_field("scores").numpy(), scores[f, rows[k]])
        assert np.array_equal(bl.get_field("labels").numpy(), dets[f, rows[k], 5].astype(np.int64))
    assert E.seq_nms_boxlists([], 30, 0.5, seq_nms_fn=_host_seq_nms, nms_fn=_host_nms) == []


def test_inference_writes_predictions_seq_nms(tmp_path):
    from diffusionvid_amd.engine import inference as E
    z = golden(G19)
    video = _Video(z)
    fn = functools.partial(E.seq_nms_boxlists, num_classes=30, nms_thresh=0.5, seq_nms_fn=_host_seq_nms, nms_fn=_host_nms)
    cpu = torch.device("cpu")
    on, off = tmp_path / "on", tmp_path / "off"
    preds, _ = E.inference(_Model(video, 1, True), video, range(17), cpu, output_folder=str(on), seq_nms=fn)
    assert sorted(os.listdir(on)) == ["predictions_seq_nms.pth"]
    want = fn(video.frames[:12]) + fn(video.frames[12:])
    assert len(preds) == 17 and all(_equal(p, w) for p, w in zip(preds, want))
    preds, _ = E.inference(_Model(video, 1, False), video, range(17), cpu, output_folder=str(off))
    assert sorted(os.listdir(off)) == ["predictions.pth"]
    assert all(_equal(p, f) for p, f in zip(preds, video.frames))
    # byte-identical to what the engine wrote before the key was honoured: the same list through the same writer
    from diffusionvid_amd.data.evaluation import vid_eval
    os.makedirs(tmp_path / "direct")
    vid_eval.save_predictions(video.frames, str(tmp_path / "direct" / "predictions.pth"), None)
    assert open(off / "predictions.pth", "rb").read() == open(tmp_path / "direct" / "predictions.pth", "rb").read()
