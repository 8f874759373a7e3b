"""TEST.SEQ_NMS, host side and reference pin -- no GPU.

tests/golden/seqnms/g19_seq_nms.npz is what the reference's seq_nms.py returned (tests/golden/make_golden_seqnms.py); the restatement in
tests/_seq_nms_host.py must equal it exactly, and stands in for the kernel where the engine is exercised without a GPU.
g20_seq_nms_bounds.npz beside it holds the videos that reach the second trip of every loop of the kernel (tests/test_gpu_seq_nms.py).
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
G20 = "seqnms/g20_seq_nms_bounds"
CASES20 = ("g", "h", "i0", "i1", "i2")
WIDE = (63, 64, 65, 128, 129, 256, 257, 320)


@pytest.fixture(scope="module")
def regenerated(tmp_path_factory):
    """one run of the generator for both files"""
    out = tmp_path_factory.mktemp("seqnms")
    env = dict(os.environ, DVID_GOLDEN_OUT=str(out))
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_seqnms.py")], check=True, env=env, capture_output=True)
    return out


@pytest.mark.skipif(not os.path.isdir("/root/reference/mega_core"), reason="the reference tree is only present in the build container")
def test_fixture_regenerates_bit_identically(regenerated):
    new, old = np.load(regenerated / "g19_seq_nms.npz"), golden(G19)
    assert sorted(new.files) == sorted(old.files) and len(old.files) == 4 * len(CASES)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k


@pytest.mark.skipif(not os.path.isdir("/root/reference/mega_core"), reason="the reference tree is only present in the build container")
def test_bounds_fixture_regenerates_bit_identically(regenerated):
    new, old = np.load(regenerated / "g20_seq_nms_bounds.npz"), golden(G20)
    assert sorted(new.files) == sorted(old.files) and len(old.files) == 4 * len(CASES20)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", G20 + ".npz")) < 128 << 10


def test_fixture_holds_the_cases_it_is_for():
    z = golden(G19)
    assert z["a_dets"].shape[0] == 12 and z["b_dets"].shape[0] == 1 and z["c_dets"].shape[0] == 6 and z["f_dets"].shape[0] == 40
    ta = H.class_counts(z["a_dets"], z["a_counts"], 30)
    assert not ta[:, 8].any() and ta[:4, 4].all() and not ta[4:7, 4].any() and ta[7:, 4].all()          # class 9 empty, class 5 absent in the middle
    assert H.class_counts(z["c_dets"], z["c_counts"], 30)[2, 3] >= 130
    live = np.arange(z["f_dets"].shape[1])[None, :] < z["f_counts"][:, None]
    s64 = np.float32(z["f_dets"][:, :, 4][live].astype(np.float64).sum() / 40)
    assert (z["f_scores"][live] != s64).all()          # the float64 sum gives other bits: case f pins the float32 accumulation


def _in_class(dets, counts, c):
    return [np.nonzero(dets[f, :counts[f], 5] == c)[0] for f in range(len(counts))]


def test_bounds_fixture_holds_the_cases_it_is_for():
    """the properties make_golden_seqnms.py asserted when it wrote g20, derived again from the stored arrays and the restatement"""
    z = golden(G20)
    for case in CASES20:
        dets, counts, keep, scores = (z[case + "_" + k] for k in ("dets", "counts", "keep", "scores"))
        live = np.arange(dets.shape[1])[None, :] < counts[:, None]
        assert (dets[:, :, 4] * 8 == np.round(dets[:, :, 4] * 8)).all()          # the coarse score grid: ties are frequent
        assert not keep[~live].any() and not scores[~live].any()
    trace = {c: {} for c in CASES20}
    for c in CASES20:
        H.seq_nms_video(z[c + "_dets"], z[c + "_counts"], 30, trace=trace[c])
    ends = {c: {k: [(root, root + len(p) - 1) for root, p in t] for k, t in trace[c].items()} for c in CASES20}

    # g: long
    dets, counts = z["g_dets"], z["g_counts"]
    assert len(counts) >= 300 and counts[150] == 0 and ((counts >= 2) & (counts <= 8))[np.arange(len(counts)) != 150].all()
    assert ends["g"][3][0][0] > 256 and ends["g"][3][0][1] >= 256          # class 3's first winner lies behind frame 256
    assert ends["g"][7][0] == (160, 209) and (200, 259) in ends["g"][7][1:3]          # two equal sums: the lower frame wins, the other branch follows
    assert all(r > 0 for r, _ in ends["g"][7][:3]) and ends["g"][7][1][1] < ends["g"][7][0][0]          # three roots > 0, one in front of the last root
    r59 = _in_class(dets, counts, 12)[59]
    a, b = (int(np.nonzero(dets[59, r59, 0] == x)[0][0]) for x in (167, 233))
    assert ends["g"][12][0] == (50, 69) and trace["g"][12][0][1][9] == min(a, b)          # two equal predecessors: the lower row stays

    # h: wide
    dets, counts, keep, scores = z["h_dets"], z["h_counts"], z["h_keep"], z["h_scores"]
    tab = H.class_counts(dets, counts, 30)
    assert tuple(tab[:, 4]) == WIDE and (tab[:, 8] > 0).all() and len(trace["h"][5]) >= 8
    rows = _in_class(dets, counts, 5)
    assert any(((keep[f, r] == 1) & (scores[f, r] != dets[f, r, 4]))[256:].any() for f, r in enumerate(rows))
    assert any(i >= 64 for _, p in trace["h"][5] for i in p[:-1])          # a backpointer >= 64 on a taken path
    assert any(not np.array_equal(np.sort(r), np.arange(len(r))) for r in rows)          # the two classes' rows interleave

    # i: busy
    assert [len(z["i%d_counts" % v]) for v in range(3)] == [9, 1, 5]
    assert all(len(trace["i0"].get(c, ())) >= 1 for c in range(1, 31))          # every class of video 0 gives up a path
    t2, tab = trace["i2"], H.class_counts(z["i2_dets"], z["i2_counts"], 30)
    live2 = [c for c in range(1, 31) if t2.get(c)]
    idle2 = [c for c in range(1, 31) if tab[:, c - 1].any() and not t2.get(c)]
    assert len(live2) >= 3 and len(idle2) >= 3
    assert any(not (tab[:-1, c - 1] * tab[1:, c - 1]).any() for c in idle2) and any((tab[:-1, c - 1] * tab[1:, c - 1]).any() for c in idle2)
    for v in range(3):
        dets, counts, keep, scores = (z["i%d_%s" % (v, k)] for k in ("dets", "counts", "keep", "scores"))
        live = np.arange(dets.shape[1])[None, :] < counts[:, None]
        assert (counts < dets.shape[1]).sum() * 2 > len(counts) and (dets[~live][:, 4] > 0).all() and (dets[~live][:, 5] >= 1).all()
        alien = live & ((dets[:, :, 5] < 1) | (dets[:, :, 5] > 30))
        assert (dets[:, :, 5][alien] == 31).any() and (v == 1 or (dets[:, :, 5][alien] == 0).any())
        assert (keep[alien] == 1).all() and np.array_equal(scores[alien], dets[:, :, 4][alien])          # the restatement's: the reference never saw them


@pytest.mark.parametrize("case", CASES20)
def test_restatement_equals_the_reference_exactly_on_the_bounds(case):
    z = golden(G20)
    keep, scores, rounds = H.seq_nms_rounds(z[case + "_dets"], z[case + "_counts"], 30)
    assert np.array_equal(keep, z[case + "_keep"])
    assert np.array_equal(scores.view(np.uint32), z[case + "_scores"].view(np.uint32))
    assert rounds.shape == (1, 30) and (rounds >= 0).all()


def test_rounds_helper_leaves_the_results_alone():
    z = golden(G19)
    keep, scores = H.seq_nms_video(z["a_dets"], z["a_counts"], 30)
    seen, trace = {}, {}
    k2, s2, rounds = H.seq_nms_rounds(z["a_dets"], z["a_counts"], 30)
    k3, s3 = H.seq_nms_video(z["a_dets"], z["a_counts"], 30, progress=seen.__setitem__, trace=trace)
    assert np.array_equal(keep, k2) and np.array_equal(keep, k3) and scores.tobytes() == s2.tobytes() == s3.tobytes()
    assert [int(rounds[0, c - 1]) for c in seen] == list(seen.values()) == [len(trace[c]) for c in seen] and rounds.sum() == sum(seen.values()) > 0


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
