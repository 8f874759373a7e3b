"""Local box-level attention (MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE), host side and reference pin -- no GPU.

The expected values of tests/test_gpu_local_attention.py come from the restatement in tests/_local_ref.py; this file pins that
restatement to the reference's own DynamicHead through tests/golden/local/g18_dynamic_head_local.npz (tests/golden/make_golden_local.py).
"""
import os
import subprocess
import sys
from collections import deque

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, golden_sd
from oracle.head import HeadCfg

import _local_ref as L

RED = HeadCfg(hidden_dim=16, nheads=2, dim_dynamic=4, num_classes=30)
G18 = "local/g18_dynamic_head_local"


def T(a):
    return torch.from_numpy(np.asarray(a))


def _cfg(*opts):
    from diffusionvid_amd.config import get_cfg
    return get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), list(opts), os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))


def test_dynamic_head_constructs_with_local_attention_and_refuses_a_third_stage():
    from diffusionvid_amd.modeling.roi_heads.box_head.box_head import DynamicHead
    for stage in (1, 2):
        h = DynamicHead(_cfg("MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", True, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE", stage))
        assert h.local_enable and h.local_stage == stage and h.proposal_feats_local == [None, None]
    for stage in (0, 3):
        with pytest.raises(NotImplementedError, match="STAGE"):
            DynamicHead(_cfg("MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", True, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE", stage))
    assert DynamicHead(_cfg()).local_stage == 0          # the key off: STAGE (default 3) is not read


def test_synthetic_state_dict_grows_local_stages_without_touching_the_rest():
    from diffusionvid_amd.utils import synthetic
    base = synthetic.make_state_dict(0, blocks=(1, 1, 1, 1))
    zero = synthetic.make_state_dict(0, blocks=(1, 1, 1, 1), local_stages=0)
    assert list(base) == list(zero) and all(torch.equal(base[k], zero[k]) for k in base)
    two = synthetic.make_state_dict(0, blocks=(1, 1, 1, 1), local_stages=2)
    assert all(torch.equal(base[k], two[k]) for k in base)
    new = {k: tuple(v.shape) for k, v in two.items() if k not in base}
    want = {}
    for i in range(2):
        p = f"head.local_attention.{i}."
        want.update({p + "0.in_proj_weight": (768, 256), p + "0.in_proj_bias": (768,), p + "0.out_proj.weight": (256, 256),
                     p + "0.out_proj.bias": (256,), p + "2.weight": (256,), p + "2.bias": (256,)})
    assert new == want


def test_restatement_reproduces_the_reference_head():
    """Tolerances: those of test_oracle_golden.py::test_g5_dynamic_head_extract_and_final for the final stage (rtol 1e-5, atol 1e-4), the
    relative part of a BOX coordinate taken against the box's largest coordinate: x2 = ctr + exp(dh) * h / 2 of a box spanning
    -883 .. -48 px carries the rounding of its 835 px size whatever |x2| is (measured: one such coordinate of 800 off by 6.7e-4 = 0.8e-6
    of the size; every other element inside the plain bound; logits 1.4e-6)."""

    def boxes_close(got, want):
        bound = 1e-4 + 1e-5 * np.abs(want).max(-1, keepdims=True)
        assert (np.abs(got.numpy() - want) <= bound).all(), float((np.abs(got.numpy() - want) / bound).max())

    z = golden(G18)
    sd = golden_sd(z)
    feats = [T(z["p3"]), T(z["p4"]), T(z["p5"])]
    cached = (T(z["ext_logits"]), T(z["ext_boxes"]), T(z["ext_feats"]))
    local = [T(z["loc0"]), T(z["loc1"])]
    for stages in (1, 2):
        fc, fb = L.head_final_local(sd, "head.", feats, T(z["boxes"]), T(z["t"]), RED, cached, local, stages)
        np.testing.assert_allclose(fc.numpy(), z[f"s{stages}_logits"], rtol=1e-5, atol=1e-4)
        boxes_close(fb, z[f"s{stages}_boxes"])
    # only the last stage is observable: stage 1's parameters on the top-25 memory alone give the STAGE 2 result
    q = cached[2]
    two = L.local_attention(sd, "head.", q, local, 2, RED)
    sd1 = {k.replace("local_attention.1.", "local_attention.0."): v for k, v in sd.items() if "local_attention.0." not in k}
    assert torch.equal(two, L.local_attention(sd1, "head.", q, [local[1]], 1, RED))
    # local + global == global alone: the oracle's global-only final stage reproduces the reference's local + global output
    from oracle import head as ohead
    fc, fb = ohead.head_final(sd, "head.", feats, T(z["boxes"]), T(z["t"]), RED, cached=cached, memory=[T(z["mem0"]), T(z["mem1"])])
    np.testing.assert_allclose(fc.numpy(), z["lg_logits"], rtol=1e-5, atol=1e-4)
    boxes_close(fb, z["lg_boxes"])


@pytest.mark.skipif(not os.path.isdir("/root/reference/mega_core"), reason="the reference tree is only present in the build container")
def test_g18_regeneration_is_a_no_op(tmp_path):
    env = dict(os.environ, DVID_GOLDEN_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_local.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    old, new = golden(G18), np.load(os.path.join(tmp_path, "g18_dynamic_head_local.npz"))
    assert sorted(old.files) == sorted(new.files)
    for k in old.files:
        a, b = old[k], new[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind in "fc":          # as test_golden_regeneration.py: BLAS summation order, 1e-5 of the array's scale
            assert float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) <= 1e-5 * max(1.0, float(np.abs(a).max())), k
        else:
            assert np.array_equal(a, b), k


def test_checkpoint_ingests_the_local_attention_names():
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import checkpoint, synthetic
    cfg = _cfg("MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", True, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE", 2, "MODEL.VID.MEGA.GLOBAL.ENABLE", False,
               "MODEL.DEVICE", "cpu")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    m = build_detection_model(cfg).eval()
    names = [k for k in m.state_dict() if ".local_attention." in k]
    assert len(names) == 12
    other = synthetic.make_state_dict(7, blocks=(1, 1, 1, 1), local_stages=2)
    ckpt = {"module." + k: v for k, v in {**m.state_dict(), **other}.items()}          # a DataParallel checkpoint
    missed = checkpoint.load_state_dict(m, ckpt)
    assert not missed
    for k in names:
        assert torch.equal(m.state_dict()[k], other[k]) and k.startswith("head.local_attention.")


@pytest.mark.parametrize("length", [5, 20])
def test_detector_local_queue_follows_fill_idx(length, monkeypatch):
    """The engine stubbed: every frame's top-75 / top-25 rows carry the frame's number.  A 5-frame video (short first delivery: the last
    frame repeated up to the queue length) and a 20-frame one (clamped tail: frame 19 delivered five times in the last call): the row
    blocks of head.proposal_feats_local after each working call name the frames an independent run of the reference's deque rule holds."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    cfg = _cfg("MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", True, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE", 1, "MODEL.VID.MEGA.GLOBAL.ENABLE", False,
               "MODEL.DEVICE", "cpu")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    m = build_detection_model(cfg).eval()
    d, ib = m.hidden_dim, m.infer_batch
    ds = SyntheticVIDDataset([length], cfg, height=32, width=32)
    ds.frame = lambda v, f: torch.full((1, 3, 32, 32), float(f))          # a frame that knows its number

    def fake_extract(frame_id, ref_l, ref_g, ahead, whwh, on_global=None, box_init=None):
        ids = torch.tensor([float(im.tensors[0, 0, 0, 0]) for im in ref_l])
        n = len(ref_l)
        split = {"feats": [torch.zeros(n, 1, 1, d)] * 3, "logits": torch.zeros(n, 1, 30), "boxes": torch.zeros(n, 1, 4), "obj": torch.zeros(n, 1, d),
                 "k1": ids.view(n, 1, 1).expand(n, 75, d).clone(), "k2": ids.view(n, 1, 1).expand(n, 25, d).clone()}
        return split, None, {}

    seen = []
    monkeypatch.setattr(m, "_extract", fake_extract)
    monkeypatch.setattr(m, "_gather_entries", lambda entries: (None, None))
    monkeypatch.setattr(m, "_final_stage", lambda *a, **k: seen.append([t.clone() for t in m.head.proposal_feats_local]) or ["ok"])
    q1, waiting, want = None, [], []
    for idx in range(length):
        item = ds[idx][0]
        ref_l, _, _ = ds.ref_ids(idx)
        out = m(item)
        waiting += ref_l
        if item["frame_id"] % ib:
            assert out == []
            continue
        if item["frame_category"] == 0:
            q1 = deque(maxlen=m.all_frame_interval)
        for i in L.fill_indices(item["frame_category"], item["frame_id"], 0, len(waiting), 0, m.all_frame_interval):
            q1.append(waiting[i])
        want.append(list(q1))
        waiting = []
    assert len(seen) == len(want) == (length + ib - 1) // ib
    for (k1, k2), frames in zip(seen, want):
        assert k1.shape == (len(frames) * 75, d) and k2.shape == (len(frames) * 25, d) and len(frames) == m.all_frame_interval
        assert k1.view(len(frames), 75, d)[:, 0, 0].tolist() == [float(f) for f in frames]
        assert k2.view(len(frames), 25, d)[:, 0, 0].tolist() == [float(f) for f in frames]
        assert bool((k1.view(len(frames), -1).std(dim=1) == 0).all())
    if length == 5:
        assert want == [[0, 1, 2, 3, 4, 4, 4, 4]]
    else:
        assert want[-1] == [16, 17, 18, 19, 19, 19, 19, 19]


def test_c_abi_declares_and_exports_the_local_attention_entry_points():
    from diffusionvid_amd import _lib
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    lib = _lib.load()
    for name, nargs in (("dvid_local_memory_project", 6), ("dvid_local_xattn", 8)):
        assert f"int {name}(dvid_model* m, int stage," in header
        assert len(_lib.SIGNATURES[name][1]) == nargs and getattr(lib, name) is not None
