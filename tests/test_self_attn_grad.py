"""The backward of the head's self-attention + norm1 and the chain over the heads without a GPU: the C ABI's declaration and refusals, the
scratch query, the host restatement (attention.self_attention_host under torch's autograd) against the gradients the reference's own RCNNHead
backpropagates (tests/golden/self_attn/link.npz), the host composition of all heads against the reference's own DynamicHead.forward
(chain.npz: d_obj, the mean of the tiles, the boxes detached, time_mlp), self_attention on CPU tensors, and what head_gradients refuses."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import _self_attn_cases as SC

from diffusionvid_amd import _lib
from diffusionvid_amd.modeling.roi_heads.box_head import attention as A


def test_abi_carries_the_self_attention_entry_points():
    """fails before the self-attention backward exists: the header, _lib.SIGNATURES and the library carry the two symbols, dvid_version() >= 16"""
    with open(os.path.join(ROOT, "include", "dvid_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ("dvid_self_attn_backward", "dvid_self_attn_backward_scratch_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        decl = header.split(" %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1])
    assert lib.dvid_version() >= 16
    doc = header.split("dvid_self_attn_backward (dvid_version >= 16)")[1].split("*/")[0]
    at = [doc.index(" %s" % k) for k in A.PARAM_NAMES]          # the documented order of the pointer table is attention.PARAM_NAMES
    assert at == sorted(at) and len(A.PARAM_NAMES) == 6
    for words in ("no atomics", "Padded keys", "an exact 0", "DVID_HEAD_TAIL_BWD_ROW_CHUNK", "65535 images"):
        assert words in doc, words


def test_the_scratch_query_needs_no_device():
    """it grows linearly in rows and returns -1 for a refused size"""
    q = _lib.load().dvid_self_attn_backward_scratch_bytes
    assert 0 < q(1, 1) < q(2, 300)
    for n, m in ((0, 5), (5, 0), (1, 4097), (65536, 1), (1024, 1025)):
        assert q(n, m) == -1, (n, m)
    assert q(1, 4096) > 0 and q(65535, 1) > 0 and q(1024, 1024) > 0
    per_row = (q(8, 1024) - q(4, 1024)) / (4 * 1024)
    assert abs((q(16, 1024) - q(8, 1024)) / (8 * 1024) - per_row) < 1e-9 and q(4, 1024) == q(8, 512)          # rows, however they are split
    # qkv and its cotangent, seven [256] rows, the statistics, and in_proj's weight-gradient partial per 256-row chunk
    assert (2 * 768 + 7 * 256) * 4 <= per_row <= (2 * 768 + 8 * 256 + 64) * 4 + 768 * 256 * 4 / 256


def test_the_entry_point_refuses_before_any_launch():
    """sizes first, with the numbers in the message; then null pointers (no device is touched: every pointer here is null)"""
    lib = _lib.load()

    def refused(n=2, m=5, hidden=256, nheads=8, n_params=6):
        rc = lib.dvid_self_attn_backward(None, n, m, hidden, nheads, None, n_params, *([None] * 5), 0, None)
        return rc, lib.dvid_last_error().decode()

    for kw, code, words in (({"hidden": 128}, 3, "hidden size 128"), ({"nheads": 4}, 3, "4 heads"), ({"m": 4097}, 3, "4097 rows per image"),
                            ({"n": 1024, "m": 1025}, 3, "1049600 rows"), ({"n": 65536, "m": 1}, 3, "65536 images"), ({"n": 0}, 1, "0 images"),
                            ({"m": 0}, 1, "of 0 rows"), ({"n_params": 12}, 1, "12 parameter pointers"), ({}, 1, "null pointer")):
        rc, msg = refused(**kw)
        assert rc == code and words in msg and msg.startswith("self-attention backward:"), (kw, rc, msg)


def test_fixtures_hold_the_link_and_the_chain():
    link, chain = SC.link_fixture(), SC.chain_fixture()
    assert link["in"]["x"].shape == (14, 16) == link["in"]["G_y"].shape and int(link["in"]["n"]) == 2
    assert sorted(link["sd"]) == sorted(A.PARAM_NAMES) and link["sd"]["self_attn.in_proj_weight"].shape == (48, 16)
    assert sorted(link["grad"]) == sorted(["x"] + list(link["sd"])) and sorted(link["dev32"]) == sorted(list(link["grad"]) + ["y"])
    assert chain["in"]["tiles"].shape == (3, 14, 49, 16) == chain["grad"]["tiles"].shape and chain["in"]["boxes"].shape == (2, 7, 4)
    assert sorted(chain["grad"]) == sorted(["tiles"] + list(chain["sd"]))
    assert all(k.startswith(("head_series.", "time_mlp.")) for k in chain["sd"]) and len([k for k in chain["sd"] if k.startswith("time_mlp.")]) == 4
    assert {k.split(".")[1] for k in chain["sd"] if k.startswith("head_series.")} == {"0", "1", "2"}
    for name in ("link.npz", "chain.npz"):
        assert os.path.getsize(os.path.join(SC.GOLDEN, name)) < 1 << 20


@pytest.mark.skipif(not os.path.isdir("/root/reference/mega_core"), reason="the reference tree is only present in the build container")
def test_the_generator_reproduces_the_committed_fixtures():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_self_attn_grads.py"), "--check"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "fixtures reproduced" in r.stdout, r.stderr[-2000:]


def _meets(got, want, dev32, exact):
    """float64 (`exact`): the stored truth is the reference's float64 run rounded to float32, so the result is rounded the same way before the
    1e-10 comparison.  fp32: within the bound of the reference's own fp32 run, per tensor, and within 2 x that yardstick (floored at 2^-24),
    as test_inst_interact_grad reads it"""
    assert sorted(got) == sorted(want)
    for k, v in got.items():
        dev, yard = SC.deviation(v.float(), want[k]), float(dev32[k])
        if exact:
            assert v.dtype == torch.float64 and dev <= 1e-10, (k, dev)
        else:
            assert v.dtype == torch.float32 and dev <= SC.bound(yard) and dev <= 2 * max(yard, 2.0 ** -24), (k, dev, yard)


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_self_attention_host_meets_the_reference(dtype):
    fx = SC.link_fixture()
    leaf = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)
    x, w = leaf(fx["in"]["x"]), {k: leaf(v) for k, v in fx["sd"].items()}
    y = A.self_attention_host(x, int(fx["in"]["n"]), w, nheads=2)
    (torch.from_numpy(fx["in"]["G_y"]).to(dtype) * y).sum().backward()
    got = {"y": y.detach(), "x": x.grad, **{k: v.grad for k, v in w.items()}}
    _meets(got, {"y": fx["out"]["y"], **fx["grad"]}, fx["dev32"], dtype == torch.float64)


def _chain(dtype, deep=True):
    """the host composition of the three heads on the chain fixture's inputs -> (logits, boxes, {tiles, <parameter>: gradient})"""
    fx = SC.chain_fixture()
    leaf = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)
    w = {k: leaf(v) for k, v in fx["sd"].items()}
    tiles = [leaf(t) for t in fx["in"]["tiles"]]
    time_in = torch.from_numpy(fx["in"]["time_in"]).to(dtype)          # the fp32 sinusoid, cast: what the reference's time_mlp saw
    time_emb = F.linear(F.gelu(F.linear(time_in, w["time_mlp.1.weight"], w["time_mlp.1.bias"])), w["time_mlp.3.weight"], w["time_mlp.3.bias"])
    heads = [{k[len("head_series.%d." % h):]: v for k, v in w.items() if k.startswith("head_series.%d." % h)} for h in range(3)]
    logits, boxes = SC.chain_host(tiles, torch.from_numpy(fx["in"]["boxes"]).to(dtype), time_emb, heads, 3, nheads=2)
    logits, boxes = torch.stack(logits).reshape(3, 2, 7, -1), torch.stack(boxes).reshape(3, 2, 7, 4)
    own = slice(None) if deep else slice(2, 3)
    ((torch.from_numpy(fx["in"]["G_logits"]).to(dtype)[own] * logits[own]).sum() + (torch.from_numpy(fx["in"]["G_boxes"]).to(dtype)[own] * boxes[own]).sum()).backward()
    return logits.detach(), boxes.detach(), {"tiles": torch.stack([t.grad for t in tiles]), **{k: v.grad for k, v in w.items()}}


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_the_host_composition_meets_the_references_own_forward_over_all_heads(dtype):
    """the chain's wiring is the reference's: the mean of the tiles in front of head 0, a head's obj_features as the next head's x (d_obj),
    the boxes detached between heads, time_mlp under all heads"""
    fx = SC.chain_fixture()
    logits, boxes, grads = _chain(dtype)
    _meets({"logits": logits, "boxes": boxes, **grads}, {**fx["out"], **fx["grad"]}, fx["dev32"], dtype == torch.float64)


def test_a_head_without_a_loss_of_its_own_gets_exact_zeros_behind_fc_feature():
    """without the earlier heads' own terms (no DEEP_SUPERVISION) what lies behind their fc_feature sees nothing, and what lies in front of
    their obj_features still does -- through the next head's self-attention"""
    _, _, grads = _chain(torch.float64, deep=False)
    for h in (0, 1):
        for k, v in grads.items():
            if k.startswith("head_series.%d." % h):
                dead = k.split(".", 2)[2].startswith(("class_logits.", "bboxes_delta.", "cls_module.", "reg_module.", "block_time_mlp."))
                assert bool(v.any()) != dead, k
    assert all(bool(grads[k].any()) for k in grads if k.startswith(("head_series.2.", "time_mlp."))) and bool(grads["tiles"][0].any())


def test_self_attention_on_cpu_tensors_is_autograd_on_the_host_path():
    c = SC.make_case(34, 3, 37)
    _, want = SC.host_run(A, c["x"], 3, c["params"], c["d_y"], torch.float32)
    leaf = lambda t: t.clone().requires_grad_(True)
    x, w = leaf(c["x"]), {k: leaf(v) for k, v in c["params"].items()}
    (c["d_y"] * A.self_attention(x, 3, w)).sum().backward()
    got = {"x": x.grad, **{k: v.grad for k, v in w.items()}}
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
    # the restatement is nn.MultiheadAttention's function
    mha = torch.nn.MultiheadAttention(256, 8)
    with torch.no_grad():
        for name, k in (("in_proj_weight", "self_attn.in_proj_weight"), ("in_proj_bias", "self_attn.in_proj_bias")):
            getattr(mha, name).copy_(c["params"][k])
        mha.out_proj.weight.copy_(c["params"]["self_attn.out_proj.weight"]), mha.out_proj.bias.copy_(c["params"]["self_attn.out_proj.bias"])
        seq = c["x"].reshape(3, 37, 256).permute(1, 0, 2)
        y = F.layer_norm(seq + mha(seq, seq, seq)[0], (256,), c["params"]["norm1.weight"], c["params"]["norm1.bias"]).permute(1, 0, 2).reshape(111, 256)
        assert SC.deviation(A.self_attention_host(c["x"], 3, c["params"]), y.double()) < 1e-5


def test_what_head_gradients_refuses():
    """each by key, before an engine exists; loss_gradients and its THROUGH stay as they are"""
    from test_head_tail_grad import _model
    from diffusionvid_amd.structures.bounding_box import BoxList
    target = BoxList(torch.tensor([[4.0, 4.0, 20.0, 20.0]]), (32, 32), mode="xyxy")
    target.add_field("labels", torch.ones(1, dtype=torch.int64))
    batch = ([torch.zeros(3, 32, 32)], [target])
    model = _model(["DTYPE", "float16"])
    assert model.objective.THROUGH == ("outputs", "tail", "interact")
    with pytest.raises(NotImplementedError, match=r"head_gradients: needs DTYPE float32.*float16"):
        model.head_gradients(*batch, roi_gradients=True)
    assert model._engine is None
    model = _model(["DTYPE", "float32", "MODEL.DiffusionDet.DROPOUT", 0.1])
    with pytest.raises(NotImplementedError, match=r"head_gradients: MODEL\.DiffusionDet\.DROPOUT is 0\.1"):
        model.head_gradients(*batch)
    assert model._engine is None
    model = _model(["DTYPE", "float32"])
    with pytest.raises(NotImplementedError, match=r"head_gradients: the video item dict"):
        model.head_gradients({"cur": batch[0][0]}, batch[1])
    assert model._engine is None
    model = _model(["DTYPE", "float32", "MODEL.DiffusionDet.USE_FED_LOSS", True])
    with pytest.raises(NotImplementedError, match=r"USE_FED_LOSS"):
        model.head_gradients(*batch)
    assert model._engine is None
