"""DiffusionDet.head_gradients end to end on the GPU, on the small DTYPE float32 model of test_gpu_inst_interact_e2e (one bottleneck per
ResNet stage, two heads, 100 boxes, two images of different sizes, settled off the ReLU kinks on this batch): the other paths keep their
bits; "param_grads" has exactly the state dict's keys under head.head_series. and head.time_mlp.; every gradient of both heads, time_mlp's
four and d_roi of both heads against torch's autograd in float64 through the host composition of BOTH heads (_self_attn_cases.chain_host:
the mean of the tiles, self_attention_host, inst_interact_host, head_tail_host, per head) fed with the kept tiles, boxes_in, the steps and
the call's own d_logits / d_boxes, its fp32 run being the yardstick; the exact zeros of a head without a loss of its own."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import _self_attn_cases as SC
from test_gpu_head_tail_e2e import BLOCKS, IDS, SMALL, _images, _same_detections, _targets
from test_gpu_inst_interact_e2e import _head_params, _model as _deep_model

pytestmark = pytest.mark.gpu

R, H = 2 * 100, 2
PREFIXES = ("head.head_series.", "head.time_mlp.")
BEHIND_FC = ("class_logits.", "bboxes_delta.", "cls_module.", "reg_module.", "block_time_mlp.")          # what only a head's own loss reaches


@functools.lru_cache(maxsize=None)
def _model(deep):
    """test_gpu_inst_interact_e2e's settled model; without DEEP_SUPERVISION the same weights (the forward does not depend on the key)"""
    if deep:
        return _deep_model()[1]
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    _, model = E._build(1, BLOCKS, "trained_like", extra=SMALL + ["MODEL.DiffusionDet.DEEP_SUPERVISION", False], dtype="float32")
    model.noise_fn = synthetic.noise_fn
    model.load_state_dict({k: v.detach().cpu().clone() for k, v in _deep_model()[1].state_dict().items()})
    return model


def _host(model, out, dtype):
    """torch's autograd through the host composition of both heads -> {state-dict name: gradient, "d_roi": [H, R, 49, 256]}"""
    sd = model.state_dict()
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)
    cpu = lambda t: t.detach().cpu().to(dtype)
    w = {k: leaf(v) for k, v in sd.items() if k.startswith(PREFIXES)}
    tiles = [leaf(out["roi_tiles"][h]) for h in range(H)]
    # time_mlp on the fp32 sinusoid of the steps (Objective.time_embedding's arithmetic), cast
    steps = torch.tensor([model.objective.train_step(i) for i in IDS], dtype=torch.int64)
    half = 128
    arg = steps.to(torch.float32)[:, None] * torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000.0) / (half - 1)))[None, :]
    emb = torch.cat((arg.sin(), arg.cos()), dim=-1).to(dtype)
    t = lambda k: w["head.time_mlp." + k]
    time_emb = F.linear(F.gelu(F.linear(emb, t("1.weight"), t("1.bias"))), t("3.weight"), t("3.bias"))
    heads = [_head_params(w, h, lambda k: True) for h in range(H)]
    boxes_in = [cpu(out["boxes_in"][h]).reshape(R, 4) for h in range(H)]
    logits, boxes = SC.chain_host(tiles, cpu(out["boxes_in"][0]), time_emb, heads, H, boxes_in=boxes_in)
    S = out["d_logits"].shape[0]
    loss = 0
    for s in range(S):          # the kept head outputs, the last head's last
        h = H - S + s
        loss = loss + (cpu(out["d_logits"][s]).reshape(R, -1) * logits[h]).sum() + (cpu(out["d_boxes"][s]).reshape(R, 4) * boxes[h]).sum()
    loss.backward()
    return {"d_roi": torch.stack([x.grad for x in tiles]), **{k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in w.items()}}


def _check(model, out, label):
    sd = model.state_dict()
    want = {k for k in sd if k.startswith(PREFIXES)}
    assert set(out["param_grads"]) == want and "partial" not in out
    assert all(v.shape == sd[k].shape and v.dtype == torch.float32 and v.is_cuda for k, v in out["param_grads"].items())
    assert tuple(out["d_roi"].shape) == (H, R, 49, 256) == tuple(out["roi_tiles"].shape) and tuple(out["boxes_in"].shape) == (H, 2, 100, 4)
    truth, yard = _host(model, out, torch.float64), _host(model, out, torch.float32)
    got = {"d_roi": out["d_roi"], **out["param_grads"]}
    failed = []
    for k in sorted(truth):
        y, dev = SC.deviation(yard[k], truth[k]), SC.deviation(got[k], truth[k])
        print("%-5s %-56s max|truth| %.3e  yardstick %.3e  device %.3e  bound %.3e" % (label, k, float(truth[k].abs().max()), y, dev, SC.bound(y)))
        if dev > SC.bound(y):
            failed.append((k, dev, SC.bound(y)))
    assert not failed, failed
    return truth


def test_head_gradients_meets_autograd_through_both_heads_and_disturbs_nothing():
    model = _model(True)
    before = model.detect_images(_images(), IDS)
    losses = model.compute_losses(_images(), _targets(), IDS)
    through = {t: model.loss_gradients(_images(), _targets(), IDS, through=t) for t in ("outputs", "tail", "interact")}
    out = model.head_gradients(_images(), _targets(), IDS, roi_gradients=True)
    lean = model.head_gradients(_images(), _targets(), IDS)
    # detect_images, loss_gradients(through=...) for all three values and compute_losses keep their bits
    _same_detections(before, model.detect_images(_images(), IDS))
    assert model.compute_losses(_images(), _targets(), IDS) == losses == out["losses"]
    for t, old in through.items():
        new = model.loss_gradients(_images(), _targets(), IDS, through=t)
        if t == "outputs":
            assert new[0] == old[0] and torch.equal(new[1], old[1]) and torch.equal(new[2], old[2])
            continue
        assert sorted(new) == sorted(old) and new["losses"] == old["losses"]
        for k, v in old.items():
            if isinstance(v, dict) and k != "losses":
                assert sorted(new[k]) == sorted(v) and all(torch.equal(new[k][n], v[n]) for n in v), (t, k)
            elif torch.is_tensor(v):
                assert torch.equal(new[k], v), (t, k)
    inter = through["interact"]
    assert torch.equal(out["d_logits"], inter["d_logits"]) and torch.equal(out["d_boxes"], inter["d_boxes"])
    assert torch.equal(out["roi_tiles"], inter["roi_tiles"]) and torch.equal(out["boxes_in"], inter["boxes_in"])
    # without roi_gradients: the same gradients, no hand-over
    assert sorted(lean) == ["d_boxes", "d_logits", "losses", "param_grads"]
    assert all(torch.equal(lean["param_grads"][k], v) for k, v in out["param_grads"].items())
    truth = _check(model, out, "deep")
    # head 0's own-output terms were "partial": with the next head's path through pro_features they are another, the complete, gradient
    for k, part in inter["partial"].items():
        if k.startswith("head.head_series.0.") and k.split(".", 3)[3].startswith(("linear1.", "inst_interact.")):
            assert not torch.equal(out["param_grads"][k], part), k
            assert SC.deviation(part, truth[k]) > SC.bound(0.0), k          # the partial term alone is not the gradient
    assert not model.training and len(model._graphs) == 0


def test_without_deep_supervision_the_earlier_head_learns_through_the_next():
    model = _model(False)
    out = model.head_gradients(_images(), _targets(), IDS, roi_gradients=True)
    assert out["d_logits"].shape[0] == 1
    truth = _check(model, out, "last")
    for k, v in out["param_grads"].items():
        if k.startswith("head.head_series.0."):
            name = k.split(".", 3)[3]
            if name.startswith(BEHIND_FC):
                assert not bool(v.any()) and not bool(truth[k].any()), k          # exact zeros, in truth and on the device
            elif name.startswith(("self_attn.", "inst_interact.", "linear1.")):
                assert bool(v.any()) and bool(truth[k].any()), k


def test_a_float16_model_refuses_by_key():
    import test_gpu_e2e as E
    _, model = E._build(1, BLOCKS, "trained_like", extra=SMALL, dtype="float16")
    with pytest.raises(NotImplementedError, match="head_gradients: needs DTYPE float32"):
        model.head_gradients(_images(), _targets(), IDS)
