"""The backward of the head's tail on the GPU (ops.head_tail_backward; csrc/headtail_bwd.hip) against torch's autograd through
tail.head_tail_host on the CPU, at the library's size (hidden 256, dff 2048) with seeded weights.

Truth: head_tail_host in float64 on the CPU at the case's own shape.  Yardstick: the same function's fp32 run on the CPU.  Measure:
max|got - truth| / max|truth| per tensor, an all-zero truth met exactly.  Bound: max(8 x yardstick, 16 x 2^-24) per tensor.  Every case
prints its yardstick and its measured deviation (profiles/head_tail_grad_parity.txt keeps a run's lines)."""
import functools

import pytest
import torch

import _head_tail_cases as HC

pytestmark = pytest.mark.gpu

from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import tail as T  # noqa: E402

CHUNK = ops.HEAD_TAIL_BWD_ROW_CHUNK          # DVID_HEAD_TAIL_BWD_ROW_CHUNK = 256: the rows of one partial of a weight-gradient sum

# name: (seed, n, M, classes, cond head, d_obj given)
SHAPES = {
    "plain_33": (11, 1, 33, 30, False, False),              # one row past a 32-row tile
    "cond_3x37": (12, 3, 37, 80, True, True),               # image boundaries inside row tiles, C no multiple of 64, three time_emb rows
    "classes_1203": (13, 1, 64, 1203, False, False),
    "classes_1": (14, 1, 64, 1, False, True),
    "chunk_minus_1": (15, 1, CHUNK - 1, 30, False, False),
    "chunk": (16, 1, CHUNK, 30, False, False),
    "chunk_plus_1": (17, 1, CHUNK + 1, 30, False, True),
    "two_chunks_plus_1": (18, 1, 2 * CHUNK + 1, 30, False, False),
    "image_over_a_chunk": (19, 2, CHUNK + 3, 30, True, False),          # the per-image sums of d_scale cross a chunk inside each image
}


def _device_run(case, **kw):
    c = lambda t: None if t is None else t.cuda()
    out = ops.head_tail_backward(c(case["x"]), c(case["boxes_in"]), c(case["time_emb"]), {k: v.cuda() for k, v in case["params"].items()}, cond=c(case["cond"]),
                                 d_logits=c(case["cots"]["logits"]), d_boxes=c(case["cots"]["boxes"]), d_obj=c(case["cots"]["obj"]), **kw)
    outs = {k: out[k] for k in ("logits", "boxes", "obj")}
    grads = {"x": out["d_x"], "time_emb": out["d_time_emb"], **out["param_grads"]}
    if case["cond"] is not None:
        grads["cond"] = out["d_cond"]
    return outs, grads


def _host(case, dtype, **kw):
    return HC.host_run(T, case["x"], case["boxes_in"], case["time_emb"], case["params"], case["cond"], case["cots"], dtype, **kw)


def _compare(name, case, **kw):
    """every forward output and every gradient of the device against the float64 truth, under the bound of the fp32 host run"""
    t_out, t_grad = _host(case, torch.float64, **kw)
    y_out, y_grad = _host(case, torch.float32, **kw)
    g_out, g_grad = _device_run(case, **kw)
    assert sorted(g_grad) == sorted(t_grad)
    failed = []
    for kind, truth, yard, got in (("out", t_out, y_out, g_out), ("grad", t_grad, y_grad, g_grad)):
        for k in truth:
            y, dev = HC.deviation(yard[k], truth[k]), HC.deviation(got[k], truth[k])
            print("%-20s %-4s %-26s max|truth| %.3e  yardstick %.3e  device %.3e  bound %.3e" % (name, kind, k, float(truth[k].abs().max()), y, dev, HC.bound(y)))
            assert got[k].dtype == torch.float32 and got[k].is_cuda
            if dev > HC.bound(y):
                off = (got[k].detach().cpu().double() - truth[k]).abs() > HC.bound(y) * float(truth[k].abs().max())
                failed.append((kind, k, dev, HC.bound(y), "%d of %d entries" % (int(off.sum()), off.numel())))
    assert not failed, failed
    return (t_out, t_grad), (g_out, g_grad)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_gradients_meet_the_float64_host_path(name):
    seed, n, m, c, cond, with_obj = SHAPES[name]
    _compare(name, HC.make_case(seed, n, m, c, cond, with_obj))


def _kink_case():
    """rows above the clamp (bias of dw raised by 8: a mix), dh exactly AT the clamp in every row (weight row 0, bias = the clamp), a
    zero-width box, and a cls tower whose every unit is dead in every row"""
    case = HC.make_case(21, 2, 35, 30, False, True)
    p = case["params"]
    clamp = float(torch.tensor(T.SCALE_CLAMP, dtype=torch.float32))          # representable, so that the fp32 and float64 paths agree at equality
    p["bboxes_delta.bias"] = p["bboxes_delta.bias"].clone()
    p["bboxes_delta.weight"] = p["bboxes_delta.weight"].clone()
    p["bboxes_delta.bias"][2] += 8.0
    p["bboxes_delta.weight"][3] = 0.0
    p["bboxes_delta.bias"][3] = clamp
    p["cls_module.1.bias"] = torch.full_like(p["cls_module.1.bias"], -1e4)
    case["boxes_in"][7, 2] = case["boxes_in"][7, 0]
    return case, clamp


def test_exact_zeros_at_the_kinks():
    case, clamp = _kink_case()
    (t_out, t_grad), (g_out, g_grad) = _compare("kinks", case, scale_clamp=clamp)
    # the truth has the zeros the contract names, so _compare's deviation held the device to them exactly
    for k in ("cls_module.0.weight", "cls_module.1.weight", "cls_module.1.bias", "class_logits.weight"):
        assert not bool(t_grad[k].any()) and not bool(g_grad[k].any()), k
    assert bool(t_grad["class_logits.bias"].any())
    assert bool(t_grad["bboxes_delta.bias"][3] != 0), "at equality the clamp passes the gradient"
    assert float(g_out["boxes"][7, 0]) == float(g_out["boxes"][7, 2]), "a zero-width box stays one"
    # every row clamped in dw, every box of zero height: exact zeros for exactly those terms
    p = case["params"]
    p["bboxes_delta.bias"][2] += 50.0
    case["boxes_in"][:, 3] = case["boxes_in"][:, 1]
    case["cots"]["logits"] = None
    _, grads = _device_run(case, scale_clamp=clamp)
    assert not bool(grads["bboxes_delta.bias"][[1, 2, 3]].any()) and not bool(grads["bboxes_delta.weight"][[1, 2, 3]].any())
    assert bool(grads["bboxes_delta.bias"][0] != 0) and bool(grads["bboxes_delta.weight"][0].any()), "a clamped dw leaves dx its gradient"
    assert not bool(grads["class_logits.bias"].any()), "a null cotangent is zeros"


def test_two_runs_give_the_same_bits_and_autograd_is_the_direct_call():
    seed, n, m, c, cond, with_obj = SHAPES["cond_3x37"]
    case = HC.make_case(seed, n, m, c, cond, with_obj)
    one, two = _device_run(case), _device_run(case)
    for a, b in zip(one, two):
        assert all(torch.equal(a[k], b[k]) for k in a)
    # the torch.autograd.Function path: the same entry point forward and backward
    leaf = lambda t: t.cuda().requires_grad_(True)
    x, te, cd, p = leaf(case["x"]), leaf(case["time_emb"]), leaf(case["cond"]), {k: leaf(v) for k, v in case["params"].items()}
    outs = T.head_tail(x, case["boxes_in"].cuda(), te, p, cd)
    assert all(o.grad_fn is not None for o in outs)
    for o, k in zip(outs, ("logits", "boxes", "obj")):
        assert torch.equal(o, one[0][k])
    sum((case["cots"][k].cuda() * o).sum() for o, k in zip(outs, ("logits", "boxes", "obj"))).backward()
    got = {"x": x.grad, "time_emb": te.grad, "cond": cd.grad, **{k: v.grad for k, v in p.items()}}
    assert sorted(got) == sorted(one[1]) and all(torch.equal(got[k], one[1][k]) for k in got)
    # only what requires grad gets one
    x2 = case["x"].cuda().requires_grad_(True)
    frozen = {k: v.cuda() for k, v in case["params"].items()}
    T.head_tail(x2, case["boxes_in"].cuda(), case["time_emb"].cuda(), frozen, case["cond"].cuda())[0].sum().backward()
    assert x2.grad is not None and all(v.grad is None for v in frozen.values())


def test_forward_only_call_and_optional_outputs():
    seed, n, m, c, cond, with_obj = SHAPES["plain_33"]
    case = HC.make_case(seed, n, m, c, cond, with_obj)
    full = _device_run(case)[0]
    fwd = ops.head_tail_backward(case["x"].cuda(), case["boxes_in"].cuda(), case["time_emb"].cuda(), {k: v.cuda() for k, v in case["params"].items()},
                                 forward_only=True)
    assert sorted(fwd) == ["boxes", "logits", "obj"] and all(torch.equal(fwd[k], full[k]) for k in fwd)
