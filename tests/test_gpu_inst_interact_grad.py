"""The backward of the head's instance interaction on the GPU (ops.inst_interact_backward; csrc/interact_bwd.hip) against torch's autograd
through interact.inst_interact_host on the CPU, at the library's size (hidden 256, dim_dynamic 64, 7 x 7 bins) with seeded weights.

Truth: inst_interact_host in float64 on the CPU at the case's own shape.  Yardstick: the same function's fp32 run on the CPU.  Measure:
max|got - truth| / max|truth| per tensor, an all-zero truth met exactly.  Bound: max(8 x yardstick, 16 x 2^-24) per tensor.  Every case
prints its yardstick and its measured deviation (profiles/inst_interact_grad_parity.txt keeps a run's lines)."""
import pytest
import torch

import _inst_interact_cases as IC

pytestmark = pytest.mark.gpu

from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import interact as I  # noqa: E402

SLAB = ops.INST_BWD_ROW_SLAB          # DVID_INST_BWD_ROW_SLAB: the rows whose dynamic parameters exist at a time

# name: (seed, R); each size is the smallest at which one mechanism can fail
SHAPES = {
    "one_box": (11, 1),                      # a reduction chunk of one row
    "rows_3x37": (12, 111),                  # no multiple of the 64-row GEMM tile
    "chunk_plus_1": (13, 257),               # one row into the second 256-row chunk
    "slab_plus_1": (14, SLAB + 1),           # one row into the second slab
}


def _device_run(case, params=None, **kw):
    kw.setdefault("d_y", case["d_y"].cuda())
    out = ops.inst_interact_backward(case["p"].cuda(), case["roi"].cuda(), {k: v.cuda() for k, v in (params or case["params"]).items()}, **kw)
    grads = {"p": out["d_p"], "roi": out["d_roi"], **out["param_grads"]}
    return out["y"], grads


def _report(name, truth, yard, got):
    """every tensor of `truth` against `got` under the bound of its yardstick; -> the misses"""
    failed = []
    for k in truth:
        dev, b = IC.deviation(got[k], truth[k]), IC.bound(yard[k])
        print("%-14s %-36s max|truth| %.3e  yardstick %.3e  device %.3e  bound %.3e" % (name, k, float(truth[k].abs().max()), yard[k], dev, b))
        assert got[k].dtype == torch.float32 and got[k].is_cuda
        if dev > b:
            off = (got[k].detach().cpu().double() - truth[k]).abs() > b * float(truth[k].abs().max())
            failed.append((k, dev, b, "%d of %d entries" % (int(off.sum()), off.numel())))
    return failed


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_gradients_meet_the_float64_host_path(name):
    seed, R = SHAPES[name]
    y64, g64, yard = IC.truth(seed, R)
    y, grads = _device_run(IC.make_case(seed, R))
    assert sorted(grads) == sorted(g64)
    failed = _report(name, {"y": y64, **g64}, yard, {"y": y, **grads})
    assert not failed, failed


def test_exact_zeros_at_the_kinks():
    """a dead unit (weight 0, bias 0: a pre-activation of exactly 0 in every row) in each of the three LayerNorms: the truth has exact zeros
    there and the deviation holds the device to them; then a d_y of zeros gives all-zero gradients, exactly"""
    case = IC.make_case(21, 37)
    p = {k: v.clone() for k, v in case["params"].items()}
    for name, unit in (("inst_interact.norm1", 5), ("inst_interact.norm2", 77), ("inst_interact.norm3", 130)):
        p[name + ".weight"][unit] = 0.0
        p[name + ".bias"][unit] = 0.0
    y64, g64 = IC.host_run(I, case["p"], case["roi"], p, case["d_y"], torch.float64)
    y32, g32 = IC.host_run(I, case["p"], case["roi"], p, case["d_y"], torch.float32)
    yard = {"y": IC.deviation(y32, y64), **{k: IC.deviation(g32[k], g64[k]) for k in g64}}
    y, grads = _device_run(case, p)
    failed = _report("dead_units", {"y": y64, **g64}, yard, {"y": y, **grads})
    assert not failed, failed
    # (a LayerNorm's backward spreads over its units, so the cotangent in FRONT of a dead unit's LayerNorm is not zero: only what the dead
    # unit's own output multiplies is)
    for tensors in (g64, grads):
        assert tensors["inst_interact.norm1.weight"][5] == 0 and tensors["inst_interact.norm1.bias"][5] == 0
        assert tensors["inst_interact.norm2.weight"][77] == 0 and tensors["inst_interact.norm2.bias"][77] == 0
        assert tensors["inst_interact.norm3.weight"][130] == 0 and tensors["inst_interact.norm3.bias"][130] == 0
        assert tensors["inst_interact.norm2.weight"][78] != 0 and tensors["inst_interact.norm1.bias"][6] != 0
        assert not bool(tensors["inst_interact.out_layer.weight"].reshape(256, 49, 256)[:, :, 77].any())          # F2's unit 77 is 0 in every row
        w2 = tensors["inst_interact.dynamic_layer.weight"][64 * 256:].reshape(64, 256, 256)          # param2 [64][256]: rows j * 256 + c
        b2 = tensors["inst_interact.dynamic_layer.bias"][64 * 256:].reshape(64, 256)
        assert not bool(w2[5].any()) and not bool(b2[5].any()) and bool(w2[6].any()) and bool(b2[6].any())          # F1's unit 5 is 0 in every row
    _, zero = _device_run(case, d_y=torch.zeros_like(case["d_y"]).cuda())
    _, null = _device_run(case, d_y=None)
    for k in zero:
        assert not bool(zero[k].any()) and not bool(null[k].any()), k


def test_two_runs_give_the_same_bits_and_autograd_is_the_direct_call():
    seed, R = SHAPES["chunk_plus_1"]
    case = IC.make_case(seed, R)
    one, two = _device_run(case), _device_run(case)
    assert torch.equal(one[0], two[0]) and all(torch.equal(one[1][k], two[1][k]) for k in one[1])
    # the torch.autograd.Function path: the same entry point forward and backward
    leaf = lambda t: t.cuda().requires_grad_(True)
    p, roi, w = leaf(case["p"]), leaf(case["roi"]), {k: leaf(v) for k, v in case["params"].items()}
    y = I.inst_interact(p, roi, w)
    assert y.grad_fn is not None and torch.equal(y, one[0])
    (case["d_y"].cuda() * y).sum().backward()
    got = {"p": p.grad, "roi": roi.grad, **{k: v.grad for k, v in w.items()}}
    assert sorted(got) == sorted(one[1]) and all(torch.equal(got[k], one[1][k]) for k in got)
    # only what requires grad gets one
    p2 = case["p"].cuda().requires_grad_(True)
    frozen = {k: v.cuda() for k, v in case["params"].items()}
    roi2 = case["roi"].cuda()
    I.inst_interact(p2, roi2, frozen).sum().backward()
    assert p2.grad is not None and roi2.grad is None and all(v.grad is None for v in frozen.values())


def test_forward_only_call_and_optional_d_roi():
    seed, R = SHAPES["rows_3x37"]
    case = IC.make_case(seed, R)
    y, grads = _device_run(case)
    y2, without = _device_run(case, want_d_roi=False)
    assert without["roi"] is None and torch.equal(y, y2)
    assert all(torch.equal(without[k], grads[k]) for k in grads if k != "roi")
    fwd = ops.inst_interact_backward(case["p"].cuda(), case["roi"].cuda(), {k: v.cuda() for k, v in case["params"].items()}, forward_only=True)
    assert sorted(fwd) == ["y"] and torch.equal(fwd["y"], y)
