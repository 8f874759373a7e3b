"""The backward of the head's self-attention + norm1 on the GPU (ops.self_attn_backward; csrc/selfattn_bwd.hip) against torch's autograd
through attention.self_attention_host on the CPU, at the library's size (hidden 256, 8 heads of 32) with seeded weights.

Truth: self_attention_host in float64 on the CPU at the case's own shape.  Yardstick: the same function's fp32 run on the CPU.  Measure:
max|got - truth| / max|truth| per tensor, an all-zero truth met exactly.  Bound: max(8 x yardstick, 16 x 2^-24) per tensor.  Every case
prints its yardstick and its measured deviation (profiles/self_attn_grad_parity.txt keeps a run's lines)."""
import pytest
import torch

import _self_attn_cases as SC

pytestmark = pytest.mark.gpu

from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import attention as A  # noqa: E402

# name: (seed, n, m, kind); each size is the smallest at which one mechanism can fail.  The attention's tile is 32 keys by 32 queries.
SHAPES = {
    "one_key": (31, 1, 1, "norm"),                # softmax of one key: dQ and dK are exact zeros
    "short_tile": (32, 2, 31, "norm"),            # a short key tile whose padding is followed by the next image's rows
    "tile_plus_1": (33, 2, 33, "mean"),           # one key into the second tile; the second image starts at an unaligned row
    "rows_3x37": (34, 3, 37, "norm"),             # 111 rows, no multiple of the 64-row GEMM tile
    "chunk_plus_1": (35, 1, 257, "norm"),         # one row into the second 256-row reduction chunk
    "default_300": (36, 2, 300, "mean"),          # the default proposal count
    "peaked": (37, 2, 40, "peaked"),              # scores spanning more than 100 units
}


def _device_run(case, **kw):
    kw.setdefault("d_y", case["d_y"].cuda())
    out = ops.self_attn_backward(case["x"].cuda(), case["n"], {k: v.cuda() for k, v in case["params"].items()}, **kw)
    return out["y"], {"x": out["d_x"], **out["param_grads"]}


def _report(name, truth, yard, got):
    """every tensor of `truth` against `got` under the bound of its yardstick; -> the misses"""
    failed = []
    for k in truth:
        dev, b = SC.deviation(got[k], truth[k]), SC.bound(yard[k])
        print("%-14s %-28s max|truth| %.3e  yardstick %.3e  device %.3e  bound %.3e" % (name, k, float(truth[k].abs().max()), yard[k], dev, b))
        assert got[k].dtype == torch.float32 and got[k].is_cuda
        if dev > b:
            failed.append((k, dev, b))
    return failed


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_gradients_meet_the_float64_host_path(name):
    seed, n, m, kind = SHAPES[name]
    y64, g64, yard = SC.truth(seed, n, m, kind)
    case = SC.make_case(seed, n, m, kind)
    if kind == "peaked":
        s = SC.scores(case["x"], n, case["params"])
        assert float(s.max()) > 89 and float(s.max() - s.min()) > 100          # exp(S) alone overflows fp32
    y, grads = _device_run(case)
    assert sorted(grads) == sorted(g64)
    failed = _report(name, {"y": y64, **g64}, yard, {"y": y, **grads})
    assert not failed, failed
    if name == "one_key":          # P = 1: dS = dP - delta = 0, so nothing reaches q and k, in truth and on the device
        for tensors in (g64, grads):
            assert not bool(tensors["self_attn.in_proj_weight"][:512].any()) and not bool(tensors["self_attn.in_proj_bias"][:512].any())
            assert bool(tensors["self_attn.in_proj_weight"][512:].any()) and bool(tensors["self_attn.in_proj_bias"][512:].any())


def test_a_zero_and_a_null_cotangent_give_exact_zeros():
    case = SC.make_case(*SHAPES["rows_3x37"])
    _, zero = _device_run(case, d_y=torch.zeros_like(case["d_y"]).cuda())
    _, null = _device_run(case, d_y=None)
    for k in zero:
        assert not bool(zero[k].any()) and not bool(null[k].any()), k


def test_two_runs_give_the_same_bits_and_autograd_is_the_direct_call():
    case = SC.make_case(*SHAPES["chunk_plus_1"])
    one, two = _device_run(case), _device_run(case)
    assert torch.equal(one[0], two[0]) and all(torch.equal(one[1][k], two[1][k]) for k in one[1])
    # the torch.autograd.Function path: the same entry point forward and backward
    leaf = lambda t: t.cuda().requires_grad_(True)
    x, w = leaf(case["x"]), {k: leaf(v) for k, v in case["params"].items()}
    y = A.self_attention(x, case["n"], w)
    assert y.grad_fn is not None and torch.equal(y, one[0])
    (case["d_y"].cuda() * y).sum().backward()
    got = {"x": x.grad, **{k: v.grad for k, v in w.items()}}
    assert sorted(got) == sorted(one[1]) and all(torch.equal(got[k], one[1][k]) for k in got)
    # only what requires grad gets one
    x2 = case["x"].cuda().requires_grad_(True)
    frozen = {k: v.cuda() for k, v in case["params"].items()}
    A.self_attention(x2, case["n"], frozen).sum().backward()
    assert x2.grad is not None and all(v.grad is None for v in frozen.values())


def test_forward_only_call_returns_only_y():
    case = SC.make_case(*SHAPES["rows_3x37"])
    y, _ = _device_run(case)
    fwd = ops.self_attn_backward(case["x"].cuda(), case["n"], {k: v.cuda() for k, v in case["params"].items()}, forward_only=True)
    assert sorted(fwd) == ["y"] and torch.equal(fwd["y"], y)


def test_an_image_does_not_see_its_neighbour():
    """y and d_x of image 0 in the 2 x 33 case equal, bit for bit, the run of image 0 alone: its last key tile holds one key and 31 padded
    ones, behind which the second image's rows lie"""
    seed, n, m, kind = SHAPES["tile_plus_1"]
    case = SC.make_case(seed, n, m, kind)
    y, grads = _device_run(case)
    alone = dict(case, x=case["x"][:m].contiguous(), n=1, d_y=case["d_y"][:m].contiguous())
    y0, grads0 = _device_run(alone)
    assert torch.equal(y[:m], y0) and torch.equal(grads["x"][:m], grads0["x"])
