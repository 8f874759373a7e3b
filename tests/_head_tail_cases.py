"""What the tests of the head tail's gradient share: the fixture tests/golden/head_tail/grads.npz (made by tests/golden/
make_golden_head_tail_grads.py from the reference's own RCNNHead / RCNNHead_cond and torch's autograd), torch's autograd through
tail.head_tail_host as the truth and the yardstick, the bound, and the seeded full-size cases of the GPU tests."""
import functools
import os

import numpy as np
import torch

from _criterion_grad_cases import deviation  # noqa: F401  (the measure: max|got - truth| / max|truth|, an all-zero truth met exactly)

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("cond", "cond_obj", "plain", "plain_clamped", "plain_obj", "plain_zero_width")
FLOOR = 16 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def fixture():
    """{case: {"in": {x, boxes_in, time_emb[, cond]}, "cot": {logits, boxes[, obj]}, "sd": {...}, "out": {...}, "grad": {...}, "dev32": {...}}}"""
    z = np.load(os.path.join(HERE, "golden", "head_tail", "grads.npz"))
    cases = {}
    for key in z.files:
        name, rest = key.split(".", 1)
        c = cases.setdefault(name, {"in": {}, "cot": {}, "sd": {}, "out": {}, "grad": {}, "dev32": {}})
        if rest.startswith("G_"):
            c["cot"][{"l": "logits", "b": "boxes", "o": "obj"}[rest[2]]] = z[key]
        elif rest.split(".")[0] in ("sd", "out", "grad", "dev32"):
            kind, k = rest.split(".", 1)
            c[kind][k] = z[key]
        else:
            c["in"][rest] = z[key]
    return cases


def bound(yard):
    """the project's rule, per tensor: 8 x the fp32 host run's own deviation from the float64 truth, with a floor of 16 x 2^-24"""
    return max(8 * yard, FLOOR)


def host_run(T, x, boxes_in, time_emb, params, cond, cots, dtype, **kw):
    """torch's autograd through tail.head_tail_host in `dtype` on the CPU -> ({logits, boxes, obj}, {x, time_emb[, cond], <parameter>:
    gradient}) of sum_k sum(cots[k] * out[k]); a tensor the loss does not reach gets zeros"""
    leaf = lambda t: torch.as_tensor(t).detach().cpu().to(dtype).clone().requires_grad_(True)
    x, te, p = leaf(x), leaf(time_emb), {k: leaf(v) for k, v in params.items()}
    cd = None if cond is None else leaf(cond)
    outs = dict(zip(("logits", "boxes", "obj"), T.head_tail_host(x, torch.as_tensor(boxes_in).detach().cpu().to(dtype), te, p, cd, **kw)))
    sum((torch.as_tensor(c).detach().cpu().to(dtype) * outs[k]).sum() for k, c in cots.items() if c is not None).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    grads = {"x": zero(x), "time_emb": zero(te), **{k: zero(v) for k, v in p.items()}}
    if cd is not None:
        grads["cond"] = zero(cd)
    return {k: v.detach() for k, v in outs.items()}, grads


TAIL = ("linear1.", "linear2.", "norm3.", "block_time_mlp.", "c_mlp.", "cls_module.", "reg_module.", "class_logits.", "bboxes_delta.")


@functools.lru_cache(maxsize=None)
def tail_params(seed, num_classes, cond):
    """the tail's parameters of one seeded full-size head (hidden 256, dff 2048: what the library takes), names without the prefix"""
    from diffusionvid_amd.utils.synthetic import make_head_state_dict
    sd = make_head_state_dict(seed=seed, num_classes=num_classes, num_heads=1, num_heads_cond=1)
    pfx = "head.head_series_cond.0." if cond else "head.head_series.0."
    return {k[len(pfx):]: v.float().contiguous() for k, v in sd.items() if k.startswith(pfx) and k[len(pfx):].startswith(TAIL)}


# A ReLU's gradient is discontinuous at a pre-activation of 0, and fp32 rounding (the device's, or the fp32 host run's) decides the side of an
# entry that the float64 truth puts within ~1e-6 of it: one such entry among the R x 2048 hidden units and R x 256 tower units of a case moves
# whole gradient tensors by 1e-3 of their largest entry (seen on the first device run: one tower unit at 1.2e-07 of the kink).  The
# cases therefore keep off the kinks by construction, as the criterion's fixtures do: linear1's bias and the tower LayerNorms' biases are
# moved, unit by unit, by the smallest multiple of MARGIN that leaves no row of the float64 forward within MARGIN of 0.  Only the float64
# host forward is consulted.  The exact zeros AT a kink are tested apart (dead units, the clamp, zero-width boxes).
MARGIN = 1e-4


def _settled_bias(pre, bias):
    """pre [R, U] float64 pre-activations including `bias` [U] -> the fp32 bias that keeps every |pre| >= MARGIN (checked at 0.9 MARGIN after
    the rounding to fp32)"""
    shift = torch.zeros_like(bias)
    done = torch.zeros(bias.shape, dtype=torch.bool)
    for k in range(400):
        for sgn in ((1,) if k == 0 else (1, -1)):
            s = sgn * k * MARGIN
            ok = ((pre + s).abs().min(dim=0).values >= MARGIN) & ~done
            shift[ok], done = s, done | ok
        if bool(done.all()):
            break
    assert bool(done.all()), "no shift below 400 x MARGIN settles a unit"
    new = (bias + shift).float()
    assert float((pre - bias + new.double()).abs().min()) >= 0.9 * MARGIN
    return new


def settle_off_kinks(x, time_emb, params, cond=None):
    """-> a copy of `params` (fp32) whose ReLU pre-activations on (x, time_emb, cond) all lie at least MARGIN from 0 in the float64 forward"""
    import torch.nn.functional as F
    p = {k: v.detach().cpu().float().clone() for k, v in params.items()}
    d64 = lambda k: p[k].double()
    x, te = x.detach().cpu().double(), time_emb.detach().cpu().double()
    ln = lambda v, name: F.layer_norm(v, (v.shape[-1],), d64(name + ".weight"), d64(name + ".bias"), 1e-5)
    p["linear1.bias"] = _settled_bias(F.linear(x, d64("linear1.weight"), d64("linear1.bias")), d64("linear1.bias"))
    obj = ln(x + F.linear(F.relu(F.linear(x, d64("linear1.weight"), d64("linear1.bias"))), d64("linear2.weight"), d64("linear2.bias")), "norm3")
    ss = torch.repeat_interleave(F.linear(F.silu(te), d64("block_time_mlp.1.weight"), d64("block_time_mlp.1.bias")), x.shape[0] // te.shape[0], dim=0)
    if cond is None:
        scale, shift = ss.chunk(2, dim=1)
    else:
        scale, shift = ss, F.linear(F.silu(cond.detach().cpu().double()), d64("c_mlp.1.weight"), d64("c_mlp.1.bias"))
    fc = obj * (scale + 1) + shift
    for tower in ("cls_module", "reg_module"):
        cur, i = fc, 0
        while "%s.%d.weight" % (tower, 3 * i) in p:
            name = "%s.%d" % (tower, 3 * i + 1)
            p[name + ".bias"] = _settled_bias(ln(F.linear(cur, d64("%s.%d.weight" % (tower, 3 * i))), name), d64(name + ".bias"))
            cur, i = F.relu(ln(F.linear(cur, d64("%s.%d.weight" % (tower, 3 * i))), name)), i + 1
    return p


def make_case(seed, n, m, num_classes, cond=False, with_obj=False):
    """a seeded case at the library's size: inputs, cotangents, parameters; three different t are three different time_emb rows"""
    g = torch.Generator().manual_seed(seed)
    R = n * m
    x = torch.nn.functional.layer_norm(torch.randn(R, 256, generator=g), (256,))          # the tail's input is a LayerNorm output
    xy = torch.rand(R, 2, generator=g) * 300
    wh = torch.exp(torch.rand(R, 2, generator=g) * 4.0 + 1.0)
    case = {"x": x, "boxes_in": torch.cat([xy, xy + wh], dim=1), "time_emb": torch.randn(n, 1024, generator=g) * 0.5,
            "cond": torch.randn(R, 256, generator=g) if cond else None, "params": dict(tail_params(seed % 7, num_classes, cond)),
            "cots": {"logits": torch.randn(R, num_classes, generator=g) / 16, "boxes": torch.randn(R, 4, generator=g) * 0.01,
                     "obj": torch.randn(R, 256, generator=g) / 16 if with_obj else None}}
    case["params"] = settle_off_kinks(case["x"], case["time_emb"], case["params"], case["cond"])
    return case
