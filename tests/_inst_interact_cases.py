"""What the tests of the instance interaction's gradient share: the fixture tests/golden/inst_interact/grads.npz (made by tests/golden/
make_golden_inst_interact_grads.py from the reference's own RCNNHead / RCNNHead_cond and torch's autograd), torch's autograd through
interact.inst_interact_host as the truth and the yardstick, the bound, and the seeded full-size cases of the GPU tests."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from _criterion_grad_cases import deviation  # noqa: F401  (the measure: max|got - truth| / max|truth|, an all-zero truth met exactly)
from _head_tail_cases import FLOOR, MARGIN, _settled_bias, bound  # noqa: F401  (the project's rule max(8 x yardstick, 16 x 2^-24))

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("cond", "plain", "plain_dead_unit")
DEAD = 3          # the dead unit of inst_interact.norm2 in "plain_dead_unit"


@functools.lru_cache(maxsize=None)
def fixture():
    """{case: {"in": {p, roi}, "cot": G_y, "sd": {...}, "out": {y}, "grad": {...}, "dev32": {...}}}"""
    z = np.load(os.path.join(HERE, "golden", "inst_interact", "grads.npz"))
    cases = {}
    for key in z.files:
        name, rest = key.split(".", 1)
        c = cases.setdefault(name, {"in": {}, "cot": None, "sd": {}, "out": {}, "grad": {}, "dev32": {}})
        if rest == "G_y":
            c["cot"] = z[key]
        elif rest.split(".")[0] in ("sd", "out", "grad", "dev32"):
            kind, k = rest.split(".", 1)
            c[kind][k] = z[key]
        else:
            c["in"][rest] = z[key]
    return cases


def host_run(I, p, roi, params, d_y, dtype):
    """torch's autograd through interact.inst_interact_host in `dtype` on the CPU -> (y, {p, roi, <parameter>: gradient}) of sum(d_y * y)"""
    leaf = lambda t: torch.as_tensor(t).detach().cpu().to(dtype).clone().requires_grad_(True)
    p, roi, w = leaf(p), leaf(roi), {k: leaf(v) for k, v in params.items()}
    y = I.inst_interact_host(p, roi, w)
    (torch.as_tensor(d_y).detach().cpu().to(dtype) * y).sum().backward()
    return y.detach(), {"p": p.grad, "roi": roi.grad, **{k: v.grad for k, v in w.items()}}


@functools.lru_cache(maxsize=None)
def link_params(seed):
    """the link's twelve parameters of one seeded full-size head (hidden 256, dim_dynamic 64, 7 x 7 bins), names without the prefix"""
    from diffusionvid_amd.modeling.roi_heads.box_head.interact import PARAM_NAMES
    from diffusionvid_amd.utils.synthetic import make_head_state_dict
    sd = make_head_state_dict(seed=seed, num_classes=30, num_heads=1, num_heads_cond=1)
    return {k: sd["head.head_series.0." + k].float().contiguous() for k in PARAM_NAMES}


def pre_activations(p, roi, params):
    """the float64 forward's three ReLU pre-activations, as rows: [R * 49, 64], [R * 49, 256], [R, 256]"""
    w = {k: v.detach().cpu().double() for k, v in params.items()}
    p, roi = p.detach().cpu().double(), roi.detach().cpu().double()
    d, dd = p.shape[1], w["inst_interact.norm1.weight"].shape[0]
    ln = lambda v, name: F.layer_norm(v, (v.shape[-1],), w[name + ".weight"], w[name + ".bias"], 1e-5)
    dyn = F.linear(p, w["inst_interact.dynamic_layer.weight"], w["inst_interact.dynamic_layer.bias"])
    a1 = ln(torch.bmm(roi, dyn[:, :d * dd].reshape(-1, d, dd)), "inst_interact.norm1")
    a2 = ln(torch.bmm(F.relu(a1), dyn[:, d * dd:].reshape(-1, dd, d)), "inst_interact.norm2")
    a3 = ln(F.linear(F.relu(a2).flatten(1), w["inst_interact.out_layer.weight"], w["inst_interact.out_layer.bias"]), "inst_interact.norm3")
    return a1.reshape(-1, dd), a2.reshape(-1, d), a3


# As _head_tail_cases says: a ReLU's gradient is discontinuous at a pre-activation of 0, and fp32 rounding decides the side of an entry the
# float64 truth puts within ~1e-6 of it.  The cases keep off the kinks by construction: the biases of inst_interact.norm1, norm2 and norm3 are
# moved, unit by unit and in this order (each after the previous is fixed), by the smallest multiple of MARGIN that leaves no row of the
# float64 forward within MARGIN of 0.  Only the float64 forward is consulted.  The exact zeros AT a kink are tested apart (dead units).
def settle_off_kinks(p, roi, params):
    w = {k: v.detach().cpu().float().clone() for k, v in params.items()}
    for i, name in enumerate(("inst_interact.norm1.bias", "inst_interact.norm2.bias", "inst_interact.norm3.bias")):
        w[name] = _settled_bias(pre_activations(p, roi, w)[i], w[name].double())
    return w


@functools.lru_cache(maxsize=None)
def make_case(seed, R):
    """a seeded case at the library's size: p (a LayerNorm output), roi, the cotangent d_y, the settled parameters"""
    g = torch.Generator().manual_seed(seed)
    p = F.layer_norm(torch.randn(R, 256, generator=g), (256,))
    roi = 0.5 * torch.randn(R, 49, 256, generator=g)
    d_y = torch.randn(R, 256, generator=g) / 16
    return {"p": p, "roi": roi, "d_y": d_y, "params": settle_off_kinks(p, roi, link_params(seed % 7))}


@functools.lru_cache(maxsize=None)
def truth(seed, R):
    """-> (y64, grads64, {name: yardstick}): the float64 host run of make_case(seed, R), and the fp32 host run's deviation from it"""
    from diffusionvid_amd.modeling.roi_heads.box_head import interact as I
    c = make_case(seed, R)
    y64, g64 = host_run(I, c["p"], c["roi"], c["params"], c["d_y"], torch.float64)
    y32, g32 = host_run(I, c["p"], c["roi"], c["params"], c["d_y"], torch.float32)
    yard = {"y": deviation(y32, y64), **{k: deviation(g32[k], g64[k]) for k in g64}}
    return y64, g64, yard
