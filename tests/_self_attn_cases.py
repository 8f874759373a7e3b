"""What the tests of the self-attention link's gradient and of the chain over the heads share: the fixtures under tests/golden/self_attn/
(made by tests/golden/make_golden_self_attn_grads.py from the reference's own RCNNHead / DynamicHead and torch's autograd), torch's autograd
through attention.self_attention_host as the truth and the yardstick, the bound, the host composition of a chain of heads, and the seeded
full-size cases of the GPU tests."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from _criterion_grad_cases import deviation  # noqa: F401  (the measure: max|got - truth| / max|truth|, an all-zero truth met exactly)
from _head_tail_cases import bound  # noqa: F401  (the project's rule max(8 x yardstick, 16 x 2^-24))

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "self_attn")


def _split(z):
    """{first key part: {rest: array}} of an npz"""
    out = {}
    for key in z.files:
        kind, rest = key.split(".", 1)
        out.setdefault(kind, {})[rest] = z[key]
    return out


@functools.lru_cache(maxsize=None)
def link_fixture():
    """{"in": {x, G_y, n}, "sd": {...}, "out": {y}, "grad": {x, <parameter>}, "dev32": {...}}"""
    return _split(np.load(os.path.join(GOLDEN, "link.npz")))


@functools.lru_cache(maxsize=None)
def chain_fixture():
    """{"in": {tiles [H, R, 49, d], boxes [n, M, 4], steps [n], time_in [n, d], G_logits, G_boxes [H, n, M, .]}, "sd": {head_series.*, time_mlp.*},
    "grad": {<parameter>, tiles}, "dev32": {...}}"""
    return _split(np.load(os.path.join(GOLDEN, "chain.npz")))


def host_run(A, x, n, params, d_y, dtype):
    """torch's autograd through attention.self_attention_host in `dtype` on the CPU -> (y, {x, <parameter>: gradient}) of sum(d_y * y)"""
    leaf = lambda t: torch.as_tensor(t).detach().cpu().to(dtype).clone().requires_grad_(True)
    x, w = leaf(x), {k: leaf(v) for k, v in params.items()}
    y = A.self_attention_host(x, n, w)
    (torch.as_tensor(d_y).detach().cpu().to(dtype) * y).sum().backward()
    return y.detach(), {"x": x.grad, **{k: v.grad for k, v in w.items()}}


def chain_host(tiles, boxes0, time_emb, sd, num_heads, nheads=8, boxes_in=None):
    """The host composition of the heads of a DynamicHead pass without the pooler: per head the mean of the tiles (head 0) or the previous
    head's obj_features, self_attention_host, inst_interact_host, head_tail_host, the boxes detached between heads (box_head.py:299).
    tiles [H][n * M, 49, d] (any sequence), boxes0 [n, M, 4], time_emb [n, 4 d]; sd {name under head_series.<h>.: tensor} per head, a
    sequence.  boxes_in [H][n * M, 4]: the boxes every head starts from, given (they carry no gradient either way) instead of the previous
    head's own output.  -> (logits [H][R, C], boxes [H][R, 4])"""
    from diffusionvid_amd.modeling.roi_heads.box_head import attention as A
    from diffusionvid_amd.modeling.roi_heads.box_head import interact as I
    from diffusionvid_amd.modeling.roi_heads.box_head import tail as T
    n, M = boxes0.shape[:2]
    boxes, feats, logits_all, boxes_all = boxes0.reshape(n * M, 4), None, [], []
    for h in range(num_heads):
        x = tiles[h].mean(1) if feats is None else feats
        p = A.self_attention_host(x, n, sd[h], nheads)
        y = I.inst_interact_host(p, tiles[h], sd[h])
        logits, new_boxes, feats = T.head_tail_host(y, boxes if boxes_in is None else boxes_in[h], time_emb, sd[h])
        logits_all.append(logits), boxes_all.append(new_boxes)
        boxes = new_boxes.detach()
    return logits_all, boxes_all


@functools.lru_cache(maxsize=None)
def link_params(seed):
    """the link's six parameters of one seeded full-size head (hidden 256, 8 heads), names without the prefix"""
    from diffusionvid_amd.modeling.roi_heads.box_head.attention import PARAM_NAMES
    from diffusionvid_amd.utils.synthetic import make_head_state_dict
    sd = make_head_state_dict(seed=seed, num_classes=30, num_heads=1, num_heads_cond=1)
    return {k: sd["head.head_series.0." + k].float().contiguous() for k in PARAM_NAMES}


def scores(x, n, params):
    """the float64 forward's scaled scores [n, 8, m, m]"""
    x = x.detach().cpu().double()
    m = x.shape[0] // n
    qkv = F.linear(x, params["self_attn.in_proj_weight"].double(), params["self_attn.in_proj_bias"].double()).reshape(n, m, 3, 8, 32).permute(2, 0, 3, 1, 4)
    return torch.matmul(qkv[0], qkv[1].transpose(-1, -2)) / 32 ** 0.5


@functools.lru_cache(maxsize=None)
def make_case(seed, n, m, kind="norm"):
    """a seeded case at the library's size: x (kind "norm": a LayerNorm output, what heads 1.. see; "mean": the mean over 49 bins of
    non-negative tiles, what head 0 sees; "peaked": a LayerNorm output scaled until the scores span more than 100 units, so that an exp
    without the subtraction of the row's log-sum-exp overflows fp32's 88.7), the cotangent d_y ~ N(0, 1) / 16, the parameters"""
    g = torch.Generator().manual_seed(seed)
    R = n * m
    params = link_params(seed % 7)
    if kind == "mean":
        x = F.relu(0.5 * torch.randn(R, 49, 256, generator=g)).mean(1)
    else:
        x = F.layer_norm(torch.randn(R, 256, generator=g), (256,))
    if kind == "peaked":
        for _ in range(8):
            s = scores(x, n, params)
            span = float(s.max() - s.min())
            if span > 100 and float(s.max()) > 89:
                break
            x = x * (130.0 / min(span, float(s.max()))) ** 0.5
    d_y = torch.randn(R, 256, generator=g) / 16
    return {"x": x.contiguous(), "n": n, "d_y": d_y, "params": params}


@functools.lru_cache(maxsize=None)
def truth(seed, n, m, kind="norm"):
    """-> (y64, grads64, {name: yardstick}): the float64 host run of make_case, and the fp32 host run's deviation from it"""
    from diffusionvid_amd.modeling.roi_heads.box_head import attention as A
    c = make_case(seed, n, m, kind)
    y64, g64 = host_run(A, c["x"], n, c["params"], c["d_y"], torch.float64)
    y32, g32 = host_run(A, c["x"], n, c["params"], c["d_y"], torch.float32)
    yard = {"y": deviation(y32, y64), **{k: deviation(g32[k], g64[k]) for k in g64}}
    return y64, g64, yard
