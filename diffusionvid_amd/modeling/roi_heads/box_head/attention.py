"""The self-attention of an RCNNHead pass with its residual and norm1 (box_head.py:514-518) as a differentiable function: the link in front
of box_head.interact, and the one that lets the links compose over the heads -- a head's x is the previous head's obj_features.

  self_attention_host   the plain torch restatement, in any float dtype and any sizes, under torch's autograd on any device: the truth of the tests
  self_attention        differentiable: CPU tensors go through self_attention_host, CUDA tensors through dvid_self_attn_backward
                        (csrc/selfattn_bwd.hip: the fp32 recompute and its backward, ops.self_attn_backward)

x [n * m, d] are the proposal features, rows image-major: the m rows of each of the n images attend to each other (the reference's
nn.MultiheadAttention over [m, n, d]).  `params` maps the reference's parameter names WITHOUT the head's prefix ("self_attn.in_proj_weight",
..., "norm1.bias") to tensors in the reference's layout.  Dropout is the identity (tail.check_dropout refuses a config that asks for
another).  Returns y [n * m, d], the norm1 output, the interaction's p.
"""
import torch
import torch.nn.functional as F

from .... import ops

# the order of dvid_self_attn_backward's pointer table (include/dvid_hip.h)
PARAM_NAMES = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "norm1.weight", "norm1.bias")
PREFIXES = ("self_attn.", "norm1.")
NHEADS = 8


def self_attention_host(x, n, params, nheads=NHEADS):
    w = params
    assert x.dim() == 2 and x.shape[0] % n == 0 and x.shape[1] % nheads == 0, "x is [n * m, d], d whole heads"
    R, d = x.shape
    seq = x.reshape(n, R // n, d).permute(1, 0, 2)          # [m, n, d], as the reference hands it to nn.MultiheadAttention
    # the function nn.MultiheadAttention.forward calls, with its default need_weights=True: the explicit q k^T / softmax / . v, q scaled first
    o = F.multi_head_attention_forward(seq, seq, seq, d, nheads, w["self_attn.in_proj_weight"], w["self_attn.in_proj_bias"], None, None, False, 0.0,
                                       w["self_attn.out_proj.weight"], w["self_attn.out_proj.bias"], training=False, need_weights=True)[0]
    return F.layer_norm(seq + o, (d,), w["norm1.weight"], w["norm1.bias"], 1e-5).permute(1, 0, 2).reshape(R, d)


class _SelfAttention(torch.autograd.Function):
    """forward: the entry point's recompute; backward: the same entry point with the cotangent"""

    @staticmethod
    def forward(ctx, x, n, *plist):
        out = ops.self_attn_backward(x, n, dict(zip(PARAM_NAMES, plist)), forward_only=True)
        ctx.save_for_backward(x, *plist)
        ctx.n = n
        return out["y"]

    @staticmethod
    def backward(ctx, d_y):
        x, *plist = ctx.saved_tensors
        need = ctx.needs_input_grad
        out = ops.self_attn_backward(x, ctx.n, dict(zip(PARAM_NAMES, plist)), d_y=d_y)
        grads = [out["param_grads"][k] if need[2 + i] else None for i, k in enumerate(PARAM_NAMES)]
        return (out["d_x"] if need[0] else None, None, *grads)


def self_attention(x, n, params):
    """Differentiable with respect to x and the parameter tensors that require grad"""
    if x.device.type != "cuda":
        return self_attention_host(x, n, params)
    return _SelfAttention.apply(x, n, *(params[k] for k in PARAM_NAMES))
