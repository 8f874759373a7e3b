"""The instance interaction of an RCNNHead pass (DynamicConv, box_head.py:666-711) with its residual and norm2 (box_head.py:521-524) as a
differentiable function: the link in front of box_head.tail.

  inst_interact_host   the plain torch restatement, in any float dtype and any sizes, under torch's autograd on any device: the truth of the tests
  inst_interact        differentiable: CPU tensors go through inst_interact_host, CUDA tensors through dvid_inst_interact_backward
                       (csrc/interact_bwd.hip: the fp32 recompute and its backward, ops.inst_interact_backward)

p [R, d] is the norm1 output, R = n * M rows image-major; roi [R, P * P, d] the RoI tiles, bin-major.  `params` maps the reference's
parameter names WITHOUT the head's prefix ("inst_interact.dynamic_layer.weight", ..., "norm2.bias") to tensors in the reference's layout.
Dropout is the identity (tail.check_dropout refuses a config that asks for another).  Returns y [R, d], the norm2 output, the tail's x.
"""
import torch
import torch.nn.functional as F

from .... import ops

# the order of dvid_inst_interact_backward's pointer table (include/dvid_hip.h)
PARAM_NAMES = ("inst_interact.dynamic_layer.weight", "inst_interact.dynamic_layer.bias", "inst_interact.out_layer.weight", "inst_interact.out_layer.bias",
               "inst_interact.norm1.weight", "inst_interact.norm1.bias", "inst_interact.norm2.weight", "inst_interact.norm2.bias",
               "inst_interact.norm3.weight", "inst_interact.norm3.bias", "norm2.weight", "norm2.bias")
PREFIXES = ("inst_interact.", "norm2.")


def inst_interact_host(p, roi, params):
    w = params
    d = p.shape[-1]
    dd = w["inst_interact.norm1.weight"].shape[0]
    ln = lambda v, name: F.layer_norm(v, (v.shape[-1],), w[name + ".weight"], w[name + ".bias"], 1e-5)
    assert p.dim() == 2 and roi.dim() == 3 and roi.shape[0] == p.shape[0] and roi.shape[2] == d, "p is [R, d], roi [R, bins, d]"
    dyn = F.linear(p, w["inst_interact.dynamic_layer.weight"], w["inst_interact.dynamic_layer.bias"])
    param1, param2 = dyn[:, :d * dd].reshape(-1, d, dd), dyn[:, d * dd:].reshape(-1, dd, d)
    f1 = F.relu(ln(torch.bmm(roi, param1), "inst_interact.norm1"))
    f2 = F.relu(ln(torch.bmm(f1, param2), "inst_interact.norm2"))
    o = F.relu(ln(F.linear(f2.flatten(1), w["inst_interact.out_layer.weight"], w["inst_interact.out_layer.bias"]), "inst_interact.norm3"))
    return ln(p + o, "norm2")


class _InstInteract(torch.autograd.Function):
    """forward: the entry point's recompute; backward: the same entry point with the cotangent"""

    @staticmethod
    def forward(ctx, p, roi, *plist):
        out = ops.inst_interact_backward(p, roi, dict(zip(PARAM_NAMES, plist)), forward_only=True)
        ctx.save_for_backward(p, roi, *plist)
        return out["y"]

    @staticmethod
    def backward(ctx, d_y):
        p, roi, *plist = ctx.saved_tensors
        need = ctx.needs_input_grad
        out = ops.inst_interact_backward(p, roi, dict(zip(PARAM_NAMES, plist)), d_y=d_y, want_d_roi=need[1])
        grads = [out["param_grads"][k] if need[2 + i] else None for i, k in enumerate(PARAM_NAMES)]
        return (out["d_p"] if need[0] else None, out["d_roi"] if need[1] else None, *grads)


def inst_interact(p, roi, params):
    """Differentiable with respect to p, roi and the parameter tensors that require grad"""
    if p.device.type != "cuda":
        return inst_interact_host(p, roi, params)
    return _InstInteract.apply(p, roi, *(params[k] for k in PARAM_NAMES))
