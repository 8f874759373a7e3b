"""The tail of an RCNNHead / RCNNHead_cond pass (box_head.py:524-548 / :636-664) as a differentiable function: FFN (linear1, ReLU,
linear2) + residual + norm3, the time (and cond) modulation, the cls tower + class_logits, the reg tower + bboxes_delta, apply_deltas.

  head_tail_host   the plain torch restatement, in any float dtype, under torch's autograd on any device: the truth of the tests
  head_tail        differentiable: CPU tensors go through head_tail_host, CUDA tensors through dvid_head_tail_backward
                   (csrc/headtail_bwd.hip: the fp32 recompute and its backward, ops.head_tail_backward)

x [R, 256] is the tail's input, the norm2 output, R = n * M rows image-major; boxes_in [R, 4]; time_emb [n, 1024]; cond [R, 256] for the
cond head.  `params` maps the reference's parameter names WITHOUT the head's prefix ("linear1.weight", "cls_module.0.weight", ...) to
tensors in the reference's layout.  Dropout is the identity (MODEL.DiffusionDet.DROPOUT 0.0, the reference's default).  Returns
(class_logits [R, C], pred_boxes [R, 4], obj [R, 256]), obj being the norm3 output the next head takes.
"""
import math

import torch
import torch.nn.functional as F

from .... import ops

BBOX_WEIGHTS = (2.0, 2.0, 1.0, 1.0)                  # box_head.py:458
SCALE_CLAMP = math.log(100000.0 / 16)                # box_head.py:19

_FIXED = ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm3.weight", "norm3.bias", "block_time_mlp.1.weight",
          "block_time_mlp.1.bias", "c_mlp.1.weight", "c_mlp.1.bias", "class_logits.weight", "class_logits.bias", "bboxes_delta.weight",
          "bboxes_delta.bias")


def tower_depths(params):
    """(num_cls, num_reg): the tower layers `params` holds, cls_module.{3 i} / reg_module.{3 i}"""
    depth = lambda tower: sum(1 for k in params if k.startswith(tower + ".") and k.endswith(".weight") and int(k.split(".")[1]) % 3 == 0)
    return depth("cls_module"), depth("reg_module")


def param_names(num_cls, num_reg, cond):
    """The tail's parameter names in the order of dvid_head_tail_backward's pointer table (include/dvid_hip.h); the c_mlp.1 slots hold
    None for the plain head"""
    names = [k if cond or not k.startswith("c_mlp") else None for k in _FIXED]
    for tower, count in (("cls_module", num_cls), ("reg_module", num_reg)):
        for i in range(count):
            names += ["%s.%d.weight" % (tower, 3 * i), "%s.%d.weight" % (tower, 3 * i + 1), "%s.%d.bias" % (tower, 3 * i + 1)]
    return names


def check_dropout(cfg, what):
    """the tail's dropout is the identity: a config that asks for another is refused by key"""
    if float(cfg.MODEL.DiffusionDet.DROPOUT) != 0.0:
        raise NotImplementedError("%s: MODEL.DiffusionDet.DROPOUT is %r; the differentiable tail takes 0.0 (dropout is the identity)"
                                  % (what, cfg.MODEL.DiffusionDet.DROPOUT))


def apply_deltas_host(deltas, boxes, bbox_weights=BBOX_WEIGHTS, scale_clamp=SCALE_CLAMP):
    """box_head.py:550-590 for [R, 4] deltas; the boxes carry no gradient (the reference detaches them between heads)"""
    boxes = boxes.detach().to(deltas.dtype)
    widths, heights = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    ctr_x, ctr_y = boxes[:, 0] + 0.5 * widths, boxes[:, 1] + 0.5 * heights
    wx, wy, ww, wh = bbox_weights
    dx, dy = deltas[:, 0] / wx, deltas[:, 1] / wy
    dw, dh = torch.clamp(deltas[:, 2] / ww, max=scale_clamp), torch.clamp(deltas[:, 3] / wh, max=scale_clamp)
    pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
    pw, ph = torch.exp(dw) * widths, torch.exp(dh) * heights
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=1)


def head_tail_host(x, boxes_in, time_emb, params, cond=None, bbox_weights=BBOX_WEIGHTS, scale_clamp=SCALE_CLAMP):
    p = params
    d = x.shape[-1]
    ln = lambda v, name: F.layer_norm(v, (d,), p[name + ".weight"], p[name + ".bias"], 1e-5)
    n = time_emb.shape[0]
    assert x.dim() == 2 and x.shape[0] % n == 0, "x is [n * M, d], image-major"
    m = x.shape[0] // n
    obj = ln(x + F.linear(F.relu(F.linear(x, p["linear1.weight"], p["linear1.bias"])), p["linear2.weight"], p["linear2.bias"]), "norm3")
    ss = F.linear(F.silu(time_emb), p["block_time_mlp.1.weight"], p["block_time_mlp.1.bias"])
    ss = torch.repeat_interleave(ss, m, dim=0)
    if cond is None:
        scale, shift = ss.chunk(2, dim=1)
    else:
        scale, shift = ss, F.linear(F.silu(cond), p["c_mlp.1.weight"], p["c_mlp.1.bias"])
    fc = obj * (scale + 1) + shift
    num_cls, num_reg = tower_depths(p)
    cls, reg = fc, fc
    for i in range(num_cls):
        cls = F.relu(ln(F.linear(cls, p["cls_module.%d.weight" % (3 * i)]), "cls_module.%d" % (3 * i + 1)))
    for i in range(num_reg):
        reg = F.relu(ln(F.linear(reg, p["reg_module.%d.weight" % (3 * i)]), "reg_module.%d" % (3 * i + 1)))
    logits = F.linear(cls, p["class_logits.weight"], p["class_logits.bias"])
    deltas = F.linear(reg, p["bboxes_delta.weight"], p["bboxes_delta.bias"])
    return logits, apply_deltas_host(deltas, boxes_in, bbox_weights, scale_clamp), obj


class _HeadTail(torch.autograd.Function):
    """forward: the entry point's recompute; backward: the same entry point with the cotangents"""

    @staticmethod
    def forward(ctx, x, boxes_in, time_emb, cond, names, bbox_weights, scale_clamp, *plist):
        params = dict(zip(names, plist))
        out = ops.head_tail_backward(x, boxes_in, time_emb, params, cond=cond, bbox_weights=bbox_weights, scale_clamp=scale_clamp, forward_only=True)
        ctx.save_for_backward(x, boxes_in, time_emb, *plist) if cond is None else ctx.save_for_backward(x, boxes_in, time_emb, *plist, cond)
        ctx.names, ctx.has_cond, ctx.bbox_weights, ctx.scale_clamp = names, cond is not None, bbox_weights, scale_clamp
        return out["logits"], out["boxes"], out["obj"]

    @staticmethod
    def backward(ctx, d_logits, d_boxes, d_obj):
        saved = ctx.saved_tensors
        x, boxes_in, time_emb = saved[:3]
        cond = saved[-1] if ctx.has_cond else None
        plist = saved[3:3 + len(ctx.names)]
        out = ops.head_tail_backward(x, boxes_in, time_emb, dict(zip(ctx.names, plist)), cond=cond, d_logits=d_logits, d_boxes=d_boxes, d_obj=d_obj,
                                     bbox_weights=ctx.bbox_weights, scale_clamp=ctx.scale_clamp)
        need = ctx.needs_input_grad
        grads = [out["param_grads"][k] if need[7 + i] else None for i, k in enumerate(ctx.names)]
        return (out["d_x"] if need[0] else None, None, out["d_time_emb"] if need[2] else None, out["d_cond"] if cond is not None and need[3] else None,
                None, None, None, *grads)


def head_tail(x, boxes_in, time_emb, params, cond=None, bbox_weights=BBOX_WEIGHTS, scale_clamp=SCALE_CLAMP):
    """Differentiable with respect to x, time_emb, cond and the parameter tensors that require grad"""
    if x.device.type != "cuda":
        return head_tail_host(x, boxes_in, time_emb, params, cond, bbox_weights, scale_clamp)
    names = tuple(k for k in param_names(*tower_depths(params), cond is not None) if k is not None)
    return _HeadTail.apply(x, boxes_in, time_emb, cond, names, tuple(bbox_weights), float(scale_clamp), *(params[k] for k in names))
