"""Generate the golden gradients of the head's tail by running the REFERENCE's own RCNNHead / RCNNHead_cond and backpropagating through
them on the CPU (build container only).

    python tests/golden/make_golden_head_tail_grads.py            # writes tests/golden/head_tail/grads.npz
    python tests/golden/make_golden_head_tail_grads.py --check    # regenerates in memory and compares with the committed file

The reference is imported by make_golden.py (same shims), at make_golden.make_head()'s reduced size (hidden 16, dff 32, 30 classes).  The
tail -- everything behind the module's norm2 -- is isolated without restating it: a forward hook on `norm2` returns a LEAF tensor x (the
norm2 output of an fp32 run, recorded first), so the gradient reaches x, time_emb, cond and the tail's parameters and stops there.  Only
data is stored.

Per case: loss = sum(G_l * logits) + sum(G_b * boxes) [+ sum(G_o * obj)] with seeded cotangents, backward() once with the module and the
inputs in float64 and once in fp32.  n = 3 images with three different t, M = 37 boxes each.

grads.npz   `<case>.x` [R, 16], `.boxes_in` [R, 4], `.time_emb` [3, 64], `.cond` [R, 16] (cond head), `.G_l`, `.G_b`, `.G_o` (where given),
            `<case>.sd.<name>`: the tail's parameters, the reference's names without the head's prefix;
            `<case>.out.{logits,boxes,obj}` and `<case>.grad.{x,time_emb,cond,<parameter name>}`: the float64 run, stored as float32;
            `<case>.dev32.<the same names>`: the deviation of the fp32 run from the float64 run, max|got - truth| / max|truth|.
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the shims, imports the reference)

import torch  # noqa: E402

OUT = os.path.join(G.OUT, "head_tail")
M = 37
STEPS = (999, 499, 249)
TAIL = ("linear1.", "linear2.", "norm3.", "block_time_mlp.", "c_mlp.", "cls_module.", "reg_module.", "class_logits.", "bboxes_delta.")
# name: (cond head, G_o given, bboxes_delta.bias[2:] raised, a zero-width box)
CASES = {"plain": (False, False, False, False), "plain_obj": (False, True, False, False), "cond": (True, False, False, False),
         "cond_obj": (True, True, False, False), "plain_clamped": (False, True, True, False), "plain_zero_width": (False, False, False, True)}


def deviation(got, truth):
    scale = float(truth.abs().max())
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0, "the truth is all zero, the fp32 run is not"
        return 0.0
    return float((got.double() - truth).abs().max()) / scale


def run_reference(module, pooler, feats, boxes, time_emb, cond, x, cots, dtype):
    """-> ({logits, boxes, obj}, {x, time_emb, cond, <parameter>: gradient}) of the seeded loss, the module and every input in `dtype`"""
    mod = copy.deepcopy(module).to(dtype)
    leaf = x.detach().to(dtype).reshape(1, -1, x.shape[-1]).clone().requires_grad_(True)
    te = time_emb.detach().to(dtype).clone().requires_grad_(True)
    cd = None if cond is None else cond.detach().to(dtype).clone().requires_grad_(True)
    hook = mod.norm2.register_forward_hook(lambda m, i, o: leaf)
    args = ([f.to(dtype) for f in feats], boxes.to(dtype), None, pooler, te) + (() if cond is None else (cd,))
    logits, pred, obj = mod(*args)
    hook.remove()
    outs = {"logits": logits.reshape(-1, logits.shape[-1]), "boxes": pred.reshape(-1, 4), "obj": obj.reshape(-1, obj.shape[-1])}
    loss = sum((cots[k].to(dtype) * outs[k]).sum() for k in outs if k in cots)
    loss.backward()
    grads = {"x": leaf.grad[0], "time_emb": te.grad}
    if cd is not None:
        grads["cond"] = cd.grad
    for k, p in mod.named_parameters():
        if k.startswith(TAIL):
            grads[k] = p.grad
        else:
            assert p.grad is None, "%s lies in front of the tail and got a gradient" % k
    return {k: v.detach() for k, v in outs.items()}, grads


def make_grads():
    h, _ = G.make_head()
    feats, boxes, g = G.make_inputs(410, n_frames=len(STEPS))
    boxes = boxes[:, :M].contiguous()
    with torch.no_grad():
        time_emb = h.time_mlp(torch.tensor(STEPS, dtype=torch.long))
    R, d = boxes.shape[0] * M, G.RED["hidden"]
    cond = torch.randn(R, d, generator=g)
    out, report = {}, []
    for name, (is_cond, with_obj, clamped, zero_width) in CASES.items():
        module = copy.deepcopy(h.head_series_cond[0] if is_cond else h.head_series[0])
        bx = boxes.clone()
        if zero_width:
            bx[1, 5] = torch.tensor([40.0, 20.0, 40.0, 90.0])          # zero width, a height of 70
        if clamped:
            module.bboxes_delta.bias.data[2:] += 8.0                     # scale_clamp is log(100000 / 16) = 8.74
        caught = []
        hook = module.norm2.register_forward_hook(lambda m, i, o: caught.append(o.detach()))
        with torch.no_grad():
            module(feats, bx, None, h.box_pooler, time_emb, *((cond,) if is_cond else ()))
        hook.remove()
        x = caught[0].reshape(R, d)
        gc = torch.Generator().manual_seed(4100 + len(out))
        cots = {"logits": torch.randn(R, G.RED["num_classes"], generator=gc), "boxes": torch.randn(R, 4, generator=gc) * 0.1}
        if with_obj:
            cots["obj"] = torch.randn(R, d, generator=gc)
        o64, g64 = run_reference(module, h.box_pooler, feats, bx, time_emb, cond if is_cond else None, x, cots, torch.float64)
        o32, g32 = run_reference(module, h.box_pooler, feats, bx, time_emb, cond if is_cond else None, x, cots, torch.float32)
        assert g32["x"].dtype == torch.float32 and g64["x"].dtype == torch.float64
        if clamped:          # rows on both sides of the clamp, none so close to it that the two runs could disagree about the side
            with torch.no_grad():
                mod64 = copy.deepcopy(module).double()
                hk = mod64.norm2.register_forward_hook(lambda m, i, o: x.double().reshape(1, R, d))
                seen = []
                hd = mod64.bboxes_delta.register_forward_hook(lambda m, i, o: seen.append(o))
                mod64([f.double() for f in feats], bx.double(), None, h.box_pooler, time_emb.double())
                hk.remove(), hd.remove()
            dwh = seen[0][:, 2:]
            clamp = module.scale_clamp
            assert bool((dwh > clamp).any()) and bool((dwh < clamp).any()) and float((dwh - clamp).abs().min()) > 1e-3
            report.append("%-18s %d of %d dw / dh above the clamp" % (name, int((dwh > clamp).sum()), dwh.numel()))
        pre = name + "."
        out[pre + "x"], out[pre + "boxes_in"], out[pre + "time_emb"] = x.detach().numpy(), bx.detach().reshape(R, 4).numpy(), time_emb.detach().numpy()
        if is_cond:
            out[pre + "cond"] = cond.detach().numpy()
        for k, v in cots.items():
            out[pre + "G_" + k[0]] = v.detach().numpy()
        for k, v in module.state_dict().items():
            if k.startswith(TAIL):
                out[pre + "sd." + k] = v.detach().numpy()
        for kind, t64, t32 in (("out", o64, o32), ("grad", g64, g32)):
            for k in t64:
                out["%s%s.%s" % (pre, kind, k)] = t64[k].numpy().astype(np.float32)
                dev = deviation(t32[k], t64[k])
                out["%sdev32.%s" % (pre, k)] = np.array(dev, dtype=np.float64)
                report.append("%-18s %-5s %-28s max|.| %.6e  fp32 run %.3e" % (name, kind, k, float(t64[k].abs().max()), dev))
    return out, report


def main():
    torch.set_num_threads(1)
    torch.backends.mha.set_fastpath_enabled(False)
    arrays, report = make_grads()
    path = os.path.join(OUT, "grads.npz")
    if "--check" in sys.argv:
        have = np.load(path)
        assert sorted(have.files) == sorted(arrays), "grads.npz: the keys differ"
        for k, v in arrays.items():
            assert have[k].dtype == v.dtype and np.array_equal(have[k], v), "grads.npz: %s differs from the committed fixture" % k
        print("head tail gradient fixtures reproduced")
        return
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(path, **arrays)
    print("grads.npz", os.path.getsize(path), "bytes")
    print("\n".join(report))


if __name__ == "__main__":
    main()
