"""Generate the golden gradients of the head's instance interaction (DynamicConv, its residual and norm2) by running the REFERENCE's own
RCNNHead / RCNNHead_cond and backpropagating through them on the CPU (build container only).

    python tests/golden/make_golden_inst_interact_grads.py            # writes tests/golden/inst_interact/grads.npz
    python tests/golden/make_golden_inst_interact_grads.py --check    # regenerates in memory and compares with the committed file

The reference is imported by make_golden.py (same shims), at make_golden.make_head()'s reduced size (hidden 16, dim_dynamic 4, 7 x 7 bins).
The link is isolated with hooks, without restating it: a forward hook on the head's `norm1` returns a LEAF p (the norm1 output of an fp32
run, recorded first), a forward hook on the pooler returns a LEAF roi (its recorded output), and a hook on `norm2` captures y.  The loss is
sum(G_y * y) with a seeded cotangent, so the gradient reaches p, roi and the link's twelve parameters and nothing else (asserted).  Only
data is stored.  backward() runs once with the module and the inputs in float64 and once in fp32.  n = 2 images, M = 7 boxes each.

grads.npz   `<case>.p` [R, 16] (rows image-major), `.roi` [R, 49, 16] (bin-major), `.G_y` [R, 16];
            `<case>.sd.<name>`: the link's parameters, the reference's names without the head's prefix;
            `<case>.out.y` and `<case>.grad.{p,roi,<parameter name>}`: the float64 run, stored as float32;
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

from make_golden_head_tail_grads import deviation  # noqa: E402

OUT = os.path.join(G.OUT, "inst_interact")
M = 7
STEPS = (999, 249)
LINK = ("inst_interact.", "norm2.")
DEAD = 3          # the unit of inst_interact.norm2 whose weight and bias are 0 in the dead-unit case
# name: (cond head, a dead unit)
CASES = {"plain": (False, False), "cond": (True, False), "plain_dead_unit": (False, True)}


def run_reference(module, pooler, feats, boxes, time_emb, cond, p, roi, g_y, dtype):
    """-> (y, {p, roi, <parameter>: gradient}) of sum(g_y * y), the module and every input in `dtype`.  p [R, d] rows image-major, roi
    [R, 49, d] bin-major: the hooks hand them to the module in its own layouts ([M, n, d] behind norm1, [R, d, 7, 7] behind the pooler)"""
    mod = copy.deepcopy(module).to(dtype)
    n, m = boxes.shape[:2]
    d = p.shape[-1]
    pl = p.detach().to(dtype).clone().requires_grad_(True)
    rl = roi.detach().to(dtype).clone().requires_grad_(True)
    caught = []
    hooks = [mod.norm1.register_forward_hook(lambda mo, i, o: pl.reshape(n, m, d).permute(1, 0, 2)),
             pooler.register_forward_hook(lambda mo, i, o: rl.permute(0, 2, 1).reshape(n * m, d, 7, 7)),
             mod.norm2.register_forward_hook(lambda mo, i, o: caught.append(o))]
    try:
        mod(*(([f.to(dtype) for f in feats], boxes.to(dtype), None, pooler, time_emb.to(dtype)) + (() if cond is None else (cond.to(dtype),))))
    finally:
        for h in hooks:
            h.remove()
    y = caught[0].reshape(n * m, d)
    (g_y.to(dtype) * y).sum().backward()
    grads = {"p": pl.grad, "roi": rl.grad}
    for k, w in mod.named_parameters():
        if k.startswith(LINK):
            grads[k] = w.grad
        else:
            assert w.grad is None, "%s lies outside the link and got a gradient" % k
    return y.detach(), grads


def make_grads():
    h, _ = G.make_head()
    feats, boxes, g = G.make_inputs(510, n_frames=len(STEPS))
    boxes = boxes[:, :M].contiguous()
    with torch.no_grad():
        time_emb = h.time_mlp(torch.tensor(STEPS, dtype=torch.long))
    n, d = boxes.shape[0], G.RED["hidden"]
    R = n * M
    cond = torch.randn(R, d, generator=g)
    out, report = {}, []
    for name, (is_cond, dead) in CASES.items():
        module = copy.deepcopy(h.head_series_cond[0] if is_cond else h.head_series[0])
        if dead:
            module.inst_interact.norm2.weight.data[DEAD] = 0.0
            module.inst_interact.norm2.bias.data[DEAD] = 0.0
        caught = {}
        hooks = [module.norm1.register_forward_hook(lambda mo, i, o: caught.__setitem__("p", o.detach())),
                 h.box_pooler.register_forward_hook(lambda mo, i, o: caught.__setitem__("roi", o.detach()))]
        with torch.no_grad():
            module(feats, boxes, None, h.box_pooler, time_emb, *((cond,) if is_cond else ()))
        for hk in hooks:
            hk.remove()
        p = caught["p"].permute(1, 0, 2).reshape(R, d).contiguous()                   # [M, n, d] -> rows image-major
        roi = caught["roi"].reshape(R, d, 49).permute(0, 2, 1).contiguous()           # [R, d, 7, 7] -> bin-major
        g_y = torch.randn(R, d, generator=torch.Generator().manual_seed(5100 + len(out)))
        y64, g64 = run_reference(module, h.box_pooler, feats, boxes, time_emb, cond if is_cond else None, p, roi, g_y, torch.float64)
        y32, g32 = run_reference(module, h.box_pooler, feats, boxes, time_emb, cond if is_cond else None, p, roi, g_y, torch.float32)
        assert g32["p"].dtype == torch.float32 and g64["p"].dtype == torch.float64
        if dead:
            assert float(g64["inst_interact.norm2.weight"][DEAD].abs()) == 0.0 and float(g64["inst_interact.norm2.bias"][DEAD].abs()) == 0.0
            assert float(g64["inst_interact.out_layer.weight"].reshape(d, 49, d)[:, :, DEAD].abs().max()) == 0.0
        pre = name + "."
        out[pre + "p"], out[pre + "roi"], out[pre + "G_y"] = p.numpy(), roi.numpy(), g_y.numpy()
        for k, v in module.state_dict().items():
            if k.startswith(LINK):
                out[pre + "sd." + k] = v.detach().numpy()
        for kind, t64, t32 in (("out", {"y": y64}, {"y": y32}), ("grad", g64, g32)):
            for k in t64:
                out["%s%s.%s" % (pre, kind, k)] = t64[k].numpy().astype(np.float32)
                dev = deviation(t32[k], t64[k])
                out["%sdev32.%s" % (pre, k)] = np.array(dev, dtype=np.float64)
                report.append("%-16s %-5s %-36s max|.| %.6e  fp32 run %.3e" % (name, kind, k, float(t64[k].abs().max()), dev))
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
        print("instance interaction gradient fixtures reproduced")
        return
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(path, **arrays)
    print("grads.npz", os.path.getsize(path), "bytes")
    print("\n".join(report))


if __name__ == "__main__":
    main()
