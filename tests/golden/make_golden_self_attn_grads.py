"""Generate the golden gradients of the head's self-attention link and of the chain over all heads by running the REFERENCE's own RCNNHead
and DynamicHead.forward and backpropagating through them on the CPU (build container only).

    python tests/golden/make_golden_self_attn_grads.py            # writes tests/golden/self_attn/{link,chain}.npz
    python tests/golden/make_golden_self_attn_grads.py --check    # regenerates in memory and compares with the committed files

The reference is imported by make_golden.py (same shims), at make_golden.make_head()'s reduced size (hidden 16, 2 attention heads of 8,
dim_dynamic 4, 7 x 7 bins, 3 RCNNHeads).  n = 2 images, M = 7 boxes each.  Only data is stored.  backward() runs once with the module and the
inputs in float64 and once in fp32.

link    The reference's RCNNHead, the link isolated with hooks, without restating it: the head receives a LEAF pro_features x, a forward hook
        on `norm1` captures y, and the loss is sum(G_y * y) with a seeded cotangent, so the gradient reaches x and the link's six parameters
        and nothing else (asserted).
        link.npz   `in.x` [R, 16] (rows image-major), `in.G_y` [R, 16], `in.n`; `sd.<name>`: the link's parameters, the reference's names
                   without the head's prefix; `out.y` and `grad.{x,<name>}`: the float64 run, stored as float32; `dev32.<the same names>`:
                   the deviation of the fp32 run from the float64 run, max|got - truth| / max|truth|.
chain   The reference's DynamicHead.forward in training mode with return_intermediate (DEEP_SUPERVISION) and dropout 0, so the `detach` of
        the boxes between heads is the reference's own and not a restatement.  The attention branches behind head_series are switched off
        (`local_enable` / `global_enable`: the chain is head_series), `top_k` is cut to M.  A forward hook on the pooler returns recorded
        LEAF tiles per head (its outputs in a run without hooks, recorded first); a hook on time_mlp's sinusoid casts its fp32 output to the
        run's dtype.  The loss is a seeded linear functional of every head's logits and boxes.  Only head_series.* and time_mlp.* get a
        gradient (asserted).
        chain.npz  `in.tiles` [3, R, 49, 16] (bin-major), `in.boxes` [n, M, 4], `in.steps` [n], `in.time_in` [n, 16] (the sinusoid, fp32),
                   `in.G_logits` [3, n, M, 30], `in.G_boxes` [3, n, M, 4]; `sd.<name>`: head_series.* and time_mlp.* under the
                   DynamicHead's names; `out.{logits,boxes}`, `grad.{tiles,<name>}`, `dev32.<...>` as above.
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

OUT = os.path.join(G.OUT, "self_attn")
M = 7
STEPS = (999, 249)
LINK = ("self_attn.", "norm1.")
CHAIN = ("head_series.", "time_mlp.")


def store(out, report, name, kinds):
    """kinds: (kind, {key: float64 tensor}, {key: fp32 tensor}) -> `kind.key` as float32 and `dev32.key`"""
    for kind, t64, t32 in kinds:
        for k in t64:
            out["%s.%s" % (kind, k)] = t64[k].detach().numpy().astype(np.float32)
            dev = deviation(t32[k].detach(), t64[k].detach())
            out["dev32." + k] = np.array(dev, dtype=np.float64)
            report.append("%-6s %-5s %-52s max|.| %.6e  fp32 run %.3e" % (name, kind, k, float(t64[k].abs().max()), dev))


def run_link(module, pooler, feats, boxes, time_emb, x, g_y, dtype):
    """-> (y, {x, <parameter>: gradient}) of sum(g_y * y), the module and every input in `dtype`; x [R, d] rows image-major"""
    mod = copy.deepcopy(module).to(dtype)
    n, m = boxes.shape[:2]
    d = x.shape[-1]
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    caught = []
    hook = mod.norm1.register_forward_hook(lambda mo, i, o: caught.append(o))
    try:
        mod([f.to(dtype) for f in feats], boxes.to(dtype), xl.reshape(n, m, d), pooler, time_emb.to(dtype))
    finally:
        hook.remove()
    y = caught[0].permute(1, 0, 2).reshape(n * m, d)          # [M, n, d] -> rows image-major
    (g_y.to(dtype) * y).sum().backward()
    grads = {"x": xl.grad}
    for k, w in mod.named_parameters():
        if k.startswith(LINK):
            grads[k] = w.grad
        else:
            assert w.grad is None, "%s lies outside the link and got a gradient" % k
    return y.detach(), grads


def make_link(h, feats, boxes):
    module = h.head_series[1]
    n, d = boxes.shape[0], G.RED["hidden"]
    R = n * M
    g = torch.Generator().manual_seed(5200)
    x = torch.nn.functional.layer_norm(torch.randn(R, d, generator=g), (d,))
    g_y = torch.randn(R, d, generator=g)
    with torch.no_grad():
        time_emb = h.time_mlp(torch.tensor(STEPS, dtype=torch.long))
    y64, g64 = run_link(module, h.box_pooler, feats, boxes, time_emb, x, g_y, torch.float64)
    y32, g32 = run_link(module, h.box_pooler, feats, boxes, time_emb, x, g_y, torch.float32)
    assert g32["x"].dtype == torch.float32 and g64["x"].dtype == torch.float64 and len(g64) == 7
    out, report = {"in.x": x.numpy(), "in.G_y": g_y.numpy(), "in.n": np.array(n, dtype=np.int64)}, []
    for k, v in module.state_dict().items():
        if k.startswith(LINK):
            out["sd." + k] = v.detach().numpy()
    store(out, report, "link", (("out", {"y": y64}, {"y": y32}), ("grad", g64, g32)))
    return out, report


def run_chain(head, feats, boxes, steps, tiles, g_logits, g_boxes, dtype):
    """The reference's DynamicHead.forward in training mode -> (logits [H, n, M, C], boxes [H, n, M, 4], {tiles, <parameter>: gradient}).
    tiles [H, R, 49, d] bin-major: the pooler's hook hands head h its own, in the pooler's layout [R, d, 7, 7]"""
    mod = copy.deepcopy(head).to(dtype).train()
    d = tiles.shape[-1]
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in tiles]
    calls = []

    def pooled(mo, i, o):
        calls.append(len(calls))
        return leaves[calls[-1]].permute(0, 2, 1).reshape(-1, d, 7, 7)

    hooks = [mod.box_pooler.register_forward_hook(pooled), mod.time_mlp[0].register_forward_hook(lambda mo, i, o: o.to(dtype))]
    try:
        logits, out_boxes = mod([f.to(dtype) for f in feats], boxes.to(dtype), steps, None)
    finally:
        for hk in hooks:
            hk.remove()
    assert len(calls) == len(leaves) == logits.shape[0]
    ((g_logits.to(dtype) * logits).sum() + (g_boxes.to(dtype) * out_boxes).sum()).backward()
    grads = {"tiles": torch.stack([t.grad for t in leaves])}
    for k, w in mod.named_parameters():
        if k.startswith(CHAIN):
            grads[k] = w.grad
        else:
            assert w.grad is None, "%s lies outside the chain and got a gradient" % k
    assert all(v is not None for v in grads.values())
    return logits.detach(), out_boxes.detach(), grads


def make_chain(h, feats, boxes):
    head = copy.deepcopy(h)
    head.local_enable = head.global_enable = False          # the chain is head_series; the attention branches behind it are other links
    head.top_k = [M, M]
    assert head.return_intermediate and all(m.p == 0.0 for m in head.modules() if isinstance(m, torch.nn.Dropout))
    steps = torch.tensor(STEPS, dtype=torch.long)
    n, H = boxes.shape[0], len(head.head_series)
    recorded, sinus = [], []
    hooks = [head.box_pooler.register_forward_hook(lambda mo, i, o: recorded.append(o.detach())),
             head.time_mlp[0].register_forward_hook(lambda mo, i, o: sinus.append(o.detach()))]
    with torch.no_grad():
        head.train()(feats, boxes, steps, None)
    for hk in hooks:
        hk.remove()
    d = G.RED["hidden"]
    tiles = torch.stack([r.reshape(n * M, d, 49).permute(0, 2, 1).contiguous() for r in recorded])          # [R, d, 7, 7] -> bin-major
    g = torch.Generator().manual_seed(5300)
    g_logits = torch.randn(H, n, M, G.RED["num_classes"], generator=g)
    g_boxes = torch.randn(H, n, M, 4, generator=g) / 16
    l64, b64, g64 = run_chain(head, feats, boxes, steps, tiles, g_logits, g_boxes, torch.float64)
    l32, b32, g32 = run_chain(head, feats, boxes, steps, tiles, g_logits, g_boxes, torch.float32)
    assert g32["tiles"].dtype == torch.float32 and g64["tiles"].dtype == torch.float64
    out = {"in.tiles": tiles.numpy(), "in.boxes": boxes.numpy(), "in.steps": steps.numpy(), "in.time_in": sinus[0].numpy(),
           "in.G_logits": g_logits.numpy(), "in.G_boxes": g_boxes.numpy()}
    report = []
    for k, v in head.state_dict().items():
        if k.startswith(CHAIN):
            out["sd." + k] = v.detach().numpy()
    store(out, report, "chain", (("out", {"logits": l64, "boxes": b64}, {"logits": l32, "boxes": b32}), ("grad", g64, g32)))
    return out, report


def main():
    torch.set_num_threads(1)
    torch.backends.mha.set_fastpath_enabled(False)
    h, _ = G.make_head()
    feats, boxes, _ = G.make_inputs(520, n_frames=len(STEPS))
    boxes = boxes[:, :M].contiguous()
    made = {"link.npz": make_link(h, feats, boxes), "chain.npz": make_chain(h, feats, boxes)}
    for name, (arrays, report) in made.items():
        path = os.path.join(OUT, name)
        if "--check" in sys.argv:
            have = np.load(path)
            assert sorted(have.files) == sorted(arrays), "%s: the keys differ" % name
            for k, v in arrays.items():
                assert have[k].dtype == v.dtype and np.array_equal(have[k], v), "%s: %s differs from the committed fixture" % (name, k)
            continue
        os.makedirs(OUT, exist_ok=True)
        np.savez_compressed(path, **arrays)
        print(name, os.path.getsize(path), "bytes")
        print("\n".join(report))
    if "--check" in sys.argv:
        print("self-attention gradient fixtures reproduced")


if __name__ == "__main__":
    main()
