"""Generate the golden vectors of the local box-level attention branch by importing the REFERENCE modules (build container only).

    python tests/golden/make_golden_local.py

Builds the reference's own DynamicHead (mega_core/modeling/roi_heads/box_head/box_head.py:155-435) with
MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE True and MEGA.GLOBAL.ENABLE False at the reduced dimensions g5 uses, for STAGE 1 and
STAGE 2, and one local + global head whose output must equal the global-only head's on the same weights (asserted here: it is
the premise of "global overrides local", box_head.py:366-371).  Only data is stored: weights, inputs, outputs.

The fixture lives in tests/golden/local/: tests/test_golden_regeneration.py requires every .npz directly under tests/golden/ to come
out of make_golden.py, which this generator must not touch.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.environ.get("DVID_GOLDEN_OUT", os.path.join(HERE, "local"))
import _ref_shims as S  # noqa: E402

S.install()

import torch  # noqa: E402

from mega_core.modeling.roi_heads.box_head import box_head as BH  # noqa: E402

RED = dict(hidden=16, nheads=2, dim_ff=32, dim_dynamic=4, num_classes=30, num_proposals=100)


def randomize_norms(module, gen):
    """as make_golden.py: LayerNorm affine parameters and attention biases away from their defaults"""
    for m in module.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.weight.data.uniform_(0.5, 1.5, generator=gen)
            m.bias.data.uniform_(-0.3, 0.3, generator=gen)
        if isinstance(m, torch.nn.MultiheadAttention):
            m.in_proj_bias.data.uniform_(-0.2, 0.2, generator=gen)
            m.out_proj.bias.data.uniform_(-0.2, 0.2, generator=gen)


def make_head(local, stage, glob, seed):
    cfg = S.head_cfg(**RED)
    cfg.MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE = local
    cfg.MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE = stage
    cfg.MODEL.VID.MEGA.GLOBAL.ENABLE = glob
    shape = {k: SimpleNamespace(stride=s, channels=RED["hidden"]) for k, s in zip(["p3", "p4", "p5"], [8, 16, 32])}
    torch.manual_seed(seed)
    h = BH.DynamicHead(cfg, shape).eval()
    randomize_norms(h, torch.Generator().manual_seed(seed + 1))
    return h


def main():
    g = torch.Generator().manual_seed(180)
    n, (H, W), d, M = 2, (128, 192), RED["hidden"], RED["num_proposals"]
    feats = [torch.randn(n, d, H // s, W // s, generator=g) for s in (8, 16, 32)]
    cxcy = torch.rand(n, M, 2, generator=g) * torch.tensor([W, H]) * 1.2 - torch.tensor([W, H]) * 0.1
    wh = torch.exp(torch.rand(n, M, 2, generator=g) * 5.0 + 0.5)
    boxes = torch.cat([cxcy - wh / 2, cxcy + wh / 2], dim=-1)
    t = torch.full((n,), 999, dtype=torch.long)
    arrs = dict(p3=feats[0], p4=feats[1], p5=feats[2], boxes=boxes, t=t)

    # ONE set of weights: the local + global head holds every tensor, the others load the subset they have
    hlg = make_head(True, 2, True, 181)
    full = hlg.state_dict()
    h2 = make_head(True, 2, False, 182)          # two local stages
    h2.load_state_dict({k: v for k, v in full.items() if not k.startswith("global_attention.")})
    h1 = make_head(True, 1, False, 183)          # one: stage 0's parameters, the top-75 memory
    h1.load_state_dict({k: v for k, v in full.items() if not k.startswith(("global_attention.", "local_attention.1."))})
    hg = make_head(False, 1, True, 184)
    hg.load_state_dict({k: v for k, v in full.items() if not k.startswith("local_attention.")})
    with torch.no_grad():
        (cl, bx, pf), k1, k2 = h2(feats, boxes, t, None, box_extract=1)
        # the local memories of a 3-frame queue: this call's own top-k rows and one more frame's worth of other rows
        loc0 = torch.cat([k1, torch.randn(75, d, generator=g)])
        loc1 = torch.cat([k2, torch.randn(25, d, generator=g)])
        outs = {}
        for name, h in (("s1", h1), ("s2", h2)):
            h.proposal_feats_global = [None, None]
            h.proposal_feats_local = [loc0, loc1]
            h.proposals_feat_cur = [[cl.clone(), bx.clone(), pf.clone()]]
            outs[name] = h(feats, boxes, t, None)
        # local + global against global only, same weights
        mem0, mem1 = torch.randn(37, d, generator=g), torch.randn(11, d, generator=g)
        res = []
        for h in (hg, hlg):
            h.proposal_feats_global = [mem0, mem1]
            h.proposal_feats_local = [loc0, loc1]
            h.proposals_feat_cur = [[cl.clone(), bx.clone(), pf.clone()]]
            res.append(h(feats, boxes, t, None))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "local + global must equal global alone (box_head.py:366-371)"
    assert not torch.equal(outs["s1"][0], outs["s2"][0])
    arrs.update(ext_logits=cl, ext_boxes=bx, ext_feats=pf, loc0=loc0, loc1=loc1, s1_logits=outs["s1"][0], s1_boxes=outs["s1"][1],
                s2_logits=outs["s2"][0], s2_boxes=outs["s2"][1], mem0=mem0, mem1=mem1, lg_logits=res[1][0], lg_boxes=res[1][1])
    arrs.update({"sd.head." + k: v for k, v in full.items()})
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "g18_dynamic_head_local.npz"),
                        **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in arrs.items()})
    print("wrote g18_dynamic_head_local", {k: tuple(v.shape) for k, v in arrs.items() if not k.startswith("sd")})


if __name__ == "__main__":
    main()
