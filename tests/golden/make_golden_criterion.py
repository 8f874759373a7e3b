"""Generate the golden vectors of the training objective's forward by running the REFERENCE's own matcher, criterion and
prepare_diffusion_concat on the CPU (build container only).

    python tests/golden/make_golden_criterion.py            # writes tests/golden/criterion/*.npz
    python tests/golden/make_golden_criterion.py --check    # regenerates in memory and compares with the committed files

The reference's `box_head/loss.py` and `detector/diffusion_det.py` are imported under `_ref_shims.install()`.  The three third-party
functions the criterion calls through are stand-ins written here from their published definitions: torchvision.ops.box_iou,
torchvision.ops.boxes.box_area, fvcore.nn.sigmoid_focal_loss_jit.  Only data is stored.

sets.npz      per case (S = 1 head output, n images): `<case>.logits` [n, M, C], `.boxes` [n, M, 4] absolute xyxy, `.gt_boxes` [G, 4],
              `.gt_labels` [G] (1-based), `.gt_starts` [n + 1], `.sizes` [n, 2] (w, h); the reference's matching as `.assign` [n, M]
              (ground-truth index per query, -1 for none: the boolean mask and the index list in one array) and `.matched` [G] (the
              matcher's second return value, images one after the other); its loss dict from the fp32 run `.loss32` and from the same
              code on float64 inputs `.loss64` (loss_ce, loss_bbox, loss_giou); `.rounds` repair-loop rounds per image, `.conflicts`
              queries taken by several columns per image, `.dyn_k` [G].
q_sample.npz  per case: the recorded draws (`t`, `noise` [M, 4], `placeholder` [M, 4]: the reference reads its first M - G rows),
              `gt` [G, 4] normalised cxcywh, `size` (w, h) and the reference's diffused boxes times (w, h, w, h) as `_forward_train` scales them.

Stability is a condition on the sets, not a tolerance: a case is kept only if the reference's matching is identical in three runs --
fp32, float64, and fp32 with logits and boxes perturbed by a relative 1e-4.  A seed that fails, or that does not show what the case
is for, is skipped; a case for which no seed in 0 .. 39 does both fails the generator.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.environ.get("DVID_GOLDEN_OUT", os.path.join(HERE, "criterion"))
import _ref_shims as S  # noqa: E402

S.install()

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


# ---- stand-ins, from the published definitions --------------------------------------------------------------------------------------
def box_area(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def box_iou(boxes1, boxes2):
    area1, area2 = box_area(boxes1), box_area(boxes2)
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def sigmoid_focal_loss(inputs, targets, alpha=-1, gamma=2, reduction="none"):
    p = torch.sigmoid(inputs)
    ce_loss = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce_loss * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    if reduction == "mean":
        loss = loss.mean()
    elif reduction == "sum":
        loss = loss.sum()
    return loss


import torchvision.ops  # noqa: E402  (stub modules)
import torchvision.ops.boxes  # noqa: E402
import fvcore.nn  # noqa: E402

torchvision.ops.box_iou = box_iou
torchvision.ops.boxes.box_area = box_area
fvcore.nn.sigmoid_focal_loss_jit = sigmoid_focal_loss

from mega_core.modeling.roi_heads.box_head import loss as R  # noqa: E402
from mega_core.modeling.detector import diffusion_det as RD  # noqa: E402

ALPHA, GAMMA, OTA_K = 0.25, 2.0, 5
W_CLASS, W_L1, W_GIOU = 2.0, 5.0, 2.0
SEEDS = 40


def _cfg():
    return S.CfgNode({"MODEL": {"DiffusionDet": {"USE_FED_LOSS": False, "OTA_K": OTA_K, "ALPHA": ALPHA, "GAMMA": GAMMA}}})


def _criterion(num_classes):
    matcher = R.HungarianMatcherDynamicK(cfg=_cfg(), cost_class=W_CLASS, cost_bbox=W_L1, cost_giou=W_GIOU, use_focal=True)
    weights = {"loss_ce": W_CLASS, "loss_bbox": W_L1, "loss_giou": W_GIOU}
    return R.SetCriterionDynamicK(cfg=_cfg(), num_classes=num_classes, matcher=matcher, weight_dict=weights, eos_coef=0.1,
                                  losses=["labels", "boxes"], use_focal=True)


def _targets(gt_boxes, gt_labels, starts, sizes, dtype):
    """the dicts prepare_targets makes (diffusion_det.py:727-750), in `dtype`"""
    out = []
    for i in range(len(starts) - 1):
        b = gt_boxes[starts[i]:starts[i + 1]].to(dtype)
        w, h = sizes[i].to(dtype)
        whwh = torch.stack((w, h, w, h))
        n = b / whwh
        cxcywh = torch.stack(((n[:, 0] + n[:, 2]) / 2, (n[:, 1] + n[:, 3]) / 2, n[:, 2] - n[:, 0], n[:, 3] - n[:, 1]), dim=-1)
        out.append({"labels": gt_labels[starts[i]:starts[i + 1]].long(), "boxes": cxcywh, "boxes_xyxy": b, "image_size_xyxy": whwh,
                    "image_size_xyxy_tgt": whwh[None].repeat(len(b), 1)})
    return out


def run_reference(case, dtype, logits=None, boxes=None):
    """-> (assign [n, M], matched [G], loss dict, rounds [n], conflicts [n], dyn_k [G])"""
    logits = (case["logits"] if logits is None else logits).to(dtype)
    boxes = (case["boxes"] if boxes is None else boxes).to(dtype)
    starts = case["gt_starts"].tolist()
    targets = _targets(case["gt_boxes"], case["gt_labels"], starts, case["sizes"], dtype)
    crit = _criterion(logits.shape[-1])
    # what the cases are asserted on, read off the reference's own run: the repair loop calls torch.nonzero once per round, and
    # dynamic_k_matching receives the cost and the IoUs
    seen = {"rounds": [], "conflicts": [], "dyn_k": []}
    inner = crit.matcher.dynamic_k_matching
    real_nonzero = torch.nonzero

    def counted(cost, ious, num_gt):
        calls = [0]

        def nonzero(*a, **k):
            calls[0] += 1
            return real_nonzero(*a, **k)
        k = torch.clamp(torch.topk(ious, OTA_K, dim=0)[0].sum(0).int(), min=1)
        order = torch.sort(cost, dim=0, stable=True)[1]
        taken = torch.zeros_like(cost)
        for g in range(num_gt):
            taken[order[:int(k[g]), g], g] = 1
        seen["conflicts"].append(int((taken.sum(1) > 1).sum()))
        seen["dyn_k"].append(k.clone())
        torch.nonzero = nonzero
        try:
            out = inner(cost, ious, num_gt)
        finally:
            torch.nonzero = real_nonzero
        seen["rounds"].append(calls[0])
        return out
    crit.matcher.dynamic_k_matching = counted
    outputs = {"pred_logits": logits, "pred_boxes": boxes}
    indices, matched = crit.matcher(outputs, targets)
    losses = crit(outputs, targets)
    n, M = logits.shape[:2]
    assign = torch.full((n, M), -1, dtype=torch.int64)
    rounds, conflicts = [], []
    it = iter(range(10 ** 9))
    for i, (mask, idx) in enumerate(indices):
        assign[i, mask.bool()] = idx.long()
        if starts[i + 1] > starts[i]:
            j = next(it)
            rounds.append(seen["rounds"][j]), conflicts.append(seen["conflicts"][j])
        else:
            rounds.append(0), conflicts.append(0)
    dyn_k = torch.cat(seen["dyn_k"][:sum(1 for i in range(n) if starts[i + 1] > starts[i])]) if seen["dyn_k"] else torch.zeros(0, dtype=torch.int32)
    matched = torch.cat([m.long() for m in matched]) if matched else torch.zeros(0, dtype=torch.int64)
    return (assign, matched, {k: float(v) for k, v in losses.items()}, torch.tensor(rounds), torch.tensor(conflicts), dyn_k.to(torch.int32))


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
def natural(seed, M, C, counts, sizes=None, near=2, jitter=0.08, gt_scale=(0.08, 0.5)):
    """n images: random ground truth; the first near * G queries of an image are jittered copies of its boxes with a raised logit at the
    box's class, the rest random boxes with low logits"""
    g = torch.Generator().manual_seed(seed)
    n = len(counts)
    sizes = sizes or [(192 - 16 * (i % 3), 128 - 8 * (i % 2)) for i in range(n)]
    logits = torch.randn((n, M, C), generator=g) * 1.5 - 3.0
    boxes = torch.zeros((n, M, 4))
    gts, labs, starts = [], [], [0]
    for i, G in enumerate(counts):
        w, h = sizes[i]
        wh = torch.tensor([w, h], dtype=torch.float32)
        bw = (gt_scale[0] + (gt_scale[1] - gt_scale[0]) * torch.rand((G, 2), generator=g)) * wh
        c = bw / 2 + torch.rand((G, 2), generator=g) * (wh - bw)
        gt = torch.cat((c - bw / 2, c + bw / 2), dim=1)
        lab = torch.randint(1, C + 1, (G,), generator=g)
        rb = (0.05 + 0.4 * torch.rand((M, 2), generator=g)) * wh
        rc = rb / 2 + torch.rand((M, 2), generator=g) * (wh - rb)
        bx = torch.cat((rc - rb / 2, rc + rb / 2), dim=1)
        for r in range(min(near * G, M)):
            k = r % G
            size = gt[k, 2:] - gt[k, :2]
            d = (torch.rand((4,), generator=g) - 0.5) * 2 * jitter * torch.cat((size, size))
            bx[r] = gt[k] + d
            logits[i, r, lab[k] - 1] += 4.0 + torch.rand((), generator=g)
        boxes[i] = bx
        gts.append(gt), labs.append(lab), starts.append(starts[-1] + G)
    return {"logits": logits, "boxes": boxes, "gt_boxes": torch.cat(gts) if gts else torch.zeros((0, 4)),
            "gt_labels": torch.cat(labs).to(torch.int32) if labs else torch.zeros((0,), dtype=torch.int32),
            "gt_starts": torch.tensor(starts, dtype=torch.int32), "sizes": torch.tensor(sizes, dtype=torch.float32)}


def shared_query(seed, M=100, C=30):
    """two overlapping boxes of different classes, and a few queries near both: two columns claim one query"""
    case = natural(seed, M, C, [2], near=0)
    g = torch.Generator().manual_seed(1000 + seed)
    case["gt_boxes"] = torch.tensor([[40.0, 30.0, 100.0, 90.0], [44.0, 33.0, 104.0, 92.0]])
    case["gt_labels"] = torch.tensor([3, 7], dtype=torch.int32)
    for r in range(3):
        case["boxes"][0, r] = torch.tensor([42.0, 31.0, 102.0, 91.0]) + (torch.rand((4,), generator=g) - 0.5) * 3
        case["logits"][0, r, 2] += 5.0
        case["logits"][0, r, 6] += 4.0 - r
    return case


def repair_twice(seed, M=64, C=30):
    """two near-identical boxes of different classes with ONE query nearby, every other query thousands of image widths away: the loser's
    cheapest query of round 1 is the shared one again (the far ones cost more than the 100000 added to it), it loses it again, and round
    2 takes a far one"""
    case = natural(seed, M, C, [2], near=0)
    g = torch.Generator().manual_seed(2000 + seed)
    case["gt_boxes"] = torch.tensor([[40.0, 30.0, 100.0, 90.0], [40.5, 30.5, 100.5, 90.5]])
    case["gt_labels"] = torch.tensor([3, 7], dtype=torch.int32)
    w = float(case["sizes"][0, 0])
    far = 6000.0 * w + 50.0 * w * torch.rand((M, 2), generator=g)
    case["boxes"][0] = torch.cat((far, far * 1.002 + 20.0 * torch.rand((M, 2), generator=g)), dim=1)          # wide enough to survive the 1e-4
    case["boxes"][0, 5] = torch.tensor([41.0, 31.0, 99.0, 89.0])
    case["logits"][0, 5, 2] += 6.0
    return case


def all_outside(seed, M=65, C=30):
    """small boxes in one corner, every query in the opposite one: no centre in any box or centre region, the + 10000 branch decides"""
    case = natural(seed, M, C, [3], near=0)
    g = torch.Generator().manual_seed(3000 + seed)
    c = torch.tensor([12.0, 10.0]) + 6 * torch.rand((3, 2), generator=g)
    case["gt_boxes"] = torch.cat((c - 4, c + 4), dim=1)
    rc = torch.tensor([120.0, 80.0]) + torch.rand((M, 2), generator=g) * torch.tensor([50.0, 30.0])
    rb = 4 + 10 * torch.rand((M, 2), generator=g)
    case["boxes"][0] = torch.cat((rc - rb, rc + rb), dim=1)
    return case


CASES = [
    # name, maker, what the generator asserts about the reference's run
    ("empty_alone", lambda s: natural(s, 100, 30, [0]), lambda r, c: True),
    ("empty_mid_batch", lambda s: natural(s, 100, 30, [3, 0, 1]), lambda r, c: True),
    ("one_box", lambda s: natural(s, 63, 30, [1]), lambda r, c: True),
    ("ota_k_boxes", lambda s: natural(s, 64, 30, [OTA_K]), lambda r, c: True),
    ("boxes_64", lambda s: natural(s, 300, 30, [64], gt_scale=(0.04, 0.2)), lambda r, c: True),
    ("boxes_65", lambda s: natural(s, 300, 30, [65], gt_scale=(0.04, 0.2)), lambda r, c: True),
    ("boxes_256", lambda s: natural(s, 1000, 30, [256], gt_scale=(0.03, 0.12)), lambda r, c: True),
    ("shared_query", shared_query, lambda r, c: int(r[4].sum()) >= 1),
    ("repair_twice", repair_twice, lambda r, c: int(r[3].max()) >= 2),
    ("dynamic_k_above_1", lambda s: natural(s, 100, 30, [4], near=6, jitter=0.03), lambda r, c: int(r[5].max()) > 1),
    ("dynamic_k_all_1", lambda s: natural(s, 100, 30, [6], near=1, jitter=0.2, gt_scale=(0.05, 0.12)), lambda r, c: int(r[5].max()) == 1),
    ("all_outside", all_outside, lambda r, c: bool((r[0] >= 0).any())),
    ("rows_65", lambda s: natural(s, 65, 30, [7, 2]), lambda r, c: True),
    ("classes_1", lambda s: natural(s, 64, 1, [4]), lambda r, c: True),
    ("classes_64", lambda s: natural(s, 64, 64, [4]), lambda r, c: True),
    ("classes_65", lambda s: natural(s, 64, 65, [4]), lambda r, c: True),
    ("classes_80", lambda s: natural(s, 64, 80, [7]), lambda r, c: True),
    ("classes_1203", lambda s: natural(s, 64, 1203, [7]), lambda r, c: True),
]


def _outside_everything(case):
    """no query centre of `case` lies in a box or in a box's 2.5-radius centre region (computed here in float64)"""
    b, g = case["boxes"][0].double(), case["gt_boxes"].double()
    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    gx, gy, gw, gh = (g[:, 0] + g[:, 2]) / 2, (g[:, 1] + g[:, 3]) / 2, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    inside = ((cx[:, None] - gx[None]).abs() < 2.5 * gw[None]) & ((cy[:, None] - gy[None]).abs() < 2.5 * gh[None])
    return not bool(inside.any())


def make_sets():
    out, report = {}, []
    for name, maker, holds in CASES:
        for seed in range(SEEDS):
            case = maker(seed)
            r32 = run_reference(case, torch.float32)
            r64 = run_reference(case, torch.float64)
            g = torch.Generator().manual_seed(77 + seed)
            lp = case["logits"] * (1 + 1e-4 * (2 * torch.rand(case["logits"].shape, generator=g) - 1))
            bp = case["boxes"] * (1 + 1e-4 * (2 * torch.rand(case["boxes"].shape, generator=g) - 1))
            rp = run_reference(case, torch.float32, lp, bp)
            stable = all(torch.equal(r32[0], o[0]) and torch.equal(r32[1], o[1]) for o in (r64, rp))
            if stable and holds(r32, case):
                break
        else:
            raise SystemExit("case %s: no seed in 0 .. %d shows what the case is for with a matching that is identical in fp32, float64 and "
                             "perturbed fp32" % (name, SEEDS - 1))
        if name == "all_outside":
            assert _outside_everything(case)
        if name == "empty_mid_batch":
            assert case["gt_starts"].tolist() == [0, 3, 3, 4]
        for k, v in case.items():
            out["%s.%s" % (name, k)] = v.numpy()
        keys = ("loss_ce", "loss_bbox", "loss_giou")
        out[name + ".assign"], out[name + ".matched"] = r32[0].numpy().astype(np.int32), r32[1].numpy().astype(np.int32)
        out[name + ".loss32"] = np.array([r32[2][k] for k in keys], dtype=np.float64)
        out[name + ".loss64"] = np.array([r64[2][k] for k in keys], dtype=np.float64)
        out[name + ".rounds"], out[name + ".conflicts"], out[name + ".dyn_k"] = r32[3].numpy(), r32[4].numpy(), r32[5].numpy()
        report.append("%-18s seed %2d  M %4d  C %4d  G %-12s rounds %-10s conflicts %-10s max k %d" % (
            name, seed, case["logits"].shape[1], case["logits"].shape[2], np.diff(case["gt_starts"].numpy()).tolist(), r32[3].tolist(),
            r32[4].tolist(), int(r32[5].max()) if r32[5].numel() else 0))
    rows = sorted({out[n + ".logits"].shape[1] for n, _, _ in CASES})
    classes = sorted({out[n + ".logits"].shape[2] for n, _, _ in CASES})
    assert set(rows) >= {63, 64, 65, 100, 300, 1000} and set(classes) >= {1, 30, 64, 65, 80, 1203}, (rows, classes)
    return out, report


# ---- prepare_diffusion_concat on recorded draws ---------------------------------------------------------------------------------------
def make_q_sample(M=100, scale=2.0):
    betas = RD.cosine_beta_schedule(1000)
    ac = torch.cumprod(1.0 - betas, dim=0).to(torch.float32)
    stub = types.SimpleNamespace(num_timesteps=1000, device="cpu", num_proposals=M, scale=scale, sqrt_alphas_cumprod=torch.sqrt(ac),
                                 sqrt_one_minus_alphas_cumprod=torch.sqrt(1.0 - ac))
    stub.q_sample = lambda x_start, t, noise=None: RD.DiffusionDet.q_sample(stub, x_start=x_start, t=t, noise=noise)
    out = {"sqrt_alphas_cumprod": stub.sqrt_alphas_cumprod.numpy(), "sqrt_one_minus_alphas_cumprod": stub.sqrt_one_minus_alphas_cumprod.numpy(),
           "scale": np.float32(scale)}
    real_randn, real_randint = torch.randn, torch.randint
    for name, G, t, size in (("none", 0, 500, (192, 128)), ("three", 3, 0, (176, 120)), ("three_late", 3, 999, (176, 120)),
                             ("many", 37, 250, (160, 128)), ("full", M, 731, (192, 120))):
        g = torch.Generator().manual_seed(500 + G + t)
        wh = 0.05 + 0.5 * torch.rand((G, 2), generator=g)
        gt = torch.cat((wh / 2 + torch.rand((G, 2), generator=g) * (1 - wh), wh), dim=1)
        noise, placeholder = real_randn((M, 4), generator=g), real_randn((M, 4), generator=g)
        draws = [noise, placeholder[:M - max(G, 1)]]
        torch.randn = lambda *a, **k: draws.pop(0)
        torch.randint = lambda *a, **k: torch.tensor([t])
        try:
            diffused, noise_out, t_out = RD.DiffusionDet.prepare_diffusion_concat(stub, gt)
        finally:
            torch.randn, torch.randint = real_randn, real_randint
        assert torch.equal(noise_out, noise) and int(t_out) == t and len(draws) == (0 if G < M else 1)
        whwh = torch.tensor([size[0], size[1], size[0], size[1]], dtype=torch.float32)
        for k, v in (("gt", gt), ("t", torch.tensor(t)), ("noise", noise), ("placeholder", placeholder), ("size", torch.tensor(size, dtype=torch.float32)),
                     ("boxes", diffused * whwh[None, :])):
            out["%s.%s" % (name, k)] = v.numpy()
    return out


def main():
    torch.set_num_threads(1)
    sets, report = make_sets()
    made = {"sets.npz": sets, "q_sample.npz": make_q_sample()}
    if "--check" in sys.argv:
        for fname, arrays in made.items():
            have = np.load(os.path.join(OUT, fname))
            assert sorted(have.files) == sorted(arrays), "%s: the keys differ" % fname
            for k, v in arrays.items():
                assert have[k].dtype == np.asarray(v).dtype and np.array_equal(have[k], v), "%s: %s differs from the committed fixture" % (fname, k)
        print("criterion fixtures reproduced")
        return
    os.makedirs(OUT, exist_ok=True)
    for fname, arrays in made.items():
        np.savez_compressed(os.path.join(OUT, fname), **arrays)
        print(fname, os.path.getsize(os.path.join(OUT, fname)), "bytes")
    print("\n".join(report))


if __name__ == "__main__":
    main()
