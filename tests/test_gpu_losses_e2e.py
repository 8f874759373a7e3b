"""DiffusionDet.compute_losses end to end on the GPU, against the composition of the pieces it sequences: the host form of q_sample on
the same draws, the detect path's backbone + plain_heads(intermediate=True), and the host restatement of the criterion on the downloaded
head outputs.  The reduced synthetic model: one bottleneck per ResNet stage, two heads, 100 boxes, a 128 x 192 canvas, both pyramids, fp16
and fp32 (the engine builds the heads at HIDDEN_DIM 256 only, so the head is not reduced).  Matching equal, losses within
_criterion_cases.BOUND of a float64 evaluation of the same sums; independent of batch order and chunking."""
import functools
import os

import pytest
import torch

import _criterion_cases as CC

pytestmark = pytest.mark.gpu

from diffusionvid_amd.modeling.roi_heads.box_head import loss as L  # noqa: E402

BLOCKS = (1, 1, 1, 1)
SMALL = ["MODEL.VID.MEGA.GLOBAL.ENABLE", False, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", False, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 0,
         "MODEL.DiffusionDet.NUM_HEADS", 2, "MODEL.DiffusionDet.NUM_PROPOSALS", 100, "MODEL.DiffusionDet.NUM_CLASSES", 30]
P2_OPTS = ["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"], "MODEL.FPN.IN_FEATURES", ["res2", "res3", "res4", "res5"]]
IMAGE_HW = [(96, 160), (128, 96), (128, 192)]
IDS = [12, 3, 40]
GT = [([[20.0, 10.0, 90.0, 70.0], [100.0, 30.0, 150.0, 90.0], [5.0, 50.0, 60.0, 95.0]], [3, 17, 30]), ([], []),
      ([[30.0, 20.0, 120.0, 100.0], [130.0, 60.0, 190.0, 120.0]], [1, 9])]
VARIANTS = [(p2, dtype) for p2 in (False, True) for dtype in ("float16", "float32")]


@functools.lru_cache(maxsize=None)
def _model(p2, dtype):
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    cfg, model = E._build(1, BLOCKS, "trained_like", extra=SMALL + (P2_OPTS if p2 else []), dtype=dtype)
    model.noise_fn = synthetic.noise_fn
    return cfg, model


@functools.lru_cache(maxsize=None)
def _images():
    from diffusionvid_amd.utils import synthetic
    return [synthetic.synthetic_frame(50 + i, h, w, smooth=True) for i, (h, w) in enumerate(IMAGE_HW)]


def _targets(order=(0, 1, 2)):
    from diffusionvid_amd.structures.bounding_box import BoxList
    out = []
    for i in order:
        boxes, labels = GT[i]
        t = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), (IMAGE_HW[i][1], IMAGE_HW[i][0]), mode="xyxy")
        t.add_field("labels", torch.tensor(labels, dtype=torch.int64))
        out.append(t)
    return out


def _run(model, order=(0, 1, 2), chunk=None):
    model.still_chunk, model.debug_taps = chunk, {}
    try:
        sums, dev = model.loss_sums([_images()[i] for i in order], _targets(order), [IDS[i] for i in order])
        return sums, dev, model.debug_taps["train_heads"][0]
    finally:
        model.still_chunk, model.debug_taps = None, None


def _sums64(logits, boxes, assign, gt, lab, whwh):
    """the four sums of one set in float64 from their definitions, under a given matching"""
    lg, bx, gt, whwh = logits.double(), boxes.double(), gt.double(), whwh.double()
    rows = torch.nonzero(assign >= 0)[:, 0]
    a = assign[rows].long()
    onehot = torch.zeros_like(lg)
    onehot[rows, lab[a].long() - 1] = 1
    focal = L.focal_terms(lg, onehot, CC.ALPHA, CC.GAMMA).sum()
    if rows.numel() == 0:
        return torch.stack((focal, focal * 0, focal * 0, focal * 0))
    l1 = (bx[rows] / whwh - gt[a] / whwh).abs().sum()
    giou = torch.diagonal(L._giou_pairs(bx[rows], gt[a])[0])
    return torch.stack((focal, l1, (1 - giou).sum(), torch.tensor(float(rows.numel()), dtype=torch.float64)))


@pytest.mark.parametrize("p2,dtype", VARIANTS)
def test_compute_losses_equals_the_composition_of_its_pieces(p2, dtype):
    from diffusionvid_amd import ops
    from diffusionvid_amd.utils import synthetic
    cfg, model = _model(p2, dtype)
    d = cfg.MODEL.DiffusionDet
    sums, dev, (logits, boxes, x_boxes, steps) = _run(model)
    S, n, M = logits.shape[:3]
    assert (S, n, M, logits.shape[3]) == (2, 3, 100, 30) and int(dev[3].abs().sum()) == 0
    # 1. t and the noisy boxes: the documented derivation of t, the host form of q_sample on the same draws
    sizes = torch.tensor([(w, h) for h, w in IMAGE_HW], dtype=torch.float32)
    assert steps.tolist() == [model.objective.train_step(i) for i in IDS] and all(0 <= t < 1000 for t in steps.tolist())
    gt_abs = torch.tensor(sum((g[0] for g in GT), []), dtype=torch.float32).reshape(-1, 4)
    lab = torch.tensor(sum((g[1] for g in GT), []), dtype=torch.int32)
    starts = torch.tensor([0, 3, 3, 5], dtype=torch.int32)
    whwh = torch.cat((sizes, sizes), dim=1)
    nb = gt_abs / whwh[[0, 0, 0, 2, 2]]
    gt_norm = torch.stack(((nb[:, 0] + nb[:, 2]) / 2, (nb[:, 1] + nb[:, 3]) / 2, nb[:, 2] - nb[:, 0], nb[:, 3] - nb[:, 1]), dim=1)
    noise = torch.stack([synthetic.noise_fn("train_noise", i, 0, 0, (M, 4)) for i in IDS])
    placeholder = torch.stack([synthetic.noise_fn("train_placeholder", i, 0, 0, (M, 4)) for i in IDS])
    want_x = L.q_sample_boxes_host(gt_norm, starts, steps, model.sqrt_alphas_cumprod.cpu(), model.sqrt_one_minus_alphas_cumprod.cpu(), noise,
                                   placeholder, model.scale, sizes)
    assert torch.equal(x_boxes.cpu(), want_x)
    # 2. the heads: the detect path's backbone and plain_heads(intermediate=True) on those boxes, launched here
    with torch.no_grad():
        canvas = torch.zeros((3, 3, 128, 192))
        for i, im in enumerate(_images()):
            canvas[i, :, :im.shape[1], :im.shape[2]] = im
        canvas = canvas.cuda()
        feats = model._get_engine().backbone_frames([canvas[i:i + 1] for i in range(3)])
        lg, bx = model.head.plain_heads(feats, want_x.cuda(), steps, intermediate=True)
        last = model.head.plain_heads(feats, want_x.cuda(), steps)
    assert torch.equal(lg, logits) and torch.equal(bx, boxes) and torch.equal(last[0], lg[-1]) and torch.equal(last[1], bx[-1])
    # 3. the criterion: the host restatement on the downloaded head outputs
    p = (d.ALPHA, d.GAMMA, d.OTA_K, d.CLASS_WEIGHT, d.L1_WEIGHT, d.GIOU_WEIGHT)
    host = L.criterion_host(logits.cpu(), boxes.cpu(), gt_abs, lab, starts, sizes, *p)
    assert torch.equal(host[0], dev[0].cpu()) and torch.equal(host[1], dev[1].cpu()), "the matching differs from the host restatement's"
    assert int((host[0] >= 0).sum()) >= 2
    truth = torch.stack([torch.stack([_sums64(logits[s, i].cpu(), boxes[s, i].cpu(), host[0][s, i], gt_abs[starts[i]:starts[i + 1]],
                                              lab[starts[i]:starts[i + 1]], whwh[i]) for i in range(n)]) for s in range(S)])
    want, got, hst = L.losses_from_sums(truth), L.losses_from_sums(sums), L.losses_from_sums(host[2])
    assert sorted(got) == sorted(k + s for k in CC.KEYS for s in ("", "_0"))
    worst = CC.rel_dev([got[k] for k in sorted(got)], [want[k] for k in sorted(got)])
    print("p2 %s %s: device losses vs float64 %.3e, host restatement %.3e (bound %.3e)" % (
        p2, dtype, worst, CC.rel_dev([hst[k] for k in sorted(got)], [want[k] for k in sorted(got)]), CC.BOUND))
    assert worst <= CC.BOUND
    # 4. the weighted dict
    losses = model.compute_losses(_images(), _targets(), IDS)
    w = {"loss_ce": d.CLASS_WEIGHT, "loss_bbox": d.L1_WEIGHT, "loss_giou": d.GIOU_WEIGHT}
    assert losses == {k: got[k] * w[k.split("_")[0] + "_" + k.split("_")[1]] for k in got}
    assert not model.training and len(model._graphs) == 0


def test_losses_do_not_depend_on_batch_order_or_chunking():
    _, model = _model(False, "float16")
    sums, dev, _ = _run(model)
    order = (2, 0, 1)
    for chunk in (None, 1, 2):
        s2, d2, _ = _run(model, order, chunk)
        for k, i in enumerate(order):
            assert torch.equal(s2[:, k], sums[:, i]), "image %d: its sums depend on the batch (chunk %s)" % (i, chunk)
            assert torch.equal(d2[0][:, k], dev[0][:, i])
    assert float(sums[:, 1, 3].sum()) == 0.0 and float(sums[:, 1, 1:3].abs().sum()) == 0.0          # the image with no ground truth


def test_validation_losses_sum_numerators_over_the_set(tmp_path):
    from diffusionvid_amd.engine.inference import validation_losses
    _, model = _model(False, "float16")
    whole = model.compute_losses(_images(), _targets(), IDS)
    from diffusionvid_amd.structures.image_list import ImageList
    tg = _targets()
    canvas = torch.zeros((3, 3, 128, 192))          # every batch on the whole set's canvas: a smaller canvas is another input to the backbone
    for i, im in enumerate(_images()):
        canvas[i, :, :im.shape[1], :im.shape[2]] = im
    batch = lambda idx: (ImageList(canvas[idx], [torch.Size(IMAGE_HW[i]) for i in idx]), [tg[i] for i in idx], [IDS[i] for i in idx])
    loader = [batch([2]), batch([0, 1])]
    out = validation_losses(model, loader, str(tmp_path))
    assert list(out)[:3] == ["loss_ce", "loss_bbox", "loss_giou"] and list(out)[-1] == "total_loss"
    for k, v in whole.items():
        assert abs(out[k] - v) <= 1e-12 * abs(v), k
    assert abs(out["total_loss"] - sum(whole.values())) <= 1e-12 * out["total_loss"]
    lines = open(os.path.join(str(tmp_path), "losses.txt")).read().split("\n")
    assert lines[0].startswith("loss_ce ") and len(lines) == len(out) + 1
    with pytest.raises(ValueError, match="image id 12 appears twice"):
        validation_losses(model, [loader[1], loader[1]])


def test_what_compute_losses_refuses():
    _, model = _model(False, "float16")
    with pytest.raises(NotImplementedError, match=r"the video item dict \(cur / ref_l / ref_g\) of the training protocol is not built"):
        model.compute_losses({"cur": None, "ref_l": [], "ref_g": []}, [])
    many = _targets()
    from diffusionvid_amd.structures.bounding_box import BoxList
    many[0] = BoxList(torch.tensor([[1.0, 1.0, 9.0, 9.0]]).repeat(101, 1), (160, 96), mode="xyxy")
    many[0].add_field("labels", torch.ones(101, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match=r"image 0 holds 101 ground-truth boxes, MODEL\.DiffusionDet\.NUM_PROPOSALS is 100"):
        model.compute_losses(_images(), many, IDS)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="training is out of scope"):
            model.compute_losses(_images(), _targets(), IDS)
    finally:
        model.eval()
