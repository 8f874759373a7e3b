"""DiffusionDet.loss_gradients end to end on the GPU: the dict of compute_losses, and the gradient of the sum of the weighted losses with
respect to every kept head output -- bit-equal to ops.set_criterion_backward on the recorded head outputs, and within the bound of
_criterion_grad_cases of torch's autograd on loss.losses_host in float64 on their CPU copy.  The reduced synthetic model of the loss
tests: one bottleneck per ResNet stage, two heads, 100 boxes, a 128 x 192 canvas, fp16."""
import functools

import pytest
import torch

import _criterion_grad_cases as GC

pytestmark = pytest.mark.gpu

from diffusionvid_amd.modeling.roi_heads.box_head import loss as L  # noqa: E402

BLOCKS = (1, 1, 1, 1)
SMALL = ["MODEL.VID.MEGA.GLOBAL.ENABLE", False, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", False, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 0,
         "MODEL.DiffusionDet.NUM_HEADS", 2, "MODEL.DiffusionDet.NUM_PROPOSALS", 100, "MODEL.DiffusionDet.NUM_CLASSES", 30]
IMAGE_HW = [(96, 160), (128, 96), (128, 192)]
IDS = [12, 3, 40]
GT = [([[20.0, 10.0, 90.0, 70.0], [100.0, 30.0, 150.0, 90.0], [5.0, 50.0, 60.0, 95.0]], [3, 17, 30]), ([], []),
      ([[30.0, 20.0, 120.0, 100.0], [130.0, 60.0, 190.0, 120.0]], [1, 9])]


@functools.lru_cache(maxsize=None)
def _model(deep):
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    cfg, model = E._build(1, BLOCKS, "trained_like", extra=SMALL + ["MODEL.DiffusionDet.DEEP_SUPERVISION", deep], dtype="float16")
    model.noise_fn = synthetic.noise_fn
    return cfg, model


@functools.lru_cache(maxsize=None)
def _images():
    from diffusionvid_amd.utils import synthetic
    return [synthetic.synthetic_frame(50 + i, h, w, smooth=True) for i, (h, w) in enumerate(IMAGE_HW)]


def _targets():
    from diffusionvid_amd.structures.bounding_box import BoxList
    out = []
    for i in range(3):
        boxes, labels = GT[i]
        t = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), (IMAGE_HW[i][1], IMAGE_HW[i][0]), mode="xyxy")
        t.add_field("labels", torch.tensor(labels, dtype=torch.int64))
        out.append(t)
    return out


def _run(model):
    model.debug_taps = {}
    try:
        out = model.loss_gradients(_images(), _targets(), IDS)
        return out, model.debug_taps["train_heads"][0]
    finally:
        model.debug_taps = None


@pytest.mark.parametrize("deep", (True, False))
def test_loss_gradients_equal_the_backward_of_the_recorded_head_outputs(deep):
    from diffusionvid_amd import ops
    cfg, model = _model(deep)
    d = cfg.MODEL.DiffusionDet
    S = 2 if deep else 1
    (losses, d_logits, d_boxes), (logits, boxes, _, _) = _run(model)
    assert losses == model.compute_losses(_images(), _targets(), IDS)
    assert sorted(losses) == sorted(k + x for k in L.LOSS_KEYS for x in (("", "_0") if deep else ("",)))
    assert d_logits.is_cuda and d_boxes.is_cuda and d_logits.dtype == d_boxes.dtype == torch.float32
    assert tuple(d_logits.shape) == (S, 3, 100, 30) == tuple(logits.shape) and tuple(d_boxes.shape) == (S, 3, 100, 4) == tuple(boxes.shape)
    # the direct call on the recorded head outputs
    gt = torch.tensor(sum((g[0] for g in GT), []), dtype=torch.float32).reshape(-1, 4)
    lab = torch.tensor(sum((g[1] for g in GT), []), dtype=torch.int32)
    starts = torch.tensor([0, 3, 3, 5], dtype=torch.int32)
    sizes = torch.tensor([(w, h) for h, w in IMAGE_HW], dtype=torch.float32)
    p = (d.ALPHA, d.GAMMA, d.OTA_K, d.CLASS_WEIGHT, d.L1_WEIGHT, d.GIOU_WEIGHT)
    assign, _, _, status = ops.set_criterion(logits, boxes, gt.cuda(), lab.cuda(), starts, sizes.cuda(), *p)
    weights = (d.CLASS_WEIGHT, d.L1_WEIGHT, d.GIOU_WEIGHT)
    direct = ops.set_criterion_backward(logits, boxes, gt.cuda(), lab.cuda(), starts, sizes.cuda(), d.ALPHA, d.GAMMA, assign, status,
                                        GC.reference_coef(assign, weights))
    assert int(status.abs().sum()) == 0 and int((assign >= 0).sum()) >= 2 * S
    assert torch.equal(direct[0], d_logits) and torch.equal(direct[1], d_boxes)
    assert not bool(d_boxes[:, 1].any()) and bool(d_logits[:, 1].any()) and bool(d_boxes[:, 0].any())          # image 1 has no ground truth
    # torch's autograd on the host path, float64, on the CPU copy
    _, hl, hb = GC.host_gradients(L, logits, boxes, (gt, lab, starts, sizes), assign, torch.float64, d.ALPHA, d.GAMMA, weights)
    dev = (GC.deviation(d_logits, hl), GC.deviation(d_boxes, hb))
    print("deep supervision %s: loss_gradients vs losses_host float64: d_logits %.3e  d_boxes %.3e (bound %.3e / %.3e)" % ((deep,) + dev + GC.bound()))
    assert dev[0] <= GC.bound()[0] and dev[1] <= GC.bound()[1]
    assert not model.training and len(model._graphs) == 0


def test_what_loss_gradients_refuses():
    _, model = _model(True)
    with pytest.raises(NotImplementedError, match=r"the video item dict \(cur / ref_l / ref_g\) of the training protocol is not built"):
        model.loss_gradients({"cur": None, "ref_l": [], "ref_g": []}, [])
    many = _targets()
    from diffusionvid_amd.structures.bounding_box import BoxList
    many[0] = BoxList(torch.tensor([[1.0, 1.0, 9.0, 9.0]]).repeat(101, 1), (160, 96), mode="xyxy")
    many[0].add_field("labels", torch.ones(101, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match=r"image 0 holds 101 ground-truth boxes, MODEL\.DiffusionDet\.NUM_PROPOSALS is 100"):
        model.loss_gradients(_images(), many, IDS)
    with pytest.raises(ValueError, match=r"2 image_ids and 3 targets for 3 images"):
        model.loss_gradients(_images(), _targets(), IDS[:2])
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="training is out of scope"):
            model.loss_gradients(_images(), _targets(), IDS)
    finally:
        model.eval()
