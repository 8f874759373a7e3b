"""The gradient of the training objective on the GPU (ops.set_criterion_backward; csrc/criterion.hip: criterion_grad_kernel) against the
gradients the reference's own criterion backpropagates (tests/golden/criterion/grads.npz) and against torch's autograd on the host path
(loss.losses_host, float64, CPU), by the measure and the bound of _criterion_grad_cases; then autograd through SetCriterionDynamicK on
CUDA tensors."""
import os

import pytest
import torch

import _criterion_cases as CC
import _criterion_grad_cases as GC

from diffusionvid_amd.modeling.roi_heads.box_head import loss as L

pytestmark = pytest.mark.gpu

FOCAL = (CC.ALPHA, CC.GAMMA)


def _ops():
    from diffusionvid_amd import ops
    return ops


def _forward_backward(logits, boxes, gt, lab, starts, sizes, alpha=CC.ALPHA, gamma=CC.GAMMA, coef=None, out=None):
    """host tensors -> (assign, status, coef, d_logits, d_boxes) on the device: ops.set_criterion, the reference's coefficients, the gradient"""
    ops = _ops()
    dev = [t.cuda() for t in (logits, boxes, gt, lab)]
    sz = sizes.cuda()
    assign, _, _, status = ops.set_criterion(*dev, starts, sz, alpha, gamma, *CC.PARAMS[2:])
    coef = GC.reference_coef(assign) if coef is None else coef.cuda()
    d_logits, d_boxes = ops.set_criterion_backward(*dev, starts, sz, alpha, gamma, assign, status, coef, out=out)
    return assign, status, coef, d_logits, d_boxes


def _meets_host(logits, boxes, gt, lab, starts, sizes, assign, d_logits, d_boxes, alpha=CC.ALPHA, gamma=CC.GAMMA, what=""):
    """the device gradients against torch's autograd on losses_host in float64 on the CPU"""
    _, hl, hb = GC.host_gradients(L, logits, boxes, (gt, lab, starts, sizes), assign, torch.float64, alpha, gamma)
    dev = (GC.deviation(d_logits, hl), GC.deviation(d_boxes, hb))
    print("%s: device vs losses_host float64: d_logits %.3e  d_boxes %.3e (bound %.3e / %.3e)" % ((what,) + dev + GC.bound()))
    assert dev[0] <= GC.bound()[0] and dev[1] <= GC.bound()[1], what
    assert not bool(d_boxes.cpu()[assign.cpu() < 0].any()), "an unmatched query has a box gradient"


@pytest.mark.parametrize("name", CC.NAMES)
def test_fixture_gradients_bounded(name):
    case, truth = CC.sets()[name], GC.grads()[name]
    assign, status, _, d_logits, d_boxes = _forward_backward(*CC.tensors(case))
    assert int(status.abs().sum()) == 0 and torch.equal(assign[0].cpu(), torch.from_numpy(case["assign"]))
    dev = (GC.deviation(d_logits[0], truth["d_logits"]), GC.deviation(d_boxes[0], truth["d_boxes"]))
    print("%s: device vs the float64 reference: d_logits %.3e  d_boxes %.3e (the reference's fp32 run %.3e / %.3e, bound %.3e / %.3e)" % (
        (name,) + dev + tuple(truth["dev32"]) + GC.bound()))
    assert d_logits.dtype == d_boxes.dtype == torch.float32
    assert dev[0] <= GC.bound()[0] and dev[1] <= GC.bound()[1]
    assert not bool(d_boxes[0].cpu()[torch.from_numpy(case["assign"]) < 0].any()), "an unmatched query has a box gradient"
    if name == "empty_alone":
        assert not bool(d_boxes.any()) and bool(d_logits.any())


# M: the last chunk of 16 rows is full / holds one row; C: rows * C with a scalar tail, without one, not a multiple of 4
@pytest.mark.parametrize("M,C", [(16, 1), (17, 1), (65, 1), (16, 3), (17, 3), (65, 3), (17, 4), (65, 4), (16, 5), (17, 5), (65, 5), (17, 65), (65, 65),
                                 (17, 1203)])
def test_edges_of_the_decomposition(M, C):
    """two head outputs of two images: with M * C odd the second set starts off a 16-byte boundary, so the leading scalars run too"""
    args = CC.random_set(300 + M * 7 + C, 2, M, C, [3, 2])
    assign, status, _, d_logits, d_boxes = _forward_backward(*args)
    assert int(status.abs().sum()) == 0 and int((assign >= 0).sum()) >= 5
    _meets_host(*args, assign, d_logits, d_boxes, what="M %d C %d" % (M, C))


def test_seven_head_outputs_three_images_equal_the_head_outputs_alone_bit_for_bit():
    ops = _ops()
    S, n, M, C = 7, 3, 65, 31
    args = CC.random_set(12, S, M, C, [3, 0, 40])
    logits, boxes, gt, lab, starts, sizes = args
    assign, status, coef, d_logits, d_boxes = _forward_backward(*args)
    assert int(status.abs().sum()) == 0 and int((assign[:, 1] >= 0).sum()) == 0 and not bool(d_boxes[:, 1].any())
    _meets_host(*args, assign, d_logits, d_boxes, what="S 7 n 3")
    dev = [t.cuda() for t in (gt, lab)]
    for s in range(S):
        one = ops.set_criterion_backward(logits[s:s + 1].cuda(), boxes[s:s + 1].cuda(), *dev, starts, sizes.cuda(), *FOCAL, assign[s:s + 1].contiguous(),
                                         status[s:s + 1].contiguous(), coef[s:s + 1].contiguous())
        for i in range(n):
            assert torch.equal(one[0][0, i], d_logits[s, i]) and torch.equal(one[1][0, i], d_boxes[s, i]), "head output %d, image %d" % (s, i)


def test_kinks_follow_torch_autograd():
    """assign handed over directly: a query equal to its box, one sharing only x1 with it, one touching it with zero intersection width,
    one disjoint from it -- equal operands of a maximum / minimum split the gradient, clamp(min=0) passes it at exactly 0"""
    ops = _ops()
    gt = torch.tensor([[32.0, 24.0, 96.0, 88.0]])
    boxes = torch.tensor([[32.0, 24.0, 96.0, 88.0], [32.0, 30.0, 80.0, 70.0], [96.0, 30.0, 120.0, 70.0], [110.0, 90.0, 150.0, 120.0], [10.0, 10.0, 50.0, 50.0],
                          [40.0, 30.0, 90.0, 80.0]])[None, None]
    M, C = boxes.shape[2], 6
    logits = torch.linspace(-3.0, 2.0, M * C).reshape(1, 1, M, C)
    lab, starts, sizes = torch.tensor([4], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), torch.tensor([[256.0, 128.0]])          # dyadic: the L1 target is exact
    assign = torch.tensor([0, 0, 0, 0, -1, 0], dtype=torch.int32).reshape(1, 1, M)
    status = torch.zeros((1, 1), dtype=torch.int32)
    coef = GC.reference_coef(assign)
    d_logits, d_boxes = ops.set_criterion_backward(logits.cuda(), boxes.cuda(), gt.cuda(), lab.cuda(), starts, sizes.cuda(), *FOCAL, assign.cuda(),
                                                   status.cuda(), coef.cuda())
    _meets_host(logits, boxes, gt, lab, starts, sizes, assign, d_logits, d_boxes, what="kinks")
    db = d_boxes[0, 0].cpu()
    assert not bool(db[4].any()) and bool(db[[1, 2, 3, 5]].abs().sum(1).gt(0).all())
    # the equal query sits at GIoU's maximum: the L1 term is sign(0) = 0 and every maximum / minimum splits evenly, which leaves no
    # gradient at all (handing a tie to one operand would leave one of the size of its neighbours')
    assert float(db[0].abs().max()) <= GC.bound()[1] * float(db.abs().max())
    # the touching query (zero intersection width): the intersection still sends its gradient on -- a disjoint one does not; checked
    # against the host with the L1 and focal terms off
    only_giou = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)
    _, gb = ops.set_criterion_backward(logits.cuda(), boxes.cuda(), gt.cuda(), lab.cuda(), starts, sizes.cuda(), *FOCAL, assign.cuda(), status.cuda(),
                                       only_giou.cuda())
    _, _, hb = GC.host_gradients(L, logits, boxes, (gt, lab, starts, sizes), assign, torch.float64, weights=(0.0, 0.0, float(M - 1)))
    assert GC.deviation(gb, hb) <= GC.bound()[1]
    # query 2 touches the box: its intersection width is exactly 0 and clamp(min=0) still passes d inter / dw = h = 40 on to x1, which is
    # 8.1e-4 of the 7.9e-3 there (worked by hand: union 5056, hull 88 x 64).  Moved a quarter pixel off the box the width is negative, the
    # term is gone, and nothing else changes by more than a part in a thousand
    off = boxes.clone()
    off[0, 0, 2, 0] += 0.25
    _, gb_off = ops.set_criterion_backward(logits.cuda(), off.cuda(), gt.cuda(), lab.cuda(), starts, sizes.cuda(), *FOCAL, assign.cuda(), status.cuda(),
                                           only_giou.cuda())
    assert float(gb[0, 0, 2, 0]) > 1.05 * float(gb_off[0, 0, 2, 0]) > 0.0
    assert abs(float(gb[0, 0, 2, 0]) - 7.912e-3) <= 1e-5


def test_zeros_determinism_and_out():
    ops = _ops()
    S, n, M, C = 3, 2, 33, 30
    args = CC.random_set(31, S, M, C, [3, 4])
    logits, boxes, gt, lab, starts, sizes = args
    logits[1, 0, 20, 3] = float("inf")          # a legitimate input: NONFINITE on head output 1, image 0
    dev = [t.cuda() for t in (logits, boxes, gt, lab)]
    assign, _, _, status = ops.set_criterion(*dev, starts, sizes.cuda(), *CC.PARAMS)
    assert int(status[1, 0]) & L.STATUS_NONFINITE and int(status.abs().sum()) == int(status[1, 0])
    coef = GC.reference_coef(assign)
    coef[2] = 0          # head output 2: every coefficient 0
    coef[0, 1] = 0       # head output 0: no L1 term
    out = (torch.full((S, n, M, C), float("nan"), device="cuda"), torch.full((S, n, M, 4), float("nan"), device="cuda"))
    got = ops.set_criterion_backward(*dev, starts, sizes.cuda(), *FOCAL, assign, status, coef, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    d_logits, d_boxes = out
    assert bool(torch.isfinite(d_logits).all()) and bool(torch.isfinite(d_boxes).all())
    assert not bool(d_logits[2].any()) and not bool(d_boxes[2].any()), "a coef of 0 gives exact zeros"
    assert not bool(d_logits[1, 0].any()) and not bool(d_boxes[1, 0].any()), "a NONFINITE set gives zeros"
    assert bool(d_logits[1, 1].any()) and bool(d_boxes[1, 1].any()) and bool(d_logits[0].any()) and bool(d_boxes[0].any()), "beside nonzero neighbours"
    again = ops.set_criterion_backward(*dev, starts, sizes.cuda(), *FOCAL, assign, status, coef)
    assert torch.equal(again[0], d_logits) and torch.equal(again[1], d_boxes), "two runs give the same bits"
    # head output 0 without its L1 term, against the host with the same weights
    keep = [0]
    _, hl, hb = GC.host_gradients(L, logits[keep], boxes[keep], (gt, lab, starts, sizes), assign[keep], torch.float64, weights=(CC.W_CLASS, 0.0, CC.W_GIOU))
    assert GC.deviation(d_logits[keep], hl) <= GC.bound()[0] and GC.deviation(d_boxes[keep], hb) <= GC.bound()[1]


@pytest.mark.parametrize("alpha,gamma", [(-1.0, 2.0), (0.25, 1.5)])
def test_the_other_focal_branches(alpha, gamma):
    args = CC.random_set(41, 1, 33, 30, [4])
    assign, status, _, d_logits, d_boxes = _forward_backward(*args, alpha=alpha, gamma=gamma)
    assert int(status.abs().sum()) == 0
    _meets_host(*args, assign, d_logits, d_boxes, alpha, gamma, what="alpha %g gamma %g" % (alpha, gamma))


def test_refusals_before_any_launch():
    ops = _ops()
    lib = ops._lib.load()
    DvidError = ops._lib.DvidError
    logits, boxes, gt, lab, starts, sizes = CC.random_set(6, 1, 64, 30, [3])
    c = lambda t: t.cuda()
    assign, status = torch.full((1, 1, 64), -1, dtype=torch.int32).cuda(), torch.zeros((1, 1), dtype=torch.int32).cuda()
    coef = torch.ones((1, 3), dtype=torch.float64).cuda()
    with pytest.raises(DvidError, match=r"1281 classes exceed the limit of 1280 \(DVID_MAX_CLASSES\)"):
        ops.set_criterion_backward(torch.zeros((1, 1, 64, 1281)).cuda(), c(boxes), c(gt), c(lab), starts, sizes, *FOCAL, assign, status, coef)
    with pytest.raises(DvidError, match=r"4097 queries per image, the limit is 4096 \(DVID_CRITERION_MAX_ROWS\)"):
        ops.set_criterion_backward(torch.zeros((1, 1, 4097, 2)).cuda(), torch.zeros((1, 1, 4097, 4)).cuda(), c(gt), c(lab), starts, sizes, *FOCAL,
                                   torch.full((1, 1, 4097), -1, dtype=torch.int32).cuda(), status, coef)
    with pytest.raises(DvidError, match=r"image 0 holds 257 ground-truth boxes, the limit is 256 \(DVID_CRITERION_MAX_GT\)"):
        ops.set_criterion_backward(c(logits), c(boxes), c(gt[:1].repeat(257, 1)), c(lab[:1].repeat(257)), torch.tensor([0, 257], dtype=torch.int32), sizes,
                                   *FOCAL, assign, status, coef)
    assert lib.dvid_set_criterion_backward(None, None, 1, 1, 64, 30, None, None, None, None, None, 0.25, 2.0, None, None, None, None, None, None) != 0
    assert b"set criterion backward: null pointer" in lib.dvid_last_error()
    assert lib.dvid_set_criterion_backward(None, None, 70000, 1, 64, 30, None, None, None, None, None, 0.25, 2.0, None, None, None, None, None, None) != 0
    assert b"70000 head outputs x 1 images exceed 65535 sets per call" in lib.dvid_last_error()


def _criterion(num_classes):
    from diffusionvid_amd.config import get_cfg
    root = os.path.dirname(CC.HERE)
    cfg = get_cfg(os.path.join(root, "configs/still_R_101_DiffusionDet_p2.yaml"), [], os.path.join(root, "configs/BASE_RCNN_1gpu.yaml"))
    d = cfg.MODEL.DiffusionDet
    matcher = L.HungarianMatcherDynamicK(cfg, cost_class=d.CLASS_WEIGHT, cost_bbox=d.L1_WEIGHT, cost_giou=d.GIOU_WEIGHT, use_focal=True)
    return L.SetCriterionDynamicK(cfg, num_classes, matcher, {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0}, 0.1, ["labels", "boxes"], True)


def test_autograd_through_the_criterion_on_cuda_tensors():
    S, n, M, C = 3, 3, 40, 30
    args = CC.random_set(51, S, M, C, [3, 0, 5])
    logits, boxes, gt, lab, starts, sizes = args
    s = starts.tolist()
    targets = [{"labels": lab[s[i]:s[i + 1]].long().cuda(), "boxes_xyxy": gt[s[i]:s[i + 1]].cuda(),
                "image_size_xyxy": torch.cat((sizes[i], sizes[i])).cuda()} for i in range(n)]
    crit = _criterion(C)
    heads = [{"pred_logits": logits[k].cuda().requires_grad_(True), "pred_boxes": boxes[k].cuda().requires_grad_(True)} for k in range(S)]
    losses = crit(dict(heads[-1], aux_outputs=heads[:-1]), targets)
    sfx = ["_%d" % k for k in range(S - 1)] + [""]
    assert sorted(losses) == sorted(k + x for k in CC.KEYS for x in sfx)
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float64 and v.grad_fn is not None for v in losses.values())
    sum(w * losses[k + x] for x in sfx for k, w in zip(CC.KEYS, GC.WEIGHTS)).backward()
    # the bits of the direct call
    assign, status, _, d_logits, d_boxes = _forward_backward(*args)
    for k in range(S):
        assert torch.equal(heads[k]["pred_logits"].grad, d_logits[k]) and torch.equal(heads[k]["pred_boxes"].grad, d_boxes[k]), "head output %d" % k
    assert bool(d_logits.any()) and bool(d_boxes.any())
    # the values of the path without a gradient
    with torch.no_grad():
        plain = crit(dict(heads[-1], aux_outputs=heads[:-1]), targets)
    for k, v in plain.items():
        assert not v.is_cuda and v.grad_fn is None and v.dtype == torch.float64
        assert abs(losses[k].item() - float(v)) <= 1e-12 * abs(float(v)), k
