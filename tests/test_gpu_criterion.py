"""The forward of the training objective on the GPU (ops.set_criterion, ops.q_sample_boxes; csrc/criterion.hip) against the fixtures made
from the reference's own matcher, criterion and prepare_diffusion_concat (tests/golden/make_golden_criterion.py).

The matching is compared exactly: every fixture is stable (identical in the reference's fp32, float64 and perturbed fp32 runs), so a
difference is a wrong kernel.  The losses are bounded against the reference's float64 run by _criterion_cases.BOUND.  q_sample_boxes is
compared exactly: the reference's path is plain fp32 arithmetic on the recorded draws, one operation at a time, which the kernel restates
with contraction off and correctly rounded divisions."""
import os

import numpy as np
import pytest
import torch

import _criterion_cases as CC

from diffusionvid_amd.modeling.roi_heads.box_head import loss as L

pytestmark = pytest.mark.gpu


def _ops():
    from diffusionvid_amd import ops
    return ops


@pytest.mark.parametrize("name", CC.NAMES)
def test_fixture_matching_equal_and_losses_bounded(name):
    case = CC.sets()[name]
    out = _ops().set_criterion(*CC.tensors(case, "cuda"), *CC.PARAMS)
    assign, mq, sums, status = (o.cpu() for o in out)
    assert int(status.abs().sum()) == 0
    assert np.array_equal(assign[0].numpy(), case["assign"]), "assign differs from the reference's matching"
    assert np.array_equal(CC.flat_matched(mq[0].numpy(), case["gt_starts"]), case["matched"]), "matched_query differs from the reference's"
    n, gmax = mq.shape[1:]
    counts = np.diff(case["gt_starts"])
    assert all((mq[0, i, counts[i]:] == -1).all() for i in range(n))
    assert float(sums[0, :, 3].sum()) == float((case["assign"] >= 0).sum())
    d = L.losses_from_sums(sums)
    dev = CC.rel_dev([d[k] for k in CC.KEYS], case["loss64"])
    print("%s: device vs float64 reference %.3e (the reference's fp32 run %.3e, bound %.3e)" % (
        name, dev, CC.rel_dev(case["loss32"], case["loss64"]), CC.BOUND))
    assert dev <= CC.BOUND


def test_seven_head_outputs_three_images_equal_the_sets_alone_bit_for_bit():
    """no cross-talk through the scratch or the outputs, and two runs of one call give the same bits"""
    ops = _ops()
    S, n, M, C = 7, 3, 65, 30
    logits, boxes, gt, lab, starts, sizes = CC.random_set(11, S, M, C, [3, 0, 40])
    dev = lambda t: t.cuda()
    first = [o.cpu() for o in ops.set_criterion(dev(logits), dev(boxes), dev(gt), dev(lab), starts, dev(sizes), *CC.PARAMS)]
    again = [o.cpu() for o in ops.set_criterion(dev(logits), dev(boxes), dev(gt), dev(lab), starts, dev(sizes), *CC.PARAMS)]
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert int(first[3].abs().sum()) == 0 and int((first[0] >= 0).sum()) > 0
    s = starts.tolist()
    for k in range(S):
        for i in range(n):
            g = s[i + 1] - s[i]
            one = ops.set_criterion(dev(logits[k:k + 1, i:i + 1]), dev(boxes[k:k + 1, i:i + 1]), dev(gt[s[i]:s[i + 1]]), dev(lab[s[i]:s[i + 1]]),
                                    torch.tensor([0, g], dtype=torch.int32), dev(sizes[i:i + 1]), *CC.PARAMS)
            a, q, sm, st = (o.cpu() for o in one)
            assert torch.equal(a[0, 0], first[0][k, i]) and torch.equal(q[0, 0, :g], first[1][k, i, :g]) and int(st) == 0
            assert torch.equal(sm[0, 0], first[2][k, i]), "the sums of head output %d, image %d differ in their bits" % (k, i)
    # and the host restatement matches the same sets the same way
    host = L.criterion_host(logits, boxes, gt, lab, starts, sizes, *CC.PARAMS)
    assert torch.equal(host[0], first[0]) and torch.equal(host[1], first[1])


def test_out_tuple_is_written_in_place():
    ops = _ops()
    case = CC.sets()["rows_65"]
    args = CC.tensors(case, "cuda")
    want = ops.set_criterion(*args, *CC.PARAMS)
    out = tuple(torch.full_like(o, 7) for o in want)
    got = ops.set_criterion(*args, *CC.PARAMS, out=out)
    assert all(g is o for g, o in zip(got, out)) and all(torch.equal(g, w) for g, w in zip(got, want))
    assert ops.set_criterion_scratch_bytes(1, 2, 65, 7) >= 2 * 7 * 65 * 5


def test_q_sample_boxes_equals_the_reference_on_the_recorded_draws():
    ops = _ops()
    z = np.load(os.path.join(CC.HERE, "golden", "criterion", "q_sample.npz"))
    names = ("none", "three", "three_late", "many", "full")
    t = lambda k: torch.from_numpy(z[k])
    gt = torch.cat([t(n + ".gt") for n in names])
    starts = torch.tensor(np.cumsum([0] + [z[n + ".gt"].shape[0] for n in names]), dtype=torch.int32)
    steps = torch.tensor([int(z[n + ".t"]) for n in names])
    noise, placeholder = torch.stack([t(n + ".noise") for n in names]), torch.stack([t(n + ".placeholder") for n in names])
    sizes = torch.stack([t(n + ".size") for n in names])
    got = ops.q_sample_boxes(gt.cuda(), starts, steps, t("sqrt_alphas_cumprod").cuda(), t("sqrt_one_minus_alphas_cumprod").cuda(), noise.cuda(),
                             placeholder.cuda(), float(z["scale"]), sizes).cpu()
    for i, n in enumerate(names):
        assert torch.equal(got[i], t(n + ".boxes")), "case %s: largest difference %g" % (n, float((got[i] - t(n + ".boxes")).abs().max()))
    host = L.q_sample_boxes_host(gt, starts, steps, t("sqrt_alphas_cumprod"), t("sqrt_one_minus_alphas_cumprod"), noise, placeholder,
                                 float(z["scale"]), sizes)
    assert torch.equal(host, got)
    with pytest.raises(_ops()._lib.DvidError, match=r"image 0 holds 101 ground-truth boxes, NUM_PROPOSALS is 100"):
        ops.q_sample_boxes(torch.rand((101, 4)).cuda(), torch.tensor([0, 101], dtype=torch.int32), steps[:1], t("sqrt_alphas_cumprod").cuda(),
                           t("sqrt_one_minus_alphas_cumprod").cuda(), noise[:1].cuda(), placeholder[:1].cuda(), 2.0, sizes[:1])


def _status_of(logits, boxes, gt, lab, ota_k=5):
    n = logits.shape[1]
    starts = torch.tensor([0, gt.shape[0]] + [gt.shape[0]] * (n - 1), dtype=torch.int32)
    sizes = torch.tensor([[192.0, 128.0]] * n)
    p = (CC.ALPHA, CC.GAMMA, ota_k, CC.W_CLASS, CC.W_L1, CC.W_GIOU)
    out = _ops().set_criterion(logits.cuda(), boxes.cuda(), gt.cuda(), lab.cuda(), starts, sizes, *p)
    host = L.criterion_host(logits, boxes, gt, lab, starts, sizes, *p)
    assert torch.equal(out[3].cpu(), host[3]), "the device and the host report different statuses"
    return out


def test_status_paths_through_legitimate_inputs():
    """each status from an input a caller can hand over; nothing here faults: the kernels check before they index"""
    logits, boxes, gt, lab, _, _ = CC.random_set(5, 1, 64, 30, [3])
    # a query with x2 < x1: the reference's assert
    bad = boxes.clone()
    bad[0, 0, 9] = torch.tensor([50.0, 10.0, 40.0, 30.0])
    out = _status_of(logits, bad, gt, lab)
    assert int(out[3][0, 0]) == L.STATUS_DEGENERATE and int((out[0] >= 0).sum()) == 0
    with pytest.raises(ValueError, match=r"image 0 of head output 0 ended with status 0x2: a box has x2 < x1"):
        L.raise_on_status(out[3])
    # a ground-truth box with y2 < y1
    gbad = gt.clone()
    gbad[1] = torch.tensor([10.0, 60.0, 40.0, 30.0])
    assert int(_status_of(logits, boxes, gbad, lab)[3][0, 0]) == L.STATUS_DEGENERATE
    # a label outside 1 .. C
    lbad = lab.clone()
    lbad[2] = 31
    assert int(_status_of(logits, boxes, gt, lbad)[3][0, 0]) == L.STATUS_LABEL
    # a logit that is not finite
    nf = logits.clone()
    nf[0, 0, 40, 3] = float("inf")
    st = int(_status_of(nf, boxes, gt, lab)[3][0, 0])
    assert st & L.STATUS_NONFINITE
    # the loop bound: one query, two boxes -- the query can serve one of them, the other stays empty in every round (the reference would
    # not return); reported after num_gt + 32 rounds
    out = _status_of(logits[:, :, :1], boxes[:, :, :1], gt[:2], lab[:2], ota_k=1)
    assert int(out[3][0, 0]) == L.STATUS_ROUNDS
    with pytest.raises(ValueError, match=r"status 0x1: the matcher's repair loop reached its bound of num_gt \+ 32 rounds"):
        L.raise_on_status(out[3])


def test_refusals_before_any_launch():
    ops = _ops()
    logits, boxes, gt, lab, starts, sizes = CC.random_set(6, 1, 64, 30, [3])
    c = lambda t: t.cuda()
    with pytest.raises(NotImplementedError, match=r"image 0 holds 257 ground-truth boxes, the limit is 256 \(DVID_CRITERION_MAX_GT\)"):
        ops.set_criterion(c(logits), c(boxes), c(gt[:1].repeat(257, 1)), c(lab[:1].repeat(257)), torch.tensor([0, 257], dtype=torch.int32), sizes, *CC.PARAMS)
    with pytest.raises(NotImplementedError, match=r"4 queries per image, the limit is OTA_K = 5 <= queries <= 4096"):
        ops.set_criterion(c(logits[:, :, :4]), c(boxes[:, :, :4]), c(gt), c(lab), starts, sizes, *CC.PARAMS)
    lib = ops._lib.load()
    assert lib.dvid_set_criterion(None, None, 1, 1, 64, 30, None, None, None, None, None, 0.25, 2.0, 65, 2.0, 5.0, 2.0, None, None, 1, None, None, None, 0,
                                  None) != 0
    assert b"OTA_K 65, the limit is 1 .. 64 (DVID_CRITERION_MAX_OTA_K)" in lib.dvid_last_error()
