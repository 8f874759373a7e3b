"""The forward of the training objective without a GPU: the C ABI's declarations, the host restatement of the matcher and the criterion
(modeling/roi_heads/box_head/loss.py) against the fixtures made from the reference's own code, hand-worked cases, q_sample's two ends,
and every refusal's message."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _criterion_cases as CC

from diffusionvid_amd import _lib
from diffusionvid_amd.config import get_cfg
from diffusionvid_amd.modeling.roi_heads.box_head import loss as L

ROOT = os.path.dirname(CC.HERE)


def test_abi_carries_the_two_entry_points():
    """fails before the criterion exists: the header, _lib.SIGNATURES and the library carry the symbols, dvid_version() >= 12"""
    with open(os.path.join(ROOT, "include", "dvid_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in ("dvid_q_sample_boxes", "dvid_set_criterion", "dvid_set_criterion_scratch_bytes"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        decl = header.split(" %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
    assert lib.dvid_version() >= 12
    from diffusionvid_amd import ops
    for macro, value in (("MAX_GT", ops.CRITERION_MAX_GT), ("MAX_ROWS", ops.CRITERION_MAX_ROWS), ("MAX_OTA_K", ops.CRITERION_MAX_OTA_K),
                         ("REPAIR_SLACK", ops.CRITERION_REPAIR_SLACK), ("ERR_ROUNDS", L.STATUS_ROUNDS), ("ERR_DEGENERATE", L.STATUS_DEGENERATE),
                         ("ERR_NONFINITE", L.STATUS_NONFINITE), ("ERR_LABEL", L.STATUS_LABEL)):
        assert int(re.search(r"#define DVID_CRITERION_%s (\d+)" % macro, header).group(1)) == value
    assert (L.MAX_GT, L.MAX_ROWS, L.MAX_OTA_K) == (ops.CRITERION_MAX_GT, ops.CRITERION_MAX_ROWS, ops.CRITERION_MAX_OTA_K) and ops.CRITERION_MAX_GT == 256
    assert L.repair_bound(7) == 7 + ops.CRITERION_REPAIR_SLACK
    # the scratch: the cost matrix, one byte per entry of the matching matrix, the chunks' partial sums (no GPU needed)
    assert lib.dvid_set_criterion_scratch_bytes(6, 8, 500, 7) >= 6 * 8 * 7 * 500 * 5


def test_fixtures_cover_the_required_cases():
    s = CC.sets()
    assert tuple(sorted(s)) == CC.NAMES
    rows = {c["logits"].shape[1] for c in s.values()}
    classes = {c["logits"].shape[2] for c in s.values()}
    boxes = {int(g) for c in s.values() for g in np.diff(c["gt_starts"])}
    assert rows >= {63, 64, 65, 100, 300, 1000} and classes >= {1, 30, 64, 65, 80, 1203} and boxes >= {0, 1, CC.OTA_K, 64, 65, 256}
    assert s["empty_mid_batch"]["gt_starts"].tolist() == [0, 3, 3, 4] and s["empty_alone"]["gt_starts"].tolist() == [0, 0]
    assert s["shared_query"]["conflicts"].sum() >= 1 and s["repair_twice"]["rounds"].max() >= 2
    assert s["dynamic_k_above_1"]["dyn_k"].max() > 1 and s["dynamic_k_all_1"]["dyn_k"].max() == 1
    assert s["classes_1203"]["logits"].shape[1] == 64
    assert max(CC.rel_dev(c["loss32"], c["loss64"]) for c in s.values()) == CC.YARDSTICK


@pytest.mark.parametrize("name", CC.NAMES)
def test_host_restatement_equals_the_reference_matching_and_meets_the_bound(name):
    case = CC.sets()[name]
    info = {}
    assign, mq, sums, status = L.criterion_host(*CC.tensors(case), *CC.PARAMS, info=info)
    assert int(status.abs().sum()) == 0
    assert np.array_equal(assign[0].numpy(), case["assign"])
    assert np.array_equal(CC.flat_matched(mq[0].numpy(), case["gt_starts"]), case["matched"])
    live = [i for i in range(len(case["rounds"])) if case["gt_starts"][i + 1] > case["gt_starts"][i]]
    assert [info[(0, i)]["rounds"] for i in live] == [int(case["rounds"][i]) for i in live]
    assert [info[(0, i)]["conflict_rows"] for i in live] == [int(case["conflicts"][i]) for i in live]
    if live:
        assert np.array_equal(torch.cat([info[(0, i)]["dynamic_k"] for i in live]).numpy(), case["dyn_k"])
    d = L.losses_from_sums(sums)
    assert CC.rel_dev([d[k] for k in CC.KEYS], case["loss64"]) <= CC.BOUND


def _cfg(*extra):
    cfg = get_cfg(os.path.join(ROOT, "configs/still_R_101_DiffusionDet_p2.yaml"), list(extra), os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    return cfg


def _criterion(cfg, num_classes):
    d = cfg.MODEL.DiffusionDet
    matcher = L.HungarianMatcherDynamicK(cfg, cost_class=d.CLASS_WEIGHT, cost_bbox=d.L1_WEIGHT, cost_giou=d.GIOU_WEIGHT, use_focal=True)
    return L.SetCriterionDynamicK(cfg, num_classes, matcher, {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0}, 0.1, ["labels", "boxes"], True)


def _target(boxes, labels, w, h):
    b = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    whwh = torch.tensor([w, h, w, h], dtype=torch.float32)
    return {"labels": torch.tensor(labels, dtype=torch.int64), "boxes_xyxy": b, "image_size_xyxy": whwh,
            "image_size_xyxy_tgt": whwh[None].repeat(len(b), 1)}


def _focal(x, t, alpha=0.25, gamma=2.0):
    p = 1 / (1 + math.exp(-x))
    ce = max(x, 0) - x * t + math.log1p(math.exp(-abs(x)))
    pt = p * t + (1 - p) * (1 - t)
    return (alpha * t + (1 - alpha) * (1 - t)) * ce * (1 - pt) ** gamma


def test_one_prediction_on_one_box_by_hand():
    """the surface of the reference: dict in, dict out; GIoU loss 0, L1 0, and the closed-form focal value"""
    crit = _criterion(_cfg("MODEL.DiffusionDet.OTA_K", 1), 3)
    logits = torch.tensor([[[1.5, -2.0, 0.25]]])
    out = {"pred_logits": logits, "pred_boxes": torch.tensor([[[16.0, 8.0, 80.0, 72.0]]])}
    tg = [_target([[16.0, 8.0, 80.0, 72.0]], [2], 128, 128)]          # dyadic coordinates: the (cx, cy, w, h) round trip is exact
    losses = crit(out, tg)
    assert sorted(losses) == ["loss_bbox", "loss_ce", "loss_giou"]
    assert float(losses["loss_giou"]) == 0.0 and float(losses["loss_bbox"]) == 0.0
    want = _focal(1.5, 0) + _focal(-2.0, 1) + _focal(0.25, 0)
    assert abs(float(losses["loss_ce"]) - want) <= 4 * 2.0 ** -24 * want
    indices, matched = crit.matcher(out, tg)
    assert indices[0][0].tolist() == [True] and indices[0][1].tolist() == [0] and matched[0].tolist() == [0]
    assert indices[0][0].dtype == torch.bool and indices[0][1].dtype == torch.int64
    # auxiliary outputs: `_0 .. _{S-2}`, the final output without a suffix
    out["aux_outputs"] = [{"pred_logits": logits + 1, "pred_boxes": out["pred_boxes"]}, {"pred_logits": logits - 1, "pred_boxes": out["pred_boxes"]}]
    losses = crit(out, tg)
    assert sorted(losses) == sorted(k + s for k in CC.KEYS for s in ("", "_0", "_1"))
    assert abs(float(losses["loss_ce_0"]) - (_focal(2.5, 0) + _focal(-1.0, 1) + _focal(1.25, 0))) <= 1e-6
    assert abs(float(losses["loss_ce"]) - want) <= 4 * 2.0 ** -24 * want


def test_no_ground_truth_by_hand():
    crit = _criterion(_cfg(), 4)
    g = torch.Generator().manual_seed(3)
    logits = torch.randn((1, 9, 4), generator=g)
    boxes = torch.tensor([[10.0, 10.0, 50.0, 40.0]]).repeat(9, 1)[None]
    losses = crit({"pred_logits": logits, "pred_boxes": boxes}, [_target([], [], 128, 96)])
    assert float(losses["loss_bbox"]) == 0.0 and float(losses["loss_giou"]) == 0.0
    want = sum(_focal(float(x), 0) for x in logits.reshape(-1))          # divided by max(matched, 1) = 1
    assert abs(float(losses["loss_ce"]) - want) <= 1e-6 * want
    indices, matched = crit.matcher({"pred_logits": logits, "pred_boxes": boxes}, [_target([], [], 128, 96)])
    assert not indices[0][0].any() and indices[0][1].numel() == 0 and matched[0].numel() == 0


def test_q_sample_at_the_two_ends_of_the_schedule():
    """sqrt_alphas_cumprod 1: the ground truth comes back (and the placeholder rows); 0: the clamped noise"""
    g = torch.Generator().manual_seed(9)
    M, scale = 8, 2.0
    gt = torch.tensor([[0.5, 0.25, 0.25, 0.125], [0.75, 0.5, 0.125, 0.5]])
    noise, placeholder = torch.randn((2, M, 4), generator=g) * 1.5, torch.randn((2, M, 4), generator=g)
    sizes = torch.tensor([[128.0, 64.0], [96.0, 160.0]])
    starts = torch.tensor([0, 2, 2], dtype=torch.int32)
    table_a, table_b = torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0])
    at0 = L.q_sample_boxes_host(gt, starts, torch.tensor([0, 0]), table_a, table_b, noise, placeholder, scale, sizes)
    want = torch.tensor([[(0.5 - 0.125) * 128, (0.25 - 0.0625) * 64, (0.5 + 0.125) * 128, (0.25 + 0.0625) * 64],
                         [(0.75 - 0.0625) * 128, 0.25 * 64, (0.75 + 0.0625) * 128, 0.75 * 64]])
    assert torch.equal(at0[0, :2], want)
    assert torch.equal(at0[1, 0], torch.tensor([0.0, 0.0, 96.0, 160.0]))          # no ground truth: the fake box over the whole image
    pad = (placeholder[0, :M - 2] / 6.0 + 0.5)
    pad[:, 2:] = pad[:, 2:].clamp(min=1e-4)
    x = ((((pad * 2.0 - 1.0) * scale).clamp(-scale, scale) / scale) + 1) / 2.0
    assert torch.allclose(at0[0, 2:, 0], (x[:, 0] - 0.5 * x[:, 2]) * 128, rtol=0, atol=1e-4)
    at1 = L.q_sample_boxes_host(gt, starts, torch.tensor([1, 1]), table_a, table_b, noise, placeholder, scale, sizes)
    x = ((noise.clamp(-scale, scale) / scale) + 1) / 2.0
    whwh = torch.stack((sizes[:, 0], sizes[:, 1], sizes[:, 0], sizes[:, 1]), dim=1)[:, None, :]
    want = torch.stack((x[..., 0] - 0.5 * x[..., 2], x[..., 1] - 0.5 * x[..., 3], x[..., 0] + 0.5 * x[..., 2], x[..., 1] + 0.5 * x[..., 3]), dim=-1) * whwh
    assert torch.equal(at1, want) and bool((noise.abs() > scale).any())
    # and the recorded draws of the reference's prepare_diffusion_concat
    z = np.load(os.path.join(CC.HERE, "golden", "criterion", "q_sample.npz"))
    for n in ("none", "three", "three_late", "many", "full"):
        t = lambda k: torch.from_numpy(z[n + "." + k])
        got = L.q_sample_boxes_host(t("gt"), [0, t("gt").shape[0]], [int(z[n + ".t"])], torch.from_numpy(z["sqrt_alphas_cumprod"]),
                                    torch.from_numpy(z["sqrt_one_minus_alphas_cumprod"]), t("noise")[None], t("placeholder")[None], float(z["scale"]),
                                    t("size")[None])
        assert torch.equal(got[0], t("boxes")), n


def test_every_refusal_carries_its_message():
    logits, boxes, gt, lab, starts, sizes = CC.random_set(6, 1, 64, 30, [3])
    with pytest.raises(NotImplementedError, match=r"image 0 holds 257 ground-truth boxes, the limit is 256 \(DVID_CRITERION_MAX_GT\)"):
        L.criterion_host(logits, boxes, gt[:1].repeat(257, 1), lab[:1].repeat(257), [0, 257], sizes, *CC.PARAMS)
    with pytest.raises(NotImplementedError, match=r"4 queries per image, the limit is OTA_K = 5 <= queries <= 4096 \(DVID_CRITERION_MAX_ROWS\)"):
        L.criterion_host(logits[:, :, :4], boxes[:, :, :4], gt, lab, starts, sizes, *CC.PARAMS)
    with pytest.raises(NotImplementedError, match=r"1281 classes, the limit is 1 <= classes <= 1280 \(DVID_MAX_CLASSES\)"):
        L.criterion_host(torch.zeros((1, 1, 64, 1281)), boxes, gt, lab, starts, sizes, *CC.PARAMS)
    with pytest.raises(NotImplementedError, match=r"image 0 holds 9 ground-truth boxes, NUM_PROPOSALS is 8"):
        L.q_sample_boxes_host(torch.rand((9, 4)), [0, 9], [0], torch.ones(1), torch.zeros(1), torch.zeros((1, 8, 4)), torch.zeros((1, 8, 4)), 2.0, sizes)
    cfg = _cfg("MODEL.DiffusionDet.USE_FED_LOSS", True)
    with pytest.raises(NotImplementedError, match=r"MODEL\.DiffusionDet\.USE_FED_LOSS True is not built"):
        L.HungarianMatcherDynamicK(cfg, 2.0, 5.0, 2.0, use_focal=True)
    with pytest.raises(NotImplementedError, match=r"MODEL\.DiffusionDet\.USE_FED_LOSS True is not built"):
        L.SetCriterionDynamicK(cfg, 30, None, {}, 0.1, ["labels", "boxes"], True)
    with pytest.raises(NotImplementedError, match=r"only the focal-loss \(sigmoid\) branch is built \(USE_FOCAL: True\)"):
        L.HungarianMatcherDynamicK(_cfg(), 2.0, 5.0, 2.0, use_focal=False)
    # degenerate boxes, a label outside the classes, logits that are not finite: reported through the status, raised with image and head
    crit = _criterion(_cfg(), 30)
    bad = boxes.clone()
    bad[0, 0, 9] = torch.tensor([50.0, 10.0, 40.0, 30.0])
    tg = [_target(gt.tolist(), lab.tolist(), 192, 128)]
    with pytest.raises(ValueError, match=r"image 0 of head output 0 ended with status 0x2: a box has x2 < x1 or y2 < y1"):
        crit({"pred_logits": logits[0], "pred_boxes": bad[0]}, tg)
    with pytest.raises(ValueError, match=r"status 0x8: a ground-truth label lies outside 1 \.\. num_classes"):
        crit({"pred_logits": logits[0], "pred_boxes": boxes[0]}, [_target(gt.tolist(), [1, 31, 2], 192, 128)])
    nf = logits.clone()
    nf[0, 0, 3, 3] = float("nan")
    with pytest.raises(ValueError, match=r"status 0x4: the logits or a cost are not finite"):
        crit({"pred_logits": nf[0], "pred_boxes": boxes[0]}, tg)
    # the loop bound: one query for two boxes
    st = L.criterion_host(logits[:, :, :1], boxes[:, :, :1], gt[:2], lab[:2], [0, 2], sizes, 0.25, 2.0, 1, 2.0, 5.0, 2.0)[3]
    assert int(st[0, 0]) == L.STATUS_ROUNDS
    with pytest.raises(ValueError, match=r"image 0 of head output 0 ended with status 0x1: the matcher's repair loop reached its bound"):
        L.raise_on_status(st)


def test_training_draw_keys_leave_the_inference_keys_alone():
    from diffusionvid_amd.utils import synthetic
    from oracle import noise
    for kind in ("box_init", "img", "ddim", "renew"):
        for frame, step, image, video in ((0, 0, 0, 0), (7, 3, 2, 5), (100002, 63, 63, 9)):
            assert synthetic.draw_key(kind, frame, step, image, video) == noise.draw_key(kind, frame, step, image, video)
    keys = {synthetic.draw_key(k, f, 0, 0) for k in synthetic._KINDS for f in range(50)}
    assert len(keys) == len(synthetic._KINDS) * 50


@pytest.mark.skipif(not os.path.isdir("/root/reference/mega_core"), reason="the reference tree is only present in the build container")
def test_generator_check_mode_reproduces_the_fixtures():
    r = subprocess.run([sys.executable, os.path.join(CC.HERE, "golden", "make_golden_criterion.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "criterion fixtures reproduced" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
