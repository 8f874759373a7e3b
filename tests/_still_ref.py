"""Test-local restatement of still-image detection -- a batch of images, each with its own size, every frame on its own: no global
memory, no local attention, no conditioned heads -- composed from the oracle's existing primitives with a per-image `images_whwh` [B, 4]
(oracle/ itself is a yardstick and stays as it is).  tests/test_still_images.py pins it to OracleDiffusionDet.forward's state machine on a
batch of equal sizes; the GPU tests take their expected values from it.

The reference normalises x_start by the FIRST image's size for every image (diffusion_det.py:666-672, oracle/schedule.boxes_to_x_start);
here each image is normalised by its own row, as the published DiffusionDet does with its per-image images_whwh."""
import torch

from oracle import backbone_r101, detector as odet, head as ohead, postproc, schedule
from oracle.schedule import time_mlp


def canvas_of(images, divisible=32):
    """a list of [3, h, w] images -> (zero-padded canvas [n, 3, H, W] with H, W multiples of `divisible`, [(h, w)])"""
    sizes = [tuple(int(v) for v in im.shape[-2:]) for im in images]
    H = -(-max(s[0] for s in sizes) // divisible) * divisible
    W = -(-max(s[1] for s in sizes) // divisible) * divisible
    canvas = torch.zeros((len(images), 3, H, W), dtype=torch.float32)
    for i, im in enumerate(images):
        canvas[i, :, :sizes[i][0], :sizes[i][1]] = im
    return canvas, sizes


def plain_heads(sd, pfx, features, init_bboxes, t, cfg):
    """DynamicHead.forward for a model without attention: the NUM_HEADS RCNNHeads (box_head.py:286-299) and nothing behind them"""
    time = time_mlp(sd, pfx, t, cfg.hidden_dim)
    class_logits, bboxes, proposal_features = None, init_bboxes, None
    for i in range(cfg.num_heads):
        class_logits, bboxes, proposal_features = ohead.rcnn_head(sd, f"{pfx}head_series.{i}", features, bboxes, proposal_features, time, cfg)
    return class_logits, bboxes, proposal_features


def x_start_per_image(pred_boxes, images_whwh, scale):
    """schedule.boxes_to_x_start image by image: image i divided by its own row"""
    return torch.cat([schedule.boxes_to_x_start(pred_boxes[i:i + 1], images_whwh[i:i + 1], scale) for i in range(pred_boxes.shape[0])])


def detect_images(sd, cfg, noise_fn, canvas, sizes_hw, image_ids=None, backbone_fn=None, taps=None):
    """canvas [n, 3, H, W] fp32 in [0, 1] (zero-padded raw images), sizes_hw [(h, w)] -> [dict(boxes, scores, labels)] per image.
    Draws: noise_fn(kind, image_id, step, 0, (M, 4)) with kinds box_init (SAMPLE_STEP 1) / img, ddim, renew."""
    c = cfg
    n, M = canvas.shape[0], c.num_proposals
    ids = list(range(n)) if image_ids is None else list(image_ids)
    backbone_fn = backbone_fn or (lambda x: backbone_r101.backbone_r101_fpn(x, sd, "backbone.", c.blocks))
    fmaps = backbone_fn(backbone_r101.normalizer(canvas, c.pixel_mean, c.pixel_std))          # pad the raw image with zeros, then normalise
    feats = [fmaps[p] for p in c.in_features]
    whwh = torch.tensor([[w, h, w, h] for h, w in sizes_hw], dtype=torch.float32)
    buf = schedule.schedule_buffers(1000)
    pairs = schedule.time_pairs(1000, c.sample_step)

    def draw(kind, step):
        return torch.stack([noise_fn(kind, i, step, 0, (M, 4)) for i in ids])

    if c.sample_step == 1:
        t = torch.full((n,), pairs[0][0], dtype=torch.long)
        logits, boxes, _ = plain_heads(sd, "head.", feats, schedule.noise_to_boxes(draw("box_init", 0), whwh, c.snr_scale), t, c.head)
        if taps is not None:
            taps["final_0"] = (logits, boxes)
        return [postproc.inference_x1(logits[i:i + 1], boxes[i:i + 1], (sizes_hw[i][1], sizes_hw[i][0]), c.num_classes, c.use_nms)[0] for i in range(n)]
    img = draw("img", 0)
    ensemble = []
    for step, (time, time_next) in enumerate(pairs):
        if time_next < 0:
            break          # the last step's outputs reach nothing (diffusion_det.py:573-575)
        t = torch.full((n,), time, dtype=torch.long)
        logits, boxes, _ = plain_heads(sd, "head.", feats, schedule.noise_to_boxes(img, whwh, c.snr_scale), t, c.head)
        if taps is not None:
            taps[f"final_{step}"] = (logits, boxes)
        x_start = x_start_per_image(boxes, whwh, c.snr_scale)
        pred_noise = schedule.predict_noise_from_start(buf, img, t, x_start)
        img = odet.renew_and_ddim_step(buf, logits, pred_noise, x_start, time, time_next, list(draw("ddim", step)), list(draw("renew", step)))
        ensemble.append([postproc.topk_candidates(logits[b], boxes[b], c.num_classes)[:3] for b in range(n)])
    return [postproc.inference_ensemble([[e[i]] for e in ensemble], (sizes_hw[i][1], sizes_hw[i][0]), c.use_nms)[0] for i in range(n)]


class BaselineOracleDet(odet.OracleDiffusionDet):
    """OracleDiffusionDet's state machine (forward, unchanged) for the baseline configuration -- GLOBAL.ENABLE False, ATTENTION.ENABLE False:
    DynamicHead.forward returns the head series' outputs (box_head.py:319-321), the cached ones at SAMPLE_STEP 1.  oracle/head.head_final
    always attends a memory, so the final stage is restated here as _local_ref.LocalOracleDet restates the local branch."""

    def model_predictions(self, feats, images_whwh, x, t, cached=None, mem=None, box_extract=0):
        if box_extract:
            return super().model_predictions(feats, images_whwh, x, t, box_extract=box_extract)
        c = self.cfg
        if c.sample_step > 1:
            logits, boxes, _ = plain_heads(self.sd, "head.", feats, schedule.noise_to_boxes(x, images_whwh, c.snr_scale), t, c.head)
        else:
            logits, boxes, _ = cached
        x_start = schedule.boxes_to_x_start(boxes, images_whwh, c.snr_scale)
        return (schedule.predict_noise_from_start(self.buf, x, t, x_start), x_start), logits[None], boxes[None]


def video_noise_fn(image_noise_fn):
    """The draws of a video call whose frame f is still image f: `image_noise_fn(kind, image_id, step, 0, (M, 4))` re-keyed to the video
    protocol's (kind, call frame, step, image, shape) -- a batched draw [B, M, 4] (box_init, img) stacks the images' own, a per-image draw
    (ddim, renew) is image `call frame + image`'s.  One extraction split per call (no global frames), so box_init's step is 0."""
    def fn(kind, frame_id, step, image, shape, video=0):
        if len(shape) == 3:
            return torch.stack([image_noise_fn(kind, frame_id + j, 0, 0, tuple(shape[1:])) for j in range(shape[0])])
        return image_noise_fn(kind, frame_id + image, step, 0, tuple(shape))
    return fn
