"""DiffusionDet.detect_images_aug end to end on the tiny models of test_gpu_still_images.py, bitwise against the composition the package
already allowed: the views built on the host with Pillow, plain detect_images per scale group with the draws of (image, view), and the
merge restated on the CPU (tests/_bbox_aug_ref.py) around the library's own tiled NMS -- so only the new code is under test."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _bbox_aug_ref as R  # noqa: E402
from test_gpu_still_images import BLOCKS, P2_OPTS, SMALL, _same  # noqa: E402

# 96 on the short side; scale 128 under MAX_SIZE 160 clamps the views of the two oblong images (128 * 1.4 = 179 > 160 -> 114 x 159)
AUG = ["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 1000, "TEST.BBOX_AUG.ENABLED", True]
FULL = AUG + ["TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (64, 128), "TEST.BBOX_AUG.SCALE_H_FLIP", True, "TEST.BBOX_AUG.MAX_SIZE", 160]
IMAGE_HW = [(70, 50), (50, 70), (64, 64), (50, 40)]          # the last one is only a companion: no view of it is larger than image 0's
IDS = [12, 3, 40, 7]
VARIANTS = [(False, "float16", 1), (False, "float16", 3), (False, "float32", 1), (False, "float32", 3), (True, "float16", 1)]


@functools.lru_cache(maxsize=None)
def _model(p2, dtype, step, full=True):
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    cfg, model = E._build(step, BLOCKS, "trained_like", extra=SMALL + (P2_OPTS if p2 else []) + (FULL if full else AUG), dtype=dtype)
    model.noise_fn = synthetic.noise_fn
    return cfg, model


@functools.lru_cache(maxsize=None)
def _images():
    from diffusionvid_amd.utils import synthetic
    out = []
    for i, (h, w) in enumerate(IMAGE_HW):
        f = synthetic.synthetic_frame(60 + i, h, w, smooth=True)
        out.append((f.permute(1, 2, 0) * 255).round().clamp(0, 255).to(torch.uint8).numpy())
    return out


def _canvas_hw(cfg, sel, group):
    from diffusionvid_amd.data.transforms import bbox_aug_views
    views = [[v for v in bbox_aug_views(cfg, (IMAGE_HW[i][1], IMAGE_HW[i][0])) if v.group == group] for i in sel]
    return -(-max(v[0].h for v in views) // 32) * 32, -(-max(v[0].w for v in views) // 32) * 32


def _composition(cfg, model, sel):
    """what the package allowed before detect_images_aug, for the images `sel`: -> one BoxList per image"""
    from PIL import Image
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.transforms import bbox_aug_scales, bbox_aug_views
    from diffusionvid_amd.structures.image_list import ImageList
    from diffusionvid_amd.utils import synthetic
    views = [bbox_aug_views(cfg, (IMAGE_HW[i][1], IMAGE_HW[i][0])) for i in sel]
    per_view = [[None] * len(views[0]) for _ in sel]
    model.noise_fn = lambda kind, fid, step, image, shape: synthetic.noise_fn(kind, fid // 64, step, fid % 64, shape)
    try:
        for g in range(len(bbox_aug_scales(cfg))):
            PH, PW = _canvas_hw(cfg, sel, g)
            slots, sizes, ids, where = [], [], [], []
            for k, i in enumerate(sel):
                for v, view in enumerate(views[k]):
                    if view.group != g:
                        continue
                    im = Image.fromarray(_images()[i]).resize((view.w, view.h), Image.BILINEAR)
                    if view.flip:
                        im = im.transpose(Image.FLIP_LEFT_RIGHT)
                    slot = torch.zeros(3, PH, PW)
                    slot[:, :view.h, :view.w] = torch.from_numpy(np.array(im)).permute(2, 0, 1).to(torch.float32).div(255)
                    slots.append(slot)
                    sizes.append(torch.Size((view.h, view.w)))
                    ids.append(IDS[i] * 64 + v)
                    where.append((k, v))
            with torch.no_grad():
                out = model.detect_images(ImageList(torch.stack(slots), sizes), ids)
            for (k, v), bl in zip(where, out):
                per_view[k][v] = bl.to(torch.device("cpu"))
    finally:
        model.noise_fn = synthetic.noise_fn

    def nms(boxes, scores, labels, size_wh, thr):
        ob, osc, ol, oc = ops.nms_frames_tiled(boxes[None].cuda(), scores[None].cuda(), labels.to(torch.int32)[None].cuda(), size_wh[0], size_wh[1], thr)
        m = int(oc[0])
        return ob[0, :m].cpu(), osc[0, :m].cpu(), ol[0, :m].cpu()
    heads = cfg.MODEL.ROI_HEADS
    merged = [R.merge(per_view[k], views[k], float(heads.NMS), int(heads.DETECTIONS_PER_IMG), nms=nms if len(per_view[k][0]) else R.plain_nms)
              for k in range(len(sel))]
    return merged, per_view


def _aug(model, sel):
    with torch.no_grad():
        out = model.detect_images_aug([_images()[i] for i in sel], [IDS[i] for i in sel])
    return [o.to(torch.device("cpu")) for o in out]


@pytest.mark.parametrize("p2,dtype,step", VARIANTS)
def test_aug_equals_the_composition_and_is_invariant(p2, dtype, step):
    cfg, model = _model(p2, dtype, step)
    sel = [0, 1, 2]
    got = _aug(model, sel)
    want, per_view = _composition(cfg, model, sel)
    differs = 0
    for k, i in enumerate(sel):
        h, w = IMAGE_HW[i]
        from diffusionvid_amd.data.transforms import get_size
        oh, ow = get_size((w, h), 96, 1000)
        assert got[k].size == (ow, oh) and got[k].mode == "xyxy" and got[k].get_field("labels").dtype == torch.int64 and len(got[k]) > 0
        assert got[k].bbox.min() >= 0 and got[k].bbox[:, 0::2].max() <= ow - 1 and got[k].bbox[:, 1::2].max() <= oh - 1
        assert len(per_view[k]) == 6 and all(len(bl) > 0 for bl in per_view[k])
        assert _same(got[k], want[k]), f"image {i}: {len(got[k])} detections, the composition has {len(want[k])}"
        differs += not (len(got[k]) == len(per_view[k][0]) and torch.equal(got[k].bbox, per_view[k][0].bbox))
    assert differs > 0          # the other views changed something
    # the batch in another order (the same canvases)
    order = [2, 0, 1]
    perm = _aug(model, order)
    for k, i in enumerate(order):
        assert _same(perm[k], got[sel.index(i)]), f"image {i} at position {k}"
    # tensors on the device and PIL images are the same input
    from PIL import Image
    with torch.no_grad():
        other = model.detect_images_aug([torch.from_numpy(_images()[0]).cuda(), Image.fromarray(_images()[1])], [IDS[0], IDS[1]])
    # (its canvases are those of images 0 and 1, which span the batch's: image 2 is smaller in every view)
    assert all(_canvas_hw(cfg, [0, 1], g) == _canvas_hw(cfg, sel, g) for g in range(3))
    assert _same(other[0].to(torch.device("cpu")), got[0]) and _same(other[1].to(torch.device("cpu")), got[1])


@pytest.mark.parametrize("dtype,step", [("float16", 1), ("float32", 3)])
def test_an_image_alone_equals_the_image_with_a_companion(dtype, step):
    """a scale group's canvas is as large as the group's largest view, and the backbone sees the padding: an image's detections do not
    depend on what shares its batch, or where it stands, as long as the canvases are the same -- image 0 alone against image 0 behind a
    companion that is smaller than it in every view"""
    cfg, model = _model(False, dtype, step)
    assert all(_canvas_hw(cfg, [0], g) == _canvas_hw(cfg, [3, 0], g) for g in range(3))
    alone = _aug(model, [0])
    pair = _aug(model, [3, 0])
    assert len(alone[0]) > 0 and _same(alone[0], pair[1])
    assert _same(_aug(model, [0, 3])[1], pair[0])


def test_enabled_without_any_augmentation_is_detect_images_after_the_extra_nms_and_cut():
    cfg, model = _model(False, "float16", 1, full=False)
    got = _aug(model, [0, 1, 2])
    want, per_view = _composition(cfg, model, [0, 1, 2])
    for k in range(3):
        assert len(per_view[k]) == 1 and _same(got[k], want[k]), k
        assert 0 < len(got[k]) <= len(per_view[k][0])


def test_device_draws_give_view_0_the_draws_of_detect_images():
    """synthetic.DeviceNoise: one launch per view and kind for consecutive ids; the result equals the run with the ids apart"""
    from diffusionvid_amd.utils import synthetic
    _, model = _model(False, "float16", 3)
    dn = synthetic.DeviceNoise()
    try:
        model.noise_fn = dn
        with torch.no_grad():
            both = model.detect_images_aug([_images()[0], _images()[1]], [5, 6])
            one = model.detect_images_aug([_images()[0], _images()[1]], [9, 6])
        got = model.stills.draws("renew", [5, 6], 1, (0, 1))
        assert torch.equal(got[0], dn.draw("renew", 5, 1, 0, 1, (40, 4), "cuda")[0]) and torch.equal(got[3], dn.draw("renew", 6, 1, 1, 1, (40, 4), "cuda")[0])
    finally:
        model.noise_fn = synthetic.noise_fn
    assert len(both[1]) > 0 and _same(both[1], one[1]) and not _same(both[0], one[0])


def test_refusals():
    _, model = _model(False, "float16", 1)
    with pytest.raises(ValueError, match="uint8"):
        model.detect_images_aug([torch.zeros(3, 40, 50)])
    with pytest.raises(ValueError, match="image_ids"):
        model.detect_images_aug([_images()[0]], [1, 2])
    assert model.detect_images_aug([]) == []
    import test_gpu_still_images as S
    _, plain = S._model(False, "float16", 1)
    with pytest.raises(NotImplementedError, match="ENABLED"):
        plain.detect_images_aug([_images()[0]])
