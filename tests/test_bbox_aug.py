"""TEST.BBOX_AUG, host side -- no GPU: the config keys, the view plan and its limits, the mirror of the Pillow-identical resize, the CPU
restatement of the merge on hand-placed boxes, the engine's routing, the raw dataset mode and the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

import _bbox_aug_ref as R
from conftest import ROOT

STILL = os.path.join(ROOT, "configs/still_R_101_DiffusionDet_p2.yaml")
BASE = os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml")


def _cfg(opts=(), yaml=STILL):
    from diffusionvid_amd.config import get_cfg
    cfg = get_cfg(yaml, list(opts), BASE)
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    return cfg


COCO_SIZES = ["INPUT.MIN_SIZE_TEST", 800, "INPUT.MAX_SIZE_TEST", 1333]          # (the base file's are the video path's 600 / 1000)


def _aug(h_flip=False, scales=(), scale_h_flip=False, max_size=4000, extra=COCO_SIZES):
    return ["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", h_flip, "TEST.BBOX_AUG.SCALES", tuple(scales),
            "TEST.BBOX_AUG.SCALE_H_FLIP", scale_h_flip, "TEST.BBOX_AUG.MAX_SIZE", max_size] + list(extra)


# ---- config -----------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_the_references():
    """mega_core/config/defaults.py:552-567, stated literally"""
    aug = _cfg().TEST.BBOX_AUG
    assert aug.ENABLED is False and aug.H_FLIP is False and tuple(aug.SCALES) == () and aug.MAX_SIZE == 4000 and aug.SCALE_H_FLIP is False
    shipped = _cfg(yaml=os.path.join(ROOT, "configs/still_R_101_DiffusionDet_p2_aug.yaml")).TEST.BBOX_AUG
    assert shipped.ENABLED and shipped.H_FLIP and tuple(shipped.SCALES) == (640, 960) and shipped.SCALE_H_FLIP and shipped.MAX_SIZE == 4000


# ---- the view plan ------------------------------------------------------------------------------------------------------------------------
def test_views_come_in_the_references_order():
    from diffusionvid_amd.data.transforms import bbox_aug_views, get_size
    cfg = _cfg(_aug(True, (640, 960), True))
    views = bbox_aug_views(cfg, (640, 480))
    assert [(v.flip, v.group) for v in views] == [(False, 0), (True, 0), (False, 1), (True, 1), (False, 2), (True, 2)]
    assert (views[0].h, views[0].w) == get_size((640, 480), 800, 1333) == (800, 1066)
    assert views[1][:2] == views[0][:2] and views[3][:2] == views[2][:2] == (853, 640) and views[4][:2] == (1280, 960)
    # the flips are independent switches
    assert [(v.w, v.flip) for v in bbox_aug_views(_cfg(_aug(False, (640,), True)), (640, 480))] == [(1066, False), (853, False), (853, True)]
    assert [(v.w, v.flip) for v in bbox_aug_views(_cfg(_aug(True, (640,), False)), (640, 480))] == [(1066, False), (1066, True), (853, False)]
    assert len(bbox_aug_views(_cfg(_aug()), (640, 480))) == 1


def test_max_size_clamps_a_scale_and_truncation_splits_the_ratios():
    from diffusionvid_amd.data.transforms import bbox_aug_views
    # 1000 x 400 at scale 960: 960 * 2.5 = 2400 > 2000 -> the short side becomes round(2000 * 400 / 1000) = 800
    v = bbox_aug_views(_cfg(_aug(False, (960,), False, max_size=2000)), (1000, 400))
    assert (v[0].w, v[0].h) == (1332, 533) and (v[1].w, v[1].h) == (2000, 800)
    assert (bbox_aug_views(_cfg(_aug(False, (960,))), (1000, 400))[1][:2]) == (2400, 960)          # the default 4000 does not clamp
    # 50 x 70: view 0 is 96 x int(96 * 70 / 50) = 96 x 134, scale 64 gives 64 x int(89.6) = 64 x 89: 96 / 64 != 134 / 89
    v = bbox_aug_views(_cfg(_aug(False, (64,), extra=["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 1000])), (50, 70))
    assert (v[0].w, v[0].h, v[1].w, v[1].h) == (96, 134, 64, 89)
    assert float(v[0].w) / v[1].w != float(v[0].h) / v[1].h


def test_construction_refuses_what_the_merge_cannot_take():
    from diffusionvid_amd.modeling.detector import build_detection_model
    eight = _aug(True, (640, 960, 1120), True)          # 2 + 3 * 2 = 8 views
    assert build_detection_model(_cfg(eight + ["MODEL.DiffusionDet.NUM_PROPOSALS", 512])).num_proposals == 512          # 4096 exactly
    with pytest.raises(NotImplementedError, match=r"BBOX_AUG.*8 views.*NUM_PROPOSALS.*513.*4104.*4096"):
        build_detection_model(_cfg(eight + ["MODEL.DiffusionDet.NUM_PROPOSALS", 513]))
    seventeen = _aug(False, tuple(range(400, 400 + 16 * 32, 32)), False)          # 1 + 16 views
    with pytest.raises(NotImplementedError, match=r"17 views.*241.*4097.*4096"):
        build_detection_model(_cfg(seventeen + ["MODEL.DiffusionDet.NUM_PROPOSALS", 241]))
    assert build_detection_model(_cfg(seventeen + ["MODEL.DiffusionDet.NUM_PROPOSALS", 240])).num_proposals == 240
    # SAMPLE_STEP 3: two sets of candidates per view
    with pytest.raises(NotImplementedError, match=r"SAMPLE_STEP.*3 - 1.*4104"):
        build_detection_model(_cfg(_aug(True, (640,), True) + ["MODEL.DiffusionDet.NUM_PROPOSALS", 513, "MODEL.DiffusionDet.SAMPLE_STEP", 3]))
    with pytest.raises(NotImplementedError, match=r"65 views.*limit is 64"):
        build_detection_model(_cfg(_aug(True, tuple(range(300, 363)), False) + ["MODEL.DiffusionDet.NUM_PROPOSALS", 10]))
    assert build_detection_model(_cfg(_aug(True, tuple(range(300, 362)), False) + ["MODEL.DiffusionDet.NUM_PROPOSALS", 10])).num_proposals == 10
    # the keys are not read while ENABLED is False
    off = _aug(True, (640, 960, 1120), True) + ["TEST.BBOX_AUG.ENABLED", False, "MODEL.DiffusionDet.NUM_PROPOSALS", 4096]
    assert build_detection_model(_cfg(off)).num_proposals == 4096


def test_views_plan_concatenates_the_tables():
    from diffusionvid_amd.data.transforms import ViewsPlan, resample_tables
    plan = ViewsPlan([(101, 150), (20, 30), (40, 64)], [(30, 45), (44, 66), (40, 32)])
    d = plan.desc
    assert d.shape == (3, 11) and d[:, :4].tolist() == [[101, 150, 30, 45], [20, 30, 44, 66], [40, 64, 40, 32]]
    assert d[2, 7] == -1 and (d[:, 4] >= 0).all() and (d[:2, 7] >= 0).all()          # image 2 keeps its height: no y pass
    for i, (a, b, col) in enumerate([(150, 45, 4), (30, 66, 4), (64, 32, 4)]):
        bd, kk = resample_tables(a, b)
        row, k0, ks = (int(x) for x in d[i, col:col + 3])
        assert ks == kk.shape[1] and np.array_equal(plan.bounds[row:row + b], bd) and np.array_equal(plan.weights[k0:k0 + kk.size], kk.reshape(-1))
    bd, kk = resample_tables(101, 30)
    assert np.array_equal(plan.bounds[d[0, 7]:d[0, 7] + 30], bd) and d[0, 9] == kk.shape[1]
    offs = d[:, 10].tolist()
    assert offs[0] == 0 and offs[1] >= 101 * 45 * 3 and offs[2] >= offs[1] + 20 * 66 * 3 and plan.tmp_bytes >= offs[2] + 40 * 32 * 3
    assert (plan.max_h, plan.max_ow, plan.max_oh) == (101, 66, 44)


# ---- resize + mirror ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,out_hw", [((101, 150), (30, 45)), ((20, 30), (44, 66)), ((40, 64), (40, 32)), ((33, 17), (70, 37))])
def test_resize_then_mirror_is_pillows(hw, out_hw):
    """a strong downscale (wide filter, odd ow), an upscale x2.2 (even ow), one axis kept, an odd upscale"""
    from PIL import Image
    from diffusionvid_amd.data.transforms import resize_u8_numpy
    img = np.random.default_rng(hw[0]).integers(0, 256, size=hw + (3,), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), Image.BILINEAR).transpose(Image.FLIP_LEFT_RIGHT))
    got = resize_u8_numpy(img, out_hw)[:, ::-1]
    assert got.shape == ref.shape and np.array_equal(got, ref)


# ---- the merge's restatement ---------------------------------------------------------------------------------------------------------------
THR = 0.5


def _views(cfg_opts, size_wh):
    from diffusionvid_amd.data.transforms import bbox_aug_views
    return bbox_aug_views(_cfg(cfg_opts), size_wh)


def test_a_box_of_the_flipped_view_survives_in_view_0():
    views = _views(_aug(True, extra=["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 1000]), (64, 64))          # 96 x 96 twice
    per_view = [R.boxlist([[10, 10, 30, 40]], [0.9], [2], (96, 96)), R.boxlist([[5, 20, 25, 50]], [0.8], [3], (96, 96))]
    out = R.merge(per_view, views, THR, 100)
    assert out.size == (96, 96) and out.get_field("labels").tolist() == [2, 3] and out.get_field("labels").dtype == torch.int64
    assert out.bbox.tolist() == [[10, 10, 30, 40], [96 - 25 - 1, 20, 96 - 5 - 1, 50]]


def test_a_duplicate_across_views_is_suppressed_inside_its_class_only():
    views = _views(_aug(False, (48,), extra=["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 1000]), (64, 64))          # 96 x 96, 48 x 48
    a, half = [20.0, 20.0, 60.0, 60.0], [10.0, 11.0, 30.0, 30.0]          # x2 -> (20, 22, 60, 60): IoU 0.95 with a
    assert R.iou(a, [2 * c for c in half]) >= THR + 0.05
    per_view = [R.boxlist([a], [0.9], [1], (96, 96)), R.boxlist([half, half], [0.8, 0.7], [1, 2], (48, 48))]
    out = R.merge(per_view, views, THR, 100)
    assert out.get_field("scores").tolist() == pytest.approx([0.9, 0.7]) and out.get_field("labels").tolist() == [1, 2]
    assert out.bbox[1].tolist() == [20, 22, 60, 60]
    # a neighbour below the threshold stays
    far = [25.0, 5.0, 45.0, 20.0]          # x2 -> (50, 10, 90, 40)
    assert R.iou(a, [2 * c for c in far]) <= THR - 0.05
    out = R.merge([per_view[0], R.boxlist([far], [0.8], [1], (48, 48))], views, THR, 100)
    assert len(out) == 2


def test_the_cut_keeps_a_tie_and_zero_keeps_all():
    views = _views(_aug(True, extra=["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 1000]), (64, 64))
    boxes = [[2.0 + 22 * i, 2.0, 20.0 + 22 * i, 20.0] for i in range(4)]          # disjoint
    per_view = [R.boxlist(boxes, [0.9, 0.5, 0.5, 0.3], [1, 1, 1, 1], (96, 96)), R.boxlist(np.zeros((0, 4)), [], [], (96, 96))]
    assert R.merge(per_view, views, THR, 2).get_field("scores").tolist() == pytest.approx([0.9, 0.5, 0.5])          # >= the 2nd score
    assert len(R.merge(per_view, views, THR, 3)) == 3 and len(R.merge(per_view, views, THR, 4)) == 4
    assert len(R.merge(per_view, views, THR, 0)) == 4 and len(R.merge(per_view, views, THR, 1)) == 1


def test_mapping_beyond_view_0_is_clipped():
    views = _views(_aug(False, (64,), extra=["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 1000]), (50, 70))          # 96 x 134, 64 x 89
    out = R.merge([R.boxlist(np.zeros((0, 4)), [], [], (96, 134)), R.boxlist([[10, 10, 63.8, 88.9]], [0.5], [1], (64, 89))], views, THR, 100)
    assert out.bbox[0, 2] == 95 and out.bbox[0, 3] == 133 and out.bbox[0, 0] == np.float32(10) * np.float32(96 / 64)


# ---- engine and data ---------------------------------------------------------------------------------------------------------------------
class _Fake:
    def __init__(self, enabled):
        self.cfg = _cfg(_aug() if enabled else [])
        self.calls = []

    def _out(self, name, images, ids):
        self.calls.append((name, len(images), list(ids)))
        return [R.boxlist([[1, 2, 30, 40]], [0.5], [1], (100, 50)) for _ in ids]

    def detect_images(self, images, image_ids=None):
        return self._out("plain", images, image_ids)

    def detect_images_aug(self, images, image_ids=None):
        return self._out("aug", images, image_ids)


@pytest.mark.parametrize("enabled,arg,want", [(False, None, "plain"), (True, None, "aug"), (False, True, "aug"), (True, False, "plain")])
def test_inference_images_routes_by_bbox_aug(enabled, arg, want):
    from diffusionvid_amd.engine.inference import inference_images
    model = _Fake(enabled)
    loader = [([np.zeros((50, 100, 3), np.uint8)] * 2, [7, 9], [(200, 100), (100, 50)])]
    preds = inference_images(model, loader, bbox_aug=arg)
    assert model.calls == [(want, 2, [7, 9])]
    assert preds[7].size == (200, 100) and preds[7].bbox.tolist() == [[2, 4, 60, 80]] and preds[9].size == (100, 50)


def test_raw_dataset_mode_and_collate_raw():
    from diffusionvid_amd.data.datasets import still
    files = {"a": np.full((40, 60, 3), 7, np.uint8), "b": np.full((60, 40, 3), 9, np.uint8), "c": np.full((30, 90, 3), 1, np.uint8)}
    ds = still.StillImageDataset(list(files), loader=files.__getitem__, image_ids=[5, 6, 8], min_size=80, max_size=160, raw=True)
    img, image_id, size = ds[1]
    assert img is files["b"] and image_id == 6 and size == (40, 60)
    assert ds.resized_size(2) == (159, 53)          # the sampler still sees the plain transform's sizes
    got = list(still.batches(ds, 2, raw=True))
    assert [(len(b[0]), b[1], b[2]) for b in got] == [(2, [5, 8], [(60, 40), (90, 30)]), (1, [6], [(40, 60)])]
    assert got[0][0][1] is files["c"] and got[0][0][0].dtype == np.uint8
    with pytest.raises(ValueError, match="raw"):
        next(still.batches(still.StillImageDataset(list(files), loader=files.__getitem__), 2, raw=True))
    plain = still.StillImageDataset(list(files), loader=files.__getitem__, min_size=80, max_size=160)
    assert tuple(plain[0][0].shape) == (3, 80, 120)          # the default mode is what it was


def test_c_abi_carries_the_two_entries():
    from diffusionvid_amd import _lib, ops
    lib = _lib.load()
    assert lib.dvid_version() >= 7
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    for name in ("dvid_resize_views_u8", "dvid_bbox_aug_merge"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header)
    from diffusionvid_amd.data import transforms
    assert int(re.search(r"#define DVID_BBOX_AUG_MAX_VIEWS (\d+)", header).group(1)) == transforms.BBOX_AUG_MAX_VIEWS == 64
    t = ops.bbox_aug_table([_views(_aug(True, (64,), True, extra=["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 1000]), (50, 70))])
    assert t.dtype == torch.float32 and t.shape == (4, 5)
    assert t[:, 2].tolist() == [0, 1, 0, 1] and t[0, 3:].tolist() == [1, 1] and t[2].tolist() == [64, 89, 0, np.float32(96 / 64), np.float32(134 / 89)]
