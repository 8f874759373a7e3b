"""The four-level pyramid p2..p5 (the reference's default config node, diffusion_det.py:155-159) on the host side: config acceptance and
refusals, the synthetic state dicts, the C ABI surface and the checkpoint path.  No GPU."""
import os
import re

import pytest
import torch

from conftest import ROOT

from _p2_ref import LEVEL2_RESNET, LEVEL2_SWIN

P2_YAML = os.path.join(ROOT, "configs", "still_R_101_DiffusionDet_p2.yaml")
BASE = os.path.join(ROOT, "configs", "BASE_RCNN_1gpu.yaml")
R101_YAML = os.path.join(ROOT, "configs", "vid_R_101_DiffusionVID.yaml")
NEW_SYMBOLS = {"dvid_backbone_resnet_fpn_levels_frames": 8, "dvid_backbone_swin_fpn_levels_frames": 8, "dvid_rcnn_head_levels": 18,
               "dvid_roialign_v2_levels": 11, "dvid_roialign_v2_levels_f32": 11}


def _cfg(yaml, opts=(), base=BASE):
    from diffusionvid_amd.config import get_cfg
    cfg = get_cfg(yaml, list(opts), base)
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)          # the pyramid does not depend on the depth: keep the state dict small
    return cfg


def _detector(cfg):
    from diffusionvid_amd.modeling.detector.diffusion_det import DiffusionDet
    return DiffusionDet(cfg)


def test_default_config_node_constructs_with_resnet():
    """the node as add_diffusiondet_config leaves it -- p2..p5 over res2..res5, COCO's 80 classes -- with the ResNet-FPN builder"""
    cfg = _cfg(None, ["MODEL.BACKBONE.NAME", "build_resnet_fpn_backbone"], None)
    assert list(cfg.MODEL.ROI_HEADS.IN_FEATURES) == ["p2", "p3", "p4", "p5"] and list(cfg.MODEL.FPN.IN_FEATURES) == ["res2", "res3", "res4", "res5"]
    model = _detector(cfg)
    assert model.fpn_levels == (2, 3, 4, 5) and model.num_classes == 80
    keys = set(model.state_dict())
    assert set(LEVEL2_RESNET) <= keys
    assert model.state_dict()["backbone.fpn_lateral2.weight"].shape == (256, 256, 1, 1)
    assert model.state_dict()["backbone.fpn_output2.weight"].shape == (256, 256, 3, 3)


def test_still_image_yaml_constructs():
    from diffusionvid_amd.modeling.detector import build_detection_model
    cfg = _cfg(P2_YAML)
    d = cfg.MODEL.DiffusionDet
    assert (cfg.MODEL.RESNETS.DEPTH, d.NUM_CLASSES, d.NUM_PROPOSALS, d.NUM_HEADS) == (101, 80, 500, 6)
    assert not cfg.MODEL.VID.MEGA.GLOBAL.ENABLE and not cfg.MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE
    model = build_detection_model(cfg)
    assert model.fpn_levels == (2, 3, 4, 5) and model.num_heads == 6 and set(LEVEL2_RESNET) <= set(model.state_dict())


def test_three_level_configs_are_unchanged():
    model = _detector(_cfg(R101_YAML))
    assert model.fpn_levels == (3, 4, 5) and not set(LEVEL2_RESNET) & set(model.state_dict())


SWIN_SMALL = dict(embed_dim=32, depths=(1, 1, 1, 1), heads=(1, 2, 4, 8), window=7)


def _swin_cfg(opts):
    from diffusionvid_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "configs", "vid_Swin_B_DiffusionVID.yaml"), list(opts), BASE)
    cfg.MODEL.SWIN.CONFIG_OVERRIDE = dict(SWIN_SMALL)
    return cfg


def test_swin_four_levels_construct():
    model = _detector(_swin_cfg(["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"], "MODEL.SWIN.OUT_FEATURES", (0, 1, 2, 3),
                                 "MODEL.FPN.IN_FEATURES", ["swin0", "swin1", "swin2", "swin3"]]))
    assert model.fpn_levels == (2, 3, 4, 5) and set(LEVEL2_SWIN) <= set(model.state_dict())
    assert model.state_dict()["backbone.fpn_lateral2.weight"].shape == (256, 32, 1, 1)


@pytest.mark.parametrize("case,opts,words", [
    ("p2 without res2", ["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"]], ("ROI_HEADS.IN_FEATURES", "FPN.IN_FEATURES")),
    ("res2 without p2", ["MODEL.FPN.IN_FEATURES", ["res2", "res3", "res4", "res5"]], ("ROI_HEADS.IN_FEATURES", "FPN.IN_FEATURES")),
    ("five levels", ["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5", "p6"], "MODEL.FPN.IN_FEATURES", ["res2", "res3", "res4", "res5"]],
     ("ROI_HEADS.IN_FEATURES", "FPN.IN_FEATURES")),
    ("two levels", ["MODEL.ROI_HEADS.IN_FEATURES", ["p4", "p5"], "MODEL.FPN.IN_FEATURES", ["res4", "res5"]], ("ROI_HEADS.IN_FEATURES", "FPN.IN_FEATURES")),
])
def test_inconsistent_pyramids_are_refused_resnet(case, opts, words):
    cfg = _cfg(R101_YAML, opts)
    with pytest.raises(NotImplementedError) as e:
        _detector(cfg)
    for w in words:
        assert w in str(e.value), (case, str(e.value))


@pytest.mark.parametrize("case,opts", [
    ("OUT_FEATURES (1,2,3) with p2", ["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"], "MODEL.FPN.IN_FEATURES", ["swin0", "swin1", "swin2", "swin3"]]),
    ("OUT_FEATURES (0,1,2,3) with p3", ["MODEL.SWIN.OUT_FEATURES", (0, 1, 2, 3)]),
])
def test_inconsistent_pyramids_are_refused_swin(case, opts):
    with pytest.raises(NotImplementedError) as e:
        _detector(_swin_cfg(opts))
    assert "ROI_HEADS.IN_FEATURES" in str(e.value) and "SWIN.OUT_FEATURES" in str(e.value), (case, str(e.value))


def test_synthetic_state_dicts_keep_every_value_and_add_the_level():
    """every existing seed keeps every existing value: the level-2 tensors are drawn behind everything else.  The expected values are a
    second draw with the level-less default plus hashes of two tensors recorded from the code before the level existed."""
    from diffusionvid_amd.utils import synthetic
    blocks = (1, 2, 2, 1)
    a = synthetic.make_state_dict(0, blocks=blocks)
    b = synthetic.make_state_dict(0, blocks=blocks, fpn_levels=(2, 3, 4, 5))
    assert set(b) - set(a) == set(LEVEL2_RESNET) and list(b)[:len(a)] == list(a)
    assert all(torch.equal(a[k], b[k]) for k in a)
    # recorded on the parent commit: float64 sums of two tensors drawn late
    assert abs(a["backbone.fpn_output5.weight"].double().sum().item() - PARENT_SUMS["r.fpn_output5.weight"]) < 1e-9
    assert abs(a["backbone.fpn_lateral3.bias"].double().sum().item() - PARENT_SUMS["r.fpn_lateral3.bias"]) < 1e-9
    sw = dict(embed_dim=32, depths=(2, 2, 2, 2), heads=(1, 2, 4, 8))
    s3 = synthetic.make_swin_state_dict(3, **sw)
    s4 = synthetic.make_swin_state_dict(3, **sw, fpn_levels=(2, 3, 4, 5))
    assert set(s4) - set(s3) == set(LEVEL2_SWIN) and all(torch.equal(s3[k], s4[k]) for k in s3)
    assert abs(s3["backbone.fpn_output5.weight"].double().sum().item() - PARENT_SUMS["s.fpn_output5.weight"]) < 1e-9
    assert s4["backbone.fpn_lateral2.weight"].shape == (256, 32, 1, 1) and s4["backbone.bottom_up.norm0.weight"].shape == (32,)
    with pytest.raises(ValueError):
        synthetic.make_state_dict(0, blocks=blocks, fpn_levels=(2, 3, 4, 5, 6))


# make_state_dict(0, blocks=(1, 2, 2, 1)) / make_swin_state_dict(3, embed_dim=32, depths=(2, 2, 2, 2), heads=(1, 2, 4, 8)) before fpn_levels existed
PARENT_SUMS = {"r.fpn_output5.weight": -30.963268854026378, "r.fpn_lateral3.bias": 0.08140076615381986, "s.fpn_output5.weight": 5.794623528419088}


def test_header_binding_and_library_carry_the_new_symbols():
    from diffusionvid_amd import _lib
    lib = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvid_hip.h")).read(), flags=re.S)
    for name, nargs in NEW_SYMBOLS.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert decl, f"{name} is not declared in include/dvid_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None
    assert lib.dvid_version() >= 2


def test_new_entry_points_are_documented_with_the_lines_they_replace():
    txt = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    assert "box_head.py:250-271" in txt and "FPN.forward" in txt


def _small_detector(levels):
    opts = []
    if levels == 4:
        opts += ["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"], "MODEL.FPN.IN_FEATURES", ["res2", "res3", "res4", "res5"]]
    return _detector(_cfg(R101_YAML, opts))


def test_four_level_state_dict_loads_through_the_checkpoint_path(tmp_path):
    """a DiffusionDet-style checkpoint (DataParallel prefix, all heads in one head_series list) with the level-2 tensors, through
    DetectronCheckpointer: every tensor arrives, the level-2 ones included"""
    from diffusionvid_amd.utils import checkpoint
    model = _small_detector(4)
    src = {k: v.clone() + 0.25 for k, v in model.state_dict().items() if torch.is_floating_point(v)}
    ck = {}
    for k, v in src.items():
        m = re.match(r"head\.head_series_cond\.(\d+)\.(.*)", k)
        ck["module." + (f"head.head_series.{int(m.group(1)) + model.num_heads}.{m.group(2)}" if m else k)] = v
    path = str(tmp_path / "p2.pth")
    torch.save({"model": ck}, path)
    ckpt = checkpoint.DetectronCheckpointer(model.cfg, model)
    ckpt.load(path, use_latest=False)
    assert ckpt.missed_keys == []
    got = model.state_dict()
    for k in LEVEL2_RESNET + ("backbone.fpn_lateral3.weight", "head.head_series_cond.0.class_logits.weight"):
        assert torch.equal(got[k], src[k]), k


def test_three_level_checkpoint_into_a_four_level_model_names_the_level(tmp_path):
    from diffusionvid_amd.utils import checkpoint
    three, four = _small_detector(3), _small_detector(4)
    path = str(tmp_path / "p3.pth")
    torch.save({"model": three.state_dict()}, path)
    with pytest.raises(KeyError) as e:
        checkpoint.DetectronCheckpointer(four.cfg, four).load(path, use_latest=False)
    assert "fpn_lateral2" in str(e.value)
    with pytest.raises(RuntimeError) as e:          # and the plain strict load
        four.load_state_dict(three.state_dict())
    assert "fpn_lateral2" in str(e.value)
    # the other way round nothing is missing for the three-level model: the checkpoint's extra level is ignored, as the reference's loader does
    ck = checkpoint.DetectronCheckpointer(three.cfg, three)
    torch.save({"model": four.state_dict()}, path)
    ck.load(path, use_latest=False)
    assert ck.missed_keys == []
