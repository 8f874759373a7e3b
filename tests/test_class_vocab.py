"""The class-count limit (1 <= MODEL.DiffusionDet.NUM_CLASSES <= DVID_MAX_CLASSES = 1280: COCO 80, Objects365 365, LVIS 1203) and the
checkpoint ingest of a wide class_logits: host logic, no GPU."""
import os
import re

import pytest
import torch

from conftest import ROOT


def _default_num_classes():
    """NUM_CLASSES of the default config node (config/defaults.py: add_diffusiondet_config), the value of the DiffusionDet family"""
    from diffusionvid_amd.config import get_cfg
    return get_cfg().MODEL.DiffusionDet.NUM_CLASSES


def _model(num_classes):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), ["MODEL.DiffusionDet.NUM_CLASSES", num_classes],
                  os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    return cfg, build_detection_model(cfg)


def test_limit_is_one_number():
    from diffusionvid_amd import ops
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    mirror = open(os.path.join(ROOT, "diffusionvid_amd", "csrc", "common.h")).read()
    assert int(re.search(r"#define DVID_MAX_CLASSES (\d+)", header).group(1)) == ops.MAX_CLASSES == 1280
    assert int(re.search(r"#define DVID_MAX_CLASSES (\d+)", mirror).group(1)) == ops.MAX_CLASSES
    assert ops.MAX_CLASSES % 64 == 0 and ops.MAX_CLASSES >= 1203          # LVIS, in whole 64-row tiles of class_logits


def test_default_class_count_passes_and_a_count_beyond_the_limit_fails_at_construction():
    """The default node's 80 classes and LVIS's 1203 are built (no device is needed for that; the engine behind is created on the GPU:
    tests/test_gpu_class_vocab.py); one class more than the limit, or none, is refused when the model is built, and the message names
    the limit."""
    from diffusionvid_amd import ops
    assert _default_num_classes() == 80
    for c in (80, 1203, ops.MAX_CLASSES):
        _, model = _model(c)
        assert model.num_classes == c
        assert model.state_dict()["head.head_series.0.class_logits.weight"].shape == (c, 256)
    with pytest.raises(NotImplementedError, match=r"NUM_CLASSES 1281.*1280.*DVID_MAX_CLASSES"):
        _model(ops.MAX_CLASSES + 1)
    with pytest.raises(NotImplementedError, match=r"NUM_CLASSES 0.*1280"):
        _model(0)


def test_library_bindings_name_the_streaming_selection():
    """dvid_topk_candidates_stream is declared in the header and bound with the header's ten arguments (the library itself is checked
    against the header by test_host_logic.py)."""
    from diffusionvid_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    decl = re.search(r"int dvid_topk_candidates_stream\(([^;]*)\);", header)
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["dvid_topk_candidates_stream"][1]) == 10
    assert callable(ops.topk_candidates_stream)


@pytest.mark.parametrize("num_classes", [80, 1203])
def test_checkpoint_ingest_loads_a_wide_class_logits(tmp_path, num_classes):
    """A checkpoint under the reference's naming variations (`module.` prefix, DiffusionDet head numbering) whose class_logits is
    [80, 256] / [1203, 256] loads through DetectronCheckpointer into a model of that class count, bit for bit; into a 30-class model
    it fails (torch's strict load), it is not cut to size."""
    from diffusionvid_amd.utils.checkpoint import DetectronCheckpointer
    cfg, src = _model(num_classes)
    g = torch.Generator().manual_seed(num_classes)
    sd = {k: (torch.randn(v.shape, generator=g) if "class_logits" in k else v.clone()) for k, v in src.state_dict().items()}
    f = tmp_path / "ckpt.pth"
    torch.save({"model": {"module." + k.replace("head_series_cond.0", "head_series.3"): v for k, v in sd.items()}}, f)
    _, dst = _model(num_classes)
    DetectronCheckpointer(cfg, dst).load(str(f))
    got = dst.state_dict()
    names = [k for k in sd if "class_logits" in k]
    assert len(names) == 2 * (cfg.MODEL.DiffusionDet.NUM_HEADS + cfg.MODEL.DiffusionDet.NUM_HEADS_LOCAL)
    for k in names:
        assert got[k].shape[0] == num_classes and torch.equal(got[k], sd[k])
    cfg30, small = _model(30)
    with pytest.raises(RuntimeError, match="size mismatch"):
        DetectronCheckpointer(cfg30, small).load(str(f))
