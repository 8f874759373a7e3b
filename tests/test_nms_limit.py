"""The candidate limit of the NMS (4096 per frame = max(1, SAMPLE_STEP - 1) * NUM_PROPOSALS) and the scratch rule of
dvid_postproc_topk_nms: host logic, no GPU."""
import os
import re

import pytest

from conftest import ROOT


def _cfg(sample_step, num_proposals):
    from diffusionvid_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"),
                  ["MODEL.DiffusionDet.SAMPLE_STEP", sample_step, "MODEL.DiffusionDet.NUM_PROPOSALS", num_proposals],
                  os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    return cfg


def test_a_configuration_beyond_the_limit_fails_at_construction():
    """8 steps x 700 boxes = 4900 candidates per frame: refused when the model is built, not in its first call; the message names both
    keys and the limit.  8 x 585 = 4095 and 1 x 4096 are built."""
    from diffusionvid_amd.modeling.detector import build_detection_model
    with pytest.raises(NotImplementedError, match=r"SAMPLE_STEP 8.*NUM_PROPOSALS 700.*4900.*4096"):
        build_detection_model(_cfg(8, 700))
    with pytest.raises(NotImplementedError, match="4096"):
        build_detection_model(_cfg(1, 4097))
    assert build_detection_model(_cfg(8, 585)).num_proposals == 585
    assert build_detection_model(_cfg(1, 4096)).num_proposals == 4096


def test_limit_is_one_number():
    from diffusionvid_amd import ops
    header = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    assert int(re.search(r"#define DVID_NMS_MAX_CANDIDATES (\d+)", header).group(1)) == ops.NMS_MAX_CANDIDATES == 4096


def test_postproc_scratch_rule():
    """dvid_postproc_scratch_bytes: the candidate lists alone (24 bytes per candidate) where the single-workgroup NMS runs -- up to 997
    candidates per frame -- and the sorted boxes plus the bit matrix of one chunk of frames on top where the tiled form does; a
    chunk's matrices stay within 64 MiB however many frames the call has."""
    from diffusionvid_amd import ops
    for S, n, M in ((1, 8, 300), (3, 304, 300), (1, 8, 997), (3, 2, 332)):
        assert ops.postproc_scratch_bytes(S, n, M) == n * S * M * 24
    matrix = lambda N: N * ((N + 63) // 64) * 8          # noqa: E731
    for S, n, M in ((1, 2, 1000), (1, 2, 998), (7, 2, 300), (5, 2, 205), (4, 2, 1024)):
        N = S * M
        assert ops.postproc_scratch_bytes(S, n, M) == n * N * 24 + 256 + n * (N * 24 + matrix(N))
    # 304 frames at x8: 121 frames of 2100 candidates per chunk (64 MiB / 554400 B), not 304
    assert ops.postproc_scratch_bytes(7, 304, 300) == 304 * 2100 * 24 + 256 + 121 * (2100 * 24 + matrix(2100))
    assert ops.postproc_scratch_bytes(4, 304, 1024) == 304 * 4096 * 24 + 256 + 32 * (4096 * 24 + matrix(4096))
    assert ops.postproc_scratch_bytes(17, 1, 241) == 17 * 241 * 24          # refused by the call itself; no tiled part to size
