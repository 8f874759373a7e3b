"""The Swin backbone with 12x12 windows (MODEL.SWIN.SIZE B-22k-384 / L-22k-384) through the model: the small backbone of
test_backbone_swin_small / test_f32_backbone_swin_small with window 12 against oracle.swin.backbone_swin_fpn(window=12) at those
tests' bounds, the refusal of a window that is not built, and one video end to end (test_video_e2e_swin with window 12)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import backbone_r101  # noqa: E402
from oracle import detector as odet  # noqa: E402
from oracle import swin as oswin  # noqa: E402
from test_gpu_kernels import check  # noqa: E402

SW12 = dict(embed_dim=64, depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), window=12)


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


@pytest.mark.parametrize("precision,bound", [("float16", 3e-2), ("float32", 2e-4)])
@pytest.mark.parametrize("size", [(160, 224), (160, 192)], ids=["160x224", "160x192"])
def test_backbone_swin_small_window_12(dv, size, precision, bound):
    """Swin-Transformer + FPN at reduced widths / depths with 12x12 windows (shift 6) against the CPU oracle; fp16 path 3e-2 / 3e-2
    (test_backbone_swin_small's bound), DTYPE float32 2e-4 / 2e-4 (test_f32_backbone_swin_small's).  160 x 224: token maps 40x56 ->
    20x28 -> 10x14 -> 5x7, padded to 48x60, 24x36, 12x24, 12x12; 160 x 192: 40x48 -> 20x24 -> 10x12 -> 5x6, padded to 48x48, 24x24,
    12x12, 12x12.  Every stage map pads on at least one axis, the last two are single windows per image (or two), smaller than a window."""
    from diffusionvid_amd.utils import synthetic
    sd = synthetic.make_state_dict(0, swin=SW12)
    g = torch.Generator().manual_seed(15)
    imgs = torch.rand(2, 3, size[0], size[1], generator=g)
    mean, std = (123.675, 116.280, 103.530), (58.395, 57.120, 57.375)
    ref = oswin.backbone_swin_fpn(backbone_r101.normalizer(imgs, mean, std), sd, "backbone.", embed_dim=64, depths=SW12["depths"],
                                  num_heads=SW12["heads"], window=12)
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0), backbone="swin", swin_embed_dim=64, swin_depths=SW12["depths"],
                     swin_heads=SW12["heads"], swin_window=12, precision=precision)
    model.reserve(2, size[0], size[1], 300)
    p3, p4, p5 = model.backbone(imgs.cuda())
    assert p3.dtype == (torch.float32 if precision == "float32" else torch.float16)
    for name, got in (("p3", p3), ("p4", p4), ("p5", p5)):
        check(f"backbone_swin_small_w12[{precision},{size[0]}x{size[1]}].{name}", dv.nchw_from_nhwc(got), ref[name], bound, bound)
    model.close()


def test_model_refuses_a_window_that_is_not_built(dv):
    """swin_window 8 still fails at finalisation, and the message names the value"""
    from diffusionvid_amd._lib import DvidError
    from diffusionvid_amd.utils import synthetic
    sw = dict(SW12, window=8)
    sd = synthetic.make_state_dict(0, swin=sw)
    with pytest.raises(DvidError, match=r"code 3\b.*window size 8"):
        dv.Model(sd, res_blocks=(0, 0, 0, 0), backbone="swin", swin_embed_dim=64, swin_depths=sw["depths"], swin_heads=sw["heads"],
                 swin_window=8)


def test_model_refuses_a_window_7_table_for_window_12(dv):
    """the bias-table shape check follows the window: [169, heads] tables are refused by a window-12 model"""
    from diffusionvid_amd._lib import DvidError
    from diffusionvid_amd.utils import synthetic
    sd = synthetic.make_state_dict(0, swin=dict(SW12, window=7))
    with pytest.raises(DvidError, match="bad bias table shape"):
        dv.Model(sd, res_blocks=(0, 0, 0, 0), backbone="swin", swin_embed_dim=64, swin_depths=SW12["depths"], swin_heads=SW12["heads"],
                 swin_window=12)


def test_video_e2e_swin_window_12():
    """test_gpu_e2e.test_video_e2e_swin with CONFIG_OVERRIDE window 12: extraction pass, memory and detections vs the CPU oracle under
    the same gates."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    from test_gpu_e2e import _match_rate, _oracle_items, _stage_check
    sw = SW12
    cfg = get_cfg("configs/vid_Swin_B_DiffusionVID.yaml", ["DTYPE", "float16"], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.SWIN.CONFIG_OVERRIDE = sw
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    L, H0, W0 = 4, 250, 380
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = odet.DetCfg(infer_batch=4, all_frame_interval=4)
    oracle = odet.OracleDiffusionDet(sd, ocfg, synthetic.noise_fn,
                                     backbone_fn=lambda x: oswin.backbone_swin_fpn(x, sd, "backbone.", embed_dim=64, depths=sw["depths"],
                                                                                   num_heads=sw["heads"], window=12))
    model.noise_fn = synthetic.noise_fn
    model.debug_taps = {}
    images, oitem, ids = _oracle_items(ds, 0)
    with torch.no_grad():
        ref_out = oracle.forward(oitem)
        got_out = model(images)
    assert len(got_out) == len(ref_out) == L and ids == [0, 1, 2, 3]
    ocl, obx, opf = oracle.taps["extract"]
    gcl = torch.cat([e[0] for e in model.debug_taps["extract"]]).cpu()
    gbx = torch.cat([e[1] for e in model.debug_taps["extract"]]).cpu()
    gpf = torch.cat([e[2] for e in model.debug_taps["extract"]]).cpu().view(-1, 300, 256)
    assert gcl.shape[0] == 28                                   # 4 local + 24 global frames in 7 splits of 4
    _stage_check("[swin window 12 x1] extraction", gpf, opf, gcl, ocl, gbx, obx)
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    print(f"[swin window 12 x1] detections kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]}; match {rates}")
    assert min(rates) >= 0.9
