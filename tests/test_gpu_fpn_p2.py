"""The four-level pyramid p2..p5 on the GPU: the RoI gather and its level map, the fused DynamicConv gather, the FPN's stride-4 level
in both backbones and both precisions, sub-batch chains and workspace growth, the refusals of the C ABI, one head pass and the detector
end to end.  Bounds are those of the existing test of the same kernel (named in each test): they were set against the oracle for that
arithmetic and the fourth level adds none.  Invariant used throughout: the FPN's top-down pass only flows downwards, so p3 / p4 / p5 of
a four-level model equal those of the three-level model with the same tensors bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import backbone_r101, detector as odet, head as ohead, roi_align as oroi, schedule as osch  # noqa: E402
from test_gpu_kernels import check, h16  # noqa: E402
from test_gpu_f32 import nhwc  # noqa: E402

import _p2_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


def _maps(dv, feats, dtype):
    """NCHW fp32 -> the engine's NHWC maps of `dtype`"""
    return [nhwc(f) for f in feats] if dtype == "float32" else [dv.nhwc_from_nchw(f.cuda()) for f in feats]


@pytest.fixture(scope="module")
def roi_case():
    """inputs of the RoIAlign / fused-gather tests and the oracle's tiles on them, computed once"""
    n, M, H, W = 2, 96, 160, 256
    g, feats, boxes = R.maps_and_boxes(4, n, M, H, W)
    counts = R.level_counts(boxes)
    assert counts == [75, 64, 43, 10] and min(counts) >= 10, counts          # every level is read
    boxes = R.with_edge_boxes(boxes, H, W)
    f16 = [h16(f) for f in feats]
    return dict(n=n, M=M, H=H, W=W, g=g, feats=feats, feats16=f16, boxes=boxes,
                ref32=oroi.roi_pooler(feats, boxes, 7, R.SCALES4, 2), ref16=oroi.roi_pooler(f16, boxes, 7, R.SCALES4, 2))


# ---- 1. RoIAlign over four levels ---------------------------------------------------------------------------------------------------
def test_roialign_four_levels_f16(dv, roi_case):
    """bounds of test_gpu_kernels.py::test_roialign_multilevel"""
    c = roi_case
    n, M = c["n"], c["M"]
    roi, mean = dv.roialign(_maps(dv, c["feats16"], "float16"), c["boxes"].cuda(), c["H"], c["W"], want_mean=True)
    check("p2.roialign", roi.float().view(n * M, 7, 7, 256).permute(0, 3, 1, 2), c["ref16"], 2e-3, 2e-3)
    check("p2.roialign_mean", mean, c["ref16"].view(n * M, 256, -1).mean(-1), 1e-3, 1e-3)


def test_roialign_four_levels_f32(dv, roi_case):
    """bounds of test_gpu_f32.py::test_f32_roialign"""
    c = roi_case
    n, M = c["n"], c["M"]
    roi, mean = dv.roialign_f32(_maps(dv, c["feats"], "float32"), c["boxes"].cuda(), c["H"], c["W"], want_mean=True)
    check("p2.f32_roialign.tiles", roi.view(n * M, 49, 256).permute(0, 2, 1), c["ref32"].reshape(n * M, 256, 49), 1e-5, 1e-5)
    check("p2.f32_roialign.mean", mean, c["ref32"].reshape(n * M, 256, 49).mean(-1), 1e-5, 1e-5)


def test_roialign_refuses_other_pyramids(dv, roi_case):
    from diffusionvid_amd._lib import DvidError
    c = roi_case
    maps = _maps(dv, c["feats16"], "float16")
    with pytest.raises(DvidError):
        dv.roialign(maps[:2], c["boxes"].cuda(), c["H"], c["W"])
    with pytest.raises(DvidError):          # four maps whose finest one is at stride 8
        dv.roialign(maps[1:] + maps[3:], c["boxes"].cuda(), c["H"], c["W"])
    with pytest.raises(DvidError):          # three maps starting at stride 4
        dv.roialign(maps[:3], c["boxes"].cuda(), c["H"], c["W"])


# ---- 2. the level map, known answers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_level_map_known_answers_four_levels(dv, dtype):
    """closed-form tiles on affine maps with a different plane per level (tests/_p2_ref.py), tolerances of
    test_known_answers.py::test_roialign_v2_affine_known_answers_gpu: one fp16 rounding of the stored tile / fp32 2e-5"""
    n = 2
    want = R.ka_closed_form(n)
    feats = [f.permute(0, 2, 3, 1).contiguous().cuda() for f in R.ka_pyramid(n)]
    if dtype == "float16":
        roi = dv.roialign([f.half() for f in feats], R.ka_boxes(n).cuda(), R.KA_IMG, R.KA_IMG)
        tol = 1.5e-3
    else:
        roi = dv.roialign_f32(feats, R.ka_boxes(n).cuda(), R.KA_IMG, R.KA_IMG)
        tol = 2e-5
    K = len(R.KA_BOXES)
    got = roi.float().view(n * K, 7, 7, 256).permute(0, 3, 1, 2).double().cpu().numpy()
    for j in range(n * K):
        e = np.abs(got[j] - want[j]).max() / max(1.0, np.abs(want[j]).max())
        assert e <= tol, f"{R.KA_BOXES[j % K][0]} (frame {j // K}): kernel differs from the closed form by {e:.3e} (relative)"


# ---- 3. the fused gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", [False, True])
def test_roi_fused_dynconv_bit_identical_four_levels(dv, roi_case, cond):
    """test_gpu_kernels.py::test_roi_fused_dynconv_bit_identical over p2..p5: the gather inside the DynamicConv launch (roi_fuse 1)
    against RoIAlign followed by DynamicConv (roi_fuse 0), every output of the head pass bit for bit"""
    from diffusionvid_amd.utils import synthetic
    c = roi_case
    n, M, H, W = c["n"], c["M"], c["H"], c["W"]
    sd = synthetic.make_head_state_dict(0)
    g = torch.Generator().manual_seed(21)
    pro = torch.randn(n * M, 256, generator=g)
    cnd = torch.randn(n * M, 256, generator=g) if cond else None
    fd = _maps(dv, [f * 0.5 for f in c["feats16"]], "float16")
    t = torch.tensor([999, 499], dtype=torch.long)
    outs = {}
    for mode in (0, 1):
        dv.set_option("roi_fuse", mode)
        try:
            model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
            model.reserve(n, H, W, M)
            outs[mode] = tuple(x.clone() for x in model.rcnn_head(0 if cond else 1, fd, H, W, c["boxes"].cuda(), pro.cuda(), t,
                                                                  cond=None if cnd is None else cnd.cuda()))
            model.close()
        finally:
            dv.reset_options()
    for a, b, name in zip(outs[0], outs[1], ("logits", "boxes", "obj_features")):
        assert torch.isfinite(a).all() and torch.equal(a, b), f"{name}: fused and unfused head passes differ, max |d| {(a.float() - b.float()).abs().max().item():.3e}"


# ---- 4. three-level results are unchanged -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_three_level_entry_points_equal_levels_form(dv, roi_case, dtype):
    """the same three maps through dvid_roialign_v2_multilevel[_f32] and dvid_roialign_v2_levels[_f32] with n_levels 3, and through
    dvid_rcnn_head / dvid_rcnn_head_levels on a head-only model: bit-identical"""
    from diffusionvid_amd._lib import call, ptr, stream_ptr
    from diffusionvid_amd.utils import synthetic
    c = roi_case
    n, M, H, W = c["n"], c["M"], c["H"], c["W"]
    f32 = dtype == "float32"
    fd = _maps(dv, [f * 0.5 for f in (c["feats"] if f32 else c["feats16"])[1:]], dtype)
    boxes = c["boxes"].cuda()
    sfx = "_f32" if f32 else ""
    lv = (C.c_void_p * 3)(*[ptr(f) for f in fd])

    def tiles():
        return torch.full((n * M, 49, 256), float("nan"), dtype=fd[0].dtype, device="cuda"), torch.full((n * M, 256), float("nan"), device="cuda")
    r_old, m_old = tiles()
    r_new, m_new = tiles()
    call("dvid_roialign_v2_multilevel" + sfx, ptr(fd[0]), ptr(fd[1]), ptr(fd[2]), n, H, W, 256, ptr(boxes), M, ptr(r_old), ptr(m_old), stream_ptr())
    call("dvid_roialign_v2_levels" + sfx, lv, 3, n, H, W, 256, ptr(boxes), M, ptr(r_new), ptr(m_new), stream_ptr())
    assert torch.isfinite(r_old.float()).all() and torch.equal(r_old, r_new) and torch.equal(m_old, m_new)

    model = dv.Model(synthetic.make_head_state_dict(0), res_blocks=(0, 0, 0, 0), precision=dtype)
    model.reserve(n, H, W, M)
    t = torch.tensor([999, 499], dtype=torch.int64)
    tp = C.cast(t.data_ptr(), C.POINTER(C.c_int64))
    g = torch.Generator().manual_seed(22)
    pro = torch.randn(n * M, 256, generator=g).cuda()
    outs = []
    for form in ("three", "levels"):
        lo, bo, ob = torch.empty(n, M, model.num_classes, device="cuda"), torch.empty(n, M, 4, device="cuda"), torch.empty(n * M, 256, device="cuda")
        args = (n, H, W, M, ptr(boxes), ptr(pro), tp, None, ptr(lo), ptr(bo), ptr(ob), None, stream_ptr())
        if form == "three":
            call("dvid_rcnn_head", model.handle, 1, 0, ptr(fd[0]), ptr(fd[1]), ptr(fd[2]), *args)
        else:
            call("dvid_rcnn_head_levels", model.handle, 1, 0, lv, 3, *args)
        outs.append((lo, bo, ob))
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    model.close()


# ---- 5. ResNet ----------------------------------------------------------------------------------------------------------------------
def _drop_level2(sd):
    return {k: v for k, v in sd.items() if k not in R.LEVEL2_SWIN}


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_backbone_small_p2(dv, dtype):
    """test_gpu_kernels.py::test_backbone_small (3e-2 / 3e-2) and test_gpu_f32.py::test_f32_backbone_small (2e-4 / 2e-4) with the
    stride-4 level: every level against the oracle's four-level FPN, p3 / p4 / p5 bit-identical to the three-level model's, and in
    fp16 the fused and the layer-by-layer form of res2's last block hand the same c2 to the FPN"""
    from diffusionvid_amd import _lib
    from diffusionvid_amd.utils import synthetic
    lib = _lib.load()
    blocks = (1, 2, 2, 1)
    sd = synthetic.make_state_dict(0, blocks=blocks, fpn_levels=(2, 3, 4, 5))
    g = torch.Generator().manual_seed(14)
    imgs = torch.rand(2, 3, 128, 192, generator=g)
    ref = backbone_r101.fpn(backbone_r101.resnet_bottom_up(backbone_r101.normalizer(imgs, R.MEAN, R.STD), sd, "backbone.bottom_up.", blocks),
                            sd, "backbone.", in_features=R.RES4)
    tol = 2e-4 if dtype == "float32" else 3e-2
    model = dv.Model(sd, res_blocks=blocks, precision=dtype)
    assert model.fpn_levels == 4
    model.reserve(2, 128, 192, 300)
    four = model.backbone(imgs.cuda())
    assert len(four) == 4 and four[0].shape == (2, 32, 48, 256) and four[0].dtype == model.feat_dtype
    for name, got in zip(("p2", "p3", "p4", "p5"), four):
        check(f"backbone_small_p2[{dtype}].{name}", dv.nchw_from_nhwc(got), ref[name], tol, tol)
    frames = model.backbone_frames([imgs[i:i + 1].cuda() for i in range(2)])          # the pointer-table entry point gives the same maps
    assert all(torch.equal(a, b) for a, b in zip(frames, four))
    if dtype == "float16":
        try:
            _lib.check(lib.dvid_igemm_set_conv3x3(0), "set_conv3x3")          # (both runs: see test_backbone_bottleneck_fusion_bit_identical)
            _lib.check(lib.dvid_igemm_set_bottleneck_fusion(2), "set_bottleneck_fusion")
            fused = [t.clone() for t in model.backbone(imgs.cuda())]
            _lib.check(lib.dvid_igemm_set_bottleneck_fusion(0), "set_bottleneck_fusion")
            plain = [t.clone() for t in model.backbone(imgs.cuda())]
        finally:
            lib.dvid_igemm_set_bottleneck_fusion(-1)
            lib.dvid_igemm_set_conv3x3(-1)
        for name, a, b in zip(("p2", "p3", "p4", "p5"), fused, plain):
            assert torch.equal(a, b), f"{name}: fused and layer-by-layer res2 / res3 differ"
        check("backbone_small_p2[fused].p2", dv.nchw_from_nhwc(fused[0]), ref["p2"], tol, tol)
    model.close()
    three = dv.Model(_drop_level2(sd), res_blocks=blocks, precision=dtype)
    assert three.fpn_levels == 3
    three.reserve(2, 128, 192, 300)
    for name, a, b in zip(("p3", "p4", "p5"), three.backbone(imgs.cuda()), four[1:]):
        assert torch.equal(a, b), f"{name} of the four-level model differs from the three-level model's"
    three.close()


# ---- 6. chains and workspace growth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_chains_and_workspace_growth_p2(dv, dtype):
    """32 frames of 64 x 96 are split into two sub-batch chains (from 16 frames per chain on): the c2 / lateral slices of the second
    chain start at frame 16.  All four maps equal the single-chain run's; a larger second call moves the workspace, is counted, and
    gives what a fresh model gives."""
    from diffusionvid_amd.utils import synthetic
    blocks = (1, 1, 1, 1)
    sd = synthetic.make_state_dict(2, blocks=blocks, fpn_levels=(2, 3, 4, 5))
    g = torch.Generator().manual_seed(31)
    imgs = torch.rand(32, 3, 64, 96, generator=g).cuda()
    big = torch.rand(3, 3, 96, 128, generator=g).cuda()
    model = dv.Model(sd, res_blocks=blocks, precision=dtype)
    model.reserve(32, 64, 96, 100)
    model.set_chains(1)
    one = [t.clone() for t in model.backbone(imgs)]
    model.set_chains(2)
    two = [t.clone() for t in model.backbone(imgs)]
    for name, a, b in zip(("p2", "p3", "p4", "p5"), one, two):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), f"{name}: two chains differ from one"
    gen = model.workspace_generation()
    model.reserve(32, 96, 128, 100)
    assert model.workspace_generation() > gen
    grown = [t.clone() for t in model.backbone(big)]
    again = [t.clone() for t in model.backbone(imgs)]          # the first size still runs in the grown workspace
    model.close()
    fresh = dv.Model(sd, res_blocks=blocks, precision=dtype)
    fresh.reserve(3, 96, 128, 100)
    for name, a, b in zip(("p2", "p3", "p4", "p5"), grown, fresh.backbone(big)):
        assert torch.equal(a, b), f"{name}: the grown workspace gives another result than a fresh model"
    fresh.close()
    for a, b in zip(again, two):
        assert torch.equal(a, b)


# ---- 7. Swin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_backbone_swin_small_p2(dv, dtype):
    """test_backbone_swin_small / test_f32_backbone_swin_small at their 160 x 224 size with out_indices (0, 1, 2, 3): stage 0's norm0
    feeds lateral2 (embed_dim -> 256).  Bounds 3e-2 (fp16) / 2e-4 (fp32); p3..p5 bit-identical to the three-level model's."""
    from diffusionvid_amd.utils import synthetic
    from oracle import swin as oswin
    sw = dict(embed_dim=64, depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), window=7)
    sd = synthetic.make_state_dict(0, swin=sw, fpn_levels=(2, 3, 4, 5))
    g = torch.Generator().manual_seed(15)
    imgs = torch.rand(2, 3, 160, 224, generator=g)
    body = oswin.swin_body(backbone_r101.normalizer(imgs, R.MEAN, R.STD), sd, "backbone.bottom_up.", embed_dim=64, depths=sw["depths"],
                           num_heads=sw["heads"], out_indices=(0, 1, 2, 3))
    ref = backbone_r101.fpn({f"res{i + 2}": body[f"swin{i}"] for i in range(4)}, sd, "backbone.", in_features=R.RES4)
    kw = dict(res_blocks=(0, 0, 0, 0), backbone="swin", swin_embed_dim=64, swin_depths=sw["depths"], swin_heads=sw["heads"], precision=dtype)
    tol = 2e-4 if dtype == "float32" else 3e-2
    model = dv.Model(sd, **kw)
    model.reserve(2, 160, 224, 300)
    four = model.backbone(imgs.cuda())
    assert len(four) == 4 and four[0].shape == (2, 40, 56, 256)
    for name, got in zip(("p2", "p3", "p4", "p5"), four):
        check(f"backbone_swin_small_p2[{dtype}].{name}", dv.nchw_from_nhwc(got), ref[name], tol, tol)
    model.close()
    three = dv.Model(_drop_level2(sd), **kw)
    three.reserve(2, 160, 224, 300)
    for name, a, b in zip(("p3", "p4", "p5"), three.backbone(imgs.cuda()), four[1:]):
        assert torch.equal(a, b), f"{name} of the four-level model differs from the three-level model's"
    three.close()


# ---- 8. refusals through the C ABI --------------------------------------------------------------------------------------------------
def test_abi_refuses_the_wrong_level_count(dv):
    """a model with the p2 level: the three-pointer backbone entry answers DVID_ERR_STATE (4) naming the _levels form, n_levels 3
    answers DVID_ERR_ARG (1); a three-level model answers n_levels 4 the same way.  Nothing is written to the guard-banded outputs."""
    from diffusionvid_amd import _lib
    from diffusionvid_amd._lib import ptr, stream_ptr
    from diffusionvid_amd.utils import synthetic
    lib = _lib.load()
    blocks = (1, 1, 1, 1)
    sd = synthetic.make_state_dict(0, blocks=blocks, fpn_levels=(2, 3, 4, 5))
    h, w = 64, 96
    img = torch.rand(1, 3, h, w).cuda()
    table = (C.c_void_p * 1)(img.data_ptr())
    guard = 4096
    SENTINEL = 16384.0          # exact in fp16, far outside the maps' values

    def outputs():          # one buffer per level, each between two bands of a sentinel
        return [torch.full((guard + (h >> s) * (w >> s) * 256 + guard,), SENTINEL, dtype=torch.float16, device="cuda") for s in (2, 3, 4, 5)]

    def untouched(bufs):
        torch.cuda.synchronize()
        return all(bool((b == SENTINEL).all()) for b in bufs)
    model = dv.Model(sd, res_blocks=blocks)
    model.reserve(1, h, w, 100)
    bufs = outputs()
    p = [b.data_ptr() + guard * 2 for b in bufs]
    rc = lib.dvid_backbone_resnet_fpn_frames(model.handle, table, 1, h, w, p[1], p[2], p[3], stream_ptr())
    assert rc == 4 and b"_levels" in lib.dvid_last_error() and untouched(bufs)
    rc = lib.dvid_backbone_resnet_fpn(model.handle, ptr(img), 1, h, w, p[1], p[2], p[3], stream_ptr())
    assert rc == 4 and untouched(bufs)
    rc = lib.dvid_backbone_resnet_fpn_levels_frames(model.handle, table, 1, h, w, (C.c_void_p * 3)(*p[1:]), 3, stream_ptr())
    assert rc == 1 and untouched(bufs)
    rc = lib.dvid_backbone_resnet_fpn_levels_frames(model.handle, table, 1, h, w, (C.c_void_p * 5)(*(p + p[:1])), 5, stream_ptr())
    assert rc == 1 and untouched(bufs)
    # the head of a model with a four-level backbone refuses three maps
    t = torch.tensor([999], dtype=torch.int64)
    outs = [torch.full((100 * k,), SENTINEL, device="cuda") for k in (model.num_classes, 4, 256)]
    boxes = torch.tensor([[[4.0, 4.0, 40.0, 40.0]] * 100], device="cuda")
    rc = lib.dvid_rcnn_head(model.handle, 0, 0, p[1], p[2], p[3], 1, h, w, 100, ptr(boxes), None, C.cast(t.data_ptr(), C.POINTER(C.c_int64)), None,
                            ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), None, stream_ptr())
    assert rc == 4 and b"dvid_rcnn_head_levels" in lib.dvid_last_error() and untouched(outs)
    # ... and the four-map call on the same arguments is accepted and writes all four maps
    rc = lib.dvid_backbone_resnet_fpn_levels_frames(model.handle, table, 1, h, w, (C.c_void_p * 4)(*p), 4, stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:guard] == SENTINEL).all()) and bool((b[-guard:] == SENTINEL).all()) and bool((b[guard:-guard] != SENTINEL).all())
    model.close()
    three = dv.Model(_drop_level2(sd), res_blocks=blocks)
    three.reserve(1, h, w, 100)
    bufs = outputs()
    p = [b.data_ptr() + guard * 2 for b in bufs]
    rc = lib.dvid_backbone_resnet_fpn_levels_frames(three.handle, table, 1, h, w, (C.c_void_p * 4)(*p), 4, stream_ptr())
    assert rc == 1 and untouched(bufs)
    three.close()


def test_finalize_names_the_first_missing_level2_tensor(dv):
    from diffusionvid_amd._lib import DvidError
    from diffusionvid_amd.utils import synthetic
    blocks = (1, 1, 1, 1)
    sd = synthetic.make_state_dict(0, blocks=blocks, fpn_levels=(2, 3, 4, 5))
    for missing in ("backbone.fpn_lateral2.bias", "backbone.fpn_output2.weight", "backbone.fpn_output2.bias"):
        with pytest.raises(DvidError) as e:
            dv.Model({k: v for k, v in sd.items() if k != missing}, res_blocks=blocks)
        assert missing in str(e.value) and "code 4" in str(e.value), str(e.value)
    sw = dict(embed_dim=64, depths=(1, 1, 1, 1), heads=(2, 4, 8, 16), window=7)          # (the linear layers take multiples of 64)
    ssd = synthetic.make_state_dict(0, swin=sw, fpn_levels=(2, 3, 4, 5))
    with pytest.raises(DvidError) as e:
        dv.Model({k: v for k, v in ssd.items() if k != "backbone.bottom_up.norm0.weight"}, res_blocks=(0, 0, 0, 0), backbone="swin", swin_embed_dim=64,
                 swin_depths=sw["depths"], swin_heads=sw["heads"])
    assert "backbone.bottom_up.norm0.weight" in str(e.value)


# ---- 9. one head pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_rcnn_head_four_levels(dv, dtype):
    """test_gpu_kernels.py::test_rcnn_head (fp16: 2e-2, boxes 3e-2 of their size) / test_gpu_f32.py::test_f32_rcnn_head (2e-4, 3e-4) at
    their shapes, over p2..p5 with the boxes of the four-level recipe (260 / 204 / 106 / 30 per level)"""
    from diffusionvid_amd.utils import synthetic
    f32 = dtype == "float32"
    n, M, H, W = 2, 300, 160, 256
    g, feats, boxes = R.maps_and_boxes(4, n, M, H, W)
    assert min(R.level_counts(boxes)) >= 10
    boxes = R.with_edge_boxes(boxes, H, W)
    boxes[0, 0] = torch.tensor([10.0, 10.0, 14.0, 13.0])
    feats = [(f if f32 else h16(f)) * 0.5 for f in feats]
    sd = synthetic.make_head_state_dict(0)
    sdo = {k: v.float() for k, v in sd.items()} if f32 else {k: (h16(v) if v.dim() > 1 else v) for k, v in sd.items()}
    cfg = ohead.HeadCfg(scales=R.SCALES4)
    t = torch.tensor([999, 499], dtype=torch.long)
    time = osch.time_mlp(sdo if f32 else sd, "head.", t, 256)
    pro = torch.randn(1, n * M, 256, generator=g)
    cl, bx, of = ohead.rcnn_head(sdo, "head.head_series.1", feats, boxes, pro, time, cfg)
    cl0, bx0, of0 = ohead.rcnn_head(sdo, "head.head_series.0", feats, boxes, None, time, cfg)
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0), precision=dtype)
    model.reserve(n, H, W, M)
    fd = _maps(dv, feats, dtype)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    gl, gb, go = model.rcnn_head(1, fd, H, W, boxes.cuda(), pro[0].cuda(), t, bad_flag=flag)
    tol, btol = (2e-4, 3e-4) if f32 else (2e-2, 3e-2)
    check(f"p2.rcnn_head[{dtype}].obj_features", go, of[0], tol, tol)
    check(f"p2.rcnn_head[{dtype}].logits", gl, cl, tol, tol)
    bw = (boxes[..., 2:] - boxes[..., :2]).clamp(min=1.0).max(-1).values
    err = ((gb.cpu() - bx).abs().max(-1).values / bw).max().item()
    print(f"p2.rcnn_head[{dtype}].boxes rel-to-size err max={err:.3e}")
    assert err < btol and int(flag.item()) == 0
    gl0, gb0, go0 = model.rcnn_head(0, fd, H, W, boxes.cuda(), None, t)          # first head: the mean of the RoI tiles as features
    check(f"p2.rcnn_head[{dtype}].first.obj_features", go0, of0[0], tol, tol)
    model.close()


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------------
P2_OPTS = ["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"], "MODEL.FPN.IN_FEATURES", ["res2", "res3", "res4", "res5"]]


def _oracle_p2(sd, blocks, sample_step, noise_fn):
    ocfg = odet.DetCfg(sample_step=sample_step, blocks=blocks, in_features=("p2", "p3", "p4", "p5"), head=ohead.HeadCfg(scales=R.SCALES4))
    ocfg.head.sampling_timesteps = sample_step

    def backbone_fn(x):
        return backbone_r101.fpn(backbone_r101.resnet_bottom_up(x, sd, "backbone.bottom_up.", blocks), sd, "backbone.", in_features=R.RES4)
    return ocfg, odet.OracleDiffusionDet(sd, ocfg, noise_fn, backbone_fn=backbone_fn)


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_video_e2e_p2(dtype):
    """test_gpu_e2e.py::test_video_e2e (sample step 1, host noise) with IN_FEATURES [p2..p5]: its configuration (blocks (1, 1, 2, 1), 8
    frames of 250 x 380), its staged comparison and its gates -- backbone features per level (now four), the extraction pass, the final
    stage with the oracle's memory, the detections; float32 with that test's 10 x tighter bounds."""
    import test_gpu_e2e as E
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    blocks = (1, 1, 2, 1)
    cfg, model = E._build(1, blocks, extra=P2_OPTS, dtype=dtype)
    assert model.fpn_levels == (2, 3, 4, 5)
    f32 = dtype == "float32"
    sb = dict(b_logit=0.008, b_feat=0.008, b_px=0.05, b_rel=0.001) if f32 else {}
    L, H0, W0 = 8, 250, 380
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg, oracle = _oracle_p2(sd, blocks, 1, synthetic.noise_fn)
    model.noise_fn = synthetic.noise_fn
    model.debug_taps = {}
    images, oitem, ids = E._oracle_items(ds, 0)
    with torch.no_grad():
        ref_out = oracle.forward(oitem)
        got_out = model(images)
    assert len(got_out) == len(ref_out) == L
    tag = f"[p2 x1{' float32' if f32 else ''}]"
    # backbone features: _feature_check's measures and bounds, over four levels
    bound_max, bound_rms = (2e-3, 1e-4) if f32 else (0.06, 0.012)
    assert all(len(e[3]) == 4 for e in model.debug_taps["extract"])
    for lvl, name in enumerate(("p2", "p3", "p4", "p5")):
        gq = torch.cat([e[3][lvl].float().cpu() for e in model.debug_taps["extract"]]).permute(0, 3, 1, 2)
        o = oracle.taps["feats"][name]
        assert gq.shape == o.shape, (gq.shape, o.shape)
        rms = o.pow(2).mean().sqrt().item()
        e_max, e_rms = (gq - o).abs().max().item() / rms, (gq - o).pow(2).mean().sqrt().item() / rms
        gain = (gq * o).sum().item() / o.pow(2).sum().item()
        print(f"{tag} {name}: max |err| / rms = {e_max:.3e}, rms err / rms = {e_rms:.3e}, scale = {gain:.5f}")
        assert e_max <= bound_max and e_rms <= bound_rms and abs(gain - 1) <= 2e-3, (name, e_max, e_rms, gain)
    ocl, obx, opf = oracle.taps["extract"]
    gcl = torch.cat([e[0] for e in model.debug_taps["extract"]]).cpu()
    gbx = torch.cat([e[1] for e in model.debug_taps["extract"]]).cpu()
    gpf = torch.cat([e[2] for e in model.debug_taps["extract"]]).cpu().view(-1, 300, 256)
    lv = oroi.assign_boxes_to_levels(obx.reshape(-1, 4), 2, 5)
    print(f"{tag} boxes of the last extraction head per level: {torch.bincount(lv, minlength=4).tolist()}")
    E._stage_check(f"{tag} extraction", gpf, opf, gcl, ocl, gbx, obx, **sb)
    model.debug_taps = {}
    sb.pop("b_feat", None)
    E._final_stage_vs_oracle(model, oracle, L, W0, H0, 1, tag, **sb)
    rates = [E._match_rate(r, g) for r, g in zip(ref_out, got_out)]
    print(f"{tag} detections: kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]}; match rates {['%.2f' % r for r in rates]}")
    assert min(rates) >= 0.9
    ap = E._ap50_vs_oracle(ref_out, got_out, (W0, H0))
    print(f"{tag} AP50 of the GPU detections with the oracle's detections as ground truth: {ap:.4f}")
    assert ap >= 0.95


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_call_graph_replay_is_bit_identical_p2(dtype):
    """test_gpu_e2e.py::test_call_graph_replay_is_bit_identical over p2..p5: one video of five full batches, so the steady call is
    reached, captured and replayed; the captured launches carry the fourth map (c2 and the stride-4 lateral inside the workspace, p2
    among the capture's outputs).  Every detection bit for bit against kernel-by-kernel launches."""
    import test_gpu_e2e as E
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    lens = [43]
    outs, replays = {}, {}
    for graphs in (False, True):
        cfg, model = E._build(1, (1, 1, 2, 1), "trained_like", extra=P2_OPTS, dtype=dtype)
        model.noise_fn = synthetic.DeviceNoise()
        model.use_call_graph = graphs
        ds = SyntheticVIDDataset(lens, cfg, height=250, width=380, device="cuda", smooth=True)
        res = []
        with torch.no_grad():
            for idx in range(len(ds)):
                res += model(ds[idx][0])
        assert len(res) == sum(lens)
        outs[graphs], replays[graphs] = [r.to(torch.device("cpu")) for r in res], model.graph_replays
        del model, ds
        torch.cuda.empty_cache()
    assert replays[False] == 0 and replays[True] >= 3, replays
    for f, (a, b) in enumerate(zip(outs[False], outs[True])):
        assert len(a) == len(b) and len(a) > 0, f
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores")) and \
            torch.equal(a.get_field("labels"), b.get_field("labels")), f"frame {f} differs between graph replay and kernel-by-kernel launches"
