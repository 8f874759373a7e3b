"""Per-kernel parity: HIP kernels (through the C ABI) vs the CPU oracle on identical seeded inputs.

Tolerances.  Kernels compute fp16 x fp16 -> fp32 on MFMA and store fp16 or fp32.  The oracle is fed
the SAME fp16-rounded operands in fp32, so what remains is accumulation order (fp32) and the final
fp16 store (2^-11 relative): fp16 outputs rtol 2e-3 (+ atol 2e-3 of the output RMS), fp32 outputs
rtol 1e-3/atol 1e-3 of RMS unless stated.  Index outputs (top-k / NMS keep sets / FPS picks) are
compared exactly on inputs without near-ties.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import backbone_r101, detector as odet, head as ohead, memory as omem, postproc as opost, roi_align as oroi, schedule as osch  # noqa: E402


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


REPORT = []


def _report_path():
    """reports/parity_report.txt under the repository root, the report every parity line is appended to; the directory is
    kept out of git, so it is created on first use"""
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reports")
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, "parity_report.txt")


def check(name, got, want, rtol, atol_rms):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float32)
    want = want.detach().float().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, f"{name}: shape {got.shape} vs {want.shape}"
    rms = float(np.sqrt(np.mean(want.astype(np.float64) ** 2))) + 1e-12
    err = np.abs(got - want)
    bound = atol_rms * rms + rtol * np.abs(want)
    worst = float((err / bound).max()) if err.size else 0.0
    line = f"{name}: max_abs={err.max():.3e} rms_ref={rms:.3e} worst/bound={worst:.3f} nan={int(np.isnan(got).sum())}"
    REPORT.append(line)
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")
    assert not np.isnan(got).any(), f"{name}: NaN in output"
    assert worst <= 1.0, line


def h16(x):
    return x.to(torch.float16).to(torch.float32)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [
    dict(n=2, h=20, w=28, cin=64, cout=128, k=3, stride=1, pad=1, relu=True, res=1),
    dict(n=2, h=21, w=27, cin=128, cout=64, k=3, stride=2, pad=1, relu=False, res=0),
    dict(n=3, h=16, w=24, cin=256, cout=256, k=1, stride=1, pad=0, relu=True, res=1),
    dict(n=1, h=16, w=24, cin=128, cout=512, k=1, stride=2, pad=0, relu=False, res=0),
    dict(n=2, h=38, w=64, cin=256, cout=1024, k=1, stride=1, pad=0, relu=True, res=1),   # 128x128 tiles
    dict(n=1, h=12, w=16, cin=512, cout=256, k=1, stride=1, pad=0, relu=False, res=2),   # FPN lateral + upsample add
])
def test_igemm_conv(dv, cfg):
    g = torch.Generator().manual_seed(1)
    n, h, w, cin, cout, k = cfg["n"], cfg["h"], cfg["w"], cfg["cin"], cfg["cout"], cfg["k"]
    x = h16(torch.randn(n, cin, h, w, generator=g))
    wt = h16(torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k))
    bias = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x, wt, bias, stride=cfg["stride"], padding=cfg["pad"])
    res = None
    if cfg["res"] == 1:
        res = h16(torch.randn(ref.shape, generator=g))
        ref = ref + res
    elif cfg["res"] == 2:
        res = h16(torch.randn(n, cout, ref.shape[2] // 2, ref.shape[3] // 2, generator=g))
        ref = ref + F.interpolate(res, scale_factor=2.0, mode="nearest")
    if cfg["relu"]:
        ref = F.relu(ref)
    wp, kpad = dv.pack_conv_weight(wt)
    xd = dv.nhwc_from_nchw(x.cuda())
    resd = dv.nhwc_from_nchw(res.cuda()) if res is not None else None
    out = dv.conv2d_nhwc(xd, wp.cuda(), kpad, bias.cuda(), cout, k, k, cfg["stride"], cfg["pad"], relu=cfg["relu"],
                         residual=resd, residual_mode=cfg["res"])
    check(f"igemm_conv{cfg}", dv.nchw_from_nhwc(out), ref, 2e-3, 2e-3)


def test_igemm_stem(dv):
    g = torch.Generator().manual_seed(2)
    x = h16(torch.randn(2, 3, 64, 96, generator=g))
    wt = h16(torch.randn(64, 3, 7, 7, generator=g) / math.sqrt(147))
    bias = torch.randn(64, generator=g) * 0.1
    ref = F.relu(F.conv2d(x, wt, bias, stride=2, padding=3))
    wp, kpad = dv.pack_conv_weight(wt, cin_pad=8)
    x8 = torch.zeros(2, 8, 64, 96)
    x8[:, :3] = x
    out = dv.conv2d_nhwc(dv.nhwc_from_nchw(x8.cuda()), wp.cuda(), kpad, bias.cuda(), 64, 7, 7, 2, 3, relu=True)
    check("igemm_stem", dv.nchw_from_nhwc(out), ref, 2e-3, 2e-3)


@pytest.mark.parametrize("rows,k,nout", [(600, 256, 768), (600, 256, 30), (300, 256, 4), (257, 12544, 256), (600, 2048, 256)])
def test_igemm_linear_f32(dv, rows, k, nout):
    g = torch.Generator().manual_seed(3)
    x = h16(torch.randn(rows, k, generator=g))
    wt = h16(torch.randn(nout, k, generator=g) / math.sqrt(k))
    bias = torch.randn(nout, generator=g)
    ref = F.linear(x, wt, bias)
    wp, kpad = dv.pack_conv_weight(wt)
    out = dv.linear(x.cuda().half(), wp.cuda(), kpad, bias.cuda())
    check(f"igemm_linear[{rows}x{k}->{nout}]", out, ref, 1e-3, 1e-3)


def _pyramid(g, n, H, W, c=256):
    return [h16(torch.randn(n, c, H // s, W // s, generator=g)) for s in (8, 16, 32)]


def _boxes(g, n, M, H, W):
    cxcy = torch.rand(n, M, 2, generator=g) * torch.tensor([W, H]) * 1.2 - torch.tensor([W, H]) * 0.1
    wh = torch.exp(torch.rand(n, M, 2, generator=g) * 5.5 + 0.3)
    b = torch.cat([cxcy - wh / 2, cxcy + wh / 2], dim=-1)
    b[0, 0] = torch.tensor([10.0, 10.0, 10.0, 10.0])          # zero area
    b[0, 1] = torch.tensor([-50.0, -40.0, W + 80.0, H + 60.0])  # larger than the image
    b[0, 2] = torch.tensor([W - 3.0, H - 3.0, W + 40.0, H + 40.0])
    return b


def test_roialign_multilevel(dv):
    g = torch.Generator().manual_seed(4)
    n, M, H, W = 2, 300, 160, 256
    feats = _pyramid(g, n, H, W)
    boxes = _boxes(g, n, M, H, W)
    ref = oroi.roi_pooler(feats, boxes)                     # [n*M, C, 7, 7]
    roi, mean = dv.roialign([dv.nhwc_from_nchw(f.cuda()) for f in feats], boxes.cuda(), H, W, want_mean=True)
    check("roialign", roi.float().view(n * M, 7, 7, 256).permute(0, 3, 1, 2), ref, 2e-3, 2e-3)
    check("roialign_mean", mean, ref.view(n * M, 256, -1).mean(-1), 1e-3, 1e-3)


@pytest.mark.parametrize("B,lq,lk", [(2, 300, 300), (1, 777, 900), (1, 64, 37), (3, 17, 1)])
def test_mha_mfma(dv, B, lq, lk):
    """MFMA attention: fp16 operands (oracle gets the same rounded q/k/v), fp32 softmax, fp16 output.  Key and query counts around the
    16 / 32-key tiles, the model's packed pitches, wide score ranges and a stale V^T scratch: tests/test_gpu_mha.py."""
    g = torch.Generator().manual_seed(55)
    d, nh = 256, 8
    q, k, v = (h16(torch.randn(B, l, d, generator=g)) for l in (lq, lk, lk))
    qh = q.view(B, lq, nh, 32).transpose(1, 2) / math.sqrt(32)
    kh, vh = k.view(B, lk, nh, 32).transpose(1, 2), v.view(B, lk, nh, 32).transpose(1, 2)
    ref = (torch.softmax(qh @ kh.transpose(-1, -2), dim=-1) @ vh).transpose(1, 2).reshape(B, lq, d)
    out = dv.mha_f16(q.cuda(), k.cuda(), v.cuda(), nh)
    # P is rounded to fp16 before the PV product (as apex O1's fp16 bmm does): ~1e-3 relative
    check(f"mha_mfma[{B},{lq},{lk}]", out, ref, 4e-3, 4e-3)


def test_add_layernorm(dv):
    g = torch.Generator().manual_seed(6)
    x, r = torch.randn(601, 256, generator=g) * 3 + 1, torch.randn(601, 256, generator=g)
    gm, bt = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.2
    ref = F.relu(F.layer_norm(x + r, (256,), gm, bt))
    out = dv.add_layernorm(x.cuda(), r.cuda(), gm.cuda(), bt.cuda(), relu=True)
    check("add_layernorm", out, ref, 1e-4, 1e-4)


@pytest.mark.parametrize("rows,d,with_r,relu", [(1003, 128, False, False), (1003, 128, True, True), (777, 256, True, False), (5, 256, False, True),
                                                 (40, 512, True, False)])
def test_add_layernorm_rows_per_wave_bit_identical(dv, tmp_path, rows, d, with_r, relu):
    """The several-rows-per-wave LayerNorm (d = 128 / 256) against the oracle AND bit for bit against the one-row-per-wave kernel
    (library option ln_rows = 0) on the same inputs."""
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) * 3 + 1
    r = torch.randn(rows, d, generator=g) if with_r else None
    gm, bt = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.2
    ref = F.layer_norm(x + r if with_r else x, (d,), gm, bt)
    ref = F.relu(ref) if relu else ref
    out = dv.add_layernorm(x.cuda(), None if r is None else r.cuda(), gm.cuda(), bt.cuda(), relu=relu)
    check(f"add_layernorm_rows[{rows},{d}]", out, ref, 1e-4, 1e-4)
    dv.set_option("ln_rows", 0)
    try:
        one_row = dv.add_layernorm(x.cuda(), None if r is None else r.cuda(), gm.cuda(), bt.cuda(), relu=relu)
    finally:
        dv.reset_options()
    assert torch.equal(out, one_row), "rows-per-wave LayerNorm differs from the one-row-per-wave kernel"


def _head_setup(seed=0):
    from diffusionvid_amd.utils import synthetic
    sd = synthetic.make_head_state_dict(seed)
    # the GPU path holds GEMM weights in fp16: give the oracle the same rounded matrices
    sdo = {k: (h16(v) if v.dim() > 1 else v) for k, v in sd.items()}
    return sd, sdo


def test_dynconv(dv):
    sd, sdo = _head_setup()
    g = torch.Generator().manual_seed(7)
    R, d, dd = 64, 256, 64
    pfx = "head.head_series.0.inst_interact"
    roi = h16(torch.randn(R, 49, d, generator=g))
    pro = h16(torch.randn(1, R, d, generator=g))
    params = h16(F.linear(pro, sdo[pfx + ".dynamic_layer.weight"], sdo[pfx + ".dynamic_layer.bias"]))[0]   # [R, 32768]
    p1 = params[:, :d * dd].view(R, d, dd)
    p2 = params[:, d * dd:].view(R, dd, d)
    f = torch.bmm(roi, p1)
    f = h16(F.relu(F.layer_norm(f, (dd,), sd[pfx + ".norm1.weight"], sd[pfx + ".norm1.bias"])))
    f = torch.bmm(f, p2)
    ref = F.relu(F.layer_norm(f, (d,), sd[pfx + ".norm2.weight"], sd[pfx + ".norm2.bias"]))
    packed = torch.cat([p1.transpose(1, 2).reshape(R, -1), p2.transpose(1, 2).reshape(R, -1)], dim=1)   # P1T | P2T
    out = dv.dynconv(roi.cuda().half(), packed.cuda().half(), sd[pfx + ".norm1.weight"].cuda(), sd[pfx + ".norm1.bias"].cuda(),
                     sd[pfx + ".norm2.weight"].cuda(), sd[pfx + ".norm2.bias"].cuda())
    check("dynconv", out, ref, 4e-3, 4e-3)


@pytest.mark.parametrize("cond", [False, True])
def test_rcnn_head(dv, cond):
    """Whole RCNNHead / RCNNHead_cond pass (box_head.py:495-548 / :605-664) at full dims."""
    sd, sdo = _head_setup()
    g = torch.Generator().manual_seed(8)
    n, M, H, W = 2, 300, 160, 256
    feats = _pyramid(g, n, H, W)
    feats = [f * 0.5 for f in feats]
    boxes = _boxes(g, n, M, H, W)
    boxes[0, 0] = torch.tensor([10.0, 10.0, 14.0, 13.0])
    cfg = ohead.HeadCfg()
    t = torch.tensor([999, 499], dtype=torch.long)
    time = osch.time_mlp(sd, "head.", t, 256)
    pfx = "head.head_series_cond.0" if cond else "head.head_series.1"
    pro = None if cond else torch.randn(1, n * M, 256, generator=g)
    cnd = torch.randn(n * M, 256, generator=g) if cond else None
    if cond:
        pro = torch.randn(1, n * M, 256, generator=g)
    taps = {}
    cl, bx, of = ohead.rcnn_head(sdo, pfx, feats, boxes, pro, time, cfg, cond=cnd, taps=taps)
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
    model.reserve(n, H, W, M)
    fd = [dv.nhwc_from_nchw(f.cuda()) for f in feats]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    gl, gb, go = model.rcnn_head(0 if cond else 1, fd, H, W, boxes.cuda(), None if pro is None else pro[0].cuda(), t,
                                 cond=None if cnd is None else cnd.cuda(), bad_flag=flag)
    tag = "cond" if cond else "plain"
    # fp16 GEMM operands through ~12 chained layers: activations are LayerNorm-ed O(1) values
    check(f"rcnn_head[{tag}].obj_features", go, of[0], 2e-2, 2e-2)
    check(f"rcnn_head[{tag}].logits", gl, cl, 2e-2, 2e-2)
    bw = (boxes[..., 2:] - boxes[..., :2]).clamp(min=1.0).max(-1).values   # box size sets the pixel scale of the error
    err = (gb.cpu() - bx).abs().max(-1).values / bw
    print(f"rcnn_head[{tag}].boxes rel-to-size err max={err.max():.3e}")
    assert err.max() < 3e-2
    assert int(flag.item()) == 0
    # first head: pro_features None -> mean of RoI features
    cl0, bx0, of0 = ohead.rcnn_head(sdo, "head.head_series.0", feats, boxes, None, time, cfg)
    gl0, gb0, go0 = model.rcnn_head(0, fd, H, W, boxes.cuda(), None, t)
    check(f"rcnn_head[{tag}].first.obj_features", go0, of0[0], 2e-2, 2e-2)
    model.close()


@pytest.mark.parametrize("cond", [False, True])
def test_roi_fused_dynconv_bit_identical(dv, cond):
    """RoIAlign gathered straight into DynamicConv's LDS tile (csrc/dynconv.hip FUSED_ROI, library option roi_fuse = 1, the default for
    a pass with incoming proposal features) against the two launches (roi_fuse = 0): one copy of the tap arithmetic (csrc/roi_taps.h),
    the same fp16 tile, so every output of the head pass is the same bit for bit -- incl. zero-area, oversize and edge boxes."""
    sd, _ = _head_setup()
    g = torch.Generator().manual_seed(21)
    n, M, H, W = 3, 300, 160, 256
    feats = [f * 0.5 for f in _pyramid(g, n, H, W)]
    boxes = _boxes(g, n, M, H, W)
    boxes[0, 0] = torch.tensor([10.0, 10.0, 14.0, 13.0])
    boxes[1, 5] = torch.tensor([40.0, 40.0, 40.0, 40.0])                # zero area
    boxes[2, 7] = torch.tensor([-30.0, -20.0, 400.0, 300.0])            # beyond the image on every side
    t = torch.tensor([999, 499, 249], dtype=torch.long)
    pro = torch.randn(n * M, 256, generator=g)
    cnd = torch.randn(n * M, 256, generator=g) if cond else None
    fd = [dv.nhwc_from_nchw(f.cuda()) for f in feats]
    outs = {}
    for mode in (0, 1):
        dv.set_option("roi_fuse", mode)
        try:
            model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
            model.reserve(n, H, W, M)
            outs[mode] = tuple(x.clone() for x in model.rcnn_head(0 if cond else 1, fd, H, W, boxes.cuda(), pro.cuda(), t, cond=None if cnd is None else cnd.cuda()))
            model.close()
        finally:
            dv.reset_options()
    for a, b, name in zip(outs[0], outs[1], ("logits", "boxes", "obj_features")):
        assert torch.equal(a, b), f"{name}: fused and unfused head passes differ, max |d| {(a.float() - b.float()).abs().max().item():.3e}"


def test_head_kernels_against_full_dimension_reference_fixture(dv):
    """dvid_rcnn_head and dvid_dynconv against the REFERENCE's own RCNNHead / RCNNHead_cond / DynamicConv at the kernels'
    dimensions (256 / 8 / 2048 / 64, 300 boxes), no oracle in between: tests/golden/g16_full_dim_head.npz holds inputs and
    outputs of the reference modules run on synthetic.make_head_state_dict(0) with fp16-representable matrices
    (make_golden.py: g16_full_dim_head; box_head.py:495-548, :605-664, :687-711).  What separates the two sides is fp16
    storage of the activations between ~12 chained layers and the fp32 summation order.  Measured: object features within
    3.4e-3 (LayerNorm-ed O(1) values), logits within 1.9e-3, DynamicConv within 2e-3; bounds 6e-3 / 2e-3 of RMS + relative, boxes
    1 % of the box size."""
    from conftest import golden
    from diffusionvid_amd.utils import synthetic
    z = golden("g16_full_dim_head")
    n, M, H, W = (int(z[k]) for k in ("n", "M", "H", "W"))
    sd = synthetic.make_head_state_dict(int(z["weights_seed"]))
    T32 = lambda k: torch.from_numpy(z[k].astype(np.float32))
    fd = [dv.nhwc_from_nchw(T32(k).cuda()) for k in ("p3", "p4", "p5")]
    t = torch.from_numpy(z["t"])
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
    model.reserve(n, H, W, M)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def boxes_close(tag, got, want, inp):
        bw = (inp[..., 2:] - inp[..., :2]).clamp(min=1.0).max(-1).values
        err = ((got.cpu() - want).abs().max(-1).values / bw).max().item()
        print(f"{tag}: boxes rel-to-size err max={err:.3e}")
        assert err < 1e-2, tag

    stages = (("head_series.0", 0, False, "boxes", None, "0"), ("head_series.1", 1, False, "bx0", "of0", "1"),
              ("head_series_cond.0", 0, True, "bx1", "of1", "2"))
    for name, idx, is_cond, kb, kf, o in stages:
        bin_ = T32(kb)
        pro = None if kf is None else T32(kf)[0].cuda()
        gl, gb, go = model.rcnn_head(idx, fd, H, W, bin_.cuda(), pro, t, cond=T32("cond").cuda() if is_cond else None, bad_flag=flag)
        check(f"reference_fixture[{name}].obj_features", go, T32("of" + o)[0], 6e-3, 6e-3)
        check(f"reference_fixture[{name}].logits", gl, T32("cl" + o), 2e-3, 2e-3)
        boxes_close(f"reference_fixture[{name}]", gb, T32("bx" + o), bin_)
    assert int(flag.item()) == 0
    model.close()

    # DynamicConv's two per-box products + LayerNorm + ReLU on the fixture's own parameters
    pfx = "head.head_series.2.inst_interact"
    R, d, dd = z["dc_params"].shape[0], 256, 64
    roi = T32("dc_roi").permute(1, 0, 2).contiguous()              # [R, 49, 256]
    params = T32("dc_params")
    p1 = params[:, :d * dd].view(R, d, dd)
    p2 = params[:, d * dd:].view(R, dd, d)
    packed = torch.cat([p1.transpose(1, 2).reshape(R, -1), p2.transpose(1, 2).reshape(R, -1)], dim=1)   # P1T | P2T (weights.hip: make_head)
    out = dv.dynconv(roi.cuda().half(), packed.cuda().half(), sd[pfx + ".norm1.weight"].cuda(), sd[pfx + ".norm1.bias"].cuda(),
                     sd[pfx + ".norm2.weight"].cuda(), sd[pfx + ".norm2.bias"].cuda())
    check("reference_fixture[dynconv]", out, T32("dc_mid"), 4e-3, 4e-3)


@pytest.mark.parametrize("cond,n", [(False, 1), (True, 3), (False, 60)])
def test_head_tail_fused_matches_layerwise(dv, tmp_path, cond, n):
    """csrc/headtail.hip (FFN + norm3 + modulation + towers + class_logits + bboxes_delta + apply_deltas in one row-tile kernel)
    against the layer-by-layer launches it replaces (library option head_tail = 0) on the same inputs: the
    same fp16 operands and fp32 statistics in another summation order, so logits / object features agree to rounding (3e-3 of
    the O(1) values) and boxes to 5e-3 of their size.  300, 900 and 18000 rows, all on 32-row tiles (dvid_head_tail_launch takes them at
    every size) with a ragged last one; 300 rows per frame, so every tenth tile or so straddles two frames.  The three frames of the 900-row
    case carry a time step each (the tile's rows then read different scale rows of the per-frame table), the others one for all frames."""
    sd, _ = _head_setup()
    g = torch.Generator().manual_seed(80 + n)
    M, H, W = 300, 96, 160
    feats = [f * 0.5 for f in _pyramid(g, n, H, W)]
    boxes = _boxes(g, n, M, H, W)
    boxes[0, 0] = torch.tensor([10.0, 10.0, 14.0, 13.0])
    pro = torch.randn(n * M, 256, generator=g)
    cnd = torch.randn(n * M, 256, generator=g) if cond else None
    t = torch.tensor([999, 499, 0], dtype=torch.long) if n == 3 else torch.full((n,), 499, dtype=torch.long)
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
    model.reserve(n, H, W, M)
    fd = [dv.nhwc_from_nchw(f.cuda()) for f in feats]
    dv.set_option("head_tail", 0)
    try:
        ll, lb, lo = (x.cpu() for x in model.rcnn_head(0 if cond else 1, fd, H, W, boxes.cuda(), pro.cuda(), t, cond=None if cnd is None else cnd.cuda()))
    finally:
        dv.reset_options()
    gl, gb, go = model.rcnn_head(0 if cond else 1, fd, H, W, boxes.cuda(), pro.cuda(), t, cond=None if cnd is None else cnd.cuda())
    tag = f"head_tail[{'cond' if cond else 'plain'},{n}]"
    check(tag + ".obj_features", go, lo, 3e-3, 3e-3)
    check(tag + ".logits", gl, ll, 3e-3, 3e-3)
    bw = (boxes[..., 2:] - boxes[..., :2]).clamp(min=1.0).max(-1).values
    err = ((gb.cpu() - lb).abs().max(-1).values / bw).max().item()
    print(f"{tag}.boxes rel-to-size err max={err:.3e}")
    assert err < 5e-3          # exp(dw) on boxes near the clamp amplifies a 1e-3 delta difference (measured 2.3e-3)
    model.close()


def test_global_xattn(dv):
    sd, sdo = _head_setup()
    g = torch.Generator().manual_seed(9)
    R, Lk = 600, 900
    q = torch.randn(1, R, 256, generator=g)
    mem = torch.randn(Lk, 256, generator=g)
    ref = ohead.global_attention(sdo, "head.", h16(q), [h16(mem), None], ohead.HeadCfg())
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
    model.reserve(2, 64, 64, 300)
    out = model.global_xattn(q[0].cuda(), mem.cuda())
    check("global_xattn", out, ref, 5e-3, 5e-3)
    model.close()


def test_noise_to_boxes_and_topk_select(dv):
    g = torch.Generator().manual_seed(10)
    x = torch.randn(3, 300, 4, generator=g) * 1.5
    whwh = torch.tensor([[1000.0, 600.0, 1000.0, 600.0]]).repeat(3, 1)
    ref = osch.noise_to_boxes(x, whwh, 2.0)
    check("noise_to_boxes", dv.noise_to_boxes(x.cuda(), 2.0, 1000.0, 600.0), ref, 1e-6, 1e-6)
    logits = torch.randn(3, 300, 30, generator=g)
    feats = torch.randn(1, 900, 256, generator=g)
    k1, k2 = ohead.select_topk_features(logits, feats, ohead.HeadCfg())
    o1, o2 = dv.select_topk_features(logits.cuda(), feats[0].cuda(), 75, 25)
    assert torch.equal(o1.cpu(), k1) and torch.equal(o2.cpu(), k2)      # pure selection: bit-exact


@pytest.mark.parametrize("time,time_next", [(999, 749), (749, 499), (499, 249)])
def test_ddim_renew_step(dv, time, time_next):
    """A11 (diffusion_det.py:559-596) directly: keep mask, index-order compaction, DDIM update (eta 1), refill.
    Logits sit around the sigmoid 0.5 threshold (|logit| >= 1e-3 so that no keep decision rides on the last ulp of
    expf), include frames with no box kept and with every box kept.  Kept rows must land in the oracle's slots
    (checked through the refill rows, which are copied bit for bit) and agree to 1e-6 relative / 2e-6 absolute:
    the kernel evaluates (sra * x - v) / srm1 in fp32 like the reference, with its own operation order."""
    g = torch.Generator().manual_seed(40 + time)
    n, M, C = 6, 300, 30
    W, H, scale = 1000.0, 600.0, 2.0
    logits = torch.randn(n, M, C, generator=g) * 0.6 - 1.2          # best-of-30 logit straddles 0
    logits[1] = -4.0                                                 # nothing kept
    logits[2] = 3.0                                                  # everything kept
    tiny = logits.abs() < 1e-3
    logits[tiny] = 1e-3
    boxes = _cluster_boxes(g, n, M)
    boxes[:, ::7, 2:] = boxes[:, ::7, :2] + 1500.0                   # x_start beyond the clamp
    x_t = torch.randn(n, M, 4, generator=g) * 1.5
    noise = torch.randn(n, M, 4, generator=g)
    fresh = torch.randn(n, M, 4, generator=g)
    buf = osch.schedule_buffers(1000)
    whwh = torch.tensor([[W, H, W, H]]).repeat(n, 1)
    t = torch.full((n,), time, dtype=torch.long)
    x_start = osch.boxes_to_x_start(boxes, whwh, scale)
    pred_noise = osch.predict_noise_from_start(buf, x_t, t, x_start)
    ref = odet.renew_and_ddim_step(buf, logits, pred_noise, x_start, time, time_next, list(noise), list(fresh))
    sqrt_an, cc, sigma = osch.ddim_coefficients(buf["alphas_cumprod"], time, time_next)
    got = dv.ddim_renew_step(logits.cuda(), boxes.cuda(), x_t.cuda(), noise.cuda(), fresh.cuda(), (W, H), scale,
                             float(buf["sqrt_recip_alphas_cumprod"][time]), float(buf["sqrt_recipm1_alphas_cumprod"][time]),
                             float(sqrt_an), float(cc), float(sigma), 0.5).cpu()
    keep = torch.sigmoid(logits).amax(-1) > 0.5
    nr = keep.sum(-1)
    assert int(nr[1]) == 0 and int(nr[2]) == M and 20 < int(nr[0]) < M - 20
    for f in range(n):
        k = int(nr[f])
        assert torch.equal(got[f, k:], fresh[f, :M - k]), f"frame {f}: refill rows differ (kept {k})"     # bit-exact copies
        np.testing.assert_allclose(got[f, :k].numpy(), ref[f, :k].numpy(), rtol=1e-6, atol=2e-6)
    # the slot of a kept box is its rank among the kept boxes: recompute one frame's rows from scratch, per box
    f = 0
    idx = torch.nonzero(keep[f]).flatten()
    for slot in (0, len(idx) // 2, len(idx) - 1):
        i = int(idx[slot])
        want = x_start[f, i] * sqrt_an + cc * pred_noise[f, i] + sigma * noise[f, slot]
        np.testing.assert_allclose(got[f, slot].numpy(), want.numpy(), rtol=1e-6, atol=2e-6)


def _separated_logits(g, n, M, C):
    """Logits whose sigmoid values are pairwise distinct by a wide margin (no rounding-level ties)."""
    vals = torch.linspace(-9.0, 3.0, n * M * C)
    perm = torch.randperm(n * M * C, generator=g)
    return vals[perm].view(n, M, C)


def _cluster_boxes(g, n, M, W=1000.0, H=600.0):
    ctr = torch.rand(n, 12, 2, generator=g) * torch.tensor([W, H])
    which = torch.randint(0, 12, (n, M), generator=g)
    c = torch.gather(ctr, 1, which[..., None].expand(-1, -1, 2)) + torch.randn(n, M, 2, generator=g) * 8
    wh = torch.rand(n, M, 2, generator=g) * 120 + 30
    return torch.cat([c - wh / 2, c + wh / 2], dim=-1)


def test_postproc_x1_exact(dv):
    g = torch.Generator().manual_seed(11)
    n, M, C = 4, 300, 30
    logits = _separated_logits(g, n, M, C)
    boxes = _cluster_boxes(g, n, M)
    ref = opost.inference_x1(logits, boxes, (1000, 600), C)
    ob, osc, ol, oc = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), 1000.0, 600.0)
    for b in range(n):
        k = int(oc[b])
        assert k == len(ref[b]["scores"]), f"frame {b}: kept {k} vs {len(ref[b]['scores'])}"
        np.testing.assert_array_equal(ol[b, :k].cpu().numpy(), ref[b]["labels"])
        np.testing.assert_array_equal(ob[b, :k].cpu().numpy(), ref[b]["boxes"])          # selection + clip: exact
        np.testing.assert_allclose(osc[b, :k].cpu().numpy(), ref[b]["scores"], rtol=0, atol=2e-7)
    assert 5 < int(oc.min()) and int(oc.max()) < M      # NMS really suppressed something


@pytest.mark.parametrize("levels,M", [(7, 300), (1, 300), (40, 100), (5000, 500)])
def test_topk_select_with_ties_exact(dv, levels, M):
    """The radix-select top-k (csrc/postproc.hip: topk_select_kernel) on logits quantised to a few levels: hundreds of exact score
    ties straddle the top-M boundary (levels = 1: every score equal), which must resolve by ascending flat index exactly as the
    oracle's stable sort (and the full bitonic sort this kernel replaces) does.  Use NMS off so that the candidate list itself is
    what is compared."""
    g = torch.Generator().manual_seed(200 + levels)
    n, C = 3, 30
    logits = (torch.randint(0, levels, (n, M, C), generator=g).float() - levels / 2) * (6.0 / max(levels, 2))
    boxes = _cluster_boxes(g, n, M)
    ob, osc, ol, oc = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), 1000.0, 600.0, use_nms=False)
    for b in range(n):
        rb, rs, rl, _ = opost.topk_candidates(logits[b], boxes[b], C)
        assert int(oc[b]) == M
        np.testing.assert_array_equal(ol[b, :M].cpu().numpy(), rl)
        np.testing.assert_array_equal(ob[b, :M].cpu().numpy(), opost.clip_to_image(rb, (1000, 600)))
        np.testing.assert_allclose(osc[b, :M].cpu().numpy(), rs, rtol=0, atol=2e-7)


def test_postproc_ensemble_exact(dv):
    g = torch.Generator().manual_seed(12)
    S, n, M, C = 3, 2, 300, 30
    logits = _separated_logits(g, S * n, M, C).view(S, n, M, C)
    boxes = _cluster_boxes(g, S * n, M).view(S, n, M, 4)
    cands = [[opost.topk_candidates(logits[s, b], boxes[s, b], C)[:3] for b in range(n)] for s in range(S)]
    ref = opost.inference_ensemble(cands, (1000, 600))
    ob, osc, ol, oc = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), 1000.0, 600.0)
    for b in range(n):
        k = int(oc[b])
        assert k == len(ref[b]["scores"])
        np.testing.assert_array_equal(ol[b, :k].cpu().numpy(), ref[b]["labels"])
        np.testing.assert_array_equal(ob[b, :k].cpu().numpy(), ref[b]["boxes"])


def test_postproc_on_reference_nms_vectors(dv):
    """The reference's own NMS test boxes / scores (tests/test_nms.py, golden g12) through the HIP top-k + NMS kernels:
    one class, one frame, so the kept set must equal the oracle's torchvision-convention sweep on the same data (whose
    legacy twin is pinned to the reference's expected indices in tests/test_oracle_golden.py::test_g12_nms_known_answers)."""
    from conftest import golden
    z = golden("g12_nms_known_answers")
    for i in range(int(z["n_cases"])):
        b, sc, th = z[f"boxes{i}"], z[f"scores{i}"], float(z[f"thresh{i}"])
        M, C = len(sc), 30
        logits = torch.full((1, M, C), -20.0)
        logits[0, :, 0] = torch.log(torch.from_numpy(sc) / (1 - torch.from_numpy(sc)))
        boxes = torch.from_numpy(b)[None]
        ref = opost.inference_x1(logits, boxes, (1000, 600), C, iou=th)
        ob, osc, ol, oc = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), 1000.0, 600.0, iou=th)
        k = int(oc[0])
        assert k == len(ref[0]["scores"]), f"case {i}: kept {k} vs {len(ref[0]['scores'])}"
        np.testing.assert_array_equal(ob[0, :k].cpu().numpy(), ref[0]["boxes"])
        assert (ol[0, :k].cpu().numpy() == 1).all()


def test_cdist_fps_gather(dv):
    """cdist -> greedy FPS -> gather at the model's sizes, all on the register kernel.  The thresholds between the FPS kernels, the LDS
    form beyond 4096 points, emulated block sizes, tile edges of cdist and equal rows: tests/test_gpu_fps.py."""
    g = torch.Generator().manual_seed(13)
    x = torch.randn(1800, 256, generator=g)
    D = torch.cdist(x, x, p=2.0)
    Dg = dv.cdist(x.cuda())
    off = ~torch.eye(1800, dtype=torch.bool)
    check("cdist(offdiag)", Dg.cpu()[off], D[off], 1e-5, 1e-5)
    assert Dg.cpu().diagonal().abs().max() < 0.05       # sqrt of an fp32 cancellation residue, as in torch
    # FPS on the SAME matrix: integer picks are exact
    ref = omem.fps_kernel_order(D.numpy(), 900)
    idx = dv.fps_greedy(D.cuda(), 900)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref)
    got = dv.gather_rows(x.cuda(), idx)
    assert torch.equal(got.cpu(), x[torch.from_numpy(ref.astype(np.int64))])
    # tie-heavy matrix: exercises fps.cu's thread-mapping tie rule
    rng = np.random.RandomState(0)
    Dt = torch.from_numpy(rng.randint(0, 4, size=(600, 600)).astype(np.float32))
    np.testing.assert_array_equal(dv.fps_greedy(Dt.cuda(), 150).cpu().numpy(), omem.fps_kernel_order(Dt.numpy(), 150))
    # the sizes of the streaming mode (900 + 75 -> 900, 150 + 25 -> 150), a size beyond 2048 points, tie-heavy and not
    for n, m, ties in ((975, 900, False), (175, 150, True), (3000, 40, True), (975, 900, True)):
        Dn = torch.from_numpy(rng.randint(0, 5, size=(n, n)).astype(np.float32)) if ties else torch.cdist(x[:n], x[:n], p=2.0)
        np.testing.assert_array_equal(dv.fps_greedy(Dn.cuda(), m).cpu().numpy(), omem.fps_kernel_order(Dn.numpy(), m))


def test_backbone_small(dv):
    """Reduced-depth ResNet-FPN (same kernels, same graph) on 2 frames of 128x192 vs the CPU oracle."""
    from diffusionvid_amd.utils import synthetic
    blocks = (1, 2, 2, 1)
    sd = synthetic.make_state_dict(0, blocks=blocks)
    g = torch.Generator().manual_seed(14)
    imgs = torch.rand(2, 3, 128, 192, generator=g)
    cfg_mean, cfg_std = (123.675, 116.280, 103.530), (58.395, 57.120, 57.375)
    ref = backbone_r101.backbone_r101_fpn(backbone_r101.normalizer(imgs, cfg_mean, cfg_std), sd, "backbone.", blocks)
    model = dv.Model(sd, res_blocks=blocks)
    model.reserve(2, 128, 192, 300)
    p3, p4, p5 = model.backbone(imgs.cuda())
    for name, got in (("p3", p3), ("p4", p4), ("p5", p5)):
        # fp16 activations + fp16 folded-BN weights through ~20 conv layers
        check(f"backbone_small.{name}", dv.nchw_from_nhwc(got), ref[name], 3e-2, 3e-2)
    model.close()


@pytest.mark.parametrize("geom", [(3, 16, 64), (2, 19, 40), (1, 8, 32), (5, 38, 96), (2, 76, 128), (1, 7, 20)])
@pytest.mark.parametrize("variant", ["conv2+next", "conv2", "next", "plain"])
def test_bottleneck128_tail_matches_layers(dv, geom, variant):
    """The 128-wide form (res3): conv2 3x3 -> conv3 + residual + ReLU -> the next block's conv1 in one launch with the weights
    streamed through an LDS ring, against the same layers run one by one on the igemm2 kernel (the chunked 3x3 patch kernel sums in
    another order) -- bit for bit -- and against torch on the same fp16-rounded operands.  Variants: with / without the block's conv2
    in the launch (res3's first block hands in its strided conv2's output), with / without the next conv1."""
    from diffusionvid_amd import _lib
    lib = _lib.load()
    n, hh, ww = geom
    c2, tail = variant.startswith("conv2"), variant.endswith("next")
    g = torch.Generator().manual_seed(n * 1000 + hh * 10 + ww + len(variant))
    res = h16(torch.randn(n, hh, ww, 512, generator=g))
    t1 = h16(torch.randn(n, hh, ww, 128, generator=g).clamp_min(0))      # conv1 output (or, without conv2, the conv2 output)
    w2 = h16(torch.randn(128, 128, 3, 3, generator=g) * (1.5 / 1152 ** 0.5))
    w3 = h16(torch.randn(512, 128, generator=g) * (1.5 / 128 ** 0.5))
    w1n = h16(torch.randn(128, 512, generator=g) * (1.5 / 512 ** 0.5))
    b2, b3, b1n = (torch.randn(c, generator=g) * 0.3 for c in (128, 512, 128))
    t2 = h16(F.relu(F.conv2d(t1.permute(0, 3, 1, 2), w2, b2, padding=1))) if c2 else t1.permute(0, 3, 1, 2)
    out_ref = h16(F.relu(F.conv2d(t2, w3[:, :, None, None], b3) + res.permute(0, 3, 1, 2)))
    t1n_ref = F.relu(F.conv2d(out_ref, w1n[:, :, None, None], b1n))
    (w2p, k2), (w3p, k3), (w1p, k1) = (dv.pack_conv_weight(w) for w in (w2, w3, w1n))
    assert (k2, k3, k1) == (1152, 128, 512)
    resd, t1d = res.to(torch.float16).cuda(), t1.to(torch.float16).cuda()
    w2d, w3d, w1d, b2d, b3d, b1d = w2p.cuda(), w3p.cuda(), w1p.cuda(), b2.cuda(), b3.cuda(), b1n.cuda()
    try:
        _lib.check(lib.dvid_igemm_set_conv3x3(0), "set_conv3x3")
        t2d = dv.conv2d_nhwc(t1d, w2d, k2, b2d, 128, 3, 3, 1, 1, relu=True) if c2 else t1d
    finally:
        lib.dvid_igemm_set_conv3x3(-1)
    out_l = dv.conv2d_nhwc(t2d, w3d, k3, b3d, 512, 1, 1, 1, 0, relu=True, residual=resd, residual_mode=1)
    t1n_l = dv.conv2d_nhwc(out_l, w1d, k1, b1d, 128, 1, 1, 1, 0, relu=True)
    out_f, t1n_f = dv.bottleneck128_tail(t1d, w2d if c2 else None, b2d if c2 else None, w3d, b3d, resd, w1d if tail else None,
                                         b1d if tail else None)
    torch.cuda.synchronize()
    check("bneck128 out", out_f, out_ref.permute(0, 2, 3, 1), 2e-3, 2e-3)
    print("bneck128 vs layers: out identical %.6f" % (out_f == out_l).float().mean().item())
    assert torch.equal(out_f, out_l)
    if tail:
        check("bneck128 t1_next", t1n_f, t1n_ref.permute(0, 2, 3, 1), 2e-3, 2e-3)
        print("bneck128 vs layers: t1_next identical %.6f" % (t1n_f == t1n_l).float().mean().item())
        assert torch.equal(t1n_f, t1n_l)
    else:
        assert t1n_f is None


def test_fused_blocks_reproducible_beside_another_stream(dv):
    """The fused block kernels repeated while a second stream runs the global-memory build's farthest-point sweep (one long-lived small
    workgroup that shares a CU with whatever else is scheduled there -- the situation of a video's first call): every repetition must
    reproduce the first bit for bit.  With 155 KB of LDS instead of the CU's whole 160 KB single patch rows came out wrong about once in
    ten 24-frame launches (csrc/bneck.hip, note at kBytes)."""
    n, hh, ww = 24, 76, 128
    g = torch.Generator().manual_seed(21)
    mk = lambda *s, sc=0.1: torch.randn(*s, generator=g) * sc
    res = torch.randn(n, hh, ww, 512, generator=g, dtype=torch.float16).cuda()
    t1 = res[..., :128].clamp_min(0).contiguous()
    (w2p, _), (w3p, _), (w1p, _) = (dv.pack_conv_weight(w) for w in (mk(128, 128, 3, 3, sc=0.05), mk(512, 128), mk(128, 512, sc=0.06)))
    w2d, w3d, w1d = w2p.cuda(), w3p.cuda(), w1p.cuda()
    b2, b3, b1 = (mk(c, sc=0.3).cuda() for c in (128, 512, 128))
    x256 = torch.randn(n, 2 * hh, 2 * ww, 256, generator=g, dtype=torch.float16).cuda()
    u1 = x256[..., 64:128].clamp_min(0).contiguous()
    (v2p, _), (v3p, _), (v1p, _) = (dv.pack_conv_weight(w) for w in (mk(64, 64, 3, 3), mk(256, 64), mk(128, 256)))
    v2d, v3d, v1d = v2p.cuda(), v3p.cuda(), v1p.cuda()
    c2, c3, c1 = (mk(c, sc=0.3).cuda() for c in (64, 256, 128))
    d0 = dv.cdist(torch.randn(1800, 256, generator=g).cuda())
    side = torch.cuda.Stream()

    def launches():
        a, _ = dv.bottleneck128_tail(t1, w2d, b2, w3d, b3, res)                      # res3 identity block, no next conv1 (where it showed)
        b, bt = dv.bottleneck128_tail(t1, w2d, b2, w3d, b3, res, w1d, b1)
        c, ct = dv.bottleneck64_tail(u1, v2d, c2, v3d, c3, x256, None, None, v1d, c1)
        return [a, b, bt, c, ct]

    base = [o.clone() for o in launches()]
    torch.cuda.synchronize()
    bad = []
    for r in range(40):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dv.fps_greedy(d0, 900)
        outs = [[o.clone() for o in launches()] for _ in range(2)]
        torch.cuda.synchronize()
        for k, got in enumerate(outs):
            for i, (x, y) in enumerate(zip(got, base)):
                if not torch.equal(x, y):
                    bad.append((r, k, i, int((x != y).sum())))
    assert not bad, f"launches beside the other stream differ from the first run: {bad[:8]}"


def test_fused_blocks_counted_waits_beside_lds_traffic():
    """The fault behind the wrong patch rows of the first fused-block build, kept reproducible: with less than the whole LDS
    (library option bneck_lds) a fused workgroup shares its CU with a synthetic neighbour that keeps the LDS pipe busy (tools/lab/spin_kernel.hip,
    mode 3: LDS writes / reads + barriers) -- the condition under which counted vmcnt waits that had ordinary loads among their DMA
    pieces let a step start early (85 of 450 chains differed).  Runs tools/diag_chain_contention.py in a child process; every repetition of the res2 -> res3 chain must reproduce the first bit for bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "tools", "lab", "libspin.so")
    if not os.path.exists(so):
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", os.path.join(root, "tools", "lab", "spin_kernel.hip"), "-o", so],
                       check=True)
    env = dict(os.environ, BNECK_LDS="158720", SIDE="spin:1024:256:4000000:3")          # (the tool's own variables: it sets the library option)
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "diag_chain_contention.py"), "60"], cwd=root, env=env, capture_output=True,
                         text=True, timeout=600)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "60 x 3 chains, 0 differing stage outputs" in out.stdout, out.stdout[-2000:]


@pytest.mark.parametrize("size", [(128, 192), (256, 512), (608, 1024)])
def test_backbone_bottleneck_fusion_bit_identical(dv, size):
    """The ResNet-FPN backbone with res2's and res3's blocks as one launch each behind conv1 (csrc/bneck.hip) against the same backbone with
    layer-by-layer launches: p3 / p4 / p5 bit for bit, at a size the shape rule skips (forced on), a mid size and the bench's frame
    size; 3 frames, so the patch rows of res2 straddle images.  The fused run is also checked against the CPU oracle at the small size."""
    from diffusionvid_amd import _lib
    from diffusionvid_amd.utils import synthetic
    lib = _lib.load()
    blocks = (3, 4, 1, 1)
    sd = synthetic.make_state_dict(3, blocks=blocks)
    g = torch.Generator().manual_seed(size[0])
    imgs = torch.rand(3, 3, size[0], size[1], generator=g)
    model = dv.Model(sd, res_blocks=blocks)
    model.reserve(3, size[0], size[1], 300)
    try:
        # the 3x3 layers on igemm2 in both runs: the fused res3 blocks sum their conv2 in igemm2's order, the patch kernel in another
        _lib.check(lib.dvid_igemm_set_conv3x3(0), "set_conv3x3")
        _lib.check(lib.dvid_igemm_set_bottleneck_fusion(2), "set_bottleneck_fusion")
        fused = [t.clone() for t in model.backbone(imgs.cuda())]
        _lib.check(lib.dvid_igemm_set_bottleneck_fusion(0), "set_bottleneck_fusion")
        plain = [t.clone() for t in model.backbone(imgs.cuda())]
    finally:
        lib.dvid_igemm_set_bottleneck_fusion(-1)
        lib.dvid_igemm_set_conv3x3(-1)
    torch.cuda.synchronize()
    for name, a, b in zip(("p3", "p4", "p5"), fused, plain):
        print("fused vs layer by layer %s: identical %.6f" % (name, (a == b).float().mean().item()))
        assert torch.equal(a, b), name
    if size[0] <= 128:
        cfg_mean, cfg_std = (123.675, 116.280, 103.530), (58.395, 57.120, 57.375)
        ref = backbone_r101.backbone_r101_fpn(backbone_r101.normalizer(imgs, cfg_mean, cfg_std), sd, "backbone.", blocks)
        for name, got in zip(("p3", "p4", "p5"), fused):
            check(f"backbone_fused.{name}", dv.nchw_from_nhwc(got), ref[name], 3e-2, 3e-2)
    model.close()


@pytest.mark.parametrize("size", [(96, 128), (160, 224), (608, 800), (608, 1024)])
def test_stem_pool_fusion_bit_identical(dv, size):
    """The ResNet stem + ReLU + 3x3 / stride-2 max pool as one launch (csrc/conv3x3.hip: stem_pool_kernel -- the half-resolution 64-channel
    map never reaches memory) against the two launches: p3 / p4 / p5 of a shallow backbone bit for bit; 3 frames; pooled maps whose width
    is not a multiple of the 16-pixel patch (56, 100) and whose height is not a multiple of 8 (20); the bench's frame size."""
    from diffusionvid_amd import _lib
    from diffusionvid_amd.utils import synthetic
    lib = _lib.load()
    blocks = (1, 1, 1, 1)
    sd = synthetic.make_state_dict(5, blocks=blocks)
    g = torch.Generator().manual_seed(size[1])
    imgs = torch.rand(3, 3, size[0], size[1], generator=g)
    model = dv.Model(sd, res_blocks=blocks)
    model.reserve(3, size[0], size[1], 300)
    try:
        _lib.check(lib.dvid_set_stem_pool(1), "set_stem_pool")
        fused = [t.clone() for t in model.backbone(imgs.cuda())]
        _lib.check(lib.dvid_set_stem_pool(0), "set_stem_pool")
        plain = [t.clone() for t in model.backbone(imgs.cuda())]
    finally:
        lib.dvid_set_stem_pool(-1)
    torch.cuda.synchronize()
    for name, a, b in zip(("p3", "p4", "p5"), fused, plain):
        print("stem + pool in one launch vs two, %s: identical %.6f" % (name, (a == b).float().mean().item()))
        assert torch.isfinite(a.float()).all() and torch.equal(a, b), name
    model.close()


@pytest.mark.parametrize("size", [(160, 224), (160, 192)], ids=["160x224", "160x192"])
def test_backbone_swin_small(dv, size):
    """Swin-Transformer + FPN (same kernels/graph as Swin-B, reduced widths/depths) vs the CPU oracle:
    patch embed, (shifted-)window MFMA attention with padding + relative-position bias + shift mask,
    GELU MLP, fp32 residual stream, PatchMerging, per-output LayerNorm, FPN.
    160 x 224: token maps 40x56 -> 20x28 -> 10x14 -> 5x7, windows pad along H only (to 42, 21, 14, 7 rows; every width is a multiple
    of 7).  160 x 192: 40x48 -> 20x24 -> 10x12 -> 5x6, windows pad along H as before AND along W at every stage (48 -> 49, 24 -> 28,
    12 -> 14, 6 -> 7); the last map is smaller than a window on both axes.  Every merged map here is even (a frame is padded to a
    multiple of 32): merging an odd map, and the window kernels on their own at single-kernel bounds, are tests/test_gpu_swin.py's."""
    from diffusionvid_amd.utils import synthetic
    from oracle import swin as oswin
    sw = dict(embed_dim=64, depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), window=7)
    sd = synthetic.make_state_dict(0, swin=sw)
    g = torch.Generator().manual_seed(15)
    imgs = torch.rand(2, 3, size[0], size[1], generator=g)
    mean, std = (123.675, 116.280, 103.530), (58.395, 57.120, 57.375)
    ref = oswin.backbone_swin_fpn(backbone_r101.normalizer(imgs, mean, std), sd, "backbone.", embed_dim=64, depths=sw["depths"],
                                  num_heads=sw["heads"])
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0), backbone="swin", swin_embed_dim=64, swin_depths=sw["depths"],
                     swin_heads=sw["heads"])
    model.reserve(2, size[0], size[1], 300)
    p3, p4, p5 = model.backbone(imgs.cuda())
    tag = "backbone_swin_small" if size == (160, 224) else "backbone_swin_small[%dx%d]" % size
    for name, got in (("p3", p3), ("p4", p4), ("p5", p5)):
        check(f"{tag}.{name}", dv.nchw_from_nhwc(got), ref[name], 3e-2, 3e-2)
    model.close()


@pytest.mark.parametrize("case", [
    # (image dims, Cin, Cout, kernel, stride, residual, relu, out_f32)
    dict(n=1, h=1, w=777, cin=256, cout=1024, stride=1, res=True, relu=1),        # bottleneck conv3 + residual, ragged M
    dict(n=2, h=30, w=44, cin=64, cout=256, stride=1, res=True, relu=1),          # res2 conv3 (one K tile)
    dict(n=2, h=30, w=44, cin=128, cout=512, stride=2, res=False, relu=0),        # strided 1x1 shortcut
    dict(n=1, h=1, w=300, cin=256, cout=2048 + 64, stride=1, res=False, relu=0),  # wide N with a ragged last tile
    dict(n=1, h=1, w=500, cin=256, cout=1280, stride=1, res=False, relu=2, f32=True),   # GELU, fp32 out
    dict(n=2, h=19, w=27, cin=64, cout=128, k=3, stride=1, res=False, relu=1),    # 3x3, pad 1 (tap walk + lean epilogue)
    dict(n=2, h=19, w=27, cin=128, cout=128, k=3, stride=2, res=True, relu=1),    # 3x3 stride 2 with residual
    dict(n=1, h=1, w=333, cin=1024, cout=250, stride=1, res=False, relu=0),       # N not a multiple of 8 -> general epilogue
    dict(n=1, h=1, w=640, cin=128, cout=512, stride=1, res=False, relu=2),        # fp16 out + GELU (Swin fc1)
    dict(n=1, h=1, w=640, cin=512, cout=128, stride=1, res=False, relu=1, f32=True),    # fp32 out + ReLU (decoder linears)
    # the shapes the weights-from-L2 configuration (NSTAGE 6) takes: res4 conv1 with a ragged last row tile, a two-column-tile layer
    # with residual, K = 2048 without bias-free shortcuts
    dict(n=1, h=1, w=256 * 11 + 77, cin=1024, cout=256, stride=1, res=False, relu=1),
    dict(n=1, h=1, w=1300, cin=512, cout=512, stride=1, res=True, relu=1),
    dict(n=1, h=1, w=700, cin=2048, cout=256, stride=1, res=False, relu=0),
])
def test_igemm_configs_bit_identical(case):
    """Every tile configuration of the implicit-GEMM kernel must give bit-identical outputs (the per-shape tuner swaps
    them freely), and so must its specialised code paths (FLAT 1x1 addressing, lean epilogue) against the general ones
    (library option igemm_generic = 1); configuration 0 is also checked against fp32 math."""
    from diffusionvid_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    n, h, w, cin, cout, stride = (case[k] for k in ("n", "h", "w", "cin", "cout", "stride"))
    k = case.get("k", 1)
    pad = k // 2
    x = (torch.randn(n, h, w, cin, generator=g) * 0.5).half().cuda()
    wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / (cin * k * k) ** 0.5)
    bias = torch.randn(cout, generator=g).cuda()
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    res = (torch.randn(n, ho, wo, cout, generator=g)).half().cuda() if case["res"] else None
    wp, kpad = ops.pack_conv_weight(wt)
    wp = wp.cuda()

    def run():
        return ops.conv2d_nhwc(x, wp, kpad, bias, cout, k, k, stride, pad, relu=case["relu"], residual=res,
                               residual_mode=1 if res is not None else 0, out_f32=case.get("f32", False)).clone()
    outs = {}
    try:
        for cfg in range(lib.dvid_igemm_num_configs()):
            _lib.check(lib.dvid_igemm_set_config(cfg), "set_config")
            outs[cfg] = run()
        ops.set_option("igemm_generic", 1)
        _lib.check(lib.dvid_igemm_set_config(0), "set_config")
        generic = run()
    finally:
        ops.reset_options()
    ref = outs[0]
    for cfg, o in outs.items():
        assert torch.equal(o, ref), f"configuration {cfg} differs from configuration 0 (max |d| = {(o.float() - ref.float()).abs().max().item():.3e})"
    assert torch.equal(generic, ref), f"specialised paths differ from the general ones (max |d| = {(generic.float() - ref.float()).abs().max().item():.3e})"
    y = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wt.half().float().cuda(), bias, stride=stride, padding=pad).permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.float()
    y = torch.relu(y) if case["relu"] == 1 else torch.nn.functional.gelu(y) if case["relu"] == 2 else y
    assert torch.allclose(ref.float(), y, rtol=2e-3, atol=4e-3)


def test_swin_backbone_specialised_paths_bit_identical():
    """Swin-FPN backbone (fp32 residual stream updated in place, GELU MLP): the specialised igemm code paths against the
    general ones (library option igemm_generic = 1), bit for bit."""
    from diffusionvid_amd import ops
    from diffusionvid_amd.utils import synthetic
    swin = dict(embed_dim=64, depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), window=7)
    sd = synthetic.make_state_dict(3, swin=swin)
    m = ops.Model(sd, res_blocks=(0, 0, 0, 0), backbone="swin", swin_embed_dim=64, swin_depths=swin["depths"], swin_heads=swin["heads"])
    x = torch.rand(2, 3, 160, 224, generator=torch.Generator().manual_seed(1)).cuda()
    m.reserve(2, 160, 224, 300)
    fast = [t.clone() for t in m.backbone(x)]
    ops.set_option("igemm_generic", 1)
    try:
        slow = [t.clone() for t in m.backbone(x)]
    finally:
        ops.reset_options()
    for a, b in zip(fast, slow):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    m.close()


@pytest.mark.parametrize("hw,mn,mx", [((720, 1280), 600, 1000), ((1280, 720), 600, 1000), ((480, 640), 600, 1000), ((600, 1000), 600, 1000),
                                      ((375, 500), 600, 1000), ((97, 161), 60, 100), ((53, 37), 84, 120)])
def test_resize_u8_matches_pillow(dv, hw, mn, mx):
    """csrc/resize.hip: uint8 frame at native size -> Resize(min, max) + ToTensor + /32 zero padding on the device, against
    Pillow's BILINEAR resize (what torchvision's F.resize runs on the reference's PIL images, transforms.py:61-70) --
    byte work, so bit-exact; covers down- and up-scaling, portrait frames, an axis that keeps its size, full VID sizes."""
    from PIL import Image
    from diffusionvid_amd.data import transforms as T
    rng = np.random.RandomState(hw[0])
    img = rng.randint(0, 256, size=hw + (3,)).astype(np.uint8)
    tf = T.ResizeToTensorDevice("cuda", mn, mx, 32)
    out = tf(img, True)
    oh, ow = T.get_size((hw[1], hw[0]), mn, mx)
    assert out.image_size == (oh, ow) and out.shape == (1, 3, -(-oh // 32) * 32, -(-ow // 32) * 32)
    ref = torch.from_numpy(np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR)).copy()).permute(2, 0, 1).float().div(255)
    got = out.cpu()[0]
    assert torch.equal(got[:, :oh, :ow], ref)
    assert got[:, oh:].abs().sum() == 0 and got[:, :, ow:].abs().sum() == 0
    # a reference frame re-uses the current frame's size (transforms.py:63-65)
    other = rng.randint(0, 256, size=hw + (3,)).astype(np.uint8)
    assert tf(other, False).image_size == (oh, ow)


def test_igemm_smallc_16_channels(dv):
    """The Cin = 16 form of the small-channel addressing (two 16-byte chunks per filter tap): a 4x4 / stride-1 / pad-2
    convolution, the shape of the space-to-depth stem, against torch conv2d on the same fp16-rounded operands."""
    g = torch.Generator().manual_seed(61)
    n, h, w, cin, cout = 2, 19, 23, 16, 64
    x = h16(torch.randn(n, cin, h, w, generator=g))
    wt = h16(torch.randn(cout, cin, 4, 4, generator=g) * 0.1)
    bias = torch.randn(cout, generator=g)
    ref = F.relu(F.conv2d(x, wt, bias, stride=1, padding=2))
    wp, kpad = dv.pack_conv_weight(wt)
    assert kpad == 256
    got = dv.conv2d_nhwc(dv.nhwc_from_nchw(x.cuda()), wp.cuda(), kpad, bias.cuda(), cout, 4, 4, 1, 2, relu=True)
    check("igemm_smallc16", dv.nchw_from_nhwc(got), ref, 2e-3, 2e-3)


def test_stem_space_to_depth_equals_nhwc8_form(dv):
    """The stem as a 4x4 convolution over the 2x2 space-to-depth image (default) against the 7x7 / stride-2 form over NHWC8:
    the same fp16 products summed in another order -- last-bit flips at the fp16 stores propagate through the stages (about
    half of the FPN values differ, by a few fp16 ulps at most), and both forms meet the oracle within the backbone tolerance (odd sizes of the padded border included: 96 x 160 and 64 x 96)."""
    from diffusionvid_amd.utils import synthetic
    blocks = (1, 1, 1, 1)
    sd = synthetic.make_state_dict(0, blocks=blocks)
    g = torch.Generator().manual_seed(62)
    for hw in ((96, 160), (64, 96)):
        imgs = torch.rand(3, 3, hw[0], hw[1], generator=g)
        model = dv.Model(sd, res_blocks=blocks)
        model.reserve(3, hw[0], hw[1], 300)
        model.set_chains(1)
        model.set_stem_layout(False)
        a = [t.clone() for t in model.backbone(imgs.cuda())]
        model.set_stem_layout(True)
        b = model.backbone(imgs.cuda())
        torch.cuda.synchronize()
        mean, std = (123.675, 116.280, 103.530), (58.395, 57.120, 57.375)
        ref = backbone_r101.backbone_r101_fpn(backbone_r101.normalizer(imgs, mean, std), sd, "backbone.", blocks)
        for name, x, y in zip(("p3", "p4", "p5"), a, b):
            same = (x == y).float().mean().item()
            d = (x.float() - y.float()).abs().max().item()
            print(f"stem layouts {hw} {name}: identical {same:.4f}, max |diff| {d:.3e}")
            assert d < 0.05, (name, d)
            check(f"backbone_s2d.{name}", dv.nchw_from_nhwc(y), ref[name], 3e-2, 3e-2)
        model.close()


@pytest.mark.parametrize("shape", [(2, 19, 35, 64, 128, True), (3, 38, 64, 256, 256, True), (1, 8, 32, 128, 512, False),
                                   (2, 5, 70, 192, 128, True), (1, 76, 128, 128, 128, True),
                                   (3, 19, 35, 64, 64, True), (1, 40, 64, 64, 64, False)])
def test_conv3x3_halo(dv, shape):
    """csrc/conv3x3.hip (3x3 / stride 1 / pad 1, the 8 x 32 patch's halo staged once per 32-channel chunk) against torch conv2d
    on the same fp16-rounded operands and against the igemm2 kernel on the same launch (same products, another summation
    order): ragged patch grids (19 x 35, 5 x 70), one-patch images, Cout of one or two 256-wide / 128-wide tiles, bias, ReLU.
    The 64 -> 64 channel variant (res2) keeps igemm2's K order and must equal it bit for bit."""
    from diffusionvid_amd import _lib
    lib = _lib.load()
    n, h, w, cin, cout, relu = shape
    g = torch.Generator().manual_seed(70 + h)
    x = h16(torch.randn(n, cin, h, w, generator=g))
    wt = h16(torch.randn(cout, cin, 3, 3, generator=g) * (1.5 / (9 * cin) ** 0.5))
    bias = torch.randn(cout, generator=g) * 0.5
    ref = F.conv2d(x, wt, bias, stride=1, padding=1)
    if relu:
        ref = F.relu(ref)
    wp, kpad = dv.pack_conv_weight(wt)
    xn = dv.nhwc_from_nchw(x.cuda())
    try:
        _lib.check(lib.dvid_igemm_set_conv3x3(2), "set_conv3x3")       # 2: wherever the layer type fits, whatever the shape rule says
        got = dv.conv2d_nhwc(xn, wp.cuda(), kpad, bias.cuda(), cout, 3, 3, 1, 1, relu=relu)
        _lib.check(lib.dvid_igemm_set_conv3x3(0), "set_conv3x3")
        base = dv.conv2d_nhwc(xn, wp.cuda(), kpad, bias.cuda(), cout, 3, 3, 1, 1, relu=relu)
    finally:
        lib.dvid_igemm_set_conv3x3(-1)
    torch.cuda.synchronize()
    check("conv3x3_halo", dv.nchw_from_nhwc(got), ref, 2e-3, 2e-3)
    d = (got.float() - base.float()).abs().max().item()
    print("halo vs igemm2: max |diff| %.3e, identical %.4f" % (d, (got == base).float().mean().item()))
    assert d <= 4e-3 * max(1.0, ref.abs().max().item())
    if cout == 64:
        assert torch.equal(got, base)


@pytest.mark.parametrize("shape", [(2, 19, 35), (1, 40, 64), (3, 9, 33)])
def test_conv4x4_s2d_stem_kernel(dv, shape):
    """The space-to-depth stem's window (4x4 taps, stride 1, 2 rows / columns before and 1 after, 16 -> 64 channels) on
    csrc/conv3x3.hip's conv4x4_s2d_kernel against torch (explicit asymmetric padding) and against the igemm2 small-channel path,
    whose K order it keeps: bit-identical.  Ragged patch grids, patches straddling images."""
    from diffusionvid_amd import _lib
    lib = _lib.load()
    n, h, w = shape
    g = torch.Generator().manual_seed(90 + h)
    x = h16(torch.randn(n, 16, h, w, generator=g))
    wt = h16(torch.randn(64, 16, 4, 4, generator=g) * 0.1)
    bias = torch.randn(64, generator=g)
    ref = F.relu(F.conv2d(F.pad(x, (2, 1, 2, 1)), wt, bias, stride=1))
    wp, kpad = dv.pack_conv_weight(wt)
    assert kpad == 256
    xn = dv.nhwc_from_nchw(x.cuda())
    try:
        _lib.check(lib.dvid_igemm_set_conv3x3(2), "set_conv3x3")
        got = dv.conv2d_nhwc(xn, wp.cuda(), kpad, bias.cuda(), 64, 4, 4, 1, -2, relu=True)
        _lib.check(lib.dvid_igemm_set_conv3x3(0), "set_conv3x3")
        base = dv.conv2d_nhwc(xn, wp.cuda(), kpad, bias.cuda(), 64, 4, 4, 1, -2, relu=True)
    finally:
        lib.dvid_igemm_set_conv3x3(-1)
    torch.cuda.synchronize()
    check("conv4x4_s2d", dv.nchw_from_nhwc(got), ref, 2e-3, 2e-3)
    check("conv4x4_s2d.igemm2", dv.nchw_from_nhwc(base), ref, 2e-3, 2e-3)
    assert torch.equal(got, base)


@pytest.mark.parametrize("geom", [(3, 16, 64), (2, 19, 40), (1, 8, 32), (5, 38, 96), (2, 152, 256), (1, 7, 20)])
@pytest.mark.parametrize("variant", ["shortcut+next", "identity+next", "identity", "shortcut", "identity+next128"])
def test_bottleneck_tail_matches_layers(dv, geom, variant):
    """csrc/bneck.hip (conv2 3x3 -> conv3 + shortcut / residual + ReLU -> the next block's conv1 in one launch, intermediates in
    registers) against the same layers run one by one through dvid_conv2d_nhwc_f16 -- bit for bit -- and against torch on the same
    fp16-rounded operands.  Geometries: several images per launch (patch rows straddle images), heights that are not a multiple
    of 8, widths that are not a multiple of 32, a single-patch map, the bench's 152 x 256 map."""
    n, hh, ww = geom
    sc, tail = variant.startswith("shortcut"), "next" in variant
    nn = 128 if variant.endswith("128") else 64          # next conv1: a res2 block's (64) or res3's first (128)
    g = torch.Generator().manual_seed(n * 1000 + hh * 10 + ww + len(variant))
    cin = 64 if sc else 256
    x = h16(torch.randn(n, hh, ww, cin, generator=g))                   # block input
    t1 = h16(torch.randn(n, hh, ww, 64, generator=g).clamp_min(0))      # conv1 output (after ReLU)
    w2 = h16(torch.randn(64, 64, 3, 3, generator=g) * (1.5 / 576 ** 0.5))
    w3 = h16(torch.randn(256, 64, generator=g) * (1.5 / 8))
    wsc = h16(torch.randn(256, 64, generator=g) * (1.5 / 8))
    w1n = h16(torch.randn(nn, 256, generator=g) * (1.5 / 16))
    b2, b3, bsc, b1n = (torch.randn(c, generator=g) * 0.3 for c in (64, 256, 256, nn))
    # torch reference on the same operands (fp32), rounding where the layer-by-layer path stores fp16
    t2 = h16(F.relu(F.conv2d(t1.permute(0, 3, 1, 2), w2, b2, padding=1)))
    y = F.conv2d(t2, w3[:, :, None, None], b3)
    res = h16(F.conv2d(x.permute(0, 3, 1, 2), wsc[:, :, None, None], bsc)) if sc else x.permute(0, 3, 1, 2)
    out_ref = h16(F.relu(y + res))
    t1n_ref = F.relu(F.conv2d(out_ref, w1n[:, :, None, None], b1n))
    # layer by layer on the device
    w2p, k2 = dv.pack_conv_weight(w2)
    w3p, k3 = dv.pack_conv_weight(w3)
    wsp, ks = dv.pack_conv_weight(wsc)
    w1p, k1 = dv.pack_conv_weight(w1n)
    assert (k2, k3, ks, k1) == (576, 64, 64, 256)
    xd, t1d = x.to(torch.float16).cuda(), t1.to(torch.float16).cuda()
    w2d, w3d, wsd, w1d = w2p.cuda(), w3p.cuda(), wsp.cuda(), w1p.cuda()
    b2d, b3d, bsd, b1d = b2.cuda(), b3.cuda(), bsc.cuda(), b1n.cuda()
    t2d = dv.conv2d_nhwc(t1d, w2d, k2, b2d, 64, 3, 3, 1, 1, relu=True)
    resd = dv.conv2d_nhwc(xd, wsd, ks, bsd, 256, 1, 1, 1, 0) if sc else xd
    out_l = dv.conv2d_nhwc(t2d, w3d, k3, b3d, 256, 1, 1, 1, 0, relu=True, residual=resd, residual_mode=1)
    t1n_l = dv.conv2d_nhwc(out_l, w1d, k1, b1d, nn, 1, 1, 1, 0, relu=True)
    # one launch
    out_f, t1n_f = dv.bottleneck64_tail(t1d, w2d, b2d, w3d, b3d, xd, wsd if sc else None, bsd if sc else None,
                                        w1d if tail else None, b1d if tail else None)
    torch.cuda.synchronize()
    check("bneck out", out_f, out_ref.permute(0, 2, 3, 1), 2e-3, 2e-3)
    print("bneck vs layers: out identical %.6f" % (out_f == out_l).float().mean().item())
    assert torch.equal(out_f, out_l)
    if tail:
        check("bneck t1_next", t1n_f, t1n_ref.permute(0, 2, 3, 1), 2e-3, 2e-3)
        print("bneck vs layers: t1_next identical %.6f" % (t1n_f == t1n_l).float().mean().item())
        assert torch.equal(t1n_f, t1n_l)
    else:
        assert t1n_f is None


@pytest.mark.parametrize("shape", [(8 * 32 * 40 + 13, 256, 1024, True, True), (5000, 128, 512, True, True), (70001, 256, 2048, False, True),
                                   (3000, 256, 8192, False, False), (2400, 256, 32768, False, False), (31, 256, 256, True, False),
                                   (9000, 128, 256, True, True), (40000, 256, 256, False, True),
                                   (38912 + 5, 128, 512, False, 2), (9728, 256, 1024, False, 2),           # Swin-B fc1 of stages 1 / 2: exact GELU
                                   (2432 * 3 + 7, 512, 2048, False, 2), (5000, 512, 2048, False, True),     # ... of stage 3 (K = 512)
                                   (2432 * 5 + 3, 512, 1536, False, False), (9728 * 2 + 1, 256, 768, False, False)])   # Swin qkv (N = 3C: 6 / 3 slabs)
def test_wstat_matches_igemm2(dv, shape):
    """csrc/wstat.hip (weights stationary in registers, rows streamed through a DMA ring, epilogue from the accumulator layout)
    against torch on the same fp16-rounded operands and against igemm2 on the same launch -- bit for bit: same MFMA, same K
    order, same epilogue arithmetic.  Row counts that are not a multiple of 32, launches with idle workgroups (31 rows), one
    slab per workgroup (N 256 .. 8192) and several (N 32768), with / without residual, bias, ReLU."""
    from diffusionvid_amd import _lib
    lib = _lib.load()
    m, k, n, res, relu = shape
    g = torch.Generator().manual_seed(m + n)
    x = h16(torch.randn(m, k, generator=g))
    wt = h16(torch.randn(n, k, generator=g) * (1.5 / k ** 0.5))
    bias = torch.randn(n, generator=g) * 0.5
    r = h16(torch.randn(m, n, generator=g)) if res else None
    ref = x @ wt.t() + bias
    if res:
        ref = ref + r
    if relu:
        ref = F.gelu(ref) if relu == 2 else F.relu(ref)
    wp, kpad = dv.pack_conv_weight(wt)
    xd = x.to(torch.float16).cuda().view(m, 1, 1, k)
    rd = r.to(torch.float16).cuda().view(m, 1, 1, n) if res else None
    try:
        _lib.check(lib.dvid_igemm_set_wstat(2), "set_wstat")           # 2: wherever the layer type fits, whatever the size rule says
        got = dv.conv2d_nhwc(xd, wp.cuda(), kpad, bias.cuda(), n, 1, 1, 1, 0, relu=relu, residual=rd, residual_mode=1 if res else 0)
        _lib.check(lib.dvid_igemm_set_wstat(0), "set_wstat")
        base = dv.conv2d_nhwc(xd, wp.cuda(), kpad, bias.cuda(), n, 1, 1, 1, 0, relu=relu, residual=rd, residual_mode=1 if res else 0)
    finally:
        lib.dvid_igemm_set_wstat(-1)
    torch.cuda.synchronize()
    check("wstat", got.view(m, n), ref, 2e-3, 2e-3)
    same = (got == base).float().mean().item()
    print("wstat vs igemm2: identical %.6f, max |diff| %.3e" % (same, (got.float() - base.float()).abs().max().item()))
    assert torch.equal(got, base)



def test_counter_normal_matches_oracle():
    """dvid_counter_normal (device-side draws of the DDIM loop) vs oracle/noise.py: the integer part (Philox4x32-10) is exact by
    construction; the fp64 Box-Muller of the device math library and of numpy may differ in the last fp64 bits, which survives the
    rounding to fp32 with probability ~4e-9 per value -- over 1.2 million values at most 4 may differ, by one fp32 ulp."""
    from diffusionvid_amd import ops
    from oracle import noise
    key0 = noise.draw_key("renew", 296, 2, 0)
    got = ops.counter_normal(key0, 5, (60001, 4)).cpu().numpy()
    assert got.shape == (5, 60001, 4)
    n_diff = 0
    for i in range(5):
        ref = noise.counter_normal(key0 + i, 60001 * 4).reshape(60001, 4)
        d = got[i] != ref
        n_diff += int(d.sum())
        if d.any():
            ulp = np.spacing(np.abs(ref[d]).astype(np.float32))
            assert (np.abs(got[i][d] - ref[d]) <= ulp).all()
    assert n_diff <= 4, n_diff
    # ragged sizes (the tail quad is cut), one image, and a 64-bit key
    for per in (1, 2, 3, 5, 1023):
        g = ops.counter_normal((1 << 40) + 17, 1, (per,)).cpu().numpy()[0]
        np.testing.assert_array_equal(g, noise.counter_normal((1 << 40) + 17, per))


