"""Tensor-level wrappers over the libdvid_hip C ABI (torch supplies device memory and streams only).

Every function launches HIP kernels on the current torch stream; none falls back to torch math.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr


def _cuda(t, dtype=None):
    if not t.is_cuda:
        raise _lib.DvidError("libdvid_hip ops need tensors on the GPU (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return t.contiguous()


def nhwc_from_nchw(x):
    """fp32 NCHW -> fp16 NHWC."""
    x = _cuda(x, torch.float32)
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, c), dtype=torch.float16, device=x.device)
    call("dvid_nhwc_from_nchw", ptr(x), ptr(out), n, h, w, c, stream_ptr())
    return out


def nchw_from_nhwc(x):
    """fp16 NHWC -> fp32 NCHW (an fp32 NHWC map, DTYPE float32, is a pure permutation: a strided copy)."""
    if x.dtype == torch.float32:
        return _cuda(x).permute(0, 3, 1, 2).contiguous()
    x = _cuda(x, torch.float16)
    n, h, w, c = x.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    call("dvid_nchw_from_nhwc", ptr(x), ptr(out), n, h, w, c, stream_ptr())
    return out


def pack_conv_weight(w, cin_pad=0):
    """OIHW fp32 (or [out,in]) -> fp16 [cout, kpad] with k = (ky*kw+kx)*cin + c (host side repack)."""
    w = w.detach().float().cpu()
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    cp = cin_pad or cin
    kreal = kh * kw * cp
    kpad = (kreal + 63) // 64 * 64
    packed = torch.zeros((cout, kh * kw, cp), dtype=torch.float32)
    packed[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    out = torch.zeros((cout, kpad), dtype=torch.float16)
    out[:, :kreal] = packed.reshape(cout, kreal).to(torch.float16)
    return out, kpad


def conv2d_nhwc(x, w_packed, kpad, bias, cout, kh, kw, stride, pad, relu=False, residual=None, residual_mode=0,
                out_f32=False):
    """x fp16 NHWC; returns NHWC fp16 (or fp32)."""
    x = _cuda(x, torch.float16)
    n, h, wd, cin = x.shape
    if pad < 0:          # same-size window: |pad| before, the rest after (stride 1)
        ho, wo = h, wd
    else:
        ho = (h + 2 * pad - kh) // stride + 1
        wo = (wd + 2 * pad - kw) // stride + 1
    out = torch.empty((n, ho, wo, cout), dtype=torch.float32 if out_f32 else torch.float16, device=x.device)
    call("dvid_conv2d_nhwc_f16", ptr(x), ptr(w_packed), ptr(bias), ptr(residual), ptr(out), n, h, wd, cin, cout, kh, kw,
         stride, pad, kpad, int(relu), int(out_f32), residual_mode, stream_ptr())
    return out


# ---- DTYPE float32 forms (csrc/f32.hip for conv / linear, the f32_* kernels of csrc/roialign.hip, attention.hip, dynconv.hip): fp32 NHWC activations, un-rounded weights, fp32 MFMA --------------------------------------
def pack_conv_weight_f32(w, scale_rows=False):
    """OIHW fp32 (or [out, in]) -> fp32 [cout, kpad], k = (ky*kw+kx)*cin4 + c with cin4 = cin rounded up to 4, kpad to 16 (zeros).
    scale_rows: additionally multiply each row by the power of two that puts its largest magnitude in [0.5, 1) and return
    (packed, kpad, row_scale) with row_scale = 2^-e for conv2d_nhwc_f32 (what csrc/weights.hip: make_conv does for DTYPE float32)."""
    w = w.detach().float().cpu()
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    c4 = (cin + 3) // 4 * 4
    kpad = (kh * kw * c4 + 15) // 16 * 16
    packed = torch.zeros((cout, kh * kw, c4), dtype=torch.float32)
    packed[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    out = torch.zeros((cout, kpad), dtype=torch.float32)
    out[:, :kh * kw * c4] = packed.reshape(cout, -1)
    if scale_rows:
        mx = out.abs().amax(dim=1)
        e = torch.where(mx > 0, torch.frexp(mx)[1], torch.zeros_like(mx, dtype=torch.int32)).to(torch.float32)
        return out * torch.exp2(-e)[:, None], kpad, torch.exp2(e)
    return out, kpad


def split_f16(w_packed):
    """fp32 -> (hi, lo) fp16 planes, hi = fp16(w), lo = fp16(w - hi): the weight operand of the split-operand kernel (conv2d_nhwc_f32)"""
    hi = w_packed.to(torch.float16)
    return hi, (w_packed - hi.to(torch.float32)).to(torch.float16)


def conv2d_nhwc_f32(x, w_packed, kpad, bias, cout, kh, kw, stride, pad, relu=0, residual=None, residual_mode=0, row_scale=None, w_split=None):
    """x fp32 NHWC (channels a multiple of 4); returns fp32 NHWC.  relu: 0 none, 1 ReLU, 2 exact GELU; row_scale: see pack_conv_weight_f32;
    w_split = split_f16(w_packed): run the products on split fp16 operands (library option f32_split, default on); None: the fp32 MFMA."""
    x = _cuda(x, torch.float32)
    n, h, wd, cin = x.shape
    ho = (h + 2 * pad - kh) // stride + 1
    wo = (wd + 2 * pad - kw) // stride + 1
    out = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
    wh, wl = w_split if w_split is not None else (None, None)
    call("dvid_conv2d_nhwc_f32", ptr(x), ptr(w_packed), ptr(wh), ptr(wl), ptr(bias), ptr(row_scale), ptr(residual), ptr(out), n, h, wd, cin, cout, kh, kw, stride, pad, kpad,
         int(relu), residual_mode, stream_ptr())
    return out


def linear_f32(x, w_packed, kpad, bias, relu=0, row_scale=None, w_split=None):
    rows, k = x.shape
    return conv2d_nhwc_f32(x.view(rows, 1, 1, k), w_packed, kpad, bias, w_packed.shape[0], 1, 1, 1, 0, relu=relu, row_scale=row_scale, w_split=w_split).view(rows, -1)


def _pyramid(feats_nhwc, height, width, what):
    """The maps as the `levels, n_levels` arguments of the library's _levels entries: three maps p3..p5 or four p2..p5, finest first;
    the finest map decides the stride (8 or 4) and every map must have its level's size."""
    feats = list(feats_nhwc)
    if len(feats) not in (3, 4):
        raise _lib.DvidError(f"{what}: the pyramid is 3 maps (p3, p4, p5) or 4 (p2, p3, p4, p5), got {len(feats)}")
    stride = 32 >> (len(feats) - 1)
    for l, f in enumerate(feats):
        if f.dim() != 4 or f.shape[1] * (stride << l) != height or f.shape[2] * (stride << l) != width:
            raise _lib.DvidError(f"{what}: map {l} of {len(feats)} must be NHWC at stride {stride << l} of the {height} x {width} image "
                                 f"(height / feats[0].shape[1] is {stride} for {len(feats)} maps), got shape {tuple(f.shape)}")
    return (C.c_void_p * len(feats))(*[ptr(f) for f in feats]), len(feats)


def roialign_f32(feats_nhwc, boxes, height, width, want_mean=False):
    """feats_nhwc: [p3, p4, p5] or [p2, p3, p4, p5] fp32 NHWC; boxes fp32 [n, M, 4] -> roi fp32 [n*M, 49, C] (+ mean fp32 [n*M, C])."""
    feats = [_cuda(f, torch.float32) for f in feats_nhwc]
    levels, nl = _pyramid(feats, height, width, "roialign_f32")
    boxes = _cuda(boxes, torch.float32)
    n, M = boxes.shape[:2]
    c = feats[0].shape[-1]
    roi = torch.empty((n * M, 49, c), dtype=torch.float32, device=boxes.device)
    mean = torch.empty((n * M, c), dtype=torch.float32, device=boxes.device) if want_mean else None
    call("dvid_roialign_v2_levels_f32", levels, nl, n, height, width, c, ptr(boxes), M, ptr(roi), ptr(mean), stream_ptr())
    return (roi, mean) if want_mean else roi


def mha_f32(q, k, v, nheads):
    """fp32 attention: q [B, Lq, d], k / v [B, Lk, d] -> fp32 [B, Lq, d] (head dim 32)."""
    q, k, v = _cuda(q, torch.float32), _cuda(k, torch.float32), _cuda(v, torch.float32)
    B, lq, d = q.shape
    lk = k.shape[1]
    out = torch.empty_like(q)
    call("dvid_mha_f32", ptr(q), ptr(k), ptr(v), ptr(out), B, lq, lk, nheads, d, d, d, lq * d, lk * d, lq * d, stream_ptr())
    return out


def dynconv_f32(roi, params, g1, b1, g2, b2):
    """roi fp32 [R, 49, 256], params fp32 [R, 32768] as P1T[64][256] | P2T[256][64] -> fp32 [R, 49, 256]"""
    roi, params = _cuda(roi, torch.float32), _cuda(params, torch.float32)
    out = torch.empty_like(roi)
    call("dvid_dynconv_f32", ptr(roi), ptr(params), ptr(g1), ptr(b1), ptr(g2), ptr(b2), ptr(out), roi.shape[0], stream_ptr())
    return out


def bottleneck64_tail(t1, w2, b2, w3, b3, residual, w_sc=None, b_sc=None, w1n=None, b1n=None):
    """Everything behind conv1 of a res2 bottleneck block as one launch (csrc/bneck.hip): t1 fp16 [n,h,w,64]; packed weights w2
    [64,576], w3 [256,64], optional shortcut [256,64] (then `residual` is the 64-channel block input) and next conv1 [64 or 128, 256].
    Returns (out [n,h,w,256], t1_next [n,h,w,64 or 128] or None)."""
    t1 = _cuda(t1, torch.float16)
    n, h, wd, _ = t1.shape
    nn = int(w1n.shape[0]) if w1n is not None else 0
    out = torch.empty((n, h, wd, 256), dtype=torch.float16, device=t1.device)
    t1n = torch.empty((n, h, wd, nn), dtype=torch.float16, device=t1.device) if w1n is not None else None
    call("dvid_bottleneck64_tail_f16", ptr(t1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(residual), ptr(w_sc), ptr(b_sc), ptr(w1n),
         ptr(b1n), nn, ptr(out), ptr(t1n), n, h, wd, stream_ptr())
    return out, t1n


def bottleneck128_tail(t1, w2, b2, w3, b3, residual, w1n=None, b1n=None):
    """The 128-wide form (res3; csrc/bneck.hip): t1 fp16 [n,h,w,128] (w2 None: already the conv2 output); packed w2 [128,1152],
    w3 [512,128], optional next conv1 [128,512]; residual [n,h,w,512].  Returns (out [n,h,w,512], t1_next [n,h,w,128] or None)."""
    t1 = _cuda(t1, torch.float16)
    n, h, wd, _ = t1.shape
    out = torch.empty((n, h, wd, 512), dtype=torch.float16, device=t1.device)
    t1n = torch.empty((n, h, wd, 128), dtype=torch.float16, device=t1.device) if w1n is not None else None
    call("dvid_bottleneck128_tail_f16", ptr(t1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(residual), ptr(w1n), ptr(b1n), ptr(out),
         ptr(t1n), n, h, wd, stream_ptr())
    return out, t1n


def linear(x16, w_packed, kpad, bias, relu=False, out_f32=True):
    rows, k = x16.shape
    y = conv2d_nhwc(x16.view(rows, 1, 1, k), w_packed, kpad, bias, w_packed.shape[0], 1, 1, 1, 0, relu=relu, out_f32=out_f32)
    return y.view(rows, -1)


def roialign(feats_nhwc, boxes, height, width, want_mean=False):
    """feats_nhwc: [p3, p4, p5] or [p2, p3, p4, p5] fp16 NHWC; boxes fp32 [n, M, 4] -> roi fp16 [n*M, 49, C] (+ mean fp32 [n*M, C])."""
    feats = [_cuda(f, torch.float16) for f in feats_nhwc]
    levels, nl = _pyramid(feats, height, width, "roialign")
    boxes = _cuda(boxes, torch.float32)
    n, M = boxes.shape[:2]
    c = feats[0].shape[-1]
    roi = torch.empty((n * M, 49, c), dtype=torch.float16, device=boxes.device)
    mean = torch.empty((n * M, c), dtype=torch.float32, device=boxes.device) if want_mean else None
    call("dvid_roialign_v2_levels", levels, nl, n, height, width, c, ptr(boxes), M, ptr(roi), ptr(mean), stream_ptr())
    return (roi, mean) if want_mean else roi


def mha_f16(q, k, v, nheads):
    """MFMA attention: q [B, Lq, d], k/v [B, Lk, d] (fp32 or fp16, rounded to fp16) -> fp16 [B, Lq, d]."""
    def h(t):
        t = _cuda(t)
        if t.dtype == torch.float16:
            return t
        o = torch.empty(t.shape, dtype=torch.float16, device=t.device)
        call("dvid_f32_to_f16", ptr(t), ptr(o), t.numel(), stream_ptr())
        return o
    q, k, v = h(q), h(k), h(v)
    B, lq, d = q.shape
    lk = k.shape[1]
    out = torch.empty_like(q)
    vt = torch.empty((B * nheads * 32 * ((lk + 31) // 32 * 32 + 32),), dtype=torch.float16, device=q.device)
    call("dvid_mha_f16", ptr(q), ptr(k), ptr(v), ptr(out), ptr(vt), B, lq, lk, nheads, d, d, d, lq * d, lk * d, lq * d,
         stream_ptr())
    return out


def dynconv(roi16, params16, g1, b1, g2, b2):
    roi16, params16 = _cuda(roi16, torch.float16), _cuda(params16, torch.float16)
    out = torch.empty_like(roi16)
    call("dvid_dynconv", ptr(roi16), ptr(params16), ptr(g1), ptr(b1), ptr(g2), ptr(b2), ptr(out), roi16.shape[0], stream_ptr())
    return out


def add_layernorm(x, r, g, b, relu=False):
    x = _cuda(x, torch.float32)
    y = torch.empty_like(x)
    call("dvid_add_layernorm", ptr(x), ptr(r), ptr(g), ptr(b), ptr(y), x.shape[0], x.shape[1], int(relu), stream_ptr())
    return y


def _swin_relbias_pitch(window):
    return (window * window + 31) // 32 * 32


def swin_pack_relbias(table, window=7):
    """relative_position_bias_table fp32 [(2w-1)^2, heads] (host) -> the table the Swin attention kernels read, fp32 [heads, w*w, pitch]
    (host; pitch = w*w rounded up to a multiple of 32: [heads, 49, 64] for window 7, [heads, 144, 160] for window 12; keys w*w.. zero),
    packed by the library's own loader code."""
    table = table.detach().cpu().contiguous()
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[0] != (2 * window - 1) ** 2:
        raise TypeError(f"expected a float32 [{(2 * window - 1) ** 2}, heads] table, got {table.dtype} {tuple(table.shape)}")
    out = torch.empty((table.shape[1], window * window, _swin_relbias_pitch(window)), dtype=torch.float32)
    if window == 7:
        call("dvid_swin_pack_relbias", ptr(table), table.shape[1], ptr(out))
    else:
        call("dvid_swin_pack_relbias_ws", ptr(table), table.shape[1], window, ptr(out))
    return out


def _swin_window_attn(name, dtype, qkv, qkv_bias, relbias, B, H, W, nheads, shift, out, window):
    qkv, qkv_bias, relbias = _cuda(qkv, dtype), _cuda(qkv_bias, dtype), _cuda(relbias, torch.float32)
    C = qkv.shape[1] // 3
    assert tuple(qkv.shape) == (B * H * W, 3 * C) and qkv_bias.numel() == 3 * C
    assert tuple(relbias.shape) == (nheads, window * window, _swin_relbias_pitch(window))
    if out is None:
        out = torch.empty((B * H * W, C), dtype=dtype, device=qkv.device)
    out = _cuda(out, dtype)
    assert out.shape[0] >= B * H * W and out.shape[1] == C
    if window == 7:
        call(name, ptr(qkv), ptr(qkv_bias), ptr(relbias), ptr(out), B, H, W, C, nheads, shift, stream_ptr())
    else:
        call(name + "_ws", ptr(qkv), ptr(qkv_bias), ptr(relbias), ptr(out), B, H, W, C, nheads, shift, window, stream_ptr())
    return out


def swin_window_attn_f16(qkv16, qkv_bias16, relbias, B, H, W, nheads, shift, out=None, window=7):
    """Swin (shifted-)window attention on a [B, H, W] token map: qkv fp16 [B*H*W, 3C] (C = 32 * heads), qkv_bias16 fp16 [3C] (what a
    padded window position holds), relbias fp32 [heads, w*w, pitch] (swin_pack_relbias with the same `window`, 7 or 12) -> fp16
    [B*H*W, C], written into `out`'s first B*H*W rows when one is given."""
    return _swin_window_attn("dvid_swin_window_attn_f16", torch.float16, qkv16, qkv_bias16, relbias, B, H, W, nheads, shift, out, window)


def swin_window_attn_f32(qkv, qkv_bias, relbias, B, H, W, nheads, shift, out=None, window=7):
    """the fp32 form of swin_window_attn_f16 (csrc/attention.hip: f32_swin_window_attn_kernel / f32_swin_window12_attn_kernel)"""
    return _swin_window_attn("dvid_swin_window_attn_f32", torch.float32, qkv, qkv_bias, relbias, B, H, W, nheads, shift, out, window)


def patch_merge_ln(x, g, b, f16=True, f32=True, out16=None, out32=None):
    """Swin PatchMerging up to its LayerNorm: x fp32 [B, H, W, C], g / b fp32 [4C] -> ([B * ceil(H/2) * ceil(W/2), 4C] fp16 or None,
    the same in fp32 or None); `out16` / `out32` (at least that many rows) are written in place of fresh buffers."""
    x, g, b = _cuda(x, torch.float32), _cuda(g, torch.float32), _cuda(b, torch.float32)
    B, H, W, C = x.shape
    rows = B * ((H + 1) // 2) * ((W + 1) // 2)
    assert g.numel() == 4 * C and b.numel() == 4 * C
    if f16 and out16 is None:
        out16 = torch.empty((rows, 4 * C), dtype=torch.float16, device=x.device)
    if f32 and out32 is None:
        out32 = torch.empty((rows, 4 * C), dtype=torch.float32, device=x.device)
    for o, dt in ((out16, torch.float16), (out32, torch.float32)):
        assert o is None or (_cuda(o, dt) is o and o.shape[0] >= rows and o.shape[1] == 4 * C)
    call("dvid_patch_merge_ln", ptr(x), ptr(g), ptr(b), ptr(out16), ptr(out32), B, H, W, C, stream_ptr())
    return out16, out32


def resize_u8_to_f32(src_hwc, oh, ow, ph, pw, xtab, ytab):
    """uint8 [H, W, 3] (device) -> fp32 [1, 3, ph, pw] in [0, 1]: Pillow-identical bilinear resize to (oh, ow), zero padding to
    (ph, pw).  xtab / ytab: (bounds, weights) int32 device tensors of data/transforms.resample_tables, None for an axis
    that keeps its size."""
    src = _cuda(src_hwc, torch.uint8)
    h, w = src.shape[:2]
    out = torch.empty((1, 3, ph, pw), dtype=torch.float32, device=src.device)
    tmp = torch.empty((h, ow, 3), dtype=torch.uint8, device=src.device) if xtab is not None else None
    xb, xk = xtab if xtab is not None else (None, None)
    yb, yk = ytab if ytab is not None else (None, None)
    call("dvid_resize_u8_to_f32", ptr(src), h, w, ptr(tmp), ptr(out), oh, ow, ph, pw, ptr(xb), ptr(xk), 0 if xk is None else xk.shape[1],
         ptr(yb), ptr(yk), 0 if yk is None else yk.shape[1], stream_ptr())
    return out


class ImageTable:
    """The pointer table of n uint8 [h_i, w_i, 3] device images (kept alive here), uploaded once: what resize_views_u8 reads its sources through"""

    def __init__(self, images):
        self.images = [_cuda(t, torch.uint8) for t in images]
        if not self.images or any(t.dim() != 3 or t.shape[2] != 3 for t in self.images):
            raise _lib.DvidError("ImageTable takes a non-empty list of uint8 [h, w, 3] images")
        self.sizes_hw = [(int(t.shape[0]), int(t.shape[1])) for t in self.images]
        self.dev = torch.tensor([t.data_ptr() for t in self.images], dtype=torch.int64).to(self.images[0].device)

    def __len__(self):
        return len(self.images)


def resize_views_u8(srcs, plan, PH, PW, flip):
    """n uint8 [h_i, w_i, 3] device images (a list, or an ImageTable made before the call) -> fp32 [n * (1 + flip), 3, PH, PW] in [0, 1]:
    slot i * (1 + flip) is image i resized Pillow-identically to its (oh_i, ow_i) of `plan` (data/transforms.ViewsPlan), zero outside; with
    `flip` the next slot is its mirror inside its own ow_i columns.  Two launches however many images (dvid_resize_views_u8)."""
    table = srcs if isinstance(srcs, ImageTable) else ImageTable(srcs)
    if len(table) != plan.n or any(hw != (int(d[0]), int(d[1])) for hw, d in zip(table.sizes_hw, plan.desc)):
        raise _lib.DvidError(f"resize_views_u8: the plan describes {plan.n} images of other sizes than the {len(table)} sources")
    dev = table.dev.device
    desc, bounds, weights = plan.to(dev).dev
    flip = 1 if flip else 0
    out = torch.empty((plan.n * (1 + flip), 3, int(PH), int(PW)), dtype=torch.float32, device=dev)
    tmp = torch.empty((plan.tmp_bytes,), dtype=torch.uint8, device=dev)
    host = torch.from_numpy(plan.desc)
    call("dvid_resize_views_u8", ptr(table.dev), plan.n, ptr(desc), ptr(host), ptr(bounds), bounds.shape[0], ptr(weights), weights.numel(), ptr(tmp),
         tmp.numel(), ptr(out), int(PH), int(PW), flip, stream_ptr())
    return out


def bbox_aug_table(views_per_image):
    """fp32 [n * V, 5] rows (w_v, h_v, flip, rw, rh) of bbox_aug_merge from every image's data/transforms.bbox_aug_views: the multipliers
    are the Python doubles w_0 / w_v and h_0 / h_v rounded to fp32, as BoxList.resize's scalar multiplication rounds them"""
    rows = []
    for views in views_per_image:
        w0, h0 = views[0].w, views[0].h
        rows += [(v.w, v.h, 1.0 if v.flip else 0.0, float(w0) / float(v.w), float(h0) / float(v.h)) for v in views]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


def bbox_aug_merge(boxes, scores, labels, counts, table, views):
    """The per-view detections of n images -- boxes [n * V, cap, 4], scores, labels int32 [n * V, cap], counts int32 [n * V], slot
    i * V + v -- mapped into view 0's frame (BoxList.transpose / resize in fp32) -> (cand_boxes [n, V * cap, 4], cand_scores, cand_labels
    int32, live int32 [n]): what nms_frames_tiled takes, live rows first, the padding rows of engine.inference.seq_nms_boxlists behind."""
    boxes, scores = _cuda(boxes, torch.float32), _cuda(scores, torch.float32)
    labels, counts, table = _cuda(labels, torch.int32), _cuda(counts, torch.int32), _cuda(table, torch.float32)
    V = int(views)
    slots, cap = scores.shape
    if V < 1 or slots % V or slots == 0 or cap == 0:
        raise _lib.DvidError(f"bbox_aug_merge: {slots} slots of {cap} rows do not split into images of {V} views")
    n = slots // V
    if boxes.shape != (slots, cap, 4) or labels.shape != (slots, cap) or counts.shape != (slots,) or table.shape != (slots, 5):
        raise _lib.DvidError("bbox_aug_merge: boxes [n * V, cap, 4], scores / labels [n * V, cap], counts [n * V] and table [n * V, 5] must agree")
    dev = boxes.device
    cb = torch.empty((n, V * cap, 4), dtype=torch.float32, device=dev)
    cs = torch.empty((n, V * cap), dtype=torch.float32, device=dev)
    cl = torch.empty((n, V * cap), dtype=torch.int32, device=dev)
    live = torch.empty((n,), dtype=torch.int32, device=dev)
    call("dvid_bbox_aug_merge", ptr(boxes), ptr(scores), ptr(labels), ptr(counts), ptr(table), n, V, cap, ptr(cb), ptr(cs), ptr(cl), ptr(live),
         stream_ptr())
    return cb, cs, cl, live


def bbox_aug_finish(cand_boxes, cand_scores, cand_labels, live, sizes, iou, max_det):
    """Behind bbox_aug_merge: the class-aware NMS at `iou`, clipped to view 0 (`sizes`), minus the padding rows, cut as filter_results
    cuts (more than max_det > 0 survivors: those scoring >= the max_det-th; survivors are in score order, so a prefix) -> (boxes, scores,
    labels, counts) as postproc_topk_nms returns them, the counts rewritten in place."""
    N = cand_scores.shape[1]
    ob, osc, ol, oc = nms_frames_tiled(cand_boxes, cand_scores, cand_labels, sizes, None, iou, True)
    kept = oc - (N - live)
    K = int(max_det)
    if 0 < K < N:
        cut = ((osc >= osc[:, K - 1:K]) & (torch.arange(N, device=osc.device)[None, :] < kept[:, None])).sum(dim=1).to(torch.int32)
        kept = torch.where(kept > K, cut, kept)
    oc.copy_(kept)
    return ob, osc, ol, oc


# ---- the demo surface (csrc/overlay.hip; engine/demo.py) -----------------------------------------------------------------------------------
OVERLAY_MAX_DRAWN = 256          # DVID_OVERLAY_MAX_DRAWN of include/dvid_hip.h: rows drawn per frame, the latest in draw order
OVERLAY_NAME_MAX = 24            # DVID_OVERLAY_NAME_MAX: bytes of a class name on a plate
OVERLAY_TILE = (64, 16)          # (tw, th): the pixels one workgroup of the draw kernel resolves (dvid_overlay_tile)


def overlay_scratch_bytes(n, cap):
    """bytes of scratch dvid_overlay_detections needs for n frames of `cap` rows: the frames' draw lists"""
    return int(_lib.load().dvid_overlay_scratch_bytes(int(n), int(cap)))


def overlay_detections(frames, dets, counts, ratios, names, atlas, threshold=0.7, thickness=2, text_scale=1):
    """Paint detections onto uint8 RGB frames on the device, in place (the contract: include/dvid_hip.h, dvid_overlay_detections).
    frames: one CUDA uint8 tensor [n, H, W, 3] or a list of n [h_i, w_i, 3] CUDA tensors; dets fp32 [n, cap, 6] = box, score, label in the
    model's frame, counts int32 [n]; ratios fp32 [n, 2] = (rw, rh), native / model size; names uint8 [num_classes + 1, 24]
    (engine.demo.name_table); atlas uint8 [95, gh, gw] of 0 / 1 (engine.demo.glyph_atlas).  Returns `frames`.  Scores stay on the device:
    two launches on the current stream, no synchronisation."""
    batch = isinstance(frames, torch.Tensor)
    images = list(frames.unbind(0)) if batch and frames.dim() == 4 else ([frames] if batch else list(frames))
    if batch and frames.dim() != 4:
        raise _lib.DvidError(f"overlay_detections: frames are [n, H, W, 3] or a list of [h, w, 3], got {tuple(frames.shape)}")
    for t in images:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous()):
            raise _lib.DvidError("overlay_detections: every frame is a contiguous CUDA uint8 [h, w, 3] tensor (drawn in place)")
    n = len(images)
    dev = images[0].device if n else None
    dets, counts, ratios = _cuda(dets, torch.float32), _cuda(counts, torch.int32), _cuda(ratios, torch.float32)
    names, atlas = _cuda(names, torch.uint8), _cuda(atlas, torch.uint8)
    if n == 0 or dets.dim() != 3 or dets.shape[0] != n or dets.shape[2] != 6 or counts.shape != (n,) or ratios.shape != (n, 2):
        raise _lib.DvidError(f"overlay_detections: {n} frames take dets [n, cap, 6], counts [n] and ratios [n, 2], got {tuple(dets.shape)}, "
                             f"{tuple(counts.shape)}, {tuple(ratios.shape)}")
    if names.dim() != 2 or names.shape[0] < 2 or names.shape[1] != OVERLAY_NAME_MAX or atlas.dim() != 3 or atlas.shape[0] != 95:
        raise _lib.DvidError(f"overlay_detections: names are [num_classes + 1, {OVERLAY_NAME_MAX}] and the atlas [95, gh, gw], got "
                             f"{tuple(names.shape)}, {tuple(atlas.shape)}")
    cap = dets.shape[1]
    if cap == 0:
        return frames
    host_sizes = torch.tensor([(t.shape[0], t.shape[1]) for t in images], dtype=torch.int32)
    table = torch.tensor([t.data_ptr() for t in images], dtype=torch.int64).to(dev)
    sizes = host_sizes.to(dev)
    scratch = torch.empty((overlay_scratch_bytes(n, cap) // 4,), dtype=torch.int32, device=dev)
    call("dvid_overlay_detections", ptr(table), ptr(sizes), ptr(host_sizes), n, ptr(dets), ptr(counts), cap, ptr(ratios), ptr(names),
         names.shape[0] - 1, ptr(atlas), atlas.shape[1], atlas.shape[2], float(threshold), int(thickness), int(text_scale), ptr(scratch),
         scratch.numel() * 4, stream_ptr())
    return frames


JPEG_PLAN_COLS = 10          # DVID_JPEG_PLAN_COLS


def jpeg_reconstruct_u8(coef, quant, plan_host, plan=None):
    """The device half of the split JPEG decode (the contract: include/dvid_hip.h, dvid_jpeg_reconstruct_u8): dequantise, ISLOW IDCT,
    fancy upsampling, YCbCr -> RGB, equal to libjpeg's (Pillow's) decode bit for bit.  coef: CUDA int16 [n_coef], the coefficients of n
    frames as data.jpeg.entropy_decode leaves them; quant: CUDA int16 holding the uint16 tables' bits, 192 per frame; plan_host: int64
    [n, JPEG_PLAN_COLS] on the host (data.jpeg.plan_rows), checked by the library before anything is launched; plan: the same rows on
    the device (uploaded here when None).  -> a list of n CUDA uint8 [h_i, w_i, 3] tensors, views of one buffer.  Two launches on the
    current stream however many frames, no synchronisation."""
    coef, quant = _cuda(coef, torch.int16), _cuda(quant, torch.int16)
    plan_host = torch.as_tensor(plan_host)
    if plan_host.is_cuda or plan_host.dtype != torch.int64 or plan_host.dim() != 2 or plan_host.shape[1] != JPEG_PLAN_COLS or plan_host.shape[0] < 1:
        raise _lib.DvidError(f"jpeg_reconstruct_u8: the plan is a host int64 [n, {JPEG_PLAN_COLS}] tensor, got {plan_host.dtype} {tuple(plan_host.shape)}")
    plan_host = plan_host.contiguous()
    n = plan_host.shape[0]
    dev = coef.device
    plan = plan_host.to(dev) if plan is None else _cuda(plan, torch.int64)
    if plan.shape != plan_host.shape:
        raise _lib.DvidError("jpeg_reconstruct_u8: the device plan and the host plan differ in shape")
    w, h, off = plan_host[:, 0], plan_host[:, 1], plan_host[:, 9]
    sane = bool(((w >= 1) & (w <= 65535) & (h >= 1) & (h <= 65535) & (off >= 0) & (off < 2 ** 44)).all())
    out_bytes = int((off + h * w * 3).max()) if sane else 1          # a plan the library is about to refuse: nothing to size the output by
    out = torch.empty((out_bytes,), dtype=torch.uint8, device=dev)
    planes = torch.empty((coef.numel(),), dtype=torch.uint8, device=dev)
    call("dvid_jpeg_reconstruct_u8", ptr(coef), coef.numel(), ptr(quant), quant.numel(), ptr(plan), ptr(plan_host), n, ptr(planes), planes.numel(),
         ptr(out), out_bytes, stream_ptr())
    return [out[int(o):int(o) + int(hh) * int(ww) * 3].view(int(hh), int(ww), 3) for ww, hh, o in zip(w.tolist(), h.tolist(), off.tolist())]


class FrameSizes:
    """The per-frame size table of the `_sizes` entry points, checked once on the host and uploaded once: rows (w, h) fp32 [n, 2], every
    entry positive and finite.  `fs[a:b]` is the table of frames a..b (views of both copies, nothing checked or uploaded again)."""

    def __init__(self, sizes, device, _checked=None):
        if _checked is not None:
            self.host, self.dev = _checked
            return
        host = torch.as_tensor(sizes).detach().to("cpu", torch.float32)          # a device tensor is read back: the check is on the host
        if host.dim() != 2 or host.shape[1] != 2:
            raise _lib.DvidError(f"sizes must be [n_frames, 2] rows of (w, h), got {tuple(host.shape)}")
        if not bool(torch.isfinite(host).all()) or not bool((host > 0).all()):
            raise _lib.DvidError("sizes: every (w, h) must be positive and finite")
        self.host = host.contiguous()
        self.dev = self.host.to(device)

    def __len__(self):
        return self.host.shape[0]

    def __getitem__(self, sl):
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError("FrameSizes takes contiguous slices")
        return FrameSizes(None, None, _checked=(self.host[sl], self.dev[sl]))


def _is_sizes(img_w):
    return isinstance(img_w, FrameSizes) or (isinstance(img_w, torch.Tensor) and img_w.dim() >= 1)


def frame_sizes(sizes, n, device):
    """-> the device table [n, 2] of a `sizes` argument: a FrameSizes as it is, a tensor (host or device) checked and uploaded"""
    fs = sizes if isinstance(sizes, FrameSizes) else FrameSizes(sizes, device)
    if len(fs) != n:
        raise _lib.DvidError(f"sizes holds {len(fs)} rows for {n} frames")
    return fs.dev


def noise_to_boxes(x, snr_scale, img_w, img_h=None):
    """x [..., 4] noise -> xyxy boxes scaled to (img_w, img_h); img_w a `sizes` tensor [n, 2]: x is [n, M, 4], frame f scaled to sizes[f]."""
    x = _cuda(x, torch.float32)
    out = torch.empty_like(x)
    if _is_sizes(img_w):
        if x.dim() != 3 or x.shape[-1] != 4:
            raise _lib.DvidError(f"noise_to_boxes with a sizes table takes x [n, M, 4], got {tuple(x.shape)}")
        sizes = frame_sizes(img_w, x.shape[0], x.device)
        if x.numel():
            call("dvid_noise_to_boxes_sizes", ptr(x), ptr(out), x.numel() // 4, x.shape[1], float(snr_scale), ptr(sizes), stream_ptr())
        return out
    call("dvid_noise_to_boxes", ptr(x), ptr(out), x.numel() // 4, float(snr_scale), float(img_w), float(img_h), stream_ptr())
    return out


def counter_normal(key0, n_images, shape, device=None, key_stride=1):
    """[n_images, *shape] N(0, 1) draws generated on the device: image i is the stream keyed `key0 + i * key_stride` (dvid_counter_normal,
    dvid_counter_normal_strided)."""
    if not torch.cuda.is_available():
        raise _lib.DvidError("no HIP device visible: counter_normal draws on the GPU (no CPU fallback; the CPU restatement is oracle/noise.py)")
    out = torch.empty((n_images,) + tuple(shape), dtype=torch.float32, device=device or torch.device("cuda", torch.cuda.current_device()))
    per = 1
    for v in shape:
        per *= int(v)
    if int(key_stride) != 1:
        call("dvid_counter_normal_strided", ptr(out), per, int(n_images), int(key0) & 0xFFFFFFFFFFFFFFFF, int(key_stride) & 0xFFFFFFFFFFFFFFFF, stream_ptr())
        return out
    call("dvid_counter_normal", ptr(out), per, int(n_images), int(key0) & 0xFFFFFFFFFFFFFFFF, stream_ptr())
    return out


def ddim_renew_step(logits, boxes, x_t, noise, fresh, whwh, snr_scale, sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac_next, coef_c,
                    sigma, keep_thr=0.5):
    """Box renewal + DDIM update (diffusion_det.py:559-596); all [n, M, 4] fp32, logits [n, M, C]."""
    logits, boxes, x_t = _cuda(logits, torch.float32), _cuda(boxes, torch.float32), _cuda(x_t, torch.float32)
    noise, fresh = _cuda(noise, torch.float32), _cuda(fresh, torch.float32)
    n, M, c = logits.shape
    out = torch.empty_like(x_t)
    if _is_sizes(whwh):          # a sizes table [n, 2]: frame f normalised by its own (w, h)
        sizes = frame_sizes(whwh, n, logits.device)
        call("dvid_ddim_renew_step_sizes", ptr(logits), ptr(boxes), ptr(x_t), ptr(noise), ptr(fresh), ptr(out), n, M, c, ptr(sizes),
             float(snr_scale), float(sqrt_recip_ac), float(sqrt_recipm1_ac), float(sqrt_ac_next), float(coef_c), float(sigma), float(keep_thr),
             stream_ptr())
        return out
    call("dvid_ddim_renew_step", ptr(logits), ptr(boxes), ptr(x_t), ptr(noise), ptr(fresh), ptr(out), n, M, c, float(whwh[0]),
         float(whwh[1]), float(snr_scale), float(sqrt_recip_ac), float(sqrt_recipm1_ac), float(sqrt_ac_next), float(coef_c),
         float(sigma), float(keep_thr), stream_ptr())
    return out


def select_topk_features(logits, feats, k1, k2):
    """logits [n, M, C], feats [n*M, d] -> ([n*k1, d], [n*k2, d]) in box-index (mask) order."""
    logits, feats = _cuda(logits, torch.float32), _cuda(feats, torch.float32)
    n, M, c = logits.shape
    d = feats.shape[-1]
    o1 = torch.empty((n * k1, d), dtype=torch.float32, device=feats.device)
    o2 = torch.empty((n * k2, d), dtype=torch.float32, device=feats.device)
    call("dvid_select_topk_features", ptr(logits), n, M, c, k1, k2, ptr(feats), d, ptr(o1), ptr(o2), stream_ptr())
    return o1, o2


# Candidates per frame the NMS takes (DVID_NMS_MAX_CANDIDATES of include/dvid_hip.h): (SAMPLE_STEP - 1) * NUM_PROPOSALS with the ensemble,
# NUM_PROPOSALS at SAMPLE_STEP 1.  torchvision's batched_nms keeps the coordinate trick the kernels reproduce only below 5000 boxes.
NMS_MAX_CANDIDATES = 4096


# Largest MODEL.DiffusionDet.NUM_CLASSES a model is built with (DVID_MAX_CLASSES of include/dvid_hip.h): LVIS's 1203 rounded up to whole
# 64-row tiles of class_logits.
MAX_CLASSES = 1280


def postproc_scratch_bytes(nsets, n_frames, m):
    """bytes of scratch dvid_postproc_topk_nms needs for [nsets, n_frames, m, C] logits"""
    return int(_lib.load().dvid_postproc_scratch_bytes(int(nsets), int(n_frames), int(m)))


def postproc_topk_nms(logits, boxes, img_w, img_h=None, iou=0.5, use_nms=True):
    """logits [S, n, M, C] (or [n, M, C]), boxes [S, n, M, 4] -> (boxes [n,S*M,4], scores, labels int32, counts int32).
    img_w a `sizes` tensor [n, 2]: frame f is clipped to sizes[f]."""
    if logits.dim() == 3:
        logits, boxes = logits[None], boxes[None]
    logits, boxes = _cuda(logits, torch.float32), _cuda(boxes, torch.float32)
    S, n, M, c = logits.shape
    dev = logits.device
    ob, osc, ol, oc = split_detection_buffer(torch.empty((n * S * M * 6 + n,), dtype=torch.float32, device=dev), n, S * M)
    scratch = torch.empty(((postproc_scratch_bytes(S, n, M) + 3) // 4,), dtype=torch.float32, device=dev)
    if _is_sizes(img_w):
        sizes = frame_sizes(img_w, n, dev)
        call("dvid_postproc_topk_nms_sizes", ptr(logits), ptr(boxes), S, n, M, c, ptr(sizes), float(iou), int(use_nms),
             ptr(ob), ptr(osc), ptr(ol), ptr(oc), ptr(scratch), stream_ptr())
        return ob, osc, ol, oc
    call("dvid_postproc_topk_nms", ptr(logits), ptr(boxes), S, n, M, c, float(img_w), float(img_h), float(iou), int(use_nms),
         ptr(ob), ptr(osc), ptr(ol), ptr(oc), ptr(scratch), stream_ptr())
    return ob, osc, ol, oc


def topk_candidates_stream(logits, boxes):
    """The candidate selection on its own in its streaming form (topk_stream_kernel), forced at any M <= NMS_MAX_CANDIDATES and
    C <= MAX_CLASSES: logits [S, n, M, C] (or [n, M, C]), boxes [S, n, M, 4] -> (cand_boxes [n, S*M, 4], cand_scores [n, S*M],
    cand_labels int32 [n, S*M]): per (frame, set) the M largest sigmoid scores in (score desc, flat index asc) order."""
    if logits.dim() == 3:
        logits, boxes = logits[None], boxes[None]
    logits, boxes = _cuda(logits, torch.float32), _cuda(boxes, torch.float32)
    S, n, M, c = logits.shape
    assert boxes.shape == (S, n, M, 4)
    dev = logits.device
    cb = torch.empty((n, S * M, 4), dtype=torch.float32, device=dev)
    cs = torch.empty((n, S * M), dtype=torch.float32, device=dev)
    cl = torch.empty((n, S * M), dtype=torch.int32, device=dev)
    call("dvid_topk_candidates_stream", ptr(logits), ptr(boxes), S, n, M, c, ptr(cb), ptr(cs), ptr(cl), stream_ptr())
    return cb, cs, cl


def nms_frames_tiled(cand_boxes, cand_scores, cand_labels, img_w, img_h=None, iou=0.5, use_nms=True):
    """The tiled NMS on its own, at any 1 <= N <= NMS_MAX_CANDIDATES: cand_boxes [n, N, 4] (unclipped xyxy), cand_scores [n, N], cand_labels
    [n, N] int32 -> (boxes [n, N, 4], scores, labels int32, counts int32) as postproc_topk_nms returns them."""
    cand_boxes, cand_scores = _cuda(cand_boxes, torch.float32), _cuda(cand_scores, torch.float32)
    cand_labels = _cuda(cand_labels, torch.int32)
    n, N = cand_scores.shape
    assert cand_boxes.shape == (n, N, 4) and cand_labels.shape == (n, N)
    dev = cand_boxes.device
    ob, osc, ol, oc = split_detection_buffer(torch.empty((n * N * 6 + n,), dtype=torch.float32, device=dev), n, N)
    scratch = torch.empty((max(1, (int(_lib.load().dvid_nms_tiled_scratch_bytes(n, N)) + 3) // 4),), dtype=torch.float32, device=dev)
    if _is_sizes(img_w):          # a sizes table [n, 2]: frame f is clipped to sizes[f]
        sizes = frame_sizes(img_w, n, dev)
        call("dvid_nms_frames_tiled_sizes", ptr(cand_boxes), ptr(cand_scores), ptr(cand_labels), n, N, ptr(sizes), float(iou),
             int(use_nms), N, ptr(ob), ptr(osc), ptr(ol), ptr(oc), ptr(scratch), stream_ptr())
        return ob, osc, ol, oc
    call("dvid_nms_frames_tiled", ptr(cand_boxes), ptr(cand_scores), ptr(cand_labels), n, N, float(img_w), float(img_h), float(iou),
         int(use_nms), N, ptr(ob), ptr(osc), ptr(ol), ptr(oc), ptr(scratch), stream_ptr())
    return ob, osc, ol, oc


SEQ_NMS_ERR_ROUNDS, SEQ_NMS_ERR_COUNTS = 1 << 30, 1 << 29          # include/dvid_hip.h


def seq_nms_class_counts(dets, counts, num_classes):
    """[frames, num_classes] int32 on the host: the frame's detections with label c + 1 (the table dvid_seq_nms_video lays its scratch out from)"""
    dets, counts = dets.detach().cpu(), counts.detach().cpu().to(torch.int64)
    F, cap = dets.shape[:2]
    lab = dets[:, :, 5].to(torch.int64)
    ok = (torch.arange(cap)[None, :] < counts[:, None]) & (lab >= 1) & (lab <= num_classes)
    table = torch.zeros((F, num_classes), dtype=torch.int32)
    rows = torch.arange(F)[:, None].expand(F, cap)[ok]
    table.index_put_((rows, lab[ok] - 1), torch.ones((), dtype=torch.int32), accumulate=True)
    return table


def seq_nms_video(dets, counts, num_classes, video_starts=None, return_status=False):
    """Seq-NMS (TEST.SEQ_NMS, the reference's seq_nms.py) over one video in engine.pack_predictions' layout -- dets [frames, cap, 6] fp32
    (box4, score, label), counts [frames] -- or over several at once: `video_starts` [n_videos + 1] splits the frames.  Returns (keep
    [frames, cap] uint8, scores [frames, cap] fp32: the rescored values, 0 for a suppressed row), on the device; with return_status also
    the [n_videos, num_classes] int32 status words (the rounds each class ran).  Independent of any model handle and of DTYPE."""
    dets, counts = _cuda(dets, torch.float32), _cuda(counts, torch.int32)
    F, cap = counts.shape[0], dets.shape[1] if dets.dim() == 3 else -1
    assert dets.shape == (F, cap, 6), "dets is [frames, cap, 6]"
    starts = torch.tensor([0, F] if video_starts is None else [int(v) for v in video_starts], dtype=torch.int32)
    assert int(starts[-1]) == F and num_classes >= 1, "video_starts ends at the frame count"
    nv = starts.numel() - 1
    dev = dets.device
    keep = torch.empty((F, cap), dtype=torch.uint8, device=dev)
    scores = torch.empty((F, cap), dtype=torch.float32, device=dev)
    status = torch.empty((nv, num_classes), dtype=torch.int32, device=dev)
    if F == 0 or cap == 0:
        return (keep, scores, status.zero_()) if return_status else (keep, scores)
    table = seq_nms_class_counts(dets, counts, num_classes).contiguous() if cap <= NMS_MAX_CANDIDATES and num_classes <= MAX_CLASSES else \
        torch.zeros((F, num_classes), dtype=torch.int32)          # over a limit: the library refuses before it reads the table
    need = max(0, int(_lib.load().dvid_seq_nms_scratch_bytes(ptr(table), ptr(starts), nv, num_classes)))
    scratch = torch.empty((max(16, need),), dtype=torch.uint8, device=dev) if need <= (1 << 30) else None
    call("dvid_seq_nms_video", ptr(dets), ptr(counts), ptr(table), ptr(starts), nv, cap, num_classes, ptr(keep), ptr(scores), ptr(status),
         ptr(scratch), need if scratch is not None else 0, stream_ptr())
    st = status.cpu()
    if int((st & (SEQ_NMS_ERR_ROUNDS | SEQ_NMS_ERR_COUNTS)).ne(0).sum()):
        v, c = [int(x) for x in torch.nonzero(st & (SEQ_NMS_ERR_ROUNDS | SEQ_NMS_ERR_COUNTS))[0]]
        raise _lib.DvidError("Seq-NMS: video %d class %d ended with status 0x%x (%s)" % (
            v, c + 1, int(st[v, c]), "round bound reached" if int(st[v, c]) & SEQ_NMS_ERR_ROUNDS else "class_counts does not describe dets"))
    return (keep, scores, st) if return_status else (keep, scores)


VID_EVAL_MAX_GT, VID_EVAL_MAX_RANGES = 256, 4          # include/dvid_hip.h


def vid_eval_label_range(dets, counts, gt_labels=None):
    """(least, greatest) label among the rows of dets [frames, cap, 6] in front of counts[f] and gt_labels; (0, 0) when there is none.
    What dvid_vid_eval_match checks against num_classes before it launches."""
    cap = dets.shape[1]
    lab = dets[:, :, 5][torch.arange(cap, device=dets.device)[None, :] < counts[:, None]].to(torch.int64)
    if gt_labels is not None:
        lab = torch.cat((lab, gt_labels.reshape(-1).to(torch.int64)))
    if lab.numel() == 0:
        return 0, 0
    lo, hi = torch.stack((lab.amin(), lab.amax())).tolist()
    return int(lo), int(hi)


def vid_eval_match(dets, counts, gt_boxes, gt_labels, gt_starts, num_classes, motion=None, ranges=((0.0, 1.0),), empty_w=None, iou_thresh=0.5,
                   label_range=None, out=None):
    """The VID evaluator's greedy matching (vid_eval.calc_prec_rec's loop) and CorLoc test for all motion ranges in one launch
    (csrc/videval.hip).  dets [F, cap, 6] fp32 and counts [F] int32 in engine.pack_predictions' layout with the boxes in annotation
    pixels; gt_boxes [G, 4] fp32, gt_labels [G] int32, gt_starts [F + 1] int32: the ragged ground truth (vid_eval.pack_groundtruth);
    motion [G] float64 or None; ranges: R pairs (lo, hi); empty_w: R floats (default 0).  All tensors on the device.  Returns
    (match [R, F, cap] int8, weight [R, F, cap] float64, rank [F, cap] int32, n_pos [R, num_classes + 1] float64, top_row [F] int32,
    top_hit [F] int8) on the device (include/dvid_hip.h says what each holds); `out`: such a tuple to write into.  label_range: what
    vid_eval_label_range returns, when the caller has it already."""
    dets, counts = _cuda(dets, torch.float32), _cuda(counts, torch.int32)
    F, cap = counts.shape[0], dets.shape[1] if dets.dim() == 3 else -1
    assert dets.shape == (F, cap, 6), "dets is [frames, cap, 6]"
    dev = dets.device
    rng = torch.tensor([[float(lo), float(hi)] for lo, hi in ranges], dtype=torch.float64).reshape(-1, 2)
    R = rng.shape[0]
    ew = torch.zeros((R,), dtype=torch.float64) if empty_w is None else torch.tensor([float(w) for w in empty_w], dtype=torch.float64)
    assert ew.numel() == R and num_classes >= 1, "one empty_w per range"
    if out is None:
        out = (torch.empty((R, F, cap), dtype=torch.int8, device=dev), torch.empty((R, F, cap), dtype=torch.float64, device=dev),
               torch.empty((F, cap), dtype=torch.int32, device=dev), torch.zeros((R, num_classes + 1), dtype=torch.float64, device=dev),
               torch.empty((F,), dtype=torch.int32, device=dev), torch.empty((F,), dtype=torch.int8, device=dev))
    match, weight, rank, n_pos, top_row, top_hit = out
    assert match.shape == weight.shape == (R, F, cap) and rank.shape == (F, cap) and n_pos.shape == (R, num_classes + 1) and \
        top_row.shape == top_hit.shape == (F,), "output shapes"
    assert (match.dtype, weight.dtype, rank.dtype, n_pos.dtype, top_row.dtype, top_hit.dtype) == \
        (torch.int8, torch.float64, torch.int32, torch.float64, torch.int32, torch.int8), "output dtypes"
    if F == 0 or cap == 0:
        n_pos.zero_()
        return out
    gt_boxes, gt_labels, gt_starts = _cuda(gt_boxes, torch.float32).reshape(-1, 4), _cuda(gt_labels, torch.int32), _cuda(gt_starts, torch.int32)
    assert gt_starts.shape == (F + 1,) and gt_labels.shape[0] == gt_boxes.shape[0], "gt_starts is [frames + 1]"
    starts_host = gt_starts.cpu()
    assert int(starts_host[-1]) == gt_boxes.shape[0], "gt_starts ends at the box count"
    if motion is not None:
        motion = _cuda(motion, torch.float64)
        assert motion.shape == (gt_boxes.shape[0],), "one motion IoU per ground-truth box"
    lo, hi = label_range if label_range is not None else vid_eval_label_range(dets, counts, gt_labels)
    call("dvid_vid_eval_match", ptr(dets), ptr(counts), F, cap, ptr(gt_boxes), ptr(gt_labels), ptr(gt_starts), ptr(starts_host), int(lo), int(hi),
         ptr(motion), ptr(rng), ptr(ew), R, float(iou_thresh), int(num_classes), *(ptr(_cuda(o)) for o in out), stream_ptr())
    return out


COCO_EVAL_MAX_GT, COCO_EVAL_THRESHOLDS, COCO_EVAL_AREAS, COCO_EVAL_MAX_DETS = 256, 10, 4, 100          # include/dvid_hip.h


def _eval_match_tables(dets, counts, num_classes, iou_thrs, area_ranges, out):
    """what coco_eval_match and lvis_eval_match do alike in front of the ground truth -> (dets, counts, thr, rng, out): the casts, the
    threshold and range tables on the host, and the (match, ignore, rank, npig) tuple, made or checked"""
    dets, counts = _cuda(dets, torch.float32), _cuda(counts, torch.int32)
    N, cap = counts.shape[0], dets.shape[1] if dets.dim() == 3 else -1
    assert dets.shape == (N, cap, 6), "dets is [images, cap, 6]"
    dev = dets.device
    A, T = COCO_EVAL_AREAS, COCO_EVAL_THRESHOLDS
    thr = torch.tensor([float(t) for t in iou_thrs], dtype=torch.float64)
    rng = torch.tensor([[float(lo), float(hi)] for lo, hi in area_ranges], dtype=torch.float64).reshape(-1, 2)
    assert thr.shape == (T,) and rng.shape == (A, 2) and num_classes >= 1, "ten thresholds and four area ranges"
    if out is None:
        out = (torch.empty((A, T, N, cap), dtype=torch.int8, device=dev), torch.empty((A, T, N, cap), dtype=torch.int8, device=dev),
               torch.empty((N, cap), dtype=torch.int32, device=dev), torch.zeros((A, num_classes + 1), dtype=torch.int32, device=dev))
    match, ignore, rank, npig = out
    assert match.shape == ignore.shape == (A, T, N, cap) and rank.shape == (N, cap) and npig.shape == (A, num_classes + 1), "output shapes"
    assert (match.dtype, ignore.dtype, rank.dtype, npig.dtype) == (torch.int8, torch.int8, torch.int32, torch.int32), "output dtypes"
    return dets, counts, thr, rng, out


def _eval_match_groundtruth(N, gt_boxes, gt_areas, gt_flag, gt_labels, gt_starts):
    """the five ground-truth tensors of N images, cast and checked, and gt_starts on the host"""
    gt_boxes, gt_areas = _cuda(gt_boxes, torch.float64).reshape(-1, 4), _cuda(gt_areas, torch.float64)
    gt_flag, gt_labels, gt_starts = _cuda(gt_flag, torch.uint8), _cuda(gt_labels, torch.int32), _cuda(gt_starts, torch.int32)
    G = gt_boxes.shape[0]
    assert gt_starts.shape == (N + 1,) and gt_areas.shape == gt_flag.shape == gt_labels.shape == (G,), "gt_starts is [images + 1]"
    starts_host = gt_starts.cpu()
    assert int(starts_host[-1]) == G, "gt_starts ends at the box count"
    return gt_boxes, gt_areas, gt_flag, gt_labels, gt_starts, starts_host


def coco_eval_match(dets, counts, gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts, num_classes, iou_thrs, area_ranges, out=None):
    """The COCO bbox evaluator's matching (coco_eval.evaluate_numpy's loop) for the ten IoU thresholds and the four area ranges in one
    launch (csrc/cocoeval.hip).  dets [N, cap, 6] fp32 and counts [N] int32 in engine.pack_predictions' layout with the boxes in
    annotation pixels; gt_boxes [G, 4] float64 xywh, gt_areas [G] float64, gt_crowd [G] uint8, gt_labels [G] int32, gt_starts [N + 1]
    int32: the ragged ground truth (coco_eval.pack_groundtruth).  All tensors on the device.  iou_thrs: 10 floats, area_ranges: 4 pairs
    (lo, hi), taken as float64.  Returns (match [4, 10, N, cap] int8, ignore [4, 10, N, cap] int8, rank [N, cap] int32, npig
    [4, num_classes + 1] int32) on the device (include/dvid_hip.h says what each holds); `out`: such a tuple to write into.  The scores
    must be finite."""
    dets, counts, thr, rng, out = _eval_match_tables(dets, counts, num_classes, iou_thrs, area_ranges, out)
    N, cap = dets.shape[:2]
    if N == 0 or cap == 0:
        out[3].zero_()
        return out
    gt = _eval_match_groundtruth(N, gt_boxes, gt_areas, gt_crowd, gt_labels, gt_starts)
    call("dvid_coco_eval_match", ptr(dets), ptr(counts), N, cap, *(ptr(t) for t in gt), ptr(thr), ptr(rng), int(num_classes),
         *(ptr(_cuda(o)) for o in out), stream_ptr())
    return out


LVIS_EVAL_MAX_GT, LVIS_EVAL_MAX_DETS = 1024, 300          # include/dvid_hip.h


def lvis_eval_match(dets, counts, gt_boxes, gt_areas, gt_ignore, gt_labels, gt_starts, neg_starts, neg_labels, nex_starts, nex_labels,
                    num_classes, iou_thrs, area_ranges, out=None):
    """The LVIS bbox evaluator's matching (lvis_eval.match_numpy, the federated protocol) for the ten IoU thresholds and the four area
    ranges in one launch (csrc/lviseval.hip).  dets, counts, gt_boxes, gt_areas, gt_labels, gt_starts, iou_thrs, area_ranges and the
    returned (match, ignore, rank, npig) are coco_eval_match's; gt_ignore [G] uint8 is the annotation's `ignore`; neg_starts [N + 1] int32
    with neg_labels and nex_starts [N + 1] int32 with nex_labels are the images' negative and not-exhaustive label lists as CSR tables
    (lvis_eval.pack_groundtruth).  All tensors on the device.  The scores must be finite."""
    dets, counts, thr, rng, out = _eval_match_tables(dets, counts, num_classes, iou_thrs, area_ranges, out)
    N, cap = dets.shape[:2]
    if N == 0 or cap == 0:
        out[3].zero_()
        return out
    gt = _eval_match_groundtruth(N, gt_boxes, gt_areas, gt_ignore, gt_labels, gt_starts)
    lists = []
    for name, starts, labels in (("neg", neg_starts, neg_labels), ("nex", nex_starts, nex_labels)):
        starts, labels = _cuda(starts, torch.int32), _cuda(labels, torch.int32).reshape(-1)
        assert starts.shape == (N + 1,), "%s_starts is [images + 1]" % name
        host = starts.cpu()
        assert int(host[-1]) == labels.shape[0], "%s_starts ends at the length of %s_labels" % (name, name)
        lists += [starts, labels, host]
    call("dvid_lvis_eval_match", ptr(dets), ptr(counts), N, cap, *(ptr(t) for t in gt), *(ptr(t) for t in lists), ptr(thr), ptr(rng),
         int(num_classes), *(ptr(_cuda(o)) for o in out), stream_ptr())
    return out


EVAL_ACCUMULATE_RECALLS, EVAL_ACCUMULATE_MAX_LIMITS, EVAL_ACCUMULATE_MAX_SCRATCH_BYTES = 101, 3, 1 << 30          # include/dvid_hip.h


def eval_accumulate(dets, counts, rank, match, ignore, npig, max_dets, rec_thrs, out=None):
    """The COCO / LVIS evaluators' accumulation (coco_eval.accumulate_arrays) on the device, with that function's bits
    (csrc/evalaccum.hip).  dets [N, cap, 6] fp32 and counts [N] int32 as the matching read them, (match [4, 10, N, cap] int8, ignore
    [4, 10, N, cap] int8, rank [N, cap] int32, npig [4, K + 1] int32) as coco_eval_match / lvis_eval_match return them, all on the
    device; max_dets: 1 .. 3 ascending limits; rec_thrs: 101 floats, taken as float64.  Returns (precision [10, 101, K, 4, M] float64,
    recall [10, K, 4, M] float64) on the device; `out`: such a pair to write into.  The scores must be finite."""
    dets, counts, rank = _cuda(dets, torch.float32), _cuda(counts, torch.int32), _cuda(rank, torch.int32)
    match, ignore, npig = _cuda(match, torch.int8), _cuda(ignore, torch.int8), _cuda(npig, torch.int32)
    N, cap = counts.shape[0], dets.shape[1] if dets.dim() == 3 else -1
    assert dets.shape == (N, cap, 6) and rank.shape == (N, cap), "dets is [images, cap, 6], rank [images, cap]"
    assert match.dim() == 4 and match.shape == ignore.shape and match.shape[2:] == (N, cap), "match and ignore are [areas, thresholds, images, cap]"
    A, T = match.shape[:2]
    assert npig.dim() == 2 and npig.shape[0] == A and npig.shape[1] >= 2, "npig is [areas, classes + 1]"
    K = npig.shape[1] - 1
    lim = torch.tensor([int(m) for m in max_dets], dtype=torch.int32)
    thr = torch.tensor([float(r) for r in rec_thrs], dtype=torch.float64)
    M, R = lim.numel(), thr.numel()
    dev = dets.device
    if out is None:
        out = (torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev), torch.empty((T, K, A, M), dtype=torch.float64, device=dev))
    precision, recall = out
    assert precision.shape == (T, R, K, A, M) and recall.shape == (T, K, A, M), "output shapes"
    assert precision.dtype == recall.dtype == torch.float64 and precision.is_contiguous() and recall.is_contiguous(), "outputs are contiguous float64"
    if N == 0 or cap == 0:
        N, cap = 0, 1          # no row at all: the counted categories get 0
    need = int(_lib.load().dvid_eval_accumulate_scratch_bytes(N, cap, M))
    scratch = torch.empty((max(16, need),), dtype=torch.uint8, device=dev) if 0 <= need <= EVAL_ACCUMULATE_MAX_SCRATCH_BYTES else None
    call("dvid_eval_accumulate", ptr(dets), ptr(counts), ptr(rank), ptr(match), ptr(ignore), ptr(npig), N, cap, K, A, T, ptr(lim), M, ptr(thr), R,
         ptr(_cuda(precision)), ptr(_cuda(recall)), ptr(scratch), need if scratch is not None else 0, stream_ptr())
    return out


def split_detection_buffer(buf, n, cap):
    """The four post-processing outputs are views of ONE flat fp32 buffer [boxes | scores | labels(int32) |
    counts(int32)], so a caller can bring a whole batch to the host with a single D2H copy
    (`split_detection_buffer(ob.untyped... ` see DiffusionDet._to_boxlists)."""
    a, b = n * cap * 4, n * cap * 5
    ob = buf[:a].view(n, cap, 4)
    osc = buf[a:b].view(n, cap)
    ol = buf[b:b + n * cap].view(torch.int32).view(n, cap)
    oc = buf[b + n * cap:b + n * cap + n].view(torch.int32)
    ob._dvid_flat = buf            # keep the flat buffer reachable from the first view
    return ob, osc, ol, oc


def cdist(x):
    x = _cuda(x, torch.float32)
    n, d = x.shape
    out = torch.empty((n, n), dtype=torch.float32, device=x.device)
    call("dvid_cdist", ptr(x), n, d, ptr(out), stream_ptr())
    return out


def fps_greedy(dist, m, bs_emul=0):
    dist = _cuda(dist, torch.float32)
    n = dist.shape[0]
    idx = torch.empty((m,), dtype=torch.int32, device=dist.device)
    call("dvid_fps_greedy", ptr(dist), n, m, bs_emul, ptr(idx), stream_ptr())
    return idx


def gather_rows(x, idx):
    x = _cuda(x, torch.float32)
    idx = _cuda(idx, torch.int32)
    out = torch.empty((idx.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    call("dvid_gather_rows", ptr(x), ptr(idx), ptr(out), idx.shape[0], x.shape[1], stream_ptr())
    return out


def update_erase_memory(feats_new, feats_mem, target_size):
    """diffusion_det.py:841-867 on device: cat -> (cdist -> greedy FPS -> gather) if over target."""
    merged = feats_new if feats_mem is None else torch.cat([feats_mem, feats_new], dim=0)
    merged = merged.contiguous()
    if merged.shape[0] <= target_size:
        return merged, None
    idx = fps_greedy(cdist(merged), target_size)
    return gather_rows(merged, idx), idx


# ---- the grouped forms: G independent problems of one shape per launch, each computed as the single form computes it ----
UPDATE_MEMORY_MAX_SCRATCH_BYTES = 1 << 30          # DVID_UPDATE_MEMORY_MAX_SCRATCH_BYTES of include/dvid_hip.h


def cdist_groups(x):
    """x [G, n, d] -> [G, n, n]: group g bit-equal to cdist(x[g])"""
    x = _cuda(x, torch.float32)
    G, n, d = x.shape
    need = G * n * n * 4
    out = torch.empty((G, n, n) if need <= UPDATE_MEMORY_MAX_SCRATCH_BYTES else (0,), dtype=torch.float32, device=x.device)          # over the limit: the library refuses before it writes
    call("dvid_cdist_groups", ptr(x), G, n, d, ptr(out), stream_ptr())
    return out


def fps_greedy_groups(dist, m, bs_emul=0):
    """dist [G, n, n] -> int32 [G, m]: the picks of fps_greedy(dist[g], m), the G sweeps side by side (one workgroup each)"""
    dist = _cuda(dist, torch.float32)
    G, n = dist.shape[:2]
    idx = torch.empty((G, m), dtype=torch.int32, device=dist.device)
    call("dvid_fps_greedy_groups", ptr(dist), G, n, m, bs_emul, ptr(idx), stream_ptr())
    return idx


def gather_rows_groups(x, idx, out=None):
    """out[g, r, :] = x[g, idx[g, r], :]; x [G, n, d], idx int32 [G, m] -> [G, m, d] (written into `out` when one is given)"""
    x = _cuda(x, torch.float32)
    idx = _cuda(idx, torch.int32)
    G, n, d = x.shape
    m = idx.shape[1]
    if out is None:
        out = torch.empty((G, m, d), dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and tuple(out.shape) == (G, m, d) and out.dtype == torch.float32
    call("dvid_gather_rows_groups", ptr(x), ptr(idx), ptr(out), G, n, m, d, stream_ptr())
    return out


def update_erase_memory_groups(feats_new, feats_mem, target_size, out=None):
    """update_erase_memory for G memories of one shape at once: feats_new [G, k, d], feats_mem [G, r, d] or None -> (memory
    [G, min(r + k, target), d], idx int32 [G, target] or None), group g bit-equal to update_erase_memory(feats_new[g], feats_mem[g], target).
    Rows in update_erase_memory's order: the memory's first, the new ones behind.  r + k <= target: the concatenation, nothing launched.
    `out` [G, target, d]: the pruned memories are written there (it may be `feats_mem` itself: the merged rows are a copy)."""
    if feats_new.dim() != 3 or (feats_mem is not None and (feats_mem.dim() != 3 or feats_mem.shape[0] != feats_new.shape[0] or feats_mem.shape[2] != feats_new.shape[2])):
        raise _lib.DvidError(f"update_erase_memory_groups takes feats_new [G, k, d] and feats_mem [G, r, d], got {tuple(feats_new.shape)} and "
                             f"{None if feats_mem is None else tuple(feats_mem.shape)}")
    merged = _cuda(feats_new if feats_mem is None else torch.cat([feats_mem, feats_new], dim=1), torch.float32)
    G, n, d = merged.shape
    if n <= target_size:
        return merged, None
    need = G * n * n * 4
    scratch = torch.empty((G, n, n) if need <= UPDATE_MEMORY_MAX_SCRATCH_BYTES else (0,), dtype=torch.float32, device=merged.device)
    idx = torch.empty((G, target_size), dtype=torch.int32, device=merged.device)
    if out is None:
        out = torch.empty((G, target_size, d), dtype=torch.float32, device=merged.device)
    assert out.is_contiguous() and tuple(out.shape) == (G, target_size, d) and out.dtype == torch.float32
    call("dvid_update_memory_groups", ptr(merged), G, n, d, target_size, ptr(scratch), ptr(idx), ptr(out), stream_ptr())
    return out, idx


def set_option(name, value):
    """one entry of the library's option table (include/dvid_hip.h: dvid_set_option; csrc/options.h lists names and defaults)"""
    call("dvid_set_option", name.encode(), int(value))


def get_option(name):
    v = C.c_int()
    call("dvid_get_option", name.encode(), C.byref(v))
    return v.value


def reset_options():
    call("dvid_reset_options")


def effective_config():
    """"name=value ..." of every library option + the environment variables the library still reads (dvid_effective_config)"""
    buf = C.create_string_buffer(1024)
    call("dvid_effective_config", buf, 1024)
    return buf.value.decode()




PRECISIONS = {"float16": 0, "float32": 1}          # the reference's DTYPE values (mega_core/config/defaults.py:582) -> dvid_model_set_precision


class Model:
    """Owns a dvid_model handle: repacked weights + activation workspace on the current device."""

    def __init__(self, state_dict, *, hidden_dim=256, nheads=8, dim_feedforward=2048, dim_dynamic=64, num_classes=30,
                 num_cls=1, num_reg=3, num_heads=3, num_heads_cond=1, pooler_resolution=7, sampling_ratio=2,
                 res_blocks=(3, 4, 23, 3), pixel_mean=(123.675, 116.280, 103.530), pixel_std=(58.395, 57.120, 57.375),
                 backbone="resnet", swin_embed_dim=128, swin_depths=(2, 2, 18, 2), swin_heads=(4, 8, 16, 32), swin_window=7,
                 precision="float16"):
        """precision: the reference's DTYPE key -- "float16" (fp16 storage, fp16 MFMA, fp32 accumulation) or "float32" (fp32 storage,
        fp32 MFMA; csrc/f32.hip).  Feature maps are fp16 / fp32 NHWC tensors accordingly."""
        if precision not in PRECISIONS:
            raise _lib.DvidError(f"precision must be one of {sorted(PRECISIONS)} (the reference's DTYPE), got {precision!r}")
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.DvidError("no HIP device visible: the DiffusionVID hot path runs only on the GPU (no CPU fallback)")
        cfg = _lib.DvidConfig(hidden_dim, nheads, dim_feedforward, dim_dynamic, num_classes, num_cls, num_reg, num_heads,
                              num_heads_cond, pooler_resolution, sampling_ratio, (C.c_int * 4)(*res_blocks),
                              (C.c_float * 3)(*pixel_mean), (C.c_float * 3)(*pixel_std),
                              1 if backbone == "swin" else 0, swin_embed_dim, (C.c_int * 4)(*swin_depths),
                              (C.c_int * 4)(*swin_heads), swin_window)
        self.backbone_kind = backbone
        self.cfg = cfg
        self.precision = precision
        self.feat_dtype = torch.float32 if precision == "float32" else torch.float16
        h = C.c_void_p()
        _lib.check(lib.dvid_model_create(C.byref(cfg), C.byref(h)), "dvid_model_create")
        self.handle = h
        _lib.check(lib.dvid_model_set_precision(h, PRECISIONS[precision]), "dvid_model_set_precision")
        self.hidden_dim, self.num_classes, self.nheads = hidden_dim, num_classes, nheads
        self.has_backbone = (swin_depths[0] > 0) if backbone == "swin" else (res_blocks[0] > 0)
        wanted = ("head.", "backbone.") if self.has_backbone else ("head.",)
        for name, t in state_dict.items():
            if not name.startswith(wanted) or not torch.is_floating_point(t):
                continue
            t = t.detach().to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            _lib.check(lib.dvid_model_set_tensor(h, name.encode(), t.data_ptr(), shape, t.dim()), f"set_tensor({name})")
        _lib.check(lib.dvid_model_finalize(h), "dvid_model_finalize")
        self._ws = None
        self.chains = -1                 # the library's default until set_chains
        # local box-level attention: present when the state dict carries it (the library infers the same from the tensors it was given)
        self.local_stages = 0
        while f"head.local_attention.{self.local_stages}.0.in_proj_weight" in state_dict:
            self.local_stages += 1
        # the pyramid: four levels (p2..p5) when the state dict carries the stride-4 lateral, as the library infers it; a head-only model
        # takes what rcnn_head is given
        self.fpn_levels = 4 if self.has_backbone and "backbone.fpn_lateral2.weight" in state_dict else 3
        # what the library's three projected memories hold: "video" | "groups" | "local" -> (memory tensor, its version, shape key)
        self._projected = {}

    def take_range_flag(self):
        """DTYPE float32 with split operands: True if a launch since the last call met an activation beyond the fp16 range (65504); synchronises
        the current stream and clears the flag (include/dvid_hip.h: dvid_model_take_range_flag).  Always False for float16."""
        if self.precision != "float32":
            return False
        v = C.c_int(0)
        call("dvid_model_take_range_flag", self.handle, C.byref(v), stream_ptr())
        return bool(v.value)

    def workspace_generation(self):
        """moves of this model's workspace buffers so far (include/dvid_hip.h: dvid_workspace_generation); a captured launch sequence is
        valid only while this stays what it was at capture time"""
        return int(_lib.load().dvid_workspace_generation(self.handle))

    def set_chains(self, n):
        """concurrent sub-batch chains inside the library (1 = sequential kernels, for per-kernel profiling)"""
        call("dvid_set_chains", self.handle, int(n))
        self.chains = int(n)

    def set_stem_layout(self, space_to_depth=True):
        """ResNet stem over the 2x2 space-to-depth image (default) or the NHWC8 image; see dvid_set_stem_layout"""
        call("dvid_set_stem_layout", self.handle, int(bool(space_to_depth)))

    def reserve(self, max_frames, height, width, boxes_per_frame):
        """Workspace for up to max_frames frames of height x width with boxes_per_frame boxes; only ever grows."""
        key = (max_frames, height, width, boxes_per_frame)
        if self._ws is not None:
            key = tuple(max(a, b) for a, b in zip(key, self._ws))
        if self._ws != key:
            call("dvid_workspace_reserve", self.handle, *key)
            self._ws = key

    def backbone(self, images, frames_per_launch=None):
        """images fp32 NCHW [n,3,H,W] in [0,1] -> [p3, p4, p5], or [p2, p3, p4, p5] for a model with the p2 level, fp16 (precision float32:
        fp32) NHWC.  frames_per_launch: run the n frames as consecutive launch sequences of at most that many frames (same results;
        smaller activation working set)."""
        images = _cuda(images, torch.float32)
        n, _, h, w = images.shape
        dev = images.device
        outs = self._empty_pyramid(n, h, w, dev)
        fn = "dvid_backbone_swin_fpn_levels_frames" if self.backbone_kind == "swin" else "dvid_backbone_resnet_fpn_levels_frames"
        step = n if not frames_per_launch else max(1, min(n, int(frames_per_launch)))
        for a in range(0, n, step):
            b = min(n, a + step)
            table = (C.c_void_p * (b - a))(*[images[i].data_ptr() for i in range(a, b)])
            levels = (C.c_void_p * len(outs))(*[ptr(o[a:b]) for o in outs])
            call(fn, self.handle, table, b - a, h, w, levels, len(outs), stream_ptr())
        return outs

    def _empty_pyramid(self, n, h, w, dev):
        return [torch.empty((n, h >> s, w >> s, self.hidden_dim), dtype=self.feat_dtype, device=dev) for s in range(6 - self.fpn_levels, 6)]

    def backbone_frames(self, frames):
        """The same over a LIST of per-frame tensors, each fp32 [1, 3, H, W] (or [3, H, W]) on the device, all of one size: the
        kernels read every frame where it lies (a table of pointers), no concatenated copy is made
        (diffusion_det.py:418-421 concatenates)."""
        first = frames[0]
        h, w = first.shape[-2:]
        keep = []
        for f in frames:
            if not f.is_cuda or f.dtype != torch.float32 or f.shape[-2:] != (h, w) or f.shape[-3] != 3 or f.numel() != 3 * h * w:
                raise _lib.DvidError("backbone_frames: frames must be fp32 [1, 3, H, W] device tensors of one size")
            keep.append(f if f.is_contiguous() else f.contiguous())
        n = len(keep)
        dev = first.device
        outs = self._empty_pyramid(n, h, w, dev)
        table = (C.c_void_p * n)(*[f.data_ptr() for f in keep])
        levels = (C.c_void_p * len(outs))(*[ptr(o) for o in outs])
        fn = "dvid_backbone_swin_fpn_levels_frames" if self.backbone_kind == "swin" else "dvid_backbone_resnet_fpn_levels_frames"
        call(fn, self.handle, table, n, h, w, levels, len(outs), stream_ptr())
        return outs          # `keep` may die here: the stream-ordered caching allocator re-uses a frame's block only behind this stream's reads

    def rcnn_head(self, head_index, feats_nhwc, height, width, boxes, pro_features, t, cond=None, bad_flag=None, keep_tail_input=False,
                  keep_interact_input=False):
        """One RCNNHead / RCNNHead_cond pass over the maps it is given, [p3, p4, p5] or [p2, p3, p4, p5].  boxes [n, M, 4]; pro_features
        [n*M, d] or None; t: int64 [n] (CPU).  keep_tail_input=True (DTYPE float32 models only): a fourth return value, the tail's input
        -- the fp32 norm2 output [n*M, d] that head_tail_backward takes as x (dvid_rcnn_head_levels_keep); the other three keep their bits.
        keep_interact_input=True (float32 models only): two more return values behind those, what inst_interact_backward takes as p and roi
        -- the fp32 norm1 output [n*M, d] and the fp32 RoI tiles [n*M, 49, d] (dvid_rcnn_head_levels_keep2); the others keep their bits."""
        if keep_tail_input and self.precision != "float32":
            raise _lib.DvidError(f"rcnn_head: keep_tail_input needs a DTYPE float32 model, this one is {self.precision} (fp16 gradients are out of scope)")
        if keep_interact_input and self.precision != "float32":
            raise _lib.DvidError(f"rcnn_head: keep_interact_input needs a DTYPE float32 model, this one is {self.precision} (fp16 gradients are out of scope)")
        boxes = _cuda(boxes, torch.float32)
        n, M = boxes.shape[:2]
        dev = boxes.device
        d = self.hidden_dim
        for f in feats_nhwc:          # the library reads them as the model's precision says: a mismatch would be silent garbage
            if f.dtype != self.feat_dtype or not f.is_contiguous():
                raise _lib.DvidError(f"rcnn_head: feature maps must be contiguous {self.feat_dtype} NHWC tensors for precision {self.precision}")
        logits = torch.empty((n, M, self.num_classes), dtype=torch.float32, device=dev)
        boxes_out = torch.empty((n, M, 4), dtype=torch.float32, device=dev)
        obj = torch.empty((n * M, d), dtype=torch.float32, device=dev)
        t = torch.as_tensor(t, dtype=torch.int64, device="cpu").contiguous()
        assert t.numel() == n
        tp = C.cast(t.data_ptr(), C.POINTER(C.c_int64))
        if pro_features is not None:
            pro_features = _cuda(pro_features, torch.float32)
        if cond is not None:
            cond = _cuda(cond, torch.float32)
        levels, nl = _pyramid(feats_nhwc, height, width, "rcnn_head")
        if keep_interact_input:
            tail_in = torch.empty((n * M, d), dtype=torch.float32, device=dev) if keep_tail_input else None
            inter_in = torch.empty((n * M, d), dtype=torch.float32, device=dev)
            tiles = torch.empty((n * M, 49, d), dtype=torch.float32, device=dev)
            call("dvid_rcnn_head_levels_keep2", self.handle, head_index, int(cond is not None), levels, nl, n, height, width, M, ptr(boxes),
                 ptr(pro_features), tp, ptr(cond), ptr(logits), ptr(boxes_out), ptr(obj), ptr(bad_flag), ptr(tail_in), ptr(inter_in), ptr(tiles), stream_ptr())
            return (logits, boxes_out, obj) + ((tail_in,) if keep_tail_input else ()) + (inter_in, tiles)
        if keep_tail_input:
            tail_in = torch.empty((n * M, d), dtype=torch.float32, device=dev)
            call("dvid_rcnn_head_levels_keep", self.handle, head_index, int(cond is not None), levels, nl, n, height, width, M, ptr(boxes),
                 ptr(pro_features), tp, ptr(cond), ptr(logits), ptr(boxes_out), ptr(obj), ptr(bad_flag), ptr(tail_in), stream_ptr())
            return logits, boxes_out, obj, tail_in
        call("dvid_rcnn_head_levels", self.handle, head_index, int(cond is not None), levels, nl, n, height, width, M, ptr(boxes),
             ptr(pro_features), tp, ptr(cond), ptr(logits), ptr(boxes_out), ptr(obj), ptr(bad_flag), stream_ptr())
        return logits, boxes_out, obj

    def _project_unless_current(self, which, memory, key, project):
        """THE cache rule of the three projected memories (`which`: "video", "groups" or "local"): the library's K / V rows are current when
        they came from this tensor object at this version counter with this shape key; otherwise `project(memory as fp32 device tensor)`
        runs.  The entry is dropped before the call, so a call that fails leaves nothing that points at rows never written, and it holds
        the tensor afterwards, so the storage cannot be recycled under the cache."""
        hit = self._projected.get(which)
        if hit is None or hit[0] is not memory or hit[1] != memory._version or hit[2] != key:
            self._projected.pop(which, None)
            project(_cuda(memory, torch.float32))
            self._projected[which] = (memory, memory._version, key)

    def invalidate_memory(self):
        """The global memory changed (new video, memory update, adopted memory, or an in-place write through a raw pointer,
        which no tensor version counter sees): the next global_xattn projects K/V again."""
        self._projected.pop("video", None)

    def ensure_memory_projected(self, memory):
        """K / V projections of `memory` into the engine's buffers unless they are current (_project_unless_current).
        global_xattn calls it; a captured launch sequence that READS those buffers (DiffusionDet._graphed_call) calls it before
        every replay, because the projection itself is not part of the capture."""
        self._project_unless_current("video", memory, tuple(memory.shape), lambda mem: call(
            "dvid_global_memory_project", self.handle, ptr(mem), mem.shape[0], stream_ptr()))

    def global_xattn(self, query, memory):
        """cond = MHA(query, memory, memory).  The K/V projections of `memory` are kept until `invalidate_memory()` (the
        detector calls it wherever it assigns the memory) or until another tensor object is passed, i.e. they are computed
        once per memory update of a video.  The cache key is (tensor object, its version counter, its shape): an in-place torch
        write to the memory (copy_, index_put_, ...) bumps the counter and projects again; a write through a raw pointer, which
        no counter sees, needs `invalidate_memory()`."""
        query = _cuda(query, torch.float32)
        self.ensure_memory_projected(memory)
        out = torch.empty_like(query)
        call("dvid_global_xattn", self.handle, ptr(query), query.shape[0], None, memory.shape[0], ptr(out), stream_ptr())
        return out

    def invalidate_memory_groups(self):
        """The grouped global memories changed behind the cache's back (a write through a raw pointer: update_erase_memory_groups writing
        a set's memories in place): the next global_xattn_groups projects K/V again.  The video's projection is not touched."""
        self._projected.pop("groups", None)

    def ensure_memory_groups_projected(self, memory):
        """K / V projections of G global memories (memory [G, lk, d], one per live stream) into the engine's buffer for them unless
        they are current (_project_unless_current).  That buffer is separate from the one ensure_memory_projected fills, so a video's
        cached projection survives."""
        self._project_unless_current("groups", memory, tuple(memory.shape), lambda mem: call(
            "dvid_global_memory_project_groups", self.handle, ptr(mem), mem.shape[1], mem.shape[0], stream_ptr()))

    def global_xattn_groups(self, query, memory):
        """cond = MHA(query, memory[g], memory[g]) per group: query [rows, d] is G consecutive blocks of rows / G, memory [G, lk, d]; block
        g attends memory g, bit-equal to global_xattn(block g, memory[g]).  K/V are projected once per (memory object, version, shape);
        an in-place write no version counter sees needs invalidate_memory_groups()."""
        query = _cuda(query, torch.float32)
        if memory.dim() != 3 or query.shape[0] % memory.shape[0]:
            raise _lib.DvidError(f"global_xattn_groups: {query.shape[0]} query rows against memories of shape {tuple(memory.shape)} ([G, lk, d])")
        self.ensure_memory_groups_projected(memory)
        out = torch.empty_like(query)
        call("dvid_global_xattn_groups", self.handle, ptr(query), query.shape[0], memory.shape[0], memory.shape[1], ptr(out), stream_ptr())
        return out

    def invalidate_local_memory(self):
        """The local memory changed behind the cache's back (a write through a raw pointer, e.g. a replayed launch sequence): the next
        local_xattn projects K/V again."""
        self._projected.pop("local", None)

    def ensure_local_memory_projected(self, memory, groups=1, stage=None):
        """K / V projections of `groups` local memories (memory [groups * lk, d], group g = rows [g lk, (g + 1) lk)) into the engine's
        buffer unless they are current (_project_unless_current; the stage and the grouping are part of the key).  The library keeps ONE
        projected local memory, so projecting a stage drops the others."""
        stage = self.local_stages - 1 if stage is None else int(stage)
        if memory.shape[0] % groups:
            raise _lib.DvidError(f"local memory of {memory.shape[0]} rows does not split into {groups} groups")
        self._project_unless_current("local", memory, (stage, int(groups), tuple(memory.shape)), lambda mem: call(
            "dvid_local_memory_project", self.handle, stage, ptr(mem), mem.shape[0] // groups, int(groups), stream_ptr()))

    def local_xattn(self, query, memory, groups=1, stage=None):
        """cond = LayerNorm(MHA(query, memory, memory)) of the local box-level stage `stage` (default and only legal value: the last one,
        the only observable one -- box_head.py:360-363).  query [rows, d] and memory [groups * lk, d] are `groups` consecutive blocks:
        block g of the queries attends block g of the memory (every look-ahead batch has its own local memory).  K/V are projected
        once per (memory object, version, groups), see ensure_local_memory_projected / invalidate_local_memory."""
        stage = self.local_stages - 1 if stage is None else int(stage)
        query = _cuda(query, torch.float32)
        if query.shape[0] % groups:
            raise _lib.DvidError(f"{query.shape[0]} query rows do not split into {groups} groups")
        self.ensure_local_memory_projected(memory, groups, stage)
        out = torch.empty_like(query)
        call("dvid_local_xattn", self.handle, stage, ptr(query), query.shape[0], int(groups), memory.shape[0] // groups, ptr(out), stream_ptr())
        return out

    def close(self):
        if getattr(self, "handle", None):
            _lib.load().dvid_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the forward of the training objective (csrc/criterion.hip; the host mirror is modeling/roi_heads/box_head/loss.py) -----------------
CRITERION_MAX_GT, CRITERION_MAX_ROWS, CRITERION_MAX_OTA_K, CRITERION_REPAIR_SLACK = 256, 4096, 64, 32          # include/dvid_hip.h
CRITERION_ERR_ROUNDS, CRITERION_ERR_DEGENERATE, CRITERION_ERR_NONFINITE, CRITERION_ERR_LABEL = 1, 2, 4, 8


def q_sample_boxes(gt_cxcywh, gt_starts, t, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, noise, placeholder, snr_scale, sizes):
    """The noisy boxes of a labelled batch in one launch (dvid_q_sample_boxes: the reference's prepare_diffusion_concat + q_sample and the
    scaling by (w, h, w, h)).  gt_cxcywh [G, 4] fp32 normalised (cx, cy, w, h) and gt_starts [n + 1] int32: the ragged ground truth;
    t [n] integer time steps (the caller's draw, any device; read on the host for the range check); the two schedule tables [T] fp32;
    noise and placeholder [n, M, 4] fp32 (the caller's draws); sizes: [n, 2] (w, h) or a FrameSizes.  -> absolute xyxy boxes [n, M, 4].
    An image with more than M boxes is refused (the reference's random subset is not built)."""
    noise, placeholder = _cuda(noise, torch.float32), _cuda(placeholder, torch.float32)
    if noise.dim() != 3 or noise.shape[-1] != 4 or placeholder.shape != noise.shape:
        raise _lib.DvidError(f"q_sample_boxes takes noise and placeholder [n, M, 4], got {tuple(noise.shape)} and {tuple(placeholder.shape)}")
    n, M = noise.shape[:2]
    dev = noise.device
    starts_host = torch.as_tensor(gt_starts).detach().to("cpu", torch.int32).contiguous()
    t_host = torch.as_tensor(t).detach().to("cpu", torch.int32).contiguous()
    assert starts_host.shape == (n + 1,) and t_host.shape == (n,), "gt_starts is [n + 1], t is [n]"
    gt = _cuda(gt_cxcywh, torch.float32).reshape(-1, 4)
    assert int(starts_host[-1]) == gt.shape[0], "gt_starts ends at the box count"
    sa, so = _cuda(sqrt_alphas_cumprod, torch.float32), _cuda(sqrt_one_minus_alphas_cumprod, torch.float32)
    assert sa.dim() == 1 and sa.shape == so.shape, "the schedule tables are [T]"
    fs = frame_sizes(sizes, n, dev)
    out = torch.empty_like(noise)
    starts_dev, t_dev = starts_host.to(dev), t_host.to(dev)          # named: a temporary would be freed, and its block reused, before the call
    call("dvid_q_sample_boxes", ptr(gt), ptr(starts_dev), ptr(starts_host), n, M, ptr(t_dev), ptr(t_host), ptr(sa), ptr(so), sa.shape[0],
         ptr(noise), ptr(placeholder), float(snr_scale), ptr(fs), ptr(out), stream_ptr())
    return out


HEAD_TAIL_BWD_ROW_CHUNK = 256          # DVID_HEAD_TAIL_BWD_ROW_CHUNK: the rows of one partial of a sum over rows


def head_tail_backward_scratch_bytes(n, M, dff, num_classes, num_cls, num_reg, cond):
    """bytes of scratch dvid_head_tail_backward needs for n images of M boxes (-1: sizes it does not take)"""
    return int(_lib.load().dvid_head_tail_backward_scratch_bytes(int(n), int(M), int(dff), int(num_classes), int(num_cls), int(num_reg), int(bool(cond))))


def head_tail_backward(x, boxes_in, time_emb, params, cond=None, d_logits=None, d_boxes=None, d_obj=None, bbox_weights=(2.0, 2.0, 1.0, 1.0),
                       scale_clamp=None, forward_only=False):
    """The tail of an RCNNHead / RCNNHead_cond pass recomputed in fp32 and its gradient (dvid_head_tail_backward, csrc/headtail_bwd.hip;
    box_head.tail states the function).  x [R, 256] (the norm2 output, R = n * M image-major), boxes_in [R, 4], time_emb [n, 1024], cond
    [R, 256] or None, all fp32 on the device; params {name without the head's prefix: fp32 device tensor in the reference's layout}.
    Cotangents d_logits [R, C], d_boxes [R, 4], d_obj [R, 256]: None means zeros.  Returns a dict: the forward outputs "logits", "boxes",
    "obj", and -- unless forward_only -- "d_x", "d_time_emb", "d_cond" (None without cond) and "param_grads" {name: gradient}, every element
    written.  include/dvid_hip.h states the arithmetic (fp32 MFMA products, fixed-order sums without atomics: two runs give the same bits) and
    the conventions at the kinks."""
    from .modeling.roi_heads.box_head import tail as T
    x, boxes_in, time_emb = _cuda(x, torch.float32), _cuda(boxes_in, torch.float32), _cuda(time_emb, torch.float32)
    assert x.dim() == 2 and time_emb.dim() == 2 and time_emb.shape[0] >= 1 and x.shape[0] % time_emb.shape[0] == 0, "x is [n * M, d], time_emb [n, 4 d]"
    R, d = x.shape
    n = time_emb.shape[0]
    M = R // n
    assert boxes_in.shape == (R, 4) and time_emb.shape == (n, 4 * d), "boxes_in is [R, 4], time_emb [n, 4 d]"
    if cond is not None:
        cond = _cuda(cond, torch.float32)
        assert cond.shape == (R, d), "cond is [R, d]"
    num_cls, num_reg = T.tower_depths(params)
    names = T.param_names(num_cls, num_reg, cond is not None)
    plist = [None if k is None else _cuda(params[k].detach(), torch.float32) for k in names]
    dff, c = plist[0].shape[0], plist[10].shape[0]
    want = {"linear1.weight": (dff, d), "linear1.bias": (dff,), "linear2.weight": (d, dff), "linear2.bias": (d,), "block_time_mlp.1.weight":
            (d if cond is not None else 2 * d, 4 * d), "block_time_mlp.1.bias": (d if cond is not None else 2 * d,), "class_logits.weight": (c, d),
            "class_logits.bias": (c,), "bboxes_delta.weight": (4, d), "bboxes_delta.bias": (4,)}
    for k, t in zip(names, plist):
        if k is not None:
            shape = want.get(k, (d, d) if k.endswith("weight") and t.dim() == 2 else (d,))
            assert tuple(t.shape) == shape, "%s is %s, expected %s" % (k, tuple(t.shape), shape)
    dev = x.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"logits": new(R, c), "boxes": new(R, 4), "obj": new(R, d)}
    cot = [None if t is None else _cuda(t, torch.float32) for t in (d_logits, d_boxes, d_obj)]
    for t, shape in zip(cot, ((R, c), (R, 4), (R, d))):
        assert t is None or tuple(t.shape) == shape, "a cotangent has its output's shape"
    glist = []
    if forward_only:
        assert all(t is None for t in cot), "cotangents without a backward"
    else:
        out.update({"d_x": new(R, d), "d_time_emb": new(n, 4 * d), "d_cond": new(R, d) if cond is not None else None})
        glist = [None if t is None else torch.empty_like(t) for t in plist]
        out["param_grads"] = {k: g for k, g in zip(names, glist) if k is not None}
    table = lambda ts: (C.c_void_p * len(names))(*[None if t is None else t.data_ptr() for t in ts])
    ptable = table(plist)
    gtable = table(glist) if glist else None
    nbytes = head_tail_backward_scratch_bytes(n, M, dff, c, num_cls, num_reg, cond is not None)
    scratch = torch.empty((max(nbytes, 16) + 15) // 16 * 4, dtype=torch.float32, device=dev)
    call("dvid_head_tail_backward", ptr(x), ptr(boxes_in), ptr(time_emb), ptr(cond), n, M, d, dff, c, num_cls, num_reg, C.cast(ptable, C.c_void_p),
         len(names), *(float(w) for w in bbox_weights), float(T.SCALE_CLAMP if scale_clamp is None else scale_clamp), *(ptr(t) for t in cot),
         ptr(out["logits"]), ptr(out["boxes"]), ptr(out["obj"]), ptr(out.get("d_x")), ptr(out.get("d_time_emb")), ptr(out.get("d_cond")),
         None if gtable is None else C.cast(gtable, C.c_void_p), ptr(scratch), scratch.numel() * 4, stream_ptr())
    return out


INST_BWD_ROW_SLAB = 512          # DVID_INST_BWD_ROW_SLAB: the rows whose dynamic parameters and their gradient exist at a time


def inst_interact_backward_scratch_bytes(R):
    """bytes of scratch dvid_inst_interact_backward needs for R rows (-1: a row count it does not take)"""
    return int(_lib.load().dvid_inst_interact_backward_scratch_bytes(int(R)))


def inst_interact_backward(p, roi, params, d_y=None, forward_only=False, want_d_roi=True):
    """An RCNNHead's DynamicConv with its residual and norm2 recomputed in fp32, and its gradient (dvid_inst_interact_backward,
    csrc/interact_bwd.hip; box_head.interact states the function).  p [R, 256] (the norm1 output), roi [R, 49, 256] (the fp32 RoI tiles), fp32
    on the device; params {name without the head's prefix: fp32 device tensor in the reference's layout}, the twelve of
    box_head.interact.PARAM_NAMES.  Cotangent d_y [R, 256]: None means zeros.  Returns a dict: "y", and -- unless forward_only -- "d_p",
    "d_roi" (None with want_d_roi=False: it is then not computed, every other output keeps its bits) and "param_grads" {name: gradient},
    every element written.  include/dvid_hip.h states the arithmetic (fp32 MFMA products, fixed-order sums without atomics: two runs give the
    same bits)."""
    from .modeling.roi_heads.box_head.interact import PARAM_NAMES
    p, roi = _cuda(p, torch.float32), _cuda(roi, torch.float32)
    assert p.dim() == 2 and roi.dim() == 3 and roi.shape[0] == p.shape[0] and roi.shape[2] == p.shape[1], "p is [R, d], roi [R, bins, d]"
    R, d = p.shape
    bins = roi.shape[1]
    pooler = int(round(bins ** 0.5))
    assert pooler * pooler == bins, "roi holds the bins of a square pooler"
    plist = [_cuda(params[k].detach(), torch.float32) for k in PARAM_NAMES]
    dd = plist[4].shape[0]
    want = ((2 * d * dd, d), (2 * d * dd,), (d, bins * d), (d,), (dd,), (dd,), (d,), (d,), (d,), (d,), (d,), (d,))
    for k, t, shape in zip(PARAM_NAMES, plist, want):
        assert tuple(t.shape) == shape, "%s is %s, expected %s" % (k, tuple(t.shape), shape)
    dev = p.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"y": new(R, d)}
    d_y = None if d_y is None else _cuda(d_y, torch.float32)
    assert d_y is None or tuple(d_y.shape) == (R, d), "the cotangent has y's shape"
    glist = []
    if forward_only:
        assert d_y is None, "a cotangent without a backward"
    else:
        out.update({"d_p": new(R, d), "d_roi": new(R, bins, d) if want_d_roi else None})
        glist = [torch.empty_like(t) for t in plist]
        out["param_grads"] = dict(zip(PARAM_NAMES, glist))
    table = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    ptable = table(plist)
    gtable = table(glist) if glist else None
    nbytes = inst_interact_backward_scratch_bytes(R)
    scratch = torch.empty((max(nbytes, 16) + 15) // 16 * 4, dtype=torch.float32, device=dev)
    call("dvid_inst_interact_backward", ptr(p), ptr(roi), R, d, dd, pooler, C.cast(ptable, C.c_void_p), len(plist), ptr(d_y), ptr(out["y"]),
         ptr(out.get("d_p")), ptr(out.get("d_roi")), None if gtable is None else C.cast(gtable, C.c_void_p), ptr(scratch), scratch.numel() * 4, stream_ptr())
    return out


def self_attn_backward_scratch_bytes(n, m):
    """bytes of scratch dvid_self_attn_backward needs for n images of m rows (-1: sizes it does not take)"""
    return int(_lib.load().dvid_self_attn_backward_scratch_bytes(int(n), int(m)))


def self_attn_backward(x, n, params, d_y=None, forward_only=False):
    """An RCNNHead's self-attention with its residual and norm1 recomputed in fp32, and its gradient (dvid_self_attn_backward,
    csrc/selfattn_bwd.hip; box_head.attention states the function).  x [n * m, 256], fp32 on the device, rows image-major: the m rows of each
    of the n images attend to each other.  params {name without the head's prefix: fp32 device tensor in the reference's layout}, the six of
    box_head.attention.PARAM_NAMES.  Cotangent d_y [n * m, 256]: None means zeros.  Returns a dict: "y", and -- unless forward_only -- "d_x"
    and "param_grads" {name: gradient}, every element written.  include/dvid_hip.h states the arithmetic (fp32 MFMA products, fixed-order
    sums without atomics: two runs give the same bits)."""
    from .modeling.roi_heads.box_head.attention import NHEADS, PARAM_NAMES
    x = _cuda(x, torch.float32)
    n = int(n)
    assert x.dim() == 2 and n >= 1 and x.shape[0] % n == 0, "x is [n * m, d]"
    R, d = x.shape
    m = R // n
    plist = [_cuda(params[k].detach(), torch.float32) for k in PARAM_NAMES]
    want = ((3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,))
    for k, t, shape in zip(PARAM_NAMES, plist, want):
        assert tuple(t.shape) == shape, "%s is %s, expected %s" % (k, tuple(t.shape), shape)
    dev = x.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"y": new(R, d)}
    d_y = None if d_y is None else _cuda(d_y, torch.float32)
    assert d_y is None or tuple(d_y.shape) == (R, d), "the cotangent has y's shape"
    glist = []
    if forward_only:
        assert d_y is None, "a cotangent without a backward"
    else:
        out["d_x"] = new(R, d)
        glist = [torch.empty_like(t) for t in plist]
        out["param_grads"] = dict(zip(PARAM_NAMES, glist))
    table = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    ptable = table(plist)
    gtable = table(glist) if glist else None
    nbytes = self_attn_backward_scratch_bytes(n, m)
    scratch = torch.empty((max(nbytes, 16) + 15) // 16 * 4, dtype=torch.float32, device=dev)
    call("dvid_self_attn_backward", ptr(x), n, m, d, NHEADS, C.cast(ptable, C.c_void_p), len(plist), ptr(d_y), ptr(out["y"]), ptr(out.get("d_x")),
         None if gtable is None else C.cast(gtable, C.c_void_p), ptr(scratch), scratch.numel() * 4, stream_ptr())
    return out


def set_criterion_scratch_bytes(S, n, M, gmax):
    """bytes of scratch dvid_set_criterion needs for S head outputs of n images with M queries and at most gmax boxes per image"""
    return int(_lib.load().dvid_set_criterion_scratch_bytes(int(S), int(n), int(M), int(gmax)))


def set_criterion(logits, boxes, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma, ota_k, cost_class, cost_bbox, cost_giou, out=None, gmax=None):
    """The dynamic-k matcher and the loss sums of S head outputs of n images in ONE call (dvid_set_criterion, csrc/criterion.hip).
    logits [S, n, M, C] and boxes [S, n, M, 4] (absolute xyxy) fp32; gt_boxes [G, 4] fp32 absolute xyxy, gt_labels [G] int32 1-based,
    gt_starts [n + 1] int32 (any device: the counts are checked on the host); sizes [n, 2] (w, h) or a FrameSizes.  Returns (assign
    [S, n, M] int32, matched_query [S, n, gmax] int32, sums [S, n, 4] float64, status [S, n] int32) on the device -- include/dvid_hip.h
    says what each holds; the caller reads `status` (box_head.loss.raise_on_status).  `out`: such a tuple to write into; gmax: the width
    of matched_query, by default the batch's largest box count (at least 1)."""
    logits, boxes = _cuda(logits, torch.float32), _cuda(boxes, torch.float32)
    assert logits.dim() == 4 and boxes.shape == logits.shape[:3] + (4,), "logits is [S, n, M, C], boxes [S, n, M, 4]"
    S, n, M, c = logits.shape
    dev = logits.device
    starts_host = torch.as_tensor(gt_starts).detach().to("cpu", torch.int32).contiguous()
    assert starts_host.shape == (n + 1,), "gt_starts is [n + 1]"
    counts = (starts_host[1:] - starts_host[:-1]).tolist()
    from .modeling.roi_heads.box_head.loss import check_limits
    check_limits(M, c, int(ota_k), counts)
    if gmax is None:
        gmax = max(counts + [1])
    gt_boxes, gt_labels = _cuda(gt_boxes, torch.float32).reshape(-1, 4), _cuda(gt_labels, torch.int32).reshape(-1)
    assert int(starts_host[-1]) == gt_boxes.shape[0] == gt_labels.shape[0], "gt_starts ends at the box count"
    fs = frame_sizes(sizes, n, dev)
    if out is None:
        out = (torch.empty((S, n, M), dtype=torch.int32, device=dev), torch.empty((S, n, gmax), dtype=torch.int32, device=dev),
               torch.empty((S, n, 4), dtype=torch.float64, device=dev), torch.empty((S, n), dtype=torch.int32, device=dev))
    assign, mq, sums, status = out
    assert assign.shape == (S, n, M) and mq.shape == (S, n, gmax) and sums.shape == (S, n, 4) and status.shape == (S, n), "output shapes"
    assert (assign.dtype, mq.dtype, sums.dtype, status.dtype) == (torch.int32, torch.int32, torch.float64, torch.int32), "output dtypes"
    if S == 0 or n == 0:
        return out
    nbytes = set_criterion_scratch_bytes(S, n, M, gmax)
    scratch = torch.empty(((nbytes + 15) // 16 * 2,), dtype=torch.float64, device=dev)
    starts_dev = starts_host.to(dev)          # named: a temporary would be freed before the call
    call("dvid_set_criterion", ptr(logits), ptr(boxes), S, n, M, c, ptr(gt_boxes), ptr(gt_labels), ptr(starts_dev), ptr(starts_host), ptr(fs),
         float(alpha), float(gamma), int(ota_k), float(cost_class), float(cost_bbox), float(cost_giou), *(ptr(_cuda(o)) for o in (assign, mq)), int(gmax),
         ptr(_cuda(sums)), ptr(_cuda(status)), ptr(scratch), scratch.numel() * 8, stream_ptr())
    return out


def set_criterion_backward(logits, boxes, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma, assign, status, coef, out=None):
    """The gradient of sum_s sum_k coef[s, k] * (focal, L1, 1 - GIoU sum of head output s over the batch) with respect to logits and boxes in
    ONE launch (dvid_set_criterion_backward, csrc/criterion.hip).  logits, boxes, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma: what
    set_criterion was handed; assign [S, n, M] int32 and status [S, n] int32: what it returned; coef [S, 3] float64 (for the reference's
    losses: upstream gradient / denominator, see box_head.loss).  Returns (d_logits [S, n, M, C], d_boxes [S, n, M, 4]) fp32 on the device,
    every element written; include/dvid_hip.h states the arithmetic, the zeros and the conventions at the kinks.  `out`: such a pair to write
    into."""
    logits, boxes = _cuda(logits, torch.float32), _cuda(boxes, torch.float32)
    assert logits.dim() == 4 and boxes.shape == logits.shape[:3] + (4,), "logits is [S, n, M, C], boxes [S, n, M, 4]"
    S, n, M, c = logits.shape
    dev = logits.device
    starts_host = torch.as_tensor(gt_starts).detach().to("cpu", torch.int32).contiguous()
    assert starts_host.shape == (n + 1,), "gt_starts is [n + 1]"
    gt_boxes, gt_labels = _cuda(gt_boxes, torch.float32).reshape(-1, 4), _cuda(gt_labels, torch.int32).reshape(-1)
    assert int(starts_host[-1]) == gt_boxes.shape[0] == gt_labels.shape[0], "gt_starts ends at the box count"
    fs = frame_sizes(sizes, n, dev)
    assign, status, coef = _cuda(assign, torch.int32), _cuda(status, torch.int32), _cuda(coef, torch.float64)
    assert assign.shape == (S, n, M) and status.shape == (S, n) and coef.shape == (S, 3), "assign is [S, n, M], status [S, n], coef [S, 3]"
    if out is None:
        out = (torch.empty((S, n, M, c), dtype=torch.float32, device=dev), torch.empty((S, n, M, 4), dtype=torch.float32, device=dev))
    d_logits, d_boxes = out
    assert d_logits.shape == (S, n, M, c) and d_boxes.shape == (S, n, M, 4), "output shapes"
    assert d_logits.dtype == d_boxes.dtype == torch.float32 and d_logits.is_contiguous() and d_boxes.is_contiguous(), "outputs are contiguous fp32"
    starts_dev = starts_host.to(dev)          # named: a temporary would be freed before the call
    call("dvid_set_criterion_backward", ptr(logits), ptr(boxes), S, n, M, c, ptr(gt_boxes), ptr(gt_labels), ptr(starts_dev), ptr(starts_host), ptr(fs),
         float(alpha), float(gamma), ptr(assign), ptr(status), ptr(coef), ptr(_cuda(d_logits)), ptr(_cuda(d_boxes)), stream_ptr())
    return out
