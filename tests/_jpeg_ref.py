"""numpy restatement of what libjpeg does behind its Huffman decoder (jidctint ISLOW, jdsample fancy upsampling, jdcolor), and the set of
Pillow-written files the JPEG tests share.  Written from libjpeg's definition, independently of csrc/jpeg.hip: whole planes at a time in
int64, where the kernel works per block and per pixel in int32."""
import io

import numpy as np
from PIL import Image

# h x w.  1x1 .. 48x64: sizes below one block, odd sizes, sizes whose chroma row has at most two samples (3x5, 17x3: libjpeg replicates
# there instead of interpolating), several MCUs.  The last two cross the kernels' own tile edges:
#   72x136 at 4:2:0 has 180 luma + 2 * 45 chroma = 270 blocks -- several 32-block IDCT workgroups and a part of one (270 = 8 * 32 + 14),
#   with both component boundaries (180, 225) inside a workgroup; in greyscale 153 = 4 * 32 + 25;
#   9x521 is wider than two colour workgroups (256 pixels each) by nine pixels, with an odd width and a one-row chroma plane at 4:2:0.
SIZES = [(1, 1), (3, 5), (8, 4), (9, 17), (16, 16), (17, 3), (33, 6), (37, 53), (40, 33), (48, 64), (72, 136), (9, 521)]
MODES = ["444", "422", "420", "grey"]
_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
# (quality, extra save arguments) per case index, cycled so that every size meets every mode, and every mode every variant
VARIANTS = [(30, {}), (90, {}), (100, {}), (90, {"optimize": True}), (90, {"restart_marker_blocks": 3}), (30, {"restart_marker_rows": 1}),
            (100, {"optimize": True, "restart_marker_blocks": 3})]


def picture(h, w, seed, saturate):
    """smooth blocks plus noise (many non-zero AC coefficients); with `saturate`, a few pixels at the ends of the range"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)], -1)
    base += rng.integers(0, 4, (h // 8 + 1, w // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:h, :w] * 20.0 - 30
    img = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    if saturate:
        for _ in range(max(1, h * w // 40)):
            img[rng.integers(h), rng.integers(w)] = rng.choice([0, 255], 3)
    return img


def encode(img, mode, quality, **kw):
    buf = io.BytesIO()
    if mode == "grey":
        Image.fromarray(img[..., 0]).save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=_SUBSAMPLING[mode], **kw)
    return buf.getvalue()


def pillow_rgb(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).copy()


_cases = None


def cases():
    """[(name, jpeg bytes, Pillow's uint8 [h, w, 3])]: every size in every mode, the variants cycled; built once and shared"""
    global _cases
    if _cases is None:
        _cases = []
        k = 0
        for si, (h, w) in enumerate(SIZES):
            for mi, mode in enumerate(MODES):
                quality, kw = VARIANTS[(si + 2 * mi) % len(VARIANTS)]
                data = encode(picture(h, w, 1000 + k, quality == 100), mode, quality, **kw)
                name = "%dx%d-%s-q%d%s" % (h, w, mode, quality, "".join("-" + a.split("_")[-1] for a in sorted(kw)))
                _cases.append((name, data, pillow_rgb(data)))
                k += 1
    return _cases


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------
def _descale(x, s):
    return (x + (1 << (s - 1))) >> s


def _idct_1d(i, s):
    """i: int64 [8, ...] along axis 0 -> the eight outputs, descaled by s"""
    z1 = (i[2] + i[6]) * 4433
    t2 = z1 - i[6] * 15137
    t3 = z1 + i[2] * 6270
    t0 = (i[0] + i[4]) << 13
    t1 = (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([_descale(v, s) for v in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)])


def component_plane(coef, quant, blocks_h, blocks_w):
    """int16 [blocks_h * blocks_w * 64] + uint16 [64] -> uint8 [blocks_h * 8, blocks_w * 8]"""
    blk = coef.astype(np.int64).reshape(-1, 8, 8) * quant.astype(np.int64).reshape(1, 8, 8)
    ws = _idct_1d(blk.transpose(1, 0, 2), 11)                    # pass 1: down the columns; [row, block, col]
    px = _idct_1d(ws.transpose(2, 1, 0), 18)                     # pass 2: along the rows;   [col, block, row]
    px = np.clip((((px & 1023) ^ 512) - 512) + 128, 0, 255).transpose(1, 2, 0)          # [block, row, col]
    return px.reshape(blocks_h, blocks_w, 8, 8).transpose(0, 2, 1, 3).reshape(blocks_h * 8, blocks_w * 8).astype(np.uint8)


def _h2v1(p):
    p = p.astype(np.int64)
    dw = p.shape[1]
    if dw <= 2:
        return p.repeat(2, 1)
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
    return np.stack([even, odd], -1).reshape(p.shape[0], 2 * dw)


def _h2v2(p):
    p = p.astype(np.int64)
    dh, dw = p.shape
    if dw <= 2:
        return p.repeat(2, 0).repeat(2, 1)
    above, below = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    out = np.empty((2 * dh, 2 * dw), dtype=np.int64)
    for v, other in ((0, above), (1, below)):
        cs = 3 * p + other
        left, right = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[v::2, 0::2] = (3 * cs + left + 8) >> 4
        out[v::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def reconstruct(coef, info):
    """the coefficients of one file (data.jpeg.JpegCoefficients' two fields) -> uint8 [h, w, 3], by libjpeg's arithmetic"""
    h, w = info.height, info.width
    hmax, vmax = info.hsamp[0], info.vsamp[0]
    planes = []
    for c in range(info.ncomp):
        n = info.blocks_w[c] * info.blocks_h[c] * 64
        full = component_plane(coef[info.coef_offset[c]:info.coef_offset[c] + n], info.quant[c], info.blocks_h[c], info.blocks_w[c])
        dh, dw = -(-h * info.vsamp[c] // vmax), -(-w * info.hsamp[c] // hmax)
        planes.append(full[:dh, :dw])
    y = planes[0].astype(np.int64)
    if info.ncomp == 1:
        return np.stack([y, y, y], -1).astype(np.uint8)
    up = {(1, 1): lambda p: p.astype(np.int64), (2, 1): _h2v1, (2, 2): _h2v2}[(hmax, vmax)]
    cb, cr = up(planes[1])[:h, :w] - 128, up(planes[2])[:h, :w] - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
