"""Test-time image transform of the DiffusionVID path: Resize(min 600, max 1000) + ToTensor.

Reference: mega_core/data/transforms/build.py:89-97 (test pipeline for METHOD "diffusion": Resize, ToTensor, no Normalize --
the model normalises itself, diffusion_det.py:301-303) and transforms.py:31-70 (`Resize`: the size is chosen from the
CURRENT frame and re-used for its reference frames; `torchvision.transforms.functional.resize` on a PIL image, i.e.
`PIL.Image.resize(..., BILINEAR)`).

Pillow's bilinear resize is a separable triangle filter whose support grows with the down-scaling factor, evaluated in
8-bit fixed point: per axis, double-precision weights normalised to sum 1 and rounded to 22-bit integers, an integer
dot product per output sample, rounding and clamping to uint8 BETWEEN the horizontal and the vertical pass (Pillow
src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal/Vertical_8bpc).
`resample_tables` builds those integer tables on the host; the two passes themselves run either in numpy
(`resize_u8_numpy`, small images / tests) or on the GPU (csrc/resize.hip through ops.resize_u8_to_f32), bit-identical
to Pillow's output, so that frames can travel to the GPU as uint8 at their native size (a 1280x720 JPEG frame is 2.8 MB
instead of 7.5 MB of padded fp32) and be resized, scaled to [0,1] and zero-padded there.
"""
import collections
import math

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2


def get_size(image_size_wh, min_size=600, max_size=1000):
    """transforms.py:39-59: (w, h) of the source -> (oh, ow); shorter side to `min_size` unless that pushes the longer side
    beyond `max_size`."""
    w, h = image_size_wh
    size = min_size
    if max_size is not None:
        lo, hi = float(min(w, h)), float(max(w, h))
        if hi / lo * size > max_size:
            size = int(round(max_size * lo / hi))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        return (int(size * h / w), size)
    return (size, int(size * w / h))


def resample_tables(in_size, out_size):
    """One axis of Pillow's BILINEAR resample: -> (bounds int32 [out, 2] = (first source sample, count), weights int32
    [out, ksize]) in 22-bit fixed point."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    inv = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([max(0.0, 1.0 - abs((x + xmin - center + 0.5) * inv)) for x in range(xmax)], dtype=np.float64)
        total = 0.0
        for v in w:                      # left-to-right double accumulation, as the C loop does
            total += float(v)
        if total != 0.0:
            w = w / total
        q = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
        kk[xx, :xmax] = q.astype(np.int32)
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass_numpy(img, bounds, kk, axis):
    """one integer resample pass along `axis` (0: rows / vertical, 1: columns / horizontal) of a uint8 HWC array"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    for o in range(bounds.shape[0]):
        a, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[o, :n].astype(np.int64), src[a:a + n], axes=(0, 0))
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_u8_numpy(img_hwc, out_hw):
    """Pillow-identical BILINEAR resize of a uint8 HWC image (horizontal pass, then vertical; a pass whose size does not
    change is skipped, as in ImagingResample)."""
    h, w = img_hwc.shape[:2]
    oh, ow = out_hw
    out = np.ascontiguousarray(img_hwc)
    if ow != w:
        out = _pass_numpy(out, *resample_tables(w, ow), axis=1)
    if oh != h:
        out = _pass_numpy(out, *resample_tables(h, oh), axis=0)
    return out


# ---- TEST.BBOX_AUG: the views of a still image (mega_core/engine/bbox_aug.py: im_detect_bbox_aug) --------------------------------------
BBOX_AUG_MAX_VIEWS = 64          # the draw key's `image` slot holds the view index (utils/synthetic.py: 64 images per step)


# one view: the (w, h) its `Resize` gives, whether it is mirrored behind it, and its scale group
View = collections.namedtuple("View", ["w", "h", "flip", "group"])


def bbox_aug_scales(cfg):
    """[(min_size, max_size, n_views)] per scale group, in im_detect_bbox_aug's order: the identity scale (INPUT.MIN_SIZE_TEST,
    INPUT.MAX_SIZE_TEST; two views with H_FLIP), then every TEST.BBOX_AUG.SCALES entry under BBOX_AUG.MAX_SIZE (two with SCALE_H_FLIP)"""
    aug = cfg.TEST.BBOX_AUG
    groups = [(int(cfg.INPUT.MIN_SIZE_TEST), int(cfg.INPUT.MAX_SIZE_TEST), 2 if aug.H_FLIP else 1)]
    groups += [(int(s), int(aug.MAX_SIZE), 2 if aug.SCALE_H_FLIP else 1) for s in aug.SCALES]
    return groups


def bbox_aug_num_views(cfg):
    return sum(g[2] for g in bbox_aug_scales(cfg))


def bbox_aug_views(cfg, image_size_wh):
    """The views of an image of (w, h), in the order im_detect_bbox_aug detects them -- view 0 is the plain test transform; a scale group
    is one scale entry with its one or two views (the second one the mirror of the first, same size)."""
    views = []
    for g, (lo, hi, n) in enumerate(bbox_aug_scales(cfg)):
        oh, ow = get_size(image_size_wh, lo, hi)
        views += [View(int(ow), int(oh), k == 1, g) for k in range(n)]
    return views


def bbox_aug_check(cfg, num_proposals, sample_step, max_candidates):
    """TEST.BBOX_AUG.ENABLED: refuses what the merge cannot take (NotImplementedError with the keys and the numbers)"""
    n_views = bbox_aug_num_views(cfg)
    aug = cfg.TEST.BBOX_AUG
    what = "TEST.BBOX_AUG (H_FLIP %s, SCALES %s, SCALE_H_FLIP %s) gives %d views" % (aug.H_FLIP, tuple(aug.SCALES), aug.SCALE_H_FLIP, n_views)
    if n_views > BBOX_AUG_MAX_VIEWS:
        raise NotImplementedError("%s: the limit is %d (the view index is the `image` slot of the draw key)" % (what, BBOX_AUG_MAX_VIEWS))
    per_view = max(1, int(sample_step) - 1) * int(num_proposals)
    if n_views * per_view > max_candidates:
        raise NotImplementedError(
            "%s of max(1, SAMPLE_STEP - 1) * NUM_PROPOSALS = max(1, %d - 1) * %d = %d candidates each: the merging NMS gets %d per image, the limit is %d"
            % (what, sample_step, num_proposals, per_view, n_views * per_view, max_candidates))
    return n_views


class ViewsPlan:
    """What ops.resize_views_u8 reads for n images, each resized from its own (h, w) to its own (oh, ow): per image one descriptor row
    (int64: h, w, oh, ow, first row of its x tables in `bounds` or -1 for a skipped pass, first weight, ksize, the same three for y, byte
    offset of its share of the intermediate buffer) and the images' resample_tables concatenated -- bounds int32 [rows, 2], weights int32
    flat, `ksize` per image.  Host arrays; `.to(device)` uploads them once."""
    COLS = 11

    def __init__(self, sizes_hw, out_hw, cache=None):
        assert len(sizes_hw) == len(out_hw) and len(sizes_hw) > 0
        cache = {} if cache is None else cache
        desc = np.zeros((len(sizes_hw), self.COLS), dtype=np.int64)
        bounds, weights, rows, nk, tmp = [], [], 0, 0, 0
        for i, ((h, w), (oh, ow)) in enumerate(zip(sizes_hw, out_hw)):
            h, w, oh, ow = int(h), int(w), int(oh), int(ow)
            assert min(h, w, oh, ow) > 0
            desc[i, :4] = (h, w, oh, ow)
            for col, (a, b) in ((4, (w, ow)), (7, (h, oh))):
                if a == b:
                    desc[i, col:col + 3] = (-1, 0, 0)
                    continue
                if (a, b) not in cache:
                    cache[(a, b)] = resample_tables(a, b)
                bd, kk = cache[(a, b)]
                assert bd[:, 0].min() >= 0 and bd[:, 1].min() >= 0 and (bd[:, 0] + bd[:, 1]).max() <= a and bd[:, 1].max() <= kk.shape[1]
                desc[i, col:col + 3] = (rows, nk, kk.shape[1])
                bounds.append(bd)
                weights.append(kk.reshape(-1))
                rows += bd.shape[0]
                nk += kk.size
            desc[i, 10] = tmp
            if ow != w:
                tmp += -(-h * ow * 3 // 16) * 16
        self.n = len(sizes_hw)
        self.desc = desc
        self.bounds = np.concatenate(bounds) if bounds else np.zeros((1, 2), dtype=np.int32)
        self.weights = np.concatenate(weights) if weights else np.zeros((1,), dtype=np.int32)
        self.tmp_bytes = max(tmp, 16)
        self.max_h = int(desc[desc[:, 4] >= 0, 0].max()) if (desc[:, 4] >= 0).any() else 0          # rows of the widest h-pass grid
        self.max_ow = int(desc[:, 3].max())
        self.max_oh = int(desc[:, 2].max())
        self.dev = None

    def to(self, device):
        if self.dev is None or self.dev[0].device != torch.device(device):
            self.dev = tuple(torch.from_numpy(a).to(device) for a in (self.desc, self.bounds, self.weights))
        return self


def _as_u8_hwc(image):
    """PIL image / numpy HWC / torch HWC uint8 -> contiguous numpy uint8 [H, W, 3] (RGB)"""
    if isinstance(image, torch.Tensor):
        image = image.cpu().numpy()
    if not isinstance(image, np.ndarray):
        image = np.asarray(image.convert("RGB"))
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    return np.ascontiguousarray(image)


class ResizeToTensor:
    """Resize + ToTensor on the HOST with Pillow itself -- the reference's path; frames come out as fp32 CHW in [0, 1]."""

    def __init__(self, min_size=600, max_size=1000):
        self.min_size, self.max_size = min_size, max_size
        self.size = None

    def __call__(self, image, is_current=False):
        from PIL import Image
        if not hasattr(image, "resize") or isinstance(image, (np.ndarray, torch.Tensor)):
            image = Image.fromarray(_as_u8_hwc(image))
        if is_current or self.size is None:
            self.size = get_size(image.size, self.min_size, self.max_size)
        oh, ow = self.size
        out = np.array(image.convert("RGB").resize((ow, oh), Image.BILINEAR))          # a writable copy
        return torch.from_numpy(out).permute(2, 0, 1).to(torch.float32).div(255)


class ResizeToTensorDevice:
    """The same transform with the resample on the GPU: the uint8 frame is uploaded at its native size and leaves the
    kernels as fp32 CHW in [0, 1], zero-padded to `size_divisible` (what to_image_list would do next), bit-identical to
    ResizeToTensor + padding."""

    def __init__(self, device, min_size=600, max_size=1000, size_divisible=32):
        self.device = torch.device(device)
        self.min_size, self.max_size, self.div = min_size, max_size, size_divisible
        self.size = None
        self._tables = {}
        self._pinned_ring = {}

    def _pinned(self, shape, depth=4):
        """next [pinned buffer, event of its last upload] of a ring of `depth` staging buffers for frames of this shape"""
        ring = self._pinned_ring.setdefault(shape, {"slots": [], "next": 0})
        if len(ring["slots"]) < depth:
            ring["slots"].append([torch.empty(shape, dtype=torch.uint8).pin_memory(), None])
            return ring["slots"][-1]
        slot = ring["slots"][ring["next"]]
        ring["next"] = (ring["next"] + 1) % depth
        return slot

    def tables(self, in_size, out_size):
        key = (in_size, out_size)
        if key not in self._tables:
            b, k = resample_tables(in_size, out_size)
            self._tables[key] = (torch.from_numpy(b).to(self.device), torch.from_numpy(k).to(self.device))
        return self._tables[key]

    def __call__(self, image, is_current=False):
        from .. import ops
        if isinstance(image, torch.Tensor) and image.is_cuda:
            src = image
        else:
            # decoded frame -> a pinned, writable staging buffer of its size (kept per size) -> async H2D.  (A from_numpy view
            # of the decoder's read-only buffer is pageable: its "non_blocking" upload only works because the runtime stages it
            # synchronously.)  The staging buffer is reused, so the copy engine must have read it before the next frame lands.
            u8 = _as_u8_hwc(image)
            slot = self._pinned(u8.shape)
            if slot[1] is not None:
                slot[1].synchronize()          # four uploads back: long done in practice
            slot[0].numpy()[...] = u8
            src = slot[0].to(self.device, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record(torch.cuda.current_stream(self.device))
        h, w = src.shape[:2]
        if is_current or self.size is None:
            self.size = get_size((w, h), self.min_size, self.max_size)
        oh, ow = self.size
        d = self.div
        ph, pw = (-(-oh // d) * d, -(-ow // d) * d) if d else (oh, ow)
        tx = self.tables(w, ow) if ow != w else None
        ty = self.tables(h, oh) if oh != h else None
        out = ops.resize_u8_to_f32(src, oh, ow, ph, pw, tx, ty)
        out.image_size = (oh, ow)
        return out
