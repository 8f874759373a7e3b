"""The demo surface: detections drawn onto frames (mirror of the reference's demo/predictor.py: VIDDemo, select_top_predictions,
compute_colors_for_labels, overlay_boxes, overlay_class_names, generate_images).

What is the reference's: which detections are drawn (score > threshold, strict), in which order (ascending score, so the best ends on
top; ties by row), where (the BoxList resized to the image's native size, corners truncated as `box.to(torch.int64)` truncates them),
in which colour (`labels * palette % 255`, its BGR triple shown as it looks) and with which text ("{}: {:.2f}").
What is this project's: the rasterisation.  The reference draws with OpenCV (Hershey fonts, its own line rasteriser); OpenCV is no
dependency here, so a box is a ring of whole pixels and the text a plate of bitmap glyphs at the box's corner (include/dvid_hip.h,
dvid_overlay_detections, states every rule).  The pixels therefore do not match OpenCV's.  Two limits: the ops.OVERLAY_MAX_DRAWN = 256
latest rows in draw order are drawn per frame, and a class name shows its first ops.OVERLAY_NAME_MAX = 24 bytes.

CUDA frames are drawn by csrc/overlay.hip where they lie (ops.overlay_detections: scores never visit the host); numpy frames by
`render_numpy`, the same rules as a per-pixel gather in numpy.  The two are bit-equal (tests/test_gpu_overlay.py)."""
import glob
import os

import numpy as np
import torch

from ..data.datasets.vid import VID_CLASSES, VIDFrameList, VIDMEGATestDataset
from ..structures.bounding_box import BoxList

MAX_DRAWN = 256          # ops.OVERLAY_MAX_DRAWN
NAME_MAX = 24            # ops.OVERLAY_NAME_MAX
PALETTE = (2 ** 25 - 1, 2 ** 15 - 1, 2 ** 21 - 1)
_INT32 = (-2 ** 31, 2 ** 31 - 1)


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
def name_table(names):
    """class names, indexed by label (0 = background) -> uint8 [len(names), 24]: zero-padded, cut at 24 bytes, bytes outside 32 .. 126 as '?'"""
    table = np.zeros((len(names), NAME_MAX), dtype=np.uint8)
    for i, name in enumerate(names):
        raw = str(name).encode("utf-8", "replace")[:NAME_MAX]
        table[i, :len(raw)] = [b if 32 <= b <= 126 else ord("?") for b in raw]
    return table


def glyph_atlas(font=None):
    """uint8 [95, gh, gw] of 0 / 1: the characters 32 .. 126 of a Pillow font, each through `font.getmask(ch, mode="1")`, pasted top-left into
    a cell of the largest glyph's size.  Default: Pillow's built-in bitmap font, rasterised here and now (no font data is kept in the tree)."""
    if font is None:
        from PIL import ImageFont
        font = ImageFont.load_default_imagefont() if hasattr(ImageFont, "load_default_imagefont") else ImageFont.load_default()
    glyphs = []
    for code in range(32, 127):
        mask = font.getmask(chr(code), mode="1")
        w, h = mask.size
        glyphs.append((np.asarray(mask, dtype=np.int64).reshape(h, w) != 0).astype(np.uint8) if w and h else np.zeros((0, 0), dtype=np.uint8))
    gh, gw = max(1, max(g.shape[0] for g in glyphs)), max(1, max(g.shape[1] for g in glyphs))
    if gh > 32 or gw > 32:
        raise ValueError("the font's glyphs are %d x %d pixels, the overlay takes cells up to 32 x 32" % (gw, gh))
    atlas = np.zeros((95, gh, gw), dtype=np.uint8)
    for k, g in enumerate(glyphs):
        atlas[k, :g.shape[0], :g.shape[1]] = g
    return atlas


# ---- the rules on the host ---------------------------------------------------------------------------------------------------------------
def select_top_predictions(boxlist, threshold):
    """predictor.py:726-743: the rows with scores > threshold, in ascending order of score (stable), as a BoxList"""
    scores = boxlist.get_field("scores")
    kept = boxlist[torch.nonzero(scores > threshold).squeeze(1)]
    order = torch.sort(kept.get_field("scores"), dim=0, descending=False, stable=True)[1]
    return kept[order]


def score_hundredths(score):
    """|score| (an fp32 value) correctly rounded to hundredths, ties to even, clamped to 999 -- in integers, as the kernel forms it: the
    24-bit significand times 100, shifted by the exponent, the remainder compared with one half.  "%d.%02d" of it is "{:.2f}".format."""
    bits = int(np.float32(score).view(np.uint32)) & 0x7fffffff
    e, m = bits >> 23, bits & 0x7fffff
    if e == 0:
        e = 1
    else:
        m |= 0x800000
    v, shift = m * 100, 150 - e
    if shift <= 0:
        return 999
    q, rem, half = v >> shift, v & ((1 << shift) - 1), 1 << (shift - 1)
    if rem > half or (rem == half and q & 1):
        q += 1
    return min(q, 999)


def score_text(score):
    q = score_hundredths(score)
    sign = "-" if int(np.float32(score).view(np.uint32)) >> 31 else ""
    return "%s%d.%02d" % (sign, q // 100, q % 100)


def label_colour(label):
    """(r, g, b) of an integer label: the reference's (label * palette) % 255 is its BGR triple"""
    c = [(int(label) * p) % 255 for p in PALETTE]
    return c[2], c[1], c[0]


def _trunc_i32(v):
    """an fp32 value truncated toward zero and clamped to the int32 range (an overflowed product included; NaN -> 0)"""
    v = float(v)
    if v != v:
        return 0
    return _INT32[1] if v >= 2.0 ** 31 else _INT32[0] if v <= -2.0 ** 31 else int(v)


def draw_list(dets, ratio, names, threshold):
    """the rows of fp32 `dets` [k, 6] (model frame) that one frame draws, in draw order: (x1, y1, x2, y2, (r, g, b), text bytes)"""
    dets = np.ascontiguousarray(dets, dtype=np.float32).reshape(-1, 6)
    thr = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(dets[:, :5]).all(axis=1) & (dets[:, 4] > thr)
    rows = np.nonzero(ok)[0]
    rows = rows[np.argsort(dets[rows, 4], kind="stable")][-MAX_DRAWN:]
    rw, rh = np.float32(ratio[0]), np.float32(ratio[1])
    out = []
    for r in rows:
        with np.errstate(over="ignore"):
            x1, y1, x2, y2 = (_trunc_i32(np.float32(dets[r, c]) * m) for c, m in ((0, rw), (1, rh), (2, rw), (3, rh)))
        if x2 < x1 or y2 < y1:
            continue
        L = _trunc_i32(dets[r, 5])
        name = bytes(names[L][names[L] != 0].tolist()) if 0 <= L < len(names) else b""
        text = (name + b": " if name else b"") + score_text(dets[r, 4]).encode()
        out.append((x1, y1, x2, y2, label_colour(L), text))
    return out


def _rows_of(b):
    """a BoxList as fp32 [k, 6] rows (box, score, label) on the host"""
    return torch.cat([b.bbox.float(), b.get_field("scores").float()[:, None], b.get_field("labels").float()[:, None]], dim=1).cpu().numpy()


def render_numpy(frame, dets, ratio=(1.0, 1.0), names=None, threshold=0.7, thickness=2, text_scale=1, atlas=None):
    """The product's CPU path: one numpy uint8 [h, w, 3] frame, drawn in place and returned.  dets: fp32 [k, 6] rows (box, score, label) with
    `ratio` = (rw, rh) toward the frame, or a BoxList already at the frame's size.  Every pixel takes the latest plate that covers it,
    else the latest ring (owner maps, then one gather)."""
    if isinstance(dets, BoxList):
        dets = _rows_of(dets)
    names = name_table(VID_CLASSES) if names is None else names
    atlas = glyph_atlas() if atlas is None else atlas
    if not (1 <= int(thickness) <= 16 and 1 <= int(text_scale) <= 4):
        raise ValueError("thickness is 1 .. 16 and text_scale 1 .. 4")
    t, s = int(thickness), int(text_scale)
    gh, gw = atlas.shape[1:]
    h, w = frame.shape[:2]
    items = draw_list(dets, ratio, names, threshold)
    ring = np.full((h, w), -1, dtype=np.int32)
    plate = np.full((h, w), -1, dtype=np.int32)
    white = np.zeros((h, w), dtype=bool)
    o, i = t // 2, t - t // 2

    def clip(a, b, n):          # inclusive [a, b] -> slice inside [0, n)
        return slice(min(max(a, 0), n), min(max(b + 1, 0), n))
    for d, (x1, y1, x2, y2, _, text) in enumerate(items):
        ys, xs = clip(y1 - o, y2 + o, h), clip(x1 - o, x2 + o, w)
        yy, xx = np.arange(ys.start, ys.stop)[:, None], np.arange(xs.start, xs.stop)[None, :]
        hole = (yy >= y1 + i) & (yy <= y2 - i) & (xx >= x1 + i) & (xx <= x2 - i)          # empty on either axis: the rectangle is solid
        ring[ys, xs][~hole] = d          # basic slicing: a view, written through
        n = len(text)
        bits = np.concatenate([atlas[c - 32] if 32 <= c <= 126 else atlas[ord("?") - 32] for c in text], axis=1)          # [gh, n * gw]
        cell = np.zeros((gh * s + 2 * s, n * gw * s + 2 * s), dtype=bool)
        cell[s:s + gh * s, s:s + n * gw * s] = np.repeat(np.repeat(bits != 0, s, axis=0), s, axis=1)
        ys, xs = clip(y1, y1 + cell.shape[0] - 1, h), clip(x1, x1 + cell.shape[1] - 1, w)
        if ys.stop > ys.start and xs.stop > xs.start:
            plate[ys, xs] = d
            white[ys, xs] = cell[ys.start - y1:ys.stop - y1, xs.start - x1:xs.stop - x1]
    owner = np.where(plate >= 0, plate, ring)
    if items:
        colours = np.array([it[4] for it in items], dtype=np.uint8)
        hit = owner >= 0
        frame[hit] = colours[owner[hit]]
        frame[(plate >= 0) & white] = 255
    return frame


def boxlist_ratios(boxlist, frame_hw):
    """(rw, rh) as BoxList.resize((W, H)) forms them: Python doubles new / old, rounded to fp32 by the multiplication"""
    h, w = frame_hw
    return float(w) / float(boxlist.size[0]), float(h) / float(boxlist.size[1])


def pack_boxlists(boxlists, device=None):
    """BoxLists -> (dets fp32 [n, cap, 6], counts int32 [n]) on `device` (default: where the first one lives), pack_predictions' layout;
    device BoxLists are packed on the device, nothing is read back"""
    device = boxlists[0].bbox.device if device is None else torch.device(device)
    cap = max(1, max(len(b) for b in boxlists))
    dets = torch.zeros((len(boxlists), cap, 6), dtype=torch.float32, device=device)
    for j, b in enumerate(boxlists):
        k = len(b)
        if k:
            dets[j, :k, :4] = b.bbox.to(device)
            dets[j, :k, 4] = b.get_field("scores").to(device)
            dets[j, :k, 5] = b.get_field("labels").to(device, torch.float32)
    counts = torch.tensor([len(b) for b in boxlists], dtype=torch.int32).to(device)
    return dets, counts


def render_boxlists(frames, boxlists, names, threshold=0.7, thickness=2, text_scale=1, atlas=None):
    """Draw `boxlists[i]` (in the model's size, as the detector returns it) onto `frames[i]` (native-size uint8 [h, w, 3]), in place.
    CUDA frames -- a list, or one [n, H, W, 3] tensor -- go through ops.overlay_detections in one launch sequence and stay on the device;
    numpy frames go through render_numpy.  names: a list of class names or a name_table.  Returns `frames`."""
    names = names if isinstance(names, (np.ndarray, torch.Tensor)) else name_table(names)
    atlas = glyph_atlas() if atlas is None else atlas
    views = list(frames)
    if len(views) != len(boxlists):
        raise ValueError("%d frames for %d BoxLists" % (len(views), len(boxlists)))
    if not views:
        return frames
    ratios = [boxlist_ratios(b, f.shape[:2]) for b, f in zip(boxlists, views)]
    if isinstance(views[0], torch.Tensor) and views[0].is_cuda:
        from .. import ops
        dev = views[0].device
        dets, counts = pack_boxlists(boxlists, dev)
        ops.overlay_detections(frames, dets, counts, torch.tensor(ratios, dtype=torch.float64).to(torch.float32).to(dev),
                               torch.as_tensor(names).to(dev), torch.as_tensor(atlas).to(dev), threshold, thickness, text_scale)
        return frames
    names_np = names.cpu().numpy() if isinstance(names, torch.Tensor) else names
    atlas_np = atlas.cpu().numpy() if isinstance(atlas, torch.Tensor) else atlas
    for f, b, r in zip(views, boxlists, ratios):
        if not isinstance(f, np.ndarray):
            raise TypeError("frames are numpy arrays or CUDA tensors")
        render_numpy(f, _rows_of(b), np.array(r, dtype=np.float64).astype(np.float32), names_np, threshold, thickness, text_scale, atlas_np)
    return frames


# ---- the demo -------------------------------------------------------------------------------------------------------------------------------
class VIDDemo:
    """The reference's VIDDemo for the DiffusionVID path.  The model is handed in (checkpoints are the caller's business); any
    configuration the video path accepts works, the streaming one (INFER_BATCH 1) included: frames travel the video protocol of
    VIDMEGATestDataset over a frame list made of the video's length."""
    CATEGORIES = VID_CLASSES

    def __init__(self, cfg, model, confidence_threshold=0.7, output_folder=None, categories=VID_CLASSES, thickness=2, text_scale=1, font=None):
        self.cfg, self.model = cfg, model
        self.confidence_threshold = confidence_threshold
        self.output_folder = output_folder
        self.categories = tuple(categories)
        self.thickness, self.text_scale = thickness, text_scale
        self.names = name_table(self.categories)
        self.atlas = glyph_atlas(font)
        self.device = torch.device(getattr(model, "device", cfg.MODEL.DEVICE))
        self._dev_tables = None

    def _tables(self, device):
        if self._dev_tables is None or self._dev_tables[0].device != device:
            self._dev_tables = (torch.from_numpy(self.names).to(device), torch.from_numpy(self.atlas).to(device))
        return self._dev_tables

    def run_on_frames(self, frames):
        """one video as a list of native-size uint8 [h, w, 3] frames (numpy or tensors) -> (annotated frames, predictions): CUDA uint8
        tensors and the model's own BoxLists (model size, on the device), one per frame.  Each frame is uploaded once; the same tensor
        feeds the resize kernels, and a copy of it is drawn on."""
        from ..data import transforms as T
        from . import inference as eng
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("VIDDemo detects on the GPU (MODEL.DEVICE %s); render_numpy draws host frames" % dev)
        n = len(frames)
        if n == 0:
            return [], []
        src = [f.to(dev) if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
        for f in src:
            if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
                raise ValueError("frames are uint8 [h, w, 3] RGB")
        src = [f.contiguous() for f in src]
        cfg = self.cfg
        transform = T.ResizeToTensorDevice(dev, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, cfg.DATALOADER.SIZE_DIVISIBILITY)
        dataset = VIDMEGATestDataset(cfg, "", VIDFrameList.from_lengths({"video": n}), transform=transform,
                                     loader=lambda path: src[int(os.path.basename(path).split(".")[0])])
        results = {}
        model = self.model
        la = int(getattr(model, "lookahead", 1) or 1)
        for _, item in eng.lookahead_items(dataset, range(n), getattr(model, "infer_batch", cfg.INPUT.INFER_BATCH), la):
            images, _, ids = item
            with torch.no_grad():
                output = model(images)
            results.update(zip(ids, output))
        predictions = [results[i] for i in range(n)]
        drawn = [f.clone() for f in src]
        names, atlas = self._tables(dev)
        render_boxlists(drawn, predictions, names, self.confidence_threshold, self.thickness, self.text_scale, atlas)
        return drawn, predictions

    def run_on_image_folder(self, image_folder, suffix=".JPEG"):
        """predictor.py:425-428: the folder's `*suffix` files in sorted order are one video"""
        from ..data.datasets.vid import _pil_loader
        paths = sorted(glob.glob(image_folder + "/*" + suffix))
        if not paths:
            raise FileNotFoundError("no *%s files in %s" % (suffix, image_folder))
        return self.run_on_frames([_pil_loader(p) for p in paths])

    def run_on_image(self, frame, boxlist):
        """draw only: `boxlist` (model size) onto a copy of `frame` (native size; numpy or CUDA) -> the annotated copy"""
        out = frame.clone() if isinstance(frame, torch.Tensor) else np.array(frame, copy=True)
        if isinstance(out, torch.Tensor) and out.is_cuda:
            names, atlas = self._tables(out.device)
            render_boxlists([out], [boxlist], names, self.confidence_threshold, self.thickness, self.text_scale, atlas)
        else:
            out = out.numpy() if isinstance(out, torch.Tensor) else out
            render_boxlists([out], [boxlist], self.names, self.confidence_threshold, self.thickness, self.text_scale, self.atlas)
        return out

    def run_on_video(self, video_path, start_frame=0):
        raise NotImplementedError("run_on_video needs a video decoder, and none is a dependency of this package: extract the frames first "
                                  "(for instance `ffmpeg -i %s frames/%%06d.JPEG`) and call run_on_image_folder" % video_path)

    def generate_images(self, frames, folder=None):
        """predictor.py:844-846: `%06d.jpg` per frame into `folder` (default: output_folder), written with Pillow.  No zip, nothing removed."""
        from PIL import Image
        folder = folder or self.output_folder
        if not folder:
            raise ValueError("generate_images needs a folder (or output_folder at construction)")
        os.makedirs(folder, exist_ok=True)
        paths = []
        for i, f in enumerate(frames):
            arr = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
            paths.append(os.path.join(folder, "%06d.jpg" % i))
            Image.fromarray(arr).save(paths[-1])
        return paths
