"""The demo overlay restated the reference's way (demo/predictor.py), as a painter: select, sort, draw every ring in order, then every
plate in order, each with plain array slicing; the text from Python's own "{}: {:.2f}".format and the colour from Python integers.
Shares no code with diffusionvid_amd/engine/demo.py (owner maps and an integer score text) or with the kernel's per-pixel gather.
The rasterisation rules are the contract's (include/dvid_hip.h, dvid_overlay_detections)."""
import math

import numpy as np

MAX_DRAWN = 256
NAME_MAX = 24
KIND_NONE, KIND_RING, KIND_PLATE, KIND_GLYPH = 0, 1, 2, 3


def _to_int(v):
    """box.to(torch.int64) on a value the int32 clamp then bounds: truncation toward zero"""
    if math.isinf(v):
        return 2 ** 31 - 1 if v > 0 else -2 ** 31
    return max(-2 ** 31, min(2 ** 31 - 1, int(v)))


def _span(a, b, n):
    """the inclusive range [a, b] clipped to an axis of n pixels, as a slice (empty when nothing is left)"""
    lo, hi = max(a, 0), min(b, n - 1)
    return slice(lo, hi + 1) if lo <= hi else slice(0, 0)


def _name(class_names, label):
    if not 0 <= label < len(class_names):
        return ""
    raw = class_names[label].encode("utf-8", "replace")[:NAME_MAX]
    return "".join(chr(b) if 32 <= b <= 126 else "?" for b in raw)


def selected(dets, count, threshold):
    """select_top_predictions: rows of the first `count` with finite box and score and score > threshold, ascending score, stable; the
    last MAX_DRAWN of them"""
    rows = []
    thr = np.float32(threshold)
    for r in range(int(count)):
        x = dets[r]
        if all(math.isfinite(float(v)) for v in x[:5]) and np.float32(x[4]) > thr:
            rows.append(r)
    rows.sort(key=lambda r: float(dets[r, 4]))          # list.sort is stable
    return rows[-MAX_DRAWN:]


def render(frame, dets, count, ratio, class_names, atlas, threshold=0.7, thickness=2, text_scale=1):
    """-> (the painted copy of uint8 `frame` [h, w, 3], info): info["kind"] [h, w] says what each pixel shows at the end (KIND_*),
    info["cover"] [h, w] how many drawn detections' rings or plates lie over it, info["drawn"] the rows in draw order"""
    out = np.array(frame, copy=True)
    h, w = out.shape[:2]
    kind = np.zeros((h, w), dtype=np.int8)
    cover = np.zeros((h, w), dtype=np.int32)
    dets = np.asarray(dets, dtype=np.float32)
    rw, rh = np.float32(ratio[0]), np.float32(ratio[1])
    t, s = int(thickness), int(text_scale)
    o = t // 2
    i = t - o
    gh, gw = atlas.shape[1:]
    todo = []
    for r in selected(dets, count, threshold):
        with np.errstate(over="ignore"):
            x1, y1, x2, y2 = _to_int(float(dets[r, 0] * rw)), _to_int(float(dets[r, 1] * rh)), _to_int(float(dets[r, 2] * rw)), _to_int(float(dets[r, 3] * rh))
        if x2 < x1 or y2 < y1:
            continue
        label = int(dets[r, 5])
        c = [(label * p) % 255 for p in (2 ** 25 - 1, 2 ** 15 - 1, 2 ** 21 - 1)]          # the reference's BGR triple
        name = _name(class_names, label)
        text = "{}: {:.2f}".format(name, float(dets[r, 4])) if name else "{:.2f}".format(float(dets[r, 4]))
        todo.append((r, x1, y1, x2, y2, (c[2], c[1], c[0]), text))
    masks = [np.zeros((h, w), dtype=bool) for _ in todo]          # what each drawn detection lies over, ring and plate together
    for touched, (_, x1, y1, x2, y2, rgb, _) in zip(masks, todo):          # overlay_boxes
        if x1 + i > x2 - i or y1 + i > y2 - i:
            bands = [(y1 - o, y2 + o, x1 - o, x2 + o)]
        else:
            bands = [(y1 - o, y1 + i - 1, x1 - o, x2 + o), (y2 - i + 1, y2 + o, x1 - o, x2 + o),
                     (y1 + i, y2 - i, x1 - o, x1 + i - 1), (y1 + i, y2 - i, x2 - i + 1, x2 + o)]
        for ya, yb, xa, xb in bands:
            ys, xs = _span(ya, yb, h), _span(xa, xb, w)
            out[ys, xs] = rgb
            kind[ys, xs] = KIND_RING
            touched[ys, xs] = True
    for touched, (_, x1, y1, x2, y2, rgb, text) in zip(masks, todo):          # overlay_class_names
        n = len(text)
        glyphs = np.zeros((gh * s + 2 * s, n * gw * s + 2 * s), dtype=bool)
        for k, ch in enumerate(text):
            cell = np.kron(atlas[ord(ch) - 32] != 0, np.ones((s, s), dtype=bool))
            glyphs[s:s + gh * s, s + k * gw * s:s + (k + 1) * gw * s] = cell
        ys, xs = _span(y1, y1 + glyphs.shape[0] - 1, h), _span(x1, x1 + glyphs.shape[1] - 1, w)
        if ys.stop == ys.start or xs.stop == xs.start:
            continue
        out[ys, xs] = rgb
        kind[ys, xs] = KIND_PLATE
        sub = glyphs[ys.start - y1:ys.stop - y1, xs.start - x1:xs.stop - x1]
        out[ys, xs][sub] = 255
        kind[ys, xs][sub] = KIND_GLYPH
        touched[ys, xs] = True
    for touched in masks:
        cover += touched
    return out, {"kind": kind, "cover": cover, "drawn": [d[0] for d in todo], "texts": [d[6] for d in todo]}
