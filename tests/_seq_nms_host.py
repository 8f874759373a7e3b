"""Seq-NMS restated in plain numpy on the packed layout (dets [frames, cap, 6] = box4, score, label; counts [frames]): the expected values
of the CPU tests, the stand-in for the kernel where a test has no GPU, and the host side of tools/bench_seq_nms.py.

It follows the reference's seq_nms.py statement by statement (createLinks, maxPath, findMaxPath, rescore, deleteLink) per class, and is
pinned to it bit for bit by tests/golden/seqnms/g19_seq_nms.npz (tests/test_seq_nms.py).  Arithmetic as the reference's: IoU terms and
the running sums in float32, `maxsum < 1e-2` in float64, `maxsum / len` a float64 quotient rounded to float32.
"""
import numpy as np

IOU_THRESH = np.float32(0.5)
NMS_THRESH = np.float32(0.3)
MAX_THRESH = 1e-2
ONE = np.float32(1)
ZERO = np.float32(0)


def _areas(b):
    return (b[:, 2] - b[:, 0] + ONE) * (b[:, 3] - b[:, 1] + ONE)


def _iou(box, area, boxes, areas):
    """seq_nms.py:69-76 / :191-199"""
    x1 = np.maximum(box[0], boxes[:, 0])
    y1 = np.maximum(box[1], boxes[:, 1])
    x2 = np.minimum(box[2], boxes[:, 2])
    y2 = np.minimum(box[3], boxes[:, 3])
    w = np.maximum(ZERO, x2 - x1 + ONE)
    h = np.maximum(ZERO, y2 - y1 + ONE)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area + areas - inter)


def seq_nms_class(boxes, scores, trace=None):
    """One class of one video.  boxes: list over frames of [n_f, 4] float32, scores: list of [n_f] float32; both are changed in place
    (suppressed rows zeroed, path rows rescored).  Returns (deleted: list of bool [n_f], rounds).  A list given as `trace` receives one
    (root frame, path) per round: path[i] is the in-class index of the path's box in frame root + i."""
    F = len(boxes)
    deleted = [np.zeros(len(s), dtype=bool) for s in scores]
    on_path = [np.zeros(len(s), dtype=bool) for s in scores]
    links = []
    for f in range(F - 1):
        a1, a2 = _areas(boxes[f]), _areas(boxes[f + 1])
        m = np.zeros((len(a1), len(a2)), dtype=bool)
        for i in range(len(a1)):
            m[i] = _iou(boxes[f][i], a1[i], boxes[f + 1], a2) >= IOU_THRESH
        links.append(m)
    sum_links = int(sum(int(m.sum()) for m in links))
    a = [None] * F
    b = [None] * F
    fmax = np.full(F, -np.inf, dtype=np.float32)
    farg = np.zeros(F, dtype=np.int64)
    start, rounds = 0, 0
    while True:
        # findMaxPath: a[l] for l below the last path's root has not changed
        for f in range(start, F):
            s = scores[f]
            init = np.where(on_path[f], ZERO, s).astype(np.float32)
            back = np.full(len(s), -1, dtype=np.int64)
            if f > 0 and len(s) and len(a[f - 1]):
                cand = np.where(links[f - 1], a[f - 1][:, None] + s[None, :], np.float32(-np.inf)).astype(np.float32)
                arg = cand.argmax(axis=0)                      # first occurrence: the lowest predecessor
                best = cand[arg, np.arange(len(s))]
                upd = best > init
                init = np.where(upd, best, init).astype(np.float32)
                back = np.where(upd, arg, back)
            a[f], b[f] = init, back
            if len(s):
                farg[f] = int(init.argmax())
                fmax[f] = init[farg[f]]
            else:
                fmax[f] = -np.inf
        f = int(fmax.argmax())                                  # row-major first occurrence
        maxsum = fmax[f]
        if not maxsum > 0 or float(maxsum) < MAX_THRESH or sum_links == 0:
            break
        rounds += 1
        j = int(farg[f])
        path = [j]
        while b[f][j] != -1:
            j = int(b[f][j])
            f -= 1
            path.append(j)
        root = f
        path.reverse()
        if trace is not None:
            trace.append((root, list(path)))
        fresh = np.float32(np.float64(maxsum) / len(path))
        for i, p in enumerate(path):
            scores[root + i][p] = fresh
            on_path[root + i][p] = True
        # deleteLink on the boxes as they stand; the zeroing follows it
        dels = []
        for i, p in enumerate(path):
            f = root + i
            ar = _areas(boxes[f])
            d = np.nonzero(_iou(boxes[f][p], ar[p], boxes[f], ar) >= NMS_THRESH)[0]
            dels.append(d)
            if f < F - 1:
                sum_links -= int(links[f][d].sum())
                links[f][d] = False
            if f > 0:
                sum_links -= int(links[f - 1][:, d].sum())
                links[f - 1][:, d] = False
        for i, p in enumerate(path):
            f = root + i
            for k in dels[i]:
                if k != p:
                    boxes[f][k] = 0
                    scores[f][k] = 0
                    deleted[f][k] = True
        start = root
    return deleted, rounds


def seq_nms_video(dets, counts, num_classes, progress=None, trace=None):
    """dets [frames, cap, 6], counts [frames] -> (keep [frames, cap] uint8, scores [frames, cap] float32), as ops.seq_nms_video.
    `progress(c, rounds)` is called per class that has a box; a dict given as `trace` receives {c: seq_nms_class's trace}."""
    dets = np.asarray(dets, dtype=np.float32)
    counts = np.asarray(counts).astype(np.int64)
    F, cap = dets.shape[:2]
    keep = (np.arange(cap)[None, :] < counts[:, None]).astype(np.uint8)
    out = np.where(keep.astype(bool), dets[:, :, 4], ZERO).astype(np.float32)
    labels = dets[:, :, 5].astype(np.int64)
    for c in range(1, num_classes + 1):
        rows = [np.nonzero(labels[f, :counts[f]] == c)[0] for f in range(F)]
        if sum(len(r) for r in rows) == 0:
            continue
        boxes = [dets[f, rows[f], :4].copy() for f in range(F)]
        scores = [dets[f, rows[f], 4].copy() for f in range(F)]
        deleted, rounds = seq_nms_class(boxes, scores, None if trace is None else trace.setdefault(c, []))
        if progress is not None:
            progress(c, rounds)
        for f in range(F):
            keep[f, rows[f]] = ~deleted[f]
            out[f, rows[f]] = scores[f]
    return keep, out


def seq_nms_rounds(dets, counts, num_classes, video_starts=None):
    """(keep, scores, rounds [n_videos, num_classes] int32): seq_nms_video per video, with the paths each class gave up -- the status
    words of ops.seq_nms_video(..., return_status=True)"""
    dets, counts = np.asarray(dets, dtype=np.float32), np.asarray(counts)
    starts = [0, len(counts)] if video_starts is None else [int(v) for v in video_starts]
    keep = np.zeros(dets.shape[:2], dtype=np.uint8)
    out = np.zeros(dets.shape[:2], dtype=np.float32)
    rounds = np.zeros((len(starts) - 1, num_classes), dtype=np.int32)
    for v in range(len(starts) - 1):
        a, b = starts[v], starts[v + 1]
        keep[a:b], out[a:b] = seq_nms_video(dets[a:b], counts[a:b], num_classes, progress=lambda c, r, v=v: rounds.__setitem__((v, c - 1), r))
    return keep, out, rounds


def class_counts(dets, counts, num_classes):
    """[frames, num_classes] int32: the frame's detections with label c + 1 (what ops.seq_nms_video sizes its scratch from)"""
    dets = np.asarray(dets)
    counts = np.asarray(counts).astype(np.int64)
    F = dets.shape[0]
    t = np.zeros((F, num_classes), dtype=np.int32)
    for f in range(F):
        lab = dets[f, :counts[f], 5].astype(np.int64)
        lab = lab[(lab >= 1) & (lab <= num_classes)]
        t[f] = np.bincount(lab - 1, minlength=num_classes)
    return t


def scratch_bytes(table, video_starts):
    """the formula of include/dvid_hip.h (dvid_seq_nms_scratch_bytes)"""
    r16 = lambda x: (x + 15) // 16 * 16          # noqa: E731
    table = np.asarray(table, dtype=np.int64)
    C = table.shape[1]
    total = 0
    for v in range(len(video_starts) - 1):
        t = table[video_starts[v]:video_starts[v + 1]]
        F = t.shape[0]
        for c in range(C):
            n = t[:, c]
            L = int((n[:-1] * ((n[1:] + 63) // 64)).sum()) if F > 1 else 0
            if L == 0:
                continue
            total += r16(12 * (F + 1)) + r16(8 * (L + int(((n + 63) // 64).sum())) + 36 * int(n.sum()) + 12 * F)
    return total + r16(40 * (len(video_starts) - 1) * C) if total else 0
