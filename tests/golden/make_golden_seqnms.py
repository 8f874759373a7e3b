"""Generate the golden vectors of Seq-NMS by running the REFERENCE's own seq_nms.py (build container only).

    python tests/golden/make_golden_seqnms.py

Six small synthetic videos (a few moving tracks with near-duplicates, plus clutter; all 30 class lists allocated) go through the
reference's `seq_nms(dets)` on its own `BoxList`s, split by label as this project's hand-over defines it.  Only data is stored, in the
packed layout of engine.pack_predictions: per case `dets` [frames, cap, 6] (box4, score, label), `counts` [frames], and the reference's
result as `keep` [frames, cap] (uint8) and `scores` [frames, cap] (the rescored values; 0 for a dropped row).

  a  12 frames: several tracks per class, a class absent from the middle frames, a class with no box at all
  b  1 frame
  c  6 frames: one class holds 130 boxes in one frame (two 64-bit link words, more than a wave); scores on a coarse grid, so that the
     ties of the DP predecessor, of the argmax and of two equal-sum paths all occur
  d  a class whose links remain while every path sums below 1e-2 (the early stop), and a class where a lone box outscores every linked
     path and is taken as a path of length 1 while links remain
  e  a tiny box at the image origin whose IoU with an already-zeroed (0, 0, 0, 0) box is >= 0.3
  f  one 40-frame track whose sequential float32 sum differs from the float64 sum in the rescored bits (asserted here)

The fixture lives in tests/golden/seqnms/: tests/test_golden_regeneration.py requires every .npz directly under tests/golden/ to come
out of make_golden.py, which this generator must not touch.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.environ.get("DVID_GOLDEN_OUT", os.path.join(HERE, "seqnms"))
import _ref_shims as S  # noqa: E402

S.install()

import torch  # noqa: E402

from mega_core.structures.bounding_box import BoxList  # noqa: E402
from seq_nms import seq_nms  # noqa: E402

NUM_CLASSES = 30
SIZE = (640, 360)


class Video:
    def __init__(self, frames, seed):
        self.rows = [[] for _ in range(frames)]
        self.rng = np.random.RandomState(seed)

    def add(self, f, box, score, label):
        self.rows[f].append([float(v) for v in box] + [float(score), float(label)])

    def track(self, label, f0, f1, box, vel, score, dup=2, jitter=3.0, dup_score=0.6, grid=None):
        """one box per frame moving by `vel`, with `dup` jittered near-duplicates of lower score"""
        box = np.asarray(box, dtype=np.float64)
        for f in range(f0, f1):
            b = box + (f - f0) * np.asarray(list(vel) * 2, dtype=np.float64)
            s = score(f) if callable(score) else score
            self.add(f, b, s, label)
            for _ in range(dup):
                sd = s * dup_score * (0.7 + 0.3 * self.rng.rand())
                if grid:
                    sd = max(grid, round(sd / grid) * grid)
                self.add(f, b + self.rng.uniform(-jitter, jitter, 4), sd, label)

    def clutter(self, n_per_frame, labels, lo=0.02, hi=0.2, grid=None):
        for f in range(len(self.rows)):
            for _ in range(n_per_frame):
                x, y = self.rng.uniform(0, SIZE[0] - 80), self.rng.uniform(0, SIZE[1] - 60)
                w, h = self.rng.uniform(10, 80), self.rng.uniform(10, 60)
                s = self.rng.uniform(lo, hi)
                if grid:
                    s = max(grid, round(s / grid) * grid)
                self.add(f, (x, y, x + w, y + h), s, labels[self.rng.randint(len(labels))])

    def packed(self, shuffle=True):
        cap = max(1, max(len(r) for r in self.rows))
        dets = np.zeros((len(self.rows), cap, 6), dtype=np.float32)
        counts = np.zeros((len(self.rows),), dtype=np.int32)
        for f, r in enumerate(self.rows):
            if r:
                a = np.asarray(r, dtype=np.float32)
                if shuffle:
                    a = a[self.rng.permutation(len(a))]
                dets[f, :len(a)] = a
            counts[f] = len(r)
        return dets, counts


def run_reference(dets, counts):
    """the reference on the packed layout: class lists of per-frame BoxLists in, (keep, scores) out"""
    frames, cap = dets.shape[:2]
    video = []
    for c in range(1, NUM_CLASSES + 1):
        per_frame = []
        for f in range(frames):
            rows = np.nonzero(dets[f, :counts[f], 5] == c)[0]
            bl = BoxList(torch.from_numpy(dets[f, rows, :4].copy()).reshape(-1, 4), SIZE, mode="xyxy")
            bl.add_field("scores", torch.from_numpy(dets[f, rows, 4].copy()))
            bl.add_field("orig", torch.from_numpy(rows.astype(np.int64)))
            per_frame.append(bl)
        video.append(per_frame)
    out = seq_nms(video)
    keep = np.zeros((frames, cap), dtype=np.uint8)
    scores = np.zeros((frames, cap), dtype=np.float32)
    for per_frame in out:
        for f, bl in enumerate(per_frame):
            rows = bl.get_field("orig").numpy()
            keep[f, rows] = 1
            scores[f, rows] = bl.get_field("scores").numpy()
    return keep, scores


def case_a():
    v = Video(12, 190)
    v.track(1, 0, 12, (40, 40, 140, 120), (6, 2), lambda f: 0.55 + 0.03 * f)
    v.track(1, 2, 10, (300, 200, 380, 300), (-5, 1), 0.7)
    v.track(1, 0, 5, (500, 50, 600, 150), (3, 3), lambda f: 0.4 + 0.05 * (f % 3), dup=1)
    v.track(2, 0, 12, (100, 150, 260, 330), (2, -1), lambda f: 0.9 - 0.02 * f, dup=3)
    v.track(2, 5, 12, (420, 30, 520, 110), (8, 4), 0.35)
    v.track(3, 1, 11, (200, 60, 330, 190), (12, 0), lambda f: 0.5 + 0.4 * ((f * 7) % 5) / 5)          # fast: some frames do not link
    v.track(5, 0, 4, (60, 220, 150, 320), (4, 0), 0.8)                                                    # class 5: absent from frames 4..6
    v.track(5, 7, 12, (88, 220, 178, 320), (4, 0), 0.75)
    v.track(30, 0, 12, (350, 100, 450, 260), (1, 1), lambda f: 0.3 + 0.05 * f, dup=2)
    v.track(30, 0, 12, (380, 120, 470, 270), (1, 1), lambda f: 0.6 - 0.03 * f, dup=0)                   # crosses the other's 0.3 neighbourhood
    v.clutter(8, [1, 2, 3, 7, 12, 30])                                                                    # class 9 (and most others): no box
    return v.packed()


def case_b():
    v = Video(1, 191)
    v.track(1, 0, 1, (40, 40, 140, 120), (0, 0), 0.8)
    v.track(4, 0, 1, (300, 100, 400, 220), (0, 0), 0.6)
    v.clutter(6, [1, 4, 8])
    return v.packed()


def case_c():
    G = 0.125
    v = Video(6, 192)
    # class 4: two identical-score tracks far apart (two equal-sum paths), near-duplicates on the score grid
    v.track(4, 0, 6, (30, 30, 130, 130), (5, 0), 0.75, dup=4, grid=G)
    v.track(4, 0, 6, (330, 30, 430, 130), (5, 0), 0.75, dup=4, grid=G)
    v.track(4, 1, 5, (180, 200, 300, 330), (3, 2), lambda f: G * (3 + f % 3), dup=3, grid=G)
    # frame 2 grows to 130 boxes of class 4: a dense cloud around the third track, every score on the grid
    have = sum(1 for r in v.rows[2] if r[5] == 4)
    base = np.asarray((186, 204, 306, 334), dtype=np.float64)
    for k in range(130 - have):
        v.add(2, base + v.rng.uniform(-14, 14, 4), G * (1 + k % 3), 4)
    v.track(11, 0, 6, (480, 220, 600, 340), (0, 0), 0.5, dup=2, jitter=0.0, grid=G)                    # identical boxes, tied scores
    v.clutter(5, [4, 11, 20], grid=G)
    assert sum(1 for r in v.rows[2] if r[5] == 4) >= 130
    return v.packed()


def case_d():
    v = Video(5, 193)
    v.track(6, 0, 5, (50, 50, 150, 150), (2, 2), 0.0015, dup=1, dup_score=0.5)                           # links, every path below 1e-2
    v.add(2, (400, 200, 500, 300), 0.95, 8)                                                              # alone: a path of length 1 ...
    v.track(8, 0, 5, (100, 200, 200, 300), (3, 0), lambda f: 0.16 + 0.01 * f, dup=1)                                          # ... while this 0.9-sum path waits
    v.add(2, (405, 204, 503, 302), 0.5, 8)                                                               # inside the lone box's 0.3 ring
    v.track(9, 0, 5, (300, 30, 380, 110), (2, 1), 0.4, dup=1)
    return v.packed()


def case_e():
    v = Video(4, 194)
    v.track(2, 0, 4, (0, 0, 90, 70), (0, 0), lambda f: 0.8 - 0.05 * f, dup=3, jitter=2.0)          # its duplicates are zeroed to (0, 0, 0, 0) first
    for f in range(4):                                                       # then the tiny box at the origin: IoU with a zero box 1 / 2.25
        v.add(f, (0, 0, 0.5, 0.5), 0.3, 2)
        v.add(f, (200, 100, 280, 190), 0.2, 2)
    dets, counts = v.packed()
    return np.maximum(dets, 0), counts                                       # the jittered duplicates stay inside the image


def case_f():
    for seed in range(195, 260):          # the first seed whose scores tell the two accumulations apart
        v = Video(40, seed)
        s = v.rng.uniform(0.05, 0.95, 40).astype(np.float32)
        v.track(3, 0, 40, (100, 100, 220, 240), (2, 1), lambda f: s[f], dup=0)
        dets, counts = v.packed()
        acc32 = np.float32(0)
        for x in dets[:, 0, 4]:
            acc32 = np.float32(acc32 + x)
        as32 = np.float32(np.float64(acc32) / 40)
        as64 = np.float32(dets[:, 0, 4].astype(np.float64).sum() / 40)
        if as32 != as64:
            return dets, counts, as32
    raise AssertionError("case f must tell the float32 accumulation from a float64 one")


def main():
    arrs = {}
    for name, make in (("a", case_a), ("b", case_b), ("c", case_c), ("d", case_d), ("e", case_e), ("f", case_f)):
        made = make()
        dets, counts = made[0], made[1]
        keep, scores = run_reference(dets.copy(), counts)
        live = np.arange(dets.shape[1])[None, :] < counts[:, None]
        assert not keep[~live].any()
        if name == "b":
            assert (keep == live).all() and np.array_equal(scores, np.where(live, dets[:, :, 4], 0))
        if name == "d":
            six = live & (dets[:, :, 5] == 6)
            assert keep[six].all() and np.array_equal(scores[six], dets[:, :, 4][six]), "class 6 stops before its first path"
            lone = live & (dets[:, :, 4] == np.float32(0.95))
            assert lone.sum() == 1 and keep[lone].all() and scores[lone][0] == np.float32(0.95)
            ring = live & (dets[:, :, 5] == 8) & (dets[:, :, 4] == np.float32(0.5))
            assert ring.sum() == 1 and not keep[ring].any(), "the length-1 path suppresses its neighbourhood"
        if name == "e":
            tiny = live & (dets[:, :, 2] == np.float32(0.5))
            assert tiny.sum() == 4 and keep[tiny].all()
        if name == "f":
            assert keep[live].all() and (scores[live] == made[2]).all(), "the reference accumulates in float32"
        arrs.update({name + "_dets": dets, name + "_counts": counts, name + "_keep": keep, name + "_scores": scores})
        print("case", name, "frames", dets.shape[0], "cap", dets.shape[1], "boxes", int(counts.sum()), "kept", int(keep.sum()),
              "rescored", int((live & (keep == 1) & (scores != dets[:, :, 4])).sum()))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "g19_seq_nms.npz"), **arrs)
    print("wrote g19_seq_nms")


if __name__ == "__main__":
    main()
