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

A second file, g20_seq_nms_bounds.npz, holds videos that reach the second trip of every loop of csrc/seqnms.hip (a 256-thread workgroup,
64-lane waves, 64-bit link words); every score is a multiple of 1/8, so ties are frequent.  This generator asserts what each is for:

  g   304 frames, 2 to 8 boxes each and one empty frame: class 3's best path of the first round lies wholly behind frame 256; class 7
      has a trunk that forks into two branches of equal sum ending at frames 209 and 259 (the lower frame wins), and three successive
      paths rooted behind frame 0, the second in front of the first's root; class 12 has two equal tracks that merge (the DP's
      predecessor tie)
  h   8 frames in which class 5 holds 63, 64, 65, 128, 129, 256, 257 and 320 boxes in sixteen clusters, interleaved with a small class 9:
      at least 8 rounds, a rescored box at in-class index >= 256, a backpointer >= 64 on a taken path
  i0, i1, i2   three videos of 9, 1 and 5 frames for ONE call: in i0 every class has links; i1 is a single frame; i2 mixes live classes
      with classes that have boxes but no link.  Most frames hold fewer rows than `cap`, and the rows behind `counts` are copies of live
      rows, not zeros; they come back keep 0, score 0.  A few rows in front of `counts` carry label 0 or 31.  The reference never sees
      those (its class lists are 1..30), so they are left out of the comparison with it and stored with the restatement's result, which
      is this project's contract: kept, score unchanged.

The fixtures live in tests/golden/seqnms/: tests/test_golden_regeneration.py requires every .npz directly under tests/golden/ to come
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

sys.path.insert(0, os.path.dirname(HERE))
import _seq_nms_host as H  # noqa: E402

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


G = 0.125
WIDE = (63, 64, 65, 128, 129, 256, 257, 320)


def case_g():
    v = Video(304, 200)
    v.track(3, 20, 41, (60, 40, 160, 120), (1, 0), 0.5, dup=1, grid=G)
    v.track(3, 262, 304, (60, 40, 160, 120), (1, 0), 0.875, dup=1, grid=G)                                # 36.75 behind frame 256: round 1
    # class 7: the trunk forks at frame 200 into P (10 x 0.75, to frame 209) and Q (60 x 0.125, to frame 259): 20 + 7.5 either way
    v.track(7, 160, 200, (300, 100, 400, 200), (0, 0), 0.5, dup=0)
    v.track(7, 200, 210, (267, 100, 367, 200), (-4, 0), 0.75, dup=0)
    v.track(7, 200, 260, (333, 100, 433, 200), (1, 0), 0.125, dup=0)
    v.track(7, 100, 131, (300, 240, 400, 340), (0, 0), 0.25, dup=1, grid=G)                               # in front of the first path's root
    # class 12: A and B (equal scores, 50..59) both link to the tail's first box at frame 60
    v.track(12, 50, 60, (167, 220, 267, 320), (0, 0), 0.5, dup=0)
    v.track(12, 50, 60, (233, 220, 333, 320), (0, 0), 0.5, dup=0)
    v.track(12, 60, 70, (200, 220, 300, 320), (0, 0), 0.625, dup=0)
    for f in range(304):                                                                                  # clutter away from the tracks
        for _ in range(2):
            x, y = v.rng.uniform(450, 560), v.rng.uniform(0, 300)
            v.add(f, (x, y, x + v.rng.uniform(20, 70), y + v.rng.uniform(20, 50)), G * v.rng.randint(1, 4), (3, 7, 12, 21)[v.rng.randint(4)])
    v.rows[150] = []
    return v.packed()


def case_h():
    v = Video(len(WIDE), 201)
    for f, n in enumerate(WIDE):
        for k in range(n):                                                                                # sixteen clusters, 160 x 90 apart
            c = k % 16
            x, y = 30 + 150 * (c % 4) + v.rng.uniform(-32, 32), 15 + 85 * (c // 4) + v.rng.uniform(-20, 20)
            v.add(f, (x, y, x + 80 + v.rng.uniform(-24, 24), y + 50 + v.rng.uniform(-14, 14)), G * v.rng.randint(1, 8), 5)
    v.track(9, 0, len(WIDE), (250, 150, 330, 230), (3, 1), 0.75, dup=4, grid=G)
    return v.packed()


def _garbage(v, extra):
    """packed, with `extra` more rows per frame and every row behind counts a copy of a live row of the video (score and label included)"""
    dets, counts = v.packed()
    dets = np.concatenate([dets, np.zeros((dets.shape[0], extra, 6), dtype=np.float32)], axis=1)
    live = dets[np.arange(dets.shape[1])[None, :] < counts[:, None]]
    live = live[(live[:, 5] >= 1) & (live[:, 5] <= NUM_CLASSES)]
    for f in range(dets.shape[0]):
        k = dets.shape[1] - counts[f]
        dets[f, counts[f]:] = live[v.rng.randint(len(live), size=k)]
    return dets, counts


def _cell(c):
    x, y = 8 + 105 * ((c - 1) % 6), 6 + 70 * ((c - 1) // 6)
    return (x, y, x + 70, y + 45)


def case_i0():
    v = Video(9, 202)
    for c in range(1, NUM_CLASSES + 1):
        v.track(c, c % 3, 9 - c % 2, _cell(c), (2, 1), lambda f, c=c: G * (2 + (c + f) % 5), dup=1 + c % 2, grid=G)
        if c % 3:                                                                                         # a second, shorter track that crosses the first's 0.3 ring
            x0, y0 = _cell(c)[:2]
            v.track(c, 2, 7, (x0 + 45, y0 + 6, x0 + 115, y0 + 51), (-6, 0), G * (1 + c % 4), dup=c % 2, grid=G)
    for f in (0, 3, 4, 8):
        v.add(f, _cell(4), 0.875, 0)                                                                      # on top of a live track
        v.add(f, _cell(31 - f), 0.875, 31)
    v.clutter(3, [2, 11, 29], grid=G)
    for f in (1, 5):
        v.clutter(1, [6], grid=G)
    return _garbage(v, 4)


def case_i1():
    v = Video(1, 203)
    for c in (1, 7, 30):
        v.track(c, 0, 1, _cell(c), (0, 0), 0.5, dup=2, grid=G)
    v.add(0, _cell(7), 0.25, 31)
    return _garbage(v, 3)


LIVE_I2, LONE_I2, FAR_I2 = (2, 5, 9, 14, 30), (1, 8, 20), 17


def case_i2():
    v = Video(5, 204)
    for c in LIVE_I2:
        v.track(c, c % 2, 5, _cell(c), (3, 0), lambda f, c=c: G * (1 + (c * f) % 6), dup=2, grid=G)
    for c in LONE_I2:                                                                                     # never in two adjacent frames
        for f in (0, 2, 4):
            v.add(f, _cell(c), 0.5, c)
            v.add(f, _cell(c), 0.25, c)
    for f in range(5):                                                                                    # adjacent frames, too far apart to link
        v.add(f, (100 * f, 290, 100 * f + 60, 340), 0.375, FAR_I2)
    v.add(1, _cell(5), 0.75, 0)
    v.add(3, _cell(9), 0.75, 31)
    for f in (0, 4):
        v.clutter(4, [2, 5], grid=G)
    return _garbage(v, 2)


def _in_class(dets, counts, c):
    """per frame the rows of class c, in order"""
    return [np.nonzero(dets[f, :counts[f], 5] == c)[0] for f in range(len(counts))]


def check_bounds(name, dets, counts, keep, scores):
    """what each g20 case is for, from the arrays and the restatement (tests/test_seq_nms.py asserts the same of the stored file)"""
    trace = {}
    hk, hs = H.seq_nms_video(dets, counts, NUM_CLASSES, trace=trace)
    live = np.arange(dets.shape[1])[None, :] < counts[:, None]
    alien = live & ((dets[:, :, 5] < 1) | (dets[:, :, 5] > NUM_CLASSES))
    assert (hk[alien] == 1).all() and np.array_equal(hs[alien], dets[:, :, 4][alien])
    assert np.array_equal(hk[~alien], keep[~alien]) and np.array_equal(hs[~alien].view(np.uint32), scores[~alien].view(np.uint32)), name
    assert not keep[~live].any() and not scores[~live].any()
    assert (dets[:, :, 4] * 8 == np.round(dets[:, :, 4] * 8)).all(), "scores on the 1/8 grid"
    tab = H.class_counts(dets, counts, NUM_CLASSES)
    ends = {c: [(root, root + len(p) - 1) for root, p in t] for c, t in trace.items()}
    if name == "g":
        assert len(counts) >= 300 and counts[150] == 0 and ((counts >= 2) & (counts <= 8))[np.arange(len(counts)) != 150].all()
        assert ends[3][0][0] > 256 and ends[3][0][1] >= 256, "class 3: the first round's winner lies behind frame 256"
        assert ends[7][0] == (160, 209) and (200, 259) in ends[7][1:3], "class 7: of the two equal sums the lower frame wins"
        assert all(r > 0 for r, _ in ends[7][:3]) and ends[7][1][1] < ends[7][0][0], "class 7: three paths rooted behind frame 0, the second in front of the first's root"
        r59 = _in_class(dets, counts, 12)[59]
        a, b = (int(np.nonzero(dets[59, r59, 0] == x)[0][0]) for x in (167, 233))
        assert ends[12][0] == (50, 69) and trace[12][0][1][9] == min(a, b), "class 12: of two equal predecessors the lower row stays"
    if name == "h":
        assert tuple(tab[:, 4]) == WIDE and (tab[:, 8] > 0).all() and len(trace[5]) >= 8
        rows = _in_class(dets, counts, 5)
        assert any(((keep[f, r] == 1) & (scores[f, r] != dets[f, r, 4]))[256:].any() for f, r in enumerate(rows)), "a rescored box at in-class index >= 256"
        assert any(i >= 64 for _, p in trace[5] for i in p[:-1]), "a backpointer >= 64 on a taken path"
        assert any(not np.array_equal(np.sort(r), np.arange(len(r))) for r in rows), "the classes' rows interleave"
    if name == "i0":
        assert len(counts) == 9 and all(len(trace.get(c, ())) >= 1 for c in range(1, NUM_CLASSES + 1)), "every class has links"
    if name == "i1":
        assert len(counts) == 1 and (hk[live] == 1).all()
    if name == "i2":
        assert len(counts) == 5 and all(len(trace[c]) >= 1 for c in LIVE_I2) and all(tab[:, c - 1].sum() > 0 and not trace[c] for c in LONE_I2 + (FAR_I2,))
        assert all(not (tab[:-1, c - 1] * tab[1:, c - 1]).any() for c in LONE_I2) and (tab[:-1, FAR_I2 - 1] * tab[1:, FAR_I2 - 1]).all()
    if name.startswith("i"):
        assert (counts < dets.shape[1]).sum() * 2 > len(counts) and (dets[~live][:, 4] > 0).all() and (dets[~live][:, 5] >= 1).all()
        if name != "i1":
            assert (dets[:, :, 5][live] == 0).any()
        assert (dets[:, :, 5][live] == 31).any()
    return len(trace)


def main_bounds():
    arrs = {}
    for name, make in (("g", case_g), ("h", case_h), ("i0", case_i0), ("i1", case_i1), ("i2", case_i2)):
        dets, counts = make()
        keep, scores = run_reference(dets.copy(), counts)
        alien = (np.arange(dets.shape[1])[None, :] < counts[:, None]) & ((dets[:, :, 5] < 1) | (dets[:, :, 5] > NUM_CLASSES))
        assert not keep[alien].any()                                         # the reference never saw them: the restatement's result instead
        keep[alien], scores[alien] = 1, dets[:, :, 4][alien]
        classes = check_bounds(name, dets, counts, keep, scores)
        arrs.update({name + "_dets": dets, name + "_counts": counts, name + "_keep": keep, name + "_scores": scores})
        print("case", name, "frames", dets.shape[0], "cap", dets.shape[1], "boxes", int(counts.sum()), "kept", int(keep.sum()), "classes", classes)
    np.savez_compressed(os.path.join(OUT, "g20_seq_nms_bounds.npz"), **arrs)
    print("wrote g20_seq_nms_bounds")


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
    main_bounds()
