"""What the device evaluator's tests share: the goldens g11 / g15 and synthetic sets as packed arrays and as BoxLists, and an
INSTRUMENTED restatement of vid_eval.calc_prec_rec's matching loop that records, at every row's own place, what the loop appends
(match, weight), the row's position in its (frame, class) list (rank) and the counted boxes (n_pos) -- the arrays
ops.vid_eval_match returns.  With `stable` the rows of a (frame, class) are ordered by `argsort(kind="stable")` on the negated scores:
equal scores lower row first, the order the kernel fixes; without it by calc_prec_rec's own `argsort()[::-1]`."""
import numpy as np
import torch

from conftest import golden

from diffusionvid_amd.data.evaluation import vid_eval
from diffusionvid_amd.structures.bounding_box import BoxList

SIZE = (500, 400)


class Case:
    """dets [F, cap, 6] float32, counts [F] int32, gt_boxes [G, 4] float32, gt_labels [G] int32, gt_starts [F + 1] int32, motion [G]
    float64 | None"""

    def __init__(self, dets, counts, gt_boxes, gt_labels, gt_starts, motion=None):
        self.dets, self.counts = np.ascontiguousarray(dets, dtype=np.float32), np.ascontiguousarray(counts, dtype=np.int32)
        self.gt_boxes = np.ascontiguousarray(gt_boxes, dtype=np.float32).reshape(-1, 4)
        self.gt_labels, self.gt_starts = np.ascontiguousarray(gt_labels, dtype=np.int32), np.ascontiguousarray(gt_starts, dtype=np.int32)
        self.motion = None if motion is None else np.ascontiguousarray(motion, dtype=np.float64)

    @property
    def frames(self):
        return len(self.counts)

    def boxlists(self):
        preds, gts = [], []
        for f in range(self.frames):
            n, a, b = int(self.counts[f]), int(self.gt_starts[f]), int(self.gt_starts[f + 1])
            pr = BoxList(torch.from_numpy(self.dets[f, :n, :4].copy()), SIZE)
            pr.add_field("scores", torch.from_numpy(self.dets[f, :n, 4].copy()))
            pr.add_field("labels", torch.from_numpy(self.dets[f, :n, 5].astype(np.int64)))
            gt = BoxList(torch.from_numpy(self.gt_boxes[a:b].copy()), SIZE)
            gt.add_field("labels", torch.from_numpy(self.gt_labels[a:b].astype(np.int64)))
            preds.append(pr)
            gts.append(gt)
        return preds, gts

    def motion_lists(self):
        return None if self.motion is None else [self.motion[self.gt_starts[f]:self.gt_starts[f + 1]].tolist() for f in range(self.frames)]


def pack(frames, motion=None):
    """frames: per frame (pred rows [n, 6], gt boxes [g, 4], gt labels [g]); motion: per frame a list of g floats -> Case"""
    cap = max(1, max((len(p) for p, _, _ in frames), default=1))
    dets, counts = np.zeros((len(frames), cap, 6), dtype=np.float32), np.zeros(len(frames), dtype=np.int32)
    starts = [0]
    for f, (p, gb, gl) in enumerate(frames):
        p = np.asarray(p, dtype=np.float32).reshape(-1, 6)
        dets[f, :len(p)], counts[f] = p, len(p)
        starts.append(starts[-1] + len(gl))
    gb = np.concatenate([np.asarray(b, dtype=np.float32).reshape(-1, 4) for _, b, _ in frames]) if frames else np.zeros((0, 4))
    gl = np.concatenate([np.asarray(l, dtype=np.int32).reshape(-1) for _, _, l in frames]) if frames else np.zeros(0)
    mo = None if motion is None else np.concatenate([np.asarray(m, dtype=np.float64).reshape(-1) for m in motion])
    return Case(dets, counts, gb, gl, starts, mo)


def golden_case(name):
    """g11 (one range) or g15 (four, with motion IoUs) -> (Case, the npz)"""
    z = golden(name)
    if name == "g11_vid_eval":
        keys, n = ("pr_box_%d", "pr_sc_%d", "pr_lab_%d", "gt_box_%d", "gt_lab_%d"), int(z["nframes"])
    else:
        keys, n = ("pr_boxes%d", "pr_scores%d", "pr_labels%d", "gt_boxes%d", "gt_labels%d"), int(z["n_frames"])
    frames, motion = [], []
    for f in range(n):
        pb, ps, pl, gb, gl = (z[k % f] for k in keys)
        frames.append((np.concatenate((pb.reshape(-1, 4), ps.reshape(-1, 1), pl.reshape(-1, 1)), axis=1), gb.reshape(-1, 4), gl))
        if name != "g11_vid_eval":
            motion.append(z["motion%d" % f])
    return pack(frames, motion or None), z


def random_case(seed, frames=64, cap=48, max_gt=6, classes=30, ties=False):
    """seeded frames with 0 .. cap rows and 0 .. max_gt boxes; about half the rows are jittered copies of a box of the frame, so every
    branch of the matching is met.  Scores are distinct over the whole set (a shuffled grid), or drawn from five values with `ties`.
    Motion IoUs include 0.7 and 0.9 exactly."""
    rng = np.random.RandomState(seed)
    grid = rng.permutation(frames * cap).astype(np.float32) / np.float32(frames * cap)
    out, motion = [], []
    for f in range(frames):
        g = int(rng.randint(0, max_gt + 1))
        xy = rng.uniform(0, 300, size=(g, 2))
        gb = np.concatenate((xy, xy + rng.uniform(10, 150, size=(g, 2))), axis=1).astype(np.float32)
        gl = rng.randint(1, classes + 1, size=g) if g == 0 or rng.rand() < 0.5 else np.full(g, rng.randint(1, classes + 1))
        if g > 1 and rng.rand() < 0.3:
            gb[1] = gb[0]          # two identical boxes: the exact IoU tie
            gl[1] = gl[0]
        n = int(rng.randint(0, cap + 1)) if f % 7 else (0 if f % 14 else cap)
        p = np.zeros((n, 6), dtype=np.float32)
        xy = rng.uniform(0, 300, size=(n, 2))
        p[:, :4] = np.concatenate((xy, xy + rng.uniform(10, 150, size=(n, 2))), axis=1)
        p[:, 5] = rng.randint(1, classes + 1, size=n)
        for i in range(n):
            if g and rng.rand() < 0.5:
                k = int(rng.randint(g))
                p[i, :4] = gb[k] + (rng.randint(-12, 13, size=4) if rng.rand() < 0.7 else 0)
                p[i, 5] = gl[k] if rng.rand() < 0.8 else p[i, 5]
        p[:, 4] = rng.choice(np.array([0.9, 0.5, 0.25, 0.1, 0.0], dtype=np.float32), size=n) if ties else grid[f * cap:f * cap + n]
        out.append((p, gb, gl))
        motion.append(rng.choice([0.0, 0.3, 0.7, 0.8, 0.9, 0.95, 1.0], size=g))
    return pack(out, motion)


def cpu_matches(case, ranges=((0.0, 1.0),), iou_thresh=0.5, num_classes=30, stable=False, use_motion=True):
    """vid_eval.calc_prec_rec lines 50-102 per range, recording instead of appending -> match [R, F, cap] int8, weight [R, F, cap]
    float64, rank [F, cap] int32 (-1 behind counts), n_pos [R, num_classes + 1] float64"""
    F, cap = case.dets.shape[:2]
    R = len(ranges)
    match, weight = np.zeros((R, F, cap), dtype=np.int8), np.zeros((R, F, cap), dtype=np.float64)
    rank, n_pos = np.full((F, cap), -1, dtype=np.int32), np.zeros((R, num_classes + 1), dtype=np.float64)
    motion = case.motion if use_motion else None
    for r, (lo, hi) in enumerate(ranges):
        empty_w = 0.0
        if motion is not None:
            empty_w = float(((motion >= lo) & (motion <= hi)).sum() / float(len(motion))) if len(motion) else 0.0
            if empty_w == 1:
                empty_w = 0.0
        for f in range(F):
            n, a, b = int(case.counts[f]), int(case.gt_starts[f]), int(case.gt_starts[f + 1])
            pb, ps, pl = case.dets[f, :n, :4], case.dets[f, :n, 4], case.dets[f, :n, 5].astype(np.int64)
            gb, gl = case.gt_boxes[a:b], case.gt_labels[a:b].astype(np.int64)
            ignored = np.zeros(len(gb))
            if motion is not None and b > a:
                mi = motion[a:b]
                ignored = ((mi < lo) | (mi > hi)).astype(np.float64)
            for l in np.unique(np.concatenate((pl, gl)).astype(int)):
                rows = np.nonzero(pl == l)[0]
                order = (-ps[rows]).argsort(kind="stable") if stable else ps[rows].argsort()[::-1]
                rows = rows[order]
                rank[f, rows] = np.arange(len(rows))
                gb_l, ig_l = gb[gl == l], ignored[gl == l]
                n_pos[r, l] += gb_l.shape[0] - ig_l.sum()
                if len(rows) == 0:
                    continue
                if len(gb_l) == 0:
                    weight[r, f, rows] = empty_w
                    continue
                iou = vid_eval._iou_vid(pb[rows], gb_l)
                taken = np.zeros(gb_l.shape[0], dtype=bool)
                for j in range(iou.shape[0]):
                    best, arg = iou_thresh, -1
                    top_ig = top_cnt = -1.0
                    for k in range(iou.shape[1]):
                        v = iou[j, k]
                        if ig_l[k] == 1:
                            top_ig = max(top_ig, v)
                        else:
                            top_cnt = max(top_cnt, v)
                        if taken[k] or v < best:
                            continue
                        if v == best and arg >= 0 and not ig_l[arg]:
                            continue
                        best, arg = v, k
                    if arg >= 0:
                        taken[arg] = True
                        match[r, f, rows[j]], weight[r, f, rows[j]] = 1, ig_l[arg]
                    else:
                        weight[r, f, rows[j]] = 0.0 if top_cnt > top_ig else (1.0 if top_ig > top_cnt else ig_l.sum() / float(len(ig_l)))
    return match, weight, rank, n_pos


def same_ap(got, want):
    """two results of eval_detection_vid (a dict, or a list of them): the `ap` arrays equal element for element (NaNs equal), `map` equal"""
    got, want = (x if isinstance(x, (list, tuple)) else [x] for x in (got, want))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["ap"].shape == w["ap"].shape and np.array_equal(g["ap"], w["ap"], equal_nan=True), (g["ap"], w["ap"])
        assert g["map"] == w["map"] or (np.isnan(g["map"]) and np.isnan(w["map"]))
