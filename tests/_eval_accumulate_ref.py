"""What the tests of the evaluators' accumulation share: a second restatement of coco_eval.accumulate_arrays in plain Python -- ONE sort of
the live rows by the tuple (label, -score with -0 folded into +0, image, rank), then loops with integer counters -- and a builder of
synthetic (match, ignore, rank, npig) arrays.  No lexsort, cumsum or searchsorted: if this equals accumulate_arrays, the order that the
device sort has to reproduce is the total order written here."""
import numpy as np

REC_THRS = np.linspace(0, 1, 101)
EPS = float(np.spacing(1))


def accumulate_plain(scores, labels, counts, rank, match, ignore, npig, max_dets, rec_thrs=REC_THRS):
    """-> (precision [T, R, K, A, M], recall [T, K, A, M]) float64; arguments as coco_eval.accumulate_arrays takes them"""
    scores, labels, rank = np.asarray(scores, dtype=np.float32), np.asarray(labels).astype(np.int64), np.asarray(rank)
    match, ignore, npig, counts = np.asarray(match), np.asarray(ignore), np.asarray(npig), np.asarray(counts)
    A, T, N, cap = match.shape
    K, R, M = npig.shape[1] - 1, len(rec_thrs), len(max_dets)
    thr = [np.float64(v) for v in rec_thrs]
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    rows = []
    for f in range(N):
        for r in range(min(max(int(counts[f]), 0), cap)):
            l = int(labels[f, r])
            if rank[f, r] >= 0 and 1 <= l <= K:
                s = np.float32(scores[f, r])
                neg = np.float32(0.0) if s == 0 else -s          # -0 and +0 are one score
                rows.append((l, neg, f, int(rank[f, r]), r))
    rows.sort(key=lambda e: e[:4])          # the total order; nothing is left to the sort's stability
    for k in range(K):
        block = [e for e in rows if e[0] == k + 1]
        for a in range(A):
            n_gt = int(npig[a, k + 1])
            if n_gt <= 0:
                continue
            for mi, max_det in enumerate(max_dets):
                sel = [e for e in block if e[3] < max_det]
                for t in range(T):
                    tp = fp = 0
                    rc, pr = [], []
                    for _, _, f, _, r in sel:
                        if not ignore[a, t, f, r]:
                            if match[a, t, f, r]:
                                tp += 1
                            else:
                                fp += 1
                        rc.append(np.float64(tp) / np.float64(n_gt))
                        pr.append(np.float64(tp) / (np.float64(fp + tp) + np.float64(EPS)))
                    recall[t, k, a, mi] = rc[-1] if sel else 0.0
                    for i in range(len(sel) - 2, -1, -1):          # the greatest precision from row i on
                        if pr[i + 1] > pr[i]:
                            pr[i] = pr[i + 1]
                    i = 0
                    for ri in range(R):          # the first row with rc >= thr; rc never falls and thr rises, so i only moves on
                        while i < len(sel) and rc[i] < thr[ri]:
                            i += 1
                        precision[t, ri, k, a, mi] = pr[i] if i < len(sel) else 0.0
    return precision, recall


def synthetic(seed, images, cap, classes, scores=None, p_match=0.4, p_ignore=0.2, counts=None, max_rank=None, npig=None):
    """random arrays in the matching's layout: dets [N, cap, 6] float32 (only columns 4, 5 matter), counts [N] int32, rank [N, cap] int32
    (a permutation of 0 .. within every (image, label), -1 past max_rank when given), match and ignore [4, 10, N, cap] int8, npig
    [4, classes + 1] int32.  scores: a list to draw from (ties) or None for distinct values."""
    rng = np.random.RandomState(seed)
    N = images
    dets = np.zeros((N, cap, 6), dtype=np.float32)
    dets[:, :, 5] = rng.randint(1, classes + 1, size=(N, cap))
    if scores is None:
        dets[:, :, 4] = ((rng.permutation(N * cap) + 1.0) / (N * cap + 1)).reshape(N, cap)
    else:
        dets[:, :, 4] = np.asarray(scores, dtype=np.float32)[rng.randint(0, len(scores), size=(N, cap))]
    counts = rng.randint(0, cap + 1, size=N).astype(np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
    # a random order within every (image, label): the place within the label's group after a sort by (label, a random number)
    live = np.arange(cap)[None, :] < counts[:, None]
    group = np.where(live, dets[:, :, 5].astype(np.int64), classes + 1)
    order = np.lexsort((rng.rand(N, cap), group), axis=1)
    in_order = np.take_along_axis(group, order, axis=1)
    place = np.broadcast_to(np.arange(cap), (N, cap))
    starts = np.ones((N, cap), dtype=bool)
    starts[:, 1:] = in_order[:, 1:] != in_order[:, :-1]
    rank = np.empty((N, cap), dtype=np.int32)
    np.put_along_axis(rank, order, (place - np.maximum.accumulate(np.where(starts, place, 0), axis=1)).astype(np.int32), axis=1)
    if max_rank is not None:
        rank[rank >= max_rank] = -1
    rank[~live] = -1
    match = (rng.rand(4, 10, N, cap) < p_match).astype(np.int8)
    ignore = (rng.rand(4, 10, N, cap) < p_ignore).astype(np.int8)
    if npig is None:
        npig = rng.randint(0, 30, size=(4, classes + 1)).astype(np.int32)
        npig[rng.rand(4, classes + 1) < 0.2] = 0
    return dets, counts, rank, match, ignore, np.asarray(npig, dtype=np.int32)


def numpy_args(dets, counts, rank, match, ignore, npig):
    """the synthetic tuple -> accumulate_arrays' positional arguments (scores, labels, counts, rank, match, ignore, npig)"""
    return np.ascontiguousarray(dets[:, :, 4]), dets[:, :, 5].astype(np.int64), counts, rank, match, ignore, npig
