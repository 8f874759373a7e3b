"""ops.bbox_aug_merge (+ ops.bbox_aug_finish: the tiled NMS and the cut) against tests/_bbox_aug_ref.py on hand-placed boxes with distinct
scores: the mapped candidates bit for bit against BoxList on the CPU before any NMS, then the survivors."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _bbox_aug_ref as R  # noqa: E402
from test_bbox_aug import _aug, _cfg  # noqa: E402

THR = 0.5
SMALL_SIZES = ["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 1000]
AUGS = {1: _aug(extra=SMALL_SIZES), 2: _aug(True, extra=SMALL_SIZES), 4: _aug(True, (64,), True, extra=SMALL_SIZES)}
IMAGES_WH = [(50, 70), (70, 50), (64, 64)]          # 50 x 70: view 0 is 96 x 134, the scale-64 views 64 x 89 -- rw = 1.5, rh = 134 / 89


@functools.lru_cache(maxsize=None)
def _views(V, size_wh):
    from diffusionvid_amd.data.transforms import bbox_aug_views
    views = bbox_aug_views(_cfg(AUGS[V]), size_wh)
    assert len(views) == V
    return views


def _cells(w0, h0):
    """disjoint 12 x 10 cells in view 0, 16 apart; the last one hangs over the right and bottom edge"""
    cells = [(2.0 + 16 * i, 3.0 + 14 * j, 14.0 + 16 * i, 13.0 + 14 * j) for j in range(int((h0 - 16) // 14)) for i in range(int((w0 - 16) // 16))]
    return cells + [(w0 - 9.0, h0 - 8.0, w0 + 3.5, h0 + 2.5)]


def _inputs(n, V, cap, counts, seed):
    """per (image, view) `counts` rows: row r of a view is a cell of view 0 (cells in turn, the view's own start), jittered by up to 0.4
    and carried into the view's frame -- so two candidates of one image are near-duplicates (one cell) or disjoint; labels 1 .. 3 by
    cell; pairwise distinct scores.  The overhanging cell is only placed in views that are not mirrored (its mirror would start left of 0)."""
    g = torch.Generator().manual_seed(seed)
    boxes, labels = torch.zeros(n * V, cap, 4), torch.zeros(n * V, cap, dtype=torch.int32)
    scores = torch.zeros(n * V, cap)
    pool = torch.linspace(0.05, 0.95, n * V * cap)[torch.randperm(n * V * cap, generator=g)].view(n * V, cap)
    for i in range(n):
        views = _views(V, IMAGES_WH[i % 3])
        cells = _cells(views[0].w, views[0].h)
        for v, view in enumerate(views):
            usable = cells[:-1] if view.flip else cells
            for r in range(counts[i * V + v]):
                c = (r + 5 * v) % len(usable)
                x1, y1, x2, y2 = (torch.tensor(usable[c]) + (torch.rand(4, generator=g) - 0.5) * 0.8).tolist()
                x1, x2, y1, y2 = x1 * view.w / views[0].w, x2 * view.w / views[0].w, y1 * view.h / views[0].h, y2 * view.h / views[0].h
                if view.flip:
                    x1, x2 = view.w - x2 - 1, view.w - x1 - 1
                boxes[i * V + v, r] = torch.tensor([x1, y1, x2, y2])
                labels[i * V + v, r] = 1 + (c + v // 2) % 3          # views 2, 3 name a cell's class differently: overlap across classes
                scores[i * V + v, r] = pool[i * V + v, r]
    return boxes, scores, labels, torch.tensor(counts, dtype=torch.int32)


def _counts(mode, n, V, cap):
    if mode == "full":
        return [cap] * (n * V)
    if mode == "empty":
        return [0] * (n * V)
    # mixed: per view 0, full, or something in between; image 1 (where there is one) has no detection in any view
    pattern = [cap // 2 + 1, cap, 0, max(1, cap - 1)]
    return [0 if (n > 1 and k // V == 1) else pattern[k % 4] for k in range(n * V)]


def _check(n, V, cap, mode, max_det):
    from diffusionvid_amd import ops
    counts = _counts(mode, n, V, cap)
    boxes, scores, labels, cnt = _inputs(n, V, cap, counts, seed=1000 * V + cap)
    all_views = [_views(V, IMAGES_WH[i % 3]) for i in range(n)]
    table = ops.bbox_aug_table(all_views)
    cb, cs, cl, live = ops.bbox_aug_merge(boxes.cuda(), scores.cuda(), labels.cuda(), cnt.cuda(), table.cuda(), V)
    N = V * cap
    assert cb.shape == (n, N, 4) and cs.shape == (n, N) and cl.shape == (n, N) and cl.dtype == torch.int32
    sizes0 = torch.tensor([(vs[0].w, vs[0].h) for vs in all_views], dtype=torch.float32)
    ob, osc, ol, oc = ops.bbox_aug_finish(cb, cs, cl, live, sizes0, THR, max_det)
    cb, cs, cl, live, ob, osc, ol, oc = (t.cpu() for t in (cb, cs, cl, live, ob, osc, ol, oc))
    clipped = 0
    for i, views in enumerate(all_views):
        per_view = [R.boxlist(boxes[i * V + v, :counts[i * V + v]], scores[i * V + v, :counts[i * V + v]], labels[i * V + v, :counts[i * V + v]],
                              (view.w, view.h)) for v, view in enumerate(views)]
        wb, ws, wl = R.candidates(per_view, views)
        k = sum(counts[i * V:(i + 1) * V])
        assert int(live[i]) == k == len(ws)
        # the mapped candidates, bit for bit, before any NMS; behind them the padding rows
        assert torch.equal(cb[i, :k], wb) and torch.equal(cs[i, :k], ws) and torch.equal(cl[i, :k].to(torch.int64), wl), f"image {i}"
        assert not cb[i, k:].any() and bool((cs[i, k:] == torch.finfo(torch.float32).tiny).all()) and bool((cl[i, k:] == 1).all())
        if V == 1:
            assert torch.equal(cb[i, :k], boxes[i, :k])          # view 0 is a copy
        if k:
            assert R.iou_margin(wb, wl, THR) >= 0.05
        want = R.merge(per_view, views, THR, max_det)
        m = int(oc[i])
        assert m == len(want), f"image {i}: {m} survivors, the restatement keeps {len(want)}"
        assert torch.equal(ob[i, :m], want.bbox) and torch.equal(osc[i, :m], want.get_field("scores"))
        assert torch.equal(ol[i, :m].to(torch.int64), want.get_field("labels"))
        if max_det and k:
            assert m <= max_det
        clipped += int((wb[:, 2] > views[0].w - 1).sum())
    return clipped


@pytest.mark.parametrize("n,V,cap,mode,max_det", [
    (1, 1, 40, "mixed", 100),          # identity
    (3, 2, 64, "mixed", 100),          # the mirror alone; image 1 empty in every view
    (3, 4, 65, "mixed", 20),           # rw != rh, the cut
    (3, 4, 40, "full", 0),             # every view full, no cut
    (1, 4, 1, "full", 100),
    (1, 2, 1, "empty", 100),
    (3, 4, 64, "mixed", 7),
    (1, 4, 1024, "full", 100),         # V * cap = 4096, the NMS's limit
])
def test_merge_equals_boxlist_then_the_restatement(n, V, cap, mode, max_det):
    clipped = _check(n, V, cap, mode, max_det)
    if V == 4 and cap >= 40:
        assert clipped > 0          # a mapped box reached beyond view 0 and the NMS clipped it


def test_ratios_differ_and_merge_refuses_what_it_cannot_take():
    from diffusionvid_amd import ops
    t = ops.bbox_aug_table([_views(4, (50, 70))])
    assert t[2, 3] != t[2, 4] and t[1, 3:].tolist() == [1.0, 1.0]
    z = torch.zeros
    with pytest.raises(ops._lib.DvidError, match="4100 candidates"):
        ops.bbox_aug_merge(z(4, 1025, 4).cuda(), z(4, 1025).cuda(), z(4, 1025, dtype=torch.int32).cuda(), z(4, dtype=torch.int32).cuda(), z(4, 5).cuda(), 4)
    with pytest.raises(ops._lib.DvidError, match="do not split"):
        ops.bbox_aug_merge(z(3, 8, 4).cuda(), z(3, 8).cuda(), z(3, 8, dtype=torch.int32).cuda(), z(3, dtype=torch.int32).cuda(), z(3, 5).cuda(), 2)
