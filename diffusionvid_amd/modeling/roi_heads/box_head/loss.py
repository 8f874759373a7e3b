"""DiffusionDet's training objective: the SimOTA-style matcher `HungarianMatcherDynamicK` and the set-prediction criterion
`SetCriterionDynamicK` (the reference's box_head/loss.py:257-688), with the reference's constructor signatures, `outputs` / `targets`
dicts and loss dict.

Two paths compute the same values:
  * CUDA tensors: `ops.set_criterion` (csrc/criterion.hip), ONE call for all head outputs of the batch;
  * CPU tensors: `criterion_host` below, torch fp32 one operation at a time in the reference's order -- the default host path, and what
    the CPU suite holds the arithmetic with.

Gradient.  The matcher never carries one (the reference's runs under no_grad too).  The criterion does when grad mode is on and a
`pred_logits` / `pred_boxes` tensor requires grad: its losses then are 0-dim float64 tensors with a `grad_fn` on the inputs' device, and
`backward()` reaches the head outputs -- on CUDA tensors through `ops.set_criterion_backward` (one launch for all head outputs), on CPU
tensors through torch's autograd on `losses_host`.  In every other situation (no_grad, inputs that do not require grad) what comes out is
detached, float64, on the CPU, as before.  The gradient stops at the head outputs: the HIP head has no backward.

Both return, per (head output s, image i): `assign` [M] (the ground-truth index a query is matched to, -1 for none), `matched_query`
[Gmax] (per ground-truth box the matched query of least cost, the matcher's second return value), `sums` [4] float64 (focal sum over the
M x C elements, L1 sum and 1 - GIoU sum over the matched queries, the matched count) and `status`.  Every term is computed in fp32 and
summed in float64.  The loss dict is formed from the sums on the host (`losses_from_sums`).

The matcher as the reference executes it (loss.py:533-688), which both paths restate:
  cost      ((cost_bbox * L1 + cost_class * class) + cost_giou * (-GIoU)) + 100 * (not in box and centre), then + 10000 on the queries
            whose centre lies in no box and no 2.5-radius centre region; fp32, in this order (the constants quantise the small terms).
            L1 over the four coordinates of the boxes normalised by the image's (w, h, w, h), added first to last; the focal class cost
            with its 1e-8; the box test on the ground truth converted to (cx, cy, w, h) and back, as the reference does
  dynamic k max(1, int(sum of the OTA_K largest IoUs of the column)), summed from the largest down
  phase 1   every column takes its k cheapest queries (equal costs: the lower query); a query taken by several columns goes to the
            column of ITS least cost over all columns (equal costs: the lower column)
  repair    while a column is empty: + 100000 on the cost rows of the matched queries; every empty column takes its cheapest query; if
            any query now holds several columns, the queries that held several BEFORE the loop (that mask is never refreshed) are
            re-assigned to their least-cost column -- and only those, so another query may keep several columns: it then reports the
            lowest one.  Bounded by `repair_bound(G)` rounds; a set that reaches the bound sets STATUS_ROUNDS.
"""
import torch
from torch import nn

STATUS_ROUNDS, STATUS_DEGENERATE, STATUS_NONFINITE, STATUS_LABEL = 1, 2, 4, 8          # include/dvid_hip.h: DVID_CRITERION_ERR_*
MAX_GT, MAX_ROWS, MAX_OTA_K = 256, 4096, 64                                              # DVID_CRITERION_MAX_GT / _MAX_ROWS / _MAX_OTA_K
MAX_CLASSES = 1280                                                                       # DVID_MAX_CLASSES
LOSS_KEYS = ("loss_ce", "loss_bbox", "loss_giou")


def repair_bound(num_gt):
    """Rounds of the repair loop after which a set is reported instead of continued: num_gt + 32 (DESIGN.md section 5 derives it)."""
    return int(num_gt) + 32


def check_limits(M, C, ota_k, counts, num_proposals=None):
    """The refusals that need no look at the values, with the key and the numbers in the message."""
    if not 1 <= ota_k <= MAX_OTA_K:
        raise NotImplementedError("MODEL.DiffusionDet.OTA_K %d: the limit is 1 <= OTA_K <= %d (DVID_CRITERION_MAX_OTA_K)" % (ota_k, MAX_OTA_K))
    if not ota_k <= M <= MAX_ROWS:
        raise NotImplementedError("set criterion: %d queries per image, the limit is OTA_K = %d <= queries <= %d (DVID_CRITERION_MAX_ROWS)"
                                  % (M, ota_k, MAX_ROWS))
    if not 1 <= C <= MAX_CLASSES:
        raise NotImplementedError("set criterion: %d classes, the limit is 1 <= classes <= %d (DVID_MAX_CLASSES)" % (C, MAX_CLASSES))
    for i, g in enumerate(counts):
        if g > MAX_GT:
            raise NotImplementedError("set criterion: image %d holds %d ground-truth boxes, the limit is %d (DVID_CRITERION_MAX_GT)" % (i, g, MAX_GT))


def raise_on_status(status, what="set criterion"):
    """status [S, n] (any device) -> raises with the head output and the image of the first set that reported something"""
    st = status.detach().cpu()
    bad = torch.nonzero(st)
    if bad.numel() == 0:
        return
    s, i = (int(v) for v in bad[0])
    code = int(st[s, i])
    if code & STATUS_LABEL:
        why = "a ground-truth label lies outside 1 .. num_classes"
    elif code & STATUS_NONFINITE:
        why = "the logits or a cost are not finite"
    elif code & STATUS_DEGENERATE:
        why = "a box has x2 < x1 or y2 < y1 (the reference asserts boxes[:, 2:] >= boxes[:, :2])"
    else:
        why = "the matcher's repair loop reached its bound of num_gt + 32 rounds: some ground-truth box can get no query"
    raise ValueError("%s: image %d of head output %d ended with status 0x%x: %s" % (what, i, s, code, why))


# ---- the arithmetic, fp32 one operation at a time ------------------------------------------------------------------------------------
def _iou_pairs(a, b):
    """a [M, 4], b [G, 4] xyxy -> (iou [M, G], union [M, G]) as torchvision's box_iou computes them"""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    h = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = w * h
    union = (area_a[:, None] + area_b[None, :]) - inter
    return inter / union, union


def _giou_pairs(a, b):
    iou, union = _iou_pairs(a, b)
    w = (torch.maximum(a[:, None, 2], b[None, :, 2]) - torch.minimum(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    h = (torch.maximum(a[:, None, 3], b[None, :, 3]) - torch.minimum(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    area = w * h
    return iou - (area - union) / area, iou


def _pow(x, gamma):
    return x * x if gamma == 2.0 else x ** gamma


def focal_terms(logits, onehot, alpha, gamma):
    """sigmoid focal loss per element from its definition (Lin et al. 2017; fvcore's sigmoid_focal_loss): BCE-with-logits times
    (1 - p_t)^gamma times alpha_t (alpha < 0: no alpha weight)"""
    p = torch.sigmoid(logits)
    ce = logits.clamp(min=0) - logits * onehot + torch.log1p(torch.exp(-logits.abs()))
    p_t = p * onehot + (1 - p) * (1 - onehot)
    loss = ce * _pow(1 - p_t, gamma)
    if alpha >= 0:
        loss = (alpha * onehot + (1 - alpha) * (1 - onehot)) * loss
    return loss


def match_image(logits, boxes, gt, labels0, whwh, alpha, gamma, ota_k, cost_class, cost_bbox, cost_giou, info=None):
    """One image of one head output.  logits [M, C], boxes [M, 4] absolute xyxy, gt [G, 4] absolute xyxy with G >= 1, labels0 [G] int64
    0-based, whwh [4]; all fp32 (or all float64: the fixtures' second run).  -> (assign [M] int64, matched_query [G] int64, rounds_hit)
    info: a dict that receives what the fixtures' cases are asserted on (dynamic k, conflict rows, repair rounds)."""
    M, G = boxes.shape[0], gt.shape[0]
    one = logits.new_tensor(1.0)
    prob = torch.sigmoid(logits)[:, labels0]                                            # [M, G]
    # centres of the queries; the ground truth to (cx, cy, w, h) and back (get_in_boxes_info is handed cxcywh)
    cx, cy = ((boxes[:, 0] + boxes[:, 2]) / 2)[:, None], ((boxes[:, 1] + boxes[:, 3]) / 2)[:, None]
    gcx, gcy, gw, gh = (gt[:, 0] + gt[:, 2]) / 2, (gt[:, 1] + gt[:, 3]) / 2, gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    x1, y1, x2, y2 = gcx - 0.5 * gw, gcy - 0.5 * gh, gcx + 0.5 * gw, gcy + 0.5 * gh
    in_box = (cx > x1[None]) & (cx < x2[None]) & (cy > y1[None]) & (cy < y2[None])
    rx, ry = 2.5 * (x2 - x1), 2.5 * (y2 - y1)
    in_ctr = (cx > (gcx - rx)[None]) & (cx < (gcx + rx)[None]) & (cy > (gcy - ry)[None]) & (cy < (gcy + ry)[None])
    fg = in_box.any(1) | in_ctr.any(1)
    both = in_box & in_ctr
    giou, iou = _giou_pairs(boxes, gt)
    neg = ((1 - alpha) * _pow(prob, gamma)) * (-torch.log((1 - prob) + 1e-8))
    pos = (alpha * _pow(1 - prob, gamma)) * (-torch.log(prob + 1e-8))
    cls = pos - neg
    d = (boxes / whwh)[:, None, :] - (gt / whwh)[None, :, :]
    d = d.abs()
    l1 = ((d[..., 0] + d[..., 1]) + d[..., 2]) + d[..., 3]
    cost = ((cost_bbox * l1 + cost_class * cls) + cost_giou * (-giou)) + 100.0 * (~both).to(logits.dtype)
    cost = torch.where(fg[:, None], cost, cost + 10000.0)
    bad = not bool(torch.isfinite(cost).all() and torch.isfinite(iou).all())
    if bad:
        return None, None, STATUS_NONFINITE
    # dynamic k: the ota_k largest IoUs of a column, added from the largest down
    top = torch.sort(iou, dim=0, descending=True, stable=True)[0][:ota_k]
    ksum = top[0].clone()
    for j in range(1, ota_k):
        ksum = ksum + top[j]
    dyn_k = ksum.to(torch.int32).clamp(min=1)
    order = torch.sort(cost, dim=0, stable=True)[1]                                     # equal costs: the lower query first
    match = torch.zeros((M, G), dtype=torch.bool)
    for g in range(G):
        match[order[:int(dyn_k[g]), g], g] = True
    held = match.sum(1) > 1                                                              # never refreshed
    if info is not None:
        info.update(dynamic_k=dyn_k.clone(), conflict_rows=int(held.sum()), rounds=0)

    def reassign():
        rows = torch.nonzero(held)[:, 0]
        if rows.numel():
            match[rows] = False
            match[rows, torch.min(cost[rows], dim=1)[1]] = True

    reassign()
    rounds, status = 0, 0
    while bool((match.sum(0) == 0).any()):
        if rounds == repair_bound(G):
            status = STATUS_ROUNDS
            break
        rounds += 1
        taken = match.sum(1) > 0
        cost[taken] = cost[taken] + 100000.0
        empty = torch.nonzero(match.sum(0) == 0)[:, 0]
        match[torch.min(cost[:, empty], dim=0)[1], empty] = True
        if bool((match.sum(1) > 1).any()):
            reassign()
    if info is not None:
        info["rounds"] = rounds
    sel = match.any(1)
    first = torch.where(match, torch.arange(G)[None, :], torch.full((1, 1), G)).min(1)[0]          # a query that kept several: the lowest
    assign = torch.where(sel, first, torch.full((M,), -1, dtype=torch.int64))
    masked = torch.where(match, cost, torch.full_like(cost, float("inf")))
    return assign, torch.min(masked, dim=0)[1], status


def criterion_host(logits, boxes, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma, ota_k, cost_class, cost_bbox, cost_giou, info=None):
    """The host path.  logits [S, n, M, C], boxes [S, n, M, 4] absolute xyxy, gt_boxes [G, 4] absolute xyxy, gt_labels [G] 1-based,
    gt_starts [n + 1], sizes [n, 2] (w, h); fp32 (float64 inputs are computed in float64).  -> (assign [S, n, M] int32, matched_query
    [S, n, Gmax] int32, sums [S, n, 4] float64, status [S, n] int32), what ops.set_criterion returns."""
    S, n, M, C = logits.shape
    dt = logits.dtype
    starts = [int(v) for v in gt_starts]
    counts = [starts[i + 1] - starts[i] for i in range(n)]
    check_limits(M, C, ota_k, counts)
    gmax = max(counts + [1])
    assign = torch.full((S, n, M), -1, dtype=torch.int32)
    mq = torch.full((S, n, gmax), -1, dtype=torch.int32)
    sums = torch.zeros((S, n, 4), dtype=torch.float64)
    status = torch.zeros((S, n), dtype=torch.int32)
    gt_boxes, gt_labels = gt_boxes.reshape(-1, 4).to(dt), gt_labels.reshape(-1).to(torch.int64)
    for i in range(n):
        gt, lab = gt_boxes[starts[i]:starts[i + 1]], gt_labels[starts[i]:starts[i + 1]] - 1
        whwh = torch.stack((sizes[i, 0], sizes[i, 1], sizes[i, 0], sizes[i, 1])).to(dt)
        gt_bad = bool(((gt[:, 2] < gt[:, 0]) | (gt[:, 3] < gt[:, 1])).any())
        lab_bad = bool(((lab < 0) | (lab >= C)).any())
        # the L1 target: normalised, to (cx, cy, w, h) and back, as prepare_targets and loss_boxes do
        gn = gt / whwh
        ncx, ncy, nw, nh = (gn[:, 0] + gn[:, 2]) / 2, (gn[:, 1] + gn[:, 3]) / 2, gn[:, 2] - gn[:, 0], gn[:, 3] - gn[:, 1]
        target = torch.stack((ncx - 0.5 * nw, ncy - 0.5 * nh, ncx + 0.5 * nw, ncy + 0.5 * nh), dim=1)
        for s in range(S):
            lg, bx = logits[s, i], boxes[s, i]
            st = 0
            if not bool(torch.isfinite(lg).all()):
                st |= STATUS_NONFINITE
            if gt_bad or bool(((bx[:, 2] < bx[:, 0]) | (bx[:, 3] < bx[:, 1])).any()):
                st |= STATUS_DEGENERATE
            if lab_bad:
                st |= STATUS_LABEL
            a = None
            if counts[i] and not st:
                sub = {} if info is not None else None
                a, q, st = match_image(lg, bx, gt, lab, whwh, alpha, gamma, ota_k, cost_class, cost_bbox, cost_giou, sub)
                if info is not None:
                    info[(s, i)] = sub
            status[s, i] = st
            if st & ~STATUS_ROUNDS:
                continue
            onehot = torch.zeros_like(lg)
            if a is not None:
                assign[s, i], mq[s, i, :counts[i]] = a.to(torch.int32), q.to(torch.int32)
                rows = torch.nonzero(a >= 0)[:, 0]
                onehot[rows, lab[a[rows]]] = 1
                d = (bx[rows] / whwh - target[a[rows]]).abs()
                l1 = ((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]
                giou = torch.diagonal(_giou_pairs(bx[rows], gt[a[rows]])[0]) if rows.numel() else l1
                sums[s, i, 1], sums[s, i, 2], sums[s, i, 3] = l1.double().sum(), (1 - giou).double().sum(), float(rows.numel())
            sums[s, i, 0] = focal_terms(lg, onehot, alpha, gamma).double().sum()
    return assign, mq, sums, status


def losses_from_sums(sums):
    """sums [S, n, 4] float64 -> the reference's dict, unweighted, as Python floats: head output S - 1 is the final one (`loss_ce`, ...),
    head output j < S - 1 the auxiliary one `_j`.  loss_ce = focal sum / max(matched, 1); loss_bbox and loss_giou divide by the
    matched count and are 0 when nothing matched (loss_labels / loss_boxes as written)."""
    tot = sums.detach().to("cpu", torch.float64).sum(1)                                 # over the batch
    S = tot.shape[0]
    out = {}
    for s in [S - 1] + list(range(S - 1)):
        sfx = "" if s == S - 1 else "_%d" % s
        focal, l1, giou, cnt = (float(v) for v in tot[s])
        out["loss_ce" + sfx] = focal / max(cnt, 1.0)
        out["loss_bbox" + sfx] = l1 / cnt if cnt else 0.0
        out["loss_giou" + sfx] = giou / cnt if cnt else 0.0
    return out


def _giou_rows(a, b):
    """a, b [K, 4] xyxy -> GIoU of row k of a with row k of b: _giou_pairs' arithmetic on the pairs alone"""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.minimum(a[:, 2], b[:, 2]) - torch.maximum(a[:, 0], b[:, 0])).clamp(min=0)
    h = (torch.minimum(a[:, 3], b[:, 3]) - torch.maximum(a[:, 1], b[:, 1])).clamp(min=0)
    inter = w * h
    union = (area_a + area_b) - inter
    cw = (torch.maximum(a[:, 2], b[:, 2]) - torch.minimum(a[:, 0], b[:, 0])).clamp(min=0)
    ch = (torch.maximum(a[:, 3], b[:, 3]) - torch.minimum(a[:, 1], b[:, 1])).clamp(min=0)
    area = cw * ch
    return inter / union - (area - union) / area


def losses_host(logits, boxes, packed, assign, alpha=0.25, gamma=2.0):
    """The differentiable host path: the three losses of every head output as torch operations on the tensors handed over, no loop over
    elements, images or head outputs.  logits [S, n, M, C], boxes [S, n, M, 4] absolute xyxy, fp32 or float64 (the ground truth is taken
    to their dtype); packed: pack_targets' tuple (gt_boxes [G, 4], gt_labels [G] 1-based, gt_starts [n + 1], sizes [n, 2]); assign
    [S, n, M]: the matching (criterion_host's or ops.set_criterion's), not differentiated.  -> [S, 3] float64: loss_ce, loss_bbox,
    loss_giou of head output s with the reference's denominators -- loss_ce = focal sum / max(matched, 1), the box terms / matched, and 0
    with zero gradient when nothing matched.  The terms are criterion_host's arithmetic in the inputs' dtype, added in float64.

    This is what torch's autograd differentiates on the CPU, and what states the device kernel's conventions at the kinks: torch.maximum
    / torch.minimum of equal operands hand each half of the gradient, clamp(min=0) passes it at exactly 0, sign(0) = 0 in the L1 term."""
    S, n, M, C = logits.shape
    dt, dev = logits.dtype, logits.device
    gt_boxes, gt_labels, gt_starts, sizes = packed
    gt_boxes = gt_boxes.detach().reshape(-1, 4).to(dev, dt)
    lab0 = gt_labels.detach().reshape(-1).to(dev, torch.int64) - 1
    starts = torch.as_tensor(gt_starts).detach().to(dev, torch.int64)
    sizes = torch.as_tensor(sizes).detach().to(dev, dt)
    whwh = torch.cat((sizes, sizes), dim=1)                                             # [n, 4]
    s_idx, i_idx, m_idx = torch.nonzero(assign.to(dev) >= 0, as_tuple=True)              # the matched queries, K of them
    g_idx = starts[i_idx] + assign.to(dev)[s_idx, i_idx, m_idx].to(torch.int64)
    onehot = torch.zeros((S, n, M, C), dtype=dt, device=dev)
    onehot[s_idx, i_idx, m_idx, lab0[g_idx]] = 1
    focal = focal_terms(logits, onehot, alpha, gamma).double().sum((1, 2, 3))
    # the L1 target: normalised, to (cx, cy, w, h) and back, as prepare_targets and loss_boxes do
    gt, w4 = gt_boxes[g_idx], whwh[i_idx]
    gn = gt / w4
    ncx, ncy, nw, nh = (gn[:, 0] + gn[:, 2]) / 2, (gn[:, 1] + gn[:, 3]) / 2, gn[:, 2] - gn[:, 0], gn[:, 3] - gn[:, 1]
    target = torch.stack((ncx - 0.5 * nw, ncy - 0.5 * nh, ncx + 0.5 * nw, ncy + 0.5 * nh), dim=1)
    q = boxes[s_idx, i_idx, m_idx]
    d = (q / w4 - target).abs()
    l1 = ((d[:, 0] + d[:, 1]) + d[:, 2]) + d[:, 3]
    zero = torch.zeros((S,), dtype=torch.float64, device=dev)
    l1 = zero.index_add(0, s_idx, l1.double())
    giou = zero.index_add(0, s_idx, (1 - _giou_rows(q, gt)).double())
    cnt = zero.index_add(0, s_idx, torch.ones_like(s_idx, dtype=torch.float64)).clamp(min=1)          # nothing matched: the box sums are 0
    return torch.stack((focal / cnt, l1 / cnt, giou / cnt), dim=1)


def _denominators(cnt):
    """matched counts [S] float64 -> ([S, 3] what the three sums are divided by, [S, 3] 1 where the loss exists, 0 where it is defined as 0)"""
    one = torch.ones_like(cnt)
    return torch.stack((cnt.clamp(min=1),) * 3, dim=1), torch.stack((one, (cnt > 0).to(cnt.dtype), (cnt > 0).to(cnt.dtype)), dim=1)


def coef_from_counts(upstream, cnt):
    """upstream [S, 3] (d objective / d loss_ce, loss_bbox, loss_giou of each head output) and the matched counts [S] of the batch -> the
    coef [S, 3] float64 ops.set_criterion_backward takes: upstream / max(matched, 1), and 0 for the box terms when nothing matched.
    Device tensors stay on the device: nothing here synchronises."""
    den, live = _denominators(cnt.to(torch.float64))
    return (upstream.to(torch.float64) / den * live).contiguous()


class _DeviceCriterion(torch.autograd.Function):
    """ops.set_criterion forward, ops.set_criterion_backward backward: [S, n, M, C] logits and [S, n, M, 4] boxes -> losses [S, 3] float64
    on the device (loss_ce, loss_bbox, loss_giou per head output, the reference's denominators)."""

    @staticmethod
    def forward(ctx, logits, boxes, packed, params, what):
        from .... import ops
        gt_boxes, gt_labels, gt_starts, sizes = packed
        dev = logits.device
        if not isinstance(sizes, ops.FrameSizes):
            sizes = sizes.to(dev, torch.float32)
        lg, bx = logits.detach().float().contiguous(), boxes.detach().float().contiguous()
        gt_boxes, gt_labels = gt_boxes.to(dev, torch.float32), gt_labels.to(dev, torch.int32)
        assign, _, sums, status = ops.set_criterion(lg, bx, gt_boxes, gt_labels, gt_starts, sizes, params["alpha"], params["gamma"], params["ota_k"],
                                                    params["cost_class"], params["cost_bbox"], params["cost_giou"])
        raise_on_status(status, what)
        tot = sums.sum(1)                                                                # over the batch, on the device
        den, live = _denominators(tot[:, 3])
        ctx.save_for_backward(lg, bx, gt_boxes, gt_labels, assign, status, tot[:, 3])
        ctx.rest = (gt_starts, sizes, params["alpha"], params["gamma"], logits.dtype, boxes.dtype)
        return tot[:, :3] / den * live

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        from .... import ops
        lg, bx, gt_boxes, gt_labels, assign, status, cnt = ctx.saved_tensors
        gt_starts, sizes, alpha, gamma, dt_logits, dt_boxes = ctx.rest
        d_logits, d_boxes = ops.set_criterion_backward(lg, bx, gt_boxes, gt_labels, gt_starts, sizes, alpha, gamma, assign, status,
                                                       coef_from_counts(grad, cnt))
        return d_logits.to(dt_logits), d_boxes.to(dt_boxes), None, None, None


def q_sample_boxes_host(gt_cxcywh, gt_starts, t, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, noise, placeholder, snr_scale, sizes):
    """The host form of ops.q_sample_boxes (the reference's prepare_diffusion_concat + q_sample, diffusion_det.py:681-725, and the scaling
    by the image's (w, h, w, h)), torch fp32 one operation at a time: same arguments on the CPU, -> absolute xyxy boxes [n, M, 4]."""
    n, M = noise.shape[:2]
    starts = [int(v) for v in gt_starts]
    out = torch.empty((n, M, 4), dtype=torch.float32)
    for i in range(n):
        G = starts[i + 1] - starts[i]
        if G > M:
            raise NotImplementedError("q_sample_boxes: image %d holds %d ground-truth boxes, NUM_PROPOSALS is %d (the reference's random subset is "
                                      "not built)" % (i, G, M))
        ti = int(t[i])
        if not 0 <= ti < sqrt_alphas_cumprod.shape[0]:
            raise ValueError("q_sample_boxes: t[%d] is %d, outside 0 .. %d" % (i, ti, sqrt_alphas_cumprod.shape[0] - 1))
        gt = gt_cxcywh[starts[i]:starts[i + 1]].float() if G else torch.tensor([[0.5, 0.5, 1.0, 1.0]])
        pad = placeholder[i, :M - gt.shape[0]].float() / 6.0 + 0.5
        pad[:, 2:] = pad[:, 2:].clamp(min=1e-4)
        x = (torch.cat((gt, pad)) * 2.0 - 1.0) * snr_scale
        x = sqrt_alphas_cumprod[ti] * x + sqrt_one_minus_alphas_cumprod[ti] * noise[i].float()
        x = ((x.clamp(min=-1 * snr_scale, max=snr_scale) / snr_scale) + 1) / 2.0
        w, h = float(sizes[i][0]), float(sizes[i][1])
        xyxy = torch.stack((x[:, 0] - 0.5 * x[:, 2], x[:, 1] - 0.5 * x[:, 3], x[:, 0] + 0.5 * x[:, 2], x[:, 1] + 0.5 * x[:, 3]), dim=1)
        out[i] = xyxy * torch.tensor([w, h, w, h])
    return out


def pack_targets(targets):
    """the reference's list of target dicts (`labels` 1-based, `boxes_xyxy` absolute, `image_size_xyxy`) -> (gt_boxes [G, 4], gt_labels
    [G] int32, gt_starts [n + 1] int32, sizes [n, 2]) on the CPU"""
    starts, boxes, labels, sizes = [0], [], [], []
    for t in targets:
        b = t["boxes_xyxy"].detach().reshape(-1, 4).to("cpu")
        boxes.append(b), labels.append(t["labels"].detach().reshape(-1).to("cpu", torch.int32))
        sizes.append(t["image_size_xyxy"].detach().to("cpu")[:2])
        starts.append(starts[-1] + b.shape[0])
    dt = boxes[0].dtype if boxes else torch.float32
    return (torch.cat(boxes) if boxes else torch.zeros((0, 4), dtype=dt), torch.cat(labels) if labels else torch.zeros((0,), dtype=torch.int32),
            torch.tensor(starts, dtype=torch.int32), torch.stack(sizes).to(dt) if sizes else torch.zeros((0, 2), dtype=dt))


def _run(logits, boxes, packed, p):
    """[S, n, M, C] / [S, n, M, 4] through the device op (CUDA tensors) or the host path (CPU tensors)"""
    gt_boxes, gt_labels, gt_starts, sizes = packed
    args = (p["alpha"], p["gamma"], p["ota_k"], p["cost_class"], p["cost_bbox"], p["cost_giou"])
    if logits.is_cuda:
        from .... import ops
        dev = logits.device
        if not isinstance(sizes, ops.FrameSizes):
            sizes = sizes.to(dev, torch.float32)
        return ops.set_criterion(logits.detach().float(), boxes.detach().float(), gt_boxes.to(dev, torch.float32), gt_labels.to(dev), gt_starts,
                                 sizes, *args)
    return criterion_host(logits.detach(), boxes.detach(), gt_boxes, gt_labels, gt_starts, sizes, *args)


class HungarianMatcherDynamicK(nn.Module):
    """The dynamic-k matcher with the reference's constructor (loss.py:514).  forward(outputs, targets) -> (indices, matched_ids): per
    image (boolean query mask [M], ground-truth index of every selected query in query order) and the matched query of every ground-truth
    box -- int64, on the device of the outputs."""

    def __init__(self, cfg, cost_class=1, cost_bbox=1, cost_giou=1, cost_mask=1, use_focal=False):
        super().__init__()
        d = cfg.MODEL.DiffusionDet
        if d.USE_FED_LOSS:
            raise NotImplementedError("MODEL.DiffusionDet.USE_FED_LOSS True is not built: the federated loss needs the data set's class frequencies "
                                      "and a multinomial draw")
        if not use_focal:
            raise NotImplementedError("only the focal-loss (sigmoid) branch is built (USE_FOCAL: True)")
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.cost_class, self.cost_bbox, self.cost_giou, self.use_focal = float(cost_class), float(cost_bbox), float(cost_giou), use_focal
        self.use_fed_loss = False
        self.ota_k = int(d.OTA_K)
        self.focal_loss_alpha, self.focal_loss_gamma = float(d.ALPHA), float(d.GAMMA)

    def params(self):
        return dict(alpha=self.focal_loss_alpha, gamma=self.focal_loss_gamma, ota_k=self.ota_k, cost_class=self.cost_class,
                    cost_bbox=self.cost_bbox, cost_giou=self.cost_giou)

    @torch.no_grad()
    def forward(self, outputs, targets):
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        assert logits.shape[0] == len(targets)
        packed = pack_targets(targets)
        assign, mq, _, status = _run(logits[None], boxes[None], packed, self.params())
        raise_on_status(status, "HungarianMatcherDynamicK")
        starts = packed[2].tolist()
        indices, matched = [], []
        for i in range(len(targets)):
            a = assign[0, i].to(torch.int64)
            indices.append((a >= 0, a[a >= 0]))
            matched.append(mq[0, i, :starts[i + 1] - starts[i]].to(torch.int64))
        return indices, matched


class SetCriterionDynamicK(nn.Module):
    """The set-prediction loss with the reference's constructor (loss.py:263).  forward(outputs, targets) -> {loss_ce, loss_bbox, loss_giou,
    and `_0 .. _{S-2}` for outputs["aux_outputs"]}, unweighted 0-dim float64 tensors: detached and on the CPU, unless grad mode is on and a
    `pred_logits` / `pred_boxes` requires grad -- then on the inputs' device with a grad_fn (the module docstring says through what)."""

    def __init__(self, cfg, num_classes, matcher, weight_dict, eos_coef, losses, use_focal):
        super().__init__()
        if cfg.MODEL.DiffusionDet.USE_FED_LOSS:
            raise NotImplementedError("MODEL.DiffusionDet.USE_FED_LOSS True is not built: the federated loss needs the data set's class frequencies "
                                      "and a multinomial draw")
        if not use_focal:
            raise NotImplementedError("only the focal-loss (sigmoid) branch is built (USE_FOCAL: True)")
        if sorted(losses) != ["boxes", "labels"]:
            raise NotImplementedError("SetCriterionDynamicK computes losses ['labels', 'boxes'], got %s" % (list(losses),))
        self.cfg, self.num_classes, self.matcher, self.weight_dict, self.eos_coef = cfg, num_classes, matcher, weight_dict, eos_coef
        self.losses, self.use_focal, self.use_fed_loss = list(losses), use_focal, False
        self.focal_loss_alpha, self.focal_loss_gamma = float(cfg.MODEL.DiffusionDet.ALPHA), float(cfg.MODEL.DiffusionDet.GAMMA)

    @torch.no_grad()
    def sums(self, logits, boxes, packed):
        """[S, n, M, C], [S, n, M, 4] and pack_targets' tuple -> (assign, matched_query, sums, status), statuses raised"""
        if logits.shape[-1] != self.num_classes:
            raise ValueError("SetCriterionDynamicK: the logits hold %d classes, num_classes is %d" % (logits.shape[-1], self.num_classes))
        out = _run(logits, boxes, packed, self.matcher.params())
        raise_on_status(out[3], "SetCriterionDynamicK")
        return out

    def losses_with_grad(self, logits, boxes, packed):
        """The differentiable path.  [S, n, M, C], [S, n, M, 4] and pack_targets' tuple -> losses [S, 3] float64 on the inputs' device
        (loss_ce, loss_bbox, loss_giou per head output) with a grad_fn: the device pair ops.set_criterion / ops.set_criterion_backward on
        CUDA tensors, the matcher under no_grad and then losses_host on CPU tensors.  Statuses are raised as `sums` raises them."""
        if logits.shape[-1] != self.num_classes:
            raise ValueError("SetCriterionDynamicK: the logits hold %d classes, num_classes is %d" % (logits.shape[-1], self.num_classes))
        p = self.matcher.params()
        if logits.is_cuda:
            return _DeviceCriterion.apply(logits, boxes, packed, p, "SetCriterionDynamicK")
        assign = self.sums(logits, boxes, packed)[0]
        return losses_host(logits, boxes, packed, assign, p["alpha"], p["gamma"])

    def forward(self, outputs, targets):
        heads = list(outputs.get("aux_outputs", [])) + [outputs]                        # the final output last
        wanted = torch.is_grad_enabled() and any(h[k].requires_grad for h in heads for k in ("pred_logits", "pred_boxes"))
        with torch.set_grad_enabled(wanted):
            logits = torch.stack([h["pred_logits"] for h in heads])
            boxes = torch.stack([h["pred_boxes"] for h in heads])
        packed = pack_targets(targets)
        if not wanted:
            sums = self.sums(logits, boxes, packed)[2]
            return {k: torch.tensor(v, dtype=torch.float64) for k, v in losses_from_sums(sums).items()}
        losses = self.losses_with_grad(logits, boxes, packed)
        S = losses.shape[0]
        return {key + ("" if s == S - 1 else "_%d" % s): losses[s, k] for s in [S - 1] + list(range(S - 1)) for k, key in enumerate(LOSS_KEYS)}
