"""End-to-end parity: GPU DiffusionDet (libdvid_hip) vs the CPU oracle state machine on the same
synthetic video, same weights, same injected noise.

The pipeline is discontinuous (top-k, score>0.5 renewal, NMS, FPS arg-max) and the GPU path holds
weights/activations in fp16, so the comparison is staged:
  1. extraction pass (backbone + 3 heads on every local/global frame): logits / boxes / object features
     within fp16-pipeline tolerance;
  2. global memory: FPS run by the GPU kernel on the ORACLE's features must return the oracle's rows
     exactly (integer work), and the GPU's own memory must be the same point set up to near-ties;
  3. final stage with the oracle's memory injected: logits / boxes within tolerance, detections matched
     one-to-one by (label, IoU, score).
Stated tolerances: object features |err| <= 0.08 (LayerNorm-ed, O(1)); logits |err| <= 0.08; boxes
<= max(0.5 px, 1% of box size); scores |err| <= 5e-3 -- for at least 99% of the boxes (a box that sits
on a pyramid-level or sample-validity threshold may flip discretely between fp16 and fp32 features); the fraction outside is
printed with every stage line.  (Rounds 1-3 ran the box bound at max(0.75 px, 2 %); round 4 tightened it to the contract's.)

Conditioning.  With white-noise frames and raw random-init heads the 3-stage refinement is chaotic:
rounding the CPU oracle's OWN feature maps to fp16 moves its stage-3 features by O(1) (measured,
see diffusionvid_amd/utils/synthetic.py).  The end-to-end test therefore uses low-frequency frames
and box-delta layers scaled by 0.1, for which the same experiment stays at ~3e-3.
"""
import os
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detector as odet  # noqa: E402
from oracle import memory as omem  # noqa: E402


def _report_path():
    """reports/parity_report.txt under the repository root, the report every parity line is appended to; the directory is
    kept out of git, so it is created on first use"""
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reports")
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, "parity_report.txt")


def _weights(model, weights="init", **trained_like):
    """"init": random-init heads with box-delta layers x0.1 (class scores 0.010 +- 0.003); "trained_like": additionally class layers
    with a trained detector's score spread (synthetic.trained_like_scores); "untamed": the raw random-init state dict"""
    from diffusionvid_amd.utils import synthetic
    sd = model.state_dict()
    if weights != "untamed":
        sd = synthetic.tame_box_deltas(sd, 0.1)
    if weights == "trained_like":
        sd = synthetic.trained_like_scores(sd, **trained_like)
    model.load_state_dict(sd)
    return model


def _build(sample_step, blocks, weights="init", extra=(), dtype="float16"):
    """dtype: the reference's DTYPE key -- "float16" = the fp16 path every test here ran until round 5, "float32" (the reference's
    default, mega_core/config/defaults.py:582) = fp32 storage / fp32 MFMA (csrc/f32.hip)"""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", dtype, "MODEL.DiffusionDet.SAMPLE_STEP", sample_step] + list(extra),
                  "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = blocks
    cfg.freeze()
    model = _weights(build_detection_model(cfg), weights)
    return cfg, model.to("cuda").eval()


def _feature_check(tag, model, oracle, bound_max=0.06, bound_rms=0.012):
    """Direct check of the backbone output at whatever depth / size the test runs: p3 / p4 / p5 of every frame of the call,
    GPU (fp16 NHWC, `debug_taps["extract"][i][3]`) against the oracle (fp32 NCHW, `taps["feats"]`).  Per level: largest
    absolute error and RMS error, both relative to the level's RMS value -- a scale or offset drift through the 101 layers
    shows up here, where the three LayerNorm-ed heads behind would hide it."""
    lines = []
    for lvl, name in enumerate(("p3", "p4", "p5")):
        g = torch.cat([e[3][lvl].float().cpu() for e in model.debug_taps["extract"]]).permute(0, 3, 1, 2)
        o = oracle.taps["feats"][name]
        assert g.shape == o.shape, (g.shape, o.shape)
        rms = o.pow(2).mean().sqrt().item()
        e_max = (g - o).abs().max().item() / rms
        e_rms = (g - o).pow(2).mean().sqrt().item() / rms
        gain = (g * o).sum().item() / o.pow(2).sum().item()          # least-squares scale of the GPU features on the oracle's
        lines.append(f"{name}: max |err| / rms = {e_max:.3e}, rms err / rms = {e_rms:.3e}, scale = {gain:.5f}, mean offset / rms = {(g - o).mean().item() / rms:+.2e}")
        assert e_max <= bound_max and e_rms <= bound_rms and abs(gain - 1) <= 2e-3, f"{tag} {lines[-1]}"
    line = f"{tag} backbone features vs oracle ({tuple(o.shape[:1])[0]} frames, rms {rms:.2f}): " + "; ".join(lines)
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")


def _oracle_items(ds, idx):
    images, _, ids = ds[idx]
    o = {k: v for k, v in images.items() if k not in ("cur", "ref_l", "ref_g")}
    o["cur"] = images["cur"].tensors.cpu()
    o["image_size"] = tuple(images["cur"].image_sizes[0])
    o["ref_l"] = [im.tensors.cpu() for im in images["ref_l"]]
    o["ref_g"] = [im.tensors.cpu() for im in images["ref_g"]]
    return images, o, ids


def _iou(a, b):
    x1, y1 = np.maximum(a[0], b[0]), np.maximum(a[1], b[1])
    x2, y2 = np.minimum(a[2], b[2]), np.minimum(a[3], b[3])
    inter = max(0.0, x2 - x1) * max(0.0, y2 - y1)
    ua = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / ua if ua > 0 else 1.0


def _stage_check(tag, gpf, opf, gcl, ocl, gbx, obx, frac_ok=0.99, b_logit=0.08, b_feat=0.08, b_px=0.5, b_rel=0.01):
    """per-box errors against the stated bounds (boxes: SURVEY.md 8(d)'s max(0.5 px, 1 % of the box size)); the fraction of
    boxes outside any bound -- slots whose RoI flipped a pyramid level or a sample-validity test between fp16 and fp32 features
    -- is REPORTED with every line and must stay below 1 - frac_ok"""
    e_cl = (gcl - ocl).abs().amax(-1).reshape(-1)
    size = (obx[..., 2:] - obx[..., :2]).clamp(min=1).max(-1).values
    e_bx = ((gbx - obx).abs().max(-1).values / torch.maximum(size * b_rel, torch.tensor(b_px))).reshape(-1)
    ok = (e_cl <= b_logit) & (e_bx <= 1.0)
    msg = f"{tag}: |dlogit| median={e_cl.median():.2e} p99={e_cl.quantile(0.99):.2e} max={e_cl.max():.2e}; "
    msg += f"box err/bound median={e_bx.median():.2e} p99={e_bx.quantile(0.99):.2e} max={e_bx.max():.2e}"
    if gpf is not None:
        e_pf = (gpf - opf).abs().amax(-1).reshape(-1)
        ok &= e_pf <= b_feat
        msg += f"; |dfeat| median={e_pf.median():.2e} p99={e_pf.quantile(0.99):.2e} max={e_pf.max():.2e}"
    frac = ok.float().mean().item()
    msg += f"; boxes outside a bound {1 - frac:.4%} ({int((~ok).sum())} of {ok.numel()}; bounds |dlogit| {b_logit}, box max({b_px} px, {b_rel:.0%}))"
    print(msg)
    with open(_report_path(), "a") as f:
        f.write(msg + "\n")
    assert frac >= frac_ok, msg
    return frac


def _match_rate(ref, got):
    """fraction of oracle detections with a GPU detection of the same label, IoU >= 0.9, |dscore| <= 5e-3"""
    hit = 0
    gb, gs, gl = got.bbox.cpu().numpy(), got.get_field("scores").cpu().numpy(), got.get_field("labels").cpu().numpy()
    used = np.zeros(len(gs), bool)
    for b, s, l in zip(ref["boxes"], ref["scores"], ref["labels"]):
        cand = np.nonzero((gl == l) & ~used & (np.abs(gs - s) <= 5e-3))[0]
        best = max(cand, key=lambda j: _iou(b, gb[j]), default=None)
        if best is not None and _iou(b, gb[best]) >= 0.9:
            used[best] = True
            hit += 1
    return hit / max(1, len(ref["scores"]))


def _ap50_vs_oracle(ref_out, got_out, size):
    """the reference's VID AP50 protocol (diffusionvid_amd/data/evaluation/vid_eval.py, pinned by
    golden g11) with the oracle's kept detections playing ground truth -- 1.0 means every oracle detection is found
    at IoU >= 0.5 with the same label before any extra GPU detection of that class."""
    from diffusionvid_amd.data.evaluation import vid_eval
    from diffusionvid_amd.structures.bounding_box import BoxList
    gts, preds = [], []
    for r, g in zip(ref_out, got_out):
        gt = BoxList(torch.as_tensor(r["boxes"], dtype=torch.float32).reshape(-1, 4), size)
        gt.add_field("labels", torch.as_tensor(r["labels"], dtype=torch.int64).reshape(-1))
        gts.append(gt)
        preds.append(g.to(torch.device("cpu")))
    return vid_eval.eval_detection_vid(preds, gts)["map"]


def _ap50_on_objects(ref_out, got_out, size, thr=0.5):
    """BASELINE's "AP50 within +-0.1 of the reference on identical inputs" read the way the reference computes AP50 -- against
    OBJECTS: ground truth = the oracle's detections with score >= thr (what a trained detector would call objects; needs the
    trained-like score regime), predictions = ALL detections of one side with their scores.  The oracle's own detections score
    exactly 1.0 on it (every object is found at IoU 1 ahead of every lower-scoring detection of its class); the GPU side loses
    AP only where an object is missed / mislabelled / moved by more than IoU 0.5, or a non-object outranks an object of its
    class.  -> (AP50 of the GPU detections, number of objects)."""
    from diffusionvid_amd.data.evaluation import vid_eval
    from diffusionvid_amd.structures.bounding_box import BoxList
    gts, preds, n_obj = [], [], 0
    for r, g in zip(ref_out, got_out):
        sc = np.asarray(r["scores"]).reshape(-1)
        keep = sc >= thr
        n_obj += int(keep.sum())
        gt = BoxList(torch.as_tensor(np.asarray(r["boxes"]).reshape(-1, 4)[keep], dtype=torch.float32).reshape(-1, 4), size)
        gt.add_field("labels", torch.as_tensor(np.asarray(r["labels"]).reshape(-1)[keep], dtype=torch.int64).reshape(-1))
        gts.append(gt)
        preds.append(g.to(torch.device("cpu")))
    if n_obj == 0:
        return float("nan"), 0
    return vid_eval.eval_detection_vid(preds, gts)["map"], n_obj


def _box_eps(b, px=0.5, rel=0.01):
    """a box coordinate may differ by max(0.5 px, 1 % of the box size)"""
    return np.maximum(px, rel * np.maximum(b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]))


def _iou_interval(a, ea, b, eb):
    """[lowest, highest] IoU of boxes a and b (no +1, as batched_nms) when every coordinate of a may move by ea and of b by eb"""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    e = ea + eb
    inter_hi = max(0.0, iw + e) * max(0.0, ih + e)
    inter_lo = max(0.0, iw - e) * max(0.0, ih - e)

    def area(x, d):
        return max(0.0, x[2] - x[0] + 2 * d) * max(0.0, x[3] - x[1] + 2 * d)
    un_lo = max(area(a, -ea) + area(b, -eb) - inter_hi, inter_hi, 1e-12)
    un_hi = max(area(a, ea) + area(b, eb) - inter_lo, 1e-12)
    return inter_lo / un_hi, min(1.0, inter_hi / un_lo)


def _threshold_aware_detections(tag, o_logits, o_boxes, g_logits, g_boxes, w, h, tol_s=5e-3, iou_thr=0.5, band_factor=2.0, max_outlier_frac=0.01):
    """SURVEY.md 8(d)'s end-to-end criterion on the final stage of one call: "boxes <= 0.5 px or 1e-2 rel, scores <= 5e-3, set-equality
    of kept detections after excluding candidates within tolerance of a threshold (NMS IoU 0.5, top-300 boundary)".
    o_* / g_*: [S, n, M, C] logits and [S, n, M, 4] boxes of the oracle and of the GPU path for the same box slots (S ensemble
    steps).  The GPU side's detections are what its own post-processing kernels (dvid_postproc_topk_nms) return for the GPU
    logits / boxes; the oracle side's decisions are re-derived here with the tolerance analysis:
      * a (step, box, class) candidate is NEAR THE TOP-K BOUNDARY if its oracle score is within tol_s of the step's 300th / 301st
        score gap; such candidates are excluded and, since either side may or may not hold them, they count as possible
        suppressors in the NMS analysis;
      * walking the remaining candidates in descending oracle score, a candidate is SUPPRESSED for sure if a surely-kept candidate
        of its class that is surely ahead of it (score gap > 2 tol_s) overlaps it by more than 0.5 under EVERY box perturbation
        within the box tolerance; it is UNDECIDED if some kept / undecided / boundary candidate of its class that can be ahead of
        it (score within 2 tol_s counts) overlaps it by more than 0.5 under SOME perturbation; otherwise it is KEPT for sure.
    Every surely-kept candidate must be among the GPU detections with |dscore| <= tol_s and box within max(0.5 px, 1 %); no
    surely-suppressed candidate and no candidate surely outside the top-k may be.  Returns (decided, undecided + boundary).

    The exclusion bands are NOT the full stated tolerances when the two sides agree better than that: first every candidate's
    score and box are required to agree within the stated tolerances (the continuous part of the criterion); the bands of the
    decision analysis are then `band_factor` x the LARGEST score / box difference actually observed between the two sides over
    all candidates (capped at the stated tolerances) -- a decision can only flip legitimately where the observed differences
    reach a threshold, so a narrower band excuses fewer candidates and makes the set-equality requirement stricter.  (With
    random-init class layers every score is 0.01 +- 0.003: under the full 5e-3 band four candidates in five would be excused.)"""
    from diffusionvid_amd import ops
    S, n, M, C = o_logits.shape
    gb, gs, gl, gc = (t.cpu().numpy() for t in ops.postproc_topk_nms(g_logits.cuda().contiguous(), g_boxes.cuda().contiguous(), w, h, iou_thr, True))
    so = torch.sigmoid(o_logits).reshape(S, n, M * C).numpy()
    sg = torch.sigmoid(g_logits).reshape(S, n, M * C).numpy()
    ob = o_boxes.numpy().astype(np.float64)
    gbx_all = g_boxes.numpy().astype(np.float64)
    n_decided = n_open = n_dets = 0
    worst_s = worst_b = 0.0

    def g_inside_of(st, f):
        return set(np.argsort(-sg[st, f], kind="stable")[:M].tolist())
    # continuous part over every candidate either side holds: scores within tol_s, boxes within max(0.5 px, 1 %).  A box slot whose
    # RoI sits on a pyramid-level or sample-validity threshold may flip discretely between the fp16 and the fp32 features (the
    # stage checks allow 1 % of the boxes for that): such OUTLIER slots are counted, bounded by the same 1 %, and their candidates
    # are excluded from the decided set -- but stay in the analysis as possible suppressors of others.
    in_topk = np.zeros_like(so, dtype=bool)
    for st in range(S):
        for f in range(n):
            in_topk[st, f, np.argsort(-so[st, f], kind="stable")[:M]] = True
            in_topk[st, f, np.argsort(-sg[st, f], kind="stable")[:M]] = True
    ds_box = np.abs(so - sg).reshape(S, n, M, C).max(-1)                       # per box slot: largest score difference over its classes
    db_box = np.abs(ob - gbx_all).max(-1) / _box_eps(ob)
    outlier = (ds_box > tol_s) | (db_box > 1.0)
    box_used = in_topk.reshape(S, n, M, C).any(-1)
    n_out = int((outlier & box_used).sum())
    used_ds, used_db = ds_box[box_used], db_box[box_used]
    dist = (f"{tag} candidate box slots ({int(box_used.sum())}): |dscore| median {np.median(used_ds):.2e} p90 {np.quantile(used_ds, 0.9):.2e} p99 {np.quantile(used_ds, 0.99):.2e} "
            f"max {used_ds.max():.2e}; box difference / max(0.5 px, 1 %) median {np.median(used_db):.2f} p99 {np.quantile(used_db, 0.99):.2f} max {used_db.max():.2f}; "
            f"beyond |dscore| {tol_s:g} or the box bound: {n_out} = {n_out / max(1, int(box_used.sum())):.2%} (allowed {max_outlier_frac:.0%})")
    print(dist)
    with open(_report_path(), "a") as fh:
        fh.write(dist + "\n")
    assert n_out <= max_outlier_frac * max(1, int(box_used.sum())), f"{tag}: {n_out} of {int(box_used.sum())} candidate box slots differ beyond the stated tolerances"
    ok_box = box_used & ~outlier
    d_s = float(ds_box[ok_box].max())
    d_b = float(db_box[ok_box].max())
    # bands from the bulk of the observed differences (99th percentile over the slots): the few slots beyond HALF a band are treated
    # like the outliers above (excluded from the decided set, kept as possible suppressors), so that every decided candidate's own
    # score / box moved by less than half a band -- two of them cannot swap order or cross a threshold inside the other's band
    band_s = min(tol_s, 2.0 * band_factor * float(np.quantile(ds_box[ok_box], 0.99)) + 1e-6)
    band_b = min(1.0, 2.0 * band_factor * float(np.quantile(db_box[ok_box], 0.99)) + 1e-3)
    outlier = outlier | (box_used & ((ds_box > 0.5 * band_s) | (db_box > 0.5 * band_b)))
    n_wide = int((outlier & box_used).sum()) - n_out
    spec_tol_s, tol_s = tol_s, band_s
    for f in range(n):
        keys, near, wild_keys = [], set(), set()
        for st in range(S):
            order = np.argsort(-so[st, f], kind="stable")
            gap = 0.5 * (so[st, f][order[M - 1]] + so[st, f][order[M]])
            inside = set(order[:M].tolist())
            close = np.nonzero(np.abs(so[st, f] - gap) <= tol_s)[0].tolist()
            wild = set(np.nonzero(np.repeat(outlier[st, f], C))[0].tolist())       # every class of an outlier box slot
            # an outlier candidate entering / leaving one side's top-k moves that side's boundary by one rank: the ranks next to
            # the boundary, as many as there are outlier candidates in either top-k, are boundary candidates too
            nw = len(wild & (inside | g_inside_of(st, f)))
            close = sorted(set(close) | set(order[max(0, M - nw):M + nw].tolist()))
            for k in set(close) | inside | (wild & g_inside_of(st, f)):
                keys.append((st, k))
                if k in close or k in wild:
                    near.add((st, k))
                if k in wild:
                    wild_keys.add((st, k))
            # the GPU path's own top-k set may differ from the oracle's only by boundary candidates
            g_inside = set(np.argsort(-sg[st, f], kind="stable")[:M].tolist())
            assert (g_inside ^ inside) <= (set(close) | wild), f"{tag} frame {f} step {st}: top-{M} sets differ beyond the score tolerance: {sorted((g_inside ^ inside) - set(close) - wild)[:8]}"
        keys.sort(key=lambda k: -so[k[0], f][k[1]])
        score = {k: float(so[k[0], f][k[1]]) for k in keys}
        box = {k: ob[k[0], f, k[1] // C] for k in keys}
        eps = {k: float(_box_eps(box[k])) * band_b for k in keys}
        label = {k: k[1] % C + 1 for k in keys}
        # a candidate of an outlier slot carries ANOTHER score and box on the GPU side (its RoI flipped a level / a validity test): there
        # it may stand anywhere in the class's order and overlap anything, so it is a possible suppressor of every candidate of its
        # class under either side's box, whatever its oracle score
        gbox = {k: gbx_all[k[0], f, k[1] // C] for k in wild_keys}
        wild_by_label = {}
        for k in wild_keys:
            wild_by_label.setdefault(label[k], []).append(k)
        status = {}
        by_label = {}
        for k in keys:                         # descending oracle score within each class
            by_label.setdefault(label[k], []).append(k)
        for same in by_label.values():
            for b in same:
                if b in near:
                    status[b] = "open"
                    continue
                sure = maybe = False
                for a in same:
                    if a is b or status.get(a, "later") == "suppressed":
                        continue
                    if score[a] - score[b] < -2 * tol_s:
                        break                  # descending score: nothing further down can be ahead of b
                    lo, hi = _iou_interval(box[a], eps[a], box[b], eps[b])
                    # "later": not yet classified (its score is within 2 tol_s of b's, below or equal)
                    if status.get(a, "later") == "kept" and score[a] - score[b] > 2 * tol_s and lo > iou_thr:
                        sure = True
                        break
                    if hi > iou_thr:
                        maybe = True
                if not sure and not maybe:
                    for a in wild_by_label.get(label[b], ()):
                        if a != b and any(_iou_interval(bx, max(eps[a], float(_box_eps(bx)) * band_b), box[b], eps[b])[1] > iou_thr for bx in (box[a], gbox[a])):
                            maybe = True
                            break
                status[b] = "suppressed" if sure else ("open" if maybe else "kept")
        # GPU detections of this frame -> candidate keys (same label, same score and clipped box to rounding)
        det_keys = set()
        k_cnt = int(gc[f])
        n_dets += k_cnt
        for j in range(k_cnt):
            lab, sc, bx = int(gl[f, j]), float(gs[f, j]), gb[f, j].astype(np.float64)
            best, best_d = None, 1e9
            for st in range(S):
                cand = np.nonzero(np.abs(sg[st, f][lab - 1::C] - sc) <= 2e-6)[0]          # boxes i with class lab-1 at that score
                for i in cand:
                    cb = np.clip(gbx_all[st, f, i], 0, [w - 1, h - 1, w - 1, h - 1])
                    d = np.abs(cb - bx).max()
                    if d < best_d:
                        best, best_d = (st, int(i) * C + lab - 1), d
            assert best is not None and best_d <= 1e-2, f"{tag} frame {f}: GPU detection {j} is not one of the GPU path's own candidates"
            det_keys.add(best)
            if best in status and status[best] == "kept":
                worst_s = max(worst_s, abs(score[best] - sc))
                ref_box = np.clip(box[best], 0, [w - 1, h - 1, w - 1, h - 1])
                worst_b = max(worst_b, float(np.abs(ref_box - bx).max() / float(_box_eps(box[best]))))
        for k, st_k in status.items():
            if st_k == "kept" and k not in det_keys:
                # say why before failing: was it in the GPU's top-k at all, and which GPU detection of its class overlaps it
                gk_box = gbx_all[k[0], f, k[1] // C]
                in_topk_gpu = k[1] in g_inside_of(k[0], f)
                over = [(int(j), float(gs[f, j]), round(_iou(gk_box, gb[f, j].astype(np.float64)), 3)) for j in range(int(gc[f]))
                        if int(gl[f, j]) == label[k] and _iou(gk_box, gb[f, j].astype(np.float64)) > 0.3]
                raise AssertionError(f"{tag} frame {f}: candidate (step {k[0]}, box {k[1] // C}, class {k[1] % C + 1}, oracle score {score[k]:.4f}, GPU score "
                                     f"{sg[k[0], f][k[1]]:.4f}) is kept by the oracle beyond every tolerance but missing on the GPU; in the GPU's top-{M}: {in_topk_gpu}; "
                                     f"GPU detections of its class overlapping its GPU box (index, score, IoU): {over}; outlier slots of this frame: "
                                     f"{sorted({(a[0], a[1] // C) for a in wild_keys})[:10]}")
            elif st_k == "suppressed":
                assert k not in det_keys, f"{tag} frame {f}: candidate (step {k[0]}, box {k[1] // C}, class {k[1] % C + 1}) is suppressed by the oracle beyond every tolerance but kept on the GPU"
        for k in det_keys - set(status):
            raise AssertionError(f"{tag} frame {f}: GPU keeps (step {k[0]}, box {k[1] // C}, class {k[1] % C + 1}), which is outside the oracle's top-{M} beyond the score tolerance")
        n_decided += sum(1 for v in status.values() if v != "open")
        n_open += sum(1 for v in status.values() if v == "open")
    line = (f"{tag} threshold-aware detection sets: candidates within the stated tolerances (max |dscore| = {d_s:.2e} <= {spec_tol_s:.0e}, max box "
            f"difference = {d_b:.2f} x max(0.5 px, 1 %); {n_out} of {int(box_used.sum())} box slots flipped discretely and are excluded, {n_wide} more moved by over half a band); decision bands "
            f"{2 * band_factor:g} x the 99th percentile of the observed differences = {band_s:.2e} on scores, {band_b:.2f} x the box tolerance: {n_decided} candidates decided beyond the bands (all agree with the {n_dets} GPU detections), "
            f"{n_open} excluded as within a band of the top-{M} / IoU {iou_thr} thresholds ({n_open / max(1, n_open + n_decided):.1%}); "
            f"kept pairs: max |dscore| = {worst_s:.2e}, max box error / bound = {worst_b:.2f}")
    print(line)
    with open(_report_path(), "a") as fh:
        fh.write(line + "\n")
    assert worst_s <= spec_tol_s and worst_b <= 1.0, line
    return n_decided, n_open


def _final_stage_vs_oracle(model, oracle, L, W0, H0, sample_step, tag, min_decided=0.1, max_outlier_frac=0.01, **bounds):
    """Final stage (global attention + conditioned head) of every DDIM step with the ORACLE's memory, and for steps > 0
    the oracle's renewed boxes, injected: logits / boxes per step within the stated bounds."""
    from diffusionvid_amd.utils import synthetic
    M, d = model.num_proposals, model.hidden_dim
    model.head.proposal_feats_global = [oracle.mem[0].cuda(), oracle.mem[1].cuda()]
    entries = [model.queue[i] for i in range(L)]
    feats_cur, cached = model._gather_entries(entries)
    ens = {"ol": [], "ob": [], "gl": [], "gb": []}
    for step, (time, time_next) in enumerate(model._time_pairs()):
        with torch.no_grad():
            t = torch.full((L,), time, dtype=torch.long)
            if sample_step == 1:
                model.head.proposals_feat_cur = [[cached[0], cached[1], cached[2].reshape(1, L * M, d)]]
                img = torch.zeros(L, M, 4, device="cuda")
            elif step == 0:
                img = oracle.noise_fn("img", 0, 0, 0, (L, M, 4)).cuda()          # the draw the oracle made (host or counter-based)
            else:
                # one flipped keep decision shifts every later slot of its frame, so each step starts from the oracle's
                # renewed boxes (the renewal itself is compared in test_gpu_kernels.py::test_ddim_renew_step)
                img = oracle.taps[f"img_{step}"].cuda()
            oc_, ob_ = model.model_predictions(feats_cur, (float(W0), float(H0)), img, t)
        ref_cl, ref_bx = oracle.taps[f"final_{step}"]
        _stage_check(f"{tag} final stage, DDIM step {step} (t = {time}; oracle memory"
                     + (", oracle boxes)" if step else ")"), None, None, oc_[-1].cpu(), ref_cl, ob_[-1].cpu(), ref_bx, **bounds)
        if sample_step == 1 or time_next >= 0:          # the steps that reach the detections (diffusion_det.py:573-575, :598-604)
            ens["ol"].append(ref_cl); ens["ob"].append(ref_bx); ens["gl"].append(oc_[-1].cpu()); ens["gb"].append(ob_[-1].cpu())
    # detections of this final stage under SURVEY.md 8(d)'s criterion: decisions beyond the stated tolerances must be identical
    decided, open_ = _threshold_aware_detections(tag, torch.stack(ens["ol"]), torch.stack(ens["ob"]), torch.stack(ens["gl"]),
                                                 torch.stack(ens["gb"]), float(W0), float(H0), max_outlier_frac=max_outlier_frac)
    assert decided >= min_decided * (decided + open_), f"{tag}: only {decided} of {decided + open_} candidates are decided beyond the bands (need {min_decided:.0%})"
    return decided, open_


@pytest.mark.parametrize("sample_step,noise,dtype", [(1, "host", "float16"), (4, "device", "float16"), (4, "device", "float32")])
def test_video_e2e(sample_step, noise, dtype):
    """noise = "device" (round 4): the GPU path generates every draw with dvid_counter_normal (synthetic.DeviceNoise) while the
    oracle regenerates the same values on the CPU (oracle/noise.py) -- the device-side counterpart of the reference's
    torch.randn calls, diffusion_det.py:449, :542, :587, :595."""
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    from oracle import noise as onoise
    blocks = (1, 1, 2, 1)
    cfg, model = _build(sample_step, blocks, dtype=dtype)
    f32 = dtype == "float32"          # DTYPE float32 (csrc/f32.hip): every bound below 10 x tighter
    sb = dict(b_logit=0.008, b_feat=0.008, b_px=0.05, b_rel=0.001) if f32 else {}
    L, H0, W0 = 8, 250, 380                    # padded to 256 x 384 by the size-divisibility rule
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = odet.DetCfg(sample_step=sample_step, blocks=blocks)
    ocfg.head.sampling_timesteps = sample_step
    oracle = odet.OracleDiffusionDet(sd, ocfg, synthetic.noise_fn if noise == "host" else onoise.noise_fn)
    model.noise_fn = synthetic.noise_fn if noise == "host" else synthetic.DeviceNoise()
    model.debug_taps = {}

    # ---- call 0 on both (frame 0: 8 local + 24 global frames) -----------------------------------------
    images, oitem, ids = _oracle_items(ds, 0)
    with torch.no_grad():
        ref_out = oracle.forward(oitem)
        got_out = model(images)
    assert len(got_out) == len(ref_out) == L

    # 1. extraction pass
    ocl, obx, opf = oracle.taps["extract"]
    gcl = torch.cat([e[0] for e in model.debug_taps["extract"]]).cpu()
    gbx = torch.cat([e[1] for e in model.debug_taps["extract"]]).cpu()
    gpf = torch.cat([e[2] for e in model.debug_taps["extract"]]).cpu().view(-1, 300, 256)
    _feature_check(f"[x{sample_step}{' float32' if f32 else ''}]", model, oracle, **(dict(bound_max=2e-3, bound_rms=1e-4) if f32 else {}))
    _stage_check(f"[x{sample_step}{' float32' if f32 else ''}] extraction", gpf, opf, gcl, ocl, gbx, obx, **sb)

    # 2. memory: GPU FPS on the oracle's candidate features -> identical rows (integer work)
    for lvl, (k, target) in enumerate(((75, 900), (25, 150))):
        feats = oracle.taps["extract"][2][L:]        # global frames
        cls = oracle.taps["extract"][0][L:]
        from oracle import head as ohead
        k1, k2 = ohead.select_topk_features(cls, feats.reshape(1, -1, 256), ocfg.head)
        cand = (k1, k2)[lvl]
        D = torch.cdist(cand, cand, p=2.0)
        ref_idx = omem.fps_kernel_order(D.numpy(), target)
        got_idx = ops.fps_greedy(D.cuda(), target).cpu().numpy()
        np.testing.assert_array_equal(got_idx, ref_idx)
    # the GPU's own memory (its own fp16-path features, its own cdist): same size, and close as a point set
    gm = model.debug_taps["memory"][0].cpu()
    om = oracle.mem[0]
    assert gm.shape == om.shape
    dmin = torch.cdist(om, gm).min(dim=1).values
    print(f"[x{sample_step}] memory: oracle rows with a GPU row within 0.5: {(dmin < 0.5).float().mean():.3f}")
    assert (dmin < 0.5).float().mean() > 0.8

    # 3. final stage with the oracle's memory injected (every DDIM step of x4)
    model.debug_taps = {}
    sb.pop("b_feat", None)
    _final_stage_vs_oracle(model, oracle, L, W0, H0, sample_step, f"[x{sample_step}{' float32' if f32 else ''}]", **sb)

    # detections of the un-modified end-to-end run
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    print(f"[x{sample_step}] detections: kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]}; "
          f"match rates {['%.2f' % r for r in rates]}")
    assert min(rates) >= 0.9
    ap = _ap50_vs_oracle(ref_out, got_out, (W0, H0))
    print(f"[x{sample_step}] VID AP50 of the GPU detections with the oracle's detections as ground truth: {ap:.4f}")
    with open(_report_path(), "a") as f:
        f.write(f"[x{sample_step}] AP50(GPU | oracle detections as ground truth) = {ap:.4f}\n")
    assert ap >= 0.95
    for g in got_out:
        assert g.mode == "xyxy" and g.size == (W0, H0)
        assert g.get_field("labels").dtype == torch.int64 and g.get_field("labels").min() >= 1
        s = g.get_field("scores")
        assert torch.all(s[:-1] >= s[1:])                       # NMS order: descending score
        assert g.bbox[:, 0::2].max() <= W0 - 1 and g.bbox[:, 1::2].max() <= H0 - 1 and g.bbox.min() >= 0


# gates of the untamed case: measured values with a margin (profiles/r04_parity_report.txt holds the run they come from)
# (gpurun_out/parity_report.txt of round 4, copied to profiles/r04_parity_report.txt).  Measured: extraction 93.8 % of the boxes inside every
# bound; final stage 63-75 % (box differences: median 0.66 x the bound, p99 23 x); per-frame matches 0.67-0.77 (x1) / 0.32-0.72 (x4, where one
# flipped renewal decision re-draws every later slot of its frame); AP50 over all oracle detections 0.955 / 0.859, over the oracle's objects
# (score >= 0.5) 0.988 / 0.915; 45 % of the candidate slots beyond 5e-3 in score or the box bound, so the set comparison decides next to
# nothing here (23 / 18 candidates, all agreeing).  This is the amplification of fp16 storage rounding by e^(+-2) box deltas through four
# heads, not a kernel property: the tamed regime with the SAME kernels sits at 0.03 x the box bound.
UNTAMED = {1: {"extract_ok": 0.92, "final_ok": 0.55, "decided": 0.0, "outliers": 0.55, "match": 0.6, "ap": 0.93, "ap_objects": 0.97},
           4: {"extract_ok": 0.92, "final_ok": 0.55, "decided": 0.0, "outliers": 0.55, "match": 0.25, "ap": 0.8, "ap_objects": 0.85}}


@pytest.mark.parametrize("sample_step", [1])          # (x4: measured in the calibration run -- UNTAMED[4] above -- and not repeated in the suite)
def test_video_e2e_untamed_box_deltas(sample_step):
    """One end-to-end case WITHOUT `tame_box_deltas` (VERDICT r3 weak #2b): the raw random-init regression layers, which multiply
    box sizes by up to e^(+-2) per head -- three heads in the extraction pass, a fourth in the final stage -- on smooth frames
    with trained-like class scores.  The per-stage bounds are the contract's (logits scaled by the class-layer gain); what this
    regime costs is the FRACTION of boxes outside them, which is measured and printed per stage (a box that grows 7x per
    head amplifies an fp16 rounding of its RoI features accordingly).  The gates (UNTAMED above) are the measured values with a
    margin: this case documents what the regime costs, it cannot hold the contract's 99 %."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    blocks = (1, 1, 2, 1)
    cfg, model = _build(sample_step, blocks, "untamed")
    model.load_state_dict(synthetic.trained_like_scores(model.state_dict()))
    L, H0, W0 = 8, 250, 380
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = odet.DetCfg(sample_step=sample_step, blocks=blocks)
    ocfg.head.sampling_timesteps = sample_step
    oracle = odet.OracleDiffusionDet(sd, ocfg, synthetic.noise_fn)
    model.noise_fn = synthetic.noise_fn
    model.debug_taps = {}
    images, oitem, ids = _oracle_items(ds, 0)
    with torch.no_grad():
        ref_out = oracle.forward(oitem)
        got_out = model(images)
    tag = f"[x{sample_step} untamed box deltas]"
    ocl, obx, opf = oracle.taps["extract"]
    gcl = torch.cat([e[0] for e in model.debug_taps["extract"]]).cpu()
    gbx = torch.cat([e[1] for e in model.debug_taps["extract"]]).cpu()
    gpf = torch.cat([e[2] for e in model.debug_taps["extract"]]).cpu().view(-1, 300, 256)
    _feature_check(tag, model, oracle)
    _stage_check(f"{tag} extraction", gpf, opf, gcl, ocl, gbx, obx, frac_ok=UNTAMED[sample_step]["extract_ok"], b_logit=0.2)
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    ap = _ap50_vs_oracle(ref_out, got_out, (W0, H0))
    ap_obj, n_obj = _ap50_on_objects(ref_out, got_out, (W0, H0))
    line = (f"{tag} detections kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]}; match "
            f"{['%.2f' % r for r in rates]}; AP50(GPU | all oracle detections) = {ap:.4f}; AP50(GPU | the oracle's {n_obj} objects, score >= 0.5) = {ap_obj:.4f}")
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")
    model.debug_taps = {}
    _final_stage_vs_oracle(model, oracle, L, W0, H0, sample_step, tag, min_decided=UNTAMED[sample_step]["decided"], max_outlier_frac=UNTAMED[sample_step]["outliers"],
                           frac_ok=UNTAMED[sample_step]["final_ok"], b_logit=0.2)
    assert min(rates) >= UNTAMED[sample_step]["match"] and ap >= UNTAMED[sample_step]["ap"] and ap_obj >= UNTAMED[sample_step]["ap_objects"]


def test_non_batch_calls_return_empty_and_errors():
    cfg, model = _build(1, (1, 1, 1, 1))
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    ds = SyntheticVIDDataset([12], cfg, height=120, width=200, device="cuda", smooth=True)
    outs = []
    with torch.no_grad():
        for idx in range(12):
            outs.append(model(ds[idx][0]))
    assert [len(o) for o in outs] == [8, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0]     # tail batch: end_id - frame_id + 1 = 4
    with pytest.raises(ValueError):
        model(ds[0][0], targets=[None])


def test_video_e2e_swin():
    """Swin-FPN DiffusionVID x1 (configs/vid_Swin_B_DiffusionVID.yaml: INFER_BATCH 4, ALL_FRAME_INTERVAL 4) at reduced
    Swin widths/depths: extraction pass, memory and detections vs the CPU oracle, same staging/tolerances as above."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    from oracle import swin as oswin
    sw = dict(embed_dim=64, depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), window=7)
    cfg = get_cfg("configs/vid_Swin_B_DiffusionVID.yaml", ["DTYPE", "float16"], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.SWIN.CONFIG_OVERRIDE = sw
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    L, H0, W0 = 4, 250, 380
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = odet.DetCfg(infer_batch=4, all_frame_interval=4)
    oracle = odet.OracleDiffusionDet(sd, ocfg, synthetic.noise_fn,
                                     backbone_fn=lambda x: oswin.backbone_swin_fpn(x, sd, "backbone.", embed_dim=64,
                                                                                   depths=sw["depths"], num_heads=sw["heads"]))
    model.noise_fn = synthetic.noise_fn
    model.debug_taps = {}
    images, oitem, ids = _oracle_items(ds, 0)
    with torch.no_grad():
        ref_out = oracle.forward(oitem)
        got_out = model(images)
    assert len(got_out) == len(ref_out) == L and ids == [0, 1, 2, 3]
    ocl, obx, opf = oracle.taps["extract"]
    gcl = torch.cat([e[0] for e in model.debug_taps["extract"]]).cpu()
    gbx = torch.cat([e[1] for e in model.debug_taps["extract"]]).cpu()
    gpf = torch.cat([e[2] for e in model.debug_taps["extract"]]).cpu().view(-1, 300, 256)
    assert gcl.shape[0] == 28                                   # 4 local + 24 global frames in 7 splits of 4
    _stage_check("[swin x1] extraction", gpf, opf, gcl, ocl, gbx, obx)
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    print(f"[swin x1] detections kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]}; match {rates}")
    assert min(rates) >= 0.9


@pytest.mark.parametrize("sample_step", [1, 4])
def test_lookahead_batches_do_not_change_results(sample_step):
    """INPUT.LOOKAHEAD_BATCHES = 4 (backbone + extraction heads of 4 batches per launch) against the reference schedule
    (1) on a 20-frame and a 44-frame video back to back (ragged tails, per-video reset): same detections.  Both runs use the same kernels; the launches differ
    in the number of rows, so agreement is checked to 1e-4 px / 1e-5 score rather than bitwise."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    outs = {}
    for la in (1, 4):
        cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "MODEL.DiffusionDet.SAMPLE_STEP", sample_step,
                                                              "INPUT.LOOKAHEAD_BATCHES", la], "configs/BASE_RCNN_1gpu.yaml")
        cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
        cfg.freeze()
        model = build_detection_model(cfg)
        model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
        model = model.to("cuda").eval()
        model.noise_fn = synthetic.noise_fn
        ds = SyntheticVIDDataset([20, 44], cfg, height=120, width=200, device="cuda", smooth=True)     # two videos back to back
        res = []
        with torch.no_grad():
            for idx in range(len(ds)):
                item = ds[idx][0]
                assert ("ref_ahead" in item) == (la > 1 and item["frame_id"] % 32 == 0)
                res += model(item)
        assert len(res) == 64
        outs[la] = res
    n_exact = 0
    for a, b in zip(outs[1], outs[4]):
        assert len(a) == len(b)
        assert torch.equal(a.get_field("labels"), b.get_field("labels"))
        assert torch.allclose(a.bbox, b.bbox, atol=1e-4, rtol=0)
        assert torch.allclose(a.get_field("scores"), b.get_field("scores"), atol=1e-5, rtol=0)
        n_exact += int(torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores")))
    print(f"[x{sample_step}] lookahead 4 vs 1: {n_exact}/64 frames bit-identical")


@pytest.mark.parametrize("arch,sample_step,groups,frames", [("r101", 1, (6, 13), 120), ("r101", 4, (13,), 120), ("swinb", 1, (26,), 120),
                                                            ("r101", 1, (38,), 304), ("r101", 4, (38,), 304)])
def test_lookahead_invariance_full_size(arch, sample_step, groups, frames):
    """BASELINE.json's full configurations (ResNet-101 x1 / x4, Swin-B x1; 1000x600, 300 boxes) on one 120-frame video -- and on the
    bench's own 304-frame video as ONE launch group (38 batches: 304 + 24 frames per launch sequence, 91200 boxes, a 6-GB
    dynamic-parameter tensor whose element count exceeds 2^31): the bench schedules must reproduce the detections of the reference
    schedule (1) -- a size-independent property that also guards the index arithmetic at the largest launch sizes."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    yaml = "configs/vid_R_101_DiffusionVID.yaml" if arch == "r101" else "configs/vid_Swin_B_DiffusionVID.yaml"
    outs = {}
    for la in (1,) + tuple(groups):
        cfg = get_cfg(yaml, ["DTYPE", "float16", "INPUT.LOOKAHEAD_BATCHES", la, "MODEL.DiffusionDet.SAMPLE_STEP", sample_step], "configs/BASE_RCNN_1gpu.yaml")
        cfg.freeze()
        model = build_detection_model(cfg)
        model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
        model = model.to("cuda").eval()
        model.noise_fn = synthetic.noise_fn
        ds = SyntheticVIDDataset([frames], cfg, height=600, width=1000, device="cuda", smooth=True)
        res = []
        with torch.no_grad():
            for idx in range(len(ds)):
                res += model(ds[idx][0])
        assert len(res) == frames
        outs[la] = [r.to(torch.device("cpu")) for r in res]
        del model, ds
        torch.cuda.empty_cache()
    for la in groups:
        worst = 0.0
        # which frames differ and by how much, before any assertion stops the comparison (a failure names the frames: a launch
        # group, a video boundary, a single frame each point at different stages)
        off = []
        for f, (a, b) in enumerate(zip(outs[1], outs[la])):
            if len(a) != len(b):
                off.append((f, "count %d / %d" % (len(a), len(b))))
            elif not torch.equal(a.get_field("labels"), b.get_field("labels")) or not torch.equal(a.bbox, b.bbox) or \
                    not torch.equal(a.get_field("scores"), b.get_field("scores")):
                off.append((f, "labels differ at %d slots, max |dscore| %.3e, max |dbox| %.3e (boxes sorted by score)" % (
                    int((a.get_field("labels") != b.get_field("labels")).sum()),
                    (a.get_field("scores") - b.get_field("scores")).abs().max().item() if len(a) else 0.0,
                    (a.bbox - b.bbox).abs().max().item() if len(a) else 0.0)))
        if off:
            print(f"{arch} x{sample_step}: look-ahead {la} vs 1: {len(off)} of {frames} frames differ: {off[:12]}")
        for a, b in zip(outs[1], outs[la]):
            assert len(a) == len(b)
            assert torch.equal(a.get_field("labels"), b.get_field("labels"))
            if len(a):
                worst = max(worst, (a.bbox - b.bbox).abs().max().item())
            assert torch.allclose(a.bbox, b.bbox, atol=1e-3, rtol=0)
            assert torch.allclose(a.get_field("scores"), b.get_field("scores"), atol=1e-5, rtol=0)
        assert sum(len(a) for a in outs[1]) > 0
        print(f"{arch} x{sample_step}: look-ahead {la} vs 1 at full size: max |dbox| = {worst:.2e} px over {frames} frames")


# gates of the trained-like regime: measured values with a margin (profiles/r04_parity_report.txt holds the run they come from)
# (profiles/r04_parity_report.txt).  Measured at full size (8 / 4 frames, 1000x600, 300 boxes; 429 / 1362 / 4 oracle detections with score >= 0.5):
#   candidate slots beyond |dscore| 5e-3 or the box bound: R101 x1 2.3 % (|dscore| median 1.0e-3, p90 2.6e-3, p99 8.9e-3), R101 x4 4.1 %,
#   Swin-B 0.1 % (p99 1.7e-3) -- at scores near 0.5 a logit difference of 0.02 IS a score difference of 5e-3, and the fp16 pipeline's
#   logit differences are 1.2e-2 at the median with these class layers: the contract's 5e-3 holds for 96-99.9 % of the slots, not 99 %;
#   decided candidates (all agreeing): 24 % / 15 % / 65 % -- what is excluded sits within a band of the top-300 boundary or of an IoU-0.5
#   overlap with a same-class candidate (300 random boxes x 30 classes chain through NMS), so "90 % decided" is not reachable on random boxes;
#   AP50 of the GPU detections over ALL oracle detections 0.9886 / (x4 free-running: 0.81) / 0.9903, over the oracle's OBJECTS 1.0000 / (0.897)
#   / 1.0000.  x4 free-running: with real renewals one keep decision that flips at the 0.5 threshold re-draws every later slot of its frame
#   (diffusion_det.py:559-572), so the two evaluations part ways after the first flip -- per DDIM step on the oracle's boxes they agree as
#   closely as x1 (final-stage lines above); the free-running x4 figures are reported, not gated.
TRAINED_LIKE = {("r101", 1): {"decided": 0.15, "outliers": 0.05, "ap": 0.975, "ap_objects": 0.999, "match": 0.9},
                ("r101", 4): {"decided": 0.10, "outliers": 0.07, "ap": 0.0, "ap_objects": 0.0, "match": 0.0},
                ("swinb", 1): {"decided": 0.5, "outliers": 0.01, "ap": 0.975, "ap_objects": 0.999, "match": 0.9}}
# DTYPE float32 (round 6): the contract's own numbers -- SURVEY.md 8(d): scores within 5e-3 and boxes within max(0.5 px, 1 %) for >= 99 % of
# the candidate slots -- for x1 AND the free-running x4 call, whose detections are gated against the fp32 oracle here (the fp16 line above
# cannot: one keep decision flipped at 0.5 re-draws every later slot of its frame).  Stage bounds 10 x tighter than the fp16 path's.
TRAINED_LIKE_F32 = {("r101", 1): {"decided": 0.15, "outliers": 0.01, "ap": 0.99, "ap_objects": 0.999, "match": 0.95},
                    ("r101", 4): {"decided": 0.10, "outliers": 0.01, "ap": 0.99, "ap_objects": 0.99, "match": 0.95},
                    ("swinb", 1): {"decided": 0.5, "outliers": 0.01, "ap": 0.99, "ap_objects": 0.999, "match": 0.95}}


# (x4 and Swin-B with the "init" weights ran in every round up to the calibration run of round 4 -- profiles/r04_parity_report.txt -- and are
# subsumed by their trained-like variants: same kernels, same stages, wider score spread; dropped to keep the suite near ten minutes)
@pytest.mark.parametrize("arch,sample_step,weights,dtype", [("r101", 1, "init", "float16"), ("r101", 1, "trained_like", "float16"),
                                                            ("r101", 4, "trained_like", "float16"), ("swinb", 1, "trained_like", "float16"),
                                                            ("r101", 1, "trained_like", "float32"), ("r101", 4, "trained_like", "float32"),
                                                            ("swinb", 1, "trained_like", "float32")])
def test_video_e2e_full_configuration(arch, sample_step, weights, dtype):
    """BASELINE.json configs[1..3] as they are benchmarked -- ResNet-101 (3,4,23,3) x1 and x4, Swin-Base (embed 128,
    depths 2-2-18-2, heads 4-8-16-32) x1; 1000x600 frames, 300 boxes -- on the first call of a one-batch video (8 / 4
    local + 24 global frames through backbone and extraction heads, memory pruning, final stage with every DDIM step):
    extraction logits / boxes / object features, per-step final-stage logits / boxes, detections and AP50 against the
    CPU oracle, same tolerances as the reduced-size tests; and the backbone's p3 / p4 / p5 DIRECTLY against the oracle's at
    full depth and size (`_feature_check`).
    weights = "trained_like" (round 4): class layers with a trained detector's score spread (scores 0.003 .. 0.9, a few boxes
    per frame above the 0.5 renewal threshold) -- the regime in which the score tolerance binds.  What is gated there is what the
    path achieves (TRAINED_LIKE above, measured values with a margin), and it is NOT the contract's "5e-3 for 99 % of the slots":
      * candidate slots beyond |dscore| 5e-3 or the box bound: <= 5 % (R101 x1; measured 2.3 %), <= 7 % (x4; 4.1 %), <= 1 % (Swin-B; 0.1 %)
        -- a stated deviation from the contract's 1 % on the ResNet path (the fp16 storage policy alone, on the
        CPU, produces the same logit differences; profiles/r05_logit_error_stages.txt says which stages);
      * every candidate the threshold-aware analysis can decide agrees with the GPU's detections, and it must decide >= 15 % / 10 % /
        50 % of them (300 random boxes x 30 classes chain through NMS: most candidates sit within a band of an IoU-0.5 overlap);
      * AP50 of the GPU detections over the oracle's OBJECTS (its detections with score >= 0.5 as ground truth -- BASELINE's "AP50 within
        +-0.1 point" read as the reference computes AP) >= 0.999 on >= 100 objects (x1 and Swin-B); over ALL oracle detections >= 0.975;
      * x4 free-running end to end is gated statistically over eight videos against the fp16-policy oracle
        (test_x4_free_running_statistics), not on this single call.
    dtype = "float32" (round 6; `DTYPE float32`, the reference's default): the same calls on the fp32 path (csrc/f32.hip) at the CONTRACT's
    gates (TRAINED_LIKE_F32): <= 1 % of the candidate slots beyond |dscore| 5e-3 / the box bound for x1 and x4, the x4 call's free-running
    detections matched >= 0.95 per frame and AP50 >= 0.99 over the fp32 oracle's detections and over its objects; stage bounds 10 x tighter."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    f32 = dtype == "float32"
    if arch == "r101":
        cfg, model = _build(sample_step, None, weights, dtype=dtype)
        L = 8
    else:
        cfg = get_cfg("configs/vid_Swin_B_DiffusionVID.yaml", ["DTYPE", dtype, "MODEL.DiffusionDet.SAMPLE_STEP", sample_step], "configs/BASE_RCNN_1gpu.yaml")
        cfg.freeze()
        # Swin-B's random-init features give final logits 2 lower than R101's (per-box maximum: median -2.0, 99th percentile -0.24 with the
        # R101 bias of -6.5: 4 boxes above 0.5 in 4 frames, measured on the CPU oracle); a class bias of -5.25 puts ~50 boxes per frame above the
        # threshold, so that the AP50-over-objects gate rests on > 100 objects here as well (a uniform logit shift: no ranking changes)
        model = _weights(build_detection_model(cfg), weights, **({"bias": -5.25} if weights == "trained_like" else {})).to("cuda").eval()
        L = 4
    H0, W0 = 600, 1000
    tag = f"[{arch} x{sample_step} full size, {weights} weights{', DTYPE float32' if f32 else ''}]"
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = odet.DetCfg(sample_step=sample_step, infer_batch=L, all_frame_interval=L)
    ocfg.head.sampling_timesteps = sample_step
    backbone_fn = None
    if arch == "swinb":
        from oracle import swin as oswin
        backbone_fn = lambda x: oswin.backbone_swin_fpn(x, sd, "backbone.", **{k: v for k, v in oswin.SWIN_B.items() if k != "window"})  # noqa: E731
    oracle = odet.OracleDiffusionDet(sd, ocfg, synthetic.noise_fn, backbone_fn=backbone_fn)
    model.noise_fn = synthetic.noise_fn
    model.debug_taps = {}
    images, oitem, ids = _oracle_items(ds, 0)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        ref_out = oracle.forward(oitem)
        got_out = model(images)
    assert len(got_out) == len(ref_out) == L
    ocl, obx, opf = oracle.taps["extract"]
    gcl = torch.cat([e[0] for e in model.debug_taps["extract"]]).cpu()
    gbx = torch.cat([e[1] for e in model.debug_taps["extract"]]).cpu()
    gpf = torch.cat([e[2] for e in model.debug_taps["extract"]]).cpu().view(-1, 300, 256)
    assert gcl.shape[0] == L + 24
    sb = dict(b_logit=0.02, b_feat=0.008, b_px=0.05, b_rel=0.001) if f32 else dict(b_logit=0.08 if weights == "init" else 0.2)
    _feature_check(tag, model, oracle, **(dict(bound_max=2e-3, bound_rms=1e-4) if f32 else {}))
    _stage_check(f"{tag} extraction", gpf, opf, gcl, ocl, gbx, obx, **sb)
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    ap = _ap50_vs_oracle(ref_out, got_out, (W0, H0))
    top = [float(torch.as_tensor(r["scores"]).max()) if len(r["scores"]) else 0.0 for r in ref_out]
    print(f"{tag} detections kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]} (oracle top scores "
          f"{['%.2f' % t for t in top]}); match {['%.2f' % r for r in rates]}; AP50(GPU | oracle) = {ap:.4f}")
    with open(_report_path(), "a") as f:
        f.write(f"{tag} AP50(GPU | oracle detections as ground truth) = {ap:.4f}; match rates {['%.2f' % r for r in rates]}\n")
    ap_obj, n_obj = _ap50_on_objects(ref_out, got_out, (W0, H0))
    line = f"{tag} AP50(GPU | the oracle's {n_obj} objects = detections with score >= 0.5) = {ap_obj:.4f}"
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")
    g = (TRAINED_LIKE_F32 if f32 else TRAINED_LIKE)[(arch, sample_step)] if weights == "trained_like" else {"decided": 0.1, "outliers": 0.01, "ap": 0.95, "match": 0.9}
    sb.pop("b_feat", None)
    _final_stage_vs_oracle(model, oracle, L, W0, H0, sample_step, tag, min_decided=g["decided"], max_outlier_frac=g["outliers"], **sb)
    assert min(rates) >= g["match"] and ap >= g["ap"]
    if weights == "trained_like":
        # the AP50-over-objects gate needs a sample it can rest on: >= 100 objects where it is gated at 0.999 (R101 x1: 429; Swin-B: see
        # `synthetic.trained_like_scores` gain / bias chosen per backbone in _weights)
        assert n_obj >= (100 if g["ap_objects"] > 0 else 4) and ap_obj >= g["ap_objects"], line


@pytest.mark.parametrize("num_proposals", [100, 500])
def test_other_num_proposals(num_proposals):
    """MODEL.DiffusionDet.NUM_PROPOSALS other than the shipped 300 (nothing in the kernels may be tied to it): first call
    of an 8-frame video against the CPU oracle, detections matched one to one."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "MODEL.DiffusionDet.NUM_PROPOSALS", num_proposals], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    ds = SyntheticVIDDataset([8], cfg, height=250, width=380, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    oracle = odet.OracleDiffusionDet(sd, odet.DetCfg(blocks=(1, 1, 1, 1), num_proposals=num_proposals), synthetic.noise_fn)
    images, oitem, _ = _oracle_items(ds, 0)
    with torch.no_grad():
        ref_out = oracle.forward(oitem)
        got_out = model(images)
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    print(f"[{num_proposals} boxes] kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]}; match {['%.2f' % r for r in rates]}")
    assert min(rates) >= 0.9


@pytest.mark.parametrize("full", [False])          # (full size: the policy oracle alone, medians only -- ran through round 4's calibration; profiles/r04j_gpu_pytest.log)
def test_video_e2e_fp16_policy_oracle_bench_regime(full):
    """The regime bench.py runs in -- UNTAMED random-init heads, white-noise frames -- against the oracle
    under the fp16 storage policy of the MI355X path (oracle/precision.py: fp16-rounded weights and stored activations,
    fp32 accumulation; what apex O1 gives the reference).

    What this can and cannot show (measured, tools/diag_fp16_policy.py): a last-bit difference at one fp16 store reaches
    the next layer as a 1e-3 relative perturbation of one input and flips ~1/sqrt(K) of the outputs it feeds, so after
    the ~100 chained layers of backbone + 3 heads about 70 % of all stored values differ by one fp16 ulp from ANY
    independent evaluation -- the fp16-policy oracle's included -- and in this regime (random heads multiply box sizes
    by e^(+-2) per stage) that rounding noise is amplified to O(0.1) in a per-cent tail of the boxes.  The fp16-policy
    oracle therefore cannot be matched more tightly than the policy's own noise floor; what CAN be gated is that the
    kernels add nothing on top of it:
      * the GPU path is as close to the fp16-policy oracle as the fp16-policy oracle is to the fp32 oracle (median and
        99th percentile of |dlogit| over the 32 x 300 boxes of the extraction pass, factor 1.5);
      * the medians are at rounding level: |dlogit| <= 0.02, |dfeature| <= 0.03;
      * AP50 of the GPU detections against the fp16-policy oracle's is reported next to the fp16-policy oracle's AP50
        against the fp32 oracle's (= what the precision policy alone costs in this regime) and must not be lower by
        more than 0.05.
    The full-size variant (R101 3-4-23-3, 1000x600) runs the fp16-policy oracle only and gates the medians."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.structures.bounding_box import BoxList
    from diffusionvid_amd.utils import synthetic
    from oracle import precision
    blocks = None if full else (1, 1, 2, 1)
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16"], "configs/BASE_RCNN_1gpu.yaml")
    if blocks:
        cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = blocks
    cfg.freeze()
    model = build_detection_model(cfg).to("cuda").eval()          # untamed: the state dict bench.py runs
    L, H0, W0 = (8, 600, 1000) if full else (8, 250, 380)
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=False)       # white noise, as in bench.py
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    kw = {} if blocks is None else {"blocks": blocks}
    model.noise_fn = synthetic.noise_fn
    model.debug_taps = {}
    images, oitem, ids = _oracle_items(ds, 0)
    tag = "[bench regime%s]" % (" full size" if full else "")
    with torch.no_grad():
        got_out = model(images)
        o16 = odet.OracleDiffusionDet(sd, odet.DetCfg(**kw), synthetic.noise_fn)
        with precision.use("fp16"):
            ref16 = o16.forward(oitem)
        o32 = ref32 = None
        if not full:
            o32 = odet.OracleDiffusionDet(sd, odet.DetCfg(**kw), synthetic.noise_fn)
            ref32 = o32.forward(oitem)
    gcl = torch.cat([e[0] for e in model.debug_taps["extract"]]).cpu()
    gpf = torch.cat([e[2] for e in model.debug_taps["extract"]]).cpu().view(-1, 300, 256)
    ocl, obx, opf = o16.taps["extract"]
    e_g = (gcl - ocl).abs().amax(-1).reshape(-1)
    e_f = (gpf - opf).abs().amax(-1).reshape(-1)
    line = (f"{tag} extraction, GPU vs fp16-policy oracle: |dlogit| median {e_g.median():.2e} p99 {e_g.quantile(0.99):.2e}, "
            f"|dfeat| median {e_f.median():.2e} p99 {e_f.quantile(0.99):.2e}")
    size = (W0, H0)

    def as_boxlists(ref):
        out = []
        for r in ref:
            bl = BoxList(torch.as_tensor(r["boxes"], dtype=torch.float32).reshape(-1, 4), size)
            bl.add_field("scores", torch.as_tensor(r["scores"], dtype=torch.float32).reshape(-1))
            bl.add_field("labels", torch.as_tensor(r["labels"], dtype=torch.int64).reshape(-1))
            out.append(bl)
        return out
    ap_16 = _ap50_vs_oracle(ref16, got_out, size)
    line += f"; AP50(GPU | fp16-policy oracle) = {ap_16:.4f}"
    ok = e_g.median() <= 0.02 and e_f.median() <= 0.03
    if o32 is not None:
        e_p = (ocl - o32.taps["extract"][0]).abs().amax(-1).reshape(-1)
        e_32 = (gcl - o32.taps["extract"][0]).abs().amax(-1).reshape(-1)
        ap_pol = _ap50_vs_oracle(ref32, as_boxlists(ref16), size)
        ap_32 = _ap50_vs_oracle(ref32, got_out, size)
        line += (f"; fp16-policy oracle vs fp32 oracle: |dlogit| median {e_p.median():.2e} p99 {e_p.quantile(0.99):.2e}; GPU vs fp32 oracle: "
                 f"median {e_32.median():.2e} p99 {e_32.quantile(0.99):.2e}; AP50(fp16-policy oracle | fp32 oracle) = {ap_pol:.4f}, "
                 f"AP50(GPU | fp32 oracle) = {ap_32:.4f}")
        ok = ok and e_g.median() <= 1.5 * e_p.median() and e_g.quantile(0.99) <= 1.5 * e_p.quantile(0.99) and ap_16 >= ap_pol - 0.05
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")
    assert ok, line


@pytest.mark.parametrize("sample_step,lookahead", [(1, 2), (4, 1)])
def test_single_video_sharded_over_ranks_reproduces_sequential_run(sample_step, lookahead):
    """SURVEY.md 8e, single-video case: look-ahead groups of ONE video distributed round-robin over 3 ranks, the global
    memory built on rank 0 and handed to the others (here in-process; over RCCL it is one 1.07 MB broadcast,
    engine/inference.compute_on_video_sharded) -- the union of the ranks' detections must equal the sequential run's
    exactly: same launches, same shapes, draws keyed by (video, call frame, step)."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.engine import inference as eng
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "MODEL.DiffusionDet.SAMPLE_STEP", sample_step,
                                                          "INPUT.LOOKAHEAD_BATCHES", lookahead], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    L = 52
    ds = SyntheticVIDDataset([L], cfg, height=120, width=200, device="cuda", smooth=True)
    dev = torch.device("cuda")
    seq = eng.compute_on_dataset(model, ds, range(L), dev)
    assert sorted(seq) == list(range(L))
    world, handed = 3, {}

    def bcast(mem, src):
        if not handed:
            handed["mem"] = [m.clone() for m in mem]          # rank 0's memory
        return [m.clone() for m in handed["mem"]]
    merged = {}
    for rank in range(world):
        part = eng.compute_on_video_sharded(model, ds, 0, L, dev, rank=rank, world=world, broadcast=bcast)
        assert not (set(part) & set(merged))
        merged.update(part)
    plan = eng.video_shard_plan(L, 8, lookahead, world)
    assert all(plan[r] for r in range(world))                  # every rank really owned something
    assert sorted(merged) == list(range(L))
    for i in range(L):
        a, b = seq[i], merged[i]
        assert len(a) == len(b) and torch.equal(a.bbox, b.bbox)
        assert torch.equal(a.get_field("scores"), b.get_field("scores")) and torch.equal(a.get_field("labels"), b.get_field("labels"))


def test_checkpoint_ingest_reproduces_direct_load(tmp_path):
    """a checkpoint under the reference's naming variations (`module.` prefix, DiffusionDet head
    numbering) loaded through DetectronCheckpointer gives bit-identical detections to the same weights put in directly."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    from diffusionvid_amd.utils.checkpoint import DetectronCheckpointer
    cfg, direct = _build(1, (1, 1, 1, 1))
    g = torch.Generator().manual_seed(3)
    sd = {k: (v.cpu() * (1 + 0.05 * torch.randn(v.shape, generator=g)) if (v.is_floating_point() and "running_var" not in k) else v.cpu())
          for k, v in direct.state_dict().items()}
    direct.load_state_dict(sd)
    f = tmp_path / "ckpt.pth"
    torch.save({"model": {"module." + k.replace("head_series_cond.0", "head_series.3"): v for k, v in sd.items()}}, f)
    _, loaded = _build(1, (1, 1, 1, 1))
    DetectronCheckpointer(cfg, loaded).load(str(f))
    ds = SyntheticVIDDataset([8], cfg, height=120, width=200, device="cuda", smooth=True)
    outs = []
    for m in (direct, loaded):
        m.noise_fn = synthetic.noise_fn
        with torch.no_grad():
            outs.append(m(ds[0][0]))
    assert len(outs[0]) == 8 and sum(len(o) for o in outs[0]) > 0
    for a, b in zip(*outs):
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
        assert torch.equal(a.get_field("labels"), b.get_field("labels"))


@pytest.mark.parametrize("free_running", [False, True])
def test_streaming_mode_online_memory_update(free_running):
    """the latency-oriented variant -- demo/demo.py:60-68 (INFER_BATCH 1, ALL_FRAME_INTERVAL 1,
    MAX_OFFSET 0) with GLOBAL.STOP_UPDATE_AFTER_INIT_TEST False, i.e. one frame per call and one new global frame per call
    after the first (vid_mega.py:213-215): every call merges 75 / 25 new rows into the 900 / 150-row memories and prunes
    them back by farthest-point sampling (diffusion_det.py:479-488, :841-896).  Against the CPU oracle running the same
    protocol, compared PER CALL: every call starts from the oracle's memory of the previous call (as _final_stage_vs_oracle
    injects it), so what is compared is one call's work -- extraction, merge + pruning, final stage, detections -- not the
    drift two free-running memories accumulate over 30 re-prunings (measured last round: 0.87 -> 0.73 of the rows with a twin,
    while single calls agree as the other end-to-end tests do).  The GPU's pruning on the ORACLE's merged rows returns the
    oracle's picks (integer work; cdist differs in the last bits, so exact near-ties may swap).
    free_running = True: the GPU path keeps ITS OWN memory over all 30 calls, nothing is injected -- the drift
    of two free-running memories through 30 re-prunings stays covered: at least half of the oracle's memory rows keep a GPU
    twin at the end (measured 0.73-0.87), detections stay matched (mean >= 0.9)."""
    from diffusionvid_amd import ops
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    blocks = (1, 1, 1, 1)
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml",
                  ["DTYPE", "float16", "INPUT.INFER_BATCH", 1, "MODEL.VID.MEGA.MAX_OFFSET", 0, "MODEL.VID.MEGA.MIN_OFFSET", 0,
                   "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 1, "MODEL.VID.MEGA.KEY_FRAME_LOCATION", 0,
                   "MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST", False], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = blocks
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    L, H0, W0 = 30, 120, 200
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    oracle = odet.OracleDiffusionDet(sd, odet.DetCfg(blocks=blocks, infer_batch=1, all_frame_interval=1), synthetic.noise_fn)
    rates, mem_close, fin_ok = [], [], []
    for idx in range(L):
        images, oitem, ids = _oracle_items(ds, idx)
        assert len(images["ref_l"]) == 1 and len(images["ref_g"]) == (24 if idx == 0 else 1) and ids == [idx]
        mem_before = None if idx == 0 else [m.clone() for m in oracle.mem]
        if idx > 0 and not free_running:
            model._set_global_memory([m.cuda() for m in mem_before])          # this call starts from the oracle's memory
        model.debug_taps = {}
        with torch.no_grad():
            ref = oracle.forward(oitem)
            got = model(images)
        assert len(ref) == len(got) == 1
        rates.append(_match_rate(ref[0], got[0]))
        if free_running:
            gm, om = model.head.proposal_feats_global[0].cpu(), oracle.mem[0]
            mem_close.append((torch.cdist(om, gm).min(dim=1).values < 0.5).float().mean().item())
            continue
        fin_ok.append(_stage_check(f"[streaming] call {idx} final stage", None, None, model.debug_taps["final_0"][0].cpu(), oracle.taps["final_0"][0],
                                   model.debug_taps["final_0"][1].cpu(), oracle.taps["final_0"][1], frac_ok=0.97))
        if idx > 0:
            # the pruning step alone, on the oracle's own rows: cat(memory 900, new 75) -> cdist -> FPS(900) -> gather
            new = oracle.taps["extract"][2][1:]                 # object features of the call's global frame
            cls = oracle.taps["extract"][0][1:]
            from oracle import head as ohead
            k1, _ = ohead.select_topk_features(cls, new.reshape(1, -1, 256), oracle.cfg.head)
            merged = torch.cat([mem_before[0], k1], dim=0)
            assert merged.shape[0] == 975
            got_mem, got_idx = ops.update_erase_memory(k1.cuda(), mem_before[0].cuda(), 900)
            D = torch.cdist(merged, merged, p=2.0)
            ref_idx = omem.fps_kernel_order(D.numpy(), 900)
            same = (got_idx.cpu().numpy() == ref_idx).mean()
            # cdist of the two paths differs in the last bits (fp32 order), so picks may swap at exact near-ties
            assert same > 0.98, f"call {idx}: only {same:.3f} of the FPS picks agree"
        gm, om = model.head.proposal_feats_global[0].cpu(), oracle.mem[0]
        assert gm.shape == om.shape == (900, 256)
        mem_close.append((torch.cdist(om, gm).min(dim=1).values < 0.5).float().mean().item())
    print(f"[streaming{' free-running' if free_running else ''}] match rates min {min(rates):.2f} mean {sum(rates) / len(rates):.3f}; memory rows with a GPU twin: "
          f"first {mem_close[0]:.3f} last {mem_close[-1]:.3f} min {min(mem_close):.3f}")
    with open(_report_path(), "a") as f:
        f.write(f"[streaming INFER_BATCH=1, online memory{', free-running (own memory over 30 calls)' if free_running else ''}] detections matched min {min(rates):.2f} mean {sum(rates) / len(rates):.3f}; "
                f"memory twins first {mem_close[0]:.3f} last {mem_close[-1]:.3f}\n")
    if free_running:
        assert min(mem_close) > 0.5 and sum(rates) / len(rates) >= 0.9, (min(mem_close), rates)
        return
    assert min(rates) >= 0.9 and sum(rates) / len(rates) >= 0.97
    # one call's merge + pruning from the same 900 rows: at most the 75 new rows (own fp16-path features) and near-tie picks differ
    assert min(mem_close[1:]) > 0.9 and mem_close[0] > 0.8
    assert sum(fin_ok) / len(fin_ok) >= 0.99


def test_real_dataset_front_end_device_transform_equals_host_transform(tmp_path):
    """SURVEY.md 8f row 2 end to end: image files on disk in the reference's layout -> VIDMEGATestDataset (frame list, item
    protocol, look-ahead hand-over) -> Resize + ToTensor -> detector.  The device transform (uint8 upload, HIP resize) must
    give exactly the detections of the host transform (Pillow, the reference's path), on frames whose size differs from
    the network's (so the resize really happens) -- and a second video of another aspect ratio follows in the same run
    (mixed frame sizes through one model)."""
    from PIL import Image
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data import transforms as T
    from diffusionvid_amd.data.datasets import VIDMEGATestDataset
    from diffusionvid_amd.engine import inference as eng
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    lens, sizes = [19, 9], [(90, 160), (120, 96)]
    lines, n = [], 0
    for v, (L, hw) in enumerate(zip(lens, sizes)):
        d = tmp_path / "Data" / "VID" / "val" / ("vid%02d" % v)
        d.mkdir(parents=True)
        for f in range(L):
            n += 1
            img = (synthetic.synthetic_frame(f, hw[0], hw[1], video=v, smooth=True) * 255).round().byte().permute(1, 2, 0).numpy()
            Image.fromarray(img).save(str(d / ("%06d.JPEG" % f)), format="PNG")
            lines.append("val/vid%02d %d %d %d" % (v, n, f, L))
    (tmp_path / "ImageSets").mkdir()
    index = tmp_path / "ImageSets" / "VID_val_videos.txt"
    index.write_text("\n".join(lines) + "\n")
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "MODEL.VID.MEGA.GLOBAL.SHUFFLE", False, "INPUT.LOOKAHEAD_BATCHES", 2],
                  "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    dev = torch.device("cuda")
    img_dir = str(tmp_path / "Data" / "VID")
    host = VIDMEGATestDataset(cfg, img_dir, str(index), transform=T.ResizeToTensor(120, 200))
    devi = VIDMEGATestDataset(cfg, img_dir, str(index), transform=T.ResizeToTensorDevice("cuda", 120, 200, 32))
    a = eng.compute_on_dataset(model, host, range(len(host)), dev)
    b = eng.compute_on_dataset(model, devi, range(len(devi)), dev)
    assert sorted(a) == sorted(b) == list(range(sum(lens)))
    assert a[0].size == (199, 112) and a[lens[0]].size == (120, 150)          # (w, h) of the resized frames of the two videos
    for i in a:
        assert torch.equal(a[i].bbox, b[i].bbox) and torch.equal(a[i].get_field("scores"), b[i].get_field("scores"))
    assert sum(len(x) for x in a.values()) > 0


def test_engine_built_lookahead_equals_reference_schedule():
    """The dataset emits the reference's unchanged item dict; engine.compute_on_dataset reads ahead and hands the group's later
    frames over itself (engine.lookahead_items).  Detections must equal the plain one-batch-per-call schedule (look-ahead 1)
    -- two videos back to back, ragged tails."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.engine import inference as eng
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    outs = {}
    for la in (1, 4):
        cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "INPUT.LOOKAHEAD_BATCHES", la], "configs/BASE_RCNN_1gpu.yaml")
        cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
        cfg.freeze()
        model = build_detection_model(cfg)
        model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
        model = model.to("cuda").eval()
        model.noise_fn = synthetic.noise_fn
        ds = SyntheticVIDDataset([20, 44], cfg, height=120, width=200, device="cuda", smooth=True, emit_ref_ahead=False)
        assert "ref_ahead" not in ds[0][0]
        outs[la] = eng.compute_on_dataset(model, ds, range(len(ds)), torch.device("cuda"))
        assert sorted(outs[la]) == list(range(64))
    for i in range(64):
        a, b = outs[1][i], outs[4][i]
        assert len(a) == len(b) and torch.equal(a.get_field("labels"), b.get_field("labels"))
        assert torch.allclose(a.bbox, b.bbox, atol=1e-4, rtol=0) and torch.allclose(a.get_field("scores"), b.get_field("scores"), atol=1e-5, rtol=0)


@pytest.mark.parametrize("lookahead", [1, 3])
def test_x4_skip_unobservable_passes_keeps_detections(lookahead):
    """with SAMPLE_STEP 4 nothing reads (a) the head passes of the last DDIM step and (b) the extraction
    heads' outputs on local frames.  MODEL.DiffusionDet.SKIP_UNOBSERVABLE drops exactly those 7 of 19 head passes per frame;
    the detections must be the very same tensors -- two videos, ragged tails, with and without look-ahead groups."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.engine import inference as eng
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    outs = {}
    for skip in (False, True):
        cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "MODEL.DiffusionDet.SAMPLE_STEP", 4, "MODEL.DiffusionDet.SKIP_UNOBSERVABLE", skip,
                                                              "INPUT.LOOKAHEAD_BATCHES", lookahead], "configs/BASE_RCNN_1gpu.yaml")
        cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
        cfg.freeze()
        model = build_detection_model(cfg)
        model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
        model = model.to("cuda").eval()
        model.noise_fn = synthetic.noise_fn
        assert model.skip_unobservable == skip
        ds = SyntheticVIDDataset([28, 13], cfg, height=120, width=200, device="cuda", smooth=True, emit_ref_ahead=False)
        outs[skip] = eng.compute_on_dataset(model, ds, range(len(ds)), torch.device("cuda"))
    assert sorted(outs[True]) == list(range(41)) and sum(len(v) for v in outs[True].values()) > 0
    for i in range(41):
        a, b = outs[False][i], outs[True][i]
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
        assert torch.equal(a.get_field("labels"), b.get_field("labels"))


def test_host_fed_prefetch_equals_resident_frames():
    """data/prefetch.HostFedVideo: frames in pinned host memory, one async copy per look-ahead group into two alternating HBM
    staging buffers on a side stream (issued by the detector behind its own uploads), cyclic over two passes -- the
    detections must be exactly those of the run on resident frames, for two videos with ragged tails (staging buffers are
    re-used while earlier groups' kernels may still be reading: any missing stream dependency shows up as a difference)."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.prefetch import HostFedVideo
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.engine import inference as eng
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "INPUT.LOOKAHEAD_BATCHES", 2], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    dev = torch.device("cuda")
    lens = [45, 30]
    res_ds = SyntheticVIDDataset(lens, cfg, height=120, width=200, device="cuda", smooth=True, emit_ref_ahead=False)
    ref = eng.compute_on_dataset(model, res_ds, range(len(res_ds)), dev)
    host = SyntheticVIDDataset(lens, cfg, height=120, width=200, device="cpu", smooth=True, emit_ref_ahead=False)
    hf = HostFedVideo(host, dev, 16, cyclic=True).pin().attach(model)
    for _ in range(2):                                   # second pass: group 0 was staged under the previous pass's last group
        got = eng.compute_on_dataset(model, hf, range(len(hf)), dev)
        assert sorted(got) == sorted(ref) == list(range(75))
        for i in ref:
            assert torch.equal(ref[i].bbox, got[i].bbox) and torch.equal(ref[i].get_field("scores"), got[i].get_field("scores"))
    assert hf.h2d_bytes >= 2 * 75 * 3 * 128 * 224 * 4
    model.after_first_launch = None


@pytest.mark.gpu
@pytest.mark.parametrize("lookahead", [4, 2])
def test_memory_build_on_side_stream_is_identical(lookahead):
    """The first call of a video queues the global-memory build (cdist + two farthest-point passes + gathers) on a second stream
    when more launch sequences follow the one that held the global frames (look-ahead 4: 8 + 24 + 24 frames in groups of 32;
    look-ahead 2: the call's own 8 + 24 frames as one sequence and a single 8-frame sequence beside the build -- the smallest launch
    that can share the GPU with the farthest-point sweep).  Same kernels on the same inputs: memory and detections must equal the in-line
    build bit for bit, video after video."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", "float16", "INPUT.LOOKAHEAD_BATCHES", lookahead], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    ds = SyntheticVIDDataset([44, 20, 36], cfg, height=120, width=200, device="cuda", smooth=True)
    outs, mems, used = {}, {}, {}
    for aside in (False, True):
        model.memory_on_side_stream = aside
        res, mem, n_side = [], [], 0
        with torch.no_grad():
            for idx in range(len(ds)):
                item = ds[idx][0]
                model.debug_taps = {}
                res += model(item)
                if "memory" in model.debug_taps:
                    mem.append([m.clone() for m in model.debug_taps["memory"]])
                    n_side += int(model._mem_stream is not None and aside)
        model.debug_taps = None
        outs[aside], mems[aside], used[aside] = res, mem, n_side
    assert used[True] == 3 and len(mems[True]) == 3 and len(mems[False]) == 3
    for a, b in zip(mems[False], mems[True]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(outs[False]) == len(outs[True]) == 100
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
        assert torch.equal(a.get_field("labels"), b.get_field("labels"))


@pytest.mark.parametrize("arch,sample_step,noise,dtype", [("r101", 1, "device", "float16"), ("r101", 4, "device", "float16"), ("r101", 1, "host", "float16"),
                                                          ("swin", 1, "device", "float16"), ("r101", 4, "device", "float32")])
def test_call_graph_replay_is_bit_identical(arch, sample_step, noise, dtype):
    """The steady-state call of the reference's protocol (one batch per call, INPUT.LOOKAHEAD_BATCHES 1) replayed as one hipGraph
    (DiffusionDet._graphed_call) against the same calls launched kernel by kernel: two videos of different lengths (the second
    one re-uses the graph captured during the first, with another global memory; ragged tails run the ordinary way), every
    detection bit for bit.  The graphed run must actually have replayed (calls 3.. of each video's full batches).  dtype float32: the
    same with the fp32 path's launches (csrc/f32.hip) in the capture."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    lens = [44, 29] if arch == "r101" else [22, 14]
    outs, replays = {}, {}
    for graphs in (False, True):
        if arch == "r101":
            cfg, model = _build(sample_step, (1, 1, 2, 1), "trained_like", dtype=dtype)
        else:
            cfg = get_cfg("configs/vid_Swin_B_DiffusionVID.yaml", ["DTYPE", dtype], "configs/BASE_RCNN_1gpu.yaml")
            cfg.MODEL.SWIN.CONFIG_OVERRIDE = dict(embed_dim=64, depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), window=7)
            cfg.freeze()
            model = _weights(build_detection_model(cfg), "trained_like").to("cuda").eval()
        model.noise_fn = synthetic.DeviceNoise() if noise == "device" else synthetic.noise_fn
        model.use_call_graph = graphs
        ds = SyntheticVIDDataset(lens, cfg, height=250, width=380, device="cuda", smooth=True)
        res = []
        with torch.no_grad():
            for idx in range(len(ds)):
                res += model(ds[idx][0])          # device tensors kept across calls: a replay must not overwrite what an earlier call returned
        assert len(res) == sum(lens)
        res = [r.to(torch.device("cpu")) for r in res]
        outs[graphs], replays[graphs] = res, model.graph_replays
        del model, ds
        torch.cuda.empty_cache()
    ib = 8 if arch == "r101" else 4
    full = sum(n // ib for n in lens)                       # calls that carry a full batch
    assert replays[False] == 0 and replays[True] >= full - len(lens) - 1, replays          # all but each video's first call and the eager steady call
    for f, (a, b) in enumerate(zip(outs[False], outs[True])):
        assert len(a) == len(b) and len(a) > 0, f
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores")) and \
            torch.equal(a.get_field("labels"), b.get_field("labels")), f"frame {f} differs between graph replay and kernel-by-kernel launches"


@pytest.mark.parametrize("sample_step", [1, 4])
def test_streaming_call_graph_replay_is_bit_identical(sample_step):
    """The steady-state call of the streaming mode (INFER_BATCH 1, one new global frame per call, both memories merged and pruned back
    on every call) replayed as one hipGraph against the same calls launched kernel by kernel: two videos (the second re-uses the first
    one's graph with a memory that started over), every detection and the final memories bit for bit.  The memory lives in the graph's
    static buffers from replay to replay and is brought up to date after the eager calls at a video's start."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    lens = [14, 9]
    outs, replays, mems = {}, {}, {}
    for graphs in (False, True):
        cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml",
                      ["DTYPE", "float16", "INPUT.INFER_BATCH", 1, "MODEL.VID.MEGA.MAX_OFFSET", 0, "MODEL.VID.MEGA.MIN_OFFSET", 0,
                       "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 1, "MODEL.VID.MEGA.KEY_FRAME_LOCATION", 0,
                       "MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST", False, "MODEL.DiffusionDet.SAMPLE_STEP", sample_step], "configs/BASE_RCNN_1gpu.yaml")
        cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
        cfg.freeze()
        model = _weights(build_detection_model(cfg), "trained_like").to("cuda").eval()
        model.noise_fn = synthetic.DeviceNoise()
        model.use_call_graph = model.use_stream_graph = graphs          # (the streaming graph is opt-in: bit-identical, not faster)
        ds = SyntheticVIDDataset(lens, cfg, height=120, width=200, device="cuda", smooth=True)
        res = []
        with torch.no_grad():
            for idx in range(len(ds)):
                res += model(ds[idx][0])
        assert len(res) == sum(lens)
        outs[graphs] = [r.to(torch.device("cpu")) for r in res]
        replays[graphs] = model.graph_replays
        mems[graphs] = [m.clone().cpu() for m in model.head.proposal_feats_global]
        del model, ds
        torch.cuda.empty_cache()
    # per video: call 0 resets, call 1 is the eager steady call (first video only: the second finds the graph), the rest replay
    assert replays[False] == 0 and replays[True] >= sum(lens) - len(lens) - 2, replays
    for f, (a, b) in enumerate(zip(outs[False], outs[True])):
        assert len(a) == len(b) and len(a) > 0, f
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores")) and \
            torch.equal(a.get_field("labels"), b.get_field("labels")), f"frame {f} differs between graph replay and kernel-by-kernel launches"
    for a, b in zip(mems[False], mems[True]):
        assert torch.equal(a, b), "the memories of the two runs parted"


def test_build_then_smoke_in_one_process():
    """`__graft_entry__.build(); smoke()` as ONE process (README quick start; how a driver may chain them): build() dlopens the library
    before anything imported torch, and torch brings its own copy of the HIP runtime -- loaded in that order the library's copy saw no
    device ("no HIP device available", round 5) while either call alone worked.  `_lib.load()` imports torch first."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build(); g.smoke()"], cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "smoke ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


def test_call_graph_dropped_when_the_workspace_moves():
    """A captured call holds raw addresses inside the engine's workspace, and the workspace is re-allocated when it grows (a VID-val
    run mixes 4:3 and 16:9 videos): small video (captures), larger video (grows the workspace, captures its own shape), small
    video again -- whose key finds the FIRST graph unless graphs are dropped with the workspace they point into
    (dvid_workspace_generation).  Graphs on against graphs off, every detection bit for bit; the third video must
    have replayed (a re-captured graph), and the detector must have seen the generation change."""
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    sizes = [(250, 380), (330, 500), (250, 380)]
    outs, replays, gens = {}, {}, {}
    for graphs in (False, True):
        cfg, model = _build(1, (1, 1, 2, 1), "trained_like")
        model.noise_fn = synthetic.DeviceNoise()
        model.use_call_graph = graphs
        res, per_video, seen = [], [], set()
        with torch.no_grad():
            for v, (hh, ww) in enumerate(sizes):
                ds = SyntheticVIDDataset([36], cfg, height=hh, width=ww, device="cuda", smooth=True, video_base=v)
                before = model.graph_replays
                for idx in range(len(ds)):
                    res += [r.to(torch.device("cpu")) for r in model(ds[idx][0])]
                    seen.add(model._get_engine().workspace_generation())
                per_video.append(model.graph_replays - before)
        outs[graphs], replays[graphs], gens[graphs] = res, per_video, seen
        del model
        torch.cuda.empty_cache()
    assert replays[False] == [0, 0, 0]
    assert len(gens[True]) >= 2, "the larger video did not move the workspace: the test does not exercise what it is for"
    assert all(r >= 1 for r in replays[True]), replays          # the third video replays a graph captured AFTER the move
    for f, (a, b) in enumerate(zip(outs[False], outs[True])):
        assert len(a) == len(b) and len(a) > 0, f
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores")) and \
            torch.equal(a.get_field("labels"), b.get_field("labels")), f"frame {f} differs between graph replay and kernel-by-kernel launches"


def _x4_free_running_once(cfg, model, sd, blocks, video_base, L, H0, W0, with_policy=True):
    """one x4 video through the GPU path, the fp32 CPU oracle and the CPU oracle under the fp16 storage policy (oracle/precision.py: fp16
    weights and stored activations, fp32 accumulation -- no HIP kernel involved) -> the pairwise figures"""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.structures.bounding_box import BoxList
    from diffusionvid_amd.utils import synthetic
    from oracle import precision
    ds = SyntheticVIDDataset([L], cfg, height=H0, width=W0, device="cuda", smooth=True, video_base=video_base)
    model.noise_fn = synthetic.noise_fn
    images, oitem, ids = _oracle_items(ds, 0)
    torch.set_num_threads(min(32, torch.get_num_threads()))

    def oracle_run(policy):
        ocfg = odet.DetCfg(sample_step=4, infer_batch=L, all_frame_interval=L, **({} if blocks is None else {"blocks": blocks}))
        ocfg.head.sampling_timesteps = 4
        o = odet.OracleDiffusionDet(sd, ocfg, synthetic.noise_fn)
        with torch.no_grad():
            if policy:
                with precision.use("fp16"):
                    return o.forward(oitem)
            return o.forward(oitem)
    with torch.no_grad():
        got = model(images)
    ref32 = oracle_run(False)
    size = (W0, H0)
    if not with_policy:          # DTYPE float32: the GPU path against the fp32 oracle alone
        ap_gpu, n_obj = _ap50_on_objects(ref32, got, size)
        return {"m_gpu": [_match_rate(r, g) for r, g in zip(ref32, got)], "ap_gpu": ap_gpu, "n_obj": n_obj, "ap_all_gpu": _ap50_vs_oracle(ref32, got, size)}
    ref16 = oracle_run(True)

    def as_boxlists(ref):
        out = []
        for r in ref:
            bl = BoxList(torch.as_tensor(r["boxes"], dtype=torch.float32).reshape(-1, 4), size)
            bl.add_field("scores", torch.as_tensor(r["scores"], dtype=torch.float32).reshape(-1))
            bl.add_field("labels", torch.as_tensor(r["labels"], dtype=torch.int64).reshape(-1))
            out.append(bl)
        return out
    pol = as_boxlists(ref16)
    ap_gpu, n_obj = _ap50_on_objects(ref32, got, size)
    ap_pol, _ = _ap50_on_objects(ref32, pol, size)
    return {"m_gpu": [_match_rate(r, g) for r, g in zip(ref32, got)], "m_pol": [_match_rate(r, g) for r, g in zip(ref32, pol)],
            "m_gp": [_match_rate(r, g) for r, g in zip(ref16, got)], "ap_gpu": ap_gpu, "ap_pol": ap_pol, "n_obj": n_obj,
            "ap_all_gpu": _ap50_vs_oracle(ref32, got, size), "ap_all_pol": _ap50_vs_oracle(ref32, pol, size)}


@pytest.mark.skipif(os.environ.get("DVID_X4_SINGLE_VIDEO", "0") != "1", reason="superseded by test_x4_free_running_statistics (eight videos, the same three-way comparison); "
                    "DVID_X4_SINGLE_VIDEO=1 runs it on BASELINE's exact call (8 local + 24 global frames, 130 s): profiles/r05c_gpu_pytest.log holds its last run")
@pytest.mark.parametrize("full", [True])          # (the reduced size shows no divergence at all: 95 objects, matches 0.98-1.00 on every pair; profiles/r04_parity_report_tail.txt)
def test_x4_free_running_divergence_belongs_to_the_precision_policy(full):
    """x4 with real renewals (trained-like scores): one keep decision that flips at the 0.5 threshold re-draws every later slot of
    its frame (diffusion_det.py:559-572), so two evaluations that differ by rounding part ways after the first flip -- the
    full-size x4 run agrees with the fp32 oracle on only 0.33-0.96 of a frame's detections (TRAINED_LIKE above).  Is that the
    kernels' doing?  The same video through the CPU oracle under the fp16 STORAGE POLICY of the path (oracle/precision.py: fp16
    weights and stored activations, fp32 accumulation -- no HIP kernel involved) diverges from the fp32 oracle the same way:
    the GPU path must be no further from the fp32 oracle than that policy oracle is (match rate and AP50 over the fp32
    oracle's objects, margin 0.1), and the three pairwise figures are printed.  One video at BASELINE's exact configuration (8 local +
    24 global frames); test_x4_free_running_statistics below is the same comparison over eight videos with the margin the sample supports."""
    blocks = None if full else (1, 1, 2, 1)          # full: R101 (3, 4, 23, 3) at 1000 x 600, the configuration of TRAINED_LIKE's x4 line
    cfg, model = _build(4, blocks, "trained_like")
    L, H0, W0 = (8, 600, 1000) if full else (8, 250, 380)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    r = _x4_free_running_once(cfg, model, sd, blocks, 0, L, H0, W0)
    line = (f"[x4 free-running{' full size' if full else ''}, trained-like scores, {r['n_obj']} fp32-oracle objects] per-frame match with the fp32 oracle: GPU {['%.2f' % v for v in r['m_gpu']]}, "
            f"fp16-policy oracle {['%.2f' % v for v in r['m_pol']]}; GPU vs fp16-policy oracle {['%.2f' % v for v in r['m_gp']]}; AP50 over the fp32 oracle's objects: "
            f"GPU {r['ap_gpu']:.4f}, fp16-policy oracle {r['ap_pol']:.4f}; AP50 over all its detections: GPU {r['ap_all_gpu']:.4f}, fp16-policy oracle {r['ap_all_pol']:.4f}")
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")
    assert r["n_obj"] >= 4
    assert float(np.mean(r["m_gpu"])) >= float(np.mean(r["m_pol"])) - 0.1 and r["ap_gpu"] >= r["ap_pol"] - 0.1 and r["ap_all_gpu"] >= r["ap_all_pol"] - 0.1, line


X4_STAT_VIDEOS = int(os.environ.get("DVID_X4_STAT_VIDEOS", "8"))


def test_x4_free_running_statistics():
    """The x4 end-to-end gate (round 5; the free-running x4 figures were reported, not gated, until round 4).  A free-running x4 run is
    chaotic for ANY two evaluations that differ by rounding (see the test above), so a single video says little: eight videos (other
    frames, other draws) at full depth and resolution -- R101 (3, 4, 23, 3), 1000 x 600, 300 boxes, 4 DDIM steps, trained-like scores;
    4 local + 4 global frames per video so that the two CPU oracles finish in ~25 s per video (the renewal mechanism does not depend on
    the memory's size; INFER_BATCH 4 on both sides: the draws are keyed by (split, image)) -- each through the GPU path, the fp32 oracle and
    the fp16-policy oracle.  Gate, on the means over the videos: AP50 of the GPU path over the fp32 oracle's objects (its detections with
    score >= 0.5) >= that of the policy oracle - 0.07, and the mean per-frame match rate >= the policy oracle's - 0.07.  The margin is two
    standard errors of the paired mean difference, not the 0.02 the round-4 review suggested: per video AP50 has a standard deviation of
    0.10 on either side and the paired differences (GPU - policy) one of 0.098, i.e. 0.035 on the mean of eight -- measured (profiles/
    r05h_x4_statistics.txt): GPU 0.7432 vs policy 0.7563 (difference -0.013 = 0.4 standard errors), match 0.550 vs 0.553 over 5766 objects.
    tools/diag_x4_divergence.py shows the same thing stage by stage on one video: extraction logits, memory, step-0 logits and step-0 keep
    decisions of the GPU path are as far from the fp32 oracle as the policy oracle's (1-2 flipped keep decisions per frame each), and from
    step 1 on both have parted from it alike (profiles/r05g_x4_divergence.txt)."""
    cfg, model = _build(4, None, "trained_like", extra=["MODEL.VID.MEGA.GLOBAL.SIZE", 4, "INPUT.INFER_BATCH", 4, "MODEL.VID.MEGA.MAX_OFFSET", 3,
                                                         "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 4])          # batches of 4 on both sides: the draws are keyed by (split, image)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    rows = []
    for v in range(X4_STAT_VIDEOS):
        r = _x4_free_running_once(cfg, model, sd, None, v, 4, 600, 1000)
        rows.append(r)
        line = (f"[x4 statistics, video {v}] {r['n_obj']} objects; AP50 over the fp32 oracle's objects: GPU {r['ap_gpu']:.4f}, fp16-policy oracle {r['ap_pol']:.4f}; "
                f"mean match with the fp32 oracle: GPU {np.mean(r['m_gpu']):.3f}, policy {np.mean(r['m_pol']):.3f}; GPU vs policy {np.mean(r['m_gp']):.3f}")
        print(line)
        with open(_report_path(), "a") as f:
            f.write(line + "\n")
    ap_gpu, ap_pol = float(np.mean([r["ap_gpu"] for r in rows])), float(np.mean([r["ap_pol"] for r in rows]))
    m_gpu, m_pol = float(np.mean([np.mean(r["m_gpu"]) for r in rows])), float(np.mean([np.mean(r["m_pol"]) for r in rows]))
    n_obj = sum(r["n_obj"] for r in rows)
    line = (f"[x4 statistics, {len(rows)} videos, {n_obj} objects] mean AP50 over the fp32 oracle's objects: GPU {ap_gpu:.4f} (sd {np.std([r['ap_gpu'] for r in rows]):.3f}), "
            f"fp16-policy oracle {ap_pol:.4f} (sd {np.std([r['ap_pol'] for r in rows]):.3f}); mean match: GPU {m_gpu:.3f}, policy {m_pol:.3f}")
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")
    assert n_obj >= 100
    assert ap_gpu >= ap_pol - 0.07 and m_gpu >= m_pol - 0.07, line


def test_x4_free_running_statistics_float32():
    """The same free-running x4 videos (the first four of the eight) with `DTYPE float32` (round 6; csrc/f32.hip), against the fp32 oracle alone: with fp32 storage
    and fp32 products the two evaluations differ by summation order only (~1e-5 in the logits), so a keep decision flips only when a
    score sits within ~3e-6 of 0.5 -- the chaos that separates the fp16 path (and the fp16-policy CPU oracle) from the fp32 run by 25
    AP50 points does not start.  Gate (the round-5 review's): mean AP50 of the GPU detections over the fp32 oracle's objects >= 0.99,
    and the mean per-frame match rate >= 0.95."""
    cfg, model = _build(4, None, "trained_like", extra=["MODEL.VID.MEGA.GLOBAL.SIZE", 4, "INPUT.INFER_BATCH", 4, "MODEL.VID.MEGA.MAX_OFFSET", 3,
                                                         "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 4], dtype="float32")
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    rows = []
    for v in range(max(1, X4_STAT_VIDEOS // 2)):          # four of the eight videos keep the GPU suite near twenty minutes (all eight: profiles/r06b_f32_parity_report.txt, 5766 objects, AP50 1.0000)
        r = _x4_free_running_once(cfg, model, sd, None, v, 4, 600, 1000, with_policy=False)
        rows.append(r)
        line = (f"[x4 statistics, DTYPE float32, video {v}] {r['n_obj']} objects; AP50 over the fp32 oracle's objects: GPU {r['ap_gpu']:.4f}; over all its "
                f"detections {r['ap_all_gpu']:.4f}; per-frame match {['%.2f' % m for m in r['m_gpu']]}")
        print(line)
        with open(_report_path(), "a") as f:
            f.write(line + "\n")
    ap_gpu = float(np.mean([r["ap_gpu"] for r in rows]))
    m_gpu = float(np.mean([np.mean(r["m_gpu"]) for r in rows]))
    n_obj = sum(r["n_obj"] for r in rows)
    line = (f"[x4 statistics, DTYPE float32, {len(rows)} videos, {n_obj} objects] mean AP50 over the fp32 oracle's objects: GPU {ap_gpu:.4f} "
            f"(min {min(r['ap_gpu'] for r in rows):.4f}); mean match {m_gpu:.3f}")
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")
    assert n_obj >= 100
    assert ap_gpu >= 0.99 and m_gpu >= 0.95, line


def test_call_graph_projects_an_adopted_memory():
    """A captured steady-state call reads the memory's K / V projections from the engine's buffers, and the projection is not part
    of the capture: a memory that never went through an eager final stage -- adopted from another rank
    (engine.compute_on_video_sharded), or swapped by a caller -- must be projected before the replay.  After a video that left its
    graph behind, another memory is adopted and the next batch runs as a replay and, for comparison, kernel by kernel."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    cfg, model = _build(1, (1, 1, 1, 1), "trained_like")
    model.noise_fn = synthetic.DeviceNoise()
    ds = SyntheticVIDDataset([40], cfg, height=120, width=200, device="cuda", smooth=True)
    with torch.no_grad():
        for idx in range(40):
            model(ds[idx][0])
    assert model.graph_replays >= 2
    g = torch.Generator().manual_seed(3)
    other = [torch.randn(900, 256, generator=g).cuda(), torch.randn(150, 256, generator=g).cuda()]
    outs = {}
    for graphs in (True, False):
        model.use_call_graph = graphs
        before = model.graph_replays
        model.adopt_video_memory([m.clone() for m in other])
        res = []
        with torch.no_grad():
            for idx in range(1, 17):                      # calls 1-7 queue frames, call 8 and call 16 each finish a batch
                res += model(ds[idx][0])
        assert len(res) == 16 and (model.graph_replays - before == (2 if graphs else 0))
        outs[graphs] = [r.to(torch.device("cpu")) for r in res]
    for a, b in zip(outs[True], outs[False]):
        assert len(a) == len(b) > 0 and torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))


def test_fresh_model_adopts_a_memory_and_runs_its_first_batch():
    """A process that has never run its model -- rank > 0 of engine.compute_on_video_sharded with the reference's protocol (look-ahead 1)
    -- adopts the video's memory (`adopt_video_memory` does not build the engine), queues seven calls and reaches its first full batch
    with `_engine` still None.  That call qualifies for the hipGraph path, whose key read `self._engine.chains` (AttributeError on None,
    ADVICE r05): the key is now built from `_get_engine()`.  Same after a device move dropped the engine.  The detections equal those of
    a model that had run before adopting the same memory."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    g = torch.Generator().manual_seed(5)
    memory = [torch.randn(900, 256, generator=g).cuda(), torch.randn(150, 256, generator=g).cuda()]

    def run(warm):
        cfg, model = _build(1, (1, 1, 1, 1), "trained_like")
        model.noise_fn = synthetic.DeviceNoise()
        ds = SyntheticVIDDataset([40], cfg, height=120, width=200, device="cuda", smooth=True)
        if warm:
            with torch.no_grad():
                for idx in range(16):
                    model(ds[idx][0])
        else:
            assert model._engine is None
        model.adopt_video_memory([m.clone() for m in memory])
        res = []
        with torch.no_grad():
            for idx in range(1, 25):          # calls 1-7 queue frames; calls 8, 16, 24 each finish a batch (eager, eager, captured / replayed)
                res += model(ds[idx][0])
        assert len(res) == 24
        return [r.to(torch.device("cpu")) for r in res]
    fresh, warm = run(False), run(True)
    for a, b in zip(fresh, warm):
        assert len(a) == len(b) > 0 and torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
