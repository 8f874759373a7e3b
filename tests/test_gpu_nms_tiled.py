"""The tiled NMS (csrc/postproc.hip: nms_tiled_sort / _mask / _sweep kernels): the post-processing of frames with more candidates than
one workgroup's LDS holds -- more than 997, up to ops.NMS_MAX_CANDIDATES = 4096 -- which is what SAMPLE_STEP 8, or 500 boxes at x4, or
1000 boxes at x1 need.

Kernel level (exact, as all index work here: same kept set, order, labels and clipped boxes; scores to 2e-7) against oracle.postproc,
which is generic in the number of candidates; the tiled form against the single-workgroup kernel bit for bit where both run; the
refusal above the limit.  Detector level: SAMPLE_STEP 8 against the ensemble oracle on the GPU's own per-step outputs (exact), against
the fp32 CPU oracle end to end (the project's float32 gate), and look-ahead 1 against 3 where a group's frames are chunked."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detector as odet, postproc as opost  # noqa: E402

W, H, C = 1000.0, 600.0, 30
SIZE = (1000, 600)


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


# the inputs of tests/test_gpu_kernels.py's post-processing tests; the boxes' negative coordinates are wanted (clip, cross-class overlap)
def _separated_logits(g, n, M, C):
    """Logits whose sigmoid values are pairwise distinct by a wide margin (no rounding-level ties)."""
    vals = torch.linspace(-9.0, 3.0, n * M * C)
    perm = torch.randperm(n * M * C, generator=g)
    return vals[perm].view(n, M, C)


def _cluster_boxes(g, n, M, W=1000.0, H=600.0):
    ctr = torch.rand(n, 12, 2, generator=g) * torch.tensor([W, H])
    which = torch.randint(0, 12, (n, M), generator=g)
    c = torch.gather(ctr, 1, which[..., None].expand(-1, -1, 2)) + torch.randn(n, M, 2, generator=g) * 8
    wh = torch.rand(n, M, 2, generator=g) * 120 + 30
    return torch.cat([c - wh / 2, c + wh / 2], dim=-1)


SHAPES = {  # name: (sets, frames, boxes)
    "x8_300": (7, 2, 300),          # 2100 candidates: SAMPLE_STEP 8 with the shipped 300 boxes
    "x4_350": (3, 2, 350),          # 1050
    "x1_1000": (1, 2, 1000),        # 1000 in one set: 416 bytes more LDS than the single-workgroup kernel may have
    "x6_205": (5, 2, 205),          # 1025: the smallest count above 1024, no multiple of 64, sorted in 2048 padded keys
    "x5_1024": (4, 2, 1024),        # 4096: the limit, all 64 words of every mask row full
}
_inputs_cache = {}


def _inputs(name):
    """(logits [S, n, M, C], boxes [S, n, M, 4], per-frame oracle candidates (boxes, scores, labels) in set-major order), computed once"""
    if name not in _inputs_cache:
        S, n, M = SHAPES[name]
        g = torch.Generator().manual_seed(1000 + S * 31 + M)
        logits = _separated_logits(g, S * n, M, C).view(S, n, M, C)
        boxes = _cluster_boxes(g, S * n, M).view(S, n, M, 4)
        cands = [[opost.topk_candidates(logits[s, b], boxes[s, b], C)[:3] for b in range(n)] for s in range(S)]
        _inputs_cache[name] = (logits, boxes, cands)
    return _inputs_cache[name]


def _assert_frames_equal(out, ref, cap):
    """GPU outputs against the oracle's list of dict(boxes, scores, labels): exact but for the scores; the tail behind the count is zero"""
    ob, osc, ol, oc = (t.cpu().numpy() for t in out)
    for b, r in enumerate(ref):
        k = int(oc[b])
        assert k == len(r["scores"]), f"frame {b}: kept {k} vs {len(r['scores'])}"
        np.testing.assert_array_equal(ol[b, :k], r["labels"])
        np.testing.assert_array_equal(ob[b, :k], r["boxes"])
        np.testing.assert_allclose(osc[b, :k], r["scores"], rtol=0, atol=2e-7)
        assert ob.shape[1] == cap and not ob[b, k:].any() and not osc[b, k:].any() and not ol[b, k:].any()


@pytest.mark.parametrize("name", list(SHAPES))
def test_postproc_beyond_one_workgroup_exact(dv, name):
    """dvid_postproc_topk_nms on the shapes its single-workgroup NMS refuses (all but the last raised DvidError before the tiled form)"""
    S, n, M = SHAPES[name]
    logits, boxes, cands = _inputs(name)
    ref = opost.inference_ensemble(cands, SIZE)
    out = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), W, H)
    kept = [int(k) for k in out[3].cpu()]
    print(f"[{name}] {S * M} candidates: kept {kept} vs oracle {[len(r['scores']) for r in ref]}")
    _assert_frames_equal(out, ref, S * M)
    assert all(S * M / 2 < k < S * M for k in kept)          # suppression happened, and did not remove everything


def test_postproc_beyond_one_workgroup_without_nms(dv):
    """use_nms = False at 2100 candidates: every candidate comes back, in the stable merge order (score descending, position ascending)"""
    S, n, M = SHAPES["x8_300"]
    logits, boxes, cands = _inputs("x8_300")
    ref = []
    for r in opost.inference_ensemble(cands, SIZE, use_nms=False):          # the oracle leaves the un-suppressed list in set order
        order = np.argsort(-r["scores"], kind="stable")
        ref.append({k: v[order] for k, v in r.items()})
    out = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), W, H, use_nms=False)
    assert out[3].tolist() == [S * M] * n
    _assert_frames_equal(out, ref, S * M)


def _nms_ref(boxes, scores, labels, iou):
    """oracle of ops.nms_frames_tiled: per frame batched_nms on the raw candidates, then the clip"""
    ref = []
    for b, s, l in zip(boxes.numpy(), scores.numpy(), labels.numpy()):
        keep = opost.batched_nms(b, s, l, iou)
        ref.append({"boxes": opost.clip_to_image(b[keep], SIZE), "scores": s[keep], "labels": l[keep], "keep": keep})
    return ref


def _tiled(dv, boxes, scores, labels, iou=0.5, use_nms=True):
    return dv.nms_frames_tiled(boxes.cuda(), scores.cuda(), labels.to(torch.int32).cuda(), W, H, iou, use_nms)


CROSS_BOXES = torch.tensor([[100.0, 100.0, 400.0, 400.0], [-250.0, -250.0, 50.0, 50.0]])          # labels 1 and 2, scores 0.9 and 0.8


@pytest.mark.parametrize("iou,kept", [(0.5, [0]), (0.55, [0, 1])])
def test_cross_class_pair_is_tested(dv, iou, kept):
    """torchvision's coordinate trick moves class k by k * (max_coord + 1) = 401 k here: [100, 400] + 401 and [-250, 50] + 802 overlap with
    IoU 62001 / 117999 = 0.525, so the box of class 2 falls to the box of class 1 at threshold 0.5 and stays at 0.55.  No pair of
    different classes may be skipped.  On its own (n = 2) and among 1098 far-away boxes that keep max_coord at 400, the pair ten mask words apart."""
    scores, labels = torch.tensor([[0.9, 0.8]]), torch.tensor([[1, 2]])
    ref = _nms_ref(CROSS_BOXES[None], scores, labels, iou)
    assert ref[0]["keep"].tolist() == kept
    out = _tiled(dv, CROSS_BOXES[None], scores, labels, iou)
    assert int(out[3][0]) == len(kept)
    _assert_frames_equal(out, ref, 2)
    # padded to 1100: small boxes of one class far out at negative coordinates, none overlapping another or the pair
    n, a, b = 1100, 3, 700
    k = torch.arange(n, dtype=torch.float32)
    boxes = torch.stack([-1000.0 - 50.0 * k, torch.full((n,), -5000.0), -990.0 - 50.0 * k, torch.full((n,), -4990.0)], dim=1)
    scores = 0.95 - 0.00016 * k
    labels = torch.full((n,), 3)
    boxes[a], scores[a], labels[a] = CROSS_BOXES[0], 0.9, 1
    boxes[b], scores[b], labels[b] = CROSS_BOXES[1], 0.8, 2
    ref = _nms_ref(boxes[None], scores[None], labels[None], iou)
    assert a in ref[0]["keep"] and (b in ref[0]["keep"]) == (1 in kept) and len(ref[0]["keep"]) == n - 2 + len(kept)
    out = _tiled(dv, boxes[None], scores[None], labels[None], iou)
    _assert_frames_equal(out, ref, n)


def test_tied_scores_resolve_by_position(dv):
    """1100 candidates with 8 distinct score values: the order among equal scores is the position, ascending (the oracle's stable sort)"""
    g = torch.Generator().manual_seed(77)
    n = 1100
    boxes = _cluster_boxes(g, 2, n)
    scores = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2])[torch.randint(0, 8, (2, n), generator=g)]
    labels = torch.randint(1, C + 1, (2, n), generator=g)
    ref = _nms_ref(boxes, scores, labels, 0.5)
    out = _tiled(dv, boxes, scores, labels)
    _assert_frames_equal(out, ref, n)
    assert all(n / 2 < len(r["keep"]) < n for r in ref)
    ref = [{k: v[np.argsort(-r["scores"], kind="stable")] for k, v in r.items()}
           for r in ({"boxes": opost.clip_to_image(b, SIZE), "scores": s, "labels": l} for b, s, l in zip(boxes.numpy(), scores.numpy(), labels.numpy()))]
    _assert_frames_equal(_tiled(dv, boxes, scores, labels, use_nms=False), ref, n)


def _gpu_candidates(dv, logits, boxes):
    """The candidate lists dvid_postproc_topk_nms hands its NMS -- [n, S * M] in set-major order, each set by descending score -- with the
    GPU's own scores (its sigmoid may differ from the CPU's in the last bit): scores and labels from a run without NMS, put back from the
    merged order into the candidate order, which the oracle's stable sort gives."""
    S, n, M, _ = logits.shape
    _, osc, ol, _ = (t.cpu() for t in dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), W, H, use_nms=False))
    cb, cs, cl = torch.empty(n, S * M, 4), torch.empty(n, S * M), torch.empty(n, S * M, dtype=torch.int64)
    for b in range(n):
        per_set = [opost.topk_candidates(logits[s, b], boxes[s, b], C)[:3] for s in range(S)]
        bx, sc, lb = (np.concatenate([c[i] for c in per_set]) for i in range(3))
        order = np.argsort(-sc, kind="stable")
        np.testing.assert_array_equal(ol[b].numpy(), lb[order])
        np.testing.assert_allclose(osc[b].numpy(), sc[order], rtol=0, atol=2e-7)
        cb[b], cl[b] = torch.from_numpy(bx), torch.from_numpy(lb)
        cs[b, torch.from_numpy(order)] = osc[b]
    return cb, cs, cl


@pytest.mark.parametrize("S,M", [(3, 300), (1, 64), (1, 65), (1, 997), (4, 256)])
def test_tiled_equals_single_workgroup_kernel_bitwise(dv, S, M):
    """The same candidates through dvid_nms_frames_tiled and through dvid_postproc_topk_nms's NMS: 900 (test_postproc_ensemble_exact's shape),
    64, 65 and 997 candidates run nms_frame_kernel there (997 is the most its LDS holds); 1024 already the tiled form.  All four outputs
    are equal over the whole out_cap, the zero-filled tail included."""
    g = torch.Generator().manual_seed(12 + S * M)
    n = 2
    logits = _separated_logits(g, S * n, M, C).view(S, n, M, C)
    boxes = _cluster_boxes(g, S * n, M).view(S, n, M, 4)
    cb, cs, cl = _gpu_candidates(dv, logits, boxes)
    want = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), W, H)
    got = _tiled(dv, cb, cs, cl)
    for name, a, b in zip(("boxes", "scores", "labels", "counts"), got, want):
        assert torch.equal(a, b), f"{S * M} candidates: {name} differ"
    assert all(0 < int(k) <= S * M for k in want[3])


def test_more_than_the_limit_is_refused(dv):
    """4097 candidates (17 sets of 241): DvidError that names the configuration keys and the limit; nothing is launched"""
    from diffusionvid_amd._lib import DvidError
    assert dv.NMS_MAX_CANDIDATES == 4096
    logits, boxes = torch.zeros(17, 1, 241, 2).cuda(), torch.zeros(17, 1, 241, 4).cuda()
    with pytest.raises(DvidError, match=r"(?s)4097.*4096.*SAMPLE_STEP.*NUM_PROPOSALS"):
        dv.postproc_topk_nms(logits, boxes, W, H)
    with pytest.raises(DvidError, match="4096"):
        dv.nms_frames_tiled(torch.zeros(1, 4097, 4).cuda(), torch.zeros(1, 4097).cuda(), torch.ones(1, 4097, dtype=torch.int32).cuda(), W, H)


# ---- detector level: the reduced R101 (1, 1, 1, 1), 250 x 380 frames, as tests/test_gpu_e2e.py's test_other_num_proposals ----------------
def _detector(dtype, sample_step, num_proposals, lookahead=1):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", dtype, "MODEL.DiffusionDet.SAMPLE_STEP", sample_step,
                                                          "MODEL.DiffusionDet.NUM_PROPOSALS", num_proposals, "INPUT.LOOKAHEAD_BATCHES", lookahead],
                  "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    return cfg, model


def test_x8_detections_are_the_ensemble_of_the_steps(dv):
    """SAMPLE_STEP 8 with 160 boxes (1120 candidates), float16: the returned detections are exactly what the CPU ensemble oracle makes of
    the GPU's own per-step logits and boxes (debug taps final_0 .. final_6; the eighth step never reaches the ensemble) -- the tiled NMS
    in the detector's sequencing, independent of the precision of the layers before it."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    cfg, model = _detector("float16", 8, 160)
    model.debug_taps = {}
    ds = SyntheticVIDDataset([8], cfg, height=250, width=380, device="cuda", smooth=True)
    with torch.no_grad():
        got = model(ds[0][0])
    assert len(got) == 8
    taps = [model.debug_taps[f"final_{s}"] for s in range(7)]
    cands = [[opost.topk_candidates(lg[b].float().cpu(), bx[b].float().cpu(), C)[:3] for b in range(8)] for lg, bx in taps]
    ref = opost.inference_ensemble(cands, got[0].size)
    print(f"[x8, 160 boxes] kept {[len(g) for g in got]} of 1120 vs ensemble oracle {[len(r['scores']) for r in ref]}")
    for g, r in zip(got, ref):
        assert len(g) == len(r["scores"])
        np.testing.assert_array_equal(g.get_field("labels").cpu().numpy(), r["labels"])
        np.testing.assert_array_equal(g.bbox.cpu().numpy(), r["boxes"])
        np.testing.assert_allclose(g.get_field("scores").cpu().numpy(), r["scores"], rtol=0, atol=2e-7)


def test_x8_float32_against_the_fp32_oracle(dv):
    """The same configuration with DTYPE float32, free running over its eight steps, against the fp32 CPU oracle: the project's float32
    gate (tests/test_gpu_e2e.py: TRAINED_LIKE_F32, test_x4_free_running_statistics_float32), per-frame match rate >= 0.95."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    from test_gpu_e2e import _match_rate, _oracle_items
    cfg, model = _detector("float32", 8, 160)
    ds = SyntheticVIDDataset([8], cfg, height=250, width=380, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = odet.DetCfg(blocks=(1, 1, 1, 1), sample_step=8, num_proposals=160)
    ocfg.head.sampling_timesteps = 8
    oracle = odet.OracleDiffusionDet(sd, ocfg, synthetic.noise_fn)
    images, oitem, _ = _oracle_items(ds, 0)
    with torch.no_grad():
        ref_out = oracle.forward(oitem)
        got_out = model(images)
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    print(f"[x8, 160 boxes, DTYPE float32] kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]}; match {['%.3f' % r for r in rates]}")
    assert len(got_out) == len(ref_out) == 8
    assert min(rates) >= 0.95


def test_lookahead_does_not_change_tiled_detections(dv):
    """x4 with 350 boxes (1050 candidates) on a 20-frame video: INPUT.LOOKAHEAD_BATCHES 1 against 3 -- the NMS of one batch (8 frames) per
    call against the whole video's frames in one call: bit-identical detections, so neither the frames per launch nor the scratch
    layout that depends on them reaches a result."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    outs = {}
    for la in (1, 3):
        cfg, model = _detector("float16", 4, 350, lookahead=la)
        ds = SyntheticVIDDataset([20], cfg, height=250, width=380, device="cuda", smooth=True)
        res = []
        with torch.no_grad():
            for idx in range(len(ds)):
                res += model(ds[idx][0])
        assert len(res) == 20 and all(len(r) > 0 for r in res)
        outs[la] = res
    same = [torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores")) and torch.equal(a.get_field("labels"), b.get_field("labels"))
            for a, b in zip(outs[1], outs[3])]
    print(f"[x4, 350 boxes] look-ahead 3 vs 1: {sum(same)}/20 frames bit-identical; kept {[len(r) for r in outs[1]]}")
    assert all(same)
