"""Class vocabularies above 64 (COCO 80, LVIS 1203; the limit is ops.MAX_CLASSES = 1280): the streaming candidate selection on its own
(csrc/postproc.hip: topk_stream_kernel through dvid_topk_candidates_stream), the same bits where the LDS forms also run, the wave-per-row
class maximum of topk_mask_kernel / ddim_renew_kernel (csrc/boxes.hip), and reduced models of 80 and 1203 classes end to end against
the CPU oracle.

Grid logits.  The stand-alone cases draw logits from integer multiples of 1/64 in [-8, 4]: equal logits give exactly equal scores
(ties are plentiful), unequal ones differ by at least 1.5 % of the score at -8 and 2.7e-4 at 4 -- thousands of ulps of the sigmoid --
so the order of the scores is the order of the logits however expf rounds, and the CPU reference is a stable sort by
(logit desc, flat index asc): exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT  # noqa: E402
from oracle import detector as odet  # noqa: E402
from test_gpu_e2e import _match_rate, _oracle_items  # noqa: E402

W, H = 1000.0, 600.0


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


def _grid(g, shape, lo=-512, hi=256):
    """integer multiples of 1/64 in [lo / 64, hi / 64]"""
    return torch.randint(lo, hi + 1, shape, generator=g).float() / 64.0


def _inside_boxes(g, *lead):
    """boxes inside the W x H image (clipping leaves them alone), pairwise distinct with overwhelming probability"""
    p = torch.rand(*lead, 2, generator=g) * torch.tensor([W - 200.0, H - 200.0])
    return torch.cat([p, p + 1.0 + torch.rand(*lead, 2, generator=g) * 190.0], dim=-1)


def _ref_topk(logits, boxes):
    """logits [M, C], boxes [M, 4] -> (boxes [M, 4], scores [M], labels [M] int32, flat indices) by (logit desc, flat index asc)"""
    M, C = logits.shape
    flat = logits.flatten()
    order = torch.sort(flat, descending=True, stable=True).indices[:M]
    return boxes[order // C], torch.sigmoid(flat[order]), (order % C + 1).to(torch.int32), order


def _check_stream(dv, logits, boxes):
    """logits [S, n, M, C], boxes [S, n, M, 4] through ops.topk_candidates_stream against _ref_topk: labels and boxes exactly, scores
    within 1e-6 of torch.sigmoid, set s of frame f at columns [s M, (s + 1) M)"""
    S, n, M, C = logits.shape
    cb, cs, cl = (t.cpu() for t in dv.topk_candidates_stream(logits.cuda(), boxes.cuda()))
    assert cb.shape == (n, S * M, 4) and cs.shape == (n, S * M) and cl.shape == (n, S * M) and cl.dtype == torch.int32
    for s in range(S):
        for f in range(n):
            rb, rs, rl, _ = _ref_topk(logits[s, f], boxes[s, f])
            sl = slice(s * M, (s + 1) * M)
            assert torch.equal(cl[f, sl], rl), f"set {s} frame {f}: labels differ at {torch.nonzero(cl[f, sl] != rl).flatten()[:5].tolist()}"
            assert torch.equal(cb[f, sl], rb), f"set {s} frame {f}: boxes differ"
            assert (cs[f, sl] - rs).abs().max().item() <= 1e-6
            assert torch.all(cs[f, sl][:-1] >= cs[f, sl][1:])
    return cb, cs, cl


# (a) fewer keys than threads: most lanes and whole waves have an empty range; (b) nothing a power of two; (c) well past both LDS forms;
# (d) the class limit with M equal to its padded size
@pytest.mark.parametrize("M,C", [(3, 70), (37, 65), (100, 1203), (64, 1280)])
def test_stream_select_on_grid_logits(dv, M, C):
    g = torch.Generator().manual_seed(1000 + M * C)
    n = 2
    _check_stream(dv, _grid(g, (1, n, M, C)), _inside_boxes(g, 1, n, M))


def test_stream_select_all_logits_equal(dv):
    """(e) the whole selection is the equal-key path: flat indices 0 .. M - 1, that is box 0 with the labels 1 .. M"""
    g = torch.Generator().manual_seed(1)
    M, C = 50, 200
    logits = torch.full((1, 2, M, C), -1.25)
    boxes = _inside_boxes(g, 1, 2, M)
    cb, cs, cl = _check_stream(dv, logits, boxes)
    for f in range(2):
        assert torch.equal(cl[f], torch.arange(1, M + 1, dtype=torch.int32))
        assert torch.equal(cb[f], boxes[0, f, :1].expand(M, 4))


def test_stream_select_takes_one_of_many_equal_keys(dv):
    """(f) exactly M - 1 keys above a value that 500 others share: one of the 500 completes the M, the one with the smallest flat index"""
    g = torch.Generator().manual_seed(2)
    n, M, C = 2, 64, 300
    logits = _grid(g, (1, n, M, C), -512, -64)                     # everything else at or below -1
    want_last = []
    for f in range(n):
        pos = torch.randperm(M * C, generator=g)
        flat = logits[0, f].view(-1)
        flat[pos[:500]] = 0.0
        flat[pos[500:500 + M - 1]] = _grid(g, (M - 1,), 1, 256)     # M - 1 keys in (0, 4]
        want_last.append(int(pos[:500].min()))
    boxes = _inside_boxes(g, 1, n, M)
    cb, cs, cl = _check_stream(dv, logits, boxes)
    for f in range(n):
        assert cs[f, M - 1].item() == 0.5 and cs[f, M - 2].item() > 0.5
        assert int(cl[f, M - 1]) == want_last[f] % C + 1 and torch.equal(cb[f, M - 1], boxes[0, f, want_last[f] // C])


def test_stream_select_output_layout(dv):
    """(g) three sets, two frames: logits [S, n, M, C] -> [n, S * M]"""
    g = torch.Generator().manual_seed(3)
    S, n, M, C = 3, 2, 37, 65
    _check_stream(dv, _grid(g, (S, n, M, C)), _inside_boxes(g, S, n, M))


def test_stream_select_limits(dv):
    from diffusionvid_amd._lib import DvidError
    with pytest.raises(DvidError, match=r"1281 classes.*1280.*DVID_MAX_CLASSES"):
        dv.topk_candidates_stream(torch.zeros(1, 2, dv.MAX_CLASSES + 1).cuda(), torch.zeros(1, 2, 4).cuda())


@pytest.mark.parametrize("M,C", [(100, 30), (300, 30), (300, 64)])
def test_stream_select_gives_the_bits_of_the_lds_forms(dv, M, C):
    """Ordinary Gaussian logits where dvid_postproc_topk_nms selects with topk_select_kernel: its outputs with the NMS off are the
    candidates in the same order (boxes inside the image, so its clip changes nothing); all three arrays are equal bit for bit."""
    g = torch.Generator().manual_seed(500 + M + C)
    n = 3
    logits = torch.randn(n, M, C, generator=g) * 1.5 - 3.0
    boxes = _inside_boxes(g, n, M)
    ob, osc, ol, oc = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), W, H, use_nms=False)
    cb, cs, cl = dv.topk_candidates_stream(logits.cuda(), boxes.cuda())
    assert torch.all(oc == M)
    assert torch.equal(cs, osc) and torch.equal(cl, ol) and torch.equal(cb, ob)


def test_postproc_takes_the_stream_form_beyond_the_lds_forms(dv):
    """dvid_postproc_topk_nms at 100 x 1203 and 500 x 80, refused before (neither LDS form holds the keys): the candidates of the
    stream form, NMS off"""
    g = torch.Generator().manual_seed(4)
    for M, C in ((100, 1203), (500, 80)):
        logits, boxes = _grid(g, (2, M, C)), _inside_boxes(g, 2, M)
        ob, osc, ol, oc = dv.postproc_topk_nms(logits.cuda(), boxes.cuda(), W, H, use_nms=False)
        cb, cs, cl = dv.topk_candidates_stream(logits.cuda(), boxes.cuda())
        assert torch.all(oc == M) and torch.equal(cs, osc) and torch.equal(cl, ol) and torch.equal(cb, ob)
        for f in range(2):
            assert torch.equal(ol[f].cpu(), _ref_topk(logits[f], boxes[f])[2])


# ---- the class maximum of a box row ---------------------------------------------------------------------------------------------------

ROWMAX_N, ROWMAX_M, ROWMAX_D, ROWMAX_K1, ROWMAX_K2 = 2, 100, 8, 25, 10
# keep threshold between the grid points 0 and 1/64: a box is kept iff its largest logit is >= 1/64, however expf rounds
ROWMAX_THR = float(torch.sigmoid(torch.tensor(1.0 / 128.0)))
# DDIM coefficients of the step 749 -> 499 (any finite values do: they do not touch the decisions)
ROWMAX_COEF = dict(snr_scale=2.0, sqrt_recip_ac=2.6131, sqrt_recipm1_ac=2.4142, sqrt_ac_next=0.7071, coef_c=0.25, sigma=0.6614)


def rowmax_inputs(C, seed=7):
    """Grid logits [n, M, C] whose row maxima are multiples of 1/4 in [-3, 3] (25 values over 100 boxes: ties between boxes), each held by
    ONE column of the row -- the last, the first, 63, 64 (the second element of lane 0 in the wave-per-row form) for the first rows, a
    random one for the others -- and everything a kernel of either form reads beside them."""
    g = torch.Generator().manual_seed(seed + C)
    n, M = ROWMAX_N, ROWMAX_M
    top = torch.randint(-12, 13, (n, M, 1), generator=g).float() / 4.0
    logits = torch.minimum(_grid(g, (n, M, C)), top - 1.0 / 64.0)
    col = torch.randint(0, C, (n, M, 1), generator=g)
    for i, c in enumerate((C - 1, 0, min(63, C - 1), min(64, C - 1))):
        col[:, i, 0] = c
    logits.scatter_(2, col, top)
    return dict(logits=logits, feats=torch.randn(n * M, ROWMAX_D, generator=g), boxes=_inside_boxes(g, n, M),
                x_t=torch.randn(n, M, 4, generator=g) * 1.5, noise=torch.randn(n, M, 4, generator=g), fresh=torch.randn(n, M, 4, generator=g))


def rowmax_run(dv, x, logits=None):
    """ops.select_topk_features and ops.ddim_renew_step on rowmax_inputs (or on other logits beside the same tensors)"""
    lg = (x["logits"] if logits is None else logits).cuda()
    o1, o2 = dv.select_topk_features(lg, x["feats"].cuda(), ROWMAX_K1, ROWMAX_K2)
    c = ROWMAX_COEF
    xn = dv.ddim_renew_step(lg, x["boxes"].cuda(), x["x_t"].cuda(), x["noise"].cuda(), x["fresh"].cuda(), (W, H), c["snr_scale"], c["sqrt_recip_ac"],
                            c["sqrt_recipm1_ac"], c["sqrt_ac_next"], c["coef_c"], c["sigma"], ROWMAX_THR)
    return o1.cpu(), o2.cpu(), xn.cpu()


def _restate_select(logits, feats, k):
    """box_head.py:304-317: per frame the k boxes of largest class maximum, ranked by (max logit desc, index asc), in index order"""
    n, M, _ = logits.shape
    rows = []
    for f in range(n):
        order = torch.sort(logits[f].amax(-1), descending=True, stable=True).indices[:k]
        rows.append(feats[f * M + torch.sort(order).values])
    return torch.cat(rows)


def _restate_renew(x, thr):
    """diffusion_det.py:559-596 in the kernel's operation order: (keep mask, kept rows' values per frame)"""
    c = ROWMAX_COEF
    keep = torch.sigmoid(x["logits"].amax(-1)) > thr
    whwh = torch.tensor([W, H, W, H])
    nb = x["boxes"] / whwh
    xs = torch.stack([(nb[..., 0] + nb[..., 2]) / 2, (nb[..., 1] + nb[..., 3]) / 2, nb[..., 2] - nb[..., 0], nb[..., 3] - nb[..., 1]], -1)
    v = ((xs * 2 - 1) * c["snr_scale"]).clamp(-c["snr_scale"], c["snr_scale"])
    pn = (c["sqrt_recip_ac"] * x["x_t"] - v) / c["sqrt_recipm1_ac"]
    return keep, v * c["sqrt_ac_next"] + c["coef_c"] * pn           # + sigma * noise[slot], added per frame by the caller


@pytest.mark.parametrize("C", [65, 80, 1203])
def test_wide_row_maximum(dv, C):
    """topk_mask_kernel / ddim_renew_kernel above 64 classes (one wave per box row).  Everything the class maximum decides is compared
    exactly with the torch restatement: the selected feature rows (pure copies), the keep mask and the kept boxes' slots (through the
    refill rows, copied bit for bit behind them).  The kept rows' VALUES are fp32 arithmetic behind the decision, the same instructions
    in both forms: they are equal bit for bit to the same call on the [n, M, 1] row maxima, which takes the one-thread-per-row form, and
    within 1e-6 relative / 2e-6 absolute of the restatement (operation order of the kernel, fused multiply-adds aside), the bound of
    test_gpu_kernels.py::test_ddim_renew_step."""
    x = rowmax_inputs(C)
    o1, o2, xn = rowmax_run(dv, x)
    assert torch.equal(o1, _restate_select(x["logits"], x["feats"], ROWMAX_K1))
    assert torch.equal(o2, _restate_select(x["logits"], x["feats"], ROWMAX_K2))
    keep, part = _restate_renew(x, ROWMAX_THR)
    M = ROWMAX_M
    for f in range(ROWMAX_N):
        idx = torch.nonzero(keep[f]).flatten()
        k = len(idx)
        assert 20 < k < M - 20
        assert torch.equal(xn[f, k:], x["fresh"][f, :M - k]), f"frame {f}: refill rows differ (kept {k})"
        want = part[f, idx] + ROWMAX_COEF["sigma"] * x["noise"][f, :k]
        np.testing.assert_allclose(xn[f, :k].numpy(), want.numpy(), rtol=1e-6, atol=2e-6)
    n1, n2, nn = rowmax_run(dv, x, x["logits"].amax(-1, keepdim=True).contiguous())
    assert torch.equal(o1, n1) and torch.equal(o2, n2) and torch.equal(xn, nn)


@pytest.mark.parametrize("C", [30, 64])
def test_narrow_row_maximum_is_unchanged(dv, C):
    """Up to 64 classes the one-thread-per-row form runs (its ISA is the one of the kernels before the wide form):
    the same decisions, exactly, as the torch restatement -- selected rows, keep mask and slots through the refill rows -- and the kept
    rows' values bit for bit those of the call on the [n, M, 1] row maxima."""
    x = rowmax_inputs(C)
    o1, o2, xn = rowmax_run(dv, x)
    assert torch.equal(o1, _restate_select(x["logits"], x["feats"], ROWMAX_K1))
    assert torch.equal(o2, _restate_select(x["logits"], x["feats"], ROWMAX_K2))
    keep, _ = _restate_renew(x, ROWMAX_THR)
    for f in range(ROWMAX_N):
        k = int(keep[f].sum())
        assert torch.equal(xn[f, k:], x["fresh"][f, :ROWMAX_M - k]), f"frame {f}: refill rows differ (kept {k})"
    n1, n2, nn = rowmax_run(dv, x, x["logits"].amax(-1, keepdim=True).contiguous())
    assert torch.equal(o1, n1) and torch.equal(o2, n2) and torch.equal(xn, nn)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

BLOCKS = (1, 1, 1, 1)
E2E_H, E2E_W, E2E_L = 120, 180, 8
_ORACLE = {}


def _cfg(num_classes, sample_step, dtype):
    from diffusionvid_amd.config import get_cfg
    opts = ["DTYPE", dtype, "MODEL.DiffusionDet.NUM_CLASSES", num_classes, "MODEL.DiffusionDet.SAMPLE_STEP", sample_step]
    if sample_step > 1:
        opts += ["MODEL.DiffusionDet.NUM_PROPOSALS", 100]
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), opts, os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = BLOCKS
    cfg.freeze()
    return cfg


def _oracle_run(num_classes, sample_step, sd, oitem):
    """the CPU oracle's detections of the first call, computed once per (classes, steps) and shared by the two precisions (the
    seeded initialisation does not depend on DTYPE)"""
    key = (num_classes, sample_step)
    if key not in _ORACLE:
        from diffusionvid_amd.utils import synthetic
        ocfg = odet.DetCfg(blocks=BLOCKS, num_classes=num_classes, sample_step=sample_step, num_proposals=100 if sample_step > 1 else 300)
        ocfg.head.num_classes = num_classes
        ocfg.head.sampling_timesteps = sample_step
        with torch.no_grad():
            _ORACLE[key] = odet.OracleDiffusionDet(sd, ocfg, synthetic.noise_fn).forward(oitem)
    return _ORACLE[key]


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("sample_step", [1, 4])
@pytest.mark.parametrize("num_classes", [80, 1203])
def test_wide_vocabulary_end_to_end(num_classes, sample_step, dtype):
    """A reduced model (one bottleneck block per stage) of 80 / 1203 classes on the first call of an 8-frame video, SAMPLE_STEP 1 with
    300 boxes and SAMPLE_STEP 4 with 100 (ensemble and NMS on wide labels), both precisions, against the CPU oracle under the gate of
    test_gpu_e2e.py::test_other_num_proposals: every frame's oracle detections matched one to one (label, IoU >= 0.9, |dscore| <= 5e-3)
    at a rate of at least 0.9.  Above 64 classes the head's tail runs layer by layer, the row maxima one wave per row, and at
    300 x 1203 / 100 x 1203 the candidates come from the streaming selection."""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = _cfg(num_classes, sample_step, dtype)
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    ds = SyntheticVIDDataset([E2E_L], cfg, height=E2E_H, width=E2E_W, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    images, oitem, _ = _oracle_items(ds, 0)
    ref_out = _oracle_run(num_classes, sample_step, sd, oitem)
    with torch.no_grad():
        got_out = model(images)
    assert len(got_out) == len(ref_out) == E2E_L
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    top = max(int(g.get_field("labels").max()) for g in got_out)
    print(f"[{num_classes} classes x{sample_step} {dtype}] kept {[len(g) for g in got_out]} vs oracle {[len(r['scores']) for r in ref_out]}; "
          f"match {['%.2f' % r for r in rates]}; largest label {top}")
    for r, g in zip(ref_out, got_out):
        lb = g.get_field("labels")
        assert int(lb.min()) >= 1 and int(lb.max()) <= num_classes
    assert max(int(np.max(r["labels"])) for r in ref_out) > 64 and top > 64          # the wide labels really occur
    assert min(rates) >= 0.9


def test_default_class_count_builds_its_engine():
    """NUM_CLASSES of the default config node (80, the DiffusionDet family's) creates the library model: dvid_model_create refused it"""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    default = get_cfg().MODEL.DiffusionDet.NUM_CLASSES
    assert default == 80
    model = build_detection_model(_cfg(default, 1, "float16")).to("cuda").eval()
    engine = model._get_engine()
    assert engine.num_classes == 80
