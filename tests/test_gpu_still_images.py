"""Batches of still images, each with its own size, on the GPU: the per-frame (`sizes`) forms of the four size-dependent kernels against
their scalar siblings -- bitwise, frame by frame -- and DiffusionDet.detect_images end to end: a mixed batch against every image alone,
another order, another chunking, the video path on equal sizes (all bitwise), the uniform-size answer it must differ from, the CPU
restatement (tests/_still_ref.py) and the video state it must not touch."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _still_ref as S  # noqa: E402
from oracle import backbone_r101, detector as odet, head as ohead  # noqa: E402

SIZES = [(64.0, 48.0), (40.0, 64.0), (33.0, 17.0)]          # (w, h) of the three frames of the kernel tests
COEF = dict(snr_scale=2.0, sqrt_recip_ac=1.6, sqrt_recipm1_ac=1.25, sqrt_ac_next=0.8, coef_c=0.35, sigma=0.45, keep_thr=0.5)


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


def _table(rows=SIZES):
    return torch.tensor(rows, dtype=torch.float32)


def _eq_out(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- noise_to_boxes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [100, 256, 1])
def test_noise_to_boxes_sizes_equals_the_scalar_call_per_frame(dv, m):
    """3 frames x m boxes: at m = 100 the 256-thread blocks straddle frames (boxes 100, 200), at 256 a block is a frame, at 1 a block is
    all three frames"""
    g = torch.Generator().manual_seed(m)
    x = (torch.randn(3, m, 4, generator=g) * 1.5).cuda()          # |x| beyond the scale of 2 in ~18 % of the entries: the clamp works
    got = dv.noise_to_boxes(x, 2.0, _table())
    assert got.shape == x.shape
    for f, (w, h) in enumerate(SIZES):
        assert torch.equal(got[f], dv.noise_to_boxes(x[f], 2.0, w, h)), f
    assert not torch.equal(got[1], dv.noise_to_boxes(x[1], 2.0, *SIZES[0]))
    # a table of equal rows is the scalar entry point
    assert torch.equal(dv.noise_to_boxes(x, 2.0, _table([SIZES[1]] * 3)), dv.noise_to_boxes(x, 2.0, *SIZES[1]))


def test_sizes_are_checked_before_any_launch(dv):
    x = torch.zeros(3, 4, 4, device="cuda")
    for bad in ([[64., 48.], [40., 64.]], [[64., 48.], [40., 0.], [33., 17.]], [[64., 48.], [40., float("nan")], [33., 17.]]):
        with pytest.raises(dv._lib.DvidError):
            dv.noise_to_boxes(x, 2.0, torch.tensor(bad))
    with pytest.raises(dv._lib.DvidError):
        dv.noise_to_boxes(x.view(12, 4), 2.0, _table())


def test_strided_counter_draws_equal_the_draws_image_by_image(dv):
    """dvid_counter_normal_strided: image i keyed key0 + i * stride, against one plain launch per image and the CPU restatement"""
    from diffusionvid_amd.utils import synthetic
    from oracle import noise as onoise
    dn = synthetic.DeviceNoise()
    got = dn.draw_ids("renew", [5, 6, 7], 1, (37, 4), "cuda")          # 148 values per image: a partial last quad is not needed, a partial block is
    assert got.shape == (3, 37, 4)
    for k, i in enumerate([5, 6, 7]):
        assert torch.equal(got[k], dn.draw("renew", i, 1, 0, 1, (37, 4), "cuda")[0]), i
        # the device's fp64 Box-Muller and numpy's may differ in the last fp64 bits: at most one fp32 ulp (test_gpu_kernels.py::test_counter_normal_matches_oracle)
        np.testing.assert_array_max_ulp(got[k].cpu().numpy(), onoise.noise_fn("renew", i, 1, 0, (37, 4)).numpy(), maxulp=1)
    assert torch.equal(dn.draw_ids("renew", [9, 5, 6], 1, (37, 4), "cuda")[1:], got[:2])


# ---- ddim_renew_step ------------------------------------------------------------------------------------------------------------------
def _renew_inputs(c, m=40):
    g = torch.Generator().manual_seed(100 + c)
    logits = torch.randn(3, m, c, generator=g) - 4.0          # sigmoid far below 0.5: nothing kept ...
    logits[1, ::3, (c - 1) // 2] = 2.0                         # ... frame 1 keeps every third box (the class in the middle: lane 32 at c = 65)
    logits[2, :, c - 1] = 3.0                                  # ... frame 2 keeps all (the last class: the wide form's second stride)
    wh = _table()[:, None, :]
    c0 = torch.rand(3, m, 2, generator=g) * wh
    boxes = torch.cat([c0 - 4, c0 + torch.rand(3, m, 2, generator=g) * wh * 0.5], dim=-1)
    x_t, noise, fresh = (torch.randn(3, m, 4, generator=g) for _ in range(3))
    return [t.cuda() for t in (logits, boxes, x_t, noise, fresh)]


@pytest.mark.parametrize("c", [3, 65])
def test_ddim_renew_step_sizes_equals_the_scalar_call_per_frame(dv, c):
    """c = 65 is the first class count of ddim_renew_kernel<WIDE>; the frames keep 0, some and all of their 40 boxes"""
    args = _renew_inputs(c)
    kept = (torch.sigmoid(args[0]).amax(-1) > 0.5).sum(-1).tolist()
    assert kept[0] == 0 and 0 < kept[1] < 40 and kept[2] == 40, kept
    got = dv.ddim_renew_step(*args, _table(), *COEF.values())
    for f, wh in enumerate(SIZES):
        ref = dv.ddim_renew_step(*[a[f:f + 1] for a in args], wh, *COEF.values())
        assert torch.equal(got[f:f + 1], ref), f
    # frame 2 (all kept) normalised by frame 0's size is another answer; frame 0 (nothing kept, all refilled) reads no size
    assert not torch.equal(got[2:3], dv.ddim_renew_step(*[a[2:3] for a in args], SIZES[0], *COEF.values()))
    assert torch.equal(got[0], args[4][0])
    assert torch.equal(dv.ddim_renew_step(*args, _table([SIZES[2]] * 3), *COEF.values()), dv.ddim_renew_step(*args, SIZES[2], *COEF.values()))


# ---- top-k / NMS ----------------------------------------------------------------------------------------------------------------------
BIG = (max(w for w, _ in SIZES), max(h for _, h in SIZES))          # the largest extent of any frame: (64, 64)
REACHING = [[10.0, 30.0, 30.0, 60.0], [20.0, 10.0, 60.0, 30.0], [5.0, 5.0, 50.0, 40.0]]          # box 0 of frame f: beyond f's own (w, h), inside BIG


def _hand_placed(S_, m, c=4):
    """logits [S, 3, m, c], boxes [S, 3, m, 4]: box 0 of every frame is REACHING[f] with the frame's best score (it survives any NMS), the
    others a grid of 6 x 5 boxes in near-duplicate pairs (half a pixel apart, best class shared: the NMS has work), one of them hanging
    over the left edge.  Pairwise distinct logits."""
    g = torch.Generator().manual_seed(S_ * 1000 + m)
    vals = torch.linspace(-8.0, -1.0, S_ * 3 * m * c)
    logits = vals[torch.randperm(vals.numel(), generator=g)].view(S_, 3, m, c)
    boxes = torch.empty(S_, 3, m, 4)
    for i in range(m):
        k = i // 2
        x0, y0 = -3.0 + (k % 9) * 7.0 + 0.5 * (i % 2), 2.0 + (k // 9) * 6.0
        boxes[:, :, i] = torch.tensor([x0, y0, x0 + 6.0, y0 + 5.0])
        logits[:, :, i, k % c] += 4.0 + 0.01 * i
    for f in range(3):
        boxes[:, f, 0] = torch.tensor(REACHING[f])
        logits[:, f, 0, 1] = 5.0 + 0.1 * torch.arange(S_, dtype=torch.float32)
    return logits.cuda(), boxes.cuda()


def _assert_reaching_inputs(boxes):
    for f, (w, h) in enumerate(SIZES):
        b = boxes[0, f, 0].tolist()
        assert (b[2] > w - 1 or b[3] > h - 1) and b[2] <= BIG[0] - 1 and b[3] <= BIG[1] - 1 and min(b) >= 0, (f, b)


def _assert_reaching_survives(out, f, w, h):
    """the frame's best detection is REACHING[f] clipped to the frame's own size"""
    x1, y1, x2, y2 = REACHING[f]
    assert int(out[3][f]) >= 1 and out[0][f, 0].tolist() == [x1, y1, min(x2, w - 1), min(y2, h - 1)], (f, out[0][f, 0].tolist())


@pytest.mark.parametrize("sets", [1, 2])
def test_postproc_topk_nms_sizes_equals_the_scalar_call_per_frame(dv, sets):
    logits, boxes = _hand_placed(sets, 20)
    _assert_reaching_inputs(boxes)
    got = dv.postproc_topk_nms(logits, boxes, _table())
    for f, (w, h) in enumerate(SIZES):
        ref = dv.postproc_topk_nms(logits[:, f:f + 1], boxes[:, f:f + 1], w, h)
        assert _eq_out([t[f:f + 1] for t in got], ref), f
        _assert_reaching_survives(got, f, w, h)
        assert 0 < int(got[3][f]) < sets * 20          # the NMS removed something
    # a kernel that ignored the table would give the scalar call with frame 0's size: equal for frame 0 only
    uniform = dv.postproc_topk_nms(logits, boxes, *SIZES[0])
    assert torch.equal(uniform[0][0], got[0][0])
    assert not torch.equal(uniform[0][1], got[0][1]) and not torch.equal(uniform[0][2], got[0][2])
    assert torch.equal(uniform[1], got[1]) and torch.equal(uniform[2], got[2]) and torch.equal(uniform[3], got[3])          # only the clip reads the size
    assert _eq_out(dv.postproc_topk_nms(logits, boxes, _table([SIZES[1]] * 3)), dv.postproc_topk_nms(logits, boxes, *SIZES[1]))
    assert _eq_out(dv.postproc_topk_nms(logits, boxes, _table(), use_nms=False)[:1], [torch.stack(
        [dv.postproc_topk_nms(logits[:, f:f + 1], boxes[:, f:f + 1], w, h, use_nms=False)[0][0] for f, (w, h) in enumerate(SIZES)])])


def test_nms_frames_tiled_sizes_equals_the_scalar_call_and_postproc(dv):
    """70 candidates: two mask words, the last one partial (6 bits)"""
    logits, boxes = _hand_placed(1, 70)
    _assert_reaching_inputs(boxes)
    cb, cs, cl = dv.topk_candidates_stream(logits, boxes)          # the lists postproc hands its NMS
    assert cs.shape == (3, 70)
    got = dv.nms_frames_tiled(cb, cs, cl, _table())
    assert _eq_out(got, dv.postproc_topk_nms(logits, boxes, _table()))          # the single-workgroup kernel runs 70 candidates
    for f, (w, h) in enumerate(SIZES):
        ref = dv.nms_frames_tiled(cb[f:f + 1], cs[f:f + 1], cl[f:f + 1], w, h)
        assert _eq_out([t[f:f + 1] for t in got], ref), f
        _assert_reaching_survives(got, f, w, h)
    uniform = dv.nms_frames_tiled(cb, cs, cl, *SIZES[0])
    assert torch.equal(uniform[0][0], got[0][0]) and not torch.equal(uniform[0][1], got[0][1]) and not torch.equal(uniform[0][2], got[0][2])
    assert _eq_out(dv.nms_frames_tiled(cb, cs, cl, _table([SIZES[2]] * 3)), dv.nms_frames_tiled(cb, cs, cl, *SIZES[2]))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
BLOCKS = (1, 1, 1, 1)
SMALL = ["MODEL.VID.MEGA.GLOBAL.ENABLE", False, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", False, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 0,
         "MODEL.DiffusionDet.NUM_HEADS", 2, "MODEL.DiffusionDet.NUM_PROPOSALS", 40, "MODEL.DiffusionDet.NUM_CLASSES", 30]
P2_OPTS = ["MODEL.ROI_HEADS.IN_FEATURES", ["p2", "p3", "p4", "p5"], "MODEL.FPN.IN_FEATURES", ["res2", "res3", "res4", "res5"]]
IMAGE_HW = [(96, 160), (128, 96), (80, 112), (128, 160)]          # on a canvas of 128 x 160; the last one fills it
IDS = [12, 3, 40, 7]
VARIANTS = [(p2, dtype, step) for p2 in (False, True) for dtype in ("float16", "float32") for step in (1, 3)]


@functools.lru_cache(maxsize=None)
def _model(p2, dtype, step, weights="trained_like"):
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    cfg, model = E._build(step, BLOCKS, weights, extra=SMALL + (P2_OPTS if p2 else []), dtype=dtype)
    model.noise_fn = synthetic.noise_fn
    return cfg, model


@functools.lru_cache(maxsize=None)
def _batch():
    from diffusionvid_amd.utils import synthetic
    images = [synthetic.synthetic_frame(20 + i, h, w, smooth=True) for i, (h, w) in enumerate(IMAGE_HW)]
    canvas, sizes = S.canvas_of(images)
    assert tuple(canvas.shape) == (4, 3, 128, 160) and sizes == IMAGE_HW
    return images, canvas, canvas.cuda()


def _image_list(canvas, sizes_hw):
    from diffusionvid_amd.structures.image_list import ImageList
    return ImageList(canvas, [torch.Size(s) for s in sizes_hw])


def _same(a, b):
    return (len(a) == len(b) and a.size == b.size and torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
            and torch.equal(a.get_field("labels"), b.get_field("labels")))


def _mixed(model):
    with torch.no_grad():
        out = model.detect_images(_image_list(_batch()[2], IMAGE_HW), IDS)
    assert len(out) == 4 and all(len(o) > 0 for o in out)
    return out


@pytest.mark.parametrize("p2,dtype,step", VARIANTS)
def test_mixed_batch_is_invariant(p2, dtype, step):
    """the mixed batch against every image alone on the same canvas, the batch in another order, and launch sequences of one image"""
    _, model = _model(p2, dtype, step)
    images, _, canvas = _batch()
    mixed = _mixed(model)
    for i, (h, w) in enumerate(IMAGE_HW):
        assert mixed[i].size == (w, h) and mixed[i].mode == "xyxy" and mixed[i].get_field("labels").dtype == torch.int64
        assert mixed[i].bbox.min() >= 0 and mixed[i].bbox[:, 0::2].max() <= w - 1 and mixed[i].bbox[:, 1::2].max() <= h - 1
        with torch.no_grad():
            alone = model.detect_images(_image_list(canvas[i:i + 1], IMAGE_HW[i:i + 1]), [IDS[i]])
        assert len(alone) == 1 and _same(alone[0], mixed[i]), f"image {i} alone"
    order = [2, 0, 3, 1]
    with torch.no_grad():
        perm = model.detect_images(_image_list(canvas[order].contiguous(), [IMAGE_HW[i] for i in order]), [IDS[i] for i in order])
        # ... and as a list of un-padded images on the host: detect_images makes the same canvas itself
        listed = model.detect_images([images[i] for i in order], [IDS[i] for i in order])
    for k, i in enumerate(order):
        assert _same(perm[k], mixed[i]), f"image {i} at position {k}"
        assert _same(listed[k], mixed[i]), f"image {i} from a list"
    model.still_chunk = 1
    try:
        with torch.no_grad():
            chunked = model.detect_images(_image_list(canvas, IMAGE_HW), IDS)
    finally:
        model.still_chunk = None
    assert all(_same(a, b) for a, b in zip(chunked, mixed))
    model.results_on_host = True
    try:
        host = _mixed(model)
    finally:
        model.results_on_host = False
    assert all(h.bbox.device.type == "cpu" and _same(h, m.to(torch.device("cpu"))) for h, m in zip(host, mixed))


@pytest.mark.parametrize("step", [1, 3])
def test_device_draws_keep_the_invariance(step):
    """synthetic.DeviceNoise: consecutive ids (one launch per kind and step for the batch) against the images alone (a launch each)"""
    from diffusionvid_amd.utils import synthetic
    _, model = _model(False, "float16", step)
    canvas, ids = _batch()[2], [5, 6, 7, 8]
    try:
        model.noise_fn = synthetic.DeviceNoise()
        with torch.no_grad():
            mixed = model.detect_images(_image_list(canvas, IMAGE_HW), ids)
            for i in range(4):
                alone = model.detect_images(_image_list(canvas[i:i + 1], IMAGE_HW[i:i + 1]), [ids[i]])
                assert len(mixed[i]) > 0 and _same(alone[0], mixed[i]), i
    finally:
        model.noise_fn = synthetic.noise_fn


@pytest.mark.parametrize("p2,dtype,step", VARIANTS)
def test_mixed_batch_differs_from_the_uniform_size_answer(p2, dtype, step):
    """what one size per call gave: every image scaled, normalised and clipped by image 0's size.  Equal for image 0, another answer for
    every image of another size -- a detector that ignored the table would pass every invariance test above"""
    _, model = _model(p2, dtype, step)
    mixed = _mixed(model)
    with torch.no_grad():
        uniform = model.detect_images(_image_list(_batch()[2], [IMAGE_HW[0]] * 4), IDS)
    assert _same(uniform[0], mixed[0])
    for i in (1, 2, 3):
        assert not (len(uniform[i]) == len(mixed[i]) and torch.equal(uniform[i].bbox, mixed[i].bbox)), i


@pytest.mark.parametrize("p2,dtype,step", VARIANTS)
def test_equal_sizes_equal_the_video_path(p2, dtype, step):
    """four frames of one size: the first call of a four-frame video of the baseline configuration (forward with the dict) against
    detect_images on the same frames, draws keyed by absolute image index on both sides -- the path the oracle tests cover"""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    cfg, model = _model(p2, dtype, step)
    ds = SyntheticVIDDataset([4], cfg, height=120, width=150, device="cuda", smooth=True)
    item = ds[0][0]
    frames = torch.cat([im.tensors for im in item["ref_l"]])
    assert frames.shape == (4, 3, 128, 160) and not item["ref_g"]
    try:
        model.noise_fn = S.video_noise_fn(synthetic.noise_fn)
        with torch.no_grad():
            video = model(item)
    finally:
        model.noise_fn = synthetic.noise_fn
    with torch.no_grad():
        still = model(_image_list(frames, [(120, 150)] * 4))          # forward routes it to detect_images; image_ids 0 .. 3
    assert len(video) == len(still) == 4
    for f in range(4):
        assert len(video[f]) > 0 and _same(video[f], still[f]), f


@pytest.mark.parametrize("step", [1, 3])
def test_video_results_do_not_depend_on_still_calls_in_between(step):
    """a 16-frame video call by call (two working calls: the second one reads the queue the first one left), then again with still
    batches detected in between"""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    cfg, model = _model(False, "float16", step)
    ds = SyntheticVIDDataset([16], cfg, height=120, width=150, device="cuda", smooth=True)
    runs = []
    for with_stills in (False, True):
        out = []
        with torch.no_grad():
            for idx in range(9):
                out.append(model(ds[idx][0]))
                if with_stills and idx in (0, 4, 7):
                    _mixed(model)
        runs.append(out)
    assert [len(o) for o in runs[0]] == [8, 0, 0, 0, 0, 0, 0, 0, 8]
    for a, b in zip(*runs):
        assert len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    # the same video call again, right behind a still call
    with torch.no_grad():
        first = model(ds[0][0])
        _mixed(model)
        again = model(ds[0][0])
    assert all(_same(x, y) for x, y in zip(first, again))


@pytest.mark.parametrize("p2", [False, True])
@pytest.mark.parametrize("step", [1, 3])
def test_mixed_batch_against_the_restatement(p2, step):
    """float32 against tests/_still_ref.py with test_gpu_e2e's helpers and its float32 bounds: logits / boxes of the first pass (the same
    boxes on both sides; later DDIM steps start from each side's own renewal) and the detections of every image"""
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    _, model = _model(p2, "float32", step, "init")
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    levels = ("p2", "p3", "p4", "p5") if p2 else ("p3", "p4", "p5")
    hc = ohead.HeadCfg(num_classes=30, num_heads=2, num_heads_local=0, top_k=(40, 25), sampling_timesteps=step,
                       scales=tuple(1.0 / (1 << int(l[1])) for l in levels))
    ocfg = odet.DetCfg(num_proposals=40, num_classes=30, sample_step=step, blocks=BLOCKS, in_features=levels, head=hc)

    def backbone_fn(x):
        return backbone_r101.fpn(backbone_r101.resnet_bottom_up(x, sd, "backbone.bottom_up.", BLOCKS), sd, "backbone.", in_features=tuple("res" + l[1] for l in levels))
    taps = {}
    with torch.no_grad():
        ref = S.detect_images(sd, ocfg, synthetic.noise_fn, _batch()[1], IMAGE_HW, IDS, backbone_fn=backbone_fn, taps=taps)
    model.debug_taps = {}
    try:
        got = _mixed(model)
        gcl, gbx = model.debug_taps["still_final_0"][0] if step == 1 else model.debug_taps["final_0"]
    finally:
        model.debug_taps = None
    tag = f"[still x{step} {'p2' if p2 else 'p3'} float32]"
    E._stage_check(f"{tag} first pass", None, None, gcl.cpu(), taps["final_0"][0], gbx.cpu(), taps["final_0"][1], b_logit=0.008, b_px=0.05, b_rel=0.001)
    rates = [E._match_rate(r, g) for r, g in zip(ref, got)]
    print(f"{tag} detections: kept {[len(g) for g in got]} vs restatement {[len(r['scores']) for r in ref]}; match rates {['%.2f' % r for r in rates]}")
    assert min(rates) >= 0.9


def test_mixed_batch_equals_singles_swin():
    """Swin-FPN, reduced (CONFIG_OVERRIDE), window 7, p3..p5, float16"""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_Swin_B_DiffusionVID.yaml", ["DTYPE", "float16"] + SMALL, "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.SWIN.CONFIG_OVERRIDE = dict(embed_dim=64, depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), window=7)
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.trained_like_scores(synthetic.tame_box_deltas(model.state_dict(), 0.1)))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    canvas = _batch()[2]
    mixed = _mixed(model)
    for i in range(4):
        with torch.no_grad():
            alone = model.detect_images(_image_list(canvas[i:i + 1], IMAGE_HW[i:i + 1]), [IDS[i]])
        assert _same(alone[0], mixed[i]), i
