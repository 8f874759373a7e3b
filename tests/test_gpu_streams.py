"""Several live streams on one model, on the GPU: the grouped memory-update kernels and the grouped global attention bit-equal per group
to their single-problem forms; a StreamSet bit-equal per stream to a private model, isolated from the video path, and close to the CPU
oracle.  120 x 200 frames, BLOCKS_OVERRIDE (1, 1, 1, 1): the shapes of test_gpu_e2e.py::test_streaming_mode_online_memory_update."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detector as odet  # noqa: E402
from oracle import memory as omem  # noqa: E402

D = 256
STREAMING = ["INPUT.INFER_BATCH", 1, "MODEL.VID.MEGA.MAX_OFFSET", 0, "MODEL.VID.MEGA.MIN_OFFSET", 0, "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 1,
             "MODEL.VID.MEGA.KEY_FRAME_LOCATION", 0, "MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST", False]
BLOCKS = (1, 1, 1, 1)


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


# ---- 1. the memory-update kernels -------------------------------------------------------------------------------------------------------
def _groups(n, seed):
    """x [3, n, 256]: three groups of different data; group 1 holds duplicated rows (every fourth row repeats its predecessor, and the
    last row repeats row 0), so exact ties occur in its sweep"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(3, n, D, generator=g)
    if n > 1:
        x[1, 1::4] = x[1, 0::4][: x[1, 1::4].shape[0]]
        x[1, n - 1] = x[1, 0]
    return x


# n -> m: the protocol's shapes; one past a 64-wide distance tile; the edges of the sweep's points-per-thread templates (4 / 8 / 16 points
# on 256 threads: 1024 | 1025, 2048 | 2049, 4096 the last size of the register kernel); m == n and m == 1
SHAPES = [(175, 150), (975, 900), (1800, 900), (65, 64), (1024, 512), (1025, 512), (2049, 1024), (4096, 2048), (300, 300), (300, 1)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_grouped_memory_update_is_bit_equal_per_group(dv, n, m):
    x = _groups(n, 100 + n).cuda()
    dist = dv.cdist_groups(x)
    idx = dv.fps_greedy_groups(dist, m)
    out = dv.gather_rows_groups(x, idx)
    assert dist.shape == (3, n, n) and idx.shape == (3, m) and idx.dtype == torch.int32 and out.shape == (3, m, D)
    r = n - n // 3          # the composed entry: memory rows first, new rows behind
    mem_g, idx_g = dv.update_erase_memory_groups(x[:, r:].contiguous(), x[:, :r].contiguous(), m) if m < n else (None, None)
    for g in range(3):
        d1 = dv.cdist(x[g])
        assert torch.equal(dist[g], d1), ("cdist", g)
        i1 = dv.fps_greedy(d1, m)
        assert torch.equal(idx[g], i1), ("fps", g)
        assert torch.equal(out[g], dv.gather_rows(x[g], i1)), ("gather", g)
        if m < n:
            m1, j1 = dv.update_erase_memory(x[g, r:], x[g, :r], m)
            assert torch.equal(mem_g[g], m1) and torch.equal(idx_g[g], j1), ("update_erase_memory", g)
    # exact ties (group 1's duplicated rows): the picks of fps.cu's tie rule on the GPU's own distances, integer-equal
    d_host = dist[1].cpu().numpy()
    if n > 1:
        assert (d_host[:, 0] == d_host[:, 1]).all()          # duplicated rows give bit-equal columns: the ties are exact
    np.testing.assert_array_equal(idx[1].cpu().numpy(), omem.fps_kernel_order(d_host, m))
    assert len(set(idx[0].tolist())) == m and int(idx.min()) >= 0 and int(idx.max()) < n


def test_grouped_memory_update_groups_are_independent(dv):
    x = _groups(975, 7).cuda()
    mem, idx = dv.update_erase_memory_groups(x[:, 900:].contiguous(), x[:, :900].contiguous(), 900)
    y = x.clone()
    y[0].normal_()
    y[2].mul_(-3.0)
    mem2, idx2 = dv.update_erase_memory_groups(y[:, 900:].contiguous(), y[:, :900].contiguous(), 900)
    assert torch.equal(mem[1], mem2[1]) and torch.equal(idx[1], idx2[1])
    assert not torch.equal(idx[0], idx2[0])
    # written in place over the memories themselves (the merged rows are a copy): the same result
    held = x[:, :900].contiguous()
    mem3, idx3 = dv.update_erase_memory_groups(x[:, 900:].contiguous(), held, 900, out=held)
    assert mem3 is held and torch.equal(mem3, mem) and torch.equal(idx3, idx)


def test_grouped_memory_update_under_target_is_the_concatenation(dv):
    g = torch.Generator().manual_seed(3)
    new, mem = torch.randn(3, 75, D, generator=g).cuda(), torch.randn(3, 300, D, generator=g).cuda()
    out, idx = dv.update_erase_memory_groups(new, mem, 900)
    assert idx is None and torch.equal(out, torch.cat([mem, new], dim=1))
    out, idx = dv.update_erase_memory_groups(new, mem, 375)          # r + k == target: still nothing to prune
    assert idx is None and out.shape == (3, 375, D)
    out, idx = dv.update_erase_memory_groups(new, None, 900)
    assert idx is None and torch.equal(out, new)


def test_grouped_memory_update_refuses_scratch_over_the_limit(dv):
    from diffusionvid_amd import _lib
    x = torch.zeros(17, 4096, 4, device="cuda")          # 17 x 4096 x 4096 x 4 bytes = 1.0625 GiB of distances
    need = 17 * 4096 * 4096 * 4
    with pytest.raises(_lib.DvidError, match=r"17 groups x 4096 x 4096 distances are %d bytes, the limit is %d" % (need, 1 << 30)):
        dv.update_erase_memory_groups(x[:, 2048:].contiguous(), x[:, :2048].contiguous(), 2048)
    with pytest.raises(_lib.DvidError, match=r"%d bytes, the limit is %d" % (need, 1 << 30)):
        dv.cdist_groups(x)
    with pytest.raises(_lib.DvidError, match=r"1 <= m <= n.*n 8, m 9"):
        dv.fps_greedy_groups(torch.zeros(2, 8, 8, device="cuda"), 9)
    torch.cuda.synchronize()


# ---- 2. grouped global attention ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["float16", "float32"])
def test_global_xattn_groups_is_bit_equal_per_group(dv, precision):
    from diffusionvid_amd.utils import synthetic
    model = dv.Model(synthetic.make_head_state_dict(0), res_blocks=(0, 0, 0, 0), precision=precision)
    model.reserve(3, 64, 64, 300)
    g = torch.Generator().manual_seed(21)
    video_mem = torch.randn(900, D, generator=g).cuda()
    q = torch.randn(3 * 300, D, generator=g).cuda()
    before = model.global_xattn(q[:300], video_mem)
    projections = []
    real_call = dv.call

    def counting(name, *a):
        if name.startswith("dvid_global_memory_project"):
            projections.append(name)
        return real_call(name, *a)
    dv.call = counting
    try:
        for lk in (900, 150, 75):          # 75 is no multiple of 32: the V-transpose padding
            mem = torch.randn(3, lk, D, generator=g).cuda()
            del projections[:]
            out = model.global_xattn_groups(q, mem)
            assert projections == ["dvid_global_memory_project_groups"]
            again = model.global_xattn_groups(q, mem)          # same object, same version: cached
            assert projections == ["dvid_global_memory_project_groups"] and torch.equal(out, again)
            # the video's own projection is still there: no re-projection, the same bits
            assert torch.equal(model.global_xattn(q[:300], video_mem), before) and projections == ["dvid_global_memory_project_groups"]
            singles = dv.Model(synthetic.make_head_state_dict(0), res_blocks=(0, 0, 0, 0), precision=precision)
            singles.reserve(3, 64, 64, 300)
            for k in range(3):
                one = singles.global_xattn(q[k * 300:(k + 1) * 300], mem[k].contiguous())
                assert torch.equal(out[k * 300:(k + 1) * 300], one), (precision, lk, k)
            singles.close()
            mem.mul_(2.0)          # an in-place torch write bumps the version: projected again
            model.global_xattn_groups(q, mem)
            assert projections.count("dvid_global_memory_project_groups") == 2
    finally:
        dv.call = real_call
        model.close()


@pytest.mark.parametrize("precision", ["float16", "float32"])
def test_three_projected_memories_are_independent(dv, precision):
    """The video's global memory, the streams' grouped global memories and the local memories on ONE model: each is projected once, each
    attention reads its own projection whatever ran between, and each gives the bits of a model that ran nothing else.  lk = 75 is no
    multiple of 32 (the V-transpose padding); 600 query rows in 2 groups."""
    import re
    from diffusionvid_amd.utils import synthetic

    def fresh():
        m = dv.Model(synthetic.make_head_state_dict(0, local_stages=1), res_blocks=(0, 0, 0, 0), precision=precision)
        m.reserve(2, 64, 64, 300)
        return m
    g = torch.Generator().manual_seed(33)
    q = torch.randn(600, D, generator=g).cuda()
    video_mem = torch.randn(75, D, generator=g).cuda()
    group_mem = torch.randn(2, 75, D, generator=g).cuda()
    local_mem = torch.randn(150, D, generator=g).cuda()
    runs = {"video": lambda m: m.global_xattn(q, video_mem), "groups": lambda m: m.global_xattn_groups(q, group_mem),
            "local": lambda m: m.local_xattn(q, local_mem, groups=2)}
    model = fresh()
    projections = []
    real_call = dv.call

    def counting(name, *a):
        if re.fullmatch(r"dvid_\w+_memory_project\w*", name):
            projections.append(name)
        return real_call(name, *a)
    dv.call = counting
    try:
        first = {k: runs[k](model) for k in ("video", "groups", "local")}
        second = {k: runs[k](model) for k in ("local", "groups", "video")}
        assert sorted(projections) == ["dvid_global_memory_project", "dvid_global_memory_project_groups", "dvid_local_memory_project"]
    finally:
        dv.call = real_call
    for k in runs:
        assert torch.equal(first[k], second[k]), (precision, k)
        alone = fresh()
        assert torch.equal(runs[k](alone), first[k]), (precision, k)
        alone.close()
    assert not torch.equal(first["video"], first["groups"]) and not torch.equal(first["groups"], first["local"])          # three different memories
    model.close()


# ---- 3.-5. end to end ---------------------------------------------------------------------------------------------------------------------
def _model(dtype, sample_step):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["DTYPE", dtype, "MODEL.DiffusionDet.SAMPLE_STEP", sample_step] + STREAMING,
                  "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = BLOCKS
    cfg.freeze()
    model = build_detection_model(cfg)
    model.load_state_dict(synthetic.tame_box_deltas(model.state_dict(), 0.1))
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    return cfg, model


def _video(cfg, length, base, first_globals=None):
    """the items of one synthetic video; first_globals: the opening call delivers only that many global frames"""
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    ds = SyntheticVIDDataset([length], cfg, height=120, width=200, device="cuda", smooth=True, video_base=base)
    items = [ds[i][0] for i in range(length)]
    if first_globals is not None:
        items[0] = dict(items[0], ref_g=items[0]["ref_g"][:first_globals])
    return items


def _schedule(cfg):
    """{stream: [item or None per step]}: stream 0 opens with 4 global frames (memories 300 / 100 rows, growing: the no-prune path, a second
    memory shape in the step, the first pruning of the 150-row memory on its call 3); stream 1 runs a 5-call video and restarts with a
    3-call one (frame_category 0 mid-run); stream 2 opens two steps late, its 24-frame opening call beside steady calls."""
    a, b, b2, c = _video(cfg, 7, 0, first_globals=4), _video(cfg, 5, 1), _video(cfg, 3, 2), _video(cfg, 4, 3)
    steps = 8
    plan = {0: a + [None] * (steps - 7), 1: b + b2, 2: [None, None] + c + [None, None]}
    assert all(len(v) == steps for v in plan.values())
    return plan, steps


def _snapshot(boxlists, memory):
    assert len(boxlists) == 1
    bl = boxlists[0]
    return (bl.bbox.clone(), bl.get_field("scores").clone(), bl.get_field("labels").clone(), [m.clone() for m in memory])


def _private_run(model, plan, steps):
    """every stream's items through `model(item)`, one stream after the other (a new video resets the model) -> {(stream, step): snapshot}"""
    ref = {}
    with torch.no_grad():
        for s, seq in plan.items():
            for t in range(steps):
                if seq[t] is not None:
                    ref[(s, t)] = _snapshot(model(seq[t]), model.global_memory())
    return ref


def _assert_same(got, want, what):
    for k, (a, b) in enumerate(zip(got[:3], want[:3])):
        assert torch.equal(a, b), (what, ("boxes", "scores", "labels")[k])
    assert len(want[0]) > 0, what
    for i in range(2):
        assert torch.equal(got[3][i], want[3][i]), (what, "memory %d" % i)


def _set_run(streams, plan, steps, ref, reverse=False, between=None):
    with torch.no_grad():
        for t in range(steps):
            items = {s: plan[s][t] for s in (sorted(plan, reverse=reverse)) if plan[s][t] is not None}
            out = streams.step(items)
            assert list(out) == list(items)
            for s in items:
                _assert_same(_snapshot(out[s], streams.global_memory(s)), ref[(s, t)], ("stream", s, "step", t))
            if between is not None:
                between(t)


_REF = {}


def _reference(dtype, sample_step):
    """(cfg, model, plan, steps, the private model's results), computed once per configuration and left unchanged"""
    key = (dtype, sample_step)
    if key not in _REF:
        cfg, model = _model(dtype, sample_step)
        plan, steps = _schedule(cfg)
        _REF[key] = (cfg, model, plan, steps, _private_run(model, plan, steps))
    return _REF[key]


@pytest.mark.parametrize("sample_step", [1, 4])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_stream_set_equals_private_models(dtype, sample_step):
    cfg, model, plan, steps, ref = _reference(dtype, sample_step)
    rows = [tuple(m.shape[0] for m in ref[(0, t)][3]) for t in range(7)]
    assert rows[:4] == [(300, 100), (375, 125), (450, 150), (525, 150)] and rows[-1] == (750, 150)          # stream 0 grows, memory 1 prunes from call 3 on
    assert tuple(m.shape[0] for m in ref[(2, 2)][3]) == (900, 150)
    _, shared = _model(dtype, sample_step)          # the same weights (seeded), its own engine
    _set_run(shared.open_streams(), plan, steps, ref)
    # three frames per launch sequence and the streams in the other order: the same bits
    _set_run(shared.open_streams(frames_per_launch=3), plan, steps, ref, reverse=True)
    assert shared.head.proposal_feats_global == [None, None] and shared.head.proposal_feats_global_groups is None


def test_stream_steps_leave_a_video_on_the_same_model_alone():
    cfg, model, plan, steps, ref = _reference("float16", 1)
    video = _video(cfg, steps, 9)
    with torch.no_grad():
        alone = [_snapshot(model(it), model.global_memory()) for it in video]
    streams = model.open_streams()

    def between(t):          # one call of the video between two steps of the set, on the same model
        _assert_same(_snapshot(model(video[t]), model.global_memory()), alone[t], ("video call", t))
    _set_run(streams, plan, steps, ref, between=between)
    # a stream can be closed and adopt a memory; the adopted rows are what it holds
    mem = streams.global_memory(2)
    streams.close(2)
    assert 2 not in streams.streams()
    streams.adopt_memory(2, mem)
    assert all(torch.equal(a, b) for a, b in zip(streams.global_memory(2), mem))


def test_stream_set_against_the_oracle():
    """Two streams, each against its own CPU oracle, per call: every call starts from its oracle's memory of the previous call (adopt_memory),
    as test_gpu_e2e.py::test_streaming_mode_online_memory_update injects it; that test's match-rate gates.  The oracle's backbone on the
    CPU is what this test's time goes to (0.6 s a frame), so the videos are short and open with 6 and 2 global frames: 18 frames in all,
    two memory shapes in every step, and stream 0's 150-row memory pruned on both of its steady calls."""
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    cfg, model = _model("float16", 1)
    L = 3
    videos = [_video(cfg, L, 0, first_globals=6), _video(cfg, L, 5, first_globals=2)]
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    oracles = [odet.OracleDiffusionDet(sd, odet.DetCfg(blocks=BLOCKS, infer_batch=1, all_frame_interval=1), synthetic.noise_fn) for _ in videos]
    streams = model.open_streams()
    rates = []
    for idx in range(L):
        items, refs = {}, {}
        for s, (video, oracle) in enumerate(zip(videos, oracles)):
            images = video[idx]
            oitem = {k: v for k, v in images.items() if k not in ("cur", "ref_l", "ref_g")}
            oitem.update(cur=images["cur"].tensors.cpu(), image_size=tuple(images["cur"].image_sizes[0]),
                         ref_l=[im.tensors.cpu() for im in images["ref_l"]], ref_g=[im.tensors.cpu() for im in images["ref_g"]])
            if idx > 0:
                streams.adopt_memory(s, [m.cuda() for m in oracle.mem])
            with torch.no_grad():
                refs[s] = oracle.forward(oitem)
            items[s] = images
        with torch.no_grad():
            got = streams.step(items)
        for s in items:
            assert len(refs[s]) == len(got[s]) == 1
            rates.append(E._match_rate(refs[s][0], got[s][0]))
    print("[streams vs oracle] detections matched min %.2f mean %.3f" % (min(rates), sum(rates) / len(rates)))
    assert min(rates) >= 0.9 and sum(rates) / len(rates) >= 0.97, rates
