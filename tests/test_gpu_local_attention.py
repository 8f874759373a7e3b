"""Local box-level attention on the GPU (dvid_local_memory_project / dvid_local_xattn, csrc/localattn.hip) against the restatement of
tests/_local_ref.py, which tests/test_local_attention.py pins to the reference through g18.

Tolerances are test_global_xattn's for the same precision: float16 rtol 5e-3 + 5e-3 of the output RMS (the oracle gets the fp16-rounded
weights and inputs), float32 1e-4 / 1e-4.  The full-dimension kernels need hidden 256 / head dim 32, g18 is the reference at the reduced
dimensions g5 uses (hidden 16), so DynamicHead.forward is compared with the pinned restatement at full dimensions on g16's inputs.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import golden  # noqa: E402
from oracle import detector as odet, head as ohead  # noqa: E402

import _local_ref as L  # noqa: E402
from test_gpu_kernels import check, h16  # noqa: E402


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


def _sd(stages, f16):
    from diffusionvid_amd.utils import synthetic
    sd = synthetic.make_head_state_dict(0, local_stages=stages)
    return sd, ({k: (h16(v) if v.dim() > 1 else v) for k, v in sd.items()} if f16 else sd)


@pytest.mark.parametrize("precision", ["float16", "float32"])
@pytest.mark.parametrize("groups,lk,stages", [(1, 600, 1), (3, 600, 1), (1, 200, 2), (3, 75, 1), (3, 77, 2)])
def test_local_xattn(dv, precision, groups, lk, stages):
    f16 = precision == "float16"
    sd, sdo = _sd(stages, f16)
    g = torch.Generator().manual_seed(90 + lk + groups)
    rows = 300 * groups + (0 if groups > 1 else 37)          # 337 rows: a ragged last 32-row tile
    q = torch.randn(1, rows, 256, generator=g)
    mem = torch.randn(groups * lk, 256, generator=g)
    qo, mo = (h16(q), h16(mem)) if f16 else (q, mem)
    local = [None, None]
    local[stages - 1] = mo
    if stages == 2:
        local[0] = mo[:groups * 8]          # stage 0 is dead: any memory
    ref = L.local_attention(sdo, "head.", qo, local, stages, ohead.HeadCfg(), groups)
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0), precision=precision)
    model.reserve(4, 64, 64, 300)
    memd, qd = mem.cuda(), q[0].cuda()
    out = model.local_xattn(qd, memd, groups=groups)
    tol = 5e-3 if f16 else 1e-4
    check(f"local_xattn[{precision},groups={groups},lk={lk},stage={stages}]", out, ref, tol, tol)
    if precision == "float32":          # the fp32 MFMA form of the fused epilogue (option f32_split = 0)
        dv.set_option("f32_split", 0)
        try:
            model.invalidate_local_memory()
            out0 = model.local_xattn(qd, memd, groups=groups)
        finally:
            dv.reset_options()
        check(f"local_xattn[{precision},f32_split=0,groups={groups},lk={lk}]", out0, ref, tol, tol)
    # the grouped call == the same groups one by one, bit for bit
    if groups > 1:
        per = rows // groups
        for gi in range(groups):
            one = model.local_xattn(qd[gi * per:(gi + 1) * per], memd[gi * lk:(gi + 1) * lk].clone(), groups=1)
            assert torch.equal(one, out[gi * per:(gi + 1) * per]), f"group {gi}"
    model.close()


def test_model_without_local_tensors_answers_err_state(dv):
    from diffusionvid_amd import _lib
    sd, _ = _sd(0, True)
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
    model.reserve(1, 64, 64, 300)
    q = torch.zeros(300, 256, device="cuda")
    lib = _lib.load()
    s = _lib.stream_ptr()
    assert lib.dvid_local_memory_project(model.handle, 0, q.data_ptr(), 300, 1, s) == 4          # DVID_ERR_STATE
    assert lib.dvid_local_xattn(model.handle, 0, q.data_ptr(), 300, 1, 300, q.data_ptr(), s) == 4
    model.close()
    sd3, _ = _sd(3, True)
    with pytest.raises(_lib.DvidError, match="code 3"):          # DVID_ERR_UNSUPPORTED: more than two stages
        dv.Model(sd3, res_blocks=(0, 0, 0, 0))


def _head_cfg(*opts):
    from diffusionvid_amd.config import get_cfg
    return get_cfg("configs/vid_R_101_DiffusionVID.yaml", list(opts), "configs/BASE_RCNN_1gpu.yaml")


@pytest.mark.parametrize("stages", [1, 2])
def test_dynamic_head_forward_local(dv, stages):
    """DynamicHead.forward (box_extract == 0, cached stages popped) through the C ABI against the pinned restatement, on g16's full-dimension
    inputs and its stage outputs as the cached tuple; bounds of test_gpu_kernels.py's reference-fixture test for the conditioned head."""
    from diffusionvid_amd.modeling.roi_heads.box_head.box_head import DynamicHead
    z = golden("g16_full_dim_head")
    n, M, H, W = (int(z[k]) for k in ("n", "M", "H", "W"))
    sd, sdo = _sd(stages, True)
    T32 = lambda k: torch.from_numpy(z[k].astype(np.float32))
    feats = [T32(k) for k in ("p3", "p4", "p5")]
    cached = (T32("cl1"), T32("bx1"), T32("of1"))
    g = torch.Generator().manual_seed(181)
    local = [h16(torch.randn(3 * 75, 256, generator=g)), h16(torch.randn(3 * 25, 256, generator=g))]
    t = torch.from_numpy(z["t"])
    rl, rb = L.head_final_local(sdo, "head.", feats, T32("boxes"), t, ohead.HeadCfg(), cached, local, stages)
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
    head = DynamicHead(_head_cfg("MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", True, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE", stages,
                                 "MODEL.VID.MEGA.GLOBAL.ENABLE", False), engine_provider=lambda: model)
    head.eval()
    head.proposal_feats_local = [m.cuda() for m in local]
    head.proposals_feat_cur = [[cached[0].cuda(), cached[1].cuda(), cached[2].cuda()]]
    gl, gb = head([dv.nhwc_from_nchw(f.cuda()) for f in feats], T32("boxes").cuda(), t, None)
    assert gl.shape == (1, n, M, 30) and gb.shape == (1, n, M, 4)
    check(f"dynamic_head_local[stage {stages}].logits", gl, rl, 2e-3, 2e-3)
    bin_ = cached[1]
    bw = (bin_[..., 2:] - bin_[..., :2]).clamp(min=1.0).max(-1).values
    err = ((gb[0].cpu() - rb[0]).abs().max(-1).values / bw).max().item()
    print(f"dynamic_head_local[stage {stages}]: boxes rel-to-size err max={err:.3e}")
    assert err < 1e-2
    head.check_boxes_valid()
    model.close()


def _video_model(dtype, la=1, local=True, glob=False, stage=1, extra=(), trained_like=False):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils import synthetic
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml",
                  ["DTYPE", dtype, "INPUT.LOOKAHEAD_BATCHES", la, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", local,
                   "MODEL.VID.ROI_BOX_HEAD.ATTENTION.STAGE", stage, "MODEL.VID.MEGA.GLOBAL.ENABLE", glob] + list(extra), "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    sd = synthetic.tame_box_deltas(model.state_dict(), 0.1)
    if trained_like:
        sd = synthetic.trained_like_scores(sd)
    model.load_state_dict(sd)
    model = model.to("cuda").eval()
    model.noise_fn = synthetic.noise_fn
    return cfg, model


def _run(cfg, model, lengths, hw=(120, 200)):
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    ds = SyntheticVIDDataset(lengths, cfg, height=hw[0], width=hw[1], device="cuda", smooth=True)
    res = []
    with torch.no_grad():
        for idx in range(len(ds)):
            res += model(ds[idx][0])
    return ds, res


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x.bbox, y.bbox) and torch.equal(x.get_field("scores"), y.get_field("scores")) and torch.equal(x.get_field("labels"), y.get_field("labels"))


def test_local_plus_global_equals_global_only():
    """the global stage overwrites the local product (box_head.py:366-371): same weights -> bit-identical detections"""
    cfg_g, m_g = _video_model("float16", local=False, glob=True)
    cfg_lg, m_lg = _video_model("float16", local=True, glob=True, stage=2)
    m_lg.load_state_dict({**m_lg.state_dict(), **m_g.state_dict()})
    _, a = _run(cfg_g, m_g, [16])
    _, b = _run(cfg_lg, m_lg, [16])
    assert len(a) == 16
    _same(a, b)


def test_local_video_lookahead_and_call_graph_are_bit_identical():
    """a 3-batch video (20 frames: ragged tail), local attention only: INPUT.LOOKAHEAD_BATCHES 1 against 3 (each batch of the group
    attends its own local memory in one grouped launch) and use_call_graph on against off"""
    outs = {}
    for la, graph in ((1, True), (1, False), (3, True)):
        cfg, model = _video_model("float16", la=la)
        model.use_call_graph = graph
        _, outs[(la, graph)] = _run(cfg, model, [20])
        assert len(outs[(la, graph)]) == 20 and all(len(o) > 0 for o in outs[(la, graph)])
    _same(outs[(1, True)], outs[(1, False)])
    _same(outs[(1, True)], outs[(3, True)])


def _against_oracle(cfg, model, ds_lengths, ocfg, stages, tag):
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.utils import synthetic
    from test_gpu_e2e import TRAINED_LIKE_F32, _ap50_on_objects, _ap50_vs_oracle, _match_rate, _oracle_items
    H0, W0 = 120, 200
    ds = SyntheticVIDDataset(ds_lengths, cfg, height=H0, width=W0, device="cuda", smooth=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    oracle = L.LocalOracleDet(sd, ocfg, synthetic.noise_fn, stages)
    ref_out, got_out = [], []
    with torch.no_grad():
        for idx in range(len(ds)):
            images, oitem, _ = _oracle_items(ds, idx)
            ref_out += oracle.forward(oitem)
            got_out += model(images)
    assert len(ref_out) == len(got_out) == sum(ds_lengths)
    rates = [_match_rate(r, g) for r, g in zip(ref_out, got_out)]
    ap = _ap50_vs_oracle(ref_out, got_out, (W0, H0))
    ap_obj, n_obj = _ap50_on_objects(ref_out, got_out, (W0, H0))
    print(f"{tag}: match min {min(rates):.3f} mean {np.mean(rates):.3f}; AP50 {ap:.4f}; AP50 over {n_obj} objects {ap_obj:.4f}")
    g = TRAINED_LIKE_F32[("r101", 1)]
    assert min(rates) >= g["match"] and ap >= g["ap"]
    if n_obj:
        assert ap_obj >= g["ap_objects"]


def test_local_video_float32_against_the_oracle_with_local_deques():
    cfg, model = _video_model("float32", trained_like=True)
    _against_oracle(cfg, model, [20], odet.DetCfg(blocks=(1, 1, 1, 1)), 1, "[local, float32, 20 frames]")


def test_local_streaming_against_the_oracle_with_local_deques():
    """INFER_BATCH 1, ALL_FRAME_INTERVAL 1: every frame is conditioned on its own top-75 features"""
    extra = ["INPUT.INFER_BATCH", 1, "MODEL.VID.MEGA.MAX_OFFSET", 0, "MODEL.VID.MEGA.MIN_OFFSET", 0, "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 1,
             "MODEL.VID.MEGA.KEY_FRAME_LOCATION", 0]
    cfg, model = _video_model("float32", extra=extra, trained_like=True)
    _against_oracle(cfg, model, [6], odet.DetCfg(blocks=(1, 1, 1, 1), infer_batch=1, all_frame_interval=1), 1, "[local, float32, streaming]")
