"""CPU tests of the host side: C-ABI surface, config API, boundary types, dataset/sampler protocol,
prediction packing.  No GPU, no compute calls into the library."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dvid_[a-z0-9_]+)\s*\(", txt)))


def test_c_abi_library_exports_every_declared_symbol():
    from diffusionvid_amd import _lib
    lib = _lib.load()                       # dlopen works without a GPU
    names = _header_symbols()
    assert len(names) >= 25
    for n in names:
        assert n in _lib.SIGNATURES, f"{n} declared in include/dvid_hip.h but not bound in _lib.SIGNATURES"
        assert getattr(lib, n) is not None
    assert set(_lib.SIGNATURES) == set(names)
    assert lib.dvid_version() >= 1


ALLOWED_ENV_SWITCHES = {"DVID_LIB", "DVID_IGEMM_TUNE", "DVID_IGEMM_TUNE_CACHE", "DVID_CHAINS", "DVID_POISON_WORKSPACE", "DVID_CALL_GRAPH", "DVID_PROFILE_DUMP"}


def test_default_library_configuration_is_the_benchmarked_one():
    """Round 6: the library's switches are one option table set through the C ABI (csrc/options.h), not 38 environment variables.  With a
    clean environment the effective configuration of a freshly loaded library equals the string bench.py quotes its numbers on
    (bench.DEFAULT_LIBRARY_CONFIG, echoed in the line's build.library_config); options round-trip through dvid_set_option /
    dvid_get_option / dvid_reset_options, bad names and values are refused; and the product sources read no DVID_* environment
    variable beyond the seven documented ones."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); from diffusionvid_amd import ops; import bench; c = ops.effective_config(); "
            "assert c.split(' DVID_')[0] == bench.DEFAULT_LIBRARY_CONFIG, c; "
            "assert c.endswith('DVID_IGEMM_TUNE= DVID_IGEMM_TUNE_CACHE= DVID_CHAINS= DVID_POISON_WORKSPACE='), c; print('ok')" % ROOT)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DVID_")}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
    from diffusionvid_amd import _lib, ops
    try:
        ops.set_option("head_tail", 0)
        ops.set_option("conv3x3", 2)
        assert ops.get_option("head_tail") == 0 and ops.get_option("conv3x3") == 2
        assert "head_tail=0" in ops.effective_config() and "conv3x3=2" in ops.effective_config()
        _lib.check(_lib.load().dvid_igemm_set_conv3x3(-1), "set_conv3x3")          # -1 = the default
        assert ops.get_option("conv3x3") == 1
        with pytest.raises(_lib.DvidError, match="unknown option"):
            ops.set_option("no_such_option", 1)
        with pytest.raises(_lib.DvidError, match="outside"):
            ops.set_option("stem_pool", 7)
    finally:
        ops.reset_options()
    import bench
    assert ops.effective_config().split(" DVID_")[0] == bench.DEFAULT_LIBRARY_CONFIG
    # environment reads of the product sources (library, package, bench.py)
    seen = set()
    for d, _, files in os.walk(os.path.join(ROOT, "diffusionvid_amd")):
        if "_build" in d:
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(d, f)).read()
                seen |= set(re.findall(r'(?:getenv\(|environ(?:\.get|\.setdefault)?[\[(]|in os\.environ)\s*"(DVID_[A-Z0-9_]+)"', src))
    src = open(os.path.join(ROOT, "bench.py")).read()
    seen |= set(re.findall(r'environ(?:\.get|\.setdefault)?[\[(]\s*"(DVID_[A-Z0-9_]+)"', src))
    assert seen <= ALLOWED_ENV_SWITCHES, sorted(seen - ALLOWED_ENV_SWITCHES)
    assert len(ALLOWED_ENV_SWITCHES) < 15


def test_split_operand_arithmetic_bound():
    """The arithmetic of the DTYPE float32 path's split-operand products (csrc/f32_split.h, used by f32x3_igemm_kernel and its four siblings), restated in numpy -- no GPU: a value v is
    carried as hi = fp16(v), lo = fp16(v - hi); a dot product is accumulated in fp32 from lo_a hi_b + hi_a lo_b + hi_a hi_b (each fp16 x fp16 product is
    exact in fp32).  With the weight rows scaled by a power of two to a largest magnitude in [0.5, 1) (ops.pack_conv_weight_f32(scale_rows=True), what
    make_conv does) the result is as close to the exact dot product as a plain fp32 evaluation is for O(1) activations, where an fp16-operand product
    (the DTYPE float16 path's arithmetic) is three orders of magnitude away.  The stated limit of the scheme is visible too: an activation below 2^-3
    carries its lo part as an fp16 subnormal (absolute 3e-8), so a tensor of UNIFORMLY 1e-3-sized activations is reproduced to ~1e-4 of the result's RMS
    -- still 10 x closer than fp16 operands, no longer fp32 grade (no tensor of this path looks like that: LayerNorm-ed rows and post-ReLU maps have O(1)
    leading entries; the end-to-end float32 gates measure what matters).
    Also: the packing helpers reconstruct the weights (hi + lo within 2^-21 of the scaled row, scale exact)."""
    from diffusionvid_amd import ops
    rng = np.random.default_rng(0)
    K, N, M = 2304, 64, 48
    w = (rng.standard_normal((N, K)) * (2.0 / K) ** 0.5).astype(np.float32)
    wp, kpad, rs = ops.pack_conv_weight_f32(torch.from_numpy(w), scale_rows=True)
    hi, lo = ops.split_f16(wp)
    assert kpad == K and wp.shape == (N, K)
    mx = wp.abs().amax(1)
    assert torch.all((mx >= 0.5) & (mx < 1.0)) and torch.equal(wp * rs[:, None], torch.from_numpy(w))          # power-of-two scaling: exact both ways
    assert float(((hi.float() + lo.float()) - wp).abs().max()) <= 2.0 ** -21
    whi, wlo = hi.float().numpy(), lo.float().numpy()
    for scale in (1.0, 1e-3):
        a = (rng.standard_normal((M, K)) * scale).astype(np.float32)
        exact = a.astype(np.float64) @ w.astype(np.float64).T
        f32 = a @ w.T
        ahi = a.astype(np.float16).astype(np.float32)
        alo = (a - ahi).astype(np.float16).astype(np.float32)
        split = ((alo @ whi.T + ahi @ wlo.T) + ahi @ whi.T) * rs.numpy()[None, :]
        f16 = ahi @ w.astype(np.float16).astype(np.float32).T
        rms = np.sqrt((exact ** 2).mean())
        e32, es, e16 = (np.abs(x - exact).max() / rms for x in (f32, split, f16))
        if scale == 1.0:
            assert es <= 4.0 * max(e32, 2e-7), (scale, es, e32)          # within a small factor of plain fp32's own rounding
            assert e16 >= 300 * es, (scale, e16, es)                      # ... where fp16 operands are ~1e-3
        else:
            assert es <= 1.5e-4 and e16 >= 10 * es, (scale, es, e16)


def test_product_path_fails_loudly_without_gpu():
    from diffusionvid_amd import _lib, ops
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.DvidError):
        ops.cdist(torch.zeros(4, 8))
    with pytest.raises(_lib.DvidError):
        ops.Model({})


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "diffusionvid_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports oracle"


def test_config_merge_order_and_freeze():
    from diffusionvid_amd.config import get_cfg
    c = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"),
                ["MODEL.DiffusionDet.SAMPLE_STEP", "4", "DTYPE", "float16"], os.path.join(ROOT, "configs/BASE_RCNN_8gpu.yaml"))
    assert c.MODEL.META_ARCHITECTURE == "DiffusionDet"
    assert c.MODEL.DiffusionDet.SAMPLE_STEP == 4 and c.DTYPE == "float16"
    assert c.MODEL.DiffusionDet.NUM_HEADS == 3 and c.MODEL.DiffusionDet.NUM_HEADS_LOCAL == 1
    assert c.INPUT.INFER_BATCH == 8 and c.MODEL.VID.MEGA.GLOBAL.SIZE == 24 and c.TEST.IMS_PER_BATCH == 8
    assert c.MODEL.RESNETS.RES5_DILATION == 1            # model yaml overrides the base file
    assert c.MODEL.PIXEL_MEAN == [123.675, 116.280, 103.530]
    c.freeze()
    with pytest.raises(AttributeError):
        c.DTYPE = "float32"
    with pytest.raises(KeyError):
        get_cfg(None, ["MODEL.NOT_A_KEY", "1"])


def test_boxlist_and_imagelist_match_reference_goldens():
    from diffusionvid_amd.structures.bounding_box import BoxList
    from diffusionvid_amd.structures.image_list import to_image_list
    z = golden("g9_structures")
    il = to_image_list((torch.from_numpy(z["img"]),), 32)
    np.testing.assert_array_equal(il.tensors.numpy(), z["padded"])
    assert tuple(il.image_sizes[0]) == tuple(z["image_size"])
    bl = BoxList(torch.from_numpy(z["boxes"]).clone(), (1000, 600)).clip_to_image(remove_empty=False)
    np.testing.assert_array_equal(bl.bbox.numpy(), z["clipped"])
    with pytest.raises(ValueError):
        BoxList(torch.zeros(3), (10, 10))
    with pytest.raises(ValueError):
        BoxList(torch.zeros(3, 4), (10, 10), mode="abcd")
    e = BoxList(torch.zeros(0, 4), (10, 10))
    e.add_field("scores", torch.zeros(0))
    assert len(e) == 0 and len(e.clip_to_image(remove_empty=True)) == 0


def test_sampler_partitions_match_reference_golden():
    from diffusionvid_amd.data.samplers import VIDTestDistributedSampler
    z = golden("g10_sampler")
    ds = type("DS", (), {"start_index": [int(i) for i in z["start_index"]], "__len__": lambda self: int(z["length"])})()
    for world, rank, start, end in z["parts"]:
        s = VIDTestDistributedSampler(ds, int(world), int(rank))
        # the reference returns None (-1 here) when no video starts at/after the offset; this build maps
        # that to len(dataset) (an empty tail shard instead of re-running the whole set)
        assert s.start == (start if start >= 0 else len(ds))
        assert s.end == (end if end >= 0 else len(ds))
    # every frame is owned by exactly one rank, shards are whole videos
    for world in (1, 2, 3, 4, 8):
        owned = []
        for r in range(world):
            owned += list(VIDTestDistributedSampler(ds, world, r))
        assert sorted(owned) == list(range(len(ds)))


def _ref_ids_formula(frame_id, seg_len, max_offset=7, interval=8, gsize=24):
    """independent restatement of vid_mega.py:198-221 for consecutive frames"""
    final = min(frame_id + max_offset, seg_len - 1)
    if frame_id == 0:
        start = max(final - interval + 1, 0)
    else:
        start = max(final - min(1, interval) + 1, 0)
    g = [(frame_id + gsize - i - 1) % seg_len for i in range(gsize if frame_id == 0 else 0)]
    return list(range(start, final + 1)), g, final


@pytest.mark.parametrize("lengths", [[8], [5], [13, 30], [304]])
def test_dataset_item_protocol(lengths):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), None, os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    ds = SyntheticVIDDataset(lengths, cfg, height=40, width=70)
    assert len(ds) == sum(lengths) and ds.start_index == list(np.cumsum([0] + lengths[:-1]))
    idx = 0
    for L in lengths:
        for f in range(L):
            rl, rg, fin = ds.ref_ids(idx)
            assert (rl, rg, fin) == _ref_ids_formula(f, L)
            idx += 1
    images, target, ids = ds[0]
    assert target is None and ids == list(range(8))
    assert images["frame_category"] == 0 and images["seg_len"] == lengths[0] and images["end_id"] == lengths[0] - 1
    assert len(images["ref_g"]) == 24 and len(images["ref_l"]) == min(8, lengths[0])
    assert images["cur"].tensors.shape == (1, 3, 64, 96) and tuple(images["cur"].image_sizes[0]) == (40, 70)
    assert float(images["cur"].tensors[0, :, 40:, :].abs().max()) == 0.0       # zero padding to /32
    if lengths[0] > 1:
        im1 = ds[1][0]
        assert im1["frame_category"] == 1 and im1["ref_g"] == [] and len(im1["ref_l"]) == 1


def test_pack_unpack_predictions_roundtrip():
    from diffusionvid_amd.engine import inference as eng
    from diffusionvid_amd.structures.bounding_box import BoxList
    g = torch.Generator().manual_seed(0)
    res = {}
    for i, k in zip((5, 2, 9), (3, 0, 300)):
        bl = BoxList(torch.rand(k, 4, generator=g) * 100, (1000, 600))
        bl.add_field("scores", torch.rand(k, generator=g))
        bl.add_field("labels", torch.randint(1, 31, (k,), generator=g))
        res[i] = bl
    back = eng.unpack_predictions(*eng.pack_predictions(res, 300))
    assert sorted(back) == [2, 5, 9]
    for i in res:
        assert torch.equal(back[i].bbox, res[i].bbox) and back[i].size == (1000, 600)
        assert torch.equal(back[i].get_field("scores"), res[i].get_field("scores"))
        assert torch.equal(back[i].get_field("labels"), res[i].get_field("labels"))
    assert [len(b) for b in eng.predictions_list(back)] == [0, 3, 300]


def test_detector_builds_with_reference_state_dict_names():
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    cfg = get_cfg(os.path.join(ROOT, "configs/vid_R_101_DiffusionVID.yaml"), None, os.path.join(ROOT, "configs/BASE_RCNN_1gpu.yaml"))
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    m = build_detection_model(cfg).eval()
    sd = m.state_dict()
    for k, shape in {
            "head.head_series.2.inst_interact.dynamic_layer.weight": (32768, 256),
            "head.head_series.0.inst_interact.out_layer.weight": (256, 12544),
            "head.head_series_cond.0.block_time_mlp.1.weight": (256, 1024),
            "head.head_series.1.block_time_mlp.1.weight": (512, 1024),
            "head.head_series_cond.0.c_mlp.1.weight": (256, 256),
            "head.global_attention.0.0.in_proj_weight": (768, 256),
            "head.time_mlp.3.weight": (1024, 1024),
            "head.head_series.0.reg_module.6.weight": (256, 256),
            "head.head_series.0.class_logits.weight": (30, 256),
            "backbone.bottom_up.stem.conv1.weight": (64, 3, 7, 7),
            "backbone.bottom_up.res2.0.shortcut.norm.running_var": (256,),
            "backbone.fpn_lateral5.weight": (256, 2048, 1, 1),
            "backbone.fpn_output3.bias": (256,),
            "alphas_cumprod": (1000,), "sqrt_recipm1_alphas_cumprod": (1000,)}.items():
        assert tuple(sd[k].shape) == shape, k
    z = golden("g1_schedule")
    np.testing.assert_array_equal(sd["alphas_cumprod"].numpy(), z["alphas_cumprod"])
    assert m.head.top_k == [75, 25] and m.num_heads_local == 1
    with pytest.raises(NotImplementedError):
        m.train()
        m({"cur": torch.zeros(1, 3, 32, 32), "ref_l": [], "ref_g": []})


def test_vid_evaluator_matches_reference_golden(tmp_path):
    """diffusionvid_amd/data/evaluation/vid_eval.py vs the reference's eval_detection_vid (golden g11)."""
    from diffusionvid_amd.data.evaluation import vid_eval
    from diffusionvid_amd.structures.bounding_box import BoxList
    z = golden("g11_vid_eval")
    preds, gts = [], []
    for f in range(int(z["nframes"])):
        gt = BoxList(torch.from_numpy(z[f"gt_box_{f}"]), (500, 400))
        gt.add_field("labels", torch.from_numpy(z[f"gt_lab_{f}"]))
        pr = BoxList(torch.from_numpy(z[f"pr_box_{f}"]), (500, 400))
        pr.add_field("labels", torch.from_numpy(z[f"pr_lab_{f}"]))
        pr.add_field("scores", torch.from_numpy(z[f"pr_sc_{f}"]))
        preds.append(pr)
        gts.append(gt)
    res = vid_eval.eval_detection_vid(preds, gts)
    np.testing.assert_allclose(res["ap"], z["ap"], rtol=0, atol=1e-12, equal_nan=True)
    assert abs(res["map"] - float(z["map"])) < 1e-12 and 0.0 < res["map"] < 1.0
    # perfect predictions -> AP50 = 1 for every class present
    perfect = []
    for gt in gts:
        p = BoxList(gt.bbox.clone(), gt.size)
        p.add_field("labels", gt.get_field("labels"))
        p.add_field("scores", torch.ones(len(gt)))
        perfect.append(p)
    assert vid_eval.eval_detection_vid(perfect, gts)["map"] == 1.0
    # predictions.pth round trip
    path = str(tmp_path / "predictions.pth")
    vid_eval.save_predictions(preds, path)
    back = vid_eval.load_predictions(path)
    assert len(back) == len(preds) and torch.equal(back[3].bbox, preds[3].bbox)


def test_dataset_lookahead_slots_match_later_calls():
    """`ref_ahead[fb]` (INPUT.LOOKAHEAD_BATCHES extension) must hold exactly the frames that calls fb-7 .. fb deliver
    through `ref_l` in the reference protocol (vid_mega.py:178-221), including the repeated last frame at the tail."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["INPUT.LOOKAHEAD_BATCHES", 4], "configs/BASE_RCNN_1gpu.yaml")
    ds = SyntheticVIDDataset([53], cfg, height=32, width=48)
    delivered = {}            # batch call fb -> frames accumulated from ref_l of calls fb-7 .. fb
    queue = []
    ahead = {}
    for idx in range(len(ds)):
        item = ds[idx][0]
        f = item["frame_id"]
        ahead.update(item.get("ref_ahead", {}))
        assert ("ref_ahead" in item) == (f % 32 == 0)
        queue += item["ref_l"]
        if f % 8 == 0:
            delivered[f] = queue
            queue = []
    assert sorted(ahead) == [8, 16, 24, 40, 48]
    for fb, frames in ahead.items():
        assert len(frames) == len(delivered[fb]) == 8
        for a, b in zip(frames, delivered[fb]):
            assert a is b                  # the same cached ImageList object -> the same frame


def test_checkpoint_key_matching_matches_reference_golden():
    """utils/checkpoint.py (strip `module.`, DiffusionDet -> DiffusionVID head renaming, longest-suffix matching) against
    what the reference's own loader functions did with the same key sets (golden g13: model_serialization.py:12-138 run
    under the import shims): every model key must take the same source key, or none."""
    from conftest import golden
    from diffusionvid_amd.utils import checkpoint as ck
    z = golden("g13_checkpoint_matching")
    model_keys = [str(k) for k in z["model_keys"]]
    cases = sorted(k[len("loaded."):] for k in z.files if k.startswith("loaded."))
    assert len(cases) == 5
    for name in cases:
        loaded = {str(k): str(k) for k in z["loaded." + name]}
        loaded = ck.strip_prefix_if_present(loaded, "module.")
        loaded = ck.remap_diffusiondet_heads(model_keys, loaded, None)
        got = ck.match_keys(sorted(model_keys), sorted(loaded.keys()))
        want = dict(zip(model_keys, (str(s) for s in z["source." + name])))
        for k in model_keys:
            src = loaded[got[k]] if got[k] is not None else ""
            assert src == want[k], f"{name}: {k} <- {src!r}, reference {want[k]!r}"
    # the cases are not vacuous
    assert sum(1 for s in z["source.diffusiondet_heads"] if "head_series.3" in str(s)) > 40
    assert sum(1 for s in z["source.backbone_pickle"] if str(s)) == 85
    amb = dict(zip(model_keys, (str(s) for s in z["source.ambiguous_suffixes"])))
    assert amb["backbone.bottom_up.res2.0.conv1.weight"] == "res2.0.conv1.weight"
    assert amb["backbone.bottom_up.res3.0.conv1.weight"] == "0.conv1.weight"


def test_detectron_checkpointer_round_trip(tmp_path):
    """A released-style checkpoint -- `module.` prefix, DiffusionDet head numbering, wrapped in {"model": ...} -- and a
    detectron2 torchvision pickle (numpy arrays, bare backbone names) load through DetectronCheckpointer into the model's
    own names with the exact values (what dvid_model_finalize then folds / repacks)."""
    import pickle
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    from diffusionvid_amd.utils.checkpoint import DetectronCheckpointer
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["MODEL.DEVICE", "cpu"], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = (1, 1, 1, 1)
    cfg.freeze()
    model = build_detection_model(cfg)
    g = torch.Generator().manual_seed(99)
    want = {k: (v + torch.randn(v.shape, generator=g) * 0.1 if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    ckpt = {"module." + k.replace("head_series_cond.0", "head_series.3"): v for k, v in want.items()}
    f = tmp_path / "model_final.pth"
    torch.save({"model": ckpt, "iteration": 7, "optimizer": {}}, f)
    extra = DetectronCheckpointer(cfg, model).load(str(f))
    assert extra == {"iteration": 7}
    got = model.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    # backbone-only pickle on top: body weights replaced, everything else untouched
    body = {k[len("backbone.bottom_up."):]: (v * 2).numpy() for k, v in want.items() if k.startswith("backbone.bottom_up.")}
    p = tmp_path / "torchvision-R-101.pkl"
    with open(p, "wb") as fh:
        pickle.dump({"model": body, "__author__": "x"}, fh)
    ck = DetectronCheckpointer(cfg, model)
    ck.load(str(p))
    got = model.state_dict()
    for k in want:
        ref = want[k] * 2 if k.startswith("backbone.bottom_up.") else want[k]
        assert torch.equal(got[k], ref), k
    assert all(not k.startswith("backbone.bottom_up.") for k in ck.missed_keys) and "head.time_mlp.1.weight" in ck.missed_keys
    with pytest.raises(NotImplementedError):
        DetectronCheckpointer(get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["MODEL.BACKBONE.CONV_BODY", "R-101-FPN", "MODEL.DEVICE", "cpu"],
                                      "configs/BASE_RCNN_1gpu.yaml"), model).load(str(p))


def _tiny_vid_set(tmp_path, lens, hw=(12, 16)):
    """on-disk set in the reference's layout; every image stores (video, frame) in pixel (0, 0)"""
    from PIL import Image
    lines, n = [], 0
    for v, L in enumerate(lens):
        d = tmp_path / "Data" / "VID" / "val" / ("vid%02d" % v)
        d.mkdir(parents=True)
        for f in range(L):
            n += 1
            img = np.zeros(hw + (3,), np.uint8)
            img[0, 0] = (v, f, 7)
            Image.fromarray(img).save(str(d / ("%06d.JPEG" % f)), format="PNG")
            lines.append("val/vid%02d %d %d %d" % (v, n, f, L))
    (tmp_path / "ImageSets").mkdir()
    index = tmp_path / "ImageSets" / "VID_val_videos.txt"
    index.write_text("\n".join(lines) + "\n")
    return str(tmp_path / "Data" / "VID"), str(index), lines


@pytest.mark.parametrize("tag", ["shipped", "streaming"])
def test_real_vid_dataset_protocol_matches_reference_class(tmp_path, tag):
    """data/datasets/vid.py against the reference's REAL VIDMEGADataset._get_test run on the same on-disk layout (golden
    g14): bookkeeping ints, the files loaded as local / global reference frames (read back from the pixels), image ids;
    the synthetic bench dataset must produce the same protocol for the same video lengths."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.datasets import VIDFrameList, VIDMEGATestDataset
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    z = golden("g14_vid_dataset_protocol")
    lens = [int(x) for x in z["lens"]]
    img_dir, index, lines = _tiny_vid_set(tmp_path, lens)
    assert lines == [str(x) for x in z["index_lines"]]
    opts = [] if tag == "shipped" else ["INPUT.INFER_BATCH", 1, "MODEL.VID.MEGA.MAX_OFFSET", 0, "MODEL.VID.MEGA.MIN_OFFSET", 0,
                                        "MODEL.VID.MEGA.ALL_FRAME_INTERVAL", 1, "MODEL.VID.MEGA.GLOBAL.STOP_UPDATE_AFTER_INIT_TEST", False]
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", opts + ["MODEL.VID.MEGA.GLOBAL.SHUFFLE", False], "configs/BASE_RCNN_1gpu.yaml")
    fl = VIDFrameList(index)
    assert len(fl) == sum(lens) and fl.frame_seg_len[0] == lens[0] and fl.image_set_index[22] == "val/vid01/000001"
    ds = VIDMEGATestDataset(cfg, img_dir, index)
    syn = SyntheticVIDDataset(lens, cfg, height=12, width=16)
    assert ds.start_index == [int(x) for x in z[tag + ".start_index"]] == syn.start_index
    rows, ref_l, ref_g = z[tag + ".rows"], list(z[tag + ".ref_l"]), list(z[tag + ".ref_g"])
    pl = pg = 0
    for idx in range(len(ds)):
        images, target, ids = ds[idx]
        px = lambda im: (int(im[0, 0, 0]), int(im[0, 0, 1]))       # noqa: E731
        got = [images["frame_category"], images["frame_id"], images["start_id"], images["end_id"], images["seg_len"],
               images["last_queue_id"], px(images["cur"])[0], len(images["ref_l"]), len(images["ref_g"])]
        assert got == [int(x) for x in rows[idx]], (idx, got, rows[idx])
        assert px(images["cur"])[1] == images["frame_id"]
        nl, ng = len(images["ref_l"]), len(images["ref_g"])
        assert [px(im)[1] for im in images["ref_l"]] == [int(x) for x in ref_l[pl:pl + nl]]
        assert [px(im)[1] for im in images["ref_g"]] == [int(x) for x in ref_g[pg:pg + ng]]
        assert ids == [int(x) for x in z[tag + ".ids"][idx]]
        # the synthetic driver emits the same protocol
        s_l, s_g, s_last = syn.ref_ids(idx)
        assert s_l == [int(x) for x in ref_l[pl:pl + nl]] and s_g == [int(x) for x in ref_g[pg:pg + ng]] and s_last == images["last_queue_id"]
        pl, pg = pl + nl, pg + ng
    assert pl == len(ref_l) and pg == len(ref_g)


def test_real_vid_dataset_lookahead_handover(tmp_path):
    """INPUT.LOOKAHEAD_BATCHES: `ref_ahead` of the real dataset holds, per later batch of the group, exactly the frames its own
    calls would deliver through `ref_l` (same files, same order), like the synthetic dataset's."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.datasets import VIDMEGATestDataset
    img_dir, index, _ = _tiny_vid_set(tmp_path, [37, 8])
    base = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["MODEL.VID.MEGA.GLOBAL.SHUFFLE", False], "configs/BASE_RCNN_1gpu.yaml")
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["MODEL.VID.MEGA.GLOBAL.SHUFFLE", False, "INPUT.LOOKAHEAD_BATCHES", 3],
                  "configs/BASE_RCNN_1gpu.yaml")
    plain, ahead = VIDMEGATestDataset(base, img_dir, index), VIDMEGATestDataset(cfg, img_dir, index)
    px = lambda im: int(im[0, 0, 1])       # noqa: E731
    delivered = {}
    for idx in range(37):
        it = plain[idx][0]
        fb = -(-it["frame_id"] // 8) * 8
        delivered.setdefault(fb, []).extend(px(im) for im in it["ref_l"])
    for idx in range(45):
        it = ahead[idx][0]
        assert ("ref_ahead" in it) == (it["frame_id"] % 24 == 0)
        if it["seg_len"] <= it["frame_id"] + 8:
            assert not it.get("ref_ahead")
        if idx < 37 and "ref_ahead" in it:
            for fb, frames in it["ref_ahead"].items():
                assert [px(im) for im in frames] == delivered[fb], fb


def test_resize_matches_pillow_and_reference_size_rule():
    """data/transforms.py: get_size against the reference's Resize.get_size table (golden g14, transforms.py:39-59); the
    integer two-pass resample (the tables the HIP kernels consume) against Pillow's own BILINEAR resize, bit for bit,
    including an axis that keeps its size and an up-scaling case."""
    from PIL import Image
    from diffusionvid_amd.data import transforms as T
    z = golden("g14_vid_dataset_protocol")
    for wh, want in zip(z["resize.wh"], z["resize.out_hw"]):
        assert tuple(T.get_size((int(wh[0]), int(wh[1])))) == (int(want[0]), int(want[1]))
    rng = np.random.RandomState(1)
    for (h, w), (mn, mx) in [((72, 128), (60, 100)), ((128, 72), (60, 100)), ((37, 53), (84, 120)), ((60, 100), (60, 100)),
                             ((200, 50), (40, 90)), ((90, 161), (60, 100))]:
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        oh, ow = T.get_size((w, h), mn, mx)
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        np.testing.assert_array_equal(T.resize_u8_numpy(img, (oh, ow)), ref)
        t = T.ResizeToTensor(mn, mx)(img, True)
        assert t.shape == (3, oh, ow) and torch.equal(t, torch.from_numpy(ref.copy()).permute(2, 0, 1).float().div(255))


def test_motion_specific_ap_matches_reference_golden(tmp_path):
    """Motion-specific AP50 (all / fast / medium / slow; vid_eval.py:39-50, :164-299) against the reference's
    calc_detection_vid_prec_rec + calc_detection_vid_ap on the same toy set (golden g15), and tools/test_prediction.py on a
    predictions.pth + ground-truth file written from it."""
    import subprocess
    import sys
    from diffusionvid_amd.data.evaluation import vid_eval
    from diffusionvid_amd.structures.bounding_box import BoxList
    z = golden("g15_vid_eval_motion")
    preds, gts, motion = [], [], []
    for f in range(int(z["n_frames"])):
        gt = BoxList(torch.from_numpy(z[f"gt_boxes{f}"]).reshape(-1, 4), (500, 400))
        gt.add_field("labels", torch.from_numpy(z[f"gt_labels{f}"]))
        pr = BoxList(torch.from_numpy(z[f"pr_boxes{f}"]).reshape(-1, 4), (500, 400))
        pr.add_field("labels", torch.from_numpy(z[f"pr_labels{f}"]))
        pr.add_field("scores", torch.from_numpy(z[f"pr_scores{f}"]))
        preds.append(pr)
        gts.append(gt)
        motion.append([float(x) for x in z[f"motion{f}"]])
    res = vid_eval.eval_detection_vid(preds, gts, motion_ious=motion)
    assert len(res) == 4
    for i, r in enumerate(res):
        np.testing.assert_allclose(r["ap"], z[f"ap{i}"], rtol=0, atol=1e-12, equal_nan=True)
        assert abs(r["map"] - float(z[f"map{i}"])) < 1e-12
    assert len({round(r["map"], 6) for r in res}) > 1                       # the ranges really differ on this set
    # the all-motion range equals the plain evaluator
    plain = vid_eval.eval_detection_vid(preds, gts)
    np.testing.assert_allclose(res[0]["ap"], plain["ap"], rtol=0, atol=1e-12, equal_nan=True)
    # tools/test_prediction.py: predictions.pth + ground truth + motion file -> result.txt
    folder = tmp_path / "inference" / "VID_val_videos"
    folder.mkdir(parents=True)
    vid_eval.save_predictions(preds, str(folder / "predictions.pth"))
    torch.save({"gt": gts, "motion_ious": motion}, str(tmp_path / "gt.pth"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "test_prediction.py"), "--prediction-folder", str(tmp_path),
                          "--dataset", "VID_val_videos", "--ground-truth", str(tmp_path / "gt.pth"), "--motion-specific"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1500:]
    text = (folder / "result.txt").read_text()
    assert "AP50 | motion=   all = %.4f" % res[0]["map"] in text and "AP50 | motion=  slow = %.4f" % res[3]["map"] in text
    assert "Category AP:" in text


def test_engine_builds_lookahead_from_unchanged_dataset(tmp_path):
    """engine.lookahead_items: from a dataset that emits the reference's unchanged item dict the engine loop builds the same
    `ref_ahead` hand-over the look-ahead-aware datasets emit themselves -- same batches, same frames in the same order --
    for the synthetic driver (frame objects compared by identity) and for the real dataset class on image files (frames
    identified by their pixels), across video boundaries and ragged tails; every item is loaded exactly once."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.data.datasets import VIDMEGATestDataset
    from diffusionvid_amd.data.synthetic_video import SyntheticVIDDataset
    from diffusionvid_amd.engine import inference as eng
    cfg = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["MODEL.VID.MEGA.GLOBAL.SHUFFLE", False, "INPUT.LOOKAHEAD_BATCHES", 3],
                  "configs/BASE_RCNN_1gpu.yaml")
    lens = [37, 8, 50]
    own = SyntheticVIDDataset(lens, cfg, height=16, width=16)
    plain = SyntheticVIDDataset(lens, cfg, height=16, width=16, emit_ref_ahead=False)
    plain._cache = own._cache
    loads = []
    real_get = plain.__class__.__getitem__

    class Counting:
        def __len__(self):
            return len(plain)

        def __getitem__(self, i):
            loads.append(i)
            return real_get(plain, i)
    seen = 0
    for idx, (images, _, ids) in eng.lookahead_items(Counting(), range(len(plain)), 8, 3):
        want = own[idx][0]
        assert ("ref_ahead" in images) == ("ref_ahead" in want)
        if "ref_ahead" in want:
            assert sorted(images["ref_ahead"]) == sorted(want["ref_ahead"])
            for fb in want["ref_ahead"]:
                assert all(a is b for a, b in zip(images["ref_ahead"][fb], want["ref_ahead"][fb])), (idx, fb)
                assert len(images["ref_ahead"][fb]) == 8
            seen += len(want["ref_ahead"])
        assert images["frame_id"] == want["frame_id"] and ids == own[idx][2]
    assert seen > 6 and sorted(loads) == list(range(len(plain)))            # each item loaded once
    # the real dataset class on files
    img_dir, index, _ = _tiny_vid_set(tmp_path, [37, 8])
    ds_own = VIDMEGATestDataset(cfg, img_dir, index)
    base = get_cfg("configs/vid_R_101_DiffusionVID.yaml", ["MODEL.VID.MEGA.GLOBAL.SHUFFLE", False], "configs/BASE_RCNN_1gpu.yaml")
    ds_plain = VIDMEGATestDataset(base, img_dir, index)
    px = lambda im: (int(im[0, 0, 0]), int(im[0, 0, 1]))       # noqa: E731
    for idx, (images, _, ids) in eng.lookahead_items(ds_plain, range(len(ds_plain)), 8, 3):
        want = ds_own[idx][0]
        got = {fb: [px(im) for im in fr] for fb, fr in images.get("ref_ahead", {}).items()}
        exp = {fb: [px(im) for im in fr] for fb, fr in want.get("ref_ahead", {}).items()}
        assert got == exp, idx


def test_take_returns_views_inside_a_launch_and_concatenations_across():
    """diffusion_det.take, the split of frame slots [a, b) that DiffusionDet._extract and StreamSet._extract share, over two launch
    results of 3 and 2 frames."""
    from diffusionvid_amd.modeling.detector.diffusion_det import take
    g = torch.Generator().manual_seed(5)
    keys = ("logits", "boxes", "obj", "k1", "k2")

    def launch(n, levels=2):
        res = {k: torch.randn(n, 4, 3 + i, generator=g) for i, k in enumerate(keys)}
        res["feats"] = [torch.randn(n, 2 << lvl, 2 << lvl, 8, generator=g) for lvl in range(levels)]
        return res
    r0, r1 = launch(3), launch(2)
    per_frame = [(r0, 0), (r0, 1), (r0, 2), (r1, 0), (r1, 1)]
    # inside one launch: views, and the back-references that let neighbouring splits be re-joined
    sp = take(per_frame, 1, 3)
    assert set(sp) == set(keys) | {"feats", "_src", "_i0", "_i1"}
    assert sp["_src"] is r0 and (sp["_i0"], sp["_i1"]) == (1, 3)
    for k in keys:
        assert sp[k].data_ptr() == r0[k][1:3].data_ptr() and sp[k].shape == r0[k][1:3].shape and torch.equal(sp[k], r0[k][1:3])
    assert len(sp["feats"]) == 2 and all(f.data_ptr() == s[1:3].data_ptr() and f.shape[0] == 2 for f, s in zip(sp["feats"], r0["feats"]))
    sp = take(per_frame, 3, 5)
    assert sp["_src"] is r1 and (sp["_i0"], sp["_i1"]) == (0, 2) and sp["k1"].data_ptr() == r1["k1"].data_ptr()
    # across both launches: the concatenation, per key and per level; nothing to re-join
    sp = take(per_frame, 1, 5)
    assert set(sp) == set(keys) | {"feats"}
    for k in keys:
        assert torch.equal(sp[k], torch.cat([r0[k][1:3], r1[k][0:2]]))
    assert len(sp["feats"]) == 2
    for lvl in range(2):
        assert torch.equal(sp["feats"][lvl], torch.cat([r0["feats"][lvl][1:3], r1["feats"][lvl][0:2]]))
    # the keyword form of the memory build: exactly those keys
    sp = take(per_frame, 2, 4, keys=("k1", "k2"), with_feats=False)
    assert set(sp) == {"k1", "k2"} and torch.equal(sp["k2"], torch.cat([r0["k2"][2:3], r1["k2"][0:1]]))
    assert set(take(per_frame, 0, 2, keys=("k1", "k2"), with_feats=False)) == {"k1", "k2", "_src", "_i0", "_i1"}
    # launches without feature maps: an empty list either way
    e0, e1 = launch(3, levels=0), launch(2, levels=0)
    empty = [(e0, 0), (e0, 1), (e0, 2), (e1, 0), (e1, 1)]
    assert take(empty, 0, 3)["feats"] == [] and take(empty, 2, 5)["feats"] == []


def test_gelu_erfc_form_matches_exact_gelu():
    """csrc/common.h gelu_erf: x * Phi(x) with Phi through erfc(z) = t exp(-z^2 + P(t)), restated here in float32 step by step (the
    coefficients are parsed from the header, so the test follows the kernel).  It must agree with nn.GELU's exact (erf) form -- the
    reference's Mlp activation, swintransformer.py:21-37 -- to well under an fp16 ulp of the fc1 output it produces."""
    src = open(os.path.join(ROOT, "diffusionvid_amd", "csrc", "common.h")).read()
    body = src[src.index("float gelu_erf(float x)"):src.index("float2v gelu_erf2(float2v x)")]
    coef = [float(c) for c in re.findall(r"(?:float p = |fmaf\(p, t, )(-?\d+\.\d+)f", body)]
    assert len(coef) == 10, coef
    f = np.float32
    x = np.concatenate([np.linspace(-12, 12, 400001), np.random.RandomState(0).randn(400000) * 2]).astype(f)
    z = (np.abs(x) * f(0.70710678118654752440)).astype(f)
    t = (f(1) / (f(0.5) * z + f(1))).astype(f)
    p = np.full_like(x, f(coef[0]))
    for c in coef[1:]:
        p = (p * t + f(c)).astype(f)
    e = (t * np.exp2(((p - z * z).astype(f) * f(1.4426950408889634)).astype(np.float64)).astype(f)).astype(f)
    phi = np.where(x >= 0, (f(1) - f(0.5) * e).astype(f), (f(0.5) * e).astype(f))
    got = (x * phi).astype(f)
    want = torch.nn.functional.gelu(torch.from_numpy(x).double()).numpy()
    err = np.abs(got - want)
    assert err.max() < 1e-6, err.max()
    big = np.abs(want) > 1e-6
    assert (err[big] / np.abs(want[big])).max() < 2e-5
    # after the fp16 store of the fc1 output: essentially always the exactly rounded value
    assert (got.astype(np.float16) != want.astype(np.float16)).mean() < 1e-3


def test_counted_dma_waits_cover_no_ordinary_load():
    """the fused-block and weight-stationary kernels count LDS-DMA pieces in hand-written vmcnt waits; an ordinary
    load among the youngest N operations of such a wait lets it return with a covered piece in flight.
    tools/check_dma_waits.py checks that on the compiled assembly of csrc/bneck.hip and csrc/wstat.hip; its rule is first
    checked on hand-made streams (the round-3 fault pattern must be flagged)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_dma_waits", os.path.join(ROOT, "tools", "check_dma_waits.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    piece, load = "\tglobal_load_lds_dwordx4 v[2:3], off", "\tglobal_load_dwordx4 v[4:7], v[2:3], off"
    stream = lambda *t: list(enumerate(t, 1))                                     # noqa: E731
    # round-3 fault: piece, then a younger ordinary load, wait allows one operation in flight -> the load may be the one that retired
    assert chk.check_kernel("k", stream(piece, load, "\ts_waitcnt vmcnt(1)"))
    assert not chk.check_kernel("k", stream(load, piece, piece, "\ts_waitcnt vmcnt(1)"))      # loads older than the pieces
    assert not chk.check_kernel("k", stream(piece, load, "\ts_waitcnt vmcnt(0)"))             # a full drain is always safe
    assert not chk.check_kernel("k", stream(piece, "\tglobal_store_dwordx4 v[2:3], v[4:7], off", piece, "\ts_waitcnt vmcnt(1)"))
    # loop-carried: the load issued at the end of the body is young at the next trip's wait
    loop = stream(".LBB0_1:", piece, "\ts_waitcnt vmcnt(2)", load, "\ts_cbranch_scc1 .LBB0_1")
    assert chk.check_kernel("k", loop)
    for f in ("bneck.hip", "wstat.hip"):
        stats, bad = chk.check_source(os.path.join(ROOT, "diffusionvid_amd", "csrc", f))
        assert len(stats) >= 9 and sum(c for _, c in stats.values()) >= 100
        assert not bad, bad[:3]
