"""Still images, each with its own size, on the host side: the restatement the GPU tests compare against (tests/_still_ref.py) pinned to
itself (batch against singles) and to the oracle's video state machine (equal sizes), the detector's refusals and routing, the
orientation sampler, the result writer, the size-table check and the C ABI surface.  No GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import _still_ref as S
from oracle import detector as odet, head as ohead

BASE = os.path.join(ROOT, "configs", "BASE_RCNN_1gpu.yaml")
R101_YAML = os.path.join(ROOT, "configs", "vid_R_101_DiffusionVID.yaml")
BASELINE = ["MODEL.VID.MEGA.GLOBAL.ENABLE", False, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", False, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 0]
SIZES_SYMBOLS = {"dvid_noise_to_boxes_sizes": 7, "dvid_ddim_renew_step_sizes": 18, "dvid_postproc_topk_nms_sizes": 15, "dvid_nms_frames_tiled_sizes": 15}
BLOCKS, M, C, HEADS = (1, 1, 1, 1), 40, 30, 2

# The same fp32 operations on a batch and on one of its images may be summed in another order by the CPU's convolution and GEMM
# libraries (their blocking depends on the batch size): values of O(100) px / O(1) score move by a few ulp, 1e-5 relative.  Boxes are
# compared within 1e-2 px, scores within 1e-5: ~100 x that noise, and far below anything the size table could change (a wrong row moves
# a box by the ratio of two image sizes).
BOX_TOL, SCORE_TOL = 1e-2, 1e-5


def _sd():
    from diffusionvid_amd.utils import synthetic
    sd = synthetic.make_state_dict(0, blocks=BLOCKS, num_classes=C, num_heads=HEADS, num_heads_cond=0)
    return synthetic.trained_like_scores(synthetic.tame_box_deltas(sd, 0.1))


def _ocfg(sample_step, interval=8):
    hc = ohead.HeadCfg(num_classes=C, num_heads=HEADS, num_heads_local=0, top_k=(min(75, M), min(25, M)), sampling_timesteps=sample_step)
    return odet.DetCfg(num_proposals=M, num_classes=C, sample_step=sample_step, blocks=BLOCKS, head=hc, infer_batch=interval, all_frame_interval=interval)


def _images(sizes_hw):
    from diffusionvid_amd.utils import synthetic
    return [synthetic.synthetic_frame(7 + i, h, w, smooth=True) for i, (h, w) in enumerate(sizes_hw)]


def _same(a, b, what):
    assert len(a["scores"]) == len(b["scores"]) > 0, (what, len(a["scores"]), len(b["scores"]))
    assert np.array_equal(a["labels"], b["labels"]), what
    assert np.abs(a["boxes"] - b["boxes"]).max() <= BOX_TOL and np.abs(a["scores"] - b["scores"]).max() <= SCORE_TOL, what


@pytest.fixture(scope="module")
def sd():
    return _sd()


@pytest.mark.parametrize("sample_step", [1, 3])
def test_restatement_mixed_batch_equals_each_image_alone(sd, sample_step):
    from diffusionvid_amd.utils import synthetic
    sizes = [(48, 96), (64, 40), (33, 50)]
    canvas, got_sizes = S.canvas_of(_images(sizes))
    assert tuple(canvas.shape) == (3, 3, 64, 96) and got_sizes == sizes
    cfg = _ocfg(sample_step)
    with torch.no_grad():
        mixed = S.detect_images(sd, cfg, synthetic.noise_fn, canvas, sizes, image_ids=[5, 9, 2])
        for i, image_id in enumerate([5, 9, 2]):
            alone = S.detect_images(sd, cfg, synthetic.noise_fn, canvas[i:i + 1], sizes[i:i + 1], image_ids=[image_id])[0]
            _same(mixed[i], alone, (sample_step, i))
            w, h = sizes[i][1], sizes[i][0]
            assert mixed[i]["boxes"][:, [0, 2]].max() <= w - 1 and mixed[i]["boxes"][:, [1, 3]].max() <= h - 1
    # the sizes matter: image 1 run with image 0's size is another answer
    with torch.no_grad():
        wrong = S.detect_images(sd, cfg, synthetic.noise_fn, canvas[1:2], sizes[0:1], image_ids=[9])[0]
    assert len(wrong["scores"]) != len(mixed[1]["scores"]) or np.abs(wrong["boxes"] - mixed[1]["boxes"]).max() > 1.0


@pytest.mark.parametrize("sample_step", [1, 3])
def test_restatement_equals_the_oracle_state_machine_on_equal_sizes(sd, sample_step):
    """three images of one size = one three-frame video of the baseline configuration (no attention), draws mapped image -> frame"""
    from diffusionvid_amd.utils import synthetic
    sizes = [(60, 90)] * 3
    canvas, _ = S.canvas_of(_images(sizes))
    cfg = _ocfg(sample_step, interval=3)
    oracle = S.BaselineOracleDet(sd, cfg, S.video_noise_fn(synthetic.noise_fn))
    item = {"cur": canvas[0:1], "image_size": sizes[0], "ref_l": [canvas[i:i + 1] for i in range(3)], "ref_g": [], "frame_category": 0,
            "frame_id": 0, "start_id": 0, "end_id": 2, "seg_len": 3, "last_queue_id": 2}
    with torch.no_grad():
        ref = oracle.forward(item)
        got = S.detect_images(sd, cfg, synthetic.noise_fn, canvas, sizes)
    assert len(ref) == len(got) == 3
    for i in range(3):
        _same(ref[i], got[i], (sample_step, i))


def _model(opts=()):
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector.diffusion_det import DiffusionDet
    cfg = get_cfg(R101_YAML, list(opts), BASE)
    cfg.MODEL.RESNETS.BLOCKS_OVERRIDE = BLOCKS
    return DiffusionDet(cfg).eval()


REFUSED = [
    (["MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", False, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 0], "GLOBAL.ENABLE"),
    (["MODEL.VID.MEGA.GLOBAL.ENABLE", False, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", True, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 0], "ATTENTION.ENABLE"),
    (["MODEL.VID.MEGA.GLOBAL.ENABLE", False, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", False, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 1], "NUM_HEADS_LOCAL"),
]


@pytest.mark.parametrize("opts,key", REFUSED)
def test_detect_images_refuses_models_with_attention(opts, key):
    model = _model(opts)
    with pytest.raises(NotImplementedError) as e:
        model.detect_images([torch.zeros(3, 32, 32)])
    assert key in str(e.value), str(e.value)
    assert model._engine is None          # refused before anything was built or launched


DIFFUSION_BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                     "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
                     "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")          # diffusion_det.py:222-267


def _call(model, entry):
    if entry == "detect_images":
        return model.detect_images([torch.zeros(3, 32, 32)])
    if entry == "detect_images_aug":
        return model.detect_images_aug([np.zeros((32, 32, 3), dtype=np.uint8)])
    target = _boxlist([[4, 4, 20, 20]], (32, 32), [1.0], [1])
    return getattr(model, entry)([torch.zeros(3, 32, 32)], [target])


@pytest.mark.parametrize("entry", ["detect_images", "detect_images_aug", "compute_losses", "loss_gradients"])
@pytest.mark.parametrize("opts,key", REFUSED)
def test_one_admission_refuses_for_every_still_entry_point(entry, opts, key):
    """the refusals of a still batch are written once (StillImages.admit's) and carry the entry point's name; the two objects that took the
    still and loss paths out of the detector are no modules, so the checkpoint's keys are the ones __init__ registers"""
    from torch import nn
    from diffusionvid_amd.modeling.detector.objective import Objective
    from diffusionvid_amd.modeling.detector.stills import StillImages
    from diffusionvid_amd.utils import synthetic
    aug = ["TEST.BBOX_AUG.ENABLED", True] if entry == "detect_images_aug" else []
    model = _model(list(opts) + aug)
    with pytest.raises(NotImplementedError) as e:
        _call(model, entry)
    assert str(e.value).startswith(entry + ":") and key in str(e.value), str(e.value)
    assert model._engine is None          # refused before anything was built or launched
    assert type(model.stills) is StillImages and type(model.objective) is Objective
    assert not isinstance(model.stills, nn.Module) and not isinstance(model.objective, nn.Module)
    base = _model(BASELINE + aug)
    d = base.cfg.MODEL.DiffusionDet
    want = synthetic.make_state_dict(0, blocks=BLOCKS, hidden=d.HIDDEN_DIM, nheads=d.NHEADS, dim_ff=d.DIM_FEEDFORWARD, dim_dynamic=d.DIM_DYNAMIC,
                                     num_classes=d.NUM_CLASSES, num_cls=d.NUM_CLS, num_reg=d.NUM_REG, num_heads=d.NUM_HEADS, num_heads_cond=0,
                                     pooler=base.cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION, prior_prob=d.PRIOR_PROB, local_stages=0, fpn_levels=base.fpn_levels)
    assert set(base.state_dict()) == set(want) | set(DIFFUSION_BUFFERS)


def test_detect_images_checks_its_arguments():
    model = _model(BASELINE)
    with pytest.raises(ValueError, match="image_ids"):
        model.detect_images([torch.zeros(3, 32, 32), torch.zeros(3, 20, 32)], image_ids=[1])
    from diffusionvid_amd.structures.image_list import ImageList
    with pytest.raises(ValueError, match="multiples of 32"):
        model.detect_images(ImageList(torch.zeros(1, 3, 40, 64), [(40, 64)]))
    with pytest.raises(ValueError, match="image_sizes"):
        model.detect_images(ImageList(torch.zeros(1, 3, 32, 64), [(40, 64)]))
    assert model.detect_images(ImageList(torch.zeros(0, 3, 32, 64), [])) == []
    assert model._engine is None


def test_forward_routes_anything_but_a_dict_to_detect_images(monkeypatch):
    model = _model(BASELINE)
    seen = []
    monkeypatch.setattr(model, "detect_images", lambda images, image_ids=None: seen.append(images) or ["routed"])
    batch = [torch.zeros(3, 32, 32)]
    assert model(batch) == ["routed"] and seen[0] is batch
    with pytest.raises(ValueError):
        model(batch, targets=[None])
    # a dict still takes the video path: it fails on the missing protocol keys, not in detect_images
    with pytest.raises(KeyError):
        model({"ref_l": []})
    assert len(seen) == 1


def test_detect_images_leaves_the_video_state_alone(monkeypatch):
    """everything the video path keeps between calls, before and after a (stubbed-out) still call"""
    model = _model(BASELINE)
    model._reset_video()
    state = ("queue", "local_img_queue", "_ahead", "_results_ahead", "video_index", "_graphs", "_graph_seen", "_graph_generation", "graph_replays")
    before = {k: (id(getattr(model, k)), repr(getattr(model, k))) for k in state}
    head_before = (list(model.head.proposal_feats_global), list(model.head.proposal_feats_local), list(model.head.proposals_feat_cur))
    monkeypatch.setattr(model.stills, "_detect", lambda canvas, sizes_wh, ids, cls: [(tuple(canvas.shape), sizes_wh, ids)])
    out = model.detect_images([torch.zeros(3, 40, 70), torch.zeros(3, 64, 30)], image_ids=[11, 4])
    assert out == [((2, 3, 64, 96), [(70, 40), (30, 64)], [11, 4])]
    assert before == {k: (id(getattr(model, k)), repr(getattr(model, k))) for k in state}
    assert head_before == (list(model.head.proposal_feats_global), list(model.head.proposal_feats_local), list(model.head.proposals_feat_cur))


def test_orientation_sampler_groups_wide_and_tall():
    from diffusionvid_amd.data.datasets import still
    sizes = [(1216, 800), (800, 1088), (1333, 800), (800, 1200), (1000, 800), (800, 800), (640, 1333)]
    batches = still.orientation_batches(sizes, 2)
    assert batches == [[0, 2], [4, 5], [1, 3], [6]]
    assert sorted(i for b in batches for i in b) == list(range(len(sizes)))
    for b in batches:
        assert len({sizes[i][0] >= sizes[i][1] for i in b}) == 1
    assert list(still.OrientationBatchSampler(sizes, 2)) == batches and len(still.OrientationBatchSampler(sizes, 4)) == 2
    # one canvas for all against a canvas per orientation
    mixed, grouped = still.padding_share(sizes, [list(range(len(sizes)))]), still.padding_share(sizes, still.orientation_batches(sizes, 8))
    assert 0 < grouped < mixed < 1


def test_still_dataset_and_collate():
    from diffusionvid_amd.data.datasets import still
    from diffusionvid_amd.data import transforms
    rng = np.random.RandomState(0)
    raws = {"a": rng.randint(0, 255, (30, 50, 3), dtype=np.uint8), "b": rng.randint(0, 255, (60, 24, 3), dtype=np.uint8)}
    ds = still.StillImageDataset(["a", "b"], loader=raws.__getitem__, image_ids=[7, 3], min_size=32, max_size=64)
    assert len(ds) == 2 and ds.original_size(1) == (24, 60) and ds.resized_size(0) == (53, 32)
    img, image_id, size = ds[0]
    assert tuple(img.shape) == (3, 32, 53) and image_id == 7 and size == (50, 30)
    assert torch.equal(img, torch.from_numpy(transforms.resize_u8_numpy(raws["a"], (32, 53))).permute(2, 0, 1).float().div(255))
    got = list(still.batches(ds, 8))
    assert [b[1] for b in got] == [[7], [3]]          # wide and tall in batches of their own
    images, ids, sizes = got[1]
    assert tuple(images.tensors.shape) == (1, 3, 96, 32) and [tuple(s) for s in images.image_sizes] == [(65, 26)] and sizes == [(24, 60)]


def _boxlist(boxes, size, scores, labels):
    from diffusionvid_amd.structures.bounding_box import BoxList
    bl = BoxList(torch.tensor(boxes, dtype=torch.float32), size, mode="xyxy")
    bl.add_field("scores", torch.tensor(scores, dtype=torch.float32))
    bl.add_field("labels", torch.tensor(labels, dtype=torch.int64))
    return bl


def test_coco_result_writer(tmp_path):
    from diffusionvid_amd.engine import inference as inf
    preds = {9: _boxlist([[10, 20, 30, 60], [0, 0, 5, 5]], (100, 80), [0.75, 0.25], [2, 1]), 4: _boxlist([[1, 2, 4, 8]], (50, 50), [0.5], [3])}
    path = str(tmp_path / "res.json")
    inf.write_coco_results(preds, path, label_map={1: 1, 2: 3, 3: 90})
    with open(path) as f:
        res = json.load(f)
    assert res == [{"image_id": 4, "category_id": 90, "bbox": [1.0, 2.0, 3.0, 6.0], "score": 0.5},
                   {"image_id": 9, "category_id": 3, "bbox": [10.0, 20.0, 20.0, 40.0], "score": 0.75},
                   {"image_id": 9, "category_id": 1, "bbox": [0.0, 0.0, 5.0, 5.0], "score": 0.25}]
    assert [r["category_id"] for r in inf.coco_results(preds)] == [3, 2, 1]
    assert [r["category_id"] for r in inf.coco_results(preds, lambda l: l + 100)] == [103, 102, 101]


def test_inference_images_maps_back_to_the_original_size(tmp_path):
    from diffusionvid_amd.engine import inference as inf

    class Model:
        calls = []

        def detect_images(self, images, image_ids=None):
            self.calls.append(list(image_ids))
            return [_boxlist([[10, 20, 30, 40]], (100, 50), [0.5], [1]) for _ in image_ids]

    loader = [("batch0", [3, 8], [(200, 100), (50, 25)]), ("batch1", [5], [(100, 50)])]
    model = Model()
    preds = inf.inference_images(model, loader, output_folder=str(tmp_path), label_map={1: 17})
    assert model.calls == [[3, 8], [5]] and sorted(preds) == [3, 5, 8]
    assert preds[3].size == (200, 100) and preds[3].bbox.tolist() == [[20.0, 40.0, 60.0, 80.0]]
    assert preds[8].size == (50, 25) and preds[8].bbox.tolist() == [[5.0, 10.0, 15.0, 20.0]]
    saved = torch.load(str(tmp_path / "predictions.pth"), weights_only=False)
    assert sorted(saved) == [3, 5, 8] and torch.equal(saved[5].bbox, preds[5].bbox)
    with open(str(tmp_path / "coco_results.json")) as f:
        res = json.load(f)
    assert [r["image_id"] for r in res] == [3, 5, 8] and res[0]["category_id"] == 17 and res[0]["bbox"] == [20.0, 40.0, 40.0, 40.0]
    with pytest.raises(ValueError, match="twice"):
        inf.inference_images(model, [("b", [1], [(1, 1)]), ("b", [1], [(1, 1)])])


def test_size_table_is_checked_on_the_host():
    from diffusionvid_amd import ops
    fs = ops.FrameSizes(torch.tensor([[64., 48.], [40., 64.], [33., 17.]]), "cpu")
    assert len(fs) == 3 and fs.host.dtype == torch.float32 and fs[1:3].host.tolist() == [[40., 64.], [33., 17.]] and len(fs[1:3]) == 2
    assert ops.frame_sizes(fs, 3, "cpu") is fs.dev
    for bad in ([[64., 0.]], [[64., -1.]], [[float("nan"), 3.]], [[float("inf"), 3.]], [64., 48.], [[1., 2., 3.]]):
        with pytest.raises(ops._lib.DvidError):
            ops.FrameSizes(torch.tensor(bad), "cpu")
    with pytest.raises(ops._lib.DvidError, match="3 rows for 2 frames"):
        ops.frame_sizes(fs, 2, "cpu")


def test_device_noise_draws_a_batch_of_consecutive_ids_in_one_launch(monkeypatch):
    from diffusionvid_amd import ops
    from diffusionvid_amd.utils import synthetic
    from oracle import noise as onoise
    calls = []

    def fake(key0, n_images, shape, device=None, key_stride=1):
        calls.append((key0, n_images, key_stride))
        return torch.zeros((n_images,) + tuple(shape))
    monkeypatch.setattr(ops, "counter_normal", fake)
    dn = synthetic.DeviceNoise()
    stride = onoise.draw_key("ddim", 6, 2, 0) - onoise.draw_key("ddim", 5, 2, 0)
    assert dn.draw_ids("ddim", [5, 6, 7, 8], 2, (40, 4)).shape == (4, 40, 4)
    assert calls == [(onoise.draw_key("ddim", 5, 2, 0), 4, stride)]          # image i of the launch is keyed as image id 5 + i
    calls.clear()
    assert dn.draw_ids("img", [12, 3, 4, 40], 0, (40, 4)).shape == (4, 40, 4)
    assert [(c[0], c[1]) for c in calls] == [(onoise.draw_key("img", 12, 0, 0), 1), (onoise.draw_key("img", 3, 0, 0), 2), (onoise.draw_key("img", 40, 0, 0), 1)]


def test_header_binding_and_library_carry_the_sizes_entry_points():
    from diffusionvid_amd import _lib
    lib = _lib.load()
    raw = open(os.path.join(ROOT, "include", "dvid_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, nargs in SIZES_SYMBOLS.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert decl, f"{name} is not declared in include/dvid_hip.h"
        assert "const float* sizes" in decl.group(1) and "img_w" not in decl.group(1), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
        sibling = re.search(r"\b%s\s*\(([^)]*)\)" % name[:-len("_sizes")], txt)
        # the sibling's arguments with `sizes` where img_w, img_h stood (noise_to_boxes also gains m)
        assert len(sibling.group(1).split(",")) == nargs + 1 - (name == "dvid_noise_to_boxes_sizes"), name
        assert getattr(lib, name) is not None
    assert "positive and finite" in raw and "[n_frames][2]" in raw
    assert re.search(r"\bdvid_counter_normal_strided\s*\(", txt) and len(_lib.SIGNATURES["dvid_counter_normal_strided"][1]) == 6 and lib.dvid_counter_normal_strided
    assert lib.dvid_version() >= 3
