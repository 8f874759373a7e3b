"""DiffusionDet.loss_gradients(through="tail") end to end on the GPU: a DTYPE float32 model (one bottleneck per ResNet stage, two heads, 100
boxes), two images of different sizes, DEEP_SUPERVISION on and off.  The last head's parameter gradients against torch's autograd through
tail.head_tail_host in float64 fed with the kept tail input and loss_gradients' own d_logits / d_boxes, under the bound of
_head_tail_cases; the default through="outputs" and detect_images keep their bits."""
import functools

import pytest
import torch

import _head_tail_cases as HC

pytestmark = pytest.mark.gpu

from diffusionvid_amd.modeling.roi_heads.box_head import tail as T  # noqa: E402

BLOCKS = (1, 1, 1, 1)
SMALL = ["MODEL.VID.MEGA.GLOBAL.ENABLE", False, "MODEL.VID.ROI_BOX_HEAD.ATTENTION.ENABLE", False, "MODEL.DiffusionDet.NUM_HEADS_LOCAL", 0,
         "MODEL.DiffusionDet.NUM_HEADS", 2, "MODEL.DiffusionDet.NUM_PROPOSALS", 100, "MODEL.DiffusionDet.NUM_CLASSES", 30]
IMAGE_HW = [(96, 160), (128, 96)]
IDS = [12, 40]
GT = [([[20.0, 10.0, 90.0, 70.0], [100.0, 30.0, 150.0, 90.0], [5.0, 50.0, 60.0, 95.0]], [3, 17, 30]), ([[30.0, 20.0, 80.0, 100.0]], [9])]
TAIL = ("linear1.", "linear2.", "norm3.", "block_time_mlp.", "cls_module.", "reg_module.", "class_logits.", "bboxes_delta.")
OWN = ("linear1.", "linear2.", "norm3.")          # complete for the last head only
LAST = "head.head_series.1."


@functools.lru_cache(maxsize=None)
def _model(deep):
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    cfg, model = E._build(1, BLOCKS, "trained_like", extra=SMALL + ["MODEL.DiffusionDet.DEEP_SUPERVISION", deep], dtype="float32")
    model.noise_fn = synthetic.noise_fn
    # keep the last head's tail off the ReLU kinks on THIS batch (_head_tail_cases.settle_off_kinks says why): its tail input and time_emb do
    # not depend on the biases that are moved, so one pass records them, the biases are settled on the host, and the model is loaded again
    first = model.loss_gradients(_images(), _targets(), IDS, through="tail")
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    settled = HC.settle_off_kinks(first["tail_in"][-1], first["time_emb"], {k[len(LAST):]: v for k, v in sd.items() if k.startswith(LAST) and k[len(LAST):].startswith(TAIL)})
    sd.update({LAST + k: v for k, v in settled.items()})
    model.load_state_dict(sd)
    return cfg, model


@functools.lru_cache(maxsize=None)
def _images():
    from diffusionvid_amd.utils import synthetic
    return [synthetic.synthetic_frame(50 + i, h, w, smooth=True) for i, (h, w) in enumerate(IMAGE_HW)]


def _targets():
    from diffusionvid_amd.structures.bounding_box import BoxList
    out = []
    for (boxes, labels), (h, w) in zip(GT, IMAGE_HW):
        t = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), (w, h), mode="xyxy")
        t.add_field("labels", torch.tensor(labels, dtype=torch.int64))
        out.append(t)
    return out


def _same_detections(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x.bbox, y.bbox) and all(torch.equal(x.get_field(k), y.get_field(k)) for k in ("scores", "labels"))


@pytest.mark.parametrize("deep", (True, False))
def test_tail_gradients_of_the_last_head_meet_autograd_on_the_host_path(deep):
    _, model = _model(deep)
    heads = [0, 1] if deep else [1]
    before = model.detect_images(_images(), IDS)
    plain = model.loss_gradients(_images(), _targets(), IDS)
    out = model.loss_gradients(_images(), _targets(), IDS, through="tail")
    again = model.loss_gradients(_images(), _targets(), IDS)
    # the default returns what it returned, and the new forward entry disturbs nothing
    for res in (again, (out["losses"], out["d_logits"], out["d_boxes"])):
        assert res[0] == plain[0] and torch.equal(res[1], plain[1]) and torch.equal(res[2], plain[2])
    _same_detections(before, model.detect_images(_images(), IDS))
    # the keys: complete gradients, the earlier heads' own-output terms apart
    sd = model.state_dict()
    want = {k for k in sd for h in heads if k.startswith("head.head_series.%d." % h) and k.split(".", 3)[3].startswith(TAIL)}
    partial = {k for k in want if k.startswith("head.head_series.0.") and k.split(".", 3)[3].startswith(OWN)}
    assert set(out["param_grads"]) == want - partial and set(out["partial"]) == partial and (len(partial) == 6) == deep
    assert all(v.shape == sd[k].shape and v.dtype == torch.float32 and v.is_cuda for k, v in {**out["param_grads"], **out["partial"]}.items())
    S, R = len(heads), 2 * 100
    assert tuple(out["d_tail_in"].shape) == (S, R, 256) == tuple(out["tail_in"].shape) and tuple(out["d_time_emb"].shape) == (2, 1024)
    assert tuple(out["boxes_in"].shape) == (S, 2, 100, 4) and not torch.equal(out["time_emb"][0], out["time_emb"][1]), "two images, two t"
    # the last head against torch's autograd through head_tail_host, fed with the kept tail input and loss_gradients' own cotangents
    pfx = LAST
    params = {k[len(pfx):]: v for k, v in sd.items() if k.startswith(pfx) and k[len(pfx):].startswith(TAIL)}
    cots = {"logits": out["d_logits"][-1].reshape(R, -1), "boxes": out["d_boxes"][-1].reshape(R, 4)}
    args = (T, out["tail_in"][-1], out["boxes_in"][-1].reshape(R, 4), out["time_emb"], params, None, cots)
    (t_out, truth), (_, yard) = HC.host_run(*args, torch.float64), HC.host_run(*args, torch.float32)
    failed = []
    for k in params:
        y, dev = HC.deviation(yard[k], truth[k]), HC.deviation(out["param_grads"][pfx + k], truth[k])
        print("deep %-5s %-26s max|truth| %.3e  yardstick %.3e  device %.3e  bound %.3e" % (deep, k, float(truth[k].abs().max()), y, dev, HC.bound(y)))
        if dev > HC.bound(y):
            failed.append((k, dev, HC.bound(y)))
    y, dev = HC.deviation(yard["x"], truth["x"]), HC.deviation(out["d_tail_in"][-1], truth["x"])
    print("deep %-5s %-26s yardstick %.3e  device %.3e  bound %.3e" % (deep, "d_tail_in (last head)", y, dev, HC.bound(y)))
    assert not failed and dev <= HC.bound(y), (failed, dev)
    if not deep:          # one kept head: d_time_emb is its own
        y, dev = HC.deviation(yard["time_emb"], truth["time_emb"]), HC.deviation(out["d_time_emb"], truth["time_emb"])
        assert dev <= HC.bound(y), (dev, y)
    assert not model.training and len(model._graphs) == 0


def test_a_float16_model_refuses_by_key():
    import test_gpu_e2e as E
    from diffusionvid_amd import _lib
    _, model = E._build(1, BLOCKS, "trained_like", extra=SMALL, dtype="float16")
    with pytest.raises(NotImplementedError, match="DTYPE float32"):
        model.loss_gradients(_images(), _targets(), IDS, through="tail")
    eng = model._get_engine()
    with pytest.raises(_lib.DvidError, match="keep_tail_input needs a DTYPE float32 model"):
        eng.rcnn_head(0, [], 32, 32, torch.zeros(1, 4, 4).cuda(), None, torch.zeros(1, dtype=torch.int64), keep_tail_input=True)
