"""DiffusionDet.loss_gradients(through="interact") end to end on the GPU, on the small DTYPE float32 model of test_gpu_head_tail_e2e (one
bottleneck per ResNet stage, two heads, 100 boxes, two images of different sizes): the tail's entries keep the bits of through="tail"; the
last head's twelve gradients and d_interact_in of both heads against torch's autograd in float64 through the host composition
head_tail_host(inst_interact_host(p, roi)) fed with the kept inputs and loss_gradients' own d_logits / d_boxes, under the bound of
_inst_interact_cases; the kept inputs are what a recompute starts from; the other paths keep their bits."""
import functools

import pytest
import torch

import _head_tail_cases as HC
import _inst_interact_cases as IC
from test_gpu_head_tail_e2e import BLOCKS, IDS, SMALL, TAIL, _images, _same_detections, _targets

pytestmark = pytest.mark.gpu

from diffusionvid_amd import ops  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import interact as I  # noqa: E402
from diffusionvid_amd.modeling.roi_heads.box_head import tail as T  # noqa: E402

R = 2 * 100


def _head_params(sd, head, names):
    pfx = "head.head_series.%d." % head
    return {k[len(pfx):]: v for k, v in sd.items() if k.startswith(pfx) and names(k[len(pfx):])}


@functools.lru_cache(maxsize=None)
def _model():
    """DEEP_SUPERVISION on; both heads kept off the ReLU kinks on THIS batch (_inst_interact_cases.settle_off_kinks says why), front to back:
    a head's interaction inputs do not depend on the biases moved in it or behind it, its tail input only on its interaction's"""
    import test_gpu_e2e as E
    from diffusionvid_amd.utils import synthetic
    cfg, model = E._build(1, BLOCKS, "trained_like", extra=SMALL + ["MODEL.DiffusionDet.DEEP_SUPERVISION", True], dtype="float32")
    model.noise_fn = synthetic.noise_fn
    for head in (0, 1):          # one pass per head: the tail is settled on the host composition's own tail input, the float64 y of the settled link
        first = model.loss_gradients(_images(), _targets(), IDS, through="interact")
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        p, roi = first["interact_in"][head].cpu(), first["roi_tiles"][head].cpu()
        settled = IC.settle_off_kinks(p, roi, _head_params(sd, head, lambda k: k in I.PARAM_NAMES))
        y = I.inst_interact_host(p.double(), roi.double(), {k: v.double() for k, v in settled.items()})
        settled.update(HC.settle_off_kinks(y, first["time_emb"], _head_params(sd, head, lambda k: k.startswith(TAIL))))
        sd.update({"head.head_series.%d.%s" % (head, k): v for k, v in settled.items()})
        model.load_state_dict(sd)
    return cfg, model


def _host(out, sd, head, dtype):
    """torch's autograd through the host composition of head `head` on the kept inputs -> {p, <the twelve>: gradient}"""
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)
    cpu = lambda t: t.detach().cpu().to(dtype)
    wi = {k: leaf(v) for k, v in _head_params(sd, head, lambda k: k in I.PARAM_NAMES).items()}
    wt = {k: cpu(v) for k, v in _head_params(sd, head, lambda k: k.startswith(TAIL)).items()}
    p = leaf(out["interact_in"][head])
    y = I.inst_interact_host(p, cpu(out["roi_tiles"][head]), wi)
    logits, boxes, _ = T.head_tail_host(y, cpu(out["boxes_in"][head]).reshape(R, 4), cpu(out["time_emb"]), wt)
    ((cpu(out["d_logits"][head]).reshape(R, -1) * logits).sum() + (cpu(out["d_boxes"][head]).reshape(R, 4) * boxes).sum()).backward()
    return {"p": p.grad, **{k: v.grad for k, v in wi.items()}}


def test_interact_keeps_the_tails_bits_and_meets_autograd_on_the_host_composition():
    _, model = _model()
    before = model.detect_images(_images(), IDS)
    plain = model.loss_gradients(_images(), _targets(), IDS)
    tail = model.loss_gradients(_images(), _targets(), IDS, through="tail")
    out = model.loss_gradients(_images(), _targets(), IDS, through="interact")
    with_roi = model.loss_gradients(_images(), _targets(), IDS, through="interact", roi_gradients=True)
    # through="outputs", through="tail" and detect_images keep their bits; through="interact" returns the tail's entries bit-equal
    assert out["losses"] == tail["losses"] == plain[0] and torch.equal(tail["d_logits"], plain[1]) and torch.equal(tail["d_boxes"], plain[2])
    for k in ("d_logits", "d_boxes", "d_tail_in", "d_time_emb", "tail_in", "boxes_in", "time_emb"):
        assert torch.equal(out[k], tail[k]), k
    for kind in ("param_grads", "partial"):
        assert set(tail[kind]) <= set(out[kind]) and all(torch.equal(out[kind][k], v) for k, v in tail[kind].items()), kind
    _same_detections(before, model.detect_images(_images(), IDS))
    # the keys: the twelve of the last head are complete, those of the earlier head are partial
    sd = model.state_dict()
    twelve = lambda h: {"head.head_series.%d.%s" % (h, k) for k in I.PARAM_NAMES}
    assert set(out["param_grads"]) - set(tail["param_grads"]) == twelve(1) and set(out["partial"]) - set(tail["partial"]) == twelve(0)
    assert all(v.shape == sd[k].shape and v.dtype == torch.float32 and v.is_cuda for k, v in {**out["param_grads"], **out["partial"]}.items())
    assert tuple(out["d_interact_in"].shape) == (2, R, 256) == tuple(out["interact_in"].shape) and tuple(out["roi_tiles"].shape) == (2, R, 49, 256)
    assert "d_roi" not in out and tuple(with_roi["d_roi"].shape) == (2, R, 49, 256)
    assert all(torch.equal(with_roi[k], out[k]) for k in ("d_interact_in", "interact_in", "roi_tiles"))
    assert all(torch.equal(with_roi["param_grads"][k], v) for k, v in out["param_grads"].items())
    # the host composition in float64 is the truth, its fp32 run the yardstick
    failed = []
    for head in (0, 1):
        truth, yard = _host(out, sd, head, torch.float64), _host(out, sd, head, torch.float32)
        got = {"p": out["d_interact_in"][head]}
        if head == 1:
            got.update({k: out["param_grads"]["head.head_series.1." + k] for k in I.PARAM_NAMES})
        for k in got:
            y, dev = IC.deviation(yard[k], truth[k]), IC.deviation(got[k], truth[k])
            print("head %d %-36s max|truth| %.3e  yardstick %.3e  device %.3e  bound %.3e" % (head, "d_interact_in" if k == "p" else k,
                                                                                            float(truth[k].abs().max()), y, dev, IC.bound(y)))
            if dev > IC.bound(y):
                failed.append((head, k, dev, IC.bound(y)))
    assert not failed, failed
    assert not model.training and len(model._graphs) == 0


def test_the_kept_inputs_are_what_a_recompute_starts_from():
    _, model = _model()
    out = model.loss_gradients(_images(), _targets(), IDS, through="interact")
    sd = model.state_dict()
    for head in (0, 1):
        w = {k: v.cuda() for k, v in _head_params(sd, head, lambda k: k in I.PARAM_NAMES).items()}
        fwd = ops.inst_interact_backward(out["interact_in"][head], out["roi_tiles"][head], w, forward_only=True)
        # the fp32 recompute on the exact MFMA against the head pass's own norm2 output (split fp16 operands): close, not equal
        assert IC.deviation(fwd["y"], out["tail_in"][head]) < 1e-4
    # the tiles are the fp32 RoIAlign of the same pyramid and boxes
    eng = model._get_engine()
    canvas = model.stills.admit("loss_gradients", _images())[0].tensors.cuda().float().contiguous()
    with torch.no_grad(), model._on_device():
        (a, b, feats), = list(model.stills.chunks(canvas))
        h, w = canvas.shape[-2:]
        for head in (0, 1):
            tiles = ops.roialign_f32(model.head._as_nhwc(feats, eng), out["boxes_in"][head], h, w)
            assert torch.equal(tiles.reshape(R, 49, 256), out["roi_tiles"][head]), head


def test_a_float16_model_refuses_by_key():
    import test_gpu_e2e as E
    from diffusionvid_amd import _lib
    _, model = E._build(1, BLOCKS, "trained_like", extra=SMALL, dtype="float16")
    with pytest.raises(NotImplementedError, match="through='interact' needs DTYPE float32"):
        model.loss_gradients(_images(), _targets(), IDS, through="interact")
    eng = model._get_engine()
    with pytest.raises(_lib.DvidError, match="keep_interact_input needs a DTYPE float32 model"):
        eng.rcnn_head(0, [], 32, 32, torch.zeros(1, 4, 4).cuda(), None, torch.zeros(1, dtype=torch.int64), keep_interact_input=True)
