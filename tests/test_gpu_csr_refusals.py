"""The start tables of the ragged inputs (gt_starts, video_starts, LVIS' neg_starts / nex_starts) are checked on the host by one helper of
csrc/ops_abi.hip before anything is launched: a table that does not begin at 0, or that decreases, is refused with the entry's name, the
table's name and the place, and the outputs stay as they were.  Every op here is first called with the smallest valid input (2 images,
4 rows, 2 classes, 1 box per image), so that a refusal is the table's doing."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

N, CAP, K = 2, 4, 2
GOOD = [0, 1, 2]
AT_ONE = [1, 1, 2]          # ends at 2 boxes
DECREASES = [0, 2, 1]       # ends at 1 box; the step down is at unit 1
FILL = 77


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _dets():
    d = torch.zeros((N, CAP, 6), dtype=torch.float32, device="cuda")
    d[:, 0] = torch.tensor([2.0, 3.0, 20.0, 30.0, 0.9, 1.0])
    return d, _i32([1, 1])


def _filled(*specs):
    return tuple(torch.full(shape, FILL, dtype=dtype, device="cuda") for shape, dtype in specs)


def _match_out():
    return _filled(((4, 10, N, CAP), torch.int8), ((4, 10, N, CAP), torch.int8), ((N, CAP), torch.int32), ((4, K + 1), torch.int32))


def _xywh(g):
    return torch.tensor([[2.0, 3.0, 18.0, 27.0]] * g, dtype=torch.float64, device="cuda").reshape(-1, 4)


def _vid(starts):
    from diffusionvid_amd import ops
    g = starts[-1]
    out = _filled(((1, N, CAP), torch.int8), ((1, N, CAP), torch.float64), ((N, CAP), torch.int32), ((1, K + 1), torch.float64), ((N,), torch.int32),
                  ((N,), torch.int8))
    boxes = torch.tensor([[2.0, 3.0, 20.0, 30.0]] * g, dtype=torch.float32, device="cuda").reshape(-1, 4)
    return (lambda: ops.vid_eval_match(*_dets(), boxes, _i32([1] * g), _i32(starts), K, out=out)), out


def _coco(starts):
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.evaluation import coco_eval
    g = starts[-1]
    out = _match_out()
    return (lambda: ops.coco_eval_match(*_dets(), _xywh(g), torch.full((g,), 486.0, dtype=torch.float64, device="cuda"),
                                        torch.zeros((g,), dtype=torch.uint8, device="cuda"), _i32([1] * g), _i32(starts), K, coco_eval.IOU_THRS,
                                        coco_eval.AREA_RANGES, out=out)), out


def _lvis(starts, neg=(0, 0, 0), nex=(0, 0, 0)):
    from diffusionvid_amd import ops
    from diffusionvid_amd.data.evaluation import coco_eval
    g = starts[-1]
    out = _match_out()
    return (lambda: ops.lvis_eval_match(*_dets(), _xywh(g), torch.full((g,), 486.0, dtype=torch.float64, device="cuda"),
                                        torch.zeros((g,), dtype=torch.uint8, device="cuda"), _i32([1] * g), _i32(starts), _i32(list(neg)),
                                        _i32([2] * neg[-1]), _i32(list(nex)), _i32([2] * nex[-1]), K, coco_eval.IOU_THRS, coco_eval.AREA_RANGES,
                                        out=out)), out


def _criterion_inputs(g):
    gen = torch.Generator().manual_seed(5)
    logits = torch.randn((1, N, CAP, K), generator=gen).cuda()
    boxes = torch.tensor([10.0, 10.0, 60.0, 50.0], device="cuda").expand(1, N, CAP, 4).contiguous() + torch.arange(CAP, device="cuda")[None, None, :, None]
    gt_boxes = torch.tensor([[12.0, 11.0, 58.0, 52.0]] * g, dtype=torch.float32, device="cuda").reshape(-1, 4)
    sizes = torch.tensor([[100.0, 80.0]] * N, device="cuda")
    return logits, boxes, gt_boxes, _i32([1] * g), sizes


def _criterion(starts):
    from diffusionvid_amd import ops
    logits, boxes, gt_boxes, gt_labels, sizes = _criterion_inputs(starts[-1])
    out = _filled(((1, N, CAP), torch.int32), ((1, N, 2), torch.int32), ((1, N, 4), torch.float64), ((1, N), torch.int32))
    return (lambda: ops.set_criterion(logits, boxes, gt_boxes, gt_labels, starts, sizes, 0.25, 2.0, 1, 2.0, 5.0, 2.0, out=out, gmax=2)), out


def _criterion_backward(starts):
    from diffusionvid_amd import ops
    logits, boxes, gt_boxes, gt_labels, sizes = _criterion_inputs(starts[-1])
    assign = torch.full((1, N, CAP), -1, dtype=torch.int32, device="cuda")
    assign[:, :, 0] = 0
    status = torch.zeros((1, N), dtype=torch.int32, device="cuda")
    coef = torch.ones((1, 3), dtype=torch.float64, device="cuda")
    out = _filled(((1, N, CAP, K), torch.float32), ((1, N, CAP, 4), torch.float32))
    return (lambda: ops.set_criterion_backward(logits, boxes, gt_boxes, gt_labels, starts, sizes, 0.25, 2.0, assign, status, coef, out=out)), out


def _q_sample(starts):
    from diffusionvid_amd import ops
    g = starts[-1]
    gen = torch.Generator().manual_seed(6)
    noise, placeholder = torch.randn((N, CAP, 4), generator=gen).cuda(), torch.randn((N, CAP, 4), generator=gen).cuda()
    gt = torch.tensor([[0.5, 0.5, 0.2, 0.3]] * g, dtype=torch.float32, device="cuda").reshape(-1, 4)
    sa = torch.linspace(0.99, 0.1, 8, device="cuda")
    return (lambda: ops.q_sample_boxes(gt, starts, [3, 5], sa, (1 - sa * sa).sqrt(), noise, placeholder, 2.0, torch.tensor([[100.0, 80.0]] * N))), ()


def _seq_nms(starts):
    from diffusionvid_amd import ops
    return (lambda: ops.seq_nms_video(*_dets(), K, video_starts=starts)), ()


# op, its entry's name in the messages, the table's name, the unit, the builder; a builder takes the table and returns (call, outputs)
OPS = {
    "vid_eval_match": ("VID evaluation", "gt_starts", "frame", _vid),
    "coco_eval_match": ("COCO evaluation", "gt_starts", "image", _coco),
    "lvis_eval_match": ("LVIS evaluation", "gt_starts", "image", _lvis),
    "lvis_eval_match neg": ("LVIS evaluation", "neg_starts", "image", lambda starts: _lvis(GOOD, neg=starts)),
    "lvis_eval_match nex": ("LVIS evaluation", "nex_starts", "image", lambda starts: _lvis(GOOD, nex=starts)),
    "set_criterion": ("set criterion", "gt_starts", "image", _criterion),
    "set_criterion_backward": ("set criterion backward", "gt_starts", "image", _criterion_backward),
    "q_sample_boxes": ("q_sample_boxes", "gt_starts", "image", _q_sample),
    # a video's frames must exist for the host's scratch plan, so the step down lies between two whole videos: 0..2, 2..1, 1..2
    "seq_nms_video": ("Seq-NMS", "video_starts", "video", lambda starts: _seq_nms([0, 2, 1, 2] if starts is DECREASES else starts)),
}


@pytest.mark.parametrize("op", sorted(OPS))
def test_a_bad_start_table_is_refused_before_the_launch(op):
    from diffusionvid_amd._lib import DvidError
    entry, table, unit, build = OPS[op]
    build(GOOD)[0]()          # the smallest valid call runs
    for starts, text in ((AT_ONE, "%s: %s[0] is 1, not 0" % (entry, table)), (DECREASES, "%s: %s decreases at %s 1" % (entry, table, unit))):
        call, out = build(starts)
        with pytest.raises(DvidError, match=re.escape(text) + "$"):
            call()
        torch.cuda.synchronize()
        assert all(bool((o == FILL).all()) for o in out), text
