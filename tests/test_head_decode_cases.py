"""The preconditions of tests/test_gpu_head_decode.py, on the oracle alone: the inputs of tests/_head_decode_cases.py really reach the scale
clamp, really carry an invalid box where the flag tests put one, really give the frames of a launch different scale / shift rows and
really open a second slab of the library's row cache.  Inputs that fail one of these are replaced, not tolerated."""
import numpy as np
import pytest
import torch

from oracle import head as ohead, schedule as osch

import _head_decode_cases as hc


@pytest.mark.parametrize("f32", [False, True], ids=["fp16-operands", "fp32-operands"])
@pytest.mark.parametrize("head", list(hc.HEADS))
def test_clamp_case_has_rows_on_both_sides_of_the_clamp(head, f32):
    """For dw and dh: at least 16 rows above the clamp by more than 0.05, at least 16 below it by as much, one of each kind in each frame,
    the oracle's own assert passes (it runs inside the pass) and its outputs are finite."""
    masks = hc.check_clamp_precondition(head, f32)
    cl, bx, of, deltas = hc.clamp_oracle(head, f32)
    # the clamped rows of the oracle are what assertion 1 of the GPU test expects of the kernels: exp(clamp) times the input side
    boxes = hc.clamp_case()["boxes"].view(-1, 4).double()
    for c, (above, _) in masks.items():
        side = (bx.view(-1, 4)[:, c] - bx.view(-1, 4)[:, c - 2]).double()
        want = np.exp(hc.CLAMP) * (boxes[:, c] - boxes[:, c - 2])
        assert ((side / want - 1).abs()[above] < 1e-5).all()
    # only bias[2] and bias[3] were edited
    sd, _, _ = hc.state_dicts(True)
    sd0, _, _ = hc.state_dicts(False)
    for pfx, _, _ in hc.HEADS.values():
        assert torch.equal(sd[pfx + ".bboxes_delta.bias"][:2], sd0[pfx + ".bboxes_delta.bias"][:2])
    assert sum(not torch.equal(sd[k], sd0[k]) for k in sd) == 2


def test_flag_case_boxes_become_invalid():
    case = hc.flag_case()
    boxes = case["boxes"]
    assert (boxes[..., 2:] > boxes[..., :2]).all()
    cfg = ohead.HeadCfg()
    zero = torch.zeros(boxes.shape[0] * boxes.shape[1], 4)
    ohead.apply_deltas(zero, boxes.view(-1, 4), cfg)          # the clean boxes pass the reference's assert
    for row in hc.FLAG_ROWS:
        bad = hc.inverted(boxes, row)
        flat = bad.view(-1, 4)
        assert flat[row, 2] < flat[row, 0] and flat[row, 3] > flat[row, 1]
        keep = torch.arange(flat.shape[0]) != row
        assert torch.equal(flat[keep], boxes.view(-1, 4)[keep])
        with pytest.raises(AssertionError):
            ohead.apply_deltas(zero, flat, cfg)
    assert hc.FLAG_ROWS[1] // 32 == 1 and hc.FLAG_ROWS[1] < hc.M          # second tile, first frame
    assert hc.FLAG_ROWS[2] == 2 * hc.M - 1 and (2 * hc.M) % 32 != 0       # last row of a ragged last tile
    nan = hc.with_nan(boxes, 40).view(-1, 4)
    assert int(torch.isnan(nan).sum()) == 1 and torch.isnan(nan[40]).any()


@pytest.mark.parametrize("head", list(hc.HEADS))
def test_mixed_t_case_frames_read_different_rows(head):
    """The three time steps give every frame a scale / shift row of its own, far enough apart that the oracle bound of the GPU test (2e-2 of
    the logits' RMS + 2e-2 relative) would notice a frame reading another frame's row: a launch within the bound of the wrong answer is
    beyond the bound of the right one when the two are more than twice the bound apart.  And a 32-row tile straddles two frames."""
    cl, _, _, _ = hc.mixed_oracle(head, False)
    rms = float(cl.double().pow(2).mean().sqrt())
    n = len(hc.MIXED_T)
    for shift in (1, 2):
        other = tuple(hc.MIXED_T[(f + shift) % n] for f in range(n))
        cl2, _, _, _ = hc.mixed_oracle(head, False, other)
        for f in range(n):
            d = (cl[f] - cl2[f]).abs()
            assert (d / (2e-2 * rms + 2e-2 * cl[f].abs())).max() > 2, f"frame {f}: t {hc.MIXED_T[f]} and {other[f]} are too close"
    assert hc.M % 32 != 0 and n * hc.M > 32
    pfx, _, is_cond = hc.HEADS[head]
    sd, _, _ = hc.state_dicts(False)
    assert sd[pfx + ".block_time_mlp.1.weight"].shape[0] == (hc.D if is_cond else 2 * hc.D)          # cond: scale only


def test_cache_case_opens_a_second_slab():
    ts = [t for k in range(hc.CACHE_CALLS) for t in hc.cache_t(k)]
    assert len(set(ts)) == len(ts) == 288 > hc.CACHE_SLAB_ROWS
    assert max(ts) < 1000          # the schedule's time steps
    assert min(hc.cache_t(8)) >= hc.CACHE_SLAB_ROWS          # every row of the last call lies in the second slab
    sd, _, _ = hc.state_dicts(False)
    rows = osch.time_mlp(sd, "head.", torch.tensor(ts), hc.D)
    assert len({tuple(r.tolist()) for r in rows}) == len(ts)          # distinct embeddings too
