"""One RCNNHead / RCNNHead_cond pass (dvid_rcnn_head_levels, csrc/head.hip) where its last steps matter: the scale clamp of apply_deltas,
the bad-box flag, frames of one launch with different time steps, and the (head slot, t) row cache past its first slab.  Inputs, oracle
answers and the preconditions are tests/_head_decode_cases.py's (tests/test_head_decode_cases.py proves them on the CPU).

The three routes through the library:
  fused      the default fp16 pass: head_tail_kernel (csrc/headtail.hip) ends it, with its own restatement of apply_deltas
  layerwise  option head_tail = 0: the layer-by-layer fp16 pass, also the path of every vocabulary above 64 classes; apply_deltas_kernel
  float32    Model(..., precision="float32"): rcnn_head_chain_f32, apply_deltas_kernel

Bounds against the oracle are those of the route's existing head test: fp16 2e-2 of RMS + 2e-2 relative for logits and object features
and 3e-2 for boxes (test_gpu_kernels.py::test_rcnn_head), float32 2e-4 / 3e-4 (test_gpu_f32.py::test_f32_rcnn_head); fused against
layerwise 3e-3 / 5e-3 (test_head_tail_fused_matches_layerwise)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _head_decode_cases as hc  # noqa: E402
from test_gpu_kernels import REPORT, _report_path, check  # noqa: E402

ORACLE_BOUNDS = {"fused": (2e-2, 3e-2), "layerwise": (2e-2, 3e-2), "float32": (2e-4, 3e-4)}          # (logits / features, boxes)
NAMES = ("logits", "boxes", "obj_features")


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


@pytest.fixture(scope="module")
def models(dv):
    """(clamp_bias, precision) -> a head-only Model with room for 3 frames of 72 boxes, built on first use"""
    made = {}

    def get(clamp_bias, precision):
        key = (bool(clamp_bias), precision)
        if key not in made:
            sd, _, _ = hc.state_dicts(key[0])
            made[key] = dv.Model(sd, res_blocks=(0, 0, 0, 0), precision=precision)
            made[key].reserve(3, hc.H, hc.W, hc.M)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def precision_of(route):
    return "float32" if route == "float32" else "float16"


def device_maps(dv, case, precision):
    if precision == "float32":
        return [f.permute(0, 2, 3, 1).contiguous().cuda() for f in case["feats"]]
    return [dv.nhwc_from_nchw(f.cuda()) for f in case["feats"]]


def launch(dv, model, route, head, case, t, boxes=None, flag=None):
    """one pass of `head` over the case on `route` -> (logits [n * m, C], boxes [n * m, 4], obj_features [n * m, 256]) on the host"""
    _, index, is_cond = hc.HEADS[head]
    fd = device_maps(dv, case, model.precision)
    boxes = case["boxes"] if boxes is None else boxes
    args = (index, fd, hc.H, hc.W, boxes.cuda(), case["pro"].cuda(), torch.as_tensor(t, dtype=torch.long))
    kw = dict(cond=case["cond"].cuda() if is_cond else None, bad_flag=flag)
    if route == "layerwise":
        dv.set_option("head_tail", 0)
        try:
            out = model.rcnn_head(*args, **kw)
        finally:
            dv.reset_options()
    else:
        out = model.rcnn_head(*args, **kw)
    gl, gb, go = (x.cpu() for x in out)
    return gl.reshape(-1, gl.shape[-1]), gb.reshape(-1, 4), go


def new_flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def box_figure(name, got, want, size, bound):
    """max |got - want| over the four coordinates, relative to `size` per row; one line of reports/parity_report.txt, then the assertion"""
    err = ((got - want).abs().max(-1).values / size).max().item()
    line = f"{name}: boxes rel-to-size err max={err:.3e} bound={bound:.1e} nan={int(torch.isnan(got).sum())}"
    REPORT.append(line)
    print(line)
    with open(_report_path(), "a") as f:
        f.write(line + "\n")
    assert not torch.isnan(got).any(), line
    assert err < bound, line
    return err


def output_size(bx):
    bx = bx.reshape(-1, 4)
    return (bx[:, 2:] - bx[:, :2]).clamp(min=1.0).max(-1).values


def input_size(boxes):
    b = boxes.reshape(-1, 4)
    return (b[:, 2:] - b[:, :2]).clamp(min=1.0).max(-1).values


def against_oracle(tag, route, got, want, size, rows=None):
    """logits, boxes and object features of a launch against the oracle's within the route's bounds (rows: a subset of the launch's rows)"""
    tol, btol = ORACLE_BOUNDS[route]
    gl, gb, go = got if rows is None else tuple(x[rows] for x in got)
    cl, bx, of = want
    check(f"{tag}.obj_features", go, of, tol, tol)
    check(f"{tag}.logits", gl, cl.reshape(-1, cl.shape[-1]), tol, tol)
    return box_figure(tag, gb, bx.reshape(-1, 4), size, btol)


# ---- A. the scale clamp -------------------------------------------------------------------------------------------------------------------
_clamp_out = {}


def clamp_launch(dv, models, route, head):
    key = (route, head)
    if key not in _clamp_out:
        flag = new_flag()
        out = launch(dv, models(True, precision_of(route)), route, head, hc.clamp_case(), hc.CLAMP_T, flag=flag)
        _clamp_out[key] = (out, int(flag.item()))
    return _clamp_out[key]


@pytest.mark.parametrize("head", list(hc.HEADS))
@pytest.mark.parametrize("route", hc.ROUTES)
def test_clamp(dv, models, route, head):
    """bboxes_delta.bias[2:4] near log(100000 / 16): about half of the 144 rows are clamped on dw, about half on dh (the precondition, asserted
    first).  (1) A row the oracle clamps by more than 0.05 must come out exp(clamp) times as wide / high as it went in, to 1e-5: five fp32
    roundings of 6e-8 each, the fp32 clamp constant (8.74 x 6e-8 in the exponent) and expf within a few ulp stay under 1e-6; the centre
    term is at most 1 / 6000 of the side; 10 x for the difference between the host's and the device's libm.  A kernel without its
    fminf is off by exp(0.05) - 1 = 5e-2 at least.  (2) All rows against the oracle, boxes relative to the OUTPUT size (exp(8.7) makes the
    output 6000 times the input).  (4) The flag stays 0.
    Measured on the MI355X, worst box error relative to the output size (plain / cond head): fused 9.96e-4 / 6.23e-4, layerwise 9.96e-4 /
    6.23e-4, float32 1.47e-6 / 1.48e-6; worst relative deviation of a clamped side 3.84e-7 on every route (62 .. 70 clamped rows each)."""
    f32 = route == "float32"
    masks = hc.check_clamp_precondition(head, f32)
    (gl, gb, go), flag = clamp_launch(dv, models, route, head)
    assert flag == 0
    assert torch.isfinite(gb).all()
    # (1) the clamped rows, from the input boxes and the constant alone
    boxes = hc.clamp_case()["boxes"].reshape(-1, 4).double()
    scale = float(np.exp(np.float64(hc.CLAMP)))
    worst = 0.0
    for c, (above, _) in masks.items():
        side = (gb[:, c].double() - gb[:, c - 2].double())[above]
        want = scale * (boxes[:, c] - boxes[:, c - 2])[above]
        dev = (side / want - 1).abs().max().item()
        worst = max(worst, dev)
        print(f"clamp[{route},{head}].{'dw' if c == 2 else 'dh'}: {int(above.sum())} clamped rows, worst relative deviation of the side {dev:.3e}")
        assert dev <= 1e-5, f"{route} {head}: a clamped {'width' if c == 2 else 'height'} is {dev:.3e} off exp(clamp) x the input's"
    with open(_report_path(), "a") as f:
        f.write(f"clamp[{route},{head}]: clamped sides worst relative deviation={worst:.3e} bound=1.0e-05\n")
    # (2) every row against the oracle
    cl, bx, of, _ = hc.clamp_oracle(head, f32)
    against_oracle(f"clamp[{route},{head}]", route, (gl, gb, go), (cl, bx, of), output_size(bx))


@pytest.mark.parametrize("head", list(hc.HEADS))
def test_clamp_fused_matches_layerwise(dv, models, head):
    """(3) The fused tail's restatement of apply_deltas against apply_deltas_kernel behind the same fp16 layers, on the clamp case: the bounds
    of test_head_tail_fused_matches_layerwise, boxes relative to the output size.  Measured (plain / cond head): boxes 3.10e-4 / 2.75e-4 of
    the output size, logits within 7.9e-4, object features within 5.8e-5."""
    hc.check_clamp_precondition(head, False)
    (gl, gb, go), f1 = clamp_launch(dv, models, "fused", head)
    (ll, lb, lo), f2 = clamp_launch(dv, models, "layerwise", head)
    assert f1 == 0 and f2 == 0
    tag = f"clamp_fused_vs_layerwise[{head}]"
    check(tag + ".obj_features", go, lo, 3e-3, 3e-3)
    check(tag + ".logits", gl, ll, 3e-3, 3e-3)
    box_figure(tag, gb, lb, output_size(lb), 5e-3)


# ---- B. the bad-box flag ----------------------------------------------------------------------------------------------------------------
def rows_but(n, row):
    return torch.arange(n) != row


@pytest.mark.parametrize("route", hc.ROUTES)
def test_bad_box_flag(dv, models, route):
    """One box with x1 and x2 swapped (row 0; row 40: second tile; row 143: last row of the ragged last tile), or with a NaN coordinate (row
    40): the flag reads 1 after the launch and 0 after the same launch on the restored boxes, and every other row is the same bit for bit
    in both -- the proposal features are the caller's, so self-attention does not see the box, RoIAlign and DynamicConv are per box, and
    box_level gathers zeros for a box without a valid area."""
    case = hc.flag_case()
    model = models(False, precision_of(route))
    flag = new_flag()
    clean = launch(dv, model, route, "plain", case, hc.FLAG_T, flag=flag)
    assert int(flag.item()) == 0
    assert all(torch.isfinite(x).all() for x in clean)
    R = clean[0].shape[0]
    for kind, row in [("inverted", r) for r in hc.FLAG_ROWS] + [("nan", 40)]:
        bad_boxes = hc.inverted(case["boxes"], row) if kind == "inverted" else hc.with_nan(case["boxes"], row)
        flag = new_flag()
        bad = launch(dv, model, route, "plain", case, hc.FLAG_T, boxes=bad_boxes, flag=flag)
        assert int(flag.item()) == 1, f"{route}: the flag stayed 0 with an {kind} box in row {row}"
        flag = new_flag()
        again = launch(dv, model, route, "plain", case, hc.FLAG_T, flag=flag)
        assert int(flag.item()) == 0, f"{route}: the flag rose on the restored boxes (after row {row})"
        keep = rows_but(R, row)
        for a, b, c, name in zip(bad, again, clean, NAMES):
            assert torch.equal(b, c), f"{route}: {name} of the clean launch changed after the launch with row {row} {kind}"
            assert torch.isfinite(a[keep]).all(), f"{route}: {name} not finite beside the {kind} row {row}"
            assert torch.equal(a[keep], b[keep]), (f"{route}: {name} of rows other than the {kind} row {row} differ, first at row "
                                                   f"{int((a != b).reshape(R, -1).any(-1).logical_and(keep).nonzero()[0])}")


def test_bad_box_flag_reaches_the_host(dv):
    """DynamicHead.plain_heads + check_boxes_valid: an inverted box raises the reference's AssertionError once -- the check clears the flag --
    and a clean pass raises nothing."""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.roi_heads.box_head.box_head import DynamicHead
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_cfg(os.path.join(root, "configs/vid_R_101_DiffusionVID.yaml"), [], os.path.join(root, "configs/BASE_RCNN_1gpu.yaml"))
    sd, _, _ = hc.state_dicts(False)
    model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
    head = DynamicHead(cfg, engine_provider=lambda: model)
    head.eval()
    case = hc.flag_case()
    fd = device_maps(dv, case, "float16")
    t = torch.tensor(hc.FLAG_T)
    head.plain_heads(fd, case["boxes"].cuda(), t)
    head.check_boxes_valid()
    head.plain_heads(fd, hc.inverted(case["boxes"], 40).cuda(), t)
    with pytest.raises(AssertionError):
        head.check_boxes_valid()
    head.check_boxes_valid()          # cleared by the check that raised
    head.plain_heads(fd, case["boxes"].cuda(), t)
    head.check_boxes_valid()
    model.close()


# ---- C. frames of one launch with different time steps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", list(hc.HEADS))
@pytest.mark.parametrize("route", hc.ROUTES)
def test_per_frame_t(dv, models, route, head):
    """t = [999, 0, 499] over 3 frames of 72 rows (the tile of rows 64..95 straddles frames 0 / 1, that of rows 128..159 frames 1 / 2): the
    launch lays the frames' scale / shift rows out in the workspace, bt_out floats apart (2 d for the plain head, d for the cond head, which
    has no shift half).  Frame f must come out bit for bit as in a launch of the same shape with t = t_f on every frame, which reads the one
    cached row with stride 0: same kernels, same tiles, and the table holds device-to-device copies of the very rows.  Then the mixed
    launch against the oracle.  Measured box error relative to the box size (plain / cond head): fused 3.45e-3 / 5.88e-3, layerwise
    3.54e-3 / 5.90e-3, float32 9.57e-6 / 4.47e-6."""
    case = hc.mixed_case()
    model = models(False, precision_of(route))
    flag = new_flag()
    mixed = launch(dv, model, route, head, case, hc.MIXED_T, flag=flag)
    for f, tf in enumerate(hc.MIXED_T):
        uniform = launch(dv, model, route, head, case, (tf,) * len(hc.MIXED_T), flag=flag)
        rows = slice(f * hc.M, (f + 1) * hc.M)
        for a, b, name in zip(mixed, uniform, NAMES):
            assert torch.equal(a[rows], b[rows]), (f"{route} {head}: {name} of frame {f} (t = {tf}) differ between the mixed launch and the uniform one, "
                                                   f"max |d| {(a[rows] - b[rows]).abs().max().item():.3e}")
        # and the uniform launch's other frames did not get frame f's answer by accident of equal rows
        other = (f + 1) % len(hc.MIXED_T)
        rows_o = slice(other * hc.M, (other + 1) * hc.M)
        assert not torch.equal(mixed[0][rows_o], uniform[0][rows_o])
    assert int(flag.item()) == 0
    cl, bx, of, _ = hc.mixed_oracle(head, route == "float32")
    against_oracle(f"per_frame_t[{route},{head}]", route, mixed, (cl, bx, of), input_size(case["boxes"]))


# ---- D. the scale / shift row cache across a slab boundary -----------------------------------------------------------------------------------
def test_row_cache_across_slabs(dv):
    """288 distinct (slot 1, t) rows from nine calls of 32 frames with a time step each: the 257th row opens the cache's second slab.  The
    first call repeated afterwards gives its first answer bit for bit (slab one survived the growth); a fresh model whose first call is the
    ninth gives the old model's ninth answer bit for bit (the same rows at slab-one addresses there, in slab two here); frames 0 and 31 of the
    ninth call are within the fp16 head bounds of the oracle.  Then head slot 1 and cond slot 0 on the same t = 7 in one model, in either
    order: each within the bounds of its own oracle, so neither reads the other's row.  Measured box error relative to the box size: 1.81e-3
    (ninth call), 2.86e-3 / 1.25e-3 (plain / cond head on t = 7).  The cache is host code shared by the three routes: the fused one runs."""
    case = hc.cache_case()
    sd, sd16, _ = hc.state_dicts(False)
    n, m = hc.CACHE_FRAMES, hc.CACHE_M
    size = input_size(case["boxes"])

    def make():
        model = dv.Model(sd, res_blocks=(0, 0, 0, 0))
        model.reserve(n, hc.H, hc.W, m)
        return model

    old = make()
    flag = new_flag()
    outs = [launch(dv, old, "fused", "plain", case, hc.cache_t(k), flag=flag) for k in range(hc.CACHE_CALLS)]
    again = launch(dv, old, "fused", "plain", case, hc.cache_t(0), flag=flag)
    for a, b, name in zip(again, outs[0], NAMES):
        assert torch.equal(a, b), f"{name} of the first call changed once the cache had grown a second slab"
    for k in range(1, hc.CACHE_CALLS):
        assert not torch.equal(outs[k][0], outs[0][0])          # the calls do read different rows
    fresh = make()
    first = launch(dv, fresh, "fused", "plain", case, hc.cache_t(8), flag=flag)
    for a, b, name in zip(first, outs[8], NAMES):
        assert torch.equal(a, b), f"{name} of the ninth call differ between the second slab of one model and the first slab of a fresh one"
    frames = (0, n - 1)
    rows = torch.cat([torch.arange(f * m, (f + 1) * m) for f in frames])
    cl, bx, of, _ = hc.oracle_pass(sd16, "plain", case, [hc.cache_t(8)[f] for f in frames], frames=frames)
    against_oracle("row_cache[call 9, frames 0 and 31]", "fused", outs[8], (cl, bx, of), size[rows], rows=rows)

    # two head slots on one time step
    t7 = (7,) * n
    want = {head: hc.oracle_pass(sd16, head, case, [7, 7], frames=frames)[:3] for head in hc.HEADS}
    for model, order, tag in ((old, ("plain", "cond"), "old"), (fresh, ("cond", "plain"), "fresh")):
        got = {head: launch(dv, model, "fused", head, case, t7, flag=flag) for head in order}
        for head in order:
            against_oracle(f"row_cache[{tag} model, {head} on t = 7]", "fused", got[head], want[head], size[rows], rows=rows)
        back = launch(dv, model, "fused", order[0], case, t7, flag=flag)
        for a, b, name in zip(back, got[order[0]], NAMES):
            assert torch.equal(a, b), f"{tag} model: {name} of the {order[0]} head changed after the {order[1]} head ran on the same t"
    assert int(flag.item()) == 0
    old.close()
    fresh.close()
