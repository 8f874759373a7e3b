"""What the head-decode tests share (tests/test_head_decode_cases.py on the CPU, tests/test_gpu_head_decode.py on the GPU): the small
geometry on which one RCNNHead / RCNNHead_cond pass is driven to its scale clamp, its bad-box flag and its per-frame time steps, the
oracle's answers for it (computed once and shared) and the precondition that keeps the clamp tests honest.  Pure CPU.

Geometry: a 64 x 64 image, a p3..p5 pyramid of fp16-representable randn * 0.5 maps (8 x 8, 4 x 4, 2 x 2), M = 72 boxes per frame (three
32-row tiles per frame with a ragged last one; with two frames the rows 64..95 of the fused tail's third tile straddle both frames),
centres inside the image and sides exp(U(0.3, 3.3)), synthetic.make_head_state_dict(0), proposal features supplied by the caller."""
import functools

import torch

from oracle import head as ohead, schedule as osch

H = W = 64
M = 72
D = 256
CLAMP = ohead._DEFAULT_SCALE_CLAMP          # log(100000 / 16), box_head.py:19
MARGIN = 0.05                               # a row counts as clamped / unclamped when its delta is this far from the clamp
MIN_ROWS = 16                               # rows of either kind that every (head, delta) needs
# head tag -> (prefix in the state dict, head_index of ops.Model.rcnn_head, is it the cond head)
HEADS = {"plain": ("head.head_series.1", 1, False), "cond": ("head.head_series_cond.0", 0, True)}
ROUTES = ("fused", "layerwise", "float32")

# The clamp cases: bboxes_delta.bias[2] and bias[3] of a head = CLAMP - CLAMP_BIAS_BELOW[head], inputs drawn with CLAMP_SEED.  With both
# biases exactly at the clamp the rows are not balanced: dw and dh spread with a standard deviation of about 0.6 around a mean that the
# head's weights put up to half a unit beside the bias (plain head: dw + 0.55, dh - 0.45; cond head: + 0.3, + 0.25), so each bias sits
# that far on the other side.  Offsets and seed were picked on the oracle alone (tests/test_head_decode_cases.py asserts what they give).
CLAMP_BIAS_BELOW = {"plain": (0.55, -0.45), "cond": (0.3, 0.25)}
CLAMP_SEED = 2


def h16(x):
    return x.to(torch.float16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def state_dicts(clamp_bias=False):
    """(sd, sd16, sd32): what the library is given, what the oracle of the fp16 routes is given (the same GEMM matrices rounded to fp16,
    as tests/test_gpu_kernels.py::test_rcnn_head feeds it) and what the oracle of the float32 route is given (test_gpu_f32.py).
    clamp_bias: bboxes_delta.bias[2] and bias[3] of both heads are set CLAMP_BIAS_BELOW below the clamp; bias[0] and bias[1] stay."""
    from diffusionvid_amd.utils import synthetic
    sd = synthetic.make_head_state_dict(0)
    if clamp_bias:
        for head, (pfx, _, _) in HEADS.items():
            b = sd[pfx + ".bboxes_delta.bias"].clone()
            b[2], b[3] = (CLAMP - off for off in CLAMP_BIAS_BELOW[head])
            sd[pfx + ".bboxes_delta.bias"] = b
    sd16 = {k: (h16(v) if v.dim() > 1 else v) for k, v in sd.items()}
    sd32 = {k: v.float() for k, v in sd.items()}
    return sd, sd16, sd32


@functools.lru_cache(maxsize=None)
def inputs(seed, n, m=M):
    """feats: NCHW p3..p5 of n frames; boxes [n, m, 4]; pro [n * m, 256] proposal features; cond [n * m, 256] (the cond head's)"""
    g = torch.Generator().manual_seed(seed)
    feats = [h16(torch.randn(n, D, H // s, W // s, generator=g) * 0.5) for s in (8, 16, 32)]
    ctr = torch.rand(n, m, 2, generator=g) * torch.tensor([float(W), float(H)])
    wh = torch.exp(torch.rand(n, m, 2, generator=g) * 3.0 + 0.3)
    boxes = torch.cat([ctr - wh / 2, ctr + wh / 2], dim=-1)
    pro = torch.randn(n * m, D, generator=g)
    cond = torch.randn(n * m, D, generator=g)
    return {"feats": feats, "boxes": boxes, "pro": pro, "cond": cond, "n": n, "m": m}


def oracle_pass(sdo, head, case, t, frames=None):
    """oracle.head.rcnn_head on the case (or on its frames `frames` only: frames are independent inside a head) with time steps t ->
    (logits [n, m, C], boxes [n, m, 4], obj_features [n * m, 256], deltas [n * m, 4])"""
    pfx, _, is_cond = HEADS[head]
    m = case["m"]
    fr = list(range(case["n"])) if frames is None else list(frames)
    rows = torch.cat([torch.arange(f * m, (f + 1) * m) for f in fr])
    t = torch.as_tensor(t, dtype=torch.long)
    assert t.numel() == len(fr)
    time = osch.time_mlp(sdo, "head.", t, D)
    taps = {}
    cl, bx, of = ohead.rcnn_head(sdo, pfx, [f[fr] for f in case["feats"]], case["boxes"][fr], case["pro"][rows][None], time, ohead.HeadCfg(),
                                 cond=case["cond"][rows] if is_cond else None, taps=taps)
    return cl, bx, of[0], taps["deltas"]


# ---- the clamp cases --------------------------------------------------------------------------------------------------------------------
CLAMP_T = (999, 499)


def clamp_case():
    return inputs(CLAMP_SEED, 2)


@functools.lru_cache(maxsize=None)
def clamp_oracle(head, f32):
    """the oracle's pass over the clamp case on the operands of the fp16 routes (f32 False) or of the float32 route (True); its own
    assert (box_head.py:588) runs inside"""
    _, sd16, sd32 = state_dicts(True)
    return oracle_pass(sd32 if f32 else sd16, head, clamp_case(), CLAMP_T)


def clamp_classes(deltas):
    """per delta (2: dw, 3: dh): boolean row masks (clamped by the margin, unclamped by the margin).  bbox_weights[2:] are 1."""
    return {c: (deltas[:, c] > CLAMP + MARGIN, deltas[:, c] < CLAMP - MARGIN) for c in (2, 3)}


def check_clamp_precondition(head, f32):
    """A condition on the inputs, not a measurement: for dw and dh, at least MIN_ROWS rows above the clamp by more than MARGIN, as many below
    it, at least one of each kind in each frame, and every output of the oracle finite.  -> the masks of clamp_classes"""
    cl, bx, of, deltas = clamp_oracle(head, f32)
    assert torch.isfinite(bx).all() and torch.isfinite(cl).all()
    masks = clamp_classes(deltas)
    for c, (above, below) in masks.items():
        name = "dw" if c == 2 else "dh"
        assert int(above.sum()) >= MIN_ROWS, f"{head} {name}: only {int(above.sum())} rows above the clamp"
        assert int(below.sum()) >= MIN_ROWS, f"{head} {name}: only {int(below.sum())} rows below the clamp"
        for f in range(2):
            assert above[f * M:(f + 1) * M].any() and below[f * M:(f + 1) * M].any(), f"{head} {name}: frame {f} has rows of one kind only"
    return masks


# ---- the flag cases: the unmodified weights, head_series.1, one box of the clamp case's geometry made invalid ------------------------------
FLAG_SEED = 5
FLAG_ROWS = (0, 40, 143)          # first row; second tile of frame 0; last row (ragged tile of the last frame)
FLAG_T = (499, 499)


def flag_case():
    return inputs(FLAG_SEED, 2)


def inverted(boxes, row):
    """a copy of boxes [n, m, 4] with x1 and x2 of flat row `row` swapped: a negative width"""
    b = boxes.clone()
    flat = b.view(-1, 4)
    flat[row, 0], flat[row, 2] = boxes.view(-1, 4)[row, 2], boxes.view(-1, 4)[row, 0]
    return b


def with_nan(boxes, row):
    b = boxes.clone()
    b.view(-1, 4)[row, 1] = float("nan")
    return b


# ---- per-frame time steps -----------------------------------------------------------------------------------------------------------------
MIXED_SEED = 6
MIXED_T = (999, 0, 499)


def mixed_case():
    return inputs(MIXED_SEED, 3)


@functools.lru_cache(maxsize=None)
def mixed_oracle(head, f32, t=MIXED_T):
    _, sd16, sd32 = state_dicts(False)
    return oracle_pass(sd32 if f32 else sd16, head, mixed_case(), t)


# ---- the scale / shift row cache: 9 calls of 32 frames x 8 boxes with 288 distinct time steps -------------------------------------------------
CACHE_SEED = 7
CACHE_FRAMES, CACHE_M, CACHE_CALLS = 32, 8, 9
CACHE_SLAB_ROWS = 256          # rows of one slab of the library's (head slot, t) cache (csrc/head.hip)


def cache_case():
    return inputs(CACHE_SEED, CACHE_FRAMES, CACHE_M)


def cache_t(k):
    return tuple(range(CACHE_FRAMES * k, CACHE_FRAMES * (k + 1)))
