"""The head's attention kernels, each on its own through the C ABI, against the float64 definition (tests/_mha_ref.py):
mha_mfma_kernel with attn_vt_kernel (dvid_mha_f16) and f32_mha_kernel (dvid_mha_f32), csrc/attention.hip.  test_mha_mfma and
test_f32_mha run four dense shapes whose key counts leave tails of 12, 4, 5 and 1; the model runs the kernels on packed q | k | v and
k | v rows, with a grow-only V^T scratch, behind projections and LayerNorms.  Here: every key and query count around the 16 / 32 / 64
tiles, the model's pitches and strides, scores of a wide known range, and a scratch that holds NaN before the launch.

Bounds are the project's: fp16 4e-3 relative + 4e-3 of RMS (test_mha_mfma), fp32 2e-5 + 2e-5 (test_f32_mha).  tests/test_mha_ref.py
shows on the CPU that the cases tell each of six mistakes of this family of kernel from the right answer by more than 20 times the
fp16 bound.

Every launch writes into a NaN-filled output with 64 guard rows behind the last row (and guard columns where out_ld > d); the fp16
kernel gets a NaN-filled V^T scratch of exactly the documented batch * heads * 32 * (round_up(lk, 32) + 32) halves plus a guard tail.
Two launches must leave no NaN in a real row, every guard NaN, and the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _mha_ref as ref  # noqa: E402
from test_gpu_kernels import check, h16  # noqa: E402

GUARD = 64                 # guard rows of an output, and the unit of the scratch's guard tail
F16 = (4e-3, 4e-3)         # rtol, atol of RMS
F32 = (2e-5, 2e-5)
DTYPES = {"f16": torch.float16, "f32": torch.float32}


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


def _vt_halves(B, nheads, lk):
    return B * nheads * 32 * ((lk + 31) // 32 * 32 + 32)


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


def _call(dtype, bufs, out, vt, B, lq, lk, nheads, q_lay, k_lay, v_lay, out_ld, out_bs):
    """one launch through the C ABI: operand = buffer + column offset, pitches and batch strides as given"""
    from diffusionvid_amd._lib import call, ptr, stream_ptr
    qb, kvb = bufs
    sz = qb.element_size()
    assert k_lay[:2] == v_lay[:2]
    q, k, v = ptr(qb) + q_lay[2] * sz, ptr(kvb) + k_lay[2] * sz, ptr(kvb) + v_lay[2] * sz
    if dtype == torch.float16:
        call("dvid_mha_f16", q, k, v, ptr(out), ptr(vt), B, lq, lk, nheads, q_lay[0], k_lay[0], out_ld, q_lay[1], k_lay[1], out_bs, stream_ptr())
    else:
        call("dvid_mha_f32", q, k, v, ptr(out), B, lq, lk, nheads, q_lay[0], k_lay[0], out_ld, q_lay[1], k_lay[1], out_bs, stream_ptr())


def _upload(p, dtype):
    """the problem's flat buffers on the device (one buffer where q | k | v share rows); fp16 problems hold fp16-representable numbers"""
    if dtype == torch.float16:
        assert torch.equal(h16(p.kvbuf), p.kvbuf) and torch.equal(h16(p.qbuf), p.qbuf)
    kvb = p.kvbuf.cuda().to(dtype)
    return (kvb if p.qbuf is p.kvbuf else p.qbuf.cuda().to(dtype)), kvb


def _launch(dtype, p, stale=float("nan")):
    """two launches into NaN-filled, guarded buffers -> [B, lq, d] of the first, after the checks that need no reference.  `stale`: what
    the V^T scratch holds before each launch (its guard tail holds NaN either way)."""
    B, lq, lk, d, ld = p.B, p.lq, p.lk, p.d, p.out_ld
    bufs = _upload(p, dtype)
    rows = B * lq
    out = _nan((rows + GUARD) * ld, dtype).view(rows + GUARD, ld)
    nvt = _vt_halves(B, p.nheads, lk)
    vt = _nan(nvt + 32 * GUARD, torch.float16) if dtype == torch.float16 else None
    runs = []
    for _ in range(2):
        out.fill_(float("nan"))
        if vt is not None:
            vt.fill_(float("nan"))
            vt[:nvt].fill_(stale)
        _call(dtype, bufs, out, vt, B, lq, lk, p.nheads, p.q_lay, p.k_lay, p.v_lay, ld, p.out_bs)
        torch.cuda.synchronize()
        runs.append(out.clone())
        if vt is not None:
            assert torch.isnan(vt[nvt:]).all(), f"{p.name}: something was written behind the documented V^T scratch"
    for r in runs:
        assert not torch.isnan(r[:rows, :d]).any(), f"{p.name}: a real row was left unwritten, or holds NaN"
        assert torch.isnan(r[rows:]).all(), f"{p.name}: something was written behind the last row"
        assert torch.isnan(r[:rows, d:]).all(), f"{p.name}: something was written into the guard columns"
    assert torch.equal(runs[0][:rows, :d], runs[1][:rows, :d]), f"{p.name}: two launches on the same inputs differ"
    return runs[0][:rows, :d].reshape(B, lq, d)


# ---- every key and query count around the tiles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk", ref.EDGE_LK)
def test_mha_f16_edges(dv, lk):
    """MFMA kernel (32 keys per step as two 16-key halves, 16 queries per wave, 64 per workgroup) on fp16-rounded operands"""
    for lq in ref.EDGE_LQ:
        p = ref.edge_problem(lq, lk, True)
        check(f"mha_f16_edges[lq{lq},lk{lk}]", _launch(torch.float16, p), ref.reference(p), *F16)


@pytest.mark.parametrize("lk", ref.EDGE_LK)
def test_mha_f32_edges(dv, lk):
    """fp32 kernel (64-key chunks in 16-key sub-chunks, one query per lane of a 64-lane workgroup) on un-rounded operands"""
    for lq in ref.EDGE_LQ:
        p = ref.edge_problem(lq, lk, False)
        check(f"mha_f32_edges[lq{lq},lk{lk}]", _launch(torch.float32, p), ref.reference(p), *F32)


@pytest.mark.parametrize("lk", ref.EDGE_LK)
def test_mha_f16_against_f32_kernel(dv, lk):
    """two implementations of one operation (swapped MFMA products with P rounded to fp16; fp32 FMAs through LDS) on the same
    fp16-representable inputs, within the fp16 bound"""
    for lq in ref.EDGE_LQ:
        p = ref.edge_problem(lq, lk, True)
        check(f"mha_f16_vs_f32[lq{lq},lk{lk}]", _launch(torch.float16, p), _launch(torch.float32, p), *F16)


# ---- the model's pitches and strides ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("case", ref.LAYOUT_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-h{c[4]}-pad{c[5]}")
def test_mha_layouts(dv, case, dt):
    """packed q | k | v rows (pitch 3d, one buffer) and packed k | v rows per group (pitch 2d) against the definition, and bit-equal to
    the same kernel on dense copies of the same q / k / v: it reads the same numbers in the same order, so a pitch may not change a bit"""
    dtype = DTYPES[dt]
    p = ref.layout_problem(*case, dtype == torch.float16)
    got = _launch(dtype, p)
    check(f"mha_{dt}_layout[{p.name}]", got, ref.reference(p), *(F16 if dtype == torch.float16 else F32))
    assert torch.equal(got, _launch(dtype, ref.dense_copy(p))), f"{p.name}: the packed launch differs from the dense one"


# ---- scores of a wide, known range -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("lk,order", ref.RANGE_CASES)
def test_mha_range(dv, lk, order, dt):
    """score(i, j) = c_i t_j with |t_j| <= 12: a running maximum that rises in every tile, one that never moves, and one that jumps by
    24 c_i at the last key.  fp16: the project's bound.  fp32: 2e-5 of RMS + (2e-5 + S 2^-18) relative with S the case's largest |score|:
    an fp32 score is one scale multiply and 32 FMAs, off by at most 33 * 2^-24 S < S 2^-18, and exp turns that absolute error into the
    same relative error of the weight (derived, not measured).  Two answers need no reference: `flat` is the mean of the V rows, the
    peaked orders give the peak's V row (how closely: _mha_ref.range_peak_answer)."""
    dtype = DTYPES[dt]
    p = ref.range_problem(lk, order, dtype == torch.float16)
    rtol, atol = F16 if dtype == torch.float16 else (F32[0] + p.max_score * 2.0 ** -18, F32[1])
    got = _launch(dtype, p)
    want = ref.reference(p)
    check(f"mha_{dt}_range[lk{lk},{order}]", got, want, rtol, atol)
    if order == "flat":
        check(f"mha_{dt}_range[lk{lk},flat]=mean(v)", got, p.v().mean(1, keepdim=True).expand_as(want), rtol, atol)
    elif order in ("peak_last", "peak_first"):
        peak, slack = ref.range_peak_answer(p)
        rms = float(peak.pow(2).mean().sqrt())
        excess = (got.double().cpu() - peak).abs() - slack - (atol * rms + rtol * peak.abs())
        assert (excess <= 0).all(), f"{p.name}: {float(excess.max()):.3e} beyond the peak's V row + lk e^-12 * span + the kernel's bound"


# ---- the V^T scratch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lk", [1, 17, 33, 52])
def test_mha_f16_stale_scratch(dv, lk):
    """The model's V^T scratch is a grow-only buffer reused across calls of different lk, and the kernel multiplies P = 0 by its padded
    columns: attn_vt_kernel has to write zeros there, 0 x stale bits is not 0.  The whole scratch holds the fp16 NaN pattern before the
    launch; the output is finite and bit-equal to the launch on a zero-filled scratch."""
    p = ref.edge_problem(17, lk, True) if lk != 52 else ref.layout_problem("self", 3, 52, 52, 8, 0, True)
    stale = _launch(torch.float16, p, stale=float("nan"))
    assert torch.isfinite(stale).all()
    assert torch.equal(stale, _launch(torch.float16, p, stale=0.0)), f"{p.name}: the output depends on what the scratch held"
    check(f"mha_f16_stale_scratch[{p.name}]", stale, ref.reference(p), *F16)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------
def test_mha_refuses_bad_arguments(dv):
    """lk = 0, a q / kv pitch that is no multiple of 8 halves (fp16), an output pitch that is no multiple of 4, any pitch that is no
    multiple of 4 floats (fp32): DVID_ERR_ARG; lq = 0 or batch = 0: nothing to do, OK.  None of them writes.  Every buffer would hold
    the launch if a check were missing: operands of 3 x 40 rows of pitch 264 behind a call for at most 2 x 32 rows of pitch <= 260."""
    from diffusionvid_amd._lib import DvidError
    B, L, nh, d, big = 2, 32, 8, 256, 264
    for dtype, bad_in in ((torch.float16, 260), (torch.float32, 258)):          # 260 % 8 = 4, 258 % 4 = 2
        g = torch.Generator().manual_seed(3)
        bufs = tuple(torch.randn(3 * 40 * big, generator=g).cuda().to(dtype) for _ in range(2))
        out = _nan(3 * 40 * big, dtype)
        vt = _nan(_vt_halves(3, nh, 64), torch.float16) if dtype == torch.float16 else None

        def launch(lq=L, lk=L, batch=B, q_ld=d, kv_ld=d, out_ld=d):
            _call(dtype, bufs, out, vt, batch, lq, lk, nh, (q_ld, 40 * big, 0), (kv_ld, 40 * big, 0), (kv_ld, 40 * big, 20 * big), out_ld, 40 * big)

        for kw in ({"lk": 0}, {"q_ld": bad_in}, {"kv_ld": bad_in}, {"out_ld": 258}):
            with pytest.raises(DvidError, match=r"code 1\b"):
                launch(**kw)
        if dtype == torch.float32:
            with pytest.raises(DvidError, match=r"code 1\b"):
                launch(out_ld=257)
        launch(lq=0)
        launch(batch=0)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "a refused or empty launch wrote to the output"
        if vt is not None:
            assert torch.isnan(vt).all(), "a refused or empty launch wrote to the V^T scratch"
        launch()                                                                   # the same buffers do run
        torch.cuda.synchronize()
        written = ~torch.isnan(out.view(3, 40 * big))                              # rows of pitch d from the start of each batch
        assert written[:B, :L * d].all() and not written[:B, L * d:].any() and not written[B:].any()
