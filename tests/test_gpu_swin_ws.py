"""The 12x12 Swin window-attention kernels (the 384-pretrained sizes), each on its own through the C ABI's `_ws` entries, against the
float64 reference of tests/_swin_ws_ref.py: swin_window12_attn_kernel<2> (csrc/attention.hip) and f32_swin_window12_attn_kernel
(csrc/attention.hip).  Same bounds and the same guarded, NaN-filled, launched-twice outputs as tests/test_gpu_swin.py: fp16 4e-3 of RMS +
4e-3 relative, fp32 2e-5 + 2e-5.  tests/test_swin_ws_ref.py shows on the CPU that every case of ATTN_CASES below tells each of five
index mistakes from the right answer by more than 20 times the fp16 bound; the 1x1 map is run as an edge case only.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _swin_ref as ref7  # noqa: E402
import _swin_ws_ref as ref  # noqa: E402
from test_gpu_kernels import check, h16  # noqa: E402

GUARD = 64
WS, SHIFT = 12, 6


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


ATTN_CASES = [
    (2, 24, 36, 4),       # no padding, 12 windows: 6 full pairs
    (1, 40, 56, 2),       # both axes pad (48, 60), 20 windows
    (2, 10, 14, 8),       # H < 12 pads to one window row, W to two columns
    (2, 13, 25, 4),       # one token beyond a window on both axes: 11 padded rows / columns, odd sizes
    (3, 5, 6, 6),         # smaller than a window on both axes: one window per image, 3 windows -> a ragged pair
    (1, 12, 12, 4),       # a single exact window; shifted, every region id is >= 4
    (1, 3, 1, 4),         # three real tokens among 141 bias tokens
    (1, 19, 32, 48),      # Swin-L's last stage at the benchmark's frame size, C = 1536
    (1, 38, 64, 16),      # Swin-B stage 2: 4 x 6 windows
    (5, 24, 24, 3),       # 20 windows x 3 heads: 30 fp16 workgroups, 60 fp32 ones, neither a multiple of the 8 XCDs
    (1, 19, 32, 32),      # Swin-B's last stage, C = 1024
]
assert ATTN_CASES == ref.ATTN_CASES_12          # the cases whose sensitivity tests/test_swin_ws_ref.py establishes
EDGE_CASES = [(1, 1, 1, 4)]                     # one real token among 143 bias tokens


def _guarded(rows, cols, dtype):
    return torch.full((rows + GUARD, cols), float("nan"), dtype=dtype, device="cuda")


def _launch_attn(dv, dtype, qkv, qb, table, B, H, W, heads, shift, ws=WS):
    """two launches into the same NaN-filled, guarded buffer -> the first T rows of the first, after the checks that need no reference"""
    fn = dv.swin_window_attn_f16 if dtype == torch.float16 else dv.swin_window_attn_f32
    T, C = B * H * W, 32 * heads
    relbias = dv.swin_pack_relbias(table, window=ws).cuda()
    qkv_d, qb_d = qkv.cuda().to(dtype), qb.cuda().to(dtype)
    out = _guarded(T, C, dtype)
    runs = []
    for _ in range(2):
        out.fill_(float("nan"))
        fn(qkv_d, qb_d, relbias, B, H, W, heads, shift, out=out, window=ws)
        torch.cuda.synchronize()
        runs.append(out.clone())
    for r in runs:
        assert not torch.isnan(r[:T]).any(), "a real token's row was left unwritten"
        assert torch.isnan(r[T:]).all(), "something was written beyond the last token"
    # two windows per workgroup reuse the same LDS behind a barrier: a race there shows as a run-to-run difference
    assert torch.equal(runs[0][:T], runs[1][:T]), "two launches on the same inputs differ"
    return runs[0][:T]


@pytest.mark.parametrize("shift", [0, SHIFT])
@pytest.mark.parametrize("B,H,W,heads", ATTN_CASES + EDGE_CASES)
def test_swin_window12_attn_f16(dv, B, H, W, heads, shift):
    """fp16 MFMA kernel against the float64 reference on the same fp16-rounded qkv and qkv bias (the bias table stays fp32 on both
    sides), 4e-3 of RMS + 4e-3 relative."""
    qkv, qb, table = ref.attn_inputs(B, H, W, heads, shift, True, WS)
    assert torch.equal(h16(qkv), qkv) and torch.equal(h16(qb), qb)
    want = ref.window_attention(qkv, qb, table, B, H, W, heads, shift, WS)
    got = _launch_attn(dv, torch.float16, qkv, qb, table, B, H, W, heads, shift)
    check(f"swin_window12_attn_f16[{B},{H},{W},heads{heads},shift{shift}]", got, want, 4e-3, 4e-3)


@pytest.mark.parametrize("shift", [0, SHIFT])
@pytest.mark.parametrize("B,H,W,heads", ATTN_CASES + EDGE_CASES)
def test_swin_window12_attn_f32(dv, B, H, W, heads, shift):
    """fp32 kernel against the float64 reference on un-rounded inputs, 2e-5 of RMS + 2e-5 relative."""
    qkv, qb, table = ref.attn_inputs(B, H, W, heads, shift, False, WS)
    want = ref.window_attention(qkv, qb, table, B, H, W, heads, shift, WS)
    got = _launch_attn(dv, torch.float32, qkv, qb, table, B, H, W, heads, shift)
    check(f"swin_window12_attn_f32[{B},{H},{W},heads{heads},shift{shift}]", got, want, 2e-5, 2e-5)


@pytest.mark.parametrize("shift", [0, SHIFT])
@pytest.mark.parametrize("B,H,W,heads", ATTN_CASES + EDGE_CASES)
def test_swin_window12_attn_f16_against_f32_kernel(dv, B, H, W, heads, shift):
    """Two independent implementations of the same mapping (nine MFMA waves, one 16-query tile each, two windows per workgroup; four
    fp32 lanes per query, one window per workgroup) on the same fp16-representable inputs, within the fp16 bound."""
    qkv, qb, table = ref.attn_inputs(B, H, W, heads, shift, True, WS)
    got16 = _launch_attn(dv, torch.float16, qkv, qb, table, B, H, W, heads, shift)
    got32 = _launch_attn(dv, torch.float32, qkv, qb, table, B, H, W, heads, shift)
    check(f"swin_window12_attn_f16_vs_f32[{B},{H},{W},heads{heads},shift{shift}]", got16, got32, 4e-3, 4e-3)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("B,H,W,heads", ref7.ATTN_CASES)
def test_ws_entries_at_window_7_are_the_existing_entries(dv, B, H, W, heads, shift):
    """dvid_swin_window_attn_f16_ws / _f32_ws with window 7 forward to the existing launchers: bit-identical outputs"""
    from diffusionvid_amd._lib import call, ptr, stream_ptr
    qkv, qb, table = ref7.attn_inputs(B, H, W, heads, shift, half=True)
    T, C = B * H * W, 32 * heads
    relbias = dv.swin_pack_relbias(table).cuda()
    for dtype, name in ((torch.float16, "dvid_swin_window_attn_f16"), (torch.float32, "dvid_swin_window_attn_f32")):
        old = _launch_attn(dv, dtype, qkv, qb, table, B, H, W, heads, shift, ws=7)
        qkv_d, qb_d = qkv.cuda().to(dtype), qb.cuda().to(dtype)
        out = _guarded(T, C, dtype)
        call(name + "_ws", ptr(qkv_d), ptr(qb_d), ptr(relbias), ptr(out), B, H, W, C, heads, shift, 7, stream_ptr())
        torch.cuda.synchronize()
        assert torch.isnan(out[T:]).all() and torch.equal(out[:T], old), name


def test_swin_window_attn_ws_refuses_bad_arguments(dv):
    """window 8 is DVID_ERR_UNSUPPORTED, shift 12 at window 12 DVID_ERR_ARG, C != 32 * heads DVID_ERR_UNSUPPORTED, in both precisions;
    none writes."""
    from diffusionvid_amd._lib import DvidError, call, ptr, stream_ptr
    qkv, qb, table = ref.attn_inputs(1, 12, 12, 2, 0, True, WS)
    relbias = dv.swin_pack_relbias(table, window=WS).cuda()
    for dtype, name in ((torch.float16, "dvid_swin_window_attn_f16_ws"), (torch.float32, "dvid_swin_window_attn_f32_ws")):
        fn = dv.swin_window_attn_f16 if dtype == torch.float16 else dv.swin_window_attn_f32
        qkv_d, qb_d = qkv.cuda().to(dtype), qb.cuda().to(dtype)
        out = _guarded(144, 64, dtype)
        with pytest.raises(DvidError, match=r"code 3\b.*window size 8"):
            call(name, ptr(qkv_d), ptr(qb_d), ptr(relbias), ptr(out), 1, 12, 12, 64, 2, 0, 8, stream_ptr())
        with pytest.raises(DvidError, match=r"code 1\b"):
            fn(qkv_d, qb_d, relbias, 1, 12, 12, 2, 12, out=out, window=WS)
        with pytest.raises(DvidError, match=r"code 1\b"):
            fn(qkv_d, qb_d, relbias, 1, 12, 12, 2, -1, out=out, window=WS)
        with pytest.raises(DvidError, match=r"code 3\b"):
            call(name, ptr(qkv_d), ptr(qb_d), ptr(relbias), ptr(out), 1, 12, 12, 48, 2, 0, 12, stream_ptr())
        with pytest.raises(DvidError, match=r"code 1\b"):
            call(name, ptr(qkv_d), None, ptr(relbias), ptr(out), 1, 12, 12, 64, 2, 0, 12, stream_ptr())
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
