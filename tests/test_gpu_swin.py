"""The Swin backbone's own kernels, each on its own through the C ABI, against float64 references of the operations
(tests/_swin_ref.py): swin_window_attn_kernel<4> (csrc/attention.hip), f32_swin_window_attn_kernel (csrc/attention.hip) and
patch_merge_ln_kernel (csrc/elementwise.hip).  The backbone tests run them only inside ~20 layers, on one geometry whose token
maps never pad along W and never merge an odd map; a slip in a border window is diluted there before anything is compared.

Bounds are the project's, not these kernels': fp16 attention 4e-3 of RMS + 4e-3 relative (test_mha_mfma: the same swapped-product
scheme with P rounded to fp16 in registers), fp32 attention 2e-5 + 2e-5 (test_f32_mha), LayerNorm 1e-4 + 1e-4 (test_add_layernorm).
tests/test_swin_ref.py shows on the CPU that every case below tells each of five index mistakes from the right answer by more than
20 times the fp16 bound.

Every output buffer carries 64 guard rows and is filled with NaN before a launch: a (window, head) pair that the launch order skipped
leaves NaN in its rows, a padded position that wrote, or a launch that ran past the end, clears NaN in the guard rows.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _swin_ref as ref  # noqa: E402
from test_gpu_kernels import check, h16  # noqa: E402

GUARD = 64


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


ATTN_CASES = [
    (2, 14, 21, 4),       # no padding, 12 windows: 3 full groups of 4
    (1, 40, 48, 2),       # W pads by 1, H by 2
    (2, 10, 12, 8),       # both axes pad, 8 windows
    (2, 8, 13, 4),        # both pad, odd W, 8 windows
    (3, 5, 6, 16),        # H < 7 and W < 7: one window per image, 3 windows -> a ragged group
    (1, 7, 7, 4),         # a single exact window; shifted, every region id is >= 4
    (1, 1, 1, 4),         # one real token among 48 bias tokens
    (1, 19, 32, 32),      # Swin-B's last stage at the benchmark's frame size, C = 1024
    (1, 38, 64, 16),      # Swin-B stage 2, 60 windows
    (5, 20, 24, 4),       # 5 x 12 = 60 windows, 15 groups x 4 heads = 60 workgroups: not a multiple of the 8 XCDs
]
assert ATTN_CASES == ref.ATTN_CASES          # the cases whose sensitivity tests/test_swin_ref.py establishes


def _guarded(rows, cols, dtype):
    return torch.full((rows + GUARD, cols), float("nan"), dtype=dtype, device="cuda")


def _launch_attn(dv, dtype, qkv, qb, table, B, H, W, heads, shift):
    """two launches into the same NaN-filled, guarded buffer -> the first T rows of the first, after the checks that need no reference"""
    fn = dv.swin_window_attn_f16 if dtype == torch.float16 else dv.swin_window_attn_f32
    T, C = B * H * W, 32 * heads
    relbias = dv.swin_pack_relbias(table).cuda()
    qkv_d, qb_d = qkv.cuda().to(dtype), qb.cuda().to(dtype)
    out = _guarded(T, C, dtype)
    runs = []
    for _ in range(2):
        out.fill_(float("nan"))
        fn(qkv_d, qb_d, relbias, B, H, W, heads, shift, out=out)
        torch.cuda.synchronize()
        runs.append(out.clone())
    for r in runs:
        assert not torch.isnan(r[:T]).any(), "a real token's row was left unwritten"
        assert torch.isnan(r[T:]).all(), "something was written beyond the last token"
    # four windows per workgroup reuse the same LDS behind a barrier: a race there shows as a run-to-run difference
    assert torch.equal(runs[0][:T], runs[1][:T]), "two launches on the same inputs differ"
    return runs[0][:T]


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("B,H,W,heads", ATTN_CASES)
def test_swin_window_attn_f16(dv, B, H, W, heads, shift):
    """fp16 MFMA kernel against the float64 reference on the same fp16-rounded qkv and qkv bias (the bias table stays fp32 on both
    sides), 4e-3 of RMS + 4e-3 relative."""
    qkv, qb, table = ref.attn_inputs(B, H, W, heads, shift, half=True)
    assert torch.equal(h16(qkv), qkv) and torch.equal(h16(qb), qb)
    want = ref.window_attention(qkv, qb, table, B, H, W, heads, shift)
    got = _launch_attn(dv, torch.float16, qkv, qb, table, B, H, W, heads, shift)
    check(f"swin_window_attn_f16[{B},{H},{W},heads{heads},shift{shift}]", got, want, 4e-3, 4e-3)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("B,H,W,heads", ATTN_CASES)
def test_swin_window_attn_f32(dv, B, H, W, heads, shift):
    """fp32 kernel against the float64 reference on un-rounded inputs, 2e-5 of RMS + 2e-5 relative."""
    qkv, qb, table = ref.attn_inputs(B, H, W, heads, shift, half=False)
    want = ref.window_attention(qkv, qb, table, B, H, W, heads, shift)
    got = _launch_attn(dv, torch.float32, qkv, qb, table, B, H, W, heads, shift)
    check(f"swin_window_attn_f32[{B},{H},{W},heads{heads},shift{shift}]", got, want, 2e-5, 2e-5)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("B,H,W,heads", ATTN_CASES)
def test_swin_window_attn_f16_against_f32_kernel(dv, B, H, W, heads, shift):
    """Two independent implementations of the same mapping (four windows per 256-thread workgroup on MFMA; one window per wave in
    fp32 FMAs) on the same fp16-representable inputs, within the fp16 bound."""
    qkv, qb, table = ref.attn_inputs(B, H, W, heads, shift, half=True)
    got16 = _launch_attn(dv, torch.float16, qkv, qb, table, B, H, W, heads, shift)
    got32 = _launch_attn(dv, torch.float32, qkv, qb, table, B, H, W, heads, shift)
    check(f"swin_window_attn_f16_vs_f32[{B},{H},{W},heads{heads},shift{shift}]", got16, got32, 4e-3, 4e-3)


def test_swin_window_attn_refuses_bad_arguments(dv):
    """C != 32 * heads is DVID_ERR_UNSUPPORTED, a shift outside [0, 7) DVID_ERR_ARG; neither writes."""
    from diffusionvid_amd._lib import DvidError, call, ptr, stream_ptr
    qkv, qb, table = ref.attn_inputs(1, 7, 7, 2, 0, half=True)
    relbias = dv.swin_pack_relbias(table).cuda()
    out = _guarded(49, 64, torch.float16)
    with pytest.raises(DvidError, match=r"code 3\b"):
        call("dvid_swin_window_attn_f16", ptr(qkv.cuda().half()), ptr(qb.cuda().half()), ptr(relbias), ptr(out), 1, 7, 7, 48, 2, 0, stream_ptr())
    with pytest.raises(DvidError, match=r"code 1\b"):
        dv.swin_window_attn_f16(qkv.cuda().half(), qb.cuda().half(), relbias, 1, 7, 7, 2, 7, out=out)
    with pytest.raises(DvidError, match=r"code 1\b"):
        dv.swin_window_attn_f32(qkv.cuda(), qb.cuda(), relbias, 1, 7, 7, 2, -1, out=_guarded(49, 64, torch.float32))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


MERGE_CASES = [
    (2, 40, 56, 64),      # the small model's first merge: even map
    (3, 5, 7, 128),       # odd H and W, three images
    (2, 7, 6, 256),       # odd H only; the widest C that stays in the first register half
    (2, 9, 13, 512),      # odd both, the widest C: both register halves full
    (1, 1, 1, 128),       # one token, three zero parts
    (1, 19, 32, 512),     # Swin-B's last merge at the benchmark's frame size: odd H
    (1, 1, 8, 64),        # one row
    (3, 8, 1, 384),       # one column; C = 384 fills half of the second register half
]


def _merge_inputs(B, H, W, C):
    """rows with a large mean, the four source tokens of a 2x2 patch offset differently (a swapped part order cannot pass), images far
    apart (the zero row below an odd image must not be the next image's first row), gamma in [0.5, 1.5], beta non-zero"""
    g = torch.Generator().manual_seed(100 * H + W + C)
    x = 3 * torch.randn(B, H, W, C, generator=g) + 5
    x[:, 1::2, 0::2] += 2.0
    x[:, 0::2, 1::2] -= 3.0
    x[:, 1::2, 1::2] += 7.0
    x += 20.0 * torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    gamma = torch.rand(4 * C, generator=g) + 0.5
    beta = 0.3 * torch.randn(4 * C, generator=g) + 0.1
    return x, gamma, beta


@pytest.mark.parametrize("B,H,W,C", MERGE_CASES)
def test_patch_merge_ln(dv, B, H, W, C):
    """2x2 gather (zeros beyond an odd H / W) + LayerNorm over 4C against F.pad + the four strided slices + F.layer_norm in float64:
    fp32 out within 1e-4 of RMS + 1e-4 relative; written together, the fp16 copy is the fp32 copy rounded, bit for bit; written alone,
    each equals what it is when written together."""
    x, gamma, beta = _merge_inputs(B, H, W, C)
    want = ref.patch_merge_ln(x, gamma, beta)
    rows = B * ((H + 1) // 2) * ((W + 1) // 2)
    assert tuple(want.shape) == (rows, 4 * C)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()

    def run(f16, f32):
        o16 = _guarded(rows, 4 * C, torch.float16) if f16 else None
        o32 = _guarded(rows, 4 * C, torch.float32) if f32 else None
        r16, r32 = dv.patch_merge_ln(xd, gd, bd, f16=f16, f32=f32, out16=o16, out32=o32)
        torch.cuda.synchronize()
        assert r16 is o16 and r32 is o32
        for o in (o16, o32):
            if o is not None:
                assert not torch.isnan(o[:rows]).any(), "an output row was left unwritten"
                assert torch.isnan(o[rows:]).all(), "something was written beyond the last output row"
        return (o16[:rows] if f16 else None), (o32[:rows] if f32 else None)

    both16, both32 = run(True, True)
    check(f"patch_merge_ln[{B},{H},{W},{C}]", both32, want, 1e-4, 1e-4)
    assert torch.equal(both16, both32.half()), "the fp16 copy is not the fp32 copy rounded to fp16"
    _, only32 = run(False, True)
    assert torch.equal(only32, both32)
    only16, _ = run(True, False)
    assert torch.equal(only16, both16)


@pytest.mark.parametrize("C", [516, 130])
def test_patch_merge_ln_refuses_unsupported_widths(dv, C):
    """C > 512 (more than two float4 per lane and source token) and C % 4 != 0: DVID_ERR_UNSUPPORTED, nothing written."""
    from diffusionvid_amd._lib import DvidError
    x, gamma, beta = _merge_inputs(1, 4, 4, C)
    o16, o32 = _guarded(4, 4 * C, torch.float16), _guarded(4, 4 * C, torch.float32)
    with pytest.raises(DvidError, match=r"code 3\b"):
        dv.patch_merge_ln(x.cuda(), gamma.cuda(), beta.cuda(), out16=o16, out32=o32)
    torch.cuda.synchronize()
    assert torch.isnan(o16).all() and torch.isnan(o32).all()
