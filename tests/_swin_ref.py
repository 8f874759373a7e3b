"""Test-local float64 references of the Swin backbone's own kernels, written from the operations' definitions
(mega_core/modeling/backbone/swintransformer.py:216-270 around :135-176 for the attention, :296-319 for the merge): whole padded maps,
torch.roll, window partition by view / permute, the relative-position index and the shift mask of oracle/swin.py (pinned to the
reference by golden g8).  Nothing here computes a token's window, a region id or a source address: that arithmetic is the kernels'.

`mutate=` makes ONE deliberate mistake, of the kind an index-heavy kernel makes; tests/test_swin_ref.py asserts that the parity
bound of tests/test_gpu_swin.py separates each of them from the right answer on the cases that test runs."""
import math

import torch
import torch.nn.functional as F

from oracle.swin import relative_position_index, shift_attn_mask

WS, SHIFT = 7, 3

# (B, H, W, heads): what each reaches is listed in tests/test_gpu_swin.py
ATTN_CASES = [
    (2, 14, 21, 4),
    (1, 40, 48, 2),
    (2, 10, 12, 8),
    (2, 8, 13, 4),
    (3, 5, 6, 16),
    (1, 7, 7, 4),
    (1, 1, 1, 4),
    (1, 19, 32, 32),
    (1, 38, 64, 16),
    (5, 20, 24, 4),
]

# name -> (needs shift 3, needs padding)
MUTATIONS = {
    "no_mask": (True, False),                # the shifted map's region mask left out
    "pad_zero": (False, True),               # padded positions hold zeros, not the qkv bias
    "table_transposed": (False, False),      # bias[query][key] read as bias[key][query]
    "roll_sign": (True, False),              # the map rolled by +shift (and back by -shift)
    "mask_unpadded": (True, True),           # region borders taken from H, W, not from the padded Hp, Wp
}


def padded(n):
    return math.ceil(n / WS) * WS


def mutation_applies(name, H, W, shift):
    needs_shift, needs_pad = MUTATIONS[name]
    return (shift > 0 or not needs_shift) and (H % WS != 0 or W % WS != 0 or not needs_pad)


def attn_inputs(B, H, W, heads, shift, half):
    """qkv [B*H*W, 3C] ~ N(0, 1), qkv bias [3C] ~ 0.5 N(0, 1), bias table [169, heads] ~ N(0, 1); `half`: qkv and its bias
    rounded to fp16 (the values the fp16 kernel is given), still held as fp32."""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + heads + shift)
    C = 32 * heads
    qkv = torch.randn(B * H * W, 3 * C, generator=g)
    qkv_bias = 0.5 * torch.randn(3 * C, generator=g)
    table = torch.randn((2 * WS - 1) ** 2, heads, generator=g)
    if half:
        qkv, qkv_bias = qkv.half().float(), qkv_bias.half().float()
    return qkv, qkv_bias, table


def _mask_from_unpadded_size(H, W):
    """shift_attn_mask's construction with the region borders measured from H and W (the mistake), on the padded map"""
    Hp, Wp = padded(H), padded(W)
    img = torch.zeros((Hp, Wp))
    cnt = 0
    for y0, y1 in ((0, max(H - WS, 0)), (max(H - WS, 0), max(H - SHIFT, 0)), (max(H - SHIFT, 0), Hp)):
        for x0, x1 in ((0, max(W - WS, 0)), (max(W - WS, 0), max(W - SHIFT, 0)), (max(W - SHIFT, 0), Wp)):
            img[y0:y1, x0:x1] = cnt
            cnt += 1
    mw = img.view(Hp // WS, WS, Wp // WS, WS).permute(0, 2, 1, 3).reshape(-1, WS * WS)
    d = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


def window_attention(qkv, qkv_bias, table, B, H, W, heads, shift, mutate=None):
    """qkv [B*H*W, 3C], qkv_bias [3C], table [169, heads] -> float64 [B*H*W, C]; shift 0 or 3"""
    assert mutate is None or mutate in MUTATIONS
    assert shift in (0, SHIFT)
    C = 32 * heads
    Hp, Wp = padded(H), padded(W)
    N = WS * WS
    qkv, qkv_bias, table = qkv.double(), qkv_bias.double(), table.double()
    x = torch.zeros(B, Hp, Wp, 3 * C, dtype=torch.float64)
    if mutate != "pad_zero":
        x[:] = qkv_bias                                   # LayerNorm output padded with zeros, then the qkv Linear: its bias
    x[:, :H, :W] = qkv.view(B, H, W, 3 * C)
    roll = -shift if mutate != "roll_sign" else shift
    if shift:
        x = torch.roll(x, shifts=(roll, roll), dims=(1, 2))
    xw = x.view(B, Hp // WS, WS, Wp // WS, WS, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, 3, heads, 32)
    q, k, v = xw.permute(2, 0, 3, 1, 4)                   # each [B * nW, heads, 49, 32]
    attn = q @ k.transpose(-2, -1) / math.sqrt(32.0)
    bias = table[relative_position_index(WS).view(-1)].view(N, N, heads).permute(2, 0, 1)
    if mutate == "table_transposed":
        bias = bias.transpose(1, 2)
    attn = attn + bias.unsqueeze(0)
    if shift and mutate != "no_mask":
        mask = (_mask_from_unpadded_size(H, W) if mutate == "mask_unpadded" else shift_attn_mask(H, W, WS, SHIFT)).double()
        nW = mask.shape[0]
        attn = (attn.view(B, nW, heads, N, N) + mask[None, :, None]).view(-1, heads, N, N)
    y = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(-1, N, C)
    y = y.view(B, Hp // WS, Wp // WS, WS, WS, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        y = torch.roll(y, shifts=(-roll, -roll), dims=(1, 2))
    return y[:, :H, :W].reshape(B * H * W, C)


def worst_over_bound(got, want, rtol, atol_rms):
    """the figure test_gpu_kernels.check asserts on: max |got - want| / (atol_rms * rms(want) + rtol * |want|)"""
    got, want = got.double(), want.double()
    rms = float(want.pow(2).mean().sqrt()) + 1e-12
    return float(((got - want).abs() / (atol_rms * rms + rtol * want.abs())).max())


def patch_merge_ln(x, g, b):
    """x [B, H, W, C], g / b [4C] -> float64 [B * ceil(H/2) * ceil(W/2), 4C]"""
    B, H, W, C = x.shape
    x = F.pad(x.double(), (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    return F.layer_norm(x.reshape(-1, 4 * C), (4 * C,), g.double(), b.double(), 1e-5)
