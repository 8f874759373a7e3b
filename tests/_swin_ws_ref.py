"""tests/_swin_ref.py's float64 reference of the Swin window attention with the window size as a parameter (7, or 12 for the
384-pretrained sizes; the shifted block rolls by ws // 2), built the same way: whole padded maps, torch.roll, window partition by view /
permute, the relative-position index and the shift mask of oracle/swin.py.  Nothing here computes a token's window, a region id or a
source address: that arithmetic is the kernels'.  At window 7 it is _swin_ref.window_attention, operation for operation
(tests/test_swin_ws_ref.py asserts a difference of exactly 0).

`mutate=` makes ONE deliberate mistake, the same five as _swin_ref.MUTATIONS; tests/test_swin_ws_ref.py asserts that the parity bound
of tests/test_gpu_swin_ws.py separates each of them from the right answer on the window-12 cases that test runs."""
import math

import torch

from oracle.swin import relative_position_index, shift_attn_mask

from _swin_ref import MUTATIONS, worst_over_bound  # noqa: F401  (the same mistakes, the same metric)

# (B, H, W, heads) at window 12: what each reaches is listed in tests/test_gpu_swin_ws.py
ATTN_CASES_12 = [
    (2, 24, 36, 4),
    (1, 40, 56, 2),
    (2, 10, 14, 8),
    (2, 13, 25, 4),
    (3, 5, 6, 6),
    (1, 12, 12, 4),
    (1, 3, 1, 4),
    (1, 19, 32, 48),
    (1, 38, 64, 16),
    (5, 24, 24, 3),
    (1, 19, 32, 32),
]


def padded(n, ws):
    return math.ceil(n / ws) * ws


def mutation_applies(name, H, W, shift, ws):
    """_swin_ref.mutation_applies, and: where 2 * shift is the window size (12 and 6), a roll by +shift and one by -shift of an axis
    that is one window long are the same roll, so `roll_sign` needs an axis longer than a window"""
    needs_shift, needs_pad = MUTATIONS[name]
    if name == "roll_sign" and (2 * shift) % ws == 0 and max(padded(H, ws), padded(W, ws)) <= ws:
        return False
    return (shift > 0 or not needs_shift) and (H % ws != 0 or W % ws != 0 or not needs_pad)


def attn_inputs(B, H, W, heads, shift, half, ws):
    """_swin_ref.attn_inputs with a [(2 ws - 1)^2, heads] bias table (other seeds than window 7's)"""
    g = torch.Generator().manual_seed(100000 * ws + 1000 * H + 10 * W + heads + shift)
    C = 32 * heads
    qkv = torch.randn(B * H * W, 3 * C, generator=g)
    qkv_bias = 0.5 * torch.randn(3 * C, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    if half:
        qkv, qkv_bias = qkv.half().float(), qkv_bias.half().float()
    return qkv, qkv_bias, table


def _mask_from_unpadded_size(H, W, ws):
    """shift_attn_mask's construction with the region borders measured from H and W (the mistake), on the padded map"""
    shift = ws // 2
    Hp, Wp = padded(H, ws), padded(W, ws)
    img = torch.zeros((Hp, Wp))
    cnt = 0
    for y0, y1 in ((0, max(H - ws, 0)), (max(H - ws, 0), max(H - shift, 0)), (max(H - shift, 0), Hp)):
        for x0, x1 in ((0, max(W - ws, 0)), (max(W - ws, 0), max(W - shift, 0)), (max(W - shift, 0), Wp)):
            img[y0:y1, x0:x1] = cnt
            cnt += 1
    mw = img.view(Hp // ws, ws, Wp // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    d = mw.unsqueeze(1) - mw.unsqueeze(2)
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


def window_attention(qkv, qkv_bias, table, B, H, W, heads, shift, ws, mutate=None):
    """qkv [B*H*W, 3C], qkv_bias [3C], table [(2 ws - 1)^2, heads] -> float64 [B*H*W, C]; shift 0 or ws // 2"""
    assert mutate is None or mutate in MUTATIONS
    assert shift in (0, ws // 2)
    C = 32 * heads
    Hp, Wp = padded(H, ws), padded(W, ws)
    N = ws * ws
    qkv, qkv_bias, table = qkv.double(), qkv_bias.double(), table.double()
    x = torch.zeros(B, Hp, Wp, 3 * C, dtype=torch.float64)
    if mutate != "pad_zero":
        x[:] = qkv_bias                                   # LayerNorm output padded with zeros, then the qkv Linear: its bias
    x[:, :H, :W] = qkv.view(B, H, W, 3 * C)
    roll = -shift if mutate != "roll_sign" else shift
    if shift:
        x = torch.roll(x, shifts=(roll, roll), dims=(1, 2))
    xw = x.view(B, Hp // ws, ws, Wp // ws, ws, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, 3, heads, 32)
    q, k, v = xw.permute(2, 0, 3, 1, 4)                   # each [B * nW, heads, ws*ws, 32]
    attn = q @ k.transpose(-2, -1) / math.sqrt(32.0)
    bias = table[relative_position_index(ws).view(-1)].view(N, N, heads).permute(2, 0, 1)
    if mutate == "table_transposed":
        bias = bias.transpose(1, 2)
    attn = attn + bias.unsqueeze(0)
    if shift and mutate != "no_mask":
        mask = (_mask_from_unpadded_size(H, W, ws) if mutate == "mask_unpadded" else shift_attn_mask(H, W, ws, ws // 2)).double()
        nW = mask.shape[0]
        attn = (attn.view(B, nW, heads, N, N) + mask[None, :, None]).view(-1, heads, N, N)
    y = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(-1, N, C)
    y = y.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        y = torch.roll(y, shifts=(-roll, -roll), dims=(1, 2))
    return y[:, :H, :W].reshape(B * H * W, C)
