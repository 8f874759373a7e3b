"""CPU side of tests/test_gpu_swin.py: the float64 reference of the Swin window attention (tests/_swin_ref.py) against the oracle's
block, the power of the parity test's cases to tell a wrong kernel from a right one, and the library's host-side packing of the
relative-position bias.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _swin_ref as ref
from oracle import swin as oswin

FP16_BOUND = (4e-3, 4e-3)          # rtol, atol of RMS: what test_gpu_swin.py allows the fp16 kernel (test_mha_mfma's bound)
MIN_RATIO = 20.0


def test_every_mutation_moves_the_reference_far_beyond_the_fp16_bound():
    """The parity test can fail: on each of its cases, each deliberate mistake that applies to the case (a mask mistake needs the
    shifted block, a padding mistake a padded map) moves the float64 reference by more than 20 times the fp16 bound, in the
    metric `check` asserts on.  Every case is told apart by at least one mistake, every mistake applies to at least three cases."""
    applied = {m: 0 for m in ref.MUTATIONS}
    for (B, H, W, heads) in ref.ATTN_CASES:
        for shift in (0, ref.SHIFT):
            qkv, qb, table = ref.attn_inputs(B, H, W, heads, shift, half=True)
            want = ref.window_attention(qkv, qb, table, B, H, W, heads, shift)
            assert torch.isfinite(want).all() and tuple(want.shape) == (B * H * W, 32 * heads)
            ratios = {}
            for m in ref.MUTATIONS:
                if not ref.mutation_applies(m, H, W, shift):
                    continue
                ratios[m] = ref.worst_over_bound(ref.window_attention(qkv, qb, table, B, H, W, heads, shift, mutate=m), want, *FP16_BOUND)
                applied[m] += 1
            print(f"({B}, {H}, {W}, heads {heads}, shift {shift}): " + ", ".join(f"{m} {r:.0f}" for m, r in ratios.items()))
            assert ratios, "no mutation applies"
            for m, r in ratios.items():
                assert r > MIN_RATIO, f"({B}, {H}, {W}, heads {heads}, shift {shift}): {m} moves the reference by only {r:.1f} x the bound"
    assert all(n >= 3 for n in applied.values()), applied


@pytest.mark.parametrize("B,H,W,heads,shift", [(2, 8, 13, 4, 3), (2, 8, 13, 4, 0), (3, 5, 6, 2, 3), (1, 14, 21, 2, 3)])
def test_reference_equals_the_oracle_block(B, H, W, heads, shift):
    """The reference takes qkv; the oracle's SwinTransformerBlock takes tokens.  With a qkv Linear whose weight is random and an identity
    output projection, the attention branch of oracle.swin.swin_block must equal the reference on the qkv that Linear gives (fp32
    against float64: 1e-5).  This pins the reference's conventions -- q | k | v order, head-major columns, bias in the padding, roll
    direction, mask -- to the code golden g8 pins to the upstream module."""
    g = torch.Generator().manual_seed(7)
    C = 32 * heads
    y = torch.randn(B, H * W, C, generator=g)
    wq, bq = torch.randn(3 * C, C, generator=g) / C ** 0.5, 0.5 * torch.randn(3 * C, generator=g)
    table = torch.randn(169, heads, generator=g)
    sd = {"a.attn.qkv.weight": wq, "a.attn.qkv.bias": bq, "a.attn.relative_position_bias_table": table,
          "a.attn.proj.weight": torch.eye(C), "a.attn.proj.bias": torch.zeros(C),
          "a.norm1.weight": torch.ones(C), "a.norm1.bias": torch.zeros(C), "a.norm2.weight": torch.ones(C), "a.norm2.bias": torch.zeros(C),
          "a.mlp.fc1.weight": torch.zeros(C, C), "a.mlp.fc1.bias": torch.zeros(C), "a.mlp.fc2.weight": torch.zeros(C, C),
          "a.mlp.fc2.bias": torch.zeros(C)}
    out = oswin.swin_block(sd, "a", y, H, W, heads, 7, shift, oswin.shift_attn_mask(H, W, 7, 3))      # y + attention (the MLP adds zero)
    ln = F.layer_norm(y, (C,))
    qkv = F.linear(ln.double(), wq.double(), bq.double()).reshape(B * H * W, 3 * C)
    want = ref.window_attention(qkv, bq, table, B, H, W, heads, shift)
    got = (out - y).reshape(B * H * W, C).double()
    assert ref.worst_over_bound(got, want, 1e-5, 1e-5) <= 1.0


@pytest.mark.parametrize("heads", [1, 4, 32])
def test_swin_pack_relbias_is_the_gathered_table(heads):
    """dvid_swin_pack_relbias (the loader's own packing, host only): [heads][49][64], entry [h][i][j] = table[relative_position_index(i, j)][h]
    exactly, columns 49..63 exactly zero."""
    from diffusionvid_amd import ops
    g = torch.Generator().manual_seed(heads)
    table = torch.randn(169, heads, generator=g)
    packed = ops.swin_pack_relbias(table).numpy()
    assert packed.shape == (heads, 49, 64)
    want = table[oswin.relative_position_index(7).view(-1)].view(49, 49, heads).permute(2, 0, 1).numpy()
    np.testing.assert_array_equal(packed[:, :, :49], want)
    np.testing.assert_array_equal(packed[:, :, 49:], np.zeros((heads, 49, 15), np.float32))


def test_patch_merge_reference_part_order():
    """the merged row of an odd map: parts in the order (0,0) (1,0) (0,1) (1,1), zeros beyond the last row / column"""
    x = torch.arange(1, 3 * 3 + 1, dtype=torch.float32).view(1, 3, 3, 1).repeat(1, 1, 1, 4)
    y = ref.patch_merge_ln(x, torch.ones(16), torch.zeros(16))
    assert tuple(y.shape) == (4, 16)
    raw = [[1, 4, 2, 5], [3, 6, 0, 0], [7, 0, 8, 0], [9, 0, 0, 0]]
    for row, parts in zip(y, raw):
        v = torch.tensor(parts, dtype=torch.float64).repeat_interleave(4)
        torch.testing.assert_close(row, (v - v.mean()) / (v.var(unbiased=False) + 1e-5).sqrt())
