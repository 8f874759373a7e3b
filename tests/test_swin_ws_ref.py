"""CPU side of tests/test_gpu_swin_ws.py (12x12 windows, the 384-pretrained Swin sizes): the window-parametrised float64 reference
(tests/_swin_ws_ref.py) against the established window-7 reference and against the oracle's block at window 12, the power of the
window-12 parity cases to tell a wrong kernel from a right one, the library's host-side bias packing at window 12, and the two size
names.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _swin_ref as ref7
import _swin_ws_ref as ref
from oracle import swin as oswin

FP16_BOUND = (4e-3, 4e-3)          # rtol, atol of RMS: what test_gpu_swin_ws.py allows the fp16 kernel (test_gpu_swin.py's bound)
MIN_RATIO = 20.0


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("B,H,W,heads", ref7.ATTN_CASES)
def test_window_7_is_the_established_reference(B, H, W, heads, shift):
    """at window 7 the parametrised reference IS tests/_swin_ref.window_attention: the same operations in the same order, difference
    exactly 0 on all of its cases at both shifts"""
    qkv, qb, table = ref7.attn_inputs(B, H, W, heads, shift, half=True)
    want = ref7.window_attention(qkv, qb, table, B, H, W, heads, shift)
    got = ref.window_attention(qkv, qb, table, B, H, W, heads, shift, 7)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    for m in ref.MUTATIONS:
        assert ref.mutation_applies(m, H, W, shift, 7) == ref7.mutation_applies(m, H, W, shift)


@pytest.mark.parametrize("B,H,W,heads,shift", [(2, 13, 25, 4, 6), (2, 13, 25, 4, 0), (3, 5, 6, 2, 6), (1, 24, 36, 2, 6)])
def test_reference_equals_the_oracle_block_at_window_12(B, H, W, heads, shift):
    """test_swin_ref.test_reference_equals_the_oracle_block at window 12, shift 6: a random qkv Linear and an identity output projection
    make the attention branch of oracle.swin.swin_block the reference's output on the qkv that Linear gives (fp32 against float64:
    1e-5 of RMS + 1e-5 relative)."""
    g = torch.Generator().manual_seed(7)
    C = 32 * heads
    y = torch.randn(B, H * W, C, generator=g)
    wq, bq = torch.randn(3 * C, C, generator=g) / C ** 0.5, 0.5 * torch.randn(3 * C, generator=g)
    table = torch.randn(23 * 23, heads, generator=g)
    sd = {"a.attn.qkv.weight": wq, "a.attn.qkv.bias": bq, "a.attn.relative_position_bias_table": table,
          "a.attn.proj.weight": torch.eye(C), "a.attn.proj.bias": torch.zeros(C),
          "a.norm1.weight": torch.ones(C), "a.norm1.bias": torch.zeros(C), "a.norm2.weight": torch.ones(C), "a.norm2.bias": torch.zeros(C),
          "a.mlp.fc1.weight": torch.zeros(C, C), "a.mlp.fc1.bias": torch.zeros(C), "a.mlp.fc2.weight": torch.zeros(C, C),
          "a.mlp.fc2.bias": torch.zeros(C)}
    out = oswin.swin_block(sd, "a", y, H, W, heads, 12, shift, oswin.shift_attn_mask(H, W, 12, 6))      # y + attention (the MLP adds zero)
    ln = F.layer_norm(y, (C,))
    qkv = F.linear(ln.double(), wq.double(), bq.double()).reshape(B * H * W, 3 * C)
    want = ref.window_attention(qkv, bq, table, B, H, W, heads, shift, 12)
    got = (out - y).reshape(B * H * W, C).double()
    worst = ref.worst_over_bound(got, want, 1e-5, 1e-5)
    print(f"({B}, {H}, {W}, heads {heads}, shift {shift}): {worst:.3f} of the bound")
    assert worst <= 1.0


def test_every_mutation_moves_the_window_12_reference_far_beyond_the_fp16_bound():
    """test_swin_ref's sensitivity harness on the window-12 cases of tests/test_gpu_swin_ws.py: each deliberate mistake that applies to a
    case moves the float64 reference by more than 20 times the fp16 bound; every case is told apart by at least one mistake, every
    mistake applies to at least three cases.  (A 1x1 map is not in this list: one real token among 143 bias tokens moves by 1 to 14
    bounds under three of the mistakes; the GPU test runs it as an edge case only.)"""
    applied = {m: 0 for m in ref.MUTATIONS}
    for (B, H, W, heads) in ref.ATTN_CASES_12:
        for shift in (0, 6):
            qkv, qb, table = ref.attn_inputs(B, H, W, heads, shift, True, 12)
            want = ref.window_attention(qkv, qb, table, B, H, W, heads, shift, 12)
            assert torch.isfinite(want).all() and tuple(want.shape) == (B * H * W, 32 * heads)
            ratios = {}
            for m in ref.MUTATIONS:
                if not ref.mutation_applies(m, H, W, shift, 12):
                    continue
                ratios[m] = ref.worst_over_bound(ref.window_attention(qkv, qb, table, B, H, W, heads, shift, 12, mutate=m), want, *FP16_BOUND)
                applied[m] += 1
            print(f"({B}, {H}, {W}, heads {heads}, shift {shift}): " + ", ".join(f"{m} {r:.0f}" for m, r in ratios.items()))
            assert ratios, "no mutation applies"
            for m, r in ratios.items():
                assert r > MIN_RATIO, f"({B}, {H}, {W}, heads {heads}, shift {shift}): {m} moves the reference by only {r:.1f} x the bound"
    assert all(n >= 3 for n in applied.values()), applied


@pytest.mark.parametrize("heads", [1, 4, 48])
def test_swin_pack_relbias_window_12_is_the_gathered_table(heads):
    """dvid_swin_pack_relbias_ws at window 12 (the loader's own packing, host only): [heads][144][160], entry [h][i][j] =
    table[relative_position_index(12)(i, j)][h] exactly, columns 144..159 exactly zero."""
    from diffusionvid_amd import ops
    g = torch.Generator().manual_seed(heads)
    table = torch.randn(529, heads, generator=g)
    packed = ops.swin_pack_relbias(table, window=12).numpy()
    assert packed.shape == (heads, 144, 160)
    want = table[oswin.relative_position_index(12).view(-1)].view(144, 144, heads).permute(2, 0, 1).numpy()
    np.testing.assert_array_equal(packed[:, :, :144], want)
    np.testing.assert_array_equal(packed[:, :, 144:], np.zeros((heads, 144, 16), np.float32))


@pytest.mark.parametrize("heads", [1, 4, 32])
def test_swin_pack_relbias_window_7_is_the_existing_call(heads):
    """window=7, and dvid_swin_pack_relbias_ws called with 7, are bit-equal to the existing entry; another window, and a table of the
    wrong height, are refused"""
    from diffusionvid_amd import _lib, ops
    g = torch.Generator().manual_seed(heads)
    table = torch.randn(169, heads, generator=g)
    old = ops.swin_pack_relbias(table)
    assert torch.equal(ops.swin_pack_relbias(table, window=7), old)
    out = torch.full((heads, 49, 64), float("nan"))
    _lib.call("dvid_swin_pack_relbias_ws", _lib.ptr(table), heads, 7, _lib.ptr(out))
    assert torch.equal(out, old)
    out.fill_(float("nan"))
    with pytest.raises(_lib.DvidError, match=r"code 3\b.*window size 8"):
        _lib.call("dvid_swin_pack_relbias_ws", _lib.ptr(table), heads, 8, _lib.ptr(out))
    assert torch.isnan(out).all()
    with pytest.raises(TypeError):
        ops.swin_pack_relbias(table, window=12)


@pytest.mark.parametrize("size,embed,heads", [("B-22k-384", 128, (4, 8, 16, 32)), ("L-22k-384", 192, (6, 12, 24, 48))])
def test_window_12_sizes_resolve_through_the_config(size, embed, heads):
    """MODEL.SWIN.SIZE B-22k-384 / L-22k-384 (size2config, swintransformer.py:655-712) reach the detector as 12x12-window models; the
    state dict it builds carries [529, heads] bias tables"""
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    cfg = get_cfg("configs/vid_Swin_B_DiffusionVID.yaml", ["DTYPE", "float16", "MODEL.SWIN.SIZE", size], "configs/BASE_RCNN_1gpu.yaml")
    cfg.freeze()
    model = build_detection_model(cfg)
    assert model.swin == dict(embed_dim=embed, depths=(2, 2, 18, 2), heads=heads, window=12)
    sd = model.state_dict()
    for st in range(4):
        assert tuple(sd[f"backbone.bottom_up.layers.{st}.blocks.1.attn.relative_position_bias_table"].shape) == (529, heads[st])


def test_window_12_config_override_and_unknown_size():
    from diffusionvid_amd.config import get_cfg
    from diffusionvid_amd.modeling.detector import build_detection_model
    sw = dict(embed_dim=64, depths=(2, 2, 2, 1), heads=(2, 4, 8, 16), window=12)
    cfg = get_cfg("configs/vid_Swin_B_DiffusionVID.yaml", ["DTYPE", "float16"], "configs/BASE_RCNN_1gpu.yaml")
    cfg.MODEL.SWIN.CONFIG_OVERRIDE = sw
    cfg.freeze()
    model = build_detection_model(cfg)
    assert model.swin == sw
    assert tuple(model.state_dict()["backbone.bottom_up.layers.0.blocks.0.attn.relative_position_bias_table"].shape) == (529, 2)
    cfg = get_cfg("configs/vid_Swin_B_DiffusionVID.yaml", ["DTYPE", "float16", "MODEL.SWIN.SIZE", "H-22k-384"], "configs/BASE_RCNN_1gpu.yaml")
    cfg.freeze()
    with pytest.raises(NotImplementedError, match="H-22k-384") as e:
        build_detection_model(cfg)
    assert "window-7" not in str(e.value)
