"""The global-memory pruning kernels of csrc/fps.hip, each on its own through the C ABI: cdist_kernel, fps_reg_kernel<4 | 8 | 16>,
fps_kernel (the LDS form beyond 4096 points) and gather_rows_kernel, at the sizes where the launcher changes kernel, where a tile
ends, and where the sweep degenerates (one point, m = 1, m = n, fewer points than a wave).  test_cdist_fps_gather runs n = 175, 600,
975, 1800 and 3000, all on the register kernel, and never passes a block size to emulate.

Index outputs are compared exactly with oracle.memory.fps_kernel_order, the thread-level emulation of the reference kernel's tie rule
(pinned by tests/test_oracle_golden.py), on two kinds of matrix: a tie-heavy integer one, where almost every step is decided by the
tie rule, and a real torch.cdist matrix of N(0, 1) rows.  Every output buffer is pre-filled (-1 or NaN) and carries a guard tail."""
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import memory as omem  # noqa: E402
from test_gpu_kernels import check  # noqa: E402

GUARD = 64


@pytest.fixture(scope="module")
def dv():
    from diffusionvid_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops


@lru_cache(maxsize=4)
def _matrix(n, kind):
    """[n, n] fp32 on the host (shared: do not write to it).  `ties`: integers 0..4, diagonal included; `real`: distances of N(0, 1) rows"""
    if kind == "ties":
        return torch.from_numpy(np.random.RandomState(n).randint(0, 5, size=(n, n)).astype(np.float32))
    x = torch.randn(n, 16, generator=torch.Generator().manual_seed(n))
    return torch.cdist(x, x, p=2.0)


def _fps(dist_d, n, m, bs_emul=0):
    """dvid_fps_greedy into an index buffer pre-filled with -1, m entries + guard -> the m picks (host, int32)"""
    from diffusionvid_amd._lib import call, ptr, stream_ptr
    idx = torch.full((m + GUARD,), -1, dtype=torch.int32, device="cuda")
    call("dvid_fps_greedy", ptr(dist_d), n, m, bs_emul, ptr(idx), stream_ptr())
    torch.cuda.synchronize()
    idx = idx.cpu().numpy()
    assert (idx[m:] == -1).all(), "something was written behind the last pick"
    return idx[:m]


def _against_emulation(n, ms, bs_emul=0):
    for kind in ("ties", "real"):
        D = _matrix(n, kind)
        Dd = D.cuda()
        for m in ms:
            want = omem.fps_kernel_order(D.numpy(), m, bs=bs_emul or None)
            np.testing.assert_array_equal(_fps(Dd, n, m, bs_emul), want, err_msg=f"n {n}, m {m}, {kind}, bs_emul {bs_emul}")


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, 2048, 2049, 4096])
def test_fps_kernel_boundaries(dv, n):
    """fps_reg_kernel<4> up to 1024 points, <8> up to 2048, <16> up to 4096: both sides of each threshold, the sizes around one wave and
    around the 256 threads (one point per thread, then a second point for thread 0 only), m = min(n, 40); up to 257 points also m = n
    (every point taken, then repeats where the integer matrix's diagonal is not its row's minimum) and m = 1 (no step at all)."""
    ms = [min(n, 40)]
    if n <= 257:
        ms += [n, 1]
    _against_emulation(n, sorted(set(ms)))


@pytest.mark.parametrize("n", [4097, 5000])
def test_fps_lds_kernel(dv, n):
    """fps_kernel, the form the launcher takes beyond 4096 points: 1024 threads, the running distances in n * 4 bytes of dynamic LDS,
    the winner found by an owner search.  m = 40 on both kinds of matrix.  The 5000 x 5000 matrix is 100 MB; larger sizes stay out of
    this suite: the launcher accepts up to 24576 points (96 KB of LDS), but beyond 16384 points, where the dynamic LDS passes 64 KB,
    the distance matrix alone is over 1 GB."""
    _against_emulation(n, [40])


@pytest.mark.parametrize("n", [600, 3000])
@pytest.mark.parametrize("bs_emul", [64, 256, 1024])
def test_fps_block_size_emulation(dv, n, bs_emul):
    """the tie rule of another block size of the reference kernel than the one it would choose for n (512 and 1024 here)"""
    _against_emulation(n, [40], bs_emul)


def test_fps_refuses_bad_arguments(dv):
    """a block size that is no power of two, and more picks than points: DVID_ERR_ARG, idx untouched (the buffers would hold either launch)"""
    from diffusionvid_amd._lib import DvidError, call, ptr, stream_ptr
    n = 600
    Dd = _matrix(n, "ties").cuda()
    idx = torch.full((n + 1 + GUARD,), -1, dtype=torch.int32, device="cuda")
    for m, bs_emul in ((40, 300), (n + 1, 0)):
        with pytest.raises(DvidError, match=r"code 1\b"):
            call("dvid_fps_greedy", ptr(Dd), n, m, bs_emul, ptr(idx), stream_ptr())
    torch.cuda.synchronize()
    assert (idx == -1).all()


@pytest.mark.parametrize("n", [1025, 4097])
def test_fps_groups_at_the_boundaries(dv, n):
    """fps_greedy_groups with two problems: fps_reg_groups_kernel<8> at 1025 points, the per-group loop over the LDS kernel at 4097;
    each group's picks are those of the single launch on its matrix, and of the emulation"""
    m = 40
    D = torch.stack([_matrix(n, "ties"), _matrix(n, "real")])
    Dd = D.cuda()
    got = dv.fps_greedy_groups(Dd, m)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, m) and got.dtype == torch.int32
    for g in range(2):
        single = _fps(Dd[g], n, m)
        np.testing.assert_array_equal(got[g].cpu().numpy(), single)
        np.testing.assert_array_equal(single, omem.fps_kernel_order(D[g].numpy(), m))


# ---- cdist --------------------------------------------------------------------------------------------------------------------------------
def _cdist(x):
    """dvid_cdist into a NaN-filled [n, n] + guard -> [n, n] on the host"""
    from diffusionvid_amd._lib import call, ptr, stream_ptr
    n, d = x.shape
    out = torch.full((n * n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    xd = x.cuda()
    call("dvid_cdist", ptr(xd), n, d, ptr(out), stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out[n * n:]).all(), "something was written behind the matrix"
    return out[:n * n].view(n, n).cpu()


def _cdist64(x):
    return torch.cdist(x.double(), x.double(), p=2.0, compute_mode="donot_use_mm_for_euclid_dist")


@pytest.mark.parametrize("d", [4, 36, 256])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_cdist_edges(dv, n, d):
    """64 x 64 tiles in k steps of 16: one row, one short of / exactly / one past a tile, three tiles with a ragged edge; d below one
    k step, no multiple of one, and the model's 256.  Off-diagonal entries against float64 torch.cdist within 1e-5 + 1e-5 of RMS
    (test_cdist_fps_gather's bound); the diagonal is finite and below 0.05, the square root of an fp32 cancellation residue."""
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(100 * n + d))
    got = _cdist(x)
    assert torch.isfinite(got).all()
    assert got.diagonal().abs().max() < 0.05
    if n > 1:
        off = ~torch.eye(n, dtype=torch.bool)
        check(f"cdist_edges[n{n},d{d}](offdiag)", got[off], _cdist64(x)[off], 1e-5, 1e-5)


def test_cdist_of_equal_rows(dv):
    """rows 3 and 70 are copies of row 0 (|x|^2 ~ 256; row 70 lies in another tile than the other two): their mutual distances are
    |a|^2 + |b|^2 - 2 a.b of equal numbers, clamped at 0 before the square root: finite, not NaN, and below 0.05 like the diagonal;
    every other entry keeps the 1e-5 + 1e-5 bound"""
    n, d = 130, 256
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(5))
    x[3] = x[0]
    x[70] = x[0]
    got = _cdist(x)
    assert torch.isfinite(got).all()
    same = torch.eye(n, dtype=torch.bool)
    for i in (0, 3, 70):
        for j in (0, 3, 70):
            same[i, j] = True
    assert got[same].abs().max() < 0.05
    check("cdist_equal_rows(others)", got[~same], _cdist64(x)[~same], 1e-5, 1e-5)


# ---- gather ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 256])
@pytest.mark.parametrize("m", [1, 257])
def test_gather_rows_edges(dv, m, d):
    """one float4 per thread, 256 threads per workgroup: a single row, and 257 rows (with d = 4 one thread past a workgroup) with
    repeated indices, first and last source row included: bit-equal to indexing, nothing written behind the last row"""
    from diffusionvid_amd._lib import call, ptr, stream_ptr
    n = 50
    g = torch.Generator().manual_seed(m + d)
    x = torch.randn(n, d, generator=g)
    idx = torch.randint(0, n, (m,), generator=g, dtype=torch.int32)
    idx[0] = n - 1
    idx[-1] = n - 1 if m == 1 else 0
    out = torch.full((m * d + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    xd, idxd = x.cuda(), idx.cuda()
    call("dvid_gather_rows", ptr(xd), ptr(idxd), ptr(out), m, d, stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out[m * d:]).all(), "something was written behind the last row"
    assert torch.equal(out[:m * d].view(m, d).cpu(), x[idx.long()])


def test_gather_rows_refuses_a_width_that_is_no_multiple_of_4(dv):
    """d = 6: DVID_ERR_ARG, nothing written"""
    from diffusionvid_amd._lib import DvidError, call, ptr, stream_ptr
    x = torch.randn(8, 8).cuda()
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda")
    with pytest.raises(DvidError, match=r"code 1\b"):
        call("dvid_gather_rows", ptr(x), ptr(idx), ptr(out), 4, 6, stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
