"""Test-local float64 references of the head's multi-head attention (csrc/attention.hip: mha_mfma_kernel with attn_vt_kernel, and
f32_mha_kernel), head dimension 32, written from the definition softmax(q k^T / sqrt(32)) v per head, and the case tables of
tests/test_gpu_mha.py.

The kernels are told where to read by (row pitch, batch stride, column offset), never by a shape, so a case here is a `Problem`: flat
buffers plus those three numbers per operand.  `strided` turns them into the [B, L, d] view the kernel is told to read; the dense cases
and the packed ones (q | k | v rows of self-attention, k | v rows of the projected memory) are built from the same generator.

`tiled_attention` is the 32-key online-softmax recurrence the MFMA kernel runs (tail rows clamped to lk - 1, tail scores masked, padded
V zero).  `mistake=` makes ONE deliberate slip of the kind this family of kernel makes; tests/test_mha_ref.py shows that the recurrence
is the definition and that the bound of tests/test_gpu_mha.py separates every slip from the right answer on named cases."""
import math
from dataclasses import dataclass
from functools import lru_cache

import torch

DH = 32          # head dimension
TILE = 32        # keys per step of the MFMA kernel (two 16-key halves); the fp32 kernel takes 64-key chunks in 16-key sub-chunks

MISTAKES = (
    "tail_unmasked",         # the clamped duplicates of key lk - 1 take part in the softmax (their V columns are the zero padding)
    "sum_not_rescaled",      # l += psum in place of l = l * f + psum
    "acc_not_rescaled",      # the accumulator is not multiplied by f
    "scale_sqrt_d",          # 1 / sqrt(d) in place of 1 / sqrt(32)
    "row_pitch_d",           # K / V rows addressed with pitch d inside a 2d- or 3d-pitched buffer
    "q_stride_for_kv",       # the query's batch stride used for K / V
)


@dataclass(frozen=True, eq=False)
class Problem:
    name: str
    B: int
    lq: int
    lk: int
    nheads: int
    qbuf: torch.Tensor          # flat fp32; the SAME tensor as kvbuf where q | k | v share rows
    kvbuf: torch.Tensor         # flat fp32
    q_lay: tuple                # (row pitch, batch stride, column offset), in elements
    k_lay: tuple
    v_lay: tuple                # pitch and batch stride equal k_lay's: the kernels take one kv_ld / kv_bs
    out_ld: int
    max_score: float = None     # RANGE_CASES: the largest |score|
    order: str = None           # RANGE_CASES: how the scores are ordered along the keys

    @property
    def d(self):
        return self.nheads * DH

    @property
    def out_bs(self):
        return self.lq * self.out_ld

    def q(self):
        return strided(self.qbuf, self.B, self.lq, self.d, *self.q_lay).double()

    def k(self):
        return strided(self.kvbuf, self.B, self.lk, self.d, *self.k_lay).double()

    def v(self):
        return strided(self.kvbuf, self.B, self.lk, self.d, *self.v_lay).double()


def strided(buf, B, L, d, ld, bs, col):
    """flat buffer + (row pitch, batch stride, column offset) -> the [B, L, d] view a kernel given these numbers reads.  A view that
    runs past the buffer (only a mistaken stride does) reads zeros there."""
    need = (B - 1) * bs + (L - 1) * ld + col + d
    if need > buf.numel():
        buf = torch.cat([buf, buf.new_zeros(need - buf.numel())])
    return buf.as_strided((B, L, d), (bs, ld, 1), col)


def _heads(x, nheads):
    B, L, _ = x.shape
    return x.view(B, L, nheads, DH).transpose(1, 2)          # [B, heads, L, 32]


def attention(q, k, v, nheads):
    """q [B, lq, d], k / v [B, lk, d] -> float64 [B, lq, d]: softmax(q k^T / sqrt(32)) v per head"""
    qh, kh, vh = (_heads(t.double(), nheads) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(DH), dim=-1)
    return (p @ vh).transpose(1, 2).reshape(q.shape)


def tiled_attention(prob, mistake=None):
    """The recurrence of mha_mfma_kernel on the problem's buffers, in float64: per 32 keys, rows k0 + j clamped to lk - 1, scores of
    keys >= lk masked, V of keys >= lk zero; running maximum m, sum l = l * f + psum and accumulator acc = acc * f + P V with
    f = exp(m_old - m_new); out = acc / l."""
    assert mistake is None or mistake in MISTAKES, mistake
    B, lq, lk, nh, d = prob.B, prob.lq, prob.lk, prob.nheads, prob.d
    k_lay, v_lay = prob.k_lay, prob.v_lay
    if mistake == "row_pitch_d":
        k_lay, v_lay = (d, k_lay[1], k_lay[2]), (d, v_lay[1], v_lay[2])
    if mistake == "q_stride_for_kv":
        k_lay, v_lay = (k_lay[0], prob.q_lay[1], k_lay[2]), (v_lay[0], prob.q_lay[1], v_lay[2])
    q = _heads(prob.q(), nh)
    k = _heads(strided(prob.kvbuf, B, lk, d, *k_lay).double(), nh)
    v = _heads(strided(prob.kvbuf, B, lk, d, *v_lay).double(), nh)
    scale = 1.0 / math.sqrt(d if mistake == "scale_sqrt_d" else DH)
    m = torch.full((B, nh, lq, 1), -math.inf, dtype=torch.float64)
    l = torch.zeros(B, nh, lq, 1, dtype=torch.float64)
    acc = torch.zeros(B, nh, lq, DH, dtype=torch.float64)
    for k0 in range(0, lk, TILE):
        key = k0 + torch.arange(TILE)
        valid = key < lk
        rows = key.clamp(max=lk - 1)
        s = q @ k[:, :, rows].transpose(-1, -2) * scale          # [B, heads, lq, 32]
        if mistake != "tail_unmasked":
            s = s.masked_fill(~valid, -math.inf)
        vt = v[:, :, rows] * valid.view(-1, 1)                   # the zero padding of the V^T scratch
        mn = torch.maximum(m, s.max(-1, keepdim=True).values)
        f = torch.exp(m - mn)
        p = torch.exp(s - mn)
        psum = p.sum(-1, keepdim=True)
        l = l + psum if mistake == "sum_not_rescaled" else l * f + psum
        acc = (acc if mistake == "acc_not_rescaled" else acc * f) + p @ vt
        m = mn
    return (acc / l).transpose(1, 2).reshape(B, lq, d)


def worst_over_bound(got, want, rtol, atol_rms):
    """the figure test_gpu_kernels.check asserts on: max |got - want| / (atol_rms * rms(want) + rtol * |want|)"""
    got, want = got.double(), want.double()
    rms = float(want.pow(2).mean().sqrt()) + 1e-12
    return float(((got - want).abs() / (atol_rms * rms + rtol * want.abs())).max())


def _round(x, half):
    return x.half().float() if half else x


# ---- EDGE_CASES: dense operands, every key and query count around the kernels' tiles ---------------------------------------------
EDGE_LK = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 97, 129)
EDGE_LQ = (1, 15, 16, 17, 63, 64, 65, 129)
EDGE_CASES = tuple((lq, lk) for lk in EDGE_LK for lq in EDGE_LQ)          # the full cross product


def _dense(name, q, k, v, nheads, **kw):
    """separate dense buffers: k and v behind each other in one flat buffer, pitch d"""
    B, lq, d = q.shape
    lk = k.shape[1]
    kv = torch.cat([k.reshape(-1), v.reshape(-1)])
    return Problem(name, B, lq, lk, nheads, q.reshape(-1).clone(), kv, (d, lq * d, 0), (d, lk * d, 0), (d, lk * d, B * lk * d), d, **kw)


@lru_cache(maxsize=None)
def edge_problem(lq, lk, half):
    """B = 2, 8 heads, d = 256, N(0, 1) operands (rounded to fp16 for the fp16 kernel)"""
    g = torch.Generator().manual_seed(1000 * lq + lk)
    q, k, v = (_round(torch.randn(2, n, 256, generator=g), half) for n in (lq, lk, lk))
    return _dense(f"edge[lq{lq},lk{lk}]", q, k, v, 8)


# ---- LAYOUT_CASES: the pitches and strides the model passes (head.hip: packed q | k | v rows, packed k | v rows per group) ----------
# (kind, B or G, lq, lk, heads, extra columns of an output row)
LAYOUT_CASES = (
    ("self", 3, 52, 52, 8, 0),            # 52 % 32 = 20: the tail class of NUM_PROPOSALS 500
    ("self", 3, 100, 100, 8, 0),
    ("memory", 1, 40, 75, 8, 0),
    ("memory", 3, 40, 75, 8, 0),
    ("memory", 1, 64, 160, 8, 0),
    ("memory", 3, 64, 160, 8, 0),
    ("memory", 3, 40, 75, 8, 64),         # out_ld = d + 64: 64 guard columns behind every output row
    ("self", 3, 52, 52, 3, 0),            # d = 96: the head offset h * 32 with a width that is no power of two
)


@lru_cache(maxsize=None)
def layout_problem(kind, B, lq, lk, nheads, out_pad, half):
    d = nheads * DH
    g = torch.Generator().manual_seed(7 + 31 * lq + lk + nheads + B)
    name = f"{kind}[B{B},lq{lq},lk{lk},heads{nheads},out_ld{d + out_pad}]"
    if kind == "self":          # one [B, M, 3d] buffer: q | k | v in every row
        assert lq == lk
        qkv = _round(torch.randn(B * lq * 3 * d, generator=g), half)
        return Problem(name, B, lq, lk, nheads, qkv, qkv, (3 * d, lq * 3 * d, 0), (3 * d, lq * 3 * d, d), (3 * d, lq * 3 * d, 2 * d), d + out_pad)
    q = _round(torch.randn(B * lq * d, generator=g), half)          # q [G, lq, d], kv [G, lk, 2d]: k | v in every row
    kv = _round(torch.randn(B * lk * 2 * d, generator=g), half)
    return Problem(name, B, lq, lk, nheads, q, kv, (d, lq * d, 0), (2 * d, lk * 2 * d, 0), (2 * d, lk * 2 * d, d), d + out_pad)


def dense_copy(prob):
    """the same q / k / v numbers in dense buffers of pitch d"""
    return _dense(prob.name + "/dense", prob.q().float(), prob.k().float(), prob.v().float(), prob.nheads)


# ---- RANGE_CASES: scores with a known, wide range ---------------------------------------------------------------------------------
# every q row is c_i * 1 (c_i from 0.5 to 1), every k row (t_j / sqrt(32)) * 1: score(i, j) = c_i * t_j in every head, |t_j| <= 12
RANGE_S = 12.0
RANGE_LQ = 40
RANGE_ORDERS = ("ascending", "descending", "peak_last", "peak_first", "flat")
RANGE_CASES = tuple((lk, order) for lk in (33, 97, 300) for order in RANGE_ORDERS)


def range_scores(lk, order):
    S = RANGE_S
    if order == "ascending":          # the maximum rises in every tile
        return torch.linspace(-S, S, lk, dtype=torch.float64)
    if order == "descending":
        return torch.linspace(S, -S, lk, dtype=torch.float64)
    t = torch.full((lk,), 0.0 if order == "flat" else -S, dtype=torch.float64)
    if order == "peak_last":
        t[-1] = S
    elif order == "peak_first":
        t[0] = S
    else:
        assert order == "flat", order
    return t


def range_peak(lk, order):
    """the key whose V row the output is, for the two peaked orders"""
    return {"peak_last": lk - 1, "peak_first": 0}[order]


def range_peak_answer(prob):
    """-> (the peak's V row [B, 1, d], how far the exact output may be from it [B, 1, d]).  The peak's score is c_i * 12, every other
    key's c_i * -12, c_i >= 0.5: the other keys weigh at most lk * e^-12 together, and the output is off the peak's row by at most that
    weight times the largest |v_j - v_peak| of the column.  (lk * e^-12 alone would do for |v_j - v_peak| <= 1; N(0, 1) rows are several
    units apart, and the float64 definition itself is 6e-4 off at 33 keys, three times 33 * e^-12.)"""
    v = prob.v()
    peak = v[:, range_peak(prob.lk, prob.order)].unsqueeze(1)
    return peak, prob.lk * math.exp(-RANGE_S) * (v - peak).abs().max(1, keepdim=True).values


@lru_cache(maxsize=None)
def range_problem(lk, order, half):
    B, nheads, d, lq = 2, 8, 256, RANGE_LQ
    g = torch.Generator().manual_seed(300 + lk)
    c = torch.linspace(0.5, 1.0, lq, dtype=torch.float64)
    t = range_scores(lk, order)
    q = _round(c.float().view(1, lq, 1).expand(B, lq, d).contiguous(), half)
    k = _round((t / math.sqrt(DH)).float().view(1, lk, 1).expand(B, lk, d).contiguous(), half)
    v = _round(torch.randn(B, lk, d, generator=g), half)
    return _dense(f"range[lk{lk},{order}]", q, k, v, nheads, max_score=float(t.abs().max()), order=order)


@lru_cache(maxsize=None)
def reference(prob):
    """attention() on the operands the problem's layouts describe; computed once per problem and shared (do not write to it)"""
    return attention(prob.q(), prob.k(), prob.v(), prob.nheads)
