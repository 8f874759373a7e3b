"""CPU side of tests/test_gpu_mha.py: the float64 references of the head's attention (tests/_mha_ref.py) against each other, and the
power of the parity test's cases to tell a wrong kernel from a right one.  No GPU.

What tells what (fp16-rounded operands, worst/bound of `check` with the fp16 bound 4e-3 relative + 4e-3 of RMS; one seed per case):
  tail_unmasked     every lk with lk % 32 not in {0, 31}, any lq: 100-200 x (lk = 1: ~180 x); lk in {31, 63}: 30-50 x, one duplicate
                    key only, so they are not relied on; lk % 32 == 0: exactly 0.  The self / memory layouts with a tail (52, 100, 75
                    keys) 130-170 x; range `flat` 91 / 46 / 11 x at 33 / 97 / 300 keys.
  sum_not_rescaled  every edge case with lk >= 33 and lq >= 15: 55-200 x (one query per (batch, head) may have its maximum in the
                    first tile); the layouts 130-190 x; range `ascending` 66-175 x and `peak_last` ~185 x; exactly 0 with lk <= 32 and
                    on `descending`, `peak_first` and `flat` (the maximum never moves after the first tile).
  acc_not_rescaled  the same cases: 200-4300 x (edge), 1100-4100 x (layouts), 350-2000 x (`ascending`), 3500-9500 x (`peak_last`).
  scale_sqrt_d      every case but lk = 1 and `flat`: 64-550 x.
  row_pitch_d       every layout case, and no dense one: 770-4000 x.
  q_stride_for_kv   the memory layouts with three groups: 1100-1550 x; exactly 0 with one group and in self-attention (one buffer,
                    one stride).  Dense edge cases with lq != lk tell it too (two batches), 180-1300 x.
The test prints the whole table (pytest -s); `_must_tell` holds the claims above, so taking a case away shows what it was for."""
import pytest
import torch

import _mha_ref as ref

FP16_BOUND = (4e-3, 4e-3)          # rtol, atol of RMS: what test_gpu_mha.py allows the fp16 kernel (test_mha_mfma's bound)
MIN_RATIO = 20.0                   # as tests/test_swin_ref.py


def _problems():
    return ([ref.edge_problem(lq, lk, True) for lq, lk in ref.EDGE_CASES] + [ref.layout_problem(*c, True) for c in ref.LAYOUT_CASES] +
            [ref.range_problem(lk, order, True) for lk, order in ref.RANGE_CASES])


def _kind(p):
    return p.name.split("[")[0]


def _must_tell(mistake, p):
    """True: this case is relied on to tell the mistake (>= MIN_RATIO); False: it cannot see it at all (factor 0); None: no claim"""
    kind, tail = _kind(p), p.lk % ref.TILE
    if mistake == "tail_unmasked":
        if tail == 0:
            return False
        if tail == 31 or p.order is not None:          # one duplicate key / a tail whose weight depends on the order: not relied on
            return None
        return True
    if mistake in ("sum_not_rescaled", "acc_not_rescaled"):
        if p.lk <= ref.TILE or p.order in ("descending", "peak_first", "flat"):
            return False
        return True if p.lq >= 15 else None          # one query per (batch, head): its maximum may sit in the first tile
    if mistake == "scale_sqrt_d":
        return not (p.lk == 1 or p.order == "flat")
    if mistake == "row_pitch_d":
        return kind in ("self", "memory")
    if mistake == "q_stride_for_kv":
        if kind == "memory":
            return p.B > 1
        if kind == "self":
            return False
        return None
    raise AssertionError(mistake)


@pytest.fixture(scope="module")
def table():
    """{mistake: {case name: worst/bound}} and the largest |tiled - definition| per case"""
    ratios, exact = {m: {} for m in ref.MISTAKES}, {}
    for p in _problems():
        want = ref.reference(p)
        assert torch.isfinite(want).all() and tuple(want.shape) == (p.B, p.lq, p.d)
        exact[p.name] = float((ref.tiled_attention(p) - want).abs().max())
        for m in ref.MISTAKES:
            ratios[m][p.name] = ref.worst_over_bound(ref.tiled_attention(p, m), want, *FP16_BOUND)
    return ratios, exact


def test_case_tables_cover_the_tile_edges():
    """every lk with lq in {17, 65}, every lq with lk in {33, 64}; the layouts: both packings, the tail class of 500 proposals, one
    padded output pitch, one width that is no power of two"""
    cases = set(ref.EDGE_CASES)
    assert all((lq, lk) in cases for lk in ref.EDGE_LK for lq in (17, 65))
    assert all((lq, lk) in cases for lq in ref.EDGE_LQ for lk in (33, 64))
    assert {lk % 32 for lk in ref.EDGE_LK} >= {0, 1, 15, 16, 17, 31} and {lk % 64 for lk in ref.EDGE_LK} >= {0, 1, 16, 32, 48, 63}
    assert any(c[0] == "self" and c[3] % 32 == 500 % 32 for c in ref.LAYOUT_CASES)
    assert sum(c[5] > 0 for c in ref.LAYOUT_CASES) == 1 and sum(c[4] == 3 for c in ref.LAYOUT_CASES) == 1
    assert {(c[1], c[2], c[3]) for c in ref.LAYOUT_CASES if c[0] == "memory"} >= {(G, lq, lk) for G in (1, 3) for lq, lk in ((40, 75), (64, 160))}


def test_the_tiled_recurrence_is_the_definition(table):
    """tiled_attention(mistake=None) equals attention to 1e-10 on every case: clamped tail rows, masked tail scores and zero padded V
    change nothing, and neither does any order of the running maximum"""
    _, exact = table
    for name, err in exact.items():
        assert err <= 1e-10, f"{name}: {err:.2e}"


def test_every_mistake_is_told_by_named_cases(table):
    """Each deliberate mistake moves the reference by at least 20 times the fp16 bound on every case `_must_tell` names for it, and by
    nothing on the cases that cannot see it; every mistake has at least three telling cases.  The table is printed."""
    ratios, _ = table
    probs = _problems()
    for m in ref.MISTAKES:
        tellers = {p.name: ratios[m][p.name] for p in probs if ratios[m][p.name] >= MIN_RATIO}
        by_kind = {}
        for p in probs:
            if p.name in tellers:
                by_kind.setdefault(_kind(p), []).append(tellers[p.name])
        print(f"{m}: told by {len(tellers)} cases; " + "; ".join(f"{k} {len(v)} cases {min(v):.0f}-{max(v):.0f} x" for k, v in by_kind.items()))
        for p in probs:
            if _kind(p) != "edge" or p.lq in (17, 65):
                print(f"    {p.name}: {ratios[m][p.name]:.1f}")
        named = 0
        for p in probs:
            claim, r = _must_tell(m, p), ratios[m][p.name]
            if claim is True:
                named += 1
                assert r >= MIN_RATIO, f"{m}: {p.name} moves the reference by only {r:.1f} x the bound"
            elif claim is False:
                assert r < 1e-6, f"{m}: {p.name} was thought blind to it, factor {r:.3g}"
        assert named >= 3, (m, named)


def test_layout_mistakes_are_told_by_the_layout_cases(table):
    """the two addressing mistakes need the packed cases: a wrong row pitch shows in every one of them and in no dense case, the query's
    batch stride used for K / V in the memory cases with more than one group"""
    ratios, _ = table
    for c in ref.LAYOUT_CASES:
        p = ref.layout_problem(*c, True)
        assert ratios["row_pitch_d"][p.name] >= MIN_RATIO, p.name
        if c[0] == "memory" and c[1] > 1:
            assert ratios["q_stride_for_kv"][p.name] >= MIN_RATIO, p.name
    for lq, lk in ref.EDGE_CASES:
        assert ratios["row_pitch_d"][ref.edge_problem(lq, lk, True).name] < 1e-6


def test_strided_reader_and_dense_copy():
    """the reader returns what plain indexing of the packed tensor returns, and a layout case's dense copy holds the same numbers"""
    for c in ref.LAYOUT_CASES:
        p = ref.layout_problem(*c, False)
        d = p.d
        if c[0] == "self":
            qkv = p.kvbuf.view(p.B, p.lq, 3 * d)
            parts = (qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:])
        else:
            kv = p.kvbuf.view(p.B, p.lk, 2 * d)
            parts = (p.qbuf.view(p.B, p.lq, d), kv[..., :d], kv[..., d:])
        dense = ref.dense_copy(p)
        for got, copy, want in zip((p.q(), p.k(), p.v()), (dense.q(), dense.k(), dense.v()), parts):
            assert torch.equal(got, want.double()) and torch.equal(copy, want.double())
        assert dense.q_lay[0] == dense.k_lay[0] == dense.out_ld == d


def test_range_cases_have_the_known_answers():
    """score(i, j) = c_i t_j in every head, exactly up to the operands' rounding; `flat` is the mean of the V rows; the peaked orders
    give the peak's V row to within lk * e^-12 (c_i >= 0.5, gap 24) times the column's largest |v_j - v_peak| -- what
    test_gpu_mha.py adds to the kernel's bound"""
    import math
    for half in (True, False):
        for lk, order in ref.RANGE_CASES:
            p = ref.range_problem(lk, order, half)
            want = ref.reference(p)
            s = (p.q()[0, :, :32] @ p.k()[0, :, :32].T) / math.sqrt(32)
            c, t = torch.linspace(0.5, 1.0, p.lq, dtype=torch.float64), ref.range_scores(lk, order)
            assert (s - c.view(-1, 1) * t.view(1, -1)).abs().max() <= 12 * 2.0 ** -10          # two fp16 roundings at most
            assert p.max_score == (0.0 if order == "flat" else 12.0)
            if order == "flat":
                assert (want - p.v().mean(1, keepdim=True)).abs().max() <= 1e-12
            elif order.startswith("peak"):
                peak, slack = ref.range_peak_answer(p)
                assert ((want - peak).abs() <= slack).all()
                assert slack.max() <= 12 * lk * math.exp(-12.0)          # N(0, 1) rows: a span of a few units, no more
