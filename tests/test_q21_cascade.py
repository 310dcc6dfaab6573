"""Parity of the staged-cascade q21 kernel (GPUE_Q21_PF=8, every
GPUE_Q21_PF8_VAR variant) against the plain numpy reference.

Every comparison is bit-exact int64 equality against ref_q21 of
test_fused_star_edges (pinned to the oracle there); no GPU mode is compared
with another. Three angles:

1. the adversarial case x shape matrix of test_fused_star_edges at 2 blocks
   of 256 and of 1024 threads;
2. stage-fill boundaries: one 64-thread block, rows built so that exactly k
   rows pass the brand test and exactly m of those the supplier test, with
   the passing rows first, last or spread, over a clean and a false-maybe
   background, so that each queue crosses its drain threshold mid-stream in
   some cases and only at the final flush in others;
3. the prefetched pk stream's last pair: quad counts around the main-loop
   span with every row passing the part stage.

GPUE_Q21_PF8_VAR: tens digit = prefetch, ones digit = cascade batch B
(10 = prefetch only, 1 = cascade only, 11 / 12 = both at B = 1 / 2).
"""

import functools

import numpy as np
import pytest

from test_fused_star_edges import (CASES, DATEKEY, MAX32, MIN32, P_FOLD, P_SMALL, _Dev,
                                   case_dims, case_rows, date_dim, false_maybe_keys,
                                   fk_dim, maybe_masks, part_dim, ref_case, ref_q21, shapes)

VARIANTS = ["10", "1", "11", "12"]
ENV = ("GPUE_Q21_PF", "GPUE_Q21_PF8_VAR", "GPUE_Q21_PF_NT", "GPUE_Q21_PF_TPB",
       "GPUE_GRID_PF")


@pytest.fixture(scope="module")
def dev(engine):
    d = _Dev(engine)
    yield d
    d.close()


def _mode8(monkeypatch, var, grid, tpb):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("GPUE_Q21_PF", "8")
    monkeypatch.setenv("GPUE_Q21_PF8_VAR", var)
    monkeypatch.setenv("GPUE_GRID_PF", str(grid))
    monkeypatch.setenv("GPUE_Q21_PF_TPB", str(tpb))


# ---------------------------------------------------------------------------
# 1. the existing adversarial matrix
# ---------------------------------------------------------------------------
N_1024 = max(shapes(2 * 1024))     # beyond the shared NMAX-row columns
_REFS_1024 = {}


def _ref_1024(name, n):
    if (name, n) not in _REFS_1024:
        _, sk, pk, od, rv, _ = (c[:n] for c in case_rows(name, N_1024))
        parts, supps, _, dates = case_dims(name, "q21")
        _REFS_1024[name, n] = ref_q21(pk, sk, od, rv, parts, supps, dates)
    return _REFS_1024[name, n]


@pytest.mark.gpu
@pytest.mark.parametrize("var", VARIANTS)
@pytest.mark.parametrize("tpb", [256, 1024])
def test_q21_cascade_adversarial_matrix(dev, monkeypatch, tpb, var):
    _mode8(monkeypatch, var, 2, tpb)
    bad = []
    for name in CASES:
        parts, supps, _, dates = dev.tables(name, "q21")
        if tpb == 256:
            _, sk, pk, od, rv, _ = dev.case(name)
        else:
            _, sk, pk, od, rv, _ = dev.rows(("n1024", name), case_rows(name, N_1024))
        for n in shapes(2 * tpb):
            exp = ref_case("q21", name, n) if tpb == 256 else _ref_1024(name, n)
            got = dev.eng.q21_star_agg(parts, supps, dates, pk, sk, od, rv, n)
            if not np.array_equal(got, exp):
                bad.append((name, n))
    assert not bad, f"PF=8 VAR={var} TPB={tpb} differs at (case, n): {bad[:12]} ({len(bad)})"


# ---------------------------------------------------------------------------
# 2. stage-fill boundaries: one wave, stride 64 quads
# ---------------------------------------------------------------------------
S_FILL = 64
Q_FILL = 2 * (2 * S_FILL) + S_FILL + 17      # 2 main-loop trips, 2 remainder trips
N_FILL = 4 * Q_FILL + 3                      # + a 3-row tail
KM = (0, 1, 63, 64, 65, 127, 128, 129, 192)
RV_VALUES = np.array([MIN32, MAX32, -1, 1], np.int64)   # no zero: every row counts


def _place(count, total, how):
    """Indices of `count` of `total` slots: first, last or spread evenly."""
    if how == "first":
        return np.arange(count)
    if how == "last":
        return np.arange(total - count, total)
    return np.arange(count) * total // max(count, 1)


@functools.lru_cache(None)
def _fill_dims(bg):
    """clean: every non-passing part key is rejected by the prefilter, so only
    brand-passing rows reach Q1; storm: every non-passing row is a false maybe,
    so Q1 fills on every push whatever k is."""
    parts = part_dim(P_SMALL if bg == "clean" else P_FOLD, "rand4", "q21")
    return parts, fk_dim("rand20", "q21", 1), date_dim("q21")


@functools.lru_cache(None)
def _fill_case(bg, k, m, how):
    """(pk, sk, od, rv) with exactly k brand-passing rows, m of them passing the
    supplier test; the passing rows sit in the quad region (they go through the
    queues), the 3-row tail holds non-passing rows unless k covers every row."""
    parts, supps, dates = _fill_dims(bg)
    rng = np.random.default_rng([k, m, len(how), bg == "storm"])
    pkeys, ppay = parts
    skeys, spay = supps
    p_pass = pkeys[ppay != 0]
    p_fail = pkeys[ppay == 0] if bg == "clean" else false_maybe_keys(parts)
    s_pass, s_fail = skeys[spay != 0], skeys[spay == 0]
    n = N_FILL
    region = n if k == n else 4 * Q_FILL
    rows_k = _place(k, region, how)
    assert len(rows_k) == k
    rows_m = rows_k[_place(m, k, how)]
    assert len(rows_m) == m
    pk = rng.choice(p_fail, n)
    pk[rows_k] = rng.choice(p_pass, k)
    sk = rng.choice(skeys, n)                # non-brand rows: any supplier
    sk[rows_k] = rng.choice(s_fail, k)
    sk[rows_m] = rng.choice(s_pass, m)
    od = rng.choice(DATEKEY, n)
    rv = rng.choice(RV_VALUES, n)
    cols = tuple(np.ascontiguousarray(c, np.int32) for c in (pk, sk, od, rv))
    exp = ref_q21(*cols, parts, supps, dates)
    return cols, exp


FILL_CASES = [(bg, k, m, how) for bg in ("clean", "storm") for how in ("first", "last", "spread")
              for k in KM + (N_FILL,) for m in KM + (N_FILL,) if m <= k]


def test_fill_cases_are_what_they_claim():
    for bg in ("clean", "storm"):
        parts, supps, dates = _fill_dims(bg)
        for k, m, how in ((0, 0, "first"), (65, 64, "spread"), (192, 127, "last"),
                          (N_FILL, N_FILL, "first"), (N_FILL, 0, "first")):
            (pk, sk, od, rv), exp = _fill_case(bg, k, m, how)
            brand = np.isin(pk, parts[0][parts[1] != 0])
            supp = np.isin(sk, supps[0][supps[1] != 0])
            assert brand.sum() == k and (brand & supp).sum() == m
            maybe = maybe_masks(parts, pk)["split18"]
            assert (maybe & ~brand).sum() == (0 if bg == "clean" else len(pk) - k)
            assert exp.any() == (m > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("var", VARIANTS)
def test_q21_cascade_stage_fill_boundaries(dev, monkeypatch, var):
    _mode8(monkeypatch, var, 1, 64)
    pk, sk, od, rv = (dev.buf(nbytes=4 * N_FILL) for _ in range(4))
    bad = []
    for case in FILL_CASES:
        parts, supps, dates = (dev.table(d) for d in _fill_dims(case[0]))
        cols, exp = _fill_case(*case)
        for b, c in zip((pk, sk, od, rv), cols):
            b.h2d(c)
        got = dev.eng.q21_star_agg(parts, supps, dates, pk, sk, od, rv, N_FILL)
        if not np.array_equal(got, exp):
            bad.append(case)
    assert not bad, f"PF=8 VAR={var} differs at (bg, k, m, placement): {bad[:12]} ({len(bad)})"


# ---------------------------------------------------------------------------
# 3. prefetch tail: fold-aliasing part dim, every part passing, so a dropped
#    or twice-consumed pk pair changes the sums
# ---------------------------------------------------------------------------
def _tail_ns(s):
    return [4 * q + t for q in (0, 1, 2 * s - 1, 2 * s, 2 * s + 1, 3 * s + 17) for t in (0, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("var", VARIANTS)
@pytest.mark.parametrize("grid,tpb", [(1, 64), (2, 256)])
def test_q21_cascade_prefetch_tail(dev, monkeypatch, grid, tpb, var):
    _mode8(monkeypatch, var, grid, tpb)
    bad = []
    for name in ("fold-all-D3", "fold-all-D1"):
        parts, supps, _, dates = dev.tables(name, "q21")
        _, sk, pk, od, rv, _ = dev.case(name)
        for n in _tail_ns(grid * tpb):
            got = dev.eng.q21_star_agg(parts, supps, dates, pk, sk, od, rv, n)
            if not np.array_equal(got, ref_case("q21", name, n)):
                bad.append((name, n))
    assert not bad, f"PF=8 VAR={var} {grid}x{tpb} differs at (case, n): {bad[:12]}"
