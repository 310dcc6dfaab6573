"""Parity of the compact-group q21 kernel (GPUE_Q21_PF=9, every
GPUE_Q21_PF9_VAR variant) and of the part table's dense payload rank against
the plain numpy reference.

Every GPU comparison is bit-exact int64 equality against ref_q21 of
test_fused_star_edges (pinned to the oracle there); no GPU mode is compared
with another.

Mode 9 needs a part table with at most 64 distinct nonzero payloads. The
`rand4` (about 113) and `all` (1000) part dims of test_fused_star_edges take
the fallback, so the dims here carry payload 441 + k % 40 on the k-th key of
the same pass sets; the row distributions of CASES depend on the pass set only and are
reused as they are.

1. CPU-only: the inputs are what they claim;
2. rank build and dispatch at 0, 1, 64 and 65 distinct payloads. An empty
   pass set (0 payloads) QUALIFIES: mode 9 runs and returns all zeros;
3. the adversarial case x shape matrix at 2 blocks of 256 and 1024 threads;
4. stage-fill boundaries on one 64-thread block, including rows that are all
   maybes for more than two bursts, so the per-quad overflow guard of the
   deep-Q1 variants fires;
5. burst boundaries: quad counts around one and two K-quad bursts with every
   row passing the part stage.

GPUE_Q21_PF9_VAR -> (fold A bits, Q1 entries per wave, quads per burst K).
"""

import functools

import numpy as np
import pytest

from starrocks_amd.engine import GpueError
from test_fused_star_edges import (CASES, DATEKEY, HASH_MUL, M19, P_FOLD, P_SMALL, _Dev,
                                   case_rows, date_dim, false_maybe_keys, fk_dim,
                                   maybe_masks, part_dim, ref_case, ref_q21, shapes)
from test_q21_cascade import KM, RV_VALUES, _place

VARS = {"1": (18, 128, 1), "2": (19, 128, 1), "3": (18, 384, 4), "4": (19, 320, 4)}
KS = sorted({k for _, _, k in VARS.values()})
ENV = ("GPUE_Q21_PF", "GPUE_Q21_PF8_VAR", "GPUE_Q21_PF9_VAR", "GPUE_Q21_PF_NT",
       "GPUE_Q21_PF_TPB", "GPUE_GRID_PF")
NBC = 64                                        # most payloads the table ranks


@pytest.fixture(scope="module")
def dev(engine):
    d = _Dev(engine)
    yield d
    d.close()


def _env(monkeypatch, mode, var, grid, tpb):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    if mode is not None:
        monkeypatch.setenv("GPUE_Q21_PF", mode)
    if var is not None:
        monkeypatch.setenv("GPUE_Q21_PF9_VAR", var)
    monkeypatch.setenv("GPUE_GRID_PF", str(grid))
    monkeypatch.setenv("GPUE_Q21_PF_TPB", str(tpb))


# ---------------------------------------------------------------------------
# dims
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def compact_part_dim(size, kind):
    """part_dim's pass set with payload 441 + k % 40 on its k-th passing key:
    40 distinct values once 40 keys pass."""
    keys, pay = part_dim(size, kind, "q21")
    k = np.cumsum(pay != 0) - 1
    return keys, np.where(pay != 0, 441 + k % 40, 0).astype(np.uint32)


def _rank_vals(d):
    """d distinct payloads in 1..1000, the values 1 and 1000 among them (d >= 2)."""
    return np.array([1, 1000] + [3 + 16 * i for i in range(d - 2)], np.int64)


RANK_VALS = {"one-lo": np.array([1]), "one-hi": np.array([1000]),
             "d64": _rank_vals(NBC), "d65": _rank_vals(NBC + 1)}


@functools.lru_cache(None)
def rank_part_dim(kind):
    """Every key of a P_SMALL dim passes; payloads cycle through RANK_VALS[kind]
    ('empty': no key passes)."""
    keys = np.arange(1, P_SMALL + 1, dtype=np.int32)
    if kind == "empty":
        return keys, np.zeros(P_SMALL, np.uint32)
    vals = RANK_VALS[kind]
    return keys, vals[(keys.astype(np.int64) * 7) % len(vals)].astype(np.uint32)


def _folds_a19_h18(parts, col):
    """Maybe masks of the 2^19 masked fold and of the 2^18 hashed fold alone."""
    keys, pay = parts
    passing = keys[pay != 0].astype(np.int64)
    smin, smax = int(passing.min()), int(passing.max())

    def fold(k):
        idx = (k - smin).astype(np.uint64)
        h = (idx * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)
        return (idx & np.uint64(M19)).astype(np.int64), (h >> np.uint64(14)).astype(np.int64)

    a19, h18 = np.zeros(2**19, bool), np.zeros(2**18, bool)
    fa, fh = fold(passing)
    a19[fa], h18[fh] = True, True
    k = col.astype(np.int64)
    inr = (k >= smin) & (k <= smax)
    ca, ch = fold(np.where(inr, k, smin))
    return inr & a19[ca], inr & h18[ch]


_REFS = {}


def _ref(parts, supps, tag, cols, n):
    """ref_q21 of the first n rows of cols = (pk, sk, od, rv), computed once."""
    key = (id(parts[1]), id(supps[1]), tag, n)
    if key not in _REFS:
        _REFS[key] = ref_q21(*(c[:n] for c in cols), parts, supps, date_dim("q21"))
    return _REFS[key]


# ---------------------------------------------------------------------------
# 4. (inputs) stage fills: one wave, stride 64 quads; two K=4 bursts, one
#    remainder trip of a full wave and one of 17 lanes, a 3-row tail
# ---------------------------------------------------------------------------
S_FILL = 64
Q_FILL = 2 * (max(KS) * S_FILL) + S_FILL + 17
N_FILL = 4 * Q_FILL + 3


@functools.lru_cache(None)
def _fill_dims(bg):
    """clean: every non-passing part key is rejected by both masked folds, so
    only brand-passing rows reach Q1; storm: every non-passing row is a false
    maybe in every fold, so each quad adds 256 entries to Q1 whatever k is."""
    parts = compact_part_dim(P_SMALL if bg == "clean" else P_FOLD, "rand4")
    return parts, fk_dim("rand20", "q21", 1), date_dim("q21")


@functools.lru_cache(None)
def _fill_case(bg, k, m, how):
    """(pk, sk, od, rv) with exactly k brand-passing rows, m of them passing the
    supplier test; the passing rows sit in the quad region, the 3-row tail
    holds non-passing rows unless k covers every row."""
    parts, supps, dates = _fill_dims(bg)
    rng = np.random.default_rng([k, m, len(how), bg == "storm", 9])
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
    sk = rng.choice(skeys, n)
    sk[rows_k] = rng.choice(s_fail, k)
    sk[rows_m] = rng.choice(s_pass, m)
    od = rng.choice(DATEKEY, n)
    rv = rng.choice(RV_VALUES, n)
    cols = tuple(np.ascontiguousarray(c, np.int32) for c in (pk, sk, od, rv))
    return cols, ref_q21(*cols, parts, supps, dates)


# 448 and 449 rows: a full 384- / 320-deep Q1 plus one batch, and one more
KM9 = KM + (448, 449, N_FILL)
FILL_CASES = [(bg, k, m, how) for bg in ("clean", "storm") for how in ("first", "last", "spread")
              for k in KM9 for m in KM9 if m <= k]


# ---------------------------------------------------------------------------
# 1. CPU-only: the inputs are what they claim
# ---------------------------------------------------------------------------
def test_compact_dims_have_40_payloads():
    for size in (P_SMALL, P_FOLD):
        keys, pay = compact_part_dim(size, "rand4")
        assert len(np.unique(pay[pay != 0])) == 40
        assert np.array_equal(pay != 0, part_dim(size, "rand4", "q21")[1] != 0)
        assert pay.max() <= 1000
    for kind, d in (("one-lo", 1), ("one-hi", 1), ("d64", 64), ("d65", 65), ("empty", 0)):
        pay = rank_part_dim(kind)[1]
        vals = np.unique(pay[pay != 0])
        assert len(vals) == d
        if d >= 2:
            assert vals[0] == 1 and vals[-1] == 1000


def test_fold_dim_has_false_maybes_in_both_folds():
    parts = compact_part_dim(P_FOLD, "rand4")
    fm = false_maybe_keys(parts)
    assert len(fm) > 0
    a19, h18 = _folds_a19_h18(parts, fm)
    assert a19.all() and h18.all()
    assert (parts[1][fm - 1] == 0).all()
    # and the small dim aliases in neither masked fold
    small = compact_part_dim(P_SMALL, "rand4")
    a19, _ = _folds_a19_h18(small, small[0])
    assert np.array_equal(a19, small[1] != 0)


def test_fill_cases_are_what_they_claim():
    for bg in ("clean", "storm"):
        parts, supps, dates = _fill_dims(bg)
        for k, m, how in ((0, 0, "first"), (65, 64, "spread"), (449, 127, "last"),
                          (N_FILL, N_FILL, "first"), (N_FILL, 0, "first")):
            (pk, sk, od, rv), exp = _fill_case(bg, k, m, how)
            brand = np.isin(pk, parts[0][parts[1] != 0])
            supp = np.isin(sk, supps[0][supps[1] != 0])
            assert brand.sum() == k and (brand & supp).sum() == m
            a19, h18 = _folds_a19_h18(parts, pk)
            a18 = maybe_masks(parts, pk)["split18"]          # masked 2^18 and hashed 2^18
            for maybe in (a19 & h18, a18):
                assert (maybe & ~brand).sum() == (0 if bg == "clean" else len(pk) - k)
            assert exp.any() == (m > 0)
    # every row a maybe for more than two bursts of the largest K
    assert N_FILL // 4 > 2 * max(KS) * S_FILL


# ---------------------------------------------------------------------------
# 2. rank build and dispatch
# ---------------------------------------------------------------------------
RANK_NS = (0, 3, 4 * 65 + 1, 4 * (3 * 512 + 17) + 3)


def _rank_run(dev, kind, n):
    parts, supps = rank_part_dim(kind), fk_dim("rand20", "q21", 1)
    _, sk, pk, od, rv, _ = case_rows("small-all-D1")
    _, dsk, dpk, dod, drv, _ = dev.case("small-all-D1")
    got = dev.eng.q21_star_agg(dev.table(parts), dev.table(supps),
                               dev.table(date_dim("q21")), dpk, dsk, dod, drv, n)
    return got, _ref(parts, supps, "small-all-D1", (pk, sk, od, rv), n)


@pytest.mark.gpu
@pytest.mark.parametrize("var", list(VARS))
@pytest.mark.parametrize("kind", ["empty", "one-lo", "one-hi", "d64"])
def test_q21_compact_rank_build(dev, monkeypatch, kind, var):
    _env(monkeypatch, "9", var, 2, 256)
    for n in RANK_NS:
        got, exp = _rank_run(dev, kind, n)
        assert np.array_equal(got, exp), (kind, var, n)
        assert exp.any() == (kind != "empty") or n < RANK_NS[-1]


@pytest.mark.gpu
def test_q21_compact_refuses_65_payloads(dev, monkeypatch):
    _env(monkeypatch, "9", "1", 2, 256)
    with pytest.raises(GpueError):
        _rank_run(dev, "d65", RANK_NS[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["empty", "one-lo", "d64", "d65"])
def test_q21_default_mode_on_ranked_dims(dev, monkeypatch, kind):
    _env(monkeypatch, None, None, 2, 256)
    for n in RANK_NS:
        got, exp = _rank_run(dev, kind, n)
        assert np.array_equal(got, exp), (kind, n)


# ---------------------------------------------------------------------------
# 3. the adversarial matrix: the CASES whose own part dim qualifies (one or no
#    passing key), and every case over the compact dim of its pass set
# ---------------------------------------------------------------------------
N_1024 = max(shapes(2 * 1024))
QUALIFY = [c for c, v in CASES.items() if v[1] in ("empty", "first", "last")]


def _matrix_inputs(dev, name, tpb):
    if tpb == 256:
        return case_rows(name), dev.case(name)
    return case_rows(name, N_1024), dev.rows(("n1024", name), case_rows(name, N_1024))


@pytest.mark.gpu
@pytest.mark.parametrize("var", list(VARS))
@pytest.mark.parametrize("tpb", [256, 1024])
def test_q21_compact_adversarial_matrix(dev, monkeypatch, tpb, var):
    _env(monkeypatch, "9", var, 2, tpb)
    dates = dev.table(date_dim("q21"))
    bad = []
    for name, (size, kind, skind, _) in CASES.items():
        (_, sk, pk, od, rv, _), (_, dsk, dpk, dod, drv, _) = _matrix_inputs(dev, name, tpb)
        supps = fk_dim(skind, "q21", 1)
        dims = [("compact", compact_part_dim(size, kind))]
        if name in QUALIFY:
            dims.append(("own", part_dim(size, kind, "q21")))
        for tag, parts in dims:
            for n in shapes(2 * tpb):
                exp = (ref_case("q21", name, n) if tag == "own" and tpb == 256 else
                       _ref(parts, supps, (name, tpb), (pk, sk, od, rv), n))
                got = dev.eng.q21_star_agg(dev.table(parts), dev.table(supps), dates,
                                           dpk, dsk, dod, drv, n)
                if not np.array_equal(got, exp):
                    bad.append((name, tag, n))
    assert not bad, f"PF=9 VAR={var} TPB={tpb} differs at (case, dim, n): {bad[:12]} ({len(bad)})"


# ---------------------------------------------------------------------------
# 4. stage-fill boundaries
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("var", list(VARS))
def test_q21_compact_stage_fill_boundaries(dev, monkeypatch, var):
    _env(monkeypatch, "9", var, 1, 64)
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
    assert not bad, f"PF=9 VAR={var} differs at (bg, k, m, placement): {bad[:12]} ({len(bad)})"


# ---------------------------------------------------------------------------
# 5. burst boundaries: every part key passes, so a dropped or twice-consumed
#    quad of a burst changes the sums
# ---------------------------------------------------------------------------
def _burst_ns(k, s):
    return [4 * q + t for q in (0, 1, k * s - 1, k * s, k * s + 1, (k + 1) * s + 17,
                                2 * k * s + 5) for t in (0, 3)]


N_BURST = max(_burst_ns(max(KS), 512))


@pytest.mark.gpu
@pytest.mark.parametrize("var", list(VARS))
@pytest.mark.parametrize("grid,tpb", [(1, 64), (2, 256)])
def test_q21_compact_burst_boundaries(dev, monkeypatch, grid, tpb, var):
    _env(monkeypatch, "9", var, grid, tpb)
    parts, supps = compact_part_dim(P_FOLD, "all"), fk_dim("rand20", "q21", 1)
    dates = dev.table(date_dim("q21"))
    bad = []
    for name in ("fold-all-D3", "fold-all-D1"):
        _, sk, pk, od, rv, _ = case_rows(name, N_BURST)
        _, dsk, dpk, dod, drv, _ = dev.rows(("burst", name), case_rows(name, N_BURST))
        for n in _burst_ns(VARS[var][2], grid * tpb):
            got = dev.eng.q21_star_agg(dev.table(parts), dev.table(supps), dates,
                                       dpk, dsk, dod, drv, n)
            if not np.array_equal(got, _ref(parts, supps, ("burst", name), (pk, sk, od, rv), n)):
                bad.append((name, n))
    assert not bad, f"PF=9 VAR={var} {grid}x{tpb} differs at (case, n): {bad[:12]}"
