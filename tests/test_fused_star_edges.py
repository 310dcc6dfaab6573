"""Adversarial-shape parity for the fused probe+aggregate kernels (q1, q21,
q43) and their untested entry points.

The seeded SF100 generator feeds these kernels one distribution (uniform
keys, ~4 % part pass rate, ~10 % maybes) at one shape regime (n % 4 == 0,
~1 M-row grid stride). Here the kernels get caller columns the C-ABI permits
but the generator never produces — 100 % maybe rates, bursts of one key,
false-maybe storms, keys outside the dim range, empty / full / single-key
pass sets, int32-extreme measures — at the row counts where the full-wave
main loop, the predicated remainder loop, the partial queue drain and the
scalar row tail each run alone and together, for every kernel variant the
dispatchers can select.

Every comparison is bit-exact int64 equality against the plain numpy
references below (int64 accumulation via np.add.at). The CPU tests pin those
references to the oracle kernels on every distribution that keeps keys in
range.

Input contract the kernels leave to the caller (all inputs here hold to it):
od values come only from real date keys (the q21/q43 date probe is not
bounds-checked; for q1 the probed dim's own keys), every q21 date key carries
a payload in 1..7, part payloads are 0 or 1..1000 (q21) / 1..40 (q43), spay
0..10, dpay 0..2, part / supplier / customer dim keys are dense from 1, all
payloads < 65536 and every column holds >= 16 bytes even when n == 0.

Not covered: GPUE_Q21_PF=0 and GPUE_Q21_GLOB are cached in function statics
at first use and cannot be switched inside one process.
"""

import functools
import zlib

import numpy as np
import pytest

from oracle import pyoracle as orc
from starrocks_amd import gen

MIN32, MAX32 = -2**31, 2**31 - 1
EXTREMES = np.array([MIN32, MAX32, -1, 0], np.int64)
DATEKEY, DYEAR = gen.gen_dates()
DATEKEY = DATEKEY.astype(np.int32)
NG_Q21, NG_Q43 = 7000, 800

P_SMALL = 3000                 # pass-set range < 2^18: neither fold aliases
P_FOLD = 2 * 2**19 + 5000      # the 2^19 fold and the 2^18 split folds alias
N_FK = 2000                    # supplier / customer dim size
M18, M19 = 2**18 - 1, 2**19 - 1
HASH_MUL = 2654435761

S_Q21 = 2 * 256                # GPUE_GRID_PF=2 x GPUE_Q21_PF_TPB=256 quads
S_Q43 = 1 * 1024               # GPUE_GRID_Q43=1 x the fixed 1024-thread block
S0 = 256 * 1024                # default geometry: 256 blocks x 1024 threads
N_BIG = 4 * (2 * S0 + 64) + 3
Q1_NS = (0, 1, 3, 5, 4 * 1024 * 3 + 2)
PIPE_NS = (3, 39, 4099, 4096, 1_000_003)


def shapes(s):
    """n = 4*q + t around the stride s (in quads): the smallest sizes at which
    the main loop, the masked remainder, the partial drain and the row tail
    run separately and together."""
    qs = (0, 1, 63, 64, 65, s - 1, s, s + 1, s + 63, s + 64,
          2 * s - 1, 2 * s, 2 * s + 63, 2 * s + 64, 3 * s + 17)
    return [4 * q + t for q in qs for t in (0, 1, 3)]


NMAX = max(shapes(S_Q43))


# ---------------------------------------------------------------------------
# plain numpy references: dims are (keys, payloads); a key absent from a dim
# or outside its key range is no match (join semantics)
# ---------------------------------------------------------------------------
_DENSE = {}


def _probe(col, dim):
    """Payload of each row's key in dim; 0 where the key is absent / outside."""
    keys, pay = dim
    memo = _DENSE.get(id(pay))
    if memo is None or memo[0] is not pay:
        lo, hi = int(keys.min()), int(keys.max())
        table = np.zeros(hi - lo + 1, np.int64)
        table[keys.astype(np.int64) - lo] = pay
        memo = _DENSE[id(pay)] = (pay, lo, hi, table)
    _, lo, hi, table = memo
    k = col.astype(np.int64)
    inr = (k >= lo) & (k <= hi)
    return np.where(inr, table[np.where(inr, k - lo, 0)], 0)


def ref_q1(od, ep, dc, dates):
    ok = _probe(od, dates) != 0
    acc = np.zeros(1, np.int64)
    np.add.at(acc, np.zeros(int(ok.sum()), np.intp),
              ep[ok].astype(np.int64) * dc[ok].astype(np.int64))
    return int(acc[0]), int(ok.sum())


def ref_q21(pk, sk, od, rv, parts, supps, dates):
    brand1, spay, year1 = _probe(pk, parts), _probe(sk, supps), _probe(od, dates)
    ok = (brand1 != 0) & (spay != 0) & (year1 != 0)
    out = np.zeros(NG_Q21, np.int64)
    np.add.at(out, (year1[ok] - 1) * 1000 + (brand1[ok] - 1), rv[ok].astype(np.int64))
    return out


def ref_q43(ck, sk, pk, od, rv, sc, custs, supps, parts, dates):
    ppay, spay = _probe(pk, parts), _probe(sk, supps)
    cpay, dpay = _probe(ck, custs), _probe(od, dates)
    ok = (ppay != 0) & (spay != 0) & (cpay != 0) & (dpay != 0)
    out = np.zeros(NG_Q43, np.int64)
    np.add.at(out, (dpay[ok] - 1) * 400 + (spay[ok] - 1) * 40 + (ppay[ok] - 1),
              rv[ok].astype(np.int64) - sc[ok].astype(np.int64))
    return out


# ---------------------------------------------------------------------------
# dims
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def part_dim(size, kind, wl):
    keys = np.arange(1, size + 1, dtype=np.int32)
    mask = np.zeros(size, bool)
    if kind == "all":
        mask[:] = True
    elif kind == "first":
        mask[0] = True
    elif kind == "last":
        mask[-1] = True
    elif kind == "rand4":
        mask = np.random.default_rng(size).random(size) < 0.04
    else:
        assert kind == "empty"
    k = keys.astype(np.int64)
    pay = 1 + (k * 7919) % 1000 if wl == "q21" else 1 + (k * 31) % 40
    return keys, np.where(mask, pay, 0).astype(np.uint32)


@functools.lru_cache(None)
def fk_dim(kind, wl, seed):
    """Supplier (seed 1) / customer (seed 2) dim: ~20 % random pass set."""
    keys = np.arange(1, N_FK + 1, dtype=np.int32)
    mask = np.random.default_rng(seed).random(N_FK) < (0.0 if kind == "empty" else 0.2)
    pay = 1 + keys.astype(np.int64) % 10 if wl == "q43" else np.ones(N_FK, np.int64)
    return keys, np.where(mask, pay, 0).astype(np.uint32)


@functools.lru_cache(None)
def date_dim(wl):
    if wl == "q21":
        pay = DYEAR - 1991                       # every key: 1..7
    elif wl == "q43":
        pay = np.where(DYEAR == 1997, 1, np.where(DYEAR == 1998, 2, 0))
    else:                                        # q1: semi join on d_year = 1993
        pay = np.where(DYEAR == 1993, 2, 0)
    return DATEKEY, pay.astype(np.uint32)


@functools.lru_cache(None)
def q1_wide_dim():
    """Date-like dim whose nonzero payloads span > 262144 keys: the pass-set
    bitset no longer fits the LDS budget, so launch_q1 takes k_q1_join_sum."""
    rng = np.random.default_rng(7)
    keys = np.unique(np.concatenate([[1, 300_001], rng.integers(2, 300_001, 400)]))
    pay = np.where(rng.random(len(keys)) < 0.6, 3, 0)
    pay[0] = pay[-1] = 3
    return keys.astype(np.int32), pay.astype(np.uint32)


def dense_first(dim):
    """Direct-mapped payload array over [min key, max key] (oracle layout)."""
    keys, pay = dim
    lo, hi = int(keys.min()), int(keys.max())
    first = np.zeros(hi - lo + 1, np.uint32)
    first[keys.astype(np.int64) - lo] = pay
    return lo, hi, first


# ---------------------------------------------------------------------------
# prefilter folds, mirrored from k_build_prefilter / _split / _split_w: index
# relative to the pass set's minimum key; & (2^19-1), & (2^18-1),
# (index * 2654435761 mod 2^32) >> 14 and >> 13
# ---------------------------------------------------------------------------
def maybe_masks(parts, col):
    """Per prefilter layout: rows of col the LDS prefilter reports as maybe."""
    keys, pay = parts
    passing = keys[pay != 0].astype(np.int64)
    smin, smax = int(passing.min()), int(passing.max())

    def fold(k):
        idx = (k - smin).astype(np.uint64)
        h = (idx * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)
        return ((idx & np.uint64(M19)).astype(np.int64), (idx & np.uint64(M18)).astype(np.int64),
                (h >> np.uint64(13)).astype(np.int64), (h >> np.uint64(14)).astype(np.int64))

    bits = [np.zeros(2**19, bool), np.zeros(2**18, bool),
            np.zeros(2**19, bool), np.zeros(2**18, bool)]
    for b, f in zip(bits, fold(passing)):
        b[f] = True
    k = col.astype(np.int64)
    inr = (k >= smin) & (k <= smax)
    a19, a18, h19, h18 = fold(np.where(inr, k, smin))
    return {"fold19": inr & bits[0][a19],
            "split18": inr & bits[1][a18] & bits[3][h18],
            "split19w": inr & bits[0][a19] & bits[2][h19]}


def false_maybe_keys(parts):
    """Non-passing dim keys that every prefilter layout reports as maybe."""
    keys, pay = parts
    m = maybe_masks(parts, keys)
    return keys[(pay == 0) & m["fold19"] & m["split18"] & m["split19w"]]


# ---------------------------------------------------------------------------
# row distributions (generated once at NMAX rows; every n is a prefix)
# ---------------------------------------------------------------------------
CASES = {}   # name -> (part dim size, part pass set, supplier set, distribution)
for _size, _tag in ((P_SMALL, "small"), (P_FOLD, "fold")):
    for _kind in ("empty", "all", "first", "last", "rand4"):
        CASES[f"{_tag}-{_kind}-D1"] = (_size, _kind, "rand20", "D1")
        if _kind != "empty":
            CASES[f"{_tag}-{_kind}-D2"] = (_size, _kind, "rand20", "D2")
    CASES[f"{_tag}-rand4-D6"] = (_size, "rand4", "rand20", "D6")
CASES.update({
    "fold-all-D3": (P_FOLD, "all", "rand20", "D3"),
    "fold-rand4-D4": (P_FOLD, "rand4", "rand20", "D4"),
    "small-rand4-D5": (P_SMALL, "rand4", "rand20", "D5"),
    "small-first-D5": (P_SMALL, "first", "rand20", "D5"),
    "fold-rand4-D5": (P_FOLD, "rand4", "rand20", "D5"),
    "fold-all-D5": (P_FOLD, "all", "rand20", "D5"),
    "fold-last-D5": (P_FOLD, "last", "rand20", "D5"),
    "fold-rand4-D7": (P_FOLD, "rand4", "rand20", "D7"),
    "small-all-D7": (P_SMALL, "all", "rand20", "D7"),
    "small-all-D1-nosupp": (P_SMALL, "all", "empty", "D1"),
    "fold-rand4-D2-nosupp": (P_FOLD, "rand4", "empty", "D2"),
})
IN_RANGE_CASES = [c for c, v in CASES.items() if v[3] != "D5"]


def case_dims(name, wl):
    size, kind, skind, _ = CASES[name]
    return (part_dim(size, kind, wl), fk_dim(skind, wl, 1), fk_dim("rand20", wl, 2),
            date_dim(wl))


def _specials(dim):
    """D5: 0, -1, the int32 extremes, dim size + 1, pass-set min - 1 and
    pass-set max + 1 (an empty pass set is the library's [min key, min key])."""
    keys, pay = dim
    passing = keys[pay != 0]
    smin, smax = (int(passing.min()), int(passing.max())) if len(passing) else (1, 1)
    return np.array([0, -1, MIN32, MAX32, len(keys) + 1, smin - 1, smax + 1], np.int64)


def _interleave(col, specials, phase):
    """Specials on every 5th row from `phase` (5 is coprime to the quad width,
    so each special visits every quad slot); the key columns use different
    phases, so a row has at most one out-of-range key."""
    col = col.copy()
    col[phase::5] = np.resize(specials, len(col[phase::5]))
    return col


def _gen_fk(dim, n, rng, p_pass=0.7):
    keys, pay = dim
    passing = keys[pay != 0]
    col = rng.integers(1, len(keys) + 1, n)
    if len(passing):
        col = np.where(rng.random(n) < p_pass, rng.choice(passing, n), col)
    return col


def _gen_pk(dist, parts, n, rng):
    keys, pay = parts
    size, passing = len(keys), keys[pay != 0]
    if dist == "D1":                     # uniform over the dim range
        return rng.integers(1, size + 1, n)
    if dist == "D2":                     # one passing key on every row
        return np.full(n, passing[len(passing) // 2])
    if dist == "D3":                     # distinct keys, all pass: 100 % maybes
        assert len(passing) == size >= n
        return rng.permutation(size)[:n] + 1
    if dist == "D4":                     # >= 95 % false maybes, rest true matches
        pk = rng.choice(false_maybe_keys(parts), n)
        true = rng.random(n) < 0.04
        pk[true] = rng.choice(passing, int(true.sum()))
        return pk
    if dist == "D5":                     # half passing keys; specials interleaved later
        return _gen_fk(parts, n, rng, 0.5)
    if dist == "D6":                     # runs of equal keys, run length 1..200
        runs = rng.integers(1, 201, n)
        vals = np.where(rng.random(n) < 0.5, rng.choice(passing, n),
                        rng.integers(1, size + 1, n))
        return np.repeat(vals, runs)[:n]
    assert dist == "D7"                  # few keys: many rows per group
    return rng.choice(passing[:3], n)


@functools.lru_cache(None)
def case_rows(name, n=NMAX):
    """(ck, sk, pk, od, rv, sc) int32 columns; q21 uses (pk, sk, od, rv)."""
    size, kind, skind, dist = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    parts, supps, custs, _ = case_dims(name, "q21")   # pass sets do not depend on wl
    pk = _gen_pk(dist, parts, n, rng)
    sk, ck = _gen_fk(supps, n, rng), _gen_fk(custs, n, rng)
    od = rng.choice(DATEKEY, n)
    rv, sc = rng.integers(-10**7, 10**7, n), rng.integers(1, 10**5, n)
    if dist == "D5":
        pk = _interleave(pk, _specials(parts), 0)
        sk = _interleave(sk, _specials(supps), 1)
        ck = _interleave(ck, _specials(custs), 2)
    if dist == "D7":                     # int32 extremes, few groups, biased signs
        od = rng.choice(DATEKEY[DYEAR == 1997][:3], n)
        rv = rng.choice(EXTREMES, n, p=[0.2, 0.4, 0.2, 0.2])
        sc = rng.choice(EXTREMES, n, p=[0.4, 0.2, 0.2, 0.2])
    return tuple(np.ascontiguousarray(c, np.int32) for c in (ck, sk, pk, od, rv, sc))


def big_rows():
    """D1 over the folding dim's key range at the default-geometry size (the
    pk column is uniform, so it serves every pass set of that dim)."""
    return case_rows("fold-rand4-D1", N_BIG)


_REFS = {}


def ref_case(wl, name, n, big=False):
    """Reference group sums of the first n rows of a case (computed once);
    big: the first n rows of big_rows() against the dims of case `name`."""
    key = (wl, name, n, big)
    if key not in _REFS:
        ck, sk, pk, od, rv, sc = (c[:n] for c in (big_rows() if big else case_rows(name)))
        parts, supps, custs, dates = case_dims(name, wl)
        _REFS[key] = (ref_q21(pk, sk, od, rv, parts, supps, dates) if wl == "q21" else
                      ref_q43(ck, sk, pk, od, rv, sc, custs, supps, parts, dates))
    return _REFS[key]


# q1 rows -------------------------------------------------------------------
Q1_DIMS = {"dates": lambda: date_dim("q1"), "wide": q1_wide_dim}
# D7 products on matching rows, in an order whose every prefix total stays
# far inside int64 (the +-2^62 terms cancel pairwise); one MIN x MIN row
_Q1_PAIRS = np.array([(MIN32, MAX32), (MAX32, MAX32), (-1, MIN32), (MAX32, MIN32),
                      (MAX32, MAX32), (0, MAX32), (MAX32, -1), (-1, -1)], np.int64)


@functools.lru_cache(None)
def q1_rows(dim_name, dist):
    keys, pay = Q1_DIMS[dim_name]()
    n = max(Q1_NS)
    rng = np.random.default_rng(zlib.crc32(f"{dim_name}-{dist}".encode()))
    passing = keys[pay != 0]
    od = np.where(rng.random(n) < 0.5, rng.choice(passing, n), rng.choice(keys, n))
    ep, dc = rng.integers(1, 100_001, n), rng.integers(0, 11, n)
    if dist == "D5":
        # od stays on the dim's own keys (contract); the out-of-range probes
        # are the dim keys outside the pass-set range and at its edges
        below, above = keys[keys < passing.min()], keys[keys > passing.max()]
        edge = [keys.min(), keys.max(), passing.min(), passing.max()]
        edge += [below.max()] if len(below) else []
        edge += [above.min()] if len(above) else []
        od = _interleave(od, np.array(edge, np.int64), 0)
    if dist == "D7":
        od[:8] = passing[len(passing) // 2]
        match = np.flatnonzero(_probe(od, (keys, pay)) != 0)
        ep, dc = rng.choice(EXTREMES, n), rng.choice(EXTREMES, n)
        pairs = _Q1_PAIRS[(np.arange(len(match)) - 1) % len(_Q1_PAIRS)]
        pairs[0] = (MIN32, MIN32)
        ep[match], dc[match] = pairs[:, 0], pairs[:, 1]
    return tuple(np.ascontiguousarray(c, np.int32) for c in (od, ep, dc))


# ---------------------------------------------------------------------------
# CPU tests: the references against the oracle kernels; the distributions
# ---------------------------------------------------------------------------
CPU_NS = (0, 1, 3, 4 * (S_Q21 + 64) + 1, max(shapes(S_Q21)), NMAX)


@pytest.mark.parametrize("name", IN_RANGE_CASES)
def test_ref_q21_matches_oracle(name):
    parts, supps, _, dates = case_dims(name, "q21")
    dmin, _, dfirst = dense_first(dates)
    pfirst, sfirst = dense_first(parts)[2], dense_first(supps)[2]
    for n in CPU_NS:
        _, sk, pk, od, rv, _ = (np.ascontiguousarray(c[:n]) for c in case_rows(name))
        exp = orc.q21_kernel(pk, sk, od, rv, pfirst, sfirst, dfirst, dmin)
        assert np.array_equal(ref_case("q21", name, n), exp), (name, n)


@pytest.mark.parametrize("name", IN_RANGE_CASES)
def test_ref_q43_matches_oracle(name):
    parts, supps, custs, dates = case_dims(name, "q43")
    dmin, _, dfirst = dense_first(dates)
    cfirst, sfirst, pfirst = (dense_first(d)[2] for d in (custs, supps, parts))
    for n in CPU_NS:
        ck, sk, pk, od, rv, sc = (np.ascontiguousarray(c[:n]) for c in case_rows(name))
        exp = orc.q43_kernel(ck, sk, pk, od, rv, sc, cfirst, sfirst, pfirst, dfirst, dmin)
        assert np.array_equal(ref_case("q43", name, n), exp), (name, n)


def test_ref_big_rows_match_oracle():
    """The default-geometry / pipe columns, both pass sets of the folding dim."""
    ck, sk, pk, od, rv, sc = big_rows()
    for name in ("fold-rand4-D1", "fold-all-D1"):
        parts, supps, _, dates = case_dims(name, "q21")
        dmin, _, dfirst = dense_first(dates)
        exp = orc.q21_kernel(pk, sk, od, rv, dense_first(parts)[2], dense_first(supps)[2],
                             dfirst, dmin)
        assert np.array_equal(ref_case("q21", name, N_BIG, big=True), exp), name
        assert np.count_nonzero(exp) > 100
    parts, supps, custs, dates = case_dims("fold-rand4-D1", "q43")
    dmin, _, dfirst = dense_first(dates)
    exp = orc.q43_kernel(ck, sk, pk, od, rv, sc, dense_first(custs)[2],
                         dense_first(supps)[2], dense_first(parts)[2], dfirst, dmin)
    assert np.array_equal(ref_case("q43", "fold-rand4-D1", N_BIG, big=True), exp)
    assert np.count_nonzero(exp) > 100


@pytest.mark.parametrize("dim_name", list(Q1_DIMS))
@pytest.mark.parametrize("dist", ["D1", "D5", "D7"])
def test_ref_q1_matches_oracle(dim_name, dist):
    dim = Q1_DIMS[dim_name]()
    mn, mx, dfirst = dense_first(dim)
    for n in Q1_NS:
        od, ep, dc = (np.ascontiguousarray(c[:n]) for c in q1_rows(dim_name, dist))
        got = ref_q1(od, ep, dc, dim)
        assert got == orc.q1_kernel(od, ep, dc, dfirst, mn, mx), (dim_name, dist, n)
        # the exact total (Python ints) must itself fit int64, or the int64
        # references would only agree modulo 2^64
        ok = _probe(od, dim) != 0
        exact = sum(int(a) * int(b) for a, b in zip(ep[ok], dc[ok]))
        assert -2**63 <= exact < 2**63 and exact == got[0], (dim_name, dist, n)
    if dist == "D7":
        od, ep, dc = q1_rows(dim_name, dist)
        ok = _probe(od, dim) != 0
        prod = ep[ok].astype(np.int64) * dc[ok].astype(np.int64)
        assert (prod == 2**62).sum() == 1                    # one MIN x MIN row
        assert (prod == MIN32 * MAX32).sum() > 100 and abs(got[0]) > 2**32


def test_q1_wide_dim_takes_fallback_kernel():
    keys, pay = q1_wide_dim()
    passing = keys[pay != 0]
    assert int(passing.max()) - int(passing.min()) + 1 > 262_144
    keys, pay = date_dim("q1")
    passing = keys[pay != 0]
    assert int(passing.max()) - int(passing.min()) + 1 <= 262_144


def test_dims_fold_as_intended():
    for kind in ("all", "rand4"):
        keys, pay = part_dim(P_SMALL, kind, "q21")
        m = maybe_masks((keys, pay), keys)
        for layout in m:                 # range < 2^18: the folds are exact
            assert np.array_equal(m[layout], pay != 0), (kind, layout)
    keys, pay = part_dim(P_FOLD, "rand4", "q21")
    m = maybe_masks((keys, pay), keys)
    for layout in m:                     # aliasing: false maybes exist, no false negatives
        assert ((pay != 0) <= m[layout]).all()
        assert (m[layout] & (pay == 0)).sum() > 1000, layout
    assert len(false_maybe_keys((keys, pay))) > 1000


def test_d4_is_a_false_maybe_storm():
    parts = part_dim(P_FOLD, "rand4", "q21")
    pk = case_rows("fold-rand4-D4")[2]
    for n in (max(shapes(S_Q21)), NMAX):
        col = pk[:n]
        passes = _probe(col, parts) != 0
        for layout, maybe in maybe_masks(parts, col).items():
            false_maybe = maybe & ~passes
            assert false_maybe.sum() >= 1000, (layout, n)
            assert false_maybe.sum() >= 0.95 * n, (layout, n)
        assert passes.sum() > 50         # the rest are true matches


def test_distribution_properties():
    # D2: one passing key; D3: distinct keys, all pass; D6: runs up to 200
    for name in ("fold-rand4-D2", "small-last-D2"):
        pk = case_rows(name)[2]
        assert len(np.unique(pk)) == 1 and _probe(pk, case_dims(name, "q21")[0]).all()
    pk = case_rows("fold-all-D3")[2]
    assert len(np.unique(pk)) == len(pk) and _probe(pk, part_dim(P_FOLD, "all", "q21")).all()
    pk = case_rows("fold-rand4-D6")[2]
    runs = np.diff(np.flatnonzero(np.concatenate([[True], pk[1:] != pk[:-1], [True]])))
    assert runs.max() > 150 and runs.min() == 1
    # D5: every special value lands in every key column
    for name in (c for c, v in CASES.items() if v[3] == "D5"):
        ck, sk, pk, *_ = case_rows(name)
        parts, supps, custs, _ = case_dims(name, "q21")
        for col, dim in ((pk, parts), (sk, supps), (ck, custs)):
            assert set(_specials(dim).tolist()) <= set(col[:shapes(S_Q21)[-1]].tolist())
    # D7: extremes only, one group's sum beyond +-2^32 already at the q21 size
    for name in ("fold-rand4-D7", "small-all-D7"):
        _, _, _, _, rv, sc = case_rows(name)
        assert set(rv.tolist()) == set(sc.tolist()) == set(EXTREMES.tolist())
        for wl in ("q21", "q43"):
            assert np.abs(ref_case(wl, name, max(shapes(S_Q21)))).max() > 2**32, (name, wl)
    # empty sets give empty results; the other cases are not vacuous
    for wl in ("q21", "q43"):
        for name in CASES:
            r = ref_case(wl, name, NMAX)
            if "empty" in name or "nosupp" in name:
                assert not r.any(), (wl, name)
        for name in ("small-rand4-D1", "fold-rand4-D4", "fold-rand4-D5", "fold-all-D5",
                     "fold-rand4-D6", "fold-all-D3", "small-first-D2", "fold-last-D2"):
            assert ref_case(wl, name, max(shapes(S_Q21))).any(), (wl, name)


# ---------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------
class _Dev:
    """Device copies of the dims (as join tables) and case columns, built once."""

    def __init__(self, eng):
        self.eng, self.bufs, self.tabs, self.cols = eng, [], {}, {}

    def buf(self, arr=None, nbytes=0):
        nb = arr.nbytes if arr is not None else nbytes
        b = self.eng.alloc(max(nb, 16))
        if arr is not None and arr.nbytes:
            b.h2d(arr)
        self.bufs.append(b)
        return b

    def table(self, dim):
        keys, pay = dim
        if id(pay) not in self.tabs:
            kb, pb = self.eng.alloc(keys.nbytes), self.eng.alloc(pay.nbytes)
            kb.h2d(keys)
            pb.h2d(pay)
            self.tabs[id(pay)] = (pay, self.eng.join_build_payload(kb, pb, len(keys)))
            kb.free()
            pb.free()
        return self.tabs[id(pay)][1]

    def tables(self, name, wl):
        return [self.table(d) for d in case_dims(name, wl)]

    def rows(self, key, cols):
        if key not in self.cols:
            self.cols[key] = [self.buf(c) for c in cols]
        return self.cols[key]

    def case(self, name):
        return self.rows(name, case_rows(name))

    def close(self):
        self.eng.sync()
        for b in self.bufs:
            b.free()
        for _, t in self.tabs.values():
            t.destroy()


@pytest.fixture(scope="module")
def dev(engine):
    d = _Dev(engine)
    yield d
    d.close()


def _clear_env(monkeypatch):
    for v in ("GPUE_Q21_PF", "GPUE_Q21_PF_NT", "GPUE_Q21_PF_TPB", "GPUE_GRID_PF",
              "GPUE_Q43_PF", "GPUE_GRID_Q43", "GPUE_GRID_WIDE"):
        monkeypatch.delenv(v, raising=False)


def _q21(dev, name, n):
    parts, supps, _, dates = dev.tables(name, "q21")
    _, sk, pk, od, rv, _ = dev.case(name)
    return dev.eng.q21_star_agg(parts, supps, dates, pk, sk, od, rv, n)


def _q43(dev, name, n, acc):
    parts, supps, custs, dates = dev.tables(name, "q43")
    dev.eng.q43_star_agg_async(custs, supps, parts, dates, *dev.case(name), n, acc)
    return acc.d2h(np.int64, NG_Q43)


def _check_all(run, wl, variant, ns):
    bad = [(variant, name, n) for name in CASES for n in ns
           if not np.array_equal(run(name, n), ref_case(wl, name, n))]
    assert not bad, f"{wl} differs from the reference at (variant, case, n): {bad[:12]}" \
                    f" ({len(bad)} in all)"


# GPUE_Q21_PF: 1 = LDS prefilter, 2 = global-group form (both x GPUE_Q21_PF_NT),
# 4 = single-fold wave queue, 6 = split-fold wave queue, 7 = deferred loads
Q21_VARIANTS = [("1", "0"), ("1", "1"), ("2", "0"), ("2", "1"), ("4", None), ("6", None),
                ("7", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("pf,nt", Q21_VARIANTS)
def test_q21_variants_small_geometry(dev, monkeypatch, pf, nt):
    _clear_env(monkeypatch)
    monkeypatch.setenv("GPUE_Q21_PF", pf)
    if nt is not None:
        monkeypatch.setenv("GPUE_Q21_PF_NT", nt)
    monkeypatch.setenv("GPUE_GRID_PF", "2")
    monkeypatch.setenv("GPUE_Q21_PF_TPB", "256")
    _check_all(lambda name, n: _q21(dev, name, n), "q21", f"PF={pf},NT={nt}",
               shapes(S_Q21))


@pytest.mark.gpu
def test_q21_default_kernel_tpb512(dev, monkeypatch):
    _clear_env(monkeypatch)
    monkeypatch.setenv("GPUE_GRID_PF", "2")
    monkeypatch.setenv("GPUE_Q21_PF_TPB", "512")
    _check_all(lambda name, n: _q21(dev, name, n), "q21", "default,TPB=512",
               shapes(2 * 512))


# GPUE_Q43_PF: 0 = exact bitset, 1 = LDS prefilter, 4 = wave queue, 6 = wide split fold
@pytest.mark.gpu
@pytest.mark.parametrize("pf", ["0", "1", "4", "6"])
def test_q43_variants_small_geometry(dev, monkeypatch, pf):
    _clear_env(monkeypatch)
    monkeypatch.setenv("GPUE_Q43_PF", pf)
    monkeypatch.setenv("GPUE_GRID_Q43", "1")
    acc = dev.buf(nbytes=NG_Q43 * 8)
    _check_all(lambda name, n: _q43(dev, name, n, acc), "q43", f"PF={pf}", shapes(S_Q43))


def _big(dev):
    return dev.rows("big", big_rows())


@pytest.mark.gpu
def test_q21_default_geometry(dev, monkeypatch):
    """No geometry variables: two full strides + one wave + a 3-row tail."""
    _clear_env(monkeypatch)
    _, sk, pk, od, rv, _ = _big(dev)
    for name in ("fold-rand4-D1", "fold-all-D1"):
        parts, supps, _, dates = dev.tables(name, "q21")
        got = dev.eng.q21_star_agg(parts, supps, dates, pk, sk, od, rv, N_BIG)
        assert np.array_equal(got, ref_case("q21", name, N_BIG, big=True)), name


@pytest.mark.gpu
def test_q43_default_geometry(dev, monkeypatch):
    _clear_env(monkeypatch)
    acc = dev.buf(nbytes=NG_Q43 * 8)
    for name in ("fold-rand4-D1", "fold-all-D1"):
        parts, supps, custs, dates = dev.tables(name, "q43")
        dev.eng.q43_star_agg_async(custs, supps, parts, dates, *_big(dev), N_BIG, acc)
        assert np.array_equal(acc.d2h(np.int64, NG_Q43),
                              ref_case("q43", name, N_BIG, big=True)), name


@pytest.mark.gpu
def test_q21_async_equals_sync(dev, monkeypatch):
    _clear_env(monkeypatch)
    acc = dev.buf(nbytes=NG_Q21 * 8)
    for name in ("fold-rand4-D1", "small-all-D1", "fold-rand4-D5", "fold-all-D5"):
        parts, supps, _, dates = dev.tables(name, "q21")
        _, sk, pk, od, rv, _ = dev.case(name)
        for n in (NMAX, 4 * 65 + 3):
            dev.eng.q21_star_agg_async(parts, supps, dates, pk, sk, od, rv, n, acc)
            got = acc.d2h(np.int64, NG_Q21)
            assert np.array_equal(got, _q21(dev, name, n)), (name, n)
            assert np.array_equal(got, ref_case("q21", name, n)), (name, n)


# ---- q1: LDS-bitset kernel (real date dim) and the payload-gather fallback ----
@pytest.mark.gpu
@pytest.mark.parametrize("dim_name", list(Q1_DIMS))
def test_q1_distributions(dev, dim_name):
    dim = Q1_DIMS[dim_name]()
    dates = dev.table(dim)
    for dist in ("D1", "D5", "D7"):
        host = q1_rows(dim_name, dist)
        od, ep, dc = dev.rows(("q1", dim_name, dist), host)
        for n in Q1_NS:
            exp = ref_q1(*(c[:n] for c in host), dim)
            assert dev.eng.q1_join_sum(dates, od, ep, dc, n) == exp, (dim_name, dist, n)


@pytest.mark.gpu
@pytest.mark.parametrize("dim_name", list(Q1_DIMS))
def test_q1_async_zeroes_and_accum_accumulates(dev, dim_name):
    dim = Q1_DIMS[dim_name]()
    dates = dev.table(dim)
    acc = dev.buf(nbytes=16)
    for dist in ("D1", "D7"):
        host = q1_rows(dim_name, dist)
        od, ep, dc = dev.rows(("q1", dim_name, dist), host)
        n = max(Q1_NS)
        exp = ref_q1(*host, dim)
        assert exp[1] > 0
        for _ in range(2):               # the second call must not double
            dev.eng.q1_join_sum_async(dates, od, ep, dc, n, acc)
            got = acc.d2h(np.int64, 2)
            assert (int(got[0]), int(got[1])) == exp, (dim_name, dist)
        # two uneven halves into an accumulator zeroed once == the whole
        cut = 4 * 1001 + 3
        acc.h2d(np.zeros(2, np.int64))
        halves = [dev.eng.wrap_ptr_offset(b, cut * 4, (n - cut) * 4) for b in (od, ep, dc)]
        dev.eng.q1_join_sum_accum(dates, od, ep, dc, cut, acc)
        dev.eng.q1_join_sum_accum(dates, *halves, n - cut, acc)
        got = acc.d2h(np.int64, 2)
        assert (int(got[0]), int(got[1])) == exp, (dim_name, dist)
        for b in halves:
            b.free()


# ---- accumulate-only forms over uneven, unaligned row blocks ----
@pytest.mark.gpu
def test_q43_accum_blocks_equal_one_call(dev, monkeypatch):
    _clear_env(monkeypatch)
    starts = [0, 997, 3001, 3002, 9999, NMAX]     # block starts not multiples of 4
    acc, one = dev.buf(nbytes=NG_Q43 * 8), dev.buf(nbytes=NG_Q43 * 8)
    for name in ("small-all-D1", "fold-rand4-D2", "fold-rand4-D5", "fold-rand4-D7"):
        parts, supps, custs, dates = dev.tables(name, "q43")
        cols = dev.case(name)
        acc.h2d(np.zeros(NG_Q43, np.int64))
        for lo, hi in zip(starts[:-1], starts[1:]):
            block = [dev.eng.wrap_ptr_offset(b, lo * 4, (hi - lo) * 4) for b in cols]
            dev.eng.q43_star_agg_accum_async(custs, supps, parts, dates, *block, hi - lo, acc)
            dev.eng.sync()
            for b in block:
                b.free()
        dev.eng.q43_star_agg_async(custs, supps, parts, dates, *cols, NMAX, one)
        got = acc.d2h(np.int64, NG_Q43)
        assert np.array_equal(got, one.d2h(np.int64, NG_Q43)), name
        assert np.array_equal(got, ref_case("q43", name, NMAX)), name


@pytest.mark.gpu
def test_q3_probe_accum_blocks_equal_one_call(engine):
    """agg_table_reset, lineitem rows in 4 uneven blocks, hash_agg_emit ==
    one q3_probe_agg_t call over the same rows (key-sorted)."""
    seed, n, n_orders, n_custs, cutoff = 42, 300_000, 100_000, 20_000, 19950315
    mkt = engine.alloc(n_custs * 16)
    engine.gen_cust_mkt16(seed, n_custs, mkt)
    cbits = engine.alloc((n_custs + 31) // 32 * 4)
    engine.bits_str16_eq(mkt, n_custs, orc.mkt_literal(1), cbits)
    oc, od = engine.alloc(n_orders * 4), engine.alloc(n_orders * 4)
    engine.gen_orders_q3(seed, n_orders, n_custs, oc, od)
    obits = engine.alloc((n_orders + 31) // 32 * 4)
    engine.q3_order_bits(oc, od, n_orders, cbits, cutoff, obits)
    lk, ext, disc = (engine.alloc(n * 8) for _ in range(3))
    ship = engine.alloc(n * 4)
    engine.gen_lineitem_q3(seed, 0, n, n_orders, lk, ext, disc, ship)
    at = engine.agg_table_create(1 << 18)
    ok_b, os_b = engine.alloc(n_orders * 8), engine.alloc(n_orders * 8)

    g = engine.q3_probe_agg_t(lk, ext, disc, ship, n, obits, cutoff, at, ok_b, os_b, n_orders)
    ek, es = ok_b.d2h(np.uint64, g), os_b.d2h(np.int64, g)
    order = np.argsort(ek)
    ek, es = ek[order], es[order]

    engine.agg_table_reset(at)
    starts = [0, 70_001, 70_002, 199_999, n]
    for lo, hi in zip(starts[:-1], starts[1:]):
        block = [engine.wrap_ptr_offset(b, lo * w, (hi - lo) * w)
                 for b, w in ((lk, 8), (ext, 8), (disc, 8), (ship, 4))]
        engine.q3_probe_accum(*block, hi - lo, obits, cutoff, at)
        engine.sync()
        for b in block:
            b.free()
    g2 = engine.hash_agg_emit(at, ok_b, os_b, n_orders)
    gk, gs = ok_b.d2h(np.uint64, g2), os_b.d2h(np.int64, g2)
    order = np.argsort(gk)
    assert g2 == g and g > 1000
    assert np.array_equal(gk[order], ek)
    assert np.array_equal(gs[order], es)
    wk, ws = orc.q3_pipeline(seed, 0, n, n_orders, n_custs)
    assert np.array_equal(ek, wk) and np.array_equal(es, ws)
    for b in (mkt, cbits, oc, od, obits, lk, ext, disc, ship, ok_b, os_b):
        b.free()
    engine.agg_table_destroy(at)


# ---- two-stream pipelined q21: chunks must cover every row ----
@pytest.mark.gpu
@pytest.mark.parametrize("n_chunks", [1, 3, 4, 8])
def test_q21_pipe_covers_every_row(dev, monkeypatch, n_chunks):
    """n / n_chunks a multiple of 4 with n % n_chunks != 0 used to drop the
    trailing rows (39 rows in 8 chunks: 7; 4099 in 4: 3; 3 in 8: all)."""
    _clear_env(monkeypatch)
    _, sk, pk, od, rv, _ = _big(dev)
    scratch = dev.buf(nbytes=2 * max(PIPE_NS))
    acc = dev.buf(nbytes=NG_Q21 * 8)
    for name in ("fold-all-D1", "fold-rand4-D1"):
        parts, supps, _, dates = dev.tables(name, "q21")
        for n in (0,) + PIPE_NS:
            dev.eng.sync()               # brand_scratch is reused across calls
            dev.eng.q21_star_agg_pipe(parts, supps, dates, pk, sk, od, rv, n, scratch, acc,
                                      n_chunks)
            got = acc.d2h(np.int64, NG_Q21)
            assert np.array_equal(got, ref_case("q21", name, n, big=True)), (name, n_chunks, n)
    dev.eng.sync()
