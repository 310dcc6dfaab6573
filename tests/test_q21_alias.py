"""Parity of the alias-resolved q21 kernel (GPUE_Q21_PF=10, every
GPUE_Q21_PF10_VAR variant) and of the part table's alias codes against the
plain numpy reference.

Every GPU comparison is bit-exact int64 equality against ref_q21 of
test_fused_star_edges (pinned to the oracle there); no GPU mode is compared
with another.

Mode 10 needs mode 9's part table (at most 64 distinct payloads), a pass set
spanning at most 3 * 2^19 keys and at most 65,535 set bits in the 2^19-bit
fold. With idx = key - (smallest passing key), a key's bit is idx & (2^19-1)
and its alias is idx >> 19. The table keeps, per set bit, the one alias that
passes (0..2) or 3 when several do; the kernel's first drain keeps a key iff
its bit's code is 3 or equals its alias, and rejects the rest of code 3's
keys exactly by their payload rank in the last drain.

1. CPU-only: a numpy model of that structure (set bits, per-128-bit prefix,
   packed codes, the resolved maybe mask); the dims are what they claim;
2. build and dispatch: explicit mode 10 is an error on tables that do not
   qualify, the default mode returns the reference on all of them;
3. the adversarial case x shape matrix at 2 blocks of 256 and 1024 threads;
4. exactness of the late rejection: stage fills over a background of keys
   that survive the first drain without passing;
5. stage fills over a background of keys the fold reports and the codes
   reject: Q1 overflows while Q2 sees the placed rows only;
6. burst boundaries with every row passing the part stage.

GPUE_Q21_PF10_VAR -> (Q1 entries per wave, quads per burst K).
"""

import functools

import numpy as np
import pytest

from starrocks_amd.engine import GpueError
from test_fused_star_edges import (CASES, DATEKEY, M19, P_FOLD, P_SMALL, _Dev, _gen_fk,
                                   case_rows, date_dim, fk_dim, maybe_masks, part_dim,
                                   ref_case, ref_q21, shapes)
from test_q21_cascade import RV_VALUES, _place
from test_q21_compact import (KM9, N_1024, N_BURST, N_FILL, Q_FILL, QUALIFY, RANK_NS, S_FILL,
                              _burst_ns, _env, _ref, compact_part_dim, rank_part_dim)

VARS = {"1": (128, 1), "2": (320, 4)}
KS = sorted({k for _, k in VARS.values()})
P_EDGE = 3 * 2**19             # the widest span that qualifies: aliases 0..2
P_OVER = P_EDGE + 1000         # one alias too many


@pytest.fixture(scope="module")
def dev(engine):
    d = _Dev(engine)
    yield d
    d.close()


def _env10(monkeypatch, mode, var, grid, tpb):
    _env(monkeypatch, mode, None, grid, tpb)
    monkeypatch.delenv("GPUE_Q21_PF10_VAR", raising=False)
    if var is not None:
        monkeypatch.setenv("GPUE_Q21_PF10_VAR", var)


# ---------------------------------------------------------------------------
# the numpy model of the table's alias structure
# ---------------------------------------------------------------------------
_MODELS = {}


def alias_model(parts):
    """Set bits of the 2^19 fold, the passing aliases behind each, and the
    table's layout of them: pref[b] = set bits before 128-bit block b, packed =
    2-bit codes at each set bit's rank, 16 per word."""
    keys, pay = parts
    m = _MODELS.get(id(pay))
    if m is not None and m["pay"] is pay:
        return m
    passing = keys[pay != 0].astype(np.int64)
    smin, smax = (int(passing.min()), int(passing.max())) if len(passing) else (1, 1)
    idx = passing - smin
    cnt = np.bincount(idx & M19, minlength=2**19)        # passing aliases per bit
    bit_code = np.full(2**19, -1, np.int64)
    bit_code[idx & M19] = idx >> 19
    bit_code[cnt > 1] = 3
    isset = cnt > 0
    rank = np.cumsum(isset) - isset                      # set bits below each bit
    nset, span = int(isset.sum()), smax - smin + 1
    qualifies = span <= 3 * 2**19 and nset <= 65535
    packed = np.zeros(4096, np.int64)
    if qualifies:
        pos = np.arange(nset)
        np.bitwise_or.at(packed, pos >> 4, bit_code[isset] << (2 * (pos & 15)))
    m = _MODELS[id(pay)] = dict(
        pay=pay, smin=smin, smax=smax, span=span, nset=nset, qualifies=qualifies,
        ambiguous=int((cnt > 1).sum()), amax=int((idx >> 19).max()) if len(idx) else 0,
        isset=isset, rank=rank, pref=rank[::128], packed=packed)
    return m


def resolved_maybes(parts, col):
    """Rows of col that survive the kernel's first drain: in range, bit set,
    and the bit's code is 3 or the key's own alias."""
    m = alias_model(parts)
    assert m["qualifies"]
    k = col.astype(np.int64)
    inr = (k >= m["smin"]) & (k <= m["smax"])
    idx = np.where(inr, k - m["smin"], 0)
    j, a = idx & M19, idx >> 19
    # the kernel's lookup: block prefix + set bits of the block below j
    blocks = m["isset"].reshape(4096, 128)
    inblock = np.cumsum(blocks, axis=1) - blocks
    pos = m["pref"][j >> 7] + inblock[j >> 7, j & 127]
    assert np.array_equal(pos, m["rank"][j])
    code = (m["packed"][(pos >> 4) & 4095] >> (2 * (pos & 15))) & 3
    return inr & m["isset"][j] & ((code == 3) | (code == a))


def _passes(parts, col):
    keys, pay = parts
    return np.isin(col, keys[pay != 0])


@functools.lru_cache(None)
def late_part_dim():
    """P_EDGE keys. For 20,000 seeded bits j (bit 0 among them), keys j + 1 and
    j + 1 + 2^19 pass and key j + 1 + 2^20 does not: each of those bits is
    ambiguous, so its third alias survives the first drain and only its
    payload rank rejects it. Key P_EDGE (bit 2^19 - 1, alias 2) passes too and
    puts the third aliases inside the pass set's range."""
    rng = np.random.default_rng(21)
    j = np.sort(np.concatenate([[0], 1 + rng.permutation(2**19 - 2)[:19_999]]))
    keys = np.arange(1, P_EDGE + 1, dtype=np.int32)
    mask = np.zeros(P_EDGE, bool)
    mask[j] = mask[j + 2**19] = mask[P_EDGE - 1] = True
    k = np.cumsum(mask) - 1
    return keys, np.where(mask, 441 + k % 40, 0).astype(np.uint32)


def late_false_maybes():
    keys, pay = late_part_dim()
    low = keys[:2**19 - 1][pay[:2**19 - 1] != 0].astype(np.int64)
    return (low + 2**20).astype(np.int32)


def wrong_alias_keys(parts):
    """Non-passing keys the 2^19 fold reports and the codes reject."""
    keys, pay = parts
    return keys[(pay == 0) & maybe_masks(parts, keys)["fold19"] & ~resolved_maybes(parts, keys)]


@functools.lru_cache(None)
def d1_cols(size, n):
    """(pk, sk, od, rv): pk uniform over a part dim of `size` keys."""
    rng = np.random.default_rng([size, n, 10])
    pk = rng.integers(1, size + 1, n)
    sk = _gen_fk(fk_dim("rand20", "q21", 1), n, rng)
    od, rv = rng.choice(DATEKEY, n), rng.integers(-10**7, 10**7, n)
    return tuple(np.ascontiguousarray(c, np.int32) for c in (pk, sk, od, rv))


# ---------------------------------------------------------------------------
# 1. CPU-only
# ---------------------------------------------------------------------------
def test_alias_model_of_the_dims():
    m = alias_model(compact_part_dim(P_FOLD, "rand4"))
    assert (m["span"], m["nset"], m["ambiguous"], m["amax"]) == (1_053_473, 41_435, 834, 2)
    assert m["qualifies"]
    m = alias_model(compact_part_dim(P_EDGE, "rand4"))
    assert (m["span"], m["nset"], m["amax"]) == (1_572_840, 60_518, 2) and m["qualifies"]
    m = alias_model(compact_part_dim(P_OVER, "rand4"))
    assert (m["span"], m["nset"]) == (1_573_776, 60_276)
    assert m["span"] > 3 * 2**19 and m["nset"] <= 65535 and not m["qualifies"]
    m = alias_model(compact_part_dim(P_FOLD, "all"))
    assert m["nset"] == 2**19 and m["span"] <= 3 * 2**19 and not m["qualifies"]
    m = alias_model(compact_part_dim(P_SMALL, "rand4"))
    assert m["qualifies"] and m["ambiguous"] == 0 and m["amax"] == 0
    for kind in ("empty", "one-lo", "d64"):
        assert alias_model(rank_part_dim(kind))["qualifies"]
    assert alias_model(rank_part_dim("empty"))["nset"] == 0
    for m in _MODELS.values():                           # the u16 prefix holds
        assert not m["qualifies"] or m["pref"].max() <= 65535


def test_resolved_maybes_are_passers_plus_ambiguous_bits():
    for parts in (compact_part_dim(P_FOLD, "rand4"), compact_part_dim(P_EDGE, "rand4"),
                  compact_part_dim(P_SMALL, "rand4"), late_part_dim()):
        keys, pay = parts
        m = alias_model(parts)
        got = resolved_maybes(parts, keys)
        k = keys.astype(np.int64)
        inr = (k >= m["smin"]) & (k <= m["smax"])
        j = np.where(inr, k - m["smin"], 0) & M19
        passing = keys[pay != 0].astype(np.int64)
        amb = np.bincount((passing - m["smin"]) & M19, minlength=2**19) > 1
        assert np.array_equal(got, (pay != 0) | (inr & (pay == 0) & amb[j]))
        assert ((pay != 0) <= maybe_masks(parts, keys)["fold19"]).all()
    # the benchmark-like dim: the fold alone lets several percent of the
    # non-passing keys through, the codes a small fraction of that
    parts = compact_part_dim(P_FOLD, "rand4")
    keys, pay = parts
    fold = (maybe_masks(parts, keys)["fold19"] & (pay == 0)).sum()
    res = (resolved_maybes(parts, keys) & (pay == 0)).sum()
    assert fold > 20 * res > 0


def test_late_dim_is_what_it_claims():
    parts = late_part_dim()
    keys, pay = parts
    m = alias_model(parts)
    assert m["qualifies"] and (m["smin"], m["span"]) == (1, P_EDGE)
    assert (m["nset"], m["ambiguous"]) == (20_001, 20_000)
    assert len(np.unique(pay[pay != 0])) == 40
    fm = late_false_maybes()
    assert len(fm) == 20_000 and (pay[fm - 1] == 0).all()
    assert resolved_maybes(parts, fm).all()              # all survive the first drain


def test_wrong_alias_keys_are_what_they_claim():
    parts = compact_part_dim(P_FOLD, "rand4")
    wa = wrong_alias_keys(parts)
    assert len(wa) > 10_000 and (parts[1][wa - 1] == 0).all()
    assert maybe_masks(parts, wa)["fold19"].all() and not resolved_maybes(parts, wa).any()


def test_fill_cases_are_what_they_claim():
    supps = fk_dim("rand20", "q21", 1)
    for bg in ("late", "wrong"):
        parts = _fill_parts(bg)
        for k, m, how in ((0, 0, "first"), (65, 64, "spread"), (449, 127, "last"),
                          (N_FILL, N_FILL, "first"), (N_FILL, 0, "first")):
            (pk, sk, od, rv), exp = _fill_case(bg, k, m, how)
            brand, supp = _passes(parts, pk), _passes(supps, sk)
            assert brand.sum() == k and (brand & supp).sum() == m
            assert maybe_masks(parts, pk)["fold19"].all()
            res = resolved_maybes(parts, pk)
            assert (res & ~brand).sum() == (len(pk) - k if bg == "late" else 0)
            assert exp.any() == (m > 0)
            if bg == "late" and k < N_FILL:              # false maybes on both supplier sides
                assert (~brand & supp).any() and (~brand & ~supp).any()
    # every row a maybe of the fold for more than two bursts of the largest K
    assert N_FILL // 4 > 2 * max(KS) * S_FILL and Q_FILL > 2 * max(KS) * S_FILL


# ---------------------------------------------------------------------------
# 2. build and dispatch
# ---------------------------------------------------------------------------
NOT_QUALIFYING = {"over": lambda: compact_part_dim(P_OVER, "rand4"),
                  "all": lambda: compact_part_dim(P_FOLD, "all"),
                  "d65": lambda: rank_part_dim("d65")}
DISPATCH_DIMS = dict(NOT_QUALIFYING, **{k: functools.partial(rank_part_dim, k)
                                        for k in ("empty", "one-lo", "d64")})


def _dispatch_run(dev, kind, n):
    parts, supps = DISPATCH_DIMS[kind](), fk_dim("rand20", "q21", 1)
    size = len(parts[0])
    cols = d1_cols(size, RANK_NS[-1])
    dpk, dsk, dod, drv = dev.rows(("d1", size), cols)
    got = dev.eng.q21_star_agg(dev.table(parts), dev.table(supps), dev.table(date_dim("q21")),
                               dpk, dsk, dod, drv, n)
    return got, _ref(parts, supps, ("d1", size), cols, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(NOT_QUALIFYING))
def test_q21_alias_refuses_tables_that_do_not_qualify(dev, monkeypatch, kind):
    for var in VARS:
        _env10(monkeypatch, "10", var, 2, 256)
        with pytest.raises(GpueError):
            _dispatch_run(dev, kind, RANK_NS[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(DISPATCH_DIMS))
def test_q21_default_mode_on_alias_dims(dev, monkeypatch, kind):
    _env10(monkeypatch, None, None, 2, 256)
    for n in RANK_NS:
        got, exp = _dispatch_run(dev, kind, n)
        assert np.array_equal(got, exp), (kind, n)
    assert exp.any() == (kind != "empty")


@pytest.mark.gpu
@pytest.mark.parametrize("var", list(VARS))
@pytest.mark.parametrize("kind", ["empty", "one-lo", "d64"])
def test_q21_alias_on_ranked_dims(dev, monkeypatch, kind, var):
    _env10(monkeypatch, "10", var, 2, 256)
    for n in RANK_NS:
        got, exp = _dispatch_run(dev, kind, n)
        assert np.array_equal(got, exp), (kind, var, n)


# ---------------------------------------------------------------------------
# 3. the adversarial matrix: every case whose compact (or own) part dim
#    qualifies, and D1 rows over the dim at the edge of alias 2
# ---------------------------------------------------------------------------
def _matrix_inputs(dev, name, tpb):
    if tpb == 256:
        return case_rows(name), dev.case(name)
    return case_rows(name, N_1024), dev.rows(("n1024", name), case_rows(name, N_1024))


@pytest.mark.gpu
@pytest.mark.parametrize("var", list(VARS))
@pytest.mark.parametrize("tpb", [256, 1024])
def test_q21_alias_adversarial_matrix(dev, monkeypatch, tpb, var):
    _env10(monkeypatch, "10", var, 2, tpb)
    dates = dev.table(date_dim("q21"))
    bad, ran = [], 0
    for name, (size, kind, skind, _) in CASES.items():
        (_, sk, pk, od, rv, _), (_, dsk, dpk, dod, drv, _) = _matrix_inputs(dev, name, tpb)
        supps = fk_dim(skind, "q21", 1)
        dims = [("compact", compact_part_dim(size, kind))]
        if name in QUALIFY:
            dims.append(("own", part_dim(size, kind, "q21")))
        for tag, parts in dims:
            if not alias_model(parts)["qualifies"]:
                continue
            ran += 1
            for n in shapes(2 * tpb):
                exp = (ref_case("q21", name, n) if tag == "own" and tpb == 256 else
                       _ref(parts, supps, (name, tpb), (pk, sk, od, rv), n))
                got = dev.eng.q21_star_agg(dev.table(parts), dev.table(supps), dates,
                                           dpk, dsk, dod, drv, n)
                if not np.array_equal(got, exp):
                    bad.append((name, tag, n))
    parts, supps = compact_part_dim(P_EDGE, "rand4"), fk_dim("rand20", "q21", 1)
    cols = d1_cols(P_EDGE, N_1024)
    dpk, dsk, dod, drv = dev.rows(("d1", P_EDGE, N_1024), cols)
    for n in shapes(2 * tpb):
        got = dev.eng.q21_star_agg(dev.table(parts), dev.table(supps), dates,
                                   dpk, dsk, dod, drv, n)
        if not np.array_equal(got, _ref(parts, supps, ("d1", P_EDGE), cols, n)):
            bad.append(("edge-rand4-D1", "compact", n))
    assert ran >= 20
    assert not bad, f"PF=10 VAR={var} TPB={tpb} differs at (case, dim, n): {bad[:12]} ({len(bad)})"


# ---------------------------------------------------------------------------
# 4. / 5. stage-fill boundaries on one 64-thread block (test_q21_compact's
#    shape: two K=4 bursts, a full and a 17-lane remainder trip, a 3-row tail)
#    late:  the background is late_part_dim's third aliases. They pass the
#           fold and the codes, go on to the supplier test with passing and
#           failing suppliers, and are rejected by their rank 0 alone: one
#           that reaches the atomic changes a sum;
#    wrong: the background is keys the fold reports and the codes reject. Q1
#           takes 256 entries a quad for more than two bursts, so the
#           per-quad guard fires, while Q2 receives the k placed rows only.
# ---------------------------------------------------------------------------
def _fill_parts(bg):
    return late_part_dim() if bg == "late" else compact_part_dim(P_FOLD, "rand4")


@functools.lru_cache(None)
def _fill_bg(bg):
    parts = _fill_parts(bg)
    return late_false_maybes() if bg == "late" else wrong_alias_keys(parts)


@functools.lru_cache(None)
def _fill_case(bg, k, m, how):
    """(pk, sk, od, rv) with exactly k brand-passing rows, m of them passing the
    supplier test, placed in the quad region; background rows carry any
    supplier."""
    parts, supps, dates = _fill_parts(bg), fk_dim("rand20", "q21", 1), date_dim("q21")
    rng = np.random.default_rng([k, m, len(how), bg == "late", 10])
    (pkeys, ppay), (skeys, spay) = parts, supps
    p_pass = pkeys[ppay != 0]
    s_pass, s_fail = skeys[spay != 0], skeys[spay == 0]
    n = N_FILL
    region = n if k == n else 4 * Q_FILL
    rows_k = _place(k, region, how)
    assert len(rows_k) == k
    rows_m = rows_k[_place(m, k, how)]
    assert len(rows_m) == m
    pk = rng.choice(_fill_bg(bg), n)
    pk[rows_k] = rng.choice(p_pass, k)
    sk = rng.choice(skeys, n)
    sk[rows_k] = rng.choice(s_fail, k)
    sk[rows_m] = rng.choice(s_pass, m)
    od = rng.choice(DATEKEY, n)
    rv = rng.choice(RV_VALUES, n)
    cols = tuple(np.ascontiguousarray(c, np.int32) for c in (pk, sk, od, rv))
    return cols, ref_q21(*cols, parts, supps, dates)


FILL_CASES = [(k, m, how) for how in ("first", "last", "spread")
              for k in KM9 for m in KM9 if m <= k]


@pytest.mark.gpu
@pytest.mark.parametrize("var", list(VARS))
@pytest.mark.parametrize("bg", ["late", "wrong"])
def test_q21_alias_stage_fill_boundaries(dev, monkeypatch, bg, var):
    _env10(monkeypatch, "10", var, 1, 64)
    pk, sk, od, rv = (dev.buf(nbytes=4 * N_FILL) for _ in range(4))
    parts, supps, dates = (dev.table(d) for d in (_fill_parts(bg), fk_dim("rand20", "q21", 1),
                                                  date_dim("q21")))
    bad = []
    for case in FILL_CASES:
        cols, exp = _fill_case(bg, *case)
        for b, c in zip((pk, sk, od, rv), cols):
            b.h2d(c)
        got = dev.eng.q21_star_agg(parts, supps, dates, pk, sk, od, rv, N_FILL)
        if not np.array_equal(got, exp):
            bad.append(case)
    assert not bad, f"PF=10 VAR={var} {bg} differs at (k, m, placement): {bad[:12]} ({len(bad)})"


# ---------------------------------------------------------------------------
# 6. burst boundaries: every row's part key passes, so a dropped or
#    twice-consumed quad of a burst changes the sums
# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def _burst_cols():
    keys, pay = compact_part_dim(P_FOLD, "rand4")
    pk, sk, od, rv = d1_cols(P_FOLD, N_BURST)
    rng = np.random.default_rng(6)
    return np.ascontiguousarray(rng.choice(keys[pay != 0], N_BURST), np.int32), sk, od, rv


def test_burst_rows_all_pass_the_part_stage():
    parts = compact_part_dim(P_FOLD, "rand4")
    pk = _burst_cols()[0]
    assert _passes(parts, pk).all() and resolved_maybes(parts, pk).all()
    assert len(np.unique(pk)) > N_BURST // 2


@pytest.mark.gpu
@pytest.mark.parametrize("var", list(VARS))
@pytest.mark.parametrize("grid,tpb", [(1, 64), (2, 256)])
def test_q21_alias_burst_boundaries(dev, monkeypatch, grid, tpb, var):
    _env10(monkeypatch, "10", var, grid, tpb)
    parts, supps = compact_part_dim(P_FOLD, "rand4"), fk_dim("rand20", "q21", 1)
    dates = dev.table(date_dim("q21"))
    cols = _burst_cols()
    dpk, dsk, dod, drv = dev.rows("alias-burst", cols)
    bad = []
    for n in _burst_ns(VARS[var][1], grid * tpb):
        got = dev.eng.q21_star_agg(dev.table(parts), dev.table(supps), dates,
                                   dpk, dsk, dod, drv, n)
        exp = _ref(parts, supps, "alias-burst", cols, n)
        if not np.array_equal(got, exp):
            bad.append(n)
    assert exp.any()
    assert not bad, f"PF=10 VAR={var} {grid}x{tpb} differs at n: {bad[:12]}"
