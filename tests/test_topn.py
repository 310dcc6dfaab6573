"""General TopN (gpue_topn) on the GPU: multi-key ORDER BY ... LIMIT/OFFSET
for any k, exact against the numpy reference of tests/test_topn_cpu.py
(dense ranks + lexsort with the row index last). Every comparison is
np.array_equal — there are no tolerances.

Implementation edges the shapes aim at: 256-thread blocks, the 2048-row
select tile, the 1024-block grid cap (blocks own whole tiles, so large inputs
leave trailing blocks empty), 4096-row LDS sort tile (also the "skip
selection" and "stop selecting" threshold), K >= n (full ORDER BY, no
selection) and the multi-launch sort beyond one tile."""

import numpy as np
import pytest

from starrocks_amd.engine import GpueError
from oracle import pyoracle as orc
from test_topn_cpu import (TYPE_CODE, operator_case, run_operator, topn_order,
                           topn_reference)

pytestmark = pytest.mark.gpu

SEED = 42
SORT_TILE = 4096
I64 = np.iinfo(np.int64)
I32 = np.iinfo(np.int32)


class Uploaded:
    """Key columns resident on the device + their full reference order,
    computed once and sliced per (limit, offset)."""

    def __init__(self, engine, keys, n):
        self.e, self.n, self.keys = engine, n, keys
        self.bufs, self.desc = [], []
        for vals, nulls, desc, nulls_first in keys:
            vb = engine.alloc(max(n, 1) * vals.itemsize)
            if n:
                vb.h2d(vals[:n])
            nb = None
            if nulls is not None:
                nb = engine.alloc(max(n, 1))
                if n:
                    nb.h2d(np.asarray(nulls[:n], np.uint8))
            self.bufs += [b for b in (vb, nb) if b is not None]
            self.desc.append((vb, nb, TYPE_CODE[vals.dtype], desc, nulls_first))
        self.order = topn_order(keys, n)

    def check(self, limit, offset=0):
        got = self.e.topn_indices(self.desc, self.n, limit, offset)
        want = self.order[offset:offset + limit]
        assert got.dtype == np.uint32
        assert len(got) == len(want) == min(limit, max(self.n - offset, 0))
        assert np.array_equal(got.astype(np.int64), want), (self.n, limit, offset)
        return got

    def free(self):
        for b in self.bufs:
            b.free()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049,
                               SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 1_000_003,
                               1025 * 2048 + 5])  # 1025 tiles on 1024 blocks: empty trailing blocks
def test_row_counts_around_tile_edges(engine, n):
    rng = np.random.default_rng(100 + n % 97)
    vals = rng.integers(-(n // 3) - 1, n // 3 + 1, max(n, 1)).astype(np.int64)
    up = Uploaded(engine, [(vals, None, False, False)], n)
    for limit, offset in [(10, 0), (7, 3), (n, 0), (n + 5, 0), (5, max(n - 2, 0))]:
        up.check(limit, offset)
    up.free()


@pytest.fixture(scope="module")
def ties_300k(engine):
    n = 300_007
    rng = np.random.default_rng(7)
    vals = rng.integers(0, 50_000, n).astype(np.int64)
    up = Uploaded(engine, [(vals, None, True, False)], n)
    yield up
    up.free()


@pytest.mark.parametrize("k", [1, 16, 17, 64, 100, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1,
                               10_000, 300_006, 300_007, 300_012])
def test_k_around_thresholds(ties_300k, k):
    ties_300k.check(k, 0)


@pytest.mark.parametrize("limit,offset", [(100, 50), (1, SORT_TILE), (SORT_TILE, 1),
                                          (100, 300_007 - 20), (10, 300_007),
                                          (10, 300_007 + 7), (0, 0), (0, 12)])
def test_offset_and_limit_edges(ties_300k, limit, offset):
    ties_300k.check(limit, offset)


@pytest.mark.parametrize("k,offset", [(10, 0), (10, 3), (5000, 0), (5000, 17)])
def test_all_rows_identical(engine, k, offset):
    """Selection never narrows: the answer is the first K row indices."""
    n = 100_000
    a = np.full(n, -12345, np.int64)
    b = np.full(n, 7, np.int32)
    up = Uploaded(engine, [(a, None, True, False), (b, None, False, False)], n)
    got = up.check(k - offset, offset)
    assert np.array_equal(got, np.arange(offset, k, dtype=np.uint32))
    up.free()


def test_ties_straddle_the_cut(engine):
    """3-value domain; K lands inside a tie run, ascending and descending."""
    n = 200_000
    rng = np.random.default_rng(11)
    vals = rng.integers(0, 3, n).astype(np.int32)
    for desc in (False, True):
        up = Uploaded(engine, [(vals, None, desc, False)], n)
        first_run = int((vals == (2 if desc else 0)).sum())
        for k in (first_run - 1, first_run, first_run + 1, first_run + 1234,
                  first_run + int((vals == 1).sum()) + 5000):
            up.check(k, 0)
        up.check(300, first_run - 100)
        up.free()


def _extreme_column(dtype, n, rng):
    if dtype == np.uint64:
        special = np.array([0, 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1], np.uint64)
        body = rng.integers(0, 2**64, n, dtype=np.uint64)
    else:
        info = np.iinfo(dtype)
        special = np.array([info.min, info.max, -1, 0, 1, info.min + 1], dtype)
        body = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    pos = rng.choice(n, 60, replace=False)
    body[pos] = np.tile(special, 10)   # each extreme 10x: ties among extremes
    return body


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.uint64])
@pytest.mark.parametrize("desc", [False, True])
def test_digit_extremes(engine, dtype, desc):
    n = 50_000
    rng = np.random.default_rng(13)
    col = _extreme_column(dtype, n, rng)
    up = Uploaded(engine, [(col, None, desc, False)], n)
    for k in (1, 25, 100, 5000):
        up.check(k, 0)
    up.free()
    # one column whose keys differ only in the lowest byte, one only in the highest
    bits = 8 * np.dtype(dtype).itemsize
    low = np.full(n, 1234567 << 8, dtype) + rng.integers(0, 256, n).astype(dtype)
    high = (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(bits - 8)) + np.uint64(0x1234)
    high = high.astype(np.uint32).view(np.int32) if dtype == np.int32 else high.view(dtype)
    for col2 in (low, high):
        up = Uploaded(engine, [(col2, None, desc, False)], n)
        for k in (1, 100, 5000):
            up.check(k, 0)
        up.free()


def test_multi_key_first_constant_second_decides(engine):
    n = 120_000
    rng = np.random.default_rng(17)
    a = np.full(n, I64.min, np.int64)
    b = rng.integers(0, 2**64, n, dtype=np.uint64)
    up = Uploaded(engine, [(a, None, False, False), (b, None, True, False)], n)
    for k in (1, 100, 5000):
        up.check(k, 0)
    up.free()


def test_multi_key_three_mixed(engine):
    """d_year ASC, revenue DESC, id ASC — mixed types and directions with
    low-cardinality leading keys."""
    n = 400_000
    rng = np.random.default_rng(19)
    year = rng.integers(1992, 1999, n).astype(np.int32)
    rev = rng.integers(-500, 500, n).astype(np.int64) * 1_000_003
    uid = rng.integers(2**63 - 40, 2**63 + 40, n, dtype=np.uint64)
    up = Uploaded(engine, [(year, None, False, False), (rev, None, True, False),
                           (uid, None, False, False)], n)
    for limit, offset in [(100, 0), (100, 57_000), (5000, 0), (20_000, 10)]:
        up.check(limit, offset)
    up.free()


def test_multi_key_eight(engine):
    """8 low-cardinality keys: ties survive all of them (4^8 < n)."""
    n = 150_000
    rng = np.random.default_rng(23)
    dts = [np.int32, np.int64, np.uint64, np.int32, np.int64, np.uint64, np.int32, np.int64]
    keys = [(rng.integers(0, 4, n).astype(dt), None, bool(i % 2), False)
            for i, dt in enumerate(dts)]
    up = Uploaded(engine, keys, n)
    for limit, offset in [(10, 0), (1000, 0), (5000, 100)]:
        up.check(limit, offset)
    up.free()


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
def test_nulls_all_four_placements(engine, desc, nulls_first):
    n = 100_000
    rng = np.random.default_rng(29)
    vals = rng.integers(-1000, 1000, n).astype(np.int64)
    nulls = (rng.random(n) < 0.2).astype(np.uint8)
    vals[nulls != 0] = rng.integers(I64.min, I64.max, int(nulls.sum()))  # garbage
    b = rng.integers(0, 50, n).astype(np.int32)
    up = Uploaded(engine, [(vals, nulls, desc, nulls_first), (b, None, False, False)], n)
    nn = int(nulls.sum())
    for limit, offset in [(10, 0), (100, nn - 50), (5000, 0), (100, n - nn - 50),
                          (nn + 5000, 0)]:
        up.check(limit, offset)
    up.free()


def test_nulls_all_null_column_and_leading_nulls(engine):
    n = 60_000
    rng = np.random.default_rng(31)
    garbage = rng.integers(I32.min, I32.max, n).astype(np.int32)
    allnull = np.ones(n, np.uint8)
    b = rng.integers(0, 2**64, n, dtype=np.uint64)
    # an all-NULL leading key ties every row: the second key decides
    up = Uploaded(engine, [(garbage, allnull, True, True), (b, None, False, False)], n)
    for k in (1, 100, 5000):
        up.check(k, 0)
    up.free()
    # NULLs on the leading key, NULLS_FIRST, K inside the NULL run: the
    # second key decides among them
    lead = rng.integers(0, 10, n).astype(np.int64)
    nulls = (rng.random(n) < 0.5).astype(np.uint8)
    up = Uploaded(engine, [(lead, nulls, False, True), (b, None, True, False)], n)
    for k in (10, 5000, int(nulls.sum()) - 1, int(nulls.sum()) + 1):
        up.check(k, 0)
    up.free()


def test_null_rows_ignore_stored_values(engine):
    n = 80_000
    rng = np.random.default_rng(37)
    nulls = (rng.random(n) < 0.3).astype(np.uint8)
    b = rng.integers(0, 30, n).astype(np.int32)
    for dt in (np.int32, np.uint64):
        clean = rng.integers(0, 100, n).astype(dt)
        clean[nulls != 0] = 0
        dirty = clean.copy()
        info = np.iinfo(dt)
        dirty[nulls != 0] = rng.integers(info.min, info.max, int(nulls.sum()), dtype=dt,
                                         endpoint=True)
        res = []
        for col in (clean, dirty):
            up = Uploaded(engine, [(col, nulls, True, False), (b, None, False, True)], n)
            res.append([up.check(k, off) for k, off in [(100, 0), (6000, 20)]])
            up.free()
        for x, y in zip(*res):
            assert np.array_equal(x, y)


def test_parity_with_topk_i64(engine):
    """value DESC then key DESC + gather == the old k<=16 entry."""
    rng = np.random.default_rng(47)
    n = 300_000
    keys = rng.integers(1, 2**40, n).astype(np.uint64)
    vals = rng.integers(0, 50_000, n).astype(np.int64)  # many ties
    kb = engine.alloc(keys.nbytes)
    kb.h2d(keys)
    vb = engine.alloc(vals.nbytes)
    vb.h2d(vals)
    for k in (1, 10, 16):
        idx, cnt = engine.topn([(vb, None, 1, True, False), (kb, None, 2, True, False)], n, k)
        assert cnt == k
        gk, gv = engine.alloc(k * 8), engine.alloc(k * 8)
        engine.gather_u64(kb, idx, k, gk)
        engine.gather_u64(vb, idx, k, gv)
        ok, ov = engine.topk_i64(kb, vb, n, k)
        assert np.array_equal(gv.d2h(np.int64, k), ov)
        assert np.array_equal(gk.d2h(np.uint64, k), ok)
        for b in (idx, gk, gv):
            b.free()
    kb.free()
    vb.free()


def test_q3_composition(engine):
    """Q3 join + high-cardinality agg, then ORDER BY revenue DESC, orderkey
    DESC LIMIT k on the device-resident groups, for k past the old limit."""
    n, n_orders, n_custs = 2_000_000, 150_000, 30_000
    mkt = engine.alloc(n_custs * 16)
    engine.gen_cust_mkt16(SEED, n_custs, mkt)
    cbits = engine.alloc((n_custs + 31) // 32 * 4)
    engine.bits_str16_eq(mkt, n_custs, orc.mkt_literal(1), cbits)
    oc, od = engine.alloc(n_orders * 4), engine.alloc(n_orders * 4)
    engine.gen_orders_q3(SEED, n_orders, n_custs, oc, od)
    obits = engine.alloc((n_orders + 31) // 32 * 4)
    engine.q3_order_bits(oc, od, n_orders, cbits, 19950315, obits)
    lk, ext, disc = (engine.alloc(n * 8) for _ in range(3))
    ship = engine.alloc(n * 4)
    engine.gen_lineitem_q3(SEED, 0, n, n_orders, lk, ext, disc, ship)
    ok_b, os_b = engine.alloc(n * 8), engine.alloc(n * 8)
    g = engine.q3_probe_agg(lk, ext, disc, ship, n, obits, 19950315, ok_b, os_b, n)
    ek, es = orc.q3_pipeline(SEED, 0, n, n_orders, n_custs)
    assert g == len(ek)
    assert g >= 10_000
    full = np.lexsort((ek, es))[::-1]
    for k in (10, 100, 10_000):
        idx, cnt = engine.topn([(os_b, None, 1, True, False), (ok_b, None, 2, True, False)],
                               g, k)
        assert cnt == k
        tk, tv = engine.alloc(k * 8), engine.alloc(k * 8)
        engine.gather_u64(ok_b, idx, k, tk)
        engine.gather_u64(os_b, idx, k, tv)
        assert np.array_equal(tv.d2h(np.int64, k), np.asarray(es)[full[:k]].astype(np.int64))
        assert np.array_equal(tk.d2h(np.uint64, k), np.asarray(ek)[full[:k]].astype(np.uint64))
        for b in (idx, tk, tv):
            b.free()
    for b in (mkt, cbits, oc, od, obits, lk, ext, disc, ship, ok_b, os_b):
        b.free()


def test_argument_errors(engine):
    """Host-side checks: each raises before anything is launched."""
    col = engine.alloc(1000 * 8)
    key = (col, None, 1, False, False)
    with pytest.raises(GpueError):
        engine.topn([], 1000, 10)
    with pytest.raises(GpueError):
        engine.topn([key] * 9, 1000, 10)
    with pytest.raises(GpueError):
        engine.topn([(col, None, 3, False, False)], 1000, 10)
    with pytest.raises(GpueError):
        engine.topn([(col, None, -1, False, False)], 1000, 10)
    small = engine.alloc(9 * 4)
    with pytest.raises(GpueError):
        engine.topn_into([key], 1000, 10, 0, small)
    with pytest.raises(GpueError):   # key buffer shorter than n_rows elements
        engine.topn([key], 1001, 10)
    nm = engine.alloc(999)
    with pytest.raises(GpueError):   # null mask shorter than n_rows
        engine.topn([(col, nm, 1, False, False)], 1000, 10)
    with pytest.raises(GpueError):
        engine.topn_into([key], 2**32, 10, 0, small)
    # a 9-slot buffer is enough when only 9 rows remain after the offset
    col.h2d(np.arange(1000, dtype=np.int64))
    assert engine.topn_into([key], 1000, 10, 991, small) == 9
    assert list(small.d2h(np.uint32, 9)) == list(range(991, 1000))
    for b in (col, small, nm):
        b.free()


@pytest.fixture(scope="module")
def op_case():
    return operator_case()


@pytest.mark.parametrize("bound_factor", [2, 4])
def test_operator_chunked_equals_single_call(engine, op_case, bound_factor):
    a, b, rid, ref = op_case
    sink, out = run_operator(engine, a, b, rid, bound_factor)
    assert np.array_equal(out[2].astype(np.int64), ref)
    assert np.array_equal(out[0], a[ref]) and np.array_equal(out[1], b[ref])
    assert sink.max_candidate_rows <= sink.capacity
    up = Uploaded(engine, [(a, None, False, False), (b, None, True, False)], len(a))
    single = up.check(len(ref), 100)
    up.free()
    assert np.array_equal(out[2], single)
