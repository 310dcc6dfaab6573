"""Top 3 rows per group through the GENERIC operator chain — the query shape
that needs a window function:

    SELECT * FROM (SELECT region, year, revenue,
                          ROW_NUMBER() OVER (PARTITION BY region, year
                                             ORDER BY revenue DESC) AS rn
                   FROM (SELECT region, year, price * (100 - disc) AS revenue FROM t))
    WHERE rn <= 3

as Engine.project -> Engine.window -> Engine.project to a mask -> mask_compact,
with a nullable `year`. The surviving rows must equal a numpy computation as a
sorted set of rows; a running SUM(revenue) per group from the same window call
is checked against np.cumsum per group."""

import numpy as np
import pytest

from starrocks_amd.expr import XO_I64, XO_MASK
from starrocks_amd.window import PT_I32, PT_I64, ROW_NUMBER, ROWS, SUM, UNBOUNDED, WinFunc

pytestmark = pytest.mark.gpu

N, SEED, TOP = 50_000, 20, 3


def up(eng, arr):
    b = eng.alloc(arr.nbytes)
    b.h2d(arr)
    return b


def test_top3_revenue_rows_per_region_and_year(engine):
    eng = engine
    rng = np.random.default_rng(SEED)
    region = rng.integers(0, 25, N).astype(np.int32)
    year_nulls = (rng.random(N) < 0.05).astype(np.uint8)
    year = np.where(year_nulls != 0, rng.integers(-9, 9, N), rng.integers(1992, 1999, N)).astype(
        np.int32)                                           # garbage under the NULLs
    price = rng.integers(100, 5000, N).astype(np.int32)     # few values: ties in revenue
    disc = rng.integers(0, 11, N).astype(np.int32)
    d_region, d_year, d_ynul, d_price, d_disc = (up(eng, a) for a in
                                                 (region, year, year_nulls, price, disc))
    bufs = [d_region, d_year, d_ynul, d_price, d_disc]
    try:
        (d_rev, rev_nulls), = eng.project(
            [("*", ("col", 0), ("-", ("const", 100), ("col", 1)))],
            [(d_price, None, PT_I32), (d_disc, None, PT_I32)], [XO_I64], N)
        bufs.append(d_rev)
        assert rev_nulls is None
        (d_rn, rn_nulls), (d_run, run_nulls) = eng.window(
            [(d_region, None, PT_I32), (d_year, d_ynul, PT_I32)],
            [(d_rev, None, PT_I64, True, False)],
            [WinFunc(ROW_NUMBER), WinFunc(SUM, d_rev, None, PT_I64, mode=ROWS, lo=UNBOUNDED, hi=0)],
            N)
        bufs += [d_rn, d_run]
        assert rn_nulls is None and run_nulls is None
        (d_mask, _), = eng.project([("cmp", "<=", ("col", 0), ("const", TOP))],
                                   [(d_rn, None, PT_I64)], [XO_MASK], N)
        bufs.append(d_mask)
        count = eng.mask_compact(d_mask, N, [])
        srcs = [(d_region, 4, np.int32), (d_year, 4, np.int32), (d_ynul, 1, np.uint8),
                (d_rev, 8, np.int64), (d_rn, 8, np.int64)]
        dsts = [eng.alloc(max(count * w, 1)) for _, w, _ in srcs]
        bufs += dsts
        assert eng.mask_compact(d_mask, N, [(s, d, w) for (s, w, _), d in zip(srcs, dsts)]) == count
        g_region, g_year, g_ynul, g_rev, g_rn = (d.d2h(dt, count) for d, (_, _, dt) in
                                                 zip(dsts, srcs))
        running = d_run.d2h(np.int64, N)
    finally:
        for b in bufs:
            b.free()

    # numpy: stable sort by (region, year NULLS FIRST, revenue DESC), then rank inside the group
    rev = price.astype(np.int64) * (100 - disc.astype(np.int64))
    yv = np.where(year_nulls != 0, 0, year).astype(np.int64)
    order = np.lexsort([-rev, yv, year_nulls == 0, region])
    gkey = region[order].astype(np.int64) * 100_000 + np.where(year_nulls[order] != 0, 0, yv[order] + 1)
    first = np.append(True, gkey[1:] != gkey[:-1])
    start = np.maximum.accumulate(np.where(first, np.arange(N), 0))
    rn = np.arange(N) - start + 1
    keep = order[rn <= TOP]
    assert count == len(keep) and count > 0

    def row_set(reg, yn, yr, rv, r):
        rows = np.stack([reg.astype(np.int64), (yn != 0).astype(np.int64),
                         np.where(yn != 0, 0, yr).astype(np.int64), rv, r], axis=1)
        return rows[np.lexsort(rows.T[::-1])]
    np.testing.assert_array_equal(
        row_set(g_region, g_ynul, g_year, g_rev, g_rn),
        row_set(region[keep], year_nulls[keep], year[keep], rev[keep], rn[rn <= TOP]))

    csum = np.cumsum(rev[order])
    before = np.where(start > 0, csum[np.maximum(start - 1, 0)], 0)
    want_running = np.empty(N, np.int64)
    want_running[order] = csum - before
    np.testing.assert_array_equal(running, want_running)
