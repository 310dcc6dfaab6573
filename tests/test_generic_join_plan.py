"""Plans written on the general operators only, with the general hash join
in the middle: filter -> project -> JOIN -> group_agg.

test_project_full_outer_join_group_agg drives the two new pipeline operators
end to end: both inputs go through ProjectOperator (a nullable a / b column),
are joined FULL OUTER on (int32, nullable int64) in 4096-row chunks, and the
joined chunks go into GroupAggSinkOperator; the result is compared key-sorted
against numpy.

test_q21_on_the_general_join is SSB Q2.1 as tests/test_generic_q21.py runs it
— dim predicates applied at the dim scans, three joins, payload gathers, a
two-key GROUP BY — with Engine.hash_join / gather_outer / group_agg in place
of the RANGE_DIRECT tables, the 2xi32 key packing and the one-key aggregate.
It must equal the oracle's result, which is what that test compares with.
"""

import numpy as np
import pytest

from oracle import pyoracle as orc
from starrocks_amd import gen, groupagg
from starrocks_amd import hashjoin as hj
from starrocks_amd.expr import XO_I64
from starrocks_amd.hashjoin import NO_ROW, PT_I32, PT_I64
from starrocks_amd.pipeline import (ChunkSourceOperator, GeneralHashJoinBuildOperator,
                                    GeneralHashJoinProbeOperator, GroupAggSinkOperator,
                                    PipelineDriver, ProjectOperator)

pytestmark = pytest.mark.gpu

CHUNK = 4096
N_BUILD, N_PROBE = 20_000, 19_000  # neither a multiple of the chunk


def _source(engine, cols, n):
    def gen_chunk(row_start, rows):
        out = []
        for c in cols:
            b = engine.alloc(rows * c.itemsize)
            b.h2d(c[row_start:row_start + rows])
            out.append(b)
        return {"n": rows, "cols": out}
    return ChunkSourceOperator(gen_chunk, n, CHUNK)


def _table(rng, n, pay_dtype):
    k = rng.integers(0, 1000, n).astype(np.int32)
    a = rng.integers(0, 20, n).astype(np.int32)
    b = rng.integers(0, 5, n).astype(np.int32)  # a / 0 is NULL
    pay = rng.integers(-1000, 1000, n).astype(pay_dtype)
    return k, a, b, pay


def test_project_full_outer_join_group_agg(engine):
    rng = np.random.default_rng(11)
    bk, ba, bb, bv = _table(rng, N_BUILD, np.int64)
    pk, pa, pb, pw = _table(rng, N_PROBE, np.int32)
    pk[:50] = 5000  # probe-only and build-only keys
    bk[:50] = 6000
    quotient = [("/", ("col", 0), ("col", 1))]
    project = lambda: ProjectOperator(engine, quotient, [(1, None, PT_I32), (2, None, PT_I32)],
                                      [XO_I64], keep=[0, 3])
    # projected chunks: key, payload, q, q's null mask
    build_op = GeneralHashJoinBuildOperator(
        engine, [(0, None, PT_I32), (2, 3, PT_I64)], [np.int32, np.int64, np.int64, np.uint8])
    try:
        PipelineDriver([_source(engine, [bk, ba, bb, bv], N_BUILD), project(),
                        build_op]).process()
        assert build_op.rows == N_BUILD
        probe_op = GeneralHashJoinProbeOperator(
            engine, build_op, "full_outer", [(0, None, PT_I32), (2, 3, PT_I64)],
            [np.int32, np.int32, np.int64, np.uint8],
            probe_payload=[(0, None), (1, None), (2, 3)], build_payload=[(0, None), (1, None)])
        u8 = np.dtype(np.uint8)
        assert probe_op.out_dtypes == [np.dtype(np.int32), u8, np.dtype(np.int32), u8,
                                       np.dtype(np.int64), u8, np.dtype(np.int32), u8,
                                       np.dtype(np.int64), u8]
        sink = GroupAggSinkOperator(
            engine, [(0, 1, PT_I32), (6, 7, PT_I32)],
            [("count_star", None, None, PT_I64), ("sum", 8, 9, PT_I64), ("sum", 2, 3, PT_I32),
             ("count", 4, 5, PT_I64)])
        g, keys, aggs = PipelineDriver([_source(engine, [pk, pa, pb, pw], N_PROBE), project(),
                                        probe_op, sink]).process()
    finally:
        build_op.release()

    # numpy: the quotient, the join's pairs, the payload through them, the groups
    quot = lambda a, b: (np.where(b == 0, 0, a // np.maximum(b, 1)).astype(np.int64),
                         (b == 0).astype(np.uint8))
    bq, bqn = quot(ba, bb)
    pq, pqn = quot(pa, pb)
    pairs = hj.hash_join_how_ref([(bk, None, PT_I32), (bq, bqn, PT_I64)],
                                 [(pk, None, PT_I32), (pq, pqn, PT_I64)], "full_outer")
    pi, bi = pairs[:, 0], pairs[:, 1]
    n = len(pairs)
    assert np.sum(pi == NO_ROW) > 50 and np.sum(bi == NO_ROW) > 50 and n > N_PROBE + 5000
    assert probe_op.rows == n and sink.rows == n
    take = lambda col, nulls, idx: hj.gather_outer_ref(col, nulls, idx.astype(np.uint32))
    jpk, jpk_n = take(pk, None, pi)
    jw, jw_n = take(pw, None, pi)
    jq, jq_n = take(pq, pqn, pi)
    jbk, jbk_n = take(bk, None, bi)
    jv, jv_n = take(bv, None, bi)
    want_g, want_keys, want_aggs = groupagg.group_agg_ref(
        [(jpk, jpk_n, PT_I32), (jbk, jbk_n, PT_I32)],
        [("count_star", None, None, PT_I64), ("sum", jv, jv_n, PT_I64), ("sum", jw, jw_n, PT_I32),
         ("count", jq, jq_n, PT_I64)], n)
    assert g == want_g
    for (v, nl), (wv, wnl) in zip(keys + aggs, want_keys + want_aggs):
        assert np.array_equal(v, wv)
        assert (nl is None) == (wnl is None) and (nl is None or np.array_equal(nl, wnl))


SEED, CAT, REG = 42, 12, 2
N = 500_000


def test_q21_on_the_general_join(engine):
    bufs = []

    def put(arr):
        b = engine.alloc(max(arr.nbytes, 4))
        b.h2d(arr)
        bufs.append(b)
        return b

    def out(n, width=4):
        bufs.append(engine.alloc(max(n, 1) * width))
        return bufs[-1]

    def join(dim_keys, fact_col, n_fact):
        """INNER join of a fact column with filtered dim keys (build rows from 0)."""
        op, ob, c = engine.hash_join([(put(dim_keys), None, PT_I32, len(dim_keys))],
                                     [(fact_col, None, PT_I32, n_fact)], "inner")
        bufs.extend([op, ob])
        return op, ob, c

    def gather(cols, idx, c):
        res = []
        for col in cols:
            res.append(out(c))
            engine.gather_u32(col, idx, c, res[-1])
        return res

    try:
        pk, sk, od, rv = (out(N) for _ in range(4))
        engine.gen_lineorder_q21(SEED, 0, N, pk, sk, od, rv)

        # dim scans with their predicates applied
        pfirst = gen.build_part_dim_payload(SEED, gen.N_PARTS_SF100, CAT)
        part_keys = (np.flatnonzero(pfirst) + 1).astype(np.int32)
        brand_by_row = pfirst[part_keys - 1].astype(np.uint32)
        sfirst = gen.build_supp_dim_payload(SEED, gen.N_SUPPS_SF100, REG)
        supp_keys = (np.flatnonzero(sfirst) + 1).astype(np.int32)
        datekey, dyear = gen.gen_dates()
        year_by_row = (dyear - 1992 + 1).astype(np.uint32)

        # join 1: lineorder with parts; the brand comes through the build index
        rows1, bidx1, c1 = join(part_keys, pk, N)
        assert 0 < c1 < N
        brand1 = out(c1)
        engine.gather_outer(put(brand_by_row), None, len(part_keys), 4, bidx1, c1, brand1)
        sk1, od1, rv1 = gather((sk, od, rv), rows1, c1)

        # join 2: with suppliers (unique keys: INNER is the semi-join filter)
        rows2, _, c2 = join(supp_keys, sk1, c1)
        assert 0 < c2 < c1
        od2, rv2, brand2 = gather((od1, rv1, brand1), rows2, c2)

        # join 3: with dates; the year comes through the build index
        rows3, bidx3, c3 = join(datekey.astype(np.int32), od2, c2)
        assert c3 == c2  # every order date is a date
        year3 = out(c3)
        engine.gather_outer(put(year_by_row), None, len(datekey), 4, bidx3, c3, year3)
        rv3, brand3 = gather((rv2, brand2), rows3, c3)

        # GROUP BY (year, brand), SUM(revenue)
        g, keys, aggs = engine.group_agg([(year3, None, PT_I32), (brand3, None, PT_I32)],
                                         [("sum", rv3, None, PT_I32)], c3)
        bufs.extend(b for pair in keys + aggs for b in pair if b is not None)
        got = np.zeros(7000, np.int64)
        year = keys[0][0].d2h(np.int32, g).astype(np.int64)
        brand = keys[1][0].d2h(np.int32, g).astype(np.int64)
        got[(year - 1) * 1000 + (brand - 1)] = aggs[0][0].d2h(np.int64, g)
        assert np.array_equal(got, orc.q21_pipeline(SEED, 0, N, CAT, REG))
    finally:
        for b in bufs:
            b.free()
