"""SSB Q1 (config 2) through the GENERIC operator chain with a Project step —
no special-purpose kernel.

SUM(lo_extendedprice * lo_discount) over lineorder JOIN dates WHERE d_year =
1993, the way a plan of generic operators computes it: a selector-built
RANGE_DIRECT table over the filtered dim keys, probe-emit, gathers of the two
fact columns, Engine.project of [ep * dc AS BIGINT, 0 AS BIGINT] (the value and
the constant group key), and the generic hash aggregate. gpue_sum_prod_u32 —
the one-off kernel the operator pipeline uses for this aggregate — is not
called. The result must equal the oracle and the fused kernel bit-exactly.

It also widens an int32 column to int64 on the device (("col", 0) -> XO_I64),
the step tests/test_generic_q21.py does with a host round trip.
"""

import numpy as np
import pytest

from oracle import pyoracle as orc
from starrocks_amd import gen
from starrocks_amd.expr import XO_I64
from starrocks_amd.predicate import PT_I32

pytestmark = pytest.mark.gpu

SEED, YEAR = 42, 1993
N = 1_000_000


def test_q1_generic_chain_with_project(engine):
    od, ep, dc = (engine.alloc(N * 4) for _ in range(3))
    engine.gen_lineorder_q1(SEED, 0, N, od, ep, dc)

    # dim scan with its predicate applied, then the selector-driven build
    datekey, dyear = gen.gen_dates()
    dkeys = np.concatenate([[0], datekey[dyear == YEAR]]).astype(np.int32)   # rows are 1-based
    kb = engine.alloc(dkeys.nbytes)
    kb.h2d(dkeys)
    dates_t, method = engine.join_build_auto(kb, len(dkeys) - 1)
    kb.free()
    assert "RANGE_DIRECT" in engine.JM_NAMES[method], engine.JM_NAMES[method]

    # join: INNER emit, then the probe-side gathers
    c = engine.join_probe_emit(dates_t, od, N)
    assert 0 < c < N
    rows, bidx, ep1, dc1 = (engine.alloc(c * 4) for _ in range(4))
    engine.join_probe_emit(dates_t, od, N, rows, bidx)
    engine.gather_u32(ep, rows, c, ep1)
    engine.gather_u32(dc, rows, c, dc1)

    # project: the aggregate's argument and its (constant) group key, one pass
    (prod, prod_nulls), (key, key_nulls) = engine.project(
        [("*", ("col", 0), ("col", 1)), ("const", 0)],
        [(ep1, None, PT_I32), (dc1, None, PT_I32)], [XO_I64, XO_I64], c)
    assert prod_nulls is None and key_nulls is None
    assert prod.nbytes == c * 8 and key.nbytes == c * 8

    # aggregate: one group
    ok_b, os_b, oc_b = (engine.alloc(16 * 8) for _ in range(3))
    ng = engine.hash_agg_sum_u64(key, prod, c, ok_b, os_b, oc_b, max_out=16, capacity_hint=16)
    assert ng == 1
    got = (int(os_b.d2h(np.int64, 1)[0]), int(oc_b.d2h(np.int64, 1)[0]))
    assert int(ok_b.d2h(np.uint64, 1)[0]) == 0

    assert got == orc.q1_pipeline(SEED, 0, N, YEAR)

    # the fused kernel over the payload table, as the bench runs it
    k = engine.alloc(datekey.nbytes)
    k.h2d(datekey.astype(np.int32))
    payload = np.where(dyear == YEAR, dyear - 1992 + 1, 0).astype(np.uint32)
    p = engine.alloc(payload.nbytes)
    p.h2d(payload)
    fused_t = engine.join_build_payload(k, p, len(datekey))
    assert got == engine.q1_join_sum(fused_t, od, ep, dc, N)

    # widen int32 -> int64 on the device
    (wide, wide_nulls), = engine.project([("col", 0)], [(ep, None, PT_I32)], [XO_I64], N)
    assert wide_nulls is None
    assert np.array_equal(wide.d2h(np.int64, N), ep.d2h(np.int32, N).astype(np.int64))

    for b in (od, ep, dc, rows, bidx, ep1, dc1, prod, key, ok_b, os_b, oc_b, k, p, wide):
        b.free()
    dates_t.destroy()
    fused_t.destroy()
