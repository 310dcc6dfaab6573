"""General GROUP BY without a GPU: the numpy reference against a plain-Python
brute force, merge of partials, AVG finalize, everything GroupAggSpec
rejects, the static nullability rule, and GroupAggSinkOperator over a numpy
stand-in engine."""

import numpy as np
import pytest

from starrocks_amd import groupagg as ga
from starrocks_amd.groupagg import (COUNT, COUNT_STAR, MAX, MIN, PT_I32, PT_I64, SUM,
                                    GroupAggSpec, avg_finalize, group_agg_ref, merge_ref,
                                    sort_result)
from starrocks_amd.pipeline import GroupAggSinkOperator

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DT = {PT_I32: np.int32, PT_I64: np.int64}


def wrap64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def brute(keys, aggs, n, merge=False):
    """dict of tuples; every rule written out the slow way."""
    groups = {}
    for i in range(n):
        kt = []
        for v, nl, _ in keys:
            isn = nl is not None and nl[i] != 0
            kt.append((1, 0) if isn else (0, int(v[i])))
        st = groups.setdefault(tuple(kt), [[0, False] if fn in (COUNT_STAR, COUNT, SUM)
                                           else [None, False] for fn, _, _, _ in aggs])
        for a, (fn, v, nl, _) in enumerate(aggs):
            if fn == COUNT_STAR and not merge:
                st[a][0] += 1
                continue
            if nl is not None and nl[i] != 0:
                continue
            x = int(v[i])
            st[a][1] = True
            if fn == COUNT and not merge:
                st[a][0] += 1
            elif fn in (COUNT_STAR, COUNT, SUM):
                st[a][0] = wrap64(st[a][0] + x)
            elif fn == MIN:
                st[a][0] = x if st[a][0] is None else min(st[a][0], x)
            else:
                st[a][0] = x if st[a][0] is None else max(st[a][0], x)
    order = sorted(groups)
    out_keys = []
    for k, (_, nl, t) in enumerate(keys):
        out_keys.append((np.array([g[k][1] for g in order], DT[t]),
                         None if nl is None else np.array([g[k][0] for g in order], np.uint8)))
    out_aggs = []
    for a, (fn, _, nl, _) in enumerate(aggs):
        nullable = fn >= SUM and nl is not None
        vals, nulls = [], []
        for g in order:
            v, seen = groups[g][a]
            if fn >= MIN and not seen:
                v = {MIN: I64_MAX, MAX: I64_MIN}[fn]
            isn = nullable and not seen
            vals.append(0 if isn else v)
            nulls.append(1 if isn else 0)
        out_aggs.append((np.array(vals, np.int64).reshape(-1),
                         np.array(nulls, np.uint8) if nullable else None))
    return len(order), out_keys, out_aggs


def assert_same(got, want):
    assert got[0] == want[0]
    for gp, wp in ((got[1], want[1]), (got[2], want[2])):
        assert len(gp) == len(wp)
        for (gv, gn), (wv, wn) in zip(gp, wp):
            assert gv.dtype == wv.dtype
            np.testing.assert_array_equal(gv, wv)
            assert (gn is None) == (wn is None)
            if gn is not None:
                assert gn.dtype == np.uint8
                np.testing.assert_array_equal(gn, wn)


def rand_col(rng, n, t, card, extremes=False):
    if t == PT_I32:
        v = rng.integers(-card, card, n).astype(np.int32)
        if extremes and n:
            v[rng.integers(0, n, max(n // 8, 1))] = np.iinfo(np.int32).min
    else:
        v = rng.integers(-card, card, n).astype(np.int64)
        if extremes and n:
            v[rng.integers(0, n, max(n // 8, 1))] = I64_MAX
            v[rng.integers(0, n, max(n // 8, 1))] = I64_MIN
            v[rng.integers(0, n, max(n // 8, 1))] = -1
    return v


def rand_nulls(rng, n, rate):
    if rate is None:
        return None
    return (rng.random(n) < rate).astype(np.uint8) * rng.integers(1, 255, n).astype(np.uint8)


def make_case(seed, n, key_spec, agg_spec, card=5):
    """key_spec = [(type, null rate or None)], agg_spec = [(fn, type, null rate or None)].
    Cells under a NULL hold garbage."""
    rng = np.random.default_rng(seed)
    keys = []
    for t, rate in key_spec:
        v, nl = rand_col(rng, n, t, card, extremes=True), rand_nulls(rng, n, rate)
        if nl is not None:
            v = np.where(nl != 0, rng.integers(-99, 99, n).astype(v.dtype), v)
        keys.append((v, nl, t))
    aggs = []
    for fn, t, rate in agg_spec:
        if fn == COUNT_STAR:
            aggs.append((fn, None, None, PT_I64))
        else:
            aggs.append((fn, rand_col(rng, n, t, 1 << 20, extremes=True),
                         rand_nulls(rng, n, rate), t))
    return keys, aggs


ALL5 = lambda t, r: [(COUNT_STAR, t, None), (COUNT, t, r), (SUM, t, r), (MIN, t, r), (MAX, t, r)]
REF_CASES = [
    (0, [(PT_I32, None)], []),
    (1, [(PT_I64, None)], [(COUNT_STAR, PT_I64, None)]),
    (2, [(PT_I32, None), (PT_I32, None)], ALL5(PT_I64, None)),
    (3, [(PT_I32, None), (PT_I64, 0.3)], ALL5(PT_I64, 0.3)),
    (4, [(PT_I64, 0.3), (PT_I32, 0.3), (PT_I64, 0.3), (PT_I32, 0.3)], ALL5(PT_I32, 0.3)),
    (5, [(PT_I64, 1.0), (PT_I32, 0.3)], ALL5(PT_I64, 1.0)),
    (6, [(PT_I32, 0.0)], ALL5(PT_I64, 0.0) + [(SUM, PT_I32, 0.3), (MIN, PT_I32, 1.0),
                                             (MAX, PT_I64, None)]),
]


@pytest.mark.parametrize("n", [0, 1, 7, 500, 2000])
@pytest.mark.parametrize("seed,key_spec,agg_spec", REF_CASES)
def test_ref_matches_brute_force(seed, key_spec, agg_spec, n):
    keys, aggs = make_case(seed * 100 + n, n, key_spec, agg_spec)
    assert_same(group_agg_ref(keys, aggs, n), brute(keys, aggs, n))


def test_ref_garbage_under_null_is_one_group():
    n = 64
    k0 = np.arange(n, dtype=np.int64)           # all different, all NULL
    k1 = np.repeat(np.array([3, 4], np.int32), n // 2)
    g, keys, aggs = group_agg_ref([(k0, np.ones(n, np.uint8), PT_I64), (k1, None, PT_I32)],
                                  [(COUNT_STAR, None, None, PT_I64)], n)
    assert g == 2
    np.testing.assert_array_equal(keys[0][0], [0, 0])
    np.testing.assert_array_equal(keys[0][1], [1, 1])
    np.testing.assert_array_equal(aggs[0][0], [32, 32])


def test_ref_sum_wraps_and_extremes():
    v = np.array([I64_MAX, 1, I64_MIN, I64_MIN], np.int64)
    k = np.array([0, 0, 1, 1], np.int32)
    g, _, aggs = group_agg_ref([(k, None, PT_I32)],
                               [(SUM, v, None, PT_I64), (MIN, v, None, PT_I64),
                                (MAX, v, None, PT_I64)], 4)
    assert g == 2
    np.testing.assert_array_equal(aggs[0][0], [I64_MIN, 0])
    np.testing.assert_array_equal(aggs[1][0], [1, I64_MIN])
    np.testing.assert_array_equal(aggs[2][0], [I64_MAX, I64_MIN])


def test_ref_all_null_group_is_null():
    k = np.array([1, 1, 2], np.int32)
    v = np.array([5, 6, 7], np.int64)
    nl = np.array([1, 9, 0], np.uint8)
    _, _, aggs = group_agg_ref([(k, None, PT_I32)], [(f, v, nl, PT_I64) for f in
                                                     (COUNT, SUM, MIN, MAX)], 3)
    np.testing.assert_array_equal(aggs[0][0], [0, 1])
    assert aggs[0][1] is None
    for a in (1, 2, 3):
        np.testing.assert_array_equal(aggs[a][0], [0, 7])
        np.testing.assert_array_equal(aggs[a][1], [1, 0])


@pytest.mark.parametrize("parts", [1, 2, 4, 7])
@pytest.mark.parametrize("seed,key_spec,agg_spec", REF_CASES[2:6])
def test_merge_of_partials_equals_one_shot(seed, key_spec, agg_spec, parts):
    n = 1500
    keys, aggs = make_case(seed, n, key_spec, agg_spec)
    cuts = np.linspace(0, n, parts + 1).astype(int)
    sl = lambda x, lo, hi: None if x is None else x[lo:hi]
    partials = []
    for lo, hi in zip(cuts, cuts[1:]):
        partials.append(group_agg_ref([(sl(v, lo, hi), sl(nl, lo, hi), t) for v, nl, t in keys],
                                      [(f, sl(v, lo, hi), sl(nl, lo, hi), t)
                                       for f, v, nl, t in aggs], hi - lo))
    merged = merge_ref(partials, [t for _, _, t in keys], [a[0] for a in aggs])
    assert_same(merged, group_agg_ref(keys, aggs, n))


def test_merge_skips_null_partials_and_adds_counts():
    k = np.array([1, 1, 2], np.int32)
    part = [(k, None, PT_I32)]
    cnt = np.array([3, 4, 5], np.int64)
    s = np.array([10, 999, 0], np.int64)
    s_null = np.array([0, 1, 1], np.uint8)
    g, _, aggs = group_agg_ref(part, [(COUNT_STAR, cnt, None, PT_I64),
                                      (SUM, s, s_null, PT_I64)], 3, merge=True)
    assert g == 2
    np.testing.assert_array_equal(aggs[0][0], [7, 5])
    np.testing.assert_array_equal(aggs[1][0], [10, 0])
    np.testing.assert_array_equal(aggs[1][1], [0, 1])


def test_avg_finalize():
    v, nl = avg_finalize([10, 7, 0, -9], [0, 0, 1, 0], [4, 2, 0, 3])
    np.testing.assert_array_equal(v, [2.5, 3.5, 0.0, -3.0])
    np.testing.assert_array_equal(nl, [0, 0, 1, 0])
    assert v.dtype == np.float64 and nl.dtype == np.uint8
    v, nl = avg_finalize([6, 0], None, [3, 0])     # NOT NULL input, empty group
    np.testing.assert_array_equal(v, [2.0, 0.0])
    np.testing.assert_array_equal(nl, [0, 1])


def test_static_output_nullability():
    spec = GroupAggSpec([PT_I32], [False], [COUNT_STAR, COUNT, SUM, MIN, MAX, SUM, MIN, MAX],
                        [PT_I64] * 8, [True, True, True, True, True, False, False, False])
    assert spec.out_nullable == [False, False, True, True, True, False, False, False]
    named = GroupAggSpec([PT_I64], [True], ["count_star", "sum"], [0, PT_I32], [False, True])
    assert named.agg_fns == [COUNT_STAR, SUM] and named.out_nullable == [False, True]


class B:
    def __init__(self, nbytes):
        self.nbytes = nbytes


@pytest.mark.parametrize("args", [
    ([], []),                                                   # n_keys 0
    ([PT_I32] * 5, [False] * 5),                                # n_keys 5
    ([7], [False]),                                             # unknown key type
    ([PT_I32], [False, True]),                                  # lengths differ
    ([PT_I32], [False], [SUM] * 9, [PT_I64] * 9, [False] * 9),  # n_aggs 9
    ([PT_I32], [False], [5], [PT_I64], [False]),                # unknown function
    ([PT_I32], [False], ["median"], [PT_I64], [False]),
    ([PT_I32], [False], [SUM], [3], [False]),                   # unknown input type
    ([PT_I32], [False], [SUM], [PT_I64], []),                   # lengths differ
])
def test_spec_value_errors(args):
    with pytest.raises(ValueError):
        GroupAggSpec(*args)


def test_push_and_emit_value_errors():
    spec = GroupAggSpec([PT_I32, PT_I64], [False, True], [COUNT_STAR, SUM, COUNT],
                        [0, PT_I64, PT_I32], [False, True, False])
    n = 10
    keys = [(B(40), None), (B(80), B(10))]
    aggs = [(None, None), (B(80), B(10)), (B(40), None)]
    spec.check_push(keys, aggs, n)
    spec.check_push(keys, aggs, 0)
    bad = [
        (keys, aggs, 1 << 32, 0),                                        # n_rows >= 2^32
        (keys, aggs, n, 2),                                              # unknown flag
        (keys[:1], aggs, n, 0),                                          # layout mismatch
        ([(B(39), None), keys[1]], aggs, n, 0),                          # short key
        ([keys[0], (B(80), B(9))], aggs, n, 0),                          # short key nulls
        ([(None, None), keys[1]], aggs, n, 0),                           # missing key
        ([(B(40), B(10)), keys[1]], aggs, n, 0),                         # nulls for NOT NULL key
        (keys, [aggs[0], (None, None), aggs[2]], n, 0),                  # missing input
        (keys, [aggs[0], (B(79), None), aggs[2]], n, 0),                 # short input
        (keys, [aggs[0], (B(80), B(9)), aggs[2]], n, 0),                 # short input nulls
        (keys, [aggs[0], aggs[1], (B(40), B(10))], n, 0),                # nulls for NOT NULL input
        (keys, aggs, n, 1),                                              # merge: COUNT_STAR input
        (keys, [(B(80), None), aggs[1], (B(40), None)], n, 1),           # merge: int64 partials
    ]
    for k, a, rows, flags in bad:
        with pytest.raises(ValueError):
            spec.check_push(k, a, rows, flags)
    spec.check_push(keys, [(B(80), None), aggs[1], (B(80), None)], n, 1)

    ok_k = [(B(40), None), (B(80), B(10))]
    ok_a = [(B(80), None), (B(80), B(10)), (B(80), None)]
    spec.check_emit(ok_k, ok_a, n)
    shared = B(80)
    bad = [
        (ok_k, ok_a, 1 << 32),
        (ok_k[:1], ok_a, n),
        ([(B(39), None), ok_k[1]], ok_a, n),                             # short key output
        ([ok_k[0], (B(80), None)], ok_a, n),                             # nullable key, no nulls
        (ok_k, [ok_a[0], (B(80), None), ok_a[2]], n),                    # nullable output, no nulls
        (ok_k, [ok_a[0], (B(80), B(9)), ok_a[2]], n),
        (ok_k, [(B(72), None), ok_a[1], ok_a[2]], n),                    # short aggregate output
        (ok_k, [(shared, None), ok_a[1], (shared, None)], n),            # one buffer twice
    ]
    for k, a, m in bad:
        with pytest.raises(ValueError):
            spec.check_emit(k, a, m)


def test_ref_rejects_bad_input():
    k = np.zeros(4, np.int32)
    with pytest.raises(ValueError):
        group_agg_ref([(k, None, PT_I32)], [(SUM, None, None, PT_I64)], 4)
    with pytest.raises(ValueError):
        group_agg_ref([(k, None, PT_I32)], [], 5)
    with pytest.raises(ValueError):
        group_agg_ref([], [], 0)


# ---- GroupAggSinkOperator over a numpy stand-in engine -------------------

class NpBuf:
    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.mem = np.zeros(nbytes, np.uint8)
        self.freed = False

    def h2d(self, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.mem[:raw.size] = raw
        return self

    def d2h(self, dtype, count, src_off=0):
        assert not self.freed
        return self.mem[src_off:src_off + count * np.dtype(dtype).itemsize].view(dtype).copy()

    def free(self):
        assert not self.freed, "double free"
        self.freed = True


class NpGroupAggEngine:
    """Just what GroupAggSinkOperator may call. The table is the list of
    pushed (possibly merged) inputs, folded with the numpy reference."""

    def __init__(self):
        self.bufs = []
        self.destroyed = 0

    def alloc(self, nbytes):
        assert nbytes > 0
        self.bufs.append(NpBuf(nbytes))
        return self.bufs[-1]

    def group_agg_create(self, key_types, key_nullable, agg_fns=(), agg_types=(),
                         agg_nullable=(), capacity_hint=0):
        return {"spec": GroupAggSpec(key_types, key_nullable, agg_fns, agg_types, agg_nullable),
                "partials": []}

    def group_agg_push(self, t, keys, aggs, n_rows, merge=False):
        spec = t["spec"]
        spec.check_push(keys, aggs, n_rows, 1 if merge else 0)
        for b in [x for p in keys + aggs for x in p if x is not None]:
            assert not b.freed
        view = lambda b, dt: None if b is None else b.d2h(dt, n_rows)
        null = lambda nl, declared: (np.zeros(n_rows, np.uint8) if nl is None and declared
                                     else view(nl, np.uint8))
        k = [(view(v, DT[tp]), null(nl, spec.key_nullable[i]), tp)
             for i, ((v, nl), tp) in enumerate(zip(keys, spec.key_types))]
        a = []
        for i, ((v, nl), fn, tp) in enumerate(zip(aggs, spec.agg_fns, spec.agg_types)):
            used = spec.needs_input(i, merge)
            a.append((fn, view(v, np.int64 if merge else DT[tp]) if used else None,
                      null(nl, spec.agg_nullable[i]) if used else None, tp))
        t["partials"].append(group_agg_ref(k, a, n_rows, merge=merge))

    def group_agg_emit_alloc(self, t):
        spec = t["spec"]
        if t["partials"]:
            g, keys, aggs = merge_ref(t["partials"], spec.key_types, spec.agg_fns)
        else:
            g, keys, aggs = 0, [(np.empty(0, DT[tp]), np.empty(0, np.uint8) if nl else None)
                                for tp, nl in zip(spec.key_types, spec.key_nullable)], \
                [(np.empty(0, np.int64), np.empty(0, np.uint8) if nl else None)
                 for nl in spec.out_nullable]
        put = lambda arr: None if arr is None else self.alloc(max(arr.nbytes, 1)).h2d(arr)
        return g, [(put(v), put(nl)) for v, nl in keys], [(put(v), put(nl)) for v, nl in aggs]

    def group_agg_destroy(self, t):
        self.destroyed += 1


def to_chunks(eng, cols, n, chunk_rows):
    chunks = []
    for lo in range(0, n, chunk_rows):
        hi = min(lo + chunk_rows, n)
        chunks.append({"n": hi - lo,
                       "cols": [eng.alloc(max(c[lo:hi].nbytes, 1)).h2d(c[lo:hi]) for c in cols]})
    return chunks


def test_sink_operator_multi_chunk():
    n = 1000
    keys, aggs = make_case(11, n, [(PT_I32, None), (PT_I64, 0.3)], ALL5(PT_I64, 0.3))
    cols = [keys[0][0], keys[1][0], keys[1][1], aggs[1][1], aggs[1][2]]
    eng = NpGroupAggEngine()
    op = GroupAggSinkOperator(eng, [(0, None, PT_I32), (1, 2, PT_I64)],
                              [("count_star", None, None, PT_I64), ("count", 3, 4, PT_I64),
                               (SUM, 3, 4, PT_I64), (MIN, 3, 4, PT_I64), (MAX, 3, 4, PT_I64)])
    chunks = to_chunks(eng, cols, n, 130) + [{"n": 0, "cols": [eng.alloc(1)]}]
    for c in chunks:
        assert op.need_input() and not op.has_output()
        op.push_chunk(c)
    op.set_finishing()
    assert op.is_finished() and op.rows == n
    v = aggs[1][1]
    nl = aggs[1][2]
    want = group_agg_ref(keys, [(COUNT_STAR, None, None, PT_I64)] +
                         [(f, v, nl, PT_I64) for f in (COUNT, SUM, MIN, MAX)], n)
    assert_same(op.result(), want)
    assert all(b.freed for b in eng.bufs)      # pushed chunks and emit buffers
    assert eng.destroyed == 1


def test_sink_operator_merge_mode():
    n, parts = 1200, 3
    keys, aggs = make_case(12, n, [(PT_I32, 0.3)], ALL5(PT_I32, 0.3))
    want = group_agg_ref(keys, aggs, n)
    eng = NpGroupAggEngine()
    final = GroupAggSinkOperator(
        eng, [(0, 1, PT_I32)],
        [(COUNT_STAR, 2, None, PT_I64), (COUNT, 3, None, PT_I32), (SUM, 4, 5, PT_I32),
         (MIN, 6, 7, PT_I32), (MAX, 8, 9, PT_I32)], merge=True)
    cuts = np.linspace(0, n, parts + 1).astype(int)
    sl = lambda x, lo, hi: None if x is None else x[lo:hi]
    for lo, hi in zip(cuts, cuts[1:]):
        g, pk, pa = group_agg_ref([(sl(v, lo, hi), sl(nl, lo, hi), t) for v, nl, t in keys],
                                  [(f, sl(v, lo, hi), sl(nl, lo, hi), t)
                                   for f, v, nl, t in aggs], hi - lo)
        cols = [pk[0][0], pk[0][1], pa[0][0], pa[1][0], pa[2][0], pa[2][1], pa[3][0],
                pa[3][1], pa[4][0], pa[4][1]]
        final.push_chunk(to_chunks(eng, cols, g, g)[0])
    assert_same(final.result(), want)
    assert all(b.freed for b in eng.bufs)


def test_sink_operator_rejects_bad_maps():
    eng = NpGroupAggEngine()
    with pytest.raises(ValueError):
        GroupAggSinkOperator(eng, [], [])
    with pytest.raises(ValueError):
        GroupAggSinkOperator(eng, [(0, None, PT_I32)], [(SUM, None, None, PT_I64)])
    with pytest.raises(ValueError):
        GroupAggSinkOperator(eng, [(0, None, PT_I32)], [(COUNT_STAR, None, None, PT_I64)],
                             merge=True)
    with pytest.raises(ValueError):
        GroupAggSinkOperator(eng, [(-1, None, PT_I32)], [])
    with pytest.raises(ValueError):
        GroupAggSinkOperator(eng, [(0, None, 9)], [])


def test_sort_result_orders_nulls_last_per_key():
    keys = [(np.array([5, 0, -3, 0], np.int64), np.array([0, 1, 0, 1], np.uint8)),
            (np.array([1, 2, 1, 1], np.int32), None)]
    aggs = [(np.array([10, 20, 30, 40], np.int64), None)]
    k, a = sort_result(keys, aggs)
    np.testing.assert_array_equal(k[0][0], [-3, 5, 0, 0])
    np.testing.assert_array_equal(k[0][1], [0, 0, 1, 1])
    np.testing.assert_array_equal(k[1][0], [1, 1, 1, 2])
    np.testing.assert_array_equal(a[0][0], [30, 10, 40, 20])
    assert ga.MERGE == 1 and ga.MAX_KEYS == 4 and ga.MAX_AGGS == 8
