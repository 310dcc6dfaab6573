"""General GROUP BY on the device: gpue_group_agg_* against the numpy
reference (starrocks_amd/groupagg.py), bit for bit after a key sort."""

import numpy as np
import pytest

from starrocks_amd.groupagg import (COUNT, COUNT_STAR, MAX, MIN, PT_I32, PT_I64, SUM,
                                    group_agg_ref, merge_ref, sort_result)

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DT = {PT_I32: np.int32, PT_I64: np.int64}
SIZES = [0, 1, 63, 64, 65, 4097, 70_001]
CARDS = ["one", "sqrt", "all"]


def up(eng, arr):
    if arr is None:
        return None
    arr = np.ascontiguousarray(arr)
    b = eng.alloc(max(arr.nbytes, 1))
    if arr.nbytes:
        b.h2d(arr)
    return b


def free_all(bufs):
    for b in bufs:
        if b is not None:
            b.free()


def download(g, keys, aggs, key_types):
    """Emitted DBuf pairs -> key-sorted numpy pairs; frees the buffers."""
    pull = lambda b, dt: np.empty(0, dt) if g == 0 else b.d2h(dt, g)
    hk = [(pull(v, DT[t]), None if nl is None else pull(nl, np.uint8))
          for (v, nl), t in zip(keys, key_types)]
    ha = [(pull(v, np.int64), None if nl is None else pull(nl, np.uint8)) for v, nl in aggs]
    free_all([b for p in keys + aggs for b in p])
    return (g,) + sort_result(hk, ha)


def run_gpu(eng, keys, aggs, n, capacity_hint=0, merge=False):
    dk = [(up(eng, v), up(eng, nl), t) for v, nl, t in keys]
    da = [(f, up(eng, v), up(eng, nl), t) for f, v, nl, t in aggs]
    try:
        g, ok, oa = eng.group_agg(dk, da, n, capacity_hint=capacity_hint, merge=merge)
    finally:
        free_all([k[0] for k in dk] + [k[1] for k in dk] + [a[1] for a in da] +
                 [a[2] for a in da])
    return download(g, ok, oa, [t for _, _, t in keys])


def assert_same(got, want):
    assert got[0] == want[0]
    for gp, wp in ((got[1], want[1]), (got[2], want[2])):
        assert len(gp) == len(wp)
        for (gv, gn), (wv, wn) in zip(gp, wp):
            assert gv.dtype == wv.dtype
            np.testing.assert_array_equal(gv, wv)
            assert (gn is None) == (wn is None)
            if gn is not None:
                np.testing.assert_array_equal(gn, wn)


def group_ids(rng, n, card):
    if card == "one" or n == 0:
        return np.zeros(n, np.int64)
    if card == "all":
        return rng.permutation(n).astype(np.int64)
    return rng.integers(0, max(int(np.sqrt(n)), 2), n).astype(np.int64)


def garbage(rng, n, dtype):
    return rng.integers(-1000, 1000, n).astype(dtype)


def key_shape(rng, gid, shape):
    """Key columns that are a function of the group id (so the cardinality is
    as asked, up to NULL groups merging); cells under a NULL hold per-row
    garbage."""
    n = len(gid)
    if shape == "i32":
        return [((gid * 7 - 1000).astype(np.int32), None, PT_I32)]
    if shape == "i64":
        lut = np.arange(int(gid.max()) + 1 if n else 1, dtype=np.int64) * 0x10000000001 + 5
        lut[:3] = [-1, I64_MIN, I64_MAX][:len(lut)]   # -1 is the old tables' sentinel pattern
        return [(lut[gid], None, PT_I64)]
    if shape == "2xi32":
        return [((gid // 50 - 3).astype(np.int32), None, PT_I32),
                ((gid % 50).astype(np.int32), None, PT_I32)]
    if shape == "i32+ni64":
        k1 = gid // 3
        nl = ((k1 % 4 == 0) * 200).astype(np.uint8)
        return [((gid % 3).astype(np.int32), None, PT_I32),
                (np.where(nl != 0, garbage(rng, n, np.int64), k1 - 7), nl, PT_I64)]
    assert shape == "4xnull"
    keys = []
    for j in range(4):
        t = PT_I64 if j % 2 else PT_I32
        nl = ((gid % 16 >> j & 1) != 0).astype(np.uint8)     # gid % 16 == 15: NULL on every key
        keys.append((np.where(nl != 0, garbage(rng, n, DT[t]), (gid + j).astype(DT[t])), nl, t))
    return keys


def agg_set(rng, gid, which):
    n = len(gid)
    if which == "none":
        return []
    if which == "count_star":
        return [(COUNT_STAR, None, None, PT_I64)]
    if which == "all5":
        v = rng.integers(-10**15, 10**15, n).astype(np.int64)
        # every input of the groups with gid % 3 == 0 is NULL, plus a random third
        nl = (((gid % 3 == 0) | (rng.random(n) < 0.3)) * 1).astype(np.uint8)
        v = np.where(nl != 0, garbage(rng, n, np.int64), v)
        return [(COUNT_STAR, None, None, PT_I64)] + [(f, v, nl, PT_I64)
                                                     for f in (COUNT, SUM, MIN, MAX)]
    assert which == "8x4"
    c0 = rng.integers(-2**31, 2**31, n).astype(np.int32)
    n0 = (rng.random(n) < 0.5).astype(np.uint8)
    c1 = rng.integers(-2**62, 2**62, n).astype(np.int64)
    if n:
        c1[rng.integers(0, n, max(n // 16, 1))] = I64_MAX
        c1[rng.integers(0, n, max(n // 16, 1))] = I64_MIN
    c2 = rng.integers(-100, 100, n).astype(np.int32)
    c3 = rng.integers(-2**40, 2**40, n).astype(np.int64)
    n3 = ((gid % 2 == 1) * 7).astype(np.uint8)
    return [(SUM, c0, n0, PT_I32), (MIN, c0, n0, PT_I32), (MAX, c1, None, PT_I64),
            (SUM, c1, None, PT_I64), (COUNT, c3, n3, PT_I64), (MAX, c3, n3, PT_I64),
            (MIN, c2, None, PT_I32), (COUNT_STAR, None, None, PT_I64)]


SHAPES = ["i32", "i64", "2xi32", "i32+ni64", "4xnull"]
AGG_SETS = ["none", "count_star", "all5", "8x4"]


@pytest.mark.parametrize("card", CARDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_cardinalities_shapes(engine, n, card):
    rng = np.random.default_rng(n * 3 + CARDS.index(card))
    gid = group_ids(rng, n, card)
    for i, shape in enumerate(SHAPES):
        keys = key_shape(rng, gid, shape)
        for which in (AGG_SETS[i % 4], AGG_SETS[(i + 1) % 4], AGG_SETS[(i + 2) % 4]):
            aggs = agg_set(rng, gid, which)
            got = run_gpu(engine, keys, aggs, n, capacity_hint=64)
            assert_same(got, group_agg_ref(keys, aggs, n))


def test_garbage_under_null_lands_in_one_group(engine):
    n = 4097
    k0 = np.arange(n, dtype=np.int64)                  # all different, all NULL
    k1 = (np.arange(n) % 2).astype(np.int32)
    keys = [(k0, np.full(n, 255, np.uint8), PT_I64), (k1, None, PT_I32)]
    g, hk, ha = run_gpu(engine, keys, [(COUNT_STAR, None, None, PT_I64)], n)
    assert g == 2
    np.testing.assert_array_equal(hk[0][0], [0, 0])    # 0 under NULL
    np.testing.assert_array_equal(hk[0][1], [1, 1])
    np.testing.assert_array_equal(hk[1][0], [0, 1])
    np.testing.assert_array_equal(ha[0][0], [2049, 2048])


def test_all_null_groups_emit_null(engine):
    n = 1000
    k = (np.arange(n) % 10).astype(np.int32)
    v = np.arange(n, dtype=np.int64) - 500
    nl = (k < 5).astype(np.uint8)                      # groups 0..4 see only NULLs
    g, hk, ha = run_gpu(engine, [(k, None, PT_I32)],
                        [(f, v, nl, PT_I64) for f in (COUNT, SUM, MIN, MAX)], n)
    assert g == 10
    np.testing.assert_array_equal(ha[0][0][:5], 0)
    assert ha[0][1] is None
    for a in (1, 2, 3):
        np.testing.assert_array_equal(ha[a][0][:5], 0)
        np.testing.assert_array_equal(ha[a][1], [1] * 5 + [0] * 5)
    assert_same((g, hk, ha), group_agg_ref([(k, None, PT_I32)],
                                           [(f, v, nl, PT_I64) for f in (COUNT, SUM, MIN, MAX)],
                                           n))


def test_growth_from_capacity_16(engine):
    n = 70_001
    rng = np.random.default_rng(7)
    gid = rng.permutation(n).astype(np.int64)
    keys = key_shape(rng, gid, "i64")
    aggs = agg_set(rng, gid, "all5")
    got = run_gpu(engine, keys, aggs, n, capacity_hint=16)
    assert got[0] == n
    assert_same(got, group_agg_ref(keys, aggs, n))


def test_overlapping_pushes_size_and_emit_between(engine):
    eng = engine
    n = 70_001
    k = np.arange(n, dtype=np.int64) * 3 - 5
    v = (np.arange(n, dtype=np.int64) % 1000) - 500
    spans = [(0, 30_000), (20_000, 50_001), (10_000, n)]
    ga = eng.group_agg_create([PT_I64], [False], [SUM, COUNT_STAR], [PT_I64, PT_I64],
                              [False, False], capacity_hint=16)
    bufs = []
    try:
        covered = np.zeros(n, bool)
        times = np.zeros(n, np.int64)
        for lo, hi in spans:
            dk, dv = up(eng, k[lo:hi]), up(eng, v[lo:hi])
            bufs += [dk, dv]
            eng.group_agg_push(ga, [(dk, None)], [(dv, None), (None, None)], hi - lo)
            covered[lo:hi] = True
            times[lo:hi] += 1
            assert eng.group_agg_size(ga) == int(covered.sum())
            # emit between pushes leaves the table usable
            g, ok, oa = eng.group_agg_emit_alloc(ga)
            got = download(g, ok, oa, [PT_I64])
            want_k = k[covered]
            order = np.argsort(want_k)
            np.testing.assert_array_equal(got[1][0][0], want_k[order])
            np.testing.assert_array_equal(got[2][0][0], (v * times)[covered][order])
            np.testing.assert_array_equal(got[2][1][0], times[covered][order])
        eng.group_agg_reset(ga)
        assert eng.group_agg_size(ga) == 0
        dk, dv = up(eng, k[:65]), up(eng, v[:65])
        bufs += [dk, dv]
        eng.group_agg_push(ga, [(dk, None)], [(dv, None), (None, None)], 65)
        g, ok, oa = eng.group_agg_emit_alloc(ga)
        got = download(g, ok, oa, [PT_I64])
        assert_same(got, group_agg_ref([(k[:65], None, PT_I64)],
                                       [(SUM, v[:65], None, PT_I64),
                                        (COUNT_STAR, None, None, PT_I64)], 65))
    finally:
        eng.group_agg_destroy(ga)
        free_all(bufs)


@pytest.mark.parametrize("shape", ["2xi32", "4xnull"])
def test_merge_of_four_partials(engine, shape):
    n, parts = 70_001, 4
    rng = np.random.default_rng(9)
    gid = group_ids(rng, n, "sqrt")
    keys = key_shape(rng, gid, shape)
    aggs = agg_set(rng, gid, "all5") + agg_set(rng, gid, "8x4")[:3]
    cuts = np.linspace(0, n, parts + 1).astype(int)
    sl = lambda x, lo, hi: None if x is None else x[lo:hi]
    partials = []
    for lo, hi in zip(cuts, cuts[1:]):
        partials.append(run_gpu(engine, [(sl(v, lo, hi), sl(nl, lo, hi), t) for v, nl, t in keys],
                                [(f, sl(v, lo, hi), sl(nl, lo, hi), t) for f, v, nl, t in aggs],
                                hi - lo))
    want = group_agg_ref(keys, aggs, n)
    # the reference merge of the device partials, then the device merge
    assert_same(merge_ref(partials, [t for _, _, t in keys], [a[0] for a in aggs]), want)
    cat = lambda xs: np.concatenate(xs)
    total = sum(p[0] for p in partials)
    mk = [(cat([p[1][i][0] for p in partials]),
           None if keys[i][1] is None else cat([p[1][i][1] for p in partials]), keys[i][2])
          for i in range(len(keys))]
    ma = [(aggs[a][0], cat([p[2][a][0] for p in partials]),
           None if partials[0][2][a][1] is None else cat([p[2][a][1] for p in partials]),
           aggs[a][3]) for a in range(len(aggs))]
    # COUNT's output is never NULL, so its merge input has no null column even
    # where the raw input had one: the merge table is declared from the partials
    assert_same(run_gpu(engine, mk, ma, total, capacity_hint=16, merge=True), want)


def test_parity_with_hash_agg_sum_and_stats(engine):
    eng = engine
    n = 70_001
    rng = np.random.default_rng(13)
    k = rng.integers(0, 5000, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    k[k == np.uint64(0xFFFFFFFFFFFFFFFF)] = 1          # the old entries' own domain
    v = rng.integers(-10**12, 10**12, n).astype(np.int64)
    dk, dv = up(eng, k), up(eng, v)
    outs = [eng.alloc(8 * 8192) for _ in range(5)]
    try:
        g = eng.hash_agg_sum_u64(dk, dv, n, outs[0], outs[1], out_counts=outs[2], max_out=8192)
        old = [outs[i].d2h(np.int64, g) for i in range(3)]
        order = np.argsort(old[0], kind="stable")
        got = run_gpu(eng, [(k.view(np.int64), None, PT_I64)],
                      [(SUM, v, None, PT_I64), (COUNT_STAR, None, None, PT_I64)], n)
        assert got[0] == g
        np.testing.assert_array_equal(got[1][0][0], old[0][order])
        np.testing.assert_array_equal(got[2][0][0], old[1][order])
        np.testing.assert_array_equal(got[2][1][0], old[2][order])

        g = eng.hash_agg_stats_u64(dk, dv, n, *outs, max_out=8192)
        old = [outs[i].d2h(np.int64, g) for i in range(5)]
        order = np.argsort(old[0], kind="stable")
        got = run_gpu(eng, [(k.view(np.int64), None, PT_I64)],
                      [(SUM, v, None, PT_I64), (COUNT_STAR, None, None, PT_I64),
                       (MIN, v, None, PT_I64), (MAX, v, None, PT_I64)], n)
        assert got[0] == g
        np.testing.assert_array_equal(got[1][0][0], old[0][order])
        for a in range(4):
            np.testing.assert_array_equal(got[2][a][0], old[a + 1][order])
    finally:
        free_all([dk, dv] + outs)


def test_project_division_feeds_group_agg(engine):
    """a / b with zero divisors is a nullable column; SUM over it grouped by a
    third column — the plan the single-key, NOT NULL aggregate cannot run."""
    eng = engine
    n = 4097
    rng = np.random.default_rng(17)
    a = rng.integers(-10**9, 10**9, n).astype(np.int64)
    b = rng.integers(-3, 4, n).astype(np.int64)
    c = rng.integers(0, 40, n).astype(np.int32)
    b[c == 7] = 0                                      # one group divides by zero only
    da, db, dc = up(eng, a), up(eng, b), up(eng, c)
    q = nl = None
    try:
        (q, nl), = eng.project([("/", ("col", 0), ("col", 1))],
                               [(da, None, PT_I64), (db, None, PT_I64)], [eng.XO_I64], n)
        assert nl is not None
        g, ok, oa = eng.group_agg([(dc, None, PT_I32)],
                                  [(eng.GA_SUM, q, nl, PT_I64), (eng.GA_COUNT, q, nl, PT_I64)], n)
        got = download(g, ok, oa, [PT_I32])
    finally:
        free_all([da, db, dc, q, nl])
    assert got[0] == 40
    for grp in range(40):
        sel = (c == grp) & (b != 0)
        # SQL integer division truncates toward zero
        quot = np.array([int(abs(int(x)) // abs(int(y))) * (1 if (x < 0) == (y < 0) else -1)
                         for x, y in zip(a[sel], b[sel])], np.int64)
        assert got[1][0][0][grp] == grp
        assert got[2][1][0][grp] == sel.sum()
        if sel.any():
            assert got[2][0][1][grp] == 0 and got[2][0][0][grp] == quot.sum()
        else:
            assert grp == 7 and got[2][0][1][grp] == 1 and got[2][0][0][grp] == 0


def test_argument_errors(engine):
    from starrocks_amd.engine import GpueError
    eng = engine
    bad_create = [
        dict(key_types=[], key_nullable=[]),
        dict(key_types=[PT_I32] * 5, key_nullable=[0] * 5),
        dict(key_types=[9], key_nullable=[0]),
        dict(key_types=[PT_I32], key_nullable=[0], agg_fns=[SUM] * 9, agg_types=[PT_I64] * 9,
             agg_nullable=[0] * 9),
        dict(key_types=[PT_I32], key_nullable=[0], agg_fns=[5], agg_types=[PT_I64],
             agg_nullable=[0]),
        dict(key_types=[PT_I32], key_nullable=[0], agg_fns=[SUM], agg_types=[4],
             agg_nullable=[0]),
    ]
    for kw in bad_create:
        with pytest.raises(GpueError, match="bad argument"):
            eng.group_agg_create(**kw)

    n = 100
    ga = eng.group_agg_create([PT_I32, PT_I64], [False, True], [COUNT_STAR, SUM, COUNT],
                              [PT_I64, PT_I64, PT_I32], [False, True, False])
    b400, b800, b100, short = eng.alloc(400), eng.alloc(800), eng.alloc(100), eng.alloc(99)
    more = [eng.alloc(800) for _ in range(4)] + [eng.alloc(100), eng.alloc(400)]
    try:
        keys = [(b400, None), (b800, b100)]
        aggs = [(None, None), (more[0], more[4]), (more[5], None)]
        bad_push = [
            (keys, aggs, 1 << 32, False),
            ([(short, None), keys[1]], aggs, n, False),            # short key
            ([keys[0], (b800, short)], aggs, n, False),            # short key nulls
            ([(None, None), keys[1]], aggs, n, False),             # missing key
            ([(b400, b100), keys[1]], aggs, n, False),             # nulls for a NOT NULL key
            (keys, [aggs[0], (None, None), aggs[2]], n, False),    # missing input
            (keys, [aggs[0], (b400, None), aggs[2]], n, False),    # short input
            (keys, [aggs[0], (more[0], short), aggs[2]], n, False),
            (keys, [aggs[0], aggs[1], (more[5], b100)], n, False),  # nulls for a NOT NULL input
            (keys, aggs, n, True),                                 # merge: COUNT_STAR needs input
            (keys, [(more[1], None), aggs[1], (more[5], None)], n, True),   # merge reads int64
        ]
        for k, a, rows, merge in bad_push:
            with pytest.raises(GpueError, match="bad argument"):
                eng.group_agg_push(ga, k, a, rows, merge)
        assert eng.group_agg_size(ga) == 0                         # nothing was pushed
        eng.group_agg_push(ga, keys, aggs, 0)                      # n_rows == 0 is fine
        assert eng.group_agg_size(ga) == 0

        ok_k = [(b400, None), (b800, b100)]
        ok_a = [(more[0], None), (more[1], more[4]), (more[2], None)]
        assert eng.group_agg_emit(ga, ok_k, ok_a, n) == 0
        bad_emit = [
            ([(short, None), ok_k[1]], ok_a, n),                   # short key output
            ([ok_k[0], (b800, None)], ok_a, n),                    # nullable key without nulls
            (ok_k, [ok_a[0], (more[1], None), ok_a[2]], n),        # nullable output without nulls
            (ok_k, [ok_a[0], (more[1], short), ok_a[2]], n),
            (ok_k, [(short, None), ok_a[1], ok_a[2]], n),          # short aggregate output
            (ok_k, [(more[0], None), ok_a[1], (more[0], None)], n),  # outputs overlap
            ([ok_k[0], (more[1], b100)], ok_a, n),                 # key output is an agg output
        ]
        for k, a, m in bad_emit:
            with pytest.raises(GpueError, match="bad argument"):
                eng.group_agg_emit(ga, k, a, m)

        # max_out too small: an error that carries the true count
        kv = np.arange(n, dtype=np.int32)
        b400.h2d(kv)
        b800.h2d(np.arange(n, dtype=np.int64))
        more[0].h2d(np.ones(n, np.int64))
        more[5].h2d(np.ones(n, np.int32))
        eng.group_agg_push(ga, [(b400, None), (b800, None)],
                           [(None, None), (more[0], None), (more[5], None)], n)
        assert eng.group_agg_size(ga) == n
        with pytest.raises(GpueError, match="100 groups exceed max_out 99"):
            eng.group_agg_emit(ga, ok_k, ok_a, 99)
        assert eng.group_agg_emit(ga, ok_k, [ok_a[0], ok_a[1], (more[3], None)], n) == n
    finally:
        eng.group_agg_destroy(ga)
        free_all([b400, b800, b100, short] + more)

    # the one-shot entry validates on the host
    with pytest.raises(ValueError):
        eng.group_agg([], [], 0)
    d = eng.alloc(40)
    try:
        with pytest.raises(ValueError):
            eng.group_agg([(d, None, PT_I32)], [(SUM, None, None, PT_I64)], 10)
        with pytest.raises(ValueError):
            eng.group_agg([(d, None, PT_I32)], [], 11)
    finally:
        d.free()


@pytest.mark.parametrize("groups", [1, 5, 32, 33])
@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_push_into_a_table_of_few_groups(engine, n, groups):
    """From the second push on, a table of 1..32 groups takes the wave-level
    pre-combine path (33 is the first size that does not); the first push
    seeds the groups, the second is the one under test."""
    eng = engine
    rng = np.random.default_rng(n * 31 + groups)
    seed_rows = 200
    total = seed_rows + n
    gid = np.concatenate([np.arange(seed_rows) % groups, rng.integers(0, groups, n)])
    for shape, which in (("i64", "all5"), ("4xnull", "8x4"), ("2xi32", "count_star")):
        keys = key_shape(rng, gid, shape)
        aggs = agg_set(rng, gid, which)
        spec_k = [(t, nl is not None) for _, nl, t in keys]
        ga = eng.group_agg_create([t for t, _ in spec_k], [x for _, x in spec_k],
                                  [a[0] for a in aggs], [a[3] for a in aggs],
                                  [a[2] is not None for a in aggs], capacity_hint=16)
        bufs = []
        try:
            for lo, hi in ((0, seed_rows), (seed_rows, total)):
                sl = lambda x: None if x is None else up(eng, x[lo:hi])
                dk = [(sl(v), sl(nl)) for v, nl, _ in keys]
                da = [(sl(v), sl(nl)) for _, v, nl, _ in aggs]
                bufs += [b for p in dk + da for b in p]
                eng.group_agg_push(ga, dk, da, hi - lo)
            g, ok, oa = eng.group_agg_emit_alloc(ga)
            got = download(g, ok, oa, [t for t, _ in spec_k])
        finally:
            eng.group_agg_destroy(ga)
            free_all(bufs)
        assert_same(got, group_agg_ref(keys, aggs, total))
