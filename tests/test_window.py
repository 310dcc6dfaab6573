"""Window functions on the device: gpue_window_eval / Engine.window /
WindowSinkOperator against the numpy reference (starrocks_amd/window.py), bit
for bit on values and null bytes.

T = rows per scan tile and A = tile aggregates per sweep of the middle pass
are window.py's copies of GPUE_WIN_TILE / GPUE_WIN_MID, which gpue.hip pins to
its own constants with a static_assert and tests/test_window_cpu.py pins to
the header; the shapes below sit on those edges."""

import numpy as np
import pytest

from starrocks_amd.engine import GpueError
from starrocks_amd.window import (A, COUNT, COUNT_STAR, DENSE_RANK, FIRST_VALUE, LAG,
                                  LAST_VALUE, LEAD, MAX, MIN, NTILE, PT_I32, PT_I64, RANGE,
                                  RANK, ROW_NUMBER, ROWS, SUM, T, UNBOUNDED, WinFunc,
                                  WindowSpec, sort_perm_ref, window_ref)

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DT = {PT_I32: np.int32, PT_I64: np.int64}
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
SHAPES = ["one", "singletons", "sqrt", "wave_edge", "tile_edge", "three_tiles", "edges1"]
PEERS = ["none", "all", "runs", "tile_cross"]
FILL = 0x5A


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


def filled(eng, nbytes):
    b = eng.alloc(max(nbytes, 1))
    eng._lib.gpue_dbuf_memset(b._h, FILL, max(nbytes, 1))
    return b


def pull(b, dtype, n):
    return np.empty(0, dtype) if n == 0 else b.d2h(dtype, n)


def run_eval(eng, pk, ok, funcs, n, order_idx=None, sorted_out=False):
    """One gpue_window_eval over host columns; checks on the way out that no
    input changed. Returns [(values, nulls or None)]."""
    spec = WindowSpec.of(pk, ok, funcs)
    host = [order_idx] + [c for k in pk + ok for c in k[:2]] + \
           [c for f in funcs for c in (f.col, f.nulls)]
    dev = [up(eng, a) for a in host]
    outs = []
    try:
        it = iter(dev)
        d_idx = next(it)
        dpk = [(next(it), next(it), k[2]) for k in pk]
        dok = [(next(it), next(it), k[2]) for k in ok]
        dfuncs = [f.with_cols(next(it), next(it)) for f in funcs]
        outs = [(filled(eng, n * 8), filled(eng, n) if nl else None) for nl in spec.out_nullable]
        eng.window_eval(n, d_idx, dpk, dok, dfuncs, outs, sorted_out)
        res = [(pull(v, np.int64, n), None if nl is None else pull(nl, np.uint8, n))
               for v, nl in outs]
        for a, b in zip(host, dev):
            if a is not None and a.size:
                np.testing.assert_array_equal(b.d2h(a.dtype, a.size), a)
    finally:
        free_all(dev + [b for p in outs for b in p])
    return res


def assert_same(got, want):
    assert len(got) == len(want)
    for (gv, gn), (wv, wn) in zip(got, want):
        np.testing.assert_array_equal(gv, wv)
        assert (gn is None) == (wn is None)
        if gn is not None:
            np.testing.assert_array_equal(gn, wn)


def check(eng, pk, ok, funcs, n, order_idx=None, sorted_out=False):
    assert_same(run_eval(eng, pk, ok, funcs, n, order_idx, sorted_out),
                window_ref(pk, ok, funcs, n, order_idx, sorted_out))


def lengths_to_ids(lengths, n):
    ids = np.repeat(np.arange(len(lengths)), lengths)[:n]
    return np.concatenate([ids, np.full(n - len(ids), len(lengths))]).astype(np.int64)


def part_ids(rng, n, shape):
    """Non-decreasing partition ids of n pre-sorted rows."""
    pos = np.arange(n, dtype=np.int64)
    if shape == "one":
        return np.zeros(n, np.int64)
    if shape == "singletons":
        return pos
    if shape == "wave_edge":
        return pos // 64
    if shape == "tile_edge":
        return pos // T
    if shape == "three_tiles":        # rows [5, 5 + 3T + 3) are one partition: a tile without a boundary
        return lengths_to_ids([5, 3 * T + 3] + [7] * ((n // 7) + 1), n)
    lens = rng.integers(1, 2 * max(int(np.sqrt(n)), 1) + 1, n + 1)
    if shape == "edges1":             # the first and the last partition are single rows
        mid = lengths_to_ids([1] + list(lens), max(n - 1, 0))
        return np.append(mid, np.full(min(n, 1), n + 7)).astype(np.int64)
    assert shape == "sqrt"
    return lengths_to_ids(list(lens), n)


def order_ids(rng, n, peers):
    pos = np.arange(n, dtype=np.int64)
    if peers == "none":
        return pos
    if peers == "all":
        return np.zeros(n, np.int64)
    flag = rng.random(n) < 0.3
    if peers == "tile_cross":
        flag[max(T - 3, 0):T + 4] = False         # one peer run over the tile edge
    return np.cumsum(flag).astype(np.int64)


def values(rng, n, kind="mixed"):
    """(int64 values, u8 nulls): extremes next to NULLs, garbage under NULLs."""
    v = rng.integers(-2**62, 2**62, n).astype(np.int64)
    if n:
        v[rng.integers(0, n, max(n // 8, 1))] = I64_MAX
        v[rng.integers(0, n, max(n // 8, 1))] = I64_MIN
    nl = (rng.random(n) < 0.35).astype(np.uint8) * 5
    return np.where(nl != 0, rng.integers(-9, 9, n), v).astype(np.int64), nl


def standard_funcs(rng, n):
    v, nl = values(rng, n)
    w = rng.integers(-2**31, 2**31, n).astype(np.int32)
    return [WinFunc(ROW_NUMBER), WinFunc(RANK), WinFunc(DENSE_RANK), WinFunc(NTILE, param0=3),
            WinFunc(SUM, v, nl), WinFunc(MIN, v, nl, mode=ROWS, lo=UNBOUNDED, hi=0),
            WinFunc(COUNT, v, nl, mode=ROWS, lo=3, hi=2), WinFunc(LEAD, w, None, PT_I32, param0=1)]


def keys_of(pid, oid):
    return [(pid.astype(np.int32), None, PT_I32)], [(oid, None, PT_I64)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_partition_shapes(engine, n, shape):
    rng = np.random.default_rng(n * 31 + SHAPES.index(shape))
    pk, ok = keys_of(part_ids(rng, n, shape), order_ids(rng, n, "runs"))
    check(engine, pk, ok, standard_funcs(rng, n), n)


def test_middle_pass_loops(engine):
    """Just over T * A rows: the scan of the tile aggregates takes a second
    sweep, and the first partition carries across it."""
    n = T * A + T + 5
    rng = np.random.default_rng(7)
    lens = [T * A + 3] + list(rng.integers(1, 200, 64))
    pk, ok = keys_of(lengths_to_ids(lens, n), order_ids(rng, n, "runs"))
    check(engine, pk, ok, standard_funcs(rng, n), n)


@pytest.mark.parametrize("peers", PEERS)
def test_peer_shapes(engine, peers):
    n = 3 * T + 17
    rng = np.random.default_rng(PEERS.index(peers))
    v, nl = values(rng, n)
    funcs = [WinFunc(RANK), WinFunc(DENSE_RANK), WinFunc(SUM, v, nl), WinFunc(COUNT, v, nl),
             WinFunc(MAX, v, nl), WinFunc(LAST_VALUE, v, nl), WinFunc(COUNT_STAR)]
    for shape in ("one", "sqrt"):
        pk, ok = keys_of(part_ids(rng, n, shape), order_ids(rng, n, peers))
        check(engine, pk, ok, funcs, n)
    pk, _ = keys_of(part_ids(rng, n, "sqrt"), order_ids(rng, n, peers))
    check(engine, pk, [], funcs, n)              # no order keys: the partition is one peer group


def multi_keys(rng, ids, count, typ, nullable):
    """`count` key columns that differ only in the last one; with `nullable`
    the last key is NULL (garbage underneath) for id % 5 == 0, next to a real 0
    for id % 5 == 1."""
    n = len(ids)
    keys = [(np.full(n, 3, DT[typ]), None, typ) for _ in range(count - 1)]
    if count:
        last = np.where(ids % 5 == 1, 0, ids + 10).astype(DT[typ])
        nl = None
        if nullable:
            nl = (ids % 5 == 0).astype(np.uint8) * 255
            last = np.where(nl != 0, rng.integers(-5, 5, n), last).astype(DT[typ])
        keys.append((last, nl, typ))
    return keys


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("typ", [PT_I32, PT_I64])
@pytest.mark.parametrize("n_part,n_order", [(1, 0), (2, 1), (3, 2), (4, 4), (1, 3), (0, 1), (0, 0)])
def test_key_counts_types_and_nulls(engine, n_part, n_order, typ, nullable):
    n = T + 1
    rng = np.random.default_rng(n_part * 5 + n_order)
    pid = part_ids(rng, n, "sqrt") if n_part else np.zeros(n, np.int64)
    # consecutive ids 5k, 5k+1: NULL and the value 0 side by side
    pk = multi_keys(rng, pid, n_part, typ, nullable)
    ok = multi_keys(rng, order_ids(rng, n, "runs"), n_order, typ, nullable)
    check(engine, pk, ok, standard_funcs(rng, n), n)


def test_extreme_key_values(engine):
    n = 600
    rng = np.random.default_rng(3)
    lut = np.array([I64_MIN, -1, 0, I64_MAX, 1 << 32, -(1 << 32)], np.int64)
    pid = np.sort(rng.integers(0, len(lut), n))
    nl = (rng.random(n) < 0.2).astype(np.uint8)
    nl = np.sort(nl)[::-1].copy()                 # the NULL partition first, over garbage
    pk = [(np.where(nl != 0, lut[rng.integers(0, 6, n)], lut[pid]), nl, PT_I64)]
    ok = [(lut[rng.integers(0, 6, n)], None, PT_I64)]
    check(engine, pk, ok, standard_funcs(rng, n), n)


def test_value_edges(engine):
    n = 2 * T + 9
    rng = np.random.default_rng(11)
    pid = lengths_to_ids([T + 100, 50, 1, 300, 40], n)
    pk, ok = keys_of(pid, order_ids(rng, n, "runs"))
    v, nl = values(rng, n)
    start = np.flatnonzero(np.append(True, pid[1:] != pid[:-1]))
    for s in start:                                # NULL-only prefixes (one longer than a tile row run)
        nl[s:s + 70] = 1
    nl[pid == 1] = 1                               # a partition whose inputs are all NULL
    only_max, only_min = pid == 3, pid == 4        # the only non-NULL value of the partition
    nl[only_max | only_min] = 1
    i, j = np.flatnonzero(only_max)[150], np.flatnonzero(only_min)[20]
    nl[i] = nl[j] = 0
    v[i], v[j] = I64_MAX, I64_MIN
    big = np.full(n, I64_MAX - 3, np.int64)        # sums that wrap again and again
    funcs = []
    for col, cn in ((v, nl), (big, None)):
        funcs += [WinFunc(SUM, col, cn), WinFunc(MIN, col, cn), WinFunc(MAX, col, cn),
                  WinFunc(SUM, col, cn, mode=ROWS, lo=5, hi=5)]
    check(engine, pk, ok, funcs, n)
    funcs = [WinFunc(fn, v, nl, mode=ROWS, lo=UNBOUNDED, hi=hi) for fn in (MIN, MAX)
             for hi in (0, 7, UNBOUNDED)] + [WinFunc(FIRST_VALUE, v, nl), WinFunc(COUNT, v, nl)]
    check(engine, pk, ok, funcs, n)


FRAMES = [(ROWS, UNBOUNDED, 0), (ROWS, UNBOUNDED, UNBOUNDED), (RANGE, UNBOUNDED, 0),
          (RANGE, UNBOUNDED, UNBOUNDED), (ROWS, 0, 0), (ROWS, 1, 0), (ROWS, 0, 1), (ROWS, 3, 2),
          (ROWS, T + 5, 0), (ROWS, 0, T + 5), (ROWS, 10**9, 10**9), (ROWS, UNBOUNDED, 2),
          (ROWS, UNBOUNDED, T + 5)]


@pytest.fixture(scope="module")
def frame_table():
    n = 4 * T + 100
    rng = np.random.default_rng(5)
    lens = [1, 3 * T + 5] + list(rng.integers(1, 90, 40))
    pk, ok = keys_of(lengths_to_ids(lens, n), order_ids(rng, n, "runs"))
    v, nl = values(rng, n)
    w = rng.integers(-2**31, 2**31, n).astype(np.int32)
    return n, pk, ok, v, nl, w


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("frame", FRAMES)
def test_frames(engine, frame_table, frame, nullable):
    n, pk, ok, v, nl, w = frame_table
    mode, lo, hi = frame
    fns = [COUNT_STAR, COUNT, SUM, FIRST_VALUE, LAST_VALUE] + ([MIN, MAX] if lo == UNBOUNDED else [])
    funcs = [WinFunc(fn, v, nl if nullable else None, mode=mode, lo=lo, hi=hi) for fn in fns]
    funcs.append(WinFunc(SUM, w, None, PT_I32, mode=mode, lo=lo, hi=hi))
    check(engine, pk, ok, funcs, n)


@pytest.mark.parametrize("fn", [LAG, LEAD])
def test_lag_lead(engine, frame_table, fn):
    n, pk, ok, v, nl, w = frame_table
    for cols in ((v, nl, PT_I64), (w, None, PT_I32)):
        funcs = [WinFunc(fn, *cols, param0=k, param1=I64_MIN + 1, has_default=d)
                 for k in (0, 1, 2, T + 1, n) for d in (False, True)]
        check(engine, pk, ok, funcs[:8], n)
        check(engine, pk, ok, funcs[8:], n)


def test_eight_in_one_call_equal_eight_calls(engine, frame_table):
    n, pk, ok, v, nl, w = frame_table
    funcs = [WinFunc(DENSE_RANK), WinFunc(NTILE, param0=1000), WinFunc(SUM, v, nl),
             WinFunc(MIN, v, nl), WinFunc(MAX, w, None, PT_I32),
             WinFunc(COUNT, v, nl, mode=ROWS, lo=2, hi=T + 5),
             WinFunc(LAG, v, nl, param0=2), WinFunc(LAST_VALUE, v, nl)]
    together = run_eval(engine, pk, ok, funcs, n)
    assert_same(together, window_ref(pk, ok, funcs, n))
    assert_same(together, [run_eval(engine, pk, ok, [f], n)[0] for f in funcs])


def test_sorted_out_against_default_order(engine):
    n = T + 77
    rng = np.random.default_rng(13)
    pk, ok = keys_of(part_ids(rng, n, "sqrt"), order_ids(rng, n, "runs"))
    funcs = standard_funcs(rng, n)
    perm = rng.permutation(n).astype(np.uint32)
    inv = np.argsort(perm)
    spread = lambda c: None if c is None else c[inv]        # order_idx = perm restores the order
    spk = [(spread(v), spread(nl), t) for v, nl, t in pk]
    sok = [(spread(v), spread(nl), t) for v, nl, t in ok]
    sf = [f.with_cols(spread(f.col), spread(f.nulls)) for f in funcs]
    ident = run_eval(engine, pk, ok, funcs, n)
    assert_same(run_eval(engine, pk, ok, funcs, n, None, True), ident)   # identity: same thing
    in_order = run_eval(engine, spk, sok, sf, n, perm, True)
    assert_same(in_order, ident)
    lined_up = run_eval(engine, spk, sok, sf, n, perm, False)
    assert_same(lined_up, [(v[inv], None if nl is None else nl[inv]) for v, nl in ident])
    assert_same(lined_up, window_ref(spk, sok, sf, n, perm, False))


def run_window(eng, pk, ok, funcs, n, sorted_out=False):
    """Engine.window over host columns; ok = [(values, nulls, type, desc, nulls_first)]."""
    host = [c for k in pk + ok for c in k[:2]] + [c for f in funcs for c in (f.col, f.nulls)]
    dev = [up(eng, a) for a in host]
    outs, perm = [], None
    try:
        it = iter(dev)
        dpk = [(next(it), next(it), k[2]) for k in pk]
        dok = [(next(it), next(it)) + tuple(k[2:]) for k in ok]
        dfuncs = [f.with_cols(next(it), next(it)) for f in funcs]
        outs = eng.window(dpk, dok, dfuncs, n, sorted_out)
        if sorted_out:
            outs, perm = outs
        res = [(pull(v, np.int64, n), None if nl is None else pull(nl, np.uint8, n))
               for v, nl in outs]
        hperm = None if perm is None else perm.d2h(np.uint32, n)
        for a, b in zip(host, dev):
            if a is not None and a.size:
                np.testing.assert_array_equal(b.d2h(a.dtype, a.size), a)
    finally:
        free_all(dev + [b for p in outs for b in p] + [perm])
    return (res, hperm) if sorted_out else res


@pytest.mark.parametrize("n", [0, 1, 5000])
def test_engine_window_sorts_with_topn(engine, n):
    rng = np.random.default_rng(n)
    p = rng.integers(0, 12, n).astype(np.int32)
    pn = (rng.random(n) < 0.1).astype(np.uint8)
    a = rng.integers(-3, 3, n).astype(np.int64)
    an = (rng.random(n) < 0.2).astype(np.uint8)
    b = rng.integers(0, 4, n).astype(np.int32)
    v, nl = values(rng, n)
    pk = [(p, pn, PT_I32)]
    ok = [(a, an, PT_I64, True, False), (b, None, PT_I32, False, True)]     # DESC NULLS LAST, ASC
    funcs = standard_funcs(rng, n) [:6] + [WinFunc(LAG, v, nl, param0=1),
                                          WinFunc(SUM, v, nl, mode=ROWS, lo=1, hi=1)]
    want_perm = sort_perm_ref(pk, [k[:3] for k in ok], [k[3:] for k in ok], n)
    keys3 = [k[:3] for k in ok]
    assert_same(run_window(engine, pk, ok, funcs, n),
                window_ref(pk, keys3, funcs, n, want_perm, False))
    got, perm = run_window(engine, pk, ok, funcs, n, True)
    if n:
        np.testing.assert_array_equal(perm, want_perm)
    assert_same(got, window_ref(pk, keys3, funcs, n, want_perm, True))


def test_ties_in_every_key_follow_row_index(engine):
    n = 3000
    pk = [(np.full(n, 4, np.int32), None, PT_I32)]
    ok = [(np.full(n, -1, np.int64), np.ones(n, np.uint8), PT_I64, True, False)]
    x = np.arange(n, dtype=np.int64) * 3
    (rn, _), (rk, _), (lag, lag_nulls) = run_window(
        engine, pk, ok, [WinFunc(ROW_NUMBER), WinFunc(RANK), WinFunc(LAG, x, param0=1)], n)
    np.testing.assert_array_equal(rn, np.arange(1, n + 1))
    np.testing.assert_array_equal(rk, np.ones(n, np.int64))
    np.testing.assert_array_equal(lag[1:], x[:-1])
    assert lag_nulls[0] == 1 and not lag_nulls[1:].any()


def test_argument_errors_leave_outputs_untouched(engine):
    eng, n = engine, 100
    idx = up(eng, np.arange(n, dtype=np.uint32))
    k32, k64, knul = eng.alloc(4 * n), eng.alloc(8 * n), eng.alloc(n)
    c64, c32, cnul = eng.alloc(8 * n), eng.alloc(4 * n), eng.alloc(n)
    for b in (k32, k64, knul, c64, c32, cnul):
        eng._lib.gpue_dbuf_memset(b._h, 0, b.nbytes)
    short8, short4, short1 = eng.alloc(8 * n - 1), eng.alloc(4 * n - 1), eng.alloc(n - 1)
    outs = [(filled(eng, 8 * n), filled(eng, n)) for _ in range(9)]
    pk = [(k32, knul, PT_I32)]
    ok = [(k64, None, PT_I64)]
    base = [WinFunc(SUM, c64, cnul), WinFunc(ROW_NUMBER), WinFunc(COUNT, c32, None, PT_I32)]
    o3 = [outs[0], (outs[1][0], None), (outs[2][0], None)]

    def call(n_rows=n, order_idx=idx, part=pk, order=ok, funcs=base, out=o3, flags=0):
        eng.window_eval(n_rows, order_idx, part, order, funcs, out, flags=flags)

    call()                                           # the baseline is legal
    for v, nl in outs[:3]:
        eng._lib.gpue_dbuf_memset(v._h, FILL, v.nbytes)
        eng._lib.gpue_dbuf_memset(nl._h, FILL, nl.nbytes)
    f0 = lambda **kw: [WinFunc(SUM, c64, cnul, **kw)] + base[1:]
    swap = lambda lst, i, item: lst[:i] + [item] + lst[i + 1:]
    big = filled(eng, 16 * n)
    front = eng.wrap_ptr_offset(big, 0, 8 * n)                # front and half share 4 n bytes
    half = eng.wrap_ptr_offset(big, 4 * n, 8 * n)
    bad = [
        dict(part=pk * 5), dict(order=ok * 5),                              # counts
        dict(funcs=[], out=[]),
        dict(funcs=[WinFunc(ROW_NUMBER)] * 9, out=[(o[0], None) for o in outs]),
        dict(part=[(k32, knul, 2)]), dict(order=[(k64, None, -1)]),         # unknown types
        dict(funcs=swap(base, 2, WinFunc(COUNT, c32, None, 7))),
        dict(funcs=swap(base, 1, WinFunc(13))), dict(funcs=swap(base, 1, WinFunc(-1))),
        dict(funcs=f0(mode=2)), dict(flags=2), dict(flags=-1),
        dict(funcs=f0(mode=ROWS, lo=-2, hi=0)), dict(funcs=f0(mode=ROWS, lo=0, hi=-2)),
        dict(funcs=f0(mode=RANGE, lo=0, hi=0)), dict(funcs=f0(mode=RANGE, lo=UNBOUNDED, hi=1)),
        dict(funcs=swap(base, 0, WinFunc(MIN, c64, cnul, mode=ROWS, lo=1, hi=0))),
        dict(funcs=swap(base, 0, WinFunc(MAX, c64, cnul, mode=ROWS, lo=0, hi=UNBOUNDED))),
        dict(funcs=swap(base, 1, WinFunc(NTILE, param0=0))),
        dict(funcs=swap(base, 1, WinFunc(LAG, c64, param0=-1))),
        dict(funcs=swap(base, 1, WinFunc(LEAD, c64, param0=-1))),
        dict(n_rows=1 << 32),
        dict(order_idx=short4),                                             # short buffers
        dict(part=[(short4, knul, PT_I32)]), dict(part=[(k32, short1, PT_I32)]),
        dict(order=[(short8, None, PT_I64)]),
        dict(funcs=swap(base, 0, WinFunc(SUM, short8, cnul))),
        dict(funcs=swap(base, 0, WinFunc(SUM, c64, short1))),
        dict(funcs=swap(base, 2, WinFunc(COUNT, short4, None, PT_I32))),
        dict(out=swap(o3, 1, (short8, None))), dict(out=swap(o3, 0, (outs[0][0], short1))),
        dict(funcs=swap(base, 0, WinFunc(SUM, None, None, nullable=True))),  # missing columns
        dict(part=[(None, None, PT_I32)]),
        dict(out=swap(o3, 1, (None, None))), dict(out=swap(o3, 0, (outs[0][0], None))),
        dict(order=[(k64, knul, PT_I64, False)]),                           # nulls for NOT NULL
        dict(funcs=swap(base, 2, WinFunc(COUNT, c32, cnul, PT_I32, nullable=False))),
        dict(out=swap(o3, 1, (outs[0][0], None))),                          # overlaps
        dict(out=[(front, outs[0][1]), (half, None), o3[2]]),
        dict(out=swap(o3, 1, (c64, None))), dict(out=swap(o3, 1, (k64, None))),
        dict(out=swap(o3, 0, (outs[0][0], outs[1][0]))),
        dict(out=swap(o3, 1, (half, None)), funcs=swap(base, 0, WinFunc(SUM, big, cnul))),
    ]
    try:
        for kw in bad:
            with pytest.raises(GpueError, match="status 2"):
                call(**kw)
        for v, nl in outs:
            assert (v.d2h(np.uint8, 8 * n) == FILL).all()
            assert (nl.d2h(np.uint8, n) == FILL).all()
        assert (big.d2h(np.uint8, 16 * n) == FILL).all()
    finally:
        free_all([idx, k32, k64, knul, c64, c32, cnul, short8, short4, short1, front, half, big] +
                 [b for p in outs for b in p])


def test_bad_order_idx_is_an_error_not_a_fault(engine):
    n = T + 10
    rng = np.random.default_rng(1)
    pk, ok = keys_of(part_ids(rng, n, "sqrt"), order_ids(rng, n, "runs"))
    funcs = standard_funcs(rng, n)
    idx = np.arange(n, dtype=np.uint32)
    idx[5], idx[T + 2] = n, 0xFFFFFFFF
    with pytest.raises(GpueError, match="order_idx"):
        run_eval(engine, pk, ok, funcs, n, idx)
    check(engine, pk, ok, funcs, n)                  # the latch is cleared: the session goes on


def test_window_sink_operator_equals_one_shot(engine):
    from starrocks_amd.pipeline import WindowSinkOperator
    n = T + 500
    rng = np.random.default_rng(17)
    p = rng.integers(0, 30, n).astype(np.int32)
    pn = (rng.random(n) < 0.1).astype(np.uint8)
    o = rng.integers(-50, 50, n).astype(np.int64)
    v, nl = values(rng, n)
    cols = [p, pn, o, v, nl]
    funcs = [WinFunc(ROW_NUMBER), WinFunc(SUM, 3, 4), WinFunc(LAG, 3, 4, param0=1),
             WinFunc(MAX, 3, 4, mode=ROWS, lo=UNBOUNDED, hi=0)]
    op = WindowSinkOperator(engine, [c.dtype for c in cols], [(0, 1, PT_I32)],
                            [(2, None, PT_I64, True, False)], funcs)
    at = 0
    for size in (1, 700, 0, 64, 3, n):
        size = min(size, n - at)
        op.push_chunk({"n": size, "cols": [up(engine, c[at:at + size]) for c in cols]})
        at += size
    assert at == n and op.need_input()
    op.set_finishing()
    assert op.is_finished()
    got_cols, got = op.result()
    for g, c in zip(got_cols, cols):
        np.testing.assert_array_equal(g, c)
    hf = [f.with_cols(None if f.col is None else cols[f.col],
                      None if f.nulls is None else cols[f.nulls]) for f in funcs]
    assert_same(got, run_window(engine, [(p, pn, PT_I32)], [(o, None, PT_I64, True, False)], hf, n))
    perm = sort_perm_ref([(p, pn, PT_I32)], [(o, None, PT_I64)], [(True, False)], n)
    assert_same(got, window_ref([(p, pn, PT_I32)], [(o, None, PT_I64)], hf, n, perm))
