"""Full sort (gpue_sort) on the GPU: multi-key ORDER BY without LIMIT, the
whole permutation exact against the numpy reference of tests/test_topn_cpu.py
(dense ranks + lexsort with the row index last). Every comparison is
np.array_equal — there are no tolerances.

Implementation edges the shapes aim at: 64-lane waves that rank by ballot,
the T = 4096-row scatter tile (each wave owns 1024 contiguous rows of it),
the 1024-block grid cap (past 1024 tiles a block loops over several), the
switch to gpue_topn's single-tile path up to SMALL = 2048 rows (the radix path
is also forced below it through GPUE_SORT_SMALL_MAX), 8-bit digits cut from
the lowest varying bit of a key, the class folded into the image or given a
pass of its own, and keys or digits on which nothing varies costing no pass."""

import numpy as np
import pytest

from starrocks_amd.engine import Engine, GpueError
from starrocks_amd.pipeline import SortSinkOperator  # noqa: F401  (fails on a tree without it)
from starrocks_amd.window import PT_I32, PT_I64, ROW_NUMBER, SUM, WinFunc, sort_perm_ref
from test_sort_cpu import SINK_CHUNKS, run_sink, sink_case
from test_topn_cpu import TYPE_CODE, topn_order

pytestmark = pytest.mark.gpu

T = Engine.SORT_TILE
CAP = Engine.SORT_MAX_BLOCKS
SMALL = Engine.SORT_SMALL_MAX
I64 = np.iinfo(np.int64)
I32 = np.iinfo(np.int32)


class Uploaded:
    """Key columns resident on the device; keys = [(values, nulls or None,
    desc, nulls_first)], most significant first."""

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

    def sort(self):
        got = self.e.sort_indices(self.desc, self.n)
        assert got.dtype == np.uint32 and len(got) == self.n
        return got

    def free(self):
        for b in self.bufs:
            b.free()


def check(engine, keys, n):
    """Sort on the device and compare the whole permutation with the reference."""
    up = Uploaded(engine, keys, n)
    try:
        got = up.sort()
    finally:
        up.free()
    assert np.array_equal(got.astype(np.int64), topn_order(keys, n)), n
    return got


@pytest.fixture
def radix_everywhere(monkeypatch):
    """No small-input switch: every size takes the radix passes."""
    monkeypatch.setenv("GPUE_SORT_SMALL_MAX", "0")


# ---- row counts -------------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7, SMALL - 1, SMALL, SMALL + 1]


def _ties_key(n):
    rng = np.random.default_rng(100 + n % 97)
    return rng.integers(-(n // 3) - 1, n // 3 + 1, max(n, 1)).astype(np.int64)


@pytest.mark.parametrize("n", sorted(set(SIZES)))
def test_row_counts_around_tile_edges(engine, n):
    check(engine, [(_ties_key(n), None, False, False)], n)


@pytest.mark.parametrize("n", sorted(s for s in set(SIZES) if s <= SMALL))
def test_row_counts_on_the_radix_path(engine, radix_everywhere, n):
    check(engine, [(_ties_key(n), None, True, False)], n)


def test_more_tiles_than_blocks(engine):
    """cap*T + 1 rows: every block loops over two tiles and the last row is alone."""
    n = CAP * T + 1
    rng = np.random.default_rng(3)
    check(engine, [(rng.integers(0, 1000, n).astype(np.int32), None, False, False)], n)


# ---- pass skipping ----------------------------------------------------------
N_SKIP = 2 * T + 77


def _two_values(dtype, lo, hi, n=N_SKIP, seed=5):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.5, np.array(lo, dtype), np.array(hi, dtype)).astype(dtype)


def test_constant_key_gives_the_identity(engine):
    for col in (np.full(N_SKIP, -12345, np.int64), np.full(N_SKIP, 7, np.int32)):
        got = check(engine, [(col, None, True, False)], N_SKIP)
        assert np.array_equal(got, np.arange(N_SKIP, dtype=np.uint32))


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("case", ["bit0", "i32_bit31", "i64_bit63", "u64_bit63",
                                  "digit_boundary", "bits_7_and_40"])
def test_keys_that_vary_in_few_bits(engine, case, desc):
    if case == "bit0":
        col = _two_values(np.int64, 0x1234_5678_0000, 0x1234_5678_0001)
    elif case == "i32_bit31":
        col = _two_values(np.int32, 0x1234, 0x1234 - 2**31)
    elif case == "i64_bit63":
        col = _two_values(np.int64, 0x1234, 0x1234 - 2**63)
    elif case == "u64_bit63":
        col = _two_values(np.uint64, 0x1234, 0x1234 + 2**63)
    elif case == "digit_boundary":
        col = _two_values(np.int32, 0x00FF, 0x0100)
    else:
        rng = np.random.default_rng(9)
        col = (np.int64(0x55_0000_0000_0000) + (rng.integers(0, 2, N_SKIP) << 7) +
               (rng.integers(0, 2, N_SKIP) << 40)).astype(np.int64)
    check(engine, [(col, None, desc, False)], N_SKIP)


def test_first_key_constant_second_decides(engine):
    rng = np.random.default_rng(17)
    a = np.full(N_SKIP, I64.min, np.int64)
    b = rng.integers(0, 2**64, N_SKIP, dtype=np.uint64)
    check(engine, [(a, None, False, False), (b, None, True, False)], N_SKIP)


# ---- extremes ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.uint64])
@pytest.mark.parametrize("desc", [False, True])
def test_extremes(engine, dtype, desc):
    n = 3 * T + 7
    rng = np.random.default_rng(13)
    if dtype == np.uint64:
        special = np.array([0, 2**63, 2**64 - 1, 1, 2**63 - 1, 2**63 + 1], np.uint64)
        body = rng.integers(0, 2**64, n, dtype=np.uint64)
    else:
        info = np.iinfo(dtype)
        special = np.array([info.min, info.max, -1, 0, 1, info.min + 1], dtype)
        body = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    pos = rng.choice(n, 60, replace=False)
    body[pos] = np.tile(special, 10)   # each extreme 10x: ties among extremes
    check(engine, [(body, None, desc, False)], n)
    only = special[:3] if dtype == np.uint64 else special[:4]   # nothing but the extremes
    check(engine, [(only[rng.integers(0, len(only), n)], None, desc, False)], n)


# ---- NULLs ------------------------------------------------------------------
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
@pytest.mark.parametrize("dtype,wide", [(np.int64, False), (np.int64, True), (np.int32, False),
                                        (np.int32, True), (np.uint64, True)])
def test_nulls_all_four_placements(engine, desc, nulls_first, dtype, wide):
    """wide: the values span the whole type, so the class has no room in the
    image and gets a pass of its own; otherwise it is folded into the top digit."""
    n = 2 * T + 301
    rng = np.random.default_rng(29)
    info = np.iinfo(dtype)
    if wide:
        vals = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        vals[:2] = [info.min, info.max]
    else:
        vals = rng.integers(0, 1000, n).astype(dtype)
    nulls = (rng.random(n) < 0.2).astype(np.uint8)
    nulls[:2] = 0
    b = rng.integers(0, 50, n).astype(np.int32)
    check(engine, [(vals, nulls, desc, nulls_first)], n)
    check(engine, [(vals, nulls, desc, nulls_first), (b, None, False, False)], n)


def test_all_null_column(engine):
    n = 2 * T + 5
    rng = np.random.default_rng(31)
    garbage = rng.integers(I32.min, I32.max, n).astype(np.int32)
    allnull = np.ones(n, np.uint8)
    got = check(engine, [(garbage, allnull, True, True)], n)
    assert np.array_equal(got, np.arange(n, dtype=np.uint32))
    b = rng.integers(0, 2**64, n, dtype=np.uint64)
    check(engine, [(garbage, allnull, True, True), (b, None, False, False)], n)


@pytest.mark.parametrize("nulls_first", [False, True])
def test_nulls_plus_one_constant_value(engine, nulls_first):
    """Only the class varies: one 2-bit pass."""
    n = 2 * T + 5
    rng = np.random.default_rng(33)
    nulls = (rng.random(n) < 0.4).astype(np.uint8)
    vals = np.full(n, -77, np.int64)
    vals[nulls != 0] = rng.integers(I64.min, I64.max, int(nulls.sum()))
    got = check(engine, [(vals, nulls, False, nulls_first)], n)
    parts = [np.flatnonzero(nulls != 0), np.flatnonzero(nulls == 0)]
    want = np.concatenate(parts if nulls_first else parts[::-1])
    assert np.array_equal(got, want.astype(np.uint32))


def test_null_rows_ignore_stored_values(engine):
    n = 2 * T + 9
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
        res = [check(engine, [(col, nulls, True, False), (b, None, False, True)], n)
               for col in (clean, dirty)]
        assert np.array_equal(res[0], res[1])


# ---- multi-key --------------------------------------------------------------
def _eight_keys(n, seed=23):
    rng = np.random.default_rng(seed)
    dts = [np.int32, np.int64, np.uint64, np.int32, np.int64, np.uint64, np.int32, np.int64]
    keys = []
    for i, dt in enumerate(dts):
        nulls = (rng.random(n) < 0.1).astype(np.uint8) if i % 3 == 0 else None
        keys.append((rng.integers(0, 4, n).astype(dt), nulls, bool(i % 2), bool(i % 4 == 0)))
    return keys


def test_multi_key_eight(engine):
    """8 low-cardinality keys of mixed types and flags: ties survive all of them."""
    n = 50_000
    check(engine, _eight_keys(n), n)


def _three_values_unique_minor(n, seed=41):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 3, n).astype(np.int32), None, True, False),
            (rng.permutation(n).astype(np.int64) - n // 2, None, False, False)]


def test_three_values_times_unique_minor_key(engine):
    n = 5 * T + 11
    check(engine, _three_values_unique_minor(n), n)


def _nullable_major(n, seed=43):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 10, n).astype(np.int64), (rng.random(n) < 0.5).astype(np.uint8),
             False, True),
            (rng.integers(0, 2**64, n, dtype=np.uint64), None, True, False)]


def test_nullable_major_key_with_plain_minor(engine):
    n = 5 * T + 11
    check(engine, _nullable_major(n), n)


# ---- stability at size ------------------------------------------------------
def test_stability_at_size(engine):
    n = 2**20 + 3
    rng = np.random.default_rng(47)
    vals = rng.integers(0, 2, n).astype(np.int32) * 1000
    up = Uploaded(engine, [(vals, None, False, False)], n)
    got = up.sort()
    up.free()
    want = np.concatenate([np.flatnonzero(vals == 0), np.flatnonzero(vals == 1000)])
    assert np.array_equal(got, want.astype(np.uint32))   # rows of each value ascend
    same = np.full(n, 1000, np.int32)
    up = Uploaded(engine, [(same, None, True, False), (same.astype(np.int64), None, False, True)],
                  n)
    got = up.sort()
    up.free()
    assert np.array_equal(got, np.arange(n, dtype=np.uint32))


# ---- the contract with gpue_topn -------------------------------------------
@pytest.mark.parametrize("shape", ["eight", "three_x_unique", "nullable_major"])
def test_bytes_equal_topn_with_limit_n(engine, shape):
    n = 300_000
    keys = {"eight": _eight_keys, "three_x_unique": _three_values_unique_minor,
            "nullable_major": _nullable_major}[shape](n)
    up = Uploaded(engine, keys, n)
    try:
        first, second = up.sort(), up.sort()
        topn = engine.topn_indices(up.desc, n, n)
    finally:
        up.free()
    assert first.tobytes() == second.tobytes()
    assert first.tobytes() == topn.tobytes()


# ---- errors -----------------------------------------------------------------
def test_argument_errors(engine):
    """Host-side checks: each raises before anything is launched, and the
    session sorts correctly afterwards."""
    col = engine.alloc(1000 * 8)
    key = (col, None, 1, False, False)
    out = engine.alloc(1000 * 4)
    with pytest.raises(GpueError):
        engine.sort_into([], 1000, out)
    with pytest.raises(GpueError):
        engine.sort_into([key] * 9, 1000, out)
    with pytest.raises(GpueError):
        engine.sort_into([(col, None, 3, False, False)], 1000, out)
    with pytest.raises(GpueError):
        engine.sort_into([(col, None, -1, False, False)], 1000, out)
    with pytest.raises(GpueError):
        engine.sort_into([key], 2**32, out)
    with pytest.raises(GpueError):   # key buffer shorter than n_rows elements
        engine.sort_into([key], 1001, out)
    nm = engine.alloc(999)
    with pytest.raises(GpueError):   # null mask shorter than n_rows
        engine.sort_into([(col, nm, 1, False, False)], 1000, out)
    small = engine.alloc(999 * 4)
    with pytest.raises(GpueError):   # output shorter than n_rows * 4 bytes
        engine.sort_into([key], 1000, small)
    with pytest.raises(GpueError):
        engine.sort_into([key], 1000, None)
    col.h2d(np.arange(1000, dtype=np.int64)[::-1].copy())
    engine.sort_into([key], 1000, out)
    assert list(out.d2h(np.uint32, 1000)) == list(range(999, -1, -1))
    engine.sort_into([key], 0, None)     # zero rows: nothing to write
    for b in (col, out, nm, small):
        b.free()


# ---- gather_u8 --------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65, 100_003])
def test_gather_u8(engine, n):
    rng = np.random.default_rng(n)
    src = rng.integers(0, 256, max(n, 1)).astype(np.uint8)
    perm = rng.permutation(max(n, 1)).astype(np.uint32)
    d_src, d_idx, d_out = (engine.alloc(max(n, 1)), engine.alloc(max(n, 1) * 4),
                           engine.alloc(max(n, 1)))
    d_src.h2d(src)
    d_idx.h2d(perm)
    engine.gather_u8(d_src, d_idx, n, d_out)
    if n:
        assert np.array_equal(d_out.d2h(np.uint8, n), src[perm[:n]])
    if n > 1:   # the siblings' argument checks: short output, short index
        with pytest.raises(GpueError):
            engine.gather_u8(d_src, d_idx, n + 1, d_out)
        with pytest.raises(GpueError):
            engine.gather_u8(d_src, d_src, n, d_out)
    for b in (d_src, d_idx, d_out):
        b.free()


# ---- Engine.window sorts with gpue_sort ------------------------------------
def test_engine_window_permutation(engine):
    n = 50_000
    rng = np.random.default_rng(53)
    p = rng.integers(0, 300, n).astype(np.int32)
    pn = (rng.random(n) < 0.1).astype(np.uint8)
    o = rng.integers(-1000, 1000, n).astype(np.int64)
    v = rng.integers(-100, 100, n).astype(np.int64)
    bufs = []

    def dev(arr):
        bufs.append(engine.alloc(arr.nbytes))
        bufs[-1].h2d(arr)
        return bufs[-1]

    try:
        outs, perm = engine.window([(dev(p), dev(pn), PT_I32)],
                                   [(dev(o), None, PT_I64, True, False)],
                                   [WinFunc(ROW_NUMBER), WinFunc(SUM, dev(v), None)], n,
                                   sorted_out=True)
        bufs += [b for pair in outs for b in pair if b is not None] + [perm]
        got = perm.d2h(np.uint32, n)
    finally:
        for b in bufs:
            b.free()
    want = sort_perm_ref([(p, pn, PT_I32)], [(o, None, PT_I64)], [(True, False)], n)
    assert np.array_equal(got, want)


# ---- SortSinkOperator on the device ----------------------------------------
def test_operator_chunked_equals_single_call(engine):
    cols, ref = sink_case()
    sink, out = run_sink(engine, cols, SINK_CHUNKS)
    assert sink.rows == len(ref)
    assert np.array_equal(out[3].astype(np.int64), ref)
    for got, col in zip(out, cols):
        assert got.dtype == col.dtype and np.array_equal(got, col[ref])
    a, an, b = cols[0], cols[1], cols[2]
    single = check(engine, [(a, an, True, True), (b, None, False, False)], len(ref))
    assert np.array_equal(out[3], single)
