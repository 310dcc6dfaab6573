"""The general hash join (gpue_hash_join_*, gpue_gather_outer) on the GPU,
against hashjoin.hash_join_ref — not the oracle, not the old join entries.

Pinned per probe: the exact pair multiset (for LEFT_SEMI the probe-row set
plus that each reported build row truly matches), out_probe_idx
non-decreasing, the count-only call agreeing with the emit call, and
emit_build exact and ascending for both the marked and the unmarked rows.

The matrix draws keys as tests/test_join_probe_matrix.py does: 0..50 so chains
are long, probe keys below the build minimum and above its maximum, and with
two or more build rows one build key no probe row has. Wherever both sides
have at least two rows the reference result is first checked to hold a
matched pair, an unmatched probe row and an unmatched build row; a one-row
side cannot be both matched and unmatched, so those cases match their one
row (the other outcome is covered by every larger size).
"""

import ctypes
import functools

import numpy as np
import pytest

from starrocks_amd import hashjoin as hj
from starrocks_amd.engine import GpueError
from starrocks_amd.hashjoin import (INNER, LEFT_ANTI, LEFT_OUTER, LEFT_SEMI, MARK_BUILD,
                                    MARK_ONLY, NO_ROW, NULL_AWARE_LEFT_ANTI, PT_I32, PT_I64)

pytestmark = pytest.mark.gpu

N_BUILD = (0, 1, 37, 300, 5000)
N_PROBE = (0, 1, 65, 257, 1000)
ABOVE = 99  # a probe-only key above every build key
I64_MIN = -(1 << 63)
BAD_ARG = r"^gpue status 2: bad argument"


def matrix_keys(n_build, n_probe):
    """(build keys, probe keys) as int32 columns without NULLs. Probe row 0
    matches build row 0; with two or more build rows the last one's key never
    appears in the probe."""
    bk = np.random.default_rng(n_build).integers(0, 51, n_build).astype(np.int32)
    rng = np.random.default_rng(100 * n_build + n_probe + 1)
    if n_build >= 2:
        bk[0] = 0
        if bk[-1] == 0:
            bk[-1] = 50
    pk = rng.integers(-5, 57, n_probe).astype(np.int32)
    if n_probe >= 1 and n_build >= 1:
        pk[0] = bk[0]
    if n_probe >= 3:
        pk[1], pk[2] = -3, 57
    if n_build >= 2:
        pk[pk == bk[-1]] = ABOVE
    return [(bk, None, PT_I32)], [(pk, None, PT_I32)]


@functools.lru_cache(maxsize=None)
def matrix_ref(n_build, n_probe, mode):
    """The reference of one matrix cell, computed once: (pairs, matched)."""
    bk, pk = matrix_keys(n_build, n_probe)
    pairs, matched = hj.hash_join_ref(bk, pk, None, mode)
    pairs.setflags(write=False)
    matched.setflags(write=False)
    return pairs, matched


def assert_not_vacuous(n_build, n_probe):
    pairs, matched = matrix_ref(n_build, n_probe, LEFT_OUTER)
    if n_build >= 1 and n_probe >= 1:
        assert np.any(pairs[:, 1] != NO_ROW), "no matched pair"
    if n_build >= 2 and n_probe >= 2:
        assert np.any(pairs[:, 1] == NO_ROW), "no unmatched probe row"
        assert not matched.all(), "no unmatched build row"


class _Dev:
    """Device buffers and tables of one case, freed together."""

    def __init__(self, engine):
        self.engine, self.bufs, self.tables = engine, [], []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        b = self.engine.alloc(max(arr.nbytes, 8))
        if arr.nbytes:
            b.h2d(arr)
        self.bufs.append(b)
        return b

    def out(self, count, width=4):
        b = self.engine.alloc(max(count, 1) * width)
        self.bufs.append(b)
        return b

    def cols(self, keys):
        """[(values, nulls or None, type)] -> [(DBuf, DBuf or None)]"""
        return [(self.put(v), None if nl is None else self.put(nl)) for v, nl, _ in keys]

    def table(self, build_keys, probe_keys, null_safe=None, capacity_hint=0, push=True):
        spec = hj.HashJoinSpec.of(build_keys, probe_keys, null_safe)
        t = self.engine.hash_join_create(spec.build_types, spec.probe_types, spec.key_nullable,
                                         spec.key_null_safe, capacity_hint)
        self.tables.append(t)
        if push:
            self.engine.hash_join_build_push(t, self.cols(build_keys), len(build_keys[0][0]))
        return t

    def close(self):
        for t in self.tables:
            self.engine.hash_join_destroy(t)
        for b in self.bufs:
            b.free()


@pytest.fixture
def dev(engine):
    d = _Dev(engine)
    yield d
    d.close()


def pull(buf, dtype, n):
    return np.empty(0, dtype) if n == 0 else buf.d2h(dtype, n)


def raw_probe(dev, t, pcols, n, mode, flags=0):
    """count-only call, then the emit call into exact-size outputs"""
    e = dev.engine
    cnt = e.hash_join_probe(t, pcols, n, mode, flags)
    op, ob = dev.out(cnt), dev.out(cnt)
    assert e.hash_join_probe(t, pcols, n, mode, flags, op, ob) == cnt, "count-only call"
    p, b = pull(op, np.uint32, cnt), pull(ob, np.uint32, cnt)
    assert np.all(np.diff(p.astype(np.int64)) >= 0), "out_probe_idx decreases"
    return p, b


def check_pairs(p, b, mode, ref_pairs):
    if mode == LEFT_SEMI:  # the reference lists every true match of a row
        assert np.array_equal(p, np.unique(ref_pairs[:, 0]))
        allowed = set(map(tuple, ref_pairs.tolist()))
        assert all(pair in allowed for pair in zip(p.tolist(), b.tolist()))
    else:
        assert np.array_equal(hj.sort_pairs(p, b), ref_pairs)


def check_marks(dev, t, matched):
    e = dev.engine
    for m in (1, 0):
        want = np.nonzero(matched if m else ~matched)[0]
        cnt = e.hash_join_emit_build(t, m)
        assert cnt == len(want), "count-only call"
        out = dev.out(cnt)
        assert e.hash_join_emit_build(t, m, out, cnt) == cnt
        assert np.array_equal(pull(out, np.uint32, cnt), want)


def check_all_modes(dev, t, build_keys, probe_keys, null_safe, modes):
    n = len(probe_keys[0][0])
    pcols = dev.cols(probe_keys)
    for mode in modes:
        ref_pairs, matched = hj.hash_join_ref(build_keys, probe_keys, null_safe, mode)
        dev.engine.hash_join_reset_marks(t)
        p, b = raw_probe(dev, t, pcols, n, mode, MARK_BUILD)
        check_pairs(p, b, mode, ref_pairs)
        check_marks(dev, t, matched)


@pytest.mark.parametrize("n_build", N_BUILD)
@pytest.mark.parametrize("how", sorted(hj.HOWS))
def test_matrix(engine, dev, how, n_build):
    """Every join type x build size, each over every probe size, through the
    raw entries (one table from the smallest capacity_hint) and through
    Engine.hash_join."""
    mode, flags, tail = hj.plan(how)
    bk, _ = matrix_keys(n_build, 0)
    t = dev.table(bk, bk, capacity_hint=0)
    assert engine.hash_join_build_rows(t) == n_build
    stats = engine.hash_join_stats(t)
    assert stats["distinct"] == len(np.unique(bk[0][0]))
    if n_build == 5000:  # 16 slots to start with: 5000 rows force the array to double
        assert stats["doublings"] >= 2 and stats["capacity"] >= 5000 * 3 // 2
    for n_probe in N_PROBE:
        assert_not_vacuous(n_build, n_probe)
        _, pk = matrix_keys(n_build, n_probe)
        ref_pairs, matched = matrix_ref(n_build, n_probe, mode)
        pcols = dev.cols(pk)
        engine.hash_join_reset_marks(t)
        p, b = raw_probe(dev, t, pcols, n_probe, mode, flags)
        check_pairs(p, b, mode, ref_pairs)
        if tail is not None:
            check_marks(dev, t, matched)
        # the one-shot form
        tup = lambda cols, keys: [(v, nl, k[2], len(k[0])) for (v, nl), k in zip(cols, keys)]
        op, ob, n = engine.hash_join(tup(dev.cols(bk), bk), tup(pcols, pk), how)
        dev.bufs += [op, ob]
        gp, gb = pull(op, np.uint32, n), pull(ob, np.uint32, n)
        if how == "left_semi":
            check_pairs(gp, gb, mode, ref_pairs)
        else:
            want = hj.hash_join_how_ref(bk, pk, how)
            assert np.array_equal(hj.sort_pairs(gp, gb), want)
            if tail is not None:  # the tail follows the probe's pairs, ascending
                m = int(np.sum(gp == NO_ROW))
                assert np.all(gp[n - m:] == NO_ROW) and np.all(np.diff(gb[n - m:].astype(np.int64)) > 0)


# key shapes: (build type, probe type) per key
SHAPES = {
    1: [(PT_I64, PT_I64)],
    2: [(PT_I32, PT_I64), (PT_I64, PT_I32)],
    3: [(PT_I64, PT_I64), (PT_I32, PT_I64), (PT_I32, PT_I32)],
    4: [(PT_I32, PT_I64), (PT_I64, PT_I32), (PT_I64, PT_I64), (PT_I32, PT_I32)],
}
NULL_CFGS = ("none", "plain", "null_safe", "mixed")


def shape_side(rng, n, types, other_types, with_nulls, fixed):
    """One side's key columns. Values come from a domain of extremes: ~0, 0
    and INT64_MIN on an int64 key facing an int64 key, and on an int64 key
    facing an int32 key also 2^32-1 and 2^32, which must not meet -1 and 0.
    Rows listed in `fixed` (value or None per key) come first. NULL cells hold
    garbage that differs from row to row."""
    cols = []
    for k, (t, ot) in enumerate(zip(types, other_types)):
        dom = [-1, 0, 7]
        if t == PT_I64:
            dom += [I64_MIN] if ot == PT_I64 else [0xFFFFFFFF, 1 << 32]
        dt = np.int64 if t == PT_I64 else np.int32
        v = rng.choice(np.array(dom, np.int64), n)
        nl = (rng.random(n) < 0.2) if with_nulls else np.zeros(n, bool)
        for r, row in enumerate(fixed):
            v[r], nl[r] = (0, True) if row[k] is None else (row[k], False)
        v = np.where(nl, rng.integers(-1000, 1000, n), v).astype(dt)
        cols.append((v, nl.astype(np.uint8) if with_nulls else None, t))
    return cols


@pytest.mark.parametrize("cfg", NULL_CFGS)
@pytest.mark.parametrize("n_keys", (1, 2, 3, 4))
def test_key_shapes(dev, n_keys, cfg):
    """1..4 keys, int32 against int64 both ways, the extreme values, tuples
    that differ only in the last key or only in a null flag (value 0 against
    NULL, whose cell is canonically 0), garbage under NULLs, and per-key mixes
    of null-safe and plain equality."""
    rng = np.random.default_rng(50 + 4 * n_keys + NULL_CFGS.index(cfg))
    bt = [s[0] for s in SHAPES[n_keys]]
    pt = [s[1] for s in SHAPES[n_keys]]
    nulls = cfg != "none"
    ns = {"none": None, "plain": None, "null_safe": [True] * n_keys,
          "mixed": [k % 2 == 0 for k in range(n_keys)]}[cfg]
    ones = [7] * (n_keys - 1)
    fixed = [ones + [7], ones + [-1], ones + [0]] + ([ones + [None]] if nulls else [])
    if nulls and n_keys > 1:
        fixed.append([None] + ones)
    build = shape_side(rng, 300, bt, pt, nulls, fixed)
    probe = shape_side(rng, 257, pt, bt, nulls, fixed)
    build[0][0][-1], probe[0][0][-1] = 3, 4  # a build-only and a probe-only value
    if nulls:
        build[0][1][-1] = probe[0][1][-1] = 0
    _, matched = hj.hash_join_ref(build, probe, ns, INNER)
    assert matched.any() and not matched.all(), "vacuous case"
    t = dev.table(build, probe, ns)
    check_all_modes(dev, t, build, probe, ns, (INNER, LEFT_SEMI, LEFT_ANTI, LEFT_OUTER, MARK_ONLY))


def test_multi_push_equals_one_push(engine, dev):
    """100, then 0, then 4000 rows give the table one push of the same rows
    gives; the second push re-inserts the first one's slots into a grown
    array. (build_push does not work in sub-batches.)"""
    rng = np.random.default_rng(5)
    mk = lambda n: [(rng.integers(0, 700, n).astype(np.int32), None, PT_I32),
                    (rng.integers(0, 3, n).astype(np.int64), (rng.random(n) < 0.1).astype(np.uint8),
                     PT_I64)]
    build = mk(4100)
    probe = mk(1000)
    t = dev.table(build, probe, [False, True], push=False)
    for lo, hi in ((0, 100), (100, 100), (100, 4100)):
        part = [(v[lo:hi], None if nl is None else nl[lo:hi], ty) for v, nl, ty in build]
        engine.hash_join_build_push(t, dev.cols(part), hi - lo)
    assert engine.hash_join_build_rows(t) == 4100
    stats = engine.hash_join_stats(t)
    assert stats["rehashes"] >= 1 and stats["doublings"] >= 2
    one = dev.table(build, probe, [False, True])
    assert engine.hash_join_stats(one)["distinct"] == stats["distinct"]
    check_all_modes(dev, t, build, probe, [False, True], (INNER, LEFT_SEMI, LEFT_OUTER))
    check_all_modes(dev, one, build, probe, [False, True], (INNER,))


def test_three_growing_pushes(engine, dev):
    """37, 300, then 5000 rows from the smallest capacity_hint: two re-insert
    passes over a non-empty table."""
    bk, pk = matrix_keys(5337, 1000)
    t = dev.table(bk, pk, push=False)
    for lo, hi in ((0, 37), (37, 337), (337, 5337)):
        engine.hash_join_build_push(t, dev.cols([(bk[0][0][lo:hi], None, PT_I32)]), hi - lo)
    assert engine.hash_join_stats(t)["rehashes"] >= 2
    check_all_modes(dev, t, bk, pk, None, (INNER, LEFT_ANTI))


def test_skew(engine, dev):
    """One key with 3000 build duplicates probed by 500 rows: 1.5 M pairs."""
    bk = np.full(3001, 9, np.int64)
    bk[3000] = 4  # one build row nothing matches
    pk = np.full(501, 9, np.int32)
    pk[500] = 5
    build, probe = [(bk, None, PT_I64)], [(pk, None, PT_I32)]
    t = dev.table(build, probe)
    pcols = dev.cols(probe)
    assert engine.hash_join_stats(t)["distinct"] == 2
    p, b = raw_probe(dev, t, pcols, 501, INNER, MARK_BUILD)
    assert len(p) == 1_500_000
    assert np.array_equal(p, np.repeat(np.arange(500, dtype=np.uint32), 3000))
    assert np.array_equal(np.sort(b.reshape(500, 3000), axis=1),
                          np.broadcast_to(np.arange(3000, dtype=np.uint32), (500, 3000)))
    matched = np.arange(3001) < 3000
    check_marks(dev, t, matched)
    engine.hash_join_reset_marks(t)
    p, b = raw_probe(dev, t, pcols, 501, LEFT_SEMI)
    assert np.array_equal(p, np.arange(500)) and np.all(b < 3000)
    check_marks(dev, t, np.zeros(3001, bool))  # no MARK_BUILD, no marks
    assert engine.hash_join_probe(t, pcols, 501, MARK_ONLY) == 0
    check_marks(dev, t, matched)


def test_marks_across_calls(engine, dev):
    """Three probe chunks with MARK_BUILD mark what one probe of their
    concatenation marks; reset_marks clears; a build_push between probes
    keeps the marks and its rows join the later chunks."""
    bk, pk = matrix_keys(300, 1000)
    pk = [(pk[0][0].copy(), None, PT_I32)]
    pk[0][0][999] = -3
    # -3 is probed before and after these rows arrive, 57 only before, 60 never
    more = [(np.array([-3, 60, 57], np.int32), None, PT_I32)]
    t = dev.table(bk, pk)
    chunks = [(0, 400), (400, 401), (401, 1000)]
    got = np.zeros(303, bool)
    for c, (lo, hi) in enumerate(chunks):
        part = [(pk[0][0][lo:hi], None, PT_I32)]
        if c == 2:
            engine.hash_join_build_push(t, dev.cols(more), 3)
        raw_probe(dev, t, dev.cols(part), hi - lo, INNER, MARK_BUILD)
        built = [(np.concatenate([bk[0][0], more[0][0]]) if c == 2 else bk[0][0], None, PT_I32)]
        _, m = hj.hash_join_ref(built, part, None, INNER)
        got[:len(m)] |= m
        check_marks(dev, t, got[:len(m)])
    assert got[:300].any() and not got[:300].all() and got[300:].tolist() == [True, False, False]
    engine.hash_join_reset_marks(t)
    check_marks(dev, t, np.zeros(303, bool))
    both = [(np.concatenate([bk[0][0], more[0][0]]), None, PT_I32)]
    raw_probe(dev, t, dev.cols(pk), 1000, LEFT_OUTER, MARK_BUILD)
    _, whole = hj.hash_join_ref(both, pk, None, LEFT_OUTER)
    check_marks(dev, t, whole)
    assert whole[300] and whole[302] and not whole[301]


def test_null_aware_left_anti(engine, dev):
    pk = [(np.array([1, 2, 0, 7], np.int32), np.array([0, 0, 1, 0], np.uint8), PT_I32)]
    for bvals, bnulls in (([], []), ([1, 5], [0, 1]), ([1, 5], [0, 0])):
        bk = [(np.array(bvals, np.int64), np.array(bnulls, np.uint8), PT_I64)]
        t = dev.table(bk, pk)
        ref, _ = hj.hash_join_ref(bk, pk, None, NULL_AWARE_LEFT_ANTI)
        p, b = raw_probe(dev, t, dev.cols(pk), 4, NULL_AWARE_LEFT_ANTI)
        assert np.array_equal(hj.sort_pairs(p, b), ref)
    assert [len(hj.hash_join_ref([(np.array(v, np.int64), np.array(n, np.uint8), PT_I64)], pk,
                                 None, NULL_AWARE_LEFT_ANTI)[0])
            for v, n in (([], []), ([1, 5], [0, 1]), ([1, 5], [0, 0]))] == [4, 0, 2]
    two = [(np.zeros(4, np.int32), None, PT_I32)] * 2
    t2 = dev.table(two, two)
    with pytest.raises(GpueError, match=BAD_ARG):
        engine.hash_join_probe(t2, dev.cols(two), 4, NULL_AWARE_LEFT_ANTI)
    ts = dev.table(pk, pk, [True])
    with pytest.raises(GpueError, match=BAD_ARG):
        engine.hash_join_probe(ts, dev.cols(pk), 4, NULL_AWARE_LEFT_ANTI)


@pytest.mark.parametrize("with_in_nulls", (False, True))
@pytest.mark.parametrize("dtype", (np.uint8, np.int32, np.int64))
def test_gather_outer(engine, dev, dtype, with_in_nulls):
    rng = np.random.default_rng(3)
    rows, n = 1000, 2500  # more than one block; n is no multiple of the block
    vals = rng.integers(0, 200, rows).astype(dtype)
    nulls = (rng.random(rows) < 0.3).astype(np.uint8) if with_in_nulls else None
    idx = rng.integers(0, rows, n).astype(np.uint32)
    idx[rng.random(n) < 0.2] = NO_ROW
    idx[0], idx[-1] = NO_ROW, rows - 1
    w = np.dtype(dtype).itemsize
    d_in, d_nl = dev.put(vals), None if nulls is None else dev.put(nulls)
    out, onl = dev.out(n, w), dev.out(n, 1)
    engine.gather_outer(d_in, d_nl, rows, w, dev.put(idx), n, out, onl)
    want, want_nl = hj.gather_outer_ref(vals, nulls, idx)
    assert np.array_equal(out.d2h(dtype, n), want)
    assert np.array_equal(onl.d2h(np.uint8, n), want_nl)
    if not with_in_nulls:  # no NO_ROW, no in_nulls: out_nulls may be left out
        inner = np.where(idx == NO_ROW, 5, idx).astype(np.uint32)
        engine.gather_outer(d_in, None, rows, w, dev.put(inner), n, out)
        assert np.array_equal(out.d2h(dtype, n), vals[inner])


def test_gather_outer_errors(engine, dev):
    """The defined error returns: an index >= in_rows and a NO_ROW without
    out_nulls are reported after the kernel, which never dereferences them;
    the entry works again afterwards."""
    vals = np.arange(100, dtype=np.int64)
    d_in, out, onl = dev.put(vals), dev.out(10, 8), dev.out(10, 1)
    good = np.arange(10, dtype=np.uint32)
    for bad_at, bad in ((3, 100), (9, 0xFFFFFFFE), (0, 1 << 31)):
        idx = good.copy()
        idx[bad_at] = bad
        with pytest.raises(GpueError, match=r"^gpue status 2: gather_outer: idx holds an index"):
            engine.gather_outer(d_in, None, 100, 8, dev.put(idx), 10, out, onl)
    idx = good.copy()
    idx[4] = NO_ROW
    with pytest.raises(GpueError, match=r"^gpue status 2: gather_outer: idx holds NO_ROW"):
        engine.gather_outer(d_in, None, 100, 8, dev.put(idx), 10, out)
    engine.gather_outer(d_in, None, 100, 8, dev.put(idx), 10, out, onl)
    assert out.d2h(np.int64, 10).tolist() == [0, 1, 2, 3, 0, 5, 6, 7, 8, 9]
    d_idx = dev.put(good)
    for kw in (dict(width=2), dict(in_rows=101), dict(n=11), dict(out=dev.out(9, 8)),
               dict(onl=dev.out(9, 1)), dict(out=d_in), dict(nl=dev.out(99, 1)),
               dict(nl=dev.out(100, 1), onl=None), dict(n=1 << 32)):
        a = dict(nl=None, in_rows=100, width=8, n=10, out=out, onl=onl)
        a.update(kw)
        with pytest.raises(GpueError, match=BAD_ARG):
            engine.gather_outer(d_in, a["nl"], a["in_rows"], a["width"], d_idx, a["n"], a["out"],
                                a["onl"])


def test_bad_arguments(engine, dev):
    lib, h = engine._lib, engine._h
    i32 = lambda xs: np.array(xs, np.int32).ctypes.data_as(ctypes.c_void_p)
    out = ctypes.c_void_p()
    for types, n_keys in (([0], 0), ([0] * 5, 5), ([2], 1), ([-1], 1)):
        assert lib.gpue_hash_join_create(h, i32(types), i32([0] * 5), i32([0] * 5), i32([0] * 5),
                                         n_keys, 0, ctypes.byref(out)) == 2
        assert lib.gpue_hash_join_create(h, i32([0] * 5), i32(types), i32([0] * 5), i32([0] * 5),
                                         n_keys, 0, ctypes.byref(out)) == 2
    keys = [(np.arange(10, dtype=np.int32), None, PT_I32),
            (np.arange(10, dtype=np.int64), np.zeros(10, np.uint8), PT_I64)]
    t = dev.table(keys, keys)
    v0, (v1, n1) = dev.put(keys[0][0]), dev.cols(keys[1:])[0]
    short4, short8, short1 = dev.out(9, 4), dev.out(9, 8), dev.out(9, 1)
    for cols, n in (([(v0, None), (v1, n1)], 1 << 32),      # n_rows >= 2^32
                    ([(short4, None), (v1, n1)], 10),       # short key column
                    ([(v0, None), (short8, n1)], 10),
                    ([(v0, None), (v1, short1)], 10),       # short null column
                    ([(None, None), (v1, n1)], 10),         # missing column
                    ([(v0, n1), (v1, None)], 10)):          # null buffer for a NOT NULL key
        with pytest.raises(GpueError, match=BAD_ARG):
            engine.hash_join_build_push(t, cols, n)
        with pytest.raises(GpueError, match=BAD_ARG):
            engine.hash_join_probe(t, cols, n, INNER)
    assert engine.hash_join_build_rows(t) == 10
    ok = [(v0, None), (v1, n1)]
    for mode, flags in ((-1, 0), (6, 0), (INNER, 2), (INNER, -1)):
        with pytest.raises(GpueError, match=BAD_ARG):
            engine.hash_join_probe(t, ok, 10, mode, flags)
    op, ob = dev.out(10), dev.out(10)
    with pytest.raises(GpueError, match=BAD_ARG):  # one output only
        engine.hash_join_probe(t, ok, 10, INNER, 0, op, None)
    with pytest.raises(GpueError, match=BAD_ARG):  # outputs overlap
        engine.hash_join_probe(t, ok, 10, INNER, 0, op, op)
    with pytest.raises(GpueError, match=BAD_ARG):  # an output over an input
        engine.hash_join_probe(t, ok, 10, INNER, 0, v0, ob)
    assert engine.hash_join_probe(t, ok, 10, INNER, 0, op, ob) == 10
    for matched, buf, max_out in ((2, None, 0), (-1, None, 0), (1, None, 1 << 32),
                                  (0, short4, 10)):
        with pytest.raises(GpueError, match=BAD_ARG):
            engine.hash_join_emit_build(t, matched, buf, max_out)
    # more rows than max_out: the true count comes back, nothing is written
    ob.h2d(np.full(10, 77, np.uint32))
    cnt = ctypes.c_uint64()
    assert lib.gpue_hash_join_emit_build(h, t._h, 0, ob._h, 4, ctypes.byref(cnt)) == 2
    assert cnt.value == 10 and np.all(ob.d2h(np.uint32, 10) == 77)
    # n_rows == 0 is fine everywhere
    engine.hash_join_build_push(t, ok, 0)
    assert engine.hash_join_probe(t, ok, 0, LEFT_OUTER, 0, op, ob) == 0


def test_undersized_output_frees_scratch(engine, dev):
    """Output buffers too small for the pair count: GPUE_ERR_ARG, and every
    such return frees the probe's scratch. 1 M probe rows make one leaked
    array 4 MB; 300 leaking calls would lose over 1 GB."""
    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert engine._lib.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    n, scratch = 1_000_000, 4_000_000
    bk, _ = matrix_keys(37, 0)
    pk = [(np.random.default_rng(22).integers(0, 51, n).astype(np.int32), None, PT_I32)]
    t = dev.table(bk, pk)
    pcols = dev.cols(pk)
    small_p, small_b = dev.out(1), dev.out(1)
    assert engine.hash_join_probe(t, pcols, n, LEFT_OUTER) >= n

    def undersized_call():
        with pytest.raises(GpueError, match=BAD_ARG):
            engine.hash_join_probe(t, pcols, n, LEFT_OUTER, 0, small_p, small_b)

    undersized_call()  # warm: kernel code objects
    free_before = free_bytes()
    for _ in range(300):
        undersized_call()
    free_after = free_bytes()
    # one-sided: only lost memory is a leak (other processes share the device)
    assert free_before - free_after < scratch, (free_before, free_after)
