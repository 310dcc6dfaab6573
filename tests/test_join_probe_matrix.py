"""Generic hash-join probe matrix: every table shape x join mode x the sizes
that cross a wave, a block and the scan tile, through the Engine API, against
a brute-force dict join written here (not the oracle, not the engine).

Per LEFT mode the contract pinned is: the exact multiset of (probe, build)
pairs (for SEMI the probe-row set plus key equality — which chain entry SEMI
reports depends on build scatter order), out_probe non-decreasing, build
index 0 on ANTI / unmatched OUTER rows, and the count-only call agreeing with
the emit call. RIGHT semi/anti pin the set of build rows. Mode 6 is
NULL_AWARE_LEFT_ANTI: ANTI with null probe rows dropped.

Keys are drawn from 0..50 so chains are long; every build of two or more rows
holds one key no probe row has (the 1-row build is matched instead); probes carry keys below the build minimum and above its
maximum. Build rows are 1-based (row 0 is the sentinel).

The shape x mode x size cases pin behaviour that predates the unified probe
path: they pass unchanged on the commit before it. The last test covers the
scratch leak on the undersized-output error return, which that commit had.
"""

import ctypes

import numpy as np
import pytest

from starrocks_amd.engine import GpueError
from test_asof import brute_force as asof_brute_force

pytestmark = pytest.mark.gpu

N_BUILD = (1, 37, 300)
N_PROBE = (0, 1, 65, 257, 1000)
INT_SHAPES = ("rd", "dense", "lc", "bc")
LEFT_SHAPES = INT_SHAPES + ("bc_nulls", "u64", "u128", "vc", "vc_nulls")
RIGHT_SHAPES = INT_SHAPES + ("vc",)
ABOVE = 99  # a probe-only key above every build key


def _keys(n_build, n_probe, seed):
    """(build keys [0]=sentinel, probe keys) as int64. Probe row 0 matches
    build row 1; with two or more build rows the last one's key never appears
    in the probe."""
    rng = np.random.default_rng(seed)
    bk = np.concatenate([[0], rng.integers(0, 51, n_build)]).astype(np.int64)
    if n_build >= 2:
        bk[1] = 0  # key 0 is the empty string on the varchar shapes
        if bk[n_build] == 0:
            bk[n_build] = 50
    pk = rng.integers(-5, 57, n_probe).astype(np.int64)
    if n_probe >= 1:
        pk[0] = bk[1]
    if n_probe >= 3:
        pk[1], pk[2] = -3, 57
    if n_build >= 2:  # a 1-row build cannot both match and hold an unprobed key
        pk[pk == bk[n_build]] = ABOVE
    return bk, pk


def _vc_string(k):
    """Distinct byte string per key, lengths 0..12; key 0 is the empty string."""
    j = int(k) if k >= 0 else 100 - int(k)
    return b"" if j == 0 else bytes([j]) + b"x" * (j % 12)


def _vc_cols(keys):
    rows = [_vc_string(k) for k in keys]
    offsets = np.zeros(len(rows) + 1, np.uint32)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    data = np.frombuffer(b"".join(rows) + b"\0", np.uint8).copy()  # never 0 bytes
    return data, offsets


def _u64(keys):
    return (keys.astype(np.uint64) * np.uint64(0x100000001)) ^ np.uint64(0xA5A5 << 40)


def _u128(keys):
    out = np.empty((len(keys), 2), np.uint64)
    out[:, 0] = _u64(keys)
    out[:, 1] = ~keys.astype(np.uint64)
    return out


class _Dev:
    """Device buffers of one case, freed together."""

    def __init__(self, engine):
        self.engine, self.bufs, self.tables = engine, [], []

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        b = self.engine.alloc(max(arr.nbytes, 4))
        if arr.nbytes:
            b.h2d(arr)
        self.bufs.append(b)
        return b

    def out(self, count):
        b = self.engine.alloc(max(count, 1) * 4)
        self.bufs.append(b)
        return b

    def table(self, t):
        self.tables.append(t)
        return t

    def close(self):
        for t in self.tables:
            t.destroy()
        for b in self.bufs:
            b.free()


def _build_and_probe(dev, shape, bk, pk, pnulls):
    """Build `shape`'s table over bk and return probe(mode, out_p, out_b) and,
    for the RIGHT shapes, right(anti, out)."""
    e, nb, n = dev.engine, len(bk) - 1, len(pk)
    if shape in INT_SHAPES:
        build = {"rd": e.join_build_range_direct, "dense": e.join_build_dense_range_direct,
                 "lc": e.join_build_linear_chained, "bc": e.join_build_bucket_chained}[shape]
        t = dev.table(build(dev.put(bk.astype(np.int32)), nb))
        d_pk = dev.put(pk.astype(np.int32))
        return (lambda m, op=None, ob=None: e.join_probe_emit_mode(t, d_pk, n, m, op, ob),
                lambda anti, ob=None: e.join_probe_right(t, d_pk, n, anti, ob))
    if shape == "bc_nulls":
        bnulls = np.zeros(nb + 1, np.uint8)
        t = dev.table(e.join_build_bucket_chained_nulls(
            dev.put(bk.astype(np.int32)), dev.put(bnulls), nb))
        d_pk, d_pn = dev.put(pk.astype(np.int32)), dev.put(pnulls)
        return (lambda m, op=None, ob=None:
                e.join_probe_emit_nulls(t, d_pk, d_pn, n, m, op, ob)), None
    if shape == "u64":
        t = dev.table(e.join_build_bucket_chained_u64(dev.put(_u64(bk)), nb))
        d_pk = dev.put(_u64(pk))
        return (lambda m, op=None, ob=None: e.join_probe_emit_u64(t, d_pk, n, m, op, ob)), None
    if shape == "u128":
        t = dev.table(e.join_build_bucket_chained_u128(dev.put(_u128(bk)), nb))
        d_pk = dev.put(_u128(pk))
        return (lambda m, op=None, ob=None:
                e.join_probe_emit_mode_u128(t, d_pk, n, m, op, ob)), None
    bb, bo = _vc_cols(bk)  # row 0 = the empty sentinel string; row_count + 2 offsets
    t = dev.table(e.join_build_varchar(dev.put(bb), dev.put(bo), nb))
    pb, po = _vc_cols(pk)
    d_pb, d_po = dev.put(pb), dev.put(po)
    if shape == "vc":
        return (lambda m, op=None, ob=None:
                e.join_probe_emit_varchar_mode(t, d_pb, d_po, n, m, op, ob),
                lambda anti, ob=None: e.join_probe_right_varchar(t, d_pb, d_po, n, anti, ob))
    d_pn = dev.put(pnulls)
    return (lambda m, op=None, ob=None:
            e.join_probe_emit_varchar_nulls(t, d_pb, d_po, d_pn, n, m, op, ob)), None


def _brute(bk, pk, pnulls, mode):
    """Dict join: list of (probe row, build row) pairs in probe order."""
    rows = {}
    for j in range(1, len(bk)):
        rows.setdefault(int(bk[j]), []).append(j)
    anti = mode in (2, 6)
    out = []
    for i, k in enumerate(pk.tolist()):
        null = bool(pnulls[i])
        if null and mode == 6:
            continue
        m = [] if null else rows.get(k, [])
        if anti:
            out += [] if m else [(i, 0)]
        elif mode == 1:
            out += [(i, m[0])] if m else []
        else:
            out += [(i, j) for j in m] if m or mode == 0 else [(i, 0)]
    return out


def _check_left(dev, probe, bk, pk, pnulls, mode):
    want = _brute(bk, pk, pnulls, mode)
    cnt = probe(mode)
    assert cnt == len(want), "count-only call"
    op, ob = dev.out(cnt), dev.out(cnt)
    assert probe(mode, op, ob) == cnt, "emit call count"
    gp = op.d2h(np.uint32, cnt).astype(np.int64)
    gb = ob.d2h(np.uint32, cnt).astype(np.int64)
    assert (np.diff(gp) >= 0).all(), "out_probe must be non-decreasing"
    if mode == 1:
        assert gp.tolist() == [i for i, _ in want]
        assert (gb >= 1).all() and (bk[gb] == pk[gp]).all()
        assert not pnulls[gp].any()
    else:
        assert sorted(zip(gp.tolist(), gb.tolist())) == sorted(want)
    if mode in (2, 6):
        assert (gb == 0).all()


def _modes(shape):
    return (0, 1, 2, 3, 6) if shape.endswith("_nulls") else (0, 1, 2, 3)


@pytest.mark.parametrize("n_probe", N_PROBE)
@pytest.mark.parametrize("n_build", N_BUILD)
@pytest.mark.parametrize("shape", LEFT_SHAPES)
def test_left_modes(engine, shape, n_build, n_probe):
    bk, pk = _keys(n_build, n_probe, seed=1000 * n_build + n_probe)
    rng = np.random.default_rng(n_build + n_probe)
    pnulls = (rng.random(n_probe) < 0.25).astype(np.uint8)
    if not shape.endswith("_nulls"):
        pnulls[:] = 0
    dev = _Dev(engine)
    try:
        probe, _ = _build_and_probe(dev, shape, bk, pk, pnulls)
        for mode in _modes(shape):
            _check_left(dev, probe, bk, pk, pnulls, mode)
    finally:
        dev.close()


def test_bc_nulls_build_nulls(engine):
    """Null BUILD rows never enter a chain: they match nothing in any mode."""
    bk, pk = _keys(300, 1000, seed=7)
    rng = np.random.default_rng(8)
    bnulls = np.concatenate([[0], rng.random(300) < 0.2]).astype(np.uint8)
    pnulls = (rng.random(1000) < 0.25).astype(np.uint8)
    dev = _Dev(engine)
    try:
        e = engine
        t = dev.table(e.join_build_bucket_chained_nulls(
            dev.put(bk.astype(np.int32)), dev.put(bnulls), 300))
        d_pk, d_pn = dev.put(pk.astype(np.int32)), dev.put(pnulls)
        ref_bk = np.where(bnulls == 1, -1000, bk)  # a key no probe row has
        for mode in (0, 1, 2, 3, 6):
            _check_left(dev, lambda m, op=None, ob=None:
                        e.join_probe_emit_nulls(t, d_pk, d_pn, 1000, m, op, ob),
                        ref_bk, pk, pnulls, mode)
    finally:
        dev.close()


@pytest.mark.parametrize("n_probe", N_PROBE)
@pytest.mark.parametrize("n_build", N_BUILD)
@pytest.mark.parametrize("shape", RIGHT_SHAPES)
def test_right_semi_anti(engine, shape, n_build, n_probe):
    bk, pk = _keys(n_build, n_probe, seed=2000 * n_build + n_probe)
    probed = set(pk.tolist())
    dev = _Dev(engine)
    try:
        _, right = _build_and_probe(dev, shape, bk, pk, np.zeros(n_probe, np.uint8))
        for anti in (0, 1):
            want = [j for j in range(1, n_build + 1) if (int(bk[j]) in probed) != bool(anti)]
            cnt = right(anti)
            assert cnt == len(want), "count-only call"
            ob = dev.out(n_build)
            assert right(anti, ob) == cnt
            assert sorted(ob.d2h(np.uint32, cnt).tolist()) == want
    finally:
        dev.close()


def test_scan_tile_boundary(engine):
    """524 288 + 300 probe rows: the scan tile becomes ceil(n / 2048) = 257
    rows (no longer the block size) and the last tile is short."""
    n = 524_288 + 300
    bk, _ = _keys(37, 0, seed=11)
    rng = np.random.default_rng(12)
    pk = rng.integers(-5, 57, n).astype(np.int64)
    pk[pk == bk[37]] = ABOVE
    # numpy reference for LEFT_OUTER: build rows grouped by key
    order = np.argsort(bk[1:], kind="stable") + 1
    cnt_k = np.bincount(bk[1:], minlength=ABOVE + 1)
    start_k = np.concatenate([[0], np.cumsum(cnt_k)[:-1]])
    c = np.where(pk >= 0, cnt_k[np.clip(pk, 0, ABOVE)], 0)
    reps = np.maximum(c, 1)
    wp = np.repeat(np.arange(n), reps)
    within = np.arange(len(wp)) - np.repeat(np.cumsum(reps) - reps, reps)
    wb = np.where(c[wp] > 0, order[np.minimum(start_k[np.clip(pk[wp], 0, ABOVE)] + within,
                                              36)], 0)
    dev = _Dev(engine)
    try:
        t = dev.table(engine.join_build_bucket_chained(dev.put(bk.astype(np.int32)), 37))
        d_pk = dev.put(pk.astype(np.int32))
        cnt = engine.join_probe_emit_mode(t, d_pk, n, 3)
        assert cnt == len(wp)
        op, ob = dev.out(cnt), dev.out(cnt)
        assert engine.join_probe_emit_mode(t, d_pk, n, 3, op, ob) == cnt
        gp = op.d2h(np.uint32, cnt).astype(np.int64)
        gb = ob.d2h(np.uint32, cnt).astype(np.int64)
        assert np.array_equal(gp, wp)  # non-decreasing, every row present
        assert np.array_equal(np.sort(gp << 32 | gb), np.sort(wp << 32 | wb))
        assert (gb[c[gp] == 0] == 0).all()
    finally:
        dev.close()


@pytest.mark.parametrize("n_probe", N_PROBE)
@pytest.mark.parametrize("n_build", N_BUILD)
def test_asof_le(engine, n_build, n_probe):
    """One ASOF opcode (LE) through the shared count/scan/emit driver, INNER
    and LEFT_OUTER, against test_asof's brute force."""
    bk, pk = _keys(n_build, n_probe, seed=3000 * n_build + n_probe)
    rng = np.random.default_rng(n_build * 7 + n_probe)
    ba = np.concatenate([[0], rng.integers(-40, 40, n_build)]).astype(np.int64)
    pa = rng.integers(-40, 40, n_probe).astype(np.int64)
    want = asof_brute_force(bk, ba, pk, pa, 1)
    dev = _Dev(engine)
    try:
        t = dev.table(engine.asof_build(dev.put(bk.astype(np.int32)), dev.put(ba), n_build, 1))
        d_pk, d_pa = dev.put(pk.astype(np.int32)), dev.put(pa)
        for mode in (0, 3):
            rows = np.flatnonzero(want) if mode == 0 else np.arange(n_probe)
            cnt = engine.asof_probe_emit(t, d_pk, d_pa, n_probe, mode)
            assert cnt == len(rows), "count-only call"
            op, ob = dev.out(cnt), dev.out(cnt)
            assert engine.asof_probe_emit(t, d_pk, d_pa, n_probe, mode, op, ob) == cnt
            assert np.array_equal(op.d2h(np.uint32, cnt), rows)
            assert np.array_equal(ob.d2h(np.uint32, cnt), want[rows])
    finally:
        dev.close()


def test_undersized_output_frees_scratch(engine):
    """The documented bad-argument path: output buffers too small for the
    match count return GPUE_ERR_ARG, and every such return frees the probe's
    device scratch. 1 M probe rows make one leaked row-count array 4 MB, so
    1000 leaked calls would be 4 GB."""
    def free_bytes():  # hipMemGetInfo of the HIP runtime the engine library links
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert engine._lib.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    n, scratch = 1_000_000, 4_000_000
    bk, _ = _keys(37, 0, seed=21)
    pk = np.random.default_rng(22).integers(0, 51, n).astype(np.int32)
    dev = _Dev(engine)
    try:
        t = dev.table(engine.join_build_bucket_chained(dev.put(bk.astype(np.int32)), 37))
        d_pk = dev.put(pk)
        small_p, small_b = dev.out(1), dev.out(1)
        assert engine.join_probe_emit_mode(t, d_pk, n, 3) >= n

        def undersized_call():
            with pytest.raises(GpueError, match=r"^gpue status 2: bad argument"):
                engine.join_probe_emit_mode(t, d_pk, n, 3, small_p, small_b)

        undersized_call()  # warm: kernel code objects
        free_before = free_bytes()
        for _ in range(1000):
            undersized_call()
        free_after = free_bytes()
        # one-sided: only lost memory is a leak (other processes share the device)
        assert free_before - free_after < scratch, (free_before, free_after)
    finally:
        dev.close()
