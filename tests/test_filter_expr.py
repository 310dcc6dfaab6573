"""Predicate expressions on the device: gpue_pred_eval_mask and
gpue_mask_compact against the recursive numpy reference of
tests/test_filter_expr_cpu.py (ref_eval). Every comparison is exact.

Sizes the implementation picks (starrocks_amd/csrc/gpue.hip), restated:
  * k_pred_eval_mask: a wave owns a run of WAVE_RUN = 128 rows (2 steps of 64),
    a block tile is TILE = 512 rows, at most MAX_GRID = 2048 blocks stride
    over the tiles; IN lists stage in LDS up to IN_LDS_CAP = 4096 values
    (after de-duplication, all lists of a program together), else global.
  * gpue_mask_compact: a tile is MC_TILE = 8192 rows (128 mask words, 32 per
    wave); the emit launches at most MAX_GRID blocks, the count pass at most
    256 blocks x 4 waves, one tile per wave.

Buffers are allocated at exactly n * width bytes (1 byte when that is 0), so
a tail over-read or over-write has nowhere valid to land; the mask buffer is
pre-filled with ones, so a word the kernel skipped or a tail bit it left set
shows up."""

import numpy as np
import pytest

from starrocks_amd.engine import GpueError
from starrocks_amd.predicate import PT_I32, PT_I64, compile_predicate, pack_mask
from oracle import pyoracle as orc
from test_filter_expr_cpu import (BAD_PROGRAMS, COL_TYPES, I32_MAX, I32_MIN, I64_MAX,
                                  I64_MIN, filter_operator_case, kleene_cases, make_data,
                                  random_trees, ref_eval, run_filter_operator,
                                  truth_letters, _truth_cols)

pytestmark = pytest.mark.gpu

WAVE_RUN, TILE, MC_TILE, MAX_GRID, IN_LDS_CAP = 128, 512, 8192, 2048, 4096
# more tiles than launched blocks in all three strided kernels, ragged tail
N_BIG = MAX_GRID * MC_TILE + 2 * MC_TILE + TILE + 77


def upload(eng, arr):
    arr = np.ascontiguousarray(arr)
    buf = eng.alloc(max(arr.nbytes, 1))
    if arr.nbytes:
        buf.h2d(arr)
    return buf


def download(buf, dtype, count):
    return buf.d2h(dtype, count) if count else np.empty(0, dtype)


class DevCols:
    """Predicate columns resident on the device; eval() runs one tree."""

    def __init__(self, eng, cols, nulls, types, n):
        self.eng, self.n, self.types = eng, n, list(types)
        self.cols = [upload(eng, np.asarray(c)[:n]) for c in cols]
        self.nulls = [None if nl is None else upload(eng, np.asarray(nl)[:n]) for nl in nulls]
        self.n_words = (n + 63) // 64
        self.mask = eng.alloc(max(self.n_words * 8, 1))

    def pred_cols(self):
        return list(zip(self.cols, self.nulls, self.types))

    def eval_program(self, program):
        self.mask.h2d(np.full(max(self.n_words * 8, 1), 0xFF, np.uint8))
        cnt = self.eng.pred_eval_mask(self.pred_cols(), program, self.n, self.mask)
        return download(self.mask, np.uint64, self.n_words), cnt

    def eval(self, tree):
        return self.eval_program(compile_predicate(tree, self.types))

    def close(self):
        for b in [self.mask, *self.cols, *[x for x in self.nulls if x is not None]]:
            b.free()


def check_tree(dev, tree, cols, nulls):
    """Mask words (tail bits 0 included) and count equal the reference."""
    keep, _ = ref_eval(tree, cols, nulls, dev.n)
    words, cnt = dev.eval(tree)
    assert np.array_equal(words, pack_mask(keep)), tree
    assert cnt == int(keep.sum()), tree
    return keep


def payloads(n):
    r = np.arange(n, dtype=np.uint64)
    return [((r * 7 + 1) & 0xFF).astype(np.uint8), (r * 3 + 1).astype(np.uint32),
            (r << np.uint64(33)) | r]


def check_compact(eng, mask, n, keep):
    """Compacted columns of widths 1, 4 and 8 and out_row_idx equal numpy."""
    cnt = int(keep.sum())
    arrays = payloads(n)
    srcs = [upload(eng, a) for a in arrays]
    dsts = [eng.alloc(max(cnt * a.itemsize, 1)) for a in arrays]
    idx = eng.alloc(max(cnt * 4, 1))
    try:
        got = eng.mask_compact(mask, n, [(s, d, a.itemsize) for s, d, a
                                         in zip(srcs, dsts, arrays)], idx)
        assert got == cnt
        for d, a in zip(dsts, arrays):
            assert np.array_equal(download(d, a.dtype, cnt), a[keep])
        assert np.array_equal(download(idx, np.uint32, cnt), np.flatnonzero(keep).astype(np.uint32))
        assert eng.mask_compact(mask, n, []) == cnt          # count-only
    finally:
        for b in (*srcs, *dsts, idx):
            b.free()


EDGE_TREE = ("or", ("and", ("cmp", "<", 0, 2), ("not", ("in", 3, [0, 5, -4, I64_MAX]))),
             ("and", ("is_null", 1), ("cmp_col", ">=", 2, 3)), ("between", 1, -1, 1))


assert WAVE_RUN == 128   # WAVE_RUN - 1, WAVE_RUN, WAVE_RUN + 1 are 127, 128, 129 below


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129,
                               TILE - 1, TILE, TILE + 1, 2 * TILE + WAVE_RUN + 1,
                               MC_TILE - 1, MC_TILE, MC_TILE + 1])
def test_row_count_edges(engine, n):
    cols, nulls = make_data(n, seed=21)
    dev = DevCols(engine, cols, nulls, COL_TYPES, n)
    try:
        keep = check_tree(dev, EDGE_TREE, cols, nulls)
        if n > 64:
            assert 0 < keep.sum() < n
        check_compact(engine, dev.mask, n, keep)
    finally:
        dev.close()


def test_more_tiles_than_blocks_ragged_tail(engine):
    n = N_BIG
    assert n // TILE > MAX_GRID and n // MC_TILE > MAX_GRID and n % 64 and n % TILE
    r = np.arange(n, dtype=np.uint32)
    h = r * np.uint32(2654435761)
    a = ((h >> np.uint32(9)) % np.uint32(13)).astype(np.int32) - 6
    a_null = ((h >> np.uint32(3)) % np.uint32(5) == 0).astype(np.uint8)
    b = ((h >> np.uint32(17)) % np.uint32(7)).astype(np.int64)
    cols, nulls, types = [a, b], [a_null, None], [PT_I32, PT_I64]
    tree = ("or", ("and", ("cmp", "<", 0, -2), ("cmp", "!=", 1, 3)),
            ("and", ("is_null", 0), ("cmp", "=", 1, 6)))
    dev = DevCols(engine, cols, nulls, types, n)
    try:
        keep = check_tree(dev, tree, cols, nulls)
        assert 0 < keep.sum() < n and keep[-(n % TILE):].any()
        check_compact(engine, dev.mask, n, keep)
    finally:
        dev.close()


N_MULTI = 3 * MC_TILE + TILE + 37


@pytest.mark.parametrize("name", ["none", "all", "row0", "last", "alternating", "last_tile"])
def test_survivor_patterns(engine, name):
    n = N_MULTI
    v = np.arange(n, dtype=np.int64)
    odd = (v & 1).astype(np.int32)
    last_tile = (n - 1) // MC_TILE * MC_TILE
    tree = {"none": ("cmp", "<", 0, 0), "all": ("cmp", ">=", 0, 0), "row0": ("cmp", "=", 0, 0),
            "last": ("cmp", "=", 0, n - 1), "alternating": ("cmp", "=", 1, 1),
            "last_tile": ("cmp", ">=", 0, last_tile)}[name]
    cols, nulls = [v, odd], [None, None]
    dev = DevCols(engine, cols, nulls, [PT_I64, PT_I32], n)
    try:
        keep = check_tree(dev, tree, cols, nulls)
        assert int(keep.sum()) == {"none": 0, "all": n, "row0": 1, "last": 1,
                                   "alternating": n // 2, "last_tile": n - last_tile}[name]
        check_compact(engine, dev.mask, n, keep)
    finally:
        dev.close()


def test_compare_extremes(engine):
    n = 70
    e32 = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX], np.int32)
    e64 = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64)
    c32, c64 = np.resize(e32, n), np.resize(e64, n)
    cols, nulls = [c32, c64], [None, None]
    consts = {0: [I32_MIN, I32_MIN + 1, 0, I32_MAX - 1, I32_MAX,
                  # outside int32, both sides: the column sign-extends to int64
                  I32_MIN - 1, I32_MAX + 1, -(1 << 40), 1 << 40, I64_MIN, I64_MAX],
              1: [I64_MIN, I64_MIN + 1, 0, I64_MAX - 1, I64_MAX, I32_MIN, I32_MAX]}
    dev = DevCols(engine, cols, nulls, [PT_I32, PT_I64], n)
    try:
        for c, cs in consts.items():
            for k in cs:
                for op in ("=", "!=", "<", "<=", ">", ">="):
                    check_tree(dev, ("cmp", op, c, k), cols, nulls)
            for lo in cs:
                for hi in cs:
                    check_tree(dev, ("between", c, lo, hi), cols, nulls)
        words, cnt = dev.eval(("cmp", "<", 0, 1 << 40))
        assert cnt == n
    finally:
        dev.close()


def test_rhs_col_compares(engine):
    n = 7 * 7 * 3
    e32 = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX], np.int32)
    e64 = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64)
    i = np.arange(n)
    cols = [e32[i % 7], e32[(i // 7) % 7], e64[i % 7], e64[(i // 7) % 7]]
    nulls = [None, (i % 5 == 0).astype(np.uint8), (i % 3 == 0).astype(np.uint8) * 200, None]
    dev = DevCols(engine, cols, nulls, COL_TYPES, n)
    try:
        for x, y in ((0, 1), (1, 0), (2, 3), (3, 2), (0, 0), (3, 3)):
            for op in ("=", "!=", "<", "<=", ">", ">="):
                check_tree(dev, ("cmp_col", op, x, y), cols, nulls)
                check_tree(dev, ("not", ("cmp_col", op, x, y)), cols, nulls)
    finally:
        dev.close()


def test_three_valued_logic_on_device(engine):
    _, _, cols, nulls = _truth_cols()
    types = [PT_I32, PT_I32]
    dev = DevCols(engine, cols, nulls, types, 9)
    try:
        for tree, expect in kleene_cases():
            # TRUE rows straight from the mask, FALSE rows from the negated tree's
            words, _ = dev.eval(tree)
            nwords, _ = dev.eval(("not", tree))
            t = [(int(words[0]) >> r) & 1 for r in range(9)]
            f = [(int(nwords[0]) >> r) & 1 for r in range(9)]
            assert truth_letters(t, f) == expect, tree
    finally:
        dev.close()


def test_nulls_on_device(engine):
    n = 3000
    cols, nulls = make_data(n, seed=31, garbage_seed=1)
    cols_b, nulls_b = make_data(n, seed=31, garbage_seed=2)
    assert not np.array_equal(cols[3], cols_b[3])
    trees = [("not", ("in", 1, [0, 3, -2, I32_MIN])),          # NOT IN: NULL rows drop
             ("not", ("in", 3, [])),
             ("is_null", 1), ("not", ("is_null", 3)),           # with a mask
             ("is_null", 0), ("not", ("is_null", 2)),           # without one: FALSE / TRUE
             ("or", ("is_null", 3), ("cmp", ">", 3, 0)),
             ("and", ("not", ("cmp", "=", 1, 2)), ("not", ("between", 3, -2, 2)))]
    dev, dev_b = (DevCols(engine, c, nl, COL_TYPES, n) for c, nl in
                  ((cols, nulls), (cols_b, nulls_b)))
    try:
        for tree in trees:
            keep = check_tree(dev, tree, cols, nulls)
            words_b, cnt_b = dev_b.eval(tree)     # other garbage under the NULLs: same mask
            assert np.array_equal(words_b, pack_mask(keep)) and cnt_b == int(keep.sum())
        keep = check_tree(dev, trees[0], cols, nulls)
        assert not keep[nulls[1] != 0].any() and keep.any()
        assert dev.eval(("is_null", 0))[1] == 0 and dev.eval(("not", ("is_null", 2)))[1] == n
    finally:
        dev.close()
        dev_b.close()


@pytest.mark.parametrize("size", [0, 1, 2, 17, 1000, IN_LDS_CAP, IN_LDS_CAP + 1, 5000])
def test_in_list_sizes(engine, size):
    n = 3001
    rng = np.random.default_rng(size + 1)
    pool64 = np.unique(np.concatenate([[I64_MIN, I64_MAX], rng.integers(-(1 << 62), 1 << 62, 6000)]))
    pool32 = np.unique(np.concatenate([[I32_MIN, I32_MAX], rng.integers(I32_MIN, I32_MAX, 6000)]))
    l64 = [int(x) for x in ([I64_MIN, I64_MAX] + list(rng.permutation(pool64[1:-1])))[:size]]
    l32 = [int(x) for x in ([I32_MAX, I32_MIN] + list(rng.permutation(pool32[1:-1])))[:size]]
    assert len(set(l64)) == size == len(set(l32))
    c64 = rng.choice(pool64, n)
    c32 = rng.choice(pool32, n).astype(np.int32)
    c64[:4] = [I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1]
    c32[:4] = [I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1]
    nl = (rng.random(n) < 0.2).astype(np.uint8)
    cols, nulls = [c32, c64], [None, nl]
    dev = DevCols(engine, cols, nulls, [PT_I32, PT_I64], n)
    try:
        dup = l64 + l64[: size // 2]                     # unsorted, with duplicates
        keep = check_tree(dev, ("in", 1, dup), cols, nulls)
        if size >= 17:
            assert 0 < keep.sum() < n
        check_tree(dev, ("not", ("in", 1, l64)), cols, nulls)
        # int32 column against a list that also holds values outside int32
        check_tree(dev, ("in", 0, l32 + [1 << 40, I64_MIN, I64_MAX]), cols, nulls)
        # two IN leaves of one program share in_values
        check_tree(dev, ("or", ("in", 0, l32), ("in", 1, l64[::-1])), cols, nulls)
        check_tree(dev, ("and", ("not", ("in", 0, l32[: size // 3])), ("in", 1, l64)), cols, nulls)
    finally:
        dev.close()


def test_random_trees_on_device(engine):
    n = 5003
    cols, nulls = make_data(n, seed=11)
    trees = random_trees(160)
    dev = DevCols(engine, cols, nulls, COL_TYPES, n)
    try:
        for tree in trees:
            check_tree(dev, tree, cols, nulls)
    finally:
        dev.close()


def filter_cols(eng, tree, cols_np, types):
    """engine.filter_expr over all-predicate, all-payload columns -> numpy."""
    n = len(cols_np[0])
    bufs = [upload(eng, c) for c in cols_np]
    out, cnt = eng.filter_expr(tree, [(b, None, t) for b, t in zip(bufs, types)],
                               [(b, c.itemsize) for b, c in zip(bufs, cols_np)], n)
    got = [download(o, c.dtype, cnt) for o, c in zip(out, cols_np)]
    assert all(o.nbytes == max(cnt * c.itemsize, 1) for o, c in zip(out, cols_np))
    for b in (*bufs, *out):
        b.free()
    return got, cnt


ORACLE_OPS = {0: lambda c, lo, hi: ("cmp", "=", c, lo), 1: lambda c, lo, hi: ("cmp", "<", c, hi),
              2: lambda c, lo, hi: ("between", c, lo, hi)}


@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
def test_and_chains_equal_the_c_oracle(engine, wide):
    """AND chains of EQ / LT / BETWEEN: the compacted columns equal what the
    oracle's eager-prune evaluator leaves — on the shapes of
    tests/test_edge_cases.py (Q1.1's WHERE at 200 000 rows, all-false
    short-circuit, all-true skip) and around its prune threshold
    max(0.8 * rows, 1024): zeros just above and just below 0.8 * rows, and
    fewer than 1024 rows where it never prunes early."""
    dt, typ = (np.int64, PT_I64) if wide else (np.int32, PT_I32)
    oracle = orc.eval_conjuncts_i64 if wide else orc.eval_conjuncts
    rng = np.random.default_rng(83)
    n = 200_000
    od = rng.integers(19920101, 19990101, n).astype(dt)
    dc = rng.integers(0, 11, n).astype(dt)
    qt = rng.integers(1, 51, n).astype(dt)
    ramp = np.arange(n).astype(dt)        # ramp < k keeps exactly k rows
    cases = [([od, dc, qt], [(0, 2, 19930101, 19931231), (1, 2, 1, 3), (2, 1, 0, 25)]),
             ([od, dc, qt], [(1, 0, 99, 0)]),
             ([od, dc, qt], [(2, 1, 0, 100)]),
             ([ramp, dc, qt], [(0, 1, 0, n // 5 - 1), (1, 2, 1, 3)]),     # zeros > 0.8 n
             ([ramp, dc, qt], [(0, 1, 0, n // 5 + 1), (1, 2, 1, 3)]),     # zeros < 0.8 n
             ([ramp, dc, qt], [(1, 0, 4, 0), (0, 2, 100, n - 100), (2, 1, 0, 30)]),
             ([ramp[:1000].copy(), dc[:1000].copy()], [(0, 1, 0, 10), (1, 2, 0, 5)]),
             ([ramp[:1300].copy(), dc[:1300].copy()], [(0, 1, 0, 250), (1, 1, 0, 5)])]
    if wide:
        big = (od.astype(np.int64) << 32) + dc
        cases.append(([big, qt], [(0, 2, 19930101 << 32, (19931231 << 32) + 5), (1, 1, 0, 25)]))
    for cols_np, preds in cases:
        expect = [c.copy() for c in cols_np]
        m = oracle(expect, preds)
        tree = ("and", *[ORACLE_OPS[op](c, lo, hi) for c, op, lo, hi in preds])
        got, cnt = filter_cols(engine, tree, cols_np, [typ] * len(cols_np))
        assert cnt == m, preds
        for g, e in zip(got, expect):
            assert np.array_equal(g, e[:m]), preds


def codes_of(strings):
    """Sorted dictionary + int32 codes, the form a dict-encoded page decodes to."""
    dictionary, codes = np.unique(np.asarray(strings), return_inverse=True)
    return list(dictionary), codes.astype(np.int32).reshape(-1)


def test_named_predicates(engine):
    n = 40_000
    rng = np.random.default_rng(1993)
    # SSB Q1.1: d_year = 1993 AND lo_discount BETWEEN 1 AND 3 AND lo_quantity < 25
    d_year = rng.integers(1992, 1999, n).astype(np.int32)
    disc = rng.integers(0, 11, n).astype(np.int32)
    qty = rng.integers(1, 51, n).astype(np.int32)
    got, cnt = filter_cols(engine, ("and", ("cmp", "=", 0, 1993), ("between", 1, 1, 3),
                                    ("cmp", "<", 2, 25)), [d_year, disc, qty], [PT_I32] * 3)
    keep = (d_year == 1993) & (disc >= 1) & (disc <= 3) & (qty < 25)
    assert cnt == keep.sum() > 0 and all(np.array_equal(g, c[keep]) for g, c in
                                         zip(got, (d_year, disc, qty)))

    # Q2.2: p_brand BETWEEN 'MFGR#2221' AND 'MFGR#2228' over sorted dictionary codes
    brands = np.array([f"MFGR#{m}{c}{b:02d}" for m in range(1, 6) for c in range(1, 6)
                       for b in range(1, 41)])
    p_brand = brands[rng.integers(0, len(brands), n)]
    bdict, bcode = codes_of(p_brand)
    lo = int(np.searchsorted(bdict, "MFGR#2221", "left"))
    hi = int(np.searchsorted(bdict, "MFGR#2228", "right")) - 1
    got, cnt = filter_cols(engine, ("between", 0, lo, hi), [bcode], [PT_I32])
    keep = (p_brand >= "MFGR#2221") & (p_brand <= "MFGR#2228")
    assert cnt == keep.sum() > 0 and np.array_equal(got[0], bcode[keep])

    # Q3.4: c_city IN (..) AND s_city IN (..) AND d_yearmonth = 'Dec1997'
    cities = np.array([f"UNITED KI{k}" for k in range(10)] + [f"CHINA    {k}" for k in range(10)])
    months = np.array([f"{m}{y}" for y in range(1992, 1999) for m in
                       ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct",
                        "Nov", "Dec")])
    c_city, s_city = cities[rng.integers(0, 20, n)], cities[rng.integers(0, 20, n)]
    ym = months[rng.integers(0, len(months), n)]
    (cd, cc), (sd, sc), (md, mc) = codes_of(c_city), codes_of(s_city), codes_of(ym)
    wanted = ["UNITED KI1", "UNITED KI5"]
    tree = ("and", ("in", 0, [cd.index(w) for w in wanted]),
            ("in", 1, [sd.index(w) for w in wanted]), ("cmp", "=", 2, md.index("Dec1997")))
    got, cnt = filter_cols(engine, tree, [cc, sc, mc], [PT_I32] * 3)
    keep = np.isin(c_city, wanted) & np.isin(s_city, wanted) & (ym == "Dec1997")
    assert cnt == keep.sum() > 0 and all(np.array_equal(g, c[keep]) for g, c in
                                         zip(got, (cc, sc, mc)))

    # TPC-H Q12 shape: l_commitdate < l_receiptdate AND l_shipdate < l_commitdate
    #                  AND l_shipmode IN ('MAIL', 'SHIP')
    ship = rng.integers(8000, 10500, n).astype(np.int32)
    commit = (ship + rng.integers(-30, 60, n)).astype(np.int32)
    receipt = (ship + rng.integers(1, 31, n)).astype(np.int32)
    modes = np.array(["AIR", "FOB", "MAIL", "RAIL", "REG AIR", "SHIP", "TRUCK"])
    shipmode = modes[rng.integers(0, 7, n)]
    mdict, mcode = codes_of(shipmode)
    tree = ("and", ("cmp_col", "<", 1, 2), ("cmp_col", "<", 0, 1),
            ("in", 3, [mdict.index("MAIL"), mdict.index("SHIP")]))
    got, cnt = filter_cols(engine, tree, [ship, commit, receipt, mcode], [PT_I32] * 4)
    keep = (commit < receipt) & (ship < commit) & np.isin(shipmode, ["MAIL", "SHIP"])
    assert cnt == keep.sum() > 0 and all(np.array_equal(g, c[keep]) for g, c in
                                         zip(got, (ship, commit, receipt, mcode)))

    # Q19 shape: an OR of three AND groups (brand code, container IN, quantity range, size)
    brand = rng.integers(0, 25, n).astype(np.int32)
    cont = rng.integers(0, 40, n).astype(np.int32)
    quantity = rng.integers(1, 51, n).astype(np.int64)
    size = rng.integers(1, 51, n).astype(np.int32)

    def group(b, conts, qlo, smax):
        return ("and", ("cmp", "=", 0, b), ("in", 1, conts), ("between", 2, qlo, qlo + 10),
                ("between", 3, 1, smax))

    groups = [(12, [0, 1, 2, 3], 1, 5), (23, [10, 11, 12, 13], 10, 10), (4, [20, 21, 22, 23], 20, 15)]
    tree = ("or", *[group(*g) for g in groups])
    got, cnt = filter_cols(engine, tree, [brand, cont, quantity, size],
                           [PT_I32, PT_I32, PT_I64, PT_I32])
    keep = np.zeros(n, bool)
    for b, conts, qlo, smax in groups:
        keep |= ((brand == b) & np.isin(cont, conts) & (quantity >= qlo) &
                 (quantity <= qlo + 10) & (size >= 1) & (size <= smax))
    assert cnt == keep.sum() > 0 and all(np.array_equal(g, c[keep]) for g, c in
                                         zip(got, (brand, cont, quantity, size)))


def test_mask_compact_alone(engine):
    n = 2 * MC_TILE + 3 * 64 + 21          # last word holds 21 rows
    rng = np.random.default_rng(8)
    keep = rng.random(n) < 0.3
    keep[[0, n - 1]] = True
    words = pack_mask(keep)
    words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n & 63)   # garbage past n_rows
    mask = upload(engine, words)
    cnt = int(keep.sum())
    try:
        check_compact(engine, mask, n, keep)
        a4 = payloads(n)[1]
        src = upload(engine, a4)
        short = engine.alloc((cnt - 1) * 4)
        exact = engine.alloc(cnt * 4)
        idx_short = engine.alloc((cnt - 1) * 4)
        try:
            with pytest.raises(GpueError) as ei:          # short dst reports the needed count
                engine.mask_compact(mask, n, [(src, short, 4)])
            assert ei.value.needed_count == cnt
            with pytest.raises(GpueError) as ei:
                engine.mask_compact(mask, n, [(src, exact, 4)], idx_short)
            assert ei.value.needed_count == cnt
            with pytest.raises(GpueError):                # src == dst
                engine.mask_compact(mask, n, [(src, src, 4)])
            src2 = upload(engine, a4)
            with pytest.raises(GpueError):                # dst aliases another column's src
                engine.mask_compact(mask, n, [(src, exact, 4), (src2, src, 4)])
            src2.free()
            assert engine.mask_compact(mask, n, [(src, exact, 4)]) == cnt     # retry, sized
            assert np.array_equal(exact.d2h(np.uint32, cnt), a4[keep])
            assert engine.mask_compact(mask, n, []) == cnt                    # count-only
            assert engine.mask_compact(mask, 0, []) == 0
        finally:
            for b in (src, short, exact, idx_short):
                b.free()
    finally:
        mask.free()


def test_mask_compact_many_columns(engine):
    """More columns than one emit launch carries (8), mixed widths."""
    n = MC_TILE + 100
    keep = np.random.default_rng(5).random(n) < 0.5
    mask = upload(engine, pack_mask(keep))
    cnt = int(keep.sum())
    arrays = [payloads(n)[k % 3] + np.array(k).astype(payloads(n)[k % 3].dtype)
              for k in range(11)]
    srcs = [upload(engine, a) for a in arrays]
    dsts = [engine.alloc(cnt * a.itemsize) for a in arrays]
    try:
        assert engine.mask_compact(mask, n, [(s, d, a.itemsize) for s, d, a
                                             in zip(srcs, dsts, arrays)]) == cnt
        for d, a in zip(dsts, arrays):
            assert np.array_equal(download(d, a.dtype, cnt), a[keep])
    finally:
        for b in (mask, *srcs, *dsts):
            b.free()


def test_argument_errors(engine):
    n = 200
    cols, nulls = make_data(n, seed=3)
    dev = DevCols(engine, cols, nulls, COL_TYPES, n)
    good = compile_predicate(EDGE_TREE, COL_TYPES)
    keep, _ = ref_eval(EDGE_TREE, cols, nulls, n)

    def valid_call_still_works():
        words, cnt = dev.eval_program(good)
        assert np.array_equal(words, pack_mask(keep)) and cnt == int(keep.sum())

    short4, short8, short1 = (engine.alloc(n * w - 1) for w in (4, 8, 1))
    short_mask = engine.alloc(dev.n_words * 8 - 1)
    try:
        valid_call_still_works()
        for name in sorted(BAD_PROGRAMS):
            with pytest.raises(GpueError):
                dev.eval_program(BAD_PROGRAMS[name])
            valid_call_still_works()
        pc = dev.pred_cols()
        bad_calls = [
            (pc, 1 << 32, dev.mask),                                            # n_rows >= 2^32
            ([(short4, None, PT_I32)] + pc[1:], n, dev.mask),                   # short I32 column
            (pc[:2] + [(short8, None, PT_I64)] + pc[3:], n, dev.mask),          # short I64 column
            (pc[:1] + [(pc[1][0], short1, PT_I32)] + pc[2:], n, dev.mask),      # short null mask
            (pc, n, short_mask),                                                # short mask
            ([(pc[0][0], None, 2)] + pc[1:], n, dev.mask),                      # unknown pred_type
            ([(pc[0][0], None, -1)] + pc[1:], n, dev.mask),
        ]
        for pcs, rows, m in bad_calls:
            with pytest.raises(GpueError):
                engine.pred_eval_mask(pcs, good, rows, m)
            valid_call_still_works()
        # n_rows == 0 is fine, count 0
        assert engine.pred_eval_mask(pc, good, 0, dev.mask) == 0

        src, dst = pc[0][0], engine.alloc(n * 8)
        try:
            compact_bad = [
                (dev.mask, n, [(src, dst, 2)]),                 # width outside {1, 4, 8}
                (dev.mask, n, [(src, dst, 0)]),
                (dev.mask, n, [(src, dst, 8)]),                 # src shorter than n * width
                (dev.mask, 1 << 32, [(src, dst, 4)]),           # n_rows >= 2^32
                (dev.mask, n, [(src, src, 4)]),                 # src == dst
                (short_mask, n, [(src, dst, 4)]),               # short mask
                (dev.mask, n, [(src, dev.mask, 4)]),            # dst is the mask
            ]
            for m, rows, cs in compact_bad:
                with pytest.raises(GpueError):
                    engine.mask_compact(m, rows, cs)
                valid_call_still_works()
            assert engine.mask_compact(dev.mask, n, [(src, dst, 4)]) == int(keep.sum())
            assert np.array_equal(dst.d2h(np.int32, int(keep.sum())), cols[0][keep])
        finally:
            dst.free()
    finally:
        for b in (short4, short8, short1, short_mask):
            b.free()
        dev.close()


def test_filter_operator_on_device(engine):
    """3-chunk source -> FilterOperator -> sink equals the numpy filter of the
    concatenated input; the nullable column's u8 mask rides as a width-1
    payload column."""
    arrays, keep = filter_operator_case()
    filt, out, pushed = run_filter_operator(engine, arrays)
    for got, arr in zip(out, arrays):
        assert got.dtype == arr.dtype and np.array_equal(got, arr[keep])
    assert filt.rows_in == len(keep) and filt.rows_out == int(keep.sum())
    assert all(b._h is None for b in pushed)          # inputs freed by the operator
