"""Scalar expressions on the device: gpue_expr_project against the numpy
interpreter expr.run_program (itself pinned to a brute-force evaluator in
tests/test_expr_cpu.py). Every output buffer, every null buffer and every mask
word is compared bit-exactly.

Sizes the implementation picks (starrocks_amd/csrc/gpue.hip), restated: a wave
owns a run of WAVE_RUN = 128 rows (2 steps of 64), a block tile is TILE = 512
rows, at most EXPR_GRID = 16384 blocks stride over the tiles.

Buffers are allocated at exactly their size (1 byte when that is 0), so a tail
over-read or over-write has nowhere valid to land; every output is pre-filled
with 0xFF, so a row or word the kernel skipped, or a tail bit it left set,
shows up."""

import numpy as np
import pytest

from starrocks_amd.engine import GpueError
from starrocks_amd.expr import (EXPR_MAX_INSNS, XO_I32, XO_I64, XO_MASK, compile_exprs,
                                run_program)
from starrocks_amd.predicate import PT_I32, PT_I64, compile_predicate, unpack_mask
from test_expr_cpu import (BAD_PROGRAMS, COL_NULLABLE, COL_TYPES, GARBAGE64,
                           GOOD_WITHOUT_NULLS, I32_MAX, I32_MIN, I64_MAX, I64_MIN, POOL,
                           binary_op_trees, check_project_operator, make_data, pool_cross,
                           project_operator_case, random_programs, run_project_operator,
                           unary_op_trees)

pytestmark = pytest.mark.gpu

WAVE_RUN, TILE, EXPR_GRID = 128, 512, 16384
A, B = ("col", 0), ("col", 1)
OUT_DT = {XO_I32: np.int32, XO_I64: np.int64}


def upload(eng, arr):
    arr = np.ascontiguousarray(arr)
    buf = eng.alloc(max(arr.nbytes, 1))
    if arr.nbytes:
        buf.h2d(arr)
    return buf


def download(buf, dtype, count):
    return buf.d2h(dtype, count) if count else np.empty(0, dtype)


def out_bytes(t, n):
    return (n + 63) // 64 * 8 if t == XO_MASK else n * (8 if t == XO_I64 else 4)


def filled(eng, nbytes):
    buf = eng.alloc(max(nbytes, 1))
    buf.h2d(np.full(max(nbytes, 1), 0xFF, np.uint8))
    return buf


class DevCols:
    """Input columns resident on the device; run() evaluates one program."""

    def __init__(self, eng, cols, nulls, types, n):
        self.eng, self.n, self.types = eng, n, list(types)
        self.cols = [upload(eng, np.asarray(c)[:n]) for c in cols]
        self.nulls = [None if nl is None else upload(eng, np.asarray(nl)[:n]) for nl in nulls]

    def in_cols(self):
        return list(zip(self.cols, self.nulls, self.types))

    def run_program(self, program, nullable, out_types, all_nulls=False):
        """-> per output (values, nulls or None), as expr.run_program returns
        them. A null buffer is passed for nullable outputs only, unless
        all_nulls."""
        n, outs = self.n, []
        for t, nl in zip(out_types, nullable):
            outs.append((filled(self.eng, out_bytes(t, n)),
                         filled(self.eng, n) if t != XO_MASK and (nl or all_nulls) else None, t))
        try:
            self.eng.expr_project(self.in_cols(), program, n, outs)
            res = []
            for buf, nbuf, t in outs:
                if t == XO_MASK:
                    res.append((download(buf, np.uint64, (n + 63) // 64), None))
                else:
                    res.append((download(buf, OUT_DT[t], n),
                                None if nbuf is None else download(nbuf, np.uint8, n)))
            return res
        finally:
            for buf, nbuf, _ in outs:
                buf.free()
                if nbuf is not None:
                    nbuf.free()

    def run(self, trees, out_types, all_nulls=False):
        program, nullable = compile_exprs(trees, self.types,
                                          [x is not None for x in self.nulls], out_types)
        return self.run_program(program, nullable, out_types, all_nulls), nullable

    def close(self):
        for b in [*self.cols, *[x for x in self.nulls if x is not None]]:
            b.free()


def assert_same(got, want, nullable, what=""):
    """Device outputs == interpreter outputs, bit for bit. An output without a
    null buffer must be one the interpreter never nulls."""
    assert len(got) == len(want)
    for k, ((gv, gn), (wv, wn)) in enumerate(zip(got, want)):
        assert gv.dtype == wv.dtype and np.array_equal(gv, wv), f"{what}: output {k} values"
        if wn is None:
            assert gn is None
        elif gn is None:
            assert not nullable[k] and not wn.any(), f"{what}: output {k} statically non-null"
        else:
            assert np.array_equal(gn, wn), f"{what}: output {k} nulls"


def check(eng, trees, out_types, cols, nulls, types, n, all_nulls=False):
    cols = [np.asarray(c)[:n] for c in cols]
    nulls = [None if x is None else np.asarray(x)[:n] for x in nulls]
    dev = DevCols(eng, cols, nulls, types, n)
    try:
        got, nullable = dev.run(trees, out_types, all_nulls)
    finally:
        dev.close()
    program, _ = compile_exprs(trees, types, [x is not None for x in nulls], out_types)
    want = run_program(program, cols, nulls, types, out_types, n)
    assert_same(got, want, nullable, trees)
    return want


def tiled(arr, n):
    return np.resize(arr, n)


def batches(trees, size=8):
    return [trees[i:i + size] for i in range(0, len(trees), size)]


EDGE_TREES = [("*", ("col", 0), ("col", 1), "checked"),
              ("case", [(("cmp", "<", ("col", 2), ("col", 3)), ("col", 2))], ("col", 0)),
              ("or", ("cmp", "<", ("col", 0), ("const", 1)), ("is_null", ("col", 3)))]
EDGE_TYPES = [XO_I64, XO_I32, XO_MASK]

assert (WAVE_RUN, TILE) == (128, 512)   # their -1 / +0 / +1 are spelled out below


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513,
                               (1 << 20) + 37])
def test_row_count_edges(engine, n):
    """(1 << 20) + 37 rows are 2049 tiles, one block each, the last wave run
    ragged; test_more_tiles_than_blocks has the size at which blocks loop."""
    cols, nulls = make_data(n, 3)
    check(engine, EDGE_TREES, EDGE_TYPES, cols, nulls, COL_TYPES, n)
    # and with a null buffer on every non-MASK output: non-nullable ones get zeros
    if n in (1, 129):
        check(engine, EDGE_TREES, EDGE_TYPES, cols, nulls, COL_TYPES, n, all_nulls=True)


def test_more_tiles_than_blocks(engine):
    """EXPR_GRID * TILE + TILE + 37 rows: block 0 takes a second tile and block
    1 a ragged one. Two int32 columns and arange-built data keep the numpy
    side to a fraction of a second."""
    n = EXPR_GRID * TILE + TILE + 37
    r = np.arange(n, dtype=np.int64)
    a = ((r * 2654435761) >> 7).astype(np.int32)
    b = (r % 11 - 3).astype(np.int32)
    bn = (r % 13 == 0).astype(np.uint8)
    check(engine, [("*", A, B), ("cmp", "<", A, B)], [XO_I64, XO_MASK], [a, b], [None, bn],
          [PT_I32, PT_I32], n)


N_POOL = TILE + WAVE_RUN + 45     # 685: the 121 pairs tiled over more than one block


def test_binary_ops_over_the_pool(engine):
    """Wrap against checked, DIV / MOD by 0 and -1, compares, Kleene, IFNULL
    over POOL x POOL, into I64, I32 and MASK outputs."""
    x, y = (tiled(v, N_POOL) for v in pool_cross())
    for trees in batches(binary_op_trees()):
        for t in (XO_I64, XO_I32, XO_MASK):
            check(engine, trees, [t] * len(trees), [x, y], [None, None], [PT_I64, PT_I64], N_POOL)


def test_binary_ops_with_null_operands(engine):
    """The same with NULL rows on either side (a NULL divisor included) and
    garbage stored under them."""
    x, y = (tiled(v, N_POOL) for v in pool_cross())
    xn = (np.arange(N_POOL) % 3 == 0).astype(np.uint8)
    yn = (np.arange(N_POOL) % 5 == 0).astype(np.uint8)
    xg = np.where(xn != 0, np.int64(GARBAGE64), x)
    yg = np.where(yn != 0, np.int64(GARBAGE64), y)
    for trees in batches(binary_op_trees()):
        check(engine, trees, [XO_I64] * len(trees), [xg, yg], [xn, yn], [PT_I64, PT_I64], N_POOL)


def test_div_mod_spelled_out(engine):
    x = np.array([I64_MIN, I64_MIN, -7, 7, -7, 5, 5, 0, I64_MAX, 9], np.int64)
    y = np.array([-1, 1, 2, -2, -2, 0, -1, 0, -1, 4], np.int64)
    yn = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1], np.uint8)
    want = check(engine, [("/", A, B), ("%", A, B)], [XO_I64, XO_I64], [x, y], [None, yn],
                 [PT_I64, PT_I64], len(x))
    assert want[0][0].tolist() == [I64_MIN, I64_MIN, -3, -3, 3, 0, -5, 0, -I64_MAX, 0]
    assert want[1][0].tolist() == [0, 0, -1, 1, -1, 0, 0, 0, 0, 0]
    assert want[0][1].tolist() == want[1][1].tolist() == [0, 0, 0, 0, 0, 1, 0, 1, 0, 1]


def test_unary_ops_and_cast_edges(engine):
    edge = [I32_MIN - 1, I32_MIN, I32_MAX, I32_MAX + 1, I64_MIN, I64_MAX, 0, -1]
    x = tiled(np.array(POOL + edge, np.int64), N_POOL)
    xn = (np.arange(N_POOL) % 7 == 0).astype(np.uint8)
    for nulls in ([None], [xn]):
        check(engine, unary_op_trees(), [XO_I64] * 8, [x], nulls, [PT_I64], N_POOL)
    cast = check(engine, [("cast_i32", A)], [XO_I32], [np.array(edge, np.int64)], [None],
                 [PT_I64], len(edge))
    assert cast[0][1].tolist() == [1, 0, 0, 1, 1, 1, 0, 0]
    assert cast[0][0].tolist() == [0, I32_MIN, I32_MAX, 0, 0, 0, 0, -1]


def test_if_with_null_condition_and_ifnull(engine):
    c = np.array([0, 1, -5, 9, 0], np.int64)
    cn = np.array([0, 0, 0, 1, 1], np.uint8)
    t = np.array([10, 11, 12, 13, 14], np.int64)
    tn = np.array([0, 1, 0, 0, 0], np.uint8)
    e = np.array([20, 21, 22, 23, 24], np.int32)
    trees = [("if", ("col", 0), ("col", 1), ("col", 2)), ("ifnull", ("col", 1), ("col", 2)),
             ("ifnull", ("col", 0), ("col", 1)), ("case", [(("col", 0), ("col", 2))], None)]
    want = check(engine, trees, [XO_I64] * 4, [c, t, e], [cn, tn, None],
                 [PT_I64, PT_I64, PT_I32], 5)
    assert want[0][0].tolist() == [20, 0, 12, 23, 24] and want[0][1].tolist() == [0, 1, 0, 0, 0]
    assert want[1][0].tolist() == [10, 21, 12, 13, 14] and not want[1][1].any()
    assert want[2][0].tolist() == [0, 1, -5, 13, 14] and not want[2][1].any()
    assert want[3][0].tolist() == [0, 21, 22, 0, 0] and want[3][1].tolist() == [1, 0, 0, 1, 1]


def test_kleene_truth_tables(engine):
    """AND / OR / NOT over {T, F, NULL}^2; TRUE spelled as several nonzero values."""
    vals = [(7, 0), (0, 0), (GARBAGE64, 1)]          # T, F, NULL as (value, null byte)
    pairs = [(a, b) for a in vals for b in vals]
    x = np.array([p[0][0] for p in pairs], np.int64)
    xn = np.array([p[0][1] for p in pairs], np.uint8)
    y = np.array([p[1][0] if p[1][0] != 7 else -1 for p in pairs], np.int64)
    yn = np.array([p[1][1] for p in pairs], np.uint8)
    want = check(engine, [("and", A, B), ("or", A, B), ("not", A), ("and", A, B), ("or", A, B)],
                 [XO_I64, XO_I64, XO_I64, XO_MASK, XO_MASK], [x, y], [xn, yn],
                 [PT_I64, PT_I64], 9)
    N = None

    def table(k):
        return [N if nl else int(v) for v, nl in zip(*want[k])]

    assert table(0) == [1, 0, N, 0, 0, 0, N, 0, N]
    assert table(1) == [1, 1, 1, 1, 0, N, 1, N, N]
    assert table(2) == [0, 0, 0, 1, 1, 1, N, N, N]
    assert unpack_mask(want[3][0], 9).tolist() == [v == 1 for v in table(0)]
    assert unpack_mask(want[4][0], 9).tolist() == [v == 1 for v in table(1)]


def test_garbage_under_null_never_leaks(engine):
    """Two uploads that differ ONLY in what is stored under NULL rows give
    identical device outputs, for every op."""
    n = N_POOL
    cols, nulls = make_data(n, 9)
    other = [c.copy() for c in cols]
    other[1][nulls[1] != 0] = 0x33333333
    other[3][nulls[3] != 0] = 0x3333333333333333
    trees = [(k[0], ("col", 1), ("col", 3), *k[3:]) for k in binary_op_trees() if k[0] != "cmp"]
    trees += [("cmp", k[1], ("col", 3), ("col", 1)) for k in binary_op_trees() if k[0] == "cmp"]
    trees += [(k[0], ("col", 3), *k[2:]) for k in unary_op_trees()]
    trees += [("if", ("col", 1), ("col", 3), ("col", 0)), ("if", ("col", 2), ("col", 1), ("col", 3))]
    for batch in batches(trees):
        for t in (XO_I64, XO_MASK):
            types = [t] * len(batch)
            w0 = check(engine, batch, types, cols, nulls, COL_TYPES, n)
            w1 = check(engine, batch, types, other, nulls, COL_TYPES, n)
            for (v0, n0), (v1, n1) in zip(w0, w1):
                assert np.array_equal(v0, v1) and (n0 is None or np.array_equal(n0, n1))


def test_depth_8_stack(engine):
    """a0 - (a1 - (a2 - ... - a7)): all eight slots live, every one distinct,
    so a shift that drops or duplicates a slot changes the value."""
    n = 300
    rng = np.random.default_rng(21)
    cols = [rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64) * (k + 1) for k in range(8)]
    tree = ("col", 7)
    for k in range(6, -1, -1):
        tree = ("-", ("col", k), tree)
    # and nested IFs: three pending (cond, then) pairs under the innermost else
    iff = ("col", 7)
    for k in range(2, -1, -1):
        iff = ("if", ("cmp", ">", ("col", 2 * k), ("const", 0)), ("col", 2 * k + 1), iff)
    program, _ = compile_exprs([tree, iff], [PT_I64] * 8, [False] * 8, [XO_I64, XO_I64])
    assert len(program[0]) == 8 + 7 + 1 + 16 + 1
    want = check(engine, [tree, iff], [XO_I64, XO_I64], cols, [None] * 8, [PT_I64] * 8, n)
    alt = cols[7].copy()
    for k in range(6, -1, -1):
        alt = cols[k] - alt
    assert np.array_equal(want[0][0], alt)


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_stack_depth(engine, depth):
    """The kernel has a 4-slot and an 8-slot instance, chosen by the program's
    deepest point: every depth on both sides of that threshold, as a
    right-nested subtraction and (from depth 3) with an IF as its last operand."""
    n = 200
    rng = np.random.default_rng(depth)
    cols = [rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64) for _ in range(8)]
    tree = ("col", depth - 1)
    for k in range(depth - 2, -1, -1):
        tree = ("-", ("col", k), tree)
    trees = [tree]
    if depth >= 3:
        iff = ("if", ("col", depth - 3), ("col", depth - 2), ("col", depth - 1))
        for k in range(depth - 4, -1, -1):
            iff = ("-", ("col", k), iff)
        trees.append(iff)
    check(engine, trees, [XO_I64] * len(trees), cols, [None] * 8, [PT_I64] * 8, n)


def test_64_instruction_program(engine):
    n = 700
    x = np.arange(n, dtype=np.int32) - 350
    tree = ("+", *[A] * 32)                 # 32 leaves + 31 adds + OUT
    program, _ = compile_exprs([tree], [PT_I32], [False], [XO_I64])
    assert len(program[0]) == EXPR_MAX_INSNS
    want = check(engine, [tree], [XO_I64], [x], [None], [PT_I32], n)
    assert np.array_equal(want[0][0], x.astype(np.int64) * 32)


def test_eight_mixed_outputs_one_column_read_often(engine):
    n = 2 * TILE + 77
    cols, nulls = make_data(n, 17)
    c0, c1, c2, c3 = (("col", k) for k in range(4))
    trees = [("*", c0, c0), ("+", c0, c2), ("cmp", "<", c0, c1), ("cast_i32", ("*", c0, c2)),
             ("is_null", c1), ("ifnull", c3, c0), ("or", ("cmp", ">", c0, ("const", 0)), c1),
             ("case", [(("cmp", "=", c0, ("const", 0)), c2)], c0)]
    types = [XO_I64, XO_I64, XO_MASK, XO_I32, XO_MASK, XO_I64, XO_I32, XO_I32]
    check(engine, trees, types, cols, nulls, COL_TYPES, n)


def test_mask_output_equals_pred_eval_mask_and_feeds_compact(engine):
    n = 3 * TILE + 19
    rng = np.random.default_rng(33)
    a = rng.integers(0, 10, n).astype(np.int32)
    b = rng.integers(-5, 5, n).astype(np.int64)
    bn = (rng.random(n) < 0.3).astype(np.uint8)
    n_words = (n + 63) // 64
    dev = DevCols(engine, [a, b], [None, bn], [PT_I32, PT_I64], n)
    pmask = filled(engine, n_words * 8)
    rid = upload(engine, np.arange(n, dtype=np.uint32))
    o1 = o2 = None
    try:
        got, _ = dev.run([("or", ("cmp", "<", A, ("const", 5)), ("is_null", B))], [XO_MASK])
        pred = compile_predicate(("or", ("cmp", "<", 0, 5), ("is_null", 1)), [PT_I32, PT_I64])
        cnt = engine.pred_eval_mask(dev.in_cols(), pred, n, pmask)
        words = download(pmask, np.uint64, n_words)
        assert np.array_equal(got[0][0], words)       # trailing bits of the last word too
        keep = (a < 5) | (bn != 0)
        assert cnt == int(keep.sum()) and 0 < cnt < n
        emask = upload(engine, got[0][0])
        o1, o2 = engine.alloc(cnt * 4), engine.alloc(cnt * 4)
        assert engine.mask_compact(emask, n, [(rid, o1, 4)]) == cnt
        assert engine.mask_compact(pmask, n, [(rid, o2, 4)]) == cnt
        r1, r2 = download(o1, np.uint32, cnt), download(o2, np.uint32, cnt)
        emask.free()
        assert np.array_equal(r1, r2) and np.array_equal(r1, np.flatnonzero(keep))
    finally:
        dev.close()
        for buf in (pmask, rid, o1, o2):
            if buf is not None:
                buf.free()


# ---- GPUE_ERR_ARG ------------------------------------------------------------
N_ERR = 100


def valid_call(eng):
    """A small valid call; its result proves the session is still usable."""
    x = np.arange(N_ERR, dtype=np.int32) - 50
    want = check(eng, [("*", A, A)], [XO_I64], [x], [None], [PT_I32], N_ERR)
    assert np.array_equal(want[0][0], x.astype(np.int64) ** 2)


def call_raw(eng, program, types, nullable, out_types, has_nulls, n=N_ERR):
    ins = [(eng.alloc(n * 8), eng.alloc(n) if nl else None, t) for t, nl in zip(types, nullable)]
    outs = [(eng.alloc(n * 8), eng.alloc(n) if h else None, t)
            for t, h in zip(out_types, has_nulls)]
    for b, nb, _ in ins:
        b.h2d(np.zeros(n * 8, np.uint8))
        if nb is not None:
            nb.h2d(np.zeros(n, np.uint8))
    try:
        eng.expr_project(ins, program, n, outs)
    finally:
        for b, nb, _ in ins + outs:
            b.free()
            if nb is not None:
                nb.free()


def expect_err_arg(fn):
    with pytest.raises(GpueError) as e:
        fn()
    assert "status 2" in str(e.value), e.value


@pytest.mark.parametrize("case", BAD_PROGRAMS, ids=[c[0] for c in BAD_PROGRAMS])
def test_bad_program_is_err_arg(engine, case):
    _, program, types, nullable, outs, has = case
    expect_err_arg(lambda: call_raw(engine, program, types, nullable, outs, has))
    valid_call(engine)


@pytest.mark.parametrize("case", GOOD_WITHOUT_NULLS, ids=[c[0] for c in GOOD_WITHOUT_NULLS])
def test_no_null_buffer_needed(engine, case):
    _, program, types, nullable, outs, has = case
    call_raw(engine, program, types, nullable, outs, has)


def test_short_buffers_and_row_cap_are_err_arg(engine):
    n = N_ERR
    program, _ = compile_exprs([("/", A, B)], [PT_I32, PT_I64], [False, True], [XO_I64])
    mprog, _ = compile_exprs([A], [PT_I32, PT_I64], [False, True], [XO_MASK])
    full = dict(a=n * 4, b=n * 8, bn=n, out=n * 8, outn=n)

    def call(prog=program, rows=n, out_type=XO_I64, **short):
        sz = {**full, **short}
        bufs = {k: engine.alloc(max(v, 1)) for k, v in sz.items()}
        try:
            engine.expr_project([(bufs["a"], None, PT_I32), (bufs["b"], bufs["bn"], PT_I64)],
                                prog, rows, [(bufs["out"], bufs["outn"], out_type)])
        finally:
            for b in bufs.values():
                b.free()

    call()                                            # the full-size call is fine
    for key in full:
        expect_err_arg(lambda: call(**{key: full[key] - 1}))
    call(prog=mprog, out_type=XO_MASK, out=16)        # 100 rows = 2 mask words
    expect_err_arg(lambda: call(prog=mprog, out_type=XO_MASK, out=15))
    expect_err_arg(lambda: call(rows=1 << 32))
    call(rows=0, a=0, b=0, bn=0, out=0, outn=0)       # n_rows == 0 is GPUE_OK
    valid_call(engine)


def test_aliasing_is_err_arg(engine):
    n = N_ERR
    a, b, an = engine.alloc(n * 8), engine.alloc(n * 8), engine.alloc(n * 8)
    o0, o1, n0, n1 = (engine.alloc(n * 8) for _ in range(4))
    for buf in (a, b, an):
        buf.h2d(np.zeros(n * 8, np.uint8))
    ins = [(a, an, PT_I64), (b, None, PT_I64)]
    program, _ = compile_exprs([("/", A, B), ("%", A, B)], [PT_I64, PT_I64], [True, False],
                               [XO_I64, XO_I64])

    def call(out0, nul0, out1, nul1):
        engine.expr_project(ins, program, n, [(out0, nul0, XO_I64), (out1, nul1, XO_I64)])

    try:
        call(o0, n0, o1, n1)
        for bad in [(a, n0, o1, n1),     # output over an input
                    (o0, b, o1, n1),     # out_null over an input
                    (an, n0, o1, n1),    # output over an input null
                    (o0, an, o1, n1),    # out_null over an input null
                    (o0, n0, o0, n1),    # two outputs, one buffer
                    (o0, n0, o1, n0),    # two out_nulls, one buffer
                    (o0, o0, o1, n1),    # an output and its own out_null
                    (o0, n0, o1, o0)]:   # an out_null over another output
            expect_err_arg(lambda: call(*bad))
        # a sub-range of an input is an overlap too
        part = engine.wrap_ptr_offset(a, 8, n * 8 - 8)
        try:
            expect_err_arg(lambda: engine.expr_project(
                ins, program, n - 1, [(part, n0, XO_I64), (o1, n1, XO_I64)]))
        finally:
            part.free()
        call(o0, n0, o1, n1)
    finally:
        for buf in (a, b, an, o0, o1, n0, n1):
            buf.free()


# ---- random trees ------------------------------------------------------------
RANDOM = random_programs(4242, 50)


@pytest.mark.parametrize("n", [WAVE_RUN + 1, TILE + 65, 5 * TILE + 3])
def test_random_trees(engine, n):
    cols, nulls = make_data(n, n)
    dev = DevCols(engine, cols, nulls, COL_TYPES, n)
    try:
        for trees, out_types in RANDOM:
            program, nullable = compile_exprs(trees, COL_TYPES, COL_NULLABLE, out_types)
            got = dev.run_program(program, nullable, out_types)
            want = run_program(program, cols, nulls, COL_TYPES, out_types, n)
            assert_same(got, want, nullable, trees)
    finally:
        dev.close()


# ---- the one-shot and the operator -------------------------------------------
def test_project_allocates_exact_sizes_and_null_buffers_only_when_nullable(engine):
    n = 1000
    cols, nulls = make_data(n, 2)
    dev = DevCols(engine, cols, nulls, COL_TYPES, n)
    trees = [("*", ("col", 0), ("col", 2)), ("/", ("col", 0), ("col", 2)),
             ("cmp", "<", ("col", 1), ("const", 0)), ("col", 1)]
    types = [XO_I64, XO_I32, XO_MASK, XO_I32]
    outs = engine.project(trees, dev.in_cols(), types, n)
    try:
        assert [nb is not None for _, nb in outs] == [False, True, False, True]
        assert [v.nbytes for v, _ in outs] == [8000, 4000, 128, 4000]
        assert [nb.nbytes for _, nb in outs if nb is not None] == [1000, 1000]
        program, nullable = compile_exprs(trees, COL_TYPES, COL_NULLABLE, types)
        want = run_program(program, cols, nulls, COL_TYPES, types, n)
        got = [(download(v, np.uint64, 16), None) if t == XO_MASK else
               (download(v, OUT_DT[t], n), None if nb is None else download(nb, np.uint8, n))
               for (v, nb), t in zip(outs, types)]
        assert_same(got, want, nullable)
        empty = engine.project([A], [(dev.cols[0], None, PT_I32)], [XO_I64], 0)
        assert empty[0][0].nbytes == 1 and empty[0][1] is None
        empty[0][0].free()
    finally:
        dev.close()
        for v, nb in outs:
            v.free()
            if nb is not None:
                nb.free()
    with pytest.raises(ValueError):
        engine.project([("col", 9)], [], [XO_I64], 0)


def test_project_operator_on_the_device(engine):
    arrays = project_operator_case()
    proj, out, _ = run_project_operator(engine, arrays)
    check_project_operator(out, arrays)
    assert proj.rows == len(arrays[0])
