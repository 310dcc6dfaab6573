"""Scalar expressions without a GPU: the compiler (starrocks_amd/expr.py), its
static nullability, the numpy interpreter run_program against a brute-force
evaluator, and ProjectOperator over a numpy stand-in engine.

The brute-force evaluator (ref_row) recurses over the TREE, one row at a
time, in Python ints with an explicit wrap to int64 — it never sees the
postfix program, so it checks the compiler and the interpreter together.
tests/test_expr_gpu.py reuses the cases, the generator and the bad programs
defined here against the device."""

import os
import re

import numpy as np
import pytest

from starrocks_amd.expr import (EXPR_MAX_IN_COLS, EXPR_MAX_INSNS, EXPR_MAX_OUT,
                                EXPR_MAX_STACK, X_ABS, X_ADD, X_CHECKED, X_COL, X_CONST,
                                X_DIV, X_IF, X_MUL, X_NULL, X_OUT, XO_I32, XO_I64, XO_MASK,
                                compile_exprs, run_program, validate_program)
from starrocks_amd.pipeline import ChunkSourceOperator, Operator, PipelineDriver, ProjectOperator
from starrocks_amd.predicate import PT_I32, PT_I64, pack_mask
from test_topn_cpu import NpBuf

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
GARBAGE64 = 0x5A5A5A5A5A5A5A5A      # what sits under a NULL row of an input
GARBAGE32 = 0x5A5A5A5A
# 3037000500^2 = 2^63 + 1.4e9: the smallest square that overflows
POOL = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX, I32_MIN, I32_MAX, 1 << 31, -(1 << 31) - 1,
        3037000500]
POOL32 = [v for v in POOL if I32_MIN <= v <= I32_MAX]
ARITH = ["+", "-", "*", "/", "%"]
CMPS = ["=", "!=", "<", "<=", ">", ">="]


# ---- brute force ------------------------------------------------------------
def wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _fits(v):
    return I64_MIN <= v <= I64_MAX


def _arith(op, chk, x, y):
    if x is None or y is None:
        return None
    if op in "+-*":
        r = x + y if op == "+" else x - y if op == "-" else x * y
        return None if chk and not _fits(r) else wrap64(r)
    if y == 0:
        return None
    q = abs(x) // abs(y)
    if (x < 0) != (y < 0):
        q = -q
    return wrap64(q) if op == "/" else x - q * y


def _kleene(kind, x, y):
    tx = None if x is None else x != 0
    ty = None if y is None else y != 0
    if kind == "and":
        r = False if (tx is False or ty is False) else None if (tx is None or ty is None) else True
    else:
        r = True if (tx is True or ty is True) else None if (tx is None or ty is None) else False
    return None if r is None else int(r)


def ref_row(node, vals):
    """Value of `node` for one row: a Python int in the int64 range, or None
    for NULL. vals[i] is input column i of the row (None = NULL)."""
    kind, args = node[0], list(node[1:])
    if kind == "col":
        return vals[args[0]]
    if kind == "const":
        return args[0]
    if kind == "null":
        return None
    chk = bool(args) and args[-1] == "checked"
    if chk:
        args.pop()
    if kind in ARITH:
        acc = ref_row(args[0], vals)
        for x in args[1:]:
            acc = _arith(kind, chk, acc, ref_row(x, vals))
        return acc
    if kind in ("neg", "abs"):
        x = ref_row(args[0], vals)
        if x is None:
            return None
        r = -x if kind == "neg" or x < 0 else x
        return None if chk and not _fits(r) else wrap64(r)
    if kind == "cast_i32":
        x = ref_row(args[0], vals)
        return x if x is not None and I32_MIN <= x <= I32_MAX else None
    if kind == "cmp":
        x, y = ref_row(args[1], vals), ref_row(args[2], vals)
        if x is None or y is None:
            return None
        return int({"=": x == y, "==": x == y, "!=": x != y, "<>": x != y, "<": x < y,
                    "<=": x <= y, ">": x > y, ">=": x >= y}[args[0]])
    if kind in ("and", "or"):
        acc = ref_row(args[0], vals)
        if len(args) == 1:
            return acc
        for x in args[1:]:
            acc = _kleene(kind, acc, ref_row(x, vals))
        return acc
    if kind == "not":
        x = ref_row(args[0], vals)
        return None if x is None else int(x == 0)
    if kind == "is_null":
        return int(ref_row(args[0], vals) is None)
    if kind == "if":
        c = ref_row(args[0], vals)
        return ref_row(args[1] if c is not None and c != 0 else args[2], vals)
    if kind == "ifnull":
        x = ref_row(args[0], vals)
        return ref_row(args[1], vals) if x is None else x
    if kind == "case":
        for c, t in args[0]:
            cv = ref_row(c, vals)
            if cv is not None and cv != 0:
                return ref_row(t, vals)
        return None if args[1] is None else ref_row(args[1], vals)
    raise AssertionError(kind)


def ref_outputs(trees, cols, nulls, out_types, n):
    """What the output buffers must hold, by brute force: per output (values
    with 0 under NULL, u8 null flags), or (mask words, None) for XO_MASK."""
    rows = []
    for r in range(n):
        rows.append([None if nulls[i] is not None and nulls[i][r] else int(cols[i][r])
                     for i in range(len(cols))])
    outs = []
    for tree, t in zip(trees, out_types):
        got = [ref_row(tree, vals) for vals in rows]
        isn = np.array([g is None for g in got], bool)
        if t == XO_MASK:
            outs.append((pack_mask(np.array([g is not None and g != 0 for g in got], bool)),
                         None))
            continue
        val = np.array([0 if g is None else g for g in got], np.int64).reshape(n)
        if t == XO_I32:
            val = val.view(np.uint64).astype(np.uint32).view(np.int32)
        outs.append((val, isn.astype(np.uint8)))
    return outs


def assert_outputs_equal(got, want, what=""):
    assert len(got) == len(want)
    for k, ((gv, gn), (wv, wn)) in enumerate(zip(got, want)):
        assert gv.dtype == wv.dtype and np.array_equal(gv, wv), f"{what}: output {k} values"
        if wn is None:
            assert gn is None
        else:
            assert gn is not None and gn.dtype == np.uint8 and np.array_equal(gn, wn), \
                f"{what}: output {k} nulls"


# ---- data -------------------------------------------------------------------
# input columns of the random-tree cases: 0 i32, 1 i32 nullable, 2 i64, 3 i64 nullable
COL_TYPES = [PT_I32, PT_I32, PT_I64, PT_I64]
COL_NULLABLE = [False, True, False, True]


def make_data(n, seed):
    """Adversarial pool values mixed with small ones (so =, / 0 and % -1 hit),
    ~25 % NULL rows in the nullable columns with garbage stored under them."""
    rng = np.random.default_rng(seed)

    def draw(pool):
        small = rng.integers(-3, 4, n)
        pick = np.array(pool, np.int64)[rng.integers(0, len(pool), n)]
        return np.where(rng.random(n) < 0.5, small, pick)

    cols = [draw(POOL32).astype(np.int32), draw(POOL32).astype(np.int32),
            draw(POOL).astype(np.int64), draw(POOL).astype(np.int64)]
    nulls = [None, (rng.random(n) < 0.25).astype(np.uint8), None,
             (rng.random(n) < 0.25).astype(np.uint8)]
    cols[1] = np.where(nulls[1] != 0, np.int32(GARBAGE32), cols[1]).astype(np.int32)
    cols[3] = np.where(nulls[3] != 0, np.int64(GARBAGE64), cols[3]).astype(np.int64)
    return cols, nulls


def pool_cross():
    """Every (x, y) of POOL x POOL as two non-nullable i64 columns."""
    x = np.repeat(np.array(POOL, np.int64), len(POOL))
    y = np.tile(np.array(POOL, np.int64), len(POOL))
    return x, y


def binary_op_trees():
    """Every binary op over (col 0, col 1), checked and unchecked."""
    a, b = ("col", 0), ("col", 1)
    trees = [(op, a, b) for op in ARITH] + [(op, a, b, "checked") for op in "+-*"]
    trees += [("cmp", op, a, b) for op in CMPS]
    trees += [("and", a, b), ("or", a, b), ("ifnull", a, b)]
    return trees


def unary_op_trees():
    a = ("col", 0)
    return [("neg", a), ("neg", a, "checked"), ("abs", a), ("abs", a, "checked"), ("not", a),
            ("is_null", a), ("cast_i32", a), ("if", a, ("const", 7), ("null",))]


def _gen_tree(rng, depth):
    if depth == 0 or rng.random() < 0.2:
        r = rng.random()
        if r < 0.7:
            return ("col", int(rng.integers(0, len(COL_TYPES))))
        if r < 0.95:
            return ("const", int(rng.choice(POOL)) if rng.random() < 0.5
                    else int(rng.integers(-3, 4)))
        return ("null",)
    sub = lambda: _gen_tree(rng, depth - 1)   # noqa: E731
    kind = rng.choice(["arith", "arith", "checked", "unary", "cmp", "logic", "not", "is_null",
                       "if", "ifnull", "case", "cast"])
    if kind == "arith":
        return (str(rng.choice(ARITH)), sub(), sub())
    if kind == "checked":
        if rng.random() < 0.3:
            return (str(rng.choice(["neg", "abs"])), sub(), "checked")
        return (str(rng.choice(["+", "-", "*"])), sub(), sub(), "checked")
    if kind == "unary":
        return (str(rng.choice(["neg", "abs"])), sub())
    if kind == "cmp":
        return ("cmp", str(rng.choice(CMPS)), sub(), sub())
    if kind == "logic":
        return (str(rng.choice(["and", "or"])), *[sub() for _ in range(rng.integers(2, 4))])
    if kind == "not":
        return ("not", sub())
    if kind == "is_null":
        return ("is_null", sub())
    if kind == "if":
        return ("if", sub(), sub(), sub())
    if kind == "ifnull":
        return ("ifnull", sub(), sub())
    if kind == "case":
        return ("case", [(sub(), sub()) for _ in range(rng.integers(1, 3))],
                None if rng.random() < 0.4 else sub())
    return ("cast_i32", sub())


def random_programs(seed, count):
    """`count` x (trees, out_types): 1-3 trees of depth <= 4 each, every output
    type. A draw the caps reject (stack 8, 64 instructions) is drawn again."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        trees = [_gen_tree(rng, int(rng.integers(1, 5))) for _ in range(rng.integers(1, 4))]
        out_types = [int(rng.choice([XO_I32, XO_I64, XO_MASK])) for _ in trees]
        try:
            compile_exprs(trees, COL_TYPES, COL_NULLABLE, out_types)
        except ValueError:
            continue
        out.append((trees, out_types))
    return out


def run_trees(trees, cols, nulls, types, out_types, n):
    program, nullable = compile_exprs(trees, types, [x is not None for x in nulls], out_types)
    return run_program(program, cols, nulls, types, out_types, n), nullable


# ---- programs the C-ABI must reject ------------------------------------------
def _prog(insns):
    return (np.array([i[0] for i in insns], np.int32), np.array([i[1] for i in insns], np.int32),
            np.array([i[2] for i in insns], np.int64))


def _bad_programs():
    """(label, program, col_types, col_nullable, out_types, out_has_nulls), one
    or more per GPUE_ERR_ARG class a program can hit."""
    C0, C1, OUT0 = (X_COL, 0, 0), (X_COL, 1, 0), (X_OUT, 0, 0)
    two, nn, o64, yes = [PT_I32, PT_I64], [False, False], [XO_I64], [True]
    bad = []

    def add(label, insns, types=two, nullable=nn, outs=o64, has=None):
        bad.append((label, _prog(insns), types, nullable, outs,
                    [True] * len(outs) if has is None else has))

    add("no instructions", [])
    add("65 instructions", [C0] + [(X_ABS, 0, 0)] * 63 + [OUT0])
    add("no outputs", [C0, OUT0], outs=[], has=[])
    add("9 outputs", [x for k in range(9) for x in (C0, (X_OUT, k, 0))], outs=[XO_I64] * 9)
    add("65 input columns", [C0, OUT0], types=[PT_I32] * 65, nullable=[False] * 65)
    add("unknown op (a predicate op)", [C0, (0, 0, 0), OUT0])
    add("unknown op 99", [C0, (99, 0, 0), OUT0])
    add("unknown flag", [C0, C1, (X_ADD | 0x100, 0, 0), OUT0])
    add("CHECKED on DIV", [C0, C1, (X_DIV | X_CHECKED, 0, 0), OUT0])
    add("CHECKED on COL", [(X_COL | X_CHECKED, 0, 0), OUT0])
    add("underflow: binary on one value", [C0, (X_ADD, 0, 0), OUT0])
    add("underflow: IF on two values", [C0, C1, (X_IF, 0, 0), OUT0])
    add("underflow: OUT on nothing", [C0, OUT0, (X_OUT, 1, 0)], outs=[XO_I64] * 2)
    add("stack overflow", [C0] * 9 + [(X_ADD, 0, 0)] * 8 + [OUT0])
    add("non-empty stack at OUT", [C0, C1, OUT0])
    add("does not end with OUT", [C0, OUT0, C1])
    add("output written twice", [C0, OUT0, C1, OUT0])
    add("output never written", [C0, OUT0], outs=[XO_I64] * 2)
    add("column index -1", [(X_COL, -1, 0), OUT0])
    add("column index past the end", [(X_COL, 2, 0), OUT0])
    add("output index -1", [C0, (X_OUT, -1, 0)])
    add("output index past the end", [C0, (X_OUT, 1, 0)])
    add("unknown input type", [C0, OUT0], types=[2, PT_I64])
    add("unknown output type", [C0, OUT0], outs=[3])
    add("nullable column, no null buffer", [C0, OUT0], nullable=[True, False], has=[False])
    add("DIV, no null buffer", [C0, C1, (X_DIV, 0, 0), OUT0], has=[False])
    add("NULL literal, no null buffer", [(X_NULL, 0, 0), OUT0], outs=[XO_I32], has=[False])
    add("checked MUL, no null buffer", [C0, C1, (X_MUL | X_CHECKED, 0, 0), OUT0], has=[False])
    return bad


BAD_PROGRAMS = _bad_programs()
# the same without a null buffer is fine when the output is a MASK, or not nullable
GOOD_WITHOUT_NULLS = [
    ("nullable into MASK", _prog([(X_COL, 0, 0), (X_OUT, 0, 0)]), [PT_I32, PT_I64],
     [True, False], [XO_MASK], [False]),
    ("non-nullable into I64", _prog([(X_COL, 0, 0), (X_CONST, 0, 3), (X_ADD, 0, 0),
                                     (X_OUT, 0, 0)]), [PT_I32, PT_I64], [False, False],
     [XO_I64], [False]),
]


@pytest.mark.parametrize("case", BAD_PROGRAMS, ids=[c[0] for c in BAD_PROGRAMS])
def test_validate_rejects(case):
    _, program, types, nullable, outs, has = case
    with pytest.raises(ValueError):
        validate_program(program, types, nullable, outs, has)


@pytest.mark.parametrize("case", GOOD_WITHOUT_NULLS, ids=[c[0] for c in GOOD_WITHOUT_NULLS])
def test_validate_accepts_without_null_buffer(case):
    _, program, types, nullable, outs, has = case
    validate_program(program, types, nullable, outs, has)


A, B = ("col", 0), ("col", 1)
BAD_TREES = [
    ("column out of range", [("col", 4)]),
    ("negative column", [("col", -1)]),
    ("bool column", [("col", True)]),
    ("unknown node", [("pow", A, B)]),
    ("not a node", [5]),
    ("float constant", [("const", 1.5)]),
    ("constant past int64", [("const", 1 << 63)]),
    ("checked division", [("/", A, B, "checked")]),
    ("unknown modifier", [("+", A, B, "saturating")]),
    ("one-operand plus", [("+", A)]),
    ("unknown compare", [("cmp", "~", A, B)]),
    ("if with two operands", [("if", A, B)]),
    ("case without arms", [("case", [], A)]),
    ("null with an operand", [("null", A)]),
    # right-nested: every level holds one more value -> depth 9
    ("stack depth 9", [("+", A, ("+", A, ("+", A, ("+", A, ("+", A, ("+", A, ("+", A,
                       ("+", A, B))))))))]),
    ("65 instructions", [("+", *[A] * 32)] + [A]),          # 63 + OUT, then 2 more
    ("nine outputs", [A] * 9),
    ("no outputs", []),
]


@pytest.mark.parametrize("case", BAD_TREES, ids=[c[0] for c in BAD_TREES])
def test_compile_rejects(case):
    trees = case[1]
    with pytest.raises(ValueError):
        compile_exprs(trees, COL_TYPES, COL_NULLABLE, [XO_I64] * len(trees))


def test_compile_rejects_bad_types():
    with pytest.raises(ValueError):
        compile_exprs([A], [PT_I32, 7], [False, False], [XO_I64])
    with pytest.raises(ValueError):
        compile_exprs([A], [PT_I32], [False], [5])
    with pytest.raises(ValueError):
        compile_exprs([A], [PT_I32], [False], [XO_I64, XO_I64])     # output 1 never written


def test_compile_shapes():
    """Left fold, operand order, CASE lowering and the caps' exact edges."""
    (op, col, a), nullable = compile_exprs([("-", A, B, ("const", 5))], COL_TYPES,
                                           COL_NULLABLE, [XO_I64])
    assert list(op) == [32, 32, 49, 33, 49, 68] and list(col[:2]) == [0, 1] and a[3] == 5
    assert nullable == [True]
    (op, _, _), _ = compile_exprs([("case", [(A, B), (B, A)], None)], COL_TYPES, COL_NULLABLE,
                                  [XO_I64])
    assert list(op) == [32, 32, 32, 32, 34, 66, 66, 68]
    # depth exactly 8 and exactly 64 instructions compile
    deep = B
    for _ in range(7):
        deep = ("+", A, deep)
    compile_exprs([deep], COL_TYPES, COL_NULLABLE, [XO_I64])
    (op, _, _), _ = compile_exprs([("+", *[A] * 32)], COL_TYPES, COL_NULLABLE, [XO_I64])
    assert len(op) == EXPR_MAX_INSNS
    compile_exprs([A] * EXPR_MAX_OUT, COL_TYPES, COL_NULLABLE, [XO_I64] * EXPR_MAX_OUT)
    assert (EXPR_MAX_STACK, EXPR_MAX_OUT, EXPR_MAX_IN_COLS) == (8, 8, 64)


def test_static_nullability():
    N, Q = ("col", 0), ("col", 1)       # not nullable, nullable
    rules = [
        (N, False), (Q, True), (("const", 1), False), (("null",), True),
        (("+", N, N), False), (("+", N, Q), True), (("+", Q, N), True),
        (("+", N, N, "checked"), True), (("-", N, N, "checked"), True),
        (("*", N, N, "checked"), True), (("*", N, N), False),
        (("/", N, N), True), (("%", N, N), True),
        (("neg", N), False), (("neg", N, "checked"), True), (("neg", Q), True),
        (("abs", N), False), (("abs", N, "checked"), True),
        (("cast_i32", N), True), (("not", N), False), (("not", Q), True),
        (("is_null", Q), False), (("is_null", ("null",)), False),
        (("cmp", "<", N, N), False), (("cmp", "<", N, Q), True),
        (("and", N, N), False), (("and", N, Q), True), (("or", Q, N), True),
        (("ifnull", Q, N), False), (("ifnull", N, Q), True), (("ifnull", Q, Q), True),
        (("if", Q, N, N), False), (("if", N, Q, N), True), (("if", N, N, Q), True),
        (("case", [(N, N)], None), True), (("case", [(Q, N)], N), False),
        (("case", [(N, N), (N, Q)], N), True),
    ]
    for tree, want in rules:
        _, nullable = compile_exprs([tree], [PT_I64, PT_I64], [False, True], [XO_I64])
        assert nullable == [want], tree


def test_header_and_binding_agree():
    """gpue.h's numbers are the compiler's; the X ops are disjoint from the
    predicate ops; the binding exists."""
    import starrocks_amd.expr as ex
    import starrocks_amd.predicate as pr
    code = open(os.path.join(REPO_ROOT, "include", "gpue.h")).read()
    x_vals = set()
    for name, val in re.findall(r"#define\s+GPUE_(XO?_\w+|EXPR_\w+)\s+(\w+)", code):
        assert getattr(ex, name) == int(val, 0), name
        if name.startswith("X_"):
            x_vals.add(int(val, 0))
    assert len(x_vals) == 25
    p_vals = {int(v, 0) for _, v in re.findall(r"#define\s+GPUE_(P_\w+)\s+(\w+)", code)}
    assert p_vals and not (x_vals & p_vals)
    assert not any(v & pr.P_RHS_COL for v in x_vals if v != X_CHECKED)
    from starrocks_amd import engine as eng_mod
    for name in ("expr_project", "project"):
        assert callable(getattr(eng_mod.Engine, name, None)), name
    lib = os.path.join(REPO_ROOT, "starrocks_amd", "libgpue.so")
    if os.path.exists(lib):
        import ctypes
        cdll = ctypes.CDLL(lib)
        eng_mod._declare(cdll)
        assert len(cdll.gpue_expr_project.argtypes) == 14


# ---- run_program against brute force -----------------------------------------
def test_binary_ops_over_the_pool():
    x, y = pool_cross()
    n = len(x)
    for tree in binary_op_trees():
        for t in (XO_I64, XO_I32, XO_MASK):
            got, _ = run_trees([tree], [x, y], [None, None], [PT_I64, PT_I64], [t], n)
            assert_outputs_equal(got, ref_outputs([tree], [x, y], [None, None], [t], n), tree)


def test_binary_ops_with_null_operands():
    x, y = pool_cross()
    n = len(x)
    xn = (np.arange(n) % 3 == 0).astype(np.uint8)
    yn = (np.arange(n) % 5 == 0).astype(np.uint8)
    xg = np.where(xn != 0, np.int64(GARBAGE64), x)
    yg = np.where(yn != 0, np.int64(GARBAGE64), y)
    for tree in binary_op_trees():
        got, nullable = run_trees([tree], [xg, yg], [xn, yn], [PT_I64, PT_I64], [XO_I64], n)
        assert nullable == [True]
        assert_outputs_equal(got, ref_outputs([tree], [xg, yg], [xn, yn], [XO_I64], n), tree)


def test_unary_ops_over_the_pool():
    x = np.array(POOL, np.int64)
    xn = np.zeros(len(x), np.uint8)
    xn[3] = 1
    for nulls in ([None], [xn]):
        for tree in unary_op_trees():
            got, _ = run_trees([tree], [x], nulls, [PT_I64], [XO_I64], len(x))
            assert_outputs_equal(got, ref_outputs([tree], [x], nulls, [XO_I64], len(x)), tree)


def test_spelled_out_edges():
    """The header's special cases, as literals rather than via ref_row."""
    def one(tree, x, y=0):
        got, _ = run_trees([tree], [np.array([x], np.int64), np.array([y], np.int64)],
                           [None, None], [PT_I64, PT_I64], [XO_I64], 1)
        return None if got[0][1][0] else int(got[0][0][0])

    assert one(("/", A, B), I64_MIN, -1) == I64_MIN
    assert one(("%", A, B), I64_MIN, -1) == 0
    assert one(("/", A, B), -7, 2) == -3 and one(("%", A, B), -7, 2) == -1
    assert one(("/", A, B), 7, -2) == -3 and one(("%", A, B), 7, -2) == 1
    assert one(("/", A, B), 5, 0) is None and one(("%", A, B), 5, 0) is None
    assert one(("+", A, B), I64_MAX, 1) == I64_MIN
    assert one(("+", A, B, "checked"), I64_MAX, 1) is None
    assert one(("*", A, B), 3037000500, 3037000500) == wrap64(3037000500 ** 2)
    assert one(("*", A, B, "checked"), 3037000500, 3037000500) is None
    assert one(("*", A, B, "checked"), 3037000499, 3037000499) == 3037000499 ** 2
    assert one(("*", A, B, "checked"), I64_MIN, -1) is None
    assert one(("*", A, B, "checked"), -1, I64_MIN) is None
    assert one(("neg", A), I64_MIN) == I64_MIN and one(("neg", A, "checked"), I64_MIN) is None
    assert one(("abs", A), I64_MIN) == I64_MIN and one(("abs", A, "checked"), I64_MIN) is None
    assert one(("cast_i32", A), I32_MAX) == I32_MAX and one(("cast_i32", A), 1 << 31) is None
    assert one(("cast_i32", A), I32_MIN) == I32_MIN
    assert one(("cast_i32", A), -(1 << 31) - 1) is None
    assert one(("if", ("null",), A, B), 1, 2) == 2
    assert one(("and", ("null",), A), 0) == 0 and one(("and", ("null",), A), 5) is None
    assert one(("or", ("null",), A), 5) == 1 and one(("or", ("null",), A), 0) is None


def test_i32_columns_sign_extend_and_i32_outputs_truncate():
    x = np.array(POOL32, np.int32)
    got, _ = run_trees([("*", A, A), A, ("+", A, ("const", 1 << 32))], [x], [None], [PT_I32],
                       [XO_I64, XO_I64, XO_I32], len(x))
    assert np.array_equal(got[0][0], x.astype(np.int64) * x.astype(np.int64))
    assert np.array_equal(got[1][0], x.astype(np.int64))
    assert np.array_equal(got[2][0], x)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_trees_against_brute_force(seed):
    n = 257
    cols, nulls = make_data(n, seed)
    for trees, out_types in random_programs(seed, 60):
        got, _ = run_trees(trees, cols, nulls, COL_TYPES, out_types, n)
        assert_outputs_equal(got, ref_outputs(trees, cols, nulls, out_types, n), trees)


def test_random_programs_reach_every_op():
    seen = set()
    for trees, out_types in random_programs(11, 60):
        (op, _, _), _ = compile_exprs(trees, COL_TYPES, COL_NULLABLE, out_types)
        seen |= {int(o) for o in op}
    import starrocks_amd.expr as ex
    every = {getattr(ex, k) for k in dir(ex) if k.startswith("X_") and k != "X_CHECKED"}
    assert every <= seen
    assert any(o & X_CHECKED for o in seen)


def test_run_program_rejects_a_column_of_the_wrong_dtype():
    program, _ = compile_exprs([A], [PT_I32], [False], [XO_I64])
    with pytest.raises(ValueError):
        run_program(program, [np.zeros(4, np.int64)], [None], [PT_I32], [XO_I64], 4)


# ---- ProjectOperator against a numpy stand-in engine --------------------------
class NpProjectEngine:
    """Just what ProjectOperator may call: alloc and expr_project."""
    DT = {PT_I32: np.int32, PT_I64: np.int64}

    def __init__(self):
        self.bufs = []

    def alloc(self, nbytes):
        assert nbytes > 0
        self.bufs.append(NpBuf(nbytes))
        return self.bufs[-1]

    def expr_project(self, in_cols, program, n_rows, outs):
        cols = [c.view(self.DT[t], n_rows) for c, _, t in in_cols]
        nulls = [None if nl is None else nl.view(np.uint8, n_rows) for _, nl, _ in in_cols]
        validate_program(program, [t for _, _, t in in_cols], [x is not None for x in nulls],
                         [t for _, _, t in outs], [nl is not None for _, nl, _ in outs])
        res = run_program(program, cols, nulls, [t for _, _, t in in_cols],
                          [t for _, _, t in outs], n_rows)
        for (buf, nbuf, _), (val, isn) in zip(outs, res):
            assert buf.nbytes >= val.nbytes
            if val.nbytes:
                buf.h2d(val)
            if nbuf is not None and n_rows:
                nbuf.h2d(isn)


# chunk columns: 0 ep int32, 1 dc int32 (nullable), 2 dc's u8 null mask, 3 row id int64
OP_CHUNKS = [1000, 0, 1, 129]        # multi-tile, EMPTY, single row, ragged
OP_MAP = [(0, None, PT_I32), (1, 2, PT_I32), (3, None, PT_I64)]
OP_TREES = [("*", A, B), ("case", [(("cmp", "<", A, ("const", 0)), ("neg", A))], A),
            ("or", ("is_null", B), ("cmp", ">", ("col", 2), ("const", 500)))]
OP_OUT_TYPES = [XO_I64, XO_I32, XO_MASK]
OP_KEEP = [3, 0]


def project_operator_case():
    n = sum(OP_CHUNKS)
    rng = np.random.default_rng(5)
    ep = rng.integers(-1000, 1000, n).astype(np.int32)
    dc_null = (rng.random(n) < 0.3).astype(np.uint8)
    dc = np.where(dc_null != 0, np.int32(GARBAGE32), rng.integers(0, 11, n)).astype(np.int32)
    rid = np.arange(n, dtype=np.int64)
    return ep, dc, dc_null, rid


class CollectSink(Operator):
    def __init__(self):
        super().__init__()
        self.chunks = []

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def push_chunk(self, chunk):
        self.chunks.append(chunk)

    def result(self):
        return self.chunks


def run_project_operator(engine, arrays):
    """Drive the case through PipelineDriver([source, ProjectOperator, sink]);
    returns (operator, per chunk (n, [numpy array per output chunk column]),
    the buffers the source handed out)."""
    starts = np.concatenate([[0], np.cumsum(OP_CHUNKS)])
    pushed = []

    def gen(ordinal, _one):
        lo, n = int(starts[ordinal]), OP_CHUNKS[ordinal]
        cols = []
        for arr in arrays:
            buf = engine.alloc(max(n * arr.itemsize, 1))
            if n:
                buf.h2d(arr[lo:lo + n])
            cols.append(buf)
        pushed.append(cols)
        return {"n": n, "cols": cols}

    proj = ProjectOperator(engine, OP_TREES, OP_MAP, OP_OUT_TYPES, OP_KEEP)
    chunks = PipelineDriver([ChunkSourceOperator(gen, len(OP_CHUNKS), 1), proj,
                             CollectSink()]).process()
    assert len(chunks) == len(OP_CHUNKS)
    # kept: rid i64, ep i32; then ep*dc i64 + nulls, |ep| i32, mask words
    dtypes = [np.int64, np.int32, np.int64, np.uint8, np.int32, np.uint64]
    assert proj.nullable == [True, False, False] and proj.out_widths == [8, 1, 4, 8]
    out = []
    for c in chunks:
        n = c["n"]
        assert len(c["cols"]) == len(dtypes)
        counts = [n, n, n, n, n, (n + 63) // 64]
        out.append((n, [b.d2h(dt, k) if k else np.empty(0, dt)
                        for b, dt, k in zip(c["cols"], dtypes, counts)]))
        for b in c["cols"]:
            b.free()
    return proj, out, pushed


def check_project_operator(out, arrays):
    ep, dc, dc_null, rid = arrays
    starts = np.concatenate([[0], np.cumsum(OP_CHUNKS)])
    for (n, cols), lo, want_n in zip(out, starts, OP_CHUNKS):
        assert n == want_n
        sl = slice(int(lo), int(lo) + n)
        want = ref_outputs(OP_TREES, [ep[sl], dc[sl], rid[sl]], [None, dc_null[sl], None],
                           OP_OUT_TYPES, n)
        assert np.array_equal(cols[0], rid[sl]) and np.array_equal(cols[1], ep[sl])
        assert np.array_equal(cols[2], want[0][0]) and np.array_equal(cols[3], want[0][1])
        assert np.array_equal(cols[4], want[1][0]) and np.array_equal(cols[4], np.abs(ep[sl]))
        assert np.array_equal(cols[5], want[2][0])


def test_project_operator_against_numpy_engine():
    arrays = project_operator_case()
    eng = NpProjectEngine()
    proj, out, pushed = run_project_operator(eng, arrays)
    check_project_operator(out, arrays)
    assert proj.rows == sum(OP_CHUNKS)
    assert all(b.freed for b in eng.bufs), "operator leaked a buffer"
    # kept columns (3, 0) travel on; the others were freed by the operator itself
    # (the collector above freed the kept ones afterwards)
    assert all(b.freed for cols in pushed for b in cols)


def test_project_operator_frees_what_it_does_not_keep():
    eng = NpProjectEngine()
    proj = ProjectOperator(eng, OP_TREES, OP_MAP, OP_OUT_TYPES, OP_KEEP)
    arrays = project_operator_case()
    cols = []
    for arr in arrays:
        cols.append(eng.alloc(4 * arr.itemsize))
        cols[-1].h2d(arr[:4])
    proj.push_chunk({"n": 4, "cols": cols})
    assert [b.freed for b in cols] == [False, True, True, False]
    out = proj.pull_chunk()
    assert out["cols"][0] is cols[3] and out["cols"][1] is cols[0]


def test_project_operator_rejects_bad_bindings():
    eng = NpProjectEngine()
    with pytest.raises(ValueError):
        ProjectOperator(eng, [("col", 3)], OP_MAP, [XO_I64], [])            # tree col unbound
    with pytest.raises(ValueError):
        ProjectOperator(eng, OP_TREES, OP_MAP, OP_OUT_TYPES, [0, 0])        # keep twice
    with pytest.raises(ValueError):
        ProjectOperator(eng, OP_TREES, OP_MAP, [XO_I64, XO_I32], OP_KEEP)   # 3 trees, 2 types
