"""Predicate expressions, the GPU-less part: compile_predicate / run_program
(starrocks_amd/predicate.py) against an independent recursive evaluator, the
Kleene tables, every ValueError, and FilterOperator against a numpy stand-in
engine.

The reference (also imported by tests/test_filter_expr.py) is ref_eval: it
walks the nested-tuple tree itself — it never sees the postfix program — and
returns the (is TRUE, is FALSE) row arrays of SQL three-valued logic; a row
passes the filter iff the root is TRUE."""

import os
import re

import numpy as np
import pytest

from starrocks_amd.predicate import (PRED_MAX_INSNS, PRED_MAX_STACK, PT_I32, PT_I64,
                                     P_AND, P_BETWEEN, P_EQ, P_IN, P_NOT, P_RHS_COL,
                                     compile_predicate, pack_mask, run_program,
                                     unpack_mask, validate_program)
from starrocks_amd.pipeline import ChunkSourceOperator, FilterOperator, Operator, PipelineDriver
from test_topn_cpu import NpBuf

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# the random-tree schema: 2 I32 + 2 I64 predicate columns, columns 1 and 3 nullable
COL_TYPES = [PT_I32, PT_I32, PT_I64, PT_I64]
NULLABLE = [False, True, False, True]
DTYPES = [np.int32, np.int32, np.int64, np.int64]


# ---- the reference: a recursive evaluator over the tree --------------------
def ref_eval(tree, cols, nulls, n):
    kind = tree[0]
    if kind == "and":
        t_all, f_any = np.ones(n, bool), np.zeros(n, bool)
        for x in tree[1:]:
            t, f = ref_eval(x, cols, nulls, n)
            t_all, f_any = t_all & t, f_any | f
        return t_all, f_any
    if kind == "or":
        t_any, f_all = np.zeros(n, bool), np.ones(n, bool)
        for x in tree[1:]:
            t, f = ref_eval(x, cols, nulls, n)
            t_any, f_all = t_any | t, f_all & f
        return t_any, f_all
    if kind == "not":
        t, f = ref_eval(tree[1], cols, nulls, n)
        return f, t

    def side(c):
        isn = np.zeros(n, bool) if nulls[c] is None else np.asarray(nulls[c])[:n] != 0
        return np.asarray(cols[c])[:n].astype(np.int64), isn  # int32 sign-extends

    if kind == "is_null":
        isn = side(tree[1])[1]
        return isn, ~isn
    if kind in ("cmp", "cmp_col"):
        v, isn = side(tree[2])
        if kind == "cmp":
            w = np.int64(tree[3])
        else:
            w, isn2 = side(tree[3])
            isn = isn | isn2
        r = {"=": v == w, "==": v == w, "!=": v != w, "<>": v != w, "<": v < w,
             "<=": v <= w, ">": v > w, ">=": v >= w}[tree[1]]
    elif kind == "between":
        v, isn = side(tree[1])
        r = (v >= np.int64(tree[2])) & (v <= np.int64(tree[3]))
    elif kind == "in":
        v, isn = side(tree[1])
        vals = np.unique(np.array(list(tree[2]), np.int64))
        if len(vals):
            at = np.minimum(np.searchsorted(vals, v), len(vals) - 1)
            r = vals[at] == v
        else:
            r = np.zeros(n, bool)
    else:
        raise AssertionError(kind)
    return r & ~isn, ~r & ~isn


# ---- seeded data and trees, shared with the GPU test -----------------------
def make_data(n, seed, garbage_seed=0):
    """(cols, nulls) for the schema above: small values so predicates hit,
    ~6% type extremes, ~25% NULL rows on the nullable columns with random
    garbage stored under them (garbage_seed changes only that garbage)."""
    rng = np.random.default_rng(seed)
    grng = np.random.default_rng(1000 + garbage_seed)
    cols, nulls = [], []
    for dt, nullable in zip(DTYPES, NULLABLE):
        info = np.iinfo(dt)
        v = rng.integers(-6, 7, n).astype(dt)
        ext = rng.random(n)
        v[ext < 0.03] = info.min
        v[ext > 0.97] = info.max
        nl = None
        if nullable:
            nl = (rng.random(n) < 0.25).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
            g = grng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
            v = np.where(nl != 0, g, v).astype(dt)
        cols.append(v)
        nulls.append(nl)
    return cols, nulls


CONST_POOL = [-7, -6, -3, -1, 0, 1, 2, 5, 6, 7, I32_MIN, I32_MAX, I32_MIN - 1, I32_MAX + 1,
              1 << 40, -(1 << 40), I64_MIN, I64_MAX]


def count_insns(tree):
    if tree[0] in ("and", "or"):
        return sum(count_insns(x) for x in tree[1:]) + len(tree) - 2
    if tree[0] == "not":
        return 1 + count_insns(tree[1])
    return 1


def _random_leaf(rng):
    k = rng.integers(0, 10)
    c = int(rng.integers(0, 4))
    const = lambda: int(CONST_POOL[rng.integers(0, len(CONST_POOL))])
    op = ["=", "!=", "<", "<=", ">", ">="][rng.integers(0, 6)]
    if k < 4:
        return ("cmp", op, c, const())
    if k < 6:
        return ("cmp_col", op, c, [1, 0, 3, 2, 0, 1, 2, 3][c + 4 * int(rng.integers(0, 2))])
    if k < 7:
        lo, hi = sorted((const(), const()))
        return ("between", c, lo, hi) if rng.random() < 0.8 else ("between", c, hi, lo)
    if k < 9:
        return ("in", c, [const() for _ in range(int(rng.integers(0, 7)))])
    return ("is_null", c)


def _random_tree(rng, depth):
    if depth == 0 or rng.random() < 0.25:
        return _random_leaf(rng)
    k = rng.integers(0, 5)
    if k == 0:
        return ("not", _random_tree(rng, depth - 1))
    kids = [_random_tree(rng, depth - 1) for _ in range(int(rng.integers(2, 4)))]
    return ("and" if k < 3 else "or", *kids)


def random_trees(count, seed=7, max_depth=5):
    """`count` seeded trees of depth <= max_depth that fit one program."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        t = _random_tree(rng, int(rng.integers(1, max_depth + 1)))
        if count_insns(t) <= PRED_MAX_INSNS:
            out.append(t)
    return out


N_RANDOM_TREES = 320


# ---- compiler + interpreter vs the reference -------------------------------
def test_random_trees_match_recursive_reference():
    n = 1500
    cols, nulls = make_data(n, seed=11)
    trees = random_trees(N_RANDOM_TREES)
    assert len(trees) >= 300
    kinds, deepest, any_true, any_unknown = set(), 0, 0, 0
    for tree in trees:
        prog = compile_predicate(tree, COL_TYPES)
        assert len(prog[0]) == count_insns(tree)
        t, f = run_program(prog, cols, nulls, COL_TYPES, n)
        et, ef = ref_eval(tree, cols, nulls, n)
        assert np.array_equal(t, et) and np.array_equal(f, ef), tree
        assert not (t & f).any()
        kinds.update(int(o) & ~P_RHS_COL for o in prog[0])
        deepest = max(deepest, len(prog[0]))
        any_true += bool(t.any() and not t.all())
        any_unknown += bool((~t & ~f).any())
    # the sample exercises every op, long programs, and mixed / UNKNOWN outcomes
    assert kinds == set(range(9)) | {16, 17, 18}
    assert deepest > 30 and any_true > 100 and any_unknown > 100


def _truth_cols():
    """Two nullable I32 columns whose 9 rows are every (x, y) pair over
    T / F / U for x = (col0 = 1), y = (col1 = 1): 1 -> T, 0 -> F, NULL -> U."""
    vals = {"T": (1, 0), "F": (0, 0), "U": (77, 1)}  # 77: garbage under the NULL
    xs = [a for a in "TFU" for _ in "TFU"]
    ys = [b for _ in "TFU" for b in "TFU"]
    cols = [np.array([vals[k][0] for k in s], np.int32) for s in (xs, ys)]
    nulls = [np.array([vals[k][1] for k in s], np.uint8) for s in (xs, ys)]
    return xs, ys, cols, nulls


KLEENE_AND = {("T", "T"): "T", ("T", "F"): "F", ("T", "U"): "U", ("F", "T"): "F",
              ("F", "F"): "F", ("F", "U"): "F", ("U", "T"): "U", ("U", "F"): "F",
              ("U", "U"): "U"}
KLEENE_OR = {("T", "T"): "T", ("T", "F"): "T", ("T", "U"): "T", ("F", "T"): "T",
             ("F", "F"): "F", ("F", "U"): "U", ("U", "T"): "T", ("U", "F"): "U",
             ("U", "U"): "U"}
KLEENE_NOT = {"T": "F", "F": "T", "U": "U"}


def truth_letters(t, f):
    return ["T" if a else "F" if b else "U" for a, b in zip(t, f)]


def kleene_cases():
    """[(tree, expected T/F/U letter per row)] over _truth_cols()."""
    xs, ys, _, _ = _truth_cols()
    x, y = ("cmp", "=", 0, 1), ("cmp", "=", 1, 1)
    return [(("and", x, y), [KLEENE_AND[p] for p in zip(xs, ys)]),
            (("or", x, y), [KLEENE_OR[p] for p in zip(xs, ys)]),
            (("not", x), [KLEENE_NOT[a] for a in xs]),
            (("not", ("and", x, y)), [KLEENE_NOT[KLEENE_AND[p]] for p in zip(xs, ys)]),
            (("not", ("or", x, y)), [KLEENE_NOT[KLEENE_OR[p]] for p in zip(xs, ys)])]


def test_kleene_tables_exhaustive():
    _, _, cols, nulls = _truth_cols()
    for tree, expect in kleene_cases():
        prog = compile_predicate(tree, [PT_I32, PT_I32])
        assert truth_letters(*run_program(prog, cols, nulls, [PT_I32, PT_I32], 9)) == expect
        assert truth_letters(*ref_eval(tree, cols, nulls, 9)) == expect


def test_leaf_semantics_by_hand():
    c32 = np.array([I32_MIN, -1, 0, 5, I32_MAX], np.int32)
    nl = np.array([0, 0, 9, 0, 0], np.uint8)
    run = lambda tree, nulls=(None,): truth_letters(*run_program(
        compile_predicate(tree, [PT_I32]), [c32], list(nulls), [PT_I32], 5))
    # int32 sign-extends and compares as int64: a constant outside int32 is legal
    assert run(("cmp", "<", 0, 1 << 40)) == list("TTTTT")
    assert run(("cmp", ">", 0, -(1 << 40))) == list("TTTTT")
    assert run(("cmp", "=", 0, I32_MAX + 1)) == list("FFFFF")
    assert run(("cmp", ">=", 0, I32_MIN)) == list("TTTTT")
    assert run(("cmp", "<", 0, 0), [nl]) == list("TTUFF")
    assert run(("between", 0, -1, 5), [nl]) == list("FTUTF")
    assert run(("in", 0, []), [nl]) == list("FFUFF")                  # empty IN
    assert run(("not", ("in", 0, [5, I32_MIN])), [nl]) == list("FTUFT")  # NOT IN drops NULLs
    assert run(("is_null", 0), [nl]) == list("FFTFF")                 # never UNKNOWN
    assert run(("is_null", 0)) == list("FFFFF")                       # no mask: FALSE
    assert run(("cmp_col", "<=", 0, 0), [nl]) == list("TTUTT")


def test_garbage_under_nulls_never_changes_a_result():
    n = 800
    ca, nulls = make_data(n, seed=5, garbage_seed=1)
    cb, nulls_b = make_data(n, seed=5, garbage_seed=2)
    assert all(np.array_equal(x, y) for x, y in zip(nulls[1::2], nulls_b[1::2]))
    assert not np.array_equal(ca[1], cb[1]) and not np.array_equal(ca[3], cb[3])
    for tree in random_trees(120, seed=3):
        prog = compile_predicate(tree, COL_TYPES)
        ta, fa = run_program(prog, ca, nulls, COL_TYPES, n)
        tb, fb = run_program(prog, cb, nulls, COL_TYPES, n)
        assert np.array_equal(ta, tb) and np.array_equal(fa, fb), tree


def test_nary_folding():
    leaves = [("cmp", ">", 0, -3), ("cmp", "<", 2, 4), ("is_null", 1), ("cmp", "!=", 3, 0)]
    for kind, code in (("and", 16), ("or", 17)):
        prog = compile_predicate((kind, *leaves), COL_TYPES)
        # left fold: x y OP z OP w OP — binary connectives, stack never above 2
        assert [int(o) for o in prog[0]] == [4, 2, code, 8, code, 1, code]
        nested = (kind, (kind, (kind, leaves[0], leaves[1]), leaves[2]), leaves[3])
        again = compile_predicate(nested, COL_TYPES)
        assert all(np.array_equal(p, q) for p, q in zip(prog, again))
    # one operand folds to the operand itself
    assert [int(o) for o in compile_predicate(("and", leaves[0]), COL_TYPES)[0]] == [4]
    cols, nulls = make_data(500, seed=2)
    t, f = run_program(compile_predicate(("and", *leaves), COL_TYPES), cols, nulls,
                       COL_TYPES, 500)
    et, ef = ref_eval(("and", *leaves), cols, nulls, 500)
    assert np.array_equal(t, et) and np.array_equal(f, ef)


def test_in_list_unsorted_with_duplicates():
    cols, nulls = make_data(600, seed=9)
    messy = ("in", 2, [5, -3, 5, I64_MAX, 0, -3, I64_MIN, 0, 5])
    tidy = ("in", 2, [I64_MIN, -3, 0, 5, I64_MAX])
    both = ("or", messy, ("in", 1, [2, 2, -6, I32_MAX, 1 << 40]))  # two lists share in_values
    for tree in (messy, both):
        prog = compile_predicate(tree, COL_TYPES)
        t, f = run_program(prog, cols, nulls, COL_TYPES, 600)
        et, ef = ref_eval(tree, cols, nulls, 600)
        assert np.array_equal(t, et) and np.array_equal(f, ef)
    tm = run_program(compile_predicate(messy, COL_TYPES), cols, nulls, COL_TYPES, 600)
    tt = run_program(compile_predicate(tidy, COL_TYPES), cols, nulls, COL_TYPES, 600)
    assert np.array_equal(tm[0], tt[0]) and tm[0].any()
    prog = compile_predicate(both, COL_TYPES)
    assert [(int(a), int(b)) for o, a, b in zip(prog[0], prog[2], prog[3]) if o == P_IN] == \
        [(0, 9), (9, 5)] and len(prog[4]) == 14


def chain(kind, k, leaf=("cmp", "=", 0, 1)):
    return (kind, *([leaf] * k))


def right_nested(k, leaf=("cmp", "=", 0, 1)):
    t = leaf
    for _ in range(k - 1):
        t = ("and", leaf, t)
    return t


BAD_TREES = [
    ("xor", ("is_null", 0), ("is_null", 1)),          # unknown node
    "is_null",                                        # not a node
    ("cmp", "~", 0, 1),                               # unknown compare operator
    ("cmp", "<", 4, 1),                               # column index out of range
    ("cmp", "<", -1, 1),
    ("is_null", 9),
    ("between", 7, 0, 1),
    ("in", 4, [1]),
    ("cmp_col", "<", 0, 4),                           # RHS column out of range
    ("cmp_col", "<", 0, 2),                           # RHS_COL type mismatch (I32 vs I64)
    ("cmp", "<", 0, 1 << 63),                         # constant beyond int64
    ("between", 2, -(1 << 63) - 1, 0),
    ("in", 2, [0, 1 << 64]),
    ("cmp", "<", 0, 1.5),                             # not an integer
    ("and",),                                         # no operand
    ("not", ("is_null", 0), ("is_null", 1)),          # arity
    ("cmp", "<", 0),
    chain("and", 33),                                 # 33 leaves + 32 ANDs = 65 insns
    right_nested(PRED_MAX_STACK + 1),                 # 17 values on the stack
]


@pytest.mark.parametrize("tree", BAD_TREES, ids=lambda t: str(t)[:40])
def test_compiler_rejects(tree):
    with pytest.raises(ValueError):
        compile_predicate(tree, COL_TYPES)


def test_compiler_limits_are_exact():
    assert len(compile_predicate(chain("or", 32), COL_TYPES)[0]) == 63
    assert len(compile_predicate(("not", chain("or", 32)), COL_TYPES)[0]) == PRED_MAX_INSNS
    compile_predicate(right_nested(PRED_MAX_STACK), COL_TYPES)
    with pytest.raises(ValueError):
        compile_predicate(("is_null", 0), [PT_I32, 2])     # unknown column type


def raw_program(ops, cols=None, a=None, b=None, in_values=()):
    k = len(ops)
    return (np.array(ops, np.int32), np.array(cols or [0] * k, np.int32),
            np.array(a or [0] * k, np.int64), np.array(b or [0] * k, np.int64),
            np.array(in_values, np.int64))


# raw postfix programs the C-ABI must refuse (shared with the GPU test)
BAD_PROGRAMS = {
    "no insns": raw_program([]),
    "too many insns": raw_program([P_EQ] + [P_NOT] * PRED_MAX_INSNS),
    "unknown op 9": raw_program([9]),
    "unknown op 19": raw_program([P_EQ, 19]),
    "unknown op -1": raw_program([-1]),
    "unknown flag bit": raw_program([P_EQ | 0x200]),
    "underflow AND": raw_program([P_EQ, P_AND]),
    "underflow NOT": raw_program([P_NOT, P_EQ]),
    "final depth 2": raw_program([P_EQ, P_EQ]),
    "depth 17": raw_program([P_EQ] * 17 + [P_AND] * 16),
    "col out of range": raw_program([P_EQ], cols=[4]),
    "col negative": raw_program([P_EQ], cols=[-1]),
    "rhs col out of range": raw_program([P_EQ | P_RHS_COL], a=[4]),
    "rhs col negative": raw_program([P_EQ | P_RHS_COL], a=[-1]),
    "rhs type mismatch": raw_program([P_EQ | P_RHS_COL], cols=[1], a=[3]),
    "rhs on BETWEEN": raw_program([P_BETWEEN | P_RHS_COL], a=[1]),
    "rhs on AND": raw_program([P_EQ, P_EQ, P_AND | P_RHS_COL]),
    "IN past the end": raw_program([P_IN], a=[2], b=[2], in_values=[1, 2, 3]),
    "IN negative offset": raw_program([P_IN], a=[-1], b=[1], in_values=[1, 2, 3]),
    "IN negative length": raw_program([P_IN], a=[0], b=[-1], in_values=[1, 2, 3]),
    "IN with no values": raw_program([P_IN], a=[0], b=[1]),
}


@pytest.mark.parametrize("name", sorted(BAD_PROGRAMS))
def test_validate_program_rejects(name):
    with pytest.raises(ValueError):
        validate_program(BAD_PROGRAMS[name], COL_TYPES)
    with pytest.raises(ValueError):
        run_program(BAD_PROGRAMS[name], *make_data(4, 1), COL_TYPES, 4)


def test_mask_pack_roundtrip():
    rng = np.random.default_rng(4)
    for n in (0, 1, 63, 64, 65, 200):
        sel = rng.random(n) < 0.5
        words = pack_mask(sel)
        assert words.dtype == np.uint64 and len(words) == (n + 63) // 64
        assert np.array_equal(unpack_mask(words, n), sel)
        for r in np.flatnonzero(sel):
            assert (int(words[r >> 6]) >> (int(r) & 63)) & 1
        assert sum(bin(int(w)).count("1") for w in words) == int(sel.sum())  # tail bits 0


def test_header_declares_and_engine_binds_predicates():
    src = open(os.path.join(REPO_ROOT, "include", "gpue.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym in ("gpue_pred_eval_mask", "gpue_mask_compact"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, code), f"gpue.h does not declare {sym}"
    assert "ChunkPredicateEvaluator::eval_conjuncts over compound" in " ".join(src.split())
    assert "dictionary codes" in src
    for name, val in (("GPUE_P_IN", 7), ("GPUE_P_NOT", 18), ("GPUE_P_RHS_COL", 0x100),
                      ("GPUE_PRED_MAX_INSNS", PRED_MAX_INSNS),
                      ("GPUE_PRED_MAX_STACK", PRED_MAX_STACK)):
        m = re.search(r"#define\s+%s\s+(\w+)" % name, code)
        assert m and int(m.group(1), 0) == val, name
    from starrocks_amd import engine as eng_mod
    for name in ("pred_eval_mask", "mask_compact", "filter_expr"):
        assert callable(getattr(eng_mod.Engine, name, None)), name
    lib = os.path.join(REPO_ROOT, "starrocks_amd", "libgpue.so")
    if os.path.exists(lib):
        import ctypes
        cdll = ctypes.CDLL(lib)
        eng_mod._declare(cdll)
        assert len(cdll.gpue_pred_eval_mask.argtypes) == 15
        assert len(cdll.gpue_mask_compact.argtypes) == 9


# ---- FilterOperator against a numpy stand-in engine ------------------------
class NpFilterEngine:
    """Just what FilterOperator may call: alloc, pred_eval_mask, mask_compact."""
    DT = {PT_I32: np.int32, PT_I64: np.int64}
    WD = {1: np.uint8, 4: np.uint32, 8: np.uint64}

    def __init__(self):
        self.bufs = []

    def alloc(self, nbytes):
        assert nbytes > 0
        self.bufs.append(NpBuf(nbytes))
        return self.bufs[-1]

    def pred_eval_mask(self, pred_cols, program, n_rows, mask):
        cols = [c.view(self.DT[t], n_rows) for c, _, t in pred_cols]
        nulls = [None if nl is None else nl.view(np.uint8, n_rows) for _, nl, _ in pred_cols]
        t, _ = run_program(program, cols, nulls, [t for _, _, t in pred_cols], n_rows)
        mask.h2d(pack_mask(t))
        return int(t.sum())

    def mask_compact(self, mask, n_rows, cols, out_row_idx=None):
        sel = unpack_mask(mask.view(np.uint64, (n_rows + 63) // 64), n_rows)
        cnt = int(sel.sum())
        for src, dst, w in cols:
            assert src is not dst and dst.nbytes >= cnt * w
            dst.view(self.WD[w], cnt)[:] = src.view(self.WD[w], n_rows)[sel]
        if out_row_idx is not None:
            out_row_idx.view(np.uint32, cnt)[:] = np.flatnonzero(sel)
        return cnt


# chunk columns: 0 a int32 (nullable), 1 a's u8 null mask, 2 b int64, 3 row id u32
OP_CHUNKS = [5000, 1, 4097]          # 3 chunks: multi-tile, single row, ragged
OP_WIDTHS = [4, 1, 8, 4]
OP_PRED_MAP = [(0, 1, PT_I32), (2, None, PT_I64)]   # tree col 0 = a (nullable), 1 = b
OP_TREE = ("or", ("and", ("cmp", "<", 0, 2), ("not", ("in", 1, [3, -2, 3, 0]))),
           ("is_null", 0), ("cmp", "=", 1, 6))


def filter_operator_case():
    n = sum(OP_CHUNKS)
    rng = np.random.default_rng(77)
    a = rng.integers(-6, 7, n).astype(np.int32)
    a_null = (rng.random(n) < 0.2).astype(np.uint8)
    a = np.where(a_null != 0, rng.integers(I32_MIN, I32_MAX, n), a).astype(np.int32)
    b = rng.integers(-6, 7, n).astype(np.int64)
    rid = np.arange(n, dtype=np.uint32)
    keep, _ = ref_eval(OP_TREE, [a, b], [a_null, None], n)
    return (a, a_null, b, rid), keep


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


def run_filter_operator(engine, arrays):
    """Drive the case through PipelineDriver([source, FilterOperator, sink]);
    returns (filter operator, one concatenated numpy array per chunk column,
    the input buffers the source handed out)."""
    starts = np.concatenate([[0], np.cumsum(OP_CHUNKS)])
    pushed = []

    def gen(ordinal, _one):
        lo, n = int(starts[ordinal]), OP_CHUNKS[ordinal]
        cols = []
        for arr in arrays:
            buf = engine.alloc(n * arr.itemsize)
            buf.h2d(arr[lo:lo + n])
            cols.append(buf)
        pushed.extend(cols)
        return {"n": n, "cols": cols}

    filt = FilterOperator(engine, OP_TREE, OP_PRED_MAP, OP_WIDTHS)
    chunks = PipelineDriver([ChunkSourceOperator(gen, len(OP_CHUNKS), 1), filt,
                             CollectSink()]).process()
    assert len(chunks) == len(OP_CHUNKS)
    out = []
    for k, arr in enumerate(arrays):
        out.append(np.concatenate([c["cols"][k].d2h(arr.dtype, c["n"]) if c["n"]
                                   else np.empty(0, arr.dtype) for c in chunks]))
    for c in chunks:
        for bbuf in c["cols"]:
            bbuf.free()
    return filt, out, pushed


def test_filter_operator_against_numpy_engine():
    arrays, keep = filter_operator_case()
    assert 0 < keep.sum() < len(keep)
    eng = NpFilterEngine()
    filt, out, pushed = run_filter_operator(eng, arrays)
    for got, arr in zip(out, arrays):
        assert got.dtype == arr.dtype and np.array_equal(got, arr[keep])
    assert filt.rows_in == len(keep) and filt.rows_out == int(keep.sum())
    assert all(b.freed for b in eng.bufs), "operator leaked a buffer"
    assert all(b.freed for b in pushed)


def test_filter_operator_rejects_bad_bindings():
    eng = NpFilterEngine()
    with pytest.raises(ValueError):
        FilterOperator(eng, OP_TREE, OP_PRED_MAP, [4, 1, 8, 2])            # width 2
    with pytest.raises(ValueError):
        FilterOperator(eng, OP_TREE, [(0, 1, PT_I64), (2, None, PT_I64)], OP_WIDTHS)
    with pytest.raises(ValueError):
        FilterOperator(eng, OP_TREE, [(0, 2, PT_I32), (2, None, PT_I64)], OP_WIDTHS)
    with pytest.raises(ValueError):
        FilterOperator(eng, ("cmp", "<", 2, 0), OP_PRED_MAP, OP_WIDTHS)    # tree col 2 unbound
