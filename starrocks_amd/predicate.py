"""Predicate trees -> the postfix program gpue_pred_eval_mask runs (gpue.h,
"predicate expressions"), plus a numpy interpreter of that program.

No GPU or ctypes imports: the compiler rejects what the C-ABI would reject
(ValueError, before any device call), and run_program() is the GPU-less
stand-in for the device call — FilterOperator runs against it on the CPU.

Tree forms (nested tuples; col / col2 are predicate-column indexes):
    ("and", x, y, ...)   ("or", x, y, ...)   ("not", x)
    ("cmp", "<", col, const)          ops: = == != <> < <= > >=
    ("cmp_col", "<=", col, col2)      both columns of one type
    ("between", col, lo, hi)          lo <= col <= hi
    ("in", col, [values])             any order, duplicates allowed
    ("is_null", col)
N-ary and / or fold left to binary (x y AND z AND ...), which keeps the
evaluation stack at its minimum depth. Strings are not a leaf type: lower a
varchar predicate to EQ / IN / BETWEEN over dictionary codes first.

Semantics are SQL three-valued (Kleene) logic; a row passes iff the root is
TRUE. See include/gpue.h for the full statement.
"""

import numpy as np

PT_I32, PT_I64 = 0, 1
P_EQ, P_NE, P_LT, P_LE, P_GT, P_GE, P_BETWEEN, P_IN, P_IS_NULL = range(9)
P_AND, P_OR, P_NOT = 16, 17, 18
P_RHS_COL = 0x100
PRED_MAX_INSNS = 64
PRED_MAX_STACK = 16

CMP_OPS = {"=": P_EQ, "==": P_EQ, "!=": P_NE, "<>": P_NE, "<": P_LT, "<=": P_LE,
           ">": P_GT, ">=": P_GE}
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def _const(v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"predicate constant must be an integer, got {v!r}")
    v = int(v)
    if not _I64_MIN <= v <= _I64_MAX:
        raise ValueError(f"predicate constant {v} does not fit int64")
    return v


def _col(c, col_types):
    if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
        raise ValueError(f"column index must be an integer, got {c!r}")
    if not 0 <= c < len(col_types):
        raise ValueError(f"column index {c} out of range 0..{len(col_types) - 1}")
    return int(c)


def compile_predicate(tree, col_types):
    """-> (op, col, a, b, in_values): int32, int32, int64, int64, int64 arrays,
    ready for Engine.pred_eval_mask / run_program. col_types[i] is PT_I32 or
    PT_I64 for predicate column i."""
    col_types = [int(t) for t in col_types]
    for t in col_types:
        if t not in (PT_I32, PT_I64):
            raise ValueError(f"unknown predicate column type {t}")
    ops, cols, a_s, b_s, in_vals = [], [], [], [], []

    def emit(op, col=0, a=0, b=0):
        ops.append(op)
        cols.append(col)
        a_s.append(a)
        b_s.append(b)

    def walk(node):
        if not isinstance(node, (tuple, list)) or not node or not isinstance(node[0], str):
            raise ValueError(f"not a predicate node: {node!r}")
        kind, args = node[0], node[1:]
        if kind in ("and", "or"):
            if not args:
                raise ValueError(f"'{kind}' needs at least one operand")
            walk(args[0])
            for x in args[1:]:
                walk(x)
                emit(P_AND if kind == "and" else P_OR)
        elif kind == "not":
            if len(args) != 1:
                raise ValueError("'not' takes one operand")
            walk(args[0])
            emit(P_NOT)
        elif kind in ("cmp", "cmp_col"):
            if len(args) != 3:
                raise ValueError(f"'{kind}' takes (op, col, rhs)")
            if args[0] not in CMP_OPS:
                raise ValueError(f"unknown compare operator {args[0]!r}")
            c = _col(args[1], col_types)
            if kind == "cmp":
                emit(CMP_OPS[args[0]], c, _const(args[2]))
            else:
                c2 = _col(args[2], col_types)
                if col_types[c] != col_types[c2]:
                    raise ValueError(f"cmp_col over columns {c} and {c2} of different types")
                emit(CMP_OPS[args[0]] | P_RHS_COL, c, c2)
        elif kind == "between":
            if len(args) != 3:
                raise ValueError("'between' takes (col, lo, hi)")
            emit(P_BETWEEN, _col(args[0], col_types), _const(args[1]), _const(args[2]))
        elif kind == "in":
            if len(args) != 2:
                raise ValueError("'in' takes (col, values)")
            c = _col(args[0], col_types)
            vals = [_const(v) for v in args[1]]
            emit(P_IN, c, len(in_vals), len(vals))
            in_vals.extend(vals)
        elif kind == "is_null":
            if len(args) != 1:
                raise ValueError("'is_null' takes (col)")
            emit(P_IS_NULL, _col(args[0], col_types))
        else:
            raise ValueError(f"unknown predicate node {kind!r}")

    walk(tree)
    program = (np.array(ops, np.int32), np.array(cols, np.int32), np.array(a_s, np.int64),
               np.array(b_s, np.int64), np.array(in_vals, np.int64))
    validate_program(program, col_types)
    return program


def validate_program(program, col_types):
    """The C-ABI's program checks (gpue.h), as ValueError."""
    op, col, a, b, in_values = program
    n = len(op)
    if not (len(col) == len(a) == len(b) == n):
        raise ValueError("program arrays differ in length")
    if not 1 <= n <= PRED_MAX_INSNS:
        raise ValueError(f"program has {n} instructions, outside 1..{PRED_MAX_INSNS}")
    for t in col_types:
        if t not in (PT_I32, PT_I64):
            raise ValueError(f"unknown predicate column type {t}")
    depth = 0
    for i in range(n):
        raw = int(op[i])
        o, rhs = raw & ~P_RHS_COL, bool(raw & P_RHS_COL)
        if o in (P_AND, P_OR, P_NOT):
            if rhs:
                raise ValueError(f"insn {i}: RHS_COL on a connective")
            if depth < (1 if o == P_NOT else 2):
                raise ValueError(f"insn {i}: stack underflow")
            depth -= 0 if o == P_NOT else 1
            continue
        if not P_EQ <= o <= P_IS_NULL:
            raise ValueError(f"insn {i}: unknown op {raw}")
        if rhs and o > P_GE:
            raise ValueError(f"insn {i}: RHS_COL on a non-compare op")
        if not 0 <= int(col[i]) < len(col_types):
            raise ValueError(f"insn {i}: column index {int(col[i])} out of range")
        depth += 1
        if depth > PRED_MAX_STACK:
            raise ValueError(f"insn {i}: stack depth above {PRED_MAX_STACK}")
        if rhs:
            c2 = int(a[i])
            if not 0 <= c2 < len(col_types):
                raise ValueError(f"insn {i}: RHS column index {c2} out of range")
            if col_types[c2] != col_types[int(col[i])]:
                raise ValueError(f"insn {i}: RHS_COL type mismatch")
        if o == P_IN:
            off, ln = int(a[i]), int(b[i])
            if off < 0 or ln < 0 or off + ln > len(in_values):
                raise ValueError(f"insn {i}: IN range outside [0, {len(in_values)}]")
    if depth != 1:
        raise ValueError(f"program leaves {depth} values on the stack, not 1")


def run_program(program, cols, nulls, col_types, n_rows):
    """Postfix interpreter over numpy columns: the device call's stand-in.
    cols[i] / nulls[i] (None, or u8 with nonzero = NULL row) are predicate
    column i. Returns (is_true, is_false) bool arrays of n_rows; a row that is
    neither is UNKNOWN."""
    validate_program(program, col_types)
    op, col, a, b, in_values = program
    n = int(n_rows)

    def load(c):
        dt = np.int64 if col_types[c] == PT_I64 else np.int32
        v = np.asarray(cols[c])[:n]
        if v.dtype != dt:
            raise ValueError(f"column {c} is {v.dtype}, program says {np.dtype(dt)}")
        isn = (np.zeros(n, bool) if nulls is None or nulls[c] is None
               else np.asarray(nulls[c])[:n] != 0)
        return v.astype(np.int64), isn

    stack = []
    for i in range(len(op)):
        raw = int(op[i])
        o, rhs = raw & ~P_RHS_COL, bool(raw & P_RHS_COL)
        if o == P_NOT:
            t, f = stack.pop()
            stack.append((f, t))
        elif o in (P_AND, P_OR):
            (xt, xf), (yt, yf) = stack.pop(), stack.pop()
            stack.append((xt & yt, xf | yf) if o == P_AND else (xt | yt, xf & yf))
        else:
            v, isn = load(int(col[i]))
            if o == P_IS_NULL:
                stack.append((isn, ~isn))
                continue
            if rhs:
                w, isn2 = load(int(a[i]))
                isn = isn | isn2
            else:
                w = np.int64(a[i])
            if o == P_EQ:
                r = v == w
            elif o == P_NE:
                r = v != w
            elif o == P_LT:
                r = v < w
            elif o == P_LE:
                r = v <= w
            elif o == P_GT:
                r = v > w
            elif o == P_GE:
                r = v >= w
            elif o == P_BETWEEN:
                r = (v >= np.int64(a[i])) & (v <= np.int64(b[i]))
            else:
                r = np.isin(v, in_values[int(a[i]):int(a[i]) + int(b[i])])
            stack.append((r & ~isn, ~r & ~isn))
    return stack[0]


def pack_mask(selected):
    """bool rows -> the device bitmap: ceil(n/64) u64 words, bit (r & 63) of
    word r >> 6 = row r, tail bits 0."""
    sel = np.asarray(selected, bool)
    n_words = (len(sel) + 63) // 64
    padded = np.zeros(n_words * 64, np.uint8)
    padded[:len(sel)] = sel
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def unpack_mask(words, n_rows):
    """The device bitmap -> bool rows (bits at positions >= n_rows ignored)."""
    raw = np.ascontiguousarray(np.asarray(words, np.uint64).astype("<u8")).view(np.uint8)
    return np.unpackbits(raw, bitorder="little")[:n_rows].astype(bool)
