"""Scalar expression trees -> the postfix program gpue_expr_project runs
(gpue.h, "scalar expressions"), plus a numpy interpreter of that program.

No GPU or ctypes imports: the compiler rejects what the C-ABI would reject
(ValueError, before any device call), and run_program() is the GPU-less
stand-in for the device call — ProjectOperator runs against it on the CPU.

Tree forms (nested tuples; a column index is an input-column index):
    ("col", i)   ("const", v)   ("null",)
    ("+", x, y, ...)  ("-", x, y, ...)  ("*", x, y, ...)  ("/", x, y, ...)
    ("%", x, y, ...)      wrapping; a trailing "checked" on + - * (as in
                          ("+", x, y, "checked")) turns signed overflow to NULL
    ("neg", x)  ("abs", x)          also ("neg", x, "checked") / ("abs", ...)
    ("cast_i32", x)                 out of the int32 range -> NULL
    ("cmp", "<", x, y)              ops: = == != <> < <= > >=
    ("and", x, y, ...)  ("or", x, y, ...)  ("not", x)      Kleene
    ("is_null", x)  ("if", c, t, e)  ("ifnull", a, b)
    ("case", [(c, t), ...], else_or_None)     nested IF; no ELSE is NULL
N-ary forms fold left. Every value is an int64 plus a NULL flag; see
include/gpue.h for the full statement of the semantics.
"""

import numpy as np

from starrocks_amd.predicate import PT_I32, PT_I64, pack_mask

X_COL, X_CONST, X_NULL = 32, 33, 34
X_NEG, X_ABS, X_NOT, X_IS_NULL, X_CAST_I32 = 40, 41, 42, 43, 44
X_ADD, X_SUB, X_MUL, X_DIV, X_MOD = 48, 49, 50, 51, 52
X_EQ, X_NE, X_LT, X_LE, X_GT, X_GE = 56, 57, 58, 59, 60, 61
X_AND, X_OR, X_IF, X_IFNULL, X_OUT = 64, 65, 66, 67, 68
X_CHECKED = 0x200
XO_I32, XO_I64, XO_MASK = 0, 1, 2
EXPR_MAX_INSNS = 64
EXPR_MAX_STACK = 8
EXPR_MAX_OUT = 8
EXPR_MAX_IN_COLS = 64

ARITH_OPS = {"+": X_ADD, "-": X_SUB, "*": X_MUL, "/": X_DIV, "%": X_MOD}
CMP_OPS = {"=": X_EQ, "==": X_EQ, "!=": X_NE, "<>": X_NE, "<": X_LT, "<=": X_LE,
           ">": X_GT, ">=": X_GE}
_CHECKABLE = (X_ADD, X_SUB, X_MUL, X_NEG, X_ABS)
_UNARY = (X_NEG, X_ABS, X_NOT, X_IS_NULL, X_CAST_I32)
_BINARY = (X_ADD, X_SUB, X_MUL, X_DIV, X_MOD, X_EQ, X_NE, X_LT, X_LE, X_GT, X_GE,
           X_AND, X_OR, X_IFNULL)
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def _const(v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"expression constant must be an integer, got {v!r}")
    v = int(v)
    if not _I64_MIN <= v <= _I64_MAX:
        raise ValueError(f"expression constant {v} does not fit int64")
    return v


def compile_exprs(trees, col_types, col_nullable, out_types):
    """-> ((op, col, a), nullable): int32, int32, int64 program arrays ready for
    Engine.expr_project / run_program, and one bool per output — whether the
    expression can yield NULL, i.e. whether the output needs a null buffer.
    col_types[i] is PT_I32 / PT_I64 and col_nullable[i] says whether input
    column i comes with a null mask; tree k is written to output k of type
    out_types[k] (XO_I32 / XO_I64 / XO_MASK)."""
    col_types = [int(t) for t in col_types]
    ops, cols, a_s = [], [], []

    def emit(op, col=0, a=0):
        ops.append(op)
        cols.append(col)
        a_s.append(a)

    def checked(kind, args):
        if args and isinstance(args[-1], str):
            if args[-1] != "checked":
                raise ValueError(f"unknown modifier {args[-1]!r} on '{kind}'")
            return args[:-1], X_CHECKED
        return args, 0

    def walk(node):
        if not isinstance(node, (tuple, list)) or not node or not isinstance(node[0], str):
            raise ValueError(f"not an expression node: {node!r}")
        kind, args = node[0], tuple(node[1:])
        if kind == "col":
            if len(args) != 1 or isinstance(args[0], (bool, np.bool_)) or \
                    not isinstance(args[0], (int, np.integer)):
                raise ValueError("'col' takes one integer column index")
            if not 0 <= args[0] < len(col_types):
                raise ValueError(f"column index {args[0]} out of range")
            emit(X_COL, int(args[0]))
        elif kind == "const":
            if len(args) != 1:
                raise ValueError("'const' takes one value")
            emit(X_CONST, 0, _const(args[0]))
        elif kind == "null":
            if args:
                raise ValueError("'null' takes no operand")
            emit(X_NULL)
        elif kind in ARITH_OPS:
            args, flag = checked(kind, args)
            if flag and ARITH_OPS[kind] not in _CHECKABLE:
                raise ValueError(f"'{kind}' has no checked form")
            if len(args) < 2:
                raise ValueError(f"'{kind}' needs at least two operands")
            walk(args[0])
            for x in args[1:]:
                walk(x)
                emit(ARITH_OPS[kind] | flag)
        elif kind in ("neg", "abs"):
            args, flag = checked(kind, args)
            if len(args) != 1:
                raise ValueError(f"'{kind}' takes one operand")
            walk(args[0])
            emit((X_NEG if kind == "neg" else X_ABS) | flag)
        elif kind in ("not", "is_null", "cast_i32"):
            if len(args) != 1:
                raise ValueError(f"'{kind}' takes one operand")
            walk(args[0])
            emit({"not": X_NOT, "is_null": X_IS_NULL, "cast_i32": X_CAST_I32}[kind])
        elif kind == "cmp":
            if len(args) != 3:
                raise ValueError("'cmp' takes (op, x, y)")
            if args[0] not in CMP_OPS:
                raise ValueError(f"unknown compare operator {args[0]!r}")
            walk(args[1])
            walk(args[2])
            emit(CMP_OPS[args[0]])
        elif kind in ("and", "or"):
            if not args:
                raise ValueError(f"'{kind}' needs at least one operand")
            walk(args[0])
            for x in args[1:]:
                walk(x)
                emit(X_AND if kind == "and" else X_OR)
        elif kind == "if":
            if len(args) != 3:
                raise ValueError("'if' takes (cond, then, else)")
            for x in args:
                walk(x)
            emit(X_IF)
        elif kind == "ifnull":
            if len(args) != 2:
                raise ValueError("'ifnull' takes (a, b)")
            walk(args[0])
            walk(args[1])
            emit(X_IFNULL)
        elif kind == "case":
            if len(args) != 2 or not args[0]:
                raise ValueError("'case' takes ([(cond, then), ...], else_or_None)")
            for arm in args[0]:
                if not isinstance(arm, (tuple, list)) or len(arm) != 2:
                    raise ValueError(f"not a (cond, then) arm: {arm!r}")
                walk(arm[0])
                walk(arm[1])
            walk(("null",) if args[1] is None else args[1])
            for _ in args[0]:
                emit(X_IF)
        else:
            raise ValueError(f"unknown expression node {kind!r}")

    trees = list(trees)
    for k, tree in enumerate(trees):
        walk(tree)
        emit(X_OUT, k)
    program = (np.array(ops, np.int32), np.array(cols, np.int32), np.array(a_s, np.int64))
    nullable = validate_program(program, col_types, col_nullable, out_types)
    return program, nullable


def validate_program(program, col_types, col_nullable, out_types, out_has_nulls=None):
    """The C-ABI's program checks (gpue.h), as ValueError; returns the static
    nullability of every output. out_has_nulls[k] (optional) says whether
    output k comes with a null buffer: a nullable non-MASK output without one
    is rejected."""
    op, col, a = program
    n = len(op)
    if not (len(col) == len(a) == n):
        raise ValueError("program arrays differ in length")
    if not 1 <= n <= EXPR_MAX_INSNS:
        raise ValueError(f"program has {n} instructions, outside 1..{EXPR_MAX_INSNS}")
    col_types = [int(t) for t in col_types]
    col_nullable = [bool(x) for x in col_nullable]
    out_types = [int(t) for t in out_types]
    if len(col_nullable) != len(col_types):
        raise ValueError("col_types and col_nullable differ in length")
    if len(col_types) > EXPR_MAX_IN_COLS:
        raise ValueError(f"{len(col_types)} input columns, above {EXPR_MAX_IN_COLS}")
    if not 1 <= len(out_types) <= EXPR_MAX_OUT:
        raise ValueError(f"{len(out_types)} outputs, outside 1..{EXPR_MAX_OUT}")
    for t in col_types:
        if t not in (PT_I32, PT_I64):
            raise ValueError(f"unknown input column type {t}")
    for t in out_types:
        if t not in (XO_I32, XO_I64, XO_MASK):
            raise ValueError(f"unknown output type {t}")
    stack = []          # static nullability per slot
    out_nullable = [None] * len(out_types)
    for i in range(n):
        raw = int(op[i])
        o, chk = raw & ~X_CHECKED, bool(raw & X_CHECKED)
        if chk and o not in _CHECKABLE:
            raise ValueError(f"insn {i}: CHECKED on op {o}")
        if o in (X_COL, X_CONST, X_NULL):
            if len(stack) == EXPR_MAX_STACK:
                raise ValueError(f"insn {i}: stack depth above {EXPR_MAX_STACK}")
            if o == X_COL:
                c = int(col[i])
                if not 0 <= c < len(col_types):
                    raise ValueError(f"insn {i}: column index {c} out of range")
                stack.append(col_nullable[c])
            else:
                stack.append(o == X_NULL)
        elif o in _UNARY:
            if len(stack) < 1:
                raise ValueError(f"insn {i}: stack underflow")
            if o == X_IS_NULL:
                stack[-1] = False
            elif o == X_CAST_I32 or chk:
                stack[-1] = True
        elif o in _BINARY:
            if len(stack) < 2:
                raise ValueError(f"insn {i}: stack underflow")
            yn = stack.pop()
            xn = stack.pop()
            stack.append(yn if o == X_IFNULL else (xn or yn or chk or o in (X_DIV, X_MOD)))
        elif o == X_IF:
            if len(stack) < 3:
                raise ValueError(f"insn {i}: stack underflow")
            en = stack.pop()
            tn = stack.pop()
            stack[-1] = tn or en
        elif o == X_OUT:
            if len(stack) != 1:
                raise ValueError(f"insn {i}: OUT with {len(stack)} values on the stack, not 1")
            k = int(col[i])
            if not 0 <= k < len(out_types):
                raise ValueError(f"insn {i}: output index {k} out of range")
            if out_nullable[k] is not None:
                raise ValueError(f"insn {i}: output {k} written twice")
            out_nullable[k] = stack.pop()
            if (out_nullable[k] and out_types[k] != XO_MASK and out_has_nulls is not None
                    and not out_has_nulls[k]):
                raise ValueError(f"output {k} is nullable and has no null buffer")
        else:
            raise ValueError(f"insn {i}: unknown op {raw}")
    if stack:
        raise ValueError("program does not end with an OUT")
    for k, x in enumerate(out_nullable):
        if x is None:
            raise ValueError(f"output {k} is never written")
    return out_nullable


def _u(x):
    return x.view(np.uint64)


def _wrap_neg(x):
    return (np.uint64(0) - _u(x)).view(np.int64)


def _binary(o, chk, x, xn, y, yn):
    rn = xn | yn
    if o == X_ADD:
        r = (_u(x) + _u(y)).view(np.int64)
        if chk:
            rn = rn | (((x ^ r) & (y ^ r)) < 0)
    elif o == X_SUB:
        r = (_u(x) - _u(y)).view(np.int64)
        if chk:
            rn = rn | (((x ^ y) & (x ^ r)) < 0)
    elif o == X_MUL:
        r = (_u(x) * _u(y)).view(np.int64)
        if chk:
            # x not in {0, -1}: the product overflowed iff the wrapped result
            # does not divide back to y (|r - x*y| would be a nonzero multiple
            # of 2^64 yet smaller than |x|); x == -1 overflows only for INT64_MIN
            plain = (x != 0) & (x != -1)
            back = r // np.where(plain, x, 1)
            rn = rn | (plain & (back != y)) | ((x == -1) & (y == _I64_MIN))
    elif o in (X_DIV, X_MOD):
        rn = rn | (y == 0)
        m1 = y == -1
        d = np.where(rn | m1, 1, y)         # never 0, never -1
        q = x // d                          # floor ...
        rem = x - q * d
        q = q + ((rem != 0) & ((x < 0) != (d < 0)))   # ... to truncation
        if o == X_DIV:
            r = np.where(m1, _wrap_neg(x), q)
        else:
            r = np.where(m1, 0, x - q * d)
    elif o in (X_AND, X_OR):
        xt, xf = ~xn & (x != 0), ~xn & (x == 0)
        yt, yf = ~yn & (y != 0), ~yn & (y == 0)
        rt, rf = (xt & yt, xf | yf) if o == X_AND else (xt | yt, xf & yf)
        r, rn = rt, ~(rt | rf)
    else:
        r = {X_EQ: x == y, X_NE: x != y, X_LT: x < y, X_LE: x <= y, X_GT: x > y,
             X_GE: x >= y}[o]
    return r.astype(np.int64), rn


def run_program(program, cols, nulls, col_types, out_types, n_rows):
    """Postfix interpreter over numpy columns: the device call's stand-in.
    cols[i] / nulls[i] (None, or u8 with nonzero = NULL row) are input column
    i. Returns one (values, is_null) per output, exactly what the device
    leaves in the output buffers: int64 / int32 values with 0 under a NULL
    row and a u8 array of 1 / 0, or (mask words, None) for an XO_MASK output."""
    col_types = [int(t) for t in col_types]
    validate_program(program, col_types,
                     [nulls is not None and nulls[c] is not None for c in range(len(col_types))],
                     out_types)
    op, col, a = program
    n = int(n_rows)
    outs = [None] * len(out_types)
    stack = []
    for i in range(len(op)):
        raw = int(op[i])
        o, chk = raw & ~X_CHECKED, bool(raw & X_CHECKED)
        if o == X_COL:
            c = int(col[i])
            dt = np.int64 if col_types[c] == PT_I64 else np.int32
            v = np.asarray(cols[c])[:n]
            if v.dtype != dt:
                raise ValueError(f"column {c} is {v.dtype}, program says {np.dtype(dt)}")
            isn = (np.zeros(n, bool) if nulls is None or nulls[c] is None
                   else np.asarray(nulls[c])[:n] != 0)
            stack.append((v.astype(np.int64), isn))
        elif o in (X_CONST, X_NULL):
            stack.append((np.full(n, int(a[i]) if o == X_CONST else 0, np.int64),
                          np.full(n, o == X_NULL, bool)))
        elif o in _UNARY:
            x, xn = stack.pop()
            if o in (X_NEG, X_ABS):
                r = _wrap_neg(x) if o == X_NEG else np.where(x < 0, _wrap_neg(x), x)
                rn = xn | (x == _I64_MIN) if chk else xn
            elif o == X_NOT:
                r, rn = (x == 0).astype(np.int64), xn
            elif o == X_IS_NULL:
                r, rn = xn.astype(np.int64), np.zeros(n, bool)
            else:
                r, rn = x, xn | (x != x.astype(np.int32).astype(np.int64))
            stack.append((r, rn))
        elif o == X_IFNULL:
            (y, yn), (x, xn) = stack.pop(), stack.pop()
            stack.append((np.where(xn, y, x), xn & yn))
        elif o in _BINARY:
            (y, yn), (x, xn) = stack.pop(), stack.pop()
            stack.append(_binary(o, chk, x, xn, y, yn))
        elif o == X_IF:
            (e, en), (t, tn), (c, cn) = stack.pop(), stack.pop(), stack.pop()
            take = ~cn & (c != 0)
            stack.append((np.where(take, t, e), np.where(take, tn, en)))
        else:   # X_OUT
            x, xn = stack.pop()
            x = np.where(xn, 0, x)
            k = int(col[i])
            if out_types[k] == XO_MASK:
                outs[k] = (pack_mask(x != 0), None)
            elif out_types[k] == XO_I64:
                outs[k] = (x.astype(np.int64), xn.astype(np.uint8))
            else:
                outs[k] = (_u(x).astype(np.uint32).view(np.int32), xn.astype(np.uint8))
    return outs
