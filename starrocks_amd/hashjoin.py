"""General hash join: the spec gpue_hash_join_* takes (gpue.h, "general hash
join"), its validation, the output rules and a numpy / dict reference.

No GPU or ctypes imports: HashJoinSpec rejects what the C-ABI would reject
(ValueError, before any device call), and hash_join_ref() is the GPU-less
stand-in for a whole create / build_push / probe / emit_build round.

Key columns are described as in Engine.group_agg:
    keys = [(values, nulls or None, PT_I32 / PT_I64), ...]          1..4
one list for the build side and one for the probe side. A key is declared
nullable iff either side comes with a null column (u8, nonzero = NULL).

Semantics are SQL equi-join: values compare as sign-extended int64; a row that
is NULL on a key that is not null-safe matches nothing; on a null-safe key
(<=>) NULL equals NULL and nothing else; the value under a NULL cell is never
read. Build rows are numbered from 0; NO_ROW stands for "no row on this side".
See include/gpue.h for the full statement.
"""

import numpy as np

PT_I32, PT_I64 = 0, 1
MAX_KEYS = 4
NO_ROW = 0xFFFFFFFF
INNER, LEFT_SEMI, LEFT_ANTI, LEFT_OUTER, NULL_AWARE_LEFT_ANTI, MARK_ONLY = range(6)
MARK_BUILD = 1
MODE_NAMES = {"inner": INNER, "left_semi": LEFT_SEMI, "left_anti": LEFT_ANTI,
              "left_outer": LEFT_OUTER, "null_aware_left_anti": NULL_AWARE_LEFT_ANTI,
              "mark_only": MARK_ONLY}
# how -> (probe mode, probe flags, emit_build(matched) tail or None)
HOWS = {
    "inner": (INNER, 0, None),
    "left_semi": (LEFT_SEMI, 0, None),
    "left_anti": (LEFT_ANTI, 0, None),
    "left_outer": (LEFT_OUTER, 0, None),
    "null_aware_left_anti": (NULL_AWARE_LEFT_ANTI, 0, None),
    "right_semi": (MARK_ONLY, MARK_BUILD, 1),
    "right_anti": (MARK_ONLY, MARK_BUILD, 0),
    "right_outer": (INNER, MARK_BUILD, 0),
    "full_outer": (LEFT_OUTER, MARK_BUILD, 0),
}
_DT = {PT_I32: np.int32, PT_I64: np.int64}


def _nbytes(b):
    return b.nbytes


def plan(how):
    """(probe mode, probe flags, emit_build tail or None) of a join type."""
    if how not in HOWS:
        raise ValueError(f"unknown join type {how!r}")
    return HOWS[how]


def output_sides(how):
    """The output rules: (probe side present, probe side nullable, build side
    present, build side nullable) of the joined chunk. A side is nullable
    where the join type can put NO_ROW in its index column; SEMI / ANTI joins
    carry one side only."""
    plan(how)
    return {
        "inner": (True, False, True, False),
        "left_semi": (True, False, False, False),
        "left_anti": (True, False, False, False),
        "null_aware_left_anti": (True, False, False, False),
        "left_outer": (True, False, True, True),
        "right_semi": (False, False, True, False),
        "right_anti": (False, False, True, False),
        "right_outer": (True, True, True, False),
        "full_outer": (True, True, True, True),
    }[how]


class HashJoinSpec:
    """The layout fixed at gpue_hash_join_create, validated as the C side
    validates it."""

    def __init__(self, build_types, probe_types, key_nullable, key_null_safe=None):
        self.build_types = list(build_types)
        self.probe_types = list(probe_types)
        n = len(self.build_types)
        if not 1 <= n <= MAX_KEYS:
            raise ValueError(f"n_keys {n} outside 1..{MAX_KEYS}")
        if key_null_safe is None:
            key_null_safe = [False] * n
        self.key_nullable = [bool(x) for x in key_nullable]
        self.key_null_safe = [bool(x) for x in key_null_safe]
        if not len(self.probe_types) == len(self.key_nullable) == len(self.key_null_safe) == n:
            raise ValueError("build_types, probe_types, key_nullable and key_null_safe "
                             "differ in length")
        for t in self.build_types + self.probe_types:
            if isinstance(t, bool) or t not in _DT:
                raise ValueError(f"unknown key type {t!r}")
        self.build_types = [int(t) for t in self.build_types]
        self.probe_types = [int(t) for t in self.probe_types]

    @classmethod
    def of(cls, build_keys, probe_keys, null_safe=None):
        """From column tuples: a key is nullable iff either side has a null
        column."""
        if len(build_keys) != len(probe_keys):
            raise ValueError("build and probe sides differ in key count")
        return cls([k[2] for k in build_keys], [k[2] for k in probe_keys],
                   [b[1] is not None or p[1] is not None
                    for b, p in zip(build_keys, probe_keys)], null_safe)

    @property
    def n_keys(self):
        return len(self.build_types)

    def width(self, k, side):
        t = (self.build_types if side == "build" else self.probe_types)[k]
        return 8 if t == PT_I64 else 4

    def check_keys(self, keys, n_rows, side):
        """keys = [(values, nulls or None)] of one side; buffers are anything
        with .nbytes."""
        if side not in ("build", "probe"):
            raise ValueError(f"unknown side {side!r}")
        if not 0 <= n_rows < 1 << 32:
            raise ValueError("n_rows must be below 2^32")
        if len(keys) != self.n_keys:
            raise ValueError("key column list does not match the table's layout")
        for k, (v, nl) in enumerate(keys):
            if v is None:
                raise ValueError(f"key column {k} is missing")
            if _nbytes(v) < n_rows * self.width(k, side):
                raise ValueError(f"key column {k} is shorter than n_rows")
            if nl is not None:
                if not self.key_nullable[k]:
                    raise ValueError(f"null column for key {k}, declared NOT NULL")
                if _nbytes(nl) < n_rows:
                    raise ValueError(f"null column of key {k} is shorter than n_rows")

    def check_push(self, keys, n_rows, rows_so_far=0):
        self.check_keys(keys, n_rows, "build")
        if rows_so_far + n_rows >= NO_ROW:
            raise ValueError("total build rows must stay below 2^32-1")

    def check_probe(self, keys, n_rows, mode, flags=0, out_probe=None, out_build=None):
        if isinstance(mode, bool) or mode not in range(MARK_ONLY + 1):
            raise ValueError(f"unknown probe mode {mode!r}")
        if flags not in (0, MARK_BUILD):
            raise ValueError(f"unknown probe flags {flags!r}")
        if mode == NULL_AWARE_LEFT_ANTI and (self.n_keys != 1 or self.key_null_safe[0]):
            raise ValueError("NULL_AWARE_LEFT_ANTI takes one key that is not null-safe")
        self.check_keys(keys, n_rows, "probe")
        if (out_probe is None) != (out_build is None):
            raise ValueError("give both index outputs or neither")
        if out_probe is not None and mode != MARK_ONLY:
            ins = [b for pair in keys for b in pair if b is not None]
            if out_probe is out_build or any(o is b for o in (out_probe, out_build) for b in ins):
                raise ValueError("an output buffer overlaps another buffer")


def check_emit_build(matched, out, max_out):
    if matched not in (0, 1):
        raise ValueError(f"matched must be 0 or 1, not {matched!r}")
    if not 0 <= max_out < 1 << 32:
        raise ValueError("max_out must be below 2^32")
    if out is not None and _nbytes(out) < max_out * 4:
        raise ValueError("build index output is shorter than max_out")


def check_gather_outer(inp, in_nulls, in_rows, width, idx, n, out, out_nulls):
    if width not in (1, 4, 8):
        raise ValueError(f"width {width!r} not in 1, 4, 8")
    if not (0 <= n < 1 << 32 and 0 <= in_rows < 1 << 32):
        raise ValueError("n and in_rows must be below 2^32")
    if inp is None or idx is None or out is None:
        raise ValueError("in, idx and out are required")
    if _nbytes(inp) < in_rows * width:
        raise ValueError("in is shorter than in_rows")
    if in_nulls is not None and _nbytes(in_nulls) < in_rows:
        raise ValueError("in_nulls is shorter than in_rows")
    if in_nulls is not None and out_nulls is None:
        raise ValueError("in_nulls needs out_nulls")
    if _nbytes(idx) < n * 4 or _nbytes(out) < n * width:
        raise ValueError("idx or out is shorter than n")
    if out_nulls is not None and _nbytes(out_nulls) < n:
        raise ValueError("out_nulls is shorter than n")
    bufs = [b for b in (inp, in_nulls, idx) if b is not None]
    if out is out_nulls or any(o is b for o in (out, out_nulls) for b in bufs):
        raise ValueError("an output buffer overlaps another buffer")


def _tuples(keys, n, null_safe):
    """Per row: its canonical tuple ((is_null, value or 0), ...) or None for a
    row that can match nothing."""
    cols = []
    for v, nl, t in keys:
        vals = np.asarray(v)[:n].astype(_DT[t]).astype(np.int64)
        isn = np.zeros(n, bool) if nl is None else np.asarray(nl)[:n] != 0
        cols.append((np.where(isn, 0, vals).tolist(), isn.tolist()))
    out = []
    for i in range(n):
        tup, dead = [], False
        for (vals, isn), ns in zip(cols, null_safe):
            if isn[i] and not ns:
                dead = True
                break
            tup.append((isn[i], vals[i]))
        out.append(None if dead else tuple(tup))
    return out


def _has_null(keys, n):
    return [any(nl is not None and np.asarray(nl)[i] != 0 for _, nl, _ in keys)
            for i in range(n)]


def sort_pairs(probe_idx, build_idx):
    """The pair multiset as an (n, 2) int64 array in lexicographic order."""
    p = np.asarray(probe_idx, np.int64).reshape(-1)
    b = np.asarray(build_idx, np.int64).reshape(-1)
    order = np.lexsort((b, p))
    return np.stack([p[order], b[order]], axis=1) if len(p) else np.empty((0, 2), np.int64)


def hash_join_ref(build_keys, probe_keys, null_safe, mode, n_build=None, n_probe=None):
    """Reference of build_push(all build rows) + one probe in `mode` (a
    GPUE_HJ_* number or its lower-case name). Returns (pairs, matched):
    pairs the emitted (probe_idx, build_idx) multiset as sort_pairs orders it
    (LEFT_SEMI lists EVERY true match of a row: the entry may report any one
    of them), matched the bool array of the build rows some probe row matched
    — what MARK_BUILD marks, whatever the mode emits."""
    mode = MODE_NAMES.get(mode, mode) if isinstance(mode, str) else mode
    spec = HashJoinSpec.of(build_keys, probe_keys, null_safe)
    nb = len(np.asarray(build_keys[0][0])) if n_build is None else n_build
    np_ = len(np.asarray(probe_keys[0][0])) if n_probe is None else n_probe
    spec.check_push([(np.asarray(k[0]), k[1]) for k in build_keys], nb)
    spec.check_probe([(np.asarray(k[0]), k[1]) for k in probe_keys], np_, mode)
    ns = spec.key_null_safe
    table = {}
    btup = _tuples(build_keys, nb, ns)
    for j, t in enumerate(btup):
        if t is not None:
            table.setdefault(t, []).append(j)
    matched = np.zeros(nb, bool)
    pi, bi = [], []
    ptup = _tuples(probe_keys, np_, ns)
    pnull = _has_null(probe_keys, np_)
    build_has_null = any(t is None for t in btup)
    for i, t in enumerate(ptup):
        rows = table.get(t, []) if t is not None else []
        matched[rows] = True
        if mode in (INNER, LEFT_SEMI) or (mode == LEFT_OUTER and rows):
            pi += [i] * len(rows)
            bi += rows
        elif mode == LEFT_OUTER or (mode == LEFT_ANTI and not rows):
            pi.append(i)
            bi.append(NO_ROW)
        elif mode == NULL_AWARE_LEFT_ANTI:
            if nb == 0 or (not build_has_null and not pnull[i] and not rows):
                pi.append(i)
                bi.append(NO_ROW)
    return sort_pairs(pi, bi), matched


def hash_join_how_ref(build_keys, probe_keys, how, null_safe=None, n_build=None,
                      n_probe=None):
    """Reference of Engine.hash_join: the probe's pairs followed by the RIGHT /
    FULL tail as (NO_ROW, b) rows, as one sort_pairs array. For left_semi
    every true match is listed (see hash_join_ref)."""
    mode, _, tail = plan(how)
    pairs, matched = hash_join_ref(build_keys, probe_keys, null_safe, mode, n_build, n_probe)
    if tail is None:
        return pairs
    rows = np.nonzero(matched if tail else ~matched)[0]
    return sort_pairs(np.concatenate([pairs[:, 0], np.full(len(rows), NO_ROW, np.int64)]),
                      np.concatenate([pairs[:, 1], rows.astype(np.int64)]))


def gather_outer_ref(values, in_nulls, idx, with_nulls=True):
    """Reference of gpue_gather_outer: (out, out_nulls or None). Raises
    ValueError for what the entry reports through its latch."""
    values = np.asarray(values)
    idx = np.asarray(idx, np.uint32).astype(np.int64)
    if in_nulls is not None and not with_nulls:
        raise ValueError("in_nulls needs out_nulls")
    none = idx == NO_ROW
    if np.any(~none & (idx >= len(values))):
        raise ValueError("idx holds an index >= in_rows")
    if np.any(none) and not with_nulls:
        raise ValueError("idx holds NO_ROW and there is no out_nulls")
    safe = np.where(none, 0, idx)
    if len(values) == 0:
        out = np.zeros(len(idx), values.dtype)
        nl = np.ones(len(idx), np.uint8)
    else:
        out = np.where(none, 0, values[safe]).astype(values.dtype)
        src = np.zeros(len(values), np.uint8) if in_nulls is None else \
            (np.asarray(in_nulls)[:len(values)] != 0).astype(np.uint8)
        nl = np.where(none, 1, src[safe]).astype(np.uint8)
    return out, (nl if with_nulls else None)
