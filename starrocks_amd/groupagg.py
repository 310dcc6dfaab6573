"""General GROUP BY: the spec gpue_group_agg_* takes (gpue.h, "general GROUP
BY"), its validation, and a numpy reference.

No GPU or ctypes imports: GroupAggSpec rejects what the C-ABI would reject
(ValueError, before any device call), and group_agg_ref() is the GPU-less
stand-in for a whole create / push / emit round — GroupAggSinkOperator runs
against it on the CPU.

Columns are described as in Engine.project:
    keys = [(values, nulls or None, PT_I32 / PT_I64), ...]         1..4
    aggs = [(fn, values or None, nulls or None, PT_I32 / PT_I64), ...]  0..8
A key or input is declared nullable iff it comes with a null column (u8,
nonzero = NULL). COUNT_STAR takes no input (values None) outside merge mode.

Semantics are SQL GROUP BY: NULL keys group together and the value under a
NULL cell is never read; COUNT_STAR counts rows, COUNT non-NULL inputs; SUM
(wrapping mod 2^64), MIN and MAX skip NULLs, and are NULL (value 0, null
byte 1) for a group with no non-NULL input iff their input was declared
nullable. Every aggregate output is int64. AVG is SUM and COUNT in the table
and one division at finalize (avg_finalize). See include/gpue.h for the full
statement.
"""

import numpy as np

PT_I32, PT_I64 = 0, 1
COUNT_STAR, COUNT, SUM, MIN, MAX = range(5)
MERGE = 1
MAX_KEYS = 4
MAX_AGGS = 8
FN_NAMES = {"count_star": COUNT_STAR, "count": COUNT, "sum": SUM, "min": MIN, "max": MAX}
_DT = {PT_I32: np.int32, PT_I64: np.int64}
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def _nbytes(b):
    return b.nbytes


class GroupAggSpec:
    """The layout fixed at gpue_group_agg_create, validated as the C side
    validates it."""

    def __init__(self, key_types, key_nullable, agg_fns=(), agg_types=(), agg_nullable=()):
        self.key_types = [int(t) for t in key_types]
        self.key_nullable = [bool(x) for x in key_nullable]
        self.agg_fns = [FN_NAMES[f] if isinstance(f, str) and f in FN_NAMES else f
                        for f in agg_fns]
        self.agg_types = list(agg_types)
        self.agg_nullable = [bool(x) for x in agg_nullable]
        if not 1 <= len(self.key_types) <= MAX_KEYS:
            raise ValueError(f"n_keys {len(self.key_types)} outside 1..{MAX_KEYS}")
        if len(self.key_nullable) != len(self.key_types):
            raise ValueError("key_types and key_nullable differ in length")
        if len(self.agg_fns) > MAX_AGGS:
            raise ValueError(f"n_aggs {len(self.agg_fns)} outside 0..{MAX_AGGS}")
        if not len(self.agg_fns) == len(self.agg_types) == len(self.agg_nullable):
            raise ValueError("agg_fns, agg_types and agg_nullable differ in length")
        for t in self.key_types:
            if t not in _DT:
                raise ValueError(f"unknown key type {t!r}")
        for a, f in enumerate(self.agg_fns):
            if isinstance(f, bool) or f not in (COUNT_STAR, COUNT, SUM, MIN, MAX):
                raise ValueError(f"unknown aggregate function {f!r}")
            if f == COUNT_STAR:
                self.agg_types[a] = PT_I64     # ignored by the C side
            elif self.agg_types[a] not in _DT:
                raise ValueError(f"unknown aggregate input type {self.agg_types[a]!r}")
        self.agg_types = [int(t) for t in self.agg_types]

    @classmethod
    def of(cls, keys, aggs):
        """From column tuples: nullable iff a null column is given."""
        return cls([k[2] for k in keys], [k[1] is not None for k in keys],
                   [a[0] for a in aggs], [a[3] for a in aggs],
                   [a[2] is not None for a in aggs])

    @property
    def n_keys(self):
        return len(self.key_types)

    @property
    def n_aggs(self):
        return len(self.agg_fns)

    @property
    def out_nullable(self):
        """The static rule: COUNT_STAR / COUNT never; SUM / MIN / MAX iff their
        input was declared nullable."""
        return [f >= SUM and nl for f, nl in zip(self.agg_fns, self.agg_nullable)]

    def key_width(self, k):
        return 8 if self.key_types[k] == PT_I64 else 4

    def agg_width(self, a, merge=False):
        return 8 if merge or self.agg_types[a] == PT_I64 else 4

    def needs_input(self, a, merge=False):
        return merge or self.agg_fns[a] != COUNT_STAR

    def check_push(self, keys, aggs, n_rows, merge=False):
        """keys = [(values, nulls or None)], aggs = [(values or None, nulls or
        None)]; buffers are anything with .nbytes."""
        if merge not in (0, MERGE):
            raise ValueError(f"unknown push flags {merge!r}")
        if not 0 <= n_rows < 1 << 32:
            raise ValueError("n_rows must be below 2^32")
        if len(keys) != self.n_keys or len(aggs) != self.n_aggs:
            raise ValueError("column lists do not match the table's layout")
        for k, (v, nl) in enumerate(keys):
            if v is None:
                raise ValueError(f"key column {k} is missing")
            if _nbytes(v) < n_rows * self.key_width(k):
                raise ValueError(f"key column {k} is shorter than n_rows")
            if nl is not None:
                if not self.key_nullable[k]:
                    raise ValueError(f"null column for key {k}, declared NOT NULL")
                if _nbytes(nl) < n_rows:
                    raise ValueError(f"null column of key {k} is shorter than n_rows")
        for a, (v, nl) in enumerate(aggs):
            if not self.needs_input(a, merge):
                continue
            if v is None:
                raise ValueError(f"input column of aggregate {a} is missing")
            if _nbytes(v) < n_rows * self.agg_width(a, merge):
                raise ValueError(f"input column of aggregate {a} is shorter than n_rows")
            if nl is not None:
                if not self.agg_nullable[a]:
                    raise ValueError(f"null column for aggregate {a}, declared NOT NULL")
                if _nbytes(nl) < n_rows:
                    raise ValueError(f"null column of aggregate {a} is shorter than n_rows")

    def check_emit(self, out_keys, out_aggs, max_out):
        """out_keys / out_aggs = [(values, nulls or None)]; a nullable key or
        output needs its null column, and no buffer may appear twice."""
        if not 0 <= max_out < 1 << 32:
            raise ValueError("max_out must be below 2^32")
        if len(out_keys) != self.n_keys or len(out_aggs) != self.n_aggs:
            raise ValueError("output lists do not match the table's layout")
        seen = []
        for k, (v, nl) in enumerate(out_keys):
            if v is None or _nbytes(v) < max_out * self.key_width(k):
                raise ValueError(f"key output {k} is missing or shorter than max_out")
            seen.append(v)
            if self.key_nullable[k]:
                if nl is None or _nbytes(nl) < max_out:
                    raise ValueError(f"null output of key {k} is missing or short")
                seen.append(nl)
        for a, ((v, nl), nullable) in enumerate(zip(out_aggs, self.out_nullable)):
            if v is None or _nbytes(v) < max_out * 8:
                raise ValueError(f"aggregate output {a} is missing or shorter than max_out")
            seen.append(v)
            if nullable:
                if nl is None or _nbytes(nl) < max_out:
                    raise ValueError(f"null output of aggregate {a} is missing or short")
                seen.append(nl)
        if len({id(b) for b in seen}) != len(seen):
            raise ValueError("an output buffer is used twice")


def sort_result(keys, aggs):
    """Order emitted groups by (null flag, value) of key 0, then key 1, ... —
    the order group_agg_ref returns. keys / aggs = [(values, nulls or None)]."""
    if not keys or len(keys[0][0]) == 0:
        return keys, aggs
    cols = []
    for v, nl in keys:
        cols.append(np.zeros(len(v), np.uint8) if nl is None else np.asarray(nl))
        cols.append(np.asarray(v))
    order = np.lexsort(cols[::-1])
    take = lambda pairs: [(np.asarray(v)[order], None if nl is None else np.asarray(nl)[order])
                          for v, nl in pairs]
    return take(keys), take(aggs)


def group_agg_ref(keys, aggs, n, merge=False):
    """numpy reference of create + push(n rows) + emit. Returns (n_groups,
    [(values, nulls or None)] per key, the same per aggregate), sorted as
    sort_result sorts, in exactly the emitted representation: keys in their
    own types, 0 under NULL, null columns 1/0 and only where nullable; every
    aggregate int64. merge=True reads every aggregate input as an int64
    partial state (COUNT_STAR then has an input too)."""
    spec = GroupAggSpec.of(keys, aggs)
    spec.check_push([(np.asarray(k[0]), k[1]) for k in keys],
                    [(None if a[1] is None else np.asarray(a[1]), a[2]) for a in aggs],
                    n, merge)
    if n == 0:
        return (0, [(np.empty(0, _DT[t]), None if nl is None else np.empty(0, np.uint8))
                    for _, nl, t in keys],
                [(np.empty(0, np.int64), np.empty(0, np.uint8) if nullable else None)
                 for nullable in spec.out_nullable])
    mat = np.zeros((n, 2 * spec.n_keys), np.int64)
    for k, (v, nl, t) in enumerate(keys):
        v = np.asarray(v)[:n].astype(_DT[t]).astype(np.int64)
        if nl is not None:
            isn = np.asarray(nl)[:n] != 0
            mat[:, 2 * k] = isn
            v = np.where(isn, 0, v)
        mat[:, 2 * k + 1] = v
    uniq, inv = np.unique(mat, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    g = len(uniq)
    out_keys = []
    for k, (_, nl, t) in enumerate(keys):
        out_keys.append((uniq[:, 2 * k + 1].astype(_DT[t]),
                         uniq[:, 2 * k].astype(np.uint8) if nl is not None else None))
    out_aggs = []
    for (fn, v, nl, t), nullable in zip(aggs, spec.out_nullable):
        fn = FN_NAMES.get(fn, fn) if isinstance(fn, str) else fn
        if fn == COUNT_STAR and not merge:
            out_aggs.append((np.bincount(inv, minlength=g).astype(np.int64), None))
            continue
        valid = np.ones(n, bool) if nl is None else np.asarray(nl)[:n] == 0
        gi = inv[valid]
        vals = np.asarray(v)[:n].astype(np.int64 if merge else _DT[t]).astype(np.int64)[valid]
        seen = np.bincount(gi, minlength=g) > 0
        if fn == COUNT and not merge:
            res = np.bincount(gi, minlength=g).astype(np.int64)
        elif fn in (COUNT_STAR, COUNT, SUM):
            acc = np.zeros(g, np.uint64)
            np.add.at(acc, gi, vals.astype(np.uint64))   # wraps mod 2^64
            res = acc.astype(np.int64)
        elif fn == MIN:
            res = np.full(g, _I64_MAX, np.int64)
            np.minimum.at(res, gi, vals)
        else:
            res = np.full(g, _I64_MIN, np.int64)
            np.maximum.at(res, gi, vals)
        if nullable:
            out_aggs.append((np.where(seen, res, 0), (~seen).astype(np.uint8)))
        else:
            out_aggs.append((res, None))
    return g, out_keys, out_aggs


def merge_ref(partials, key_types, agg_fns, agg_types=None):
    """Merge emitted partial results [(n_groups, keys, aggs), ...] of one
    layout into the final result: concatenate and aggregate with merge=True.
    A key / output is nullable iff the partials carry a null column for it."""
    cat = lambda xs: np.concatenate([np.asarray(x) for x in xs])
    n = sum(p[0] for p in partials)
    keys = []
    for k, t in enumerate(key_types):
        nl = None if partials[0][1][k][1] is None else cat([p[1][k][1][:p[0]] for p in partials])
        keys.append((cat([p[1][k][0][:p[0]] for p in partials]), nl, t))
    aggs = []
    for a, fn in enumerate(agg_fns):
        nl = None if partials[0][2][a][1] is None else cat([p[2][a][1][:p[0]] for p in partials])
        aggs.append((fn, cat([p[2][a][0][:p[0]] for p in partials]).astype(np.int64), nl,
                     PT_I64 if agg_types is None else agg_types[a]))
    return group_agg_ref(keys, aggs, n, merge=True)


def avg_finalize(sums, sum_nulls, counts):
    """AVG = SUM / COUNT at finalize (aggregate.h: avg keeps sum and count):
    one float64 division on the host. Returns (values, nulls u8); NULL, value
    0.0, where the group has no non-NULL input."""
    sums = np.asarray(sums, np.int64)
    counts = np.asarray(counts, np.int64)
    isn = counts == 0
    if sum_nulls is not None:
        isn = isn | (np.asarray(sum_nulls) != 0)
    out = np.zeros(len(sums), np.float64)
    np.divide(sums.astype(np.float64), counts.astype(np.float64), out=out, where=~isn)
    return out, isn.astype(np.uint8)
