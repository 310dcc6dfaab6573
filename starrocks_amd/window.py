"""Window functions: the spec gpue_window_eval takes (gpue.h, "window
functions"), its validation, and a numpy reference.

No GPU or ctypes imports: WindowSpec rejects what the C-ABI would reject
(ValueError, before any device call), window_ref() is the GPU-less stand-in
for one gpue_window_eval call and sort_perm_ref() for the gpue_topn full sort
in front of it.

Columns are described as in Engine.project / Engine.group_agg:
    part_keys  = [(values, nulls or None, PT_I32 / PT_I64), ...]    0..4
    order_keys = [(values, nulls or None, PT_I32 / PT_I64), ...]    0..4
    funcs      = [WinFunc(...), ...]                                1..8
A key or input is declared nullable iff it comes with a null column (u8,
nonzero = NULL) unless WinFunc.nullable says otherwise.

Semantics (include/gpue.h has the full statement): rows are taken in the order
of the permutation order_idx (None = as they stand). Sorted position i starts
a partition iff i == 0 or a partition key differs from position i-1, and a
peer group iff it starts a partition or an order key differs; NULL equals
NULL, the cell under a NULL is never read. All outputs are int64; a NULL
output is value 0 with null byte 1.
"""

import numpy as np

PT_I32, PT_I64 = 0, 1
(ROW_NUMBER, RANK, DENSE_RANK, NTILE, COUNT_STAR, COUNT, SUM, MIN, MAX,
 FIRST_VALUE, LAST_VALUE, LAG, LEAD) = range(13)
ROWS, RANGE = 0, 1
UNBOUNDED = -1
OUT_SORTED = 1
MAX_FUNCS = 8
MAX_KEYS = 4
# the scan geometry of gpue.hip: T rows per scan tile (GPUE_WIN_TILE), A tile
# aggregates per sweep of the middle pass
T = 2048
A = 1024
FN_NAMES = {"row_number": ROW_NUMBER, "rank": RANK, "dense_rank": DENSE_RANK, "ntile": NTILE,
            "count_star": COUNT_STAR, "count": COUNT, "sum": SUM, "min": MIN, "max": MAX,
            "first_value": FIRST_VALUE, "last_value": LAST_VALUE, "lag": LAG, "lead": LEAD}
_DT = {PT_I32: np.int32, PT_I64: np.int64}
_I64 = (-(1 << 63), (1 << 63) - 1)


def has_input(fn):
    return fn >= COUNT


def is_framed(fn):
    return COUNT_STAR <= fn <= LAST_VALUE


class WinFunc:
    """One window function: fn (a constant above or its lower-case name), the
    input column (col, nulls, type; unused for the ranking functions, NTILE
    and COUNT_STAR), the frame (mode, lo preceding, hi following; the default
    is SQL's RANGE UNBOUNDED PRECEDING .. CURRENT ROW; ignored outside the
    framed functions) and param0 / param1 / has_default (NTILE's bucket count;
    LAG / LEAD's offset and default). nullable defaults to `nulls is not
    None`."""

    def __init__(self, fn, col=None, nulls=None, type=PT_I64, nullable=None, mode=RANGE,
                 lo=UNBOUNDED, hi=0, param0=0, param1=0, has_default=False):
        self.fn = FN_NAMES[fn] if isinstance(fn, str) and fn in FN_NAMES else fn
        self.col, self.nulls, self.type = col, nulls, type
        self.nullable = (nulls is not None) if nullable is None else bool(nullable)
        self.mode, self.lo, self.hi = mode, lo, hi
        self.param0, self.param1, self.has_default = param0, param1, bool(has_default)

    def with_cols(self, col, nulls):
        """The same function over other buffers (host arrays <-> device)."""
        return WinFunc(self.fn, col, nulls, self.type, self.nullable, self.mode, self.lo,
                       self.hi, self.param0, self.param1, self.has_default)


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


class WindowSpec:
    """Everything of a gpue_window_eval call but the buffers, validated as the
    C side validates it."""

    def __init__(self, part_types, part_nullable, order_types, order_nullable, funcs):
        self.part_types = list(part_types)
        self.part_nullable = [bool(x) for x in part_nullable]
        self.order_types = list(order_types)
        self.order_nullable = [bool(x) for x in order_nullable]
        self.funcs = list(funcs)
        for what, types, nullable in (("partition", self.part_types, self.part_nullable),
                                      ("order", self.order_types, self.order_nullable)):
            if len(types) > MAX_KEYS:
                raise ValueError(f"{len(types)} {what} keys, outside 0..{MAX_KEYS}")
            if len(types) != len(nullable):
                raise ValueError(f"{what} key types and nullability differ in length")
            for t in types:
                if isinstance(t, bool) or t not in _DT:
                    raise ValueError(f"unknown {what} key type {t!r}")
        if not 1 <= len(self.funcs) <= MAX_FUNCS:
            raise ValueError(f"n_funcs {len(self.funcs)} outside 1..{MAX_FUNCS}")
        for a, f in enumerate(self.funcs):
            if isinstance(f.fn, bool) or not _is_int(f.fn) or not ROW_NUMBER <= f.fn <= LEAD:
                raise ValueError(f"function {a}: unknown function {f.fn!r}")
            if has_input(f.fn) and (isinstance(f.type, bool) or f.type not in _DT):
                raise ValueError(f"function {a}: unknown input type {f.type!r}")
            if is_framed(f.fn):
                if isinstance(f.mode, bool) or f.mode not in (ROWS, RANGE):
                    raise ValueError(f"function {a}: unknown frame mode {f.mode!r}")
                if not (_is_int(f.lo) and _is_int(f.hi)) or f.lo < UNBOUNDED or f.hi < UNBOUNDED:
                    raise ValueError(f"function {a}: frame bounds must be >= 0 or UNBOUNDED")
                if f.mode == RANGE and (f.lo != UNBOUNDED or f.hi not in (0, UNBOUNDED)):
                    raise ValueError(f"function {a}: a RANGE frame is UNBOUNDED PRECEDING to "
                                     "CURRENT ROW or UNBOUNDED FOLLOWING")
                if f.fn in (MIN, MAX) and f.lo != UNBOUNDED:
                    raise ValueError(f"function {a}: MIN / MAX need frame_lo UNBOUNDED "
                                     "(no sliding minimum)")
            elif f.fn == NTILE:
                if not _is_int(f.param0) or f.param0 < 1:
                    raise ValueError(f"function {a}: NTILE needs a bucket count >= 1")
            elif f.fn in (LAG, LEAD):
                if not _is_int(f.param0) or f.param0 < 0:
                    raise ValueError(f"function {a}: LAG / LEAD need an offset >= 0")
            for p in (f.param0, f.param1):
                if not _is_int(p) or not _I64[0] <= p <= _I64[1]:
                    raise ValueError(f"function {a}: parameters are int64")

    @classmethod
    def of(cls, part_keys, order_keys, funcs):
        """From column tuples: a key is nullable iff a null column is given."""
        return cls([k[2] for k in part_keys], [k[1] is not None for k in part_keys],
                   [k[2] for k in order_keys], [k[1] is not None for k in order_keys], funcs)

    @property
    def n_funcs(self):
        return len(self.funcs)

    @property
    def out_nullable(self):
        """The static rule: never for the ranking functions, NTILE, COUNT_STAR
        and COUNT; iff the input was declared nullable for SUM / MIN / MAX /
        FIRST_VALUE / LAST_VALUE; LAG / LEAD unless has_default is set and
        the input is not nullable."""
        out = []
        for f in self.funcs:
            if f.fn in (LAG, LEAD):
                out.append(not (f.has_default and not f.nullable))
            else:
                out.append(SUM <= f.fn <= LAST_VALUE and f.nullable)
        return out

    def check_eval(self, n_rows, order_idx, part_keys, order_keys, ins, outs, flags=0):
        """order_idx = buffer or None; part_keys / order_keys / ins / outs =
        [(values, nulls or None)]; buffers are anything with .nbytes."""
        if isinstance(flags, bool) or flags not in (0, OUT_SORTED):
            raise ValueError(f"unknown flags {flags!r}")
        if not 0 <= n_rows < 1 << 32:
            raise ValueError("n_rows must be below 2^32")
        if (len(part_keys) != len(self.part_types) or len(order_keys) != len(self.order_types)
                or len(ins) != self.n_funcs or len(outs) != self.n_funcs):
            raise ValueError("column lists do not match the spec")
        read, written = [], []
        if order_idx is not None:
            if order_idx.nbytes < n_rows * 4:
                raise ValueError("order_idx is shorter than n_rows")
            read.append(order_idx)

        def column(what, v, nl, width, nullable):
            if v is None:
                raise ValueError(f"{what} column is missing")
            if v.nbytes < n_rows * width:
                raise ValueError(f"{what} column is shorter than n_rows")
            read.append(v)
            if nl is not None:
                if not nullable:
                    raise ValueError(f"null column for {what}, declared NOT NULL")
                if nl.nbytes < n_rows:
                    raise ValueError(f"null column of {what} is shorter than n_rows")
                read.append(nl)

        for k, (v, nl) in enumerate(part_keys):
            column(f"partition key {k}", v, nl, 8 if self.part_types[k] == PT_I64 else 4,
                   self.part_nullable[k])
        for k, (v, nl) in enumerate(order_keys):
            column(f"order key {k}", v, nl, 8 if self.order_types[k] == PT_I64 else 4,
                   self.order_nullable[k])
        for a, (f, (v, nl)) in enumerate(zip(self.funcs, ins)):
            if has_input(f.fn):
                column(f"input of function {a}", v, nl, 8 if f.type == PT_I64 else 4,
                       f.nullable)
        for a, ((v, nl), nullable) in enumerate(zip(outs, self.out_nullable)):
            if v is None or v.nbytes < n_rows * 8:
                raise ValueError(f"output {a} is missing or shorter than n_rows")
            written.append(v)
            if nullable:
                if nl is None or nl.nbytes < n_rows:
                    raise ValueError(f"null output of function {a} is missing or short")
                written.append(nl)
        if len({id(b) for b in written}) != len(written):
            raise ValueError("an output buffer is used twice")
        if {id(b) for b in written} & {id(b) for b in read}:
            raise ValueError("an output buffer is also an input")


def _key_mat(keys, n):
    """Per key: (is-NULL bool, value int64 with 0 under NULL), n rows."""
    out = []
    for v, nl, t in keys:
        v = np.asarray(v)[:n].astype(_DT[t]).astype(np.int64)
        isn = np.zeros(n, bool) if nl is None else np.asarray(nl)[:n] != 0
        out.append((isn, np.where(isn, 0, v)))
    return out


def sort_perm_ref(part_keys, order_keys, flags, n):
    """The permutation gpue_topn pins for the window sort: partition keys
    ascending NULLS FIRST, then order key j by flags[j] = (desc, nulls_first);
    a NULL sorts by its placement whatever the direction and the value under
    it is never read; rows equal on every key stay in ascending row index.
    Returns uint32[n]."""
    if len(flags) != len(order_keys):
        raise ValueError("one (desc, nulls_first) pair per order key")
    cols = []
    spec = [(False, True)] * len(part_keys) + [(bool(d), bool(nf)) for d, nf in flags]
    for (isn, v), (desc, nulls_first) in zip(_key_mat(list(part_keys) + list(order_keys), n),
                                             spec):
        cols.append(np.where(isn, 0, 1) if nulls_first else np.where(isn, 1, 0))
        cols.append(~v if desc else v)       # ~v = -v-1: order reversed, no overflow
    if not cols:
        return np.arange(n, dtype=np.uint32)
    return np.lexsort(cols[::-1]).astype(np.uint32)    # lexsort is stable


def _bounds(part_keys, order_keys, perm, n):
    """part_start, part_end, peer_start, peer_end and the peer-start flags,
    all in sorted order."""
    pos = np.arange(n, dtype=np.int64)

    def starts(keys, flag):
        for isn, v in _key_mat(keys, n):
            isn, v = isn[perm], v[perm]
            flag[1:] |= (isn[1:] != isn[:-1]) | (~isn[1:] & (v[1:] != v[:-1]))
        return flag

    first = np.zeros(n, bool)
    first[0] = True
    pflag = starts(part_keys, first.copy())
    qflag = starts(order_keys, pflag.copy())

    def runs(flag):
        start = np.maximum.accumulate(np.where(flag, pos, 0))
        last = np.append(flag[1:], True)          # row i ends a run iff i+1 starts one
        end = np.minimum.accumulate(np.where(last, pos, n)[::-1])[::-1]
        return start, end

    ps, pe = runs(pflag)
    qs, qe = runs(qflag)
    return ps, pe, qs, qe, qflag


def _running_extreme(vals, has, ps, is_max):
    """Running MIN / MAX since the partition start over the rows where `has`:
    returns (value, seen-any). Ranks shifted by partition make one global
    accumulate segment-local: every rank of a later partition lies below
    (above, for MAX) every rank of an earlier one."""
    n = len(vals)
    uniq, rank = np.unique(vals, return_inverse=True)
    rank = np.asarray(rank, np.int64).reshape(-1)
    seg = np.cumsum(np.append(True, ps[1:] != ps[:-1])) - 1
    width = len(uniq) + 1                          # rank `len(uniq)` = "no value"
    if is_max:
        w = np.where(has, rank + 1, 0) + seg * width
        acc = np.maximum.accumulate(w) - seg * width
        seen = acc > 0
        return np.where(seen, uniq[np.maximum(acc - 1, 0)], 0), seen
    w = np.where(has, rank, width - 1) - seg * width
    acc = np.minimum.accumulate(w) + seg * width
    seen = acc < width - 1
    return np.where(seen, uniq[np.minimum(acc, len(uniq) - 1)], 0), seen


def window_ref(part_keys, order_keys, funcs, n, order_idx=None, sorted_out=False):
    """numpy reference of one gpue_window_eval call over host arrays. Returns
    [(values int64[n], nulls u8[n] or None), ...] in exactly the written
    representation: 0 under NULL, null columns 1/0 and only where the output is
    nullable; at out[order_idx[i]], or at out[i] with sorted_out."""
    spec = WindowSpec.of(part_keys, order_keys, funcs)
    if not 0 <= n < 1 << 32:
        raise ValueError("n_rows must be below 2^32")
    for a, f in enumerate(funcs):
        if has_input(f.fn) and f.col is None:
            raise ValueError(f"input column of function {a} is missing")
        if f.nulls is not None and not f.nullable:
            raise ValueError(f"null column for input of function {a}, declared NOT NULL")
    if n == 0:
        return [(np.empty(0, np.int64), np.empty(0, np.uint8) if nl else None)
                for nl in spec.out_nullable]
    perm = (np.arange(n, dtype=np.int64) if order_idx is None
            else np.asarray(order_idx)[:n].astype(np.int64))
    ps, pe, qs, qe, qflag = _bounds(part_keys, order_keys, perm, n)
    pos = np.arange(n, dtype=np.int64)
    results = []
    for f, nullable_out in zip(funcs, spec.out_nullable):
        isn_out = np.zeros(n, bool)
        if has_input(f.fn):
            v = np.asarray(f.col)[perm].astype(_DT[f.type]).astype(np.int64)
            isn = (np.zeros(n, bool) if f.nulls is None
                   else np.asarray(f.nulls)[perm] != 0)
            v = np.where(isn, 0, v)
        lo, hi = ps, pe
        if is_framed(f.fn):
            if f.mode == RANGE:
                hi = qe if f.hi == 0 else pe
            else:
                if f.lo != UNBOUNDED:
                    lo = np.where(f.lo < pos - ps, pos - min(f.lo, n), ps)
                if f.hi != UNBOUNDED:
                    hi = np.where(f.hi < pe - pos, pos + min(f.hi, n), pe)

        def framed(prefix):              # prefix[hi] - prefix[lo-1], wrapping
            return prefix[hi] - np.where(lo > 0, prefix[np.maximum(lo - 1, 0)], 0).astype(
                prefix.dtype)

        def at(p, inside):               # the input at sorted position p where inside
            p = np.where(inside, p, 0)
            return np.where(inside, v[p], 0), np.where(inside, isn[p], False)

        if f.fn == ROW_NUMBER:
            val = pos - ps + 1
        elif f.fn == RANK:
            val = qs - ps + 1
        elif f.fn == DENSE_RANK:
            d = np.cumsum(qflag.astype(np.int64))
            val = d - d[ps] + 1
        elif f.fn == NTILE:
            size = pe - ps + 1
            q, r, rn0 = size // f.param0, size % f.param0, pos - ps
            thr = r * (q + 1)
            val = np.where(rn0 < thr, rn0 // (q + 1) + 1,
                           r + (rn0 - thr) // np.maximum(q, 1) + 1)
        elif f.fn == COUNT_STAR:
            val = hi - lo + 1
        elif f.fn == COUNT:
            val = framed(np.cumsum((~isn).astype(np.int64)))
        elif f.fn == SUM:
            val = framed(np.cumsum(v.astype(np.uint64))).astype(np.int64)   # mod 2^64
            isn_out = framed(np.cumsum((~isn).astype(np.int64))) == 0
        elif f.fn in (MIN, MAX):
            run, seen = _running_extreme(v, ~isn, ps, f.fn == MAX)
            val, isn_out = run[hi], ~seen[hi]
        elif f.fn == FIRST_VALUE:
            val, isn_out = at(lo, np.ones(n, bool))
        elif f.fn == LAST_VALUE:
            val, isn_out = at(hi, np.ones(n, bool))
        else:
            k = min(f.param0, n)
            p = pos - k if f.fn == LAG else pos + k
            inside = (p >= ps) & (p <= pe)
            val, isn_out = at(p, inside)
            if f.has_default:
                val = np.where(inside, val, f.param1)
            else:
                isn_out = isn_out | ~inside
        val = np.where(isn_out, 0, val).astype(np.int64)
        if not sorted_out and order_idx is not None:
            out = np.empty(n, np.int64)
            out[perm] = val
            nul = np.empty(n, np.uint8)
            nul[perm] = isn_out
        else:
            out, nul = val, isn_out.astype(np.uint8)
        assert nullable_out or not isn_out.any()
        results.append((out, nul if nullable_out else None))
    return results
