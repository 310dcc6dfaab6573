"""Operator-shaped pipeline driver — the §8b boundary in the reference's own
vocabulary.

Mirrors `pipeline::Operator` (reference
be/src/exec_primitive/pipeline/operator.h:48: push_chunk/pull_chunk at
:141-144, lifecycle prepare -> finishing -> finished -> close at :59-102) and
the `PipelineDriver::process` hot loop (be/src/exec/runtime/
pipeline_driver.cpp:391-500: for each adjacent operator pair with
has_output()/need_input(), pull_chunk then push_chunk, finishing propagated
down the chain once an operator is finished and drained).

This is the THIN host-side driver SURVEY.md §2 keeps: one driver <-> one HIP
stream; every pull/push pair on the GPU operators below is a kernel launch on
the session stream, and the chunks that flow between operators are device
columnar buffers that never leave HBM. The reference's 4096-row chunks
(common/config.h:1102) are sized for L2+SIMD on a CPU; ours default to 4 M
rows — the smallest chunk that still fills 256 CUs (DESIGN.md §4's grid
findings) — with the same semantics.

The driver logic itself is backend-free (CPU-tested with plain-python
operators in tests/test_pipeline_driver.py); the GPU operators
(ChunkSourceOperator -> HashJoinBuildOperator / HashJoinProbeOperator ->
AggregateSinkOperator) are parity-tested against the oracle end to end in
tests/test_gpu_parity.py.
"""

import numpy as np


class Operator:
    """Lifecycle per operator.h:59-102. Subclasses override the four data
    methods; the driver owns when they are called."""

    def __init__(self):
        self._finishing = False
        self._closed = False

    def prepare(self):
        pass

    def has_output(self) -> bool:
        raise NotImplementedError

    def need_input(self) -> bool:
        raise NotImplementedError

    def push_chunk(self, chunk) -> None:
        raise NotImplementedError

    def pull_chunk(self):
        raise NotImplementedError

    def set_finishing(self):
        """Upstream has no more chunks (hash_join_build_operator.cpp:87-96
        triggers build_ht here)."""
        self._finishing = True

    def is_finished(self) -> bool:
        """No more output will ever be produced."""
        return self._finishing and not self.has_output()

    def close(self):
        self._closed = True

    def result(self):
        """Sinks override; pass-through operators have no result."""
        return None


class PipelineDriver:
    """pipeline_driver.cpp:391-500 restated: repeatedly sweep adjacent pairs;
    move one chunk wherever curr.has_output() && next.need_input(); propagate
    set_finishing down the chain when an upstream operator is finished. A
    `process()` call runs until the whole chain is finished (no time-slice /
    blocked states — the GPU stream absorbs the asynchrony the reference's
    poller exists for)."""

    def __init__(self, operators):
        assert len(operators) >= 2
        self.ops = operators

    def process(self):
        for op in self.ops:
            op.prepare()
        self.ops[0].set_finishing()  # sources own their input
        moved = True
        while True:
            moved = False
            for curr, nxt in zip(self.ops, self.ops[1:]):
                while curr.has_output() and nxt.need_input():
                    nxt.push_chunk(curr.pull_chunk())
                    moved = True
                if curr.is_finished() and not nxt._finishing:
                    nxt.set_finishing()
                    moved = True
            if not moved:
                break
        assert all(op.is_finished() for op in self.ops), "pipeline stalled"
        for op in self.ops:
            op.close()
        return self.ops[-1].result()


# ---------------------------------------------------------------------------
# GPU operators. A chunk is {"n": rows, "cols": [DBuf, ...]} resident in HBM.
# ---------------------------------------------------------------------------

DEFAULT_CHUNK_ROWS = 4 << 20


class ChunkSourceOperator(Operator):
    """Synthetic columnar source standing in for the scan operator
    (storage is out of scope; the source yields
    BASELINE-shaped chunks straight into HBM). gen(row_start, n) -> chunk."""

    def __init__(self, gen, total_rows, chunk_rows=DEFAULT_CHUNK_ROWS):
        super().__init__()
        self._gen = gen
        self._total = total_rows
        self._chunk = chunk_rows
        self._next_row = 0

    def need_input(self):
        return False

    def has_output(self):
        return self._next_row < self._total

    def pull_chunk(self):
        n = min(self._chunk, self._total - self._next_row)
        c = self._gen(self._next_row, n)
        self._next_row += n
        return c


class HashJoinBuildOperator(Operator):
    """push_chunk appends build-side chunks (hash_joiner.cpp:221); the table
    is built once, at set_finishing (hash_join_build_operator.cpp:87-96).
    Produces no chunks — downstream probe operators reference the one
    read-only table (hash_join_probe_operator.cpp:105-111)."""

    def __init__(self, engine, build_fn):
        super().__init__()
        self._e = engine
        self._build_fn = build_fn
        self._pending = []
        self.table = None

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def push_chunk(self, chunk):
        self._pending.append(chunk)

    def set_finishing(self):
        super().set_finishing()
        self.table = self._build_fn(self._e, self._pending)
        for c in self._pending:
            for b in c["cols"]:
                b.free()
        self._pending = []

    def close(self):
        # close() keeps the table: probe operators in the dependent pipeline
        # share the one read-only table after the build pipeline closes
        # (hash_join_probe_operator.cpp:105-111 clone_readable_table).
        # release() drops it once the probers are done.
        super().close()

    def release(self):
        if self.table is not None:
            self.table.destroy()
            self.table = None


class HashJoinProbeOperator(Operator):
    """Push one probe chunk, pull result chunks until drained
    (hash_join_components.cpp:65-82). The chain-walk emit is the engine's
    two-phase count/emit, so one probe chunk yields exactly one (exactly
    sized) result chunk — the reference's resumable cursor collapses into
    the count pass."""

    def __init__(self, engine, build_op, key_col=0):
        super().__init__()
        self._e = engine
        self._build_op = build_op
        self._key_col = key_col
        self._in = None
        self._out = None

    def need_input(self):
        return self._in is None and self._out is None and not self._finishing

    def has_output(self):
        if self._in is not None:
            self._probe()
        return self._out is not None

    def push_chunk(self, chunk):
        self._in = chunk

    def _probe(self):
        c, self._in = self._in, None
        t = self._build_op.table
        keys = c["cols"][self._key_col]
        cnt = self._e.join_probe_emit(t, keys, c["n"])
        op_buf = self._e.alloc(max(cnt, 1) * 4)
        ob_buf = self._e.alloc(max(cnt, 1) * 4)
        self._e.join_probe_emit(t, keys, c["n"], op_buf, ob_buf)
        # gather the probe-side payload columns through the match indices
        # (join_hash_map.hpp:284-330 _probe_output/append_selective)
        out_cols = []
        for i, col in enumerate(c["cols"]):
            if i == self._key_col:
                continue
            g = self._e.alloc(max(cnt, 1) * 4)
            if cnt > 0:
                self._e.gather_u32(col, op_buf, cnt, g)
            out_cols.append(g)
        for b in (op_buf, ob_buf, *c["cols"]):
            b.free()
        self._out = {"n": cnt, "cols": out_cols}

    def pull_chunk(self):
        if self._out is None:
            self._probe()
        c, self._out = self._out, None
        return c


class AggregateSinkOperator(Operator):
    """Blocking agg sink (aggregate_blocking_sink_operator.cpp:114-151):
    consumes every chunk into accumulator state; result() finalizes."""

    def __init__(self, engine, update_fn, result_fn):
        super().__init__()
        self._e = engine
        self._update = update_fn
        self._result = result_fn
        self._state = None

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def push_chunk(self, chunk):
        self._state = self._update(self._e, self._state, chunk)
        for b in chunk["cols"]:
            b.free()

    def result(self):
        return self._result(self._e, self._state)


class StreamingAggOperator(Operator):
    """AUTO-mode streaming pre-aggregation
    (aggregate_streaming_sink_operator.cpp:224-310): per chunk, the state
    machine INIT_PREAGG -> ADJUST -> {PASS_THROUGH | PREAGG |
    SELECTIVE_PREAGG} decides between aggregating into the local table,
    streaming the chunk through to the downstream (merge) aggregate, or the
    selective mix (aggregate rows whose group already exists, stream the
    rest). Thresholds are the reference's (aggregator.h:175-178,
    aggregator.cpp:150-160): LowReduction 0.2, HighReduction 0.9,
    StableLimit 5 consecutive chunks to leave ADJUST; hit count =
    build_hash_map_with_selection's existing-group rows. At finishing the
    local table streams out as pre-aggregated partials (cnt column set), the
    merge_batch form (aggregate.h:158-168).

    Chunks: {"n", "keys": DBuf u64, "vals": DBuf i64, "cnts": DBuf|None}.
    """

    LOW_REDUCTION = 0.2     # aggregator.h:175
    HIGH_REDUCTION = 0.9    # aggregator.h:176
    STABLE_LIMIT = 5        # aggregator.h:178

    def __init__(self, engine, capacity=1 << 20, max_groups=1 << 20):
        super().__init__()
        self._e = engine
        self._at = engine.agg_table_create(capacity)
        engine.agg_table_reset(self._at)
        self._max_groups = max_groups
        self._out = []
        self._state = "INIT_PREAGG"
        self._counts = {"pass": 0, "preagg": 0, "selective": 0, "adjust": 0}
        self._drained = False

    def need_input(self):
        return not self._finishing and not self._out

    def has_output(self):
        if self._finishing and not self._drained:
            self._drain()
        return bool(self._out)

    def pull_chunk(self):
        return self._out.pop(0)

    def _preagg(self, c):
        # reference shape: try_convert_to_two_level_map runs before each
        # chunk (aggregator.cpp:1237-1241) — here the table grows + rehashes
        # so the push can never overflow (gpue_agg_table_ensure)
        self._e.agg_table_ensure(self._at, c["n"])
        self._e.hash_agg_push(self._at, c["keys"], c["vals"], c["n"], cnts=c.get("cnts"))
        for b in (c["keys"], c["vals"]):
            b.free()

    def _stream(self, c):
        self._out.append(c)

    def _selective(self, c):
        import numpy as np
        n = c["n"]
        mask = self._e.alloc(n)
        self._e.hash_agg_push(self._at, c["keys"], c["vals"], n, cnts=c.get("cnts"),
                              update_only=1, miss_mask=mask)
        m = mask.d2h(np.uint8, n)
        miss = np.flatnonzero(m).astype(np.uint32)
        mask.free()
        if len(miss):
            idx = self._e.alloc(miss.nbytes)
            idx.h2d(miss)
            ks = self._e.alloc(len(miss) * 8)
            vs = self._e.alloc(len(miss) * 8)
            self._e.gather_u64(c["keys"], idx, len(miss), ks)
            self._e.gather_u64(c["vals"], idx, len(miss), vs)
            idx.free()
            self._out.append({"n": len(miss), "keys": ks, "vals": vs, "cnts": None})
        for b in (c["keys"], c["vals"]):
            b.free()

    def push_chunk(self, c):
        n = c["n"]
        if self._state == "INIT_PREAGG":
            # first chunks always pre-aggregate; leave for ADJUST once the
            # table stops reducing (ht expansion heuristic simplified to the
            # reduction test on the next chunk)
            hits = self._e.hash_agg_probe_hits(self._at, c["keys"], n)
            if self._counts["adjust"] == 0 or hits >= self.HIGH_REDUCTION * n:
                self._counts["adjust"] += 1
                self._preagg(c)
                return
            self._state = "ADJUST"
        if self._state == "ADJUST":
            hits = self._e.hash_agg_probe_hits(self._at, c["keys"], n)
            if hits <= self.LOW_REDUCTION * n:
                self._stream(c)
                self._counts["pass"] += 1
                self._counts["preagg"] = self._counts["selective"] = 0
                if self._counts["pass"] >= self.STABLE_LIMIT:
                    self._state = "PASS_THROUGH"
            elif hits >= self.HIGH_REDUCTION * n:
                self._preagg(c)
                self._counts["preagg"] += 1
                self._counts["pass"] = self._counts["selective"] = 0
                if self._counts["preagg"] >= self.STABLE_LIMIT:
                    self._state = "PREAGG"
            else:
                self._selective(c)
                self._counts["selective"] += 1
                self._counts["pass"] = self._counts["preagg"] = 0
                if self._counts["selective"] >= self.STABLE_LIMIT:
                    self._state = "SELECTIVE_PREAGG"
        elif self._state == "PASS_THROUGH":
            self._stream(c)
        elif self._state == "SELECTIVE_PREAGG":
            self._selective(c)
        else:
            self._preagg(c)

    def _drain(self):
        """Finishing: the local table streams out as pre-agg partials."""
        self._drained = True
        ok = self._e.alloc(self._max_groups * 8)
        os_ = self._e.alloc(self._max_groups * 8)
        oc = self._e.alloc(self._max_groups * 8)
        g = self._e.hash_agg_emit(self._at, ok, os_, self._max_groups, out_counts=oc)
        if g:
            self._out.append({"n": g, "keys": ok, "vals": os_, "cnts": oc})
        else:
            for b in (ok, os_, oc):
                b.free()

    def close(self):
        self._e.agg_table_destroy(self._at)
        super().close()


class FinalAggSink(Operator):
    """The downstream (merge) aggregate: accepts raw rows AND pre-agg
    partials (cnts set) into one table — merge_batch semantics."""

    def __init__(self, engine, capacity=1 << 20, max_groups=1 << 20):
        super().__init__()
        self._e = engine
        self._at = engine.agg_table_create(capacity)
        engine.agg_table_reset(self._at)
        self._max_groups = max_groups

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def push_chunk(self, c):
        self._e.hash_agg_push(self._at, c["keys"], c["vals"], c["n"], cnts=c.get("cnts"))
        for b in (c["keys"], c["vals"], c.get("cnts")):
            if b is not None:
                b.free()

    def result(self):
        import numpy as np
        ok = self._e.alloc(self._max_groups * 8)
        os_ = self._e.alloc(self._max_groups * 8)
        oc = self._e.alloc(self._max_groups * 8)
        g = self._e.hash_agg_emit(self._at, ok, os_, self._max_groups, out_counts=oc)
        keys = ok.d2h(np.uint64, g)
        sums = os_.d2h(np.int64, g)
        cnts = oc.d2h(np.int64, g)
        for b in (ok, os_, oc):
            b.free()
        self._e.agg_table_destroy(self._at)
        order = np.argsort(keys)
        return keys[order], sums[order], cnts[order]


class TopNSinkOperator(Operator):
    """ORDER BY ... LIMIT/OFFSET sink — the ChunksSorterTopn analog
    (exec/chunks_sorter_topn.cpp: update() per pushed chunk keeps a bounded
    candidate set, done()/get_next yields the ordered rows).

    Chunks are {"n": rows, "cols": [DBuf, ...]}; col_dtypes gives each
    column's numpy dtype (4- or 8-byte items). sort_keys is a list of
    (col_index, type, desc), most significant first, type as Engine.topn
    (0 int32 / 1 int64 / 2 uint64). Sort keys are NOT NULL columns here: the
    candidate set is re-materialized with gather_u32/gather_u64, and there is
    no u8 gather for a null mask — nullable keys go through Engine.topn
    directly.

    Per push: topn over the chunk for K = offset+limit rows, gather every
    column through the surviving indices, append to the candidate columns;
    when the append would pass the bound (bound_factor * K rows, >= 2K) the
    candidates are first cut back to K by topn over themselves. result() runs
    the final topn with the real offset/limit.

    Stable tie-break across chunks: topn returns rows that are equal on every
    key in ascending row index, the candidate set is kept in that sorted
    order, and new survivors are appended behind it in arrival order. So rows
    equal on every key always sit in the candidate set in global row order,
    a later topn over the candidates (whose tie-break is candidate position)
    preserves it, and whenever ties are cut the latest-arrived rows go first
    — exactly the one-shot result, for free.

    Uses only engine.alloc / topn / gather_u32 / gather_u64 / dbuf_d2d and
    DBuf.d2h / free, so the merge logic runs against a numpy stand-in engine
    without a GPU."""

    def __init__(self, engine, sort_keys, col_dtypes, limit, offset=0, bound_factor=4):
        super().__init__()
        assert bound_factor >= 2 and limit >= 0 and offset >= 0
        self._e = engine
        self._keys = list(sort_keys)
        self._dtypes = [np.dtype(d) for d in col_dtypes]
        assert all(d.itemsize in (4, 8) for d in self._dtypes)
        self._limit = limit
        self._offset = offset
        self._k = offset + limit
        self.capacity = bound_factor * self._k   # the stated candidate bound (rows)
        self.max_candidate_rows = 0              # high-water mark, for tests
        self._cand = None                        # candidate columns, capacity rows each
        self._n = 0

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def _key_desc(self, cols):
        return [(cols[c], None, t, d, False) for c, t, d in self._keys]

    def _gather(self, cols, idx, cnt):
        out = []
        for col, dt in zip(cols, self._dtypes):
            g = self._e.alloc(max(cnt, 1) * dt.itemsize)
            if cnt:
                (self._e.gather_u32 if dt.itemsize == 4 else self._e.gather_u64)(
                    col, idx, cnt, g)
            out.append(g)
        return out

    def _append(self, cols, cnt):
        if self._cand is None:
            self._cand = [self._e.alloc(max(self.capacity, 1) * dt.itemsize)
                          for dt in self._dtypes]
        for src, dst, dt in zip(cols, self._cand, self._dtypes):
            self._e.dbuf_d2d(src, dst, cnt * dt.itemsize, 0, self._n * dt.itemsize)
        self._n += cnt
        self.max_candidate_rows = max(self.max_candidate_rows, self._n)

    def _cut(self):
        """Candidates -> their own top K, sorted."""
        idx, cnt = self._e.topn(self._key_desc(self._cand), self._n, self._k, 0)
        kept = self._gather(self._cand, idx, cnt)
        idx.free()
        self._n = 0
        self._append(kept, cnt)
        for b in kept:
            b.free()

    def push_chunk(self, chunk):
        n, cols = chunk["n"], chunk["cols"]
        if n and self._k:
            idx, cnt = self._e.topn(self._key_desc(cols), n, self._k, 0)
            surv = self._gather(cols, idx, cnt)
            idx.free()
            if self._n + cnt > self.capacity:
                self._cut()          # -> at most K rows; K + cnt <= 2K <= capacity
            self._append(surv, cnt)
            for b in surv:
                b.free()
        for b in cols:
            b.free()

    def result(self):
        """Final ordered rows as one numpy array per column."""
        if self._cand is None:
            return [np.empty(0, dt) for dt in self._dtypes]
        idx, cnt = self._e.topn(self._key_desc(self._cand), self._n, self._limit,
                                self._offset)
        final = self._gather(self._cand, idx, cnt)
        idx.free()
        out = [b.d2h(dt, cnt) for b, dt in zip(final, self._dtypes)]
        for b in final + self._cand:
            b.free()
        self._cand = None
        self._n = 0
        return out


class FilterOperator(Operator):
    """WHERE as a pass-through operator — the ChunkPredicateEvaluator::
    eval_conjuncts + Chunk::filter step of the reference's scan / filter
    operators, for a whole predicate tree (starrocks_amd/predicate.py forms:
    and / or / not / cmp / cmp_col / between / in / is_null, SQL three-valued
    logic).

    Chunks are {"n": rows, "cols": [DBuf, ...]}. pred_col_map[i] = (chunk
    column index, chunk column index of its u8 null mask or None, type 0
    int32 / 1 int64) binds predicate column i of the tree; col_widths[k] is
    the byte width (1, 4 or 8) of chunk column k — a nullable column's null
    mask is just another width-1 chunk column, so it is compacted with its
    values. The tree is compiled once, at construction.

    Per pushed chunk: one pred_eval_mask pass over the predicate columns into
    a 1-bit-per-row mask, exact-size output columns, one mask_compact over
    every chunk column; the input columns are freed. One chunk in, one chunk
    out (possibly with n == 0), rows in their input order.

    Uses only engine.alloc / pred_eval_mask / mask_compact and DBuf.free, so
    it runs against a numpy stand-in engine without a GPU."""

    def __init__(self, engine, tree, pred_col_map, col_widths):
        super().__init__()
        from starrocks_amd.predicate import compile_predicate
        self._e = engine
        self._map = [(int(c), None if nl is None else int(nl), int(t))
                     for c, nl, t in pred_col_map]
        self._widths = [int(w) for w in col_widths]
        if any(w not in (1, 4, 8) for w in self._widths):
            raise ValueError("column widths must be 1, 4 or 8 bytes")
        for c, nl, t in self._map:
            if not 0 <= c < len(self._widths) or self._widths[c] != (8 if t == 1 else 4):
                raise ValueError(f"predicate column {c} does not match its declared type")
            if nl is not None and (not 0 <= nl < len(self._widths) or self._widths[nl] != 1):
                raise ValueError(f"null mask column {nl} must be a width-1 chunk column")
        self._program = compile_predicate(tree, [t for _, _, t in self._map])
        self._out = None
        self.rows_in = 0
        self.rows_out = 0

    def need_input(self):
        return self._out is None and not self._finishing

    def has_output(self):
        return self._out is not None

    def push_chunk(self, chunk):
        n, cols = chunk["n"], chunk["cols"]
        assert len(cols) == len(self._widths)
        mask = self._e.alloc(max((n + 63) // 64, 1) * 8)
        pred_cols = [(cols[c], None if nl is None else cols[nl], t) for c, nl, t in self._map]
        cnt = self._e.pred_eval_mask(pred_cols, self._program, n, mask)
        out = [self._e.alloc(max(cnt * w, 1)) for w in self._widths]
        got = self._e.mask_compact(mask, n, list(zip(cols, out, self._widths)))
        assert got == cnt
        for b in (mask, *cols):
            b.free()
        self.rows_in += n
        self.rows_out += cnt
        self._out = {"n": cnt, "cols": out}

    def pull_chunk(self):
        c, self._out = self._out, None
        return c


class ProjectOperator(Operator):
    """Project as a pass-through operator — ExprContext::evaluate over
    arithmetic, cast and conditional expressions between scan / filter and
    join / agg (starrocks_amd/expr.py forms).

    Chunks are {"n": rows, "cols": [DBuf, ...]}. col_map[i] = (chunk column
    index, chunk column index of its u8 null mask or None, type 0 int32 / 1
    int64) binds input column i of the trees, as in FilterOperator. keep lists
    the chunk columns passed through, in that order; every other input column
    is freed. The output chunk is the kept columns, then per expression its
    value column (int32 / int64 per out_types[k], or the selection bitmap for
    XO_MASK) followed by a width-1 null column iff the expression is nullable
    (never for XO_MASK). The trees are compiled once, at construction;
    out_widths gives the byte width of every output chunk column (8 for a
    bitmap: its u64 words).

    Per pushed chunk: exact-size outputs and one expr_project pass. One chunk
    in, one chunk out, same n.

    Uses only engine.alloc / expr_project and DBuf.free, so it runs against a
    numpy stand-in engine without a GPU."""

    def __init__(self, engine, trees, col_map, out_types, keep):
        super().__init__()
        from starrocks_amd.expr import XO_I32, XO_I64, XO_MASK, compile_exprs
        self._e = engine
        self._map = [(int(c), None if nl is None else int(nl), int(t))
                     for c, nl, t in col_map]
        self._keep = [int(k) for k in keep]
        if len(set(self._keep)) != len(self._keep) or any(k < 0 for k in self._keep):
            raise ValueError("keep must list distinct chunk column indexes")
        if any(c < 0 or (nl is not None and nl < 0) for c, nl, _ in self._map):
            raise ValueError("chunk column indexes must be non-negative")
        self._out_types = [int(t) for t in out_types]
        self._program, self.nullable = compile_exprs(
            trees, [t for _, _, t in self._map], [nl is not None for _, nl, _ in self._map],
            self._out_types)
        self._mask_t = XO_MASK
        self._size = {XO_I32: lambda n: n * 4, XO_I64: lambda n: n * 8,
                      XO_MASK: lambda n: (n + 63) // 64 * 8}
        self.out_widths = []
        for t, nl in zip(self._out_types, self.nullable):
            self.out_widths.append(4 if t == XO_I32 else 8)
            if nl and t != XO_MASK:
                self.out_widths.append(1)
        self._out = None
        self.rows = 0

    def need_input(self):
        return self._out is None and not self._finishing

    def has_output(self):
        return self._out is not None

    def push_chunk(self, chunk):
        n, cols = chunk["n"], chunk["cols"]
        in_cols = [(cols[c], None if nl is None else cols[nl], t) for c, nl, t in self._map]
        outs = []
        for t, nl in zip(self._out_types, self.nullable):
            outs.append((self._e.alloc(max(self._size[t](n), 1)),
                         self._e.alloc(max(n, 1)) if nl and t != self._mask_t else None, t))
        self._e.expr_project(in_cols, self._program, n, outs)
        for k, b in enumerate(cols):
            if k not in self._keep:
                b.free()
        new_cols = [cols[k] for k in self._keep]
        for v, nl, _ in outs:
            new_cols.append(v)
            if nl is not None:
                new_cols.append(nl)
        self.rows += n
        self._out = {"n": n, "cols": new_cols}

    def pull_chunk(self):
        c, self._out = self._out, None
        return c


class GroupAggSinkOperator(Operator):
    """GROUP BY as a blocking sink — the AggregateBlockingSinkOperator over
    Aggregator::compute_agg_states + update_batch (merge_batch with
    merge=True), for any key tuple and aggregate list the general table takes
    (starrocks_amd/groupagg.py).

    Chunks are {"n": rows, "cols": [DBuf, ...]}. key_map[i] = (chunk column
    index, chunk column index of its u8 null mask or None, type 0 int32 / 1
    int64) binds key i, as ProjectOperator's col_map; agg_map[j] = (function
    COUNT_STAR / COUNT / SUM / MIN / MAX or its lower-case name, chunk column
    index or None for COUNT_STAR, null mask column index or None, type) binds
    aggregate j. A key or input is nullable iff it names a null mask column.
    With merge=True every aggregate input is an int64 partial state as a
    partial GROUP BY emitted it, COUNT_STAR included.

    Per pushed chunk: one push into the table (which grows as it needs to);
    every chunk column is freed. result() emits into exact-size outputs,
    drops the table and returns (n_groups, [(values, nulls or None)] per key,
    the same per aggregate) as numpy arrays, key-sorted (groupagg.sort_result).

    Uses only engine.group_agg_create / group_agg_push / group_agg_emit_alloc
    / group_agg_destroy and DBuf.d2h / free, so it runs against a numpy
    stand-in engine without a GPU."""

    def __init__(self, engine, key_map, agg_map, merge=False, capacity_hint=0):
        super().__init__()
        from starrocks_amd.groupagg import FN_NAMES, GroupAggSpec
        self._e = engine
        self._keys = [(int(c), None if nl is None else int(nl), t) for c, nl, t in key_map]
        self._aggs = [(FN_NAMES.get(f, f) if isinstance(f, str) else f,
                       None if c is None else int(c), None if nl is None else int(nl), t)
                      for f, c, nl, t in agg_map]
        self._merge = bool(merge)
        self.spec = GroupAggSpec([t for _, _, t in self._keys],
                                 [nl is not None for _, nl, _ in self._keys],
                                 [f for f, _, _, _ in self._aggs],
                                 [t for _, _, _, t in self._aggs],
                                 [nl is not None for _, _, nl, _ in self._aggs])
        for a, (_, c, _, _) in enumerate(self._aggs):
            if c is None and self.spec.needs_input(a, self._merge):
                raise ValueError(f"aggregate {a} needs an input column")
        idx = [c for c, _, _ in self._keys] + [nl for _, nl, _ in self._keys] + \
              [c for _, c, _, _ in self._aggs] + [nl for _, _, nl, _ in self._aggs]
        if any(i is not None and i < 0 for i in idx):
            raise ValueError("chunk column indexes must be non-negative")
        self._ga = engine.group_agg_create(self.spec.key_types, self.spec.key_nullable,
                                           self.spec.agg_fns, self.spec.agg_types,
                                           self.spec.agg_nullable, capacity_hint)
        self.rows = 0

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def push_chunk(self, chunk):
        n, cols = chunk["n"], chunk["cols"]
        col = lambda i: None if i is None else cols[i]
        try:
            if n:
                self._e.group_agg_push(
                    self._ga, [(cols[c], col(nl)) for c, nl, _ in self._keys],
                    [(col(c) if self.spec.needs_input(a, self._merge) else None, col(nl))
                     for a, (_, c, nl, _) in enumerate(self._aggs)], n, self._merge)
        finally:
            for b in cols:
                b.free()
        self.rows += n

    def result(self):
        from starrocks_amd.groupagg import _DT, sort_result
        g, keys, aggs = self._e.group_agg_emit_alloc(self._ga)
        try:
            pull = lambda b, dt: np.empty(0, dt) if g == 0 else b.d2h(dt, g)
            hk = [(pull(v, _DT[t]), None if nl is None else pull(nl, np.uint8))
                  for (v, nl), t in zip(keys, self.spec.key_types)]
            ha = [(pull(v, np.int64), None if nl is None else pull(nl, np.uint8))
                  for v, nl in aggs]
        finally:
            for v, nl in keys + aggs:
                v.free()
                if nl is not None:
                    nl.free()
            self._e.group_agg_destroy(self._ga)
            self._ga = None
        hk, ha = sort_result(hk, ha)
        return g, hk, ha


class _GrowingColumns:
    """The blocking sinks' input store: one device column per chunk column,
    doubling as it fills. append() copies a chunk in and frees its buffers."""

    def __init__(self, engine, dtypes):
        self._e = engine
        self._dtypes = dtypes
        self.cols = None
        self._cap = 0
        self.rows = 0

    def reserve(self, rows):
        if self.cols is not None and rows <= self._cap:
            return
        cap = max(rows, 2 * self._cap, 1)
        grown = [self._e.alloc(cap * dt.itemsize) for dt in self._dtypes]
        if self.cols is not None:
            for src, dst, dt in zip(self.cols, grown, self._dtypes):
                if self.rows:
                    self._e.dbuf_d2d(src, dst, self.rows * dt.itemsize, 0, 0)
                src.free()
        self.cols, self._cap = grown, cap

    def append(self, chunk):
        n, cols = chunk["n"], chunk["cols"]
        try:
            if n:
                self.reserve(self.rows + n)
                for src, dst, dt in zip(cols, self.cols, self._dtypes):
                    self._e.dbuf_d2d(src, dst, n * dt.itemsize, 0, self.rows * dt.itemsize)
                self.rows += n
        finally:
            for b in cols:
                b.free()

    def release(self):
        """Hand the columns to the caller to free; the row count stays."""
        cols, self.cols = self.cols or [], None
        return cols


class WindowSinkOperator(Operator):
    """fn(...) OVER (PARTITION BY ... ORDER BY ... frame) as a blocking sink
    like TopNSinkOperator — the analytic operator's sink (exec/analytor.cpp),
    which needs every row of a partition before it can answer.

    Chunks are {"n": rows, "cols": [DBuf, ...]}; col_dtypes gives each chunk
    column's numpy dtype (1-byte null masks, 4- or 8-byte values). part_map[i]
    = (chunk column index, index of its u8 null mask or None, type 0 int32 /
    1 int64), order_map[j] = the same plus (desc, nulls_first), and funcs =
    [window.WinFunc whose col / nulls are chunk column indexes (or None)].

    Per pushed chunk: every column is appended to a device column that
    doubles as it fills, and the chunk's buffers are freed. set_finishing
    runs Engine.window once over the whole input. result() returns (the
    input columns as numpy arrays, [(values, nulls or None)] per function,
    lined up with them).

    Uses only engine.alloc / dbuf_d2d / window and DBuf.d2h / free, so it runs
    against a numpy stand-in engine without a GPU."""

    def __init__(self, engine, col_dtypes, part_map, order_map, funcs):
        super().__init__()
        from starrocks_amd.window import WindowSpec
        self._e = engine
        self._dtypes = [np.dtype(d) for d in col_dtypes]
        self._part = [(int(c), None if nl is None else int(nl), t) for c, nl, t in part_map]
        self._order = [(int(c), None if nl is None else int(nl), t, bool(d), bool(nf))
                       for c, nl, t, d, nf in order_map]
        self._funcs = list(funcs)
        self.spec = WindowSpec([t for _, _, t in self._part],
                               [nl is not None for _, nl, _ in self._part],
                               [k[2] for k in self._order],
                               [k[1] is not None for k in self._order], self._funcs)
        self._acc = _GrowingColumns(engine, self._dtypes)
        self._outs = None

    @property
    def rows(self):
        return self._acc.rows

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def push_chunk(self, chunk):
        self._acc.append(chunk)

    def set_finishing(self):
        if not self._finishing:
            self._acc.reserve(self.rows)
            col = lambda i: None if i is None else self._acc.cols[i]
            self._outs = self._e.window(
                [(col(c), col(nl), t) for c, nl, t in self._part],
                [(col(c), col(nl), t, d, nf) for c, nl, t, d, nf in self._order],
                [f.with_cols(col(f.col), col(f.nulls)) for f in self._funcs], self.rows)
        super().set_finishing()

    def result(self):
        n = self.rows
        pull = lambda b, dt: np.empty(0, dt) if n == 0 else b.d2h(dt, n)
        try:
            cols = [pull(b, dt) for b, dt in zip(self._acc.cols, self._dtypes)]
            outs = [(pull(v, np.int64), None if nl is None else pull(nl, np.uint8))
                    for v, nl in self._outs]
        finally:
            for b in self._acc.release() + [b for p in self._outs for b in p]:
                if b is not None:
                    b.free()
            self._outs = None
        return cols, outs


class SortSinkOperator(Operator):
    """ORDER BY without LIMIT as a blocking sink — the full-sort chunks sorter
    (exec/chunks_sorter_full_sort.cpp), which holds every row until the input
    ends.

    Chunks are {"n": rows, "cols": [DBuf, ...]} and col_dtypes gives each
    chunk column's numpy dtype (1-byte null masks, 4- or 8-byte values), as
    for WindowSinkOperator. key_map[i] = (chunk column index, index of its u8
    null mask or None, type 0 int32 / 1 int64 / 2 uint64, desc, nulls_first),
    most significant first.

    Per pushed chunk every column is appended to a growing device column and
    the chunk's buffers are freed. set_finishing sorts once (Engine.sort) and
    gathers every column, null masks included, through the permutation with
    gather_u8 / _u32 / _u64 by item size. result() returns the columns in
    sorted order as numpy arrays. Rows equal on every key keep arrival order:
    the sort's tie-break is the row index, which here is the arrival ordinal.

    Uses only engine.alloc / dbuf_d2d / sort / gather_* and DBuf.d2h / free, so
    it runs against a numpy stand-in engine without a GPU."""

    def __init__(self, engine, col_dtypes, key_map):
        super().__init__()
        self._e = engine
        self._dtypes = [np.dtype(d) for d in col_dtypes]
        for dt in self._dtypes:
            if dt.itemsize not in (1, 4, 8):
                raise ValueError(f"column item size {dt.itemsize} not in 1, 4, 8")
        self._keys = [(int(c), None if nl is None else int(nl), t, bool(d), bool(nf))
                      for c, nl, t, d, nf in key_map]
        self._acc = _GrowingColumns(engine, self._dtypes)
        self._sorted = None

    @property
    def rows(self):
        return self._acc.rows

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def push_chunk(self, chunk):
        self._acc.append(chunk)

    def set_finishing(self):
        if not self._finishing:
            n = self.rows
            self._acc.reserve(n)
            cols = self._acc.cols
            col = lambda i: None if i is None else cols[i]
            gather = {1: self._e.gather_u8, 4: self._e.gather_u32, 8: self._e.gather_u64}
            perm, out = None, []
            try:
                perm = self._e.sort([(col(c), col(nl), t, d, nf)
                                     for c, nl, t, d, nf in self._keys], n)
                for src, dt in zip(cols, self._dtypes):
                    out.append(self._e.alloc(max(n, 1) * dt.itemsize))
                    if n:
                        gather[dt.itemsize](src, perm, n, out[-1])
            except BaseException:
                for b in out:
                    b.free()
                raise
            finally:
                if perm is not None:
                    perm.free()
                for b in self._acc.release():
                    b.free()
            self._sorted = out
        super().set_finishing()

    def result(self):
        n = self.rows
        try:
            return [np.empty(0, dt) if n == 0 else b.d2h(dt, n)
                    for b, dt in zip(self._sorted, self._dtypes)]
        finally:
            for b in self._sorted:
                b.free()
            self._sorted = None


class GeneralHashJoinBuildOperator(Operator):
    """The build side of the general hash join (starrocks_amd/hashjoin.py) as
    a sink: HashJoinBuildOperator without the caller-written build_fn.

    Chunks are {"n": rows, "cols": [DBuf, ...]}; col_dtypes gives each chunk
    column's numpy dtype (1-byte null masks, 4- or 8-byte values). key_map[i]
    = (chunk column index, index of its u8 null mask or None, type 0 int32 /
    1 int64) binds build key i. probe_types gives the probe side's key types
    (default: the build side's), key_nullable which keys may be NULL on either
    side (default: those with a build null mask), null_safe the keys compared
    with <=>.

    Per pushed chunk: one build_push of the key columns — the table copies
    them and grows as it needs to — and every column is appended to a device
    column that doubles as it fills, the payload the probe operator gathers
    from; the chunk's buffers are freed. Build row i is row i of those
    columns. close() keeps the table and the columns for the probe pipeline;
    release() drops them.

    Uses only engine.hash_join_create / hash_join_build_push /
    hash_join_destroy / alloc / dbuf_d2d and DBuf.free."""

    def __init__(self, engine, key_map, col_dtypes, probe_types=None, key_nullable=None,
                 null_safe=None, capacity_hint=0):
        super().__init__()
        from starrocks_amd.hashjoin import HashJoinSpec
        self._e = engine
        self._keys = [(int(c), None if nl is None else int(nl), int(t)) for c, nl, t in key_map]
        self.dtypes = [np.dtype(d) for d in col_dtypes]
        for dt in self.dtypes:
            if dt.itemsize not in (1, 4, 8):
                raise ValueError(f"column item size {dt.itemsize} not in 1, 4, 8")
        if any(c < 0 or (nl is not None and nl < 0) for c, nl, _ in self._keys):
            raise ValueError("chunk column indexes must be non-negative")
        build_types = [t for _, _, t in self._keys]
        if key_nullable is None:
            key_nullable = [nl is not None for _, nl, _ in self._keys]
        self.spec = HashJoinSpec(build_types, build_types if probe_types is None else probe_types,
                                 key_nullable, null_safe)
        for k, (_, nl, _) in enumerate(self._keys):
            if nl is not None and not self.spec.key_nullable[k]:
                raise ValueError(f"null column for key {k}, declared NOT NULL")
        self.table = engine.hash_join_create(self.spec.build_types, self.spec.probe_types,
                                             self.spec.key_nullable, self.spec.key_null_safe,
                                             capacity_hint)
        self._acc = _GrowingColumns(engine, self.dtypes)

    @property
    def rows(self):
        return self._acc.rows

    @property
    def cols(self):
        return self._acc.cols

    def need_input(self):
        return not self._finishing

    def has_output(self):
        return False

    def push_chunk(self, chunk):
        n, cols = chunk["n"], chunk["cols"]
        try:
            if n:
                self._e.hash_join_build_push(
                    self.table, [(cols[c], None if nl is None else cols[nl])
                                 for c, nl, _ in self._keys], n)
        except BaseException:
            for b in cols:
                b.free()
            raise
        self._acc.append(chunk)

    def set_finishing(self):
        self._acc.reserve(self.rows)  # an empty build still has columns to gather from
        super().set_finishing()

    def release(self):
        if self.table is not None:
            self._e.hash_join_destroy(self.table)
            self.table = None
        for b in self._acc.release():
            b.free()


class GeneralHashJoinProbeOperator(Operator):
    """The probe side of the general hash join: push one probe chunk, pull the
    joined chunk; for RIGHT / FULL joins set_finishing yields one last chunk.

    how is one of hashjoin.HOWS. key_map binds the probe keys as the build
    operator's binds the build keys; col_dtypes gives the probe chunk's column
    dtypes. probe_payload / build_payload = [(chunk column index, index of its
    u8 null mask or None)] list the columns of each side that go into the
    joined chunk (the build side's indexes refer to the build chunks).

    The joined chunk holds, in this order, the probe payload and then the
    build payload, each column followed by a u8 null column iff it has a null
    mask of its own or the join type makes its side nullable
    (hashjoin.output_sides); a side the join type does not carry (the build
    side of LEFT SEMI / ANTI, the probe side of RIGHT SEMI / ANTI) is left
    out. out_dtypes gives the dtypes of the joined chunk's columns.

    Per pushed chunk: count + emit (hash_join_probe_alloc, with MARK_BUILD for
    RIGHT / FULL); the probe payload goes through gather_u32 / _u64 / _u8 by
    the pairs' probe index, the build payload through gather_outer by their
    build index, which turns NO_ROW into NULL; the probe chunk is freed. A
    RIGHT SEMI / ANTI probe chunk only marks and yields nothing. At
    set_finishing a RIGHT / FULL join emits the build rows no (or, RIGHT SEMI,
    some) probe row matched as one last chunk with an all-NULL probe side.

    Uses only engine.hash_join_probe_alloc / hash_join_emit_build / gather_* /
    gather_outer / alloc and DBuf.h2d / free."""

    def __init__(self, engine, build_op, how, key_map, col_dtypes, probe_payload,
                 build_payload):
        super().__init__()
        from starrocks_amd.hashjoin import output_sides, plan
        self._e = engine
        self._b = build_op
        self.how = how
        self._mode, self._flags, self._tail = plan(how)
        self._has_p, self._p_nullable, self._has_b, self._b_nullable = output_sides(how)
        self._keys = [(int(c), None if nl is None else int(nl), int(t)) for c, nl, t in key_map]
        if [t for _, _, t in self._keys] != build_op.spec.probe_types:
            raise ValueError("probe key types differ from the table's probe layout")
        for k, (_, nl, _) in enumerate(self._keys):
            if nl is not None and not build_op.spec.key_nullable[k]:
                raise ValueError(f"null column for key {k}, declared NOT NULL")
        self._dtypes = [np.dtype(d) for d in col_dtypes]
        pair = lambda p: [(int(c), None if nl is None else int(nl)) for c, nl in p]
        self._pp = pair(probe_payload) if self._has_p else []
        self._bp = pair(build_payload) if self._has_b else []
        self.out_dtypes = []
        for (c, nl), dts, nullable in \
                [(p, self._dtypes, self._p_nullable) for p in self._pp] + \
                [(p, build_op.dtypes, self._b_nullable) for p in self._bp]:
            if dts[c].itemsize not in (1, 4, 8):
                raise ValueError(f"column item size {dts[c].itemsize} not in 1, 4, 8")
            self.out_dtypes.append(dts[c])
            if nl is not None or nullable:
                self.out_dtypes.append(np.dtype(np.uint8))
        self._in = None
        self._out = None
        self._last = None
        self.rows = 0

    def need_input(self):
        return self._in is None and self._out is None and not self._finishing

    def has_output(self):
        if self._in is not None:
            self._probe()
        return self._out is not None or self._last is not None

    def push_chunk(self, chunk):
        self._in = chunk

    def _const_u8(self, n, value):
        b = self._e.alloc(max(n, 1))
        if n:
            b.h2d(np.full(n, value, np.uint8))
        return b

    def _gather_build(self, idx, n, out_cols):
        """The build payload through idx, NO_ROW -> NULL."""
        e, bo = self._e, self._b
        for c, nl in self._bp:
            w = bo.dtypes[c].itemsize
            want_nl = nl is not None or self._b_nullable
            out = e.alloc(max(n, 1) * w)
            out_cols.append(out)
            onl = e.alloc(max(n, 1)) if want_nl else None
            if onl is not None:
                out_cols.append(onl)
            if n:
                e.gather_outer(bo.cols[c], None if nl is None else bo.cols[nl], bo.rows, w,
                               idx, n, out, onl)

    def _probe(self):
        c, self._in = self._in, None
        e = self._e
        n_in, cols = c["n"], c["cols"]
        out_cols, op, ob = [], None, None
        try:
            keys = [(cols[k], None if nl is None else cols[nl]) for k, nl, _ in self._keys]
            op, ob, n = e.hash_join_probe_alloc(self._b.table, keys, n_in, self._mode,
                                                self._flags)
            if self._has_p:  # RIGHT SEMI / ANTI chunks only mark
                gather = {1: e.gather_u8, 4: e.gather_u32, 8: e.gather_u64}
                for k, nl in self._pp:
                    for src in (k, nl):
                        if src is None:
                            continue
                        out_cols.append(e.alloc(max(n, 1) * self._dtypes[src].itemsize))
                        if n:
                            gather[self._dtypes[src].itemsize](cols[src], op, n, out_cols[-1])
                    if nl is None and self._p_nullable:
                        out_cols.append(self._const_u8(n, 0))
                self._gather_build(ob, n, out_cols)
                self._out = {"n": n, "cols": out_cols}
                self.rows += n
        except BaseException:
            for b in out_cols:
                b.free()
            raise
        finally:
            for b in (op, ob, *cols):
                if b is not None:
                    b.free()

    def set_finishing(self):
        if not self._finishing and self._tail is not None:
            if self._in is not None:
                self._probe()
            e = self._e
            m = e.hash_join_emit_build(self._b.table, self._tail)
            tb = e.alloc(max(m, 1) * 4)
            out_cols = []
            try:
                if m:
                    assert e.hash_join_emit_build(self._b.table, self._tail, tb, m) == m
                for k, _ in self._pp:  # an all-NULL probe side
                    out_cols.append(e.alloc(max(m, 1) * self._dtypes[k].itemsize))
                    if m:
                        out_cols[-1].h2d(np.zeros(m, self._dtypes[k]))
                    out_cols.append(self._const_u8(m, 1))
                self._gather_build(tb, m, out_cols)
            except BaseException:
                for b in out_cols:
                    b.free()
                raise
            finally:
                tb.free()
            self._last = {"n": m, "cols": out_cols}
            self.rows += m
        super().set_finishing()

    def pull_chunk(self):
        if self._out is None and self._in is not None:
            self._probe()
        if self._out is not None:
            c, self._out = self._out, None
        else:
            c, self._last = self._last, None
        return c


def q1_operator_pipeline(engine, seed, total_rows, year=1993,
                         chunk_rows=DEFAULT_CHUNK_ROWS, dim_chunk_rows=1000):
    """Config-2's plan as the reference would run it — dim source -> build
    pipeline, then fact source -> probe -> agg sink over bounded chunks —
    instead of the fused q1 kernel. Bit-exact same (sum, count) as
    engine.q1_join_sum / orc.q1_pipeline; exists to exercise the push/pull
    boundary end to end, not as the bench path (the fused kernel is the fast
    form: one HBM pass, no match materialization)."""
    from starrocks_amd import gen as g

    # Dim rows pass the year predicate before the build, as the reference's
    # plan filters the dim scan below the build operator.
    datekey, dyear = g.gen_dates()
    dim_keys = datekey[dyear == year].astype(np.int32)

    def date_source(row_start, n):
        kb = engine.alloc(n * 4)
        kb.h2d(dim_keys[row_start:row_start + n])
        return {"n": n, "cols": [kb]}

    def build_dates(e, chunks):
        total = sum(c["n"] for c in chunks)
        kb = e.alloc((total + 1) * 4)  # row 0 = sentinel
        kb.h2d(np.zeros(1, np.int32))
        off = 1
        for c in chunks:
            e.dbuf_d2d(c["cols"][0], kb, c["n"] * 4, 0, off * 4)
            off += c["n"]
        t = e.join_build_range_direct(kb, total)
        kb.free()
        return t

    def gen_chunk(row_start, n):
        cols = [engine.alloc(n * 4) for _ in range(3)]
        engine.gen_lineorder_q1(seed, row_start, n, *cols)
        return {"n": n, "cols": cols}

    def agg_update(e, state, chunk):
        if state is None:
            state = e.alloc(16)
            state.h2d(np.zeros(2, np.int64))
        ep, dc = chunk["cols"]
        e.sum_prod_u32(ep, dc, chunk["n"], state)
        return state

    def agg_result(e, state):
        if state is None:
            return 0, 0
        raw = state.d2h(np.int64, 2)
        state.free()
        return int(raw[0]), int(raw[1])

    # Build pipeline first (the reference runs build and probe as two
    # pipelines with a dependency; hash_join_build_operator.cpp:87-96).
    build = HashJoinBuildOperator(engine, build_dates)
    PipelineDriver([
        ChunkSourceOperator(date_source, len(dim_keys), dim_chunk_rows),
        build,
    ]).process()

    probe_driver = PipelineDriver([
        ChunkSourceOperator(gen_chunk, total_rows, chunk_rows),
        HashJoinProbeOperator(engine, build, key_col=0),
        AggregateSinkOperator(engine, agg_update, agg_result),
    ])
    out = probe_driver.process()
    build.release()
    return out
