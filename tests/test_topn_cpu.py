"""General TopN, the GPU-less part: the C-ABI declares gpue_topn and Engine
binds it, and TopNSinkOperator's chunk-merge logic is exact against a numpy
stand-in engine whose topn IS the reference order.

The reference (also imported by tests/test_topn.py): per key, dense ranks of
the non-NULL values via np.unique(return_inverse) — safe for INT64_MIN and
uint64 >= 2^63 — reversed for DESC, NULL rows ranked -1 (NULLS_FIRST) or
max+1 (NULLS_LAST), then np.lexsort with the row index as the last key."""

import os
import re

import numpy as np
import pytest

from starrocks_amd.pipeline import ChunkSourceOperator, PipelineDriver, TopNSinkOperator

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TYPE_CODE = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.uint64): 2}


def topn_order(keys, n):
    """Full reference order. keys: [(values, nulls_or_None, desc, nulls_first)],
    most significant first. Returns row indices (int64) of all n rows."""
    ranks = []
    for vals, nulls, desc, nulls_first in keys:
        vals = np.asarray(vals)[:n]
        isnull = np.zeros(n, bool) if nulls is None else np.asarray(nulls)[:n].astype(bool)
        r = np.zeros(n, np.int64)
        nn = ~isnull
        top = 0
        if nn.any():
            uniq, inv = np.unique(vals[nn], return_inverse=True)
            inv = inv.astype(np.int64).reshape(-1)
            top = len(uniq) - 1
            r[nn] = (top - inv) if desc else inv
        r[isnull] = -1 if nulls_first else top + 1
        ranks.append(r)
    return np.lexsort(tuple([np.arange(n, dtype=np.int64)] + ranks[::-1]))


def topn_reference(keys, n, limit, offset=0):
    return topn_order(keys, n)[offset:offset + limit]


# ---- numpy stand-in engine: just what TopNSinkOperator may call ------------
class NpBuf:
    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.mem = np.zeros(nbytes, np.uint8)
        self.freed = False

    def view(self, dtype, count, off=0):
        dt = np.dtype(dtype)
        return self.mem[off:off + count * dt.itemsize].view(dt)

    def h2d(self, arr, dst_off=0):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.mem[dst_off:dst_off + raw.size] = raw
        return self

    def d2h(self, dtype, count, src_off=0):
        return self.view(dtype, count, src_off).copy()

    def free(self):
        self.freed = True


class NpEngine:
    DT = {0: np.int32, 1: np.int64, 2: np.uint64}

    def __init__(self):
        self.topn_calls = []

    def alloc(self, nbytes):
        return NpBuf(nbytes)

    def topn(self, keys, n_rows, limit, offset=0):
        ref_keys = [(col.view(self.DT[t], n_rows),
                     None if nulls is None else nulls.view(np.uint8, n_rows), desc, nf)
                    for col, nulls, t, desc, nf in keys]
        idx = topn_reference(ref_keys, n_rows, limit, offset).astype(np.uint32)
        self.topn_calls.append(n_rows)
        out = NpBuf(max(len(idx), 1) * 4)
        out.h2d(idx)
        return out, len(idx)

    def _gather(self, inp, idx, n, out, dt):
        i = idx.view(np.uint32, n)
        out.view(dt, n)[:] = inp.view(dt, inp.nbytes // np.dtype(dt).itemsize)[i]

    def gather_u32(self, inp, idx, n, out):
        self._gather(inp, idx, n, out, np.uint32)

    def gather_u64(self, inp, idx, n, out):
        self._gather(inp, idx, n, out, np.uint64)

    def dbuf_d2d(self, src, dst, nbytes, src_off=0, dst_off=0):
        assert dst_off + nbytes <= dst.nbytes and src_off + nbytes <= src.nbytes
        dst.mem[dst_off:dst_off + nbytes] = src.mem[src_off:src_off + nbytes]


# ---- the operator case shared with the GPU test ----------------------------
OP_ROWS = 500_000
OP_LIMIT, OP_OFFSET = 900, 100          # K = 1000
# uneven chunks: one smaller than K (7 rows), one empty; boundaries fall
# inside long runs of rows equal on both keys
OP_CHUNKS = [130_000, 7, 50_003, 0, 200_000, 119_990]
OP_DTYPES = [np.int32, np.int64, np.uint32]       # key a, key b, payload row id
OP_SORT_KEYS = [(0, 0, False), (1, 1, True)]      # a ASC, b DESC


def operator_case():
    assert sum(OP_CHUNKS) == OP_ROWS
    rng = np.random.default_rng(2024)
    a = rng.integers(-25, 25, OP_ROWS).astype(np.int32)
    b = rng.integers(0, 20, OP_ROWS).astype(np.int64)
    rid = np.arange(OP_ROWS, dtype=np.uint32)
    ref = topn_reference([(a, None, False, False), (b, None, True, False)], OP_ROWS,
                         OP_LIMIT, OP_OFFSET)
    return a, b, rid, ref


def run_operator(engine, a, b, rid, bound_factor):
    """Drive the case through PipelineDriver([ChunkSourceOperator,
    TopNSinkOperator]). The source's row space is the chunk ordinal, so each
    pull yields one of the uneven chunks."""
    starts = np.concatenate([[0], np.cumsum(OP_CHUNKS)])

    def gen(ordinal, _one):
        lo, n = int(starts[ordinal]), OP_CHUNKS[ordinal]
        cols = []
        for arr in (a, b, rid):
            buf = engine.alloc(max(n, 1) * arr.itemsize)
            if n:
                buf.h2d(arr[lo:lo + n])
            cols.append(buf)
        return {"n": n, "cols": cols}

    sink = TopNSinkOperator(engine, OP_SORT_KEYS, OP_DTYPES, OP_LIMIT, OP_OFFSET,
                            bound_factor=bound_factor)
    out = PipelineDriver([ChunkSourceOperator(gen, len(OP_CHUNKS), 1), sink]).process()
    return sink, out


@pytest.fixture(scope="module")
def op_case():
    return operator_case()


def test_header_declares_and_engine_binds_topn():
    src = open(os.path.join(REPO_ROOT, "include", "gpue.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+gpue_topn\s*\(", code), "gpue.h does not declare gpue_topn"
    assert "chunks_sorter_topn.cpp" in src and "SortDesc" in src
    from starrocks_amd import engine as eng_mod
    for name in ("topn", "topn_into", "topn_indices"):
        assert callable(getattr(eng_mod.Engine, name, None)), name
    lib = os.path.join(REPO_ROOT, "starrocks_amd", "libgpue.so")
    if os.path.exists(lib):  # _declare() resolves every bound symbol, gpue_topn included
        import ctypes
        cdll = ctypes.CDLL(lib)
        eng_mod._declare(cdll)
        assert cdll.gpue_topn.restype is ctypes.c_int32
        assert len(cdll.gpue_topn.argtypes) == 11


def test_reference_order_handles_extremes_and_nulls():
    """The reference itself on a hand-checked case (INT64_MIN, u64 >= 2^63,
    NULL placement independent of direction, stable ties)."""
    v = np.array([0, np.iinfo(np.int64).min, 5, 5, np.iinfo(np.int64).max], np.int64)
    nl = np.array([0, 0, 0, 0, 1], np.uint8)
    assert list(topn_order([(v, nl, False, True)], 5)) == [4, 1, 0, 2, 3]
    assert list(topn_order([(v, nl, True, True)], 5)) == [4, 2, 3, 0, 1]
    assert list(topn_order([(v, nl, True, False)], 5)) == [2, 3, 0, 1, 4]
    u = np.array([2**63, 1, 2**64 - 1, 2**63 - 1], np.uint64)
    assert list(topn_order([(u, None, False, False)], 4)) == [1, 3, 0, 2]


@pytest.mark.parametrize("bound_factor", [2, 4])
def test_operator_merge_against_numpy_engine(op_case, bound_factor):
    a, b, rid, ref = op_case
    eng = NpEngine()
    sink, out = run_operator(eng, a, b, rid, bound_factor)
    assert np.array_equal(out[2].astype(np.int64), ref)
    assert np.array_equal(out[0], a[ref]) and np.array_equal(out[1], b[ref])
    k = OP_LIMIT + OP_OFFSET
    assert sink.capacity == bound_factor * k
    assert 0 < sink.max_candidate_rows <= sink.capacity
    # every re-sort ran over the bounded candidate set or one chunk, never more
    assert max(eng.topn_calls) <= max(max(OP_CHUNKS), sink.capacity)
    if bound_factor == 2:  # 7 + 4 x 1000 survivors cannot fit 2000 without a cut
        assert sum(1 for c in eng.topn_calls if c not in OP_CHUNKS) >= 2


def test_operator_edge_shapes():
    """No input, limit 0, and offset past the end."""
    eng = NpEngine()
    for limit, offset, rows in [(5, 0, 0), (0, 0, 50), (5, 100, 50)]:
        vals = np.arange(rows, dtype=np.int64)[::-1].copy()

        def gen(start, n, vals=vals):
            buf = eng.alloc(max(n, 1) * 8)
            if n:
                buf.h2d(vals[start:start + n])
            return {"n": n, "cols": [buf]}

        sink = TopNSinkOperator(eng, [(0, 1, False)], [np.int64], limit, offset)
        src = ChunkSourceOperator(gen, rows, 16)
        out = PipelineDriver([src, sink]).process()
        assert len(out) == 1 and len(out[0]) == 0
    # and a tiny real one: 50 rows descending -> ascending top 5 after offset 2
    vals = np.arange(50, dtype=np.int64)[::-1].copy()

    def gen2(start, n):
        buf = eng.alloc(n * 8)
        buf.h2d(vals[start:start + n])
        return {"n": n, "cols": [buf]}

    sink = TopNSinkOperator(eng, [(0, 1, False)], [np.int64], 5, 2, bound_factor=2)
    out = PipelineDriver([ChunkSourceOperator(gen2, 50, 16), sink]).process()
    assert list(out[0]) == [2, 3, 4, 5, 6]
