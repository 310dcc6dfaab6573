"""Full sort, the GPU-less part: the C-ABI declares gpue_sort / gpue_gather_u8
and Engine binds them, the tile constants the GPU tests aim at equal the ones
in the kernel source, and SortSinkOperator is exact against a numpy stand-in
engine whose sort IS the reference order (test_topn_cpu.topn_order: dense
ranks + lexsort with the row index last)."""

import os
import re

import numpy as np
import pytest

from starrocks_amd.pipeline import ChunkSourceOperator, PipelineDriver, SortSinkOperator
from test_topn_cpu import NpBuf, NpEngine, topn_order

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class NpSortEngine(NpEngine):
    """NpEngine plus the two calls only SortSinkOperator needs; remembers every
    buffer it handed out so the test can see them all freed."""

    def __init__(self):
        super().__init__()
        self.bufs = []
        self.sort_calls = []

    def alloc(self, nbytes):
        self.bufs.append(NpBuf(nbytes))
        return self.bufs[-1]

    def sort(self, keys, n_rows):
        ref_keys = [(col.view(self.DT[t], n_rows),
                     None if nulls is None else nulls.view(np.uint8, n_rows), desc, nf)
                    for col, nulls, t, desc, nf in keys]
        self.sort_calls.append(n_rows)
        out = self.alloc(max(n_rows, 1) * 4)
        out.h2d(topn_order(ref_keys, n_rows).astype(np.uint32))
        return out

    def gather_u8(self, inp, idx, n, out):
        self._gather(inp, idx, n, out, np.uint8)


# ---- the operator case shared with the GPU test ----------------------------
# columns: key a (int32, nullable through column 1), its null mask, key b
# (int64), payload (uint32 row id), nullable payload (int64) and its mask
SINK_DTYPES = [np.int32, np.uint8, np.int64, np.uint32, np.int64, np.uint8]
SINK_KEYS = [(0, 1, 0, True, True), (2, None, 1, False, False)]  # a DESC NULLS FIRST, b ASC
SINK_CHUNKS = [30_000, 7, 0, 4_099, 25_001, 893]  # boundaries inside long tie runs


def sink_case(chunks=SINK_CHUNKS, seed=2025):
    n = sum(chunks)
    rng = np.random.default_rng(seed)
    a = rng.integers(-6, 6, n).astype(np.int32)
    an = (rng.random(n) < 0.15).astype(np.uint8)
    b = rng.integers(0, 9, n).astype(np.int64)
    rid = np.arange(n, dtype=np.uint32)
    pay = rng.integers(-2**62, 2**62, n).astype(np.int64)
    pn = (rng.random(n) < 0.3).astype(np.uint8)
    cols = [a, an, b, rid, pay, pn]
    ref = topn_order([(a, an, True, True), (b, None, False, False)], n)
    return cols, ref


def run_sink(engine, cols, chunks):
    starts = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64)

    def gen(ordinal, _one):
        lo, n = int(starts[ordinal]), chunks[ordinal]
        out = []
        for arr in cols:
            buf = engine.alloc(max(n, 1) * arr.itemsize)
            if n:
                buf.h2d(arr[lo:lo + n])
            out.append(buf)
        return {"n": n, "cols": out}

    sink = SortSinkOperator(engine, SINK_DTYPES, SINK_KEYS)
    out = PipelineDriver([ChunkSourceOperator(gen, len(chunks), 1), sink]).process()
    return sink, out


def test_header_declares_and_engine_binds_sort():
    src = open(os.path.join(REPO_ROOT, "include", "gpue.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+gpue_sort\s*\(", code), "gpue.h does not declare gpue_sort"
    assert re.search(r"\bint\s+gpue_gather_u8\s*\(", code), "gpue.h does not declare gpue_gather_u8"
    assert "chunks_sorter_full_sort.cpp" in src
    from starrocks_amd import engine as eng_mod
    for name in ("sort", "sort_into", "sort_indices", "gather_u8"):
        assert callable(getattr(eng_mod.Engine, name, None)), name
    lib = os.path.join(REPO_ROOT, "starrocks_amd", "libgpue.so")
    if os.path.exists(lib):  # _declare() resolves every bound symbol
        import ctypes
        cdll = ctypes.CDLL(lib)
        eng_mod._declare(cdll)
        assert cdll.gpue_sort.restype is ctypes.c_int32
        assert len(cdll.gpue_sort.argtypes) == 8
        assert len(cdll.gpue_gather_u8.argtypes) == 5


def test_tile_constants_match_the_source():
    from starrocks_amd.engine import Engine
    hip = open(os.path.join(REPO_ROOT, "starrocks_amd", "csrc", "gpue.hip")).read()
    hdr = open(os.path.join(REPO_ROOT, "include", "gpue.h")).read()
    const = lambda name: int(re.search(
        rf"static constexpr \w+ {name} = (\d+);", hip).group(1))
    assert const("SORT_TILE") == Engine.SORT_TILE
    assert const("SORT_MAX_BLOCKS") == Engine.SORT_MAX_BLOCKS
    assert const("SORT_ITEMS") * 256 == Engine.SORT_TILE
    small = int(re.search(r"#define GPUE_SORT_SMALL_MAX (\d+)", hdr).group(1))
    assert small == Engine.SORT_SMALL_MAX <= const("TOPN_SORT_TILE")


def test_sink_chunked_equals_one_reference_sort():
    cols, ref = sink_case()
    eng = NpSortEngine()
    sink, out = run_sink(eng, cols, SINK_CHUNKS)
    assert sink.rows == len(ref) and eng.sort_calls == [len(ref)]   # sorted once
    assert np.array_equal(out[3].astype(np.int64), ref)             # arrival order breaks ties
    for got, col in zip(out, cols):                                 # nullable payload carried
        assert got.dtype == col.dtype and np.array_equal(got, col[ref])
    assert all(b.freed for b in eng.bufs)


@pytest.mark.parametrize("chunks", [[], [0], [0, 0], [1], [777]])
def test_sink_zero_rows_and_one_chunk(chunks):
    cols, ref = sink_case(chunks, seed=len(chunks))
    eng = NpSortEngine()
    sink, out = run_sink(eng, cols, chunks)
    assert sink.is_finished() and sink.rows == sum(chunks)
    assert len(out) == len(cols)
    for got, col in zip(out, cols):
        assert got.dtype == col.dtype and np.array_equal(got, col[ref])
    assert all(b.freed for b in eng.bufs)


def test_sink_rejects_an_item_size_it_cannot_gather():
    with pytest.raises(ValueError):
        SortSinkOperator(NpSortEngine(), [np.int16], [(0, None, 0, False, False)])
