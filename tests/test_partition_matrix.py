"""Exchange partition matrix: every key shape x sync/async form x the row
counts at which the tiled histogram/emit kernels change shape x channel
counts, through the Engine API, against the oracle's channel of each row and
its counting sort.

Pinned per case: the sync form's start points equal the reference exactly,
and each channel's slice of row_indexes holds exactly the reference's row set
(order inside a slice is atomic-cursor emission order, so slices are compared
sorted; the reference's stable slices are ascending). Equal slices for every
channel also mean no repeats and lengths summing to n. The async forms return
no start points; their slices are cut at the reference's.

Row counts, for the default grid cap of 2048 blocks of 256 threads: 0 (one
block, tile 0), 1, 255 (under one block), 257 (two blocks, the second nearly
empty), 70 001 (tile 256, last block short) and 600 001 (grid at its cap, tile
293 > 256, so the strided row loop runs twice for some threads). At 70 001 an
all-equal key column puts every row on one channel and every LDS atomic on
one cursor.

Every case pins behaviour that predates the policy-templated kernels and the
two shared drivers: the file passes unchanged on the commit before them.
"""

import os

import numpy as np
import pytest

from oracle import pyoracle as orc
from starrocks_amd import gen
from starrocks_amd.engine import GpueError

if os.environ.get("GPUE_GRID"):
    pytest.skip("row counts are chosen for the default grid cap", allow_module_level=True)

pytestmark = pytest.mark.gpu

BLOCK, MAX_GRID = 256, 2048
N_ROWS = (0, 1, 255, 257, 70_001, 600_001)
N_CH = (1, 3, 64)
# (key shape, async form exists)
FORMS = [("fnv", False), ("fnv", True), ("xxh3", False), ("crc", False),
         ("u64", False), ("u64", True), ("2xi32", False), ("varchar", False)]
CASES = [(shape, is_async, n, "uniform") for shape, is_async in FORMS for n in N_ROWS] + \
        [(shape, is_async, 70_001, "equal") for shape, is_async in FORMS]

_host = {}  # (shape, n, dist) -> host key columns
_ref = {}   # (shape, n, dist, nch) -> (start points, row indexes) of the reference


def _blocks(n):
    return max(1, min((n + BLOCK - 1) // BLOCK, MAX_GRID))


def _host_cols(shape, n, dist):
    """The key columns of one case, as the host arrays that go to the device."""
    key = (shape, n, dist)
    if key not in _host:
        rng = np.random.default_rng(1000 + n)
        equal = dist == "equal"
        if shape == "u64":
            k = rng.integers(0, 2**64, n, dtype=np.uint64)
            cols = [np.full(n, 0x0123456789ABCDEF, np.uint64) if equal else k]
        elif shape == "2xi32":
            a = rng.integers(-2**31, 2**31, n).astype(np.int32)
            b = rng.integers(-2**31, 2**31, n).astype(np.int32)
            cols = [np.full(n, -7, np.int32), np.full(n, 11, np.int32)] if equal else [a, b]
        elif shape == "varchar":  # rows of 0..12 bytes, empty strings included
            lens = np.full(n, 5) if equal else rng.integers(0, 13, n)
            offsets = np.zeros(n + 1, np.uint32)
            np.cumsum(lens, out=offsets[1:])
            data = (np.tile(np.frombuffer(b"equal", np.uint8), n) if equal
                    else rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8))
            cols = [data, offsets]
        else:
            k = rng.integers(0, 2**32, n, dtype=np.uint32)
            cols = [np.full(n, 0xDEADBEEF, np.uint32) if equal else k]
        _host[key] = cols
    return _host[key]


def _reference(shape, n, dist, nch):
    key = (shape, n, dist, nch)
    if key not in _ref:
        cols = _host_cols(shape, n, dist)
        ch = {"fnv": orc.partition_channels, "xxh3": orc.partition_channels_xxh3,
              "crc": orc.partition_channels_crc, "u64": orc.partition_channels_u64,
              "2xi32": gen.partition_channels_2xi32,
              "varchar": orc.partition_channels_fnv_slice}[shape](*cols, nch)
        _ref[key] = orc.partition_counting_sort(np.ascontiguousarray(ch, np.uint32), nch)
    return _ref[key]


def _put(engine, arr):
    b = engine.alloc(max(arr.nbytes, arr.itemsize))  # max(n, 1) elements
    if arr.nbytes:
        b.h2d(arr)
    return b


def _call(engine, shape, is_async, d_cols, n, nch, d_rows, scratch=None):
    """One partition call; the sync forms return their start points."""
    if is_async:
        fn = engine.partition_async if shape == "fnv" else engine.partition_i64_async
        fn(d_cols[0], n, nch, d_rows, scratch)
        engine.sync()
        return None
    fn = {"fnv": engine.partition, "xxh3": engine.partition_xxh3, "crc": engine.partition_crc,
          "u64": engine.partition_i64, "2xi32": engine.partition_2xi32,
          "varchar": engine.partition_varchar}[shape]
    return fn(*d_cols, n, nch, d_rows)


@pytest.mark.parametrize("nch", N_CH)
@pytest.mark.parametrize("shape,is_async,n,dist", CASES)
def test_partition_matrix(engine, shape, is_async, n, dist, nch):
    ref_sp, ref_rows = _reference(shape, n, dist, nch)
    d_cols = [_put(engine, c) for c in _host_cols(shape, n, dist)]
    d_rows = engine.alloc(max(n, 1) * 4)
    scratch = engine.alloc(_blocks(n) * nch * 12) if is_async else None
    bufs = d_cols + [d_rows] + ([scratch] if is_async else [])
    try:
        sp = _call(engine, shape, is_async, d_cols, n, nch, d_rows, scratch)
        if not is_async:
            assert np.array_equal(sp, ref_sp), "start points"
        got = d_rows.d2h(np.uint32, n) if n else np.empty(0, np.uint32)
        assert int(ref_sp[nch]) == n
        for c in range(nch):
            lo, hi = int(ref_sp[c]), int(ref_sp[c + 1])
            assert np.array_equal(np.sort(got[lo:hi]), ref_rows[lo:hi]), f"channel {c} row set"
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("nch", (0, 65))
@pytest.mark.parametrize("shape,is_async", FORMS)
def test_partition_rejects_channel_count(engine, shape, is_async, nch):
    n = 257
    bufs = [_put(engine, c) for c in _host_cols(shape, n, "uniform")]
    d_rows, scratch = engine.alloc(n * 4), engine.alloc(_blocks(n) * 65 * 12)
    try:
        with pytest.raises(GpueError, match=r"^gpue status 2: bad argument"):
            _call(engine, shape, is_async, bufs, n, nch, d_rows, scratch)
    finally:
        for b in bufs + [d_rows, scratch]:
            b.free()


@pytest.mark.parametrize("shape", ("fnv", "u64"))
def test_partition_async_rejects_short_scratch(engine, shape):
    """Scratch one byte short of blocks * channels * 12 (u32 histogram + u64
    offsets per block and channel) is refused."""
    n, nch = 70_001, 3
    bufs = [_put(engine, c) for c in _host_cols(shape, n, "uniform")]
    d_rows, scratch = engine.alloc(n * 4), engine.alloc(_blocks(n) * nch * 12 - 1)
    try:
        with pytest.raises(GpueError, match=r"^gpue status 2: bad argument"):
            _call(engine, shape, True, bufs, n, nch, d_rows, scratch)
    finally:
        for b in bufs + [d_rows, scratch]:
            b.free()
