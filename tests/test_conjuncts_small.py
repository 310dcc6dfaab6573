"""Eager-prune conjunct evaluation at small and awkward row counts, i32 and
i64 columns, against the oracle: same survivor count, and every column equal
to the reference's first `count` values in order.

The four predicate lists are those of test_eval_conjuncts_parity (the i64
columns and literals are the i32 ones times 1000, so they need 64 bits):
prune-triggering, dense with no prune, all-false, all-true. Row counts: 0, 1,
257; 5 000, where the prune threshold max(n*8/10, 1024) still sits near its
1024 floor and the compaction runs 20 blocks of tile 250; 600 001, where the
compaction grid is at its cap.

The parity cases pass unchanged on the commit before the templated
implementation. The leak tests cover the bad-column-index return, which that
commit left with the filter array allocated.
"""

import ctypes

import numpy as np
import pytest

from oracle import pyoracle as orc
from starrocks_amd.engine import GpueError

pytestmark = pytest.mark.gpu

N_ROWS = (0, 1, 257, 5_000, 600_001)
PREDS = {
    "prune": [(0, 2, 19930101, 19931231), (1, 2, 1, 3), (2, 1, 0, 25)],
    "dense": [(2, 1, 0, 45), (1, 2, 0, 9)],
    "all_false": [(1, 0, 99, 0)],
    "all_true": [(2, 1, 0, 100)],
}
I64_SCALE = 1000

_cols = {}


def _columns(n):
    if n not in _cols:
        rng = np.random.default_rng(89 + n)
        _cols[n] = [rng.integers(19920101, 19990101, n).astype(np.int32),
                    rng.integers(0, 11, n).astype(np.int32),
                    rng.integers(1, 51, n).astype(np.int32)]
    return _cols[n]


@pytest.mark.parametrize("name", list(PREDS))
@pytest.mark.parametrize("n", N_ROWS)
@pytest.mark.parametrize("dtype", (np.int32, np.int64))
def test_conjuncts_small(engine, dtype, n, name):
    wide = dtype is np.int64
    scale = I64_SCALE if wide else 1
    cols = [c.astype(dtype) * scale for c in _columns(n)]
    preds = [(c, op, lo * scale, hi * scale) for c, op, lo, hi in PREDS[name]]
    want = [c.copy() for c in cols]
    count = (orc.eval_conjuncts_i64 if wide else orc.eval_conjuncts)(want, preds)
    dcols = []
    try:
        for c in cols:
            b = engine.alloc(max(c.nbytes, c.itemsize))
            if c.nbytes:
                b.h2d(c)
            dcols.append(b)
        got = (engine.eval_conjuncts_i64 if wide else engine.eval_conjuncts)(dcols, n, preds)
        assert got == count
        if count:
            for b, w in zip(dcols, want):
                assert np.array_equal(b.d2h(dtype, count), w[:count])
    finally:
        for b in dcols:
            b.free()


@pytest.mark.parametrize("dtype", (np.int32, np.int64))
def test_bad_column_index_frees_filter(engine, dtype):
    """A predicate naming a column that does not exist returns GPUE_ERR_ARG
    from inside the predicate loop, after the n_rows-byte filter array is
    allocated. 4 M rows make one leaked filter 4 MB, so 1000 leaked calls
    would be 4 GB; fewer than one filter array may be lost (one-sided: the
    device is shared)."""
    def free_bytes():  # hipMemGetInfo of the HIP runtime the engine library links
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert engine._lib.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    n = 4_000_000
    call = engine.eval_conjuncts_i64 if dtype is np.int64 else engine.eval_conjuncts
    dcols = [engine.alloc(n * np.dtype(dtype).itemsize) for _ in range(3)]
    try:
        def bad_call():
            with pytest.raises(GpueError, match=r"^gpue status 2: bad argument"):
                call(dcols, n, [(3, 1, 0, 25), (0, 1, 0, 25)])

        bad_call()  # warm
        free_before = free_bytes()
        for _ in range(1000):
            bad_call()
        lost = free_before - free_bytes()
        print(f"device bytes lost over 1000 bad-argument calls: {lost}")
        assert lost < n, f"{lost} bytes of device memory lost over 1000 bad-argument calls"
    finally:
        for b in dcols:
            b.free()
