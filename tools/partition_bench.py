"""Exchange-partition timing (DESIGN.md §4b evidence).

20 M rows of uniform random keys into 8 channels, for each of the six sync
entries (FNV / xxh3 / crc u32 keys, FNV u64 keys, two chained i32 columns,
varchar slices of 8 bytes) and the two async entries (FNV u32, FNV u64).
Times best-of-5 host-clocked whole calls through the Engine API only, so it
runs unchanged on any commit that has these entry points: a sync call
includes its scratch allocations, the histogram readback and the host scan;
an async call is timed through a stream synchronize after it. Prints one JSON
line per case.

Run: python tools/partition_bench.py [rows] > partition_bench.jsonl
"""

import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine

N_CH = 8
REPS = 5


def best_of(fn):
    best = None
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def put(eng, arr):
    b = eng.alloc(arr.nbytes)
    b.h2d(arr)
    return b


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
    eng = Engine()
    rng = np.random.default_rng(42)
    k32 = put(eng, rng.integers(0, 2**32, n, dtype=np.uint32))
    b32 = put(eng, rng.integers(0, 2**32, n, dtype=np.uint32))
    k64 = put(eng, rng.integers(0, 2**64, n, dtype=np.uint64))
    vc_bytes = put(eng, rng.integers(0, 256, n * 8, dtype=np.uint8))
    vc_offsets = put(eng, np.arange(n + 1, dtype=np.uint32) * 8)
    rows = eng.alloc(n * 4)
    scratch = eng.alloc(eng.partition_scratch_bytes(n, N_CH))

    def sync_case(fn, *cols):
        return lambda: fn(*cols, n, N_CH, rows)

    def async_case(fn, keys):
        def run():
            fn(keys, n, N_CH, rows, scratch)
            eng.sync()
        return run

    cases = [
        ("fnv_u32", sync_case(eng.partition, k32)),
        ("xxh3_u32", sync_case(eng.partition_xxh3, k32)),
        ("crc_u32", sync_case(eng.partition_crc, k32)),
        ("fnv_u64", sync_case(eng.partition_i64, k64)),
        ("fnv_2xi32", sync_case(eng.partition_2xi32, k32, b32)),
        ("fnv_varchar8", sync_case(eng.partition_varchar, vc_bytes, vc_offsets)),
        ("fnv_u32_async", async_case(eng.partition_async, k32)),
        ("fnv_u64_async", async_case(eng.partition_i64_async, k64)),
    ]
    for name, call in cases:
        sp = call()  # warm
        if sp is not None:
            assert int(sp[N_CH]) == n
        print(json.dumps({"case": name, "rows": n, "channels": N_CH,
                          "call_s": round(best_of(call), 6)}), flush=True)
    for b in (k32, b32, k64, vc_bytes, vc_offsets, rows, scratch):
        b.free()
    eng.close()


if __name__ == "__main__":
    main()
