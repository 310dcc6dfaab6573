"""General TopN measurement (DESIGN.md §4b row "TopN").

Times gpue_topn against the unchanged k<=16 entry gpue_topk_i64 on the same
device buffers (value DESC, key DESC; k = 10, 16), then gpue_topn alone at
k = 100 / 10 000 / 1 000 000 with one, two and three sort keys. Each step is
one call bracketed by stream events (both entries end in a stream
synchronize); after warm-up the median and min of the repeated steps are
reported, with GB/s = bytes of the key columns (one pass) / median.

Data (seed 42): value = int64 in [0, 10^7) (revenue-like, ~6.7 rows per
value at 64 Mi rows), key = a unique u64 id (row index times an odd
constant), year = int32 in [1992, 1999), brand = int32 in [0, 1000).

Run: python tools/topn_bench.py --out profiles/topn_bench.json
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine


def timed(eng, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        eng.timer_start()
        fn()
        ms.append(eng.timer_stop())
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows

    eng = Engine(0)
    rng = np.random.default_rng(42)
    vals = rng.integers(0, 10_000_000, n).astype(np.int64)
    keys = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345))
    year = rng.integers(1992, 1999, n).astype(np.int32)
    brand = rng.integers(0, 1000, n).astype(np.int32)
    bufs = {}
    for name, arr in (("vals", vals), ("keys", keys), ("year", year), ("brand", brand)):
        bufs[name] = eng.alloc(arr.nbytes)
        bufs[name].h2d(arr)
    eng.sync()

    results = {"rows": n, "warmup": args.warmup, "reps": args.reps, "cases": []}

    def record(case, med, mn, key_bytes, **extra):
        row = {"case": case, "ms_median": round(med, 4), "ms_min": round(mn, 4),
               "key_gb_per_s": round(key_bytes / (med / 1e3) / 1e9, 1)}
        row.update(extra)
        results["cases"].append(row)
        print(json.dumps(row), flush=True)

    # --- head to head with the k<=16 entry: value DESC, key DESC -----------
    vk = [(bufs["vals"], None, 1, True, False), (bufs["keys"], None, 2, True, False)]
    for k in (10, 16):
        out = eng.alloc(k * 4)
        ok, ov = eng.topk_i64(bufs["keys"], bufs["vals"], n, k)
        assert eng.topn_into(vk, n, k, 0, out) == k
        idx = out.d2h(np.uint32, k)
        assert np.array_equal(vals[idx], ov) and np.array_equal(keys[idx], ok)
        old = timed(eng, lambda: eng.topk_i64(bufs["keys"], bufs["vals"], n, k),
                    args.warmup, args.reps)
        new = timed(eng, lambda: eng.topn_into(vk, n, k, 0, out), args.warmup, args.reps)
        record(f"topk_i64 k={k} (value DESC, key DESC)", *old, 16 * n, k=k, entry="gpue_topk_i64")
        record(f"topn k={k} (value DESC, key DESC)", *new, 16 * n, k=k, entry="gpue_topn",
               speedup_vs_topk_i64=round(old[0] / new[0], 3))
        out.free()

    # --- gpue_topn alone: k x number of keys ------------------------------
    keysets = {
        "1 key (value DESC)": ([(bufs["vals"], None, 1, True, False)], 8),
        "2 keys (year ASC, value DESC)": ([(bufs["year"], None, 0, False, False),
                                           (bufs["vals"], None, 1, True, False)], 12),
        "3 keys (year ASC, brand ASC, value DESC)": (
            [(bufs["year"], None, 0, False, False), (bufs["brand"], None, 0, False, False),
             (bufs["vals"], None, 1, True, False)], 16),
    }
    for k in (100, 10_000, 1_000_000):
        out = eng.alloc(k * 4)
        reps = args.reps if k <= 10_000 else max(3, args.reps // 3)
        for label, (desc, width) in keysets.items():
            med, mn = timed(eng, lambda: eng.topn_into(desc, n, k, 0, out), args.warmup, reps)
            record(f"topn k={k} {label}", med, mn, width * n, k=k, entry="gpue_topn",
                   n_keys=len(desc), reps=reps)
        out.free()

    for b in bufs.values():
        b.free()
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
