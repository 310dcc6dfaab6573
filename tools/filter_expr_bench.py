"""Predicate-expression filter measurement (DESIGN.md §4b row "filter_expr").

Two head-to-head comparisons against entries this path leaves unchanged, on
the same device buffers; no ratio is a gate:

  A. 100 M int64 rows, `v < theta` at selectivity 0.01 / 0.1 / 0.5:
     gpue_pred_eval_mask + gpue_mask_compact (the general path: a 1-leaf
     program, bitmap, two-phase compaction) against the specialised
     single-pass lookback kernel gpue_scan_filter_i64_lt_sp.
  B. 100 M rows of three int32 columns under SSB Q1.1's WHERE
     (d_year = 1993 AND lo_discount BETWEEN 1 AND 3 AND lo_quantity < 25),
     all three columns compacted: mask + compact against the per-conjunct
     eager-prune gpue_eval_conjuncts_i32. That entry compacts in place, so
     its columns are restored from pristine copies before every timed call
     (outside the timed region).

Each step is one whole call (or mask + compact pair) bracketed by stream
events; every entry ends in a stream synchronize. After warm-up the median
and min of the repeated steps are reported.

Run: python tools/filter_expr_bench.py --out profiles/filter_expr_bench.json
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine
from starrocks_amd.predicate import PT_I32, PT_I64, compile_predicate


def timed(eng, fn, warmup, reps, before=None):
    ms = []
    for i in range(warmup + reps):
        if before:
            before()
        eng.timer_start()
        fn()
        t = eng.timer_stop()
        if i >= warmup:
            ms.append(t)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
    eng = Engine(0)
    results = {"rows": n, "warmup": args.warmup, "reps": args.reps, "cases": []}

    def record(**row):
        results["cases"].append(row)
        print(json.dumps(row), flush=True)

    mask = eng.alloc((n + 63) // 64 * 8)

    # ---- A: single int64 column, v < theta --------------------------------
    inp = eng.alloc(n * 8)
    eng.gen_i64(inp, 42, 3, 0, n)
    out = eng.alloc(n * 8)
    eng.sync()
    pc = [(inp, None, PT_I64)]
    for sel in (0.01, 0.1, 0.5):
        theta = int(-(2**63) + sel * 2**64)   # uniform domain: theta at the selectivity
        prog = compile_predicate(("cmp", "<", 0, theta), [PT_I64])
        ref_cnt = eng.scan_filter_i64_lt_sp(inp, n, theta, out)
        ref_head = out.d2h(np.int64, min(ref_cnt, 4096))

        def expr():
            c = eng.pred_eval_mask(pc, prog, n, mask)
            assert eng.mask_compact(mask, n, [(inp, out, 8)]) == c

        expr()
        assert eng.mask_compact(mask, n, []) == ref_cnt
        assert np.array_equal(out.d2h(np.int64, min(ref_cnt, 4096)), ref_head)
        sp = timed(eng, lambda: eng.scan_filter_i64_lt_sp(inp, n, theta, out),
                   args.warmup, args.reps)
        ex = timed(eng, expr, args.warmup, args.reps)
        mk = timed(eng, lambda: eng.pred_eval_mask(pc, prog, n, mask), args.warmup, args.reps)
        algo = (8 + 8 * sel) * n
        co = timed(eng, lambda: eng.mask_compact(mask, n, [(inp, out, 8)]), args.warmup, args.reps)
        cn = timed(eng, lambda: eng.mask_compact(mask, n, []), args.warmup, args.reps)
        record(case="A: int64 v < theta", selectivity=sel, matched=ref_cnt,
               scan_filter_sp_ms=round(sp[0], 4), scan_filter_sp_ms_min=round(sp[1], 4),
               mask_plus_compact_ms=round(ex[0], 4), mask_plus_compact_ms_min=round(ex[1], 4),
               mask_only_ms=round(mk[0], 4), compact_only_ms=round(co[0], 4),
               count_only_ms=round(cn[0], 4),
               mask_only_gb_per_s=round(8 * n / (mk[0] / 1e3) / 1e9, 1),
               mask_plus_compact_algorithmic_gb_per_s=round(algo / (ex[0] / 1e3) / 1e9, 1),
               expr_over_sp=round(ex[0] / sp[0], 3))
    inp.free()
    out.free()

    # ---- B: SSB Q1.1's three conjuncts over int32 columns -------------------
    specs = [(11, 7, 1992), (12, 11, 0), (13, 50, 1)]   # d_year, lo_discount, lo_quantity
    pristine, work, dst = [], [], []
    for tag, mod, add in specs:
        b = eng.alloc(n * 4)
        eng.gen_u32_mod(b, 42, tag, 0, n, mod, add)
        pristine.append(b)
        work.append(eng.alloc(n * 4))
        dst.append(eng.alloc(n * 4))
    eng.sync()

    def restore():
        for p, w in zip(pristine, work):
            eng.dbuf_d2d(p, w, n * 4, 0, 0)
        eng.sync()

    preds = [(0, 0, 1993, 0), (1, 2, 1, 3), (2, 1, 0, 25)]
    tree = ("and", ("cmp", "=", 0, 1993), ("between", 1, 1, 3), ("cmp", "<", 2, 25))
    prog = compile_predicate(tree, [PT_I32] * 3)
    pc = [(b, None, PT_I32) for b in pristine]

    def expr3():
        c = eng.pred_eval_mask(pc, prog, n, mask)
        assert eng.mask_compact(mask, n, [(s, d, 4) for s, d in zip(pristine, dst)]) == c
        return c

    restore()
    m = eng.eval_conjuncts(work, n, preds)
    assert expr3() == m
    k = min(m, 4096)
    for w, d in zip(work, dst):
        assert np.array_equal(w.d2h(np.int32, k), d.d2h(np.int32, k))
    old = timed(eng, lambda: eng.eval_conjuncts(work, n, preds), args.warmup, args.reps,
                before=restore)
    new = timed(eng, expr3, args.warmup, args.reps)
    mk = timed(eng, lambda: eng.pred_eval_mask(pc, prog, n, mask), args.warmup, args.reps)
    record(case="B: Q1.1 three conjuncts, int32 x3", matched=m,
           selectivity=round(m / n, 5),
           eval_conjuncts_ms=round(old[0], 4), eval_conjuncts_ms_min=round(old[1], 4),
           mask_plus_compact_ms=round(new[0], 4), mask_plus_compact_ms_min=round(new[1], 4),
           mask_only_ms=round(mk[0], 4),
           mask_only_gb_per_s=round(12 * n / (mk[0] / 1e3) / 1e9, 1),
           speedup_vs_eval_conjuncts=round(old[0] / new[0], 3))

    for b in (mask, *pristine, *work, *dst):
        b.free()
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
