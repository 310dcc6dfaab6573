"""Window-function measurement. No ratio is a gate.

Rows (default 100 M) in ~10^6 partitions of 100 rows, peer groups of 4:

  1. pre-sorted input (order_idx = NULL): ROW_NUMBER alone; a running SUM
     (RANGE UNBOUNDED PRECEDING .. CURRENT ROW) over one int64 column; SUM +
     MIN + RANK + LAG in one call against the same four as four calls
  2. the same with the rows scattered and a random permutation as order_idx:
     the cost of the gathers and of the scattered output
  3. Engine.window end to end (default 10 M unsorted rows), split into the
     gpue_topn full sort and the window call

Every step is a whole call (scratch allocation, every launch, the closing
stream synchronize) bracketed by stream events; after warm-up the median and
min of the repeats are reported. For 1 and 2 the algorithmic bytes are
computed from the shapes — every input column, null column and order_idx read
once, every output written once — and reported as GB/s and as a share of the
8 TB/s HBM roofline; the scans' second read of their input and the scratch
traffic are not algorithmic bytes, so they show up as a lower share.

Run: python tools/window_bench.py --out profiles/window_bench.jsonl
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine
from starrocks_amd.window import (LAG, MIN, PT_I32, PT_I64, RANK, ROW_NUMBER, SUM, WinFunc,
                                  WindowSpec, has_input)

ROOFLINE = 8e12        # bytes / s
PART_ROWS, PEER_ROWS = 100, 4


def timed(eng, fn, warmup, reps):
    ms = []
    for i in range(warmup + reps):
        eng.timer_start()
        fn()
        t = eng.timer_stop()
        if i >= warmup:
            ms.append(t)
    return float(np.median(ms)), float(np.min(ms))


def algorithmic_bytes(n, part_keys, order_keys, funcs, has_idx):
    width = lambda t: 8 if t == PT_I64 else 4
    b = 4 * n if has_idx else 0
    for k in part_keys + order_keys:
        b += n * width(k[2]) + (n if k[1] is not None else 0)
    seen = set()
    for f in funcs:                      # a column shared by several functions is read once
        if has_input(f.fn) and id(f.col) not in seen:
            seen.add(id(f.col))
            b += n * width(f.type) + (n if f.nulls is not None else 0)
    spec = WindowSpec.of(part_keys, order_keys, funcs)
    for nullable in spec.out_nullable:
        b += 8 * n + (n if nullable else 0)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--e2e-rows", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", type=int, nargs="*", default=[1, 2, 3],
                    help="which of the three measurements to run (one at a time under a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = Engine(0)
    out_f = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out_f = open(args.out, "w")

    def emit_row(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    if 1 in args.cases or 2 in args.cases:
        layouts(eng, args, emit_row)
    if 3 in args.cases:
        end_to_end(eng, args, emit_row)
    eng.close()
    if out_f:
        out_f.close()


def layouts(eng, args, emit_row):
    """Measurements 1 and 2: whole calls over sorted and over scattered rows."""
    n = args.rows

    def up(arr):
        b = eng.alloc(arr.nbytes)
        b.h2d(arr)
        return b

    # sorted columns: partition id, order key (peer groups of 4), an int64 value
    pos = np.arange(n, dtype=np.int64)
    part = up((pos // PART_ROWS).astype(np.int32))
    order = up((pos % PART_ROWS // PEER_ROWS).astype(np.int32))
    val = eng.alloc(n * 8)
    eng.gen_i64(val, 42, 7, 0, n)
    # the same rows scattered: column[j] = sorted[inv[j]], restored by order_idx = perm
    rng = np.random.default_rng(42)
    inv = rng.permutation(n).astype(np.uint32)
    perm = np.empty(n, np.uint32)
    perm[inv] = pos.astype(np.uint32)
    d_inv, d_perm = up(inv), up(perm)
    del pos, inv, perm
    s_part, s_order, s_val = eng.alloc(n * 4), eng.alloc(n * 4), eng.alloc(n * 8)
    eng.gather_u32(part, d_inv, n, s_part)
    eng.gather_u32(order, d_inv, n, s_order)
    eng.gather_u64(val, d_inv, n, s_val)
    d_inv.free()
    outs = [(eng.alloc(n * 8), eng.alloc(n)) for _ in range(4)]

    def bench(case, layout, pk, ok, col, idx):
        four = [WinFunc(SUM, col), WinFunc(MIN, col), WinFunc(RANK), WinFunc(LAG, col, param0=1)]
        sets = {"row_number": [WinFunc(ROW_NUMBER)], "running_sum": [WinFunc(SUM, col)],
                "sum_min_rank_lag_one_call": four}
        for name, funcs in sets.items():
            spec = WindowSpec.of(pk, ok, funcs)
            o = [(v, nl if nullable else None) for (v, nl), nullable in
                 zip(outs, spec.out_nullable)]
            med, mn = timed(eng, lambda: eng.window_eval(n, idx, pk, ok, funcs, o),
                            args.warmup, args.reps)
            nbytes = algorithmic_bytes(n, pk, ok, funcs, idx is not None)
            emit_row(dict(case=case, layout=layout, funcs=name, rows=n,
                          partitions=(n + PART_ROWS - 1) // PART_ROWS, ms=round(med, 3),
                          ms_min=round(mn, 3), algorithmic_bytes=nbytes,
                          gb_per_s=round(nbytes / med / 1e6, 1),
                          roofline_share=round(nbytes / (med * 1e-3) / ROOFLINE, 4)))
        spec = WindowSpec.of(pk, ok, four)
        o = [(v, nl if nullable else None) for (v, nl), nullable in zip(outs, spec.out_nullable)]

        def four_calls():
            for f, out in zip(four, o):
                eng.window_eval(n, idx, pk, ok, [f], [out])
        med, mn = timed(eng, four_calls, args.warmup, args.reps)
        nbytes = sum(algorithmic_bytes(n, pk, ok, [f], idx is not None) for f in four)
        emit_row(dict(case=case, layout=layout, funcs="sum_min_rank_lag_four_calls", rows=n,
                      partitions=(n + PART_ROWS - 1) // PART_ROWS, ms=round(med, 3),
                      ms_min=round(mn, 3), algorithmic_bytes=nbytes,
                      gb_per_s=round(nbytes / med / 1e6, 1),
                      roofline_share=round(nbytes / (med * 1e-3) / ROOFLINE, 4)))

    if 1 in args.cases:
        bench(1, "pre-sorted, order_idx = NULL", [(part, None, PT_I32)],
              [(order, None, PT_I32)], val, None)
    if 2 in args.cases:
        bench(2, "scattered, random order_idx", [(s_part, None, PT_I32)],
              [(s_order, None, PT_I32)], s_val, d_perm)
    for b in [part, order, val, s_part, s_order, s_val, d_perm] + [b for p in outs for b in p]:
        b.free()


def end_to_end(eng, args, emit_row):
    """Measurement 3: unsorted rows, the topn full sort, then the window call."""
    m = args.e2e_rows
    e_part, e_order, e_val = eng.alloc(m * 4), eng.alloc(m * 4), eng.alloc(m * 8)
    eng.gen_u32_mod(e_part, 42, 11, 0, m, max(m // PART_ROWS, 1), 0)
    eng.gen_u32_mod(e_order, 42, 12, 0, m, PART_ROWS // PEER_ROWS, 0)
    eng.gen_i64(e_val, 42, 13, 0, m)
    pk, ok = [(e_part, None, PT_I32)], [(e_order, None, PT_I32, False, True)]
    funcs = [WinFunc(SUM, e_val), WinFunc(MIN, e_val), WinFunc(RANK),
             WinFunc(LAG, e_val, param0=1)]
    e_perm = eng.alloc(m * 4)
    e_outs = [(eng.alloc(m * 8), eng.alloc(m)) for _ in funcs]
    sort_keys = [(e_part, None, PT_I32, False, True), (e_order, None, PT_I32, False, True)]
    sort_med, sort_min = timed(eng, lambda: eng.topn_into(sort_keys, m, m, 0, e_perm),
                               args.warmup, args.reps)
    spec = WindowSpec.of(pk, [k[:3] for k in ok], funcs)
    o = [(v, nl if nullable else None) for (v, nl), nullable in zip(e_outs, spec.out_nullable)]
    win_med, win_min = timed(
        eng, lambda: eng.window_eval(m, e_perm, pk, [k[:3] for k in ok], funcs, o),
        args.warmup, args.reps)

    def whole():
        for v, nl in eng.window(pk, ok, funcs, m):
            v.free()
            if nl is not None:
                nl.free()
    all_med, all_min = timed(eng, whole, args.warmup, args.reps)
    emit_row(dict(case=3, layout="unsorted, Engine.window end to end",
                  funcs="sum_min_rank_lag_one_call", rows=m,
                  partitions=max(m // PART_ROWS, 1), sort_ms=round(sort_med, 3),
                  sort_ms_min=round(sort_min, 3), window_ms=round(win_med, 3),
                  window_ms_min=round(win_min, 3), ms=round(all_med, 3),
                  ms_min=round(all_min, 3), sort_share=round(sort_med / all_med, 3)))
    for b in [e_part, e_order, e_val, e_perm] + [b for p in e_outs for b in p]:
        b.free()


if __name__ == "__main__":
    main()
