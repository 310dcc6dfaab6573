"""Scalar-expression projection measurement (DESIGN.md §4b rows "expr_project").

100 M rows of two int32 columns, a in [1, 10^7] and b in [0, 10]; no ratio is
a gate:

  a. a * b -> one int64 column: the SUM(lo_extendedprice * lo_discount)
     argument. 8 B read + 8 B written = 16 algorithmic B/row.
  b. a lone int32 -> int64 widen. 4 + 8 = 12 B/row.
  c. three outputs in ONE call — a * b (int64), a - b (int32), CASE WHEN a < b
     THEN a ELSE b END (int32): 8 + 16 = 24 B/row — against the same three as
     three separate calls: 3 x 8 read + 16 written = 40 B/row.
  d. a / b -> int64 with its null flags (b is 0 on ~1/11 of the rows):
     8 + 8 + 1 = 17 B/row. 64-bit division is a long software sequence.

Each step is one whole gpue_expr_project call (or the three of c-separate)
bracketed by stream events; the entry ends in a stream synchronize. After
warm-up the median and min of the repeated steps are reported, with the
achieved algorithmic GB/s and its fraction of the 8 TB/s HBM roofline. The
first rows of every output are checked against expr.run_program.

Run: python tools/expr_project_bench.py --out profiles/expr_project_bench.json
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine
from starrocks_amd.expr import XO_I32, XO_I64, compile_exprs, run_program
from starrocks_amd.predicate import PT_I32

ROOFLINE_GB_PER_S = 8000.0
HEAD = 4096


def timed(eng, fn, warmup, reps):
    ms = []
    for i in range(warmup + reps):
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
    results = {"rows": n, "warmup": args.warmup, "reps": args.reps,
               "roofline_gb_per_s": ROOFLINE_GB_PER_S, "cases": []}

    a, b = eng.alloc(n * 4), eng.alloc(n * 4)
    eng.gen_u32_mod(a, 42, 21, 0, n, 10_000_000, 1)
    eng.gen_u32_mod(b, 42, 22, 0, n, 11, 0)
    eng.sync()
    k = min(n, HEAD)
    head = [a.d2h(np.int32, k), b.d2h(np.int32, k)]
    A, B = ("col", 0), ("col", 1)
    mul, sub, case = ("*", A, B), ("-", A, B), ("case", [(("cmp", "<", A, B), A)], B)
    width = {XO_I32: 4, XO_I64: 8}
    in_cols = [(a, None, PT_I32), (b, None, PT_I32)]

    class Call:
        """One expr_project call over (a, b) with its own output buffers."""

        def __init__(self, trees, out_types, cols=(0, 1)):
            self.ins = [in_cols[c] for c in cols]
            self.types = out_types
            self.program, self.nullable = compile_exprs(
                trees, [PT_I32] * len(cols), [False] * len(cols), out_types)
            self.outs = [(eng.alloc(n * width[t]), eng.alloc(n) if nl else None, t)
                         for t, nl in zip(out_types, self.nullable)]
            self.write_bytes = sum(width[t] + (1 if nl else 0)
                                   for t, nl in zip(out_types, self.nullable))
            self.cols = cols

        def __call__(self):
            eng.expr_project(self.ins, self.program, n, self.outs)

        def check(self):
            self()
            want = run_program(self.program, [head[c] for c in self.cols],
                               [None] * len(self.cols), [PT_I32] * len(self.cols),
                               self.types, k)
            for (buf, nbuf, t), (val, isn) in zip(self.outs, want):
                assert np.array_equal(buf.d2h(val.dtype, k), val)
                if nbuf is not None:
                    assert np.array_equal(nbuf.d2h(np.uint8, k), isn)

        def free(self):
            for buf, nbuf, _ in self.outs:
                buf.free()
                if nbuf is not None:
                    nbuf.free()

    def record(case, calls, bytes_per_row):
        for c in calls:
            c.check()
        med, mn = timed(eng, lambda: [c() for c in calls], args.warmup, args.reps)
        gbs = bytes_per_row * n / (med / 1e3) / 1e9
        row = dict(case=case, calls=len(calls), algorithmic_bytes_per_row=bytes_per_row,
                   ms=round(med, 4), ms_min=round(mn, 4), algorithmic_gb_per_s=round(gbs, 1),
                   fraction_of_roofline=round(gbs / ROOFLINE_GB_PER_S, 3))
        results["cases"].append(row)
        print(json.dumps(row), flush=True)
        for c in calls:
            c.free()

    record("a: a * b -> int64", [Call([mul], [XO_I64])], 16)
    record("b: widen int32 -> int64", [Call([A], [XO_I64], cols=(0,))], 12)
    record("c: a*b, a-b, CASE in one call", [Call([mul, sub, case], [XO_I64, XO_I32, XO_I32])],
           24)
    record("c-separate: the same three as three calls",
           [Call([mul], [XO_I64]), Call([sub], [XO_I32]), Call([case], [XO_I32])], 40)
    record("d: a / b -> int64 + null flags", [Call([("/", A, B)], [XO_I64])], 17)

    a.free()
    b.free()
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
