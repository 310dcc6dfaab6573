"""Full-sort measurement: gpue_sort against gpue_topn with
limit = n_rows, the only full sort the engine had, on the same device buffers
in the same session.

Shapes (seed 42, generated on the device):
  a  one int64 key, random over the whole range
  b  one int32 key with 7 distinct values
  c  the window shape: int32 region (10 values) and int32 group (10^4 values)
     ascending NULLS FIRST — 10^5 partitions — then an int64 order key DESC
  d  shape c with a null mask (10 % NULL) on the region key

Row counts default to 1024, 2048, 4096, 16384, 65536, 2^20, 10^7 and 10^8. Each step
is one whole call (workspace allocation, the plan read, every launch, the
closing stream synchronize) bracketed by stream events; after warm-up the
median, min and max of the repeats are reported. Before timing, the two
permutations are compared for equality. GB/s is over the algorithmic bytes —
every key column and null mask read once, the permutation written once — and
roofline_share is that rate over the 8 TB/s HBM peak; a multi-pass sort moves
a multiple of those bytes and is not expected to come near it.

Extra rows: up to GPUE_SORT_SMALL_MAX rows gpue_sort runs gpue_topn's
single-tile path, so there the radix passes are timed separately with the
switch disabled (sort_radix_ms) to show the crossover; at 10^7 rows of shape c
the rejected variant that gathers the key column again on every pass
(GPUE_SORT_REGATHER) is timed next to the carried-key default; and
Engine.window end to end over 10^7 unsorted rows, the shape of
tools/window_bench.py case 3, split into the sort and the window call.

Run: python tools/sort_bench.py --out profiles/sort_bench.jsonl
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine
from starrocks_amd.window import LAG, MIN, PT_I32, PT_I64, RANK, SUM, WinFunc, WindowSpec

ROOFLINE = 8e12        # bytes / s
I32, I64 = Engine.TOPN_I32, Engine.TOPN_I64


def timed(eng, fn, warmup, reps):
    ms = []
    for i in range(warmup + reps):
        eng.timer_start()
        fn()
        t = eng.timer_stop()
        if i >= warmup:
            ms.append(t)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def make_shapes(eng, n):
    """Device columns for n rows; returns ({shape: (keys, algorithmic bytes)}, buffers)."""
    v64, seven, region, group = (eng.alloc(n * 8), eng.alloc(n * 4), eng.alloc(n * 4),
                                 eng.alloc(n * 4))
    eng.gen_i64(v64, 42, 1, 0, n)
    eng.gen_u32_mod(seven, 42, 2, 0, n, 7, 0)
    eng.gen_u32_mod(region, 42, 3, 0, n, 10, 0)
    eng.gen_u32_mod(group, 42, 4, 0, n, 10_000, 0)
    mask = eng.alloc(n)
    mask.h2d((np.random.default_rng(42).integers(0, 10, n, dtype=np.uint8) == 0).astype(np.uint8))
    window = lambda nulls: [(region, nulls, I32, False, True), (group, None, I32, False, True),
                            (v64, None, I64, True, False)]
    shapes = {
        "a: int64 random": ([(v64, None, I64, False, False)], 8 * n + 4 * n),
        "b: int32, 7 values": ([(seven, None, I32, False, False)], 4 * n + 4 * n),
        "c: window, 2 x int32 + int64 DESC": (window(None), 16 * n + 4 * n),
        "d: c with a nullable region": (window(mask), 17 * n + 4 * n),
    }
    return shapes, [v64, seven, region, group, mask]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*",
                    default=[1024, 2048, 4096, 16384, 65536, 1 << 20, 10_000_000, 100_000_000])
    ap.add_argument("--e2e-rows", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
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

    for n in args.rows:
        shapes, bufs = make_shapes(eng, n)
        out_s, out_t = eng.alloc(n * 4), eng.alloc(n * 4)
        reps = args.reps if n <= 10_000_000 else max(3, args.reps // 2)
        for name, (keys, nbytes) in shapes.items():
            eng.sort_into(keys, n, out_s)
            assert eng.topn_into(keys, n, n, 0, out_t) == n
            assert out_s.d2h(np.uint32, n).tobytes() == out_t.d2h(np.uint32, n).tobytes(), name
            s_med, s_min, s_max = timed(eng, lambda: eng.sort_into(keys, n, out_s),
                                        args.warmup, reps)
            t_med, t_min, t_max = timed(eng, lambda: eng.topn_into(keys, n, n, 0, out_t),
                                        args.warmup, reps)
            row = dict(shape=name, rows=n, reps=reps, sort_ms=round(s_med, 4),
                       sort_ms_min=round(s_min, 4), sort_ms_max=round(s_max, 4),
                       topn_ms=round(t_med, 4), topn_ms_min=round(t_min, 4),
                       topn_ms_max=round(t_max, 4), speedup=round(t_med / s_med, 2),
                       slowest_sort_beats_fastest_topn=bool(s_max < t_min),
                       algorithmic_bytes=nbytes, sort_gb_per_s=round(nbytes / s_med / 1e6, 1),
                       sort_roofline_share=round(nbytes / (s_med * 1e-3) / ROOFLINE, 4))
            if n <= Engine.SORT_SMALL_MAX:    # the radix passes without the small-input switch
                os.environ["GPUE_SORT_SMALL_MAX"] = "0"
                try:
                    eng.sort_into(keys, n, out_s)
                    assert out_s.d2h(np.uint32, n).tobytes() == out_t.d2h(np.uint32, n).tobytes()
                    r = timed(eng, lambda: eng.sort_into(keys, n, out_s), args.warmup, reps)
                finally:
                    del os.environ["GPUE_SORT_SMALL_MAX"]
                row.update(sort_radix_ms=round(r[0], 4), sort_radix_ms_min=round(r[1], 4))
            if n == 10_000_000 and name.startswith("c:"):   # carried key against re-gather
                os.environ["GPUE_SORT_REGATHER"] = "1"
                try:
                    eng.sort_into(keys, n, out_s)
                    assert out_s.d2h(np.uint32, n).tobytes() == out_t.d2h(np.uint32, n).tobytes()
                    r = timed(eng, lambda: eng.sort_into(keys, n, out_s), args.warmup, reps)
                finally:
                    del os.environ["GPUE_SORT_REGATHER"]
                row.update(regather_ms=round(r[0], 4), regather_ms_min=round(r[1], 4))
            emit_row(row)
        for b in bufs + [out_s, out_t]:
            b.free()

    if args.e2e_rows:
        end_to_end(eng, args, emit_row)
    eng.close()
    if out_f:
        out_f.close()


def end_to_end(eng, args, emit_row):
    """Engine.window over unsorted rows (tools/window_bench.py case 3), with
    the sort timed through both entries."""
    m = args.e2e_rows
    part_rows, peer_rows = 100, 4
    e_part, e_order, e_val = eng.alloc(m * 4), eng.alloc(m * 4), eng.alloc(m * 8)
    eng.gen_u32_mod(e_part, 42, 11, 0, m, max(m // part_rows, 1), 0)
    eng.gen_u32_mod(e_order, 42, 12, 0, m, part_rows // peer_rows, 0)
    eng.gen_i64(e_val, 42, 13, 0, m)
    pk, ok = [(e_part, None, PT_I32)], [(e_order, None, PT_I32, False, True)]
    funcs = [WinFunc(SUM, e_val), WinFunc(MIN, e_val), WinFunc(RANK),
             WinFunc(LAG, e_val, param0=1)]
    e_perm = eng.alloc(m * 4)
    e_outs = [(eng.alloc(m * 8), eng.alloc(m)) for _ in funcs]
    sort_keys = [(e_part, None, PT_I32, False, True), (e_order, None, PT_I32, False, True)]
    topn = timed(eng, lambda: eng.topn_into(sort_keys, m, m, 0, e_perm), args.warmup, args.reps)
    sort = timed(eng, lambda: eng.sort_into(sort_keys, m, e_perm), args.warmup, args.reps)
    spec = WindowSpec.of(pk, [k[:3] for k in ok], funcs)
    o = [(v, nl if nullable else None) for (v, nl), nullable in zip(e_outs, spec.out_nullable)]
    win = timed(eng, lambda: eng.window_eval(m, e_perm, pk, [k[:3] for k in ok], funcs, o),
                args.warmup, args.reps)

    def whole():
        for v, nl in eng.window(pk, ok, funcs, m):
            v.free()
            if nl is not None:
                nl.free()
    e2e = timed(eng, whole, args.warmup, args.reps)
    emit_row(dict(shape="Engine.window end to end, unsorted", rows=m,
                  partitions=max(m // part_rows, 1), funcs="sum_min_rank_lag_one_call",
                  sort_ms=round(sort[0], 3), sort_ms_min=round(sort[1], 3),
                  topn_ms=round(topn[0], 3), topn_ms_min=round(topn[1], 3),
                  window_ms=round(win[0], 3), window_ms_min=round(win[1], 3),
                  ms=round(e2e[0], 3), ms_min=round(e2e[1], 3),
                  sort_share=round(sort[0] / e2e[0], 3)))
    for b in [e_part, e_order, e_val, e_perm] + [b for p in e_outs for b in p]:
        b.free()


if __name__ == "__main__":
    main()
