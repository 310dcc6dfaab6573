"""General GROUP BY measurement against the single-key
entries, timed in the same session. No ratio is a gate.

Rows (default 100 M) at group counts 16, 10^3, 10^5, 10^6:

  a. one int64 key, SUM + COUNT_STAR            vs  hash_agg_sum_u64
  b. one int64 key, SUM, COUNT, MIN, MAX of one column
                                                vs  hash_agg_stats_u64
  c. two int32 keys, SUM / MIN / MAX / COUNT over two int64 columns in one
     pass                  vs  pack_keys_2xi32 + two hash_agg_stats_u64 calls
  d. shape c with the second key and both inputs nullable (~9 % NULLs, the
     null flags a / b leaves behind): no counterpart

Every step is the whole call sequence a caller pays for — the general path:
create (capacity hint 2 x groups, as the old entries get), push, emit into
preallocated outputs, destroy; the old path: its one-shot entry (which
allocates, builds and emits inside) — bracketed by stream events; every entry
ends in a stream synchronize. "push_ms" times the push alone into a table
that already holds every group, the streaming operator's steady state. After
warm-up the median and min of the repeated steps are reported.

--variants also runs the two layout experiments of DESIGN.md §4g through the
GPUE_GA_LAYOUT / GPUE_GA_COMBINE switches: AoS states, and the wave-level
pre-combine off / forced on.

Group counts and COUNT totals of both paths are checked against each other.

Run: python tools/group_agg_bench.py --variants --out profiles/group_agg_bench.jsonl
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine
from starrocks_amd.groupagg import COUNT, COUNT_STAR, MAX, MIN, PT_I32, PT_I64, SUM

SPLIT = {16: (4, 4), 1000: (40, 25), 100_000: (400, 250), 1_000_000: (1000, 1000)}


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
    ap.add_argument("--groups", type=int, nargs="*", default=[16, 1000, 100_000, 1_000_000])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
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

    # two int64 value columns, and a 0/1.. divisor that leaves ~9 % NULLs behind
    r32 = eng.alloc(n * 4)
    vals = []
    for tag in (31, 32):
        eng.gen_u32_mod(r32, 42, tag, 0, n, 2_000_001, 0)
        (v, _), = eng.project([("-", ("col", 0), ("const", 1_000_000))], [(r32, None, PT_I32)],
                              [eng.XO_I64], n)
        vals.append(v)
    eng.gen_u32_mod(r32, 42, 33, 0, n, 11, 0)
    nvals = []
    for v in vals:
        (q, nl), = eng.project([("/", ("col", 0), ("col", 1))],
                               [(v, None, PT_I64), (r32, None, PT_I32)], [eng.XO_I64], n)
        nvals.append((q, nl))
    max_g = max(args.groups) * 9 // 8 + 64      # shape d adds the NULL-key groups
    outs = [eng.alloc(max_g * 8) for _ in range(12)]
    onul = [eng.alloc(max_g) for _ in range(12)]

    def general(keys, aggs, g):
        """keys = [(DBuf, nulls, type)], aggs = [(fn, DBuf, nulls, type)] -> step fn."""
        kt, kn = [k[2] for k in keys], [k[1] is not None for k in keys]
        af, at, an = [a[0] for a in aggs], [a[3] for a in aggs], [a[2] is not None for a in aggs]
        pk, pa = [(k[0], k[1]) for k in keys], [(a[1], a[2]) for a in aggs]
        ok = [(outs[i], onul[i] if kn[i] else None) for i in range(len(keys))]
        oa = [(outs[4 + i], onul[4 + i] if (af[i] >= SUM and an[i]) else None)
              for i in range(len(aggs))]
        state = {}

        def step():
            ga = eng.group_agg_create(kt, kn, af, at, an, capacity_hint=2 * g)
            eng.group_agg_push(ga, pk, pa, n)
            state["groups"] = eng.group_agg_emit(ga, ok, oa, max_g)
            eng.group_agg_destroy(ga)

        def prepare():
            state["ga"] = eng.group_agg_create(kt, kn, af, at, an, capacity_hint=2 * g)
            eng.group_agg_push(state["ga"], pk, pa, n)

        def push():
            eng.group_agg_push(state["ga"], pk, pa, n)

        def done():
            eng.group_agg_destroy(state.pop("ga"))

        return step, prepare, push, done, state, oa

    def run_general(shape, g, keys, aggs, variant, env):
        for k in ("GPUE_GA_LAYOUT", "GPUE_GA_COMBINE"):
            os.environ.pop(k, None)
        os.environ.update(env)
        step, prepare, push, done, state, oa = general(keys, aggs, g)
        med, mn = timed(eng, step, args.warmup, args.reps)
        prepare()
        pmed, pmn = timed(eng, push, 0, 3)
        done()
        emit_row(dict(shape=shape, path="group_agg", variant=variant, groups=g, rows=n,
                      n_groups_out=state["groups"], ms=round(med, 3), ms_min=round(mn, 3),
                      push_ms=round(pmed, 3), push_ms_min=round(pmn, 3),
                      grows_per_s=round(n / med / 1e6, 2)))
        for k in env:
            os.environ.pop(k, None)
        return state["groups"], oa

    variants = [("soa, combine at <= 32 groups (default)", {})]
    if args.variants:
        variants += [("aos, combine at <= 32 groups", {"GPUE_GA_LAYOUT": "aos"}),
                     ("soa, no combine", {"GPUE_GA_COMBINE": "0"}),
                     ("soa, combine forced", {"GPUE_GA_COMBINE": "2"})]

    k64 = None
    for g in args.groups:
        ga_, gb_ = SPLIT.get(g, (g, 1))
        # one int64 key in [0, g); two int32 keys in [0, ga) x [0, gb)
        eng.gen_u32_mod(r32, 42, 40, 0, n, g, 0)
        (k64, _), = eng.project([("col", 0)], [(r32, None, PT_I32)], [eng.XO_I64], n)
        ka, kb = eng.alloc(n * 4), eng.alloc(n * 4)
        eng.gen_u32_mod(ka, 42, 41, 0, n, ga_, 0)
        eng.gen_u32_mod(kb, 42, 42, 0, n, gb_, 0)
        eng.gen_u32_mod(r32, 42, 43, 0, n, 11, 0)
        (kbn, kbn_nl), = eng.project([("/", ("col", 0), ("col", 1))],
                                     [(kb, None, PT_I32), (r32, None, PT_I32)],
                                     [eng.XO_I32], n)
        packed = eng.alloc(n * 8)
        v0, v1 = vals

        # ---- the single-key entries, same session ----
        st = {}

        def old_sum():
            st["g"] = eng.hash_agg_sum_u64(k64, v0, n, outs[0], outs[1], out_counts=outs[2],
                                           max_out=max_g, capacity_hint=2 * g)

        def old_stats():
            st["g"] = eng.hash_agg_stats_u64(k64, v0, n, *outs[:5], max_out=max_g,
                                             capacity_hint=2 * g)

        def old_two_stats():
            eng.pack_keys_2xi32(ka, kb, n, packed)
            st["g"] = eng.hash_agg_stats_u64(packed, v0, n, *outs[:5], max_out=max_g,
                                             capacity_hint=2 * g)
            eng.hash_agg_stats_u64(packed, v1, n, outs[0], *outs[5:9], max_out=max_g,
                                   capacity_hint=2 * g)

        old_groups = {}
        for shape, fn, name in (("a", old_sum, "hash_agg_sum_u64"),
                                ("b", old_stats, "hash_agg_stats_u64"),
                                ("c", old_two_stats,
                                 "pack_keys_2xi32 + 2 x hash_agg_stats_u64")):
            med, mn = timed(eng, fn, args.warmup, args.reps)
            old_groups[shape] = st["g"]
            assert int(outs[2].d2h(np.int64, st["g"]).sum()) == n
            emit_row(dict(shape=shape, path=name, groups=g, rows=n, n_groups_out=st["g"],
                          ms=round(med, 3), ms_min=round(mn, 3),
                          grows_per_s=round(n / med / 1e6, 2)))

        # ---- the general table ----
        two = [(SUM, v0, None, PT_I64), (MIN, v0, None, PT_I64), (MAX, v0, None, PT_I64),
               (COUNT, v0, None, PT_I64), (SUM, v1, None, PT_I64), (MIN, v1, None, PT_I64),
               (MAX, v1, None, PT_I64), (COUNT, v1, None, PT_I64)]
        (q0, n0), (q1, n1) = nvals
        two_null = [(f, q0 if i < 4 else q1, n0 if i < 4 else n1, PT_I64)
                    for i, (f, _, _, _) in enumerate(two)]
        shapes = [
            ("a", [(k64, None, PT_I64)],
             [(SUM, v0, None, PT_I64), (COUNT_STAR, None, None, PT_I64)], 1),
            ("b", [(k64, None, PT_I64)],
             [(SUM, v0, None, PT_I64), (COUNT, v0, None, PT_I64), (MIN, v0, None, PT_I64),
              (MAX, v0, None, PT_I64)], 1),
            ("c", [(ka, None, PT_I32), (kb, None, PT_I32)], two, 3),
            ("d", [(ka, None, PT_I32), (kbn, kbn_nl, PT_I32)], two_null, None),
        ]
        for shape, keys, aggs, cnt_at in shapes:
            for variant, env in variants:
                if env.get("GPUE_GA_COMBINE") == "2" and g > 1000:
                    continue            # 64 rounds per wave: only of interest at low cardinality
                groups, oa = run_general(shape, g, keys, aggs, variant, env)
                if shape in old_groups:
                    assert groups == old_groups[shape], (shape, groups, old_groups[shape])
                if cnt_at is not None:
                    assert int(oa[cnt_at][0].d2h(np.int64, groups).sum()) == n
        for b in (k64, ka, kb, kbn, kbn_nl, packed):
            b.free()

    eng.close()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
