"""General hash join measurement: gpue_hash_join_* against
the per-key-shape entries it generalises, in the same session on the same
device buffers.

Shapes (seed 42; probe columns generated on the device):
  a  one int32 key, 10^6 unique build rows, 10^8 probe rows (half match),
     INNER, against gpue_join_build_auto_i32 + gpue_join_probe_emit_mode_i32
  b  two int32 keys, same sizes, against gpue_pack_keys_2xi32 on both sides +
     gpue_join_build_bucket_chained_u64 + gpue_join_probe_emit_mode_u64
  c  shape b with ~10 % NULLs on the second key of both sides, LEFT_OUTER,
     once plain and once null-safe; no counterpart
  d  one int64 key with 16 and with 1024 duplicates per build key (2^20 build
     rows), LEFT_SEMI over 10^7 probe rows and INNER over as many probe rows
     as give ~3 x 10^7 pairs, against the _u64 bucket-chained entries
  e  the build alone: 10^7 unique int64 keys in one push (from the smallest
     capacity_hint and from an exact one) and in 4096-row pushes

Each step is one whole call (scratch allocation, every launch, the closing
stream synchronize) bracketed by gpue_timer_*; the emit calls write into
outputs sized by a count-only call made before. After warm-up the two sides
alternate, and the median, min and max of the repeats are reported. Before
timing, the two pair lists are compared: element by element where every probe
row has at most one match, else by count and an order-independent 64-bit hash
of the (probe, build) pairs. GB/s is over the algorithmic bytes — each key
column and null mask read once, the pairs written once — and roofline_share
is that rate over the 8 TB/s HBM peak.

Run: python tools/hash_join_bench.py --out profiles/hash_join_bench.jsonl
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine
from starrocks_amd.hashjoin import INNER, LEFT_OUTER, LEFT_SEMI, PT_I32, PT_I64

ROOFLINE = 8e12        # bytes / s


def timed_pair(eng, fns, warmup, reps):
    """Alternate the callables; per callable (median, min, max) ms."""
    ms = [[] for _ in fns]
    for i in range(warmup + reps):
        for j, fn in enumerate(fns):
            eng.timer_start()
            fn()
            t = eng.timer_stop()
            if i >= warmup:
                ms[j].append(t)
    return [(float(np.median(m)), float(np.min(m)), float(np.max(m))) for m in ms]


def pair_hash(p, b):
    """Order-independent hash of a pair multiset."""
    h = (p.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ b.astype(np.uint64)
    h = h * np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(29)
    return int(np.sum(h, dtype=np.uint64))


def stats(prefix, t):
    return {f"{prefix}_ms": round(t[0], 4), f"{prefix}_ms_min": round(t[1], 4),
            f"{prefix}_ms_max": round(t[2], 4)}


class Bench:
    def __init__(self, eng, args, emit_row):
        self.eng, self.args, self.emit_row = eng, args, emit_row
        self.bufs = []

    def alloc(self, nbytes):
        self.bufs.append(self.eng.alloc(max(nbytes, 8)))
        return self.bufs[-1]

    def put(self, arr):
        return self.alloc(arr.nbytes).h2d(arr)

    def view(self, buf, offset, nbytes):
        self.bufs.append(self.eng.wrap_ptr_offset(buf, offset, nbytes))
        return self.bufs[-1]

    def free_all(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def gen_mod(self, n, tag, mod, add=0):
        b = self.alloc(n * 4)
        self.eng.gen_u32_mod(b, 42, tag, 0, n, mod, add)
        return b

    def new_table(self, btypes, ptypes, nullable, null_safe, build_cols, n_build, hint=None):
        e = self.eng
        t = e.hash_join_create(btypes, ptypes, nullable, null_safe,
                               n_build if hint is None else hint)
        e.hash_join_build_push(t, build_cols, n_build)
        return t

    def probe_new(self, t, pcols, n, mode):
        """(count, out_probe, out_build) after one count-only + one emit call"""
        e = self.eng
        cnt = e.hash_join_probe(t, pcols, n, mode)
        op, ob = self.alloc(cnt * 4), self.alloc(cnt * 4)
        assert e.hash_join_probe(t, pcols, n, mode, 0, op, ob) == cnt
        return cnt, op, ob

    def compare(self, cnt, new, old, exact):
        """new / old = (out_probe, out_build) DBufs; old build rows are 1-based"""
        if cnt == 0:
            return
        np_, nb_ = new[0].d2h(np.uint32, cnt), new[1].d2h(np.uint32, cnt)
        op_, ob_ = old[0].d2h(np.uint32, cnt), old[1].d2h(np.uint32, cnt)
        ob_ = ob_ - np.uint32(1)
        if exact:
            assert np.array_equal(np_, op_) and np.array_equal(nb_, ob_), "pairs differ"
        else:
            assert pair_hash(np_, nb_) == pair_hash(op_, ob_), "pair multisets differ"

    def row(self, shape, n_build, n_probe, mode, cnt, key_bytes, new_t, old_t=None, **extra):
        nbytes = key_bytes + 8 * cnt
        r = dict(shape=shape, build_rows=n_build, probe_rows=n_probe, mode=mode, pairs=cnt,
                 reps=self.args.reps, **stats("general", new_t))
        if old_t is not None:
            r.update(stats("old", old_t))
            r.update(general_over_old=round(new_t[0] / old_t[0], 3),
                     general_is_faster=bool(new_t[0] < old_t[0]))
        r.update(algorithmic_bytes=nbytes, general_gb_per_s=round(nbytes / new_t[0] / 1e6, 1),
                 general_roofline_share=round(nbytes / (new_t[0] * 1e-3) / ROOFLINE, 4), **extra)
        self.emit_row(r)

    # ---- a: one int32 key ----
    def shape_a(self):
        e, a = self.eng, self.args
        nb, n = a.build_rows, a.probe_rows
        keys = np.random.default_rng(42).permutation(nb).astype(np.int32) + 1
        old_keys = self.put(np.concatenate([[0], keys]).astype(np.int32))  # row 0: sentinel
        new_keys = self.view(old_keys, 4, nb * 4)
        pk = self.gen_mod(n, 1, 2 * nb, 1)
        t_old, method = e.join_build_auto(old_keys, nb)
        t_new = self.new_table([PT_I32], [PT_I32], [0], [0], [(new_keys, None)], nb)
        try:
            cnt, op, ob = self.probe_new(t_new, [(pk, None)], n, INNER)
            assert e.join_probe_emit_mode(t_old, pk, n, 0) == cnt
            op2, ob2 = self.alloc(cnt * 4), self.alloc(cnt * 4)
            e.join_probe_emit_mode(t_old, pk, n, 0, op2, ob2)
            self.compare(cnt, (op, ob), (op2, ob2), exact=True)
            new_t, old_t = timed_pair(
                e, [lambda: e.hash_join_probe(t_new, [(pk, None)], n, INNER, 0, op, ob),
                    lambda: e.join_probe_emit_mode(t_old, pk, n, 0, op2, ob2)],
                a.warmup, a.reps)
            self.row("a: one int32 key, unique build", nb, n, "inner", cnt, 4 * n, new_t, old_t,
                     old_method=e.JM_NAMES[method])
        finally:
            e.hash_join_destroy(t_new)
            t_old.destroy()

    # ---- b, c: two int32 keys ----
    def shape_bc(self):
        e, a = self.eng, self.args
        nb, n = a.build_rows, a.probe_rows
        side = max(int(np.sqrt(nb)), 1)
        i = np.arange(nb)
        b1 = np.concatenate([[0], i % side]).astype(np.int32)      # row 0: sentinel
        b2 = np.concatenate([[0], i // side]).astype(np.int32)
        d_b1, d_b2 = self.put(b1), self.put(b2)
        n_b1, n_b2 = self.view(d_b1, 4, nb * 4), self.view(d_b2, 4, nb * 4)
        p1 = self.gen_mod(n, 2, side)
        p2 = self.gen_mod(n, 3, 2 * ((nb + side - 1) // side))     # half the tuples match
        packed_b, packed_p = self.alloc((nb + 1) * 8), self.alloc(n * 8)
        e.pack_keys_2xi32(d_b1, d_b2, nb + 1, packed_b)
        t_old = e.join_build_bucket_chained_u64(packed_b, nb)
        t_new = self.new_table([PT_I32] * 2, [PT_I32] * 2, [0, 0], [0, 0],
                               [(n_b1, None), (n_b2, None)], nb)
        pcols = [(p1, None), (p2, None)]
        try:
            cnt, op, ob = self.probe_new(t_new, pcols, n, INNER)
            e.pack_keys_2xi32(p1, p2, n, packed_p)
            assert e.join_probe_emit_u64(t_old, packed_p, n, 0) == cnt
            op2, ob2 = self.alloc(cnt * 4), self.alloc(cnt * 4)

            def old_probe():  # the packing is part of the old route's probe
                e.pack_keys_2xi32(p1, p2, n, packed_p)
                e.join_probe_emit_u64(t_old, packed_p, n, 0, op2, ob2)

            old_probe()
            self.compare(cnt, (op, ob), (op2, ob2), exact=True)
            new_t, old_t = timed_pair(
                e, [lambda: e.hash_join_probe(t_new, pcols, n, INNER, 0, op, ob), old_probe],
                a.warmup, a.reps)
            self.row("b: two int32 keys, unique build", nb, n, "inner", cnt, 8 * n, new_t, old_t,
                     old_route="pack_keys_2xi32 + bucket_chained_u64")
        finally:
            e.hash_join_destroy(t_new)
            t_old.destroy()
        # c: ~10 % NULLs on the second key of both sides, LEFT_OUTER
        rng = np.random.default_rng(43)
        bn = self.put((rng.random(nb) < 0.1).astype(np.uint8))
        pn = self.put((rng.random(n) < 0.1).astype(np.uint8))
        for null_safe in (0, 1):
            t = self.new_table([PT_I32] * 2, [PT_I32] * 2, [0, 1], [0, null_safe],
                               [(n_b1, None), (n_b2, bn)], nb)
            try:
                pc = [(p1, None), (p2, pn)]
                cnt, op, ob = self.probe_new(t, pc, n, LEFT_OUTER)
                assert cnt >= n
                (new_t,) = timed_pair(
                    e, [lambda: e.hash_join_probe(t, pc, n, LEFT_OUTER, 0, op, ob)],
                    a.warmup, a.reps)
                self.row("c: shape b, 10 % NULLs on key 2, " +
                         ("null-safe" if null_safe else "plain"), nb, n, "left_outer", cnt,
                         9 * n, new_t)
            finally:
                e.hash_join_destroy(t)

    # ---- d: one int64 key with duplicates ----
    def shape_d(self):
        e, a = self.eng, self.args
        nb = a.dup_build_rows
        for dup in (16, 1024):
            n_keys = max(nb // dup, 1)
            keys = (np.arange(nb) % n_keys).astype(np.int64) * 7919 + 1
            old_keys = self.put(np.concatenate([[0], keys]).astype(np.int64))
            new_keys = self.view(old_keys, 8, nb * 8)
            t_old = e.join_build_bucket_chained_u64(old_keys, nb)
            t_new = self.new_table([PT_I64], [PT_I64], [0], [0], [(new_keys, None)], nb)
            try:
                for mode, name, n in ((LEFT_SEMI, "left_semi", a.semi_probe_rows),
                                      (INNER, "inner", max(2 * a.inner_pairs // dup, 1))):
                    idx = self.gen_mod(n, 4 + mode, 2 * n_keys)    # half the rows match
                    pk = self.alloc(n * 8)
                    pk.h2d(idx.d2h(np.uint32, n).astype(np.int64) * 7919 + 1)
                    cnt, op, ob = self.probe_new(t_new, [(pk, None)], n, mode)
                    assert e.join_probe_emit_u64(t_old, pk, n, mode) == cnt
                    op2, ob2 = self.alloc(cnt * 4), self.alloc(cnt * 4)
                    e.join_probe_emit_u64(t_old, pk, n, mode, op2, ob2)
                    if mode == LEFT_SEMI:  # which match is reported may differ: rows only
                        assert np.array_equal(op.d2h(np.uint32, cnt), op2.d2h(np.uint32, cnt))
                    else:
                        self.compare(cnt, (op, ob), (op2, ob2), exact=False)
                    new_t, old_t = timed_pair(
                        e, [lambda: e.hash_join_probe(t_new, [(pk, None)], n, mode, 0, op, ob),
                            lambda: e.join_probe_emit_u64(t_old, pk, n, mode, op2, ob2)],
                        a.warmup, a.reps)
                    self.row(f"d: one int64 key, {dup} duplicates per build key", nb, n, name,
                             cnt, 8 * n, new_t, old_t)
            finally:
                e.hash_join_destroy(t_new)
                t_old.destroy()
            self.free_all()

    # ---- e: the build alone ----
    def shape_e(self):
        e, a = self.eng, self.args
        n = a.push_rows
        keys = self.alloc(n * 8)
        e.gen_i64(keys, 42, 9, 0, n)
        chunk = 4096
        parts = [(self.view(keys, lo * 8, min(chunk, n - lo) * 8), min(chunk, n - lo))
                 for lo in range(0, n, chunk)]
        last = {}

        def build(hint, pieces):
            t = e.hash_join_create([PT_I64], [PT_I64], [0], [0], hint)
            for buf, rows in pieces:
                e.hash_join_build_push(t, [(buf, None)], rows)
            last.update(e.hash_join_stats(t), rows=e.hash_join_build_rows(t))
            e.hash_join_destroy(t)

        for name, hint, pieces in (("one push, capacity_hint 0", 0, [(keys, n)]),
                                   ("one push, exact capacity_hint", n, [(keys, n)]),
                                   (f"{len(parts)} pushes of {chunk} rows, capacity_hint 0", 0,
                                    parts)):
            (t,) = timed_pair(e, [lambda: build(hint, pieces)], 1, max(3, a.reps // 2))
            assert last["rows"] == n
            self.emit_row(dict(shape="e: build alone, unique int64 keys, " + name, build_rows=n,
                               pushes=len(pieces), **stats("general", t),
                               rows_per_s=round(n / (t[0] * 1e-3)),
                               algorithmic_bytes=8 * n, general_gb_per_s=round(8 * n / t[0] / 1e6, 1),
                               general_roofline_share=round(8 * n / (t[0] * 1e-3) / ROOFLINE, 5),
                               slot_capacity=last["capacity"], doublings=last["doublings"],
                               rehashes=last["rehashes"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-rows", type=int, default=1_000_000)
    ap.add_argument("--probe-rows", type=int, default=100_000_000)
    ap.add_argument("--dup-build-rows", type=int, default=1 << 20)
    ap.add_argument("--semi-probe-rows", type=int, default=10_000_000)
    ap.add_argument("--inner-pairs", type=int, default=30_000_000)
    ap.add_argument("--push-rows", type=int, default=10_000_000)
    ap.add_argument("--shapes", default="abcde")
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

    bench = Bench(eng, args, emit_row)
    steps = (("a", bench.shape_a), ("bc", bench.shape_bc), ("d", bench.shape_d),
             ("e", bench.shape_e))
    failed = 0
    for letters, fn in steps:
        if any(c in args.shapes for c in letters):
            try:
                fn()
            except Exception as exc:  # the other shapes still run; the exit status tells
                failed += 1
                emit_row(dict(shape=letters, error=f"{type(exc).__name__}: {exc}"))
            finally:
                bench.free_all()
    eng.close()
    if out_f:
        out_f.close()
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
