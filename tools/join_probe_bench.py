"""Generic (non-fused) hash-join probe timing (DESIGN.md §4b evidence).

Per table shape: 1 M build rows with keys in [0, 250 000) (~4-entry chains),
20 M probe rows over the same key space. Times best-of-5 of the count-only
call (count kernel + scan to the total) and of the full emit call (count,
scan, offsets, emit) through the Engine API only, so it runs unchanged on any
commit that has these entry points. Prints one JSON line per case.

Cases: mode 0 (INNER) for rd, dense, lc, bc, u64, u128 and varchar (16-byte
keys); mode 3 (LEFT_OUTER) for bc; RIGHT SEMI for bc.

Run: python tools/join_probe_bench.py [probe_rows] > join_probe_bench.jsonl
"""

import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np

from starrocks_amd.engine import Engine

N_BUILD = 1_000_000
N_KEYS = 250_000
REPS = 5


def best_of(fn):
    best = None
    for _ in range(REPS):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def put(eng, arr):
    b = eng.alloc(arr.nbytes)
    b.h2d(arr)
    return b


def u64_keys(k):
    return k.astype(np.uint64) * np.uint64(0x100000001)


def u128_keys(k):
    out = np.empty((len(k), 2), np.uint64)
    out[:, 0] = u64_keys(k)
    out[:, 1] = ~k.astype(np.uint64)
    return out


def main():
    n_probe = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
    eng = Engine()
    rng = np.random.default_rng(42)
    bk = np.concatenate([[0], rng.integers(0, N_KEYS, N_BUILD)]).astype(np.int32)
    pk = rng.integers(0, N_KEYS, n_probe).astype(np.int32)

    def i32_case(build):
        d_bk = put(eng, bk)
        t = build(d_bk, N_BUILD)
        d_pk = put(eng, pk)
        return t, [d_pk, d_bk], lambda m, op=None, ob=None: eng.join_probe_emit_mode(
            t, d_pk, n_probe, m, op, ob)

    def u64_case():
        d_bk = put(eng, u64_keys(bk))
        t = eng.join_build_bucket_chained_u64(d_bk, N_BUILD)
        d_pk = put(eng, u64_keys(pk))
        return t, [d_pk, d_bk], lambda m, op=None, ob=None: eng.join_probe_emit_u64(
            t, d_pk, n_probe, m, op, ob)

    def u128_case():
        d_bk = put(eng, u128_keys(bk))
        t = eng.join_build_bucket_chained_u128(d_bk, N_BUILD)
        d_pk = put(eng, u128_keys(pk))
        return t, [d_pk, d_bk], lambda m, op=None, ob=None: eng.join_probe_emit_mode_u128(
            t, d_pk, n_probe, m, op, ob)

    def vc_case():  # the same 16 key bytes as fixed-width slices
        bo = np.arange(N_BUILD + 2, dtype=np.uint32) * 16
        po = np.arange(n_probe + 1, dtype=np.uint32) * 16
        d_bb = put(eng, u128_keys(bk).view(np.uint8).reshape(-1))
        d_bo = put(eng, bo)
        t = eng.join_build_varchar(d_bb, d_bo, N_BUILD)
        d_pb = put(eng, u128_keys(pk).view(np.uint8).reshape(-1))
        d_po = put(eng, po)
        return t, [d_pb, d_po, d_bb, d_bo], lambda m, op=None, ob=None: eng.join_probe_emit_varchar_mode(
            t, d_pb, d_po, n_probe, m, op, ob)

    cases = [
        ("rd", 0, lambda: i32_case(eng.join_build_range_direct)),
        ("dense", 0, lambda: i32_case(eng.join_build_dense_range_direct)),
        ("lc", 0, lambda: i32_case(eng.join_build_linear_chained)),
        ("bc", 0, lambda: i32_case(eng.join_build_bucket_chained)),
        ("u64", 0, u64_case),
        ("u128", 0, u128_case),
        ("varchar16", 0, vc_case),
        ("bc", 3, lambda: i32_case(eng.join_build_bucket_chained)),
    ]
    for name, mode, make in cases:
        t, bufs, probe = make()
        cnt = probe(mode)  # warm
        op, ob = eng.alloc(max(cnt, 1) * 4), eng.alloc(max(cnt, 1) * 4)
        probe(mode, op, ob)
        count_s, c1 = best_of(lambda: probe(mode))
        emit_s, c2 = best_of(lambda: probe(mode, op, ob))
        assert c1 == cnt and c2 == cnt
        print(json.dumps({"case": f"{name}_mode{mode}", "build_rows": N_BUILD,
                          "probe_rows": n_probe, "pairs": int(cnt),
                          "count_s": round(count_s, 5), "emit_s": round(emit_s, 5)}),
              flush=True)
        t.destroy()
        for b in bufs + [op, ob]:
            b.free()

    # RIGHT SEMI over bc: mark + ordered compaction of the matched build rows
    t, bufs, _ = i32_case(eng.join_build_bucket_chained)
    cnt = eng.join_probe_right(t, bufs[0], n_probe, 0)
    ob = eng.alloc(N_BUILD * 4)
    eng.join_probe_right(t, bufs[0], n_probe, 0, ob)
    count_s, c1 = best_of(lambda: eng.join_probe_right(t, bufs[0], n_probe, 0))
    emit_s, c2 = best_of(lambda: eng.join_probe_right(t, bufs[0], n_probe, 0, ob))
    assert c1 == cnt and c2 == cnt
    print(json.dumps({"case": "bc_right_semi", "build_rows": N_BUILD, "probe_rows": n_probe,
                      "pairs": int(cnt), "count_s": round(count_s, 5),
                      "emit_s": round(emit_s, 5)}), flush=True)
    t.destroy()
    for b in bufs + [ob]:
        b.free()
    eng.close()


if __name__ == "__main__":
    main()
