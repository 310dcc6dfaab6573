"""Window functions without a GPU: the numpy reference (starrocks_amd/
window.py) against a deliberately naive per-row Python loop, sort_perm_ref
against sorted(), WindowSpec's argument errors and hand-worked vectors."""

import functools

import numpy as np
import pytest

from starrocks_amd import window as W
from starrocks_amd.window import (COUNT, COUNT_STAR, DENSE_RANK, FIRST_VALUE, LAG, LAST_VALUE,
                                  LEAD, MAX, MIN, NTILE, PT_I32, PT_I64, RANGE, RANK,
                                  ROW_NUMBER, ROWS, SUM, UNBOUNDED, WinFunc, WindowSpec,
                                  sort_perm_ref, window_ref)

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DT = {PT_I32: np.int32, PT_I64: np.int64}
FRAMED = [COUNT_STAR, COUNT, SUM, MIN, MAX, FIRST_VALUE, LAST_VALUE]
FRAMES = [(ROWS, UNBOUNDED, 0), (ROWS, UNBOUNDED, UNBOUNDED), (RANGE, UNBOUNDED, 0),
          (RANGE, UNBOUNDED, UNBOUNDED), (ROWS, 0, 0), (ROWS, 1, 0), (ROWS, 0, 1), (ROWS, 3, 2),
          (ROWS, 400, 0), (ROWS, 0, 400), (ROWS, 10**9, 10**9), (ROWS, UNBOUNDED, 2),
          (ROWS, 2, UNBOUNDED)]


def wrap(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def naive(part_keys, order_keys, funcs, n, order_idx=None, sorted_out=False):
    """The semantics of gpue.h, one row and one frame at a time."""
    perm = list(range(n)) if order_idx is None else [int(x) for x in order_idx]

    def cell(keys, p):
        return tuple(None if nl is not None and nl[perm[p]] else int(DT[t](v[perm[p]]))
                     for v, nl, t in keys)

    part_start, peer_start = [0] * n, [0] * n
    for i in range(n):
        new_part = i == 0 or cell(part_keys, i) != cell(part_keys, i - 1)
        new_peer = new_part or cell(order_keys, i) != cell(order_keys, i - 1)
        part_start[i] = i if new_part else part_start[i - 1]
        peer_start[i] = i if new_peer else peer_start[i - 1]
    part_end, peer_end = [0] * n, [0] * n
    for i in reversed(range(n)):
        part_end[i] = i if i == n - 1 or part_start[i + 1] == i + 1 else part_end[i + 1]
        peer_end[i] = i if i == n - 1 or peer_start[i + 1] == i + 1 else peer_end[i + 1]
    spec = WindowSpec.of(part_keys, order_keys, funcs)
    results = []
    for f, nullable in zip(funcs, spec.out_nullable):
        def inp(p):
            r = perm[p]
            if f.nulls is not None and f.nulls[r]:
                return None
            return int(DT[f.type](f.col[r]))
        vals, nuls = [0] * n, [0] * n
        for i in range(n):
            ps, pe, qs, qe = part_start[i], part_end[i], peer_start[i], peer_end[i]
            if f.mode == ROWS:
                lo = ps if f.lo == UNBOUNDED else max(ps, i - f.lo)
                hi = pe if f.hi == UNBOUNDED else min(pe, i + f.hi)
            else:
                lo, hi = ps, (qe if f.hi == 0 else pe)
            frame = [inp(p) for p in range(lo, hi + 1)] if W.has_input(f.fn) and \
                W.is_framed(f.fn) else []
            seen = [x for x in frame if x is not None]
            if f.fn == ROW_NUMBER:
                v = i - ps + 1
            elif f.fn == RANK:
                v = qs - ps + 1
            elif f.fn == DENSE_RANK:
                v = len({peer_start[p] for p in range(ps, i + 1)})
            elif f.fn == NTILE:
                size, b, rn0 = pe - ps + 1, f.param0, i - ps
                q, r = size // b, size % b
                v = rn0 // (q + 1) + 1 if rn0 < r * (q + 1) else r + (rn0 - r * (q + 1)) // q + 1
            elif f.fn == COUNT_STAR:
                v = hi - lo + 1
            elif f.fn == COUNT:
                v = len(seen)
            elif f.fn == SUM:
                v = wrap(sum(seen)) if seen else None
            elif f.fn == MIN:
                v = min(seen) if seen else None
            elif f.fn == MAX:
                v = max(seen) if seen else None
            elif f.fn == FIRST_VALUE:
                v = frame[0]
            elif f.fn == LAST_VALUE:
                v = frame[-1]
            else:
                p = i - f.param0 if f.fn == LAG else i + f.param0
                if ps <= p <= pe:
                    v = inp(p)
                else:
                    v = f.param1 if f.has_default else None
            dst = i if sorted_out else perm[i]
            vals[dst], nuls[dst] = (0, 1) if v is None else (v, 0)
        assert nullable or not any(nuls)
        results.append((np.array(vals, np.int64).reshape(n),
                        np.array(nuls, np.uint8).reshape(n) if nullable else None))
    return results


def assert_same(got, want):
    assert len(got) == len(want)
    for (gv, gn), (wv, wn) in zip(got, want):
        assert gv.dtype == wv.dtype == np.int64
        np.testing.assert_array_equal(gv, wv)
        assert (gn is None) == (wn is None)
        if gn is not None:
            assert gn.dtype == np.uint8
            np.testing.assert_array_equal(gn, wn)


def table(rng, n, nullable_keys):
    """Pre-sorted partition / order keys with ties, and an input column with
    extremes next to NULLs."""
    part = np.sort(rng.integers(0, max(n // 9, 2), n)).astype(np.int64)
    order = np.zeros(n, np.int64)
    for p in np.unique(part):
        m = part == p
        order[m] = np.sort(rng.integers(0, 5, m.sum()))
    pk = [(part.astype(np.int32), None, PT_I32)]
    ok = [(order * (1 << 40), None, PT_I64)]
    if nullable_keys:      # partition 0 / order value 0 become NULL with garbage under them
        pnl, onl = (part == 0).astype(np.uint8) * 9, (order == 0).astype(np.uint8)
        pk = [(np.where(pnl != 0, rng.integers(-99, 99, n), part).astype(np.int32), pnl, PT_I32)]
        ok = [(np.where(onl != 0, rng.integers(-99, 99, n), order * (1 << 40)), onl, PT_I64)]
    return pk, ok


def inputs(rng, n, nullable, typ):
    if typ == PT_I32:
        v = rng.integers(-2**31, 2**31, n).astype(np.int32)
    else:
        v = rng.integers(-2**62, 2**62, n).astype(np.int64)
        v[rng.integers(0, n, n // 8)] = I64_MAX
        v[rng.integers(0, n, n // 8)] = I64_MIN
    if not nullable:
        return v, None
    nl = (rng.random(n) < 0.4).astype(np.uint8) * 3
    nl[: n // 5] = 1                                  # a NULL-only prefix
    return np.where(nl != 0, rng.integers(-7, 7, n).astype(v.dtype), v), nl


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("frame", FRAMES)
def test_framed_functions_match_naive_loop(frame, nullable):
    rng = np.random.default_rng(hash((frame, nullable)) & 0xFFFF)
    n = 257
    pk, ok = table(rng, n, nullable)
    mode, lo, hi = frame
    funcs = []
    for fn in FRAMED:
        if fn in (MIN, MAX) and lo != UNBOUNDED:
            continue
        v, nl = inputs(rng, n, nullable, PT_I32 if fn == COUNT else PT_I64)
        funcs.append(WinFunc(fn, v, nl, PT_I32 if fn == COUNT else PT_I64, mode=mode, lo=lo,
                             hi=hi))
    for sorted_out in (False, True):
        perm = rng.permutation(n).astype(np.uint32)
        inv = np.argsort(perm)

        def spread(c):         # rows scattered so that order_idx = perm restores the order
            return None if c is None else c[inv]
        spk = [(spread(v), spread(nl), t) for v, nl, t in pk]
        sok = [(spread(v), spread(nl), t) for v, nl, t in ok]
        sf = [f.with_cols(spread(f.col), spread(f.nulls)) for f in funcs]
        for chunk in (sf[:4], sf[4:]):
            assert_same(window_ref(spk, sok, chunk, n, perm, sorted_out),
                        naive(spk, sok, chunk, n, perm, sorted_out))
    assert_same(window_ref(pk, ok, funcs[:8], n), naive(pk, ok, funcs[:8], n))


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("n", [1, 2, 64, 300])
def test_ranking_and_offset_functions_match_naive_loop(n, nullable):
    rng = np.random.default_rng(n * 2 + nullable)
    pk, ok = table(rng, n, nullable)
    v, nl = inputs(rng, n, nullable, PT_I64)
    groups = [[WinFunc(ROW_NUMBER), WinFunc(RANK), WinFunc(DENSE_RANK)] +
              [WinFunc(NTILE, param0=b) for b in (1, 3, 7, 1000)]]
    for fn in (LAG, LEAD):
        groups.append([WinFunc(fn, v, nl, PT_I64, param0=k, param1=-5, has_default=d)
                       for k in (0, 1, 2, n) for d in (False, True)])
    for funcs in groups:
        assert_same(window_ref(pk, ok, funcs, n), naive(pk, ok, funcs, n))
        assert_same(window_ref([], ok, funcs, n), naive([], ok, funcs, n))
        assert_same(window_ref(pk, [], funcs, n), naive(pk, [], funcs, n))


def test_empty_input():
    out = window_ref([], [], [WinFunc(ROW_NUMBER), WinFunc(LAG, np.empty(0, np.int64))], 0)
    assert [(len(v), nl is None) for v, nl in out] == [(0, True), (0, False)]


@pytest.mark.parametrize("n", [0, 1, 200])
def test_sort_perm_ref_matches_sorted(n):
    rng = np.random.default_rng(n)
    p = rng.integers(-2, 2, n).astype(np.int32)
    pn = (rng.random(n) < 0.3).astype(np.uint8)
    a = rng.integers(-2, 3, n).astype(np.int64)
    a[rng.integers(0, max(n, 1), n // 10)] = I64_MIN
    an = (rng.random(n) < 0.3).astype(np.uint8) * 2
    b = rng.integers(0, 3, n).astype(np.int32)
    p = np.where(pn != 0, rng.integers(-50, 50, n), p).astype(np.int32)   # garbage under NULL
    a = np.where(an != 0, rng.integers(-50, 50, n), a)
    for flags in ([(False, True), (False, False)], [(True, False), (True, True)],
                  [(True, True), (False, False)]):
        def cmp_key(x, xn, y, yn, desc, nulls_first):
            if xn or yn:
                if xn and yn:
                    return 0
                return (-1 if xn else 1) * (1 if nulls_first else -1)
            c = (x > y) - (x < y)
            return -c if desc else c

        def cmp(i, j):
            for v, nl, (desc, nf) in ((p, pn, (False, True)), (a, an, flags[0]),
                                      (b, None, flags[1])):
                c = cmp_key(int(v[i]), nl is not None and nl[i], int(v[j]),
                            nl is not None and nl[j], desc, nf)
                if c:
                    return c
            return 0
        want = sorted(range(n), key=functools.cmp_to_key(cmp))     # sorted() is stable
        got = sort_perm_ref([(p, pn, PT_I32)], [(a, an, PT_I64), (b, None, PT_I32)], flags, n)
        assert got.dtype == np.uint32
        assert got.tolist() == want


class Buf:
    def __init__(self, nbytes):
        self.nbytes = nbytes


def test_spec_rejects_argument_errors():
    ok = lambda **kw: WinFunc(SUM, **kw)
    spec = lambda funcs, pt=(PT_I32,), ot=(PT_I64,): WindowSpec(
        pt, [False] * len(pt), ot, [False] * len(ot), funcs)
    spec([ok()])
    bad_specs = [
        lambda: spec([ok()], pt=(PT_I32,) * 5),                       # counts out of range
        lambda: spec([ok()], ot=(PT_I64,) * 5),
        lambda: spec([]),
        lambda: spec([ok()] * 9),
        lambda: spec([ok()], pt=(2,)),                                # unknown types
        lambda: spec([ok()], ot=(-1,)),
        lambda: spec([ok(type=7)]),
        lambda: spec([WinFunc(13)]),                                  # unknown fn
        lambda: spec([WinFunc(-1)]),
        lambda: spec([WinFunc("median")]),
        lambda: spec([ok(mode=2)]),                                   # unknown mode
        lambda: spec([ok(mode=ROWS, lo=-2, hi=0)]),                   # illegal frames
        lambda: spec([ok(mode=ROWS, lo=0, hi=-2)]),
        lambda: spec([ok(mode=RANGE, lo=0, hi=0)]),
        lambda: spec([ok(mode=RANGE, lo=UNBOUNDED, hi=1)]),
        lambda: spec([WinFunc(MIN, mode=ROWS, lo=1, hi=0)]),          # sliding minimum
        lambda: spec([WinFunc(MAX, mode=ROWS, lo=0, hi=UNBOUNDED)]),
        lambda: spec([WinFunc(NTILE, param0=0)]),
        lambda: spec([WinFunc(LAG, param0=-1)]),
        lambda: spec([WinFunc(LEAD, param0=-1)]),
    ]
    for make in bad_specs:
        with pytest.raises(ValueError):
            make()
    # frame fields are ignored outside the framed functions
    spec([WinFunc(ROW_NUMBER, mode=9, lo=-7, hi=-7), WinFunc(LAG, mode=9, lo=-7)])

    n = 10
    s = WindowSpec([PT_I32], [True], [PT_I64], [False],
                   [WinFunc(SUM, nullable=True), WinFunc(ROW_NUMBER), WinFunc(COUNT, type=PT_I32)])
    pk, ok_, idx = [(Buf(40), Buf(10))], [(Buf(80), None)], Buf(40)
    ins = [(Buf(80), Buf(10)), (None, None), (Buf(40), None)]
    outs = [(Buf(80), Buf(10)), (Buf(80), None), (Buf(80), None)]
    s.check_eval(n, idx, pk, ok_, ins, outs)
    s.check_eval(n, None, pk, ok_, ins, outs, W.OUT_SORTED)

    def swap(lst, i, item):
        return lst[:i] + [item] + lst[i + 1:]
    bad_calls = [
        dict(flags=2), dict(n_rows=1 << 32),
        dict(order_idx=Buf(39)),                                      # short buffers
        dict(part_keys=[(Buf(39), None)]), dict(part_keys=[(Buf(40), Buf(9))]),
        dict(order_keys=[(Buf(79), None)]),
        dict(ins=swap(ins, 0, (Buf(79), None))), dict(ins=swap(ins, 0, (Buf(80), Buf(9)))),
        dict(ins=swap(ins, 2, (Buf(39), None))),
        dict(outs=swap(outs, 1, (Buf(79), None))), dict(outs=swap(outs, 0, (Buf(80), Buf(9)))),
        dict(ins=swap(ins, 0, (None, None))),                         # missing input
        dict(part_keys=[(None, None)]),
        dict(outs=swap(outs, 1, (None, None))),                       # missing output
        dict(outs=swap(outs, 0, (Buf(80), None))),                    # missing null output
        dict(order_keys=[(Buf(80), Buf(10))]),                        # nulls for NOT NULL
        dict(ins=swap(ins, 2, (Buf(40), Buf(10)))),
        dict(outs=swap(outs, 1, outs[0])),                            # output twice
        dict(outs=swap(outs, 1, (outs[0][1], None))),
        dict(outs=swap(outs, 1, (ins[0][0], None))),                  # output over an input
        dict(outs=swap(outs, 1, (idx, None))),
    ]
    for kw in bad_calls:
        args = dict(n_rows=n, order_idx=idx, part_keys=pk, order_keys=ok_, ins=ins, outs=outs,
                    flags=0)
        args.update(kw)
        with pytest.raises(ValueError):
            s.check_eval(**args)


def test_spec_states_output_nullability():
    fns = [ROW_NUMBER, RANK, DENSE_RANK, NTILE, COUNT_STAR, COUNT, SUM, MIN, MAX, FIRST_VALUE,
           LAST_VALUE]
    for nullable in (False, True):
        for lo in range(0, len(fns), 8):
            s = WindowSpec([], [], [], [], [WinFunc(fn, nullable=nullable, param0=1)
                                            for fn in fns[lo:lo + 8]])
            assert s.out_nullable == [nullable and fn >= SUM for fn in fns[lo:lo + 8]]
    s = WindowSpec([], [], [], [], [WinFunc(fn, nullable=nl, has_default=d)
                                    for fn in (LAG, LEAD) for nl in (False, True)
                                    for d in (False, True)])
    assert s.out_nullable == [True, False, True, True] * 2


def test_hand_worked_ties():
    # one partition of 7 rows, order key with ties: 10 10 20 30 30 30 40
    order = np.array([10, 10, 20, 30, 30, 30, 40], np.int32)
    x = np.array([1, 2, 3, 4, 5, 6, 7], np.int64)
    funcs = [WinFunc(RANK), WinFunc(DENSE_RANK), WinFunc(NTILE, param0=3),
             WinFunc(SUM, x),                                # RANGE ..current: peers included
             WinFunc(SUM, x, mode=ROWS, lo=UNBOUNDED, hi=0), WinFunc(ROW_NUMBER)]
    out = window_ref([], [(order, None, PT_I32)], funcs, 7)
    want = [[1, 1, 3, 4, 4, 4, 7], [1, 1, 2, 3, 3, 3, 4], [1, 1, 1, 2, 2, 3, 3],
            [3, 3, 6, 21, 21, 21, 28], [1, 3, 6, 10, 15, 21, 28], [1, 2, 3, 4, 5, 6, 7]]
    for (v, nl), w in zip(out, want):
        assert nl is None
        assert v.tolist() == w


def test_hand_worked_lag_lead_at_partition_edges():
    part = np.array([1, 1, 1, 2, 2, 3], np.int32)
    x = np.array([10, 20, 30, 40, 50, 60], np.int64)
    xn = np.array([0, 1, 0, 0, 0, 0], np.uint8)
    funcs = [WinFunc(LAG, x, param0=1), WinFunc(LAG, x, param0=1, param1=-1, has_default=True),
             WinFunc(LEAD, x, param0=2), WinFunc(LEAD, x, param0=1, param1=99, has_default=True),
             WinFunc(LAG, x, xn, param0=1, param1=-1, has_default=True)]
    out = window_ref([(part, None, PT_I32)], [], funcs, 6)
    assert out[0][0].tolist() == [0, 10, 20, 0, 40, 0]
    assert out[0][1].tolist() == [1, 0, 0, 1, 0, 1]
    assert out[1][0].tolist() == [-1, 10, 20, -1, 40, -1] and out[1][1] is None
    assert out[2][0].tolist() == [30, 0, 0, 0, 0, 0]
    assert out[2][1].tolist() == [0, 1, 1, 1, 1, 1]
    assert out[3][0].tolist() == [20, 30, 99, 50, 99, 99] and out[3][1] is None
    assert out[4][0].tolist() == [-1, 10, 0, -1, 40, -1]     # the NULL input passes through
    assert out[4][1].tolist() == [0, 0, 1, 0, 0, 0]


class HostBuf:
    """Device-buffer stand-in: bytes on the host."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.a = np.zeros(nbytes, np.uint8)
        self.freed = False

    def h2d(self, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.a[:raw.size] = raw
        return self

    def d2h(self, dtype, count):
        return self.a[:count * np.dtype(dtype).itemsize].view(dtype).copy()

    def free(self):
        assert not self.freed
        self.freed = True


class HostEngine:
    """The four calls WindowSinkOperator uses, over numpy."""

    def __init__(self):
        self.bufs = []

    def alloc(self, nbytes):
        self.bufs.append(HostBuf(nbytes))
        return self.bufs[-1]

    def dbuf_d2d(self, src, dst, nbytes, src_off=0, dst_off=0):
        dst.a[dst_off:dst_off + nbytes] = src.a[src_off:src_off + nbytes]

    def window(self, part_keys, order_keys, funcs, n):
        col = lambda b, t: b.d2h(DT[t], n)
        nul = lambda b: None if b is None else b.d2h(np.uint8, n)
        pk = [(col(v, t), nul(nl), t) for v, nl, t in part_keys]
        ok = [(col(v, t), nul(nl), t) for v, nl, t, _, _ in order_keys]
        hf = [f.with_cols(None if f.col is None else col(f.col, f.type), nul(f.nulls))
              for f in funcs]
        perm = sort_perm_ref(pk, ok, [k[3:] for k in order_keys], n)
        outs = []
        for v, nl in window_ref(pk, ok, hf, n, perm):
            outs.append((self.alloc(max(v.nbytes, 1)).h2d(v),
                         None if nl is None else self.alloc(max(n, 1)).h2d(nl)))
        return outs


@pytest.mark.parametrize("chunks", [[], [0], [1, 200, 0, 64, 3, 35]])
def test_window_sink_operator_on_a_host_engine(chunks):
    from starrocks_amd.pipeline import WindowSinkOperator
    n = sum(chunks)
    rng = np.random.default_rng(n)
    p = rng.integers(0, 9, n).astype(np.int32)
    pn = (rng.random(n) < 0.2).astype(np.uint8)
    o = rng.integers(-5, 5, n).astype(np.int64)
    v, nl = inputs(rng, n, True, PT_I64) if n else (np.empty(0, np.int64), np.empty(0, np.uint8))
    cols = [p, pn, o, v, nl]
    funcs = [WinFunc(ROW_NUMBER), WinFunc(SUM, 3, 4), WinFunc(LEAD, 3, 4, param0=1),
             WinFunc(MIN, 3, 4, mode=ROWS, lo=UNBOUNDED, hi=0)]
    eng = HostEngine()
    op = WindowSinkOperator(eng, [c.dtype for c in cols], [(0, 1, PT_I32)],
                            [(2, None, PT_I64, True, False)], funcs)
    at = 0
    for size in chunks:
        op.push_chunk({"n": size, "cols": [eng.alloc(max(c[at:at + size].nbytes, 1)).h2d(
            c[at:at + size]) for c in cols]})
        at += size
    op.set_finishing()
    assert op.is_finished() and op.rows == n
    got_cols, got = op.result()
    assert all(b.freed for b in eng.bufs)             # chunks, columns and outputs: all released
    for g, c in zip(got_cols, cols):
        np.testing.assert_array_equal(g, c)
    hf = [f.with_cols(None if f.col is None else cols[f.col],
                      None if f.nulls is None else cols[f.nulls]) for f in funcs]
    perm = sort_perm_ref([(p, pn, PT_I32)], [(o, None, PT_I64)], [(True, False)], n)
    assert_same(got, window_ref([(p, pn, PT_I32)], [(o, None, PT_I64)], hf, n, perm))


def test_tile_constants_match_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gpue.h")).read()
    assert int(re.search(r"#define GPUE_WIN_TILE (\d+)", hdr).group(1)) == W.T
    assert int(re.search(r"#define GPUE_WIN_MID (\d+)", hdr).group(1)) == W.A
    for name in W.FN_NAMES:
        m = re.search(rf"#define GPUE_WFN_{name.upper()} (\d+)", hdr)
        assert int(m.group(1)) == W.FN_NAMES[name]
