"""starrocks_amd/hashjoin.py without a GPU: the dict reference against a
nested-loop join written here, the validation errors the C side also raises,
the output rules and gather_outer_ref."""

import numpy as np
import pytest

from starrocks_amd import hashjoin as hj
from starrocks_amd.hashjoin import (INNER, LEFT_ANTI, LEFT_OUTER, LEFT_SEMI, MARK_ONLY, NO_ROW,
                                    NULL_AWARE_LEFT_ANTI, PT_I32, PT_I64, HashJoinSpec)

MODES = (INNER, LEFT_SEMI, LEFT_ANTI, LEFT_OUTER, NULL_AWARE_LEFT_ANTI, MARK_ONLY)
NULL_CFGS = ("none", "plain", "null_safe", "mixed")


def _side(rng, n, n_keys, with_nulls, types, lo=-2, hi=3):
    cols = []
    for k in range(n_keys):
        dt = np.int64 if types[k] == PT_I64 else np.int32
        v = rng.integers(lo, hi, n).astype(dt)
        nl = (rng.random(n) < 0.25).astype(np.uint8) if with_nulls else None
        if nl is not None:  # garbage under NULL cells must not matter
            v = np.where(nl != 0, rng.integers(-1000, 1000, n), v).astype(dt)
        cols.append((v, nl, types[k]))
    return cols


def _null_safe(cfg, n_keys):
    return {"none": [False] * n_keys, "plain": [False] * n_keys,
            "null_safe": [True] * n_keys,
            "mixed": [k % 2 == 0 for k in range(n_keys)]}[cfg]


def _cell_eq(b, j, p, i, ns):
    bn = b[1] is not None and b[1][j] != 0
    pn = p[1] is not None and p[1][i] != 0
    if bn or pn:
        return ns and bn and pn
    return int(b[0][j]) == int(p[0][i])


def nested_loop(build, probe, null_safe, mode):
    """(sorted pair array, matched build rows) by comparing every pair."""
    nb, npr = len(build[0][0]), len(probe[0][0])
    matched = np.zeros(nb, bool)
    pi, bi = [], []
    b_null = [any(c[1] is not None and c[1][j] for c in build) for j in range(nb)]
    for i in range(npr):
        rows = [j for j in range(nb)
                if all(_cell_eq(b, j, p, i, ns) for b, p, ns in zip(build, probe, null_safe))]
        matched[rows] = True
        p_null = any(c[1] is not None and c[1][i] for c in probe)
        if mode in (INNER, LEFT_SEMI):
            out = rows
        elif mode == LEFT_OUTER:
            out = rows or [NO_ROW]
        elif mode == LEFT_ANTI:
            out = [] if rows else [NO_ROW]
        elif mode == NULL_AWARE_LEFT_ANTI:
            keep = nb == 0 or (not any(b_null) and not p_null and not rows)
            out = [NO_ROW] if keep else []
        else:
            out = []
        pi += [i] * len(out)
        bi += out
    return hj.sort_pairs(pi, bi), matched


@pytest.mark.parametrize("cfg", NULL_CFGS)
@pytest.mark.parametrize("n_keys", (1, 2, 4))
@pytest.mark.parametrize("mode", MODES)
def test_ref_against_nested_loop(mode, n_keys, cfg):
    ns = _null_safe(cfg, n_keys)
    if mode == NULL_AWARE_LEFT_ANTI and (n_keys != 1 or ns[0]):
        with pytest.raises(ValueError, match="NULL_AWARE_LEFT_ANTI"):
            HashJoinSpec([PT_I32] * n_keys, [PT_I32] * n_keys, [True] * n_keys,
                         ns).check_probe([(np.zeros(1, np.int32), None)] * n_keys, 1, mode)
        return
    rng = np.random.default_rng(1000 * mode + 10 * n_keys + NULL_CFGS.index(cfg))
    types = [PT_I32, PT_I64, PT_I32, PT_I64][:n_keys]
    # 6 values per key: 1 key -> long chains, 4 keys -> 1296 tuples, so more rows
    nb, npr = (40, 60) if n_keys < 4 else (700, 500)
    build = _side(rng, nb, n_keys, cfg != "none", types, -2, 4)  # 3 has no probe row
    probe = _side(rng, npr, n_keys, cfg != "none", types, -3, 3)
    want_pairs, want_matched = nested_loop(build, probe, ns, mode)
    pairs, matched = hj.hash_join_ref(build, probe, ns, mode)
    assert matched.any() and not matched.all(), "vacuous case"
    assert np.array_equal(pairs, want_pairs)
    assert np.array_equal(matched, want_matched)
    if mode == MARK_ONLY:
        assert len(pairs) == 0


def test_mixed_widths_and_negative_values():
    """An int32 side joins an int64 side by sign extension: -1 meets -1, and
    0xFFFFFFFF as an int64 meets nothing."""
    b = [(np.array([-1, 0xFFFFFFFF, -(1 << 63), 7], np.int64), None, PT_I64)]
    p = [(np.array([-1, 7, -(1 << 31)], np.int32), None, PT_I32)]
    pairs, matched = hj.hash_join_ref(b, p, None, INNER)
    assert pairs.tolist() == [[0, 0], [1, 3]]
    assert matched.tolist() == [True, False, False, True]
    pairs, _ = hj.hash_join_ref(p, b, None, "inner")  # and the reverse
    assert pairs.tolist() == [[0, 0], [3, 1]]


def test_null_aware_left_anti_three_cases():
    p = [(np.array([1, 2, 0], np.int32), np.array([0, 0, 1], np.uint8), PT_I32)]
    empty = [(np.empty(0, np.int32), None, PT_I32)]
    pairs, _ = hj.hash_join_ref(empty, p, None, NULL_AWARE_LEFT_ANTI)
    assert pairs.tolist() == [[0, NO_ROW], [1, NO_ROW], [2, NO_ROW]]
    with_null = [(np.array([1, 5], np.int32), np.array([0, 1], np.uint8), PT_I32)]
    pairs, _ = hj.hash_join_ref(with_null, p, None, NULL_AWARE_LEFT_ANTI)
    assert len(pairs) == 0
    plain = [(np.array([1, 5], np.int32), None, PT_I32)]
    pairs, _ = hj.hash_join_ref(plain, p, None, NULL_AWARE_LEFT_ANTI)
    assert pairs.tolist() == [[1, NO_ROW]]
    # plain LEFT_ANTI keeps the NULL row
    pairs, _ = hj.hash_join_ref(plain, p, None, LEFT_ANTI)
    assert pairs.tolist() == [[1, NO_ROW], [2, NO_ROW]]


@pytest.mark.parametrize("how", sorted(hj.HOWS))
def test_how_ref_and_output_rules(how):
    rng = np.random.default_rng(7)
    build = _side(rng, 30, 2, True, [PT_I32, PT_I64])
    probe = _side(rng, 50, 2, True, [PT_I64, PT_I32])
    ns = None if how == "null_aware_left_anti" else [False, True]
    if how == "null_aware_left_anti":
        build, probe = build[:1], probe[:1]
    mode, flags, tail = hj.plan(how)
    want, matched = nested_loop(build, probe, ns or [False], mode)
    if tail is not None:
        rows = np.nonzero(matched if tail else ~matched)[0]
        want = hj.sort_pairs(list(want[:, 0]) + [NO_ROW] * len(rows),
                             list(want[:, 1]) + list(rows))
    got = hj.hash_join_how_ref(build, probe, how, ns)
    assert np.array_equal(got, want)
    has_p, p_nullable, has_b, b_nullable = hj.output_sides(how)
    if len(got):
        # an index column holds NO_ROW only where its side is nullable or absent
        assert (p_nullable or not has_p) or not np.any(got[:, 0] == NO_ROW)
        assert (b_nullable or not has_b) or not np.any(got[:, 1] == NO_ROW)
        if not has_p:
            assert np.all(got[:, 0] == NO_ROW)
    assert has_p or has_b
    assert flags == (hj.MARK_BUILD if tail is not None else 0)


class _B:
    def __init__(self, nbytes):
        self.nbytes = nbytes


def test_spec_validation_errors():
    with pytest.raises(ValueError, match="n_keys 0"):
        HashJoinSpec([], [], [])
    with pytest.raises(ValueError, match="n_keys 5"):
        HashJoinSpec([0] * 5, [0] * 5, [0] * 5)
    with pytest.raises(ValueError, match="differ in length"):
        HashJoinSpec([0, 1], [0], [0, 0])
    with pytest.raises(ValueError, match="unknown key type"):
        HashJoinSpec([2], [0], [0])
    with pytest.raises(ValueError, match="unknown key type"):
        HashJoinSpec([0], [True], [0])
    with pytest.raises(ValueError, match="unknown join type"):
        hj.plan("cross")
    with pytest.raises(ValueError, match="key count"):
        HashJoinSpec.of([(_B(4), None, 0)], [(_B(4), None, 0)] * 2)
    spec = HashJoinSpec([PT_I32, PT_I64], [PT_I64, PT_I32], [False, True], [False, True])
    ok = [(_B(40), None), (_B(80), _B(10))]
    spec.check_push(ok, 10)
    spec.check_probe([(_B(80), None), (_B(40), _B(10))], 10, INNER)
    with pytest.raises(ValueError, match="below 2\\^32"):
        spec.check_push(ok, 1 << 32)
    with pytest.raises(ValueError, match="2\\^32-1"):
        spec.check_push(ok, 10, rows_so_far=NO_ROW - 10)
    with pytest.raises(ValueError, match="does not match"):
        spec.check_push(ok[:1], 10)
    with pytest.raises(ValueError, match="key column 1 is missing"):
        spec.check_push([ok[0], (None, None)], 10)
    with pytest.raises(ValueError, match="key column 1 is shorter"):
        spec.check_push([ok[0], (_B(79), None)], 10)
    with pytest.raises(ValueError, match="key column 0 is shorter"):  # probe widths differ
        spec.check_probe(ok, 10, INNER)
    with pytest.raises(ValueError, match="declared NOT NULL"):
        spec.check_push([(_B(40), _B(10)), ok[1]], 10)
    with pytest.raises(ValueError, match="null column of key 1 is shorter"):
        spec.check_push([ok[0], (_B(80), _B(9))], 10)
    pk = [(_B(80), None), (_B(40), None)]
    for bad in (-1, 6, True):
        with pytest.raises(ValueError, match="unknown probe mode"):
            spec.check_probe(pk, 10, bad)
    with pytest.raises(ValueError, match="unknown probe flags"):
        spec.check_probe(pk, 10, INNER, 2)
    with pytest.raises(ValueError, match="NULL_AWARE_LEFT_ANTI"):
        spec.check_probe(pk, 10, NULL_AWARE_LEFT_ANTI)
    with pytest.raises(ValueError, match="NULL_AWARE_LEFT_ANTI"):
        HashJoinSpec([0], [0], [1], [1]).check_probe([(_B(40), None)], 10, NULL_AWARE_LEFT_ANTI)
    out = _B(400)
    with pytest.raises(ValueError, match="both index outputs"):
        spec.check_probe(pk, 10, INNER, 0, out, None)
    with pytest.raises(ValueError, match="overlaps"):
        spec.check_probe(pk, 10, INNER, 0, out, out)
    with pytest.raises(ValueError, match="overlaps"):
        spec.check_probe(pk, 10, INNER, 0, pk[0][0], out)
    with pytest.raises(ValueError, match="matched must be"):
        hj.check_emit_build(2, None, 0)
    with pytest.raises(ValueError, match="max_out"):
        hj.check_emit_build(1, None, 1 << 32)
    with pytest.raises(ValueError, match="shorter than max_out"):
        hj.check_emit_build(1, _B(39), 10)


def test_gather_outer_validation_errors():
    a = dict(inp=_B(80), in_nulls=None, in_rows=10, width=8, idx=_B(20), n=5, out=_B(40),
             out_nulls=_B(5))
    hj.check_gather_outer(**a)
    for change, msg in ((dict(width=2), "width"), (dict(n=1 << 32), "below 2"),
                        (dict(inp=None), "required"), (dict(inp=_B(79)), "in is shorter"),
                        (dict(in_nulls=_B(9)), "in_nulls is shorter"),
                        (dict(in_nulls=_B(10), out_nulls=None), "needs out_nulls"),
                        (dict(idx=_B(19)), "shorter than n"), (dict(out=_B(39)), "shorter than n"),
                        (dict(out_nulls=_B(4)), "out_nulls is shorter"),
                        (dict(out=a["inp"]), "overlaps")):
        with pytest.raises(ValueError, match=msg):
            hj.check_gather_outer(**{**a, **change})


def test_gather_outer_ref():
    vals = np.array([10, -20, 30], np.int64)
    nulls = np.array([0, 1, 0], np.uint8)
    idx = np.array([2, NO_ROW, 1, 0], np.uint32)
    out, nl = hj.gather_outer_ref(vals, nulls, idx)
    assert out.tolist() == [30, 0, -20, 10] and out.dtype == np.int64
    assert nl.tolist() == [0, 1, 1, 0]
    out, nl = hj.gather_outer_ref(vals.astype(np.uint8), None, idx)
    assert out.dtype == np.uint8 and nl.tolist() == [0, 1, 0, 0]
    out, nl = hj.gather_outer_ref(vals, None, idx[[0, 2]], with_nulls=False)
    assert out.tolist() == [30, -20] and nl is None
    with pytest.raises(ValueError, match=">= in_rows"):
        hj.gather_outer_ref(vals, None, np.array([3], np.uint32))
    with pytest.raises(ValueError, match="NO_ROW"):
        hj.gather_outer_ref(vals, None, idx, with_nulls=False)
    with pytest.raises(ValueError, match="needs out_nulls"):
        hj.gather_outer_ref(vals, nulls, idx[:1], with_nulls=False)
    out, nl = hj.gather_outer_ref(np.empty(0, np.int32), None, np.array([NO_ROW], np.uint32))
    assert out.tolist() == [0] and nl.tolist() == [1]


# ---- the pipeline operators and Engine.hash_join over a numpy stand-in engine ----

from starrocks_amd.engine import Engine  # noqa: E402  (no library is loaded by the import)
from starrocks_amd.pipeline import (GeneralHashJoinBuildOperator,  # noqa: E402
                                    GeneralHashJoinProbeOperator)

DT = {PT_I32: np.int32, PT_I64: np.int64}


class NpBuf:
    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.mem = np.zeros(nbytes, np.uint8)
        self.freed = False

    def h2d(self, arr, dst_off=0):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert dst_off + raw.size <= self.nbytes
        self.mem[dst_off:dst_off + raw.size] = raw
        return self

    def d2h(self, dtype, count, src_off=0):
        assert not self.freed
        return self.mem[src_off:src_off + count * np.dtype(dtype).itemsize].view(dtype).copy()

    def free(self):
        self.freed = True

    def __bool__(self):
        return True


class NpJoinEngine:
    """Just what the two join operators and Engine.hash_join may call. The
    table is the list of pushed key columns plus a mark array; a probe runs
    the reference over it."""
    HJ_MARK_ONLY, HJ_NO_ROW = MARK_ONLY, NO_ROW
    hash_join = Engine.hash_join
    hash_join_probe_alloc = Engine.hash_join_probe_alloc

    def __init__(self):
        self.bufs = []
        self.destroyed = 0

    def alloc(self, nbytes):
        assert nbytes > 0
        self.bufs.append(NpBuf(nbytes))
        return self.bufs[-1]

    def dbuf_d2d(self, src, dst, nbytes, src_off=0, dst_off=0):
        dst.h2d(src.mem[src_off:src_off + nbytes], dst_off)

    def hash_join_create(self, build_types, probe_types, key_nullable, key_null_safe=None,
                         capacity_hint=0):
        spec = HashJoinSpec(build_types, probe_types, key_nullable, key_null_safe)
        return {"spec": spec, "rows": 0, "marks": np.zeros(0, bool),
                "keys": [[np.empty(0, DT[t]), np.empty(0, np.uint8)] for t in spec.build_types]}

    def hash_join_build_push(self, t, keys, n_rows):
        spec = t["spec"]
        spec.check_push(keys, n_rows, t["rows"])
        for k, (v, nl) in enumerate(keys):
            t["keys"][k][0] = np.concatenate([t["keys"][k][0], v.d2h(DT[spec.build_types[k]], n_rows)])
            t["keys"][k][1] = np.concatenate(
                [t["keys"][k][1], np.zeros(n_rows, np.uint8) if nl is None else nl.d2h(np.uint8, n_rows)])
        t["rows"] += n_rows
        t["marks"] = np.concatenate([t["marks"], np.zeros(n_rows, bool)])

    def hash_join_build_rows(self, t):
        return t["rows"]

    def hash_join_probe(self, t, keys, n_rows, mode, flags=0, out_probe=None, out_build=None):
        spec = t["spec"]
        spec.check_probe(keys, n_rows, mode, flags, out_probe, out_build)
        build = [(v, nl if spec.key_nullable[k] else None, spec.build_types[k])
                 for k, (v, nl) in enumerate(t["keys"])]
        probe = [(v.d2h(DT[spec.probe_types[k]], n_rows),
                  None if nl is None else nl.d2h(np.uint8, n_rows), spec.probe_types[k])
                 for k, (v, nl) in enumerate(keys)]
        for k in range(spec.n_keys):  # declare nullability as the table does
            if spec.key_nullable[k] and probe[k][1] is None:
                probe[k] = (probe[k][0], np.zeros(n_rows, np.uint8), probe[k][2])
        pairs, matched = hj.hash_join_ref(build, probe, spec.key_null_safe, mode, t["rows"],
                                          n_rows)
        if flags or mode == MARK_ONLY:
            t["marks"] |= matched
        if mode == LEFT_SEMI and len(pairs):  # one match per row: the largest
            last = np.r_[pairs[1:, 0] != pairs[:-1, 0], True]
            pairs = pairs[last]
        if out_probe is not None and mode != MARK_ONLY and len(pairs):
            if out_probe.nbytes < len(pairs) * 4 or out_build.nbytes < len(pairs) * 4:
                raise ValueError("output shorter than the pair count")
            out_probe.h2d(pairs[:, 0].astype(np.uint32))
            out_build.h2d(pairs[:, 1].astype(np.uint32))
        return len(pairs)

    def hash_join_emit_build(self, t, matched, out=None, max_out=0):
        hj.check_emit_build(matched, out, max_out)
        rows = np.nonzero(t["marks"] if matched else ~t["marks"])[0].astype(np.uint32)
        if out is not None and len(rows):
            if len(rows) > max_out:
                raise ValueError("more rows than max_out")
            out.h2d(rows)
        return len(rows)

    def hash_join_reset_marks(self, t):
        t["marks"][:] = False

    def hash_join_destroy(self, t):
        self.destroyed += 1

    def _gather(self, dtype, inp, idx, n, out):
        out.h2d(inp.mem.view(dtype)[idx.d2h(np.uint32, n)])

    def gather_u8(self, inp, idx, n, out):
        self._gather(np.uint8, inp, idx, n, out)

    def gather_u32(self, inp, idx, n, out):
        self._gather(np.uint32, inp, idx, n, out)

    def gather_u64(self, inp, idx, n, out):
        self._gather(np.uint64, inp, idx, n, out)

    def gather_outer(self, inp, in_nulls, in_rows, width, idx, n, out, out_nulls=None):
        hj.check_gather_outer(inp, in_nulls, in_rows, width, idx, n, out, out_nulls)
        dt = {1: np.uint8, 4: np.uint32, 8: np.uint64}[width]
        v, nl = hj.gather_outer_ref(inp.d2h(dt, in_rows),
                                    None if in_nulls is None else in_nulls.d2h(np.uint8, in_rows),
                                    idx.d2h(np.uint32, n), out_nulls is not None)
        out.h2d(v)
        if out_nulls is not None:
            out_nulls.h2d(nl)


def _join_case(seed, n_build, n_probe):
    rng = np.random.default_rng(seed)
    build = _side(rng, n_build, 2, True, [PT_I32, PT_I64], -2, 6)
    probe = _side(rng, n_probe, 2, True, [PT_I64, PT_I32], -4, 4)
    build[0] = (build[0][0], None, PT_I32)  # key 0 NOT NULL on both sides
    probe[0] = (probe[0][0], None, PT_I64)
    return build, probe, rng.integers(-99, 99, n_build).astype(np.int64), \
        rng.integers(0, 99, n_probe).astype(np.int32)


@pytest.mark.parametrize("how", sorted(set(hj.HOWS) - {"null_aware_left_anti"}))
def test_engine_one_shot_form(how):
    """Engine.hash_join's composition — count, emit, and the RIGHT / FULL tail
    appended as (NO_ROW, b) rows — over the stand-in entries."""
    build, probe, _, _ = _join_case(3, 120, 90)
    eng = NpJoinEngine()
    put = lambda a: None if a is None else eng.alloc(max(a.nbytes, 1)).h2d(a)
    cols = lambda keys: [(put(v), put(nl), t, len(v)) for v, nl, t in keys]
    op, ob, n = eng.hash_join(cols(build), cols(probe), how, [False, True])
    inputs = list(eng.bufs[:6])
    want = hj.hash_join_how_ref(build, probe, how, [False, True])
    got = hj.sort_pairs(op.d2h(np.uint32, n), ob.d2h(np.uint32, n))
    if how == "left_semi":
        assert np.array_equal(got[:, 0], np.unique(want[:, 0]))
        assert set(map(tuple, got.tolist())) <= set(map(tuple, want.tolist()))
    else:
        assert np.array_equal(got, want)
    assert eng.destroyed == 1
    kept = inputs + [op, ob]  # everything else the call allocated is freed
    assert all(b.freed for b in eng.bufs if not any(b is k for k in kept))


@pytest.mark.parametrize("how", sorted(set(hj.HOWS) - {"null_aware_left_anti"}))
def test_pipeline_operators(how):
    """Both operators over chunked sides, an empty chunk included: the joined
    chunks hold the reference's pairs with each side's payload, NULL where
    the pair has NO_ROW."""
    n_build, n_probe = 700, 500
    build, probe, bpay, ppay = _join_case(4, n_build, n_probe)
    eng = NpJoinEngine()
    put = lambda a: eng.alloc(max(a.nbytes, 1)).h2d(a)
    bcols = [build[0][0], build[1][0], build[1][1], bpay]
    pcols = [probe[0][0], probe[1][0], probe[1][1], ppay]
    chunks = lambda cols, cuts: [{"n": hi - lo, "cols": [put(c[lo:hi]) for c in cols]}
                                 for lo, hi in zip(cuts, cuts[1:])]
    bop = GeneralHashJoinBuildOperator(eng, [(0, None, PT_I32), (1, 2, PT_I64)],
                                       [np.int32, np.int64, np.uint8, np.int64],
                                       probe_types=[PT_I64, PT_I32], null_safe=[False, True])
    for c in chunks(bcols, [0, 130, 130, 700]):
        assert bop.need_input() and not bop.has_output()
        bop.push_chunk(c)
    bop.set_finishing()
    assert bop.is_finished() and bop.rows == n_build
    pop = GeneralHashJoinProbeOperator(eng, bop, how, [(0, None, PT_I64), (1, 2, PT_I32)],
                                       [np.int64, np.int32, np.uint8, np.int32],
                                       probe_payload=[(3, None), (1, 2)],
                                       build_payload=[(3, None), (1, 2)])
    has_p, p_nullable, has_b, b_nullable = hj.output_sides(how)
    out = []
    for c in chunks(pcols, [0, 200, 200, 201, 500]):
        assert pop.need_input()
        pop.push_chunk(c)
        while pop.has_output():
            out.append(pop.pull_chunk())
    pop.set_finishing()
    while pop.has_output():
        out.append(pop.pull_chunk())
    assert pop.is_finished()
    if hj.plan(how)[2] is not None:
        assert len(out) >= 1 and all(len(c["cols"]) == len(pop.out_dtypes) for c in out)
    n = sum(c["n"] for c in out)
    assert n == pop.rows
    got = [np.concatenate([c["cols"][j].d2h(dt, c["n"]) for c in out]) if out else np.empty(0, dt)
           for j, dt in enumerate(pop.out_dtypes)]
    # the reference pairs, probe chunk by probe chunk (indexes relative to the chunk)
    want = hj.hash_join_how_ref(build, probe, how, [False, True])
    if how == "left_semi":
        want = want[np.r_[want[1:, 0] != want[:-1, 0], True]] if len(want) else want
    pi, bi = want[:, 0].astype(np.uint32), want[:, 1].astype(np.uint32)
    cols = []
    if has_p:
        for v, nl in ((ppay, None), (probe[1][0], probe[1][1])):
            o, onl = hj.gather_outer_ref(v, nl, pi)
            cols.append(o)
            if nl is not None or p_nullable:
                cols.append(onl)
    if has_b:
        for v, nl in ((bpay, None), (build[1][0], build[1][1])):
            o, onl = hj.gather_outer_ref(v, nl, bi)
            cols.append(o)
            if nl is not None or b_nullable:
                cols.append(onl)
    assert len(cols) == len(got) and n == len(want)
    # rows are a multiset: compare row-sorted, values under NULL masked out
    def rows_of(cs):
        cs = [np.asarray(c).astype(np.int64) for c in cs]
        for j, dt in enumerate(pop.out_dtypes):
            if dt == np.uint8 and j and pop.out_dtypes[j - 1] != np.uint8:
                cs[j - 1] = np.where(cs[j] != 0, 0, cs[j - 1])
        m = np.stack(cs, axis=1) if cs else np.empty((0, 0), np.int64)
        return m[np.lexsort(m.T[::-1])] if len(m) else m
    assert np.array_equal(rows_of(got), rows_of(cols))
    bop.release()
    assert eng.destroyed == 1 and all(b.freed for b in eng.bufs if not any(
        b is x for c in out for x in c["cols"]))
