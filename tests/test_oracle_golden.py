"""Pin the oracle against the reference's own known-answer tests.

Ported values cite /root/reference/be/test/exec/join_hash_map_test.cpp (the
reference is NOT read at runtime — the expected values are literals here and
in tests/golden/).
"""

import json
import os

import numpy as np

from oracle import pyoracle as orc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_slice_hash_kat():
    # join_hash_map_test.cpp:1009-1010: JoinKeyHash<Slice>("abcd") == 11538
    assert orc.join_hash_slice(b"abcd", 1 << 16) == 11538


def test_calc_bucket_num_kats():
    # join_hash_map_test.cpp:1014-1034: calc_bucket_num(1,4,2)==2,
    # calc_bucket_nums({1,2,3,4}) == {2,0,3,1}
    lib = orc.load()
    assert lib.orc_join_hash_u32(1, 2) == 2
    assert [lib.orc_join_hash_u32(v, 2) for v in [1, 2, 3, 4]] == [2, 0, 3, 1]


def test_hash_distribution_stats():
    # join_hash_map_test.cpp:926-1006: min/max bucket occupancy for strided
    # key sets at 2^16 buckets — exact integer statistics of the hash.
    lib = orc.load()
    nb, log = 1 << 16, 16

    def stats32(step, count):
        counts = np.zeros(nb, np.int64)
        for i in range(0, count * step, step):
            counts[lib.orc_join_hash_u32(i & 0xFFFFFFFF, log)] += 1
        return counts.min(), counts.max()

    def stats64(step, count):
        counts = np.zeros(nb, np.int64)
        for i in range(0, count * step, step):
            counts[lib.orc_join_hash_u64(i, log)] += 1
        return counts.min(), counts.max()

    assert stats32(3, nb * 5) == (0, 11)   # :944-947
    assert stats32(7, nb * 5) == (0, 14)   # :956-959
    assert stats32(1, nb * 5) == (4, 6)    # :968-971
    assert stats64(3, nb * 5) == (3, 7)    # :980-983
    assert stats64(7, nb * 5) == (4, 7)    # :992-995
    assert stats64(1, nb * 5) == (4, 6)    # :1004-1006


def test_calc_bucket_size():
    # join_hash_map_helper.h:70-78 — NormalizeCapacity(n+(n-1)/4)+1
    lib = orc.load()
    assert lib.orc_calc_bucket_size(11) == 16
    assert lib.orc_calc_bucket_size(1) == 2
    assert lib.orc_calc_bucket_size(12) == 16
    assert lib.orc_calc_bucket_size(13) == 32  # 13+3=16 -> Normalize(16)=31 -> 32
    for n in [2, 5, 100, 4096, 10_000_000]:
        b = lib.orc_calc_bucket_size(n)
        assert b & (b - 1) == 0  # power of two
        assert b >= n


def test_against_reference_shim():
    """Cross-check vs the reference's OWN compiled hash code: always against
    the vectors that code produced (tests/golden/hash_kats.json) and the
    published xorshift32 sequence, and live against oracle/_ref where the
    shim is built."""
    lib = orc.load()
    with open(os.path.join(GOLDEN, "hash_kats.json")) as f:
        kats = json.load(f)
    assert len(kats["crc_hash_32"]) >= 64 and len(kats["fnv_hash"]) >= 64
    for item in kats["crc_hash_32"]:
        data = bytes.fromhex(item["data_hex"])
        assert lib.orc_crc_hash_32(data, len(data), item["seed"]) == item["expect"]
    for item in kats["fnv_hash"]:
        data = bytes.fromhex(item["data_hex"])
        assert lib.orc_fnv_hash(data, len(data), item["seed"]) == item["expect"]
    # Marsaglia, "Xorshift RNGs" (2003), the (13, 17, 5) triple: the paper's
    # seed 2463534242 steps to 723471715; 1 steps to 270369 then 67634689
    assert lib.orc_xorshift32(2463534242) == 723471715
    assert lib.orc_xorshift32(1) == 270369
    assert lib.orc_xorshift32(270369) == 67634689
    ref = orc.load_ref()
    if ref is None:
        return
    rng = np.random.default_rng(7)
    for _ in range(500):
        n = int(rng.integers(0, 64))
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        seed = int(rng.integers(0, 2**32, dtype=np.uint64))
        assert lib.orc_crc_hash_32(data, n, seed) == ref.ref_crc_hash_32(data, n, seed)
        assert lib.orc_fnv_hash(data, n, seed) == ref.ref_fnv_hash(data, n, seed)
        x = int(rng.integers(0, 2**32, dtype=np.uint64))
        assert lib.orc_xorshift32(x) == ref.ref_xorshift32(x)


def test_golden_fixture_hashes():
    """The committed fixture (generated from the reference KATs + the shim)
    must keep matching — this is what the GPU box checks without /root/reference."""
    with open(os.path.join(GOLDEN, "hash_kats.json")) as f:
        kats = json.load(f)
    lib = orc.load()
    for item in kats["crc_hash_32"]:
        data = bytes.fromhex(item["data_hex"])
        assert lib.orc_crc_hash_32(data, len(data), item["seed"]) == item["expect"]
    for item in kats["fnv_hash"]:
        data = bytes.fromhex(item["data_hex"])
        assert lib.orc_fnv_hash(data, len(data), item["seed"]) == item["expect"]


def test_bucket_chained_build_probe_property():
    """Port of JoinBuildProbeFunc (join_hash_map_test.cpp:1140-1186): build
    keys 0..9 (1-based rows), probe the same keys — every probe key finds
    exactly one match by chain walk; row 0 is the chain-end sentinel."""
    build_keys = np.concatenate([[0], np.arange(10, dtype=np.uint32)]).astype(np.uint32)
    first, nxt, bucket_size, log = orc.bucket_chained_build(build_keys)
    assert bucket_size == 16
    probe = np.arange(10, dtype=np.uint32)
    heads = orc.bucket_chained_lookup(probe, first, bucket_size, log)
    op, ob = orc.probe_emit(build_keys, nxt, probe, heads)
    assert len(op) == 10
    # each probe row i matched build row with equal key
    assert (build_keys[ob] == probe[op]).all()
    assert sorted(op.tolist()) == list(range(10))


def test_bucket_chained_duplicates():
    rng = np.random.default_rng(3)
    build_keys = np.concatenate([[0], rng.integers(0, 50, 200)]).astype(np.uint32)
    first, nxt, bucket_size, log = orc.bucket_chained_build(build_keys)
    probe = rng.integers(0, 80, 300).astype(np.uint32)
    heads = orc.bucket_chained_lookup(probe, first, bucket_size, log)
    op, ob = orc.probe_emit(build_keys, nxt, probe, heads)
    # brute force expected multiset
    expect = []
    for i, k in enumerate(probe):
        for j in range(1, len(build_keys)):
            if build_keys[j] == k:
                expect.append((i, j))
    got = sorted(zip(op.tolist(), ob.tolist()))
    assert got == sorted(expect)


def test_linear_chained_matches_bucket_chained_multiset():
    rng = np.random.default_rng(11)
    build_keys = np.concatenate([[0], rng.integers(0, 1000, 500)]).astype(np.uint32)
    probe = rng.integers(0, 1200, 700).astype(np.uint32)
    bf, bn, bs, bl = orc.bucket_chained_build(build_keys)
    bh = orc.bucket_chained_lookup(probe, bf, bs, bl)
    bop, bob = orc.probe_emit(build_keys, bn, probe, bh)
    lf, ln, ls, ll = orc.linear_chained_build(build_keys)
    lh = orc.linear_chained_lookup(build_keys, probe, lf, ls, ll)
    lop, lob = orc.probe_emit(build_keys, ln, probe, lh)
    assert sorted(zip(bop.tolist(), bob.tolist())) == sorted(zip(lop.tolist(), lob.tolist()))


def test_range_direct_matches_bucket_chained():
    rng = np.random.default_rng(5)
    build_keys = np.concatenate([[0], rng.integers(100, 400, 300)]).astype(np.int32)
    probe = rng.integers(0, 500, 500).astype(np.int32)
    mn, mx = int(build_keys[1:].min()), int(build_keys[1:].max())
    rf, rn = orc.range_direct_build(build_keys, mn, mx)
    rh = orc.range_direct_lookup(probe, mn, mx, rf)
    rop, rob = orc.probe_emit(build_keys.view(np.uint32), rn, probe.view(np.uint32), rh)
    bf, bn_, bs, bl = orc.bucket_chained_build(build_keys.view(np.uint32))
    bh = orc.bucket_chained_lookup(probe.view(np.uint32), bf, bs, bl)
    bop, bob = orc.probe_emit(build_keys.view(np.uint32), bn_, probe.view(np.uint32), bh)
    assert sorted(zip(rop.tolist(), rob.tolist())) == sorted(zip(bop.tolist(), bob.tolist()))


def test_filter_stable():
    rng = np.random.default_rng(9)
    data = rng.integers(0, 2**32, 100_000).astype(np.int64)
    theta = 2**31
    out = orc.filter_i64_lt(data, theta)
    expect = data[data < theta]
    assert np.array_equal(out, expect)
    out_mt = orc.filter_i64_lt(data, theta, mt=True)
    assert np.array_equal(out_mt, expect)


def test_partition_channel_and_layout():
    rng = np.random.default_rng(13)
    keys = rng.integers(0, 2**32, 50_000).astype(np.uint32)
    nch = 8
    ch = orc.partition_channels(keys, nch)
    # ReduceOp semantics: channel = (fnv(key)*nch)>>32
    lib = orc.load()
    for i in rng.integers(0, len(keys), 50):
        h = lib.orc_fnv_hash(keys[i : i + 1].tobytes(), 4, 0x811C9DC5)
        assert ch[i] == (h * nch) >> 32
    sp, ri = orc.partition_counting_sort(ch, nch)
    assert sp[0] == 0 and sp[-1] == len(keys)
    for c in range(nch):
        rows = ri[int(sp[c]) : int(sp[c + 1])]
        assert (ch[rows] == c).all()
        # stable: ascending source order (exchange_sink_operator.cpp:646-649)
        assert (np.diff(rows.astype(np.int64)) > 0).all()
    counts = np.bincount(ch, minlength=nch)
    assert np.array_equal(np.diff(sp).astype(np.int64), counts)


def test_q1_pipeline_small_vs_numpy():
    from starrocks_amd import gen
    seed, n, year = 42, 200_000, 1993
    s, cnt = orc.q1_pipeline(seed, 0, n, year)
    od, ep, dc = gen.gen_lineorder_q1(seed, 0, n)
    mask = (od >= 19930101) & (od <= 19931231)
    assert cnt == int(mask.sum())
    assert s == int((ep[mask].astype(np.int64) * dc[mask]).sum())


def test_q21_pipeline_small_vs_numpy():
    from starrocks_amd import gen
    seed, n, cat, reg = 42, 300_000, 12, 2
    gs = orc.q21_pipeline(seed, 0, n, cat, reg)
    pk, sk, od, rv = gen.gen_lineorder_q21(seed, 0, n)
    pfirst = gen.build_part_dim_payload(seed, gen.N_PARTS_SF100, cat)
    sfirst = gen.build_supp_dim_payload(seed, gen.N_SUPPS_SF100, reg)
    mn, mx, dfirst = gen.build_date_dim_payload(None)
    brand1 = pfirst[pk - 1]
    ok = (brand1 != 0) & (sfirst[sk - 1] != 0)
    year1 = dfirst[od - mn]
    gid = (year1[ok].astype(np.int64) - 1) * 1000 + (brand1[ok].astype(np.int64) - 1)
    expect = np.zeros(7000, np.int64)
    np.add.at(expect, gid, rv[ok].astype(np.int64))
    assert np.array_equal(gs, expect)


def test_slice_join_oracle_vs_brute():
    """Slice-key chained join (orc_slice_build_u32/orc_slice_probe_emit) vs a
    dict-of-strings brute force: identical match-pair multisets."""
    rng = np.random.default_rng(31)
    pool = [f"s{i}".encode() + b"y" * int(rng.integers(0, 7)) for i in range(150)]
    brows = [b""] + [pool[int(i)] for i in rng.integers(0, 150, 3000)]
    prows = [pool[int(i) % 150] if i % 4 else b"missing" for i in rng.integers(0, 600, 9000)]
    bo = np.zeros(len(brows) + 1, np.uint32)
    np.cumsum([len(r) for r in brows], out=bo[1:])
    po = np.zeros(len(prows) + 1, np.uint32)
    np.cumsum([len(r) for r in prows], out=po[1:])
    bb = np.frombuffer(b"".join(brows), np.uint8).copy()
    pb = np.frombuffer(b"".join(prows), np.uint8).copy()
    op, ob = orc.slice_join(bb, bo, len(brows) - 1, pb, po, len(prows), 10_000_000)
    index = {}
    for j in range(1, len(brows)):
        index.setdefault(brows[j], []).append(j)
    expect = sorted((i, j) for i, s in enumerate(prows) for j in index.get(s, []))
    assert sorted(zip(op.tolist(), ob.tolist())) == expect
    assert len(expect) > 0


def test_phmap_mix8_vs_reference_binary():
    """orc_phmap_mix8 (the SimdBlockFilter insert hash for integer keys,
    runtime_filter.h:1271-1276) against the reference's own phmap_mix<8>
    compiled from its headers: always against the vectors that binary
    produced (tests/golden/hash_kats.json), and live against oracle/_ref
    where the shim is built."""
    with open(os.path.join(GOLDEN, "hash_kats.json")) as f:
        kats = json.load(f)
    assert len(kats["phmap_mix8"]) >= 64
    for item in kats["phmap_mix8"]:
        assert orc.load().orc_phmap_mix8(item["input"]) == item["expect"]
    ref = orc.load_ref()
    if ref is None:
        return
    import ctypes
    ref.ref_phmap_mix8.restype = ctypes.c_uint64
    ref.ref_phmap_mix8.argtypes = [ctypes.c_uint64]
    rng = np.random.default_rng(3)
    for a in rng.integers(0, 2**63, 500, dtype=np.uint64).tolist() + [0, 1, 2**64 - 1]:
        assert orc.load().orc_phmap_mix8(a) == ref.ref_phmap_mix8(a)


def test_sbf_filter_properties():
    """Split-block bloom: no false negatives ever; false-positive rate at the
    reference's sizing (~32 bits/key budget) stays low; sizing formula
    matches runtime_filter.cpp:26-31."""
    lib = orc.load()
    assert lib.orc_sbf_log_num_buckets(1) == 1
    assert lib.orc_sbf_log_num_buckets(64) == 1
    assert lib.orc_sbf_log_num_buckets(65) == 2
    assert lib.orc_sbf_log_num_buckets(200_000) == 13
    rng = np.random.default_rng(17)
    members = rng.choice(5_000_000, 100_000, replace=False).astype(np.int32)
    directory, log = orc.sbf_build(members)
    assert sbf_all_pass(members, directory, log)
    non = np.setdiff1d(rng.integers(5_000_000, 50_000_000, 100_000).astype(np.int32),
                       members)
    fp = orc.sbf_test(non, directory, log).mean()
    assert fp < 0.05, fp


def sbf_all_pass(keys, directory, log):
    return bool(orc.sbf_test(keys, directory, log).all())


def test_golden_fixture_phmap_mix8():
    """Committed phmap_mix<8> vectors (generated from the reference's own
    headers via oracle/_ref) — the GPU box pins the SimdBlockFilter insert
    hash against these without /root/reference."""
    with open(os.path.join(GOLDEN, "hash_kats.json")) as f:
        kats = json.load(f)
    lib = orc.load()
    for item in kats["phmap_mix8"]:
        assert lib.orc_phmap_mix8(item["input"]) == item["expect"]
