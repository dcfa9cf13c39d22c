"""GPU: the index handle over 16-bit codes (rq_index_create[_sharded]_wide, rq_index_set_codes_wide).
Mirrors tests/test_gpu_index.py: a base cut into LOGICAL shards of the one GPU must return what ONE rq_dev_linscan_wide call
over the whole base returns (tests/test_gpu_scan_wide.py pins that call to the oracle), ids and distance bits, plus
tests/scan_wide_oracle.py directly once."""
import ctypes as C

import numpy as np
import pytest

import scan_wide_oracle as swo
from switch_table import switches

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _data(n, m, h, sub, nq, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((m, h, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    return codes, centers, queries


def _one_scan(codes, centers, queries, k, id_offset=0, id_base=0):
    """One rq_dev_linscan_wide over the whole base: (dists f32, ids u32) on the host."""
    import torch
    from rayuela_jl_amd import device as rqd
    bt, ct, qt = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (codes, centers, queries)]
    d, i = rqd.linscan_wide(bt, ct, qt, k, id_offset=id_offset, id_base=id_base)
    return d.cpu().numpy(), i.cpu().numpy().view(np.uint32)


def _same(got, ref):
    return np.array_equal(got[1], ref[1]) and _eq_bits(got[0], ref[0])


N, M, H, SUB, NQ, K = 20_001, 8, 1024, 2, 5, 100
D = M * SUB


@pytest.fixture(scope="module")
def base(rq):
    codes, centers, queries = _data(N, M, H, SUB, NQ, seed=31)
    return dict(codes=codes, centers=centers, queries=queries, C=[centers[i] for i in range(M)],
                ref=_one_scan(codes, centers, queries, K))


@pytest.mark.parametrize("nshards", [1, 2, 3, 5, 8])
def test_logical_shards_equal_one_scan(rq, base, nshards):
    with rq.IndexU16(base["C"], D, devices=[0] * nshards) as ix:
        ix.set_codes(base["codes"])
        info = ix.info()
        assert info["shards"] == nshards and info["devices"] == 1 and info["n"] == N and sum(info["rows_per_shard"]) == N
        got = ix.search(base["queries"], K, id_base=0)
    assert _same(got, base["ref"]), nshards


def test_against_the_oracle(rq, oracle, base):
    ref = swo.scan(oracle, base["codes"], base["centers"], base["queries"], K, id_base=1)
    with rq.IndexU16(base["C"], D, devices=[0, 0, 0]) as ix:
        dists, ids = ix.set_codes(base["codes"]).search(base["queries"], K)
    assert swo.same(dists, ids, ref), swo.first_difference(dists, ids, ref)


def test_default_device_form(rq, base):
    with rq.IndexU16(base["C"], D) as ix:
        got = ix.set_codes(base["codes"]).search(base["queries"], K, id_base=0)
        assert ix.info()["shards"] == 1
    assert _same(got, base["ref"])


def test_shards_shorter_than_k_and_empty_shards(rq):
    """n = 10 over 8 shards (1-2 rows each) with k = 7 > every shard, and n = 5 over 8 shards (3 empty)."""
    m, h, sub, nq = 8, 1024, 2, 5
    for n, k in [(10, 7), (5, 5)]:
        codes, centers, queries = _data(n, m, h, sub, nq, seed=n)
        with rq.IndexU16([centers[i] for i in range(m)], m * sub, devices=[0] * 8) as ix:
            got = ix.set_codes(codes).search(queries, k, id_base=0)
        assert _same(got, _one_scan(codes, centers, queries, k)), (n, k)


def test_opq_search(rq, base):
    import rayuela_jl_amd.synth as synth
    R = synth.rotation(D, seed=3)
    ref = rq.linscan_opq_u16(base["codes"], base["queries"], base["C"], R, K)
    with rq.IndexU16(base["C"], D) as one, rq.IndexU16(base["C"], D, devices=[0] * 3) as many:
        g1 = one.set_codes(base["codes"]).search(base["queries"], K, R=R)
        g3 = many.set_codes(base["codes"]).search(base["queries"], K, R=R)
    assert _same(g1, ref) and _same(g3, ref)


def test_rccl_selftest_exchange(rq, base):
    with switches(EXCHANGE_SELFTEST=1):
        with rq.IndexU16(base["C"], D, devices=[0, 0, 0, 0]) as ix:
            ix.set_codes(base["codes"])
            exchange = ix.info()["exchange"]
            got = ix.search(base["queries"], K, id_base=0)
    assert _same(got, base["ref"]), exchange


@pytest.mark.parametrize("chunks", [2, 3])
def test_query_chunks(rq, base, chunks):
    with switches(IDX_QCHUNKS=chunks):
        with rq.IndexU16(base["C"], D, devices=[0, 0, 0]) as ix:
            ix.set_codes(base["codes"])
            for _ in range(2):
                assert _same(ix.search(base["queries"], K, id_base=0), base["ref"]), chunks
        # a shard shorter than k (KEY_MAX padding) inside a chunked search
        with rq.IndexU16(base["C"], D, devices=[0] * 7) as ix:
            got = ix.set_codes(base["codes"][:40]).search(base["queries"], 20, id_base=0)
        assert _same(got, _one_scan(base["codes"][:40], base["centers"], base["queries"], 20))


def test_bulk_k(rq):
    """k = 65_537 > RQ_MAX_K: the lists of the shards are merged by the bulk select."""
    n, m, h, sub, nq, k = 70_000, 2, 300, 2, 3, 65_537
    codes, centers, queries = _data(n, m, h, sub, nq, seed=65)
    with rq.IndexU16([centers[i] for i in range(m)], m * sub, devices=[0] * 3) as ix:
        got = ix.set_codes(codes).search(queries, k, id_base=0)
    assert _same(got, _one_scan(codes, centers, queries, k))


def test_h256_equals_the_byte_index(rq):
    n, m, sub, nq, k = 20_001, 8, 4, 5, 100
    rng = np.random.default_rng(256)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    Cl = [centers[i] for i in range(m)]
    for devices in (None, [0, 0, 0]):
        with rq.Index(Cl, m * sub, devices=devices) as b8, rq.IndexU16(Cl, m * sub, devices=devices) as b16:
            r8 = b8.set_codes(codes).search(queries, k)
            r16 = b16.set_codes(codes.astype(np.int16)).search(queries, k)
        assert _same(r16, r8), devices


def test_id_offset_past_2_to_31_and_code_bases(rq, base):
    off = 2 ** 31 + 5
    ref = _one_scan(base["codes"], base["centers"], base["queries"], K, id_offset=off, id_base=1)
    assert ref[1].min() > 2 ** 31
    with rq.IndexU16(base["C"], D, devices=[0, 0, 0]) as ix:
        zero = ix.set_codes(base["codes"], id_offset=off).search(base["queries"], K)                       # int16: zero-based
        one = ix.set_codes(base["codes"].astype(np.int32) + 1, id_offset=off).search(base["queries"], K)   # int32: one-based
        with pytest.raises(rq.RayuelaHipError):
            ix.set_codes(base["codes"], id_offset=2 ** 32 - N)
    assert _same(zero, ref) and _same(one, ref)


def _raw_set(ix, codes, code_base, id_offset=0):
    from rayuela_jl_amd import _lib
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    rc = _lib.lib().rq_index_set_codes_wide(ix._h, codes.ctypes.data, codes.shape[0], code_base, id_offset)
    return rc, _lib.lib().rq_last_error().decode()


@pytest.mark.parametrize("code_base", [0, 1])
def test_bad_code_is_refused_and_the_loaded_base_stays(rq, base, code_base):
    small = base["codes"][:5000]
    ref = _one_scan(small, base["centers"], base["queries"], K)
    with rq.IndexU16(base["C"], D, devices=[0, 0, 0]) as ix:
        ix.set_codes(small)
        for row, value in [(17, H), (12_345, -1), (N - 1, 32767)]:      # zero-based values outside [0, h); first, second, last shard
            bad = base["codes"].copy() + np.int16(code_base)
            bad[row, row % M] = min(value + code_base, 32767)
            if row < N - 1:
                bad[N - 1, 0] = -7                                      # a later bad row: the FIRST one is named
            rc, msg = _raw_set(ix, bad, code_base)
            assert rc == RQ_EINVAL and ("row %d " % row) in msg, (row, msg)
            info = ix.info()
            assert info["n"] == 5000 and sum(info["rows_per_shard"]) == 5000
            assert _same(ix.search(base["queries"], K, id_base=0), ref), row
        rc, msg = _raw_set(ix, base["codes"] + code_base, 2)
        assert rc == RQ_EINVAL and "code_base" in msg
        rc, _ = _raw_set(ix, base["codes"] + code_base, code_base)
        assert rc == 0 and ix.info()["n"] == N
        assert _same(ix.search(base["queries"], K, id_base=0), base["ref"])


def test_wrong_width_calls_are_refused(rq, base):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(1)
    c8 = rng.standard_normal((M, 256, SUB)).astype(np.float32)
    b8 = rng.integers(0, 256, (100, M), dtype=np.uint8)
    with rq.Index([c8[i] for i in range(M)], D) as narrow, rq.IndexU16(base["C"], D) as wide:
        rc, msg = _raw_set(narrow, b8.astype(np.int16), 0)
        assert rc == RQ_EINVAL and "byte index" in msg
        assert L.rq_index_set_codes(wide._h, b8.ctypes.data, 100, 0) == RQ_EINVAL
        assert "wide" in L.rq_last_error().decode()
        assert L.rq_index_set_codes_synth(wide._h, 100, 7, 0) == RQ_EINVAL
        with pytest.raises(rq.RayuelaHipError):
            wide.search(base["queries"], 10)                 # still no codes
        narrow.set_codes(b8)
        wide.set_codes(base["codes"])
        assert _same(wide.search(base["queries"], K, id_base=0), base["ref"])


def test_create_limits(rq):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    cen = np.zeros(33 * 4 * 2, dtype=np.float32)
    dev = (C.c_int * 1)(0)
    for m, h, d in [(0, 4, 8), (33, 4, 66), (4, 0, 8), (4, 32768, 8), (4, 4, 6)]:
        assert not L.rq_index_create_wide(m, h, d, cen.ctypes.data), (m, h, d)
        assert L.rq_last_error().decode() != ""
        assert not L.rq_index_create_sharded_wide(m, h, d, cen.ctypes.data, C.cast(dev, C.c_void_p), 1), (m, h, d)
    assert not L.rq_index_create_wide(4, 4, 8, None)
    hnd = L.rq_index_create_wide(4, 4, 8, cen.ctypes.data)
    assert hnd
    L.rq_index_destroy(hnd)


def test_a_sliced_shard(rq, base):
    """The scan's row slices (rq_test_scan_wide_slice_rows) under the index: three shards of 6667 rows in slices of 1000."""
    from rayuela_jl_amd import _lib
    prev = _lib.lib().rq_test_scan_wide_slice_rows(1000)
    try:
        with rq.IndexU16(base["C"], D, devices=[0, 0, 0]) as ix:
            got = ix.set_codes(base["codes"]).search(base["queries"], K, id_base=0)
        with rq.IndexU16(base["C"], D) as ix:
            one = ix.set_codes(base["codes"]).search(base["queries"], K, id_base=0)
    finally:
        _lib.lib().rq_test_scan_wide_slice_rows(prev)
    assert _same(got, base["ref"]) and _same(one, base["ref"])


def test_bindings_end_to_end(rq):
    """Dataset.quantize_u16 on a u8 base with h = 512, then IndexU16.set_codes, then search equals linscan_pq_u16."""
    n, d, m, h, nq, k = 5000, 32, 4, 512, 7, 50
    rng = np.random.default_rng(512)
    X = rng.integers(0, 256, (n, d), dtype=np.uint8)
    Q = rng.integers(0, 256, (nq, d)).astype(np.float32)
    Cl = [X[rng.integers(0, n, h), i * (d // m):(i + 1) * (d // m)].astype(np.float32) + rng.standard_normal((h, d // m)).astype(np.float32)
          for i in range(m)]
    with rq.Dataset(X) as ds:
        B = ds.quantize_u16(Cl)
    assert B.dtype == np.uint16 and B.shape == (n, m) and B.max() < h and B.max() > 255
    assert np.array_equal(B, rq.quantize_pq_u16(X.astype(np.float32), Cl))
    ref = rq.linscan_pq_u16(B, Q, Cl, k)
    with rq.IndexU16(Cl, d, devices=[0, 0]) as ix:
        got = ix.set_codes(B).search(Q, k)
    assert _same(got, ref)
