"""GPU: the ADC scan over 16-bit codes -- rq_dev_linscan_wide, rq_dev_adc_lut_wide, rq_linscan_pq_wide / rq_linscan_opq_wide and
their Python mirrors -- for 1 <= h <= 32767 codewords per codebook.  Every comparison is np.array_equal on ids and on the
distances' bit patterns against tests/scan_wide_oracle.py (the restatement built from the committed oracle, pinned on the CPU
by tests/test_scan_wide_oracle.py); bases too large for numpy are certified on the device (scan_wide_oracle.certify)."""
import ctypes

import numpy as np
import pytest

import nonfinite_ref as nf
import scan_wide_oracle as swo
import scan_wide_stream_cases  # noqa: F401  (registers the stream cases of the wide scan entry points)

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2
BULK_HOST_RESULT_BYTES = 256 << 20
BULK_USABLE_BYTES = (2 << 30) // 5 * 4


def _np(t):
    return t.cpu().numpy()


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _kernel():
    from rayuela_jl_amd import _lib
    return (_lib.lib().rq_last_scan_kernel() or b"").decode()


def _data(n, m, h, sub, nq, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((m, h, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    return codes, centers, queries


def _assert_same(d, i, ref, what):
    assert swo.same(_np(d), _np(i), ref), (what, swo.first_difference(_np(d), _np(i), ref))


# ---- tiers -----------------------------------------------------------------------------------------------------------------
TIERS = [  # (m, h, sub), queries per gather, table in LDS
    ((8, 1024, 2), 4, True),
    ((8, 2048, 2), 2, True),
    ((8, 4096, 2), 1, True),
    ((16, 4096, 2), 4, False),
]


@pytest.mark.parametrize("shape,qpg,in_lds", TIERS)
def test_tiers(rq, oracle, shape, qpg, in_lds):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    m, h, sub = shape
    n, nq = 5003, 9
    p = _lib.scan_wide_plan(m, h)
    assert (p["qpg"], bool(p["in_lds"]), p["qg"]) == (qpg, in_lds, qpg) and p["lds_bytes"] == (131072 if in_lds else 0)
    codes, centers, queries = _data(n, m, h, sub, nq, seed=h + m)
    T = swo.tables(oracle, centers, queries)
    bt, ct, qt = _dev(codes, centers, queries)
    lut = rqd.adc_lut_wide(ct, qt)
    assert np.array_equal(_np(lut).view(np.uint32), T.view(np.uint32)), "table bits"
    for k in (1, 100, n):
        d, i = rqd.linscan_wide(bt, ct, qt, k)
        assert _kernel() == "adc_keys_h16_kernel<%d, %s>" % (qpg, "true" if in_lds else "false")
        _assert_same(d, i, swo.scan_tables(T, codes, k), (shape, k))


# ---- shapes ----------------------------------------------------------------------------------------------------------------
SHAPES = [  # m, h, sub, n, nq (0: queries per group + 1)
    (1, 32767, 16, 70_001, 1),
    (1, 257, 1, 33, 0),
    (2, 32767, 1, 513, 0),
    (3, 257, 6, 33, 0),
    (3, 1000, 1, 70_001, 1),
    (5, 1000, 16, 513, 0),
    (5, 257, 6, 70_001, 0),
    (32, 257, 1, 513, 1),
    (32, 1000, 6, 33, 0),
    (32, 257, 16, 70_001, 3),
]


@pytest.mark.parametrize("m,h,sub,n,nq", SHAPES)
def test_shapes_k_eq_n_and_n_minus_1(rq, oracle, m, h, sub, n, nq):
    """Odd m: rows are 2-byte aligned only; every shape also runs from a codes pointer offset by one row.  nq = queries per
    group + 1 leaves a ragged last group."""
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    nq = nq or _lib.scan_wide_plan(m, h)["qg"] + 1
    codes, centers, queries = _data(n + 1, m, h, sub, nq, seed=n + m + h)
    T = swo.tables(oracle, centers, queries)
    bt, ct, qt = _dev(codes, centers, queries)
    assert np.array_equal(_np(rqd.adc_lut_wide(ct, qt)).view(np.uint32), T.view(np.uint32)), "table bits"
    for k in (n, n - 1):
        d, i = rqd.linscan_wide(bt[:n], ct, qt, k)
        _assert_same(d, i, swo.scan_tables(T, codes[:n], k), (m, h, k))
        shifted = bt[1:]
        assert shifted.data_ptr() == bt.data_ptr() + 2 * m and shifted.is_contiguous()
        d, i = rqd.linscan_wide(shifted, ct, qt, k)
        _assert_same(d, i, swo.scan_tables(T, codes[1:], k), (m, h, k, "offset by one row"))


# ---- h = 256: the byte scan's answer ---------------------------------------------------------------------------------------
def test_h256_equals_the_byte_scan(rq):
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq = 100_000, 8, 4, 5
    rng = np.random.default_rng(256)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    b8, b16, ct, qt = _dev(codes, codes.astype(np.int16), centers, queries)
    for k in (100, 65537):
        d0, i0 = rqd.linscan(b8, ct, qt, k)
        byte_kernel = _kernel()
        d1, i1 = rqd.linscan_wide(b16, ct, qt, k)
        assert _kernel() == "adc_keys_h16_kernel<4, true>" and byte_kernel.startswith("adc_scan" if k == 100 else "adc_bulk_keys")
        assert torch.equal(i0, i1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32)), k
        k0 = rqd.linscan(b8, ct, qt, k, want_keys=True)
        k1 = rqd.linscan_wide(b16, ct, qt, k, want_keys=True)
        assert torch.equal(k0, k1), k


# ---- ties ------------------------------------------------------------------------------------------------------------------
def test_all_rows_identical_lowest_ids(rq):
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq = 20_000, 4, 300, 2, 5
    codes, centers, queries = _data(1, m, h, sub, nq, seed=5)
    bt, ct, qt = _dev(np.tile(codes, (n, 1)), centers, queries)
    for k in (1, 1000, n):
        d, i = rqd.linscan_wide(bt, ct, qt, k)
        assert np.array_equal(_np(i), np.tile(np.arange(k, dtype=np.int32), (nq, 1))), k
        assert np.all(_np(d).view(np.uint32) == _np(d).view(np.uint32)[:, :1])


def test_heavy_duplicates(rq, oracle):
    """The "dups" construction of tests/test_gpu_bulk_topk.py at h = 300: integer tables, 4 code values per sub-quantizer."""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq = 90_000, 4, 300, 2, 9
    d = m * sub
    centers = (synth.splitmix64(np.arange(m * h * sub, dtype=np.uint64) ^ np.uint64(8)) % np.uint64(3)).astype(np.float32)
    centers = centers.reshape(m, h, sub)
    queries = (synth.splitmix64(np.arange(nq * d, dtype=np.uint64) ^ np.uint64(9)) % np.uint64(3)).astype(np.float32)
    queries = queries.reshape(nq, d)
    codes = ((synth.random_codes(n, m, seed=4) % 4).astype(np.int16) * 97)      # 0, 97, 194, 291: above 256 too
    T = swo.tables(oracle, centers, queries)
    bt, ct, qt = _dev(codes, centers, queries)
    for k in (10, 70_000, n):
        dd, ii = rqd.linscan_wide(bt, ct, qt, k)
        _assert_same(dd, ii, swo.scan_tables(T, codes, k), k)


# ---- non-finite inputs -----------------------------------------------------------------------------------------------------
def test_non_finite_inputs(rq):
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq = 4001, 4, 700, 2, 10
    codes, centers, queries = _data(n, m, h, sub, nq, seed=77)
    clean = [0, 2, 4, 5, 7, 8, 9]
    nf.put_bits(queries, (1, 3), nf.NAN_NEG)         # a NaN query: all padding
    queries[3, 0] = np.inf                           # an infinite coordinate: every distance +Inf, the k smallest ids
    queries[6, 5] = -np.inf
    bt, ct, qt = _dev(codes, centers, queries)
    for k in (1, 100, n):
        ref = swo.scan_tables(swo.direct_tables(centers, queries), codes, k)
        d, i = rqd.linscan_wide(bt, ct, qt, k)
        _assert_same(d, i, ref, ("queries", k))
        assert np.all(_np(i).view(np.uint32)[1] == 0xFFFFFFFF) and np.all(_np(d).view(np.uint32)[1] == nf.PAD_BITS)
        assert np.array_equal(_np(i)[3], np.arange(k)) and np.all(np.isposinf(_np(d)[3]))
        d2, i2 = rqd.linscan_wide(bt, ct, _dev(queries[clean])[0], k)      # the clean queries are unaffected
        assert np.array_equal(_np(i2), _np(i)[clean]) and np.array_equal(_np(d2).view(np.uint32), _np(d).view(np.uint32)[clean])
    # an Inf and a NaN codeword: rows with the NaN codeword drop out of every list, which then ends in padding
    centers2 = centers.copy()
    centers2[1, 650, 0] = np.inf
    nf.put_bits(centers2, (2, 300, 1), nf.NAN_POS)
    nbad = int((codes[:, 2] == 300).sum())
    assert nbad > 0 and (codes[:, 1] == 650).any()
    c2, q2 = _dev(centers2, queries[clean])
    for k in (100, n):
        ref = swo.scan_tables(swo.direct_tables(centers2, queries[clean]), codes, k)
        d, i = rqd.linscan_wide(bt, c2, q2, k)
        _assert_same(d, i, ref, ("codewords", k))
    assert np.all(_np(i).view(np.uint32)[:, n - nbad:] == 0xFFFFFFFF) and np.all(_np(i).view(np.uint32)[:, :n - nbad] < n)


# ---- codes outside [0, h) --------------------------------------------------------------------------------------------------
def _bad_codes(n, m, h, seed):
    codes, centers, queries = _data(n, m, h, 2, 6, seed=seed)
    bad = {17: h, 1200: 32767, n - 1: -1}
    for col, (row, value) in enumerate(bad.items()):
        codes[row, col % m] = value
    return codes, centers, queries, sorted(bad)


def test_device_entry_never_returns_a_row_with_a_bad_code(rq, oracle):
    from rayuela_jl_amd import device as rqd
    n, m, h = 3001, 3, 1000
    codes, centers, queries, bad = _bad_codes(n, m, h, seed=9)
    T = swo.tables(oracle, centers, queries)
    bt, ct, qt = _dev(codes, centers, queries)
    for k in (1, 50, n):
        d, i = rqd.linscan_wide(bt, ct, qt, k)
        _assert_same(d, i, swo.scan_tables(T, codes, k), k)
    ids = _np(i).view(np.uint32)
    assert np.all(ids[:, n - 3:] == 0xFFFFFFFF) and np.all(_np(d).view(np.uint32)[:, n - 3:] == nf.PAD_BITS)
    for q in range(ids.shape[0]):
        assert np.array_equal(np.sort(ids[q, :n - 3]), np.setdiff1d(np.arange(n), bad))


@pytest.mark.parametrize("code_base", [0, 1])
def test_host_entry_refuses_bad_codes(rq, code_base):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    n, m, h, k = 3001, 3, 1000, 10
    codes, centers, queries, bad = _bad_codes(n, m, h, seed=10)
    codes = (codes.astype(np.int32) + code_base).astype(np.int16)      # 32767 + 1 wraps to -32768: bad either way
    nq, d = queries.shape
    dists = np.full((nq, k), -7.0, dtype=np.float32)
    ids = np.full((nq, k), 0xA5A5A5A5, dtype=np.uint32)
    R = np.eye(d, dtype=np.float32)
    rc = L.rq_linscan_pq_wide(dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, centers.ctypes.data, queries.ctypes.data,
                              n, nq, m, h, d, k, code_base, 1)
    msg = L.rq_last_error().decode()
    assert rc == RQ_EINVAL and "row %d " % bad[0] in msg, (rc, msg)
    rc = L.rq_linscan_opq_wide(dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, centers.ctypes.data,
                               queries.ctypes.data, R.ctypes.data, n, nq, m, h, d, k, code_base, 1)
    assert rc == RQ_EINVAL and "row %d " % bad[0] in L.rq_last_error().decode()
    assert np.all(dists == -7.0) and np.all(ids == 0xA5A5A5A5)


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_keys_id_offset_id_base_and_shard_merge(rq, oracle):
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq, k = 30_011, 5, 600, 2, 7, 300
    codes, centers, queries = _data(n, m, h, sub, nq, seed=12)
    T = swo.tables(oracle, centers, queries)
    bt, ct, qt = _dev(codes, centers, queries)
    off = 2 ** 32 - n - 2
    bits, ids, keys = swo.scan_tables(T, codes, k, id_base=1, id_offset=off)
    d, i = rqd.linscan_wide(bt, ct, qt, k, id_offset=off, id_base=1)
    _assert_same(d, i, (bits, ids), "id_offset + id_base")
    kk = rqd.linscan_wide(bt, ct, qt, k, id_offset=off, id_base=1, want_keys=True)
    assert np.array_equal(_np(kk).view(np.uint64), keys), "keys stay zero-based"
    # dists, ids and keys of one call
    from rayuela_jl_amd import _lib
    d3 = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    i3 = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    k3 = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().rq_dev_linscan_wide(d3.data_ptr(), i3.data_ptr(), k3.data_ptr(), bt.data_ptr(), ct.data_ptr(),
                                              qt.data_ptr(), n, nq, m, h, m * sub, k, off, 1, rqd._stream()))
    assert torch.equal(d3.view(torch.int32), d.view(torch.int32)) and torch.equal(i3, i) and torch.equal(k3, kk)
    # two row shards, merged by rq_dev_merge_topk, equal the single scan
    cut = 12_345
    d0, i0 = rqd.linscan_wide(bt, ct, qt, k)
    ka = rqd.linscan_wide(bt[:cut], ct, qt, k, want_keys=True)
    kb = rqd.linscan_wide(bt[cut:], ct, qt, k, id_offset=cut, want_keys=True)
    dm, im = rqd.merge_topk(torch.stack([ka, kb], dim=1).contiguous(), k)
    assert torch.equal(im, i0) and torch.equal(dm.view(torch.int32), d0.view(torch.int32))


# ---- host path -------------------------------------------------------------------------------------------------------------
def test_host_mirrors_pq_and_opq(rq, oracle):
    n, m, h, sub, nq, k = 20_000, 4, 1000, 4, 11, 500
    codes, centers, queries = _data(n, m, h, sub, nq, seed=21)
    C = [centers[j] for j in range(m)]
    ref = swo.scan(oracle, codes, centers, queries, k, id_base=1)
    for B in (codes.view(np.uint16), codes, codes.astype(np.int32) + 1, (codes + 1).astype(np.int64)):
        d, i = rq.linscan_pq_u16(B, queries, C, k)
        assert swo.same(d, i, ref), (B.dtype, swo.first_difference(d, i, ref))
    R = np.linalg.qr(np.random.default_rng(4).standard_normal((m * sub, m * sub)))[0].astype(np.float32)
    ref = swo.scan(oracle, codes, centers, oracle.rotate_T(R, queries), k, id_base=1)
    for B in (codes.view(np.uint16), codes.astype(np.int32) + 1):
        d, i = rq.linscan_opq_u16(B, queries, C, R, k)
        assert swo.same(d, i, ref), (B.dtype, swo.first_difference(d, i, ref))


def test_host_call_streams_results_in_query_chunks(rq, oracle):
    """nq * k * 8 bytes pass BULK_HOST_RESULT_BYTES: bulk_fetch brings the results back in two query chunks."""
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq = 33_000, 2, 300, 2, 1100
    k = n
    assert nq * k * 8 > BULK_HOST_RESULT_BYTES and BULK_HOST_RESULT_BYTES // (8 * k) < nq
    codes, centers, queries = _data(n, m, h, sub, nq, seed=22)
    d, i = rq.linscan_pq_u16(codes, queries, [centers[j] for j in range(m)], k)
    bt, ct, qt = _dev(codes, centers, queries)
    d0, i0 = rqd.linscan_wide(bt, ct, qt, k, id_base=1)
    assert np.array_equal(i, _np(i0).view(np.uint32)) and np.array_equal(d.view(np.uint32), _np(d0).view(np.uint32))
    chunk = BULK_HOST_RESULT_BYTES // (8 * k)
    some = [0, chunk - 1, chunk, nq - 1]
    ref = swo.scan(oracle, codes, centers, queries[some], k, id_base=1)
    assert swo.same(d[some], i[some], ref)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_end_to_end_encode_then_search(rq):
    import rayuela_jl_amd.synth as synth
    n, d, m, h = 20_000, 32, 4, 1024
    sub = d // m
    X = synth.sift_like(n, d, seed=3)
    rng = np.random.default_rng(3)
    C = [np.ascontiguousarray(X[rng.integers(0, n, h), j * sub:(j + 1) * sub]) for j in range(m)]
    B = rq.quantize_pq_u16(X, C)
    assert B.dtype == np.uint16 and B.max() < h and B.max() > 255
    rows = rng.integers(0, n, 16)
    Q = np.concatenate([C[j][B[rows, j]] for j in range(m)], axis=1)           # the reconstructions of 16 base rows
    dists, idx = rq.linscan_pq_u16(B, Q, C, 10)
    assert np.all(dists[:, 0] == 0.0) and np.all(dists[:, 0].view(np.uint32) == 0)
    for q, r in enumerate(rows):
        first = int(np.flatnonzero((B == B[r]).all(axis=1))[0])                 # the lowest id among the rows sharing that code
        assert idx[q, 0] == first + 1, (q, r, first, idx[q, 0])
        same = int((B == B[r]).all(axis=1).sum())
        assert np.all(dists[q, :min(same, 10)] == 0.0)


# ---- several batches -------------------------------------------------------------------------------------------------------
def test_several_batches_equal_one_query_at_a_time(rq):
    """n = 1e6, k = 10: a query takes 8 n bytes of keys, so at most `batch` = usable scratch / 8 n queries fit one batch (the
    tables and the select scratch only make it smaller); nq = 2 batch + 7 runs three batches at least."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, k = 1_000_000, 2, 300, 2, 10
    batch = BULK_USABLE_BYTES // (8 * n)
    assert 16 <= batch < 1000, batch
    nq = 2 * batch + 7
    codes, centers, queries = _data(1, m, h, sub, nq, seed=31)
    ct, qt = _dev(centers, queries)
    bt = torch.randint(0, h, (n, m), dtype=torch.int16, device="cuda", generator=torch.Generator("cuda").manual_seed(31))
    d1, i1 = rqd.linscan_wide(bt, ct, qt, k)
    for q in range(nq):
        d2, i2 = rqd.linscan_wide(bt, ct, qt[q:q + 1].contiguous(), k)
        assert torch.equal(i2[0], i1[q]) and torch.equal(d2[0].view(torch.int32), d1[q].view(torch.int32)), q
    assert swo.certify(d1, i1, k, rqd.adc_lut_wide(ct, qt), bt, n, chunk=1 << 19) == nq


# ---- past 2^32 bytes of codes ----------------------------------------------------------------------------------------------
def test_codes_past_4_gib_certified(rq, oracle):
    """n = 134 300 000 rows of 32 bytes: row offsets pass 2^32 bytes, key offsets 2^30 entries; every query certified."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq, k = 134_300_000, 16, 1024, 2, 2, 100
    assert n * 2 * m > 2 ** 32
    _, centers, queries = _data(1, m, h, sub, nq, seed=41)
    ct, qt = _dev(centers, queries)
    bt = torch.randint(0, h, (n, m), dtype=torch.int16, device="cuda", generator=torch.Generator("cuda").manual_seed(41))
    lut = rqd.adc_lut_wide(ct, qt)
    assert np.array_equal(_np(lut).view(np.uint32), swo.tables(oracle, centers, queries).view(np.uint32))
    # rows beyond 2^32 bytes of codes that must be among the answers: query q's best code at three rows past row 2^27
    planted = [[2 ** 27 + 3 + q, n - 5 - q, n - 1 - q] for q in range(nq)]
    for q in range(nq):
        bt[planted[q]] = lut[q].argmin(dim=1).to(torch.int16)
    d1, i1 = rqd.linscan_wide(bt, ct, qt, k)
    assert _kernel() == "adc_keys_h16_kernel<2, true>"          # 16 * 1024 entries of two queries: 128 KiB of LDS
    assert swo.certify(d1, i1, k, lut, bt, n) == nq
    for q in range(nq):
        assert i1[q, :3].tolist() == planted[q], (q, i1[q, :3].tolist())
    del bt
    torch.cuda.empty_cache()


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(rq):
    import torch
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    L = _lib.lib()
    n, m, h, sub, nq, k = 1000, 4, 300, 2, 3, 10
    d = m * sub
    codes, centers, queries = _data(n, m, h, sub, nq, seed=51)
    bt, ct, qt = _dev(codes, centers, queries)
    dd = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    ii = torch.full((nq, k), -3, dtype=torch.int32, device="cuda")
    kk = torch.full((nq, k), -5, dtype=torch.int64, device="cuda")
    lut = torch.full((nq, m, h), -7.0, dtype=torch.float32, device="cuda")
    good = dict(dists=dd.data_ptr(), ids=ii.data_ptr(), keys=kk.data_ptr(), codes=bt.data_ptr(), centers=ct.data_ptr(),
                queries=qt.data_ptr(), n=n, nq=nq, m=m, h=h, d=d, k=k, id_offset=0, id_base=0)

    def dev(**patch):
        a = dict(good, **patch)
        return L.rq_dev_linscan_wide(a["dists"], a["ids"], a["keys"], a["codes"], a["centers"], a["queries"], a["n"], a["nq"],
                                     a["m"], a["h"], a["d"], a["k"], a["id_offset"], a["id_base"], rqd._stream())

    assert dev(nq=0) == 0 and dev(nq=-1) == 0
    for patch in (dict(codes=None), dict(centers=None), dict(queries=None), dict(keys=None, dists=None), dict(keys=None, ids=None),
                  dict(id_base=2), dict(id_base=-1), dict(d=d + 1), dict(d=m - 1), dict(k=0), dict(k=n + 1), dict(n=0),
                  dict(n=2 ** 31), dict(id_offset=2 ** 32 - n + 1), dict(codes=bt.data_ptr() + 1)):
        assert dev(**patch) == RQ_EINVAL, patch
    for patch in (dict(h=0), dict(h=32768), dict(m=0, d=0), dict(m=33, d=66)):
        assert dev(**patch) == RQ_EUNSUPPORTED, patch
    assert L.rq_dev_adc_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), 0, m, h, sub, rqd._stream()) == 0
    assert L.rq_dev_adc_lut_wide(None, ct.data_ptr(), qt.data_ptr(), nq, m, h, sub, rqd._stream()) == RQ_EINVAL
    assert L.rq_dev_adc_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), nq, m, h, 0, rqd._stream()) == RQ_EINVAL
    assert L.rq_dev_adc_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), nq, 33, h, sub, rqd._stream()) == RQ_EUNSUPPORTED
    assert L.rq_dev_adc_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), nq, m, 32768, sub, rqd._stream()) == RQ_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((dd == -7.0).all()) and bool((ii == -3).all()) and bool((kk == -5).all()) and bool((lut == -7.0).all())

    # the host entries
    hd = np.full((nq, k), -7.0, dtype=np.float32)
    hi = np.full((nq, k), 0xA5A5A5A5, dtype=np.uint32)
    R = np.eye(d, dtype=np.float32)
    hgood = dict(dists=hd.ctypes.data, ids=hi.ctypes.data, codes=codes.ctypes.data, centers=centers.ctypes.data,
                 queries=queries.ctypes.data, R=R.ctypes.data, n=n, nq=nq, m=m, h=h, d=d, k=k, code_base=0, id_base=1)

    def host(opq, **patch):
        a = dict(hgood, **patch)
        if opq:
            return L.rq_linscan_opq_wide(a["dists"], a["ids"], a["codes"], a["centers"], a["queries"], a["R"], a["n"], a["nq"],
                                         a["m"], a["h"], a["d"], a["k"], a["code_base"], a["id_base"])
        return L.rq_linscan_pq_wide(a["dists"], a["ids"], a["codes"], a["centers"], a["queries"], a["n"], a["nq"], a["m"], a["h"],
                                    a["d"], a["k"], a["code_base"], a["id_base"])

    for opq in (False, True):
        assert host(opq, nq=0) == 0
        for patch in (dict(dists=None), dict(ids=None), dict(codes=None), dict(centers=None), dict(queries=None),
                      dict(code_base=2), dict(code_base=-1), dict(id_base=2), dict(d=d + 1), dict(k=0), dict(k=n + 1),
                      dict(n=0), dict(n=2 ** 31)):
            assert host(opq, **patch) == RQ_EINVAL, (opq, patch)
        for patch in (dict(h=0), dict(h=32768), dict(m=0, d=0), dict(m=33, d=66)):
            assert host(opq, **patch) == RQ_EUNSUPPORTED, (opq, patch)
    assert host(True, R=None) == RQ_EINVAL
    assert np.all(hd == -7.0) and np.all(hi == 0xA5A5A5A5)
