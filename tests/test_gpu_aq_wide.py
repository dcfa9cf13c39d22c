"""GPU: linscan_lsq / linscan_cq and the database norms over 16-bit codes -- rq_dev_aq_lut_wide, rq_dev_linscan_aq_wide,
rq_linscan_lsq_wide / rq_linscan_cq_wide / rq_linscan_lsq_cbnorms_wide, the five *_norms_wide entries and their Python
mirrors -- for up to 32767 codewords per codebook.  Every comparison is np.array_equal / torch.equal on
ids, keys and the distances' bit patterns against tests/aq_wide_oracle.py (pinned on the CPU by tests/test_aq_wide_oracle.py);
bases too large for numpy are certified on the device."""
import numpy as np
import pytest

import aq_wide_oracle as awo
import aq_wide_stream_cases  # noqa: F401  (registers the stream cases of the new `void *stream` entry points)
import nonfinite_ref as nf
import norms_oracle as no
import scan_wide_oracle as swo

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2
BULK_HOST_RESULT_BYTES = 256 << 20
BULK_USABLE_BYTES = (2 << 30) // 5 * 4
TQ = 16          # AQ_LUT_TQ: the query tile of aq_lut_h16_kernel


def _np(t):
    return t.cpu().numpy()


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _kernel():
    from rayuela_jl_amd import _lib
    return (_lib.lib().rq_last_scan_kernel() or b"").decode()


def _bits(t):
    return _np(t).view(np.uint32)


def _assert_same(d, i, ref, what):
    assert awo.same(_np(d), _np(i), ref), (what, nf.first_difference(_np(d), _np(i), ref[:2]))


def _scan(bt, ct, qt, k, nt=None, **kw):
    from rayuela_jl_amd import device as rqd
    return rqd.linscan_aq_wide(bt, ct, qt, k, dbnorms=nt, **kw)


# ---- tables ----------------------------------------------------------------------------------------------------------------
TABLE_SHAPES = [  # d, h, m, nq: every d, h, m and nq of the issue's list at least once
    (1, 1, 1, 1), (5, 2, 3, TQ - 1), (30, 257, 8, TQ + 1), (96, 1000, 3, 2 * TQ + 1), (128, 257, 1, TQ - 1),
    (128, 1000, 8, TQ + 1), (96, 2, 8, 1), (30, 1, 3, 2 * TQ + 1), (260, 257, 3, TQ + 1),
]


@pytest.mark.parametrize("d,h,m,nq", TABLE_SHAPES)
@pytest.mark.parametrize("lsq", [True, False])
def test_tables(rq, d, h, m, nq, lsq):
    """d % 4 == 0 from an aligned pointer takes the 16-byte loads, anything else the scalar path -- also d % 4 == 0 from a
    codebook pointer offset by one float.  d = 260 runs three chunks of the staged query tile."""
    import torch
    from rayuela_jl_amd import device as rqd
    _, C, q, _ = awo.case(1, m, h, d, nq, 100 * d + h + m)
    ref = awo.tables(lsq, C, q).reshape(nq, m, h).view(np.uint32)
    ct, qt = _dev(C, q)
    assert np.array_equal(_bits(rqd.aq_lut_wide(ct, qt, lsq=lsq)), ref)
    flat = torch.empty(C.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = ct.reshape(-1)
    shifted = flat[1:].view(m, h, d)
    assert shifted.data_ptr() == flat.data_ptr() + 4 and shifted.is_contiguous()
    assert np.array_equal(_bits(rqd.aq_lut_wide(shifted, qt, lsq=lsq)), ref), "codebooks offset by one float"


# ---- tiers -----------------------------------------------------------------------------------------------------------------
TIERS = [  # m, h, d, queries per gather, table in LDS
    (8, 1024, 8, 4, True), (8, 1025, 8, 2, True), (4, 4097, 8, 1, True), (8, 4097, 4, 4, False), (1, 32767, 4, 1, True),
]


@pytest.mark.parametrize("m,h,d,qpg,in_lds", TIERS)
@pytest.mark.parametrize("lsq", [True, False])
def test_tiers(rq, m, h, d, qpg, in_lds, lsq):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    p = _lib.scan_wide_plan(m, h)
    assert (p["qpg"], bool(p["in_lds"])) == (qpg, in_lds)
    n, nq = 5003, p["qg"] + 1
    codes, C, q, nrm = awo.case(n, m, h, d, nq, h + m)
    T = awo.tables(lsq, C, q)
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    assert np.array_equal(_bits(rqd.aq_lut_wide(ct, qt, lsq=lsq)), T.reshape(nq, m, h).view(np.uint32)), "table bits"
    name = "adc_keys_h16_kernel<%d, %s%s>" % (qpg, "true" if in_lds else "false", ", true" if lsq else "")
    for k in (1, 100, n):
        d_, i_ = _scan(bt, ct, qt, k, nt if lsq else None)
        assert _kernel() == name
        _assert_same(d_, i_, awo.scan_tables(T, codes, k, nrm if lsq else None), (m, h, k))


# ---- k and n ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,h,d,n", [(3, 257, 5, 33), (5, 300, 8, 513), (3, 1000, 6, 70_001), (8, 257, 4, 70_001)])
@pytest.mark.parametrize("lsq", [True, False])
def test_k_eq_n_and_n_minus_1(rq, m, h, d, n, lsq):
    """Odd m: rows are 2-byte aligned only; every shape also runs from a codes pointer offset by one row."""
    nq = 3
    codes, C, q, nrm = awo.case(n + 1, m, h, d, nq, n + m + h)
    T = awo.tables(lsq, C, q)
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    for k in (n, n - 1):
        d_, i_ = _scan(bt[:n], ct, qt, k, nt[:n] if lsq else None)
        _assert_same(d_, i_, awo.scan_tables(T, codes[:n], k, nrm[:n] if lsq else None), (m, h, k))
        shifted = bt[1:]
        assert shifted.data_ptr() == bt.data_ptr() + 2 * m and shifted.is_contiguous()
        d_, i_ = _scan(shifted, ct, qt, k, nt[1:] if lsq else None)
        _assert_same(d_, i_, awo.scan_tables(T, codes[1:], k, nrm[1:] if lsq else None), (m, h, k, "offset by one row"))


# ---- h = 256: the byte scan's answer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lsq", [True, False])
def test_h256_equals_the_byte_scan(rq, lsq):
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, d, nq = 70_001, 8, 32, 5
    codes, C, q, nrm = awo.case(n, m, 256, d, nq, 256)
    b8, b16, ct, qt, nt = _dev(codes.astype(np.uint8), codes, C, q, nrm)
    cb = ct.view(m * 256, d)
    nt = nt if lsq else None
    for k in (100, 65537):
        d0, i0 = rqd.linscan_aq(b8, cb, qt, k, dbnorms=nt)
        d1, i1 = _scan(b16, ct, qt, k, nt)
        assert _kernel() == "adc_keys_h16_kernel<4, true%s>" % (", true" if lsq else "")
        assert torch.equal(i0, i1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32)), k
        k0 = rqd.linscan_aq(b8, cb, qt, k, dbnorms=nt, want_keys=True)
        k1 = _scan(b16, ct, qt, k, nt, want_keys=True)
        assert torch.equal(k0, k1), k


# ---- the norm add ----------------------------------------------------------------------------------------------------------
def test_norm_is_added_last_in_one_rounding(rq):
    """Integer tables of magnitude < 2^24 and norms of mixed sign and magnitude: (sum T) + norm, any other order rounds
    differently on some row.  The restatement's own sensitivity to the order is asserted, so the case cannot go blunt."""
    n, m, h, d, nq, k = 20_011, 4, 300, 3, 5, 20_011
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 61, integer=True)
    C *= np.float32(1031)
    T = awo.tables(True, C, q)
    first = np.zeros(n, dtype=np.float32) + nrm                        # the norm added first instead
    for j in range(m):
        first = first + T[0][h * j + codes[:, j].astype(np.int64)]
    assert (first != awo.distances(T[0], codes, nrm)).any()
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    d_, i_ = _scan(bt, ct, qt, k, nt)
    _assert_same(d_, i_, awo.scan_tables(T, codes, k, nrm), "mixed norms")
    # zero norms (+0 and -0): the sums of the LSQ tables alone, -0 sums included
    zeros = np.zeros(n, dtype=np.float32)
    zeros[::2] = -0.0
    d0, i0 = _scan(bt, ct, qt, k, _dev(zeros)[0])
    ref = awo.scan_tables(T, codes, k, None)
    _assert_same(d0, i0, ref, "zero norms")
    _assert_same(d0, i0, awo.scan_tables(T, codes, k, zeros), "zero norms through the norm add")


def test_all_rows_identical_lowest_ids(rq):
    n, m, h, d, nq = 20_000, 4, 300, 6, 5
    codes, C, q, _ = awo.case(1, m, h, d, nq, 5)
    bt, ct, qt = _dev(np.tile(codes, (n, 1)), C, q)
    nt = _dev(np.full(n, 2.5, dtype=np.float32))[0]
    for lsq in (True, False):
        for k in (1, 1000, n):
            d_, i_ = _scan(bt, ct, qt, k, nt if lsq else None)
            assert np.array_equal(_np(i_), np.tile(np.arange(k, dtype=np.int32), (nq, 1))), k
            assert np.all(_bits(d_) == _bits(d_)[:, :1])


def test_heavy_duplicates(rq):
    """Small-integer codebooks and queries, 4 code values per codebook, norms from {0, 1}: thousands of rows per distance."""
    import rayuela_jl_amd.synth as synth
    n, m, h, d, nq = 90_000, 4, 300, 4, 9
    _, C, q, _ = awo.case(1, m, h, d, nq, 8, integer=True)
    C, q = np.sign(C), np.sign(q)
    codes = ((synth.random_codes(n, m, seed=4) % 4).astype(np.int16) * 97)      # 0, 97, 194, 291: above 256 too
    nrm = (synth.random_codes(n, 1, seed=5)[:, 0] % 2).astype(np.float32)
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    for lsq in (True, False):
        T = awo.tables(lsq, C, q)
        for k in (10, 70_000, n):
            d_, i_ = _scan(bt, ct, qt, k, nt if lsq else None)
            _assert_same(d_, i_, awo.scan_tables(T, codes, k, nrm if lsq else None), (lsq, k))


# ---- non-finite inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lsq", [True, False])
def test_non_finite_inputs(rq, lsq):
    n, m, h, d, nq = 4001, 4, 700, 6, 10
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 77)
    clean = [0, 2, 4, 5, 7, 8, 9]
    nf.put_bits(q, (1, 3), nf.NAN_NEG)          # a NaN query: all padding
    q[3, 0] = np.inf                            # LSQ: -2 * Inf * c is -Inf or +Inf by the sign of c, NaN where both meet a row
    q[6, 5] = -np.inf
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    nn, nt_ = (nrm, nt) if lsq else (None, None)
    for k in (1, 100, n):
        ref = awo.scan(codes, C, q, k, nn)
        d_, i_ = _scan(bt, ct, qt, k, nt_)
        _assert_same(d_, i_, ref, ("queries", k))
        assert np.all(_np(i_).view(np.uint32)[1] == 0xFFFFFFFF) and np.all(_bits(d_)[1] == nf.PAD_BITS)
        d2, i2 = _scan(bt, ct, _dev(q[clean])[0], k, nt_)                # the clean queries are unaffected
        assert np.array_equal(_np(i2), _np(i_)[clean]) and np.array_equal(_bits(d2), _bits(d_)[clean])
    # an Inf and a NaN codeword: rows with the NaN codeword drop out of every list, which then ends in padding
    C2 = C.copy()
    C2[1, 650, 0] = np.inf
    nf.put_bits(C2, (2, 300, 1), nf.NAN_POS)
    nbad = int((codes[:, 2] == 300).sum())
    assert nbad > 0 and (codes[:, 1] == 650).any()
    c2, q2 = _dev(C2, q[clean])
    for k in (100, n):
        d_, i_ = _scan(bt, c2, q2, k, nt_)
        _assert_same(d_, i_, awo.scan(codes, C2, q[clean], k, nn), ("codewords", k))
    assert np.all(_np(i_).view(np.uint32)[:, n - nbad:] == 0xFFFFFFFF)
    if lsq:      # NaN (either sign), +Inf and -Inf norms: row data like the codes
        nrm2 = nrm.copy()
        nf.put_bits(nrm2, 7, nf.NAN_POS)
        nf.put_bits(nrm2, 8, nf.NAN_NEG)
        nrm2[100], nrm2[200], nrm2[n - 1] = np.inf, -np.inf, -np.inf
        n2 = _dev(nrm2)[0]
        qc = _dev(q[clean])[0]
        for k in (1, 3, n):
            d_, i_ = _scan(bt, ct, qc, k, n2)
            _assert_same(d_, i_, awo.scan(codes, C, q[clean], k, nrm2), ("dbnorms", k))
        ids = _np(i_).view(np.uint32)
        assert np.all(ids[:, :2] == [200, n - 1]) and np.all(ids[:, n - 3] == 100) and np.all(ids[:, n - 2:] == 0xFFFFFFFF)


# ---- codes outside [0, h) --------------------------------------------------------------------------------------------------
def _bad_codes(n, m, h, seed):
    codes, C, q, nrm = awo.case(n, m, h, 4, 6, seed)
    bad = {17: h, 1200: 32767, n - 1: -1}
    for col, (row, value) in enumerate(bad.items()):
        codes[row, col % m] = value
    return codes, C, q, nrm, sorted(bad)


@pytest.mark.parametrize("lsq", [True, False])
def test_device_entry_never_returns_a_row_with_a_bad_code(rq, lsq):
    n, m, h = 3001, 3, 1000
    codes, C, q, nrm, bad = _bad_codes(n, m, h, 9)
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    for k in (1, 50, n):
        d_, i_ = _scan(bt, ct, qt, k, nt if lsq else None)
        _assert_same(d_, i_, awo.scan(codes, C, q, k, nrm if lsq else None), k)
    ids = _np(i_).view(np.uint32)
    assert np.all(ids[:, n - 3:] == 0xFFFFFFFF) and np.all(_bits(d_)[:, n - 3:] == nf.PAD_BITS)
    for r in range(ids.shape[0]):
        assert np.array_equal(np.sort(ids[r, :n - 3]), np.setdiff1d(np.arange(n), bad))


def _host_calls(L, dists, ids, codes, C, q, nrm, cbn, R, n, nq, m, h, d, k, code_base, id_base):
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    return {
        "lsq": lambda: L.rq_linscan_lsq_wide(p(dists), p(ids), p(codes), p(q), p(C), p(nrm), p(R), n, nq, m, h, d, k, code_base,
                                             id_base),
        "cq": lambda: L.rq_linscan_cq_wide(p(dists), p(ids), p(codes), p(q), p(C), n, nq, m, h, d, k, code_base, id_base),
        "cbnorms": lambda: L.rq_linscan_lsq_cbnorms_wide(p(dists), p(ids), p(codes), p(q), p(C), p(cbn),
                                                         0 if cbn is None else cbn.shape[0], p(R), n, nq, m, h, d, k, code_base,
                                                         id_base),
    }


@pytest.mark.parametrize("code_base", [0, 1])
def test_host_entries_refuse_bad_codes(rq, code_base):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    n, m, h, k = 3001, 3, 1000, 10
    codes, C, q, nrm, bad = _bad_codes(n, m, h, 10)
    codes = (codes.astype(np.int32) + code_base).astype(np.int16)      # 32767 + 1 wraps to -32768: bad either way
    nq, d = q.shape
    dists = np.full((nq, k), -7.0, dtype=np.float32)
    ids = np.full((nq, k), 0xA5A5A5A5, dtype=np.uint32)
    cbn = np.linspace(0, 9, 300).astype(np.float32)
    for name, call in _host_calls(L, dists, ids, codes, C, q, nrm, cbn, None, n, nq, m, h, d, k, code_base, 1).items():
        rc = call()
        msg = L.rq_last_error().decode()
        assert rc == RQ_EINVAL and "row %d " % bad[0] in msg, (name, rc, msg)
    norms = np.full(n, -7.0, dtype=np.float32)
    nc = np.full(n, 0x5A5A, dtype=np.int16)
    cbo = np.full(300, -7.0, dtype=np.float32)
    assert L.rq_aq_norms_wide(norms.ctypes.data, codes.ctypes.data, C.ctypes.data, n, d, m, h, code_base) == RQ_EINVAL
    assert "row %d " % bad[0] in L.rq_last_error().decode()
    assert L.rq_quantize_norms_wide(nc.ctypes.data, norms.ctypes.data, codes.ctypes.data, C.ctypes.data, cbn.ctypes.data, n, d, m,
                                    h, 300, code_base) == RQ_EINVAL
    assert L.rq_get_norms_codebook_wide(nc.ctypes.data, cbo.ctypes.data, norms.ctypes.data, codes.ctypes.data, C.ctypes.data, n, d,
                                        m, h, 300, 3, 1, code_base) == RQ_EINVAL
    assert np.all(dists == -7.0) and np.all(ids == 0xA5A5A5A5)
    assert np.all(norms == -7.0) and np.all(nc == 0x5A5A) and np.all(cbo == -7.0)


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_keys_id_offset_id_base_and_shard_merge(rq):
    import torch
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    n, m, h, d, nq, k = 30_011, 5, 600, 6, 7, 300
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 12)
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    off = 2 ** 32 - n - 2
    bits, ids, keys = awo.scan(codes, C, q, k, nrm, id_base=1, id_offset=off)
    d_, i_ = _scan(bt, ct, qt, k, nt, id_offset=off, id_base=1)
    _assert_same(d_, i_, (bits, ids), "id_offset + id_base")
    kk = _scan(bt, ct, qt, k, nt, id_offset=off, id_base=1, want_keys=True)
    assert np.array_equal(_np(kk).view(np.uint64), keys), "keys stay zero-based"
    d3 = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    i3 = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    k3 = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().rq_dev_linscan_aq_wide(d3.data_ptr(), i3.data_ptr(), k3.data_ptr(), bt.data_ptr(), ct.data_ptr(),
                                                 qt.data_ptr(), nt.data_ptr(), n, nq, m, h, d, k, 1, off, 1, rqd._stream()))
    assert torch.equal(d3.view(torch.int32), d_.view(torch.int32)) and torch.equal(i3, i_) and torch.equal(k3, kk)
    cut = 12_345                                       # two row shards, merged by rq_dev_merge_topk, equal the single scan
    d0, i0 = _scan(bt, ct, qt, k, nt)
    ka = _scan(bt[:cut], ct, qt, k, nt[:cut], want_keys=True)
    kb = _scan(bt[cut:], ct, qt, k, nt[cut:], id_offset=cut, want_keys=True)
    dm, im = rqd.merge_topk(torch.stack([ka, kb], dim=1).contiguous(), k)
    assert torch.equal(im, i0) and torch.equal(dm.view(torch.int32), d0.view(torch.int32))


def test_several_batches_equal_one_query_at_a_time(rq):
    """n = 1e6, k = 10: at most `batch` = usable scratch / 8 n queries fit one batch; nq = 2 batch + 7 runs three batches at
    least.  The norms are quantised ones, dbnorms = cbn[code]: the norm add is then one more table look-up, and the certificate
    of tests/scan_wide_oracle.py covers it as an (m + 1)-th codebook whose table is cbn for every query."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, h, d, k = 1_000_000, 4, 1024, 16, 10
    batch = BULK_USABLE_BYTES // (8 * n)
    assert 16 <= batch < 1000, batch
    nq = 2 * batch + 7
    _, C, q, _ = awo.case(1, m, h, d, nq, 31)
    ct, qt = _dev(C, q)
    gen = torch.Generator("cuda").manual_seed(31)
    bt = torch.randint(0, h, (n, m), dtype=torch.int16, device="cuda", generator=gen)
    nc = torch.randint(0, h, (n, 1), dtype=torch.int16, device="cuda", generator=gen)
    cbn = torch.rand(h, device="cuda", generator=gen) * 40
    nt = cbn[nc[:, 0].long()].contiguous()
    d1, i1 = _scan(bt, ct, qt, k, nt)
    for r in range(nq):
        d2, i2 = _scan(bt, ct, qt[r:r + 1].contiguous(), k, nt)
        assert torch.equal(i2[0], i1[r]) and torch.equal(d2[0].view(torch.int32), d1[r].view(torch.int32)), r
    lut = torch.cat([rqd.aq_lut_wide(ct, qt), cbn[None, None, :].expand(nq, 1, h)], dim=1).contiguous()
    assert swo.certify(d1, i1, k, lut, torch.cat([bt, nc], dim=1), n, chunk=1 << 19) == nq


# ---- host path -------------------------------------------------------------------------------------------------------------
def test_host_mirrors(rq, oracle):
    n, m, h, d, nq, k = 20_000, 4, 1000, 12, 11, 500
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 21)
    Cl = [C[j] for j in range(m)]
    ref = awo.scan(codes, C, q, k, nrm, id_base=1)
    for B in (codes.view(np.uint16), codes, codes.astype(np.int32) + 1, (codes + 1).astype(np.int64)):
        for R in (None, np.eye(d, dtype=np.float32)):
            dd, ii = rq.linscan_lsq_u16(B, q, Cl, nrm, R, k)
            assert awo.same(dd, ii, ref), (B.dtype, R is None)
    dd, ii = rq.linscan_cq_u16(codes, q, Cl, k)
    assert awo.same(dd, ii, awo.scan(codes, C, q, k, None, id_base=1))
    R = np.linalg.qr(np.random.default_rng(4).standard_normal((d, d)))[0].astype(np.float32)
    dd, ii = rq.linscan_lsq_u16(codes, q, Cl, nrm, R, k)
    assert awo.same(dd, ii, awo.scan(codes, C, oracle.rotate_T(R, q), k, nrm, id_base=1))
    # the norms codebook form: equal to the scan on cbnorms[quantize(norms)]
    cbn = np.random.default_rng(5).permutation(np.linspace(0, 60, 700)).astype(np.float32)
    norms = no.aq_norms(codes, C)
    dbn = cbn[awo.quantize(norms, cbn)]
    d1, i1 = rq.linscan_lsq_cbnorms_u16(codes, q, Cl, cbn, R, k)
    d2, i2 = rq.linscan_lsq_u16(codes, q, Cl, dbn, R, k)
    assert np.array_equal(i1, i2) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
    assert awo.same(d1, i1, awo.scan(codes, C, oracle.rotate_T(R, q), k, dbn, id_base=1))


def test_host_call_streams_results_in_query_chunks(rq):
    """nq * k * 8 bytes pass BULK_HOST_RESULT_BYTES: bulk_fetch brings the results back in two query chunks."""
    n, m, h, d, nq = 33_000, 2, 300, 4, 1100
    k = n
    assert nq * k * 8 > BULK_HOST_RESULT_BYTES and BULK_HOST_RESULT_BYTES // (8 * k) < nq
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 22)
    dd, ii = rq.linscan_lsq_u16(codes, q, [C[j] for j in range(m)], nrm, None, k)
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    d0, i0 = _scan(bt, ct, qt, k, nt, id_base=1)
    assert np.array_equal(ii, _np(i0).view(np.uint32)) and np.array_equal(dd.view(np.uint32), _bits(d0))
    chunk = BULK_HOST_RESULT_BYTES // (8 * k)
    some = [0, chunk - 1, chunk, nq - 1]
    assert awo.same(dd[some], ii[some], awo.scan(codes, C, q[some], k, nrm, id_base=1))


# ---- the norm entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,h,n", [(1, 64, 32767, 1027), (63, 1, 257, 1), (64, 5, 257, 3), (65, 64, 1000, 4), (130, 5, 1000, 5),
                                     (96, 8, 1000, 1027)])
def test_aq_norms_wide(rq, d, m, h, n):
    from rayuela_jl_amd import device as rqd
    codes, C, _, _ = awo.case(n, m, h, d, 1, d + m + h + n)
    want = no.aq_norms(codes, C)
    bt, ct = _dev(codes, C)
    assert np.array_equal(_bits(rqd.aq_norms_wide(bt, ct)), want.view(np.uint32))
    assert np.array_equal(rq.utils.aq_norms(codes.astype(np.int32) + 1, [C[j] for j in range(m)]).view(np.uint32),
                          want.view(np.uint32))


def test_aq_norms_wide_equals_the_byte_entry_at_h256(rq):
    import torch
    from rayuela_jl_amd import device as rqd
    for (n, d, m, h) in ((1007, 96, 16, 256), (65, 6, 7, 255), (513, 130, 3, 2)):
        codes, C = no.norm_case(n, d, m, h)
        b8, b16, ct = _dev(codes, codes.astype(np.int16), C)
        assert torch.equal(rqd.aq_norms(b8, ct).view(torch.int32), rqd.aq_norms_wide(b16, ct).view(torch.int32)), (n, d, m, h)


@pytest.mark.parametrize("hn", [1, 257, 1000, 32767])
def test_quantize_norms_wide(rq, hn):
    """An unsorted table with every value twice (exact ties: the first index wins) and norms on and between its values."""
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(hn)
    vals = np.arange(0, 4 * ((hn + 1) // 2), 4)[: (hn + 1) // 2]
    cb = rng.permutation(np.concatenate([vals, vals])[:hn]).astype(np.float32)
    norms = rng.integers(-8, 4 * len(vals) + 8, 2003).astype(np.float32)          # multiples of 4 + 2: exact midpoints
    want = awo.quantize(norms, cb)
    nt, cbt = _dev(norms, cb)
    codes, dbn = rqd.quantize_norms_wide(nt, cbt)
    assert np.array_equal(_np(codes), want) and np.array_equal(_bits(dbn), cb[want].view(np.uint32))
    head = cbt[:min(hn, 256)].contiguous()            # at hn <= 256: the byte entry's bits, widened
    c8, d8 = rqd.quantize_norms(nt, head)
    cw, dw = rqd.quantize_norms_wide(nt, head)
    assert np.array_equal(_np(c8).astype(np.int16), _np(cw)) and np.array_equal(_bits(d8), _bits(dw))


def test_host_norm_entries(rq):
    """rq_quantize_norms_wide and rq_get_norms_codebook_wide through utils: the codebook and assignments are those of
    rq_train_pq_wide(d = 1, m = 1, h = hn) on the same norms, niter and seed."""
    n, m, h, d = 4096, 2, 300, 16
    codes, C, _, _ = awo.case(n, m, h, d, 1, 71)
    Cl = [C[j] for j in range(m)]
    B1 = codes + np.int16(1)
    norms = no.aq_norms(codes, C)
    nB, cbn = rq.utils.get_norms_codebook(B1, Cl, niter=7, seed=3)
    Cn, Bn, _ = rq.train_pq(np.ascontiguousarray(norms.reshape(-1, 1)), 1, h, niter=7, seed=3)
    assert np.array_equal(cbn.view(np.uint32), Cn[0][:, 0].view(np.uint32)) and np.array_equal(nB, Bn[:, 0].astype(np.int64))
    assert nB.max() > 256
    qB, qn = rq.utils.quantize_norms(B1, Cl, cbn)
    assert np.array_equal(qn.view(np.uint32), norms.view(np.uint32))
    assert qB.dtype == np.int16 and np.array_equal(qB.astype(np.int64) - 1, awo.quantize(norms, cbn))


def test_aq_norms_wide_past_4_gib_of_codes(rq):
    """d = 2, m = 16, n = 134 300 000: the codes pass 2^32 bytes.  Every norm is recomputed in torch: CB by adds in codebook
    order, then fl(fl(CB0^2) + fl(CB1^2)) -- with d = 2 the butterfly adds zeros until its last step."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, h, d = 134_300_000, 16, 1000, 2
    assert n * m * 2 > 2 ** 32
    C = torch.randn((m, h, d), device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    bt = torch.randint(0, h, (n, m), dtype=torch.int16, device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    got = rqd.aq_norms_wide(bt, C)
    chunk = 1 << 23
    for r0 in range(0, n, chunk):
        b = bt[r0:r0 + chunk].long()
        cb = torch.zeros((b.shape[0], d), device="cuda")
        for j in range(m):
            cb = cb + C[j][b[:, j]]
        sq = cb * cb
        assert torch.equal((sq[:, 0] + sq[:, 1]).view(torch.int32), got[r0:r0 + chunk].view(torch.int32)), r0
    del bt
    torch.cuda.empty_cache()


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norms", ["host", "device"])
def test_end_to_end_rvq_query_base(rq, monkeypatch, norms):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import Linscan, experiments
    n, d, m, h, nq, knn = 4096, 16, 2, 300, 20, 50
    Xt = synth.sift_like(n, d, seed=3)
    Xq = np.ascontiguousarray(Xt[:nq])
    gt = np.arange(1, nq + 1)
    seen = []
    real = Linscan.linscan_lsq_u16

    def spy(B, X, C, dbnorms, R, k):
        out = real(B, X, C, dbnorms, R, k)
        seen.append((np.asarray(B), np.asarray(dbnorms), out))
        return out
    monkeypatch.setattr(Linscan, "linscan_lsq_u16", spy)
    C, B, err, recall = experiments.experiment_rvq_query_base(Xt, Xq, gt, m, h, niter=5, knn=knn, seed=1, norms=norms)
    assert len(seen) == 1 and B.dtype == np.int16 and B.max() > 256 and B.min() >= 1
    Bs, dbn, (dists, idx) = seen[0]
    assert np.array_equal(Bs, B)
    ref = awo.scan(B - np.int16(1), np.stack(C), Xq, knn, dbn, id_base=1)
    assert awo.same(dists, idx, ref)
    assert recall.shape == (knn,) and np.all(np.diff(recall) >= 0) and 0.0 <= recall[0] and recall[-1] <= 1.0


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(rq):
    import torch
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    L = _lib.lib()
    n, m, h, d, nq, k = 1000, 4, 300, 6, 3, 10
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 51)
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    dd = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    ii = torch.full((nq, k), -3, dtype=torch.int32, device="cuda")
    kk = torch.full((nq, k), -5, dtype=torch.int64, device="cuda")
    lut = torch.full((nq, m, h), -7.0, dtype=torch.float32, device="cuda")
    good = dict(dists=dd.data_ptr(), ids=ii.data_ptr(), keys=kk.data_ptr(), codes=bt.data_ptr(), codebooks=ct.data_ptr(),
                queries=qt.data_ptr(), dbnorms=nt.data_ptr(), n=n, nq=nq, m=m, h=h, d=d, k=k, lut_mode=1, id_offset=0, id_base=0)

    def dev(**patch):
        a = dict(good, **patch)
        return L.rq_dev_linscan_aq_wide(a["dists"], a["ids"], a["keys"], a["codes"], a["codebooks"], a["queries"], a["dbnorms"],
                                        a["n"], a["nq"], a["m"], a["h"], a["d"], a["k"], a["lut_mode"], a["id_offset"],
                                        a["id_base"], rqd._stream())

    assert dev(nq=0) == 0 and dev(nq=-1) == 0
    for patch in (dict(codes=None), dict(codebooks=None), dict(queries=None), dict(dbnorms=None), dict(keys=None, dists=None),
                  dict(keys=None, ids=None), dict(id_base=2), dict(id_base=-1), dict(d=0), dict(k=0), dict(k=n + 1), dict(n=0),
                  dict(n=2 ** 31), dict(id_offset=2 ** 32 - n + 1), dict(codes=bt.data_ptr() + 1), dict(lut_mode=0),
                  dict(lut_mode=3)):
        assert dev(**patch) == RQ_EINVAL, patch
    for patch in (dict(h=0), dict(h=32768), dict(m=0), dict(m=33)):
        assert dev(**patch) == RQ_EUNSUPPORTED, patch
    s = rqd._stream()
    assert L.rq_dev_aq_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), 0, m, h, d, 1, s) == 0
    assert L.rq_dev_aq_lut_wide(None, ct.data_ptr(), qt.data_ptr(), nq, m, h, d, 1, s) == RQ_EINVAL
    assert L.rq_dev_aq_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), nq, m, h, 0, 1, s) == RQ_EINVAL
    assert L.rq_dev_aq_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), nq, m, h, d, 0, s) == RQ_EINVAL
    assert L.rq_dev_aq_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), nq, 33, h, d, 1, s) == RQ_EUNSUPPORTED
    assert L.rq_dev_aq_lut_wide(lut.data_ptr(), ct.data_ptr(), qt.data_ptr(), nq, m, 32768, d, 1, s) == RQ_EUNSUPPORTED
    # the device norm entries
    no_ = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    nc = torch.full((n,), -3, dtype=torch.int16, device="cuda")
    for args in ((None, bt.data_ptr(), ct.data_ptr(), n, d, m, h), (no_.data_ptr(), None, ct.data_ptr(), n, d, m, h),
                 (no_.data_ptr(), bt.data_ptr(), None, n, d, m, h), (no_.data_ptr(), bt.data_ptr(), ct.data_ptr(), n, d, 65, h),
                 (no_.data_ptr(), bt.data_ptr(), ct.data_ptr(), n, d, m, 1), (no_.data_ptr(), bt.data_ptr(), ct.data_ptr(), n, d, m, 32768),
                 (no_.data_ptr(), bt.data_ptr(), ct.data_ptr(), n, 0, m, h), (no_.data_ptr(), bt.data_ptr(), ct.data_ptr(), -1, d, m, h),
                 (no_.data_ptr(), bt.data_ptr(), ct.data_ptr(), n, d, m, h - 1)):       # h - 1: code h - 1 is out of range
        assert L.rq_dev_aq_norms_wide(*args, s) == RQ_EINVAL, args
    for hn in (0, -1, 32768):
        assert L.rq_dev_quantize_norms_wide(nc.data_ptr(), no_.data_ptr(), nt.data_ptr(), nt.data_ptr(), n, hn, s) == RQ_EINVAL
    assert L.rq_dev_quantize_norms_wide(None, no_.data_ptr(), nt.data_ptr(), nt.data_ptr(), n, 16, s) == RQ_EINVAL
    assert L.rq_dev_quantize_norms_wide(nc.data_ptr(), no_.data_ptr(), nt.data_ptr(), None, n, 16, s) == RQ_EINVAL
    torch.cuda.synchronize()
    assert bool((dd == -7.0).all()) and bool((ii == -3).all()) and bool((kk == -5).all()) and bool((lut == -7.0).all())
    assert bool((no_ == -7.0).all()) and bool((nc == -3).all())

    # the host entries
    hd = np.full((nq, k), -7.0, dtype=np.float32)
    hi = np.full((nq, k), 0xA5A5A5A5, dtype=np.uint32)
    cbn = np.linspace(0, 9, 30).astype(np.float32)
    base = dict(dists=hd, ids=hi, codes=codes, C=C, q=q, nrm=nrm, cbn=cbn, R=None, n=n, nq=nq, m=m, h=h, d=d, k=k, code_base=0,
                id_base=1)

    def host(name, **patch):
        a = dict(base, **patch)
        return _host_calls(L, a["dists"], a["ids"], a["codes"], a["C"], a["q"], a["nrm"], a["cbn"], a["R"], a["n"], a["nq"],
                           a["m"], a["h"], a["d"], a["k"], a["code_base"], a["id_base"])[name]()

    for name in ("lsq", "cq", "cbnorms"):
        assert host(name, nq=0) == 0
        for patch in (dict(dists=None), dict(ids=None), dict(codes=None), dict(C=None), dict(q=None), dict(code_base=2),
                      dict(code_base=-1), dict(id_base=2), dict(d=0), dict(k=0), dict(k=n + 1), dict(n=0), dict(n=2 ** 31)):
            assert host(name, **patch) == RQ_EINVAL, (name, patch)
        for patch in (dict(h=0), dict(h=32768), dict(m=0), dict(m=33)):
            assert host(name, **patch) == RQ_EUNSUPPORTED, (name, patch)
    assert host("lsq", nrm=None) == RQ_EINVAL and host("cbnorms", cbn=None) == RQ_EINVAL
    assert host("cbnorms", h=1, codes=np.zeros_like(codes)) == RQ_EINVAL          # the norms need h >= 2
    assert np.all(hd == -7.0) and np.all(hi == 0xA5A5A5A5)
