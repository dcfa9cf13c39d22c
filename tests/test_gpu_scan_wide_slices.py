"""GPU: row slices in the scans over 16-bit codes (rq_dev_linscan_wide, rq_dev_linscan_aq_wide).  A base
whose keys do not fit the scratch budget for one query goes through in slices whose sorted lists are folded into a running list;
the test hook rq_test_scan_wide_slice_rows forces a slice length so that the fold runs on small bases.  The expected value is
the same call without the hook (pinned to the oracle by tests/test_gpu_scan_wide.py and tests/test_gpu_aq_wide.py), bit for bit
on ids, distances and keys, plus tests/scan_wide_oracle.py directly on one shape."""
import contextlib

import numpy as np
import pytest

import aq_wide_oracle as awo
import nonfinite_ref as nf
import scan_wide_oracle as swo

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _kernel():
    from rayuela_jl_amd import _lib
    return (_lib.lib().rq_last_scan_kernel() or b"").decode()


@contextlib.contextmanager
def sliced(rows):
    from rayuela_jl_amd import _lib
    prev = _lib.lib().rq_test_scan_wide_slice_rows(rows)
    try:
        yield
    finally:
        _lib.lib().rq_test_scan_wide_slice_rows(prev)


def _data(n, m, h, sub, nq, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((m, h, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    return codes, centers, queries


def _equal(got, ref, what):
    import torch
    (d, i), (d0, i0) = got, ref
    assert torch.equal(i, i0), (what, "ids")
    assert torch.equal(d.view(torch.int32), d0.view(torch.int32)), (what, "distance bits")


N, M, H, SUB, NQ, K = 20_001, 8, 1024, 2, 5, 100


@pytest.fixture(scope="module")
def plain(rq):
    """The base of the plain-slicing tests, resident, with its unsliced answer."""
    from rayuela_jl_amd import device as rqd
    codes, centers, queries = _data(N, M, H, SUB, NQ, seed=23)
    bt, ct, qt = _dev(codes, centers, queries)
    return dict(host=(codes, centers, queries), dev=(bt, ct, qt), ref=rqd.linscan_wide(bt, ct, qt, K), kernel=_kernel())


@pytest.mark.parametrize("rows", [257, 4096, 20_000, 20_001])
def test_plain_slicing(rq, plain, rows):
    """78 slices with a short last one, 5 slices, a last slice of ONE row, and one slice through the sliced path."""
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    bt, ct, qt = plain["dev"]
    with sliced(rows):
        p = _lib.scan_wide_slices(N, NQ, M, H, K)
        assert (p["rows"], p["slices"], p["forced"]) == (rows, -(-N // rows), 1)
        got = rqd.linscan_wide(bt, ct, qt, K)
        assert _kernel() == plain["kernel"]
        _equal(got, plain["ref"], rows)
    assert _lib.scan_wide_slices(N, NQ, M, H, K)["forced"] == 0


def test_sliced_against_the_oracle(rq, oracle, plain):
    from rayuela_jl_amd import device as rqd
    codes, centers, queries = plain["host"]
    bt, ct, qt = plain["dev"]
    ref = swo.scan(oracle, codes, centers, queries, K)
    with sliced(4096):
        d, i = rqd.linscan_wide(bt, ct, qt, K)
    assert swo.same(_np(d), _np(i), ref), swo.first_difference(_np(d), _np(i), ref)


def test_outputs_keys_id_offset_id_base(rq, plain):
    """The slice offset reaches the ids: keys carry id_offset + global row, ids add id_base on top."""
    import torch
    from rayuela_jl_amd import device as rqd
    bt, ct, qt = plain["dev"]
    off = 2 ** 31 + 5
    d0, i0 = rqd.linscan_wide(bt, ct, qt, K, id_offset=off, id_base=1)
    k0 = rqd.linscan_wide(bt, ct, qt, K, id_offset=off, want_keys=True)
    with sliced(4096):
        d1, i1 = rqd.linscan_wide(bt, ct, qt, K, id_offset=off, id_base=1)
        k1 = rqd.linscan_wide(bt, ct, qt, K, id_offset=off, want_keys=True)
    _equal((d1, i1), (d0, i0), "id_offset")
    assert torch.equal(k1, k0)
    rows = (_np(k1).view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.array_equal(rows + 1, _np(i1).view(np.uint32).astype(np.int64))
    assert np.array_equal(rows - off, _np(plain["ref"][1]).astype(np.int64))


@pytest.mark.parametrize("k", [700, 1000])
def test_k_larger_than_a_slice(rq, oracle, k):
    """Slices of 300 rows (the last of 100) pad their lists with KEY_MAX up to k."""
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq = 1000, 4, 300, 2, 5
    codes, centers, queries = _data(n, m, h, sub, nq, seed=k)
    bt, ct, qt = _dev(codes, centers, queries)
    ref = rqd.linscan_wide(bt, ct, qt, k)
    with sliced(300):
        got = rqd.linscan_wide(bt, ct, qt, k)
    _equal(got, ref, k)
    want = swo.scan(oracle, codes, centers, queries, k)
    assert swo.same(_np(got[0]), _np(got[1]), want)


def test_all_rows_identical_lowest_ids(rq):
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq = 5000, 4, 300, 2, 5
    codes, centers, queries = _data(1, m, h, sub, nq, seed=5)
    bt, ct, qt = _dev(np.tile(codes, (n, 1)), centers, queries)
    for k in (1, 1000, n):
        with sliced(777):
            d, i = rqd.linscan_wide(bt, ct, qt, k)
        assert np.array_equal(_np(i), np.tile(np.arange(k, dtype=np.int32), (nq, 1))), k
        assert np.all(_np(d).view(np.uint32) == _np(d).view(np.uint32)[:, :1])


def test_nan_tables_and_bad_codes_end_in_padding(rq):
    """Rows under a NaN codeword and rows with a code outside [0, h) are never returned: lists of k = n end in the padding pair,
    exactly as many entries as there are such rows; a NaN query gives padding only."""
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq = 4001, 4, 700, 2, 6
    codes, centers, queries = _data(n, m, h, sub, nq, seed=77)
    nf.put_bits(centers, (2, 300, 1), nf.NAN_POS)
    nf.put_bits(queries, (1, 3), nf.NAN_NEG)
    codes[17, 0], codes[1200, 1], codes[n - 1, 3] = h, 32767, -1       # first, middle and last slice
    dropped = int(((codes[:, 2] == 300) | (codes < 0).any(1) | (codes >= h).any(1)).sum())
    assert dropped > 3
    bt, ct, qt = _dev(codes, centers, queries)
    for k in (100, n):
        ref = rqd.linscan_wide(bt, ct, qt, k)
        with sliced(1000):
            got = rqd.linscan_wide(bt, ct, qt, k)
        _equal(got, ref, k)
        want = swo.scan_tables(swo.direct_tables(centers, queries), codes, k)
        assert swo.same(_np(got[0]), _np(got[1]), want), k
    ids, bits = _np(got[1]).view(np.uint32), _np(got[0]).view(np.uint32)
    clean = [0, 2, 3, 4, 5]
    assert np.all(ids[clean][:, n - dropped:] == 0xFFFFFFFF) and np.all(bits[clean][:, n - dropped:] == nf.PAD_BITS)
    assert np.all(ids[clean][:, :n - dropped] < n)
    assert np.all(ids[1] == 0xFFFFFFFF) and np.all(bits[1] == nf.PAD_BITS)
    for bad_row in (17, 1200, n - 1):
        assert not (ids[clean] == bad_row).any()


@pytest.mark.parametrize("lsq", [True, False])
def test_lsq_and_cq(rq, lsq):
    """LSQ adds dbnorms[row]: the slice offset has to reach the norms.  One NaN norm in the second slice drops exactly that
    row."""
    from rayuela_jl_amd import device as rqd
    n, m, h, d, nq = 5003, 8, 1024, 8, 5
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 4)
    nan_row = 1500 + 7
    nf.put_bits(nrm, (nan_row,), nf.NAN_POS)
    bt, ct, qt, nt = _dev(codes, C, q, nrm)
    norms = nt if lsq else None
    for k in (100, n):
        ref = rqd.linscan_aq_wide(bt, ct, qt, k, dbnorms=norms)
        name = _kernel()
        with sliced(1500):
            got = rqd.linscan_aq_wide(bt, ct, qt, k, dbnorms=norms)
            assert _kernel() == name == "adc_keys_h16_kernel<4, true%s>" % (", true" if lsq else "")
        _equal(got, ref, (lsq, k))
        want = awo.scan_tables(awo.tables(lsq, C, q), codes, k, nrm if lsq else None)
        assert awo.same(_np(got[0]), _np(got[1]), want), (lsq, k)
    ids = _np(got[1]).view(np.uint32)
    assert (ids == nan_row).any() == (not lsq)
    if lsq:
        assert np.all(ids[:, n - 1] == 0xFFFFFFFF) and np.all(ids[:, :n - 1] < n)


@pytest.mark.parametrize("lsq", [None, True])
def test_global_table_tier(rq, lsq):
    """m = 16, h = 4096: the table of a query group stays in global memory."""
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    n, m, h, nq, k = 5003, 16, 4096, 5, 100
    assert not _lib.scan_wide_plan(m, h)["in_lds"]
    if lsq is None:
        codes, centers, queries = _data(n, m, h, 2, nq, seed=16)
        bt, ct, qt = _dev(codes, centers, queries)
        scan = lambda: rqd.linscan_wide(bt, ct, qt, k)                                   # noqa: E731
    else:
        codes, C, q, nrm = awo.case(n, m, h, 4, nq, 16)
        bt, ct, qt, nt = _dev(codes, C, q, nrm)
        scan = lambda: rqd.linscan_aq_wide(bt, ct, qt, k, dbnorms=nt)                    # noqa: E731
    ref = scan()
    with sliced(2000):
        got = scan()
        assert _kernel().startswith("adc_keys_h16_kernel<4, false")
    _equal(got, ref, lsq)


def test_several_query_batches(rq):
    """nq = 9: three query groups, the last ragged; against the unsliced call and against one query at a time."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, h, sub, nq, k = 3001, 8, 1024, 2, 9, 50
    codes, centers, queries = _data(n, m, h, sub, nq, seed=9)
    bt, ct, qt = _dev(codes, centers, queries)
    ref = rqd.linscan_wide(bt, ct, qt, k)
    with sliced(800):
        got = rqd.linscan_wide(bt, ct, qt, k)
        ones = [rqd.linscan_wide(bt, ct, qt[j:j + 1], k) for j in range(nq)]
    _equal(got, ref, "batch")
    _equal((torch.cat([o[0] for o in ones]), torch.cat([o[1] for o in ones])), ref, "one query at a time")


def test_no_launch_change_without_the_hook(rq, oracle, plain):
    """A call that fits the budget is one slice: the kernel and the answer of before."""
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    assert _lib.lib().rq_test_scan_wide_slice_rows(0) == 0
    codes, centers, queries = plain["host"]
    bt, ct, qt = plain["dev"]
    p = _lib.scan_wide_slices(N, NQ, M, H, K)
    assert (p["rows"], p["slices"], p["batch"], p["forced"]) == (N, 1, NQ, 0)
    d, i = rqd.linscan_wide(bt, ct, qt, K)
    assert _kernel() == "adc_keys_h16_kernel<4, true>"
    _equal((d, i), plain["ref"], "again")
    ref = swo.scan(oracle, codes, centers, queries, K)
    assert swo.same(_np(d), _np(i), ref)
