"""GPU: LSQ encoding over 16-bit codes (rq_encode_icm_wide / encode_icm_u16 and the mirrors past 256 codewords per codebook),
bit for bit against the CPU restatement tests/icm_wide_oracle.py, against the byte entry at h <= 256, and against itself under
everything the contract says cannot matter (DESIGN.md sections 2 and 4.24)."""
import ctypes

import numpy as np
import pytest

import icm_oracle as io
import icm_wide_oracle as wo

pytestmark = pytest.mark.gpu


def _data(n, d, m, h, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    B0 = rng.integers(0, h, size=(n, m)).astype(np.int16)
    B0[0, :] = h - 1                                        # the last codeword, past every full piece of the row
    return X, C, B0


def _gpu(X, C, B0, ilsiter, icmiter, npert, randord, seed=0, t0=0, nsplits=1):
    from rayuela_jl_amd.LSQ import encode_icm_u16
    return encode_icm_u16(X, B0, C, ilsiter, icmiter, npert, randord, seed=seed, t0=t0, nsplits=nsplits, with_cost=True)


def _raw(X, C, B0, ilsiter, icmiter, npert, randord, seed=0, t0=0, nsplits=1, code_base=0, out=None, cost="new"):
    """rq_encode_icm_wide itself: (return code, codes_out, cost_out)."""
    from rayuela_jl_amd import _lib
    n, d = X.shape
    m, h, _ = C.shape
    out = np.full((n, m), -3, np.int16) if out is None else out
    cost = np.full(n, -3.0, np.float32) if isinstance(cost, str) else cost
    rc = _lib.lib().rq_encode_icm_wide(out.ctypes.data, B0.ctypes.data, None if cost is None else cost.ctypes.data, X.ctypes.data,
                                       C.ctypes.data, n, d, m, h, ilsiter, icmiter, npert, 1 if randord else 0, seed, t0, nsplits,
                                       code_base)
    return rc, out, cost


def _assert_same(got, want):
    (b1, c1), (b0, c0) = got, want
    assert b1.dtype == np.int16
    bad = np.flatnonzero((b1 != b0).any(axis=1))
    assert bad.size == 0, "%d rows differ, first %d: got %s want %s" % (bad.size, bad[0], b1[bad[0]], b0[bad[0]])
    assert np.array_equal(c1.view(np.uint32), c0.view(np.uint32)), "per-row costs differ"


# ---- 1. bit for bit against the oracle -----------------------------------------------------------------------------------------------
# h = 257 and 320: one full piece of 256 entries and a short one; 1000: no multiple of 64; 1024: whole pieces; 4096: sixteen pieces;
# m = 1 (no gathers), 2, 4, 8, 16 (each register budget of the kernel)
@pytest.mark.parametrize("m,h,d,n", [(1, 257, 8, 64), (2, 320, 16, 128), (4, 1000, 16, 128), (16, 320, 8, 64), (2, 4096, 8, 64)])
def test_shapes_bit_exact(rq, oracle, m, h, d, n):
    X, C, B0 = _data(n, d, m, h, seed=m * 1000 + h + d)
    args = (2, 2, min(2, m), (m + h) % 2 == 0)
    got = _gpu(X, C, B0, *args, seed=5)
    assert got[0].min() >= 0 and got[0].max() < h
    _assert_same(got, wo.ils(oracle, X, C, B0, *args, seed=5))


@pytest.fixture(scope="module")
def big(oracle):
    """(8, 1024, 16, 96): the data and the oracle's tables, computed once."""
    X, C, B0 = _data(96, 16, 8, 1024, seed=3)
    return X, C, B0, wo.tables(oracle, X, C)


@pytest.mark.parametrize("icmiter,npert,randord,t0", [(2, 2, True, 0), (0, 1, True, 0), (1, 0, False, 0), (3, 8, True, 0),
                                                        (1, 1, False, 5), (3, 0, True, 2), (1, 8, False, 0), (3, 1, True, 4)])
def test_iteration_knobs_bit_exact_at_m8_h1024(rq, oracle, big, icmiter, npert, randord, t0):
    X, C, B0, tabs = big
    args = (2, icmiter, npert, randord)
    _assert_same(_gpu(X, C, B0, *args, seed=9, t0=t0), wo.ils(oracle, X, C, B0, *args, seed=9, t0=t0, tabs=tabs))


# ---- 2. two independent kernels: the wide entry equals the byte entry at h <= 256 -----------------------------------------------------
@pytest.mark.parametrize("m,h,d,n", [(8, 256, 32, 20000), (5, 100, 37, 777), (16, 64, 24, 2000)])
def test_wide_entry_equals_byte_entry(rq, m, h, d, n):
    from rayuela_jl_amd.LSQ import encode_icm_u8
    X, C, B0 = _data(n, d, m, h, seed=h + m)
    args = (3, 2, min(3, m), True)
    b8, c8 = encode_icm_u8(X, B0.astype(np.uint8), C, *args, seed=7, t0=1, nsplits=2, with_cost=True)
    _assert_same(_gpu(X, C, B0, *args, seed=7, t0=1, nsplits=3), (b8.astype(np.int16), c8))


# ---- 3. what cannot matter --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inv():
    X, C, B0 = _data(101, 16, 4, 300, seed=6)
    return X, C, B0, _gpu(X, C, B0, 4, 2, 2, True, seed=3)


def test_nsplits_do_not_change_results(rq, inv):
    from rayuela_jl_amd import _lib
    X, C, B0, ref = inv
    for ns in (3, 7):
        out = (ctypes.c_int64 * 5)()
        assert _lib.lib().rq_icm_wide_plan(101, 16, 4, 300, ns, ctypes.cast(out, ctypes.c_void_p), 5) == 0
        assert list(out)[3:] == [-(-101 // ns), ns]           # really that many chunks, the last one short
        _assert_same(_gpu(X, C, B0, 4, 2, 2, True, seed=3, nsplits=ns), ref)


def test_checkpoints_equal_one_run(rq, inv):
    X, C, B0, ref = inv
    cur = B0
    for t0, its in ((0, 1), (1, 2), (3, 1)):
        cur, cost = _gpu(X, C, cur, its, 2, 2, True, seed=3, t0=t0, nsplits=2)
    _assert_same((cur, cost), ref)


def test_code_base_aliasing_and_no_cost(rq, inv):
    X, C, B0, ref = inv
    rc, b1, c1 = _raw(X, C, B0 + 1, 4, 2, 2, True, seed=3, code_base=1)
    assert rc == 0
    _assert_same((b1 - 1, c1), ref)
    Bh = B0.copy()
    rc, out, cost = _raw(X, C, Bh, 4, 2, 2, True, seed=3, out=Bh, cost=None)      # codes_out == codes_in, cost_out NULL
    assert rc == 0 and out is Bh and cost is None and np.array_equal(Bh, ref[0])


def test_zero_iterations_is_veccost(rq, inv):
    X, C, B0, _ = inv
    b, c = _gpu(X, C, B0, 0, 2, 2, True, seed=3)
    assert np.array_equal(b, B0)
    assert np.array_equal(c.view(np.uint32), io.veccost(X, B0, C).view(np.uint32))


def test_stale_scratch_does_not_matter(rq, inv):
    from rayuela_jl_amd import _lib
    X, C, B0, ref = inv
    for value in (0xFF, 0x00):
        _lib.fill_scratch(value)
        _assert_same(_gpu(X, C, B0, 4, 2, 2, True, seed=3), ref)


def test_errors_leave_the_outputs_untouched(rq, inv):
    X, C, B0, _ = inv
    bad, zero = B0.copy(), B0.copy()
    bad[100, 3], zero[100, 3] = 300, 0
    for kw, codes in ((dict(npert=5), B0), (dict(), bad), (dict(nsplits=0), B0), (dict(code_base=1), zero)):
        a = dict(ilsiter=1, icmiter=1, npert=1, randord=True)
        a.update(kw)
        rc, out, cost = _raw(X, C, codes, **a)
        assert rc == -1 and (out == -3).all() and (cost == -3.0).all(), kw


def test_nonfinite_rows_keep_to_themselves(rq, inv):
    X, C, B0, ref = inv
    Xbad = X.copy()
    Xbad[5, 3], Xbad[40, 0], Xbad[77, :] = np.nan, np.inf, -np.inf
    rows = np.array([5, 40, 77])
    ok = np.setdiff1d(np.arange(len(X)), rows)
    b, c = _gpu(Xbad, C, B0, 4, 2, 2, True, seed=3, nsplits=2)
    assert b.min() >= 0 and b.max() < 300
    assert np.array_equal(b[ok], ref[0][ok]) and np.array_equal(c[ok].view(np.uint32), ref[1][ok].view(np.uint32))
    b2, c2 = _gpu(Xbad, C, B0, 4, 2, 2, True, seed=3, nsplits=2)
    assert np.array_equal(b, b2) and np.array_equal(c.view(np.uint32), c2.view(np.uint32))


# ---- 4. the mirrors ---------------------------------------------------------------------------------------------------------------
def test_mirrors_dispatch_on_h(rq, inv):
    from rayuela_jl_amd.LSQ import last_timing
    X, C, B0, ref = inv
    oldB = B0 + 1
    B = rq.encoding_icm(X, oldB, list(C), 4, 2, True, 2, cpp=False, seed=3)
    t = last_timing()                                  # rq_last_icm_timing reports the wide call too
    assert 0 < t["unary_ms"] <= t["total_ms"], t
    assert B.dtype == np.int16 and np.array_equal(oldB, B) and np.array_equal(B, ref[0] + 1)
    Bin = B0 + 1
    Bs, objs = rq.encode_icm_cuda(X, Bin, list(C), [1, 4], 2, 2, True, seed=3)
    assert np.array_equal(Bin, B0 + 1) and np.array_equal(Bs[1], B)
    assert objs[1] == np.float32(np.mean(ref[1], dtype=np.float64)) and objs[1] <= objs[0]
    assert np.array_equal(rq.veccost(X, B, list(C)).view(np.uint32), ref[1].view(np.uint32))
    assert rq.qerror(X, B, list(C)) == float(np.mean(ref[1], dtype=np.float64))


def test_end_to_end_after_train_rvq_wide(rq):
    """ICM from the greedy codes of wide RVQ codebooks: no row's cost rises, the mean falls, and the codes feed the norms."""
    import rayuela_jl_amd.synth as synth
    n, d, m, h = 4096, 16, 4, 512
    X = synth.sift_like(n, d, seed=31)
    C, B, _ = rq.train_rvq(X, m, h, niter=2)
    assert B.dtype == np.int16 and B.max() > 256
    c0 = rq.veccost(X, B, C)
    B1 = rq.encoding_icm(X, B.copy(), C, 4, 2, True, 2, cpp=False, seed=1)
    c1 = rq.veccost(X, B1, C)
    assert B1.min() >= 1 and B1.max() <= h
    assert (c1 <= c0).all() and c1.mean(dtype=np.float64) < c0.mean(dtype=np.float64)
