"""GPU: Enhanced RVQ / Stacked Quantizers with more than 256 entries per codebook (src/ERVQ.jl on Int16 codes; DESIGN.md section
4.21): rq_ervq_update_codebook_wide, rq_train_ervq_wide and their host mirrors against the numpy restatements of
tests/ervq_oracle.py driven by the wide RVQ encode of tests/wide_oracle.py, the byte entries' bits at h <= 256, the loop's
contract, the refill of entries without rows, argument checks, a non-finite row, and experiment_ervq end to end at h = 300."""
import ctypes

import numpy as np
import pytest

import ervq_oracle as eo
import wide_oracle as wo

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _p(a):
    return None if a is None else a.ctypes.data


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _encoder(oracle):
    """ervq_oracle's `encode` argument over wide codebooks: codes (n, m) int16 zero-based [, counts, final residual]."""
    def enc(X, C, with_extras=False):
        codes, counts, Xr = wo.encode_rvq_wide(oracle, X, C)
        return (codes, counts, Xr) if with_extras else codes
    return enc


def _setup(oracle, n, d, m, h, seed):
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(n, d, seed=seed)
    C = synth.rvq_codebooks(X, m, h, seed=seed + 1, iters=1, sample=min(n, 2048))
    return X, _encoder(oracle)(X, C), C


def _train(X, codes, C, niter, seed=0, base=1, raw=False):
    """rq_train_ervq_wide itself: (status, C, B, error, obj); codes zero-based in, B in `base` out."""
    n, d = X.shape
    m, h = C.shape[0], C.shape[1]
    Cs = np.ascontiguousarray(C, dtype=np.float32).copy()
    B = np.ascontiguousarray(codes.astype(np.int16) + base)
    err, obj = ctypes.c_double(-1.0), np.full(niter * m + 1, -1.0)
    st = _L().rq_train_ervq_wide(_p(Cs), _p(B), ctypes.cast(ctypes.byref(err), ctypes.c_void_p), _p(obj), _p(X), n, d, m, h, niter,
                                 seed, base)
    if raw:
        return st, Cs, B, err.value, obj
    assert st == 0, _L().rq_last_error()
    return Cs, B, err.value, obj


# ---- 1. the update step against the literal restatement in f64 ---------------------------------------------------------------
def test_update_step_matches_the_literal_f64_update(rq, oracle):
    """rtol 1e-5 / atol 1e-4 on sift_like data: the bar of tests/test_gpu_ervq.py's update test (update_centers' bar)."""
    n, d, m, h = 6000, 16, 3, 300
    X, codes, C = _setup(oracle, n, d, m, h, seed=n + d)
    a, b = 5, 6
    for j in range(m):
        codes2 = codes.copy()
        codes2[codes2[:, j] == a, j] = b                           # entry a of codebook j loses its rows
        want, cnt0 = eo.literal_update(X, codes2, C, j)
        got, counts = rq.ervq_update_codebook(X, codes2, C, j)
        assert np.array_equal(counts, np.bincount(codes2[:, j], minlength=h)) and np.array_equal(counts, cnt0)
        assert counts[a] == 0 and int(codes2[:, j].max()) >= 256
        err = np.abs(got[j].astype(np.float64) - want)
        print("(%d, %d, %d, %d) j=%d: worst entry %.3e (values up to %.1f)" % (n, d, m, h, j, err.max(), np.abs(want).max()))
        assert np.allclose(got[j], want, rtol=1e-5, atol=1e-4)
        for i in range(m):
            if i != j:
                assert np.array_equal(_u32(got[i]), _u32(C[i]))
        for k in np.flatnonzero(counts == 0):                          # no rows: the entry keeps its bits
            assert np.array_equal(_u32(got[j][k]), _u32(C[j][k]))
        got1, counts1 = rq.ervq_update_codebook(X, codes2.view(np.uint16), C, j)      # uint16 codes select the wide entry too
        assert np.array_equal(_u32(got1), _u32(got)) and np.array_equal(counts1, counts)


# ---- 2. h <= 256: the byte entries' bits ---------------------------------------------------------------------------------------
def test_up_to_256_entries_the_wide_entries_give_the_byte_entries_bits(rq, oracle):
    from rayuela_jl_amd.ERVQ import train_ervq_i16
    n, d, m, h = 12000, 32, 4, 32
    X, codes, C = eo.fixture(oracle.encode_rvq, n, d, m, h)
    C8, B8, e8, o8 = train_ervq_i16(X, codes.astype(np.int16) + 1, C, m, h, 2, seed=3)
    for base in (0, 1):
        Cw, Bw, ew, ow = _train(X, codes, C, 2, seed=3, base=base)
        assert np.array_equal(_u32(Cw), _u32(C8)) and np.array_equal(Bw, B8 - 1 + base)
        assert np.array_equal(ow.view(np.uint64), o8.view(np.uint64)) and ew == e8
    for j in (0, m - 1):
        got8, cnt8 = rq.ervq_update_codebook(X, codes, C, j)
        for base in (0, 1):
            Cs, cnt = C.copy(), np.full(h, 7, np.uint32)
            c16 = np.ascontiguousarray(codes.astype(np.int16) + base)
            assert _L().rq_ervq_update_codebook_wide(_p(Cs), _p(cnt), _p(X), _p(c16), n, d, m, h, j, base) == 0, _L().rq_last_error()
            assert np.array_equal(_u32(Cs), _u32(got8)) and np.array_equal(cnt, cnt8)


# ---- 3. against the restatement ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fix(oracle):
    import rayuela_jl_amd.synth as synth
    n = 20000
    X = synth.sift_like(n, 32, seed=41)
    C = synth.rvq_codebooks(X, 2, 257, seed=42, sample=n)
    enc = _encoder(oracle)
    codes = enc(X, C)
    return X, codes, C, eo.incremental(X, codes, C, 2, enc, np.float32)


def test_train_ervq_wide_follows_the_restatement(rq, fix):
    """rq_train_ervq_wide against `incremental` in f32 over 2 iterations at (20000, 32, 2, 257): the last block of 256 codes
    holds one entry.  On this fixture no entry is without rows at any of the 4 steps, the obj trace of the restatement runs
    21221.86 -> 19174.57, and `literal` (f64 means) and `incremental` (f32) differ by 2.52e-10 relative on the trace, by 1.5e-5
    on a codebook entry and in no code.  The bars have the form of tests/test_gpu_ervq.py's: ten times that spread, capped at
    3e-4 and 2e-2 -- 2.52e-9 on every obj entry and no differing code.  Measured on the MI355X: trace 3.820e-10 relative,
    no differing code, worst codebook entry 1.526e-05."""
    from rayuela_jl_amd.ERVQ import last_ervq_timing
    X, codes, C, ref = fix
    Cg, Bg, err, obj = _train(X, codes, C, 2, base=0)
    ph = last_ervq_timing()
    assert all(np.isfinite(v) and v >= 0 for v in ph.values()), ph
    assert all(ph[k] > 0 for k in ("init_ms", "increment_ms", "encode_ms", "error_ms")), ph     # the clock reports the wide call
    Cr, Br, objr, inv = ref
    assert all(inv) and abs(objr[0] - 21221.86) < 0.01 and abs(objr[-1] - 19174.57) < 0.01
    trace = np.abs(obj - objr) / objr
    diff = float(np.mean(Bg != Br))
    print("obj (library):", np.array2string(obj, precision=4))
    print("trace: worst relative difference %.3e; differing codes %.3e; worst codebook entry %.3e"
          % (trace.max(), diff, np.abs(Cg.astype(np.float64) - Cr).max()))
    assert trace.max() <= min(10 * 2.52e-10, 3e-4), trace
    assert diff <= min(10 * 0.0, 2e-2), diff


# ---- 4. the contract of the loop -----------------------------------------------------------------------------------------------
def test_train_ervq_wide_contract(rq, fix):
    X, codes, C, _ = fix
    m, h = C.shape[0], C.shape[1]
    B0 = codes.astype(np.int16) + 1
    Cl, B, err = rq.train_ervq(X, B0, [C[i] for i in range(m)], m, h, 2)          # the mirror dispatches on h
    Cs = np.stack(Cl)
    assert B.dtype == np.int16 and np.array_equal(B, rq.quantize_rvq(X, Cl)[0]) and int(B.max()) == h
    e0 = eo.qerror(X, B.astype(np.int64) - 1, Cs)
    assert abs(err - e0) <= 1e-6 * e0
    C1, B1, err1, obj = _train(X, codes, C, 2)
    assert obj.shape == (2 * m + 1,) and obj[-1] == err1 == err and err < obj[0]
    assert np.array_equal(_u32(C1), _u32(Cs)) and np.array_equal(B1, B)             # two calls: the same bits
    s0 = eo.qerror(X, codes, C)
    assert abs(obj[0] - s0) <= 1e-6 * s0
    C0, Bz, ez, oz = _train(X, codes, C, 0)               # niter = 0: the inputs bit for bit, and their error
    assert np.array_equal(_u32(C0), _u32(C)) and np.array_equal(Bz, B0)
    assert oz.shape == (1,) and ez == oz[0] == obj[0]


# ---- 5. entries without rows ---------------------------------------------------------------------------------------------------
def _is_a_row(P, v):
    return bool((P.view(np.uint32) == v.view(np.uint32)[None, :]).all(axis=1).any())


def test_entries_that_lose_their_rows_are_refilled(rq, oracle):
    """sift_like(12000, 16, seed=41), m = 3, h = 300: the start codes use every entry, and in the restatement the second
    codebook has entries without rows when its step comes, in both iterations.  After ONE iteration the second codebook is not
    touched again and the first stage keeps its codes, so the entries the restatement finds empty in iteration 0 must be rows of
    P_1 = X - C_0[b_0] of the result, bit for bit.  Two iterations: finite, B == quantize_rvq, the same bits under the same seed."""
    import rayuela_jl_amd.synth as synth
    n, d, m, h = 12000, 16, 3, 300
    X = synth.sift_like(n, d, seed=41)
    C = synth.rvq_codebooks(X, m, h, seed=42)
    enc = _encoder(oracle)
    codes = enc(X, C)
    assert all((np.bincount(codes[:, j], minlength=h) > 0).all() for j in range(m))
    # the restatement up to step 1 of iteration 0
    E = X.copy()
    for i in range(m):
        E -= C[i][codes[:, i]]
    C0 = C.copy()
    sums, cnt = eo.class_sums(E, codes[:, 0], h, np.float32)
    C0[0] = C0[0] + sums / cnt[:, None].astype(np.float32)
    empty = np.flatnonzero(np.bincount(enc(X, C0)[:, 1], minlength=h) == 0)
    assert empty.size > 0
    Cg, Bg, err, obj = _train(X, codes, C, 1, seed=5, base=0)
    assert np.isfinite(Cg).all() and np.isfinite(obj).all()
    P1 = X - Cg[0][Bg[:, 0]]
    for k in empty:
        assert _is_a_row(P1, Cg[1][k]), (k, Cg[1][k])
    C2, B2, e2, o2 = _train(X, codes, C, 2, seed=5)
    assert np.isfinite(C2).all() and np.isfinite(o2).all() and o2[-1] < o2[0]
    assert np.array_equal(B2, rq.quantize_rvq(X, [C2[i] for i in range(m)])[0])
    C3, B3, e3, o3 = _train(X, codes, C, 2, seed=5)                  # the same seed: the same draws
    assert np.array_equal(_u32(C3), _u32(C2)) and np.array_equal(B3, B2) and np.array_equal(o3.view(np.uint64), o2.view(np.uint64))


def test_entries_forced_empty_are_refilled_from_the_prefix_residual(rq, oracle):
    """tests/test_gpu_ervq.py's case at h = 300: entry 3 of codebook 0 has no rows in the start codes; entry 290 of codebook 2
    lies far from every residual, so it has none when step 2 comes.  With niter = 1 each refilled entry must be found among the
    rows of X - sum_{i < j} C_i[b_i] of the RESULT, bit for bit."""
    n, d, m, h = 6000, 16, 3, 300
    X, codes, C = _setup(oracle, n, d, m, h, seed=77)
    C = C.copy()
    C[2][290] = 1.0e4
    codes = _encoder(oracle)(X, C)
    codes[codes[:, 0] == 3, 0] = 4
    assert (codes[:, 2] != 290).all() and (codes[:, 0] != 3).all()
    Cg, Bg, err, obj = _train(X, codes, C, 1, seed=5, base=0)
    assert np.isfinite(Cg).all() and np.isfinite(obj).all()
    P = X.astype(np.float32, copy=True)
    for j, k in ((0, 3), (2, 290)):
        assert _is_a_row(P, Cg[j][k]), (j, k, Cg[j][k])
        if j == 0:
            P = P - Cg[0][Bg[:, 0]]
            P = P - Cg[1][Bg[:, 1]]
    C2, B2, _, o2 = _train(X, codes, C, 1, seed=5, base=0)
    assert np.array_equal(_u32(C2), _u32(Cg)) and np.array_equal(B2, Bg) and np.array_equal(o2.view(np.uint64), obj.view(np.uint64))


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(rq, oracle):
    n, d, m, h = 500, 8, 3, 300
    X, codes, C = _setup(oracle, n, d, m, h, seed=9)
    L = _L()
    B = codes.astype(np.int16) + 1
    Cs, B1, cnt = C.copy(), B.copy(), np.full(h, 7, np.uint32)
    err, obj = ctypes.c_double(-1.0), np.full(m + 1, -1.0)

    def train(Bx, mm=m, hh=h, dd=d, niter=1, base=1):
        return L.rq_train_ervq_wide(_p(Cs), _p(Bx), ctypes.cast(ctypes.byref(err), ctypes.c_void_p), _p(obj), _p(X), n, dd, mm, hh,
                                    niter, 0, base)

    def update(cx, j, mm=m, hh=h, dd=d, base=1):
        return L.rq_ervq_update_codebook_wide(_p(Cs), _p(cnt), _p(X), _p(cx), n, dd, mm, hh, j, base)

    for v in (0, h + 1, -1):
        Bb = B.copy()
        Bb[17, 1] = v
        assert train(Bb) == RQ_EINVAL and b"code" in L.rq_last_error()
        assert update(Bb, 0) == RQ_EINVAL and b"code" in L.rq_last_error()
    Bb = B.copy()
    Bb[0, 0] = h                                                    # fine one-based, out of range zero-based
    assert train(Bb, base=0) == RQ_EINVAL and update(Bb, 0, base=0) == RQ_EINVAL
    assert train(B1, hh=1) == RQ_EINVAL and train(B1, hh=32768) == RQ_EUNSUPPORTED
    assert train(B1, mm=0) == RQ_EUNSUPPORTED and train(B1, mm=65) == RQ_EUNSUPPORTED
    assert train(B1, dd=0) == RQ_EINVAL and train(B1, niter=-1) == RQ_EINVAL and train(B1, base=2) == RQ_EINVAL
    assert update(B1, m) == RQ_EINVAL and update(B1, -1) == RQ_EINVAL and update(B1, 0, base=2) == RQ_EINVAL
    assert update(B1, 0, hh=1) == RQ_EINVAL and update(B1, 0, hh=32768) == RQ_EUNSUPPORTED
    assert update(B1, 0, mm=0) == RQ_EUNSUPPORTED and update(B1, 0, mm=65) == RQ_EUNSUPPORTED and update(B1, 0, dd=0) == RQ_EINVAL
    assert L.rq_last_error()
    assert np.array_equal(_u32(Cs), _u32(C)) and np.array_equal(B1, B)
    assert err.value == -1.0 and (obj == -1.0).all() and (cnt == 7).all()
    # the byte entries refuse h > 256 as before, and the mirrors check before the library is touched
    c8 = np.zeros((n, m), np.uint8)
    assert L.rq_ervq_update_codebook(_p(Cs), _p(cnt), _p(X), _p(c8), n, d, m, 257, 0) != 0 and (cnt == 7).all()
    with pytest.raises(ValueError):
        rq.train_ervq(X, B, [np.zeros((32768, d), np.float32)] * m, m, 32768, 1)
    with pytest.raises(ValueError):
        Bb = B.copy()
        Bb[3, 2] = h + 1
        rq.train_ervq(X, Bb, [C[i] for i in range(m)], m, h, 1)


# ---- 7. a non-finite row -------------------------------------------------------------------------------------------------------
def test_a_non_finite_row_returns_codes_in_range_and_the_same_bits_twice(rq, oracle):
    n, d, m, h = 6000, 16, 3, 300
    X, codes, C = _setup(oracle, n, d, m, h, seed=n + d)
    good = _train(X, codes, C, 1, seed=2)
    Xn = X.copy()
    Xn[11, 3], Xn[4000, 0] = np.nan, np.inf
    runs = [_train(Xn, codes, C, 1, seed=2, raw=True) for _ in range(2)]
    for st, Cg, Bg, e, obj in runs:
        assert st == 0 or (st < 0 and _L().rq_last_error())
        assert int(Bg.min()) >= 1 and int(Bg.max()) <= h
    a, b = runs
    assert a[0] == b[0] and np.array_equal(_u32(a[1]), _u32(b[1])) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[4].view(np.uint64), b[4].view(np.uint64))
    again = _train(X, codes, C, 1, seed=2)                          # a finite call afterwards: its usual bits
    assert np.array_equal(_u32(again[0]), _u32(good[0])) and np.array_equal(again[1], good[1])
    assert np.array_equal(again[3].view(np.uint64), good[3].view(np.uint64))


# ---- 8. experiment_ervq end to end at h = 300 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("norms", ["host", "device"])
def test_experiment_ervq_end_to_end(rq, norms):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import experiments as ex
    d, m, h, knn, niter = 16, 3, 300, 50, 2
    Xb = synth.sift_like(8000, d, seed=5)
    Xt = Xb[:6000]
    Xq = synth.sift_like(32, d, seed=6)
    gt = ((((Xq.astype(np.float64)[:, None, :] - Xb.astype(np.float64)[None, :, :]) ** 2).sum(-1)).argmin(1) + 1).astype(np.uint32)
    C, B, train_error, B_base, recall = ex.experiment_ervq(Xt, Xb, Xq, gt, m, h, niter, knn, seed=2, norms=norms)
    assert len(C) == m and C[0].shape == (h, d) and B.shape == (6000, m) and B_base.shape == (8000, m)
    assert B.dtype == np.int16 and B_base.dtype == np.int16 and train_error > 0 and int(B.max()) > 256
    assert np.array_equal(B_base, rq.quantize_rvq(Xb, C)[0])
    assert recall.shape == (knn,) and (np.diff(recall) >= 0).all() and recall[-1] > 0.5
    gt_t = ((((Xq.astype(np.float64)[:, None, :] - Xt.astype(np.float64)[None, :, :]) ** 2).sum(-1)).argmin(1) + 1).astype(np.uint32)
    C3, B3, e3, rec3 = ex.experiment_ervq_query_base(Xt, Xq, gt_t, m, h, niter, knn, seed=2, norms=norms)
    assert B3.shape == (6000, m) and B3.dtype == np.int16 and rec3.shape == (knn,) and (np.diff(rec3) >= 0).all() and e3 > 0
