"""GPU: Enhanced RVQ / Stacked Quantizers (src/ERVQ.jl): rq_ervq_update_codebook, rq_train_ervq and their host mirrors
against the numpy restatements of tests/ervq_oracle.py, the loop's contract (B == quantize_rvq(X, C), the obj trace,
reproducibility, the refill of entries without rows, argument checks) and experiment_ervq end to end."""
import ctypes
import time

import numpy as np
import pytest

import ervq_oracle as eo

pytestmark = pytest.mark.gpu


def _setup(oracle, n, d, m, h, seed):
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(n, d, seed=seed)
    C = synth.rvq_codebooks(X, m, h, seed=seed + 1, iters=1, sample=min(n, 2048))
    return X, oracle.encode_rvq(X, C), C


# ---- 1. the update step against the literal restatement in f64 ---------------------------------------------------------------
@pytest.mark.parametrize("n,d,m,h,js", [
    (20000, 128, 8, 256, (0, 3, 7)),
    (5000, 96, 16, 64, (0, 15)),
    (4001, 5, 3, 7, (0, 1, 2)),        # d % 4 != 0: scalar epilogue; h not a multiple of 16; ragged 64-row tail
    (3000, 131, 2, 16, (0, 1)),        # d > 128, a last dimension block of 3 columns
    (3000, 32, 1, 16, (0,)),           # m = 1: the plain class means of X
    (40, 8, 2, 4, (0, 1)),             # fewer rows than one 64-row step
])
def test_update_step_matches_the_literal_f64_update(rq, oracle, n, d, m, h, js):
    """rtol 1e-5 / atol 1e-4 on sift_like data: the bar test_gpu_train.py::test_reductions_match_float64 sets for
    update_centers."""
    X, codes, C = _setup(oracle, n, d, m, h, seed=n + d)
    a, b = (5, 6) if h > 6 else (1, 2)
    for j in js:
        codes2 = codes.copy()
        codes2[codes2[:, j] == a, j] = b                           # entry a of codebook j loses its rows
        want, cnt0 = eo.literal_update(X, codes2, C, j)
        got, counts = rq.ervq_update_codebook(X, codes2, C, j)
        assert np.array_equal(counts, np.bincount(codes2[:, j], minlength=h)) and np.array_equal(counts, cnt0)
        assert counts[a] == 0
        err = np.abs(got[j].astype(np.float64) - want)
        print("(%d, %d, %d, %d) j=%d: worst entry %.3e (values up to %.1f)" % (n, d, m, h, j, err.max(), np.abs(want).max()))
        assert np.allclose(got[j], want, rtol=1e-5, atol=1e-4)
        for i in range(m):
            if i != j:
                assert np.array_equal(got[i].view(np.uint32), C[i].view(np.uint32))
        for k in np.flatnonzero(counts == 0):                          # no rows: the entry keeps its bits
            assert np.array_equal(got[j][k].view(np.uint32), C[j][k].view(np.uint32))
        if m == 1:
            for k in np.flatnonzero(counts):
                assert np.allclose(got[0][k], X[codes2[:, 0] == k].astype(np.float64).mean(0), rtol=1e-5, atol=1e-4)


# ---- the fixture of items 2, 4, 5: the one tests/test_ervq_oracle.py shows to improve on the CPU ------------------------------
@pytest.fixture(scope="module")
def fix(oracle):
    X, codes, C = eo.fixture(oracle.encode_rvq)
    ref = eo.incremental(X, codes, C, eo.FIX_NITER, oracle.encode_rvq, np.float32)
    return X, codes, C, ref


def _train(X, codes, C, niter, seed=0):
    from rayuela_jl_amd.ERVQ import train_ervq_i16
    m, h = C.shape[0], C.shape[1]
    return train_ervq_i16(X, codes.astype(np.int16) + 1, C, m, h, niter, seed=seed)


# ---- 2. bit reproducibility ----------------------------------------------------------------------------------------------------
def test_train_ervq_is_bit_reproducible(rq, fix):
    X, codes, C, _ = fix
    C1, B1, e1, o1 = _train(X, codes, C, 2)
    C2, B2, e2, o2 = _train(X, codes, C, 2)
    assert np.array_equal(C1.view(np.uint32), C2.view(np.uint32)) and np.array_equal(B1, B2)
    assert np.array_equal(o1.view(np.uint64), o2.view(np.uint64)) and e1 == e2


# ---- 3. the contract of the loop -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,m,h", [(12000, 32, 4, 32), (8000, 96, 3, 256)])
def test_train_ervq_contract(rq, oracle, n, d, m, h):
    X, codes, C = _setup(oracle, n, d, m, h, seed=3 * n + d)
    B0 = codes.astype(np.int16) + 1
    Cl, B, err = rq.train_ervq(X, B0, [C[i] for i in range(m)], m, h, 2)
    Cs = np.stack(Cl)
    assert B.dtype == np.int16 and np.array_equal(B, rq.quantize_rvq(X, Cl)[0])
    e0 = eo.qerror(X, (B - 1).astype(np.uint8), Cs)
    assert abs(err - e0) <= 1e-6 * e0                     # the bar of test_train_pq_reduces_the_error
    _, _, err2, obj = _train(X, codes, C, 2)
    assert obj.shape == (2 * m + 1,) and obj[-1] == err2 == err
    s0 = eo.qerror(X, codes, C)
    assert abs(obj[0] - s0) <= 1e-6 * s0
    C0, Bz, ez, oz = _train(X, codes, C, 0)               # niter = 0: the inputs bit for bit, and their error
    assert np.array_equal(C0.view(np.uint32), C.view(np.uint32)) and np.array_equal(Bz, B0)
    assert oz.shape == (1,) and ez == oz[0] == obj[0]


# ---- 4. against the restatement ------------------------------------------------------------------------------------------------
def test_train_ervq_follows_the_restatement(rq, fix):
    """rq_train_ervq against `incremental` in f32 (the library's formulation in numpy) over 3 iterations at
    (12000, 32, 4, 32).  The bars are ten times the spread that tests/test_ervq_oracle.py measures on this fixture between
    `literal` (f64 means) and `incremental` (f32): trace 5.342e-10 relative, worst codebook entry 7.629e-06, 0 differing
    codes -- so 5.4e-9 on every obj entry and no differing code (the caps, 3e-4 and 2e-2 of
    test_train_opq_follows_the_oracle_loop, are far above).  Measured on the MI355X: trace 9.855e-10, no differing code,
    worst codebook entry 7.629e-06 (EXPERIMENTS.md section 13).
    The call's phase clock (rq_last_ervq_timing): every slot finite and >= 0, the phases this shape runs > 0 (the refill and
    the in-place epilogue may have no work of their own), and no more in total than the wall time of the call."""
    from rayuela_jl_amd.ERVQ import last_ervq_timing
    X, codes, C, ref = fix
    t0 = time.perf_counter()
    Cg, Bg, err, obj = _train(X, codes, C, eo.FIX_NITER)
    wall_ms = (time.perf_counter() - t0) * 1e3
    ph = last_ervq_timing()
    print("phases:", "  ".join("%s=%.3f" % kv for kv in ph.items()), " wall %.3f ms" % wall_ms)
    assert all(np.isfinite(v) and v >= 0 for v in ph.values()), ph
    assert all(ph[k] > 0 for k in ("init_ms", "increment_ms", "encode_ms", "error_ms")), ph
    assert sum(ph.values()) <= wall_ms, (ph, wall_ms)
    Cr, Br, objr, _ = ref
    trace = np.abs(obj - objr) / objr
    diff = float(np.mean((Bg - 1) != Br))
    print("obj (library):", np.array2string(obj, precision=4))
    print("trace: worst relative difference %.3e; differing codes %.3e; worst codebook entry %.3e"
          % (trace.max(), diff, np.abs(Cg.astype(np.float64) - Cr).max()))
    assert trace.max() <= min(10 * 5.342e-10, 3e-4), trace
    assert diff <= min(10 * 0.0, 2e-2), diff


# ---- 5. improves on its start --------------------------------------------------------------------------------------------------
def test_train_ervq_improves_on_its_rvq_start(rq, fix):
    """The end against the start only: the trace is not monotone from step to step (the greedy re-encode may lose what the
    update won)."""
    X, codes, C, _ = fix
    _, _, err, obj = _train(X, codes, C, eo.FIX_NITER)             # the start the CPU restatement improves on
    assert err < 0.99 * obj[0], obj
    m, h = eo.FIX_M, eo.FIX_H
    C0, B0, e_rvq = rq.train_rvq(X, m, h, niter=10, seed=1)        # and a train_rvq start
    C1, B1, e1 = rq.train_ervq(X, B0, C0, m, h, eo.FIX_NITER)
    print("train_rvq %.4f -> train_ervq %.4f" % (e_rvq, e1))
    assert e1 < e_rvq
    C2, B2, e2 = rq.train_ervq(X, m, h, 2, seed=1)                 # the method that initialises with train_rvq itself
    assert len(C2) == m and B2.shape == (X.shape[0], m) and np.isfinite(e2)


# ---- 6. entries without rows ---------------------------------------------------------------------------------------------------
def test_entries_without_rows_are_refilled_from_the_prefix_residual(rq, oracle):
    """Entry 3 of codebook 0 has no rows in the start codes; entry 5 of codebook 2 lies far from every residual, so it has
    none when step 2 comes.  With niter = 1 codebook j is not touched after step j, and the stages before j keep their codes,
    so each refilled entry must be found among the rows of X - sum_{i < j} C_i[b_i] of the RESULT, bit for bit."""
    n, d, m, h = 6000, 16, 3, 16
    X, codes, C = _setup(oracle, n, d, m, h, seed=77)
    C = C.copy()
    C[2][5] = 1.0e4
    codes = oracle.encode_rvq(X, C)
    codes[codes[:, 0] == 3, 0] = 4
    assert (codes[:, 2] != 5).all() and (codes[:, 0] != 3).all()
    Cg, Bg, err, obj = _train(X, codes, C, 1, seed=5)
    assert np.isfinite(Cg).all() and np.isfinite(obj).all()
    bg = Bg.astype(np.int64) - 1
    P = X.astype(np.float32, copy=True)
    for j, k in ((0, 3), (2, 5)):
        hit = (P.view(np.uint32) == Cg[j][k].view(np.uint32)[None, :]).all(axis=1)
        assert hit.any(), (j, k, Cg[j][k])
        if j == 0:
            P = P - Cg[0][bg[:, 0]]
            P = P - Cg[1][bg[:, 1]]
    C2, B2, _, o2 = _train(X, codes, C, 1, seed=5)                  # the same seed: the same draw
    assert np.array_equal(C2.view(np.uint32), Cg.view(np.uint32)) and np.array_equal(B2, Bg)
    assert np.array_equal(o2.view(np.uint64), obj.view(np.uint64))


# ---- 7. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(rq, oracle):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd.ERVQ import train_ervq_i16
    n, d, m, h = 500, 8, 3, 16
    X, codes, C = _setup(oracle, n, d, m, h, seed=9)
    B = codes.astype(np.int16) + 1
    Cl = [C[i] for i in range(m)]
    bad = (RuntimeError, ValueError)
    assert issubclass(rq.RayuelaHipError, RuntimeError)
    for v in (0, h + 1):
        Bb = B.copy()
        Bb[17, 1] = v
        with pytest.raises(bad):
            rq.train_ervq(X, Bb, Cl, m, h, 1)
    with pytest.raises(bad):
        rq.ervq_update_codebook(X, codes, C, m)                    # j = m
    with pytest.raises(bad):
        rq.ervq_update_codebook(X, codes, C, -1)
    cb = codes.copy()
    cb[3, 2] = h
    with pytest.raises(bad):
        rq.ervq_update_codebook(X, cb, C, 0)
    with pytest.raises(bad):
        rq.train_ervq(X, B[:-1], Cl, m, h, 1)                      # mismatched shapes
    with pytest.raises(bad):
        rq.train_ervq(X, B, Cl[:2], m, h, 1)
    with pytest.raises(bad):
        rq.train_ervq(X[:, :4].copy(), B, Cl, m, h, 1)
    with pytest.raises(bad):
        train_ervq_i16(X, np.ones((n, 65), np.int16), np.zeros((65, h, d), np.float32), 65, h, 1)
    # the library's own checks (the mirror's are bypassed): every one fails with RQ_EINVAL before the data is touched
    L = _lib.lib()
    Cs, B1, cnt = C.copy(), B.copy(), np.full(h, 7, np.uint32)
    err, obj = ctypes.c_double(-1.0), np.full(m + 1, -1.0)

    def train(Bx, mm=m, hh=h, dd=d, niter=1):
        return L.rq_train_ervq(Cs.ctypes.data, Bx.ctypes.data, ctypes.cast(ctypes.byref(err), ctypes.c_void_p), obj.ctypes.data,
                               X.ctypes.data, n, dd, mm, hh, niter, 0)

    def update(cx, j, mm=m, hh=h):
        return L.rq_ervq_update_codebook(Cs.ctypes.data, cnt.ctypes.data, X.ctypes.data, cx.ctypes.data, n, d, mm, hh, j)

    for v in (0, h + 1):
        Bb = B.copy()
        Bb[17, 1] = v
        assert train(Bb) != 0 and b"code" in L.rq_last_error()
    assert train(B1, mm=65) != 0 and train(B1, mm=0) != 0 and train(B1, hh=1) != 0 and train(B1, hh=257) != 0
    assert train(B1, dd=0) != 0 and train(B1, niter=-1) != 0
    assert update(codes, m) != 0 and update(codes, -1) != 0 and update(cb, 0) != 0 and update(codes, 0, mm=65) != 0
    assert update(codes, 0, hh=1) != 0
    assert np.array_equal(Cs.view(np.uint32), C.view(np.uint32)) and np.array_equal(B1, B)
    assert err.value == -1.0 and (obj == -1.0).all() and (cnt == 7).all()


# ---- 8. experiment_ervq end to end ---------------------------------------------------------------------------------------------
def test_experiment_ervq_end_to_end(rq, oracle):
    """experiment_ervq (src/ERVQ.jl:151-184, :214-227): train_rvq -> train_ervq -> norms codebook -> quantize_ervq of the
    base -> linscan_lsq -> recall; the search leg must equal the oracle's scan given the trained model."""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import experiments as ex
    d, m, h, knn = 32, 4, 256, 50
    Xb = synth.sift_like(20000, d, seed=5)
    Xt = Xb[:8000]
    Xq = synth.sift_like(64, d, seed=6)
    dd = ((Xq.astype(np.float64)[:, None, :] - Xb.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    gt = (dd.argmin(1) + 1).astype(np.uint32)
    C, B, train_error, B_base, recall = ex.experiment_ervq(Xt, Xb, Xq, gt, m, h, 3, knn, seed=2)
    assert len(C) == m and C[0].shape == (h, d) and B.shape == (8000, m) and B_base.shape == (20000, m)
    assert B.dtype == np.int16 and B_base.dtype == np.int16 and train_error > 0
    assert recall.shape == (knn,) and (np.diff(recall) >= 0).all() and recall[-1] > 0.5
    # the search leg: oracle encode + oracle scan with the same quantised norms
    Cs = np.stack(C)
    codes0 = oracle.encode_rvq(Xb, Cs)
    assert np.array_equal(B_base, codes0.astype(np.int16) + 1)
    _, norms_C = ex._norms_codebook(B, C, h, seed=2)
    Bn, _ = ex._quantize_norms(B_base, C, norms_C)
    db_norms = norms_C[Bn - 1].astype(np.float32)
    d0, i0 = oracle.linscan_lsq(codes0, Cs.reshape(m * h, d), Xq, db_norms, knn)
    assert np.allclose(recall, oracle.eval_recall(gt, i0, knn))
    # the method with start codes and codebooks, and the query-base drivers
    C2, B2, e2, Bb2, rec2 = ex.experiment_ervq(Xt, B, C, Xb, Xq, gt, m, h, 1, knn, seed=2)
    assert B2.shape == B.shape and Bb2.shape == B_base.shape and rec2.shape == (knn,)
    gt_t = ((((Xq.astype(np.float64)[:, None, :] - Xt.astype(np.float64)[None, :, :]) ** 2).sum(-1)).argmin(1) + 1).astype(np.uint32)
    C3, B3, e3, rec3 = ex.experiment_ervq_query_base(Xt, Xq, gt_t, m, h, 2, knn, seed=2)
    assert B3.shape == (8000, m) and rec3.shape == (knn,) and (np.diff(rec3) >= 0).all() and e3 > 0
    C4, B4, e4, rec4 = ex.experiment_ervq_query_base(Xt, B3, C3, Xq, gt_t, m, h, 1, knn, seed=2)
    assert B4.shape == (8000, m) and rec4.shape == (knn,)
    C5, B5, e5, rec5 = ex.experiment_rvq_query_base(Xt, Xq, gt_t, m, h, 2, knn, seed=2)
    assert B5.shape == (8000, m) and rec5.shape == (knn,) and (np.diff(rec5) >= 0).all() and e5 > 0
