"""GPU: LSQ++ past 256 codewords per codebook (rq_train_sr_wide and its mirrors): the training loop over
16-bit codes against its public steps composed in Python, against the byte loop at h <= 256, with and without the codebook
updates that repeat work, on library scratch of any content, and the drivers end to end."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NITER, ILS, ICM, NPERT, RANDORD, SEED, P = 3, 2, 2, 2, True, 9, 0.5


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _rotation(d, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return q.astype(np.float32)


def _composed(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, randord, seed, method, schedule, p, clean, plain_last=False):
    """rq_train_sr_wide's steps through the public entries over 16-bit codes (src/SR.jl:115-172), every update computed in full.
    plain_last: the last iteration's step is a plain update + encode (what schedule 1's zero scale must amount to)."""
    from rayuela_jl_amd.LSQ import encode_icm_u16
    from rayuela_jl_amd.OPQ import rotate
    from rayuela_jl_amd.SR import sr_perturb, sr_schedule, sr_std
    from rayuela_jl_amd.codebook_update import update_codebooks_u16
    n, d = X.shape
    RX = X if R is None else rotate(R, X)
    sigma_x = sr_std(RX) if method == "SR_C" else None

    def step(codes, call):
        if plain_last and call == niter:
            C = update_codebooks_u16(RX, codes, h)
        elif method == "SR_C":
            scale = sr_schedule(schedule, call, niter, p)
            C = update_codebooks_u16(sr_perturb(RX, sigma_x, scale, "SR_C", seed=seed, call=call), codes, h)
        else:
            scale = sr_schedule(schedule, 1 if call == 0 else call, niter, p)
            flat = update_codebooks_u16(RX, codes, h).reshape(m * h, d)
            sigma = sr_std(flat) / np.float32(m)
            C = sr_perturb(flat, sigma, scale, "SR_D", seed=seed, call=call).reshape(m, h, d)
        return C, encode_icm_u16(RX, codes, C, ilsiter, icmiter, npert, randord, seed=seed, t0=call * ilsiter)

    def qerror(codes, C):
        _, cost = encode_icm_u16(RX, codes, C, 0, 0, 0, False, with_cost=True)
        return np.mean(cost, dtype=np.float64)

    C, codes = step(codes0, 0)
    obj = []
    for it in range(1, niter + 1):
        obj.append(qerror(codes, C))
        C, codes = step(codes, it)
        if clean:
            C = update_codebooks_u16(RX, codes, h)
    obj.append(qerror(codes, C))
    if R is not None:
        C = rotate(np.ascontiguousarray(R.T), C.reshape(m * h, d)).reshape(m, h, d)     # C_i <- R C_i
    return C, codes, np.array(obj)


def _data(seed, n, d, m, h, dtype=np.int16):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    return X, rng.integers(0, h, size=(n, m)).astype(dtype)


def _h257(seed=12):
    """One codeword into the second block of 256: two digits in the second pass of the update's sort."""
    X, codes0 = _data(seed, 1500, 16, 3, 257)
    codes0[:3, :] = 256
    return X, codes0, 3, 257


def _wide(X, codes0, m, h, R, method, schedule, clean, niter=NITER, **kw):
    from rayuela_jl_amd.SR import train_sr_u16
    return train_sr_u16(X, codes0, m, h, R, niter, ILS, ICM, RANDORD, NPERT, method, schedule, P, clean, seed=kw.pop("seed", SEED),
                        **kw)


def _equal(a, b):
    return _same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype and _same_bits(a[2], b[2])


# ---- the loop equals its public steps -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [1, 2, 3])
@pytest.mark.parametrize("method", ["SR_C", "SR_D"])
def test_train_sr_wide_equals_composed_steps(rq, method, schedule):
    X, codes0, m, h = _h257()
    d = X.shape[1]
    for clean, rot in ((True, "seeded"), (False, "identity")):
        R = np.eye(d, dtype=np.float32) if rot == "identity" else _rotation(d, 5)
        C, codes, obj = _wide(X, codes0, m, h, R, method, schedule, clean)
        C0, codes_0, obj0 = _composed(X, codes0, m, h, R, NITER, ILS, ICM, NPERT, RANDORD, SEED, method, schedule, P, clean)
        assert obj.shape == (NITER + 1,) and np.isfinite(obj).all()
        assert codes.dtype == np.int16 and codes.min() >= 0 and codes.max() <= h - 1
        assert np.array_equal(codes, codes_0)
        assert _same_bits(C, C0)
        assert np.allclose(obj, obj0, rtol=1e-12, atol=0)
        if rot == "identity":      # R = None skips the rotations; R = I rotates exactly
            assert _equal(_wide(X, codes0, m, h, None, method, schedule, clean), (C, codes, obj))
    # the noise matters: another seed trains another quantizer
    C2, _, _ = _wide(X, codes0, m, h, None, method, schedule, False, seed=SEED + 1)
    assert not np.array_equal(C2, C)


def test_larger_codebooks_equal_composed_steps(rq):
    """m * h = 4096: 64 block steps of the Cholesky factorisation, most codes of every codebook without a row."""
    n, d, m, h = 3000, 32, 4, 1024
    X, codes0 = _data(3, n, d, m, h)
    R = _rotation(d, 8)
    C, codes, obj = _wide(X, codes0, m, h, R, "SR_D", 1, True, niter=2)
    C0, codes_0, obj0 = _composed(X, codes0, m, h, R, 2, ILS, ICM, NPERT, RANDORD, SEED, "SR_D", 1, P, True)
    assert np.array_equal(codes, codes_0) and _same_bits(C, C0) and np.allclose(obj, obj0, rtol=1e-12, atol=0)
    assert codes.max() > 255 and np.isfinite(obj).all()


def test_schedule_one_ends_with_a_plain_lsq_step(rq):
    """Schedule 1's scale is 0 in the last iteration, so that SR step is a plain update + encode at the same t0."""
    from rayuela_jl_amd.SR import sr_schedule
    X, codes0, m, h = _h257(seed=21)
    assert sr_schedule(1, NITER, NITER, P) == 0.0
    C, codes, obj = _wide(X, codes0, m, h, None, "SR_C", 1, False, seed=5)
    C0, codes_0, obj0 = _composed(X, codes0, m, h, None, NITER, ILS, ICM, NPERT, RANDORD, 5, "SR_C", 1, P, False, plain_last=True)
    assert np.array_equal(codes, codes_0) and _same_bits(C, C0) and np.allclose(obj, obj0, rtol=1e-12, atol=0)


# ---- h <= 256: the bits of the byte loop ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [64, 256])
def test_wide_entry_gives_the_byte_loops_bits(rq, h):
    from rayuela_jl_amd.SR import last_sr_stats, train_sr_u8
    n, d, m = 4000, 32, 4
    X, codes8 = _data(12, n, d, m, h, np.uint8)
    R = _rotation(d, 5)
    for method in ("SR_C", "SR_D"):
        for clean in (True, False):
            C8, B8, obj8 = train_sr_u8(X, codes8, m, h, R, NITER, ILS, ICM, RANDORD, NPERT, method, 2, P, clean, seed=SEED)
            assert last_sr_stats() == dict(full=1 + NITER * (2 if clean else 1), reused=0, skipped=0)
            C, B, obj = _wide(X, codes8.astype(np.int16), m, h, R, method, 2, clean)
            assert _same_bits(C, C8) and np.array_equal(B, B8) and B.dtype == np.int16 and _same_bits(obj, obj8), (method, clean)


# ---- the updates that repeat ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["SR_C", "SR_D"])
def test_flags_give_the_same_bits_and_the_counts_of_the_loop(rq, method):
    from rayuela_jl_amd.SR import last_sr_stats
    X, codes0, m, h = _h257()
    R = _rotation(X.shape[1], 5)
    for clean in (True, False):
        total = 1 + NITER * (2 if clean else 1)          # step 0, then a step and (clean) a trailing update per iteration
        lean = _wide(X, codes0, m, h, R, method, 1, clean)
        s0 = last_sr_stats()
        full = _wide(X, codes0, m, h, R, method, 1, clean, recompute=True)
        s1 = last_sr_stats()
        assert _equal(lean, full), (method, clean)
        assert s1 == dict(full=total, reused=0, skipped=0)
        assert sum(s0.values()) == total
        if not clean:
            assert s0 == s1
        elif method == "SR_D":      # steps 2 .. niter open with the update that closed the step before
            assert s0 == dict(full=total - (NITER - 1), reused=0, skipped=NITER - 1) and s0["skipped"] == 2
        else:                       # ... SR_C with the same matrix and another right-hand side
            assert s0 == dict(full=total - (NITER - 1), reused=NITER - 1, skipped=0) and s0["reused"] == 2


@pytest.mark.parametrize("method", ["SR_C", "SR_D"])
def test_result_does_not_depend_on_scratch_content(rq, method):
    from rayuela_jl_amd import _lib
    X, codes0, m, h = _h257()
    _lib.check(_lib.lib().rq_release_workspaces())
    want = _wide(X, codes0, m, h, None, method, 2, True)
    for value in (0x00, 0xFF, 0x7F, 0x80):
        _lib.fill_scratch(value)
        assert _equal(_wide(X, codes0, m, h, None, method, 2, True), want), "0x%02X" % value


# ---- independence and copy rules ------------------------------------------------------------------------------------------------------
def test_nsplits_code_base_and_in_place_rules(rq):
    L = rq.lib()
    rng = np.random.default_rng(13)
    n, d, m, h = 2000, 24, 3, 320
    X = rng.standard_normal((n, d)).astype(np.float32)
    B0 = rng.integers(1, h + 1, size=(n, m)).astype(np.int16)
    B0[0, :] = h
    R = _rotation(d, 6)
    for method in ("SR_C", "SR_D"):
        res = []
        for ns in (1, 3):
            Bin = B0.copy()
            C, Bc, obj = rq.train_sr_cuda(X, m, h, R, Bin, None, 2, 2, 2, True, 2, method, 1, 0.5, ns, seed=4)
            assert np.array_equal(Bin, B0)                                  # B is left untouched
            assert obj.dtype == np.float32 and obj.shape == (3,) and np.isfinite(obj).all()
            assert Bc.dtype == np.int16 and Bc.min() >= 1 and Bc.max() <= h and len(C) == m and C[0].shape == (h, d)
            res.append((C, Bc, obj))
        assert np.array_equal(res[0][1], res[1][1]) and _same_bits(res[0][2], res[1][2])
        assert all(_same_bits(a, b) for a, b in zip(res[0][0], res[1][0]))
        B = B0.copy()
        Ct, Bt, objt = rq.train_sr(X, m, h, R, B, None, 2, 2, 2, True, 2, method, 0.5, cpp=False, seed=4)
        assert np.array_equal(B, Bt) and not np.array_equal(B, B0)          # train_sr writes B in place
        assert objt.dtype == np.float32 and objt.shape == (3,)
        assert objt[0] == res[0][2][0]          # schedule 1 without the clean update: the first encode is shared
        # code_base 1 through the C entry: the same codebooks, the same codes shifted (train_sr_cuda runs code_base 0)
        C1 = np.empty((m, h, d), np.float32)
        codes1 = B0.copy()
        obj1 = np.zeros(3)
        assert L.rq_train_sr_wide(C1.ctypes.data, codes1.ctypes.data, obj1.ctypes.data, X.ctypes.data, R.ctypes.data, n, d, m, h, 2,
                                  2, 2, 2, 1, ("SR_C", "SR_D").index(method), 1, ctypes.c_double(0.5), 1, 4, 1, 1, 0) == 0
        assert np.array_equal(codes1, res[0][1]) and all(_same_bits(C1[i], res[0][0][i]) for i in range(m))
        assert _same_bits(obj1.astype(np.float32), res[0][2])


@pytest.mark.parametrize("method", ["SR_C", "SR_D"])
def test_a_nan_in_x_returns_with_codes_in_range(rq, method):
    """rq_train_sr's contract for non-finite X: RQ_OK or a negative status with a message; returned codes are in range."""
    from rayuela_jl_amd import _lib
    X, codes0, m, h = _h257()
    X = X.copy()
    X[7, 3] = np.nan
    try:
        C, codes, obj = _wide(X, codes0, m, h, None, method, 1, True)
    except _lib.RayuelaHipError as e:
        assert str(e)
        return
    assert codes.dtype == np.int16 and codes.min() >= 0 and codes.max() <= h - 1


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_sets():
    import rayuela_jl_amd.synth as synth
    return synth.sift_like(2000, 16, seed=41), synth.sift_like(500, 16, seed=43), synth.sift_like(20, 16, seed=42)


@pytest.mark.parametrize("norms", ["host", "device"])
def test_experiment_sr_cuda_query_base_past_256_codewords(rq, driver_sets, norms):
    from rayuela_jl_amd.experiments import experiment_sr_cuda_query_base
    Xt, _, Xq = driver_sets
    m, h, knn = 2, 320, 10
    (C, B, R, train_error, recall), opq_error = experiment_sr_cuda_query_base(
        Xt, Xq, None, m, h, niter=2, knn=knn, sr_method="SR_D", seed=2, ilsiter=2, npert=2, niter_init=2, norms=norms)
    print("experiment_sr_cuda_query_base (h = %d, norms %s): train_error %s, recall@1/10 %.3f %.3f"
          % (h, norms, train_error, recall[0], recall[knn - 1]))
    assert len(C) == m and C[0].shape == (h, 16) and R.shape == (16, 16)
    assert B.dtype == np.int16 and B.shape == (2000, m) and B.min() >= 1 and B.max() <= h
    assert train_error.shape == (3,) and np.isfinite(train_error).all() and len(opq_error) >= 1
    recall = np.asarray(recall)
    assert recall.shape[0] >= knn and np.all(recall >= 0) and np.all(recall <= 1) and np.all(np.diff(recall) >= 0)


def test_experiment_sr_cuda_past_256_codewords(rq, driver_sets):
    from rayuela_jl_amd.experiments import experiment_sr_cuda
    Xt, Xb, Xq = driver_sets
    m, h, knn = 2, 320, 10
    C, B, R, train_error, B_base, recall = experiment_sr_cuda(Xt, Xb, Xq, None, m, h, niter=2, knn=knn, sr_method="SR_C", seed=2,
                                                              ilsiter=2, npert=2, niter_init=2)
    assert B.dtype == np.int16 and B.min() >= 1 and B.max() <= h and B_base.shape == (500, m)
    assert B_base.min() >= 1 and B_base.max() <= h
    assert train_error.shape == (3,) and np.isfinite(train_error).all()
    recall = np.asarray(recall)
    assert np.all(recall >= 0) and np.all(recall <= 1)
