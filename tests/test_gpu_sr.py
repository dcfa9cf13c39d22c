"""GPU: LSQ++ (rq_sr_std, rq_sr_perturb, rq_train_sr and their host mirrors): the noise bit for bit against
tests/sr_oracle.py, the standard deviation against numpy's f64 one, the training loop against its public steps composed
in Python, and the drivers end to end ("SR noise")."""
import numpy as np
import pytest

import sr_oracle as so
from sr_oracle import GPU_CASES

pytestmark = pytest.mark.gpu

KIND = {so.SR_C: "SR_C", so.SR_D: "SR_D"}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("n,d,seed,kind,call", GPU_CASES)
def test_perturb_equals_the_oracle_bit_for_bit(rq, n, d, seed, kind, call):
    """If an f64 divide or square root of the device were not correctly rounded, this comparison would say so."""
    from rayuela_jl_amd.SR import sr_perturb
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, d)) * 50).astype(np.float32)
    sigma = rng.uniform(0.5, 30.0, size=d).astype(np.float32)
    for scale in (0.0, 1e-3, 1.0):
        Y = sr_perturb(X, sigma, scale, KIND[kind], seed=seed, call=call)
        Y0 = so.perturb(X, sigma, scale, kind, seed, call)
        assert _same_bits(Y, Y0), "scale %g: %d of %d elements differ" % (scale, int((Y != Y0).sum()), Y.size)
        if scale == 0.0:
            assert np.array_equal(Y, X)
    Y1 = so.perturb(X, sigma, 1.0, kind, seed, call)
    # Y aliasing X
    Z = X.copy()
    out = sr_perturb(Z, sigma, 1.0, KIND[kind], seed=seed, call=call, out=Z)
    assert out is Z and _same_bits(Z, Y1)
    # a slice perturbed with row0 equals the same rows of the whole (the element counter starts at row0 * d)
    if n >= 3:
        a, b = n // 3, n - 1
        assert _same_bits(sr_perturb(X[a:b], sigma, 1.0, KIND[kind], seed=seed, call=call, row0=a), Y1[a:b])
    # another call, kind or seed is another stream
    assert not np.array_equal(sr_perturb(X, sigma, 1.0, KIND[kind], seed=seed, call=call + 1), Y1)
    assert not np.array_equal(sr_perturb(X, sigma, 1.0, KIND[1 - kind], seed=seed, call=call), Y1)
    assert not np.array_equal(sr_perturb(X, sigma, 1.0, KIND[kind], seed=seed + 1, call=call), Y1)


def test_perturb_refusals(rq):
    L = rq.lib()
    X = np.zeros((4, 3), np.float32)
    s = np.ones(3, np.float32)
    ok = (X.ctypes.data, X.ctypes.data, s.ctypes.data, 1.0, 4, 3, 0, 1, 0, 0)
    assert L.rq_sr_perturb(*ok) == 0

    def bad(**kw):
        names = ["Y", "X", "sigma", "scale", "n", "d", "kind", "seed", "call", "row0"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return L.rq_sr_perturb(*args)

    assert bad(kind=2) != 0 and bad(kind=-1) != 0 and bad(call=-1) != 0 and bad(row0=-1) != 0 and bad(d=0) != 0
    assert bad(n=-1) != 0 and bad(scale=float("inf")) != 0 and bad(scale=float("nan")) != 0 and bad(sigma=None) != 0
    assert bad(row0=2 ** 62) != 0 and bad(X=None) != 0
    assert bad(n=0) == 0


@pytest.mark.parametrize("n,d", [(2, 1), (5000, 7), (20000, 128), (2048, 96), (100001, 33)])
def test_std_against_numpy(rq, n, d):
    """Each entry is numpy's f64 standard deviation rounded to f32, or one of its two f32 neighbours: the f64 accumulation
    error (about n 2^-53) is far below half an f32 ulp, so only a rounding-boundary straddle can differ."""
    from rayuela_jl_amd.SR import sr_std
    rng = np.random.default_rng(n + d)
    X = (rng.standard_normal((n, d)) * rng.uniform(0.1, 100, size=d) + rng.uniform(-50, 50, size=d)).astype(np.float32)
    s1, s2 = sr_std(X), sr_std(X)
    assert s1.dtype == np.float32 and s1.shape == (d,) and _same_bits(s1, s2)
    want = np.std(X.astype(np.float64), axis=0, ddof=1).astype(np.float32)
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    print("std (%d, %d): %d of %d entries differ from the rounded numpy value" % (n, d, int((s1 != want).sum()), d))
    assert np.all((s1 == want) | (s1 == lo) | (s1 == hi))


def test_std_refuses_fewer_than_two_rows(rq):
    from rayuela_jl_amd.SR import sr_std
    L = rq.lib()
    X = np.ones((1, 4), np.float32)
    s = np.zeros(4, np.float32)
    assert L.rq_sr_std(s.ctypes.data, X.ctypes.data, 1, 4) != 0
    assert L.rq_sr_std(s.ctypes.data, X.ctypes.data, 0, 4) != 0
    assert L.rq_sr_std(s.ctypes.data, X.ctypes.data, 2, 0) != 0
    assert L.rq_sr_std(None, X.ctypes.data, 2, 2) != 0
    with pytest.raises(ValueError):
        sr_std(X)


def _rotation(d, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return q.astype(np.float32)


def _composed(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, randord, seed, method, schedule, p, clean,
              plain_last=False):
    """rq_train_sr's steps through the public entries (src/SR.jl:115-172).  plain_last: the last iteration's step is a
    plain update + encode (what schedule 1's zero scale must amount to)."""
    from rayuela_jl_amd.LSQ import encode_icm_u8
    from rayuela_jl_amd.OPQ import rotate
    from rayuela_jl_amd.SR import sr_perturb, sr_schedule, sr_std
    from rayuela_jl_amd.codebook_update import update_codebooks_u8
    n, d = X.shape
    RX = X if R is None else rotate(R, X)
    sigma_x = sr_std(RX) if method == "SR_C" else None

    def step(codes, call):
        if plain_last and call == niter:
            C = update_codebooks_u8(RX, codes, h)
        elif method == "SR_C":
            scale = sr_schedule(schedule, call, niter, p)
            C = update_codebooks_u8(sr_perturb(RX, sigma_x, scale, "SR_C", seed=seed, call=call), codes, h)
        else:
            scale = sr_schedule(schedule, 1 if call == 0 else call, niter, p)
            flat = update_codebooks_u8(RX, codes, h).reshape(m * h, d)
            sigma = sr_std(flat) / np.float32(m)
            C = sr_perturb(flat, sigma, scale, "SR_D", seed=seed, call=call).reshape(m, h, d)
        return C, encode_icm_u8(RX, codes, C, ilsiter, icmiter, npert, randord, seed=seed, t0=call * ilsiter)

    def qerror(codes, C):
        _, cost = encode_icm_u8(RX, codes, C, 0, 0, 0, False, with_cost=True)
        return np.mean(cost, dtype=np.float64)

    C, codes = step(codes0, 0)
    obj = []
    for it in range(1, niter + 1):
        obj.append(qerror(codes, C))
        C, codes = step(codes, it)
        if clean:
            C = update_codebooks_u8(RX, codes, h)
    obj.append(qerror(codes, C))
    if R is not None:
        C = rotate(np.ascontiguousarray(R.T), C.reshape(m * h, d)).reshape(m, h, d)     # C_i <- R C_i
    return C, codes, np.array(obj)


def _small(seed=12, n=4000, d=32, m=4, h=64):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    return X, rng.integers(0, h, size=(n, m)).astype(np.uint8), m, h


@pytest.mark.parametrize("schedule", [1, 2, 3])
@pytest.mark.parametrize("method", ["SR_C", "SR_D"])
def test_train_sr_equals_composed_steps(rq, method, schedule):
    from rayuela_jl_amd.SR import train_sr_u8
    X, codes0, m, h = _small()
    d = X.shape[1]
    niter, ilsiter, icmiter, npert, randord, seed, p = 3, 2, 2, 2, True, 9, 0.5
    for clean, rot in ((True, "seeded"), (False, "identity")):
        R = np.eye(d, dtype=np.float32) if rot == "identity" else _rotation(d, 5)
        C, codes, obj = train_sr_u8(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, method, schedule, p,
                                    clean, seed=seed)
        C0, codes_0, obj0 = _composed(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, randord, seed, method, schedule,
                                      p, clean)
        assert obj.shape == (niter + 1,) and np.isfinite(obj).all()
        assert np.array_equal(codes, codes_0)
        assert _same_bits(C, C0)
        assert np.allclose(obj, obj0, rtol=1e-12, atol=0)
        if rot == "identity":      # R = None skips the rotations; R = I rotates exactly
            Cn, codes_n, objn = train_sr_u8(X, codes0, m, h, None, niter, ilsiter, icmiter, randord, npert, method,
                                            schedule, p, clean, seed=seed)
            assert np.array_equal(codes_n, codes) and _same_bits(Cn, C) and _same_bits(objn, obj)
    # the noise matters: another seed trains another quantizer
    C2, _, _ = train_sr_u8(X, codes0, m, h, None, niter, ilsiter, icmiter, randord, npert, method, schedule, p, False,
                           seed=seed + 1)
    assert not np.array_equal(C2, C)


@pytest.mark.parametrize("method", ["SR_C", "SR_D"])
def test_schedule_one_ends_with_a_plain_lsq_step(rq, method):
    """Schedule 1's scale is 0 in the last iteration, so that SR step is a plain update + encode at the same t0."""
    from rayuela_jl_amd.SR import sr_schedule, train_sr_u8
    X, codes0, m, h = _small(seed=21)
    niter = 3
    assert sr_schedule(1, niter, niter, 0.5) == 0.0
    C, codes, obj = train_sr_u8(X, codes0, m, h, None, niter, 2, 2, True, 2, method, 1, 0.5, False, seed=5)
    C0, codes_0, obj0 = _composed(X, codes0, m, h, None, niter, 2, 2, 2, True, 5, method, 1, 0.5, False, plain_last=True)
    assert np.array_equal(codes, codes_0) and _same_bits(C, C0) and np.allclose(obj, obj0, rtol=1e-12, atol=0)


def test_train_sr_cuda_nsplits_and_in_place_rules(rq):
    rng = np.random.default_rng(13)
    n, d, m, h = 3000, 24, 4, 256
    X = rng.standard_normal((n, d)).astype(np.float32)
    B0 = rng.integers(1, h + 1, size=(n, m)).astype(np.int16)
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
        Ct, Bt, objt = rq.train_sr(X, m, h, R, B, None, 2, 2, 2, True, 2, method, 0.5, seed=4)
        assert np.array_equal(B, Bt) and not np.array_equal(B, B0)          # train_sr writes B in place
        assert objt.dtype == np.float32 and objt.shape == (3,)
        # train_sr is schedule 1 without the clean update: the first encode is shared, so obj[0] agrees
        assert objt[0] == res[0][2][0]


def test_perturbation_mirrors(rq):
    """SR_C_perturb / SR_D_perturb: the reference's signatures over rq_sr_std + rq_sr_perturb."""
    from rayuela_jl_amd.SR import sr_std
    rng = np.random.default_rng(17)
    X = rng.standard_normal((3000, 16)).astype(np.float32) * 4
    Y = rq.SR_C_perturb(X, 2, 10, 1, 0.5, seed=3)
    assert _same_bits(Y, so.perturb(X, sr_std(X), so.schedule(1, 2, 10, 0.5), so.SR_C, 3, 2))
    assert np.array_equal(rq.SR_C_perturb(X, 10, 10), X)
    C = [rng.standard_normal((64, 16)).astype(np.float32) for _ in range(3)]
    flat = np.concatenate(C, axis=0)
    want = so.perturb(flat, sr_std(flat) / np.float32(3), so.schedule(2, 4, 10, 0.5), so.SR_D, 3, 4).reshape(3, 64, 16)
    out = rq.SR_D_perturb(C, 4, 10, 2, 0.5, seed=3)
    assert all(o is c for o, c in zip(out, C)) and all(_same_bits(c, w) for c, w in zip(C, want))   # in place


@pytest.mark.parametrize("method", ["SR_C", "SR_D"])
def test_sift1m_shape_from_rvq_codes(rq, method):
    """1e6 x 128, m = 8: RVQ start codes, niter = 2, ilsiter = 2; obj finite, the final qerror below the start's,
    linscan_lsq runs on the result, every slot of the phase clock is positive."""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.SR import last_sr_timing, train_sr_u8
    n, d, m, h = 1_000_000, 128, 8, 256
    X = synth.sift_like(n, d, seed=31)
    Crvq, _, _ = rq.train_rvq(X[:20000], m, h, niter=4)
    Brvq, _ = rq.quantize_rvq(X, Crvq)
    q0 = rq.qerror(X, Brvq, Crvq)
    C, codes, obj = train_sr_u8(X, (Brvq - 1).astype(np.uint8), m, h, None, 2, 2, 4, True, 4, method, 1, 0.5, True, seed=3)
    t = last_sr_timing()
    q_end = rq.qerror(X, codes.astype(np.int16) + 1, list(C))
    print("SIFT1M shape %s: RVQ qerror %.6e, obj %s, final %.6e, phases (ms) %s"
          % (method, q0, obj, q_end, {k: round(v, 3) for k, v in t.items()}))
    assert np.isfinite(obj).all() and obj.shape == (3,)
    assert q_end < q0
    assert abs(q_end - obj[-1]) <= 1e-6 * q_end
    assert all(v > 0 for v in t.values()), t
    nrm = np.sum(C[np.arange(m)[None, :], codes.astype(np.int64)].sum(axis=1) ** 2, axis=1).astype(np.float32)
    Q = synth.sift_like(8, d, seed=32)
    dist, idx = rq.linscan_lsq(codes, Q, list(C), nrm, np.eye(d, dtype=np.float32), 100)
    assert idx.size == 800 and np.isfinite(dist).all()


def test_experiment_sr_cuda_query_base_on_a_small_set(rq):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.experiments import experiment_sr_cuda_query_base
    n, d, m, h, nq, knn = 6000, 32, 4, 256, 40, 100
    Xt = synth.sift_like(n, d, seed=41)
    Xq = synth.sift_like(nq, d, seed=42)
    d2 = ((Xq.astype(np.float64)[:, None, :] - Xt.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    gt = (d2.argmin(axis=1) + 1).astype(np.uint32)
    (C, B, R, train_error, recall), opq_error = experiment_sr_cuda_query_base(
        Xt, Xq, gt, m, h, niter=3, knn=knn, sr_method="SR_D", seed=2, ilsiter=2, niter_init=5)
    print("experiment_sr_cuda_query_base: train_error %s, recall@1/10/100 %.3f %.3f %.3f"
          % (train_error, recall[0], recall[9], recall[99]))
    assert len(C) == m and B.shape == (n, m) and R.shape == (d, d) and train_error.shape == (4,)
    assert np.isfinite(train_error).all() and len(opq_error) >= 1
    recall = np.asarray(recall)
    assert recall.shape[0] >= knn and np.all(np.diff(recall) >= 0) and recall[-1] <= 1.0
