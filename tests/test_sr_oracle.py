"""CPU: the SR noise contract as tests/sr_oracle.py restates it ("SR noise") -- the variate against
scipy's inverse normal CDF, the moments of the stream on the seeds and shapes the GPU tests use, the schedules by hand,
and the host mirror's argument checks (which run before the library is touched)."""
import numpy as np
import pytest

import sr_oracle as so

# The variate is only ever added to f32 data and rounded to f32: half an f32 ulp of relative error is below the
# rounding already applied.  Derived, not tuned; the construction measures 1.13e-9.
BOUND = 2.0 ** -24

GPU_CASES = so.GPU_CASES


def _worst(u):
    from scipy.special import ndtri
    z = so.variate_from_u(u)
    assert np.isfinite(z).all()
    return float(np.max(np.abs(z - ndtri(u)) / np.maximum(1.0, np.abs(z))))


def test_variate_against_ndtri_on_seeded_keys():
    worst = 0.0
    for seed, kind, call in ((0, so.SR_C, 0), (1, so.SR_D, 3), (2 ** 63 + 5, so.SR_C, 10 ** 6)):
        u = so.uniform(so.words(seed, kind, call, np.arange(400_000, dtype=np.uint64)))
        assert u.min() > 0.0 and u.max() < 1.0
        worst = max(worst, _worst(u))
    print("worst |z - ndtri(u)| / max(1, |z|) over 1.2e6 seeded keys: %.3e" % worst)
    assert worst <= BOUND


def test_variate_against_ndtri_at_the_ends_and_the_seams():
    k = np.arange(200_000, dtype=np.uint64)
    lo = (k * np.uint64(2) + np.uint64(1)).astype(np.float64) * 2.0 ** -53          # the smallest representable u
    hi = 1.0 - lo                                                                     # the largest (1 - u is exact)
    assert lo[0] == 2.0 ** -53 and hi[0] == 1.0 - 2.0 ** -53
    w_lo, w_hi = _worst(lo), _worst(hi)
    z = so.variate_from_u(np.array([lo[0], hi[0]]))
    assert z[0] == -z[1] and 8.2 < z[1] < 8.22                                        # the stream spans +-8.21
    step = 2.0 ** -52                                                                 # the spacing of u
    seams = [so.P_LOW, so.P_HIGH, 0.5]
    w_seam = max(_worst(s + np.arange(-100_000, 100_001) * step) for s in seams)
    # the log's own seam: f crossing sqrt(1/2), reached by t = sqrt(1/2) 2^-e inside the tail range
    for e in (6, 20, 40):
        t = so.SQRT_HALF * 2.0 ** -e
        w_seam = max(w_seam, _worst(t + np.arange(-50_000, 50_001) * (t * 2.0 ** -52)))
    print("worst: smallest u %.3e, largest u %.3e, seams %.3e" % (w_lo, w_hi, w_seam))
    assert max(w_lo, w_hi, w_seam) <= BOUND


def test_the_written_out_log_against_numpy():
    rng = np.random.default_rng(5)
    x = np.exp(rng.uniform(np.log(2.0 ** -53), np.log(0.5), size=1_000_000))
    rel = np.abs(so.log_pos(x) - np.log(x)) / np.abs(np.log(x))
    print("worst relative error of the log: %.3e" % rel.max())
    assert rel.max() <= 2.0 ** -50


def test_streams_are_separated_by_kind_call_and_seed():
    idx = np.arange(1000, dtype=np.uint64)
    base = so.words(7, so.SR_C, 1, idx)
    for other in (so.words(7, so.SR_D, 1, idx), so.words(7, so.SR_C, 2, idx), so.words(8, so.SR_C, 1, idx),
                  so.words(7, so.SR_D, 0, idx)):
        assert not np.any(base == other)
    # SR_D's initial call (call 0, scheduled as iter 1) does not reuse loop iteration 1's draws
    assert not np.any(so.words(7, so.SR_D, 0, idx) == so.words(7, so.SR_D, 1, idx))


@pytest.mark.parametrize("n,d,seed,kind,call", GPU_CASES)
def test_moments_of_the_oracle_on_the_gpu_cases(n, d, seed, kind, call):
    """The mean of N variates within 6 / sqrt(N); each column's noise standard deviation within a relative
    6 / sqrt(2 n) of sigma_j * scale (six standard errors of a mean and of a sample standard deviation)."""
    N = n * d
    z = so.variate(seed, kind, call, np.arange(N, dtype=np.uint64)).reshape(n, d)
    assert abs(z.mean()) <= 6.0 / np.sqrt(N)
    if n < 2:
        return
    sigma = (np.random.default_rng(seed).uniform(0.5, 2.0, size=d)).astype(np.float32)
    scale = 0.25
    X = np.random.default_rng(seed + 100).standard_normal((n, d)).astype(np.float32)
    Y = so.perturb(X, sigma, scale, kind, seed, call)
    noise = Y.astype(np.float64) - X.astype(np.float64)
    want = sigma.astype(np.float64) * scale
    got = noise.std(axis=0, ddof=1)
    # Y is rounded to f32: that adds at most 2^-24 |Y| per element, far inside the statistical bound
    assert np.all(np.abs(got - want) <= 6.0 / np.sqrt(2 * n) * want), (got / want).tolist()


def test_perturb_slices_and_zero_scale():
    rng = np.random.default_rng(9)
    X = rng.standard_normal((300, 5)).astype(np.float32)
    sigma = rng.uniform(0.5, 2, size=5).astype(np.float32)
    Y = so.perturb(X, sigma, 1.0, so.SR_C, 3, 2)
    assert np.array_equal(so.perturb(X[100:180], sigma, 1.0, so.SR_C, 3, 2, row0=100), Y[100:180])
    assert np.array_equal(so.perturb(X, sigma, 0.0, so.SR_C, 3, 2), X)
    assert not np.array_equal(Y, X)


def test_schedule_values_by_hand(rq):
    from rayuela_jl_amd.SR import apply_schedule
    one = np.ones(3, dtype=np.float32)
    assert np.array_equal(apply_schedule(one, 0, 10, 1, 0.5), np.ones(3))
    assert np.array_equal(apply_schedule(one, 10, 10, 1, 0.5), np.zeros(3))
    assert np.array_equal(apply_schedule(one, 5, 10, 1, 2.0), np.full(3, 0.25))
    assert np.array_equal(apply_schedule(2 * one, 3, 10, 2, 0.5), np.ones(3))            # 1 / sqrt(1 + 3) = 0.5
    assert np.array_equal(apply_schedule(one, 4, 10, 3, 0.5), np.full(3, 0.25))         # 0.5^(4/2)
    assert np.allclose(apply_schedule(one, 3, 10, 3, 0.5), 0.5 ** 1.5, rtol=1e-15, atol=0)
    assert apply_schedule(one, 1, 4).dtype == np.float64                                  # Float32 .* Float64
    for it, niter, sched, p in ((0, 10, 1, 0.5), (7, 10, 1, 0.5), (3, 10, 2, 0.5), (5, 9, 3, 0.7), (0, 1, 3, 0.0)):
        assert apply_schedule(one, it, niter, sched, p)[0] == so.schedule(sched, it, niter, p)
    for bad in (0, 4, -1, "1", None, 1.5):
        with pytest.raises(ValueError):
            apply_schedule(one, 1, 10, bad, 0.5)
    with pytest.raises(ValueError):
        so.schedule(4, 1, 10, 0.5)
    for p in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            apply_schedule(one, 1, 10, 1, p)
    with pytest.raises(ValueError):
        apply_schedule(one, 1, 0, 1, 0.5)                  # niter = 0: schedule 1 divides by it
    with pytest.raises(ValueError):
        apply_schedule(one, 11, 10, 1, 0.5)                # a negative base
    with pytest.raises(ValueError):
        apply_schedule(one, 4000, 5000, 3, 1e300)          # p^(iter/2) overflows: the scale must come out finite
    assert apply_schedule(one, 5, 10, 2, 1e308)[0] == 0.0  # (1 + iter)^p overflows, its reciprocal is a finite 0
    assert rq.apply_schedule is apply_schedule


def _sr_args(n=50, d=8, m=2, h=256):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, d)).astype(np.float32)
    B = rng.integers(1, h + 1, size=(n, m)).astype(np.int16)
    return X, B, m, h, np.eye(d, dtype=np.float32)


def test_python_argument_checks_run_before_the_library(rq, monkeypatch):
    from rayuela_jl_amd import _lib

    def no_lib():
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", no_lib)
    X, B, m, h, R = _sr_args()

    def cuda(X=X, m=m, h=h, R=R, B=B, niter=2, ilsiter=1, icmiter=1, randord=True, npert=1, method="SR_D", schedule=1,
             p=0.5, nsplits=1):
        return rq.train_sr_cuda(X, m, h, R, B, None, niter, ilsiter, icmiter, randord, npert, method, schedule, p, nsplits)

    with pytest.raises(ValueError, match="SR method unknown"):
        cuda(method="SR_X")
    for sched in (0, 4, "1"):
        with pytest.raises(ValueError, match="Schedule unknown"):
            cuda(schedule=sched)
    with pytest.raises(ValueError, match="niter"):
        cuda(niter=0)
    for p in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="p must be finite"):
            cuda(p=p)
    with pytest.raises(TypeError):
        cuda(B=B.astype(np.int32))
    with pytest.raises(ValueError):
        cuda(B=B[:-1])                                      # rows
    with pytest.raises(ValueError):
        cuda(m=3)                                           # columns
    with pytest.raises(ValueError):
        cuda(R=np.eye(4, dtype=np.float32))
    with pytest.raises(ValueError):
        cuda(B=np.zeros_like(B))                            # one-based codes
    with pytest.raises(ValueError):
        cuda(npert=3)
    with pytest.raises(ValueError):
        cuda(nsplits=0)
    with pytest.raises(TypeError):
        cuda(X=X.astype(np.float64))
    with pytest.raises(ValueError, match="n >= 2"):
        cuda(X=X[:1], B=B[:1], method="SR_C")
    # train_sr: the same checks, B must be an array it can write into, cpp = true is built for h = 256
    with pytest.raises(ValueError, match="SR method unknown"):
        rq.train_sr(X, m, h, R, B, None, 2, 1, 1, True, 1, "sr_c", 0.5)
    with pytest.raises(TypeError):
        rq.train_sr(X, m, h, R, B.tolist(), None, 2, 1, 1, True, 1, "SR_C", 0.5)
    with pytest.raises(ValueError, match="h = 256"):
        rq.train_sr(X, m, 64, R, np.ones_like(B), None, 2, 1, 1, True, 1, "SR_C", 0.5)
    with pytest.raises(ValueError, match="p must be finite"):
        rq.train_sr(X, m, h, R, B, None, 2, 1, 1, True, 1, "SR_C", -0.5)
    # the perturbations
    with pytest.raises(ValueError, match="Schedule unknown"):
        rq.SR_C_perturb(X, 1, 10, 5)
    with pytest.raises(ValueError):
        rq.SR_C_perturb(X[:1], 1, 10)
    with pytest.raises(ValueError, match="niter"):
        rq.SR_D_perturb([np.zeros((4, 8), np.float32)] * 2, 1, 0)


def test_library_exports_the_sr_entries(rq):
    import ctypes
    handle = ctypes.CDLL(rq.lib_path())
    for name in ("rq_sr_std", "rq_sr_perturb", "rq_sr_schedule", "rq_train_sr", "rq_last_sr_timing"):
        assert hasattr(handle, name), "missing export: " + name


def test_library_schedule_and_its_refusals(rq):
    """rq_sr_schedule is host code: it runs without a device."""
    from rayuela_jl_amd.SR import sr_schedule
    import ctypes
    assert sr_schedule(1, 0, 10, 0.5) == 1.0 and sr_schedule(1, 10, 10, 0.5) == 0.0
    assert sr_schedule(2, 3, 10, 0.5) == 0.5 and sr_schedule(3, 4, 10, 0.5) == 0.25
    for sched, it, niter, p in ((1, 3, 7, 0.5), (2, 5, 7, 1.5), (3, 5, 7, 0.9)):
        assert sr_schedule(sched, it, niter, p) == so.schedule(sched, it, niter, p)
    out = ctypes.c_double(0)
    ptr = ctypes.cast(ctypes.byref(out), ctypes.c_void_p)
    L = rq.lib()
    for sched, it, niter, p in ((0, 1, 10, 0.5), (4, 1, 10, 0.5), (1, 1, 0, 0.5), (1, 11, 10, 0.5), (1, -1, 10, 0.5),
                                (1, 1, 10, -1.0), (1, 1, 10, float("nan")), (3, 1, 10, float("inf"))):
        assert L.rq_sr_schedule(ptr, sched, it, niter, p) != 0
    assert L.rq_sr_schedule(None, 1, 1, 10, 0.5) != 0
