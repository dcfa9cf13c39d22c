"""CPU restatement of the SR noise contract ("SR noise") -- test infrastructure.

Every operation from the 64-bit word to the variate is an integer operation on uint64, an f64 + - * / sqrt (one
IEEE-754 rounding each; numpy has no fused multiply-add) or a compare, so the kernel (contraction off) gives the same
bits.  The stream is keyed by the global element index: any slice of rows can be restated (`row0`), and nothing
depends on chunking.

  variate(seed, kind, call, idx)                       -> z f64, a standard normal variate per element index
  perturb(X, sigma, scale, kind, seed, call, row0=0)   -> Y f32 = (float)((double)X + z * ((double)sigma * scale))
  schedule(schedule, iter, niter, p)                   -> the f64 scale of apply_schedule
"""
import numpy as np

from rayuela_jl_amd.synth import splitmix64

_M64 = (1 << 64) - 1
SR_C, SR_D = 0, 1
DOMAIN = 0x53525F4E4F495345          # "SR_NOISE": separates the stream from the ICM streams of the same seed

# P. J. Acklam's rational approximation of the inverse normal CDF (relative error 1.15e-9)
_A = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02,
      -3.066479806614716e+01, 2.506628277459239e+00)
_B = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01,
      -1.328068155288572e+01)
_C = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00,
      4.374664141464968e+00, 2.938163982698783e+00)
_D = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00)
P_LOW = 0.02425
P_HIGH = 0.97575
SQRT_HALF = 0.7071067811865476
LN2 = 0.6931471805599453
# (n, d, seed, kind, call) of the perturbation cases tests/test_gpu_sr.py runs on the device
GPU_CASES = [(1, 1, 1, SR_C, 0), (5000, 7, 2, SR_C, 1), (5000, 7, 2, SR_D, 1), (20000, 128, 3, SR_C, 0),
             (20000, 128, 3, SR_D, 7), (256 * 8, 96, 4, SR_D, 0), (256 * 8, 96, 4, SR_C, 25)]

LOG_TERMS = 11                       # 1 + s2/3 + ... + s2^10/21


def _z(x):
    """splitmix64 of one Python int (wrap-around)."""
    return int(splitmix64(np.uint64(x & _M64)))


def stream_key(seed, kind, call):
    """The key of one perturbation call: z(z(z(seed) ^ DOMAIN) ^ (2 call + kind))."""
    return _z(_z(_z(seed) ^ DOMAIN) ^ ((2 * int(call) + int(kind)) & _M64))


def words(seed, kind, call, idx):
    """w = z(key ^ idx) for uint64 element indices idx."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return splitmix64(np.uint64(stream_key(seed, kind, call)) ^ idx)


def uniform(w):
    """u = (2k + 1) 2^-53 with k the top 52 bits: exact, strictly inside (0, 1), and 1 - u is exact."""
    k = np.asarray(w, dtype=np.uint64) >> np.uint64(12)
    return (k * np.uint64(2) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def log_pos(x):
    """log of positive normal f64 values: x = f 2^e by bit operations with f in [sqrt(1/2), sqrt(2)), s = (f-1)/(f+1),
    log f = 2 s (1 + s^2/3 + s^4/5 + ...) by Horner, then e ln2 is added."""
    x = np.asarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    e = (bits >> np.uint64(52)).astype(np.int64) - 1022
    f = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FE0000000000000)).view(np.float64)   # [0.5, 1)
    low = f < SQRT_HALF
    f = np.where(low, f * 2.0, f)
    e = np.where(low, e - 1, e)
    s = (f - 1.0) / (f + 1.0)
    s2 = s * s
    poly = np.full(x.shape, 1.0 / (2 * LOG_TERMS - 1))
    for k in range(LOG_TERMS - 2, -1, -1):
        poly = poly * s2 + 1.0 / (2 * k + 1)
    return (2.0 * s) * poly + e.astype(np.float64) * LN2


def variate_from_u(u):
    u = np.asarray(u, dtype=np.float64)
    # central branch
    q = u - 0.5
    r = q * q
    num = _A[0]
    for a in _A[1:]:
        num = num * r + a
    den = _B[0]
    for b in _B[1:]:
        den = den * r + b
    den = den * r + 1.0
    zc = (num * q) / den
    # tails: t = min(u, 1 - u), q = sqrt(-2 log t)
    upper = u > P_HIGH
    t = np.where(upper, 1.0 - u, u)
    t = np.where(t > 0.5, 0.5, t)                    # central lanes: any valid argument (the result is discarded)
    q = np.sqrt(-2.0 * log_pos(t))
    num = _C[0]
    for c in _C[1:]:
        num = num * q + c
    den = _D[0]
    for dd in _D[1:]:
        den = den * q + dd
    den = den * q + 1.0
    zt = num / den
    zt = np.where(upper, -zt, zt)
    return np.where((u < P_LOW) | upper, zt, zc)


def variate(seed, kind, call, idx):
    return variate_from_u(uniform(words(seed, kind, call, idx)))


def perturb(X, sigma, scale, kind, seed, call, row0=0):
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    idx = (np.uint64(row0 * d) + np.arange(n * d, dtype=np.uint64)).reshape(n, d)
    z = variate(seed, kind, call, idx)
    amp = np.asarray(sigma, dtype=np.float32).astype(np.float64) * np.float64(scale)
    return (X.astype(np.float64) + z * amp[None, :]).astype(np.float32)


def schedule(sched, it, niter, p):
    """apply_schedule's factor (src/SR_perturbations.jl:4-25) in f64."""
    if sched == 1:
        return (1.0 - it / niter) ** p
    if sched == 2:
        return 1.0 / (1.0 + it) ** p
    if sched == 3:
        return float(p) ** (it / 2.0)
    raise ValueError("Schedule unknown: %r" % (sched,))
