"""Host mirror of LSQ++, the stochastic relaxations of LSQ: apply_schedule, SR_D_perturb, SR_C_perturb
(src/SR_perturbations.jl:4-73), train_sr (src/SR.jl:4-84) and train_sr_cuda (:88-176).

The training loop is device-resident (rq_train_sr; rq_train_sr_wide over 16-bit codes past 256 codewords per codebook, DESIGN.md
section 4.27); the contract is DESIGN.md section 2 ("SR noise").  Layouts are LSQ's:
X (n, d) float32, codebooks an m-long list of (h, d) arrays, codes (n, m) Int16 one-based.  The reference draws its noise
from Julia's global randn; here it is a counter-based standard normal variate keyed by (seed, method, perturbation call,
global element index), so results depend on neither nsplits, the chunking nor the run."""
import ctypes
import math

import numpy as np

from . import _lib
from .LSQ import _check, _check_wide_train, _stack
from .utils import _as_f32

METHODS = ("SR_C", "SR_D")          # src/SR.jl:27; the C ABI's RQ_SR_C = 0, RQ_SR_D = 1
SR_RECOMPUTE = 1                    # RQ_SR_RECOMPUTE: rq_train_sr_wide computes every codebook update from scratch
_U64 = (1 << 64) - 1


def _method(method):
    if method not in METHODS:
        raise ValueError("SR method unknown: %r" % (method,))
    return METHODS.index(method)


def _scale(iter, niter, schedule, p):
    """apply_schedule's factor in f64.  Every check runs here, before the library is touched."""
    if isinstance(schedule, (bool, str)) or schedule not in (1, 2, 3):
        raise ValueError("Schedule unknown: %r" % (schedule,))
    schedule = int(schedule)
    iter, niter, p = int(iter), int(niter), float(p)
    if niter < 1:
        raise ValueError("niter must be >= 1; got %d" % niter)
    if iter < 0 or (schedule == 1 and iter > niter):
        raise ValueError("iter must be in 0..niter=%d; got %d" % (niter, iter))
    if not (math.isfinite(p) and p >= 0):
        raise ValueError("p must be finite and >= 0; got %r" % p)
    base, power = ((1.0 - iter / niter, p), (1.0 + iter, p), (p, iter / 2.0))[schedule - 1]
    try:
        v = base ** power
    except OverflowError:           # C's pow returns inf where Python raises
        v = math.inf
    if schedule == 2:
        v = 1.0 / v
    if not math.isfinite(v):
        raise ValueError("schedule %d gives a non-finite scale at iter=%d, p=%r" % (schedule, iter, p))
    return v


def apply_schedule(stdev, iter, niter, schedule=1, p=0.5):
    """apply_schedule(stdev, iter, niter, schedule=1, p=0.5) -> stdev scaled       (src/SR_perturbations.jl:4-25)

    1: stdev (1 - iter/niter)^p, 2: stdev / (1 + iter)^p, 3: stdev p^(iter/2), in float64 like the reference's
    Float32-by-Float64 products.  Schedule 2 multiplies by the reciprocal where the reference divides (at most one f64
    rounding apart)."""
    return np.asarray(stdev).astype(np.float64) * _scale(iter, niter, schedule, p)


def sr_schedule(schedule, iter, niter, p):
    """The library's own factor (rq_sr_schedule; host code, no device): what rq_train_sr uses."""
    _scale(iter, niter, schedule, p)
    out = ctypes.c_double(0)
    _lib.check(_lib.lib().rq_sr_schedule(ctypes.cast(ctypes.byref(out), ctypes.c_void_p), int(schedule), int(iter),
                                         int(niter), float(p)))
    return out.value


def sr_std(X):
    """Per-column sample standard deviation of X (n, d) on the device (rq_sr_std): Statistics.std(X, dims=2) -> (d,) f32."""
    X = _as_f32(X, "X")
    if X.ndim != 2 or X.shape[1] < 1:
        raise ValueError("X must be (n, d) with d >= 1; got %s" % (X.shape,))
    if X.shape[0] < 2:
        raise ValueError("the sample standard deviation needs n >= 2 rows; got %d" % X.shape[0])
    X = np.ascontiguousarray(X)
    sigma = np.empty(X.shape[1], dtype=np.float32)
    _lib.check(_lib.lib().rq_sr_std(sigma.ctypes.data, X.ctypes.data, X.shape[0], X.shape[1]))
    return sigma


def sr_perturb(X, sigma, scale, method, seed=0, call=0, row0=0, out=None):
    """Y = (float)((double)X + z ((double)sigma * scale)) on the device (rq_sr_perturb); `out` may be X itself."""
    X = _as_f32(X, "X")
    kind = _method(method)
    if X.ndim != 2 or X.shape[1] < 1:
        raise ValueError("X must be (n, d) with d >= 1; got %s" % (X.shape,))
    n, d = X.shape
    sigma = np.ascontiguousarray(_as_f32(sigma, "sigma"))
    if sigma.shape != (d,):
        raise ValueError("sigma must be (d,) = (%d,); got %s" % (d, sigma.shape))
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError("scale must be finite; got %r" % scale)
    if int(call) < 0 or int(row0) < 0:
        raise ValueError("call and row0 must be >= 0; got %d, %d" % (call, row0))
    if not X.flags.c_contiguous:
        X = np.ascontiguousarray(X)
    if out is None:
        out = np.empty_like(X)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == X.shape and out.flags.c_contiguous):
        raise ValueError("out must be a C-contiguous float32 array of X's shape")
    _lib.check(_lib.lib().rq_sr_perturb(out.ctypes.data, X.ctypes.data, sigma.ctypes.data, scale, n, d, kind,
                                        int(seed) & _U64, int(call), int(row0)))
    return out


def SR_C_perturb(X, iter, niter, schedule=1, p=0.5, seed=0, call=None):
    """SR_C_perturb(X, iter, niter, schedule=1, p=0.5) -> Y       (src/SR_perturbations.jl:52-73)

    X (n, d) float32.  Y = X + noise with the per-dimension standard deviation of X scaled by the schedule.  `call`
    numbers the draw (default: iter), so two calls of one iteration can differ."""
    X = _as_f32(X, "X")
    scale = _scale(iter, niter, schedule, p)
    if X.ndim != 2 or X.shape[0] < 2:
        raise ValueError("SR_C_perturb needs X (n, d) with n >= 2 rows; got %s" % (X.shape,))
    call = int(iter) if call is None else int(call)
    return sr_perturb(X, sr_std(X), scale, "SR_C", seed=seed, call=call)


def SR_D_perturb(C, iter, niter, schedule=1, p=0.5, seed=0, call=None):
    """SR_D_perturb(C, iter, niter, schedule=1, p=0.5) -> C       (src/SR_perturbations.jl:27-49)

    C an m-long list of (h, d) codebooks.  The standard deviation is that of all m h codewords per dimension, divided by
    m.  Like the reference, the codebooks passed as float32 arrays are perturbed in place and returned."""
    scale = _scale(iter, niter, schedule, p)
    Cs = _stack(C)
    m, h, d = Cs.shape
    flat = Cs.reshape(m * h, d)
    sigma = sr_std(flat) / np.float32(m)
    call = int(iter) if call is None else int(call)
    new = sr_perturb(flat, sigma, scale, "SR_D", seed=seed, call=call).reshape(m, h, d)
    if isinstance(C, np.ndarray):
        if C.dtype == np.float32:
            C[...] = new
            return C
        return new
    out = []
    for i, c in enumerate(C):
        if isinstance(c, np.ndarray) and c.dtype == np.float32:
            c[...] = new[i]
            out.append(c)
        else:
            out.append(new[i])
    return out


def _check_sr(X, B, m, h, R, niter, ilsiter, icmiter, npert, method, schedule, p, nsplits, one_based, wide=False):
    """Every argument check of the training loop runs here, before the library (and the device) is touched.  wide: the loop
    over 16-bit codes (LSQ._check_wide_train's shape rule) instead of the byte one (h <= 256)."""
    kind = _method(method)
    if X.ndim != 2:
        raise ValueError("X must be (n, d); got %s" % (X.shape,))
    n, d = X.shape
    if wide:
        _check_wide_train(X, B, m, h, ilsiter, icmiter, npert, nsplits, one_based=one_based)
    else:
        _check(X, np.empty((m, h, d), np.float32), B, ilsiter, icmiter, npert, nsplits, 0, one_based=one_based)
    if int(niter) < 1:
        raise ValueError("niter must be >= 1 (schedule 1 divides by it); got %d" % niter)
    for it in range(int(niter) + 1):
        _scale(1 if (it == 0 and kind == 1) else it, niter, schedule, p)
    if kind == 0 and n < 2:
        raise ValueError("SR_C needs n >= 2 rows for the standard deviation; got %d" % n)
    if R is not None:
        R = _as_f32(R, "R")
        if R.shape != (d, d):
            raise ValueError("R must be (d, d) = (%d, %d); got %s" % (d, d, R.shape))
        R = np.ascontiguousarray(R)
    return kind, R


def train_sr_u8(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, method, schedule=1, p=0.5,
                clean_update=True, seed=0, nsplits=1):
    """The device-resident loop (rq_train_sr) on zero-based uint8 codes: (C (m, h, d), codes, obj float64 (niter + 1,)).
    R None = identity (no rotation)."""
    X = np.ascontiguousarray(_as_f32(X, "X"))
    n, d = X.shape
    B = np.asarray(codes0)
    kind, R = _check_sr(X, B, m, h, R, niter, ilsiter, icmiter, npert, method, schedule, p, nsplits, one_based=False)
    codes = np.array(B, dtype=np.uint8, order="C")
    C = np.empty((m, h, d), dtype=np.float32)
    obj = np.zeros(int(niter) + 1, dtype=np.float64)
    _lib.check(_lib.lib().rq_train_sr(C.ctypes.data, codes.ctypes.data, obj.ctypes.data, X.ctypes.data,
                                      None if R is None else R.ctypes.data, n, d, m, h, int(niter), int(ilsiter),
                                      int(icmiter), int(npert), 1 if randord else 0, kind, int(schedule), float(p),
                                      1 if clean_update else 0, int(seed) & _U64, int(nsplits)))
    return C, codes, obj


def train_sr_u16(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, method, schedule=1, p=0.5,
                 clean_update=True, seed=0, nsplits=1, recompute=False):
    """train_sr_u8 over zero-based int16 codes for any 2 <= h <= 32767 with m * h <= 16384 whose encoder tables fit
    (LSQ.wide_fits): rq_train_sr_wide, the int16 kernels at every h.  At h <= 256 C, codes and obj equal
    train_sr_u8's bit for bit.  With the clean update a step opens with an update over the codes the previous step closed with;
    that repeated work is not done again unless recompute is set.  Both settings give the same bits (last_sr_stats counts)."""
    X = np.ascontiguousarray(_as_f32(X, "X"))
    B = np.asarray(codes0)
    kind, R = _check_sr(X, B, m, h, R, niter, ilsiter, icmiter, npert, method, schedule, p, nsplits, one_based=False,
                        wide=True)
    n, d = X.shape
    codes = np.array(B, dtype=np.int16, order="C")
    C = np.empty((m, h, d), dtype=np.float32)
    obj = np.zeros(int(niter) + 1, dtype=np.float64)
    _lib.check(_lib.lib().rq_train_sr_wide(C.ctypes.data, codes.ctypes.data, obj.ctypes.data, X.ctypes.data,
                                           None if R is None else R.ctypes.data, n, d, m, h, int(niter), int(ilsiter),
                                           int(icmiter), int(npert), 1 if randord else 0, kind, int(schedule), float(p),
                                           1 if clean_update else 0, int(seed) & _U64, int(nsplits), 0,
                                           SR_RECOMPUTE if recompute else 0))
    return C, codes, obj


def _train(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, method, schedule, p, clean_update, seed, nsplits, V):
    X = _as_f32(X, "X")
    B = np.asarray(B)
    if B.dtype != np.int16:
        raise TypeError("B must be an Int16 array of one-based codes")
    wide = int(h) > 256
    _check_sr(X, B, m, h, R, niter, ilsiter, icmiter, npert, method, schedule, p, nsplits, one_based=True, wide=wide)
    if V:
        print("Doing local search with %d codebooks, %d perturbations, %d icm iterations and random order = %s"
              % (m, npert, icmiter, bool(randord)))
    if wide:      # past 256 codewords: the loop over 16-bit codes (rq_train_sr_wide); h <= 256 stays on the byte loop
        C, codes, obj = train_sr_u16(X, B - 1, m, h, R, niter, ilsiter, icmiter, randord, npert, method, schedule, p,
                                     clean_update, seed=seed, nsplits=nsplits)
    else:
        C, codes, obj = train_sr_u8(X, (B - 1).astype(np.uint8), m, h, R, niter, ilsiter, icmiter, randord, npert, method,
                                    schedule, p, clean_update, seed=seed, nsplits=nsplits)
    if V:
        for it, o in enumerate(obj, 1):
            print("%3d %e " % (it, o))
    return list(C), codes.astype(np.int16) + 1, obj.astype(np.float32)


def train_sr(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, method, p, cpp=True, V=False, seed=0):
    """train_sr(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, method, p, cpp=true, V=false) -> C, B, objarray
                                                                                               (src/SR.jl:4-84)
    method "SR_C" (noise on the data) or "SR_D" (noise on the codebooks).  As committed the reference passes p where
    the schedule is expected (:35, :66) and cannot run; its evident intent, schedule 1 with power p, is what runs here.
    No codebook update follows the encode of an iteration.  The C argument is ignored (the reference overwrites it).
    Returns C (m-long list of (h, d)), B (Int16 one-based, also written into the B passed in, as encoding_icm does)
    and objarray (niter + 1,) float32.  cpp=True requires h = 256; both settings run the same device loop.  cpp=False takes
    any 2 <= h <= 32767 with m * h <= 16384 whose encoder tables fit (LSQ.wide_fits): past 256 codewords the loop over 16-bit
    codes runs (rq_train_sr_wide)."""
    if not (isinstance(B, np.ndarray) and B.dtype == np.int16):
        raise TypeError("B must be an Int16 numpy array (it is updated in place)")
    if cpp and h != 256:
        raise ValueError("train_sr with cpp=true requires h = 256 codewords; got h=%d" % h)
    Cn, Bn, obj = _train(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, method, 1, p, False, seed, 1, V)
    B[...] = Bn
    return Cn, Bn, obj


def train_sr_cuda(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, method, schedule, p=0.5, nsplits=1, V=False,
                  seed=0):
    """train_sr_cuda(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, method, schedule, p=0.5, nsplits=1,
                     V=false) -> C, B, objarray                                                (src/SR.jl:88-176)
    As train_sr with the schedule (1, 2 or 3) chosen by the caller and a clean codebook update after every iteration's
    encode (:166).  B is left untouched (encode_icm_cuda returns new codes); the result does not depend on nsplits.  Past 256
    codewords the loop over 16-bit codes runs, as in train_sr(cpp=False)."""
    return _train(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, method, schedule, p, True, seed, nsplits, V)


SR_PHASES = ["std_ms", "perturb_ms", "update_ms", "encode_ms", "obj_ms", "other_ms"]


def last_sr_timing():
    """Phase milliseconds of this thread's last training call (rq_last_sr_timing), summed over the call.  other_ms: the
    uploads, R'X and the rotation back."""
    out = (ctypes.c_double * 6)()
    _lib.check(_lib.lib().rq_last_sr_timing(ctypes.cast(out, ctypes.c_void_p), 6))
    return dict(zip(SR_PHASES, [float(v) for v in out]))


SR_UPDATES = ["full", "reused", "skipped"]


def last_sr_stats():
    """The codebook updates of this thread's last training call (rq_last_sr_stats): computed in full, computed from the kept
    Cholesky factor and row sort, skipped outright.  The byte loop computes every update in full."""
    out = (ctypes.c_int64 * 3)()
    _lib.check(_lib.lib().rq_last_sr_stats(ctypes.cast(out, ctypes.c_void_p), 3))
    return dict(zip(SR_UPDATES, [int(v) for v in out]))
