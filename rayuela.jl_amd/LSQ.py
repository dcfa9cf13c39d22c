"""Host mirror of the LSQ encoder: encoding_icm (src/LSQ.jl:272-302), encode_icm_cuda (src/LSQ_GPU.jl:218-264),
veccost / qerror (src/qerrors.jl) for full-dimensional codebooks.

Iterated local search around ICM on the device (rq_encode_icm; rq_encode_icm_wide over 16-bit codes past 256 codewords per
codebook); the contract is DESIGN.md section 2.  Codebooks C are an
m-long list of (h, d) arrays (memory image of Julia's d-by-h matrices) or one (m, h, d) array; codes are (n, m) Int16
one-based like the reference's m-by-n matrices.  Random numbers are counter-based (`seed`), keyed by the global row index
and the ILS iteration, so results depend on neither nsplits nor checkpoints."""
import ctypes

import numpy as np

from . import _lib
from .codebook_update import MAX_MH
from .utils import MAX_H16, _as_f32

MAX_M = 16
SCRATCH_BYTES = 2 << 30      # ICM_SCRATCH_BYTES: the tables and one chunk's unaries, per device and stream


def wide_fits(m, h):
    """rq_encode_icm_wide's fit rule: the binaries [m][m][h][HS], the self-products [m][h] and four rows of unaries [m][HS]
    (f32, HS = 64 * ceil(h / 64)) within the scratch budget."""
    HS = 64 * ((h + 63) // 64)
    return m * m * h * HS * 4 + m * h * 4 + 4 * m * HS * 4 <= SCRATCH_BYTES


def _stack(C):
    if isinstance(C, np.ndarray) and C.ndim == 3:
        Cs = np.ascontiguousarray(_as_f32(C, "C"))
    else:
        Cs = [np.ascontiguousarray(_as_f32(c, "C[i]")) for c in C]
        if not Cs or len({c.shape for c in Cs}) != 1:
            raise ValueError("all LSQ codebooks must be d x h")
        Cs = np.ascontiguousarray(np.stack(Cs, axis=0))
    return Cs


def _check(X, Cs, codes0, ilsiter, icmiter, npert, nsplits, t0, one_based, wide=False):
    """Every argument check runs here, before the library (and the device) is touched.  wide: the encoder over 16-bit codes
    (2 <= h <= MAX_H16 and the tables within the scratch budget) instead of the byte one (h <= 256)."""
    n, d = X.shape
    m, h, d2 = Cs.shape
    if d2 != d:
        raise ValueError("codebooks are %d-dimensional, data is %d-dimensional" % (d2, d))
    if not 1 <= m <= MAX_M:
        raise ValueError("LSQ encoding covers 1 <= m <= %d codebooks; got m=%d" % (MAX_M, m))
    if not 2 <= h <= (MAX_H16 if wide else 256):
        raise ValueError("LSQ encoding covers 2 <= h <= %d codewords; got h=%d" % (MAX_H16 if wide else 256, h))
    if wide and not wide_fits(m, h):
        raise ValueError("LSQ encoding keeps m*m*h*h pair products in %d bytes of scratch; m=%d, h=%d do not fit"
                         % (SCRATCH_BYTES, m, h))
    for name, v in (("ilsiter", ilsiter), ("icmiter", icmiter), ("t0", t0)):
        if int(v) < 0:
            raise ValueError("%s must be >= 0; got %d" % (name, v))
    if not 0 <= int(npert) <= m:
        raise ValueError("npert must be in 0..m=%d; got %d" % (m, npert))
    if int(nsplits) < 1:
        raise ValueError("nsplits must be >= 1; got %d" % nsplits)
    B = np.asarray(codes0)
    if B.shape != (n, m):
        raise ValueError("codes must be (n, m) = (%d, %d); got %s" % (n, m, B.shape))
    lo = 1 if one_based else 0
    if B.size and (B.min() < lo or B.max() > h - 1 + lo):
        raise ValueError("codes must be in %d..%d" % (lo, h - 1 + lo))
    return n, d, m, h


def encode_icm_u8(X, codes0, C, ilsiter, icmiter, npert, randord, seed=0, t0=0, nsplits=1, with_cost=False):
    """Zero-based uint8 codes in and out: ILS iterations t0 .. t0+ilsiter-1.  with_cost -> (codes, per-row veccost)."""
    X = _as_f32(X, "X")
    Cs = _stack(C)
    n, d, m, h = _check(X, Cs, codes0, ilsiter, icmiter, npert, nsplits, t0, one_based=False)
    B = np.ascontiguousarray(codes0, dtype=np.uint8)
    out = np.empty((n, m), dtype=np.uint8)
    cost = np.empty(n, dtype=np.float32) if with_cost else None
    _lib.check(_lib.lib().rq_encode_icm(out.ctypes.data, B.ctypes.data, None if cost is None else cost.ctypes.data,
                                        X.ctypes.data, Cs.ctypes.data, n, d, m, h, int(ilsiter), int(icmiter),
                                        int(npert), 1 if randord else 0, int(seed) & ((1 << 64) - 1), int(t0),
                                        int(nsplits)))
    return (out, cost) if with_cost else out


def encode_icm_u16(X, codes0, C, ilsiter, icmiter, npert, randord, seed=0, t0=0, nsplits=1, with_cost=False):
    """encode_icm_u8 over zero-based int16 codes for any 2 <= h <= 32767 whose tables fit (wide_fits): rq_encode_icm_wide, a kernel
    of its own at every h.  At h <= 256 codes and costs equal encode_icm_u8's bit for bit."""
    X = _as_f32(X, "X")
    Cs = _stack(C)
    n, d, m, h = _check(X, Cs, codes0, ilsiter, icmiter, npert, nsplits, t0, one_based=False, wide=True)
    B = np.ascontiguousarray(codes0, dtype=np.int16)
    out = np.empty((n, m), dtype=np.int16)
    cost = np.empty(n, dtype=np.float32) if with_cost else None
    _lib.check(_lib.lib().rq_encode_icm_wide(out.ctypes.data, B.ctypes.data, None if cost is None else cost.ctypes.data,
                                             X.ctypes.data, Cs.ctypes.data, n, d, m, h, int(ilsiter), int(icmiter),
                                             int(npert), 1 if randord else 0, int(seed) & ((1 << 64) - 1), int(t0),
                                             int(nsplits), 0))
    return (out, cost) if with_cost else out


def _encode0(X, B1, Cs, *args, **kw):
    """The mirrors' encode on ONE-based codes B1 -> zero-based codes (+ cost): the byte kernel at h <= 256, else the wide one."""
    if Cs.shape[1] > 256:
        return encode_icm_u16(X, (B1 - 1).astype(np.int16), Cs, *args, **kw)
    return encode_icm_u8(X, (B1 - 1).astype(np.uint8), Cs, *args, **kw)


def encoding_icm(X, oldB, C, ilsiter, icmiter, randord, npert, cpp=True, V=False, seed=0):
    """encoding_icm(X, oldB, C, ilsiter, icmiter, randord, npert, cpp=true, V=false) -> B     (src/LSQ.jl:272-302)

    X (n, d) float32, oldB (n, m) Int16 one-based, C m-long list of (h, d) codebooks.  Returns B (n, m) Int16 one-based
    and, like the reference, writes it into oldB too.  cpp=True requires h = 256 (the reference's C++ path is built
    for H = 256); both settings run the same device kernel.  cpp=False takes any 2 <= h <= 32767 whose tables fit
    (wide_fits): past 256 codewords the encoder over 16-bit codes runs (rq_encode_icm_wide)."""
    X = _as_f32(X, "X")
    Cs = _stack(C)
    if not (isinstance(oldB, np.ndarray) and oldB.dtype == np.int16):
        raise TypeError("oldB must be an Int16 numpy array (it is updated in place)")
    if cpp and Cs.shape[1] != 256:
        raise ValueError("encoding_icm with cpp=true requires h = 256 codewords; got h=%d" % Cs.shape[1])
    _check(X, Cs, oldB, ilsiter, icmiter, npert, 1, 0, one_based=True, wide=Cs.shape[1] > 256)
    codes = _encode0(X, oldB, Cs, ilsiter, icmiter, npert, randord, seed=seed)
    B = codes.astype(np.int16) + 1
    oldB[...] = B
    if V:
        print(" ILS encoding: %d iterations done" % ilsiter)
    return B


def encode_icm_cuda(RX, B, C, ilsiters, icmiter, npert, randord, nsplits=2, V=False, seed=0):
    """encode_icm_cuda(RX, B, C, ilsiters, icmiter, npert, randord, nsplits=2, V=false) -> Bs, objs
                                                                                   (src/LSQ_GPU.jl:218-264)
    Runs max(ilsiters) ILS iterations; Bs[i] (Int16 one-based) are the codes after ilsiters[i] iterations and objs[i]
    their qerror (mean veccost).  B is left untouched.  Each checkpoint continues the previous call's random stream
    (t0), so the result equals one uninterrupted run."""
    X = _as_f32(RX, "RX")
    Cs = _stack(C)
    its = [int(i) for i in ilsiters]
    if not its or min(its) < 1:
        raise ValueError("ilsiters must list positive iteration counts")
    B = np.asarray(B)
    _check(X, Cs, B, max(its), icmiter, npert, nsplits, 0, one_based=True, wide=Cs.shape[1] > 256)
    cur = B
    Bs, objs = [None] * len(its), np.zeros(len(its), dtype=np.float32)
    done = 0
    for stop in sorted(set(its)):
        cur, cost = _encode0(X, cur, Cs, stop - done, icmiter, npert, randord, seed=seed, t0=done, nsplits=nsplits,
                             with_cost=True)
        cur = cur.astype(np.int16) + 1
        done = stop
        obj = float(np.mean(cost, dtype=np.float64))
        for i, s in enumerate(its):
            if s == stop:
                Bs[i] = cur.copy()
                objs[i] = obj
        if V:
            print(" ILS iteration %d/%d done, qerror %e" % (stop, max(its), obj))
    return Bs, objs


def veccost(X, B, C):
    """Per-row squared reconstruction error (src/qerrors.jl:36-66), B (n, m) Int16 one-based; the device's order of
    the f32 sums.  Runs the encode kernel with zero iterations."""
    X = _as_f32(X, "X")
    Cs = _stack(C)
    B = np.asarray(B)
    _check(X, Cs, B, 0, 0, 0, 1, 0, one_based=True, wide=Cs.shape[1] > 256)
    _, cost = _encode0(X, B, Cs, 0, 0, 0, False, with_cost=True)
    return cost


def qerror(X, B, C):
    """Mean veccost (src/qerrors.jl)."""
    return float(np.mean(veccost(X, B, C), dtype=np.float64))


def train_lsq_u8(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, seed=0, nsplits=1):
    """The device-resident training loop (rq_train_lsq) on zero-based uint8 codes: (C (m, h, d), codes, obj float64).
    R None = identity (no rotation)."""
    X = _as_f32(X, "X")
    n, d = X.shape
    B = np.asarray(codes0)
    _check(X, np.empty((m, h, d), np.float32), B, ilsiter, icmiter, npert, nsplits, 0, one_based=False)
    if int(niter) < 0:
        raise ValueError("niter must be >= 0; got %d" % niter)
    if R is not None:
        R = _as_f32(R, "R")
        if R.shape != (d, d):
            raise ValueError("R must be (d, d) = (%d, %d); got %s" % (d, d, R.shape))
    codes = np.array(B, dtype=np.uint8, order="C")
    C = np.empty((m, h, d), dtype=np.float32)
    obj = np.zeros(int(niter), dtype=np.float64)
    _lib.check(_lib.lib().rq_train_lsq(C.ctypes.data, codes.ctypes.data, obj.ctypes.data if niter else None,
                                       X.ctypes.data, None if R is None else R.ctypes.data, n, d, m, h, int(niter),
                                       int(ilsiter), int(icmiter), int(npert), 1 if randord else 0,
                                       int(seed) & ((1 << 64) - 1), int(nsplits)))
    return C, codes, obj


def _check_wide_train(X, B, m, h, ilsiter, icmiter, npert, nsplits, one_based):
    """_check for the loop over 16-bit codes, and the update's own limit m * h <= MAX_MH"""
    _check(X, np.broadcast_to(np.float32(0), (m, h, X.shape[1])), B, ilsiter, icmiter, npert, nsplits, 0, one_based=one_based,
           wide=True)
    if m * h > MAX_MH:
        raise ValueError("the LSQ update solves m * h <= %d unknowns per dimension; got m=%d, h=%d" % (MAX_MH, m, h))


def train_lsq_u16(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, seed=0, nsplits=1):
    """train_lsq_u8 over zero-based int16 codes for any 2 <= h <= 32767 with m * h <= 16384 whose encoder tables fit (wide_fits):
    rq_train_lsq_wide, the int16 kernels at every h.  At h <= 256 C and obj equal train_lsq_u8's bit for
    bit, and so do the codes."""
    X = _as_f32(X, "X")
    n, d = X.shape
    B = np.asarray(codes0)
    _check_wide_train(X, B, m, h, ilsiter, icmiter, npert, nsplits, one_based=False)
    if int(niter) < 0:
        raise ValueError("niter must be >= 0; got %d" % niter)
    if R is not None:
        R = _as_f32(R, "R")
        if R.shape != (d, d):
            raise ValueError("R must be (d, d) = (%d, %d); got %s" % (d, d, R.shape))
    codes = np.array(B, dtype=np.int16, order="C")
    C = np.empty((m, h, d), dtype=np.float32)
    obj = np.zeros(int(niter), dtype=np.float64)
    _lib.check(_lib.lib().rq_train_lsq_wide(C.ctypes.data, codes.ctypes.data, obj.ctypes.data if niter else None,
                                            X.ctypes.data, None if R is None else R.ctypes.data, n, d, m, h, int(niter),
                                            int(ilsiter), int(icmiter), int(npert), 1 if randord else 0,
                                            int(seed) & ((1 << 64) - 1), int(nsplits), 0))
    return C, codes, obj


def _train(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, seed, nsplits, V, label):
    X = _as_f32(X, "X")
    B = np.asarray(B)
    if B.dtype != np.int16:
        raise TypeError("B must be an Int16 array of one-based codes")
    n, d = X.shape
    wide = int(h) > 256
    if wide:
        _check_wide_train(X, B, m, h, ilsiter, icmiter, npert, nsplits, one_based=True)
    else:
        _check(X, np.empty((m, h, d), np.float32), B, ilsiter, icmiter, npert, nsplits, 0, one_based=True)
    if V:
        print("Training %s with %d codebooks, %d perturbations, %d icm iterations and random order = %s"
              % (label, m, npert, icmiter, bool(randord)))
    if wide:      # past 256 codewords: the loop over 16-bit codes (rq_train_lsq_wide); h <= 256 stays on the byte loop
        C, codes, obj = train_lsq_u16(X, B - 1, m, h, R, niter, ilsiter, icmiter, randord, npert, seed=seed, nsplits=nsplits)
    else:
        C, codes, obj = train_lsq_u8(X, (B - 1).astype(np.uint8), m, h, R, niter, ilsiter, icmiter, randord, npert,
                                     seed=seed, nsplits=nsplits)
    if V:
        for it, o in enumerate(obj, 1):
            print("%3d %e " % (it, o))
    return list(C), codes.astype(np.int16) + 1, obj.astype(np.float32)


def train_lsq(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, cpp=True, V=True, seed=0):
    """train_lsq(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, cpp=true, V=true) -> C, B, obj
                                                                                          (src/LSQ.jl:323-372)
    X (n, d) float32, R (d, d) memory image of Julia's R (None = identity), B (n, m) Int16 one-based start codes; the C
    argument is ignored (the reference overwrites it, :348).  Returns C (m-long list of (h, d)), B (Int16 one-based) and
    obj (niter,) float32, obj[iter] = qerror before iteration iter's update (NaN when n = 0).  Like encoding_icm, the final codes are also
    written into B.  cpp=True requires h = 256; both settings run the same device loop (rq_train_lsq).  cpp=False takes any
    2 <= h <= 32767 with m * h <= 16384 whose encoder tables fit (wide_fits): past 256 codewords the loop over 16-bit codes runs
    (rq_train_lsq_wide)."""
    if not (isinstance(B, np.ndarray) and B.dtype == np.int16):
        raise TypeError("B must be an Int16 numpy array (it is updated in place)")
    if cpp and h != 256:
        raise ValueError("train_lsq with cpp=true requires h = 256 codewords; got h=%d" % h)
    Cn, Bn, obj = _train(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, seed, 1, V, "LSQ")
    B[...] = Bn
    return Cn, Bn, obj


def train_lsq_cuda(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, nsplits=1, V=False, seed=0):
    """train_lsq_cuda(X, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, nsplits=1, V=false) -> C, B, obj
                                                                                          (src/LSQ_GPU.jl:267-319)
    As train_lsq, but B is left untouched (encode_icm_cuda returns new codes); the result does not depend on nsplits.  Past 256
    codewords the loop over 16-bit codes runs, as in train_lsq(cpp=False)."""
    return _train(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, seed, nsplits, V, "LSQ GPU")


def last_lsq_timing():
    """Phase milliseconds of this thread's last host-pointer LSQ update or training call (rq_last_lsq_timing), summed
    over a training call's updates; the device entries leave zeros.  other_ms: a training call's R'X, rotation back and
    obj means; encode_ms: its encodes."""
    out = (ctypes.c_double * 7)()
    _lib.check(_lib.lib().rq_last_lsq_timing(ctypes.cast(out, ctypes.c_void_p), 7))
    return dict(zip(["count_ms", "sort_ms", "b_ms", "assemble_ms", "solve_ms", "other_ms", "encode_ms"],
                    [float(v) for v in out]))


def last_timing():
    """{unary_ms, total_ms} of this thread's last host-pointer encode (rq_last_icm_timing)."""
    u, t = ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(_lib.lib().rq_last_icm_timing(ctypes.cast(ctypes.byref(u), ctypes.c_void_p),
                                             ctypes.cast(ctypes.byref(t), ctypes.c_void_p)))
    return dict(unary_ms=u.value, total_ms=t.value)
