"""Host mirror of src/ERVQ.jl: quantize_ervq, train_ervq (Enhanced RVQ / Stacked Quantizers, arXiv 1411.2173).

The training loop is device-resident (rq_train_ervq); the contract is DESIGN.md section 2 ("ERVQ").  Layouts are RVQ's:
X (n, d) float32 (memory image of the d-by-n matrix), C an m-long list of (h, d) codebooks, B (n, m) one-based codes."""
import ctypes

import numpy as np

from . import _lib
from .RVQ import _stack_codebooks, quantize_rvq, train_rvq
from .utils import _as_f32, check_wide_h

MAX_M = 64
_U64 = (1 << 64) - 1


def quantize_ervq(X, C, V=False, rng=None):
    """quantize_ervq(X, C, V=false) -> B, singletons          (src/ERVQ.jl:19-26): identical to quantize_rvq."""
    return quantize_rvq(X, C, V, rng=rng)


def _check(X, Cs, codes, m, h, one_based):
    """Every argument check runs here, before the library (and the device) is touched."""
    if X.ndim != 2:
        raise ValueError("X must be (n, d); got %s" % (X.shape,))
    n, d = X.shape
    if d < 1:
        raise ValueError("d must be >= 1")
    if Cs.ndim != 3 or Cs.shape[2] != d:
        raise ValueError("codebooks must be m matrices of (h, d) = (.., %d); got %s" % (d, Cs.shape))
    if Cs.shape[0] != int(m) or Cs.shape[1] != int(h):
        raise ValueError("C holds %d codebooks of %d entries, the call says m=%d, h=%d" % (Cs.shape[0], Cs.shape[1], m, h))
    if not 1 <= int(m) <= MAX_M:
        raise ValueError("ERVQ covers 1 <= m <= %d codebooks; got m=%d" % (MAX_M, m))
    check_wide_h(h)
    if int(h) < 2:
        raise ValueError("ERVQ covers 2 <= h <= 32767 entries; got h=%d" % h)
    B = np.asarray(codes)
    if B.dtype.kind not in "iu":
        raise TypeError("codes must be integers; got %s" % B.dtype)
    if B.shape != (n, int(m)):
        raise ValueError("codes must be (n, m) = (%d, %d); got %s" % (n, m, B.shape))
    lo = 1 if one_based else 0
    if B.size and (B.min() < lo or B.max() > int(h) - 1 + lo):
        raise ValueError("codes must be in %d..%d" % (lo, int(h) - 1 + lo))
    return n, d


def ervq_update_codebook(X, codes, C, j):
    """The codebook update of one ERVQ step alone (src/ERVQ.jl:85-90; rq_ervq_update_codebook): every entry of codebook j
    (zero-based) that has rows becomes the mean of X - sum_{i != j} C_i[b_i] over its rows.  codes (n, m) uint8 zero-based;
    int16 / uint16 codes, or more than 256 entries per codebook, take rq_ervq_update_codebook_wide (zero-based as well).
    Returns (C (m, h, d) with block j updated and every other block bit for bit, counts (h,) uint32); an entry without
    rows keeps its value, nothing is refilled."""
    X = np.ascontiguousarray(_as_f32(X, "X"))
    Cs = _stack_codebooks(C).copy()
    m, h = Cs.shape[0], Cs.shape[1]
    n, d = _check(X, Cs, codes, m, h, one_based=False)
    if not 0 <= int(j) < m:
        raise ValueError("j must be in 0..m-1 = 0..%d; got %d" % (m - 1, j))
    counts = np.zeros(h, dtype=np.uint32)
    if check_wide_h(h) or np.asarray(codes).dtype in (np.int16, np.uint16):
        codes = np.array(codes, dtype=np.int16, order="C")
        _lib.check(_lib.lib().rq_ervq_update_codebook_wide(Cs.ctypes.data, counts.ctypes.data, X.ctypes.data, codes.ctypes.data,
                                                           n, d, m, h, int(j), 0))
        return Cs, counts
    codes = np.array(codes, dtype=np.uint8, order="C")
    _lib.check(_lib.lib().rq_ervq_update_codebook(Cs.ctypes.data, counts.ctypes.data, X.ctypes.data, codes.ctypes.data, n, d,
                                                  m, h, int(j)))
    return Cs, counts


def train_ervq_i16(X, B, C, m, h, niter, seed=0):
    """The device-resident loop (rq_train_ervq; rq_train_ervq_wide when h > 256): (C (m, h, d), B (n, m) int16 one-based, error, obj float64 (niter*m + 1,)).
    obj[0] is the error of the inputs, obj[1 + it*m + j] the error after step j of iteration it."""
    X = np.ascontiguousarray(_as_f32(X, "X"))
    Cs = _stack_codebooks(C).copy()
    n, d = _check(X, Cs, B, m, h, one_based=True)
    if int(niter) < 0:
        raise ValueError("niter must be >= 0; got %d" % niter)
    if n < 1:
        raise ValueError("train_ervq needs at least one row")
    B1 = np.array(B, dtype=np.int16, order="C")
    obj = np.zeros(int(niter) * int(m) + 1, dtype=np.float64)
    err = ctypes.c_double(0.0)
    perr = ctypes.cast(ctypes.byref(err), ctypes.c_void_p)
    if check_wide_h(h):
        _lib.check(_lib.lib().rq_train_ervq_wide(Cs.ctypes.data, B1.ctypes.data, perr, obj.ctypes.data, X.ctypes.data, n, d,
                                                 int(m), int(h), int(niter), int(seed) & _U64, 1))
    else:
        _lib.check(_lib.lib().rq_train_ervq(Cs.ctypes.data, B1.ctypes.data, perr, obj.ctypes.data, X.ctypes.data, n, d, int(m),
                                            int(h), int(niter), int(seed) & _U64))
    return Cs, B1, float(err.value), obj


def train_ervq(X, *args, V=False, seed=0):
    """train_ervq(X, B, C, m, h, niter=25, V=false) -> C, B, error          (src/ERVQ.jl:51-135)
    train_ervq(X, m, h, niter=25, V=false) -> C, B, error                   (src/ERVQ.jl:138-148)

    The second method initialises with train_rvq(X, m, h, niter, V) like the reference.  C: m-long list of (h, d)
    codebooks; B: (n, m) int16 one-based, equal to quantize_ervq(X, C)[0] after every complete iteration; error =
    qerror(X, B, C).  The reference prints `Qerror is ...` after every step; here V=True prints those lines.  Entries that
    lose all their rows are refilled from the library's stream seeded by `seed` (the reference: Julia's RNG)."""
    if args and np.ndim(args[0]) == 0:
        m, h = int(args[0]), int(args[1])
        rest = list(args[2:])
        niter = int(rest.pop(0)) if rest else 25
        if rest:
            V = bool(rest.pop(0))
        if rest:
            raise TypeError("train_ervq(X, m, h, niter, V): too many arguments")
        C, B, _ = train_rvq(X, m, h, niter, V, seed=seed)
    else:
        if len(args) < 4:
            raise TypeError("train_ervq(X, B, C, m, h, niter=25, V=false) or train_ervq(X, m, h, niter=25, V=false)")
        B, C, m, h = args[0], args[1], int(args[2]), int(args[3])
        rest = list(args[4:])
        niter = int(rest.pop(0)) if rest else 25
        if rest:
            V = bool(rest.pop(0))
        if rest:
            raise TypeError("train_ervq(X, B, C, m, h, niter, V): too many arguments")
    Cs, B1, err, obj = train_ervq_i16(X, B, C, m, h, niter, seed=seed)
    if V:
        print("Error after init is %s " % obj[0])
        for it in range(niter):
            print("=== Iteration %d / %d ===" % (it + 1, niter))
            for j in range(m):
                print("Updating codebook %d... done.\nUpdating codes... done. Qerror is %s." % (j + 1, obj[1 + it * m + j]))
    return [Cs[i] for i in range(m)], B1, err


ERVQ_PHASES = ["init_ms", "increment_ms", "refill_ms", "encode_ms", "epilogue_ms", "error_ms", "other_ms"]


def last_ervq_timing():
    """Phase milliseconds of this thread's last train_ervq call (rq_last_ervq_timing), summed over the call.  refill_ms
    holds the per-step read-back of the counts; other_ms the uploads and the code conversions."""
    out = (ctypes.c_double * 7)()
    _lib.check(_lib.lib().rq_last_ervq_timing(ctypes.cast(out, ctypes.c_void_p), 7))
    return dict(zip(ERVQ_PHASES, [float(v) for v in out]))
