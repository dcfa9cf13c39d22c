"""Host mirror of chain quantization (src/ChainQ.jl): quantize_chainq (:305-348) and train_chainq (:373-431).

The Viterbi recursion over the unaries and the m-1 adjacent-pair tables runs on the device (rq_quantize_chainq); the
contract is DESIGN.md section 2, and the codes are a pure function of (X, C).  Codebooks C are an m-long list of (h, d)
arrays (memory image of Julia's d-by-h matrices) or one (m, h, d) array; codes are (n, m) Int16 one-based like the
reference's m-by-n matrices; R is the memory image of Julia's d x d matrix."""
import ctypes
import time

import numpy as np

from . import _lib
from .LSQ import _stack
from .codebook_update import _check_chain_update
from .utils import MAX_H16, _as_f32

MAX_M = 16
SCRATCH_BYTES = 2 << 30      # tables + unaries of one chunk (DESIGN.md sections 4.11 and 4.26)


def _check_encode(X, Cs, nsplits, wide=False):
    """Every argument check of the encoder runs here, before the library (and the device) is touched.  wide: the encoder over
    16-bit codes (2 <= h <= MAX_H16 and its shape rule) instead of the byte one (h <= 256)."""
    if X.ndim != 2:
        raise ValueError("X must be (n, d); got %s" % (X.shape,))
    n, d = X.shape
    m, h, d2 = Cs.shape
    if d2 != d:
        raise ValueError("codebooks are %d-dimensional, data is %d-dimensional" % (d2, d))
    if not 1 <= m <= MAX_M:
        raise ValueError("chain encoding covers 1 <= m <= %d codebooks; got m=%d" % (MAX_M, m))
    hmax = MAX_H16 if wide else 256
    if not 2 <= h <= hmax:
        raise ValueError("chain encoding covers 2 <= h <= %d codewords; got h=%d" % (hmax, h))
    if d < 1:
        raise ValueError("d must be >= 1; got %d" % d)
    if int(nsplits) < 1:
        raise ValueError("nsplits must be >= 1; got %d" % nsplits)
    if wide:
        _check_wide_shape(m, h)
    return n, d, m, h


def wide_table_bytes(m, h):
    """(HS, table bytes, bytes of one row's unaries) of the encoder over 16-bit codes: what rq_chain_wide_plan reports."""
    HS = 64 * ((h + 63) // 64)
    return HS, 2 * (m - 1) * h * HS * 4 + m * h * 4, m * HS * 4


def _check_wide_shape(m, h):
    """The shape rule of rq_quantize_chainq_wide: the tables and 32 rows of unaries within 2 GiB."""
    _, tables, row = wide_table_bytes(m, h)
    if tables + 32 * row > SCRATCH_BYTES:
        raise ValueError("the pair tables of m=%d, h=%d take %d bytes; with 32 rows of unaries they must fit %d"
                         % (m, h, tables, SCRATCH_BYTES))


def quantize_chainq_u8(X, C, nsplits=1):
    """Zero-based uint8 codes (n, m); nsplits = the minimum number of row chunks (the codes do not depend on it)."""
    X = _as_f32(X, "X")
    Cs = _stack(C)
    n, d, m, h = _check_encode(X, Cs, nsplits)
    out = np.empty((n, m), dtype=np.uint8)
    _lib.check(_lib.lib().rq_quantize_chainq(out.ctypes.data, X.ctypes.data, Cs.ctypes.data, n, d, m, h, int(nsplits)))
    return out


def quantize_chainq_u16(X, C, nsplits=1):
    """quantize_chainq_u8 for any 2 <= h <= 32767: zero-based codes (n, m) as uint16 (rq_quantize_chainq_wide, the int16 kernels
    at every h).  At h <= 256 the codes equal quantize_chainq_u8's."""
    X = _as_f32(X, "X")
    Cs = _stack(C)
    n, d, m, h = _check_encode(X, Cs, nsplits, wide=True)
    out = np.empty((n, m), dtype=np.int16)
    _lib.check(_lib.lib().rq_quantize_chainq_wide(out.ctypes.data, X.ctypes.data, Cs.ctypes.data, n, d, m, h, int(nsplits), 0))
    return out.view(np.uint16)


def quantize_chainq(X, C, use_cuda=False, use_cpp=False, *, wide=False):
    """quantize_chainq(X, C, use_cuda=false, use_cpp=false) -> B, elapsed       (src/ChainQ.jl:305-348)

    X (n, d) float32, C m-long list of (h, d) codebooks.  Returns B (n, m) Int16 one-based and the seconds spent.  Both
    flags are accepted and ignored: there is one implementation, the device's.

    wide (keyword only, not in the reference): False keeps the byte contract, 2 <= h <= 256, and raises ValueError past it before
    the library is touched -- callers and tests rely on that.  wide=True accepts 2 <= h <= 32767 and runs the encoder over 16-bit
    codes at every h (quantize_chainq_u16); the codes are the same wherever both run."""
    start = time.perf_counter()
    if wide:
        B = quantize_chainq_u16(X, C).view(np.int16) + np.int16(1)
    else:
        B = quantize_chainq_u8(X, C).astype(np.int16) + 1
    return B, time.perf_counter() - start


def train_chainq_u8(X, codes0, m, h, R, niter):
    """The device-resident training loop (rq_train_chainq) on zero-based uint8 codes:
    (C (m, h, d), codes, R, obj float64 (niter + 1,))."""
    X = _as_f32(X, "X")
    if X.ndim != 2:
        raise ValueError("X must be (n, d); got %s" % (X.shape,))
    n, d = X.shape
    B = np.asarray(codes0)
    _check_chain_update(n, d, B.shape, B.shape[1] if B.ndim == 2 else -1, h, 1e-4)
    if B.shape[1] != int(m):
        raise ValueError("codes have %d columns, m=%d" % (B.shape[1], m))
    if n < 1:
        raise ValueError("train_chainq needs at least one row")
    if int(niter) < 0:
        raise ValueError("niter must be >= 0; got %d" % niter)
    if d > 1024:
        raise ValueError("train_chainq covers d <= 1024 (the device polar factor); got d=%d" % d)
    R = _as_f32(R, "R")
    if R.shape != (d, d):
        raise ValueError("R must be (d, d) = (%d, %d); got %s" % (d, d, R.shape))
    if B.size and (B.min() < 0 or B.max() > h - 1):
        raise ValueError("codes must be in 0..%d" % (h - 1))
    codes = np.array(B, dtype=np.uint8, order="C")
    Rio = np.array(R, dtype=np.float32, order="C")
    C = np.empty((m, h, d), dtype=np.float32)
    obj = np.zeros(int(niter) + 1, dtype=np.float64)
    _lib.check(_lib.lib().rq_train_chainq(C.ctypes.data, codes.ctypes.data, Rio.ctypes.data, obj.ctypes.data,
                                          X.ctypes.data, n, d, int(m), int(h), int(niter)))
    return C, codes, Rio, obj


def train_chainq_u16(X, codes0, m, h, R, niter):
    """train_chainq_u8 over zero-based 16-bit codes for any 2 <= h <= 8192 (rq_train_chainq_wide):
    (C (m, h, d), codes uint16, R, obj float64 (niter + 1,)).  At h <= 256 every output equals train_chainq_u8's bit for bit."""
    X = _as_f32(X, "X")
    if X.ndim != 2:
        raise ValueError("X must be (n, d); got %s" % (X.shape,))
    n, d = X.shape
    B = np.asarray(codes0)
    _check_chain_update(n, d, B.shape, B.shape[1] if B.ndim == 2 else -1, h, 1e-4, wide=True)
    if B.shape[1] != int(m):
        raise ValueError("codes have %d columns, m=%d" % (B.shape[1], m))
    _check_wide_shape(int(m), int(h))
    if n < 1:
        raise ValueError("train_chainq needs at least one row")
    if int(niter) < 0:
        raise ValueError("niter must be >= 0; got %d" % niter)
    if d > 1024:
        raise ValueError("train_chainq covers d <= 1024 (the device polar factor); got d=%d" % d)
    R = _as_f32(R, "R")
    if R.shape != (d, d):
        raise ValueError("R must be (d, d) = (%d, %d); got %s" % (d, d, R.shape))
    if B.size and (B.min() < 0 or B.max() > h - 1):
        raise ValueError("codes must be in 0..%d" % (h - 1))
    codes = np.array(B, dtype=np.int16, order="C")
    Rio = np.array(R, dtype=np.float32, order="C")
    C = np.empty((int(m), int(h), d), dtype=np.float32)
    obj = np.zeros(int(niter) + 1, dtype=np.float64)
    _lib.check(_lib.lib().rq_train_chainq_wide(C.ctypes.data, codes.ctypes.data, Rio.ctypes.data, obj.ctypes.data,
                                               X.ctypes.data, n, d, int(m), int(h), int(niter), 0))
    return C, codes.view(np.uint16), Rio, obj


def train_chainq(X, m, h, R, B, C, niter, V=False):
    """train_chainq(X, m, h, R, B, C, niter, V=false) -> C, B, R, obj       (src/ChainQ.jl:373-431)

    X (n, d) float32, R (d, d) start rotation, B (n, m) Int16 one-based start codes; the C argument is ignored (the
    reference overwrites it, :397).  Returns C (m-long list of (h, d)), B (Int16 one-based), R and obj (niter + 1,)
    float32, obj[iter] = qerror(R'X, B, C) at the start of round iter.  No random numbers are drawn.  h > 256 runs the loop over
    16-bit codes (train_chainq_u16: h <= 8192); h <= 256 stays on the byte loop."""
    B = np.asarray(B)
    if B.dtype != np.int16:
        raise TypeError("B must be an Int16 array of one-based codes")
    if B.size and (B.min() < 1 or B.max() > h):
        raise ValueError("codes must be in 1..%d" % h)
    if V:
        print("Training a chain quantizer")
    if int(h) > 256:
        Cn, codes, Rn, obj = train_chainq_u16(X, B - np.int16(1), m, h, R, niter)
        codes = codes.view(np.int16)
    else:
        Cn, codes, Rn, obj = train_chainq_u8(X, B - 1, m, h, R, niter)
    if V:
        for it, o in enumerate(obj):
            print("%3d %e" % (it, o))
    return list(Cn), codes.astype(np.int16) + 1, Rn, obj.astype(np.float32)


def last_chainq_timing():
    """Phase milliseconds of this thread's last host-pointer chain call (rq_last_chainq_timing), summed over a training
    call; the device entries leave zeros."""
    out = (ctypes.c_double * 5)()
    _lib.check(_lib.lib().rq_last_chainq_timing(ctypes.cast(out, ctypes.c_void_p), 5))
    return dict(zip(["unary_ms", "tables_ms", "viterbi_ms", "update_ms", "rotation_ms"], [float(v) for v in out]))
