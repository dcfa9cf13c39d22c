"""Host mirror of the LSQ codebook update (src/codebook_update.jl): update_codebooks (:235-277) with the "fastbin"
method, update_codebooks_fast_bin (:175-206) and its normal equations fast_bin_matmul (:96-170).

The normal equations (B'B + rho I) C = B'X of the one-hot codes are built and solved in f64 on the device
(rq_update_codebooks_lsq); the contract is DESIGN.md section 2.  X is (n, d) float32, B (n, m) Int16 one-based like the
reference's m-by-n matrices; the result is an m-long list of (h, d) codebooks (memory image of Julia's d-by-h
matrices).

update_codebooks_chain_bin (:367-412) and get_cbdims_chain (:280-294) are the chain-structured update of ChainQ: the same
normal equations, solved per pair of adjacent codebooks over that pair's part of the dimensions (rq_update_codebooks_chain)."""
import time

import numpy as np

from . import _lib
from .utils import MAX_H16, _as_f32, splitarray

MAX_M = 16
MAX_MH = 16384         # the update over 16-bit codes: A = (m h)^2 f64 within 2 GiB
MAX_CHAIN_H2 = 16384   # the chain update over 16-bit codes: one (2 h)^2 f64 block within 2 GiB
METHODS = ("fast", "fastbin", "lsmr", "lsqr", "naive")      # src/codebook_update.jl:242


def _check_update(n, d, codes_shape, m, h, rho, wide=False):
    """Every argument check of the update runs here, before the library (and the device) is touched.  wide: the update over
    16-bit codes (2 <= h <= MAX_H16 and m * h <= MAX_MH) instead of the byte one (h <= 256)."""
    if len(codes_shape) != 2 or codes_shape[0] != n:
        raise ValueError("codes must be (n, m) with n = %d rows; got %s" % (n, tuple(codes_shape)))
    if not 1 <= m <= MAX_M:
        raise ValueError("the LSQ update covers 1 <= m <= %d codebooks; got m=%d" % (MAX_M, m))
    hmax = MAX_H16 if wide else 256
    if not 2 <= int(h) <= hmax:
        raise ValueError("the LSQ update covers 2 <= h <= %d codewords; got h=%d" % (hmax, h))
    if wide and m * int(h) > MAX_MH:
        raise ValueError("the LSQ update solves m * h <= %d unknowns per dimension; got m=%d, h=%d" % (MAX_MH, m, h))
    if d < 1:
        raise ValueError("d must be >= 1; got %d" % d)
    if n > 2 ** 32 - 1:
        raise ValueError("n=%d rows exceed the update's 32-bit counters" % n)
    rho = float(rho)
    if not (np.isfinite(rho) and rho > 0):
        raise ValueError("rho must be finite and > 0; got %r" % rho)
    return rho


def update_codebooks_u8(X, codes, h, rho=1e-4):
    """Zero-based uint8 codes (n, m) -> codebooks as one (m, h, d) float32 array."""
    X = _as_f32(X, "X")
    codes = np.asarray(codes)
    n, d = X.shape
    m = codes.shape[1] if codes.ndim == 2 else -1
    rho = _check_update(n, d, codes.shape, m, h, rho)
    if codes.size and (codes.min() < 0 or codes.max() > h - 1):
        raise ValueError("codes must be in 0..%d" % (h - 1))
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    C = np.empty((m, h, d), dtype=np.float32)
    _lib.check(_lib.lib().rq_update_codebooks_lsq(C.ctypes.data, X.ctypes.data, codes.ctypes.data, n, d, m, int(h), rho))
    return C


def update_codebooks_u16(X, codes, h, rho=1e-4):
    """update_codebooks_u8 over zero-based int16 codes for any 2 <= h <= 32767 with m * h <= 16384: rq_update_codebooks_lsq_wide,
    the int16 kernels at every h.  At h <= 256 the codebooks equal update_codebooks_u8's bit for bit."""
    X = _as_f32(X, "X")
    codes = np.asarray(codes)
    n, d = X.shape
    m = codes.shape[1] if codes.ndim == 2 else -1
    rho = _check_update(n, d, codes.shape, m, h, rho, wide=True)
    if codes.size and (codes.min() < 0 or codes.max() > h - 1):
        raise ValueError("codes must be in 0..%d" % (h - 1))
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    C = np.empty((m, int(h), d), dtype=np.float32)
    _lib.check(_lib.lib().rq_update_codebooks_lsq_wide(C.ctypes.data, X.ctypes.data, codes.ctypes.data, n, d, m, int(h), rho, 0))
    return C


def update_codebooks_fast_bin(X, B, h, V=False, rho=1e-4):
    """update_codebooks_fast_bin(X, B, h, V=false, rho=1e-4) -> C       (src/codebook_update.jl:175-206)

    X (n, d) float32, B (n, m) Int16 one-based.  Returns an m-long list of (h, d) float32 codebooks."""
    X = _as_f32(X, "X")
    B = np.asarray(B)
    n, d = X.shape
    m = B.shape[1] if B.ndim == 2 else -1
    _check_update(n, d, B.shape, m, h, rho)
    if B.size and (B.min() < 1 or B.max() > h):
        raise ValueError("codes must be in 1..%d" % h)
    C = update_codebooks_u8(X, (B - 1).astype(np.uint8), h, rho)
    if V:
        print("Doing fast bin codebook update... done.")
    return list(C)


def update_codebooks(X, B, h, V=False, method="fastbin"):
    """update_codebooks(X, B, h, V=false, method="fastbin") -> C       (src/codebook_update.jl:235-277)

    Only "fastbin" runs here; any other method raises ValueError naming it.  Past 256 codewords per codebook the update over
    16-bit codes runs (update_codebooks_u16: h <= 32767, m * h <= 16384); h <= 256 stays on update_codebooks_fast_bin."""
    if method not in METHODS:
        raise ValueError("Codebook update method unknown: %r" % (method,))
    if method != "fastbin":
        raise ValueError("codebook update method %r is not supported; only \"fastbin\" is" % (method,))
    if int(h) <= 256:
        return update_codebooks_fast_bin(X, B, h, V)
    X = _as_f32(X, "X")
    B = np.asarray(B)
    n, d = X.shape
    m = B.shape[1] if B.ndim == 2 else -1
    _check_update(n, d, B.shape, m, h, 1e-4, wide=True)
    if B.size and (B.min() < 1 or B.max() > h):
        raise ValueError("codes must be in 1..%d" % h)
    C = update_codebooks_u16(X, B.astype(np.int16) - 1, h)
    if V:
        print("Doing fast bin codebook update... done.")
    return list(C)


def get_cbdims_chain(d, m):
    """get_cbdims_chain(d, m) -> odims       (src/codebook_update.jl:280-294)

    The dimensions each of the m codebooks of a chain quantizer covers, as m zero-based Python ranges (the reference's
    one-based UnitRanges minus one): parts i-1 and i of splitarray(range(d), m - 1)."""
    d, m = int(d), int(m)
    if not 2 <= m <= MAX_M:
        raise ValueError("a chain has 2 <= m <= %d codebooks; got m=%d" % (MAX_M, m))
    if d < m - 1:
        raise ValueError("d=%d < m - 1 = %d leaves a chain part empty" % (d, m - 1))
    sub = splitarray(range(d), m - 1)
    return [sub[0]] + [range(sub[i - 1][0], sub[i][-1] + 1) for i in range(1, m - 1)] + [sub[-1]]


def _check_chain_update(n, d, codes_shape, m, h, rho, wide=False):
    """Every argument check of the chain update runs here, before the library (and the device) is touched.  wide: the update
    over 16-bit codes (2 <= h <= MAX_H16 and 2 h <= MAX_CHAIN_H2; no m * h limit, no (m h)^2 matrix is built)."""
    if wide:
        if not 2 <= int(h) <= MAX_H16:
            raise ValueError("the chain update covers 2 <= h <= %d codewords; got h=%d" % (MAX_H16, h))
        if 2 * int(h) > MAX_CHAIN_H2:
            raise ValueError("the chain update solves 2 h <= %d unknowns per block; got h=%d" % (MAX_CHAIN_H2, h))
        rho = _check_update(n, d, codes_shape, m, 2, rho)      # every check but h's
    else:
        rho = _check_update(n, d, codes_shape, m, h, rho)
    if m < 2:
        raise ValueError("the chain update needs m >= 2 codebooks; got m=%d" % m)
    if d < m - 1:
        raise ValueError("d=%d < m - 1 = %d leaves a chain part empty" % (d, m - 1))
    return rho


def update_codebooks_chain_u8(X, codes, h, rho=1e-4):
    """Zero-based uint8 codes (n, m) -> chain codebooks as one (m, h, d) float32 array (zero outside get_cbdims_chain)."""
    X = _as_f32(X, "X")
    codes = np.asarray(codes)
    n, d = X.shape
    m = codes.shape[1] if codes.ndim == 2 else -1
    rho = _check_chain_update(n, d, codes.shape, m, h, rho)
    if codes.size and (codes.min() < 0 or codes.max() > h - 1):
        raise ValueError("codes must be in 0..%d" % (h - 1))
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    C = np.empty((m, h, d), dtype=np.float32)
    _lib.check(_lib.lib().rq_update_codebooks_chain(C.ctypes.data, X.ctypes.data, codes.ctypes.data, n, d, m, int(h), rho))
    return C


def update_codebooks_chain_bin_u16(X, codes, h, rho=1e-4):
    """update_codebooks_chain_u8 over zero-based 16-bit codes for any 2 <= h <= 8192 (rq_update_codebooks_chain_wide, the int16
    kernels at every h).  At h <= 256 the codebooks equal update_codebooks_chain_u8's bit for bit."""
    X = _as_f32(X, "X")
    codes = np.asarray(codes)
    n, d = X.shape
    m = codes.shape[1] if codes.ndim == 2 else -1
    rho = _check_chain_update(n, d, codes.shape, m, h, rho, wide=True)
    if codes.size and (codes.min() < 0 or codes.max() > h - 1):
        raise ValueError("codes must be in 0..%d" % (h - 1))
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    C = np.empty((m, int(h), d), dtype=np.float32)
    _lib.check(_lib.lib().rq_update_codebooks_chain_wide(C.ctypes.data, X.ctypes.data, codes.ctypes.data, n, d, m, int(h), rho, 0))
    return C


def update_codebooks_chain_bin(X, B, h, V=False, rho=1e-4, *, wide=False):
    """update_codebooks_chain_bin(X, B, h, V=false, rho=1e-4) -> C, elapsed       (src/codebook_update.jl:367-412)

    X (n, d) float32, B (n, m) Int16 one-based.  Returns an m-long list of (h, d) float32 codebooks and the seconds spent.

    wide (keyword only, not in the reference): False keeps the byte contract, 2 <= h <= 256, and raises ValueError past it before
    the library is touched -- callers and tests rely on that.  wide=True accepts 2 <= h <= 8192 and runs the update over 16-bit
    codes at every h (update_codebooks_chain_bin_u16); the codebooks are the same wherever both run."""
    start = time.perf_counter()
    X = _as_f32(X, "X")
    B = np.asarray(B)
    n, d = X.shape
    m = B.shape[1] if B.ndim == 2 else -1
    _check_chain_update(n, d, B.shape, m, h, rho, wide=wide)
    if B.size and (B.min() < 1 or B.max() > h):
        raise ValueError("codes must be in 1..%d" % h)
    if wide:
        C = update_codebooks_chain_bin_u16(X, B.astype(np.int16) - np.int16(1), h, rho)
    else:
        C = update_codebooks_chain_u8(X, (B - 1).astype(np.uint8), h, rho)
    if V:
        print("Doing chain bin codebook update... done.")
    return list(C), time.perf_counter() - start
