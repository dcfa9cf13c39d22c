"""Host mirror of src/utils.jl: splitarray, and the database norms of additive-quantizer search (get_norms_codebook,
quantize_norms) on the device."""
import numpy as np

from . import _lib


def splitarray(x, nparts):
    """src/utils.jl:179-203.  Splits `x` (a range / sequence) in `nparts` contiguous parts; if
    len(x) is not a multiple of nparts the first len(x) % nparts parts carry one extra element."""
    x = list(x) if not isinstance(x, range) else x
    n = len(x)
    per, extra = divmod(n, nparts)
    out, pos = [], 0
    for i in range(nparts):
        size = per + (1 if i < extra else 0)
        out.append(x[pos:pos + size])
        pos += size
    return out


def _as_f32(a, name):
    a = np.asarray(a)
    if a.dtype != np.float32:
        # src/PQ.jl:32 allocates costs as Float32, so the reference only dispatches for Float32 data
        raise TypeError("%s must be float32 (the reference encode only dispatches for Float32)" % name)
    return np.ascontiguousarray(a)


def _as_f32_or_u8(a, name):
    """Data the encoders take: float32, or uint8 rows as bvecs files hold them (src/xvecs_read.jl:14-52), which the byte
    entry points encode without widening them on the host (the reference widens: src/read_datasets.jl:148-167)."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    return _as_f32(a, name)


def encode_chunk_rows(d):
    """Rows per upload chunk of the host-pointer encodes, f32 and bytes alike: max(32768, 2^25 / d)."""
    return max(32768, (1 << 25) // int(d))


MAX_H16 = 32767          # RQ_MAX_H16: the largest value a one-based Int16 can name


def check_wide_h(h, X=None):
    """True when h codewords per codebook take the *_wide (16-bit) entry points.  Raises ValueError -- before the library
    is touched -- for an h no Int16 code can name, and for byte rows with h > 256 (the byte kernels cover h <= 256)."""
    h = int(h)
    if h > MAX_H16:
        raise ValueError("h = %d codewords per codebook: Int16 codes name at most %d (the Int16 limit)" % (h, MAX_H16))
    if h > 256 and X is not None and X.dtype == np.uint8:
        raise ValueError("byte rows (uint8 X) cover h <= 256; got h = %d -- pass X.astype(float32)" % h)
    return h > 256


def cat_codebooks(C):
    """Vector{Matrix} -> one flat buffer: concatenation of the m [h][sub_i] blocks
    (== cat(C..., dims=3) of src/Linscan.jl:22 when all sub_i are equal)."""
    return np.concatenate([_as_f32(c, "C[i]").reshape(-1) for c in C])


def _aq_args(B, C):
    """(zero-based codes (n, m), codebooks (m, h, d)) of one-based integer codes B and an m-long list of (h, d) codebooks; the
    codes are uint8, or int16 when h > 256 (check_wide_h: the *_wide entry points)."""
    Cs = np.ascontiguousarray(np.stack([_as_f32(c, "C[i]") for c in C]))
    B = np.asarray(B)
    if not np.issubdtype(B.dtype, np.integer):
        raise TypeError("B must hold one-based integer codes")
    m, h, d = Cs.shape
    if B.ndim != 2 or B.shape[1] != m:
        raise ValueError("B must be (n, m) with m = %d codebooks; got %s" % (m, B.shape))
    if B.size and (B.min() < 1 or B.max() > h):
        raise ValueError("codes must be in 1..%d" % h)
    return np.ascontiguousarray(B.astype(np.int64) - 1, dtype=np.int16 if check_wide_h(h) else np.uint8), Cs


def aq_norms(B, C):
    """|sum_k C_k[b_k]|^2 per row (n,) float32 (rq_aq_norms): the reconstruction is never built, the order of the f32 sums is
    veccost's."""
    codes, Cs = _aq_args(B, C)
    n = codes.shape[0]
    m, h, d = Cs.shape
    norms = np.empty(n, dtype=np.float32)
    if codes.dtype == np.int16:
        _lib.check(_lib.lib().rq_aq_norms_wide(norms.ctypes.data, codes.ctypes.data, Cs.ctypes.data, n, d, m, h, 0))
    else:
        _lib.check(_lib.lib().rq_aq_norms(norms.ctypes.data, codes.ctypes.data, Cs.ctypes.data, n, d, m, h))
    return norms


def get_norms_codebook(B, C, niter=100, seed=0):
    """get_norms_codebook(B, C) -> norms_codes, norms_codebook                                  (src/utils.jl:4-26)

    B (n, m) one-based integer codes (Int16 like the reference's), C m-long list of (h, d) codebooks.  The norms of the
    reconstructions are computed on the device and clustered there by a 1-D k-means with h centres (rq_get_norms_codebook); they
    never come to the host.  Returns the k-means' final assignments (n,) int64 one-based and the codebook (h,) float32.
    niter = 100 is the default `maxiter` of Clustering v0.12.2's kmeans as recalled -- it could not be checked against the package
    here; `seed` feeds the library's stream where the reference draws from Julia's global RNG.  The assignments use the
    encoder's distance form and can differ from quantize_norms(B, C, norms_codebook) for a norm next to a cell edge."""
    codes, Cs = _aq_args(B, C)
    n = codes.shape[0]
    m, h, d = Cs.shape
    nc = np.empty(n, dtype=codes.dtype)
    cb = np.empty(h, dtype=np.float32)
    if codes.dtype == np.int16:         # h > 256: int16 codes and a norms codebook of h entries (rq_get_norms_codebook_wide)
        _lib.check(_lib.lib().rq_get_norms_codebook_wide(nc.ctypes.data, cb.ctypes.data, None, codes.ctypes.data, Cs.ctypes.data,
                                                         n, d, m, h, h, int(niter), int(seed) & ((1 << 64) - 1), 0))
    else:
        _lib.check(_lib.lib().rq_get_norms_codebook(nc.ctypes.data, cb.ctypes.data, None, codes.ctypes.data, Cs.ctypes.data, n, d,
                                                    m, h, h, int(niter), int(seed) & ((1 << 64) - 1)))
    return nc.astype(np.int64) + 1, cb


def quantize_norms(B, C, cbnorms):
    """quantize_norms(B, C, cbnorms) -> dbnormsB, dbnormsX                                       (src/utils.jl:29-59)

    For every row the first entry of cbnorms (any length up to 256 -- up to 32767 when h > 256 -- unsorted) nearest to the norm of its reconstruction, in
    f32 with the reference's (norm - c)^2 and findmin's tie rule (rq_quantize_norms).  Returns the codes (n,) one-based in
    B's dtype and the norms (n,) float32."""
    codes, Cs = _aq_args(B, C)
    n = codes.shape[0]
    m, h, d = Cs.shape
    cb = np.ascontiguousarray(_as_f32(cbnorms, "cbnorms").reshape(-1))
    norms = np.empty(n, dtype=np.float32)
    if codes.dtype == np.int16:         # h > 256: int16 codes, cbnorms of up to 32767 entries (rq_quantize_norms_wide)
        nc = np.empty(n, dtype=np.int16)
        _lib.check(_lib.lib().rq_quantize_norms_wide(nc.ctypes.data, norms.ctypes.data, codes.ctypes.data, Cs.ctypes.data,
                                                     cb.ctypes.data, n, d, m, h, cb.shape[0], 0))
    else:
        nc = np.empty(n, dtype=np.uint8)
        _lib.check(_lib.lib().rq_quantize_norms(nc.ctypes.data, norms.ctypes.data, codes.ctypes.data, Cs.ctypes.data,
                                                cb.ctypes.data, n, d, m, h, cb.shape[0]))
    out_dtype = np.asarray(B).dtype if np.asarray(B).dtype.itemsize >= 2 else np.int16
    return nc.astype(out_dtype) + out_dtype.type(1), norms
