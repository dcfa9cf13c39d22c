"""Host mirror of src/xvecs_read.jl / src/xvecs_write.jl: TEXMEX .fvecs / .ivecs / .bvecs files.

Record layout (all little endian): int32 d, then d values (float32 / int32 / uint8).  Arrays are
returned in the memory-image convention of the other mirrors: (n, d) numpy == Julia's d-by-n matrix,
so a file read here can be handed to quantize_pq / linscan_pq as is.  SURVEY section 8f rank 4."""
import numpy as np


def _read(filename, bounds, dtype, itemsize):
    """bounds: None (all), n (first n) or (a, b) one-based inclusive like the reference's UnitRange."""
    with open(filename, "rb") as f:
        d = int(np.fromfile(f, dtype="<i4", count=1)[0])
        vecsizeof = 4 + d * itemsize
        f.seek(0, 2)
        vecnum = f.tell() // vecsizeof
        if bounds is None:
            a, b = 1, vecnum
        elif isinstance(bounds, (int, np.integer)):
            a, b = 1, int(bounds)
        else:
            a, b = int(bounds[0]), int(bounds[1])
        assert a >= 1                                   # xvecs_read.jl:18  @assert bounds.start >= 1
        n = b - a + 1
        f.seek((a - 1) * vecsizeof)
        raw = np.fromfile(f, dtype=np.uint8, count=vecsizeof * n)
    if raw.size != vecsizeof * n:
        raise EOFError("%s holds %d vectors, asked for %d..%d" % (filename, vecnum, a, b))
    raw = raw.reshape(n, vecsizeof)
    dims = raw[:, :4].copy().view("<i4").reshape(-1)
    assert (dims == d).all()                            # xvecs_read.jl:43-46: every record repeats d
    return np.ascontiguousarray(raw[:, 4:]).view(dtype).reshape(n, d)


def fvecs_read(bounds=None, filename=None):
    """fvecs_read(n_or_range, filename) -> (n, d) float32     (src/xvecs_read.jl:63-98)"""
    return _read(filename, bounds, "<f4", 4)


def ivecs_read(bounds=None, filename=None):
    """ivecs_read(n_or_range, filename) -> (n, d) int32       (src/xvecs_read.jl:109-144)"""
    return _read(filename, bounds, "<i4", 4)


def bvecs_read(bounds=None, filename=None):
    """bvecs_read(n_or_range, filename) -> (n, d) uint8       (src/xvecs_read.jl:14-52)"""
    return _read(filename, bounds, np.uint8, 1)


def _write(X, filename, dtype):
    X = np.ascontiguousarray(X, dtype=dtype)
    n, d = X.shape
    rec = np.empty((n, d + 1), dtype=dtype)
    rec[:, 0] = np.array([d], dtype="<i4").view(dtype)[0]   # reinterpret(Float32, Int32(d)), xvecs_write.jl:12
    rec[:, 1:] = X
    rec.tofile(filename)


def fvecs_write(X, filename):
    """fvecs_write(X, filename)    (src/xvecs_write.jl:10-16); X (n, d) float32."""
    _write(X, filename, "<f4")


def ivecs_write(X, filename):
    """ivecs_write(X, filename)    (src/xvecs_write.jl:19-25); X (n, d) int32."""
    _write(X, filename, "<i4")


def bvecs_write(X, filename):
    """bvecs_write(X, filename); X (n, d) uint8.  The reference reads .bvecs (src/xvecs_read.jl:14-52) and has no writer for
    them; this is the inverse of bvecs_read: per vector int32 d (little endian), then d bytes."""
    X = np.asarray(X)
    if X.dtype != np.uint8 or X.ndim != 2:
        raise TypeError("X must be a (n, d) uint8 array")
    n, d = X.shape
    rec = np.empty((n, 4 + d), dtype=np.uint8)
    rec[:, :4] = np.array([d], dtype="<i4").view(np.uint8)
    rec[:, 4:] = X
    rec.tofile(filename)


def quantize_bvecs(filename, C, R=None, bounds=None, rows_per_read=1 << 20, one_based=False):
    """Codes of the vectors of a .bvecs file (bigann_base.bvecs -> Index.set_codes): the file is read piecewise with
    bvecs_read(bounds, filename), rows_per_read vectors at a time, and every piece is encoded from its bytes -- the reference
    reads the bytes and widens them to Float32 first (src/xvecs_read.jl:14-52, src/read_datasets.jl:148-167); the codes are
    the same.  R is None: quantize_pq, else quantize_opq.  bounds: None (all), n (first n) or (a, b) one-based inclusive.
    Returns (n, m) uint8 zero-based codes (the scan's wire format), or int16 one-based with one_based=True.  Codebooks of
    256 < h <= 32767 codewords (rq_encode_{pq,opq}_bytes_wide) return int16 either way: zero-based (IndexU16.set_codes takes
    them as they are), or one-based with one_based=True."""
    from . import _lib
    from .utils import _as_f32, cat_codebooks, check_wide_h
    if rows_per_read < 1:
        raise ValueError("rows_per_read must be positive")
    with open(filename, "rb") as f:
        d = int(np.fromfile(f, dtype="<i4", count=1)[0])
        f.seek(0, 2)
        vecnum = f.tell() // (4 + d)
    if bounds is None:
        a, b = 1, vecnum
    elif isinstance(bounds, (int, np.integer)):
        a, b = 1, int(bounds)
    else:
        a, b = int(bounds[0]), int(bounds[1])
    if a < 1 or b > vecnum or b < a:
        raise ValueError("%s holds %d vectors, asked for %d..%d" % (filename, vecnum, a, b))
    m = len(C)
    h = np.asarray(C[0]).shape[0]
    Cc = cat_codebooks(C)
    if Cc.size != h * d:
        raise ValueError("codebooks do not tile the %d dimensions of %s" % (d, filename))
    Rc = None if R is None else _as_f32(R, "R")
    if Rc is not None and Rc.shape != (d, d):
        raise ValueError("R must be %d x %d" % (d, d))
    n = b - a + 1
    wide = check_wide_h(h)
    out = np.empty((n, m), dtype=np.int16 if one_based or wide else np.uint8)
    L = _lib.lib()
    for r0 in range(0, n, rows_per_read):
        nr = min(rows_per_read, n - r0)
        X = bvecs_read((a + r0, a + r0 + nr - 1), filename)
        dst = out[r0:r0 + nr]                       # (a contiguous block of rows of `out`)
        if wide and Rc is None:
            _lib.check(L.rq_encode_pq_bytes_wide(dst.ctypes.data, X.ctypes.data, Cc.ctypes.data, nr, d, m, h, int(one_based)))
        elif wide:
            _lib.check(L.rq_encode_opq_bytes_wide(dst.ctypes.data, X.ctypes.data, Rc.ctypes.data, Cc.ctypes.data, nr, d, m, h,
                                                  int(one_based)))
        elif Rc is None:
            encode = L.rq_encode_pq_bytes_i16 if one_based else L.rq_encode_pq_bytes
            _lib.check(encode(dst.ctypes.data, X.ctypes.data, Cc.ctypes.data, nr, d, m, h))
        else:
            encode = L.rq_encode_opq_bytes_i16 if one_based else L.rq_encode_opq_bytes
            _lib.check(encode(dst.ctypes.data, X.ctypes.data, Rc.ctypes.data, Cc.ctypes.data, nr, d, m, h))
    return out


def _ivf_add_xvecs(ix, filename, bounds, rows_per_read, read, itemsize):
    if rows_per_read < 1:
        raise ValueError("rows_per_read must be positive")
    with open(filename, "rb") as f:
        d = int(np.fromfile(f, dtype="<i4", count=1)[0])
        f.seek(0, 2)
        vecnum = f.tell() // (4 + d * itemsize)
    if bounds is None:
        a, b = 1, vecnum
    elif isinstance(bounds, (int, np.integer)):
        a, b = 1, int(bounds)
    else:
        a, b = int(bounds[0]), int(bounds[1])
    if a < 1 or b > vecnum or b < a:
        raise ValueError("%s holds %d vectors, asked for %d..%d" % (filename, vecnum, a, b))
    if d != ix.d:
        raise ValueError("%s holds vectors of %d dimensions, the index takes d=%d" % (filename, d, ix.d))
    n = b - a + 1
    for r0 in range(0, n, rows_per_read):
        nr = min(rows_per_read, n - r0)
        ix.add(read((a + r0, a + r0 + nr - 1), filename), id_offset=a - 1 + r0)
    return n


def ivf_add_bvecs(ix, filename, bounds=None, rows_per_read=1 << 20):
    """Add the vectors of a .bvecs file (bigann_base.bvecs) to the IvfIndex ix: the file is read piecewise with
    bvecs_read(bounds, filename), rows_per_read vectors at a time, and every piece is added from its bytes with its file
    position as id_offset -- the id of a vector is its ZERO-based position in the file whatever rows_per_read and bounds are, so
    shards of a file can be added in ascending order.  bounds: None (all), n (first n) or (a, b) one-based inclusive.  Returns
    the number of vectors added."""
    return _ivf_add_xvecs(ix, filename, bounds, rows_per_read, bvecs_read, 1)


def ivf_add_fvecs(ix, filename, bounds=None, rows_per_read=1 << 20):
    """ivf_add_bvecs for a .fvecs file (float32 vectors)."""
    return _ivf_add_xvecs(ix, filename, bounds, rows_per_read, fvecs_read, 4)
