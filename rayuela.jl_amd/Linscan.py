"""Host mirror of src/Linscan.jl: linscan_pq, linscan_opq, eval_recall."""
import numpy as np

from . import _lib
from .utils import _as_f32


def _codes_u8(B):
    B = np.asarray(B)
    if B.dtype == np.uint8:
        return np.ascontiguousarray(B)  # already the zero-based wire format (src/Linscan.jl:5-10)
    if not np.issubdtype(B.dtype, np.integer):
        raise TypeError("B must be an integer array")
    Bm1 = B.astype(np.int64) - 1  # src/Linscan.jl:35  convert(Matrix{UInt8}, B .- 1)
    if Bm1.min(initial=0) < 0 or Bm1.max(initial=0) > 255:
        raise OverflowError("InexactError: a one-based code outside 1..256 does not fit UInt8")
    return np.ascontiguousarray(Bm1.astype(np.uint8))


def _centers(C, m, d):
    sub = d // m
    arr = np.stack([_as_f32(c, "C[i]") for c in C])
    if arr.shape != (m, 256, sub):
        raise ValueError("linscan needs m codebooks of shape (256, d/m); got %s" % (arr.shape,))
    return np.ascontiguousarray(arr)  # == cat(C..., dims=3), src/Linscan.jl:22


def linscan_pq(B, X, C, b, k=10000):
    """linscan_pq(B, X, C, b, k=10000) -> dists, idx          (src/Linscan.jl:5-37)

    B : (n, m) uint8 zero-based codes, or any other integer dtype holding ONE-based codes
    X : (nq, d) float32 queries;  C : list of m (256, d/m) codebooks;  b = log2(h) * m
    Returns dists (nq, k) float32 ascending and idx (nq, k) uint32, ONE-based like the reference.
    """
    Bu = _codes_u8(B)
    X = _as_f32(X, "X")
    n, m = Bu.shape
    nq, d = X.shape
    if d % m:
        raise ValueError("InexactError: Cint(d/m) with d=%d m=%d (src/Linscan.jl:23)" % (d, m))
    if b != 8 * m:
        raise ValueError("b must be log2(256)*m = %d" % (8 * m))
    cen = _centers(C, m, d)
    dists = _lib.result_empty((nq, k), np.float32)     # every element is written by the library
    idx = _lib.result_empty((nq, k), np.uint32)
    _lib.check(_lib.lib().rq_linscan_pq(dists.ctypes.data, idx.ctypes.data, Bu.ctypes.data, cen.ctypes.data,
                                        X.ctypes.data, n, nq, m, d, k, 1))
    return dists, idx


def linscan_opq(B, X, C, b, R, k=10000):
    """linscan_opq(B, X, C, b, R, k=10000)   (src/Linscan.jl:93-115) == linscan_pq(B, R'X, C, b, k)."""
    Bu = _codes_u8(B)
    X = _as_f32(X, "X")
    R = _as_f32(R, "R")
    n, m = Bu.shape
    nq, d = X.shape
    if d % m:
        raise ValueError("InexactError: Cint(d/m) with d=%d m=%d" % (d, m))
    if b != 8 * m:
        raise ValueError("b must be log2(256)*m = %d" % (8 * m))
    cen = _centers(C, m, d)
    dists = _lib.result_empty((nq, k), np.float32)     # every element is written by the library
    idx = _lib.result_empty((nq, k), np.uint32)
    _lib.check(_lib.lib().rq_linscan_opq(dists.ctypes.data, idx.ctypes.data, Bu.ctypes.data, cen.ctypes.data,
                                         X.ctypes.data, R.ctypes.data, n, nq, m, d, k, 1))
    return dists, idx


def _codes_i16(B, h):
    """(codes (n, m) int16, code_base): uint16 / int16 arrays hold zero-based codes (what quantize_*_u16 return), any other
    integer dtype one-based codes (src/Linscan.jl:35 B .- 1)."""
    B = np.asarray(B)
    if B.ndim != 2:
        raise ValueError("B must be an (n, m) matrix of codes")
    if not np.issubdtype(B.dtype, np.integer):
        raise TypeError("B must be an integer array")
    base = 0 if B.dtype in (np.uint16, np.int16) else 1
    wide = B.astype(np.int64)
    if wide.min(initial=base) < base or wide.max(initial=base) > h - 1 + base:
        raise OverflowError("InexactError: a %s-based code outside %d..%d" % ("zero" if base == 0 else "one", base, h - 1 + base))
    return np.ascontiguousarray(wide.astype(np.int16)), base


def _centers_wide(C, m, d):
    from .utils import check_wide_h
    arr = np.stack([_as_f32(c, "C[i]") for c in C])
    if arr.ndim != 3 or arr.shape[0] != m or arr.shape[2] != d // m:
        raise ValueError("linscan needs m codebooks of shape (h, d/m); got %s" % (arr.shape,))
    check_wide_h(arr.shape[1])
    return np.ascontiguousarray(arr)


def _linscan_u16(B, X, C, R, k):
    X = _as_f32(X, "X")
    nq, d = X.shape
    m = len(C)
    if m < 1 or m > 32:
        raise ValueError("the scan over 16-bit codes covers 1 <= m <= 32 codebooks; got %d" % m)
    if d % m:
        raise ValueError("InexactError: Cint(d/m) with d=%d m=%d (src/Linscan.jl:23)" % (d, m))
    cen = _centers_wide(C, m, d)
    h = cen.shape[1]
    Bi, base = _codes_i16(B, h)
    n = Bi.shape[0]
    if Bi.shape[1] != m:
        raise ValueError("B has %d columns for %d codebooks" % (Bi.shape[1], m))
    if k < 1 or k > n:
        raise ValueError("k=%d must be in [1, n=%d]" % (k, n))
    dists = _lib.result_empty((nq, k), np.float32)     # every element is written by the library
    idx = _lib.result_empty((nq, k), np.uint32)
    if R is None:
        _lib.check(_lib.lib().rq_linscan_pq_wide(dists.ctypes.data, idx.ctypes.data, Bi.ctypes.data, cen.ctypes.data,
                                                 X.ctypes.data, n, nq, m, h, d, k, base, 1))
    else:
        R = _as_f32(R, "R")
        if R.shape != (d, d):
            raise ValueError("R must be (d, d)")
        _lib.check(_lib.lib().rq_linscan_opq_wide(dists.ctypes.data, idx.ctypes.data, Bi.ctypes.data, cen.ctypes.data,
                                                  X.ctypes.data, R.ctypes.data, n, nq, m, h, d, k, base, 1))
    return dists, idx


def linscan_pq_u16(B, X, C, k=10000):
    """linscan_pq over 16-bit codes: any 1 <= h <= 32767 codewords per codebook (rq_linscan_pq_wide) -> dists, idx

    B : (n, m) uint16 / int16 zero-based codes (what quantize_pq_u16 returns), or any other integer dtype holding ONE-based codes
    X : (nq, d) float32 queries;  C : list of m (h, d/m) codebooks
    Returns dists (nq, k) float32 ascending and idx (nq, k) uint32, ONE-based like linscan_pq: the k smallest (dist, id) pairs
    of the reference's arithmetic (src/Linscan.jl:5-37, deps/src/linscan_aqd.cpp:66-97) with h entries per table."""
    return _linscan_u16(B, X, C, None, k)


def linscan_opq_u16(B, X, C, R, k=10000):
    """linscan_opq over 16-bit codes (src/Linscan.jl:93-115; rq_linscan_opq_wide) == linscan_pq_u16(B, R'X, C, k)."""
    return _linscan_u16(B, X, C, R, k)


def _hcat_wide(C, d):
    from .utils import check_wide_h
    arr = np.stack([_as_f32(c, "C[i]") for c in C])
    if arr.ndim != 3 or arr.shape[2] != d:
        raise ValueError("linscan_lsq/cq need m codebooks of shape (h, d); got %s" % (arr.shape,))
    check_wide_h(arr.shape[1])
    return np.ascontiguousarray(arr)  # hcat(C...) == [m*h][d] in memory


def _linscan_aq_u16(B, X, C, k, lsq, dbnorms=None, cbnorms=None, R=None):
    X = _as_f32(X, "X")
    nq, d = X.shape
    m = len(C)
    if m < 1 or m > 32:
        raise ValueError("the scan over 16-bit codes covers 1 <= m <= 32 codebooks; got %d" % m)
    cb = _hcat_wide(C, d)
    h = cb.shape[1]
    Bi, base = _codes_i16(B, h)
    n = Bi.shape[0]
    if Bi.shape[1] != m:
        raise ValueError("B has %d columns for %d codebooks" % (Bi.shape[1], m))
    if k < 1 or k > n:
        raise ValueError("k=%d must be in [1, n=%d]" % (k, n))
    Rp = None
    if R is not None:
        Rp = _as_f32(R, "R")
        if Rp.shape != (d, d):
            raise ValueError("R must be (d, d)")
    if dbnorms is not None:
        nrm = np.ascontiguousarray(dbnorms, dtype=np.float32)
        if nrm.shape != (n,):
            raise ValueError("dbnorms must have one entry per database row")
    if cbnorms is not None:
        cbn = np.ascontiguousarray(_as_f32(cbnorms, "cbnorms").reshape(-1))
        if cbn.shape[0] < 1 or cbn.shape[0] > 32767:
            raise ValueError("cbnorms must hold 1..32767 entries; got %d" % cbn.shape[0])
    dists = _lib.result_empty((nq, k), np.float32)     # every element is written by the library
    idx = _lib.result_empty((nq, k), np.uint32)
    L = _lib.lib()
    Rptr = None if Rp is None else Rp.ctypes.data
    if not lsq:
        _lib.check(L.rq_linscan_cq_wide(dists.ctypes.data, idx.ctypes.data, Bi.ctypes.data, X.ctypes.data, cb.ctypes.data,
                                        n, nq, m, h, d, k, base, 1))
    elif cbnorms is None:
        _lib.check(L.rq_linscan_lsq_wide(dists.ctypes.data, idx.ctypes.data, Bi.ctypes.data, X.ctypes.data, cb.ctypes.data,
                                         nrm.ctypes.data, Rptr, n, nq, m, h, d, k, base, 1))
    else:
        _lib.check(L.rq_linscan_lsq_cbnorms_wide(dists.ctypes.data, idx.ctypes.data, Bi.ctypes.data, X.ctypes.data,
                                                 cb.ctypes.data, cbn.ctypes.data, cbn.shape[0], Rptr, n, nq, m, h, d, k, base, 1))
    return dists, idx


def linscan_lsq_u16(B, X, C, dbnorms, R, k=10000):
    """linscan_lsq over 16-bit codes: any 1 <= h <= 32767 codewords per codebook (rq_linscan_lsq_wide) -> dists, idx

    B : (n, m) uint16 / int16 zero-based codes, or any other integer dtype holding ONE-based codes (the dtype rule of
    linscan_pq_u16);  X : (nq, d) float32;  C : list of m (h, d) full-dimensional codebooks;  dbnorms (n,);  R (d, d) or None.
    idx ONE-based.  The arithmetic of src/Linscan.jl:118-157 / deps/src/linscan_aqd_pairwise_byte.cpp:14-94 with h entries per
    codebook; at h = 256 the answer of linscan_lsq."""
    if dbnorms is None:
        raise ValueError("dbnorms must have one entry per database row")
    return _linscan_aq_u16(B, X, C, k, True, dbnorms=dbnorms, R=R)


def linscan_cq_u16(B, X, C, k=10000):
    """linscan_cq over 16-bit codes (src/Linscan.jl:160-193; rq_linscan_cq_wide): T = |x - c|^2 per entry, no norms."""
    return _linscan_aq_u16(B, X, C, k, False)


def linscan_lsq_cbnorms_u16(B, X, C, cbnorms, R, k=10000):
    """linscan_lsq_u16 with the database norms given as a norms codebook of up to 32767 entries: quantize_norms and
    db_norms = norms_C[B_base_norms] (src/RVQ.jl:150-155) run on the device from the uploaded codes
    (rq_linscan_lsq_cbnorms_wide)."""
    if cbnorms is None:
        raise ValueError("cbnorms is required")
    return _linscan_aq_u16(B, X, C, k, True, cbnorms=cbnorms, R=R)


def _hcat(C, m, d):
    arr = np.concatenate([_as_f32(c, "C[i]") for c in C], axis=0)   # hcat(C...) == [m*h][d] in memory
    if arr.shape != (m * 256, d):
        raise ValueError("linscan_lsq/cq need m codebooks of shape (256, d); got %s" % (arr.shape,))
    return np.ascontiguousarray(arr)


def linscan_lsq(B, X, C, dbnorms, R, k=10000):
    """linscan_lsq(B, X, C, dbnorms, R, k=10000) -> dists, idx      (src/Linscan.jl:118-157)

    ADC search for additive (non-orthogonal) quantizers with the database norms passed apart:
    table T = -2<R'x, c> per codebook entry, dist = sum_k T[k][b_k] + dbnorms[row].
    B (n, m) uint8 zero-based (or other ints one-based); C list of m (256, d) full-dimensional codebooks;
    dbnorms (n,) float32; R (d, d).  idx ONE-based (the C code already returns them so, :76)."""
    Bu = _codes_u8(B)
    X = _as_f32(X, "X")
    R = _as_f32(R, "R")
    n, m = Bu.shape
    nq, d = X.shape
    cb = _hcat(C, m, d)
    nrm = np.ascontiguousarray(dbnorms, dtype=np.float32)
    if nrm.shape != (n,):
        raise ValueError("dbnorms must have one entry per database row")
    dists = _lib.result_empty((nq, k), np.float32)     # every element is written by the library
    idx = _lib.result_empty((nq, k), np.uint32)
    _lib.check(_lib.lib().rq_linscan_lsq(dists.ctypes.data, idx.ctypes.data, Bu.ctypes.data, X.ctypes.data,
                                         cb.ctypes.data, nrm.ctypes.data, R.ctypes.data, n, nq, m, 256, d, k, 1))
    return dists, idx


class LsqIndex:
    """linscan_lsq over a PREPARED base (rq_lsq_prepare): codes, dbnorms and codebooks stay on the device together with the
    pre-filter's O(n) preprocessing, which linscan_lsq otherwise repeats on every call.  search(X, R, k) returns exactly what
    linscan_lsq(B, X, C, dbnorms, R, k) returns."""

    def __init__(self, B, C, dbnorms):
        Bu = _codes_u8(B)
        n, m = Bu.shape
        d = np.asarray(C[0]).shape[1]
        cb = _hcat(C, m, d)
        nrm = np.ascontiguousarray(dbnorms, dtype=np.float32)
        if nrm.shape != (n,):
            raise ValueError("dbnorms must have one entry per database row")
        self.n, self.m, self.d = n, m, d
        self._h = _lib.lib().rq_lsq_prepare(Bu.ctypes.data, cb.ctypes.data, nrm.ctypes.data, n, m, 256, d)
        if not self._h:
            raise _lib.RayuelaHipError("rq_lsq_prepare: " + _lib.lib().rq_last_error().decode("utf-8", "replace"))

    @classmethod
    def from_cbnorms(cls, B, C, cbnorms):
        """The same handle from a norms codebook (rq_lsq_prepare_cbnorms): dbnorms = cbnorms[quantize_norms(B, C, cbnorms)] is
        computed on the device, so no per-row array is built on the host or uploaded.  search() returns exactly what
        LsqIndex(B, C, cbnorms[quantize_norms(B, C, cbnorms)[0] - 1]) returns."""
        Bu = _codes_u8(B)
        n, m = Bu.shape
        d = np.asarray(C[0]).shape[1]
        cb = _hcat(C, m, d)
        cbn = np.ascontiguousarray(_as_f32(cbnorms, "cbnorms").reshape(-1))
        self = cls.__new__(cls)
        self.n, self.m, self.d = n, m, d
        self._h = _lib.lib().rq_lsq_prepare_cbnorms(Bu.ctypes.data, cb.ctypes.data, cbn.ctypes.data, cbn.shape[0], n, m, 256, d)
        if not self._h:
            raise _lib.RayuelaHipError("rq_lsq_prepare_cbnorms: " + _lib.lib().rq_last_error().decode("utf-8", "replace"))
        return self

    def search(self, X, R=None, k=10000):
        X = _as_f32(X, "X")
        nq, d = X.shape
        if d != self.d:
            raise ValueError("queries must have d=%d columns" % self.d)
        Rp = None if R is None else _as_f32(R, "R")
        dists = _lib.result_empty((nq, k), np.float32)
        idx = _lib.result_empty((nq, k), np.uint32)
        _lib.check(_lib.lib().rq_lsq_search(self._h, dists.ctypes.data, idx.ctypes.data, X.ctypes.data,
                                            None if Rp is None else Rp.ctypes.data, nq, k, 1))
        return dists, idx

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rq_lsq_release(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def linscan_lsq_cbnorms(B, X, C, cbnorms, R, k=10000):
    """linscan_lsq with the database norms given as a norms codebook: the search leg of the experiment_* drivers
    (quantize_norms, db_norms = norms_C[B_base_norms], linscan_lsq; src/LSQ_GPU.jl:357-362) with the norms leg on the device."""
    with LsqIndex.from_cbnorms(B, C, cbnorms) as ix:
        return ix.search(X, R, k)


def linscan_cq(B, X, C, k=10000):
    """linscan_cq(B, X, C, k=10000) -> dists, idx      (src/Linscan.jl:160-193): T = |x - c|^2 per entry."""
    Bu = _codes_u8(B)
    X = _as_f32(X, "X")
    n, m = Bu.shape
    nq, d = X.shape
    cb = _hcat(C, m, d)
    dists = _lib.result_empty((nq, k), np.float32)     # every element is written by the library
    idx = _lib.result_empty((nq, k), np.uint32)
    _lib.check(_lib.lib().rq_linscan_cq(dists.ctypes.data, idx.ctypes.data, Bu.ctypes.data, X.ctypes.data,
                                        cb.ctypes.data, n, nq, m, 256, d, k, 1))
    return dists, idx


def linscan_aqd_query_extra_byte(codes, queries, codebooks, dbnorms, K):
    """Raw C symbol of deps/src/linscan_aqd_pairwise_byte.cpp:181-188 (ids ONE-based int32)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    codebooks = np.ascontiguousarray(codebooks, dtype=np.float32)
    n, m = codes.shape
    nq, d = queries.shape
    h = codebooks.shape[0] // m
    dists = np.zeros((nq, K), dtype=np.float32)
    idx = np.zeros((nq, K), dtype=np.int32)
    if dbnorms is None:
        _lib.lib().linscan_aqd_cq_query_extra_byte(dists.ctypes.data, idx.ctypes.data, codes.ctypes.data,
                                                   queries.ctypes.data, codebooks.ctypes.data, nq, n, m, h, d, K)
    else:
        dbnorms = np.ascontiguousarray(dbnorms, dtype=np.float32)
        _lib.lib().linscan_aqd_query_extra_byte(dists.ctypes.data, idx.ctypes.data, codes.ctypes.data,
                                                queries.ctypes.data, codebooks.ctypes.data, dbnorms.ctypes.data,
                                                nq, n, m, h, d, K)
    return dists, idx


def linscan_aqd_query(codes, centers, queries, K):
    """The raw C symbol of deps/src/linscan_aqd.cpp:105-114 (zero-based ids), as Linscan.jl ccalls it."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    centers = np.ascontiguousarray(centers, dtype=np.float32)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    n, m = codes.shape
    nq, d = queries.shape
    dists = np.zeros((nq, K), dtype=np.float32)
    res = np.zeros((nq, K), dtype=np.uint32)
    _lib.lib().linscan_aqd_query(dists.ctypes.data, res.ctypes.data, codes.ctypes.data, centers.ctypes.data,
                                 queries.ctypes.data, n, nq, 8 * m, K, m, d, d // m)
    return dists, res


def eval_recall(ids_gnd, ids_predicted, k, verbose=True):
    """eval_recall(gt, idx, k) -> recall_at_i     (src/Linscan.jl:196-234)

    rank_i = position of gt[i] in idx[i, :] (the whole row, like the reference) if it occurs exactly once, else k+1;
    recall_at_i[R-1] = #{rank <= R} / nq.  Prints r@{1,2,5,...} * 100 like the reference."""
    ids_gnd = np.asarray(ids_gnd).reshape(-1)
    P = np.asarray(ids_predicted)             # the WHOLE column is searched (src/Linscan.jl:207), also beyond k
    nq = P.shape[0]
    assert nq == ids_gnd.shape[0]
    hit = P == ids_gnd[:, None]
    cnt = hit.sum(axis=1)
    ranks = np.where(cnt == 1, hit.argmax(axis=1) + 1, k + 1)        # :209-213: exactly one occurrence, else k+1
    ranks = np.minimum(ranks, k + 1)                                  # a rank beyond k counts for no R <= k (:228)
    hist = np.bincount(ranks, minlength=k + 2)[1:k + 1]
    recall = np.cumsum(hist) / float(nq)
    if verbose:
        for i in (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000, 2000, 5000, 10000):
            if i <= k:
                print("r@%d = %s" % (i, recall[i - 1] * 100))
    return recall
