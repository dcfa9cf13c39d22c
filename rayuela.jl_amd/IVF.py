"""IVFADC (Jegou, Douze, Schmid, PAMI 2011) over the rq_ivf_* handle of include/rayuela_hip.h: a coarse quantizer of nlist
centroids in front of the ADC scan, so that a search reads nprobe lists instead of the whole base.  The reference has no inverted
file; the header states what every value is, in arithmetic the library pins elsewhere.  Host arrays in,
host arrays out; ids are ONE-based by default like every search of this package."""
import ctypes as C

import numpy as np

from . import _lib
from .Linscan import _centers, _codes_u8
from .utils import _as_f32, _as_f32_or_u8

MAX_NLIST = 32767     # RQ_MAX_H16
INFO_KEYS = ("n", "nlist", "m", "d", "by_residual", "largest_list", "empty_lists", "ld", "batch", "items", "rows_scanned",
             "next_id")
TIMING_KEYS = ("probe_ms", "items_ms", "keys_ms", "select_ms",
               # of the last build / set_codes / add: uploads + assignment + encode, grouping, carry of the loaded rows, placement
               "load_encode_ms", "load_group_ms", "load_carry_ms", "load_place_ms")


class IvfIndex:
    def __init__(self, Q, C_list, by_residual=True):
        """Q: (nlist, d) coarse centroids; C_list: the m (256, d/m) codebooks of the encoded vector -- the residual x - Q[list(x)]
        with by_residual, else x itself."""
        Q = _as_f32(Q, "Q")
        if Q.ndim != 2 or Q.shape[0] < 1 or Q.shape[0] > MAX_NLIST:
            raise ValueError("Q must be (nlist, d) with 1 <= nlist <= %d; got %s" % (MAX_NLIST, Q.shape,))
        nlist, d = Q.shape
        m = len(C_list)
        if m < 1 or m > 64:
            raise ValueError("the byte scan covers 1 <= m <= 64 codebooks; got %d" % m)
        if d % m:
            raise ValueError("d=%d is not a multiple of m=%d" % (d, m))
        cen = _centers(C_list, m, d)
        self.nlist, self.d, self.m, self.by_residual = nlist, d, m, bool(by_residual)
        self.n = 0
        self.next_id = 0      # the largest id loaded plus one: the least id_offset an add may take
        lib = _lib.lib()
        self._h = lib.rq_ivf_create(d, nlist, Q.ctypes.data, m, cen.ctypes.data, int(self.by_residual))
        if not self._h:
            raise _lib.RayuelaHipError("rq_ivf_create: " + lib.rq_last_error().decode("utf-8", "replace"))

    @classmethod
    def _unbound(cls, nlist, d, m, by_residual=True):
        """An index of this shape with no library handle behind it: its methods run their argument checks (which raise before
        the library is called) and nothing else.  What the tests use where there is no device."""
        ix = cls.__new__(cls)
        ix.nlist, ix.d, ix.m, ix.by_residual, ix.n, ix._h = nlist, d, m, bool(by_residual), 0, None
        ix.next_id = 0
        return ix

    @staticmethod
    def _check_id_offset(n, id_offset):
        if n < 1:
            raise ValueError("the base must hold at least one row")
        if id_offset < 0 or n + id_offset > 0xFFFFFFFF:
            raise ValueError("n + id_offset must stay below 2^32; got %d + %d" % (n, id_offset))

    def _rows(self, X):
        """X as the library takes it: float32, or uint8 rows, which stay bytes (any other dtype: TypeError)."""
        X = _as_f32_or_u8(X, "X")
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError("X must be (n, d=%d)" % self.d)
        return X

    def _check_add(self, n, id_offset):
        """The id rule and the limits of an add behind self.n loaded rows; returns the id_offset to use (None: the next id)."""
        if id_offset is None:
            id_offset = self.next_id if self.n else 0
        self._check_id_offset(n, id_offset)
        if self.n:
            if id_offset < self.next_id:
                raise ValueError("id_offset=%d lies below the next id %d (ids ascend inside a list; gaps are allowed)"
                                 % (id_offset, self.next_id))
            if self.n + n > 0xFFFFFFFF:
                raise ValueError("%d rows loaded + %d exceed 2^32 - 1 (offsets are uint32)" % (self.n, n))
        return int(id_offset)

    def _loaded(self, n, id_offset, added):
        self.n = self.n + n if added else n
        self.next_id = id_offset + n
        return self

    def build(self, X, id_offset=0):
        """Assign, take residuals, encode and group the rows of X (n, d) on the device; the id of row i is i + id_offset.  X is
        float32, or uint8 (bvecs): then the bytes travel as bytes and mean the rows widened to float32."""
        X = self._rows(X)
        if self.m > 32:
            raise ValueError("build encodes with 1 <= m <= 32 codebooks; got %d (set_codes takes codes)" % self.m)
        self._check_id_offset(X.shape[0], id_offset)
        entry = _lib.lib().rq_ivf_build_bytes if X.dtype == np.uint8 else _lib.lib().rq_ivf_build
        _lib.check(entry(self._h, X.ctypes.data, X.shape[0], id_offset))
        return self._loaded(X.shape[0], id_offset, False)

    def add(self, X, id_offset=None):
        """Put the rows of X (float32 or uint8) BEHIND the loaded base: afterwards the index holds what one build of all rows
        would have loaded.  id_offset (None: the next id, info()["next_id"]) must not lie below the next id; gaps are allowed.
        On an index with no base this is a build."""
        X = self._rows(X)
        if self.m > 32:
            raise ValueError("add encodes with 1 <= m <= 32 codebooks; got %d (add_codes takes codes)" % self.m)
        id_offset = self._check_add(X.shape[0], id_offset)
        entry = _lib.lib().rq_ivf_add_bytes if X.dtype == np.uint8 else _lib.lib().rq_ivf_add
        _lib.check(entry(self._h, X.ctypes.data, X.shape[0], id_offset))
        return self._loaded(X.shape[0], id_offset, True)

    def _lists_codes(self, lists, B):
        lists = np.asarray(lists)
        if lists.ndim != 1 or not np.issubdtype(lists.dtype, np.integer):
            raise ValueError("lists must be a vector of integers")
        Bu = _codes_u8(B)
        if Bu.ndim != 2 or Bu.shape != (lists.shape[0], self.m):
            raise ValueError("codes must be (n, m) = (%d, %d); got %s" % (lists.shape[0], self.m, Bu.shape))
        return lists, Bu

    def _list_range(self, lists):
        if lists.min() < 0 or lists.max() >= self.nlist:
            raise ValueError("a list id lies outside [0, %d)" % self.nlist)
        return np.ascontiguousarray(lists, dtype=np.uint32)

    def set_codes(self, lists, B, id_offset=0):
        """lists (n,): the list of every row, each in [0, nlist); B (n, m): uint8 zero-based codes, or another integer dtype
        holding ONE-based codes.  Replaces the base."""
        lists, Bu = self._lists_codes(lists, B)
        self._check_id_offset(Bu.shape[0], id_offset)
        lu = self._list_range(lists)
        _lib.check(_lib.lib().rq_ivf_set_codes(self._h, lu.ctypes.data, Bu.ctypes.data, Bu.shape[0], id_offset))
        return self._loaded(Bu.shape[0], id_offset, False)

    def add_codes(self, lists, B, id_offset=None):
        """set_codes for rows that go BEHIND the loaded base (see add)."""
        lists, Bu = self._lists_codes(lists, B)
        id_offset = self._check_add(Bu.shape[0], id_offset)
        lu = self._list_range(lists)
        _lib.check(_lib.lib().rq_ivf_add_codes(self._h, lu.ctypes.data, Bu.ctypes.data, Bu.shape[0], id_offset))
        return self._loaded(Bu.shape[0], id_offset, True)

    def search(self, Xq, nprobe, k, id_base=1):
        """The k nearest rows of the nprobe nearest lists per query: (dists (nq, k) float32 ascending, ids (nq, k) uint32); a
        union of fewer than k comparable rows ends in (NaN, 0xFFFFFFFF + id_base)."""
        Xq = _as_f32(Xq, "Xq")
        if Xq.ndim != 2 or Xq.shape[1] != self.d:
            raise ValueError("queries must be (nq, d=%d)" % self.d)
        if nprobe < 1 or nprobe > self.nlist:
            raise ValueError("1 <= nprobe <= nlist=%d; got %d" % (self.nlist, nprobe))
        if k < 1:
            raise ValueError("k must be positive; got %d" % k)
        if id_base not in (0, 1):
            raise ValueError("id_base must be 0 or 1")
        nq = Xq.shape[0]
        dists = _lib.result_empty((nq, k), np.float32)
        ids = _lib.result_empty((nq, k), np.uint32)
        _lib.check(_lib.lib().rq_ivf_search(self._h, dists.ctypes.data, ids.ctypes.data, Xq.ctypes.data, nq, int(nprobe), int(k),
                                            int(id_base)))
        return dists, ids

    def search_refine(self, Xq, ds, nprobe, k, kc, id_offset=0, id_base=1):
        """search(Xq, nprobe, kc) re-ranked on the device by the exact float32 distance to the rows of the resident Dataset ds
        (rq_ivf_search_refine; Dataset.rerank states the contract): row i of ds has id i + id_offset.  Equals
        ds.rerank(Xq, self.search(Xq, nprobe, kc, id_base)[1], k, id_offset, id_base) bit for bit, without the host round trip."""
        Xq = _as_f32(Xq, "Xq")
        if Xq.ndim != 2 or Xq.shape[1] != self.d:
            raise ValueError("queries must be (nq, d=%d)" % self.d)
        if nprobe < 1 or nprobe > self.nlist:
            raise ValueError("1 <= nprobe <= nlist=%d; got %d" % (self.nlist, nprobe))
        if not 1 <= k <= kc:
            raise ValueError("1 <= k <= kc; got k=%d, kc=%d" % (k, kc))
        if id_base not in (0, 1):
            raise ValueError("id_base must be 0 or 1")
        nq = Xq.shape[0]
        dists = _lib.result_empty((nq, k), np.float32)
        ids = _lib.result_empty((nq, k), np.uint32)
        _lib.check(_lib.lib().rq_ivf_search_refine(self._h, ds._h, dists.ctypes.data, ids.ctypes.data, Xq.ctypes.data, nq, int(nprobe),
                                                   int(k), int(kc), int(id_offset), int(id_base)))
        return dists, ids

    def lists(self):
        """(offsets (nlist + 1,) int64, ids (n,) uint32 with id_offset, codes (n, m) uint8) in grouped order."""
        n = (C.c_int64 * 1)()               # the library's own count: the base may have been loaded through the C entries
        _lib.check(_lib.lib().rq_ivf_info(self._h, C.cast(n, C.c_void_p), 1))
        offsets = np.empty(self.nlist + 1, dtype=np.int64)
        ids = np.empty(int(n[0]), dtype=np.uint32)
        codes = np.empty((int(n[0]), self.m), dtype=np.uint8)
        _lib.check(_lib.lib().rq_ivf_get_lists(self._h, offsets.ctypes.data, ids.ctypes.data, codes.ctypes.data))
        return offsets, ids, codes

    def info(self):
        out = (C.c_int64 * len(INFO_KEYS))()
        _lib.check(_lib.lib().rq_ivf_info(self._h, C.cast(out, C.c_void_p), len(INFO_KEYS)))
        ms = (C.c_double * len(TIMING_KEYS))()
        _lib.check(_lib.lib().rq_ivf_last_timing(self._h, C.cast(ms, C.c_void_p), len(TIMING_KEYS)))
        res = dict(zip(INFO_KEYS, [int(x) for x in out]))
        res.update(zip(TIMING_KEYS, [float(x) for x in ms]))
        return res

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rq_ivf_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def train_ivfpq(X, nlist, m, niter=25, seed=0, by_residual=True):
    """Q (nlist, d) and the m (256, d/m) codebooks C of an IvfIndex, from what exists: train_pq(X, 1, nlist) is the k-means of
    the coarse centroids, quantize_rvq_u16 with one stage gives the residuals x - Q[list(x)] the index will encode, train_pq on
    them (on X itself without by_residual) gives C."""
    from .PQ import train_pq
    from .RVQ import quantize_rvq_u16
    X = _as_f32(X, "X")
    if X.ndim != 2 or X.shape[1] % m:
        raise ValueError("X must be (n, d) with d a multiple of m=%d" % m)
    if nlist < 1 or nlist > MAX_NLIST:
        raise ValueError("1 <= nlist <= %d; got %d" % (MAX_NLIST, nlist))
    Cq, _, _ = train_pq(X, 1, nlist, niter, seed=seed)
    Q = np.ascontiguousarray(Cq[0], dtype=np.float32)
    Xe = X
    if by_residual:
        _, _, Xe = quantize_rvq_u16(X, [Q], with_extras=True)
    Cl, _, _ = train_pq(Xe, m, 256, niter, seed=seed + 1)
    return Q, Cl
