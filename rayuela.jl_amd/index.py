"""Device-resident index handle (rq_index_* of include/rayuela_hip.h): codes uploaded once, searched many
times -- on one MI355X or row-sharded over the GPUs of a node from this ONE process (the library gathers the
per-shard top-k lists over xGMI with RCCL and merges them on the first device).  Host arrays in, host arrays
out, like linscan_pq (src/Linscan.jl:5-26); ids are ONE-based by default like the reference's return value."""
import ctypes as C

import numpy as np

from . import _lib
from .Linscan import _centers, _centers_wide, _codes_i16, _codes_u8
from .utils import _as_f32

EXCHANGE = {0: "none", 1: "peer", 2: "rccl"}


def _devices_arg(devices):
    """devices (None, or a list of device ordinals, one shard per entry) as the create calls take it: (int array as a
    pointer, or None; count).  No library call."""
    if devices is None:
        return None, 0
    ndev = len(devices)
    return C.cast((C.c_int * ndev)(*[int(x) for x in devices]), C.c_void_p), ndev


class Index:
    def __init__(self, C_list, d, devices=None):
        """C_list: the m (256, d/m) codebooks; devices: None (current device) or a list of device ordinals,
        one shard per entry (a repeated ordinal = a logical shard on that device)."""
        m = len(C_list)
        self.m, self.d = m, d
        cen = _centers(C_list, m, d)
        devs, ndev = _devices_arg(devices)
        lib = _lib.lib()
        if devs is None:
            self._h = lib.rq_index_create(m, d, cen.ctypes.data)
        else:
            self._h = lib.rq_index_create_sharded(m, d, cen.ctypes.data, devs, ndev)
        if not self._h:
            raise _lib.RayuelaHipError("rq_index_create: " + lib.rq_last_error().decode("utf-8", "replace"))
        self.n = 0

    def set_codes(self, B, id_offset=0):
        """B (n, m): uint8 zero-based codes, or another integer dtype holding ONE-based codes (src/Linscan.jl:28-37)."""
        Bu = _codes_u8(B)
        if Bu.shape[1] != self.m:
            raise ValueError("codes must have m=%d columns" % self.m)
        _lib.check(_lib.lib().rq_index_set_codes(self._h, Bu.ctypes.data, Bu.shape[0], id_offset))
        self.n = Bu.shape[0]
        return self

    def set_codes_synth(self, n, seed, id_offset=0):
        """SIFT1B-shape synthetic base generated on the devices (synth.random_codes gives the same bytes)."""
        _lib.check(_lib.lib().rq_index_set_codes_synth(self._h, int(n), int(seed), id_offset))
        self.n = int(n)
        return self

    def search(self, X, k=10000, R=None, id_base=1):
        X = _as_f32(X, "X")
        nq, d = X.shape
        if d != self.d:
            raise ValueError("queries must have d=%d columns" % self.d)
        dists = _lib.result_empty((nq, k), np.float32)
        idx = _lib.result_empty((nq, k), np.uint32)
        lib = _lib.lib()
        if R is None:
            _lib.check(lib.rq_index_search(self._h, dists.ctypes.data, idx.ctypes.data, X.ctypes.data, nq, k, id_base))
        else:
            R = _as_f32(R, "R")
            _lib.check(lib.rq_index_search_opq(self._h, dists.ctypes.data, idx.ctypes.data, X.ctypes.data,
                                               R.ctypes.data, nq, k, id_base))
        return dists, idx

    def search_refine(self, X, ds, k, kc, R=None, id_base=1):
        """search(k=kc) re-ranked by the exact distance to the rows of the resident Dataset ds (Dataset.rerank): (dists (nq, k)
        float32, ids (nq, k) uint32).  The queries are re-ranked unrotated against the unrotated base; row i of ds is row i of
        the codes AND has id i: a handle whose codes were loaded with an id_offset is not supported here (its ids would name
        other rows of ds, or none) -- call ds.rerank(X, cand, k, id_offset=...) on the result of search yourself.  Inherited by
        every index class, sharded handles included."""
        _, cand = self.search(X, k=kc, R=R, id_base=id_base)
        return ds.rerank(X, cand, k, id_offset=0, id_base=id_base)

    def info(self):
        out = (C.c_int64 * 68)()
        _lib.check(_lib.lib().rq_index_info(self._h, C.cast(out, C.c_void_p), 68))
        P = int(out[0])
        return {"shards": P, "devices": int(out[1]), "exchange": EXCHANGE.get(int(out[2]), "?"), "n": int(out[3]),
                "rows_per_shard": [int(out[4 + i]) for i in range(min(P, 64))]}

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rq_index_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class IndexU16(Index):
    """The index over 16-bit codes (rq_index_*_wide): codebooks of any 1 <= h <= 32767 codewords, 1 <= m <= 32.  search, info,
    close and the context manager are Index's; a search returns what linscan_pq_u16 / linscan_opq_u16 return on the same
    base, bit for bit."""

    def __init__(self, C_list, d, devices=None):
        """C_list: the m (h, d/m) codebooks; devices as for Index."""
        m = len(C_list)
        if m < 1 or m > 32:
            raise ValueError("the scan over 16-bit codes covers 1 <= m <= 32 codebooks; got %d" % m)
        if d % m:
            raise ValueError("InexactError: Cint(d/m) with d=%d m=%d (src/Linscan.jl:23)" % (d, m))
        self.m, self.d = m, d
        cen = _centers_wide(C_list, m, d)
        self.h = cen.shape[1]
        devs, ndev = _devices_arg(devices)
        lib = _lib.lib()
        if devs is None:
            self._h = lib.rq_index_create_wide(m, self.h, d, cen.ctypes.data)
        else:
            self._h = lib.rq_index_create_sharded_wide(m, self.h, d, cen.ctypes.data, devs, ndev)
        if not self._h:
            raise _lib.RayuelaHipError("rq_index_create_wide: " + lib.rq_last_error().decode("utf-8", "replace"))
        self.n = 0

    def set_codes(self, B, id_offset=0):
        """B (n, m): uint16 / int16 zero-based codes (what quantize_*_u16 and Dataset.quantize_u16 return), or another integer
        dtype holding ONE-based codes (Linscan._codes_i16)."""
        Bi, base = _codes_i16(B, self.h)
        if Bi.shape[1] != self.m:
            raise ValueError("codes must have m=%d columns" % self.m)
        _lib.check(_lib.lib().rq_index_set_codes_wide(self._h, Bi.ctypes.data, Bi.shape[0], base, id_offset))
        self.n = Bi.shape[0]
        return self

    def set_codes_synth(self, n, seed, id_offset=0):
        raise NotImplementedError("synthetic bases are byte codes (Index.set_codes_synth)")


AQ_KINDS = {"lsq": 1, "cq": 2}      # lut_mode of rq_index_create_aq (the values of rq_dev_linscan_aq)


class AqIndex(Index):
    """The index of an additive quantizer over byte codes (rq_index_create_aq, h = 256): LSQ / LSQ++ codes with their database
    norms (kind="lsq") or ChainQ-style codes searched with T = |q - c|^2 (kind="cq"), resident on one device or row-sharded like
    Index.  search returns what linscan_lsq / linscan_cq return on the whole base, bit for bit; close and the context manager are
    Index's."""

    WIDE = False
    M_MAX = 64
    HN_MAX = 256

    def __init__(self, C_list, kind="lsq", devices=None):
        """C_list: the m (256, d) full-dimensional codebooks; devices as for Index."""
        cb = self._check_create(C_list, kind)
        devs, ndev = _devices_arg(devices)
        lib = _lib.lib()
        if self.WIDE:
            self._h = lib.rq_index_create_aq_wide(self.m, self.h, self.d, cb.ctypes.data, AQ_KINDS[kind], devs, ndev)
        else:
            self._h = lib.rq_index_create_aq(self.m, self.d, cb.ctypes.data, AQ_KINDS[kind], devs, ndev)
        if not self._h:
            raise _lib.RayuelaHipError("rq_index_create_aq: " + lib.rq_last_error().decode("utf-8", "replace"))
        self.n = 0

    def _check_create(self, C_list, kind):
        """Shape checks of the constructor (no library call): sets m, h, d, kind; returns hcat(C...) [m*h][d] float32."""
        if kind not in AQ_KINDS:
            raise ValueError("kind must be 'lsq' or 'cq'; got %r" % (kind,))
        m = len(C_list)
        if m < 1 or m > self.M_MAX:
            raise ValueError("the %s AQ index covers 1 <= m <= %d codebooks; got %d" % ("wide" if self.WIDE else "byte", self.M_MAX, m))
        first = np.asarray(C_list[0])
        if first.ndim != 2 or first.shape[1] < 1:
            raise ValueError("codebooks must be (h, d) matrices; got %s" % (first.shape,))
        d = first.shape[1]
        if self.WIDE:
            from .Linscan import _hcat_wide
            cb = _hcat_wide(C_list, d)
            h = cb.shape[1]
        else:
            from .Linscan import _hcat
            cb = _hcat(C_list, m, d)
            h = 256
        self.m, self.h, self.d, self.kind = m, h, d, kind
        return cb

    def _check_norms(self, n, dbnorms, cbnorms):
        """(dbnorms [n] f32 or None, cbnorms [hn] f32 or None) as the library wants them, or ValueError (no library call)."""
        if self.kind == "cq":
            if dbnorms is not None or cbnorms is not None:
                raise ValueError("a CQ index takes no norms")
            return None, None
        if (dbnorms is None) == (cbnorms is None):
            raise ValueError("an LSQ index takes exactly one of dbnorms and cbnorms")
        if dbnorms is not None:
            nrm = np.ascontiguousarray(dbnorms, dtype=np.float32)
            if nrm.shape != (n,):
                raise ValueError("dbnorms must have one entry per database row")
            return nrm, None
        cbn = np.ascontiguousarray(_as_f32(cbnorms, "cbnorms").reshape(-1))
        if cbn.shape[0] < 1 or cbn.shape[0] > self.HN_MAX:
            raise ValueError("cbnorms must hold 1..%d entries; got %d" % (self.HN_MAX, cbn.shape[0]))
        return None, cbn

    def _check_codes(self, B):
        Bu = _codes_u8(B)
        if Bu.ndim != 2 or Bu.shape[1] != self.m:
            raise ValueError("codes must be (n, m=%d)" % self.m)
        if Bu.shape[0] < 1:
            raise ValueError("codes must hold at least one row")
        return Bu, 0

    def set_codes(self, B, dbnorms=None, cbnorms=None, id_offset=0):
        """B (n, m): uint8 zero-based codes, or another integer dtype holding ONE-based codes.  kind="lsq" takes exactly one of
        dbnorms (n,) and cbnorms (hn <= 256,): with cbnorms, dbnorms = cbnorms[quantize_norms(B, C, cbnorms)] is computed on the
        devices.  kind="cq" takes neither.  Replaces the previous base and its norms."""
        Bc, base = self._check_codes(B)
        n = Bc.shape[0]
        nrm, cbn = self._check_norms(n, dbnorms, cbnorms)
        pn = None if nrm is None else nrm.ctypes.data
        pc = None if cbn is None else cbn.ctypes.data
        hn = 0 if cbn is None else cbn.shape[0]
        if self.WIDE:
            _lib.check(_lib.lib().rq_index_set_codes_aq_wide(self._h, Bc.ctypes.data, pn, pc, hn, n, base, id_offset))
        else:
            _lib.check(_lib.lib().rq_index_set_codes_aq(self._h, Bc.ctypes.data, pn, pc, hn, n, id_offset))
        self.n = n
        return self

    def set_codes_synth(self, n, seed, id_offset=0):
        raise NotImplementedError("synthetic bases are PQ codes (Index.set_codes_synth)")

    def search(self, X, k=10000, R=None, id_base=1):
        """linscan_lsq(B, X, C, dbnorms, R, k) / linscan_cq(B, X, C, k) against the resident base: (dists, idx)."""
        if R is not None and np.shape(R) != (self.d, self.d):
            raise ValueError("R must be (d, d) = (%d, %d)" % (self.d, self.d))
        if np.ndim(X) != 2:
            raise ValueError("queries must be an (nq, d) matrix")
        return Index.search(self, X, k, R, id_base)

    def info(self):
        """Index.info() plus kind, h and per shard: ordered (rows in bank-aware order) and prepared (holds the LSQ pre-filter's
        norm buffer)."""
        out = Index.info(self)
        aq = (C.c_int64 * 132)()
        _lib.check(_lib.lib().rq_index_aq_info(self._h, C.cast(aq, C.c_void_p), 132))
        P = int(aq[3])
        out.update(kind={1: "lsq", 2: "cq"}.get(int(aq[0]), "pq"), wide=bool(aq[1]), h=int(aq[2]),
                   ordered=[bool(aq[4 + 2 * i]) for i in range(min(P, 64))],
                   prepared=[bool(aq[5 + 2 * i]) for i in range(min(P, 64))])
        return out


class AqIndexU16(AqIndex):
    """AqIndex over 16-bit codes (rq_index_create_aq_wide): codebooks of any 1 <= h <= 32767 codewords, 1 <= m <= 32.  search
    returns what linscan_lsq_u16 / linscan_cq_u16 / linscan_lsq_cbnorms_u16 return on the whole base, bit for bit."""

    WIDE = True
    M_MAX = 32
    HN_MAX = 32767

    def _check_codes(self, B):
        Bi, base = _codes_i16(B, self.h)
        if Bi.shape[1] != self.m:
            raise ValueError("codes must be (n, m=%d)" % self.m)
        if Bi.shape[0] < 1:
            raise ValueError("codes must hold at least one row")
        return Bi, base


class Dataset:
    """A base set resident on the device (rq_dataset_*): uploaded once, encoded as often as needed.  X float32, or uint8
    (bvecs data), which stays n * d bytes on the device and encodes to the codes of X.astype(float32)."""

    def __init__(self, X):
        from .utils import _as_f32_or_u8
        X = _as_f32_or_u8(X, "X")
        self.n, self.d = X.shape
        upload = _lib.lib().rq_dataset_upload_bytes if X.dtype == np.uint8 else _lib.lib().rq_dataset_upload
        self._h = upload(X.ctypes.data, self.n, self.d)
        if not self._h:
            raise _lib.RayuelaHipError("rq_dataset_upload: " + _lib.lib().rq_last_error().decode("utf-8", "replace"))

    def quantize(self, C_list, R=None, one_based=True):
        """quantize_pq(X, C) (R is None) or quantize_opq(X, R, C): (n, m) int16 one-based like the reference's
        return value, or uint8 zero-based (the scan's wire format) with one_based=False."""
        from .utils import cat_codebooks
        m = len(C_list)
        h = C_list[0].shape[0]
        Cc = np.ascontiguousarray(cat_codebooks(C_list), dtype=np.float32)
        Rp = None if R is None else _as_f32(R, "R")
        out = np.empty((self.n, m), dtype=np.int16 if one_based else np.uint8)
        _lib.check(_lib.lib().rq_dataset_encode(self._h, None if one_based else out.ctypes.data,
                                                out.ctypes.data if one_based else None,
                                                None if Rp is None else Rp.ctypes.data, Cc.ctypes.data, m, h))
        return out

    def quantize_u16(self, C_list, R=None, one_based=False):
        """quantize for codebooks of any 1 <= h <= 32767 codewords (rq_dataset_encode_wide), on a float32 or a uint8 base:
        (n, m) zero-based codes viewed as uint16 (what quantize_pq_u16 / quantize_opq_u16 return and IndexU16.set_codes takes),
        or int16 one-based like the reference's return value with one_based=True."""
        from .utils import cat_codebooks, check_wide_h
        m = len(C_list)
        h = np.asarray(C_list[0]).shape[0]
        check_wide_h(h)
        Cc = np.ascontiguousarray(cat_codebooks(C_list), dtype=np.float32)
        if Cc.size != h * self.d:
            raise ValueError("codebooks do not tile the %d dimensions of the base" % self.d)
        Rp = None if R is None else _as_f32(R, "R")
        if Rp is not None and Rp.shape != (self.d, self.d):
            raise ValueError("R must be %d x %d" % (self.d, self.d))
        out = np.empty((self.n, m), dtype=np.int16)
        _lib.check(_lib.lib().rq_dataset_encode_wide(self._h, out.ctypes.data, None if Rp is None else Rp.ctypes.data,
                                                     Cc.ctypes.data, m, h, 1 if one_based else 0))
        return out if one_based else out.view(np.uint16)

    def knn(self, Xq, k=1, id_base=0):
        """The exact k nearest rows of this base per query (rq_dataset_knn; see knn.groundtruth): (dists float64 [nq][k],
        ids uint32 [nq][k]), the base staying where it is."""
        Xq = _as_f32(Xq, "Xq")
        if Xq.ndim != 2 or Xq.shape[1] != self.d:
            raise ValueError("queries must be (nq, %d)" % self.d)
        nq = Xq.shape[0]
        dists = np.empty((nq, k), dtype=np.float64)
        ids = np.empty((nq, k), dtype=np.uint32)
        _lib.check(_lib.lib().rq_dataset_knn(self._h, dists.ctypes.data, ids.ctypes.data, Xq.ctypes.data, nq, int(k),
                                             int(id_base)))
        return dists, ids

    def rerank(self, Xq, cand, k, id_offset=0, id_base=1):
        """The candidates of a search ordered by their exact float32 distance to the rows of this base (rq_dataset_rerank):
        cand (nq, kc) uint32 ids as a search returned them (id_base and id_offset on them; columns of a wider array are taken in
        place), of which the k nearest per query come back as (dists (nq, k) float32 ascending, ids (nq, k) uint32).  Ids outside
        the base -- the searches' padding id among them -- are skipped, an id given twice appears twice, and a list with fewer
        than k valid candidates ends in (NaN, 0xFFFFFFFF + id_base)."""
        Xq = _as_f32(Xq, "Xq")
        if Xq.ndim != 2 or Xq.shape[1] != self.d:
            raise ValueError("queries must be (nq, %d)" % self.d)
        cand = np.asarray(cand)
        if cand.dtype != np.uint32 or cand.ndim != 2 or cand.shape[0] != Xq.shape[0]:
            raise ValueError("cand must be uint32 (nq, kc)")
        if cand.shape[1] and (cand.strides[1] != 4 or cand.strides[0] % 4 or cand.strides[0] < 4 * cand.shape[1]):
            cand = np.ascontiguousarray(cand)
        nq, kc = cand.shape
        ldc = cand.strides[0] // 4 if nq > 1 and kc else kc
        if not 1 <= k <= kc:
            raise ValueError("1 <= k <= kc=%d; got %d" % (kc, k))
        if id_base not in (0, 1):
            raise ValueError("id_base must be 0 or 1")
        dists = _lib.result_empty((nq, k), np.float32)
        ids = _lib.result_empty((nq, k), np.uint32)
        _lib.check(_lib.lib().rq_dataset_rerank(self._h, dists.ctypes.data, ids.ctypes.data, Xq.ctypes.data, nq, cand.ctypes.data,
                                                kc, ldc, int(k), int(id_offset), int(id_base)))
        return dists, ids

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rq_dataset_free(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
