"""Exact k-nearest-neighbour ground truth on the device (rq_knn* of include/rayuela_hip.h).

The reference has no such function: it reads ground truth from the *_groundtruth.ivecs / gt files of src/read_datasets.jl and
compares against it in eval_recall (src/Linscan.jl:196-234).  groundtruth() makes what those files hold: per query the k rows
with the smallest (D64, id), D64 the squared distance accumulated coordinate by coordinate in float64 -- for every input, ties
and near-ties included."""
import ctypes as C

import numpy as np

from . import _lib
from .utils import _as_f32, _as_f32_or_u8

KNN_MAX_K = 1024            # RQ_KNN_MAX_K
KNN_PHASES = ["upload_ms", "keys_ms", "select_ms", "fold_ms", "rerank_ms", "widen_ms", "download_ms"]
KNN_STATS = ["queries", "candidates", "widened", "rounds", "host_finished", "chunks"]


def _queries(Xq, d):
    Xq = _as_f32(Xq, "Xq")
    if Xq.ndim != 2 or Xq.shape[1] != d:
        raise ValueError("queries must be (nq, %d)" % d)
    return Xq


def knn_f32(Xb, Xq, k=1, id_base=0):
    """Stage 1 alone (rq_knn_f32): (dists float32 [nq][k], ids uint32 [nq][k]), the k smallest (D32, id) pairs per query, D32
    the unfused float32 chain acc = acc + (x[s] - q[s]) * (x[s] - q[s]); any 1 <= k <= n."""
    Xb = _as_f32(Xb, "Xb")
    Xq = _queries(Xq, Xb.shape[1])
    nq = Xq.shape[0]
    dists = np.empty((nq, k), dtype=np.float32)
    ids = np.empty((nq, k), dtype=np.uint32)
    _lib.check(_lib.lib().rq_knn_f32(dists.ctypes.data, ids.ctypes.data, Xb.ctypes.data, Xq.ctypes.data, Xb.shape[0], nq,
                                     Xb.shape[1], int(k), int(id_base)))
    return dists, ids


def knn_f64(Xb, Xq, k=1, id_base=0):
    """The ground truth with the library's types: (dists float64 [nq][k], ids uint32 [nq][k]).  Xb float32 or uint8 rows, or a
    resident index.Dataset (then the base is not uploaded again)."""
    from .index import Dataset
    if isinstance(Xb, Dataset):
        return Xb.knn(Xq, k, id_base)
    Xb = _as_f32_or_u8(Xb, "Xb")
    Xq = _queries(Xq, Xb.shape[1])
    nq = Xq.shape[0]
    dists = np.empty((nq, k), dtype=np.float64)
    ids = np.empty((nq, k), dtype=np.uint32)
    fn = _lib.lib().rq_knn_bytes if Xb.dtype == np.uint8 else _lib.lib().rq_knn
    _lib.check(fn(dists.ctypes.data, ids.ctypes.data, Xb.ctypes.data, Xq.ctypes.data, Xb.shape[0], nq, Xb.shape[1], int(k),
                  int(id_base)))
    return dists, ids


def groundtruth(Xb, Xq, k=1, one_based=True):
    """(ids int32 [nq][k], dists float64 [nq][k]): the exact k nearest rows of Xb per query, nearest first, ties by id.  With
    one_based the ids have the form ivecs_write stores and eval_recall expects (src/Linscan.jl:196-234)."""
    dists, ids = knn_f64(Xb, Xq, k, 1 if one_based else 0)
    return ids.view(np.int32), dists


def last_knn_stats():
    """Counters of this thread's last knn call (rq_last_knn_stats): queries, candidates evaluated in float64, queries widened at
    least once, widening rounds, queries finished on the host, row chunks."""
    out = (C.c_uint64 * 8)()
    _lib.check(_lib.lib().rq_last_knn_stats(C.cast(out, C.c_void_p)))
    return dict(zip(KNN_STATS, [int(x) for x in out[:6]]))


def last_knn_timing():
    """Phase clock of this thread's last knn call (rq_last_knn_timing), in ms."""
    out = (C.c_double * 7)()
    _lib.check(_lib.lib().rq_last_knn_timing(C.cast(out, C.c_void_p), 7))
    return dict(zip(KNN_PHASES, [float(x) for x in out]))


def knn_chunk_rows(rows):
    """Test hook, not for callers (rq_test_knn_chunk_rows): rows > 0 splits the base of every later call into chunks of that
    many rows, 0 gives the planner its choice back.  Returns the previous value."""
    return int(_lib.lib().rq_test_knn_chunk_rows(int(rows)))


def knn_plan(n, nq, d, k):
    """The planner's decision (host code only, rq_knn_plan): first-round candidates per query, rows per chunk, row chunks, queries
    per batch, scratch bytes of a batch, and whether the test hook knn_chunk_rows set the chunk."""
    out = (C.c_int64 * 6)()
    _lib.check(_lib.lib().rq_knn_plan(int(n), int(nq), int(d), int(k), C.cast(out, C.c_void_p), 6))
    return dict(zip(["candidates", "chunk_rows", "chunks", "batch", "scratch_bytes", "forced"], [int(x) for x in out]))


RERANK_STATS = ["queries", "candidates", "valid", "batches", "chain", "keys_per_query"]
RERANK_PHASES = ["upload", "keys", "select", "download"]


def last_rerank_stats():
    """Counters of this thread's last re-ranking call (rq_last_rerank_stats; Dataset.rerank, IvfIndex.search_refine): queries,
    candidates, candidates inside the base, batches, the select path (0: sorted in LDS, 1: the select chain), keys per query row."""
    out = (C.c_uint64 * 8)()
    _lib.check(_lib.lib().rq_last_rerank_stats(C.cast(out, C.c_void_p)))
    return dict(zip(RERANK_STATS, [int(x) for x in out[:6]]))


def last_rerank_timing():
    """Phase clock of this thread's last re-ranking call (rq_last_rerank_timing), in ms."""
    out = (C.c_double * 4)()
    _lib.check(_lib.lib().rq_last_rerank_timing(C.cast(out, C.c_void_p), 4))
    return dict(zip(RERANK_PHASES, [float(x) for x in out]))


def rerank_limits(lds_kc=0, batch_queries=0):
    """Test hook, not for callers (rq_test_rerank_limits): the most candidates per query that are sorted in LDS and a cap on the
    queries per batch; 0 gives the planner its choice back.  Returns the previous (lds_kc, batch_queries)."""
    prev = int(_lib.lib().rq_test_rerank_limits(int(lds_kc), int(batch_queries)))
    return prev >> 32, prev & 0xFFFFFFFF


def rerank_plan(n, nq, d, kc, k):
    """The planner's decision (host code only, rq_rerank_plan): queries per batch, scratch bytes of a batch, the select path, keys
    per query row, and whether the test hook rerank_limits set the batch."""
    out = (C.c_int64 * 5)()
    _lib.check(_lib.lib().rq_rerank_plan(int(n), int(nq), int(d), int(kc), int(k), C.cast(out, C.c_void_p), 5))
    return dict(zip(["batch", "scratch_bytes", "chain", "keys_per_query", "forced"], [int(x) for x in out]))
