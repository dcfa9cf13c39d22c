"""numpy restatement of the IVFADC index (include/rayuela_hip.h, "IVFADC").  TEST INFRASTRUCTURE.

The reference has no inverted file, so the semantics are written out from arithmetic the oracle already pins; nothing here but
oracle.pq_distmat (the canonical encode distance), oracle.encode_pq (the byte encode), oracle.adc_distances (the reference's table
and row sum) and a lexicographic sort.  oracle.encode_pq / oracle.encode_rvq at m = 1 return uint8 codes, so they state list(x) and
the residual only up to 256 lists; lists_of / residuals state them for any nlist and tests/test_ivf_oracle.py holds the two
against those functions where they apply.

  coarse value   U = oracle.pq_distmat(X, Q, 1, nlist): fl(fl(sa + sb) - 2 g);  v = U > 0 ? U : 0
  build          a NaN U counts as 0, as in the encode (oracle/rq_oracle.c:312 `v > 0 ? v : 0`); first-index argmin.  (Under a
                 non-finite CENTROID the device encode promises lists in range and nothing more -- include/rayuela_hip.h,
                 "Non-finite inputs of the encode", point 3 -- so tests load such a base through set_codes.)
  probes         a NaN U stays NaN and sorts behind every number, +Inf included; ties go to the lower list
  distance       oracle.adc_distances(codes of the list, C, q - Q[p] or q); a NaN distance is no neighbour; -0 counts as +0
  answer         the k smallest (dist, id), ids + id_base; then (PAD_BITS, 0xFFFFFFFF + id_base)

search() is take(ranked()): ranked orders the comparable rows of every query once, take cuts any k and id_base off that order;
search_tiled evaluates the distinct queries of a tiling once.  tests/test_ivf_oracle.py holds the three to one another.
"""
import numpy as np

from oracle import oracle

PAD_BITS = 0x7FFFFFFF     # the float whose ordered bits are 0xFFFFFFFF: what the select chain's unpack writes for a missing key
PAD_ID = 0xFFFFFFFF


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def coarse_u(X, Q):
    """U [n][nlist]: the unclamped canonical distances of every row to every coarse centroid."""
    Q = _f32(Q)
    return oracle.pq_distmat(_f32(X), Q, 1, Q.shape[0])[:, 0, :]


def lists_of(X, Q):
    """list(x): first-index argmin of the clamped value, a NaN counting as 0 (the encode's clamp)."""
    U = coarse_u(X, Q)
    with np.errstate(invalid="ignore"):
        v = np.where(U > 0, U, np.float32(0))
    return np.argmin(v, axis=1).astype(np.int64)


def residuals(X, Q, lists):
    """x - Q[list(x)], one f32 subtraction per element (RVQ's stage epilogue)."""
    return (_f32(X) - _f32(Q)[lists]).astype(np.float32)


def probe_order(Xq, Q):
    """[nq][nlist] list indices, nearest first: ascending (v, j), a NaN v behind every number."""
    U = coarse_u(Xq, Q)
    nan = np.isnan(U)
    with np.errstate(invalid="ignore"):
        v = np.where(nan, np.float32(0), np.where(U > 0, U, np.float32(0)))
    j = np.broadcast_to(np.arange(U.shape[1]), U.shape)
    return np.stack([np.lexsort((j[q], v[q], nan[q])) for q in range(U.shape[0])])


def group(lists, codes, nlist, id_offset=0):
    """(offsets [nlist + 1] int64, ids [n] uint32, codes [n][m]) grouped by list, inside a list in ascending id."""
    lists = np.asarray(lists, dtype=np.int64)
    order = np.argsort(lists, kind="stable")
    offsets = np.zeros(nlist + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(lists, minlength=nlist))
    ids = ((order.astype(np.int64) + int(id_offset)) & 0xFFFFFFFF).astype(np.uint32)
    return offsets, ids, np.ascontiguousarray(np.asarray(codes)[order])


def build(X, Q, centers, by_residual, id_offset=0):
    """centers [m][256][d/m].  Returns (offsets, ids, codes) as group() and the arrival-order (lists, encoded vectors, codes)."""
    centers = _f32(centers)
    m = centers.shape[0]
    lists = lists_of(X, Q)
    enc = residuals(X, Q, lists) if by_residual else _f32(X)
    codes = oracle.encode_pq(enc, centers, m, 256)
    return group(lists, codes, _f32(Q).shape[0], id_offset), (lists, enc, codes)


def ranked(grouped, Q, centers, by_residual, Xq, nprobe):
    """Per query the comparable rows of its nprobe nearest lists in answer order: a list of (dist f32, ids u32 without id_base),
    ascending (dist, id).  Every k and id_base of one (queries, nprobe) cuts its answer off these (take)."""
    offsets, ids, codes = grouped
    Q, centers, Xq = _f32(Q), _f32(centers), _f32(Xq)
    order = probe_order(Xq, Q)[:, :nprobe]
    sizes = np.diff(offsets)
    out = []
    for q in range(Xq.shape[0]):
        dd, ii = [np.empty(0, dtype=np.float32)], [np.empty(0, dtype=np.uint32)]
        for p in order[q][sizes[order[q]] > 0]:
            b, e = int(offsets[p]), int(offsets[p + 1])
            with np.errstate(invalid="ignore", over="ignore"):
                qp = (Xq[q] - Q[p]).astype(np.float32) if by_residual else Xq[q]
            dd.append(oracle.adc_distances(codes[b:e], centers, qp))
            ii.append(ids[b:e])
        dist = np.concatenate(dd) + np.float32(0)          # -0 counts as +0
        idv = np.concatenate(ii)
        keep = ~np.isnan(dist)
        dist, idv = dist[keep], idv[keep]
        top = np.lexsort((idv, dist))
        out.append((dist[top], idv[top]))
    return out


def take(rows, k, id_base=1):
    """(dists [nq][k] f32, ids [nq][k] u32): the first k entries of every query of ranked(), ids + id_base, then the padding."""
    out_d = np.full((len(rows), k), PAD_BITS, dtype=np.uint32)
    out_i = np.full((len(rows), k), (PAD_ID + id_base) & 0xFFFFFFFF, dtype=np.uint32)
    for q, (dist, idv) in enumerate(rows):
        c = min(k, dist.size)
        out_d[q, :c] = dist[:c].view(np.uint32)
        out_i[q, :c] = ((idv[:c].astype(np.int64) + id_base) & 0xFFFFFFFF).astype(np.uint32)
    return out_d.view(np.float32), out_i


def search(grouped, Q, centers, by_residual, Xq, nprobe, k, id_base=1):
    """(dists [nq][k] f32, ids [nq][k] u32) of the restated search over a grouped base."""
    return take(ranked(grouped, Q, centers, by_residual, Xq, nprobe), k, id_base)


def search_tiled(grouped, Q, centers, by_residual, Xd, tile, nprobe, k, id_base=1):
    """search() for the queries Xd[tile]: a query's answer depends on no other query, so each distinct one is evaluated once."""
    dists, ids = search(grouped, Q, centers, by_residual, Xd, nprobe, k, id_base)
    tile = np.asarray(tile, dtype=np.int64)
    return dists[tile], ids[tile]


def union_sizes(grouped, Q, Xq, nprobe):
    """rows in the probed lists of every query"""
    offsets = grouped[0]
    sizes = np.diff(offsets)
    return sizes[probe_order(Xq, Q)[:, :nprobe]].sum(axis=1)


def item_counts(grouped, Q, Xq, nprobe, segment):
    """work items of every query: one per `segment` rows, or part of that, of each probed list (IVF_SEGMENT_ROWS)"""
    sizes = np.diff(grouped[0])
    return (-(-sizes // segment))[probe_order(Xq, Q)[:, :nprobe]].sum(axis=1)
