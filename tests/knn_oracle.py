"""The contract of the exact k-nearest-neighbour entries (include/rayuela_hip.h, rq_knn*), restated in plain numpy.

A plain helper module, imported by the tests (not a conftest).  It never calls into the HIP library.  Base X [n][d] (f32, or u8
widened exactly), queries Q [nq][d] f32; one numpy operation per rounding, vectorised over the (query, row) pairs with a loop
over the coordinate s:

  D32   acc = +0; for s: t = x[s] - q[s]; acc = acc + t * t      in float32
  D64   the same on the values widened to float64, in float64

Stage 1 (rq_knn_f32) is the scans' contract (tests/nonfinite_ref.contract) on D32; the ground truth is the k smallest (D64, id)
pairs, a NaN D64 never a neighbour, a short list ending in the scans' padding id with distance +Inf.  The certification rule of
the two-stage evaluation is restated too, so that the tests can say how many candidates an input needs."""
import numpy as np

import nonfinite_ref as nf

FLT_MAX = float(np.finfo(np.float32).max)
PAD_ID = 0xFFFFFFFF


def _rows(X):
    X = np.asarray(X)
    assert X.dtype in (np.float32, np.uint8), X.dtype
    return np.ascontiguousarray(X, dtype=np.float32)           # u8 -> f32 is exact


def d32(X, Q):
    """D32 [nq][n] float32."""
    x, q = _rows(X), np.ascontiguousarray(Q, dtype=np.float32)
    acc = np.zeros((q.shape[0], x.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for s in range(x.shape[1]):
            t = x[None, :, s] - q[:, s][:, None]
            sq = t * t
            acc = acc + sq
    return acc


def d64(X, Q):
    """D64 [nq][n] float64."""
    x, q = _rows(X).astype(np.float64), np.ascontiguousarray(Q, dtype=np.float32).astype(np.float64)
    acc = np.zeros((q.shape[0], x.shape[0]), dtype=np.float64)
    with np.errstate(all="ignore"):
        for s in range(x.shape[1]):
            t = x[None, :, s] - q[:, s][:, None]
            sq = t * t
            acc = acc + sq
    return acc


def topk_f32(D32, k, id_base=0):
    """(distance bits [nq][k] u32, ids [nq][k] u32, keys [nq][k] u64): the scans' contract per query."""
    out = [nf.contract(row, k, id_base) for row in D32]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


def topk_f64(D64, k, id_base=0):
    """(dists [nq][k] f64, ids [nq][k] u32): the k smallest (D64, id) pairs, NaN never, padding (+Inf, 0xFFFFFFFF + id_base)."""
    nq = D64.shape[0]
    dists = np.full((nq, k), np.inf, dtype=np.float64)
    ids = np.full((nq, k), (PAD_ID + id_base) & 0xFFFFFFFF, dtype=np.uint32)
    for q in range(nq):
        dv = D64[q] + 0.0
        rows = np.flatnonzero(~np.isnan(dv))
        rows = rows[np.lexsort((rows, dv[rows]))][:k]
        dists[q, :rows.size] = dv[rows]
        ids[q, :rows.size] = rows + id_base
    return dists, ids


def groundtruth(X, Q, k, id_base=0):
    return topk_f64(d64(X, Q), k, id_base)


def gamma(d):
    return 2.0 * (d + 3) * 2.0 ** -24


def delta(d):
    return d * 2.0 ** -125


def first_candidates(n, k):
    return min(n, k + max(32, k // 4))


def certified(d32_row, d64_row, k, kp, d):
    """Is a query (d32_row / d64_row: its distances to all n rows) certified with kp stage-1 candidates?  The rule of the
    header: k' == n, or the candidate list ran out of comparable rows, or L > T64 (1 + gamma) + delta."""
    n = d32_row.shape[0]
    if kp >= n:
        return True
    bits, ids, keys = nf.contract(d32_row, kp)
    if keys[-1] == nf.KEY_MAX:
        return True
    cand = ids.astype(np.int64)
    c64 = d64_row[cand]
    c64 = np.sort(c64[~np.isnan(c64)])
    t64 = c64[k - 1] if c64.size >= k else np.inf
    last = np.float64(bits[-1:].view(np.float32)[0])
    L = np.float64(FLT_MAX) if np.isinf(last) else last
    with np.errstate(all="ignore"):
        rhs = np.float64(t64) * np.float64(1.0 + gamma(d))
        rhs = rhs + np.float64(delta(d))
    return bool(L > rhs)


def candidates_needed(d32_row, d64_row, k, d):
    """(k' at which the query is certified, widening rounds) along k' = first, 4 first, ... capped at n."""
    n = d32_row.shape[0]
    kp, rounds = first_candidates(n, k), 0
    while not certified(d32_row, d64_row, k, kp, d):
        kp, rounds = min(n, 4 * kp), rounds + 1
    return kp, rounds


def near_tie(d, seed=0, n=1500, nq=24, centres=8):
    """The near-tie input: rows = one of 8 Gaussian centres + 2e-6 N(0, 1), queries = a centre + 0.3 N(0, 1).  Thousands of rows
    lie within float32 rounding of one another as seen from a query, so the f32 order of the nearest rows is mostly wrong."""
    rng = np.random.default_rng(1000 + 17 * d + seed)
    cen = rng.standard_normal((centres, d))
    X = (cen[rng.integers(0, centres, n)] + 2e-6 * rng.standard_normal((n, d))).astype(np.float32)
    Q = (cen[rng.integers(0, centres, nq)] + 0.3 * rng.standard_normal((nq, d))).astype(np.float32)
    return X, Q
