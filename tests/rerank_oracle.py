"""The contract of the re-ranking entries (include/rayuela_hip.h, "exact re-ranking of search candidates"), restated in numpy.

A plain helper module, imported by the tests (not a conftest).  It never calls into the HIP library.  Built from the two
restatements the contract names: knn_oracle.d32 (the distance, one numpy operation per rounding) and nonfinite_ref (the ordered
distance bits of a packed key, the padding pair).  Per query, candidate c has row r = (c - id_base - id_offset) mod 2^32 and counts
iff r < n; the answer is the k smallest (D32, r) pairs -- a pair per candidate, so an id given twice appears twice -- with a NaN
distance never a neighbour, -0 read as +0, and the padding pair behind a short list.

The planner's arithmetic (rq_rerank_plan: csrc/rq_rerank.hip, with the scratch of the select chain from csrc/rq_bulk.hip) is
restated too."""
import numpy as np

import knn_oracle as ko
import nonfinite_ref as nf

M32 = 0xFFFFFFFF
LDS_K = 4096                                 # candidates per query that one workgroup sorts in LDS
BULK_USABLE = (2 << 30) // 5 * 4             # bulk_usable(): the usable part of BULK_SCRATCH_BYTES
BK_MAX_NB = 16384
BULKQ_BYTES = 72                             # sizeof(BulkQ): 3 x 8 + 4 x 4 + 8 x 4


def rows_of(cand, id_offset=0, id_base=0):
    """r [..] int64 in [0, 2^32) of candidate ids of any shape."""
    c = np.asarray(cand).astype(np.int64) & M32
    return (c - id_base - id_offset) % (1 << 32)


def rerank_d(D32, cand, kc, k, id_offset=0, id_base=0):
    """(distance bits [nq][k] u32, ids [nq][k] u32) from the distance matrix D32 [nq][n] (knn_oracle.d32)."""
    nq, n = D32.shape
    assert n + id_offset <= M32 and 1 <= k <= kc <= cand.shape[1]
    bits = np.full((nq, k), nf.PAD_BITS, dtype=np.uint32)
    ids = np.full((nq, k), (M32 + id_base) & M32, dtype=np.uint32)
    for q in range(nq):
        r = rows_of(cand[q, :kc], id_offset, id_base)        # what lies behind kc is never read
        r = r[r < n]
        with np.errstate(all="ignore"):
            dv = D32[q, r] + np.float32(0)                    # -0 -> +0
        keep = ~np.isnan(dv)
        r, dv = r[keep], dv[keep]
        keys = np.sort((nf.ordered_bits(dv).astype(np.uint64) << np.uint64(32)) | r.astype(np.uint64))[:k]
        m = keys.size
        ob = (keys >> np.uint64(32)).astype(np.uint32)
        bits[q, :m] = np.where(ob >> 31 != 0, ob ^ np.uint32(0x80000000), ~ob)      # nonfinite_ref.ordered_bits, inverted
        ids[q, :m] = (((keys & np.uint64(M32)).astype(np.int64) + id_offset + id_base) & M32).astype(np.uint32)
    return bits, ids


def rerank(X, Q, cand, kc, k, id_offset=0, id_base=0):
    return rerank_d(ko.d32(X, Q), cand, kc, k, id_offset, id_base)


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def _align256(b):
    return (b + 255) & ~255


def sel_bytes_per_query(k):
    tiles = (k + 4095) // 4096
    return 2 * k * 8 + tiles * 256 * 4 + 256 * 4 + BULKQ_BYTES + 4 * 256


def scratch_bytes(nb, kc, k, lds_k=LDS_K):
    ld = (kc + 3) & ~3
    chain = kc > lds_k
    return _align256(nb * 4) + _align256(nb * ld * 8) + (nb * sel_bytes_per_query(k) + 6 * 256 if chain else 0)


def plan(nq, kc, k, lds_k=LDS_K, batch_queries=0):
    """What rq_rerank_plan reports: the most queries per batch whose keys (and chain scratch) fit the bulk budget."""
    hi = min(max(nq, 1), BK_MAX_NB)
    if batch_queries > 0:
        hi = min(hi, batch_queries)
    lo = 0                                   # the bytes grow with nb: bisect for the largest batch that fits
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if scratch_bytes(mid, kc, k, lds_k) <= BULK_USABLE:
            lo = mid
        else:
            hi = mid - 1
    batch = lo
    return {"batch": batch, "scratch_bytes": scratch_bytes(batch, kc, k, lds_k) if batch else 0, "chain": int(kc > lds_k),
            "keys_per_query": (kc + 3) & ~3, "forced": int(batch_queries > 0)}
