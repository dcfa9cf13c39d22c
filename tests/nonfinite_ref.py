"""The scans' contract on non-finite inputs (include/rayuela_hip.h, "Non-finite inputs"), restated in plain numpy.

A plain helper module, imported by the tests (not a conftest).  It never calls into the HIP library or the C oracle.
Every (query, row) distance is evaluated in f32, one numpy operation per rounding, in the reference's order

  LSQ table   acc = acc - (2 * q[k]) * c[k]   over k = 0..d-1, from +0     deps/src/linscan_aqd_pairwise_byte.cpp
  CQ  table   acc = acc + (q[k] - c[k]) * (q[k] - c[k])                    (the same file, the cq entry point)
  PQ  table   acc = acc + (q[s] - c[s]) * (q[s] - c[s])  over the sub-space    deps/src/linscan_aqd.cpp:66-74
  row         acc = acc + T[h * k + b_k]      over k = 0..m-1, from +0, then + dbnorms[row] (LSQ)

and the contract is applied per query: rows with a NaN distance are dropped, -0 becomes +0, the rest is sorted by
(dist, id), and a list shorter than K ends in the padding pair (distance bits 0x7FFFFFFF, id 0xFFFFFFFF + id_base
mod 2^32; as a packed key: KEY_MAX).  On inputs without a NaN distance this is the reference's answer, which
tests/test_nonfinite_ref.py pins bit for bit against the C oracle and the compiled reference; with NaN distances the
reference's own answer is unspecified (its pair comparison is no strict weak order) and this module IS the definition.
"""
import numpy as np

PAD_BITS = 0x7FFFFFFF
KEY_MAX = 0xFFFFFFFFFFFFFFFF
NAN_POS = 0x7FC00000          # quiet NaN, sign bit clear (np.nan)
NAN_NEG = 0xFFC00000          # quiet NaN, sign bit set (what x86 gives for Inf - Inf)


def f32_from_bits(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def put_bits(a, index, bits):
    """a[index] = the f32 with exactly these bits (an assignment of a float NaN may lose its sign)."""
    a.view(np.uint32)[index] = np.uint32(bits)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def lsq_tables(queries, codebooks):
    """T [nq][m*h]: -2 <q, c> accumulated as acc = acc - (2 * q[k]) * c[k]."""
    q, c = _f32(queries), _f32(codebooks)
    acc = np.zeros((q.shape[0], c.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(q.shape[1]):
            two_q = np.float32(2) * q[:, k]
            prod = two_q[:, None] * c[None, :, k]
            acc = acc - prod
    return acc


def cq_tables(queries, codebooks):
    """T [nq][m*h]: |q - c|^2 accumulated as acc = acc + (q[k] - c[k]) * (q[k] - c[k])."""
    q, c = _f32(queries), _f32(codebooks)
    acc = np.zeros((q.shape[0], c.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(q.shape[1]):
            diff = q[:, k][:, None] - c[None, :, k]
            sq = diff * diff
            acc = acc + sq
    return acc


def pq_tables(queries, centers):
    """T [nq][m*256] of centers [m][256][sub]: the squared distance inside each sub-space, coordinate by coordinate."""
    q, c = _f32(queries), _f32(centers)
    m, h, sub = c.shape
    assert q.shape[1] == m * sub
    qs = q.reshape(q.shape[0], m, 1, sub)
    acc = np.zeros((q.shape[0], m, h), dtype=np.float32)
    with np.errstate(all="ignore"):
        for s in range(sub):
            diff = qs[:, :, :, s] - c[None, :, :, s]
            sq = diff * diff
            acc = acc + sq
    return acc.reshape(q.shape[0], m * h)


def row_distances(table, codes, dbnorms=None):
    """dist [n] of one query's table [m*h]: the entries in code order from +0, then the row's norm."""
    n, m = codes.shape
    h = table.shape[0] // m
    acc = np.zeros(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(m):
            acc = acc + table[h * k + codes[:, k].astype(np.int64)]
        if dbnorms is not None:
            acc = acc + _f32(dbnorms)
    return acc


def ordered_bits(d):
    """uint32 whose unsigned order is the float order (the high word of a packed key)."""
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def contract(dist, K, id_base=0, id_offset=0):
    """One query: (distance bits [K] u32, ids [K] u32, packed keys [K] u64) of the row distances dist [n]."""
    with np.errstate(all="ignore"):
        dv = _f32(dist) + np.float32(0)                      # -0 -> +0
    rows = np.flatnonzero(~np.isnan(dv))                     # a NaN distance is never a neighbour
    if rows.size > K:                                        # (only to keep the sort short: rows beyond the K-th distance)
        kth = np.partition(dv[rows], K - 1)[K - 1]
        rows = rows[dv[rows] <= kth]
    rows = rows[np.lexsort((rows, dv[rows]))][:K]
    bits = np.full(K, PAD_BITS, dtype=np.uint32)
    ids = np.full(K, (0xFFFFFFFF + id_base) & 0xFFFFFFFF, dtype=np.uint32)
    keys = np.full(K, KEY_MAX, dtype=np.uint64)
    gid = (rows.astype(np.uint64) + np.uint64(id_offset)) & np.uint64(0xFFFFFFFF)
    bits[:rows.size] = dv[rows].view(np.uint32)
    ids[:rows.size] = ((gid + np.uint64(id_base)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    keys[:rows.size] = (ordered_bits(dv[rows]).astype(np.uint64) << np.uint64(32)) | gid      # keys stay zero-based
    return bits, ids, keys


def scan(kind, codes, books, queries, K, dbnorms=None, id_base=0, id_offset=0, want_keys=False):
    """The contract's answer of a whole call.  kind "lsq" / "cq": books = codebooks [m*h][d]; "pq": books = centers
    [m][256][sub].  Returns (bits [nq][K] u32, ids [nq][K] u32) and, with want_keys, the packed keys [nq][K] u64."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if kind == "lsq":
        assert dbnorms is not None
        T = lsq_tables(queries, books)
    elif kind == "cq":
        assert dbnorms is None
        T = cq_tables(queries, books)
    else:
        assert kind == "pq" and dbnorms is None
        T = pq_tables(queries, books)
    nq = T.shape[0]
    bits = np.empty((nq, K), dtype=np.uint32)
    ids = np.empty((nq, K), dtype=np.uint32)
    keys = np.empty((nq, K), dtype=np.uint64)
    for q in range(nq):
        bits[q], ids[q], keys[q] = contract(row_distances(T[q], codes, dbnorms), K, id_base, id_offset)
    return (bits, ids, keys) if want_keys else (bits, ids)


def same(got_dists, got_ids, ref):
    """Do the returned (dists f32, ids of any 32-bit integer type) equal the contract's (bits, ids), bit for bit?"""
    gd = np.ascontiguousarray(got_dists).view(np.uint32)
    gi = np.ascontiguousarray(got_ids).view(np.uint32)
    return gd.shape == ref[0].shape and np.array_equal(gd, ref[0]) and np.array_equal(gi, ref[1])


def first_difference(got_dists, got_ids, ref):
    """(query, rank, got (bits, id), expected (bits, id)) of the first mismatch, for assertion messages; None if equal."""
    gd = np.ascontiguousarray(got_dists).view(np.uint32)
    gi = np.ascontiguousarray(got_ids).view(np.uint32)
    bad = np.argwhere((gd != ref[0]) | (gi != ref[1]))
    if bad.size == 0:
        return None
    q, r = (int(x) for x in bad[0])
    return (q, r, (hex(int(gd[q, r])), int(gi[q, r])), (hex(int(ref[0][q, r])), int(ref[1][q, r])), int(bad.shape[0]))
