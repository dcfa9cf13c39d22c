"""The additive-quantizer scan and the database norms over 16-bit codes (rq_linscan_lsq_wide, rq_linscan_cq_wide,
rq_dev_linscan_aq_wide, the *_norms_wide entries), restated from the committed restatements.

A plain helper module, imported by the tests (not a conftest).  The reference's arithmetic takes h at run time
(deps/src/linscan_aqd_pairwise_byte.cpp:42-49, :70-74, :124-131: tentry[h*k + code[k]]); only `unsigned char *codes` stops it at
256.  So the contract is tests/nonfinite_ref.py as it stands -- lsq_tables, cq_tables, row_distances, contract take any table
width -- with int16 codes and the rule of tests/scan_wide_oracle.py for a code outside [0, h): the row's distance is NaN, never a
neighbour.  tests/test_aq_wide_oracle.py pins this module against the C oracle and the compiled reference at h <= 256.

  tables(lsq, codebooks, queries)   T [nq][m*h] of codebooks [m*h][d]
  distances(T_q, codes, dbnorms)    [n] f32 of one query
  scan(...)                         (distance bits, ids, packed keys) [nq][K]
  quantize(norms, cb)               norms_oracle.quantize for tables of more than 256 entries: int16 codes
norms_oracle.aq_norms serves int16 codes as it is.
"""
import numpy as np

import nonfinite_ref as nf


def tables(lsq, codebooks, queries):
    cb = np.ascontiguousarray(codebooks, dtype=np.float32)
    cb = cb.reshape(-1, cb.shape[-1])
    return nf.lsq_tables(queries, cb) if lsq else nf.cq_tables(queries, cb)


def distances(table, codes, dbnorms=None):
    """dist [n] f32 of one query's table [m*h]; a row with a code outside [0, h) gets NaN (never a neighbour)."""
    c = np.asarray(codes).astype(np.int64)
    h = table.shape[0] // c.shape[1]
    bad = ((c < 0) | (c >= h)).any(axis=1)
    dist = nf.row_distances(table, np.clip(c, 0, h - 1), dbnorms)
    dist[bad] = np.nan
    return dist


def scan_tables(T, codes, K, dbnorms=None, id_base=0, id_offset=0):
    nq = T.shape[0]
    bits = np.empty((nq, K), dtype=np.uint32)
    ids = np.empty((nq, K), dtype=np.uint32)
    keys = np.empty((nq, K), dtype=np.uint64)
    for q in range(nq):
        bits[q], ids[q], keys[q] = nf.contract(distances(T[q], codes, dbnorms), K, id_base, id_offset)
    return bits, ids, keys


def scan(codes, codebooks, queries, K, dbnorms=None, id_base=0, id_offset=0):
    """LSQ when dbnorms is given, else CQ: (bits [nq][K] u32, ids [nq][K] u32, keys [nq][K] u64)."""
    return scan_tables(tables(dbnorms is not None, codebooks, queries), codes, K, dbnorms, id_base, id_offset)


def same(got_dists, got_ids, ref):
    return nf.same(got_dists, got_ids, ref[:2])


def quantize(norms, cb, chunk=512):
    """[n] f32, cb [hn] f32 (unsorted, hn <= 32767) -> zero-based int16 codes: the first index of the smallest
    fl(fl(norm - cb[j])^2), np.argmin's first minimum."""
    norms = np.asarray(norms, dtype=np.float32)
    cb = np.asarray(cb, dtype=np.float32)
    out = np.zeros(norms.shape[0], dtype=np.int16)
    with np.errstate(all="ignore"):
        for i0 in range(0, norms.shape[0], chunk):
            df = norms[i0:i0 + chunk, None] - cb[None, :]
            out[i0:i0 + chunk] = np.argmin(df * df, axis=1).astype(np.int16)
    return out


def case(n, m, h, d, nq, seed, integer=False):
    """Seeded (codes [n][m] int16 with 0 and h - 1 present, codebooks [m][h][d], queries [nq][d], dbnorms [n] of mixed sign)."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    codes[0, 0] = 0
    codes[-1, -1] = h - 1
    if integer:
        C = rng.integers(-7, 8, (m, h, d)).astype(np.float32)
        q = rng.integers(-7, 8, (nq, d)).astype(np.float32)
    else:
        C = rng.standard_normal((m, h, d)).astype(np.float32)
        q = rng.standard_normal((nq, d)).astype(np.float32)
    nrm = (rng.standard_normal(n) * np.float32(3) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
    return codes, C, q, nrm
