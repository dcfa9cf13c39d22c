"""The ADC scan over 16-bit codes (rq_linscan_pq_wide, rq_dev_linscan_wide), restated from the committed oracle.

A plain helper module, imported by the tests (not a conftest).  The reference has no scan above 256 codewords per codebook
(deps/src/linscan_aqd.cpp:58,67 hard-wire 256 entries per table), so the contract is its arithmetic (:66-97) with a wider
table index, and this module builds it from the oracle ALONE:

  table      one oracle.adc_lut call per block of 256 codewords (the last block zero-padded and trimmed): an entry depends on
             its own codeword and the query only, so the blocks are the table
  distance   acc = acc + T[k][b_k] column by column in np.float32, from +0
  answer     the k smallest (dist, id) pairs by np.lexsort((ids, dists)), with the NaN and padding rules of
             tests/nonfinite_ref.py (contract): a NaN distance is never a neighbour, a short list ends in the padding pair

A code outside [0, h) makes its row "never a neighbour" of any query (the device entry point's rule; the host entry points
refuse such codes): its distance is NaN here.  tests/test_scan_wide_oracle.py pins all of this at h = 256 against
oracle.linscan_aqd_query on the golden scan fixtures, and the block-built table against a direct numpy evaluation above 256.

`certify` is the torch certificate of tests/exact_topk.py for int16 codes and tables of any width (bases too large for numpy).
"""
import numpy as np

import nonfinite_ref as nf


def tables(oracle, centers, queries):
    """T [nq][m][h] of centers [m][h][sub], block by block of 256 codewords through oracle.adc_lut."""
    centers = np.ascontiguousarray(centers, dtype=np.float32)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    m, h, sub = centers.shape
    nblk = (h + 255) // 256
    padded = np.zeros((m, nblk * 256, sub), dtype=np.float32)
    padded[:, :h] = centers
    T = np.empty((queries.shape[0], m, nblk * 256), dtype=np.float32)
    for b in range(nblk):
        blk = np.ascontiguousarray(padded[:, b * 256:(b + 1) * 256])
        for q in range(queries.shape[0]):
            T[q, :, b * 256:(b + 1) * 256] = oracle.adc_lut(blk, queries[q])
    return np.ascontiguousarray(T[:, :, :h])


def direct_tables(centers, queries):
    """The same table in plain numpy, one operation per rounding (tests/nonfinite_ref.py pq_tables, any h)."""
    m, h, _ = np.asarray(centers).shape
    return nf.pq_tables(queries, centers).reshape(-1, m, h)


def distances(table, codes):
    """dist [n] f32 of one query's table [m][h]; a row with a code outside [0, h) gets NaN (never a neighbour)."""
    m, h = table.shape
    c = np.asarray(codes).astype(np.int64)
    bad = ((c < 0) | (c >= h)).any(axis=1)
    c = np.clip(c, 0, h - 1)
    acc = np.zeros(c.shape[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(m):
            acc = acc + table[k][c[:, k]]
    acc[bad] = np.nan
    return acc


def scan_tables(T, codes, K, id_base=0, id_offset=0):
    """(distance bits [nq][K] u32, ids [nq][K] u32, packed keys [nq][K] u64) of tables T [nq][m][h]."""
    nq = T.shape[0]
    bits = np.empty((nq, K), dtype=np.uint32)
    ids = np.empty((nq, K), dtype=np.uint32)
    keys = np.empty((nq, K), dtype=np.uint64)
    for q in range(nq):
        bits[q], ids[q], keys[q] = nf.contract(distances(T[q], codes), K, id_base, id_offset)
    return bits, ids, keys


def scan(oracle, codes, centers, queries, K, id_base=0, id_offset=0):
    return scan_tables(tables(oracle, centers, queries), codes, K, id_base, id_offset)


def same(got_dists, got_ids, ref):
    return nf.same(got_dists, got_ids, ref[:2])


def first_difference(got_dists, got_ids, ref):
    return nf.first_difference(got_dists, got_ids, ref[:2])


def certify(dists, ids, k, lut, codes, n, chunk=1 << 22):
    """Assert on the device, for every query, that (dists, ids) [nq][k] are exactly the k smallest (dist, row) pairs of the rows
    codes [n][m] int16 (in range) under the finite tables lut [nq][m][h]: the conditions of tests/exact_topk.py -- ids in
    range and distinct, every returned distance equal bit for bit to the ordered f32 sum recomputed from the table, the list
    strictly ascending in (dist, row), and exactly k rows no larger than the last pair.  Returns the queries certified."""
    import torch
    dev = lut.device
    assert bool(torch.isfinite(lut).all())
    nq, m = lut.shape[0], lut.shape[1]
    d = dists.to(dev).to(torch.float32)
    r = ids.to(dev).long() & 0xFFFFFFFF
    assert d.shape == (nq, k) and r.shape == (nq, k)
    assert bool(((r >= 0) & (r < n)).all()), "range"
    rs = torch.sort(r, dim=1).values
    assert not bool((rs[:, 1:] == rs[:, :-1]).any()), "duplicate"
    got = torch.full((nq, k), float("nan"), dtype=torch.float32, device=dev)
    cnt = torch.zeros(nq, dtype=torch.int64, device=dev)
    dk, rk = d[:, k - 1].contiguous(), r[:, k - 1].contiguous()
    L = lut.permute(1, 2, 0).contiguous()                                     # [m][h][nq]
    qi = torch.arange(nq, device=dev)[:, None].expand(-1, k)
    for row0 in range(0, n, chunk):
        rows = min(chunk, n - row0)
        ct = codes[row0:row0 + rows].t().contiguous().long()                  # [m][rows]
        D = torch.index_select(L[0], 0, ct[0])                                # [rows][nq]
        for j in range(1, m):
            D = D + torch.index_select(L[j], 0, ct[j])
        rid = torch.arange(row0, row0 + rows, device=dev)
        cnt += (D < dk[None, :]).sum(0)
        cnt += ((D == dk[None, :]) & (rid[:, None] <= rk[None, :])).sum(0)
        mine = (r >= row0) & (r < row0 + rows)
        vals = D[(r - row0).clamp(0, rows - 1), qi]
        got = torch.where(mine, vals, got)
        del D, ct
    assert torch.equal(got.view(torch.int32), d.view(torch.int32)), "distance"
    asc = (d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (r[:, 1:] > r[:, :-1]))
    assert bool(asc.all()), "order"
    assert bool((cnt == k).all()), ("rank", cnt.tolist()[:8], k)
    return nq
