"""An exact top-k certificate of ADC scan answers in plain torch, for bases too large for the CPU oracle.

A plain helper module, imported by the tests (not a conftest).  It never calls into the HIP library: the table and the
distances are restated here in the reference's arithmetic, one torch op per rounding,

  lut[q, j, r] = sum over s = 0..sub-1, in sequence from 0, of (c - q) * (c - q)      deps/src/linscan_aqd.cpp:64-72
  dist(q, row) = lut[q, 0, code[0]] + lut[q, 1, code[1]] + ... + lut[q, m-1, code[m-1]]   (left to right, :85-87)

and `certify` proves, for every query, that a returned list is exactly the reference's answer (the k smallest pairs
(dist, row) of pair<float, UINT32>, :91-97), in one O(n) pass over the rows with no top-k of its own:

  1. "range":     every id is in range;  "duplicate": no id repeats;
  2. "distance":  every returned distance equals, bit for bit, the recomputed distance of its row;
  3. "order":     the list is strictly ascending in (dist, row), lexicographically;
  4. "rank":      exactly k rows r have (d_r, r) <= (d_k, r_k), the last returned pair.

1, 2 and 4 prove that the returned set is the top-k set (k distinct rows, each no larger than the k-th pair, and only k
such rows exist); 3 proves the order.  Non-finite tables are refused: NaN breaks the lexicographic order the certificate
counts in (tests/test_gpu_nonfinite.py covers them).
"""
import torch

REASONS = ("range", "duplicate", "distance", "order", "rank")
TEMP_BYTES = 6 << 30          # the element budget of one [rows x queries] chunk (about 11 bytes of temporaries each)
MAX_CHUNK_ROWS = 1 << 22


def adc_lut(centers, queries):
    """lut [nq][m][256] f32 of centers [m][256][sub] and queries [nq][m * sub]: the reference's sequential unfused sum."""
    m, h, sub = centers.shape
    nq = queries.shape[0]
    assert queries.shape[1] == m * sub, "the scan needs d == m * sub"
    c = centers.to(torch.float32)
    q = queries.to(device=c.device, dtype=torch.float32).reshape(nq, m, 1, sub)
    acc = torch.zeros((nq, m, h), dtype=torch.float32, device=c.device)
    for s in range(sub):
        diff = c[None, :, :, s] - q[:, :, :, s]
        sq = diff * diff
        acc = acc + sq
    return acc


def distances(lut, codes):
    """dist [nq][n] of the rows codes [n][m] (uint8) for the tables lut [nq][m][256], accumulated in code order."""
    m = lut.shape[1]
    cl = codes.to(lut.device).long()
    acc = torch.gather(lut[:, 0, :], 1, cl[:, 0][None, :].expand(lut.shape[0], -1))
    for j in range(1, m):
        acc = acc + torch.gather(lut[:, j, :], 1, cl[:, j][None, :].expand(lut.shape[0], -1))
    return acc


def _as_tensor(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device)
    import numpy as np
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.astype(np.int64)
    return torch.from_numpy(a).to(device)


def failures(dists, ids, k, lut, rows, n, id_base=0, id_offset=0, limit=8):
    """The queries whose list fails the certificate: [(query, reason, detail)], at most `limit`, in query order (the
    first failing condition of each query, in the order of REASONS).  Arguments as `certify`."""
    dev = lut.device
    if not bool(torch.isfinite(lut).all()):
        raise ValueError("certify: the table has a non-finite entry; the certificate covers finite tables only")
    nq, m = lut.shape[0], lut.shape[1]
    d = _as_tensor(dists, dev).to(torch.float32)
    r = (_as_tensor(ids, dev).long() & 0xFFFFFFFF) - (int(id_base) + int(id_offset))
    assert d.shape == (nq, k) and r.shape == (nq, k), (tuple(d.shape), tuple(r.shape), nq, k)
    assert 1 <= k <= n
    bad = {}                                        # query -> (reason, detail), the first reason found

    def note(mask, reason, detail):
        for q in torch.nonzero(mask).flatten().tolist():
            bad.setdefault(q, (reason, detail(q)))

    inr = (r >= 0) & (r < n)
    note(~inr.all(1), "range", lambda q: "id %d" % (int(r[q][~inr[q]][0]) + id_base + id_offset))
    rs = torch.sort(r, dim=1).values
    dup = (rs[:, 1:] == rs[:, :-1])
    note(dup.any(1), "duplicate", lambda q: "id %d" % (int(rs[q, 1:][dup[q]][0]) + id_base + id_offset))
    rc = r.clamp(0, n - 1)

    # one pass over the rows: the recomputed distances of the returned rows and the rank count of the k-th pair
    got = torch.full((nq, k), float("nan"), dtype=torch.float32, device=dev)
    cnt = torch.zeros(nq, dtype=torch.int64, device=dev)
    dk, rk = d[:, k - 1].contiguous(), r[:, k - 1].contiguous()
    qb = max(1, min(nq, (TEMP_BYTES // 12) // min(n, MAX_CHUNK_ROWS)))
    R = max(1, min(n, MAX_CHUNK_ROWS, (TEMP_BYTES // 12) // qb))
    luts = [lut[q0:q0 + qb].permute(1, 2, 0).contiguous() for q0 in range(0, nq, qb)]     # [m][256][queries]
    for row0 in range(0, n, R):
        cnt_rows = min(R, n - row0)
        codes = rows(row0, cnt_rows) if callable(rows) else rows[row0:row0 + cnt_rows]
        assert tuple(codes.shape) == (cnt_rows, m) and codes.dtype == torch.uint8, (tuple(codes.shape), codes.dtype)
        ct = codes.to(dev).t().contiguous().long()                                  # [m][rows]
        rid = torch.arange(row0, row0 + cnt_rows, device=dev)
        for b, q0 in enumerate(range(0, nq, qb)):
            L = luts[b]
            q1 = min(nq, q0 + qb)
            D = torch.index_select(L[0], 0, ct[0])                                   # [rows][queries]
            tmp = torch.empty_like(D)
            for j in range(1, m):
                torch.index_select(L[j], 0, ct[j], out=tmp)
                D.add_(tmp)
            del tmp
            cnt[q0:q1] += (D < dk[None, q0:q1]).sum(0)
            cnt[q0:q1] += ((D == dk[None, q0:q1]) & (rid[:, None] <= rk[None, q0:q1])).sum(0)
            mine = (rc[q0:q1] >= row0) & (rc[q0:q1] < row0 + cnt_rows)
            qi = torch.arange(q1 - q0, device=dev)[:, None].expand(-1, k)
            vals = D[(rc[q0:q1] - row0).clamp(0, cnt_rows - 1), qi]
            got[q0:q1] = torch.where(mine, vals, got[q0:q1])
            del D
    wrong = got.view(torch.int32) != d.view(torch.int32)
    note(wrong.any(1), "distance", lambda q: "position %d: %r returned, %r recomputed" % (
        int(torch.nonzero(wrong[q])[0]), float(d[q][wrong[q]][0]), float(got[q][wrong[q]][0])))
    asc = (d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (r[:, 1:] > r[:, :-1]))
    note(~asc.all(1), "order", lambda q: "positions %d, %d" % (int(torch.nonzero(~asc[q])[0]),
                                                                int(torch.nonzero(~asc[q])[0]) + 1))
    note(cnt != k, "rank", lambda q: "%d rows are <= the last pair (%r, id %d), not k = %d" % (
        int(cnt[q]), float(dk[q]), int(rk[q]) + id_base + id_offset, k))
    return [(q,) + bad[q] for q in sorted(bad)[:limit]]


def certify(dists, ids, k, lut, rows, n, id_base=0, id_offset=0):
    """Assert that (dists, ids) [nq][k] are, for every query, exactly the reference's top-k of the rows under the tables
    lut [nq][m][256] (`adc_lut`): ids = row + id_offset + id_base as uint32 (int32 / uint32 / int64 tensors or numpy).
    `rows` is the resident base [n][m] uint8, or a callable (row0, count) -> codes [count][m] that regenerates it chunk by
    chunk (on any device; the work runs on lut's device).  Returns the number of queries certified; the assertion message
    names the first failing queries and the reason."""
    bad = failures(dists, ids, k, lut, rows, n, id_base=id_base, id_offset=id_offset)
    assert not bad, "certify: %s" % "; ".join("q=%d %s (%s)" % b for b in bad)
    return lut.shape[0]
