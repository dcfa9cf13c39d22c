#!/usr/bin/env python3
"""Speed of the bulk top-k path (k > RQ_MAX_K, rq_bulk.hip) on one MI355X: n = 1e6 rows, m = 8, nq in {100, 1000},
k in {65536 (candidate-buffer scan), 65537, 1e5, 5e5, 1e6}.  Per case: ms per call (device pointers, resident base),
queries per second, and the bytes each phase moves against the 6.3 TB/s achievable HBM rate:

  keys     the distance kernel writes one 8-byte key per (row, query)           nq * n * 8
  select   every radix pass re-reads the keys of the queries still open           sum over queries of passes * n * 8
  compact  one more read of the keys, the k kept keys written                     nq * (n + k) * 8
  sort     per 8-bit window: tile histogram read + stable scatter read / write     sum over queries of windows * 24 * k
  unpack   sorted keys read, dists + ids written                                   nq * k * 16

Passes and windows are exact per query, from the answer itself: the select stops at the first byte (from the top) where the
k-th and the (k+1)-th smallest keys differ, the sort runs one window per 8-bit run of the bits that vary among the k keys.
On a subset the compiled reference (oracle/_ref, CPU) is timed too.
usage: python tools/bulk_topk_perf.py [--iters N] [--ref-nq Q] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rayuela_jl_amd import _lib, device as rqd   # noqa: E402

HBM = 6.3e12
KS = [65536, 65537, 100_000, 500_000, 1_000_000]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def passes_and_windows(keys_k1, k, n):
    """keys_k1 [nq][k + 1] (or [nq][k] when k == n) sorted uint64 keys as int64 -> (passes, windows) per query."""
    kk = keys_k1[:, :k]
    if k < n:
        diff = (keys_k1[:, k - 1] ^ keys_k1[:, k])
        # first differing byte from the top: 64 - bit_length(diff), in bytes
        top = torch.zeros_like(diff)
        for b in range(63, -1, -1):
            top = torch.where((top == 0) & (((diff >> b) & 1) == 1), torch.full_like(diff, 64 - b), top)
        passes = ((top - 1) // 8 + 1).clamp(1, 8)
    else:
        passes = torch.ones(kk.shape[0], dtype=torch.int64, device=kk.device)
    orv = torch.zeros(kk.shape[0], dtype=torch.int64, device=kk.device)
    andv = torch.full((kk.shape[0],), -1, dtype=torch.int64, device=kk.device)
    for c in range(0, k, 1 << 20):
        part = kk[:, c:c + (1 << 20)]
        orv |= _red(part, torch.bitwise_or)
        andv &= _red(part, torch.bitwise_and)
    var = (orv & ~andv).cpu().numpy().view(np.uint64)
    wins = []
    for v in var:
        v, w = int(v), 0
        while v and w < 8:
            sh = (v & -v).bit_length() - 1
            w += 1
            v = 0 if sh + 8 >= 64 else (v >> (sh + 8)) << (sh + 8)
        wins.append(w)
    return passes.cpu().numpy(), np.asarray(wins)


def _red(t, op):
    while t.shape[1] > 1:
        h = t.shape[1] // 2
        r = op(t[:, :h], t[:, h:2 * h])
        t = torch.cat([r, t[:, 2 * h:]], 1) if t.shape[1] % 2 else r
    return t[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--ref-nq", type=int, default=4)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n, m, sub = 1_000_000, 8, 16
    rng = np.random.default_rng(1)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    ct = torch.from_numpy(centers).cuda()
    codes = rqd.synth_codes(n, m, seed=7)
    print("lib", (_lib.lib().rq_version() or b"").decode())
    rows = []
    for nq in (100, 1000):
        Q = torch.from_numpy(rng.standard_normal((nq, m * sub)).astype(np.float32)).cuda()
        for k in KS:
            out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                   torch.empty((nq, k), dtype=torch.int32, device="cuda"))
            ms = timed(lambda: rqd.linscan(codes, ct, Q, k, out=out), a.iters)
            kern = (_lib.lib().rq_last_scan_kernel() or b"").decode()
            plan = _lib.scan_plan(n, nq, m, m * sub, k)
            row = dict(nq=nq, k=k, ms=round(ms, 3), qps=round(nq / ms * 1e3, 1), kernel=kern, bulk=plan["bulk"],
                       batch=plan["cap"] if plan["bulk"] else None)
            del out
            if plan["bulk"]:
                kk = min(k + 1, n)
                keys = rqd.linscan(codes, ct, Q, kk, want_keys=True)
                P, W = passes_and_windows(keys, k, n)
                del keys
                ph = dict(keys=nq * n * 8, select=int(P.sum()) * n * 8, compact=nq * (n + k) * 8,
                          sort=int(W.sum()) * 24 * k, unpack=nq * k * 16)
                tot = sum(ph.values())
                row.update(passes_mean=round(float(P.mean()), 2), windows_mean=round(float(W.mean()), 2),
                           bytes={p: b for p, b in ph.items()}, frac={p: round(b / tot, 3) for p, b in ph.items()},
                           hbm_ms={p: round(b / HBM * 1e3, 3) for p, b in ph.items()},
                           hbm_floor_ms=round(tot / HBM * 1e3, 3), of_hbm=round(tot / HBM * 1e3 / ms, 3))
            torch.cuda.empty_cache()
            rows.append(row)
            print(json.dumps(row), flush=True)
    # the compiled reference on the CPU, a few queries (its time grows linearly with them)
    try:
        from oracle import oracle
        cnp = codes.cpu().numpy()
        Qn = rng.standard_normal((a.ref_nq, m * sub)).astype(np.float32)
        for k in (65537, 100_000):
            t0 = time.time()
            oracle.ref_linscan_aqd_query(cnp, centers, Qn, k)
            s = time.time() - t0
            row = dict(ref_cpu=True, nq=a.ref_nq, k=k, ms=round(s * 1e3, 1), qps=round(a.ref_nq / s, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    except Exception as e:          # the reference is optional on this tool's path
        print("reference not timed: %s" % e)
    step = {r["nq"]: r["ms"] for r in rows if not r.get("ref_cpu") and r["k"] == 65536}
    for r in rows:
        if not r.get("ref_cpu") and r["k"] == 65537:
            print("step 65536 -> 65537 at nq=%d: %.3f -> %.3f ms (x%.2f)" % (r["nq"], step[r["nq"]], r["ms"],
                                                                            r["ms"] / step[r["nq"]]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
