"""LSQ encoding throughput on one MI355X (rq_encode_icm): milliseconds per ILS iteration at the
SIFT1M (d = 128, m = 8) and Deep1M (d = 96, m = 16) shapes, n = 1e6, h = 256, icmiter = 4, npert = 4, randord; the
unaries separately; the bytes the conditioning steps gather per ICM sweep and the effective gather rate.

    python tools/icm_perf.py [--n 1000000] [--out icm_perf.json]

Times come from the host entry's own clocks (rq_last_icm_timing): total minus the unaries minus the transfers is the ILS
kernel; ms per ILS iteration is the slope between ilsiter = 8 and 32 (both also reported whole)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(n, d, m, h, its, seed=1):
    import rayuela_jl_amd as rq
    from rayuela_jl_amd.LSQ import encode_icm_u8, last_timing
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.3).astype(np.float32)
    B0 = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    encode_icm_u8(X[:4096], B0[:4096], C, 1, 1, 4, True)        # warm-up: code objects, scratch
    out = {"n": n, "d": d, "m": m, "h": h, "icmiter": 4, "npert": 4, "randord": True}
    base = None
    for it in [0] + its:
        best = None
        for _ in range(2):
            t = time.perf_counter()
            encode_icm_u8(X, B0, C, it, 4, 4, True)
            wall = (time.perf_counter() - t) * 1e3
            tm = last_timing()
            if best is None or tm["total_ms"] < best["total_ms"]:
                best = dict(tm, wall_ms=wall)
        if it == 0:
            base = best
            out["unary_ms"] = round(best["unary_ms"], 3)
            out["ilsiter0_total_ms"] = round(best["total_ms"], 3)
        else:
            out["ilsiter%d_ms" % it] = round(best["total_ms"] - base["total_ms"], 3)
    a, b = its[0], its[-1]
    per = (out["ilsiter%d_ms" % b] - out["ilsiter%d_ms" % a]) / (b - a)
    out["ms_per_ils_iteration"] = round(per, 4)
    out["gather_bytes_per_sweep"] = int(n * m * (m - 1) * h * 4)
    sweep_ms = per / 4.0
    out["gather_TBps"] = round(out["gather_bytes_per_sweep"] / (sweep_ms * 1e-3) / 1e12, 3)
    out["guide_row_gather_TBps"] = [8.6, 18.8]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = [dict(shape="SIFT1M", **run(a.n, 128, 8, 256, [8, 32])),
           dict(shape="Deep1M", **run(a.n, 96, 16, 256, [8, 32]))]
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
