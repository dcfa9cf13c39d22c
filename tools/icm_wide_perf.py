"""LSQ encoding over 16-bit codes on one MI355X (rq_encode_icm_wide): milliseconds per ILS iteration, the
bytes the conditioning steps gather per ICM sweep and the effective gather rate, at n = 1e5, d = 128, icmiter = 4, npert = 4,
randord, for (m, h) = (8, 256) through the byte entry and through the wide one, (8, 1024), (16, 1024) and (4, 4096).

    python tools/icm_wide_perf.py [--n 100000] [--out profiles/icm_wide_perf.json]

Times come from the host entries' own clocks (rq_last_icm_timing), the best of three calls each.  A call with ilsiter > 0 also
builds the tables and the unaries, which the zero-iteration call (a veccost pass) does not: `ilsiterK_ms` is the total minus the
zero-iteration call, and ms per ILS iteration is the slope between the two iteration counts, which holds the kernel alone."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ICMITER, NPERT = 4, 4


def run(n, d, m, h, its, wide, seed=1):
    from rayuela_jl_amd.LSQ import encode_icm_u16, encode_icm_u8, last_timing
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.3).astype(np.float32)
    B0 = rng.integers(0, h, size=(n, m)).astype(np.int16 if wide else np.uint8)
    enc = encode_icm_u16 if wide else encode_icm_u8
    enc(X[:4096], B0[:4096], C, 1, 1, NPERT, True)        # warm-up: code objects, scratch
    out = {"entry": "rq_encode_icm_wide" if wide else "rq_encode_icm", "n": n, "d": d, "m": m, "h": h, "icmiter": ICMITER,
           "npert": NPERT, "randord": True}
    base = None
    for it in [0] + its:
        best = None
        for _ in range(3):
            enc(X, B0, C, it, ICMITER, NPERT, True)
            tm = last_timing()
            if best is None or tm["total_ms"] < best["total_ms"]:
                best = tm
        if it == 0:
            base = best
            out["ilsiter0_total_ms"] = round(best["total_ms"], 3)
        else:
            out["unary_ms"] = round(best["unary_ms"], 3)
            out["ilsiter%d_ms" % it] = round(best["total_ms"] - base["total_ms"], 3)
    a, b = its[0], its[-1]
    per = (out["ilsiter%d_ms" % b] - out["ilsiter%d_ms" % a]) / (b - a)
    out["ms_per_ils_iteration"] = round(per, 4)
    out["tables_and_unaries_ms"] = round(out["ilsiter%d_ms" % a] - a * per, 3)
    out["gather_bytes_per_sweep"] = int(n * m * (m - 1) * h * 4)
    out["unary_bytes_per_sweep"] = int(n * m * h * 4)
    out["gather_TBps"] = round(out["gather_bytes_per_sweep"] / (per / ICMITER * 1e-3) / 1e12, 3)
    out["table_MB"] = round(m * m * h * 64 * ((h + 63) // 64) * 4 / 1e6, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    its = [4, 12]
    res = []
    for m, h, wide in [(8, 256, False), (8, 256, True), (8, 1024, True), (16, 1024, True), (4, 4096, True)]:
        res.append(run(a.n, 128, m, h, its, wide))
        print(json.dumps(res[-1]), flush=True)
    doc = {"shapes": res,
           "wide_over_byte_at_h256": round(res[1]["ms_per_ils_iteration"] / res[0]["ms_per_ils_iteration"], 3),
           "yardsticks_TBps": {"byte_kernel_same_run_m8_h256": res[0]["gather_TBps"], "byte_kernel_project_figure": 10.3,
                               "guide_register_gather_beyond_infinity_cache": [5.5, 5.8]}}
    print(json.dumps({k: v for k, v in doc.items() if k != "shapes"}))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
