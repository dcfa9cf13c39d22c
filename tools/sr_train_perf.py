"""LSQ++ noise and training throughput on one MI355X (rq_train_sr) at the SIFT1M (d = 128, m = 8)
and Deep1M (d = 96, m = 16) shapes, n = 1e6, h = 256.

    python tools/sr_train_perf.py [--n 1000000] [--niter-quality 4] [--out sr_train_perf.json]

Per shape, after a warm-up call, from the phase clocks of the host entries (hipEvents; rq_last_sr_timing,
rq_last_lsq_timing): the standard deviation of RX (one call) and one SR-C perturbation of it, with the perturbation's
bytes/s (8 n d bytes moved) as a fraction of the 6.29 TB/s float4 copy rate; one training iteration of SR-C, SR-D and plain
LSQ at ilsiter = 8 (icmiter = 4, npert = 4, randord) by phase, as the niter = 2 run minus the niter = 1 run; and the final
qerror of the three under one iteration budget and seed, from the same seeded random start codes on synthetic data."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BPS = 6.29e12          # the measured float4 copy rate


def _sr(X, codes, m, h, niter, method, clean=True, ilsiter=8):
    from rayuela_jl_amd.SR import last_sr_timing, train_sr_u8
    C, B, obj = train_sr_u8(X, codes, m, h, None, niter, ilsiter, 4, True, 4, method, 1, 0.5, clean, seed=1)
    return obj, last_sr_timing()


def _lsq(X, codes, m, h, niter, ilsiter=8):
    from rayuela_jl_amd.LSQ import last_lsq_timing, train_lsq_u8
    C, B, obj = train_lsq_u8(X, codes, m, h, None, niter, ilsiter, 4, True, 4, seed=1)
    t = last_lsq_timing()
    upd = sum(t[k] for k in ("count_ms", "sort_ms", "b_ms", "assemble_ms", "solve_ms"))
    return (C, B, obj), {"update_ms": upd, "encode_ms": t["encode_ms"], "other_ms": t["other_ms"]}


def run(shape, n, d, m, h, niter_quality):
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(n, d, seed=31) if shape == "SIFT1M" else synth.deep_like(n, d, seed=31)
    codes = np.random.default_rng(1).integers(0, h, size=(n, m)).astype(np.uint8)
    out = {"shape": shape, "n": n, "d": d, "m": m, "h": h}
    _sr(X[:20000], codes[:20000], m, h, 1, "SR_C", ilsiter=1)          # warm-up
    for method in ("SR_C", "SR_D"):
        _, t1 = _sr(X, codes, m, h, 1, method)
        _, t2 = _sr(X, codes, m, h, 2, method)
        if method == "SR_C":
            out["std_ms"] = round(t1["std_ms"], 3)                      # one pass pair over RX
            per = t1["perturb_ms"] / 2                                  # calls 0 and 1
            out["perturb_ms"] = round(per, 3)
            out["perturb_TBps"] = round(8.0 * n * d / (per * 1e-3) / 1e12, 3)
            out["perturb_fraction_of_hbm_copy"] = round(8.0 * n * d / (per * 1e-3) / HBM_COPY_BPS, 3)
        else:
            out["sr_d_std_ms"] = round(t1["std_ms"] / 2, 4)             # of the m h codewords, per call
            out["sr_d_perturb_ms"] = round(t1["perturb_ms"] / 2, 4)
        it = {k: round(t2[k] - t1[k], 3) for k in t1 if k != "other_ms"}
        it["total_ms"] = round(sum(it.values()), 3)
        out["%s_iteration_ms" % method.lower()] = it
    _, l1 = _lsq(X, codes, m, h, 1)
    _, l2 = _lsq(X, codes, m, h, 2)
    it = {k: round(l2[k] - l1[k], 3) for k in ("update_ms", "encode_ms")}
    it["total_ms"] = round(sum(it.values()), 3)
    out["lsq_iteration_ms"] = it
    # quality under one budget: niter iterations at ilsiter = 8, the same start codes and seed
    q = {}
    for method in ("SR_C", "SR_D"):
        obj, _ = _sr(X, codes, m, h, niter_quality, method)
        q[method] = float(obj[-1])
    (C, B, obj), _ = _lsq(X, codes, m, h, niter_quality)
    from rayuela_jl_amd.codebook_update import update_codebooks_u8
    q["LSQ"] = rq.qerror(X, B.astype(np.int16) + 1, list(C))
    # train_sr_cuda ends on a codebook update of the final codes, train_lsq on an encode: the same refit for LSQ
    q["LSQ_refit"] = rq.qerror(X, B.astype(np.int16) + 1, list(update_codebooks_u8(X, B, h)))
    out["final_qerror_niter_%d" % niter_quality] = {k: float("%.6e" % v) for k, v in q.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--niter-quality", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = []
    for shape, d, m in (("SIFT1M", 128, 8), ("Deep1M", 96, 16)):
        r = run(shape, a.n, d, m, 256, a.niter_quality)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
