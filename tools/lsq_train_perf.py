"""LSQ codebook update and training throughput on one MI355X (rq_dev_update_codebooks_lsq / rq_train_lsq, DESIGN.md
section 4.10) at the SIFT1M (d = 128, m = 8) and Deep1M (d = 96, m = 16) shapes, n = 1e6, h = 256, device-resident data.

    python tools/lsq_train_perf.py [--n 1000000] [--skip-cpu] [--out lsq_train_perf.json]

Per shape, after a warm-up call: the phases of one update from the host entry's phase clock (hipEvents between counts,
sort, b, assemble and solve; rq_last_lsq_timing), the device entry's whole update timed with torch events, the bytes/s of b
(m * n * d * 4 bytes of X read), the f64 FLOP/s of the solve ((mh)^3 / 3 + 2 (mh)^2 d), one train_lsq iteration at
ilsiter = 8 split into update and encode, the worst case of all n rows on one code, and the numpy restatement
(tests/lsq_update_oracle.py) as the CPU baseline."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _update_ms(X, codes, h, reps=3):
    """(best device-entry update in ms, phases of the best of reps host-entry calls)"""
    import torch
    from rayuela_jl_amd import device
    from rayuela_jl_amd.codebook_update import update_codebooks_u8
    from rayuela_jl_amd.LSQ import last_lsq_timing
    tX, tc = torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda()
    best, phases = None, None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        device.update_codebooks_lsq(tX, tc, h)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
        update_codebooks_u8(X, codes, h)
        ph = last_lsq_timing()
        if phases is None or sum(ph.values()) < sum(phases.values()):
            phases = ph
    return best, phases


def run(n, d, m, h, skip_cpu, seed=1):
    import torch
    from rayuela_jl_amd import device
    from rayuela_jl_amd.LSQ import train_lsq_u8, last_lsq_timing
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    mh = m * h
    out = {"n": n, "d": d, "m": m, "h": h}
    device.update_codebooks_lsq(torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda(), h)   # warm-up
    torch.cuda.synchronize()
    ms, ph = _update_ms(X, codes, h)
    out["update_ms"] = round(ms, 3)
    out["phases_ms"] = {k: round(v, 3) for k, v in ph.items() if k not in ("other_ms", "encode_ms")}
    out["A_ms"] = round(ph["count_ms"] + ph["assemble_ms"], 3)
    out["b_ms"] = round(ph["sort_ms"] + ph["b_ms"], 3)
    out["b_GBps"] = round(m * n * d * 4 / (ph["b_ms"] * 1e-3) / 1e9, 1)
    flops = mh ** 3 / 3 + 2 * mh ** 2 * d
    out["solve_ms"] = round(ph["solve_ms"], 3)
    out["solve_f64_TFLOPs"] = round(flops / (ph["solve_ms"] * 1e-3) / 1e12, 3)
    # worst case: every row on one code of codebook 0 (the longest sequential chain of b)
    one = codes.copy()
    one[:, 0] = 0
    ms1, ph1 = _update_ms(X, one, h)
    out["one_code_update_ms"] = round(ms1, 3)
    out["one_code_b_ms"] = round(ph1["b_ms"], 3)
    # one train_lsq iteration at ilsiter = 8 (icmiter = 4, npert = 4, randord): niter = 1 minus niter = 0
    tt = {}
    for niter in (0, 1):
        t = time.perf_counter()
        train_lsq_u8(X, codes, m, h, None, niter, 8, 4, True, 4, seed=1)
        tt[niter] = ((time.perf_counter() - t) * 1e3, last_lsq_timing())
    keys = ("count_ms", "sort_ms", "b_ms", "assemble_ms", "solve_ms")
    out["train_iteration_ms"] = round(tt[1][0] - tt[0][0], 1)
    out["train_iteration_update_ms"] = round(sum(tt[1][1][k] - tt[0][1][k] for k in keys), 3)
    out["train_iteration_encode_ms"] = round(tt[1][1]["encode_ms"] - tt[0][1]["encode_ms"], 3)
    out["train_iteration_other_ms"] = round(tt[1][1]["other_ms"] - tt[0][1]["other_ms"], 3)
    if not skip_cpu:
        import lsq_update_oracle as lo
        t = time.perf_counter()
        lo.update(X, codes, h)
        out["numpy_update_s"] = round(time.perf_counter() - t, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = []
    for shape, d, m in (("SIFT1M", 128, 8), ("Deep1M", 96, 16)):
        r = dict(shape=shape, **run(a.n, d, m, 256, a.skip_cpu))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
