"""Database norms of additive-quantizer search on one MI355X (rq_dev_aq_norms / rq_dev_quantize_norms / rq_get_norms_codebook,
DESIGN.md section 4.14) at the SIFT1M (d = 128, m = 8) and Deep1M (d = 96, m = 16) shapes, n = 1e6, h = 256.

    python tools/norms_perf.py [--n 1000000] [--skip-host] [--out profiles/norms_perf.json]

Per shape, after a warm-up call: the norms kernel and the quantise kernel on resident tensors timed with device events (best of
5), the gather rate n * m * d * 4 bytes over the norms kernel's time, the whole of rq_get_norms_codebook from host pointers
(wall clock, with the k-means iterations it ran), and -- on the same box -- the two numpy helpers of experiments.py
(_norms_codebook, _quantize_norms) on the same inputs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _best(fn, reps=5):
    import torch
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def _wall(fn, reps=2):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def run(n, d, m, h, skip_host, seed=1):
    import torch
    from rayuela_jl_amd import _lib, experiments, utils
    L = _lib.lib()
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((m, h, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    tc, tC = torch.from_numpy(codes).cuda(), torch.from_numpy(C).cuda()
    tn = torch.empty(n, dtype=torch.float32, device="cuda")
    tq = torch.empty(n, dtype=torch.uint8, device="cuda")
    td = torch.empty(n, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def norms():
        _lib.check(L.rq_dev_aq_norms(tn.data_ptr(), tc.data_ptr(), tC.data_ptr(), n, d, m, h, s))

    norms()
    torch.cuda.synchronize()
    cb = torch.quantile(tn[:100000], torch.linspace(0, 1, 256, device="cuda")).contiguous()

    def quant():
        _lib.check(L.rq_dev_quantize_norms(tq.data_ptr(), td.data_ptr(), tn.data_ptr(), cb.data_ptr(), n, 256, s))

    quant()
    out = {"n": n, "d": d, "m": m, "h": h}
    out["norms_ms"] = round(_best(norms), 4)
    out["gather_bytes"] = n * m * d * 4
    out["gather_TB_per_s"] = round(out["gather_bytes"] / (out["norms_ms"] * 1e-3) / 1e12, 3)
    out["quantize_ms"] = round(_best(quant), 4)
    B1 = codes.astype(np.int16) + 1
    Cl = list(C)
    for niter in (25, 100):
        utils.get_norms_codebook(B1, Cl, niter=niter, seed=seed)               # warm-up
        ms = _wall(lambda: utils.get_norms_codebook(B1, Cl, niter=niter, seed=seed))
        out["get_norms_codebook_niter%d_ms" % niter] = round(ms, 2)
        out["get_norms_codebook_niter%d_iterations" % niter] = int(_lib.train_profile()["iterations"])
    _, cbn = utils.get_norms_codebook(B1, Cl, niter=25, seed=seed)
    out["quantize_norms_host_pointers_ms"] = round(_wall(lambda: utils.quantize_norms(B1, Cl, cbn)), 2)
    if not skip_host:
        out["host_norms_codebook_ms"] = round(_wall(lambda: experiments._norms_codebook(B1, Cl, h, seed=seed), reps=1), 1)
        out["host_quantize_norms_ms"] = round(_wall(lambda: experiments._quantize_norms(B1, Cl, cbn), reps=1), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--shapes", default="SIFT1M,Deep1M")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = []
    for shape, d, m in (("SIFT1M", 128, 8), ("Deep1M", 96, 16)):
        if shape not in a.shapes.split(","):
            continue
        r = dict(shape=shape, **run(a.n, d, m, 256, a.skip_host))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
