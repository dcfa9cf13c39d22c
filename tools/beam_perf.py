"""Beam-search residual encoding on one MI355X (rq_dev_encode_rvq_beam) at the SIFT1M (d = 128, m = 8)
and Deep1M (d = 96, m = 16) shapes, n = 1e6, h = 256, beam widths H = 1, 4, 16, 32.

    python tools/beam_perf.py [--n 1000000] [--beams 1,4,16,32] [--out profiles/beam_perf.json]

Per shape: synthetic rows generated on the device, codebooks from train_rvq on the first 100 000 rows.  Per H, after a warm-up
call: the whole device-pointer call timed with device events (best of 3), the phases of rq_last_beam_timing of that fastest
call, the f32 matrix work 2 * n * d * h * sum_i H_i over the stage kernels' time as a rate and as a share of the 155 TFLOP/s
measured for v_mfma_f32_32x32x2_f32, and the mean squared residual.  rq_dev_encode_rvq (the greedy encoder, the yardstick of H = 1) is timed
on the same rows in the same run."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MFMA_TFLOPS = 155.0


def _timed(fn, reps=3):
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


def run(shape, n, d, m, h, beams, train_rows=100_000):
    import torch
    import rayuela_jl_amd as rq
    from rayuela_jl_amd import _lib, device as rqd, synth_torch
    L = _lib.lib()
    X = (synth_torch.sift_like(n, d, seed=11) if shape == "SIFT1M" else synth_torch.deep_like(n, d, seed=11)).contiguous()
    C, _, _ = rq.train_rvq(X[:min(n, train_rows)].cpu().numpy(), m, h, niter=4, seed=1)
    tC = torch.from_numpy(np.stack(C)).cuda()
    out = {"shape": shape, "n": n, "d": d, "m": m, "h": h, "beams": []}

    Xr = X.clone()
    codes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    rqd.encode_rvq(Xr, tC, out=codes)                                   # warm-up
    best = None
    for _ in range(3):
        Xr.copy_(X)
        t = _timed(lambda: rqd.encode_rvq(Xr, tC, out=codes), reps=1)
        best = t if best is None else min(best, t)
    out["greedy_rq_dev_encode_rvq_ms"] = round(best, 3)
    out["greedy_qerror"] = float((Xr.double() ** 2).sum(dim=1).mean().item())
    greedy = codes.clone()

    for H in beams:
        rqd.encode_rvq_beam(X, tC, H, out=codes)                        # warm-up: code objects, scratch growth
        whole, ph = None, None
        for _ in range(3):                                              # the phases kept are those of the fastest call
            t = _timed(lambda: rqd.encode_rvq_beam(X, tC, H, out=codes), reps=1)
            p3 = (ctypes.c_double * 3)()
            _lib.check(L.rq_last_beam_timing(ctypes.cast(p3, ctypes.c_void_p), 3))
            if whole is None or t < whole:
                whole, ph = t, list(p3)
        if not ph[0] > 0:
            raise SystemExit("rq_last_beam_timing reported no stage time: nothing to report")
        _, cost, Xb = rqd.encode_rvq_beam(X, tC, H, out=codes, want_extras=True)
        torch.cuda.synchronize()
        parents, Hi = 0, 1
        for _ in range(m):
            parents += Hi
            Hi = min(H, Hi * h)
        flop = 2.0 * n * d * h * parents
        r = {"H": H, "whole_call_ms": round(whole, 3), "stage_ms": round(ph[0], 3), "expand_ms": round(ph[1], 3),
             "other_ms": round(ph[2], 3), "sum_of_parents": parents, "matrix_flop": flop,
             "stage_TFLOPs": round(flop / (ph[0] * 1e-3) / 1e12, 2),
             "share_of_f32_mfma_peak": round(flop / (ph[0] * 1e-3) / 1e12 / F32_MFMA_TFLOPS, 4),
             "qerror": float((Xb.double() ** 2).sum(dim=1).mean().item())}
        if H == 1:
            r["codes_equal_greedy"] = bool(torch.equal(codes, greedy))
        del cost, Xb
        print(json.dumps(dict(shape=shape, **r)), flush=True)
        out["beams"].append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--beams", default="1,4,16,32")
    ap.add_argument("--shapes", default="SIFT1M,Deep1M")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("beam_perf needs an MI355X: no timing is taken without one")
    res = []
    for shape, d, m in (("SIFT1M", 128, 8), ("Deep1M", 96, 16)):
        if shape not in a.shapes.split(","):
            continue
        res.append(run(shape, a.n, d, m, 256, [int(b) for b in a.beams.split(",")]))
        if a.out:                                                           # after every shape: a partial file survives a time limit
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
