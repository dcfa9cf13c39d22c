"""The 16-bit encode (more than 256 codewords per codebook) on one MI355X, against a yardstick made of
the h <= 256 exact kernel.

    python tools/encode_wide_perf.py [--n 1000000] [--reps 7] [--out profiles/encode_wide_perf.json]

Device events around warmed-up resident calls, n = 1e6, sift_like data, codebooks sampled from it:
  PQ    SIFT1M shape (d = 128, m = 8) at h in {1024, 4096};  1e6 x 96, m = 16, h = 1024;
        the m = 1, d = 128 assignment at h in {4096, 16384}
  RVQ   one rq_dev_encode_rvq_wide call at d = 128, m = 4, h = 1024 (no yardstick leg: the stages depend on each other)
THE YARDSTICK of a PQ shape is ceil(h / 256) back-to-back rq_dev_encode_pq calls with ENC_SPLIT = 0 -- the exact f32-MFMA
kernels of the h <= 256 path -- on 256-codeword slices of the same codebook over the same rows: the same products, without the
merge.  The two legs run interleaved in ONE process (wide, yardstick, wide, ...); per leg the json keeps the median, the minimum
and the maximum of the repetitions, so the spread of the yardstick itself stands beside the difference.  Also reported:
2 n d h / t as a fraction of the f32 matrix peak (157.3 TFLOP/s).  A figure means something only against the other leg of
the same run."""
import argparse
import datetime
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK_TFLOPS = 157.3
PQ_SHAPES = [("SIFT1M shape", 128, 8, 1024), ("SIFT1M shape", 128, 8, 4096), ("1e6 x 96, m = 16", 96, 16, 1024),
             ("m = 1 assignment, d = 128", 128, 1, 4096), ("m = 1 assignment, d = 128", 128, 1, 16384)]
RVQ_SHAPE = ("RVQ, d = 128, m = 4", 128, 4, 1024)


def _interleaved_events(legs, reps):
    """{name: {median, min, max} ms} of the callables in `legs`, run round-robin `reps` times, each bracketed by device events"""
    import torch
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in ms.items()}


def _peak_share(n, d, h, ms):
    return round(2.0 * n * d * h / (ms * 1e-3) / 1e12 / F32_MATRIX_PEAK_TFLOPS, 4)


def _sampled(tX, m, h, seed):
    """flat concatenation of m [h][sub] codebooks, rows of the data (d % m == 0 here)"""
    import torch
    n, d = tX.shape
    sub = d // m
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.cat([tX[torch.randint(0, n, (h,), generator=g).cuda(), i * sub:(i + 1) * sub].reshape(-1) for i in range(m)])


def run_pq(name, n, d, m, h, reps, seed=1):
    import torch
    from rayuela_jl_amd import _lib, synth_torch
    L = _lib.lib()
    tX = synth_torch.sift_like(n, d, seed=seed)
    tC = _sampled(tX, m, h, seed + h).contiguous()
    sub = d // m
    nb = (h + 255) // 256
    # slice b of the codebook: the m [256][sub] blocks of codewords 256 b .. 256 b + 255
    C3 = tC.view(m, h, sub)
    slices = [C3[:, 256 * b:256 * (b + 1), :].contiguous() for b in range(nb)]
    assert h % 256 == 0
    wide = torch.empty((n, m), dtype=torch.int16, device="cuda")
    part = [torch.empty((n, m), dtype=torch.uint8, device="cuda") for _ in range(nb)]
    s = torch.cuda.current_stream().cuda_stream

    def leg_wide():
        _lib.check(L.rq_dev_encode_pq_wide(wide.data_ptr(), tX.data_ptr(), tC.data_ptr(), n, d, m, h, s))

    def leg_yardstick():
        for b in range(nb):
            _lib.check(L.rq_dev_encode_pq(part[b].data_ptr(), tX.data_ptr(), slices[b].data_ptr(), n, d, m, 256, s))

    out = {"shape": name, "n": n, "d": d, "m": m, "h": h, "reps": reps, "yardstick_calls": nb}
    _lib.set_tuning("ENC_SPLIT", 0)
    try:
        leg_wide()
        out["wide_kernel"] = (L.rq_last_encode_kernel() or b"").decode()
        leg_yardstick()
        out["yardstick_kernel"] = (L.rq_last_encode_kernel() or b"").decode()
        torch.cuda.synchronize()
        # every wide code is the slice winner of its own block
        blk = (wide.to(torch.int64) >> 8)
        own = torch.stack(part, dim=0).to(torch.int64).gather(0, blk.unsqueeze(0))[0]
        assert bool((own == (wide.to(torch.int64) & 255)).all()), "a wide code is not the winner of its own 256-codeword slice"
        res = _interleaved_events({"wide": leg_wide, "yardstick": leg_yardstick}, reps)
    finally:
        _lib.reset_tuning("ENC_SPLIT")
    out["wide"], out["yardstick"] = res["wide"], res["yardstick"]
    out["wide"]["f32_matrix_peak_share"] = _peak_share(n, d, h, res["wide"]["median_ms"])
    out["yardstick"]["f32_matrix_peak_share"] = _peak_share(n, d, h, res["yardstick"]["median_ms"])
    out["wide_over_yardstick"] = round(res["wide"]["median_ms"] / res["yardstick"]["median_ms"], 4)
    out["yardstick_spread"] = round(res["yardstick"]["max_ms"] / res["yardstick"]["min_ms"], 4)
    return out


def run_rvq(name, n, d, m, h, reps, seed=1):
    import torch
    from rayuela_jl_amd import _lib, synth_torch
    L = _lib.lib()
    tX = synth_torch.sift_like(n, d, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 5)
    tC = torch.stack([tX[torch.randint(0, n, (h,), generator=g).cuda()] * (0.5 ** i) for i in range(m)]).contiguous()
    Xr = torch.empty_like(tX)
    codes = torch.empty((n, m), dtype=torch.int16, device="cuda")
    counts = torch.empty((m, h), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def leg():
        _lib.check(L.rq_dev_encode_rvq_wide(codes.data_ptr(), Xr.data_ptr(), tC.data_ptr(), n, d, m, h, counts.data_ptr(), s))

    import statistics as st
    ms = []
    for r in range(reps + 1):
        Xr.copy_(tX)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        leg()
        e1.record()
        torch.cuda.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    med = st.median(ms)
    return {"shape": name, "n": n, "d": d, "m": m, "h": h, "reps": reps, "wide_kernel": (L.rq_last_encode_kernel() or b"").decode(),
            "wide": {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                     "f32_matrix_peak_share": _peak_share(n, d, h * m, med)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_wide_perf.json"))
    a = ap.parse_args()
    import torch
    from rayuela_jl_amd import _lib
    res = {"tool": "tools/encode_wide_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "f32_matrix_peak_tflops": F32_MATRIX_PEAK_TFLOPS, "shapes": []}
    for name, d, m, h in PQ_SHAPES:
        r = run_pq(name, a.n, d, m, h, a.reps)
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    r = run_rvq(*RVQ_SHAPE[:1], a.n, *RVQ_SHAPE[1:], a.reps)
    print(json.dumps(r), flush=True)
    res["shapes"].append(r)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
