"""Training with more than 256 codewords per codebook on one MI355X: the update_centers kernel over
16-bit codes against two yardsticks made of code that predates it, and the phases of a wide Lloyd / OPQ iteration.

    python tools/train_wide_perf.py [--n 1000000] [--reps 5] [--out profiles/train_wide_perf.json]

Shapes, all resident, sift_like rows: SIFT1M shape (d = 128, m = 8) at h in {1024, 4096}; 1e6 x 96, m = 16, h = 1024; the m = 1,
d = 128 k-means at h in {4096, 16384}.  Per shape:
  update   one rq_dev_update_centers_wide call on the codes of one rq_dev_encode_pq_wide call (also timed), beside
           (a) torch.index_add_ of the sub-vectors + torch.bincount per sub-space: what a user of this GPU could do before.  It adds
               with float atomics, so its sums are NOT reproducible run to run; it is a speed yardstick only;
           (b) the cost model of the multi-pass design: ONE byte rq_dev_update_centers call at h = 256 on `codes & 255` of the same
               rows, times ceil(h / 256).
           The three legs run interleaved in one process; per leg median, minimum and maximum of the repetitions, and the
           max / min spread of yardstick (b) beside the ratios.
  pq       rq_train_pq_wide (host pointers, TRAIN_PROFILE = 1, `--niter` iterations): seeding, and per iteration encode, centres,
           convergence check and the rest of the loop's wall time, which is the refill of emptied centres (plus the small copies);
           `codes_without_rows` counts the codewords no row is assigned to at the end.
  opq      rq_train_opq_wide, one iteration by phase.
A figure means something only against the other legs of the same run."""
import argparse
import datetime
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("SIFT1M shape", 128, 8, 1024), ("SIFT1M shape", 128, 8, 4096), ("1e6 x 96, m = 16", 96, 16, 1024),
          ("m = 1 k-means, d = 128", 128, 1, 4096), ("m = 1 k-means, d = 128", 128, 1, 16384)]


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


def _sampled(tX, m, h, seed):
    import torch
    n, d = tX.shape
    sub = d // m
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.cat([tX[torch.randint(0, n, (h,), generator=g).cuda(), i * sub:(i + 1) * sub].reshape(-1) for i in range(m)])


def run_update(tX, d, m, h, reps, seed=1):
    import torch
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    n = tX.shape[0]
    sub = d // m
    nb = (h + 255) // 256
    tC = _sampled(tX, m, h, seed + h).contiguous()
    s = torch.cuda.current_stream().cuda_stream
    codes = torch.empty((n, m), dtype=torch.int16, device="cuda")
    _lib.check(L.rq_dev_encode_pq_wide(codes.data_ptr(), tX.data_ptr(), tC.data_ptr(), n, d, m, h, s))
    low = (codes & 255).to(torch.uint8).contiguous()
    idx = codes.to(torch.int64)
    Cw, Cb = tC.clone(), tC[:256 * d].clone()
    cw = torch.empty((m, h), dtype=torch.int32, device="cuda")
    cb = torch.empty((m, 256), dtype=torch.int32, device="cuda")
    sums = [torch.zeros((h, sub), dtype=torch.float32, device="cuda") for _ in range(m)]

    def leg_encode():
        _lib.check(L.rq_dev_encode_pq_wide(codes.data_ptr(), tX.data_ptr(), tC.data_ptr(), n, d, m, h, s))

    def leg_wide():
        _lib.check(L.rq_dev_update_centers_wide(Cw.data_ptr(), cw.data_ptr(), tX.data_ptr(), codes.data_ptr(), n, d, m, h, s))

    def leg_torch():
        for i in range(m):
            sums[i].zero_()
            sums[i].index_add_(0, idx[:, i], tX[:, i * sub:(i + 1) * sub])
            cnt = torch.bincount(idx[:, i], minlength=h)
            sums[i].div_(cnt.clamp(min=1).unsqueeze(1))

    def leg_byte_once():
        _lib.check(L.rq_dev_update_centers(Cb.data_ptr(), cb.data_ptr(), tX.data_ptr(), low.data_ptr(), n, d, m, 256, s))

    for f in (leg_wide, leg_torch, leg_byte_once):
        f()
    torch.cuda.synchronize()
    # the new kernel against yardstick (a): same counts, means within float tolerance of the atomics' order
    for i in range(m):
        cnt = torch.bincount(idx[:, i], minlength=h)
        assert bool((cw[i].to(torch.int64) == cnt).all())
        got = Cw[h * sub * i:h * sub * (i + 1)].view(h, sub)
        assert torch.allclose(got[cnt > 0], sums[i][cnt > 0], rtol=1e-4, atol=1e-3)
    res = _interleaved_events({"encode_wide": leg_encode, "update_wide": leg_wide, "torch_index_add": leg_torch,
                               "byte_update_once": leg_byte_once}, reps)
    out = dict(res)
    out["byte_cost_model_ms"] = round(res["byte_update_once"]["median_ms"] * nb, 4)
    out["byte_calls_modelled"] = nb
    out["wide_over_torch"] = round(res["update_wide"]["median_ms"] / res["torch_index_add"]["median_ms"], 4)
    out["wide_over_byte_model"] = round(res["update_wide"]["median_ms"] / out["byte_cost_model_ms"], 4)
    out["byte_yardstick_spread"] = round(res["byte_update_once"]["max_ms"] / res["byte_update_once"]["min_ms"], 4)
    out["update_over_encode"] = round(res["update_wide"]["median_ms"] / res["encode_wide"]["median_ms"], 4)
    return out


def run_train(X, m, h, niter, seed=1):
    import ctypes
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    n, d = X.shape
    out = {}
    _lib.set_tuning("TRAIN_PROFILE", 1)
    try:
        C, B, err = np.empty(h * d, np.float32), np.empty((n, m), np.int16), ctypes.c_double(0)
        _lib.check(L.rq_train_pq_wide(C.ctypes.data, B.ctypes.data, ctypes.cast(ctypes.byref(err), ctypes.c_void_p), X.ctypes.data,
                                      n, d, m, h, niter, seed, 0))
        p = _lib.train_profile()
        it = max(1.0, p["iterations"])
        per = {k: round(p[k] / it, 4) for k in ("update_centers_ms", "converge_ms")}
        per["encode_ms"] = round(p["encode_ms"] / (it + 1), 4)              # the loop's encodes and the final one
        loop_it = p["loop_ms"] / it
        per["refill_and_rest_ms"] = round(max(0.0, loop_it - per["update_centers_ms"] - per["converge_ms"] - per["encode_ms"]), 4)
        per["iteration_ms"] = round(loop_it, 4)
        without = int(sum(int((np.bincount(B[:, i], minlength=h) == 0).sum()) for i in range(m)))
        out["pq"] = {"iterations": p["iterations"], "seeding_ms": round(p["init_ms"], 3), "per_iteration": per,
                     "codes_without_rows": without, "error": err.value,
                     "update_share_of_iteration": round(per["update_centers_ms"] / loop_it, 4),
                     "encode_share_of_iteration": round(per["encode_ms"] / loop_it, 4),
                     "seeding_share_of_25_iterations": round(p["init_ms"] / (p["init_ms"] + 25 * loop_it), 4)}
        R, obj = np.empty((d, d), np.float32), np.zeros(2, np.float32)
        _lib.check(L.rq_train_opq_wide(C.ctypes.data, B.ctypes.data, R.ctypes.data, obj.ctypes.data, X.ctypes.data, n, d, m, h, 1,
                                       0, seed, None, None, 0))
        p = _lib.train_profile()
        it = max(1.0, p["iterations"])
        out["opq"] = {"iterations": p["iterations"], "init_ms": round(p["init_ms"], 3), "obj": [float(x) for x in obj],
                      "per_iteration": {k: round(p[k] / it, 4) for k in ("qerror_ms", "gram_ms", "svd_ms", "rotate_ms",
                                                                         "update_centers_ms", "encode_ms", "reconstruct_ms")},
                      "iteration_ms": round(p["loop_ms"] / it, 4)}
    finally:
        _lib.reset_tuning("TRAIN_PROFILE")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--niter", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_wide_perf.json"))
    a = ap.parse_args()
    import torch
    from rayuela_jl_amd import _lib, synth_torch
    res = {"tool": "tools/train_wide_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "n": a.n, "reps": a.reps, "niter": a.niter, "shapes": []}
    data = {}
    for name, d, m, h in SHAPES:
        if d not in data:
            data[d] = synth_torch.sift_like(a.n, d, seed=1)
        tX = data[d]
        r = {"shape": name, "d": d, "m": m, "h": h}
        r["update"] = run_update(tX, d, m, h, a.reps)
        r.update(run_train(np.ascontiguousarray(tX.cpu().numpy()), m, h, a.niter))
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:                 # after every shape: a run cut short keeps what it measured
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
