"""Byte-input encode against the f32 encode on one MI355X, at the SIFT1M shape (1e6 x 128, m = 8) and
at 1e6 x 96, m = 16, on sift_like bytes (integer-valued 0..255).

    python tools/encode_bytes_perf.py [--n 1000000] [--reps 21] [--out profiles/encode_bytes_perf.json]

In ONE process, the f32 leg and the byte leg of every quantity run interleaved (f32, bytes, f32, bytes, ...) after a warm-up of
both, and the MEDIAN of the repetitions is kept:
  resident  rq_dev_encode_pq  / rq_dev_encode_pq_bytes        device events
  resident  rq_dev_encode_opq / rq_dev_encode_opq_bytes       device events
  resident  widen (u8 -> f32 into a kept buffer) + rq_dev_encode_pq: what routing a shape through the widen fallback costs
  host      rq_encode_pq / rq_encode_pq_bytes                 wall clock, with the phases of rq_last_timing (h2d / kernel / tail)
plus the share of (vector, sub-quantizer) pairs the filter leaves to the exact pass on either path (ENC_STATS = 1, outside the
timed repetitions).  The codes of the two legs are compared before anything is timed.  The json records the library build,
the date, the device and every raw median; a figure is only meaningful against the other leg of the same run."""
import argparse
import ctypes
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _interleaved_events(legs, reps):
    """{name: median ms} of the callables in `legs`, run round-robin `reps` times, each bracketed by device events"""
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
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def _interleaved_host(legs, reps):
    """host-pointer calls: {name: {total_ms (wall), h2d_ms, kernel_ms, tail_ms}} medians, round-robin"""
    from rayuela_jl_amd import _lib
    rows = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t) * 1e3
            lt = _lib.last_timing()
            rows[k].append((wall, lt["h2d_ms"], lt["kernel_ms"], lt["d2h_ms"]))
    out = {}
    for k, v in rows.items():
        a = np.array(v)
        out[k] = dict(zip(("total_ms", "h2d_ms", "kernel_ms", "tail_ms"), (round(float(x), 4) for x in np.median(a, axis=0))))
    return out


def _flagged_share(fn):
    from rayuela_jl_amd import _lib
    import torch
    _lib.set_tuning("ENC_STATS", 1)
    try:
        fn()
        torch.cuda.synchronize()
        out = (ctypes.c_uint64 * 2)()
        _lib.check(_lib.lib().rq_last_encode_stats(ctypes.cast(out, ctypes.c_void_p)))
    finally:
        _lib.reset_tuning("ENC_STATS")
    return int(out[0]), int(out[1])


def run(n, d, m, h, reps, seed=1):
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib, synth_torch
    L = _lib.lib()
    tXf = synth_torch.sift_like(n, d, seed=seed)
    tX = tXf.to(torch.uint8)
    assert bool((tX.float() == tXf).all()), "sift_like is not integer-valued 0..255"
    sample = tXf[:20000].cpu().numpy()
    C = synth.codebooks(sample, m, h, seed=seed + 1, iters=3, sample=20000)
    Cc = synth.cat_codebooks(C)
    R = synth.rotation(d)
    tC, tR = torch.from_numpy(Cc).cuda(), torch.from_numpy(R).cuda()
    cf = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    cb = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    wide = torch.empty((n, d), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def pq_f32():
        _lib.check(L.rq_dev_encode_pq(cf.data_ptr(), tXf.data_ptr(), tC.data_ptr(), n, d, m, h, s))

    def pq_bytes():
        _lib.check(L.rq_dev_encode_pq_bytes(cb.data_ptr(), tX.data_ptr(), tC.data_ptr(), n, d, m, h, s))

    def pq_widen():
        wide.copy_(tX)
        _lib.check(L.rq_dev_encode_pq(cb.data_ptr(), wide.data_ptr(), tC.data_ptr(), n, d, m, h, s))

    def opq_f32():
        _lib.check(L.rq_dev_encode_opq(cf.data_ptr(), tXf.data_ptr(), tR.data_ptr(), tC.data_ptr(), n, d, m, h, s))

    def opq_bytes():
        _lib.check(L.rq_dev_encode_opq_bytes(cb.data_ptr(), tX.data_ptr(), tR.data_ptr(), tC.data_ptr(), n, d, m, h, s))

    out = {"n": n, "d": d, "m": m, "h": h, "reps": reps}
    # the two legs give the same codes (warm-up of both at the same time)
    for f32, byt, name in ((pq_f32, pq_bytes, "pq"), (opq_f32, opq_bytes, "opq")):
        f32()
        if name == "pq":
            out["f32_kernel"] = (L.rq_last_encode_kernel() or b"").decode()
        byt()
        if name == "pq":
            out["bytes_kernel"] = (L.rq_last_encode_kernel() or b"").decode()
        torch.cuda.synchronize()
        assert bool((cf == cb).all()), name + ": the byte path's codes differ from the f32 path's"
    pq_widen()
    pq_f32()
    torch.cuda.synchronize()
    assert bool((cf == cb).all()), "widen + f32 encode differs from the f32 encode"
    out["resident_ms"] = _interleaved_events({"pq_f32": pq_f32, "pq_bytes": pq_bytes, "pq_widen_then_f32": pq_widen,
                                              "opq_f32": opq_f32, "opq_bytes": opq_bytes}, reps)
    pf, ff = _flagged_share(pq_f32)
    pb, fb = _flagged_share(pq_bytes)
    out["flagged_pairs"] = {"pairs": pf, "f32": ff, "bytes": fb, "share_f32": round(ff / pf, 6), "share_bytes": round(fb / pb, 6)}
    # host -> host
    X = tX.cpu().numpy()
    Xf = X.astype(np.float32)
    hf = np.empty((n, m), dtype=np.uint8)
    hb = np.empty((n, m), dtype=np.uint8)

    def host_f32():
        _lib.check(L.rq_encode_pq(hf.ctypes.data, Xf.ctypes.data, Cc.ctypes.data, n, d, m, h))

    def host_bytes():
        _lib.check(L.rq_encode_pq_bytes(hb.ctypes.data, X.ctypes.data, Cc.ctypes.data, n, d, m, h))

    host_f32()
    host_bytes()
    assert np.array_equal(hf, hb), "host path: the byte path's codes differ from the f32 path's"
    out["host_to_host"] = _interleaved_host({"pq_f32": host_f32, "pq_bytes": host_bytes}, reps)
    r, hh = out["resident_ms"], out["host_to_host"]
    out["ratios_bytes_over_f32"] = {
        "resident_pq": round(r["pq_bytes"] / r["pq_f32"], 4),
        "resident_pq_widen_then_f32": round(r["pq_widen_then_f32"] / r["pq_f32"], 4),
        "resident_opq": round(r["opq_bytes"] / r["opq_f32"], 4),
        "host_to_host_pq": round(hh["pq_bytes"]["total_ms"] / hh["pq_f32"]["total_ms"], 4),
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_bytes_perf.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("the median is taken over at least 20 repetitions")
    import torch
    from rayuela_jl_amd import _lib
    res = {"tool": "tools/encode_bytes_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "shapes": []}
    for shape, d, m in (("SIFT1M shape", 128, 8), ("1e6 x 96, m = 16", 96, 16)):
        r = dict(shape=shape, **run(a.n, d, m, 256, a.reps))
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
