"""The ADC scan over 16-bit codes on one MI355X, against the byte bulk path as yardstick.

    python tools/scan_wide_perf.py [--n 1000000] [--reps 7] [--out profiles/scan_wide_perf.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/scan_wide_perf.py --trace      (the kernel split; a run of its own)

Device events around warmed-up resident calls of rq_dev_linscan_wide, n = 1e6, random codes, Gaussian codebooks:
  the SIFT1M shape (d = 128, m = 8) at h in {256, 1024, 4096};  1e6 x 96 at m = 16, h = 1024
  nq in {100, 1000}, k in {100, 1000}; median, minimum and maximum of the repetitions.
THE YARDSTICK is the byte bulk path at the same n and nq: rq_dev_linscan at k = 65537 (adc_bulk_keys_kernel<8, false>, then the
same select chain), interleaved in ONE process with the new path at h = 256 and the same k -- both produce the same keys (the
tool asserts it).  Per nq the json keeps the ratio and the yardstick's own spread (max / min).  Also reported: the bytes the
keys kernel writes, 8 n nq, over the time of the WHOLE call as a share of the 6.29 TB/s copy rate -- a lower bound of the keys
kernel's own share, which the --trace run splits out (per-kernel times of the keys kernel against the select chain).
A figure means something only against the other leg of the same run."""
import argparse
import datetime
import json
import os
import statistics
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_TBS = 6.29
SHAPES = [("SIFT1M shape", 128, 8, 256), ("SIFT1M shape", 128, 8, 1024), ("SIFT1M shape", 128, 8, 4096),
          ("1e6 x 96, m = 16", 96, 16, 1024)]
NQS, KS = (100, 1000), (100, 1000)
YARD_K = 65537


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


def _base(n, d, m, h, nq, seed):
    import torch
    g = torch.Generator("cuda").manual_seed(seed)
    codes = torch.randint(0, h, (n, m), dtype=torch.int16, device="cuda", generator=g)
    centers = torch.randn((m, h, d // m), dtype=torch.float32, device="cuda", generator=g)
    queries = torch.randn((nq, d), dtype=torch.float32, device="cuda", generator=g)
    return codes, centers, queries


def run_shape(name, n, d, m, h, reps):
    import torch
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    L = _lib.lib()
    out = {"shape": name, "n": n, "d": d, "m": m, "h": h, "reps": reps, "plan": _lib.scan_wide_plan(m, h), "calls": []}
    for nq in NQS:
        codes, centers, queries = _base(n, d, m, h, nq, seed=h + nq)
        for k in KS:
            res = (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int32, device="cuda"))
            leg = lambda: rqd.linscan_wide(codes, centers, queries, k, out=res)      # noqa: E731
            leg()
            kernel = (L.rq_last_scan_kernel() or b"").decode()
            torch.cuda.synchronize()
            t = _interleaved_events({"wide": leg}, reps)["wide"]
            t.update(nq=nq, k=k, kernel=kernel,
                     key_bytes_over_call_time_share=round(8.0 * n * nq / (t["median_ms"] * 1e-3) / 1e12 / COPY_RATE_TBS, 4))
            out["calls"].append(t)
        if h == 256:      # the yardstick: the byte bulk path on the same codes, interleaved with the new path at the same k
            b8 = codes.to(torch.uint8)
            rw = (torch.empty((nq, YARD_K), dtype=torch.float32, device="cuda"), torch.empty((nq, YARD_K), dtype=torch.int32, device="cuda"))
            ry = (torch.empty_like(rw[0]), torch.empty_like(rw[1]))
            legs = {"wide": lambda: rqd.linscan_wide(codes, centers, queries, YARD_K, out=rw),
                    "yardstick": lambda: rqd.linscan(b8, centers, queries, YARD_K, out=ry)}
            legs["yardstick"]()
            ykernel = (L.rq_last_scan_kernel() or b"").decode()
            legs["wide"]()
            torch.cuda.synchronize()
            assert torch.equal(rw[1], ry[1]) and torch.equal(rw[0].view(torch.int32), ry[0].view(torch.int32)), "answers differ"
            r = _interleaved_events(legs, reps)
            out.setdefault("yardstick", []).append({
                "nq": nq, "k": YARD_K, "yardstick_kernel": ykernel, "wide": r["wide"], "yardstick": r["yardstick"],
                "wide_over_yardstick": round(r["wide"]["median_ms"] / r["yardstick"]["median_ms"], 4),
                "yardstick_spread": round(r["yardstick"]["max_ms"] / r["yardstick"]["min_ms"], 4)})
            del b8, rw, ry
        del codes, centers, queries
        torch.cuda.empty_cache()
    return out


def run_trace(n):
    """A few calls per shape at nq = 1000, k = 100 for a rocprofv3 --kernel-trace --stats run (no timing of its own)."""
    import torch
    from rayuela_jl_amd import device as rqd
    for _, d, m, h in SHAPES:
        codes, centers, queries = _base(n, d, m, h, 1000, seed=h)
        for _ in range(3):
            rqd.linscan_wide(codes, centers, queries, 100)
        if h == 256:
            b8 = codes.to(torch.uint8)
            for _ in range(3):
                rqd.linscan(b8, centers, queries, YARD_K)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_wide_perf.json"))
    a = ap.parse_args()
    import torch
    from rayuela_jl_amd import _lib
    if a.trace:
        run_trace(a.n)
        return
    res = {"tool": "tools/scan_wide_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "copy_rate_tb_s": COPY_RATE_TBS, "shapes": []}
    for name, d, m, h in SHAPES:
        r = run_shape(name, a.n, d, m, h, a.reps)
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
