"""linscan_lsq over 16-bit codes and the wide norm kernels on one MI355X, against their yardsticks.

    python tools/aq_wide_perf.py [--n 1000000] [--reps 7] [--out profiles/aq_wide_perf.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/aq_wide_perf.py --trace      (the kernel split; a run of its own)

Device events around warmed-up resident calls, n = 1e6, random codes and norms, Gaussian codebooks, LSQ mode, the legs of a
comparison interleaved in ONE process; median, minimum and maximum of the repetitions.
  d = 128: (m, h) in {(8, 256), (8, 1024), (8, 4096), (4, 16384)};  d = 96: (16, 1024);  nq in {100, 1000}, k in {100, 1000}
YARDSTICKS
  (a) h = 256: the byte bulk path rq_dev_linscan_aq at k = 65537 against rq_dev_linscan_aq_wide at the same k; the keys are
      asserted equal.  The ratio stands beside the yardstick's own max / min.
  (b) every shape: rq_dev_linscan_wide at the same (n, nq, m, h, k) with sub = d / m -- the AQ call differs from it by the table
      build and one add per row.  The table kernel is timed on its own through rq_dev_aq_lut_wide on the queries of one batch
      (the plain [nq][m][h] layout: the same kernel, one query per stored entry), and set against the AQ call.
  (c) the table kernel: 2 nq m h d VALU operations over its time, as a share of the 157.3 TFLOP/s f32 vector rate.  The obvious
      port's time comes from tools/micro/aq_lut_ab.hip, a run of its own.
NORMS: rq_dev_aq_norms_wide / rq_dev_quantize_norms_wide beside the byte entries at h = hn = 256 (same bits, asserted), then at
h = 1024 and hn in {1024, 4096}.
A figure means something only against the other leg of the same run."""
import argparse
import datetime
import json
import os
import statistics
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_VECTOR_TFLOPS = 157.3
SHAPES = [(128, 8, 256), (128, 8, 1024), (128, 8, 4096), (128, 4, 16384), (96, 16, 1024)]      # d, m, h
NQS, KS = (100, 1000), (100, 1000)
YARD_K = 65537
BULK_USABLE_BYTES = (2 << 30) // 5 * 4


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
    codebooks = torch.randn((m, h, d), dtype=torch.float32, device="cuda", generator=g)
    queries = torch.randn((nq, d), dtype=torch.float32, device="cuda", generator=g)
    norms = torch.rand((n,), dtype=torch.float32, device="cuda", generator=g) * 50
    return codes, codebooks, queries, norms


def _pq_view(codebooks, m, h, d):
    """centers [m][h][d/m] for the PQ leg of yardstick (b): the first d/m coordinates of every codeword"""
    return codebooks[:, :, :d // m].contiguous()


def run_shape(n, d, m, h, reps):
    import torch
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    L = _lib.lib()
    out = {"n": n, "d": d, "m": m, "h": h, "reps": reps, "plan": _lib.scan_wide_plan(m, h), "calls": []}
    for nq in NQS:
        codes, cb, queries, norms = _base(n, d, m, h, nq, seed=h + nq)
        centers = _pq_view(cb, m, h, d)
        for k in KS:
            ra = (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int32, device="cuda"))
            rp = (torch.empty_like(ra[0]), torch.empty_like(ra[1]))
            batch = max(1, min(nq, BULK_USABLE_BYTES // (8 * n + 16 * k + 4 * m * h)))       # an upper bound of h16_batch
            qb = queries[:batch].contiguous()
            legs = {"aq": lambda: rqd.linscan_aq_wide(codes, cb, queries, k, dbnorms=norms, out=ra),
                    "pq": lambda: rqd.linscan_wide(codes, centers, queries, k, out=rp),
                    "table": lambda: rqd.aq_lut_wide(cb, qb)}
            legs["aq"]()
            kernel = (L.rq_last_scan_kernel() or b"").decode()
            legs["pq"]()
            legs["table"]()
            torch.cuda.synchronize()
            r = _interleaved_events(legs, reps)
            batches = -(-nq // batch)
            tab = r["table"]["median_ms"]
            out["calls"].append({
                "nq": nq, "k": k, "kernel": kernel, "aq": r["aq"], "pq_same_shape": r["pq"],
                "aq_over_pq": round(r["aq"]["median_ms"] / r["pq"]["median_ms"], 4),
                "pq_spread": round(r["pq"]["max_ms"] / r["pq"]["min_ms"], 4),
                "table_queries": batch, "table": r["table"], "batches": batches,
                "table_share_of_aq_call": round(tab * nq / batch / r["aq"]["median_ms"], 4),
                "table_valu_tops": round(2.0 * batch * m * h * d / (tab * 1e-3) / 1e12, 3),
                "table_share_of_f32_vector_rate": round(2.0 * batch * m * h * d / (tab * 1e-3) / 1e12 / F32_VECTOR_TFLOPS, 4)})
        if h == 256:      # yardstick (a): the byte bulk path on the same codes, interleaved with the new path at the same k
            b8 = codes.to(torch.uint8)
            cb2 = cb.view(m * h, d)
            kw = torch.empty((nq, YARD_K), dtype=torch.int64, device="cuda")
            legs = {"wide": lambda: rqd.linscan_aq_wide(codes, cb, queries, YARD_K, dbnorms=norms, want_keys=True, out=kw),
                    "yardstick": lambda: rqd.linscan_aq(b8, cb2, queries, YARD_K, dbnorms=norms, want_keys=True)}
            ky = legs["yardstick"]()
            ykernel = (L.rq_last_scan_kernel() or b"").decode()
            legs["wide"]()
            torch.cuda.synchronize()
            assert torch.equal(kw, ky), "keys differ"
            del ky
            r = _interleaved_events(legs, reps)
            out.setdefault("yardstick", []).append({
                "nq": nq, "k": YARD_K, "yardstick_kernel": ykernel, "wide": r["wide"], "yardstick": r["yardstick"],
                "wide_over_yardstick": round(r["wide"]["median_ms"] / r["yardstick"]["median_ms"], 4),
                "yardstick_spread": round(r["yardstick"]["max_ms"] / r["yardstick"]["min_ms"], 4)})
            del b8, kw
        del codes, cb, queries, norms, centers
        torch.cuda.empty_cache()
    return out


def run_norms(n, reps):
    import torch
    from rayuela_jl_amd import device as rqd
    out = []
    d, m = 128, 8
    for h, hns in ((256, (256,)), (1024, (1024, 4096))):
        codes, cb, _, _ = _base(n, d, m, h, 1, seed=7 + h)
        norms = rqd.aq_norms_wide(codes, cb)
        legs = {"aq_norms_wide": lambda: rqd.aq_norms_wide(codes, cb, out=norms)}
        if h == 256:
            b8 = codes.to(torch.uint8)
            n8 = rqd.aq_norms(b8, cb)
            assert torch.equal(n8.view(torch.int32), norms.view(torch.int32)), "norms differ"
            legs["aq_norms_byte"] = lambda: rqd.aq_norms(b8, cb, out=n8)
        for hn in hns:
            cbn = (torch.rand((hn,), device="cuda", generator=torch.Generator("cuda").manual_seed(hn)) * float(norms.max()))
            cw, dw = rqd.quantize_norms_wide(norms, cbn)
            legs["quantize_wide_hn%d" % hn] = lambda cbn=cbn, cw=cw, dw=dw: rqd.quantize_norms_wide(norms, cbn, out=cw, dbnorms=dw)
            if hn == 256:
                c8, d8 = rqd.quantize_norms(norms, cbn)
                assert torch.equal(c8.to(torch.int16), cw) and torch.equal(d8.view(torch.int32), dw.view(torch.int32))
                legs["quantize_byte_hn256"] = lambda cbn=cbn, c8=c8, d8=d8: rqd.quantize_norms(norms, cbn, out=c8, dbnorms=d8)
        torch.cuda.synchronize()
        r = _interleaved_events(legs, reps)
        out.append({"n": n, "d": d, "m": m, "h": h, "legs": r})
    return out


def run_trace(n):
    """A few calls per shape at nq = 1000, k = 100 for a rocprofv3 --kernel-trace --stats run (no timing of its own)."""
    import torch
    from rayuela_jl_amd import device as rqd
    for d, m, h in SHAPES:
        codes, cb, queries, norms = _base(n, d, m, h, 1000, seed=h)
        for _ in range(3):
            rqd.linscan_aq_wide(codes, cb, queries, 100, dbnorms=norms)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aq_wide_perf.json"))
    a = ap.parse_args()
    import torch
    from rayuela_jl_amd import _lib
    if a.trace:
        run_trace(a.n)
        return
    res = {"tool": "tools/aq_wide_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "f32_vector_tflops": F32_VECTOR_TFLOPS, "shapes": []}
    for d, m, h in SHAPES:
        r = run_shape(a.n, d, m, h, a.reps)
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    res["norms"] = run_norms(a.n, a.reps)
    print(json.dumps(res["norms"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
