"""The resident handles over 16-bit codes on one MI355X: what the byte loader of the wide encode, the
index handle and the row slices of the wide scan cost against their yardsticks.

    python tools/handles_wide_perf.py [--n 1000000] [--reps 21] [--big-rows 300000000] [--out profiles/handles_wide_perf.json]

All legs of a comparison run interleaved in ONE process (a, b, a, b, ...) after a warm-up of each, every call bracketed by device
events on the null stream (the calls are synchronous, so this is the call's wall time on the device's clock); kept per leg: the
MEDIAN and the max / min spread over the repetitions.  A ratio is only meaningful next to the spread of its yardstick:
  (a) rq_dataset_encode_wide on a u8 base  /  the same call on the widened f32 base       PQ and OPQ; 1e6 x 128, m = 8, h = 1024
      and 4096; 1e6 x 96, m = 16, h = 1024
  (b) IndexU16.search with 1, 2 and 8 logical shards  /  rq_linscan_pq_wide from host pointers, and / rq_dev_linscan_wide on
      resident tensors                                                                    1e6 rows, 1000 queries, k = 100
  (c) rq_dev_linscan_wide cut into 4 slices by the test hook  /  the unsliced call        1e6 rows
      and, where the device has the memory, one base that really is sliced: --big-rows x 8 synthetic codes, 16 queries
The answers of the legs of a comparison are compared before anything is timed."""
import argparse
import datetime
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _interleaved(legs, reps):
    """{name: {median_ms, min_ms, max_ms, spread}} of the callables in `legs`, round-robin, each bracketed by device events"""
    import torch
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "spread": round(max(v) / min(v), 4)} for k, v in ms.items()}


def _ratio(t, leg, yardstick):
    return {"ratio": round(t[leg]["median_ms"] / t[yardstick]["median_ms"], 4), "yardstick": yardstick,
            "yardstick_spread": t[yardstick]["spread"]}


def encode_leg(n, d, m, h, reps, seed=1):
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (n, d), dtype=np.uint8)          # (the streaming kernel has no data-dependent path)
    Xf = X.astype(np.float32)
    off = synth.splitarray(d, m)
    C = [Xf[rng.integers(0, n, h), off[i]:off[i + 1]] + rng.standard_normal((h, off[i + 1] - off[i])).astype(np.float32)
         for i in range(m)]
    R = synth.rotation(d)
    out = {"n": n, "d": d, "m": m, "h": h}
    with rq.Dataset(X) as du, rq.Dataset(Xf) as df:
        for name, Rm in (("pq", None), ("opq", R)):
            assert np.array_equal(du.quantize_u16(C, R=Rm), df.quantize_u16(C, R=Rm)), name + ": byte and f32 codes differ"
            t = _interleaved({"f32": lambda: df.quantize_u16(C, R=Rm), "u8": lambda: du.quantize_u16(C, R=Rm)}, reps)
            out[name] = {"ms": t, "u8_over_f32": _ratio(t, "u8", "f32")}
    return out


def index_leg(n, nq, k, reps, m=8, h=1024, d=128, seed=3):
    import torch
    import rayuela_jl_amd as rq
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(seed)
    C = [rng.standard_normal((h, d // m)).astype(np.float32) for _ in range(m)]
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    B = rng.integers(0, h, (n, m)).astype(np.int16)
    bt, ct, qt = torch.from_numpy(B).cuda(), torch.from_numpy(np.stack(C)).cuda(), torch.from_numpy(Q).cuda()
    od = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    oi = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    ref = rq.linscan_pq_u16(B, Q, C, k)
    legs = {"host_pointers": lambda: rq.linscan_pq_u16(B, Q, C, k),
            "resident": lambda: rqd.linscan_wide(bt, ct, qt, k, id_base=1, out=(od, oi))}
    handles = []
    try:
        for P in (1, 2, 8):
            ix = rq.IndexU16(C, d, devices=[0] * P).set_codes(B)
            handles.append(ix)
            got = ix.search(Q, k)
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), P
            legs["index_%d" % P] = (lambda ix=ix: ix.search(Q, k))
        t = _interleaved(legs, reps)
    finally:
        for ix in handles:
            ix.close()
    out = {"n": n, "nq": nq, "k": k, "m": m, "h": h, "d": d, "ms": t}
    for P in (1, 2, 8):
        out["index_%d_over_host_pointers" % P] = _ratio(t, "index_%d" % P, "host_pointers")
        out["index_%d_over_resident" % P] = _ratio(t, "index_%d" % P, "resident")
    return out


def slices_leg(n, nq, k, reps, big_rows, m=8, h=1024, d=16, seed=5):
    import torch
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    L = _lib.lib()
    rng = np.random.default_rng(seed)
    ct = torch.from_numpy(rng.standard_normal((m, h, d // m)).astype(np.float32)).cuda()
    qt = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).cuda()
    bt = torch.randint(0, h, (n, m), dtype=torch.int16, device="cuda")
    rows = -(-n // 4)

    def forced():
        prev = L.rq_test_scan_wide_slice_rows(rows)
        try:
            return rqd.linscan_wide(bt, ct, qt, k)
        finally:
            L.rq_test_scan_wide_slice_rows(prev)

    d0, i0 = rqd.linscan_wide(bt, ct, qt, k)
    d1, i1 = forced()
    assert torch.equal(i0, i1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32)), "sliced and unsliced answers differ"
    t = _interleaved({"unsliced": lambda: rqd.linscan_wide(bt, ct, qt, k), "four_slices": forced}, reps)
    out = {"n": n, "nq": nq, "k": k, "m": m, "h": h, "ms": t, "four_slices_over_unsliced": _ratio(t, "four_slices", "unsliced")}
    del bt
    need = big_rows * m * 2 + (3 << 30)
    if big_rows > 0 and torch.cuda.mem_get_info(0)[0] >= need:
        big = torch.empty((big_rows, m), dtype=torch.int16, device="cuda")
        for r0 in range(0, big_rows, 1 << 26):
            r1 = min(big_rows, r0 + (1 << 26))
            big[r0:r1] = torch.randint(0, h, (r1 - r0, m), dtype=torch.int16, device="cuda")
        q16 = qt[:16].contiguous()
        plan = _lib.scan_wide_slices(big_rows, 16, m, h, k)
        tb = _interleaved({"sliced_base": lambda: rqd.linscan_wide(big, ct, q16, k)}, max(3, reps // 4))
        out["really_sliced"] = {"n": big_rows, "nq": 16, "plan": plan, "ms": tb,
                                "ns_per_row_and_query": round(tb["sliced_base"]["median_ms"] * 1e6 / (big_rows * 16.0), 5)}
    else:
        out["really_sliced"] = "skipped: needs %.1f GB of free device memory" % (need / 1e9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--big-rows", type=int, default=300_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handles_wide_perf.json"))
    a = ap.parse_args()
    import torch
    from rayuela_jl_amd import _lib
    res = {"tool": "tools/handles_wide_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "encode": [], "index": None, "slices": None}
    for d, m, h in ((128, 8, 1024), (128, 8, 4096), (96, 16, 1024)):
        r = encode_leg(a.n, d, m, h, a.reps)
        print(json.dumps(r), flush=True)
        res["encode"].append(r)
    res["index"] = index_leg(a.n, 1000, 100, a.reps)
    print(json.dumps(res["index"]), flush=True)
    res["slices"] = slices_leg(a.n, 1000, 100, a.reps, a.big_rows)
    print(json.dumps(res["slices"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
