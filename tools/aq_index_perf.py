"""The resident index of the additive quantizers on one MI355X: what AqIndex / AqIndexU16 cost against
the handles and calls that served LSQ codes before them.

    python tools/aq_index_perf.py [--n 1000000] [--nq 1000] [--k 100] [--reps 7] [--out profiles/aq_index_perf.json]

All legs of a comparison run interleaved in ONE process (a, b, c, a, b, c, ...) after a warm-up of each, at least 5 rounds, every
call bracketed by device events on the null stream (the calls are synchronous, so this is the call's wall time on the device's
clock); kept per leg: the MEDIAN and the max / min spread over the rounds.  A ratio is only meaningful next to the spread of its
yardstick, which is recorded with it:
  (a) byte LSQ, (m, d) = (8, 128): AqIndex.search with 1, 2 and 8 logical shards  /  LsqIndex.search (rq_lsq_search)
  (b) wide, (m, h, d) = (8, 1024, 128): AqIndexU16.search with 1, 2 and 8 logical shards  /  rq_dev_linscan_aq_wide on resident
      tensors, and / the one-shot linscan_lsq_u16
  (c) set_codes with cbnorms (upload, norms and their quantization on the device, order, pre-filter preparation): time recorded
The answers of the legs of a comparison are compared, bit for bit, before anything is timed; the phases of the one-shard search
(rq_last_timing) are recorded next to the ratios."""
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


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _phases(fn):
    import rayuela_jl_amd as rq
    fn()
    return {k: round(v, 4) for k, v in rq.last_timing().items()}


def byte_leg(n, nq, k, reps, m=8, d=128, seed=3):
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(seed)
    C = [rng.standard_normal((256, d)).astype(np.float32) for _ in range(m)]
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    B = synth.random_codes(n, m, seed=seed)
    nrm = rq.aq_norms(B.astype(np.int16) + 1, C)
    cbn = np.quantile(nrm, (np.arange(256) + 0.5) / 256).astype(np.float32)
    handles = []
    try:
        lsq = rq.LsqIndex(B, C, nrm)
        handles.append(lsq)
        ref = lsq.search(Q, None, k)
        legs = {"lsq_index": lambda: lsq.search(Q, None, k)}
        for P in (1, 2, 8):
            ix = rq.AqIndex(C, devices=[0] * P).set_codes(B, dbnorms=nrm)
            handles.append(ix)
            assert _same(ix.search(Q, k), ref), P
            legs["aq_index_%d" % P] = (lambda ix=ix: ix.search(Q, k))
        t = _interleaved(legs, reps)
        out = {"n": n, "nq": nq, "k": k, "m": m, "d": d, "ms": t, "info_1": {k_: v for k_, v in handles[1].info().items()
                                                                          if k_ in ("ordered", "prepared")}}
        for P in (1, 2, 8):
            out["aq_index_%d_over_lsq_index" % P] = _ratio(t, "aq_index_%d" % P, "lsq_index")
        out["phases_ms"] = {"lsq_index": _phases(legs["lsq_index"]), "aq_index_1": _phases(legs["aq_index_1"])}
        # (c) set_codes with cbnorms on the one-shard handle (replaces the base: the handle is not searched again)
        ts = _interleaved({"set_codes_cbnorms": lambda: handles[1].set_codes(B, cbnorms=cbn),
                           "set_codes_dbnorms": lambda: handles[1].set_codes(B, dbnorms=nrm)}, max(5, reps // 2))
        out["set_codes_ms"] = ts
    finally:
        for ix in handles:
            ix.close()
    return out


def wide_leg(n, nq, k, reps, m=8, h=1024, d=128, seed=5):
    import torch
    import rayuela_jl_amd as rq
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(seed)
    C = [rng.standard_normal((h, d)).astype(np.float32) for _ in range(m)]
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    B = rng.integers(0, h, (n, m)).astype(np.int16)
    nrm = (rng.random(n) * 50).astype(np.float32)
    cbn = np.linspace(0, 50, 1024).astype(np.float32)
    bt, ct, qt, nt = [torch.from_numpy(a).cuda() for a in (B, np.stack(C), Q, nrm)]
    od = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    oi = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    ref = rq.linscan_lsq_u16(B, Q, C, nrm, None, k)
    legs = {"host_pointers": lambda: rq.linscan_lsq_u16(B, Q, C, nrm, None, k),
            "resident": lambda: rqd.linscan_aq_wide(bt, ct, qt, k, dbnorms=nt, id_base=1, out=(od, oi))}
    handles = []
    try:
        for P in (1, 2, 8):
            ix = rq.AqIndexU16(C, devices=[0] * P).set_codes(B, dbnorms=nrm)
            handles.append(ix)
            assert _same(ix.search(Q, k), ref), P
            legs["aq_index_%d" % P] = (lambda ix=ix: ix.search(Q, k))
        t = _interleaved(legs, reps)
        out = {"n": n, "nq": nq, "k": k, "m": m, "h": h, "d": d, "ms": t}
        for P in (1, 2, 8):
            out["aq_index_%d_over_host_pointers" % P] = _ratio(t, "aq_index_%d" % P, "host_pointers")
            out["aq_index_%d_over_resident" % P] = _ratio(t, "aq_index_%d" % P, "resident")
        out["phases_ms"] = {"aq_index_1": _phases(legs["aq_index_1"])}
        out["set_codes_ms"] = _interleaved({"set_codes_cbnorms": lambda: handles[0].set_codes(B, cbnorms=cbn),
                                            "set_codes_dbnorms": lambda: handles[0].set_codes(B, dbnorms=nrm)}, max(5, reps // 2))
    finally:
        for ix in handles:
            ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aq_index_perf.json"))
    a = ap.parse_args()
    reps = max(5, a.reps)
    import torch
    from rayuela_jl_amd import _lib
    res = {"tool": "tools/aq_index_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "reps": reps}
    res["byte_lsq"] = byte_leg(a.n, a.nq, a.k, reps)
    print(json.dumps(res["byte_lsq"]), flush=True)
    res["wide_lsq"] = wide_leg(a.n, a.nq, a.k, reps)
    print(json.dumps(res["wide_lsq"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
