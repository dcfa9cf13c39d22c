"""IVFADC on one MI355X: what IvfIndex.search costs against the exhaustive byte scan over the same rows,
and what recall it keeps.

    python tools/ivf_perf.py [--n 1000000] [--train 100000] [--niter 10] [--k 100] [--reps 5] [--out profiles/ivf_perf.json]
                             [--shapes sift,deep] [--nlists 1024,4096] [--nprobes 1,8,32,128] [--nqs 1000,10000]

Shapes: SIFT1M (n = 1e6, d = 128, m = 8, synth.sift_like) and 1e6 x 96 with m = 16 (synth.deep_like).  Per (shape, nlist,
by_residual) the quantizers are trained with train_ivfpq on a sample, the index is built once, and per nq the legs
{Index.search (the yardstick: the exhaustive scan of the same rows, PQ codes of the same m), IvfIndex.search at every nprobe} run
interleaved in ONE process after a warm-up of each, every call bracketed by device events on the null stream (the calls are
synchronous); kept per leg: the MEDIAN and max / min over the rounds.  A ratio is recorded with the spread (max / min) of its
yardstick, without which it means nothing.  Recall@1/10/100 is that of eval_recall against groundtruth (the exact nearest row),
for both by_residual settings and for the yardstick; the split of one search into probe selection, item list, keys kernel and
select chain is the library's own (hipEvents, rq_ivf_last_timing)."""
import argparse
import datetime
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"sift": dict(d=128, m=8, gen="sift_like"), "deep": dict(d=96, m=16, gen="deep_like")}


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


def _recall(rq, gt, idx, k):
    r = rq.eval_recall(gt, idx, k, verbose=False)
    return {"r@%d" % i: round(float(r[i - 1]), 4) for i in (1, 10, 100) if i <= k}


def shape_leg(name, a):
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    sh = SHAPES[name]
    d, m = sh["d"], sh["m"]
    gen = getattr(synth, sh["gen"])
    Xb = gen(a.n, d, seed=1)
    Xt = gen(a.train, d, seed=2)
    nqmax = max(a.nqs)
    Xq = gen(nqmax, d, seed=3)
    gt = rq.groundtruth(Xb, Xq, 1)[0][:, 0]
    out = {"n": a.n, "d": d, "m": m, "k": a.k, "train_rows": a.train, "niter": a.niter, "configs": []}
    # the yardstick: PQ codes of the same m over the same rows, resident, scanned exhaustively
    Cpq, _, _ = rq.train_pq(Xt, m, 256, a.niter, seed=5)
    Bpq = rq.quantize_pq_u8(Xb, Cpq)
    with rq.Index(Cpq, d) as flat:
        flat.set_codes(Bpq)
        out["yardstick_recall"] = _recall(rq, gt, flat.search(Xq, a.k)[1], a.k)
        for nlist in a.nlists:
            for by_residual in (True, False):
                Q, C = rq.train_ivfpq(Xt, nlist, m, niter=a.niter, seed=7, by_residual=by_residual)
                with rq.IvfIndex(Q, C, by_residual=by_residual) as ix:
                    ix.build(Xb)
                    info = ix.info()
                    cfg = {"nlist": nlist, "by_residual": by_residual, "largest_list": info["largest_list"],
                           "empty_lists": info["empty_lists"], "recall": {}, "runs": []}
                    nprobes = [p for p in a.nprobes if p <= nlist]
                    for nprobe in nprobes:
                        cfg["recall"][str(nprobe)] = _recall(rq, gt, ix.search(Xq, nprobe, a.k)[1], a.k)
                    for nq in a.nqs:
                        X = np.ascontiguousarray(Xq[:nq])
                        legs = {"exhaustive": lambda X=X: flat.search(X, a.k)}
                        for nprobe in nprobes:
                            legs["nprobe_%d" % nprobe] = (lambda X=X, p=nprobe: ix.search(X, p, a.k))
                        t = _interleaved(legs, a.reps)
                        run = {"nq": nq, "ms": t, "yardstick": "exhaustive", "yardstick_spread": t["exhaustive"]["spread"],
                               "over_exhaustive": {}, "split_ms": {}, "plan": {}}
                        for nprobe in nprobes:
                            key = "nprobe_%d" % nprobe
                            run["over_exhaustive"][key] = round(t[key]["median_ms"] / t["exhaustive"]["median_ms"], 4)
                            legs[key]()
                            inf = ix.info()
                            run["split_ms"][key] = {p: round(inf[p], 4) for p in ("probe_ms", "items_ms", "keys_ms", "select_ms")}
                            run["plan"][key] = {p: inf[p] for p in ("ld", "batch", "items", "rows_scanned")}
                        cfg["runs"].append(run)
                        print(json.dumps({"shape": name, "nlist": nlist, "by_residual": by_residual, "run": run}), flush=True)
                    out["configs"].append(cfg)
    return out


def _ints(s):
    return [int(x) for x in s.split(",") if x]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--train", type=int, default=100_000)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="sift,deep")
    ap.add_argument("--nlists", type=_ints, default=[1024, 4096])
    ap.add_argument("--nprobes", type=_ints, default=[1, 8, 32, 128])
    ap.add_argument("--nqs", type=_ints, default=[1000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_perf.json"))
    a = ap.parse_args()
    a.reps = max(5, a.reps)
    import torch
    from rayuela_jl_amd import _lib
    res = {"tool": "tools/ivf_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": {}}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for name in a.shapes.split(","):
        res["shapes"][name] = shape_leg(name, a)
        with open(a.out, "w") as f:          # kept after every shape: a run that is cut short leaves what it measured
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
