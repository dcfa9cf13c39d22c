"""Exact k-nearest-neighbour ground truth on one MI355X (rq_dataset_knn): n = 1e6 resident rows, d = 128
and 96, f32 and u8 bases, nq in {1000, 10000}, k in {1, 100, 1000}.

    python tools/knn_perf.py [--n 1000000] [--nq 1000 10000] [--k 1 100 1000] [--reps 3] [--skip-host] [--out profiles/knn_perf.json]

Per case, after a warm-up call: the wall clock of the whole call (median and spread of --reps) and the library's own phase clock
(rq_last_knn_timing: keys, select, fold, rerank, widen, upload of the queries, download); from them
  * the keys kernel as a fraction of the f32 vector rate of the guides (157.3 TFLOP/s counted as packed FMA, 4 flops per lane
    and issue slot: an unfused subtract, multiply, add per pair and dimension is 1.5 slots of packed f32, so the bound is
    1.5 n nq d / (157.3e12 / 4) s = 6 n nq d / 157.3e12 s),
  * the key write (8 bytes per pair) against the 6.29 TB/s copy rate,
  * the select chain's share of the call, the f64 candidates per query and the number of widened queries.
Yardsticks, interleaved with the new call in the same process (never the code under test against itself):
  (a) torch.cdist + torch.topk on the same resident tensors, queries in chunks of 1000 -- float32 and not exact: the queries
      whose id list differs from the exact one are counted and reported;
  (b) a numpy float64 brute force ((X - q)^2 summed per row, argpartition + lexsort) on 64 queries, scaled to nq."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_FMA_TFLOPS = 157.3
COPY_TBS = 6.29


def _wall(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def _spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def _cdist_topk(Xt, Qt, k):
    import torch
    ids = []
    for q0 in range(0, Qt.shape[0], 1000):
        D = torch.cdist(Qt[q0:q0 + 1000], Xt)
        ids.append(torch.topk(D, k, dim=1, largest=False).indices)
    torch.cuda.synchronize()
    return torch.cat(ids)


def _numpy_f64(X, Q, k):
    X64 = X.astype(np.float64)
    out = np.empty((Q.shape[0], k), dtype=np.int64)
    for q in range(Q.shape[0]):
        dist = ((X64 - Q[q].astype(np.float64)) ** 2).sum(axis=1)
        part = np.argpartition(dist, k - 1)[:k] if k < dist.size else np.arange(dist.size)
        out[q] = part[np.lexsort((part, dist[part]))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--d", type=int, nargs="+", default=[128, 96])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true", help="leave out the numpy float64 yardstick (minutes of CPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_perf.json"))
    args = ap.parse_args()

    import torch
    import rayuela_jl_amd as rq
    from rayuela_jl_amd import synth

    assert torch.cuda.is_available(), "knn_perf needs an MI355X"
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "library": rq.lib().rq_version().decode(), "n": args.n, "cases": []}
    for d in args.d:
        Xf = synth.sift_like(args.n, d, seed=1234) if d == 128 else synth.deep_like(args.n, d, seed=1234)
        Xu = synth.sift_like(args.n, d, seed=1234).astype(np.uint8)
        nq_max = max(args.nq)
        Qf = synth.sift_like(nq_max, d, seed=4321) if d == 128 else synth.deep_like(nq_max, d, seed=4321)
        Qu = synth.sift_like(nq_max, d, seed=4321)
        host = None
        if not args.skip_host:
            ms = [_wall(lambda: _numpy_f64(Xf, Qf[:64], 100))[0] for _ in range(2)]
            host = {"queries": 64, "k": 100, **_spread(ms)}
        for kind, X, Qall in (("f32", Xf, Qf), ("u8", Xu, Qu)):
            Xt = torch.from_numpy(X.astype(np.float32)).cuda()
            with rq.Dataset(X) as ds:
                for nq in args.nq:
                    Q = np.ascontiguousarray(Qall[:nq])
                    Qt = torch.from_numpy(Q).cuda()
                    for k in args.k:
                        ds.knn(Q, k)                      # warm-up: scratch grown, kernels loaded
                        _cdist_topk(Xt, Qt, k)
                        new, yard, phases, stats = [], [], [], None
                        for _ in range(args.reps):        # interleaved
                            ms, (dists, ids) = _wall(lambda: ds.knn(Q, k))
                            new.append(ms)
                            phases.append(rq.last_knn_timing())
                            stats = rq.last_knn_stats()
                            ms, tid = _wall(lambda: _cdist_topk(Xt, Qt, k))
                            yard.append(ms)
                        ph = {key: statistics.median(p[key] for p in phases) for key in phases[0]}
                        total = statistics.median(new)
                        pairs = float(args.n) * nq
                        keys_bound_ms = 6.0 * pairs * d / (VALU_FMA_TFLOPS * 1e12) * 1e3
                        write_bound_ms = 8.0 * pairs / (COPY_TBS * 1e12) * 1e3
                        mism = int((tid.cpu().numpy() != ids.astype(np.int64)).any(axis=1).sum())
                        case = {"base": kind, "d": d, "nq": nq, "k": k, "call": _spread(new), "phases_ms": ph,
                                "keys_fraction_of_valu_rate": keys_bound_ms / ph["keys_ms"] if ph["keys_ms"] > 0 else None,
                                "key_write_fraction_of_copy_rate": write_bound_ms / ph["keys_ms"] if ph["keys_ms"] > 0 else None,
                                "select_share": (ph["select_ms"] + ph["fold_ms"]) / total,
                                "f64_candidates_per_query": stats["candidates"] / float(nq),
                                "widened_queries": stats["widened"], "host_finished": stats["host_finished"],
                                "chunks": stats["chunks"],
                                "cdist_topk": {**_spread(yard), "queries_with_other_ids": mism},
                                "ratio_cdist_over_new": statistics.median(yard) / total}
                        if host is not None:
                            case["numpy_f64_scaled_ms"] = host["median_ms"] * nq / 64.0
                        res["cases"].append(case)
                        print(json.dumps(case), flush=True)
            del Xt
        if host is not None:
            res.setdefault("numpy_f64", {})[str(d)] = host
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
