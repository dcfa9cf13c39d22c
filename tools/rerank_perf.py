"""Exact re-ranking of search candidates on one MI355X (rq_dataset_rerank / rq_ivf_search_refine).

    python tools/rerank_perf.py [--n 1000000] [--nq 1000 10000] [--kc 100 1000 4096 10000] [--rounds 5] [--skip-ivf]
                                [--out profiles/rerank_perf.json]

Part 1, n resident rows, d = 128 float32 and uint8 and d = 96 float32, k = kc / 10, candidates drawn uniformly over the base
(the access pattern of a search: no two candidates of a query share a cache line on purpose).  Legs, interleaved in one process,
medians of --rounds rounds with the min / max of each leg:
  * the whole call from host candidates (wall clock around Dataset.rerank),
  * its keys kernel and its select phase (the library's phase clock, rq_last_rerank_timing),
Yardsticks, never the code under test:
  * torch: gather of the candidate rows + squared difference + sum + topk on the same resident tensors, queries in chunks that keep
    the gathered block under 2 GiB (float32, not bit-exact: it is a speed yardstick only);
  * the gathered bytes (valid candidates x d x element size) over the 6.29 TB/s copy rate this project uses as its memory roof.
Part 2, the fused entry: synth.deep_like, nlist = 1024, m = 16, nprobe in {8, 32, 128}: IvfIndex.search at k = kc beside
search_refine(k = 100, kc) -- the added cost -- and recall@1 / 10 / 100 against knn.groundtruth with and without the refinement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29


def _wall(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def _spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def _torch_leg(Xt, Qt, Ct, k):
    """gather + squared difference + topk, queries in chunks; returns when the device has finished"""
    import torch
    nq, kc = Ct.shape
    d = Xt.shape[1]
    step = max(1, min(nq, (2 << 30) // (kc * d * 4)))
    for q0 in range(0, nq, step):
        rows = Xt[Ct[q0:q0 + step].reshape(-1)].reshape(-1, kc, d).float()
        dist = ((rows - Qt[q0:q0 + step, None, :]) ** 2).sum(dim=2)
        torch.topk(dist, k, dim=1, largest=False)
        del rows, dist
    torch.cuda.synchronize()


def part1(args, rq, out):
    import torch
    from rayuela_jl_amd import knn as K
    rng = np.random.default_rng(1)
    for d, kind in ((128, "f32"), (128, "u8"), (96, "f32")):
        if kind == "u8":
            X = rng.integers(0, 256, (args.n, d), dtype=np.uint8)
        else:
            X = rng.standard_normal((args.n, d), dtype=np.float32)
        Xt = torch.from_numpy(X).cuda()
        with rq.Dataset(X) as ds:
            for nq in args.nq:
                Q = rng.standard_normal((nq, d), dtype=np.float32) * (40 if kind == "u8" else 1) + (128 if kind == "u8" else 0)
                Qt = torch.from_numpy(Q).cuda()
                for kc in args.kc:
                    k = max(1, kc // 10)
                    cand = rng.integers(0, args.n, (nq, kc), dtype=np.int64).astype(np.uint32)
                    Ct = torch.from_numpy(cand.astype(np.int64)).cuda()
                    legs = {"call": [], "keys": [], "select": [], "torch": []}
                    ref = None
                    for rnd in range(args.rounds + 1):            # round 0 warms every leg up and is dropped
                        ms, got = _wall(lambda: ds.rerank(Q, cand, k, id_base=0))
                        t = K.last_rerank_timing()
                        ref = got if ref is None else ref
                        same = bool(np.array_equal(got[1], ref[1]) and np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)))
                        row = [("call", ms), ("keys", t["keys"]), ("select", t["select"])]
                        row.append(("torch", _wall(lambda: _torch_leg(Xt, Qt, Ct, k))[0]))
                        if not same:
                            raise SystemExit("two calls disagree at d=%d %s nq=%d kc=%d" % (d, kind, nq, kc))
                        if rnd:
                            for name, v in row:
                                legs[name].append(v)
                    gathered = nq * kc * d * X.itemsize
                    roof_ms = gathered / (COPY_TBS * 1e12) * 1e3
                    case = {"d": d, "base": kind, "n": args.n, "nq": nq, "kc": kc, "k": k, "gathered_bytes": gathered,
                            "roof_ms": roof_ms, "stats": K.last_rerank_stats(), "legs": {a: _spread(b) for a, b in legs.items()}}
                    case["share_of_gather_roof"] = roof_ms / statistics.median(legs["keys"])
                    out["rerank"].append(case)
                    print(json.dumps(case), flush=True)
                    del Ct
                del Qt
        del Xt
        torch.cuda.empty_cache()


def _recall(truth, ids):
    t = truth.astype(np.int64)[:, None]
    ids = ids.astype(np.int64)
    return {r: float((ids[:, :r] == t).any(axis=1).mean()) for r in (1, 10, 100) if r <= ids.shape[1]}


def part2(args, rq, out):
    import rayuela_jl_amd.synth as synth
    n, d, nq, m, nlist, k = args.n, 96, 1000, 16, 1024, 100
    Xb = synth.deep_like(n, d, seed=1)
    Xq = synth.deep_like(nq, d, seed=2)
    Q, C = rq.train_ivfpq(np.ascontiguousarray(Xb[:: max(1, n // 100000)]), nlist, m, niter=10, seed=0)
    truth = rq.groundtruth(Xb, Xq, 1)[0][:, 0]
    with rq.IvfIndex(Q, C) as ix, rq.Dataset(Xb) as ds:
        ix.build(Xb)
        for nprobe in (8, 32, 128):
            for kc in (100, 1000):
                legs = {"search_kc": [], "search_refine": []}
                for rnd in range(args.rounds + 1):
                    a, plain = _wall(lambda: ix.search(Xq, nprobe, kc))
                    b, fused = _wall(lambda: ix.search_refine(Xq, ds, nprobe, k, kc))
                    if rnd:
                        legs["search_kc"].append(a)
                        legs["search_refine"].append(b)
                case = {"n": n, "d": d, "m": m, "nlist": nlist, "nq": nq, "nprobe": nprobe, "kc": kc, "k": k,
                        "legs": {x: _spread(y) for x, y in legs.items()},
                        "recall_adc": _recall(truth, plain[1][:, :k]), "recall_refined": _recall(truth, fused[1])}
                case["added_ms"] = case["legs"]["search_refine"]["median_ms"] - case["legs"]["search_kc"]["median_ms"]
                out["ivf"].append(case)
                print(json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--kc", type=int, nargs="+", default=[100, 1000, 4096, 10000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-ivf", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_perf.json"))
    args = ap.parse_args()
    import torch
    import rayuela_jl_amd as rq
    if not torch.cuda.is_available():
        raise SystemExit("rerank_perf.py measures on the device; there is none here")
    out = {"device": torch.cuda.get_device_name(0), "version": rq.lib().rq_version().decode(), "copy_TBs": COPY_TBS,
           "rerank": [], "ivf": []}
    part1(args, rq, out)
    if not args.skip_ivf:
        part2(args, rq, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
