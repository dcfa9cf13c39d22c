"""Adding to a loaded IVFADC base on one MI355X: what it costs to load a base in adds instead of one
build, from float and from byte rows, and what the carry of the loaded rows costs.  A report, not a gate.

    python tools/ivf_add_perf.py [--n 1000000] [--train 100000] [--niter 5] [--nlist 1024] [--reps 5] [--big 100000000]
                                 [--big-add 1000000] [--out profiles/ivf_add_perf.json]

Shape: n x 128 rows of synth.sift_like (integers in 0 .. 255, so the byte rows ARE the float rows), m = 8, residual codes.  Per
form (float32, uint8) three legs load the same base into a fresh handle: one build; 10 adds of n / 10; 100 adds of n / 100.  The
six legs run interleaved in ONE process after a warm-up of each, `reps` rounds; a leg's time is a host clock around its calls,
each of which ends in a device synchronise.  Kept per leg: the MEDIAN and max / min over the rounds; per add the library's own
split (hipEvents, rq_ivf_last_timing): uploads + assignment + encode, grouping, carry, placement, medians over the rounds.  The
carry's rate is the bytes it moves, 2 (4 + MP) per loaded row (read and written; MP = the tiled row width), over its time; the
copy rate DESIGN.md section 4.18 quotes stands beside it.  A ratio is recorded with the spread (max / min) of its yardstick,
without which it means nothing.  The loaded bases are compared once: every leg must give the build's lists() bit for bit.

--big N: N rows of random codes loaded through add_codes in pieces of 2^24, then ONE add of --big-add float rows: the carry at a
size where it matters.  0 skips it, and the report then says "not measured"."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("load_encode_ms", "load_group_ms", "load_carry_ms", "load_place_ms")
COPY_RATE_TBPS = 6.29
D, M, MP = 128, 8, 8


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "spread": round(max(v) / min(v), 4)}


def _load(rq, Q, C, X, pieces):
    """A fresh handle loaded with X in `pieces` adds (1: one build).  Returns (index, total ms, [per call {loaded, ms, phases}])."""
    n = X.shape[0]
    step = n // pieces
    ix = rq.IvfIndex(Q, C, by_residual=True)
    calls, t_all = [], time.perf_counter()
    for r0 in range(0, n, step):
        t0 = time.perf_counter()
        if pieces == 1:
            ix.build(X)
        else:
            ix.add(X[r0:r0 + step])
        ms = (time.perf_counter() - t0) * 1e3
        inf = ix.info()
        calls.append(dict({"loaded": r0, "ms": ms}, **{p: inf[p] for p in PHASES}))
    return ix, (time.perf_counter() - t_all) * 1e3, calls


def _carry_rate(loaded, ms):
    return round(2 * (4 + MP) * loaded / (ms * 1e-3) / 1e9, 2) if ms > 0 and loaded else None


def main_legs(rq, synth, a):
    X = synth.sift_like(a.n, D, seed=1)
    X8 = X.astype(np.uint8)
    assert np.array_equal(X8.astype(np.float32), X)
    Q, C = rq.train_ivfpq(synth.sift_like(a.train, D, seed=2), a.nlist, M, niter=a.niter, seed=7, by_residual=True)
    forms = {"float": X, "bytes": X8}
    legs = {"%s_%s" % (f, name): (f, pieces) for name, pieces in (("build", 1), ("adds10", 10), ("adds100", 100)) for f in forms}
    want = None
    for key, (f, pieces) in legs.items():            # the warm-up, and the check that no leg changes the base
        ix, _, _ = _load(rq, Q, C, forms[f], pieces)
        got = ix.lists()
        ix.close()
        want = got if want is None else want
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), "%s loads another base than the build" % key
    total = {k: [] for k in legs}
    calls = {k: [] for k in legs}
    for _ in range(a.reps):
        for key, (f, pieces) in legs.items():
            ix, ms, cs = _load(rq, Q, C, forms[f], pieces)
            ix.close()
            total[key].append(ms)
            calls[key].append(cs)
    out = {"n": a.n, "d": D, "m": M, "nlist": a.nlist, "by_residual": True, "bases_equal": True, "legs": {}, "ratios": {}}
    for key in legs:
        per = []
        for i in range(len(calls[key][0])):
            row = {"loaded": calls[key][0][i]["loaded"], "ms": round(statistics.median(c[i]["ms"] for c in calls[key]), 4)}
            for p in PHASES:
                row[p] = round(statistics.median(c[i][p] for c in calls[key]), 4)
            row["carry_GBps"] = _carry_rate(row["loaded"], row["load_carry_ms"])
            per.append(row)
        out["legs"][key] = dict(_stats(total[key]), calls=len(per), per_call=per,
                                phase_sum_ms={p: round(sum(r[p] for r in per), 4) for p in PHASES})
    for f in forms:                                   # adds against the one build of the same form: the build is the yardstick
        for name in ("adds10", "adds100"):
            out["ratios"]["%s_%s_over_build" % (f, name)] = {
                "ratio": round(out["legs"]["%s_%s" % (f, name)]["median_ms"] / out["legs"][f + "_build"]["median_ms"], 4),
                "yardstick": f + "_build", "yardstick_spread": out["legs"][f + "_build"]["spread"]}
    for name in ("build", "adds10", "adds100"):       # byte rows against float rows: the float leg is the yardstick
        out["ratios"]["bytes_over_float_" + name] = {
            "ratio": round(out["legs"]["bytes_" + name]["median_ms"] / out["legs"]["float_" + name]["median_ms"], 4),
            "yardstick": "float_" + name, "yardstick_spread": out["legs"]["float_" + name]["spread"]}
    return out, (Q, C, X)


def big_leg(rq, Q, C, X, a):
    """a.big rows of random codes behind one another through add_codes, then one add of a.big_add float rows"""
    rng = np.random.default_rng(3)
    piece = 1 << 24
    out = {"loaded_rows": a.big, "add_rows": a.big_add, "load_calls": []}
    with rq.IvfIndex(Q, C, by_residual=True) as ix:
        for r0 in range(0, a.big, piece):
            nr = min(piece, a.big - r0)
            lists = rng.integers(0, a.nlist, nr, dtype=np.uint32)
            codes = rng.integers(0, 256, (nr, M), dtype=np.uint8)
            t0 = time.perf_counter()
            ix.add_codes(lists, codes)
            inf = ix.info()
            out["load_calls"].append(dict({"loaded": r0, "ms": round((time.perf_counter() - t0) * 1e3, 3),
                                           "carry_GBps": _carry_rate(r0, inf["load_carry_ms"])},
                                          **{p: round(inf[p], 4) for p in PHASES}))
            print(json.dumps(out["load_calls"][-1]), flush=True)
        adds = []
        for r in range(a.reps):                        # each add finds `loaded` rows more than the one before: the carry grows by 1 %
            t0 = time.perf_counter()
            ix.add(X[:a.big_add])
            inf = ix.info()
            adds.append(dict({"loaded": a.big + r * a.big_add, "ms": round((time.perf_counter() - t0) * 1e3, 3),
                              "carry_GBps": _carry_rate(a.big + r * a.big_add, inf["load_carry_ms"])},
                             **{p: round(inf[p], 4) for p in PHASES}))
        out["adds"] = adds
        out["carry_GBps"] = _stats([x["carry_GBps"] for x in adds[1:] or adds])
        out["carry_GBps"] = {k.replace("_ms", ""): v for k, v in out["carry_GBps"].items()}
        out["carry_over_quoted_copy_rate"] = round(out["carry_GBps"]["median"] / (COPY_RATE_TBPS * 1e3), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--train", type=int, default=100_000)
    ap.add_argument("--niter", type=int, default=5)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=100_000_000)
    ap.add_argument("--big-add", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_add_perf.json"))
    a = ap.parse_args()
    if a.n % 100:
        ap.error("--n must be a multiple of 100")
    import torch
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    if not torch.cuda.is_available():
        sys.exit("tools/ivf_add_perf.py measures on the GPU and found none")
    res = {"tool": "tools/ivf_add_perf.py", "library": _lib.lib().rq_version().decode(),
           "date": datetime.datetime.now(datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ"),
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "quoted_copy_rate_TBps": COPY_RATE_TBPS,
           "carry_bytes_per_loaded_row": 2 * (4 + MP), "big": "not measured"}

    def keep():
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:          # kept after every part: a run that is cut short leaves what it measured
            json.dump(res, f, indent=1)
            f.write("\n")

    res["million"], (Q, C, X) = main_legs(rq, synth, a)
    keep()
    print(json.dumps({k: {s: v[s] for s in ("median_ms", "spread")} for k, v in res["million"]["legs"].items()}), flush=True)
    print(json.dumps(res["million"]["ratios"]), flush=True)
    if a.big > 0:
        res["big"] = big_leg(rq, Q, C, X, a)
        keep()
        print(json.dumps({k: res["big"][k] for k in ("carry_GBps", "carry_over_quoted_copy_rate")}), flush=True)


if __name__ == "__main__":
    main()
