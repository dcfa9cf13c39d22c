"""LSQ++ training past 256 codewords on one MI355X (rq_train_sr_wide), host entries, phases from the
library's phase clock (hipEvents; rq_last_sr_timing).

    python tools/sr_wide_perf.py [--reps 3] [--quick] [--out profiles/sr_wide_perf.json]

One train_sr_cuda iteration in its steady state: a call with niter = 2 minus the same call with niter = 1.  The second iteration is
the first whose step opens with an update over the codes of the clean update before it, so the difference holds exactly one
repeated update, one clean update, one encode and one obj pass.  n = 1e5, d = 128, ilsiter = 8, icmiter = npert = 4, randord,
schedule 1.

Legs, interleaved in one process (every repetition runs every leg once, in turn) after one warm-up run per leg; per figure the
median and the spread (min, max) over the repetitions:
  sr         (m, h) = (8, 1024), (16, 1024), (4, 4096) x SR_C, SR_D x flags = 0 beside RQ_SR_RECOMPUTE; the counts of
             rq_last_sr_stats beside the phases
  lsq        one rq_train_lsq_wide iteration at the same shapes (niter = 1 minus niter = 0)
  yardstick  rq_train_sr at (8, 256) beside the wide entry (flags = 0 and RQ_SR_RECOMPUTE) at the same shape and inputs
Per (shape, method) the script also reports recompute minus flags = 0 per iteration: for SR_D that is one whole update, for SR_C
the update's factorisation and code-only part, which leaves the b sum and the two substitution sweeps -- the split of the solve
nobody had measured.  The yardstick of every figure is the recompute leg of the same run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ILS, ICM, NPERT = 8, 4, 4


def _stat(vals):
    v = sorted(float(x) for x in vals)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


class Inputs:
    def __init__(self, n, d, m, h, seed):
        rng = np.random.default_rng(seed)
        self.n, self.d, self.m, self.h = n, d, m, h
        self.X = rng.standard_normal((n, d)).astype(np.float32)
        self.codes = rng.integers(0, h, size=(n, m)).astype(np.int16)


class SrLeg:
    """entry: "wide" (rq_train_sr_wide) or "byte" (rq_train_sr)"""

    def __init__(self, inp, method, entry, recompute):
        self.inp, self.method, self.entry, self.recompute = inp, method, entry, recompute
        self.name = "sr %s (%d, %d) %s%s" % (method, inp.m, inp.h, entry, " recompute" if recompute else "")
        self.runs = []

    def _call(self, niter):
        from rayuela_jl_amd.SR import last_sr_stats, last_sr_timing, train_sr_u8, train_sr_u16
        i = self.inp
        if self.entry == "byte":
            train_sr_u8(i.X, i.codes.astype(np.uint8), i.m, i.h, None, niter, ILS, ICM, True, NPERT, self.method, 1, 0.5, True, seed=1)
        else:
            train_sr_u16(i.X, i.codes, i.m, i.h, None, niter, ILS, ICM, True, NPERT, self.method, 1, 0.5, True, seed=1,
                         recompute=self.recompute)
        return last_sr_timing(), last_sr_stats()

    def run(self, keep=True):
        (t1, s1), (t2, s2) = self._call(1), self._call(2)
        if keep:
            r = {k: t2[k] - t1[k] for k in t1}
            r["iteration_ms"] = sum(r.values())
            r["stats"] = {k: s2[k] - s1[k] for k in s1}
            self.runs.append(r)

    def report(self):
        i = self.inp
        out = {"leg": self.name, "entry": "rq_train_sr" if self.entry == "byte" else "rq_train_sr_wide", "method": self.method,
               "flags": "RQ_SR_RECOMPUTE" if self.recompute else "0", "n": i.n, "d": i.d, "m": i.m, "h": i.h, "mh": i.m * i.h,
               "updates_per_iteration": self.runs[0]["stats"]}
        for k in self.runs[0]:
            if k != "stats":
                out[k] = _stat(r[k] for r in self.runs)
        return out


class LsqLeg:
    def __init__(self, inp):
        self.inp = inp
        self.name = "lsq (%d, %d)" % (inp.m, inp.h)
        self.runs = []

    def run(self, keep=True):
        from rayuela_jl_amd.LSQ import last_lsq_timing, train_lsq_u16
        i, tt = self.inp, {}
        for niter in (0, 1):
            train_lsq_u16(i.X, i.codes, i.m, i.h, None, niter, ILS, ICM, True, NPERT, seed=1)
            tt[niter] = last_lsq_timing()
        if keep:
            r = {k: tt[1][k] - tt[0][k] for k in tt[0]}
            upd = sum(r[k] for k in ("count_ms", "sort_ms", "b_ms", "assemble_ms", "solve_ms"))
            self.runs.append({"update_ms": upd, "encode_ms": r["encode_ms"], "other_ms": r["other_ms"],
                              "iteration_ms": upd + r["encode_ms"] + r["other_ms"]})

    def report(self):
        i = self.inp
        out = {"leg": self.name, "entry": "rq_train_lsq_wide", "n": i.n, "d": i.d, "m": i.m, "h": i.h, "mh": i.m * i.h}
        for k in self.runs[0]:
            out[k] = _stat(r[k] for r in self.runs)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="n / 10 and no mh = 16384 shape: a rehearsal, not a measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rayuela_jl_amd as rq
    if rq.lib().rq_device_count() <= 0:
        raise SystemExit("sr_wide_perf: no MI355X visible; nothing is measured on a CPU")
    n, d = (10_000 if a.quick else 100_000), 128
    shapes = [(8, 1024), (4, 4096)] if a.quick else [(8, 1024), (16, 1024), (4, 4096)]
    legs, pairs = [], []
    for s, (m, h) in enumerate(shapes):
        inp = Inputs(n, d, m, h, s + 1)
        for method in ("SR_C", "SR_D"):
            lean, full = SrLeg(inp, method, "wide", False), SrLeg(inp, method, "wide", True)
            legs += [lean, full]
            pairs.append((lean, full))
        legs.append(LsqLeg(inp))
    small = Inputs(n, d, 8, 256, 9)
    for method in ("SR_C", "SR_D"):
        legs += [SrLeg(small, method, "byte", False), SrLeg(small, method, "wide", False), SrLeg(small, method, "wide", True)]
    for leg in legs:                       # warm-up: code objects, the scratch slots at their final sizes
        leg.run(keep=False)
    for _ in range(a.reps):
        for leg in legs:
            leg.run()
    res = {"tool": "tools/sr_wide_perf.py", "version": rq.lib().rq_version().decode(), "reps": a.reps, "quick": bool(a.quick),
           "ilsiter": ILS, "icmiter": ICM, "npert": NPERT, "legs": [leg.report() for leg in legs], "saved_per_iteration": []}
    for lean, full in pairs:
        spread = max(r["iteration_ms"] for r in full.runs) - min(r["iteration_ms"] for r in full.runs)
        saved = _stat(f["iteration_ms"] - l["iteration_ms"] for l, f in zip(lean.runs, full.runs))
        res["saved_per_iteration"].append({
            "method": lean.method, "m": lean.inp.m, "h": lean.inp.h,
            "update_ms_saved": _stat(f["update_ms"] - l["update_ms"] for l, f in zip(lean.runs, full.runs)),
            "iteration_ms_saved": saved, "recompute_iteration_spread_ms": round(spread, 3),
            "faster_by_more_than_the_spread": bool(saved["min"] > spread)})
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
