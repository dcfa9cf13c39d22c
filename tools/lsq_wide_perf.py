"""The LSQ codebook update and training past 256 codewords on one MI355X (rq_update_codebooks_lsq_wide / rq_train_lsq_wide,
DESIGN.md section 4.25), host entries, phases from the library's phase clock (hipEvents; rq_last_lsq_timing).

    python tools/lsq_wide_perf.py [--reps 3] [--quick] [--out profiles/lsq_wide_perf.json]

Legs, interleaved in one process (every repetition runs every leg once, in turn) after one warm-up call per leg; per figure the
median and the spread (min, max) over the repetitions:
  phases     count / sort / b / assemble / solve of one update: n = 1e5 at (m, h) = (8, 1024), (16, 1024), (4, 4096), n = 1e6 at
             (8, 1024); d = 128.  Per leg also ms per 64-wide Cholesky block step (mh = 8192, 16384, 16384) and the f64 FLOP/s of
             the solve ((mh)^3 / 3 + 2 (mh)^2 d).
  iteration  one rq_train_lsq_wide iteration at (8, 1024), n = 1e5, ilsiter = 8 (icmiter = 4, npert = 4, randord): niter = 1 minus
             niter = 0, split into update, encode and other.
  yardstick  rq_update_codebooks_lsq against the wide entry at (8, 256), n = 1e6, the same inputs: the ratio wide / byte per phase.
             Not a gate: the mirrors keep h <= 256 on the byte entry whatever it shows."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UPDATE_KEYS = ("count_ms", "sort_ms", "b_ms", "assemble_ms", "solve_ms")


def _stat(vals):
    v = sorted(float(x) for x in vals)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


class UpdateLeg:
    def __init__(self, name, n, d, m, h, wide, seed):
        rng = np.random.default_rng(seed)
        self.name, self.n, self.d, self.m, self.h, self.wide = name, n, d, m, h, wide
        self.X = rng.standard_normal((n, d)).astype(np.float32)
        self.codes = rng.integers(0, h, size=(n, m)).astype(np.int16 if wide else np.uint8)
        self.runs = []

    def run(self, keep=True):
        from rayuela_jl_amd.codebook_update import update_codebooks_u8, update_codebooks_u16
        from rayuela_jl_amd.LSQ import last_lsq_timing
        t = time.perf_counter()
        (update_codebooks_u16 if self.wide else update_codebooks_u8)(self.X, self.codes, self.h)
        wall = (time.perf_counter() - t) * 1e3
        if keep:
            self.runs.append(dict(last_lsq_timing(), wall_ms=wall))

    def report(self):
        mh = self.m * self.h
        steps = -(-mh // 64)
        out = {"leg": self.name, "entry": "rq_update_codebooks_lsq_wide" if self.wide else "rq_update_codebooks_lsq", "n": self.n,
               "d": self.d, "m": self.m, "h": self.h, "mh": mh, "cholesky_block_steps": steps,
               "phases_ms": {k: _stat(r[k] for r in self.runs) for k in UPDATE_KEYS},
               "update_ms": _stat(sum(r[k] for k in UPDATE_KEYS) for r in self.runs),
               "host_call_ms": _stat(r["wall_ms"] for r in self.runs)}
        out["solve_ms_per_block_step"] = _stat(r["solve_ms"] / steps for r in self.runs)
        flops = mh ** 3 / 3 + 2 * mh ** 2 * self.d
        out["solve_f64_TFLOPs"] = _stat(flops / (r["solve_ms"] * 1e-3) / 1e12 for r in self.runs)
        out["b_GBps"] = _stat(self.m * self.n * self.d * 4 / (r["b_ms"] * 1e-3) / 1e9 for r in self.runs)
        return out


class IterationLeg:
    def __init__(self, name, n, d, m, h, seed):
        rng = np.random.default_rng(seed)
        self.name, self.n, self.d, self.m, self.h = name, n, d, m, h
        self.X = rng.standard_normal((n, d)).astype(np.float32)
        self.codes = rng.integers(0, h, size=(n, m)).astype(np.int16)
        self.runs = []

    def run(self, keep=True):
        from rayuela_jl_amd.LSQ import last_lsq_timing, train_lsq_u16
        tt = {}
        for niter in (0, 1):
            train_lsq_u16(self.X, self.codes, self.m, self.h, None, niter, 8, 4, True, 4, seed=1)
            tt[niter] = last_lsq_timing()
        if keep:
            self.runs.append({"update_ms": sum(tt[1][k] - tt[0][k] for k in UPDATE_KEYS),
                              "encode_ms": tt[1]["encode_ms"] - tt[0]["encode_ms"], "other_ms": tt[1]["other_ms"] - tt[0]["other_ms"]})

    def report(self):
        out = {"leg": self.name, "entry": "rq_train_lsq_wide", "n": self.n, "d": self.d, "m": self.m, "h": self.h, "ilsiter": 8,
               "icmiter": 4, "npert": 4}
        for k in ("update_ms", "encode_ms", "other_ms"):
            out["iteration_" + k] = _stat(r[k] for r in self.runs)
        out["update_share"] = _stat(r["update_ms"] / (r["update_ms"] + r["encode_ms"] + r["other_ms"]) for r in self.runs)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="n / 10 and no mh = 16384 leg: a rehearsal, not a measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rayuela_jl_amd as rq
    if rq.lib().rq_device_count() <= 0:
        raise SystemExit("lsq_wide_perf: no MI355X visible; nothing is measured on a CPU")
    q = 10 if a.quick else 1
    d = 128
    legs = [UpdateLeg("phases (8, 1024) n=1e5", 100_000 // q, d, 8, 1024, True, 1),
            UpdateLeg("phases (4, 4096) n=1e5", 100_000 // q, d, 4, 4096, True, 3),
            UpdateLeg("phases (8, 1024) n=1e6", 1_000_000 // q, d, 8, 1024, True, 4),
            IterationLeg("iteration (8, 1024) n=1e5", 100_000 // q, d, 8, 1024, 5),
            UpdateLeg("yardstick byte (8, 256) n=1e6", 1_000_000 // q, d, 8, 256, False, 6),
            UpdateLeg("yardstick wide (8, 256) n=1e6", 1_000_000 // q, d, 8, 256, True, 6)]
    if not a.quick:
        legs.insert(1, UpdateLeg("phases (16, 1024) n=1e5", 100_000, d, 16, 1024, True, 2))
    for leg in legs:                       # warm-up: code objects, the scratch slots at their final sizes
        leg.run(keep=False)
    for _ in range(a.reps):
        for leg in legs:
            leg.run()
    res = {"tool": "tools/lsq_wide_perf.py", "version": rq.lib().rq_version().decode(), "reps": a.reps, "quick": bool(a.quick),
           "legs": [leg.report() for leg in legs]}
    byte, wide = legs[-2], legs[-1]
    res["yardstick_wide_over_byte"] = {
        k: _stat(w[k] / b[k] for w, b in zip(wide.runs, byte.runs) if b[k] > 0) for k in UPDATE_KEYS}
    res["yardstick_wide_over_byte"]["update_ms"] = _stat(
        sum(w[k] for k in UPDATE_KEYS) / sum(b[k] for k in UPDATE_KEYS) for w, b in zip(wide.runs, byte.runs))
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
