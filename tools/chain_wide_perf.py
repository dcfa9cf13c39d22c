"""Chain quantization past 256 codewords on one MI355X (rq_quantize_chainq_wide / rq_update_codebooks_chain_wide, DESIGN.md
section 4.26), host entries, phases from the library's phase clock (hipEvents; rq_last_chainq_timing).

    python tools/chain_wide_perf.py [--reps 3] [--quick] [--out profiles/chain_wide_perf.json]

n = 1e5 rows, d = 128, Gaussian X, Gaussian codebooks, uniform codes.  Legs, interleaved in one process (every repetition runs
every leg once, in turn) after one warm-up call per leg; per figure the median and the spread (min, max) over the repetitions:
  yardstick  rq_quantize_chainq at (m, h) = (8, 256) beside the wide entry at (8, 256), the same inputs: the ratio wide / byte
             per phase, with the byte kernel's own max / min spread.  Not a gate: the mirrors keep h <= 256 on the byte entries.
  encode     the wide entry at (8, 1024), (16, 1024), (4, 4096): unaries, tables, forward + back trace; the add + min operations
             of the forward pass (2 n (m - 1) h^2) against the chip's plain f32 VALU lane rate (the byte kernel reports 0.95 at
             h = 256), and the forward + back trace time against h^2 scaling from the wide entry at (8, 256).
  update     the wide update at the same three shapes: the whole update, and the solve's f64 work ((2h)^3 / 3 + 2 (2h)^2 len per
             block) as a rate over the whole update (the phase clock does not split the update; the solve is what grows)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANE_OPS_PER_S = 3.9e13      # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz: one plain f32 VALU operation per lane and clock (tools/chainq_perf.py)
ENC_KEYS = ("unary_ms", "tables_ms", "viterbi_ms")


def _stat(vals):
    v = sorted(float(x) for x in vals)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


class EncodeLeg:
    def __init__(self, name, n, d, m, h, wide, seed):
        rng = np.random.default_rng(seed)
        self.name, self.n, self.d, self.m, self.h, self.wide = name, n, d, m, h, wide
        self.X = rng.standard_normal((n, d)).astype(np.float32)
        self.C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
        self.runs = []

    def run(self, keep=True):
        from rayuela_jl_amd.ChainQ import last_chainq_timing, quantize_chainq_u8, quantize_chainq_u16
        t = time.perf_counter()
        (quantize_chainq_u16 if self.wide else quantize_chainq_u8)(self.X, self.C)
        wall = (time.perf_counter() - t) * 1e3
        if keep:
            self.runs.append(dict(last_chainq_timing(), wall_ms=wall))

    def report(self):
        ops = 2.0 * self.n * (self.m - 1) * self.h * self.h          # one add and one min per (row, stage, b, a)
        return {"leg": self.name, "entry": "rq_quantize_chainq_wide" if self.wide else "rq_quantize_chainq", "n": self.n, "d": self.d,
                "m": self.m, "h": self.h, "phases_ms": {k: _stat(r[k] for r in self.runs) for k in ENC_KEYS},
                "encode_ms": _stat(sum(r[k] for k in ENC_KEYS) for r in self.runs),
                "host_call_ms": _stat(r["wall_ms"] for r in self.runs),
                "viterbi_share_of_plain_valu": _stat(ops / (r["viterbi_ms"] * 1e-3) / LANE_OPS_PER_S for r in self.runs)}


class UpdateLeg:
    def __init__(self, name, n, d, m, h, seed):
        rng = np.random.default_rng(seed)
        self.name, self.n, self.d, self.m, self.h = name, n, d, m, h
        self.X = rng.standard_normal((n, d)).astype(np.float32)
        self.codes = rng.integers(0, h, size=(n, m)).astype(np.int16)
        self.runs = []

    def run(self, keep=True):
        from rayuela_jl_amd.ChainQ import last_chainq_timing
        from rayuela_jl_amd.codebook_update import update_codebooks_chain_bin_u16
        t = time.perf_counter()
        update_codebooks_chain_bin_u16(self.X, self.codes, self.h)
        wall = (time.perf_counter() - t) * 1e3
        if keep:
            self.runs.append(dict(last_chainq_timing(), wall_ms=wall))

    def report(self):
        from rayuela_jl_amd.utils import splitarray
        h2 = 2 * self.h
        parts = [len(p) for p in splitarray(range(self.d), self.m - 1)]
        flops = sum(h2 ** 3 / 3 + 2 * h2 ** 2 * ln for ln in parts)
        steps = (self.m - 1) * -(-h2 // 64)
        return {"leg": self.name, "entry": "rq_update_codebooks_chain_wide", "n": self.n, "d": self.d, "m": self.m, "h": self.h,
                "blocks": self.m - 1, "block_bytes": h2 * h2 * 8, "cholesky_block_steps": steps,
                "update_ms": _stat(r["update_ms"] for r in self.runs), "host_call_ms": _stat(r["wall_ms"] for r in self.runs),
                "update_ms_per_block_step": _stat(r["update_ms"] / steps for r in self.runs),
                "solve_f64_TFLOPs_over_update": _stat(flops / (r["update_ms"] * 1e-3) / 1e12 for r in self.runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="n / 10 and no h = 4096 leg: a rehearsal, not a measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rayuela_jl_amd as rq
    if rq.lib().rq_device_count() <= 0:
        raise SystemExit("chain_wide_perf: no MI355X visible; nothing is measured on a CPU")
    n = 100_000 // (10 if a.quick else 1)
    d = 128
    shapes = [(8, 1024), (16, 1024)] + ([] if a.quick else [(4, 4096)])
    byte = EncodeLeg("yardstick byte (8, 256)", n, d, 8, 256, False, 1)
    wide = EncodeLeg("yardstick wide (8, 256)", n, d, 8, 256, True, 1)
    enc = [EncodeLeg("encode (%d, %d)" % s, n, d, s[0], s[1], True, 2 + k) for k, s in enumerate(shapes)]
    upd = [UpdateLeg("update (%d, %d)" % s, n, d, s[0], s[1], 10 + k) for k, s in enumerate(shapes)]
    legs = [byte, wide] + enc + upd
    for leg in legs:                       # warm-up: code objects, the scratch slots at their final sizes
        leg.run(keep=False)
    for _ in range(a.reps):
        for leg in legs:
            leg.run()
    res = {"tool": "tools/chain_wide_perf.py", "version": rq.lib().rq_version().decode(), "reps": a.reps, "quick": bool(a.quick),
           "legs": [leg.report() for leg in legs]}
    res["yardstick_wide_over_byte"] = {k: _stat(w[k] / b[k] for w, b in zip(wide.runs, byte.runs) if b[k] > 0) for k in ENC_KEYS}
    res["yardstick_wide_over_byte"]["encode_ms"] = _stat(
        sum(w[k] for k in ENC_KEYS) / sum(b[k] for k in ENC_KEYS) for w, b in zip(wide.runs, byte.runs))
    res["yardstick_byte_spread_max_over_min"] = {
        k: round(max(r[k] for r in byte.runs) / min(r[k] for r in byte.runs), 4) for k in ENC_KEYS}
    # forward + back trace against h^2 (and m - 1) scaling from the wide entry at (8, 256)
    base = sorted(r["viterbi_ms"] for r in wide.runs)[len(wide.runs) // 2]
    res["viterbi_over_h2_scaling_from_256"] = {
        leg.name: _stat(r["viterbi_ms"] / (base * (leg.m - 1) / 7.0 * (leg.h / 256.0) ** 2) for r in leg.runs) for leg in enc}
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
