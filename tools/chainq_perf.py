"""Chain quantization throughput on one MI355X (rq_dev_quantize_chainq / rq_dev_update_codebooks_chain / rq_train_chainq,
DESIGN.md section 4.11) at the SIFT1M (d = 128, m = 8) and Deep1M (d = 96, m = 16) shapes, n = 1e6, h = 256.

    python tools/chainq_perf.py [--n 1000000] [--skip-cpu] [--cpu-rows 2048] [--out chainq_perf.json]

Per shape, after a warm-up call: the device entry's whole encode and whole chain update on resident tensors timed with
torch events (best of 3), the encode's phases from the host entry's phase clock (hipEvents between tables, unaries and
forward + back trace; rq_last_chainq_timing), the forward pass's add + min operations against the chip's plain VALU lane
rate, one train_chainq round (niter = 1 minus niter = 0) by phase, and the numpy restatement of the Viterbi
(tests/chain_oracle.py) on a row subset, scaled to n rows, as the CPU figure."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LANE_OPS_PER_S = 3.9e13      # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz: one plain f32 VALU operation per lane and clock


def _best(fn, reps=3):
    import torch
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def run(n, d, m, h, skip_cpu, cpu_rows, seed=1):
    import torch
    from rayuela_jl_amd import device
    from rayuela_jl_amd.ChainQ import quantize_chainq_u8, train_chainq_u8, last_chainq_timing
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    tX, tc = torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda()
    out = {"n": n, "d": d, "m": m, "h": h}
    tC = device.update_codebooks_chain(tX, tc, h)            # warm-up; chain-structured codebooks for the encode
    device.quantize_chainq(tX, tC)
    torch.cuda.synchronize()
    out["update_ms"] = round(_best(lambda: device.update_codebooks_chain(tX, tc, h)), 3)
    out["quantize_ms"] = round(_best(lambda: device.quantize_chainq(tX, tC)), 3)
    C = tC.cpu().numpy()
    phases = None
    for _ in range(2):
        quantize_chainq_u8(X, C)
        ph = last_chainq_timing()
        if phases is None or sum(ph.values()) < sum(phases.values()):
            phases = ph
    out["unary_ms"] = round(phases["unary_ms"], 3)
    out["tables_ms"] = round(phases["tables_ms"], 3)
    out["viterbi_ms"] = round(phases["viterbi_ms"], 3)
    ops = 2.0 * n * (m - 1) * h * h                          # one add and one min per (row, stage, b, a)
    out["viterbi_share_of_plain_valu"] = round(ops / (phases["viterbi_ms"] * 1e-3) / LANE_OPS_PER_S, 3)
    tt = {}
    R = np.eye(d, dtype=np.float32)
    train_chainq_u8(X, codes, m, h, R, 0)                    # warm-up: the training loop's buffers and scratch
    for niter in (0, 1):
        t = time.perf_counter()
        train_chainq_u8(X, codes, m, h, R, niter)
        tt[niter] = ((time.perf_counter() - t) * 1e3, last_chainq_timing())
    out["train_round_wall_ms"] = round(tt[1][0] - tt[0][0], 1)
    out["train_round_ms"] = {k: round(tt[1][1][k] - tt[0][1][k], 3) for k in tt[0][1]}
    if not skip_cpu:
        import chain_oracle as co
        from oracle import oracle
        oracle.lib()
        rows = min(cpu_rows, n)
        U, T = co.tables(oracle, X[:rows], C)
        t = time.perf_counter()
        got = co.viterbi_tables(U, T)
        dt = time.perf_counter() - t
        out["numpy_viterbi_rows"] = rows
        out["numpy_viterbi_s_scaled_to_n"] = round(dt * n / rows, 1)
        out["numpy_subset_equal"] = bool(np.array_equal(got, quantize_chainq_u8(X[:rows], C)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--cpu-rows", type=int, default=2048)
    ap.add_argument("--shapes", default="SIFT1M,Deep1M")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = []
    for shape, d, m in (("SIFT1M", 128, 8), ("Deep1M", 96, 16)):
        if shape not in a.shapes.split(","):
            continue
        r = dict(shape=shape, **run(a.n, d, m, 256, a.skip_cpu, a.cpu_rows))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
