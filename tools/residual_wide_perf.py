"""The residual quantizers past 256 codewords per stage on one MI355X: beam-search encoding
(rq_dev_encode_rvq_beam_wide) and one ERVQ iteration (rq_train_ervq_wide) at d = 128, m = 4, h = 1024 and 4096.

    python tools/residual_wide_perf.py [--n 1000000] [--hs 1024,4096] [--beams 1,4,16,32] [--out profiles/residual_wide_perf.json]

One process; SIFT-like rows generated on the device, codebooks from train_rvq on the first 100 000 rows.  Every leg is warmed
up once, then all legs of a section are timed in interleaved rounds (leg A, leg B, ..., leg A, ...) with device events; a leg
reports the minimum and the max / min spread of its rounds.

  beam      per h and H: the whole rq_dev_encode_rvq_beam_wide call and its phases (rq_last_beam_timing of the fastest round).
            Yardstick of H = 1: rq_dev_encode_rvq_wide (the greedy wide encoder) on the same rows.
  scaling   the byte kernel (rq_dev_encode_rvq_beam, h = 256) next to the wide kernel at h = 512, per H: twice the codewords.
  ervq      one rq_train_ervq_wide iteration on a host copy of the rows, by phase (rq_last_ervq_timing).  Yardstick: the sum of
            its parts called alone on resident rows -- m (m + 1) / 2 stage encodes (rq_dev_encode_rvq_wide with m = 1) and m
            rq_dev_update_centers_wide calls with m = 1 -- against the encode + epilogue and the increment phases."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def interleaved(legs, rounds=3, after=None):
    """legs: {name: fn}.  One warm-up of every leg, then `rounds` rounds over all legs in order.  -> {name: {min_ms, spread}};
    after(name, ms) is called after every timed run."""
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t = _once(fn)
            ms[k].append(t)
            if after:
                after(k, t)
    return {k: {"min_ms": round(min(v), 3), "spread_max_over_min": round(max(v) / min(v), 3), "rounds_ms": [round(t, 3) for t in v]}
            for k, v in ms.items()}


def codebooks(X, m, h, train_rows):
    import torch
    import rayuela_jl_amd as rq
    C, _, _ = rq.train_rvq(X[:train_rows].cpu().numpy(), m, h, niter=2, seed=1)
    return torch.from_numpy(np.stack(C)).cuda()


def beam_section(X, tC, beams):
    import torch
    from rayuela_jl_amd import _lib, device as rqd
    L = _lib.lib()
    n, d = X.shape
    m, h, _ = tC.shape
    wide = h > 256
    codes = torch.empty((n, m), dtype=torch.int16 if wide else torch.uint8, device="cuda")
    Xr = X.clone()
    phases = {}

    def greedy():
        Xr.copy_(X)
        (rqd.encode_rvq_wide if wide else rqd.encode_rvq)(Xr, tC, out=codes)

    def copy_only():
        Xr.copy_(X)

    def beam(H):
        return lambda: (rqd.encode_rvq_beam_wide if wide else rqd.encode_rvq_beam)(X, tC, H, out=codes)

    def after(name, t):
        if name.startswith("beam_H"):
            p3 = (ctypes.c_double * 3)()
            _lib.check(L.rq_last_beam_timing(ctypes.cast(p3, ctypes.c_void_p), 3))
            if name not in phases or t < phases[name][0]:
                phases[name] = (t, [round(v, 3) for v in p3])

    legs = {"greedy_with_copy": greedy, "copy_of_X": copy_only}
    legs.update({"beam_H%d" % H: beam(H) for H in beams})
    res = interleaved(legs, after=after)
    out = {"n": n, "d": d, "m": m, "h": h, "entry": "rq_dev_encode_rvq_beam_wide" if wide else "rq_dev_encode_rvq_beam"}
    g = res["greedy_with_copy"]["min_ms"] - res["copy_of_X"]["min_ms"]
    out["greedy_ms"] = round(g, 3)
    out["greedy_spread_max_over_min"] = res["greedy_with_copy"]["spread_max_over_min"]
    out["legs"] = res
    for H in beams:
        r = res["beam_H%d" % H]
        r["stage_expand_other_ms"] = phases["beam_H%d" % H][1]
    out["H1_over_greedy"] = round(res["beam_H%d" % beams[0]]["min_ms"] / g, 3) if beams[0] == 1 else None
    greedy()
    g_codes = codes.clone()
    beam(1)()
    torch.cuda.synchronize()
    out["H1_codes_equal_greedy"] = bool(torch.equal(codes, g_codes))
    return out


def ervq_section(X, tC):
    import torch
    from rayuela_jl_amd import _lib, device as rqd
    from rayuela_jl_amd.ERVQ import train_ervq_i16, last_ervq_timing
    n, d = X.shape
    m, h, _ = tC.shape
    Xr = X.clone()
    codes = rqd.encode_rvq_wide(Xr, tC)
    Xh, Ch = X.cpu().numpy(), tC.cpu().numpy()
    B1 = (codes.cpu().numpy() + 1).astype(np.int16)
    best = None
    for _ in range(3):                                     # the first call also warms the code objects up
        train_ervq_i16(Xh, B1, Ch, m, h, 1, seed=0)
        ph = last_ervq_timing()
        if best is None or sum(ph.values()) < sum(best.values()):
            best = ph
    # the parts alone, interleaved: one stage encode (m = 1, with its epilogue) and one update_centers (m = 1, width d)
    stage = torch.empty((n, 1), dtype=torch.int16, device="cuda")
    C1 = tC[0].clone().reshape(1, h, d).contiguous()
    Cu = tC[0].clone().contiguous()
    col = codes[:, :1].contiguous()

    def stage_encode():
        rqd.encode_rvq_wide(Xr, C1, out=stage)             # in place on Xr: the values drift, the work does not

    def update():
        rqd.update_centers_wide(Cu, X, col, 1, h)

    parts = interleaved({"stage_encode_m1": stage_encode, "update_centers_m1": update})
    nenc = m * (m + 1) // 2
    yard_enc = nenc * parts["stage_encode_m1"]["min_ms"]
    yard_upd = m * parts["update_centers_m1"]["min_ms"]
    enc = best["encode_ms"] + best["epilogue_ms"]
    return {"n": n, "d": d, "m": m, "h": h, "iteration_phases_ms": {k: round(v, 3) for k, v in best.items()},
            "iteration_device_ms": round(sum(best.values()) - best["other_ms"], 3), "parts": parts,
            "stage_encodes_per_iteration": nenc,
            "yardstick_encode_ms": round(yard_enc, 3), "encode_plus_epilogue_ms": round(enc, 3),
            "encode_over_yardstick": round(enc / yard_enc, 3),
            "yardstick_update_ms": round(yard_upd, 3), "increment_ms": round(best["increment_ms"], 3),
            "increment_over_yardstick": round(best["increment_ms"] / yard_upd, 3),
            "sum_over_yardstick": round((enc + best["increment_ms"]) / (yard_enc + yard_upd), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--hs", default="1024,4096")
    ap.add_argument("--beams", default="1,4,16,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_wide_perf.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("residual_wide_perf needs an MI355X: no timing is taken without one")
    from rayuela_jl_amd import _lib, synth_torch
    beams = [int(b) for b in a.beams.split(",")]
    X = synth_torch.sift_like(a.n, a.d, seed=11).contiguous()
    train_rows = min(a.n, 100_000)
    res = {"device": torch.cuda.get_device_name(0), "library": _lib.lib().rq_version().decode(), "beam": [], "scaling": [], "ervq": []}

    def save():                                             # after every section: a partial file survives a time limit
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    for h in [int(v) for v in a.hs.split(",")]:
        tC = codebooks(X, a.m, h, train_rows)
        res["beam"].append(beam_section(X, tC, beams))
        print(json.dumps(res["beam"][-1]), flush=True)
        save()
        res["ervq"].append(ervq_section(X, tC))
        print(json.dumps(res["ervq"][-1]), flush=True)
        save()
        del tC
    for h in (256, 512):
        tC = codebooks(X, a.m, h, train_rows)
        res["scaling"].append(beam_section(X, tC, beams))
        print(json.dumps(res["scaling"][-1]), flush=True)
        save()
    b, w = res["scaling"]
    res["scaling_wide512_over_byte256"] = {k: round(w["legs"][k]["min_ms"] / b["legs"][k]["min_ms"], 3) for k in b["legs"] if k.startswith("beam_H")}
    save()


if __name__ == "__main__":
    main()
