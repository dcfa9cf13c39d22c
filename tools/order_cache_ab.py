#!/usr/bin/env python3
"""Same-box A/B of two library builds on the RAW-CODES scan call (rq_dev_linscan on resident codes, the call bench.py times) --
tools/ab_shard.py only times prepared bases.  Written for the kept in-call row order (csrc/rq_order.hip): the parent orders a scratch
copy in every call, the new build keeps it and checks it.

Each build runs in a fresh child process, alternating A B A B.  Shapes: SIFT1M shape (m = 8) at nq = 2048, 4096, 10000 and
k = 1, 100, 1000; Deep1M shape (m = 16) at nq = 10000, k = 1000.  The adversary: two buffers of different codes alternated call by
call (`adv_two_buffers`), and one buffer with a byte edited between calls (`adv_edited`; the edit itself is timed in both builds) --
what a caller whose codes really change pays for the check.  Then `python bench.py --steps 20 --warmup 5` itself, alternated the
same way; the acceptance rule is printed: the new build lower in every pairing and the mean gain at least three times the larger
of the two builds' own max - min spread.  Every child runs under its own time limit and the first failure ends the run.
usage: python tools/order_cache_ab.py libParent.so libNew.so [rounds] [--no-bench] [--no-shapes]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys, json, numpy as np, torch
sys.path.insert(0, os.getcwd())
import rayuela_jl_amd.synth as synth
from rayuela_jl_amd import device as rqd
dev = torch.device("cuda", 0)
def bench(fn, iters, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters
out = {}
n = 1_000_000
for m, shapes in ((8, [(nq, K) for nq in (2048, 4096, 10000) for K in (1, 100, 1000)]), (16, [(10000, 1000)])):
    sub = 128 // m if m == 8 else 96 // m
    rng = np.random.default_rng(m)
    centers = torch.from_numpy(rng.standard_normal((m, 256, sub)).astype(np.float32)).to(dev)
    Qall = torch.from_numpy(rng.standard_normal((10000, m * sub)).astype(np.float32)).to(dev)
    codes = torch.from_numpy(synth.random_codes(n, m, seed=100 + m)).to(dev)
    for nq, K in shapes:
        Q = Qall[:nq].contiguous()
        o = (torch.empty((nq, K), dtype=torch.float32, device=dev), torch.empty((nq, K), dtype=torch.int32, device=dev))
        out["m%d_nq%d_k%d" % (m, nq, K)] = bench(lambda: rqd.linscan(codes, centers, Q, K, out=o), 10)
    if m == 8:
        nq, K = 10000, 1000
        other = torch.from_numpy(synth.random_codes(n, m, seed=200)).to(dev)
        state = [0]
        def two():
            state[0] ^= 1
            rqd.linscan(other if state[0] else codes, centers, Qall, K, out=o)
        out["adv_two_buffers"] = bench(two, 10)
        def edited():
            state[0] += 1
            codes[(state[0] * 7919) % n, state[0] % m] += 1
            rqd.linscan(codes, centers, Qall, K, out=o)
        out["adv_edited"] = bench(edited, 10)
print("RESULT " + json.dumps(out))
'''


def run(cmd, lib, limit):
    env = dict(os.environ, RAYUELA_HIP_LIB=os.path.abspath(lib), RAYUELA_HIP_LENIENT="1")
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print("FAILED (status %d) %s\n%s" % (p.returncode, lib, p.stderr[-800:]), flush=True)
        sys.exit(1)                     # nothing more is started on the GPU after a failure
    return p.stdout


def find(js, key):
    """the first value of `key` anywhere in bench.py's result"""
    if isinstance(js, dict):
        if key in js:
            return js[key]
        js = list(js.values())
    if isinstance(js, list):
        for v in js:
            r = find(v, key)
            if r is not None:
                return r
    return None


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    libs = [a for a in args if a.endswith(".so")]
    assert len(libs) == 2, __doc__
    rounds = int(args[-1]) if not args[-1].endswith(".so") else 3
    names = ["parent", "new"]
    if "--no-shapes" not in sys.argv:
        res = {l: [] for l in libs}
        for r in range(rounds):
            for l, nm in zip(libs, names):
                line = [x for x in run([sys.executable, "-c", CHILD], l, 300).splitlines() if x.startswith("RESULT ")]
                res[l].append(json.loads(line[0][7:]))
                print(nm, json.dumps({k: round(v, 4) for k, v in res[l][-1].items()}), flush=True)
        print()
        for k in res[libs[0]][0]:
            a, b = [x[k] for x in res[libs[0]]], [x[k] for x in res[libs[1]]]
            print("%-22s parent mean %.4f (spread %.4f)   new mean %.4f (spread %.4f)   gain %+.4f ms" %
                  (k, sum(a) / len(a), max(a) - min(a), sum(b) / len(b), max(b) - min(b), sum(a) / len(a) - sum(b) / len(b)), flush=True)
    if "--no-bench" in sys.argv:
        return
    ms = {l: [] for l in libs}
    prep = {l: [] for l in libs}
    for r in range(rounds):
        for l, nm in zip(libs, names):
            out = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu", "--no-host"], l, 420)
            js = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
            ms[l].append(js["ms_per_step"])
            prep[l].append(find(js, "prepared_ms_per_step"))
            print("bench.py %-6s ms_per_step %.4f   prepared %s" % (nm, ms[l][-1], prep[l][-1]), flush=True)
    a, b = ms[libs[0]], ms[libs[1]]
    gain = sum(a) / len(a) - sum(b) / len(b)
    spread = max(max(a) - min(a), max(b) - min(b))
    every = all(y < x for x, y in zip(a, b))
    print("\nbench.py headline: parent %s  new %s" % (a, b))
    print("mean gain %.4f ms (%.2f %%), larger spread %.4f ms, new lower in every pairing: %s -> %s" %
          (gain, 100 * gain / (sum(a) / len(a)), spread, every, "ACCEPT" if every and gain >= 3 * spread else "REJECT"))


if __name__ == "__main__":
    main()
