"""Writes tests/golden/icm_*.npz: LSQ encodes whose every conditioning step is the reference's own `condition`
(deps/src/encode_icm.cpp:1-61, compiled OUTSIDE this tree with the reference's flags, deps/build.jl:46:
g++ -O3 -shared -fPIC encode_icm.cpp -fopenmp), driven by the restated ILS loop of tests/icm_oracle.py (tables,
random streams, veccost).  Run with OMP_NUM_THREADS=1: the reference shares k, binariidx and bb across its OpenMP team.

    OMP_NUM_THREADS=1 python tests/gen_icm_golden.py /path/to/encode_icm_so.so
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import icm_oracle as io  # noqa: E402

# name: (n, d, m, h, ilsiter, icmiter, npert, randord, seed, t0, kind)
CASES = {
    "icm_m4_plain": (256, 16, 4, 256, 3, 2, 0, False, 1, 0, "normal"),
    "icm_m4_rand_pert": (256, 16, 4, 256, 3, 2, 2, True, 2, 5, "normal"),
    "icm_m8_rand_pert": (192, 16, 8, 256, 3, 2, 2, True, 3, 0, "normal"),
    "icm_m8_plain_pert": (192, 16, 8, 256, 2, 3, 2, False, 4, 1, "normal"),
    "icm_m4_ties": (256, 12, 4, 256, 3, 2, 2, True, 5, 0, "ties"),
    "icm_m4_all_rejected": (128, 16, 4, 256, 3, 1, 4, True, 6, 0, "exact"),
}


def _case(n, d, m, h, kind, seed):
    rng = np.random.default_rng(100 + seed)
    if kind == "ties":     # integer values in -1..1: many equal unaries, binaries and costs
        C_ = rng.integers(-1, 2, size=(m, h, d)).astype(np.float32)
        X = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
        B0 = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    elif kind == "exact":  # X reconstructed exactly by B0 (cost 0): no perturbation can be strictly better
        C_ = rng.integers(-8, 9, size=(m, h, d)).astype(np.float32)
        B0 = rng.integers(0, h, size=(n, m)).astype(np.uint8)
        X = C_[np.arange(m)[None, :], B0.astype(np.int64)].sum(axis=1).astype(np.float32)
    else:
        C_ = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
        X = rng.standard_normal((n, d)).astype(np.float32)
        B0 = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    return X, C_, B0


def ref_condition(lib):
    """cond(B, U, binT, j) through the reference symbol: binaries[pair(a<b)] = BinT[a][b], binaries_t[pair] = BinT[b][a]."""
    def cond(B, U, binT, j):
        m = B.shape[1]
        h = binT.shape[2]
        assert h == 256, "the reference's condition is built for H = 256"
        pairs = [(a, b) for a in range(m) for b in range(a + 1, m)]
        idx = np.zeros((m, m), dtype=np.int32)
        for p, (a, b) in enumerate(pairs):
            idx[a, b] = idx[b, a] = p
        bins = np.ascontiguousarray(np.stack([binT[a, b] for a, b in pairs]) if pairs else np.zeros(1, np.float32))
        bins_t = np.ascontiguousarray(np.stack([binT[b, a] for a, b in pairs]) if pairs else np.zeros(1, np.float32))
        tocond = np.array([k for k in range(m) if k != j], dtype=np.int32)
        ub = np.ascontiguousarray(U[j], dtype=np.float32).copy()
        Bc = np.ascontiguousarray(B)
        lib.condition(Bc.ctypes.data, ub.ctypes.data, bins.ctypes.data, bins_t.ctypes.data, idx.ctypes.data,
                      tocond.ctypes.data, j, B.shape[0], m)
        B[...] = Bc
    return cond


def main(path):
    from oracle import oracle
    lib = C.CDLL(path)
    lib.condition.restype = None
    lib.condition.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3
    for name, (n, d, m, h, ils, icm, npert, randord, seed, t0, kind) in CASES.items():
        X, C_, B0 = _case(n, d, m, h, kind, seed)
        B, cost = io.ils(oracle, X, C_, B0, ils, icm, npert, randord, seed=seed, t0=t0, cond=ref_condition(lib))
        if kind == "exact":
            assert np.array_equal(B, B0), "a perturbation was accepted in the all-rejected case"
        np.savez_compressed(os.path.join(HERE, "golden", name + ".npz"), X=X, C=C_, B0=B0, codes=B, cost=cost,
                            params=np.array([ils, icm, npert, int(randord), seed, t0], dtype=np.int64))
        print(name, "rows changed:", int((B != B0).any(axis=1).sum()), "of", n)


if __name__ == "__main__":
    main(sys.argv[1])
