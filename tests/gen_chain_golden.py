"""Writes tests/golden/chain_*.npz: chain encodes by the reference's own `viterbi_encoding`
(deps/src/encode_icm.cpp:63-152, compiled OUTSIDE this tree with the reference's flags, deps/build.jl:46:
g++ -O3 -shared -fPIC encode_icm.cpp -fopenmp), fed the restated tables of tests/chain_oracle.py.  Each file holds the
inputs X, C and the codes the reference returned; h = 256 (the reference is built for H = 256).

    python tests/gen_chain_golden.py /path/to/encode_icm_so.so
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import chain_oracle as co  # noqa: E402

H = 256
# name: (n, d, m, kind, seed)
CASES = {
    "chain_m4_gauss": (320, 32, 4, "chain", 1),
    "chain_m8_gauss": (256, 28, 8, "chain", 2),
    "chain_m5_uneven": (320, 30, 5, "chain", 3),
    "chain_m4_ties": (384, 12, 4, "ties", 4),
    "chain_m2": (384, 16, 2, "chain", 5),
    "chain_m4_dense": (320, 24, 4, "dense", 6),
}


def _case(n, d, m, kind, seed):
    rng = np.random.default_rng(200 + seed)
    if kind == "ties":      # integer values: many equal unaries, pair terms and path costs (as icm_m4_ties)
        C_ = rng.integers(-1, 2, size=(m, H, d)).astype(np.float32)
        X = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
        return X, C_
    C_ = (rng.standard_normal((m, H, d)) * 0.5).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    if kind == "chain":     # zero outside the chain dimensions, like a trained chain quantizer
        for i, dims in enumerate(co.cbdims(d, m)):
            mask = np.ones(d, dtype=bool)
            mask[dims[0]:dims[-1] + 1] = False
            C_[i][:, mask] = 0
    return X, C_


def main(path):
    from oracle import oracle
    lib = C.CDLL(path)
    lib.viterbi_encoding.restype = None
    lib.viterbi_encoding.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    for name, (n, d, m, kind, seed) in CASES.items():
        X, C_ = _case(n, d, m, kind, seed)
        U, T = co.tables(oracle, X, C_)
        un = np.ascontiguousarray(U.transpose(1, 0, 2))          # [row][codebook][H]
        bins = np.ascontiguousarray(T)                           # [i][b][a]: bb[j * H + k], j = b, k = a
        B = np.zeros((n, m), dtype=np.uint8)
        lib.viterbi_encoding(B.ctypes.data, un.ctypes.data, bins.ctypes.data, n, m)
        mine = co.viterbi_tables(U, T)
        np.savez_compressed(os.path.join(HERE, "golden", name + ".npz"), X=X, C=C_, codes=B)
        print(name, "rows where the restatement differs:", int((B != mine).any(axis=1).sum()), "of", n)


if __name__ == "__main__":
    main(sys.argv[1])
