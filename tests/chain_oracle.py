"""CPU restatement of the chain quantization contract ("Chain quantization") -- test infrastructure.

  viterbi(oracle, X, C)          codes uint8 [n][m] zero-based: the Viterbi recursion over the unaries and the m-1
                                 adjacent-pair tables of the LSQ encoding contract (tests/icm_oracle.py), every add one
                                 numpy float32 add, np.argmin = the lowest index of the minimum (src/ChainQ.jl:305-348,
                                 deps/src/encode_icm.cpp:63-152)
  chain_update(X, codes, h)      the chain codebook update (src/codebook_update.jl:367-412): the normal equations of
                                 tests/lsq_update_oracle.py, np.linalg.solve per 2h x 2h block
  train(oracle, X, codes, R, h, niter)   the training loop (src/ChainQ.jl:373-431) with numpy's SVD
"""
import numpy as np

import icm_oracle as io
import lsq_update_oracle as lo
from rayuela_jl_amd.utils import splitarray


def tables(oracle, X, C):
    """U [m][n][h] = fl(sa - 2 g) and T [m-1][h][h] with T[i][b][a] = 2 <c_ia, c_{i+1}b>: icm_oracle.tables restricted
    to the adjacent pairs (T[i] = BinT[i][i+1])."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.asarray(C, dtype=np.float32)
    m, h, d = C.shape
    U = np.empty((m, X.shape[0], h), dtype=np.float32)
    T = np.zeros((max(m - 1, 0), h, h), dtype=np.float32)
    for i in range(m):
        sa = np.ascontiguousarray(np.diagonal(io._dots(oracle, C[i], C[i])))
        U[i] = sa[None, :] - np.float32(2) * io._dots(oracle, C[i], X)
        if i + 1 < m:
            T[i] = np.float32(2) * io._dots(oracle, C[i], C[i + 1])
    return U, T


def viterbi_tables(U, T, block=64):
    """The recursion on given tables: forward with back pointers, then the back trace."""
    m, n, h = U.shape
    codes = np.zeros((n, m), dtype=np.uint8)
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        M = U[0, r0:r1]
        arg = []
        for i in range(m - 1):
            cand = M[:, None, :] + T[i][None, :, :]          # [row][b][a] = fl(M_i[a] + T_i[b][a])
            arg.append(np.argmin(cand, axis=2))              # the lowest a
            M = U[i + 1, r0:r1] + cand.min(axis=2)           # M_{i+1}[b] = fl(U_{i+1}[b] + mincost_i[b])
        b = np.argmin(M, axis=1)
        codes[r0:r1, m - 1] = b
        for i in range(m - 2, -1, -1):
            b = arg[i][np.arange(r1 - r0), b]
            codes[r0:r1, i] = b
    return codes


def viterbi(oracle, X, C):
    U, T = tables(oracle, X, C)
    return viterbi_tables(U, T)


def energy(U, T, codes):
    """sum_i U_i[b_i] + sum_i T_i[b_{i+1}][b_i] in f64, per row."""
    m, n, h = U.shape
    rows = np.arange(n)
    c = np.asarray(codes).astype(np.int64)
    e = np.zeros(n)
    for i in range(m):
        e += U[i][rows, c[:, i]].astype(np.float64)
        if i + 1 < m:
            e += T[i][c[:, i + 1], c[:, i]].astype(np.float64)
    return e


def cbdims(d, m):
    """get_cbdims_chain, zero-based ranges."""
    sub = splitarray(range(d), m - 1)
    return [sub[0]] + [range(sub[i - 1][0], sub[i][-1] + 1) for i in range(1, m - 1)] + [sub[-1]]


def chain_update(X, codes, h, rho=1e-4):
    """-> (C (m, h, d) f32, C64 (m, h, d) f64)"""
    codes = np.asarray(codes)
    n, d = X.shape
    m = codes.shape[1]
    A, b = lo.normal_eq(X, codes, h, rho)
    C64 = np.zeros((m, h, d))
    for i, part in enumerate(splitarray(range(d), m - 1)):
        if len(part) == 0:
            continue
        blk = slice(i * h, (i + 2) * h)
        sol = np.linalg.solve(A[blk, blk], b[blk][:, part[0]:part[-1] + 1])
        C64[i][:, part[0]:part[-1] + 1] = sol[:h]
        C64[i + 1][:, part[0]:part[-1] + 1] = sol[h:]
    return C64.astype(np.float32), C64


def polar(G):
    """U V' of G (numpy SVD, f64)."""
    Um, _, Vt = np.linalg.svd(G.astype(np.float64), full_matrices=False)
    return Um @ Vt


def train(oracle, X, codes, Rimg, h, niter, rotate=True):
    """-> (C, codes, Rimg, obj (niter + 1,)).  Rimg[i][k] = R[k][i] (memory image of Julia's R); R'x for a row x is
    x @ R.  rotate=False keeps R fixed (the loop then only alternates update and encode)."""
    X = np.asarray(X, dtype=np.float32)
    R = np.asarray(Rimg, dtype=np.float64).T
    RX = (X.astype(np.float64) @ R).astype(np.float32)
    C, _ = chain_update(RX, codes, h)
    codes = viterbi(oracle, RX, C)
    obj = []
    for _ in range(niter + 1):
        obj.append(lo.qerror(RX, C, codes))
        if rotate:
            CB = lo.reconstruct(C, codes)
            R = polar(X.astype(np.float64).T @ CB)
            RX = (X.astype(np.float64) @ R).astype(np.float32)
        C, _ = chain_update(RX, codes, h)
        codes = viterbi(oracle, RX, C)
    return C, codes, np.ascontiguousarray(R.T.astype(np.float32)), np.array(obj)
