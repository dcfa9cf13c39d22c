"""CPU restatement of the chain quantization contract ("Chain quantization") for any number of codewords per
codebook and int16 codes -- test infrastructure, a plain helper module built on tests/chain_oracle.py, tests/icm_wide_oracle.py
and tests/lsq_wide_oracle.py.

What differs from chain_oracle is only what h > 256 needs: the codes are int16, the dot products run block-wise
(icm_wide_oracle.dots: the same k-ordered fmaf chains from +0), the recursion takes a row-block argument so that its [rows][h][h]
candidates stay small, and the codebook update builds each 2h x 2h block by itself -- no (m h)^2 matrix.

  tables(oracle, X, C)                   -> (U [m][n][h], T [m-1][h][h]) with T[i][b][a] = 2 <c_ia, c_{i+1}b>
  viterbi_tables(U, T, block)            -> codes int16 [n][m] zero-based
  viterbi(oracle, X, C, block)
  chain_update(X, codes, h, rho)         -> (C (m, h, d) f32, C64 (m, h, d) f64)
  train(oracle, X, codes, Rimg, h, niter, rotate) -> (C, codes, Rimg, obj (niter + 1,))
"""
import numpy as np

import chain_oracle as co
import icm_wide_oracle as iw
import lsq_wide_oracle as lw
from rayuela_jl_amd.utils import splitarray


def tables(oracle, X, C):
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.asarray(C, dtype=np.float32)
    m, h, d = C.shape
    U = np.empty((m, X.shape[0], h), dtype=np.float32)
    T = np.zeros((max(m - 1, 0), h, h), dtype=np.float32)
    for i in range(m):
        sa = np.zeros(h, dtype=np.float32)
        for k0 in range(0, h, iw.BLOCK):          # <c, c> is the diagonal of a block's own products
            sa[k0:k0 + iw.BLOCK] = np.diagonal(iw.dots(oracle, C[i][k0:k0 + iw.BLOCK], C[i][k0:k0 + iw.BLOCK]))
        U[i] = sa[None, :] - np.float32(2) * iw.dots(oracle, C[i], X)
        if i + 1 < m:
            T[i] = np.float32(2) * iw.dots(oracle, C[i], C[i + 1])
    return U, T


def viterbi_tables(U, T, block=8):
    """chain_oracle.viterbi_tables with int16 codes: forward with back pointers, then the back trace, `block` rows at a time."""
    m, n, h = U.shape
    codes = np.zeros((n, m), dtype=np.int16)
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


def viterbi(oracle, X, C, block=8):
    U, T = tables(oracle, X, C)
    return viterbi_tables(U, T, block)


def pair_counts(codes, h, i):
    """(h, h) int64: the rows with (codes[:, i], codes[:, i + 1]) = (a, b)."""
    c = np.asarray(codes).astype(np.int64)
    pc = np.zeros((h, h), np.int64)
    np.add.at(pc, (c[:, i], c[:, i + 1]), 1)
    return pc


def block(cnt, pc, i, h, rho):
    """The 2h x 2h f64 block of stage i: [[diag(cnt_i + rho), P], [P', diag(cnt_{i+1} + rho)]]."""
    A = np.zeros((2 * h, 2 * h))
    idx = np.arange(h)
    A[idx, idx] = cnt[i].astype(np.float64) + rho
    A[h + idx, h + idx] = cnt[i + 1].astype(np.float64) + rho
    A[:h, h:] = pc
    A[h:, :h] = pc.T
    return A


def chain_update(X, codes, h, rho=1e-4):
    """chain_oracle.chain_update per adjacent block: b and the counts from lsq_wide_oracle.normal_eq(with_A=False), np.add.at pair
    counts, np.linalg.solve per 2h x 2h block.  -> (C (m, h, d) f32, C64 (m, h, d) f64)"""
    codes = np.asarray(codes)
    if codes.dtype != np.int16:
        codes = codes.astype(np.int16)
    n, d = X.shape
    m = codes.shape[1]
    _, b, cnt = lw.normal_eq(X, codes, h, rho, 0, with_A=False)
    C64 = np.zeros((m, h, d))
    for i, part in enumerate(splitarray(range(d), m - 1)):
        if len(part) == 0:
            continue
        A = block(cnt, pair_counts(codes, h, i), i, h, rho)
        sol = np.linalg.solve(A, b[i * h:(i + 2) * h][:, part[0]:part[-1] + 1])
        C64[i][:, part[0]:part[-1] + 1] = sol[:h]
        C64[i + 1][:, part[0]:part[-1] + 1] = sol[h:]
    return C64.astype(np.float32), C64


def train(oracle, X, codes, Rimg, h, niter, rotate=True):
    """chain_oracle.train over int16 codes.  Rimg[i][k] = R[k][i] (memory image of Julia's R); R'x for a row x is x @ R."""
    X = np.asarray(X, dtype=np.float32)
    R = np.asarray(Rimg, dtype=np.float64).T
    RX = (X.astype(np.float64) @ R).astype(np.float32)
    C, _ = chain_update(RX, codes, h)
    codes = viterbi(oracle, RX, C)
    obj = []
    for _ in range(niter + 1):
        obj.append(lw.qerror(RX, C, codes))
        if rotate:
            CB = lw.reconstruct(C, codes)
            R = co.polar(X.astype(np.float64).T @ CB)
            RX = (X.astype(np.float64) @ R).astype(np.float32)
        C, _ = chain_update(RX, codes, h)
        codes = viterbi(oracle, RX, C)
    return C, codes, np.ascontiguousarray(R.T.astype(np.float32)), np.array(obj)
