"""CPU restatement of the LSQ encoding contract ("LSQ encoding") for any number of codewords per codebook and
int16 codes -- test infrastructure, a plain helper module built on tests/icm_oracle.py.

What differs from icm_oracle is only what h > 256 needs: the codes are int16, and the dot products run through oracle.rotate_T in
blocks of codewords (icm_oracle._dots pads to one square matrix of side max(d, h): h^3 work at h in the thousands).  The chains are
the same k-ordered fmaf chains from +0 (a padding term is fma(0, 0, acc) = acc), the binaries of (k, j) are those of (j, k)
transposed (fma(a, b, acc) = fma(b, a, acc)), and the random streams, the conditioning step and veccost ARE icm_oracle's.

  tables(oracle, X, C)                                                  -> (U [m][n][h], binT [m][m][h][h])
  ils(oracle, X, C, B0, ilsiter, icmiter, npert, randord, seed, t0, ..) -> (codes int16 [n][m] zero-based, cost f32 [n])
"""
import numpy as np

import icm_oracle as io

BLOCK = 32


def dots(oracle, A, Bm):
    """out[b][a] = <A[a], Bm[b]> as k-ordered fmaf chains (A [na][d], Bm [nb][d]), BLOCK rows of A at a time."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    na, d = A.shape
    D = max(d, BLOCK)
    Bp = np.zeros((Bm.shape[0], D), dtype=np.float32)
    Bp[:, :d] = Bm
    out = np.empty((Bm.shape[0], na), dtype=np.float32)
    for a0 in range(0, na, D):
        blk = A[a0:a0 + D]
        R = np.zeros((D, D), dtype=np.float32)
        R[:blk.shape[0], :d] = blk
        out[:, a0:a0 + blk.shape[0]] = oracle.rotate_T(R, Bp)[:, :blk.shape[0]]
    return out


def tables(oracle, X, C):
    """U [m][n][h] (fl(sa - 2g)) and BinT [m][m][h][h] with BinT[j][k][b][l] = 2 <c_jl, c_kb> (zero for j == k)."""
    C = np.asarray(C, dtype=np.float32)
    m, h, d = C.shape
    U = np.empty((m, X.shape[0], h), dtype=np.float32)
    binT = np.zeros((m, m, h, h), dtype=np.float32)
    for i in range(m):
        sa = np.zeros(h, dtype=np.float32)
        for k0 in range(0, h, BLOCK):          # <c, c> is the diagonal of a block's own products
            sa[k0:k0 + BLOCK] = np.diagonal(dots(oracle, C[i][k0:k0 + BLOCK], C[i][k0:k0 + BLOCK]))
        U[i] = sa[None, :] - np.float32(2) * dots(oracle, C[i], X)
        for k in range(i + 1, m):
            binT[i, k] = np.float32(2) * dots(oracle, C[i], C[k])
            binT[k, i] = binT[i, k].T
    return U, binT


def condition_literal(B, U, binT, j):
    """io.condition spelled as scalar loops: per row, candidate l costs U[j][row][l] plus the m - 1 binaries in ascending k (one f32
    add each), and the first l with the strictly smallest cost wins."""
    n, m = B.shape
    h = U.shape[2]
    for r in range(n):
        best, arg = None, -1
        for l in range(h):
            v = np.float32(U[j][r][l])
            for k in range(m):
                if k != j:
                    v = np.float32(v + binT[j][k][int(B[r][k])][l])
            if best is None or v < best:
                best, arg = v, l
        B[r][j] = arg


def ils(oracle, X, C, B0, ilsiter, icmiter, npert, randord, seed=0, t0=0, rows=None, cond=None, tabs=None):
    """icm_oracle.ils over int16 codes: the whole encode for the rows of X (global indices `rows`, default 0..n-1)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.ascontiguousarray(C, dtype=np.float32)
    m, h, _ = C.shape
    n = X.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    cond = io.condition if cond is None else cond
    B = np.array(B0, dtype=np.int16, copy=True)
    cost = io.veccost(X, B, C)
    if ilsiter == 0:
        return B, cost
    U, binT = tables(oracle, X, C) if tabs is None else tabs
    for it in range(ilsiter):
        t = t0 + it
        perm = io.visit_order(seed, t, m, randord)
        take, vals = io.perturbation(seed, t, rows, m, h, npert)
        nb = B.copy()
        nb[take] = vals[take]
        for _ in range(icmiter):
            for j in perm:
                cond(nb, U, binT, j)
        c = io.veccost(X, nb, C)
        better = c < cost
        B[better] = nb[better]
        cost[better] = c[better]
    return B, cost
