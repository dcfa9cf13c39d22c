"""CPU restatement of the LSQ encoding contract ("LSQ encoding") -- test infrastructure.

The dot products are the oracle's k-ordered fmaf chains (oracle.rotate_T on zero-padded square matrices: a padding term
is fma(0, 0, acc) = acc); every other operation is a numpy float32 add, subtract or multiply (one rounding each) or an
integer operation on uint64.  The random streams are keyed by the global row index, so any subset of rows can be run
(`rows=`), and nothing depends on chunking.

  ils(X, C, B0, ilsiter, icmiter, npert, randord, seed, t0, rows) -> (codes uint8 [n][m] zero-based, cost f32 [n])
"""
import numpy as np

from rayuela_jl_amd.synth import splitmix64

_M64 = (1 << 64) - 1
_HI = np.uint64(32)


def z(x):
    """splitmix64 of one Python int (wrap-around)."""
    return int(splitmix64(np.uint64(x & _M64)))


def _scale(w, r):
    """((w >> 32) * r) >> 32 on uint64 arrays (r < 2^32)."""
    return ((w >> _HI) * np.uint64(r)) >> _HI


def visit_order(seed, t, m, randord):
    """pi_t: the identity, or a Fisher-Yates shuffle over q = z(z(seed) ^ (t | 1 << 63)), shared by all rows."""
    perm = list(range(m))
    if not randord:
        return perm
    q = z(z(seed) ^ (t | (1 << 63)))
    for i in range(m - 1, 0, -1):
        r = ((z(q + i) >> 32) * (i + 1)) >> 32
        perm[i], perm[r] = perm[r], perm[i]
    return perm


def perturbation(seed, t, rows, m, h, npert):
    """(take [nr][m] bool, values [nr][m]): selection sampling of npert distinct positions per row, uniform values."""
    rows = np.asarray(rows, dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = splitmix64(np.uint64(z(z(seed) ^ t)) ^ rows)
        need = np.full(rows.shape, npert, dtype=np.int64)
        take = np.zeros((rows.size, m), dtype=bool)
        vals = np.zeros((rows.size, m), dtype=np.int64)
        for p in range(m):
            r = _scale(splitmix64(base + np.uint64(p)), m - p).astype(np.int64)
            tk = r < need
            need -= tk
            take[:, p] = tk
            vals[:, p] = _scale(splitmix64(base + np.uint64(m + p)), h).astype(np.int64)
    return take, vals


def _dots(oracle, A, Bm):
    """out[b][a] = <A[a], Bm[b]> as k-ordered fmaf chains (A [na][d], Bm [nb][d])."""
    na, d = A.shape
    D = max(d, na)
    R = np.zeros((D, D), dtype=np.float32)
    R[:na, :d] = A
    Bp = np.zeros((Bm.shape[0], D), dtype=np.float32)
    Bp[:, :d] = Bm
    return oracle.rotate_T(R, Bp)[:, :na]


def tables(oracle, X, C):
    """U [m][n][h] (fl(sa - 2g)) and BinT [m][m][h][h] with BinT[j][k][b][l] = 2 <c_jl, c_kb> (zero for j == k)."""
    C = np.asarray(C, dtype=np.float32)
    m, h, d = C.shape
    U = np.empty((m, X.shape[0], h), dtype=np.float32)
    binT = np.zeros((m, m, h, h), dtype=np.float32)
    for i in range(m):
        sa = np.ascontiguousarray(np.diagonal(_dots(oracle, C[i], C[i])))
        U[i] = sa[None, :] - np.float32(2) * _dots(oracle, C[i], X)
        for k in range(m):
            if k != i:
                binT[i, k] = np.float32(2) * _dots(oracle, C[i], C[k])
    return U, binT


def condition(B, U, binT, j):
    """One conditioning step for codebook j on all rows of B (uint8 [n][m], updated in place)."""
    m = B.shape[1]
    ub = U[j].copy()
    for k in range(m):
        if k != j:
            ub = ub + binT[j, k][B[:, k].astype(np.int64)]
    B[:, j] = np.argmin(ub, axis=1)


def veccost(X, B, C):
    """veccost with the kernel's order: CB by adds from +0 in codebook order; lane l sums (CB - x)^2 over dims
    l, l+64, ... in order; an xor butterfly (32, 16, 8, 4, 2, 1) adds the 64 partial sums."""
    C = np.asarray(C, dtype=np.float32)
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    CB = np.zeros((n, d), dtype=np.float32)
    for i in range(C.shape[0]):
        CB = CB + C[i][np.asarray(B)[:, i].astype(np.int64)]
    df = CB - X
    sq = df * df
    part = np.zeros((n, 64), dtype=np.float32)
    for q in range(0, d, 64):
        cnt = min(64, d - q)
        part[:, :cnt] = part[:, :cnt] + sq[:, q:q + cnt]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ off]
    return part[:, 0].copy()


def ils(oracle, X, C, B0, ilsiter, icmiter, npert, randord, seed=0, t0=0, rows=None, cond=None, tabs=None):
    """The whole encode for the rows of X (global indices `rows`, default 0..n-1).  cond(B, U, binT, j) replaces the
    numpy conditioning step (the golden generator passes the reference's own)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.ascontiguousarray(C, dtype=np.float32)
    m, h, _ = C.shape
    n = X.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    U, binT = tables(oracle, X, C) if tabs is None else tabs
    cond = condition if cond is None else cond
    B = np.array(B0, dtype=np.uint8, copy=True)
    cost = veccost(X, B, C)
    for it in range(ilsiter):
        t = t0 + it
        perm = visit_order(seed, t, m, randord)
        take, vals = perturbation(seed, t, rows, m, h, npert)
        nb = B.copy()
        nb[take] = vals[take]
        for _ in range(icmiter):
            for j in perm:
                cond(nb, U, binT, j)
        c = veccost(X, nb, C)
        better = c < cost
        B[better] = nb[better]
        cost[better] = c[better]
    return B, cost
