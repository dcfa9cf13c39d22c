"""numpy restatement of the beam encoding contract with more than 256 codewords per stage ("Beam encoding
contract", and section 4.21; src/CompetitiveQ.jl:75-135 on Matrix{Int16} codes) -- tests/beam_oracle.py with int16 prefixes.
A plain helper module: no fixtures, no pytest hooks.  Also the inputs the wide beam tests share."""
import functools

import numpy as np

import beam_oracle as bo

BEAMS = bo.BEAMS
# (n, d, m, h, kind, beams): the parity cases of tests/test_gpu_beam_wide.py
#   h = 300    two codeword blocks, the second ragged             h = 257   a last block of ONE live codeword
#   d = 260    more than 256 dimensions, no multiple of 16         h = 1000  four blocks, three row tiles of vectors
#   m = 1 and n = 1: the shortest loops
GPU_SHAPES = [(1_000, 30, 3, 300, "deep", BEAMS), (400, 16, 4, 257, "deep", BEAMS), (300, 260, 2, 300, "deep", BEAMS),
              (600, 64, 3, 1000, "deep", (1, 3)), (400, 20, 1, 300, "deep", BEAMS), (1, 30, 3, 300, "deep", BEAMS)]
# the largest packed index j * h + k: random normal codebooks, H = 32
BIG_SHAPE = (40, 8, 2, 32767)
TIE_SHAPES = [(1_000, 30, 3, 300), (400, 16, 4, 257)]
TIE_BEAMS = (1, 3, 32)


def encode(X, C, H, stats=None):
    """codes (n, m) int16 zero-based, residual (n, d) f32, cost (n,) f32 of the contract, any 1 <= h <= 32767.  stats (a list)
    receives, per stage, the boolean rows whose values at ranks H_{i+1} and H_{i+1} + 1 are equal."""
    o = bo._oracle()
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    m, h, _ = C.shape
    R, P, rows = X[:, None, :], np.zeros((n, 1, 0), dtype=np.int16), np.arange(n)[:, None]
    for i in range(m):
        Hi = R.shape[1]
        U = o.pq_distmat(np.ascontiguousarray(R.reshape(n * Hi, d)), C[i], 1, h).reshape(n, Hi * h)
        V = np.where(U > 0, U, np.float32(0))                      # the clamp: -0 and NaN become +0
        Hn = min(H, Hi * h)
        order = np.argsort(V, axis=1, kind="stable")               # the total order (v, j * h + k)
        if stats is not None:
            Vs = np.take_along_axis(V, order[:, :Hn + 1], axis=1)
            stats.append(Vs[:, Hn - 1] == Vs[:, Hn] if Hi * h > Hn else np.zeros(n, dtype=bool))
        order = order[:, :Hn]
        j, k = order // h, order % h
        cost = np.take_along_axis(V, order[:, :1], axis=1)[:, 0]
        with np.errstate(invalid="ignore"):
            R = R[rows, j] - C[i][k]                               # fl(r_j - C_i[k]) elementwise
        P = np.concatenate([P[rows, j], k[:, :, None].astype(np.int16)], axis=2)
    return np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(R[:, 0]), np.ascontiguousarray(cost)


def data(n, d, m, h, kind="deep"):
    """beam_oracle.data: clustered rows and one Lloyd step per stage.  Fewer rows than codewords: the first n rows of the
    1000-row set, with its codebooks."""
    if n >= h:
        return bo.data(n, d, m, h, kind)
    X, C = bo.data(1_000, d, m, h, kind)
    return np.ascontiguousarray(X[:n]), C


@functools.lru_cache(maxsize=None)
def big_data():
    n, d, m, h = BIG_SHAPE
    rng = np.random.default_rng(h)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, h, d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tie_fixture(shape):
    """In every stage >= 1 entry h - 1 duplicates entry 5 and entries 20 and h - 40 are all-zero: candidates with equal values
    in DIFFERENT blocks of 256 codewords, which only the index order separates, often at the boundary of the beam."""
    n, d, m, h = shape
    X, C = data(n, d, m, h, "deep")
    C = C.copy()
    for i in range(1, m):
        C[i][h - 1] = C[i][5]
        C[i][20] = 0
        C[i][h - 40] = 0
    return X, C


def boundary_tie_share(X, C, H):
    stats = []
    encode(X, C, H, stats)
    return float(np.logical_or.reduce(stats).mean())


@functools.lru_cache(maxsize=None)
def expected(shape, H):
    """The restatement of one parity case, computed once per session: (X, C, codes, residual, cost).  shape: a GPU_SHAPES entry
    without its beams, "big", or ("ties", tie shape)."""
    if shape == "big":
        X, C = big_data()
    elif shape[0] == "ties":
        X, C = tie_fixture(shape[1])
    else:
        X, C = data(*shape)
    return (X, C) + encode(X, C, H)
