"""numpy restatement of the beam encoding contract ("Beam encoding contract"; src/CompetitiveQ.jl:75-135)
on top of oracle.pq_distmat -- a plain helper module: no fixtures, no pytest hooks.  Also the inputs the beam tests share."""
import functools

import numpy as np

BEAMS = (1, 2, 3, 16, 32)
# (n, d, m, h, kind): the parity cases of tests/test_gpu_beam.py; the first six shapes are tests/test_gpu_rvq.py's random cases,
# two of them with fewer rows here (the restatement sorts n * H * h values per stage)
RVQ_SHAPES = [(20_000, 128, 8, 256, "sift"), (5_000, 96, 4, 256, "deep"), (3_001, 64, 5, 77, "deep"), (1_000, 30, 3, 64, "sift"),
              (33, 16, 2, 16, "deep"), (2_000, 256, 3, 256, "deep")]
GPU_SHAPES = [(3_001, 64, 5, 77, "deep"), (1_000, 30, 3, 64, "sift"), (33, 16, 2, 16, "deep"), (600, 256, 3, 256, "deep"),
              (500, 128, 8, 256, "sift"), (1, 128, 8, 256, "sift"), (257, 20, 1, 40, "deep")]
TIE_SHAPE = (1_000, 32, 4, 64)


def _oracle():
    from oracle import oracle
    oracle.lib()
    return oracle


def encode(X, C, H, stats=None):
    """codes (n, m) uint8, residual (n, d) f32, cost (n,) f32 of the contract.  stats (a list) receives, per stage, the boolean
    rows whose values at ranks H_{i+1} and H_{i+1} + 1 are equal (the tie rule decides who survives)."""
    o = _oracle()
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    m, h, _ = C.shape
    R, P, rows = X[:, None, :], np.zeros((n, 1, 0), dtype=np.uint8), np.arange(n)[:, None]
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
        P = np.concatenate([P[rows, j], k[:, :, None].astype(np.uint8)], axis=2)
    return np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(R[:, 0]), np.ascontiguousarray(cost)


def data(n, d, m, h, kind):
    """tests/test_gpu_rvq.py's random inputs: clustered rows and one Lloyd step per stage."""
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(n, d, seed=n) if kind == "sift" else synth.deep_like(n, d, seed=n)
    return X, synth.rvq_codebooks(X, m, h, seed=n + 1, iters=1, sample=min(n, 2048))


@functools.lru_cache(maxsize=None)
def tie_fixture():
    """In every stage >= 1 entry 9 duplicates entry 5 and entries 20 and 40 are all-zero: candidates with equal values that
    only the index order separates, often at the boundary of the beam."""
    n, d, m, h = TIE_SHAPE
    X, C = data(n, d, m, h, "sift")
    C = C.copy()
    for i in range(1, m):
        C[i][9] = C[i][5]
        C[i][20] = 0
        C[i][40] = 0
    return X, C


def boundary_tie_share(X, C, H):
    stats = []
    encode(X, C, H, stats)
    return float(np.logical_or.reduce(stats).mean())


def qerror(X, C, codes):
    rec = np.zeros(X.shape, dtype=np.float64)
    for i in range(C.shape[0]):
        rec += C[i][codes[:, i]]
    return float(((X.astype(np.float64) - rec) ** 2).sum(axis=1).mean())


@functools.lru_cache(maxsize=None)
def expected(shape, H):
    """The restatement of one parity case, computed once per session: (X, C, codes, residual, cost)."""
    X, C = tie_fixture() if shape == "ties" else data(*shape)
    return (X, C) + encode(X, C, H)
