"""Step-by-step restatement of the library's k-means (csrc/rq_train.hip, csrc/rq_train_host.hip) for the tests: numpy,
float64 and Python ints, no library, no device.

  Rng(seed, salt)          the seeded splitmix64 stream; salt 1 = train_pq / kmpp_seeds, 2 = train_opq, 3 = train_rvq
  sample_distinct          the partial Fisher-Yates of train_opq's start (and of TRAIN_KMPP = 0)
  kmpp_seeds               kmeans++ seeding (kmpp_first / kmpp_update / kmpp_select): the m * h uniforms are drawn first,
                           sub-space major; step t picks the first row whose inclusive cumulative cost exceeds u_t * total
  repick                   repick_unused: emptied centres re-drawn with the costs of the last assignment
  lloyd_step               one iteration of train_pq_loop: encode, means, repick; the stream is carried by the caller

On integer-valued X (coordinates in [0, 255], sub-space width <= 32) every cost is an exact integer below 2^24 and every sum
an exact integer below 2^53, in float32 on the device as in float64 here, so a pick does not depend on any summation tree:
kmpp_seeds is then the mathematical answer and the kernels must equal it exactly.

Layouts: X (n, d) f32, codes (n, m) uint8 zero-based, C a list of m (h, sub_i) arrays (sub-spaces of synth.splitarray)."""
import numpy as np

from rayuela_jl_amd import synth

GOLDEN_GAMMA = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
SALT_PQ, SALT_OPQ, SALT_RVQ = 1, 2, 3


class Rng:
    """struct Rng of csrc/rq_internal.h, started like every training entry point starts it."""

    def __init__(self, seed, salt):
        self.s = (int(seed) * GOLDEN_GAMMA + int(salt)) & _M64

    def next(self):
        self.s = (self.s + GOLDEN_GAMMA) & _M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    def uniform(self):
        return (self.next() >> 11) / 2.0 ** 53


def sample_distinct(rng, n, h):
    """h distinct values below n: position i swaps with j = i + next() % (n - i) on a sparse map of touched positions."""
    swaps, out = {}, []
    for i in range(h):
        j = i + rng.next() % (n - i)
        vi, vj = swaps.get(i, i), swaps.get(j, j)
        swaps[i], swaps[j] = vj, vi
        out.append(vj)
    return out


def sub_costs(Xs, v):
    """|x - v|^2 per row of Xs in float64, the sub-space's terms added in ascending order."""
    a = np.zeros(Xs.shape[0], dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    for t in range(Xs.shape[1]):
        e = Xs[:, t].astype(np.float64) - v[t]
        a += e * e
    return a


def first_above(S, thr):
    """first index whose inclusive cumulative sum S exceeds thr (len(S) when none does)."""
    return int(np.searchsorted(S, thr, side="right"))


def kmpp_seeds(X, m, h, seed=0, salt=SALT_PQ, rng=None):
    """seeds (m, h) int64 zero-based rows of X.  `rng`: continue that stream instead of starting Rng(seed, salt)."""
    X = np.asarray(X)
    n, d = X.shape
    off = synth.splitarray(d, m)
    rng = Rng(seed, salt) if rng is None else rng
    u = [[rng.uniform() for _ in range(h)] for _ in range(m)]
    seeds = np.empty((m, h), dtype=np.int64)
    for i in range(m):
        Xs = X[:, off[i]:off[i + 1]]
        s = min(int(u[i][0] * n), n - 1)
        seeds[i, 0] = s
        mincost = None
        for t in range(1, h):
            c = sub_costs(Xs, Xs[s])
            mincost = c if mincost is None else np.minimum(mincost, c)
            mincost[s] = 0.0
            S = np.cumsum(mincost)
            total = S[-1]
            if not total > 0.0:
                s = min(int(u[i][t] * n), n - 1)
            else:
                s = first_above(S, u[i][t] * total)
                if s >= n:                      # the threshold rounded up to the total: the last row with a cost
                    s = int(np.flatnonzero(mincost > 0.0)[-1])
            seeds[i, t] = s
    return seeds


def seed_subvectors(X, m, rows):
    """the list of m (h, sub_i) f32 blocks X[rows[i], sub-space i]."""
    off = synth.splitarray(X.shape[1], m)
    return [np.ascontiguousarray(X[np.asarray(rows[i], dtype=np.int64), off[i]:off[i + 1]], dtype=np.float32)
            for i in range(m)]


def repick(X_sub, C_old_sub, codes, unused, rng):
    """repick_unused: rows drawn for the `unused` centres (ascending) and, per draw, (branch, margin): branch "cost" or
    "uniform", margin = min(|S[pick] - thr|, |S[pick - 1] - thr|) / total of a cost-proportional draw (None otherwise).
    Costs are the float64 squared distances to the OLD centre of each row's code; every draw takes one next() (the uniform
    fallback next() % n) and, with cost left, one uniform() after it; the picked row's cost drops to 0 and all costs are
    lowered to the distance to the new centre before the next draw."""
    n = X_sub.shape[0]
    Xd = X_sub.astype(np.float64)
    Cd = np.asarray(C_old_sub, dtype=np.float64)[np.asarray(codes, dtype=np.int64)]
    tc = np.zeros(n, dtype=np.float64)
    for t in range(Xd.shape[1]):
        e = Xd[:, t] - Cd[:, t]
        tc += e * e
    picks, info = [], []
    for _ in unused:
        S = np.cumsum(tc)
        total = S[-1]
        pick = rng.next() % n
        if total > 0.0:
            thr = rng.uniform() * total
            j = first_above(S, thr)
            pick = j if j < n else n - 1
            before = S[pick - 1] if pick > 0 else 0.0
            info.append(("cost", min(abs(S[pick] - thr), abs(before - thr)) / total))
        else:
            info.append(("uniform", None))
        picks.append(int(pick))
        tc[pick] = 0.0
        tc = np.minimum(tc, sub_costs(X_sub, X_sub[pick]))
    return picks, info


def lloyd_step(X, C_k, m, h, rng, encode):
    """One iteration of train_pq_loop from the centres C_k: codes = encode(X, C_k); centres with rows become their float64
    mean, centres without rows keep their value and are then re-drawn (repick, with the costs against C_k).
    Returns (C_next list of (h, sub_i) float64, repicked, codes, counts (m, h)); repicked is a list of
    (sub-space, centre, row, branch, margin) in draw order."""
    X = np.asarray(X)
    off = synth.splitarray(X.shape[1], m)
    codes = np.asarray(encode(X, C_k))
    counts = np.stack([np.bincount(codes[:, i], minlength=h) for i in range(m)])
    C_next, repicked = [], []
    for i in range(m):
        Xs = X[:, off[i]:off[i + 1]]
        sums = np.zeros((h, Xs.shape[1]), dtype=np.float64)
        np.add.at(sums, codes[:, i], Xs.astype(np.float64))
        Cn = np.asarray(C_k[i], dtype=np.float64).copy()
        used = counts[i] > 0
        Cn[used] = sums[used] / counts[i][used, None]
        unused = [int(k) for k in np.flatnonzero(~used)]
        if unused:
            picks, info = repick(Xs, C_k[i], codes[:, i], unused, rng)
            for k, row, (branch, margin) in zip(unused, picks, info):
                Cn[k] = Xs[row].astype(np.float64)
                repicked.append((i, k, row, branch, margin))
        C_next.append(Cn)
    return C_next, repicked, codes, counts


# ---- fixtures shared by tests/test_kmeans_oracle.py (CPU) and tests/test_gpu_kmeans.py -------------------------------------

def int_data(n, d, seed):
    """(n, d) f32 with integer coordinates in [0, 255], counter based: a prefix of a longer draw is the shorter draw."""
    e = np.arange(n * d, dtype=np.uint64)
    v = synth.splitmix64(e ^ (np.uint64(seed) << np.uint64(40))) % np.uint64(256)
    return v.astype(np.float32).reshape(n, d)


def five_points(n=300, d=4, seed=5):
    """n rows drawn from 5 distinct integer points: fewer distinct points than centres at h = 16, so kmeans++ runs out of
    cost (the floor(u n) fallback) and Lloyd's first iteration repicks through the next() % n branch."""
    pts = int_data(5, d, seed + 1000)
    assert len({tuple(p) for p in pts.tolist()}) == 5
    idx = (synth.splitmix64(np.arange(n, dtype=np.uint64) ^ np.uint64(seed * 7919)) % np.uint64(5)).astype(np.int64)
    return np.ascontiguousarray(pts[idx])


def crowded(n=300, d=4, seed=6, heavy=240, npts=4):
    """`heavy` copies of `npts` integer points plus n - heavy scattered integer rows, permuted.  Uniformly sampled start
    rows (TRAIN_KMPP = 0) mostly coincide, the later copies of a point get no row, and the scattered rows leave cost for
    the cost-proportional branch of the repick."""
    pts = int_data(npts, d, seed + 2000)
    assert len({tuple(p) for p in pts.tolist()}) == npts
    X = np.concatenate([pts[np.arange(heavy) % npts], int_data(n - heavy, d, seed + 3000)])
    key = synth.splitmix64(np.arange(n, dtype=np.uint64) ^ np.uint64(seed * 104729))
    return np.ascontiguousarray(X[np.argsort(key, kind="stable")])


BIG_ROWS = (1 << 20, (1 << 20) + 1, 2_200_003)      # kmpp_select: one-row chunks; two-row chunks and a two-row last block;
BIG_H, BIG_SEED = 6, 21                             # three-row chunks and a ragged last block
BIG_TAIL_SEED = 1                                   # with big_fixture(tail=True): some seed lies in the last block of rows
_big = {}


def big_fixture(n, d, tail=False):
    """the first n rows of one (2 200 003, 8) integer draw, restricted to the first d columns.  tail: the rows hold 127 or
    128 only, except the last three (all 0, all 255, alternating): most of the cost then sits in the last block of rows."""
    if "X" not in _big:
        _big["X"] = int_data(BIG_ROWS[-1], 8, 77)
    X = np.ascontiguousarray(_big["X"][:n, :d])
    if tail:
        X = 127.0 + np.mod(X, 2.0).astype(np.float32)
        X[-3], X[-2] = 0.0, 255.0
        X[-1, 0::2], X[-1, 1::2] = 0.0, 255.0
    return X


def kmpp_blocks(n):
    """(rows per block, blocks) of the seeding kernels' split of the rows (kmpp_init_launch)."""
    nblk = min(1024, (n + 1023) // 1024)
    rows = (n + nblk - 1) // nblk
    return rows, (n + rows - 1) // rows
