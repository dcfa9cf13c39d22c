"""Step-by-step restatement of training with more than 256 codewords per codebook (rq_train_pq_wide, rq_train_rvq_wide,
rq_train_opq_wide) for the tests -- a plain helper module: no fixtures, no pytest hooks, no library, no device.  Built from
tests/kmeans_oracle.py (the seeded stream, kmeans++, sample_distinct, repick) and tests/wide_oracle.py (the assignments).

  exact_means        update_centers on integer-valued X: counts by bincount, sums in float64 (exact), centres
                     float32(sum) * (float32(1) / float32(count)) -- the kernel's finishing formula, so on such data the
                     library must return these BITS whatever its summation tree; a code without rows keeps its bits
  lloyd_step         one iteration of the Lloyd loop from the centres C_k: exact means, then ko.repick against C_k
  walk               the whole restated loop alone: start rows, every C_k, the stopping iteration K, the repicks
  telescope          the library against that restatement step by step, the shape of tests/test_gpu_kmeans.py::_telescope
  train_opq          oracle/train_oracle.py::train_opq with wide assignments
  kmeans_clustering  oracle/train_oracle.py::kmeans_clustering (Clustering.kmeans' own rules) with wide assignments

Layouts: X (n, d) f32, codes (n, m) int16 zero-based, C a list of m (h, sub_i) f32 arrays."""
import numpy as np

import kmeans_oracle as ko
import wide_oracle as wo

ONE = np.float32(1)


def cat(C):
    return np.concatenate([np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in C])


def encode(oracle, X, C, m, h):
    return wo.encode_pq_wide(oracle, X, cat(C), m, h)


def exact_means(X, C_prev, codes, m, h):
    """(C list of (h, sub_i) f32, counts (m, h) int64).  Rows whose code lies outside [0, h) are ignored in that sub-space
    (codes are read zero-extended: a negative int16 is out of range)."""
    X = np.asarray(X)
    off = wo.splitarray(X.shape[1], m)
    codes = np.asarray(codes).astype(np.int16).view(np.uint16).astype(np.int64)
    out, counts = [], np.zeros((m, h), dtype=np.int64)
    for i in range(m):
        ok = codes[:, i] < h
        ci = codes[ok, i]
        cnt = np.bincount(ci, minlength=h)
        Cn = np.array(C_prev[i], dtype=np.float32, copy=True)
        used = cnt > 0
        inv = ONE / cnt[used].astype(np.float32)
        for s in range(off[i], off[i + 1]):
            sums = np.bincount(ci, weights=X[ok, s].astype(np.float64), minlength=h)
            assert np.array_equal(sums, np.round(sums)) and sums.max(initial=0) < 2 ** 24       # exact in f32 too
            Cn[used, s - off[i]] = sums[used].astype(np.float32) * inv
        out.append(Cn)
        counts[i] = cnt
    return out, counts


def lloyd_step(X, C_k, codes, m, h, rng):
    """(C_next list f32, repicked, counts): repicked is a list of (sub-space, centre, row, branch, margin) in draw order."""
    X = np.asarray(X)
    off = wo.splitarray(X.shape[1], m)
    C_next, counts = exact_means(X, C_k, codes, m, h)
    repicked = []
    for i in range(m):
        unused = [int(k) for k in np.flatnonzero(counts[i] == 0)]
        if unused:
            Xs = X[:, off[i]:off[i + 1]]
            picks, info = ko.repick(Xs, C_k[i], codes[:, i], unused, rng)
            for k, row, (branch, margin) in zip(unused, picks, info):
                C_next[i][k] = Xs[row]
                repicked.append((i, k, row, branch, margin))
    return C_next, repicked, counts


def start_rows(X, m, h, seed, salt, kmpp, rng=None):
    """(rows, rng): the restated start rows (kmeans++, or sample_distinct under TRAIN_KMPP = 0) and the stream after them."""
    rng = ko.Rng(seed, salt) if rng is None else rng
    rows = ko.kmpp_seeds(X, m, h, rng=rng) if kmpp else [ko.sample_distinct(rng, X.shape[0], h) for _ in range(m)]
    return rows, rng


def new_stats():
    return dict(cost=0, uniform=0, wide=0, margin=np.inf)


def note(stats, repicked):
    for (_, k, _, branch, margin) in repicked:
        stats[branch] += 1
        stats["wide"] += int(k >= 256)
        if branch == "cost":
            stats["margin"] = min(stats["margin"], margin)


def walk(oracle, X, m, h, seed, salt=ko.SALT_PQ, kmpp=True, kmax=250):
    """The restated loop alone.  Returns (K, Cs, codes, rows, stats): Cs[k] the centres after k iterations, codes[k] their
    assignments, K the iteration at which codes[K] == codes[K - 1]."""
    rows, rng = start_rows(X, m, h, seed, salt, kmpp)
    C_k = ko.seed_subvectors(X, m, rows)
    Cs, allcodes, stats = [C_k], [], new_stats()
    prev, k = None, 0
    while True:
        codes = encode(oracle, X, C_k, m, h)
        allcodes.append(codes)
        if prev is not None and np.array_equal(codes, prev):
            return k, Cs, allcodes, rows, stats
        assert k < kmax
        C_k, repicked, _ = lloyd_step(X, C_k, codes, m, h, rng)
        note(stats, repicked)
        Cs.append(C_k)
        prev, k = codes, k + 1


def same_bits(a, b):
    return all(x.dtype == np.float32 and y.dtype == np.float32 and np.array_equal(x.view(np.uint32), y.view(np.uint32))
               for x, y in zip(a, b))


def telescope(train, quant, oracle, X, m, h, rng, rows, stats, kmax=250):
    """train(k) -> (C list of m (h, sub_i) f32, B (n, m) int16 one-based) after k iterations; `rows` the restated start rows,
    `rng` the restated stream right after the start was drawn.  Every step is derived from the library's own state k:
    B_k == the wide encode oracle + 1 == quant(X, C_k); C_{k+1} == the exact restated step from C_k BIT FOR BIT, repicked
    centres included (so the stream is where the restatement has it).  Returns (K, C_K, B_K) at the restated stopping rule."""
    C_k, B_k = train(0)
    want = ko.seed_subvectors(X, m, rows)
    assert same_bits(C_k, want), "start rows"
    prev, k = None, 0
    while True:
        codes = encode(oracle, X, C_k, m, h)
        assert B_k.dtype == np.int16 and np.array_equal(B_k, codes + 1), k
        assert np.array_equal(B_k, quant(X, C_k)), k
        if prev is not None and np.array_equal(codes, prev):
            return k, C_k, B_k
        assert k < kmax
        C_next, repicked, counts = lloyd_step(X, C_k, codes, m, h, rng)
        C_k1, B_k1 = train(k + 1)
        for i in range(m):
            bad = np.flatnonzero((C_k1[i].view(np.uint32) != C_next[i].view(np.uint32)).any(axis=1))
            assert bad.size == 0, (k, i, bad[:8], counts[i][bad[:8]], repicked[:4])
        for (_, _, _, branch, margin) in repicked:
            if branch == "cost":
                assert margin > 1e-9, (k, margin)
        note(stats, repicked)
        prev, C_k, B_k, k = codes, C_k1, B_k1, k + 1


def reconstruct(C, codes, off, d):
    CB = np.zeros((codes.shape[0], d), dtype=np.float32)
    for i in range(len(off) - 1):
        CB[:, off[i]:off[i + 1]] = C[i][codes[:, i].astype(np.int64)]
    return CB


def float_means(C, RX, codes, off, h):
    """oracle/train_oracle.py::update_centers_fast: float64 means (real-valued rows), emptied centres keep their value."""
    out = []
    for i in range(len(off) - 1):
        ci = codes[:, i].astype(np.int64)
        cnt = np.bincount(ci, minlength=h).astype(np.float64)
        Ci = C[i].astype(np.float64).copy()
        for s in range(off[i], off[i + 1]):
            sums = np.bincount(ci, weights=RX[:, s].astype(np.float64), minlength=h)
            Ci[cnt > 0, s - off[i]] = sums[cnt > 0] / cnt[cnt > 0]
        out.append(Ci.astype(np.float32))
    return out


def train_opq(oracle, X, m, h, niter, R0, C0):
    """oracle/train_oracle.py::train_opq (src/OPQ.jl:49-139) step by step, with wo.encode_pq_wide for the assignments.
    R0: memory image of Julia's R; C0: list of (h, sub_i).  Returns C, codes (n, m) int16 zero-based, R, obj."""
    n, d = X.shape
    off = wo.splitarray(d, m)
    R = R0.astype(np.float32)
    C = [c.astype(np.float32) for c in C0]
    RX = oracle.rotate_T(R, X)
    codes = encode(oracle, RX, C, m, h)
    CB = reconstruct(C, codes, off, d)
    obj = np.zeros(niter + 1)
    for it in range(niter + 1):
        obj[it] = ((RX.astype(np.float64) - CB) ** 2).sum() / n
        G = X.astype(np.float64).T @ CB.astype(np.float64)          # X CB'
        U, _, Vt = np.linalg.svd(G, full_matrices=False)
        R = np.ascontiguousarray((U @ Vt).T.astype(np.float32))
        RX = oracle.rotate_T(R, X)
        C = float_means(C, RX, codes, off, h)
        codes = encode(oracle, RX, C, m, h)
        CB = reconstruct(C, codes, off, d)
    return C, codes, R, obj


def kmeans_clustering(oracle, Xs, h, maxiter, rng, tol=1e-6):
    """oracle/train_oracle.py::kmeans_clustering -- Clustering.kmeans(Xs, h, init=:kmpp, maxiter=...) as Clustering.jl v0.12.2
    runs it -- with the wide assignment: kmeans++ seeding; per iteration means (an emptied cluster keeps its value) ->
    repick_unused_centers -> assignments -> objv = sum(costs) in Float32; stop when |objv - prev_objv| < tol or at maxiter.
    Draws come from `rng` (a numpy Generator).  Returns (C (h, sub) f32, assignments (n,), objv, iterations)."""
    Xs = np.ascontiguousarray(Xs, dtype=np.float32)
    n, sub = Xs.shape
    X64 = Xs.astype(np.float64)

    def dist_to(c):
        e = X64 - c.astype(np.float64)[None, :]
        return (e * e).sum(1)
    C = np.empty((h, sub), dtype=np.float32)
    j = int(rng.integers(n))
    C[0] = Xs[j]
    mincost = dist_to(C[0])
    for k in range(1, h):
        tot = mincost.sum()
        j = int(np.searchsorted(np.cumsum(mincost), rng.random() * tot, side="right")) if tot > 0 else int(rng.integers(n))
        j = min(j, n - 1)
        C[k] = Xs[j]
        mincost = np.minimum(mincost, dist_to(C[k]))

    def assign(C):
        codes = wo.encode_pq_wide(oracle, Xs, np.ascontiguousarray(C).reshape(-1), 1, h)[:, 0].astype(np.int64)
        e = X64 - C.astype(np.float64)[codes]
        return codes, (e * e).sum(1).astype(np.float32)
    codes, costs = assign(C)
    objv = float(costs.sum(dtype=np.float32))
    it = 0
    while it < maxiter:
        it += 1
        cnt = np.bincount(codes, minlength=h)
        for s in range(sub):
            sums = np.bincount(codes, weights=X64[:, s], minlength=h)
            C[cnt > 0, s] = (sums[cnt > 0] / cnt[cnt > 0]).astype(np.float32)
        unused = np.flatnonzero(cnt == 0)
        if unused.size:
            tc = costs.astype(np.float64).copy()
            for k in unused:
                tot = tc.sum()
                j = int(np.searchsorted(np.cumsum(tc), rng.random() * tot, side="right")) if tot > 0 else int(rng.integers(n))
                j = min(j, n - 1)
                tc[j] = 0.0
                C[k] = Xs[j]
                tc = np.minimum(tc, dist_to(C[k]))
        codes, costs = assign(C)
        prev, objv = objv, float(costs.sum(dtype=np.float32))
        if abs(objv - prev) < tol:
            break
    return C, codes, objv, it


def train_pq_clustering(oracle, X, m, h, niter, seed):
    """train_pq (src/PQ.jl:68-99) by those rules: one kmeans_clustering per sub-space, then qerror_pq of the final assignment."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    off = wo.splitarray(d, m)
    rng = np.random.default_rng(seed)
    C = [kmeans_clustering(oracle, X[:, off[i]:off[i + 1]], h, niter, rng)[0] for i in range(m)]
    codes = encode(oracle, X, C, m, h)
    CB = reconstruct(C, codes, off, d)
    return C, codes, float(((X.astype(np.float64) - CB) ** 2).sum() / n)


# ---- fixtures shared by tests/test_train_wide_oracle.py (CPU) and tests/test_gpu_train_wide.py -----------------------------------
# name -> (X, m, h, seeds, kmeans++ start); integer-valued rows in [0, 255], h > 256
def lloyd_fixture(name):
    from rayuela_jl_amd import synth
    if name == "crowded_uniform_start":      # cost-proportional repicks, many of centres >= 256
        return ko.crowded(n=1500, d=4, seed=6, heavy=1200, npts=4), 1, 300, (1, 2, 3), False
    if name == "five_points":                # fewer distinct points than centres: the uniform branch
        return ko.five_points(n=900, d=4), 1, 300, (3,), True
    if name == "sift":                       # the long plain walk, two sub-spaces
        return synth.sift_like(6000, 16, seed=31), 2, 300, (4,), True
    if name == "one_past_a_block":           # h = 257: one codeword in the second block
        return synth.sift_like(3000, 8, seed=33), 1, 257, (2,), True
    raise KeyError(name)


FIXTURES = ("crowded_uniform_start", "five_points", "sift", "one_past_a_block")
