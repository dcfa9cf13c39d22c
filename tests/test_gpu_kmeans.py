"""The library's k-means (kmeans++ seeding, the Lloyd loop, repick_unused, the stopping rule and the position of the seeded
stream) against tests/kmeans_oracle.py, the step-by-step restatement (tests/test_kmeans_oracle.py checks that one on the CPU).

Three tolerances, no other: exact (seeds, seed sub-vectors, repicked centres, codes, stopping, iteration counts); tau =
(sub + 3) * 2^-24 * total on the cumulative costs of real-valued data (the float32 rounding of a sub-term fmaf chain of squared
float32 differences, summed); and rtol 1e-5 / atol 1e-4 on cluster means, the tolerance tests/test_gpu_train.py states for
update_centers.  The loops are telescoped: train_*(niter = k) is the state after k iterations (the loop is bit-reproducible and
niter only bounds it), and step k + 1 is derived from the library's own state k, so rounding never accumulates."""
import numpy as np
import pytest

import kmeans_oracle as ko
from switch_table import switches

pytestmark = pytest.mark.gpu

DM = [(4, 1), (8, 2), (10, 4), (9, 3), (15, 5), (14, 7), (64, 8), (33, 32), (128, 32)]


def _check_seed_rows(X, m, C, seeds):
    want = ko.seed_subvectors(X, m, seeds)
    for i in range(m):
        assert C[i].dtype == np.float32 and np.array_equal(C[i], want[i]), i


# ---- a. kmeans++ exact on integer data ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,m", DM)
def test_kmpp_exact_on_integer_data(rq, d, m):
    """Vector path and scalar path of kmpp_update (sub-space width no multiple of 4, uneven splits), m not dividing 256,
    m = 32; n = h, one ragged block, one full block, one row more, several blocks."""
    for h in (1, 2, 16):
        for n in sorted({h, 63, 1024, 1025, 4097}):
            X = ko.int_data(n, d, 1000 * d + m)
            seed = 7 * n + h
            seeds, C = rq.kmpp_seeds(X, m, h, seed=seed)
            want = ko.kmpp_seeds(X, m, h, seed)
            assert np.array_equal(seeds, want), (n, h, seeds, want)
            _check_seed_rows(X, m, C, want)


@pytest.mark.parametrize("d,m", [(8, 2), (2, 2)])
@pytest.mark.parametrize("n,tail", [(n, False) for n in ko.BIG_ROWS] + [(n, True) for n in ko.BIG_ROWS[1:]])
def test_kmpp_exact_at_the_block_and_chunk_edges(rq, n, tail, d, m):
    """n > 2^20: kmpp_select walks chunks of more than one row (tests/test_kmeans_oracle.py shows that an off-by-one row or
    a missing min changes a seed of this fixture).  tail: the cost sits in the last rows, so that seeds come from the short
    last block (two rows at 2^20 + 1)."""
    X = ko.big_fixture(n, d, tail)
    seed = ko.BIG_TAIL_SEED if tail else ko.BIG_SEED
    seeds, C = rq.kmpp_seeds(X, m, ko.BIG_H, seed=seed)
    want = ko.kmpp_seeds(X, m, ko.BIG_H, seed)
    assert np.array_equal(seeds, want), (seeds, want)
    _check_seed_rows(X, m, C, want)


# ---- b. degenerate cases, exact -------------------------------------------------------------------------------------------------

def test_kmpp_exact_when_the_cost_runs_out(rq):
    X = ko.five_points()
    n, h = X.shape[0], 16
    for seed in (3, 4, 5):
        seeds, C = rq.kmpp_seeds(X, 1, h, seed=seed)
        want = ko.kmpp_seeds(X, 1, h, seed)
        rng = ko.Rng(seed, ko.SALT_PQ)
        u = [rng.uniform() for _ in range(h)]
        assert [int(r) for r in want[0][5:]] == [min(int(x * n), n - 1) for x in u[5:]]       # 11 steps with total == 0
        assert np.array_equal(seeds, want), (seed, seeds, want)
        _check_seed_rows(X, 1, C, want)
    X2 = ko.five_points(d=8)                       # two sub-spaces run out of cost independently
    seeds, C = rq.kmpp_seeds(X2, 2, h, seed=9)
    want = ko.kmpp_seeds(X2, 2, h, 9)
    assert np.array_equal(seeds, want)
    _check_seed_rows(X2, 2, C, want)
    Z = np.full((500, 8), 3.0, dtype=np.float32)   # all rows identical: every step after the first is the fallback
    for m in (1, 2):
        seeds, C = rq.kmpp_seeds(Z, m, h, seed=1)
        rng = ko.Rng(1, ko.SALT_PQ)
        u = np.array([[rng.uniform() for _ in range(h)] for _ in range(m)])
        assert np.array_equal(seeds, np.minimum((u * 500).astype(np.int64), 499))
        assert np.array_equal(seeds, ko.kmpp_seeds(Z, m, h, 1))
        _check_seed_rows(Z, m, C, seeds)


# ---- c. real-valued data, telescoped on the library's own seeds -----------------------------------------------------------------

def _real_data(kind, n, d):
    import rayuela_jl_amd.synth as synth
    if kind == "sift":
        return synth.sift_like(n, d, seed=51)
    rng = np.random.default_rng(52)
    X = (rng.standard_normal((n, d)) * 30).astype(np.float32)
    X[::7] *= 1e-3                                  # mixed magnitudes
    return X


@pytest.mark.parametrize("kind", ["sift", "gauss_mixed"])
@pytest.mark.parametrize("d,m,h", [(32, 4, 64), (30, 4, 17)])
def test_kmpp_on_real_data_every_step_is_the_threshold_row(rq, kind, d, m, h):
    import rayuela_jl_amd.synth as synth
    n, seed = 20000, 13
    X = _real_data(kind, n, d)
    seeds, C = rq.kmpp_seeds(X, m, h, seed=seed)
    _check_seed_rows(X, m, C, seeds)
    off = synth.splitarray(d, m)
    rng = ko.Rng(seed, ko.SALT_PQ)
    u = [[rng.uniform() for _ in range(h)] for _ in range(m)]
    steps = 0
    for i in range(m):
        Xs = X[:, off[i]:off[i + 1]]
        sub = Xs.shape[1]
        assert seeds[i, 0] == min(int(u[i][0] * n), n - 1)
        mincost = None
        for t in range(1, h):
            prev = int(seeds[i, t - 1])
            c = ko.sub_costs(Xs, Xs[prev])
            mincost = c if mincost is None else np.minimum(mincost, c)
            mincost[prev] = 0.0
            S = np.cumsum(mincost)
            total = S[-1]
            assert total > 0.0
            thr, tau = u[i][t] * total, (sub + 3) * 2.0 ** -24 * total
            s = int(seeds[i, t])
            assert 0 <= s < n
            before = S[s - 1] if s > 0 else 0.0
            assert before <= thr + tau, (i, t, s, (before - thr) / total)
            assert S[s] >= thr - tau, (i, t, s, (thr - S[s]) / total)
            assert mincost[s] > 0.0, (i, t, s)
            steps += 1
    assert steps == m * (h - 1)


# ---- d / e. the Lloyd loop, telescoped over niter; stopping ---------------------------------------------------------------------

def _telescope(train, quant, X, m, h, rng, rows, oracle, stats, kmax=250):
    """train(k) -> (C list of m (h, sub_i) f32, B (n, m) int16 one-based) after k iterations; `rows` the restated start
    rows, `rng` the restated stream right after the start was drawn.  Walks k = 0, 1, ... until the restated stopping rule
    (codes_k == codes_{k-1}) holds and returns that k with the library's (C_k, B_k)."""
    import rayuela_jl_amd.synth as synth
    C_k, B_k = train(0)
    _check_seed_rows(X, m, C_k, rows)
    prev, k = None, 0
    while True:
        codes = oracle.encode_pq(X, synth.cat_codebooks(C_k), m, h)
        assert np.array_equal(B_k, codes.astype(np.int16) + 1), k
        assert np.array_equal(B_k, quant(X, C_k)), k
        if prev is not None and np.array_equal(codes, prev):
            return k, C_k, B_k
        assert k < kmax
        C_next, repicked, _, counts = ko.lloyd_step(X, C_k, m, h, rng, lambda X_, C_: codes)
        C_k1, B_k1 = train(k + 1)
        for i in range(m):
            used = counts[i] > 0
            assert np.allclose(C_k1[i][used], C_next[i][used], rtol=1e-5, atol=1e-4), (k, i)
            assert np.array_equal(C_k1[i][~used], C_next[i][~used].astype(np.float32)), (k, i, repicked)   # rows of X: exact
        for (_, _, _, branch, margin) in repicked:
            stats[branch] += 1
            if branch == "cost":
                assert margin > 1e-9, (k, margin)
                stats["margin"] = min(stats["margin"], margin)
        prev, C_k, B_k, k = codes, C_k1, B_k1, k + 1


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


def _lloyd_fixture(name):
    import rayuela_jl_amd.synth as synth
    if name == "sift":
        return synth.sift_like(6000, 32, seed=31), 4, 32, (4,), True
    if name == "five_points":
        return ko.five_points(), 1, 16, (3,), True
    return ko.crowded(), 1, 16, (1, 2, 3), False


@pytest.mark.parametrize("name", ["sift", "five_points", "crowded_uniform_start"])
def test_lloyd_loop_step_by_step_and_stopping(rq, oracle, name):
    """Every iteration of train_pq from the library's own previous state: means within the update_centers tolerance,
    repicked centres exactly the restated rows (so the stream is where the restatement has it), B_k = quantize_pq(X, C_k);
    then the stopping rule: niter = K + 1 and niter = 50 (or more) return the bits of niter = K, and rq_train_profile
    counts K iterations."""
    from rayuela_jl_amd import _lib
    X, m, h, seeds, kmpp = _lloyd_fixture(name)
    n = X.shape[0]
    stats = dict(cost=0, uniform=0, margin=np.inf)
    for seed in seeds:
        with switches(**({} if kmpp else dict(TRAIN_KMPP=0))):
            rng = ko.Rng(seed, ko.SALT_PQ)
            rows = ko.kmpp_seeds(X, m, h, rng=rng) if kmpp else [ko.sample_distinct(rng, n, h) for _ in range(m)]

            def train(k):
                C, B, _ = rq.train_pq(X, m, h, niter=k, seed=seed)
                return C, B

            K, C_K, B_K = _telescope(train, rq.quantize_pq, X, m, h, rng, rows, oracle, stats)
            assert K >= 1
            assert _lib.train_profile()["iterations"] == K              # the last call of the walk was niter = K
            for niter in (K + 1, max(50, K + 7)):
                assert _same(train(niter), (C_K, B_K)), niter
                assert _lib.train_profile()["iterations"] == K, niter
            if K > 1:
                train(K - 1)
                assert _lib.train_profile()["iterations"] == K - 1
        print("%s seed %d: converged at iteration %d; repicks so far: %d cost-proportional, %d uniform; smallest margin %.3g"
              % (name, seed, K, stats["cost"], stats["uniform"], stats["margin"]))
    # each branch of the repick is taken, by the fixture built for it
    if name == "five_points":
        assert stats["uniform"] == 11 and stats["cost"] == 0            # all in iteration 0: next() % n
    if name == "crowded_uniform_start":
        assert stats["cost"] >= 3 * 4                                   # tests/test_kmeans_oracle.py: >= 4 per seed in iteration 0


# ---- f. other entry points ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sift", "five_points"])
def test_train_rvq_one_stage_follows_the_restatement_with_salt_3(rq, oracle, name):
    import rayuela_jl_amd.synth as synth
    X, h, seed = (synth.sift_like(3000, 16, seed=32), 16, 2) if name == "sift" else (ko.five_points(), 16, 3)
    stats = dict(cost=0, uniform=0, margin=np.inf)
    rng = ko.Rng(seed, ko.SALT_RVQ)
    rows = ko.kmpp_seeds(X, 1, h, rng=rng)

    def train(k):
        C, B, _ = rq.train_rvq(X, 1, h, niter=k, seed=seed)
        return C, B

    K, C_K, B_K = _telescope(train, lambda X_, C_: rq.quantize_rvq(X_, C_)[0], X, 1, h, rng, rows, oracle, stats)
    assert K >= 1
    for niter in (K + 1, max(50, K + 7)):
        assert _same(train(niter), (C_K, B_K)), niter
    if name == "five_points":
        assert stats["uniform"] == 11
    assert not np.array_equal(rows, ko.kmpp_seeds(X, 1, h, seed, salt=ko.SALT_PQ))      # the salt matters on this fixture


def test_train_rvq_two_stages_seed_from_one_stream(rq, oracle):
    """niter = 0 on integer data: stage 0 is the kmeans++ rows of X, stage 1 the kmeans++ rows of the float32 residual, drawn
    with the NEXT h uniforms of the same stream (residual coordinates within [-255, 255], d = 8: costs below 2^24)."""
    n, d, h, seed = 700, 8, 16, 5
    X = ko.int_data(n, d, 61)
    C, B, _ = rq.train_rvq(X, 2, h, niter=0, seed=seed)
    rng = ko.Rng(seed, ko.SALT_RVQ)
    s0 = ko.kmpp_seeds(X, 1, h, rng=rng)[0]
    assert np.array_equal(C[0], X[s0])
    b0 = oracle.encode_pq(X, C[0].reshape(-1), 1, h)[:, 0]
    assert np.array_equal(B[:, 0], b0.astype(np.int16) + 1)
    Xr = X - C[0][b0]
    assert np.abs(Xr).max() <= 255 and np.array_equal(Xr, np.round(Xr))
    s1 = ko.kmpp_seeds(Xr, 1, h, rng=rng)[0]
    assert np.array_equal(C[1], Xr[s1])
    assert np.array_equal(B[:, 1], oracle.encode_pq(Xr, C[1].reshape(-1), 1, h)[:, 0].astype(np.int16) + 1)
    assert not np.array_equal(s1, ko.kmpp_seeds(Xr, 1, h, seed, salt=ko.SALT_RVQ)[0])   # a restarted stream draws other rows


@pytest.mark.parametrize("d,m", [(8, 2), (9, 3)])
def test_train_opq_starts_from_sample_distinct_with_salt_2(rq, oracle, d, m):
    """train_opq(niter = 0, "natural") without C0.  Like the reference's `for iter = 0:niter` the call runs one update of R
    and of the centres, so the sampled start C_i = X[sample_distinct(...)] (salt 2, sub-space by sub-space) is not what comes
    back; it is pinned through what it determines: obj[0], the error of the start centres and their assignments -- an exact
    integer sum on integer data, so float32(sum / n) exactly -- and the returned centres, the means of R'X over those start
    assignments (update_centers tolerance; a centre without rows keeps its sampled row exactly)."""
    import rayuela_jl_amd.synth as synth
    n, h, seed = 600, 16, 8
    X = ko.int_data(n, d, 71)
    off = synth.splitarray(d, m)
    rng = ko.Rng(seed, ko.SALT_OPQ)
    rows = [ko.sample_distinct(rng, n, h) for _ in range(m)]
    C0 = ko.seed_subvectors(X, m, rows)
    codes0 = oracle.encode_pq(X, synth.cat_codebooks(C0), m, h)
    err = 0.0
    for i in range(m):
        err += float(((X[:, off[i]:off[i + 1]].astype(np.float64) - C0[i].astype(np.float64)[codes0[:, i]]) ** 2).sum())
    C, B, R, obj = rq.train_opq(X, m, h, 0, "natural", seed=seed)
    assert obj.shape == (1,) and obj[0] == np.float32(err / n), (obj, err / n)
    other = ko.Rng(seed, ko.SALT_PQ)
    assert [ko.sample_distinct(other, n, h) for _ in range(m)] != rows
    RX = rq.rotate(R, X)
    for i in range(m):
        cnt = np.bincount(codes0[:, i], minlength=h)
        sums = np.zeros((h, off[i + 1] - off[i]))
        np.add.at(sums, codes0[:, i], RX[:, off[i]:off[i + 1]].astype(np.float64))
        used = cnt > 0
        assert np.allclose(C[i][used], sums[used] / cnt[used, None], rtol=1e-5, atol=1e-4), i
        assert np.array_equal(C[i][~used], C0[i][~used]), i
    assert np.array_equal(B, rq.quantize_opq(X, R, C))
