"""CPU tests of tests/kmeans_oracle.py, the restatement that tests/test_gpu_kmeans.py holds the library's k-means to: known
answers, a brute-force version in exact arithmetic, the D^2 law, and proof that the GPU fixtures tell the true rule from its
near misses (the mutated rules live here, as variants of the restatement; nothing in the library is mutated)."""
from fractions import Fraction

import numpy as np
import pytest

import kmeans_oracle as ko
from rayuela_jl_amd import synth


def test_rng_known_answers():
    r = ko.Rng(0, 0)
    assert r.s == 0
    assert r.next() == 0xE220A8397B1DCDAF                              # splitmix64's first output from state 0
    assert r.next() == 0x6E789E6AA1B965F4
    # synth.splitmix64(state) is next() from `state`; the start state is seed * gamma + salt mod 2^64
    for seed, salt in [(0, 1), (1, 2), (12345, 3), (2 ** 63 + 5, 1)]:
        r = ko.Rng(seed, salt)
        s0 = (seed * ko.GOLDEN_GAMMA + salt) % 2 ** 64
        assert r.s == s0
        assert r.next() == int(synth.splitmix64(np.uint64(s0)))
        s1 = (s0 + ko.GOLDEN_GAMMA) % 2 ** 64
        v = int(synth.splitmix64(np.uint64(s1)))
        assert r.uniform() == (v >> 11) / 2.0 ** 53
    us = [ko.Rng(7, 1).uniform() for _ in range(3)]
    assert all(0.0 <= u < 1.0 for u in us)


@pytest.mark.parametrize("n,h", [(16, 16), (1, 1), (17, 16), (1_000_000, 16), (300, 256)])
def test_sample_distinct(n, h):
    out = ko.sample_distinct(ko.Rng(3, 2), n, h)
    assert len(out) == h and len(set(out)) == h and min(out) >= 0 and max(out) < n
    if n == h:
        assert sorted(out) == list(range(n))
    # the sparse swap map is a Fisher-Yates on the dense array
    rng, a, ref = ko.Rng(3, 2), list(range(n)) if n <= 1000 else None, []
    if a is not None:
        for i in range(h):
            j = i + rng.next() % (n - i)
            a[i], a[j] = a[j], a[i]
            ref.append(a[i])
        assert out == ref


def _kmpp_exact(X, m, h, seed, salt=1):
    """kmeans++ in Python ints and Fractions: no floating point beyond the uniforms themselves (exact binary fractions)."""
    n, d = X.shape
    off = [int(o) for o in synth.splitarray(d, m)]
    rng = ko.Rng(seed, salt)
    u = [[Fraction(rng.next() >> 11, 2 ** 53) for _ in range(h)] for _ in range(m)]
    Xi = [[int(v) for v in row] for row in X.tolist()]
    seeds = []
    for i in range(m):
        s = min(int(u[i][0] * n), n - 1)
        row, mincost = [s], None
        for t in range(1, h):
            c = [sum((Xi[j][k] - Xi[s][k]) ** 2 for k in range(off[i], off[i + 1])) for j in range(n)]
            mincost = c if mincost is None else [min(a, b) for a, b in zip(mincost, c)]
            mincost[s] = 0
            total = sum(mincost)
            if total == 0:
                s = min(int(u[i][t] * n), n - 1)
            else:
                # the library forms the threshold in float64: u * total rounded once
                thr, run = Fraction(float(u[i][t]) * float(total)), 0
                for j in range(n):
                    run += mincost[j]
                    if run > thr:
                        s = j
                        break
            row.append(s)
        seeds.append(row)
    return np.asarray(seeds, dtype=np.int64)


@pytest.mark.parametrize("n,d,m,h", [(40, 4, 1, 8), (63, 10, 4, 16), (50, 9, 3, 5), (16, 8, 2, 16), (30, 2, 2, 30)])
def test_kmpp_seeds_equals_brute_force_in_exact_arithmetic(n, d, m, h):
    for seed in (0, 1, 2):
        X = ko.int_data(n, d, 100 + seed)
        X[n // 2] = X[0]                                               # a duplicate row: its cost is 0 once row 0 is a seed
        assert np.array_equal(ko.kmpp_seeds(X, m, h, seed), _kmpp_exact(X, m, h, seed))
    Z = np.repeat(ko.int_data(3, d, 9), [n - 4, 2, 2], axis=0)         # 3 distinct points: total == 0 from step 3 on
    assert np.array_equal(ko.kmpp_seeds(Z, m, h, 4), _kmpp_exact(Z, m, h, 4))


def test_second_seed_follows_the_d2_law():
    """6 points on a line; over 2000 seeds the second seed's frequencies against the exact law
    P(j) = sum_i 1/6 * D2(i, j) / sum_k D2(i, k), slack 4 standard deviations of the binomial."""
    pts = np.array([0, 1, 3, 7, 20, 21], dtype=np.float32).reshape(6, 1)
    D2 = (pts - pts.T).astype(np.float64) ** 2
    P = (D2 / D2.sum(1, keepdims=True)).mean(0)
    N = 2000
    first, second = np.zeros(6), np.zeros(6)
    for seed in range(N):
        s = ko.kmpp_seeds(pts, 1, 2, seed)[0]
        assert s[0] != s[1]
        first[s[0]] += 1
        second[s[1]] += 1
    assert abs(P.sum() - 1.0) < 1e-12
    for j in range(6):
        assert abs(first[j] / N - 1 / 6) <= 4 * np.sqrt((1 / 6) * (5 / 6) / N), (j, first)
        assert abs(second[j] / N - P[j]) <= 4 * np.sqrt(P[j] * (1 - P[j]) / N), (j, second, P)


# ---- the fixtures of the GPU tests tell the true rules from their near misses ------------------------------------------------

def _repick_variant(X_sub, C_old_sub, C_new_sub, codes, unused, rng, costs_from="old", lower=True, draw_next=True):
    """ko.repick with switchable mistakes: costs against the NEW centres, costs not lowered between draws, uniform() drawn
    without the preceding next()."""
    n = X_sub.shape[0]
    C = C_old_sub if costs_from == "old" else C_new_sub
    tc = ((X_sub.astype(np.float64) - np.asarray(C, dtype=np.float64)[codes]) ** 2).sum(1)
    picks = []
    for _ in unused:
        S = np.cumsum(tc)
        total = S[-1]
        pick = rng.next() % n if (draw_next or not total > 0.0) else None
        if total > 0.0:
            j = ko.first_above(S, rng.uniform() * total)
            pick = j if j < n else n - 1
        picks.append(int(pick))
        tc[pick] = 0.0
        if lower:
            tc = np.minimum(tc, ko.sub_costs(X_sub, X_sub[pick]))
    return picks


def _numpy_encode(X, C):
    """plain float64 nearest centre, ties to the lowest index (integer fixtures: exact)."""
    off = synth.splitarray(X.shape[1], len(C))
    cols = []
    for i, Ci in enumerate(C):
        Xs = X[:, off[i]:off[i + 1]].astype(np.float64)
        dm = ((Xs[:, None, :] - np.asarray(Ci, dtype=np.float64)[None, :, :]) ** 2).sum(-1)
        cols.append(dm.argmin(1))
    return np.stack(cols, axis=1).astype(np.uint8)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_repick_fixture_discriminates(seed):
    """The TRAIN_KMPP = 0 fixture of the Lloyd test: its first iteration repicks through the cost-proportional branch, and
    each of three mistaken rules gives another pick list."""
    X, m, h = ko.crowded(), 1, 16
    rng = ko.Rng(seed, ko.SALT_PQ)
    C0 = ko.seed_subvectors(X, m, [ko.sample_distinct(rng, X.shape[0], h)])
    state = rng.s
    C1, repicked, codes, counts = ko.lloyd_step(X, C0, m, h, rng, _numpy_encode)
    unused = [k for (_, k, _, _, _) in repicked]
    true = [row for (_, _, row, _, _) in repicked]
    ncost = sum(1 for r in repicked if r[3] == "cost")
    print("seed %d: %d repicks, %d cost-proportional, smallest margin %.3g"
          % (seed, len(repicked), ncost, min(r[4] for r in repicked if r[3] == "cost")))
    assert ncost >= 4 and unused == sorted(unused) and all(counts[0][k] == 0 for k in unused)
    assert all(r[4] > 1e-9 for r in repicked if r[3] == "cost")
    C1_means = [np.where((counts[0] > 0)[:, None], C1[0], C0[0])]       # the centres as update_centers leaves them

    def run(**kw):
        r = ko.Rng(0, 0)
        r.s = state
        return _repick_variant(X, C0[0], C1_means[0], codes[:, 0], unused, r, **kw)

    assert run() == true                                               # the variant without a mistake is the restatement
    assert run(costs_from="new") != true
    assert run(lower=False) != true
    assert run(draw_next=False) != true


def _kmpp_variant(X, m, h, seed, shift=0, keep_min=True):
    """ko.kmpp_seeds with switchable mistakes: the row after the right one, mincost overwritten instead of min-reduced."""
    n, d = X.shape
    off = synth.splitarray(d, m)
    rng = ko.Rng(seed, ko.SALT_PQ)
    u = [[rng.uniform() for _ in range(h)] for _ in range(m)]
    seeds = np.empty((m, h), dtype=np.int64)
    for i in range(m):
        Xs = X[:, off[i]:off[i + 1]]
        s = min(int(u[i][0] * n), n - 1)
        seeds[i, 0] = s
        mincost = None
        for t in range(1, h):
            c = ko.sub_costs(Xs, Xs[s])
            mincost = c if (mincost is None or not keep_min) else np.minimum(mincost, c)
            mincost[s] = 0.0
            S = np.cumsum(mincost)
            s = min(ko.first_above(S, u[i][t] * S[-1]) + shift, n - 1)
            seeds[i, t] = s
    return seeds


@pytest.mark.parametrize("d", [8, 2])
def test_big_seeding_fixture_discriminates(d):
    n = ko.BIG_ROWS[1]
    X = ko.big_fixture(n, d)
    assert X.shape == (n, d) and X.min() >= 0 and X.max() <= 255 and np.array_equal(X, np.round(X))
    true = ko.kmpp_seeds(X, 2, ko.BIG_H, ko.BIG_SEED)
    assert np.array_equal(_kmpp_variant(X, 2, ko.BIG_H, ko.BIG_SEED), true)
    assert not np.array_equal(_kmpp_variant(X, 2, ko.BIG_H, ko.BIG_SEED, shift=1), true)
    assert not np.array_equal(_kmpp_variant(X, 2, ko.BIG_H, ko.BIG_SEED, keep_min=False), true)
    # every cost below 2^24, every sum below 2^53: the premise of "exact"
    assert (X.shape[1] // 2) * 255 ** 2 < 2 ** 24 and n * (X.shape[1] // 2) * 255 ** 2 < 2 ** 53


@pytest.mark.parametrize("d", [8, 2])
@pytest.mark.parametrize("n", ko.BIG_ROWS[1:])
def test_tail_fixture_draws_from_the_last_block(n, d):
    rows, nblk = ko.kmpp_blocks(n)
    assert nblk == 1024 and 0 < n - (nblk - 1) * rows < rows           # a short last block (two rows at 2^20 + 1)
    assert (n - (nblk - 1) * rows == 2) == (n == (1 << 20) + 1)
    X = ko.big_fixture(n, d, tail=True)
    assert X.min() == 0 and X.max() == 255 and np.array_equal(X, np.round(X))
    s = ko.kmpp_seeds(X, 2, ko.BIG_H, ko.BIG_TAIL_SEED)
    assert (s >= (nblk - 1) * rows).any() and (s < (nblk - 1) * rows).any(), s


def test_degenerate_fixture_runs_out_of_cost():
    X = ko.five_points()
    assert len({tuple(r) for r in X.tolist()}) == 5
    s = ko.kmpp_seeds(X, 1, 16, 3)[0]
    assert len({tuple(X[r].tolist()) for r in s[:5]}) == 5            # the first five seeds are the five points
    rng = ko.Rng(3, ko.SALT_PQ)
    u = [rng.uniform() for _ in range(16)]
    assert [int(r) for r in s[5:]] == [min(int(x * 300), 299) for x in u[5:]]     # 11 steps with total == 0
    C0 = ko.seed_subvectors(X, 1, [s])
    _, repicked, _, _ = ko.lloyd_step(X, C0, 1, 16, rng, _numpy_encode)
    assert len(repicked) == 11 and all(r[3] == "uniform" for r in repicked)
