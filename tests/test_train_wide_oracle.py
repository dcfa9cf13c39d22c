"""CPU: tests/train_wide_oracle.py -- the restatement tests/test_gpu_train_wide.py holds the library to -- pins, from the
restatement alone, that the fixtures reach the branches they are there for: centres past index 255, both repick branches with
centres >= 256 among the re-drawn ones, a long plain walk, one codeword in the second block of 256.  The figures are those of
the exact formula float32(sum) * (float32(1) / float32(count)); the GPU test asserts the same ones on the library."""
import numpy as np
import pytest

import kmeans_oracle as ko
import train_wide_oracle as two
import train_wide_stream_cases  # noqa: F401  (registers the stream cases of the *_wide training reductions)
import wide_oracle as wo

# name -> per seed (K, cost-proportional repicks, uniform repicks, repicks of centres >= 256)
WALKS = {
    "crowded_uniform_start": {1: (5, 251, 0, 41), 2: (5, 259, 0, 39), 3: (5, 251, 0, 36)},
    "five_points": {3: (1, 0, 295, 44)},
    "sift": {4: (27, 0, 0, 0)},
    "one_past_a_block": {2: (18, 0, 0, 0)},
}
MARGINS = {1: 2.7e-5, 2: 3.5e-6, 3: 7.4e-6}        # crowded: the smallest draw margin per seed, to two digits
RVQ_K = 15                                          # one_past_a_block through train_rvq: salt 3


@pytest.mark.parametrize("name", two.FIXTURES)
def test_fixtures_reach_their_branches(oracle, name):
    X, m, h, seeds, kmpp = two.lloyd_fixture(name)
    assert h > 256 and np.array_equal(X, np.round(X)) and X.min() >= 0 and X.max() <= 255
    for seed in seeds:
        K, Cs, codes, rows, st = two.walk(oracle, X, m, h, seed, kmpp=kmpp)
        assert (K, st["cost"], st["uniform"], st["wide"]) == WALKS[name][seed], (seed, K, st)
        assert len(Cs) == K + 1 and len(codes) == K + 1
        if name == "crowded_uniform_start":
            assert st["margin"] > 1e-9 and abs(st["margin"] / MARGINS[seed] - 1) < 0.05, st["margin"]
        if name in ("sift", "crowded_uniform_start"):
            assert (codes[-1] >= 256).any()                             # rows are assigned to centres of the second block
        if name == "one_past_a_block":
            assert h == 257 and (codes[-1] == 256).any() and int(np.bincount(codes[-1][:, 0], minlength=h)[256]) > 0
        if name == "five_points":
            assert len({tuple(r) for r in X.tolist()}) == 5 < h


def test_one_past_a_block_with_the_rvq_salt(oracle):
    X, m, h, (seed,), kmpp = two.lloyd_fixture("one_past_a_block")
    K, _, codes, rows, st = two.walk(oracle, X, 1, h, seed, salt=ko.SALT_RVQ, kmpp=True)
    assert (K, st["cost"], st["uniform"]) == (RVQ_K, 0, 0)
    assert not np.array_equal(rows, two.start_rows(X, 1, h, seed, ko.SALT_PQ, True)[0])       # the salt matters here


def test_exact_means_formula_and_out_of_range_codes():
    """float32(sum) * (float32(1) / float32(count)), NOT the rounded float64 quotient: the two differ on this data, so a
    test that holds the library to the bits does say which formula it runs.  Codes outside [0, h) -- negative ones too -- are
    ignored in their sub-space only; a code without rows keeps its bits."""
    n, d, m, h = 4000, 6, 2, 300
    X = ko.int_data(n, d, 5)
    rng = np.random.default_rng(2)
    codes = rng.integers(0, h - 10, (n, m)).astype(np.int16)              # the last ten codes have no rows
    C0 = [rng.standard_normal((h, 3)).astype(np.float32) for _ in range(m)]
    C, counts = two.exact_means(X, C0, codes, m, h)
    off = wo.splitarray(d, m)
    quot = 0
    for i in range(m):
        assert np.array_equal(counts[i], np.bincount(codes[:, i], minlength=h)) and (counts[i][-10:] == 0).all()
        assert np.array_equal(C[i][-10:].view(np.uint32), C0[i][-10:].view(np.uint32))
        for k in (0, 7, 255, 256, 289):
            sel = codes[:, i] == k
            s = X[sel, off[i]:off[i + 1]].astype(np.float64).sum(0)
            assert np.array_equal(C[i][k], s.astype(np.float32) * (np.float32(1) / np.float32(sel.sum())))
        used = counts[i] > 0
        sums = np.stack([np.bincount(codes[:, i], weights=X[:, s].astype(np.float64), minlength=h) for s in range(off[i], off[i + 1])], 1)
        quot += int((C[i][used] != (sums[used] / counts[i][used, None]).astype(np.float32)).sum())
    assert quot > 0
    bad = codes.copy()
    rows = np.arange(0, n, 10)
    bad[rows, 0] = np.array([-1, h, h + 255, 32767], dtype=np.int16)[np.arange(rows.size) % 4]
    Cb, cb = two.exact_means(X, C0, bad, m, h)
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    Ck, ck = two.exact_means(X[keep], C0, codes[keep], m, h)
    assert two.same_bits([Cb[0]], [Ck[0]]) and np.array_equal(cb[0], ck[0])
    assert two.same_bits([Cb[1]], [C[1]]) and np.array_equal(cb[1], counts[1])


def test_opq_restatement_equals_the_byte_one_up_to_256_codewords(oracle):
    from oracle import train_oracle as to
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(1500, 8, seed=4)
    R0 = synth.rotation(8, seed=5)
    C0 = synth.codebooks(oracle.rotate_T(R0, X), 2, 32, seed=9, iters=0, sample=500)
    a = two.train_opq(oracle, X, 2, 32, 2, R0, C0)
    b = to.train_opq(X, 2, 32, 2, R0, C0, fast=True)
    assert two.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1].astype(np.int16))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_python_front_ends_refuse_more_codewords_than_int16_names(rq, monkeypatch):
    from rayuela_jl_amd import _lib

    def never(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", never)
    X = np.zeros((8, 4), dtype=np.float32)
    for call in (lambda: rq.train_pq(X, 2, 40000), lambda: rq.train_rvq(X, 2, 40000),
                 lambda: rq.train_opq(X, 2, 40000, 1, "natural")):
        with pytest.raises(ValueError, match="Int16"):
            call()
