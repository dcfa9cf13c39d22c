"""CPU: tests/knn_oracle.py -- the numpy restatement the GPU ground-truth tests compare against -- is pinned here against an
independent float64 brute force, against exact integer arithmetic, against its own error bound, and the near-tie generator is
shown to be sharp (float32 alone gets most of its queries wrong), so that tests/test_gpu_knn.py cannot pass vacuously."""
import numpy as np
import pytest

import knn_oracle as ko
from rayuela_jl_amd import synth


def _fixtures():
    yield "sift_like", synth.sift_like(700, 128, seed=5), synth.sift_like(9, 128, seed=6)
    yield "deep_like", synth.deep_like(700, 96, seed=5), synth.deep_like(9, 96, seed=6)
    for d in (6, 30, 96, 131):
        X, Q = ko.near_tie(d)
        yield "near_tie_d%d" % d, X, Q


def test_d64_order_equals_an_independent_brute_force():
    for name, X, Q in _fixtures():
        k = 10
        dists, ids = ko.groundtruth(X, Q, k)
        D = ((X.astype(np.float64)[None, :, :] - Q.astype(np.float64)[:, None, :]) ** 2).sum(axis=2)
        for q in range(Q.shape[0]):
            order = np.lexsort((np.arange(X.shape[0]), D[q]))[:k]
            # numpy's pairwise sum and the sequential chain differ in the last bits: the order may differ only among rows
            # whose brute-force distances are within that rounding of one another
            if not np.array_equal(order, ids[q]):
                assert np.allclose(D[q][order], D[q][ids[q].astype(np.int64)], rtol=1e-12, atol=0), (name, q)
            assert np.allclose(dists[q], D[q][ids[q].astype(np.int64)], rtol=1e-12, atol=0), (name, q)
    # where every operation is exact (integers) the two orders are the same list
    X = synth.sift_like(500, 128, seed=7)
    Q = synth.sift_like(7, 128, seed=8)
    dists, ids = ko.groundtruth(X, Q, 20)
    D = ((X.astype(np.float64)[None, :, :] - Q.astype(np.float64)[:, None, :]) ** 2).sum(axis=2)
    for q in range(Q.shape[0]):
        order = np.lexsort((np.arange(X.shape[0]), D[q]))[:20]
        assert np.array_equal(order, ids[q]) and np.array_equal(D[q][order], dists[q])


def test_integer_data_is_exact_in_float32():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 256, (300, 128)).astype(np.uint8)
    Q = rng.integers(0, 256, (11, 128)).astype(np.float32)
    a, b = ko.d32(X, Q), ko.d64(X, Q)
    assert a.dtype == np.float32 and b.dtype == np.float64
    assert np.array_equal(a.astype(np.float64), b)           # below 2^24: every f32 operation is exact
    assert np.array_equal(ko.d32(X.astype(np.float32), Q), a)


def test_error_bound_holds_on_every_fixture():
    for name, X, Q in _fixtures():
        d = X.shape[1]
        a, b = ko.d32(X, Q).astype(np.float64), ko.d64(X, Q)
        viol = np.abs(a - b) > ko.gamma(d) * b + ko.delta(d)
        assert int(viol.sum()) == 0, (name, int(viol.sum()))


def test_padding_and_nan_rules_of_the_f64_list():
    D = np.array([[3.0, np.nan, 0.0, np.inf, 3.0]])
    dists, ids = ko.topk_f64(D, 5, id_base=1)
    assert ids.tolist() == [[3, 1, 5, 4, 0]] and dists.tolist() == [[0.0, 3.0, 3.0, np.inf, np.inf]]


@pytest.mark.parametrize("d", [30, 96, 131])
def test_near_tie_generator_is_sharp(d):
    X, Q = ko.near_tie(d)
    assert X.shape == (1500, d) and Q.shape == (24, d)
    k = 10
    a, b = ko.d32(X, Q), ko.d64(X, Q)
    ids32 = ko.topk_f32(a, k)[1]
    ids64 = ko.topk_f64(b, k)[1]
    differ = int((ids32 != ids64).any(axis=1).sum())
    need = [ko.candidates_needed(a[q], b[q], k, d) for q in range(Q.shape[0])]
    print("d=%d: %d of %d queries differ in f32; candidates needed %d..%d" % (d, differ, Q.shape[0], min(n for n, _ in need),
                                                                           max(n for n, _ in need)))
    assert differ * 2 >= Q.shape[0]
    assert any(rounds > 0 for _, rounds in need)              # more than k + 32 candidates
    assert all(n < 1500 for n, _ in need)                     # ... but never the whole base: the certificate does the work
