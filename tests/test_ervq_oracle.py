"""CPU: the two numpy restatements of train_ervq (tests/ervq_oracle.py) against each other -- no library, no device.

The library computes the codebook update as an increment by the mean residual; the reference computes the mean of
Xd = X - sum_{i != j} C_i[b_i].  These tests show that the two are the same loop (traces, codebooks and codes), that
B == quantize_rvq(X, C) after every iteration, and that the fixture of the GPU tests improves on its start.  The spread
measured between `literal` (f64 means) and `incremental` (f32) on that fixture is printed: the bars of
tests/test_gpu_ervq.py::test_train_ervq_follows_the_restatement are ten times these figures (capped)."""
import numpy as np
import pytest

import ervq_oracle as eo


@pytest.fixture(scope="module")
def runs(oracle):
    X, codes, C = eo.fixture(oracle.encode_rvq)
    lit = eo.literal(X, codes, C, eo.FIX_NITER, oracle.encode_rvq)
    inc32 = eo.incremental(X, codes, C, eo.FIX_NITER, oracle.encode_rvq, np.float32)
    inc64 = eo.incremental(X, codes, C, eo.FIX_NITER, oracle.encode_rvq, np.float64)
    return X, codes, C, lit, inc32, inc64


def test_incremental_equals_literal_on_the_gpu_fixture(runs):
    X, codes, C, lit, inc32, inc64 = runs
    s64, s32 = eo.spread(lit, inc64), eo.spread(lit, inc32)
    print("literal f64 vs incremental f64: trace %.3e  worst entry %.3e  differing codes %.3e" % s64)
    print("literal f64 vs incremental f32: trace %.3e  worst entry %.3e  differing codes %.3e" % s32)
    print("trace (literal):", np.array2string(lit[2], precision=4))
    # f64 means of f32 data: the two forms differ by the f32 rounding of Xd and E only (data of magnitude ~200: ulp 1.5e-5)
    for s in (s64, s32):
        assert s[0] <= 1e-6 and s[1] <= 1e-3 and s[2] <= 1e-3, s


@pytest.mark.parametrize("n,d,m,h", [(3000, 16, 3, 16), (2500, 7, 2, 8), (2000, 24, 1, 16)])
def test_incremental_equals_literal_on_small_shapes(oracle, n, d, m, h):
    X, codes, C = eo.fixture(oracle.encode_rvq, n, d, m, h, seed=7)
    lit = eo.literal(X, codes, C, 2, oracle.encode_rvq)
    for acc in (np.float64, np.float32):
        s = eo.spread(lit, eo.incremental(X, codes, C, 2, oracle.encode_rvq, acc))
        print(acc.__name__, "trace %.3e  worst entry %.3e  differing codes %.3e" % s)
        assert s[0] <= 1e-6 and s[1] <= 1e-3 and s[2] <= 2e-3, s


def test_codes_equal_quantize_rvq_after_every_iteration(runs):
    X, codes, C, lit, inc32, inc64 = runs
    for r in (lit, inc32, inc64):
        assert r[3] == [True] * eo.FIX_NITER


def test_the_gpu_fixture_improves_on_its_start(runs):
    X, codes, C, lit, inc32, inc64 = runs
    for r in (lit, inc32):
        obj = r[2]
        assert obj.shape == (eo.FIX_NITER * eo.FIX_M + 1,)
        assert obj[-1] < 0.99 * obj[0], obj            # the end against the start; single steps may go up


def test_update_of_a_single_codebook_is_the_class_mean(oracle):
    """m = 1: Xd is X itself, the literal update is the plain class mean."""
    X, codes, C = eo.fixture(oracle.encode_rvq, 2000, 24, 1, 16, seed=7)
    new, cnt = eo.literal_update(X, codes, C, 0)
    for k in range(16):
        if cnt[k]:
            assert np.allclose(new[k], X[codes[:, 0] == k].astype(np.float64).mean(0), rtol=1e-12)
