"""CPU: the numpy restatement of the database-norms kernels (tests/norms_oracle.py) against independent evaluations -- the f64
value of |sum C_k[b_k]|^2 with its derived bound, and the literal findmin loop of src/utils.jl:50-55."""
import numpy as np
import pytest

import icm_oracle
import norms_oracle as no
import norms_stream_cases  # noqa: F401  (completes the table that tests/test_gpu_streams.py checks against the header)


@pytest.mark.parametrize("n,d,m,h", [s for s in no.NORM_SHAPES if s[2] <= 8 and s[1] <= 128])
def test_integer_codebooks_equal_f64_exactly(n, d, m, h):
    """Entries of magnitude <= 31, m <= 8, d <= 128: |CB[t]| <= 248, CB[t]^2 <= 61504, the whole sum <= 128 * 61504 < 2^24, so
    every f32 partial sum is an exactly represented integer."""
    codes, C = no.norm_case(n, d, m, h, integer=True)
    got = no.aq_norms(codes, C)
    assert np.array_equal(got.astype(np.float64), no.norms_f64(codes, C))


@pytest.mark.parametrize("n,d,m,h", no.NORM_SHAPES)
def test_gaussian_codebooks_stay_within_the_derived_bound(n, d, m, h):
    codes, C = no.norm_case(n, d, m, h)
    got = no.aq_norms(codes, C).astype(np.float64)
    want = no.norms_f64(codes, C)
    bound = no.norms_bound(codes, C)
    dev = np.abs(got - want)
    print("(%d, %d, %d, %d): worst relative deviation %.3e, worst deviation / bound %.3f"
          % (n, d, m, h, (dev / want).max(), (dev / bound).max()))
    assert (dev <= bound).all()


@pytest.mark.parametrize("n,d,m,h", [s for s in no.NORM_SHAPES if s[2] <= 16])
def test_norms_are_the_veccost_of_a_zero_vector(n, d, m, h):
    """The shipped restatement of veccost (tests/icm_oracle.py) on an all-zero X: the same bits."""
    codes, C = no.norm_case(n, d, m, h)
    want = icm_oracle.veccost(np.zeros((n, d), np.float32), codes, C)
    assert np.array_equal(no.aq_norms(codes, C).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", sorted(no.quant_cases()))
def test_quantize_equals_the_literal_findmin_loop(name):
    norms, cb = no.quant_cases()[name]
    got = no.quantize(norms, cb)
    assert np.array_equal(got, no.findmin_loop(norms, cb))
    assert no.quantize(norms[:0], cb).shape == (0,)


def test_quantize_tie_rules_by_hand():
    norms, cb = no.quant_cases()["duplicates"]
    got = no.quantize(norms, cb)
    assert set(got[norms == 5]) == {0} and set(got[norms == 9]) == {1} and set(got[norms == 30]) == {3}
    assert set(got[norms == 61]) == {7} and set(got[norms == 0]) == {9}
    norms, cb = no.quant_cases()["midpoints"]
    got = no.quantize(norms, cb)
    assert set(got[norms == 10]) == {0}      # 12 (index 0) and 8 (index 1) are equally far: the first listed wins
    assert set(got[norms == 5]) == {2}       # 7 (index 2) before 3 (index 3)
    assert set(got[norms == 8]) == {1} and set(got[norms == 0]) == {3}
    norms, cb = no.quant_cases()["outside_range"]
    got = no.quantize(norms, cb)
    assert set(got[::3]) == {int(np.argmax(cb))} and set(got[1::3]) == {int(np.argmin(cb))}
    norms, cb = no.quant_cases()["hn1"]
    assert not no.quantize(norms, cb).any()
