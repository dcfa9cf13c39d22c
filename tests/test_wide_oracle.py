"""CPU: tests/wide_oracle.py -- the expected codes of the 16-bit encodes -- against the oracle's own distance matrix, and the
Python mirrors' argument checks for codebooks no Int16 code (or no byte kernel) covers."""
import numpy as np
import pytest

import wide_oracle as wo
import wide_stream_cases  # noqa: F401  (registers the stream cases of the *_wide entry points)


def _int_case(n, d, m, h, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 6, (n, d)).astype(np.float32)
    C = rng.integers(0, 6, (m, h, d // m)).astype(np.float32)
    return X, C.reshape(-1)


@pytest.mark.parametrize("shape", [(500, 12, 4, 300), (300, 16, 2, 1000), (200, 8, 1, 32767)])
def test_helper_equals_the_argmin_of_the_distance_matrix(oracle, shape):
    """Integer data in 0..5: a large share of the (vector, sub-quantizer) pairs has a tied minimum, and winners sit past 255."""
    n, d, m, h = shape
    X, Ccat = _int_case(n, d, m, h, sum(shape))
    U = oracle.pq_distmat(X, Ccat, m, h)
    V = np.where(U > 0, U, 0)
    want = V.argmin(axis=2)
    got, costs = wo.encode_pq_wide(oracle, X, Ccat, m, h, with_costs=True)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(costs, V.min(axis=2))
    tied = ((V == V.min(axis=2, keepdims=True)).sum(axis=2) > 1).mean()
    assert tied > 0.1 and (got >= 256).any(), (tied, (got >= 256).mean())          # the data does what it is here for


@pytest.mark.parametrize("h", [77, 256])
def test_helper_equals_the_oracle_up_to_256_codewords(oracle, h):
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(700, 30, seed=5)
    rng = np.random.default_rng(h)
    off = wo.splitarray(30, 4)                     # uneven: 8, 8, 7, 7
    Ccat = np.concatenate([X[rng.integers(0, 700, h), off[i]:off[i + 1]].reshape(-1) for i in range(4)])
    assert np.array_equal(wo.encode_pq_wide(oracle, X, Ccat, 4, h), oracle.encode_pq(X, Ccat, 4, h).astype(np.int16))
    Cs = (rng.standard_normal((3, h, 30)) * 20 + 60).astype(np.float32)
    c0, n0, r0 = oracle.encode_rvq(X, Cs, with_extras=True)
    c1, n1, r1 = wo.encode_rvq_wide(oracle, X, Cs)
    assert np.array_equal(c1, c0.astype(np.int16)) and np.array_equal(n1, n0)
    assert np.array_equal(r1.view(np.uint32), r0.view(np.uint32))


def _never(*a, **k):
    raise AssertionError("the library was touched")


def test_more_codewords_than_int16_names_is_a_value_error(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    monkeypatch.setattr(_lib, "lib", _never)
    h, d = 40000, 4
    X = np.zeros((8, d), dtype=np.float32)
    C = [np.zeros((h, 2), dtype=np.float32)] * 2
    for call in (lambda: rq.quantize_pq(X, C), lambda: rq.quantize_pq_u16(X, C),
                 lambda: rq.quantize_opq(X, np.eye(d, dtype=np.float32), C),
                 lambda: rq.quantize_opq_u16(X, np.eye(d, dtype=np.float32), C),
                 lambda: rq.quantize_rvq(X, [np.zeros((h, d), dtype=np.float32)]),
                 lambda: rq.quantize_rvq_u16(X, [np.zeros((h, d), dtype=np.float32)])):
        with pytest.raises(ValueError, match="Int16"):
            call()


def test_byte_rows_with_wide_codebooks_are_a_value_error(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    monkeypatch.setattr(_lib, "lib", _never)
    h, d = 300, 4
    X = np.zeros((8, d), dtype=np.uint8)
    C = [np.zeros((h, 2), dtype=np.float32)] * 2
    with pytest.raises(ValueError, match="h <= 256"):
        rq.quantize_pq(X, C)
    with pytest.raises(ValueError, match="h <= 256"):
        rq.quantize_opq(X, np.eye(d, dtype=np.float32), C)
    with pytest.raises(ValueError, match="h <= 256"):
        rq.quantize_rvq(X, [np.zeros((h, d), dtype=np.float32)])
