"""CPU: the restatement of beam encoding over wide codebooks (tests/beam_wide_oracle.py) against the facts it was checked
with: it equals tests/beam_oracle.py at h <= 256 and the wide RVQ restatement at H = 1, a wider beam encodes better, and the
tie fixtures put equal candidates at the boundary of the beam at every (shape, H) the GPU tie test uses."""
import numpy as np
import pytest

import beam_oracle as bo
import beam_wide_oracle as bw
import beam_wide_stream_cases  # noqa: F401  (registers the wide beam case with tests/stream_cases.py)
import wide_oracle as wo

FIRST, SECOND = bw.TIE_SHAPES


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", [(1_000, 30, 3, 64, "sift"), (33, 16, 2, 16, "deep")])
@pytest.mark.parametrize("H", [1, 3, 16])
def test_equals_the_byte_restatement_up_to_256_codewords(oracle, shape, H):
    X, C = bo.data(*shape)
    c0, r0, v0 = bo.encode(X, C, H)
    c1, r1, v1 = bw.encode(X, C, H)
    assert c1.dtype == np.int16 and np.array_equal(c1, c0.astype(np.int16))
    assert np.array_equal(_bits(r0), _bits(r1)) and np.array_equal(_bits(v0), _bits(v1))


@pytest.mark.parametrize("shape", bw.TIE_SHAPES)
def test_beam_of_one_is_the_wide_rvq_restatement(oracle, shape):
    X, C = bw.data(*shape)
    c, r, _ = bw.encode(X, C, 1)
    c2, _, r2 = wo.encode_rvq_wide(oracle, X, C)
    assert np.array_equal(c, c2) and np.array_equal(_bits(r), _bits(r2))
    assert int(c.max()) >= 256                                      # the second block is in use


def test_a_wider_beam_encodes_better(oracle):
    X, C = bw.data(*FIRST)
    e = [bo.qerror(X, C, bw.encode(X, C, H)[0]) for H in (1, 3, 32)]
    print("qerror at H = 1, 3, 32:", e)
    assert np.allclose(e, [0.2851, 0.2735, 0.2617], atol=5e-5) and e[0] > e[1] > e[2]


@pytest.mark.parametrize("shape,want", [(FIRST, (0.245, 0.11, 0.04)), (SECOND, (0.5225, 0.455, 0.435))])
def test_tie_fixtures_put_ties_at_the_boundary_of_the_beam(oracle, shape, want):
    X, C = bw.tie_fixture(shape)
    h = shape[3]
    for i in range(1, shape[2]):
        assert np.array_equal(C[i][h - 1], C[i][5]) and not C[i][20].any() and not C[i][h - 40].any()
        assert 5 // 256 != (h - 1) // 256                           # the duplicates sit in different blocks of 256 codewords
    for H, w in zip(bw.TIE_BEAMS, want):
        share = bw.boundary_tie_share(X, C, H)
        print(shape, H, share)
        assert share >= 0.03 and abs(share - w) < 5e-3
