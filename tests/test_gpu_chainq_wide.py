"""GPU: chain quantization past 256 codewords per codebook (rq_quantize_chainq_wide / rq_update_codebooks_chain_wide /
rq_train_chainq_wide).  The Viterbi codes bit for bit against tests/chain_wide_oracle.py and, at h <= 256,
against the byte entries; the chain update against numpy's f64 block solve within the bounds tests/test_gpu_chainq.py holds the
byte update to; training against the byte loop, against its public steps composed by hand, and end to end through the LSQ driver.

The shapes are the smallest that cross the kernels' boundaries: h = 257 (one past a byte), 300 / 320 (HS larger than / equal to
h, a partial group of 64), 513 / 520 / 1025 / 2049 (several 256-wide tiles of b and slabs of a, a one-element last tile), n no
multiple of 32, m = 1, 2 and 16."""
import numpy as np
import pytest

import chain_oracle as co
import chain_wide_oracle as cw
import lsq_update_oracle as lo

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _wide(X, C, nsplits=1, base=0):
    """rq_quantize_chainq_wide itself: codes int16 in base .. base + h - 1."""
    from rayuela_jl_amd import _lib
    X, C = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(C, np.float32)
    m, h, d = C.shape
    out = np.full((X.shape[0], m), -9, np.int16)
    _lib.check(_lib.lib().rq_quantize_chainq_wide(out.ctypes.data, X.ctypes.data, C.ctypes.data, X.shape[0], d, m, h, nsplits, base))
    return out


def _byte(X, C, nsplits=1):
    from rayuela_jl_amd.ChainQ import quantize_chainq_u8
    return quantize_chainq_u8(X, C, nsplits=nsplits)


def _case(m, h, d, n, scale=0.5):
    rng = np.random.default_rng(m * 1000 + h + d + n)
    return rng.standard_normal((n, d)).astype(np.float32), (rng.standard_normal((m, h, d)) * scale).astype(np.float32)


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,h,d,n", [(1, 257, 7, 5), (2, 257, 7, 70), (3, 300, 16, 65), (4, 513, 24, 33), (8, 320, 32, 40),
                                     (16, 260, 12, 20), (2, 1025, 8, 17), (3, 2049, 4, 9)])
def test_codes_equal_the_restatement(rq, oracle, m, h, d, n):
    X, C = _case(m, h, d, n)
    want = cw.viterbi(oracle, X, C)
    got0, got1 = _wide(X, C), _wide(X, C, base=1)
    assert np.array_equal(got0, want), "rows differ: %d of %d" % (int((got0 != want).any(axis=1).sum()), n)
    assert np.array_equal(got1, want + 1)
    u16 = rq.quantize_chainq_u16(X, C)
    assert u16.dtype == np.uint16 and np.array_equal(u16, want)
    B, elapsed = rq.quantize_chainq(X, list(C), wide=True)
    assert B.dtype == np.int16 and np.array_equal(B, want + 1) and elapsed > 0


def test_no_rows(rq):
    C = np.zeros((4, 300, 8), np.float32)
    assert _wide(np.zeros((0, 8), np.float32), C).shape == (0, 4)
    assert rq.quantize_chainq_u16(np.zeros((0, 8), np.float32), C).shape == (0, 4)


def test_integer_valued_ties(rq, oracle):
    """Integer-valued inputs make equal costs common: the lowest index must win at every stage and in the last argmin."""
    rng = np.random.default_rng(5)
    m, h, d, n = 4, 300, 6, 200
    X = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    C = rng.integers(-1, 2, size=(m, h, d)).astype(np.float32)
    U, T = cw.tables(oracle, X, C)
    assert (np.sort(U[m - 1], axis=1)[:, 0] == np.sort(U[m - 1], axis=1)[:, 1]).any()      # the case does tie
    assert np.array_equal(_wide(X, C), cw.viterbi_tables(U, T))


def test_equal_costs_in_different_tiles(rq, oracle):
    """Codewords k and k + 256 are the same vector, so every cost of k + 256 equals that of k: the copies sit in different tiles of b
    (forward pass) and in different pieces of a lane (back trace), and no code may ever name the copy."""
    m, h, d, n = 3, 520, 8, 64
    X, C = _case(m, h, d, n)
    C[:, 256:512] = C[:, :256]
    want = cw.viterbi(oracle, X, C)
    assert not ((want >= 256) & (want < 512)).any() and (want >= 512).any()      # the rule in the restatement; the last tile is used
    got = _wide(X, C)
    assert np.array_equal(got, want) and not ((got >= 256) & (got < 512)).any()


def _chain_masked(C):
    m, _, d = C.shape
    for i, dims in enumerate(co.cbdims(d, m)):
        out = np.ones(d, dtype=bool)
        out[dims[0]:dims[-1] + 1] = False
        C[i][:, out] = 0
    return C


def test_chain_structured_codebooks_take_the_range_restricted_unaries(rq, oracle):
    """Codebooks that are zero outside a dimension range (odd d, odd bounds, tiles of 32 codewords that span two codebooks at
    h = 300): the unaries run over that range only and must give the same bits; then negative zeros, one all-zero codebook and one
    codebook with a single dimension, as tests/test_gpu_chainq.py does for the byte entry."""
    m, h, d, n = 5, 300, 31, 100
    X, C = _case(m, h, d, n)
    C = _chain_masked(C)
    assert np.array_equal(_wide(X, C), cw.viterbi(oracle, X, C))
    C2 = C.copy()
    C2[C2 == 0] = -0.0
    C2[m - 1] = 0
    C2[0] = 0
    C2[0][:, d - 1] = np.random.default_rng(1).standard_normal(h).astype(np.float32)
    assert np.array_equal(_wide(X, C2), cw.viterbi(oracle, X, C2))


@pytest.mark.parametrize("m,h,d,n", [(8, 256, 32, 100), (5, 65, 30, 129), (2, 2, 7, 50)])
def test_codes_equal_the_byte_entry(rq, m, h, d, n):
    X, C = _case(m, h, d, n)
    assert np.array_equal(_wide(X, C), _byte(X, C))


def test_chunked_runs_give_the_same_codes(rq, oracle):
    from rayuela_jl_amd.ChainQ import last_chainq_timing
    X, C = _case(4, 300, 16, 200)
    one = _wide(X, C)
    t = last_chainq_timing()
    assert t["unary_ms"] > 0 and t["tables_ms"] > 0 and t["viterbi_ms"] > 0 and t["update_ms"] == 0 and t["rotation_ms"] == 0
    assert np.array_equal(one, cw.viterbi(oracle, X, C))
    for ns in (3, 7):
        assert np.array_equal(_wide(X, C, nsplits=ns), one), ns


def test_non_finite_rows_stay_in_range_and_leave_the_others_alone(rq):
    m, h, d, n = 3, 300, 8, 40
    X, C = _case(m, h, d, n)
    clean = X.copy()
    clean[5] = 0
    clean[9] = 0
    X[5, 3] = np.nan
    X[9, 0], X[9, 1] = np.inf, -np.inf
    got, ref = _wide(X, C), _wide(clean, C)
    assert got.min() >= 0 and got.max() <= h - 1
    keep = np.ones(n, dtype=bool)
    keep[[5, 9]] = False
    assert np.array_equal(got[keep], ref[keep])


# ---- the chain codebook update ------------------------------------------------------------------------------------------------------
def _update(X, codes, h, base=0, rho=1e-4):
    from rayuela_jl_amd import _lib
    codes = np.ascontiguousarray(codes, np.int16)
    n, d = X.shape
    m = codes.shape[1]
    C = np.full((m, h, d), 7, np.float32)
    _lib.check(_lib.lib().rq_update_codebooks_chain_wide(C.ctypes.data, X.ctypes.data, codes.ctypes.data, n, d, m, h, rho, base))
    return C


def _check_against_numpy(X, codes, h, C, tol_rec=1e-5, tol_q=1e-6, tol_cw=1e-4):
    """The measures and tolerances of tests/test_gpu_chainq.py::_check_against_numpy, against the helper's f64 block solve."""
    Cn, _ = cw.chain_update(X, codes, h)
    scale = float(np.abs(Cn).max())
    rec = np.abs(lo.reconstruct(C, codes) - lo.reconstruct(Cn, codes)).max()
    q, qn = lo.qerror(X, C, codes), lo.qerror(X, Cn, codes)
    cwd = np.abs(C.astype(np.float64) - Cn).max()
    print("worst: reconstruction %.3e, qerror rel %.3e, codeword %.3e (x max|C| = %.3e)"
          % (rec / scale, abs(q - qn) / qn, cwd / scale, scale))
    assert rec <= tol_rec * scale
    assert abs(q - qn) <= tol_q * qn
    assert cwd <= tol_cw * scale


def _zero_outside(C):
    m, _, d = C.shape
    for i, dims in enumerate(co.cbdims(d, m)):
        out = np.ones(d, dtype=bool)
        out[dims[0]:dims[-1] + 1] = False
        if C[i][:, out].view(np.uint32).any():       # exact +0, not -0 and not tiny
            return False
    return True


@pytest.mark.parametrize("m,h,d,n,used", [(2, 257, 7, 5000, 257), (3, 300, 24, 3000, 300), (4, 513, 9, 4000, 400)])
def test_chain_update_against_numpy_solve(rq, m, h, d, n, used):
    """used < h: the codes above it never occur, and get exact zero codewords."""
    rng = np.random.default_rng(n + m)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, used, size=(n, m)).astype(np.int16)
    codes[0], codes[1] = 0, used - 1                   # both ends are used (h = 257: code 256 beside code 0)
    C = _update(X, codes, h)
    assert np.isfinite(C).all() and _zero_outside(C)
    for i in range(m):
        unused = np.setdiff1d(np.arange(h), codes[:, i])
        assert unused.size >= h - used and (C[i, unused] == 0).all()
    _check_against_numpy(X, codes, h, C)
    assert _same_bits(_update(X, codes + 1, h, base=1), C)
    assert _same_bits(rq.update_codebooks_chain_bin_u16(X, codes, h), C)
    Cl, elapsed = rq.update_codebooks_chain_bin(X, codes + 1, h, wide=True)
    assert len(Cl) == m and _same_bits(np.stack(Cl), C) and elapsed > 0


def test_chain_update_hostile_codes_and_reproducible(rq):
    """Only the codes {0, 255, 256, 257, 299} occur: a code and its low byte's twin (0 / 256, 1 / 257 would alias in a byte) share
    no count, every other codeword is an exact zero, and two runs agree bit for bit."""
    rng = np.random.default_rng(3)
    n, d, m, h = 3000, 24, 4, 300
    X = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    codes = np.array([0, 255, 256, 257, 299], np.int16)[rng.integers(0, 5, size=(n, m))]
    C = _update(X, codes, h)
    assert np.isfinite(C).all() and _zero_outside(C)
    unused = np.setdiff1d(np.arange(h), [0, 255, 256, 257, 299])
    assert (C[:, unused] == 0).all() and all(np.abs(C[:, k]).max() > 0 for k in (0, 255, 256, 257, 299))
    _check_against_numpy(X, codes, h, C)
    assert _same_bits(_update(X, codes, h), C)


@pytest.mark.parametrize("m,h,d,n", [(3, 256, 24, 3000), (5, 100, 30, 2000)])
def test_chain_update_equals_the_byte_entry(rq, m, h, d, n):
    from rayuela_jl_amd.codebook_update import update_codebooks_chain_u8
    rng = np.random.default_rng(n + h)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    assert _same_bits(_update(X, codes.astype(np.int16), h), update_codebooks_chain_u8(X, codes, h))


# ---- train_chainq -------------------------------------------------------------------------------------------------------------------
def _train_case(h, n=2000, d=24, m=3, seed=21):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)).astype(np.float32), rng.integers(0, h, size=(n, m)).astype(np.int16),
            np.eye(d, dtype=np.float32))


def test_train_equals_the_byte_loop(rq):
    from rayuela_jl_amd.ChainQ import train_chainq_u8, train_chainq_u16
    X, B0, R0 = _train_case(256)
    Cw, Bw, Rw, ow = train_chainq_u16(X, B0, 3, 256, R0, 2)
    Cb, Bb, Rb, ob = train_chainq_u8(X, B0.astype(np.uint8), 3, 256, R0, 2)
    assert Bw.dtype == np.uint16 and np.array_equal(Bw, Bb)
    assert _same_bits(Cw, Cb) and _same_bits(Rw, Rb) and _same_bits(ow, ob)


def test_train_with_no_round_equals_its_public_steps(rq):
    """niter = 0: C0 = update(R0'X, B0); B1 = viterbi(R0'X, C0); one round { R = polar; C = update(R'X, B1); B = viterbi(R'X, C) }.
    Given the returned R, the returned C and codes are those steps through the wide host entries, bit for bit."""
    from rayuela_jl_amd import _lib
    X, B0, R0 = _train_case(300)
    n, d = X.shape
    m, h = 3, 300
    C = np.empty((m, h, d), np.float32)
    codes = B0 + 1
    R = R0.copy()
    obj = np.zeros(1)
    _lib.check(_lib.lib().rq_train_chainq_wide(C.ctypes.data, codes.ctypes.data, R.ctypes.data, obj.ctypes.data, X.ctypes.data, n, d,
                                               m, h, 0, 1))
    assert codes.min() >= 1 and codes.max() <= h and np.isfinite(obj).all() and obj[0] > 0
    RX0 = rq.rotate(R0, X)
    B1 = _wide(RX0, _update(RX0, B0, h))
    RX = rq.rotate(R, X)
    assert _same_bits(C, _update(RX, B1, h))
    assert np.array_equal(codes - 1, _wide(RX, C))
    R64 = R.astype(np.float64)
    assert np.abs(R64 @ R64.T - np.eye(d)).max() < 1e-5


def test_train_objective_falls_as_the_restatement_does(rq, oracle):
    """The bound of the byte tests (tests/test_chain_oracle.py, tests/test_gpu_chainq.py): the restated sequence of this input falls
    by more than 1 % per round, so rounding, rho and polar-vs-SVD cannot turn a step around and the device's must fall strictly."""
    from rayuela_jl_amd.ChainQ import last_chainq_timing
    X, B0, R0 = _train_case(300)
    m, h, niter = 3, 300, 3
    _, _, Rn, want = cw.train(oracle, X, B0, R0, h, niter)
    print("restated obj", want)
    assert want.shape == (niter + 1,) and (want[1:] < 0.99 * want[:-1]).all()
    B1 = B0 + 1
    C, B, R, obj = rq.train_chainq(X, m, h, R0, B1, None, niter)
    print("device obj  ", obj)
    assert obj.shape == (niter + 1,) and obj.dtype == np.float32 and (obj[1:] < obj[:-1]).all()
    assert B.dtype == np.int16 and B.shape == B1.shape and B.min() >= 1 and B.max() <= h
    assert np.array_equal(B1, B0 + 1)                            # the start codes are left alone
    R64 = R.astype(np.float64)
    assert np.abs(R64 @ R64.T - np.eye(R.shape[0])).max() < 1e-5
    assert len(C) == m and all(c.shape == (h, X.shape[1]) for c in C) and _zero_outside(np.stack(C))
    t = last_chainq_timing()
    assert t["unary_ms"] > 0 and t["viterbi_ms"] > 0 and t["update_ms"] > 0 and t["rotation_ms"] > 0 and t["tables_ms"] > 0
    assert np.array_equal(rq.quantize_chainq(rq.rotate(R, X), C, wide=True)[0], B)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_lsq_driver_runs_its_own_initialisation_past_256_codewords(rq):
    """train_opq -> train_chainq -> train_lsq_cuda -> linscan_lsq_u16 at h = 260: the reference's initialisation of LSQ, which
    stopped at train_chainq before the chain entries over 16-bit codes."""
    from rayuela_jl_amd.experiments import experiment_lsq_cuda_query_base
    rng = np.random.default_rng(8)
    Xt = rng.standard_normal((800, 16)).astype(np.float32)
    Xq = rng.standard_normal((20, 16)).astype(np.float32)
    (C, B, R, train_error, recall), opq_error = experiment_lsq_cuda_query_base(
        Xt, Xq, None, 3, 260, niter=1, ilsiter=2, icmiter=2, randord=True, npert=1, init="natural", niter_opq=2, niter_chainq=1,
        knn=10)
    assert B.dtype == np.int16 and B.shape == (800, 3) and B.min() >= 1 and B.max() <= 260
    assert np.stack(C).shape == (3, 260, 16) and np.isfinite(np.stack(C)).all()
    assert np.isfinite(np.asarray(train_error, dtype=np.float64)).all()
    recall = np.asarray(recall)
    assert recall.shape[0] == 10 and np.isfinite(recall).all() and (np.diff(recall) >= 0).all() and recall[-1] > 0
