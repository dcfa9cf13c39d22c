"""GPU: the LSQ codebook update and training past 256 codewords (rq_lsq_normal_eq_wide / rq_update_codebooks_lsq_wide /
rq_train_lsq_wide): A, b and the counts bit for bit against tests/lsq_wide_oracle.py, the solve against
numpy's f64 solve within the bounds of DESIGN.md section 2 item 4, the byte path's bits at h <= 256, stale scratch, and the
training loop against its public steps composed in Python."""
import ctypes

import numpy as np
import pytest

import lsq_wide_oracle as wo

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x7F, 0x80)


def _L():
    from rayuela_jl_amd import _lib
    return _lib


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _wide(rng, n, d):
    """Gaussian values scaled by 2^-30 .. 2^30: f64 sums of f32 values of one scale are nearly always exact (and so the
    same in every order); over this range they round, and the summation order shows in the bits."""
    return (rng.standard_normal((n, d)) * np.exp2(rng.integers(-30, 31, size=(n, d)))).astype(np.float32)


def _normal_eq(X, codes, h, base=0, with_A=True, rho=1e-4):
    """rq_lsq_normal_eq_wide -> (A or None, b, counts)"""
    L = _L()
    n, d = X.shape
    m = codes.shape[1]
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    A = np.full((m * h, m * h), np.nan) if with_A else None
    b = np.full((m * h, d), np.nan)
    cnt = np.full((m, h), 0xFFFFFFFF, np.uint32)
    L.check(L.lib().rq_lsq_normal_eq_wide(None if A is None else A.ctypes.data, b.ctypes.data, cnt.ctypes.data, X.ctypes.data,
                                          codes.ctypes.data, n, d, m, h, rho, base))
    return A, b, cnt


def _update(X, codes, h, base=0, rho=1e-4):
    L = _L()
    n, d = X.shape
    m = codes.shape[1]
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    C = np.full((m, h, d), np.nan, np.float32)
    L.check(L.lib().rq_update_codebooks_lsq_wide(C.ctypes.data, X.ctypes.data, codes.ctypes.data, n, d, m, h, rho, base))
    return C


def _train(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, randord, seed, nsplits=1, base=0):
    L = _L()
    n, d = X.shape
    codes = np.array(codes0, dtype=np.int16, order="C")
    C = np.full((m, h, d), np.nan, np.float32)
    obj = np.full(niter, -1.0)
    L.check(L.lib().rq_train_lsq_wide(C.ctypes.data, codes.ctypes.data, obj.ctypes.data, X.ctypes.data,
                                      None if R is None else R.ctypes.data, n, d, m, h, niter, ilsiter, icmiter, npert,
                                      1 if randord else 0, seed, nsplits, base))
    return C, codes, obj


def _codes(rng, n, m, h, present=()):
    """uniform codes with `present` forced into the first rows of every codebook (in a different row order per codebook)"""
    codes = rng.integers(0, h, size=(n, m)).astype(np.int16)
    for i in range(m):
        for k, a in enumerate(present):
            codes[k * (i + 1) + i, i] = a
        assert set(present) <= set(codes[:, i].tolist())
    return codes


def _check_normal_eq(X, codes, h, with_A=True):
    A, b, cnt = _normal_eq(X, codes, h, with_A=with_A)
    A0, b0, cnt0 = wo.normal_eq(X, codes, h, with_A=with_A)
    assert np.array_equal(cnt, cnt0), "counts differ in %d entries" % int((cnt != cnt0).sum())
    assert _same_bits(b, b0), "b differs in %d entries" % int((b != b0).sum())
    if with_A:
        assert _same_bits(A, A0), "A differs in %d entries" % int((A != A0).sum())
    else:
        assert A is None
    return A, b, cnt


# ---- the normal equations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,h,d,n,present", [
    (2, 257, 7, 5000, (0, 256)),          # a sort that keeps 8 bits merges codes 0 and 256
    (3, 300, 33, 8200, ()),               # three tiles, the last one partial; h a multiple of neither 64 nor 256
    (2, 1024, 16, 4097, ()),
    (4, 513, 5, 100, (0, 256, 512)),      # n < 256: most codes unused
    (2, 2048, 4, 20000, ()),              # mh = 4096
    (2, 300, 5, 0, ()),                   # no rows
])
def test_normal_equations_bit_exact(rq, m, h, d, n, present):
    rng = np.random.default_rng(m * 1000 + h + d + n)
    X = _wide(rng, n, d)
    codes = _codes(rng, n, m, h, present)
    A, b, cnt = _check_normal_eq(X, codes, h)
    for a in present:
        assert (cnt[:, a] >= 1).all()
    if n == 0:
        assert not b.any() and not cnt.any() and np.array_equal(A, 1e-4 * np.eye(m * h))


def test_all_fifteen_bits_without_A(rq):
    """h = 32767, A = NULL: no mh x mh buffer, so the sort is checked over the whole code range with kilobytes of memory."""
    rng = np.random.default_rng(15)
    m, h, d, n = 1, 32767, 3, 40000
    present = (255, 256, 511, 512, 0x7F00, 32766)
    X = _wide(rng, n, d)
    codes = _codes(rng, n, m, h, present)
    _, b, cnt = _check_normal_eq(X, codes, h, with_A=False)
    assert all(cnt[0, a] >= 1 and b[a].any() for a in present)
    # and with 16 codebooks of 2048 codewords, past m * h = 16384
    codes = _codes(rng, 6000, 16, 2048, (0, 255, 256, 2047))
    _check_normal_eq(_wide(rng, 6000, 2), codes, 2048, with_A=False)


def test_code_base_one_equals_code_base_zero(rq):
    rng = np.random.default_rng(16)
    m, h, d, n = 3, 300, 33, 8200
    X = _wide(rng, n, d)
    codes = _codes(rng, n, m, h, (0, 299))
    A0, b0, c0 = _normal_eq(X, codes, h)
    A1, b1, c1 = _normal_eq(X, codes + 1, h, base=1)
    assert _same_bits(A0, A1) and _same_bits(b0, b1) and np.array_equal(c0, c1)
    Xg = rng.standard_normal((n, d)).astype(np.float32)
    assert _same_bits(_update(Xg, codes, h), _update(Xg, codes + 1, h, base=1))
    with pytest.raises(rq.RayuelaHipError, match="outside 1..300"):
        _update(Xg, codes, h, base=1)                    # a zero among one-based codes


def _hostile(kind, n=20000, d=24, m=4, h=300, seed=3):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, h, size=(n, m)).astype(np.int16)
    if kind == "one_code":
        codes[:, 0] = 299
    elif kind == "copied":
        codes[:, 1] = codes[:, 0]
    elif kind == "sparse":
        codes = rng.choice(np.array([0, 255, 256, 257, 299], np.int16), size=(n, m))
    return (rng.standard_normal((n, d)) * 3).astype(np.float32), codes, h


def _check_against(Cn, X, codes, C, tol_rec=1e-5, tol_q=1e-6, tol_cw=1e-4):
    """reconstructions of every row, qerror, codewords -- against the f64 yardstick Cn"""
    scale = float(np.abs(Cn).max())
    rec = np.abs(wo.reconstruct(C, codes) - wo.reconstruct(Cn, codes)).max()
    q, qn = wo.qerror(X, C, codes), wo.qerror(X, Cn, codes)
    cw = np.abs(C.astype(np.float64) - Cn).max()
    print("worst: reconstruction %.3e, qerror rel %.3e, codeword %.3e (x max|C| = %.3e)"
          % (rec / scale, abs(q - qn) / qn, cw / scale, scale))
    assert np.isfinite(C).all()
    assert rec <= tol_rec * scale
    assert abs(q - qn) <= tol_q * qn
    assert cw <= tol_cw * scale


@pytest.mark.parametrize("kind", ["one_code", "copied", "sparse"])
def test_hostile_codes(rq, kind):
    X, codes, h = _hostile(kind)
    _check_normal_eq(_wide(np.random.default_rng(4), *X.shape), codes, h)
    C = _update(X, codes, h)
    for i in range(codes.shape[1]):
        unused = np.setdiff1d(np.arange(h), codes[:, i])
        assert (C[i, unused] == 0).all()
    _check_against(wo.update(X, codes, h)[0], X, codes, C)


# ---- the update -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,h,d,n", [(3, 300, 33, 20000), (2, 1024, 16, 30000), (8, 512, 32, 60000)])
def test_codebooks_against_numpy_solve(rq, m, h, d, n):
    rng = np.random.default_rng(n + m)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.int16)
    _check_against(wo.update(X, codes, h)[0], X, codes, _update(X, codes, h))


def test_one_codebook_past_the_byte_paths_size(rq):
    """mh = 4097: one more than the byte path ever solved, with a last Cholesky block of one row.  A is diagonal, so the
    yardstick is b / (count + rho) in f64."""
    rng = np.random.default_rng(17)
    m, h, d, n = 1, 4097, 8, 30000
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = _codes(rng, n, m, h, (0, 4095, 4096))
    C = _update(X, codes, h)
    unused = np.setdiff1d(np.arange(h), codes[:, 0])
    assert len(unused) and (C[0, unused] == 0).all() and C[0, 4096].any()
    _check_against(wo.update_one_codebook(X, codes, h)[0], X, codes, C)


@pytest.mark.parametrize("m,h,d,n", [(4, 100, 33, 20000), (2, 256, 16, 5000)])
def test_wide_entries_give_the_byte_paths_bits(rq, m, h, d, n):
    import torch
    from rayuela_jl_amd import device
    from rayuela_jl_amd.codebook_update import update_codebooks_u8, update_codebooks_u16
    rng = np.random.default_rng(m + h)
    X = _wide(rng, n, d)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    dev = torch.device("cuda:0")
    A8, b8 = device.lsq_normal_eq(torch.from_numpy(X).to(dev), torch.from_numpy(codes).to(dev), h)
    torch.cuda.synchronize()
    A, b, cnt = _normal_eq(X, codes.astype(np.int16), h)
    assert _same_bits(A, A8.cpu().numpy()) and _same_bits(b, b8.cpu().numpy())
    assert np.array_equal(cnt, wo.counts(codes.astype(np.int16), h))
    Xg = rng.standard_normal((n, d)).astype(np.float32)
    C8 = update_codebooks_u8(Xg, codes, h)
    C16 = update_codebooks_u16(Xg, codes.astype(np.int16), h)
    assert _same_bits(C16, C8)
    assert _same_bits(update_codebooks_u16(Xg, codes.astype(np.int16), h), C16)          # two calls, the same bits


def test_stale_scratch_changes_no_bit(rq):
    """Library scratch filled with 0x00 / 0xFF / 0x7F / 0x80 before the call, and a byte-path LSQ call's pair counts left in the
    slot the wide call builds its own in: the same bits every time."""
    from rayuela_jl_amd.codebook_update import update_codebooks_u8
    L = _L()
    rng = np.random.default_rng(18)
    m, h, d, n = 3, 300, 33, 8200
    X = _wide(rng, n, d)
    Xg = rng.standard_normal((n, d)).astype(np.float32)
    codes = _codes(rng, n, m, h, (0, 255, 256, 299))
    A0, b0, c0 = _check_normal_eq(X, codes, h)
    C0 = _update(Xg, codes, h)
    # the byte path's leftovers: 4 x 256 codes used densely, so its 1024 x 1024 pair counts cover the wide call's 900 x 900
    X8 = rng.standard_normal((20000, d)).astype(np.float32)
    codes8 = rng.integers(0, 256, size=(20000, 4)).astype(np.uint8)
    C8 = update_codebooks_u8(X8, codes8, 256)

    def normal_eq_again(what):
        A, b, c = _normal_eq(X, codes, h)
        assert _same_bits(A, A0) and _same_bits(b, b0) and np.array_equal(c, c0), what

    for value in FILLS:
        rep = L.fill_scratch(value)
        assert rep["slot_bytes"] >= 900 * 900 * 12, rep            # A and the pair counts are in what was filled
        normal_eq_again(value)
        L.fill_scratch(value)
        assert _same_bits(_update(Xg, codes, h), C0), value
    assert _same_bits(update_codebooks_u8(X8, codes8, 256), C8)
    normal_eq_again("after the byte path")
    update_codebooks_u8(X8, codes8, 256)
    assert _same_bits(_update(Xg, codes, h), C0), "after the byte path"
    for value in FILLS:                                           # and the byte path after the wide one
        L.fill_scratch(value)
        _update(Xg, codes, h)
        assert _same_bits(update_codebooks_u8(X8, codes8, 256), C8)


# ---- training -------------------------------------------------------------------------------------------------------------------
def _rotation(d, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return q.astype(np.float32)


def _device_mean(cost):
    """lsq_mean_kernel's order: thread t sums rows t, t + 1024, ... in f64 from +0, then the halving tree, then / n"""
    n = len(cost)
    pad = np.zeros(-(-max(n, 1) // 1024) * 1024)
    pad[:n] = cost.astype(np.float64)
    part = np.zeros(1024)
    for row in pad.reshape(-1, 1024):
        part = part + row
    off = 512
    while off >= 1:
        part[:off] = part[:off] + part[off:2 * off]
        off //= 2
    return part[0] / np.float64(n)


def _composed(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, randord, seed):
    """train_lsq's steps through the public entries (src/LSQ.jl:345-371)."""
    from rayuela_jl_amd.LSQ import encode_icm_u16
    from rayuela_jl_amd.OPQ import rotate
    n, d = X.shape
    if R is None:
        C = _update(X, codes0, h)
    else:
        C = _update(rotate(R, X), codes0, h)
        C = rotate(np.ascontiguousarray(R.T), C.reshape(m * h, d)).reshape(m, h, d)     # C_i <- R C_i
    codes, cost = encode_icm_u16(X, codes0, C, ilsiter, icmiter, npert, randord, seed=seed, t0=0, with_cost=True)
    obj = []
    for it in range(1, niter + 1):
        obj.append(_device_mean(cost))
        C = _update(X, codes, h)
        codes, cost = encode_icm_u16(X, codes, C, ilsiter, icmiter, npert, randord, seed=seed, t0=it * ilsiter, with_cost=True)
    return C, codes, np.array(obj)


TRAIN = (2, 2, 2, 2, True, 9)          # niter, ilsiter, icmiter, npert, randord, seed


@pytest.fixture(scope="module")
def train_case():
    rng = np.random.default_rng(19)
    n, d, m, h = 3000, 24, 3, 300
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes0 = _codes(rng, n, m, h, (0, 255, 256, 299))
    return X, codes0, m, h


@pytest.mark.parametrize("rot", ["identity", "seeded"])
def test_train_lsq_wide_equals_composed_steps(rq, train_case, rot):
    X, codes0, m, h = train_case
    R = np.eye(X.shape[1], dtype=np.float32) if rot == "identity" else _rotation(X.shape[1], 5)
    C, codes, obj = _train(X, codes0, m, h, R, *TRAIN)
    C0, codes_0, obj0 = _composed(X, codes0, m, h, R, *TRAIN)
    assert codes.dtype == np.int16 and np.array_equal(codes, codes_0) and codes.max() > 255
    assert _same_bits(C, C0)
    assert _same_bits(obj, obj0), (obj, obj0)
    assert not np.array_equal(codes, codes0)
    if rot == "identity":      # R = None skips the rotations; R = I rotates exactly
        Cn, codes_n, obj_n = _train(X, codes0, m, h, None, *TRAIN)
        assert np.array_equal(codes_n, codes) and _same_bits(Cn, C) and _same_bits(obj_n, obj)


def test_train_lsq_wide_nsplits_code_base_and_clock(rq, train_case):
    from rayuela_jl_amd.LSQ import last_lsq_timing
    X, codes0, m, h = train_case
    R = _rotation(X.shape[1], 6)
    C1, B1, o1 = _train(X, codes0, m, h, R, *TRAIN, nsplits=1)
    t = last_lsq_timing()
    assert all(v >= 0 for v in t.values())
    assert t["other_ms"] > 0 and t["encode_ms"] > 0 and t["solve_ms"] > 0 and t["b_ms"] > 0 and t["sort_ms"] > 0
    C3, B3, o3 = _train(X, codes0, m, h, R, *TRAIN, nsplits=3)
    assert np.array_equal(B1, B3) and _same_bits(C1, C3) and _same_bits(o1, o3)
    Cb, Bb, ob = _train(X, codes0 + 1, m, h, R, *TRAIN, base=1)
    assert np.array_equal(Bb, B1 + 1) and _same_bits(Cb, C1) and _same_bits(ob, o1)


def test_train_lsq_wide_without_rows(rq):
    C, codes, obj = _train(np.zeros((0, 16), np.float32), np.zeros((0, 2), np.int16), 2, 300, None, 2, 1, 1, 1, True, 0)
    assert (C == 0).all() and codes.shape == (0, 2) and obj.shape == (2,) and np.isnan(obj).all()


def test_train_lsq_wide_at_256_equals_the_byte_loop(rq):
    from rayuela_jl_amd.LSQ import train_lsq_u8
    rng = np.random.default_rng(20)
    n, d, m, h = 3000, 24, 3, 256
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes0 = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    R = _rotation(d, 7)
    niter, ilsiter, icmiter, npert, randord, seed = TRAIN
    C8, B8, o8 = train_lsq_u8(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, seed=seed)
    C, B, o = _train(X, codes0.astype(np.int16), m, h, R, *TRAIN)
    assert np.array_equal(B, B8.astype(np.int16)) and _same_bits(C, C8) and _same_bits(o, o8)


def test_from_rvq_codes_the_update_and_the_training_do_not_lose(rq):
    """The update minimises qerror + rho |C|^2 / n over C, and C_rvq is a candidate: after one update qerror is at most
    qerror_rvq + rho |C_rvq|_F^2 / n, times 1 + 1e-6 (the project's qerror tolerance) for the f32 rounding of C.  Training on
    from there does not end above that first update's qerror, beyond the same slack."""
    rng = np.random.default_rng(21)
    n, d, m, h, rho = 20000, 32, 4, 320, 1e-4
    centers = rng.standard_normal((64, d)) * 4
    X = (centers[rng.integers(0, 64, n)] + rng.standard_normal((n, d))).astype(np.float32)
    Crvq, Brvq, _ = rq.train_rvq(X, m, h, niter=3, seed=1)
    codes = (Brvq - 1).astype(np.int16)
    assert codes.max() > 255
    Crvq = np.stack(Crvq)
    q_rvq = wo.qerror(X, Crvq, codes)
    bound = (q_rvq + rho * float((Crvq.astype(np.float64) ** 2).sum()) / n) * (1 + 1e-6)
    C1 = _update(X, codes, h, rho=rho)
    q1 = wo.qerror(X, C1, codes)
    C, B, obj = _train(X, codes, m, h, None, 2, 2, 2, 2, True, 3)
    q_end = wo.qerror(X, C, B)
    print("RVQ qerror %.6e, bound %.6e, after one update %.6e, obj %s, after niter = 2 %.6e" % (q_rvq, bound, q1, obj, q_end))
    assert q1 <= bound
    assert q_end <= q1 * (1 + 1e-6)


def test_python_mirrors_reach_the_wide_entries_at_h300(rq, train_case):
    from rayuela_jl_amd.LSQ import train_lsq_u16
    X, codes0, m, h = train_case
    B1 = codes0 + 1
    R = _rotation(X.shape[1], 8)
    niter, ilsiter, icmiter, npert, randord, seed = TRAIN
    C0, codes, obj0 = train_lsq_u16(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, seed=seed)
    Cw, Bw, ow = _train(X, codes0, m, h, R, *TRAIN)
    assert np.array_equal(codes, Bw) and _same_bits(C0, Cw) and _same_bits(obj0, ow)
    B = B1.copy()
    C, Bt, obj = rq.train_lsq(X, m, h, R, B, None, niter, ilsiter, icmiter, randord, npert, cpp=False, V=False, seed=seed)
    assert Bt.dtype == np.int16 and np.array_equal(Bt, codes + 1) and np.array_equal(B, Bt) and Bt.min() >= 1
    assert obj.dtype == np.float32 and _same_bits(obj, obj0.astype(np.float32))
    assert len(C) == m and all(_same_bits(np.ascontiguousarray(c), C0[i]) for i, c in enumerate(C))
    for ns in (1, 3):
        Bin = B1.copy()
        Cc, Bc, objc = rq.train_lsq_cuda(X, m, h, R, Bin, None, niter, ilsiter, icmiter, randord, npert, nsplits=ns, seed=seed)
        assert np.array_equal(Bin, B1)                                   # train_lsq_cuda leaves B alone
        assert np.array_equal(Bc, Bt) and all(_same_bits(np.ascontiguousarray(a), C0[i]) for i, a in enumerate(Cc))
        assert _same_bits(objc, obj)
    Cu = rq.update_codebooks(X, B1, h)
    assert len(Cu) == m and _same_bits(np.stack(Cu), _update(X, codes0, h))
