"""GPU: the LSQ codebook update (rq_dev_lsq_normal_eq / rq_update_codebooks_lsq) and training loop (rq_train_lsq):
A and b bit for bit against tests/lsq_update_oracle.py, the solve against numpy's f64 solve within the derived bounds
of DESIGN.md section 2, reproducibility, and train_lsq against its public steps composed in Python."""
import numpy as np
import pytest

import lsq_update_oracle as lo

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _normal_eq(X, codes, h):
    import torch
    from rayuela_jl_amd import device
    A, b = device.lsq_normal_eq(torch.from_numpy(X).to(_dev()), torch.from_numpy(codes).to(_dev()), h)
    torch.cuda.synchronize()
    return A.cpu().numpy(), b.cpu().numpy()


def _update_host(X, codes, h):
    from rayuela_jl_amd.codebook_update import update_codebooks_u8
    return update_codebooks_u8(X, codes, h)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("m,h,d,n", [(1, 256, 128, 0), (1, 256, 128, 60000), (2, 2, 7, 1), (2, 2, 7, 5000),
                                     (4, 100, 33, 20000), (8, 256, 128, 200000), (16, 256, 96, 100000),
                                     (3, 256, 960, 20000)])
def test_normal_equations_bit_exact(rq, m, h, d, n):
    rng = np.random.default_rng(m * 1000 + h + d + n)
    X = _wide(rng, n, d)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    A, b = _normal_eq(X, codes, h)
    A0, b0 = lo.normal_eq(X, codes, h)
    assert _same_bits(A, A0), "A differs in %d entries" % int((A != A0).sum())
    assert _same_bits(b, b0), "b differs in %d entries" % int((b != b0).sum())


def _wide(rng, n, d):
    """Gaussian values scaled by 2^-30 .. 2^30: f64 sums of f32 values of one scale are nearly always exact (and so the
    same in every order); over this range they round, and the summation order shows in the bits."""
    return (rng.standard_normal((n, d)) * np.exp2(rng.integers(-30, 31, size=(n, d)))).astype(np.float32)


def _hostile(kind, n=50000, d=24, m=4, h=256, seed=3):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    if kind == "one_code":
        codes[:, 0] = 7
    elif kind == "copied":
        codes[:, 1] = codes[:, 0]
    elif kind == "sparse":
        codes = rng.integers(0, 5, size=(n, m)).astype(np.uint8)
    return X, codes, h


def _check_against_numpy(X, codes, h, C, tol_rec=1e-5, tol_q=1e-6, tol_cw=1e-4):
    Cn, _ = lo.update(X, codes, h)
    scale = float(np.abs(Cn).max())
    rec = np.abs(lo.reconstruct(C, codes) - lo.reconstruct(Cn, codes)).max()
    q, qn = lo.qerror(X, C, codes), lo.qerror(X, Cn, codes)
    cw = np.abs(C.astype(np.float64) - Cn).max()
    print("worst: reconstruction %.3e, qerror rel %.3e, codeword %.3e (x max|C| = %.3e)"
          % (rec / scale, abs(q - qn) / qn, cw / scale, scale))
    assert rec <= tol_rec * scale
    assert abs(q - qn) <= tol_q * qn
    assert cw <= tol_cw * scale


@pytest.mark.parametrize("kind", ["one_code", "copied", "sparse"])
def test_hostile_codes(rq, kind):
    X, codes, h = _hostile(kind)
    Xw = _wide(np.random.default_rng(4), *X.shape)
    A, b = _normal_eq(Xw, codes, h)
    A0, b0 = lo.normal_eq(Xw, codes, h)
    assert _same_bits(A, A0) and _same_bits(b, b0)
    C = _update_host(X, codes, h)
    assert np.isfinite(C).all()
    m = codes.shape[1]
    for i in range(m):
        unused = np.setdiff1d(np.arange(h), codes[:, i])
        assert (C[i, unused] == 0).all()
    _check_against_numpy(X, codes, h, C)


@pytest.mark.parametrize("m,h,d,n", [(8, 256, 128, 100000), (16, 256, 96, 50000), (4, 100, 33, 20000)])
def test_codebooks_against_numpy_solve(rq, m, h, d, n):
    rng = np.random.default_rng(n + m)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    _check_against_numpy(X, codes, h, _update_host(X, codes, h))


def test_reproducible_host_equals_device_and_odd_offsets(rq):
    import torch
    from rayuela_jl_amd import device
    rng = np.random.default_rng(11)
    n, d, m, h = 30000, 40, 6, 200
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    C1, C2 = _update_host(X, codes, h), _update_host(X, codes, h)
    assert _same_bits(C1, C2)
    tX, tc = torch.from_numpy(X).to(_dev()), torch.from_numpy(codes).to(_dev())
    Cd = device.update_codebooks_lsq(tX, tc, h)
    torch.cuda.synchronize()
    assert _same_bits(Cd.cpu().numpy(), C1)
    # every device operand at an odd element offset
    bX = torch.empty(n * d + 1, dtype=torch.float32, device=_dev())
    bX[1:] = tX.reshape(-1)
    bc = torch.empty(n * m + 1, dtype=torch.uint8, device=_dev())
    bc[1:] = tc.reshape(-1)
    bC = torch.zeros(m * h * d + 1, dtype=torch.float32, device=_dev())
    device.update_codebooks_lsq(bX[1:].view(n, d), bc[1:].view(n, m), h, out=bC[1:].view(m, h, d))
    bA = torch.empty(m * h * m * h + 1, dtype=torch.float64, device=_dev())
    A, b = device.lsq_normal_eq(tX, tc, h)
    torch.cuda.synchronize()
    assert _same_bits(bC[1:].view(m, h, d).cpu().numpy(), C1)
    from rayuela_jl_amd import _lib
    bb = torch.empty(m * h * d + 1, dtype=torch.float64, device=_dev())
    _lib.check(_lib.lib().rq_dev_lsq_normal_eq(bA[1:].data_ptr(), bb[1:].data_ptr(), bX[1:].data_ptr(),
                                               bc[1:].data_ptr(), n, d, m, h, 1e-4,
                                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(bA[1:].view(m * h, m * h), A) and torch.equal(bb[1:].view(m * h, d), b)
    # a code >= h is refused by the device entry
    tc[5, 2] = h
    with pytest.raises(rq.RayuelaHipError):
        device.update_codebooks_lsq(tX, tc, h)


def _rotation(d, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return q.astype(np.float32)


def _composed(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, randord, seed):
    """train_lsq's steps through the public entries (src/LSQ.jl:345-371)."""
    from rayuela_jl_amd.LSQ import encode_icm_u8
    from rayuela_jl_amd.OPQ import rotate
    n, d = X.shape
    C = _update_host(rotate(R, X), codes0, h)
    C = rotate(np.ascontiguousarray(R.T), C.reshape(m * h, d)).reshape(m, h, d)     # C_i <- R C_i
    codes, cost = encode_icm_u8(X, codes0, C, ilsiter, icmiter, npert, randord, seed=seed, t0=0, with_cost=True)
    obj = []
    for it in range(1, niter + 1):
        obj.append(np.mean(cost, dtype=np.float64))
        C = _update_host(X, codes, h)
        codes, cost = encode_icm_u8(X, codes, C, ilsiter, icmiter, npert, randord, seed=seed, t0=it * ilsiter,
                                    with_cost=True)
    return C, codes, np.array(obj)


@pytest.mark.parametrize("rot", ["identity", "seeded"])
def test_train_lsq_equals_composed_steps(rq, rot):
    from rayuela_jl_amd.LSQ import train_lsq_u8
    rng = np.random.default_rng(12)
    n, d, m, h = 4000, 32, 4, 64
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes0 = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    R = np.eye(d, dtype=np.float32) if rot == "identity" else _rotation(d, 5)
    args = (3, 2, 2, 2, True, 9)          # niter, ilsiter, icmiter, npert, randord, seed
    C, codes, obj = train_lsq_u8(X, codes0, m, h, R, args[0], args[1], args[2], args[4], args[3], seed=args[5])
    C0, codes_0, obj0 = _composed(X, codes0, m, h, R, *args)
    assert np.array_equal(codes, codes_0)
    assert _same_bits(C, C0)
    assert np.allclose(obj, obj0, rtol=1e-12, atol=0)
    if rot == "identity":      # R = None skips the rotations; R = I rotates exactly
        Cn, codes_n, _ = train_lsq_u8(X, codes0, m, h, None, args[0], args[1], args[2], args[4], args[3], seed=args[5])
        assert np.array_equal(codes_n, codes) and _same_bits(Cn, C)


def test_train_lsq_cuda_nsplits_and_in_place_rules(rq):
    rng = np.random.default_rng(13)
    n, d, m, h = 3000, 24, 4, 256
    X = rng.standard_normal((n, d)).astype(np.float32)
    B0 = rng.integers(1, h + 1, size=(n, m)).astype(np.int16)
    R = _rotation(d, 6)
    B = B0.copy()
    C, Bt, obj = rq.train_lsq(X, m, h, R, B, None, 2, 2, 2, True, 2, V=False, seed=4)
    assert np.array_equal(B, Bt) and obj.dtype == np.float32 and obj.shape == (2,)
    for ns in (1, 3):
        Bin = B0.copy()
        Cc, Bc, objc = rq.train_lsq_cuda(X, m, h, R, Bin, None, 2, 2, 2, True, 2, nsplits=ns, seed=4)
        assert np.array_equal(Bin, B0)
        assert np.array_equal(Bc, Bt) and all(_same_bits(a, b) for a, b in zip(Cc, C))
        assert _same_bits(objc, obj)


def test_sift1m_shape_from_rvq_codes(rq):
    """1e6 x 128, m = 8: RVQ start codes, niter = 2, ilsiter = 2; obj does not increase beyond rounding, the final qerror is
    below the start's, and linscan_lsq runs on the result."""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.LSQ import train_lsq_u8
    n, d, m, h = 1_000_000, 128, 8, 256
    X = synth.sift_like(n, d, seed=31)
    Crvq, _, _ = rq.train_rvq(X[:20000], m, h, niter=4)
    Brvq, _ = rq.quantize_rvq(X, Crvq)
    q0 = rq.qerror(X, Brvq, Crvq)
    C, codes, obj = train_lsq_u8(X, (Brvq - 1).astype(np.uint8), m, h, None, 2, 2, 4, True, 4, seed=3)
    q_end = rq.qerror(X, codes.astype(np.int16) + 1, list(C))
    print("SIFT1M shape: RVQ qerror %.6e, obj %s, final %.6e" % (q0, obj, q_end))
    assert obj[1] <= obj[0] * (1 + 1e-6)
    assert q_end < q0
    nrm = np.sum(C[np.arange(m)[None, :], codes.astype(np.int64)].sum(axis=1) ** 2, axis=1).astype(np.float32)
    Q = synth.sift_like(8, d, seed=32)
    dist, idx = rq.linscan_lsq(codes, Q, list(C), nrm, np.eye(d, dtype=np.float32), 100)
    assert idx.size == 800 and np.isfinite(dist).all()


def test_train_lsq_without_rows_and_phase_clock(rq):
    """n = 0: zero codewords, obj NaN (the mean of no rows, as the reference's qerror).  The host entry's phase clock puts
    R'X, the rotation back and the obj means in their own slot, not in the update's."""
    from rayuela_jl_amd.LSQ import train_lsq_u8, last_lsq_timing
    C, codes, obj = train_lsq_u8(np.zeros((0, 16), np.float32), np.zeros((0, 2), np.uint8), 2, 8, None, 2, 1, 1, True, 1)
    assert (C == 0).all() and codes.shape == (0, 2) and obj.shape == (2,) and np.isnan(obj).all()
    rng = np.random.default_rng(14)
    X = rng.standard_normal((20000, 64)).astype(np.float32)
    train_lsq_u8(X, rng.integers(0, 64, size=(20000, 4)).astype(np.uint8), 4, 64, _rotation(64, 7), 2, 1, 1, True, 1)
    t = last_lsq_timing()
    assert all(v >= 0 for v in t.values())
    assert t["other_ms"] > 0 and t["encode_ms"] > 0 and t["solve_ms"] > 0 and t["b_ms"] > 0
