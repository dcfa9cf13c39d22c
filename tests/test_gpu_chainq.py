"""GPU: chain quantization (rq_quantize_chainq / rq_update_codebooks_chain / rq_train_chainq).  The Viterbi codes bit for
bit against the reference's fixtures and against tests/chain_oracle.py, the chain codebook update against numpy's f64
solve within the bounds the LSQ update is held to, reproducibility, and train_chainq against its public steps composed in
Python."""
import numpy as np
import pytest

import chain_oracle as co
import lsq_update_oracle as lo
from conftest import golden
from test_chain_oracle import CASES, TRAIN_NITER, train_case

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _host(X, C, nsplits=1):
    from rayuela_jl_amd.ChainQ import quantize_chainq_u8
    return quantize_chainq_u8(X, C, nsplits=nsplits)


def _device(X, C, nsplits=1):
    import torch
    from rayuela_jl_amd import device
    out = device.quantize_chainq(torch.from_numpy(X).to(_dev()), torch.from_numpy(np.ascontiguousarray(C)).to(_dev()),
                                 nsplits=nsplits)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- the encoder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_golden_cases_host_and_device_entry(rq, name):
    g = golden(name)
    for codes in (_host(g["X"], g["C"]), _device(g["X"], g["C"])):
        assert np.array_equal(codes, g["codes"]), "rows differ: %d" % int((codes != g["codes"]).any(axis=1).sum())
    B, elapsed = rq.quantize_chainq(g["X"], list(g["C"]), True, False)
    assert B.dtype == np.int16 and np.array_equal(B, g["codes"].astype(np.int16) + 1) and elapsed > 0


@pytest.mark.parametrize("m,h,d,n", [(1, 256, 128, 300), (1, 2, 7, 1), (2, 2, 7, 500), (2, 100, 96, 300), (8, 100, 96, 300),
                                     (8, 256, 128, 257), (8, 256, 128, 1), (16, 256, 96, 200), (3, 256, 960, 100),
                                     (16, 2, 960, 50), (5, 65, 30, 129), (16, 100, 7, 33)])
def test_codes_equal_the_restatement(rq, oracle, m, h, d, n):
    rng = np.random.default_rng(m * 1000 + h + d + n)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    want = co.viterbi(oracle, X, C)
    for codes in (_host(X, C), _device(X, C)):
        assert np.array_equal(codes, want), "rows differ: %d of %d" % (int((codes != want).any(axis=1).sum()), n)


def _chain_masked(C):
    m, _, d = C.shape
    for i, dims in enumerate(co.cbdims(d, m)):
        out = np.ones(d, dtype=bool)
        out[dims[0]:dims[-1] + 1] = False
        C[i][:, out] = 0
    return C


@pytest.mark.parametrize("m,h,d,n", [(8, 256, 128, 300), (16, 256, 96, 200), (5, 65, 31, 200), (8, 100, 29, 150),
                                     (2, 2, 7, 100), (4, 48, 960, 60), (16, 256, 15, 100)])
def test_chain_structured_codebooks_take_the_range_restricted_unaries(rq, oracle, m, h, d, n):
    """Codebooks that are zero outside a dimension range: the unaries run over that range only (found from C itself) and
    must give the same bits -- odd d, odd range bounds, tiles of 32 codewords that span two codebooks (h = 65, 100, 48, 2)."""
    rng = np.random.default_rng(m + h + d)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = _chain_masked((rng.standard_normal((m, h, d)) * 0.5).astype(np.float32))
    want = co.viterbi(oracle, X, C)
    assert np.array_equal(_device(X, C), want) and np.array_equal(_host(X, C), want)
    # other zero patterns: negative zeros outside the range, one all-zero codebook, one codebook with a single dimension
    C2 = C.copy()
    C2[C2 == 0] = -0.0
    C2[m - 1] = 0
    C2[0] = 0
    C2[0][:, d - 1] = rng.standard_normal(h).astype(np.float32)
    assert np.array_equal(_device(X, C2), co.viterbi(oracle, X, C2))


def test_integer_valued_ties_at_other_shapes(rq, oracle):
    rng = np.random.default_rng(5)
    for m, h, d, n in [(6, 100, 10, 300), (16, 256, 6, 150), (2, 2, 3, 200)]:
        X = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
        C = rng.integers(-1, 2, size=(m, h, d)).astype(np.float32)
        assert np.array_equal(_device(X, C), co.viterbi(oracle, X, C))


def test_no_rows(rq):
    C = np.zeros((4, 16, 8), np.float32)
    assert _host(np.zeros((0, 8), np.float32), C).shape == (0, 4)
    assert _device(np.zeros((0, 8), np.float32), C).shape == (0, 4)


def _max_chunk(m, h):
    """Rows of the largest chunk: what the 2 GiB workspace rule leaves after the pair tables."""
    HS = 64 * ((h + 63) // 64)
    tables = (m - 1) * h * (256 + HS) * 4 + m * h * 4
    return ((2 << 30) - tables) // (m * HS * 4)


def test_one_chunk_plus_one_row_and_forced_chunks(rq, oracle):
    m, h, d = 16, 256, 8
    n = _max_chunk(m, h) + 1
    rng = np.random.default_rng(17)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    one = _device(X, C)                    # one full chunk + a chunk of one row
    assert np.array_equal(one, _device(X, C, nsplits=3))
    assert np.array_equal(one, _host(X, C, nsplits=7))
    rows = np.r_[0:48, n - 40:n, rng.integers(0, n, size=40)]
    assert np.array_equal(one[rows], co.viterbi(oracle, X[rows], C))


def test_chunked_run_equals_one_chunk_and_calls_repeat(rq, oracle):
    rng = np.random.default_rng(18)
    n, d, m, h = 5000, 32, 8, 256
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    one = _device(X, C)
    for ns in (2, 5, 4999, 5000, 9000):
        assert np.array_equal(_device(X, C, nsplits=ns), one), ns
    assert _same_bits(_device(X, C), one) and _same_bits(_host(X, C), one)
    rows = rng.integers(0, n, size=200)
    assert np.array_equal(one[rows], co.viterbi(oracle, X[rows], C))


def test_unaligned_device_pointers(rq):
    """Every device operand at an odd element offset."""
    import torch
    from rayuela_jl_amd import device
    rng = np.random.default_rng(19)
    n, d, m, h = 777, 33, 5, 100
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    want = _device(X, C)
    bX = torch.empty(n * d + 1, dtype=torch.float32, device=_dev())
    bX[1:] = torch.from_numpy(X).reshape(-1).to(_dev())
    bC = torch.empty(m * h * d + 1, dtype=torch.float32, device=_dev())
    bC[1:] = torch.from_numpy(C).reshape(-1).to(_dev())
    bo = torch.zeros(n * m + 1, dtype=torch.uint8, device=_dev())
    device.quantize_chainq(bX[1:].view(n, d), bC[1:].view(m, h, d), out=bo[1:].view(n, m))
    torch.cuda.synchronize()
    assert np.array_equal(bo[1:].view(n, m).cpu().numpy(), want) and int(bo[0]) == 0
    # the update through the same pattern
    codes = torch.from_numpy(want).to(_dev())
    Cu = device.update_codebooks_chain(bX[1:].view(n, d), codes, h)
    bc = torch.empty(n * m + 1, dtype=torch.uint8, device=_dev())
    bc[1:] = codes.reshape(-1)
    bU = torch.zeros(m * h * d + 1, dtype=torch.float32, device=_dev())
    device.update_codebooks_chain(bX[1:].view(n, d), bc[1:].view(n, m), h, out=bU[1:].view(m, h, d))
    torch.cuda.synchronize()
    assert torch.equal(bU[1:].view(m, h, d), Cu)


# ---- the chain codebook update -------------------------------------------------------------------------------------------
def _update_host(X, codes, h):
    from rayuela_jl_amd.codebook_update import update_codebooks_chain_u8
    return update_codebooks_chain_u8(X, codes, h)


def _check_against_numpy(X, codes, h, C, tol_rec=1e-5, tol_q=1e-6, tol_cw=1e-4):
    """The measures and tolerances tests/test_gpu_lsq_train.py::_check_against_numpy holds "fastbin" to."""
    Cn, _ = co.chain_update(X, codes, h)
    scale = float(np.abs(Cn).max())
    rec = np.abs(lo.reconstruct(C, codes) - lo.reconstruct(Cn, codes)).max()
    q, qn = lo.qerror(X, C, codes), lo.qerror(X, Cn, codes)
    cw = np.abs(C.astype(np.float64) - Cn).max()
    print("worst: reconstruction %.3e, qerror rel %.3e, codeword %.3e (x max|C| = %.3e)"
          % (rec / scale, abs(q - qn) / qn, cw / scale, scale))
    assert rec <= tol_rec * scale
    assert abs(q - qn) <= tol_q * qn
    assert cw <= tol_cw * scale


def _zero_outside(C):
    m, _, d = C.shape
    for i, dims in enumerate(co.cbdims(d, m)):
        out = np.ones(d, dtype=bool)
        out[dims[0]:dims[-1] + 1] = False
        if C[i][:, out].view(np.uint32).any():       # exact +0, not -0 and not tiny
            return False
    return True


@pytest.mark.parametrize("m,h,d,n", [(8, 256, 128, 100000), (16, 256, 96, 50000), (5, 100, 30, 20000), (2, 2, 7, 5000),
                                     (16, 16, 15, 3000)])
def test_chain_update_against_numpy_solve(rq, m, h, d, n):
    rng = np.random.default_rng(n + m)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    C = _update_host(X, codes, h)
    assert _zero_outside(C)
    _check_against_numpy(X, codes, h, C)


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


@pytest.mark.parametrize("kind", ["one_code", "copied", "sparse"])
def test_chain_update_hostile_codes(rq, kind):
    X, codes, h = _hostile(kind)
    C = _update_host(X, codes, h)
    assert np.isfinite(C).all() and _zero_outside(C)
    for i in range(codes.shape[1]):
        unused = np.setdiff1d(np.arange(h), codes[:, i])
        assert (C[i, unused] == 0).all()
    _check_against_numpy(X, codes, h, C)


def test_chain_update_reproducible_and_host_equals_device(rq):
    import torch
    from rayuela_jl_amd import device
    rng = np.random.default_rng(11)
    n, d, m, h = 30000, 40, 6, 200
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    C1, C2 = _update_host(X, codes, h), _update_host(X, codes, h)
    assert _same_bits(C1, C2)
    tX, tc = torch.from_numpy(X).to(_dev()), torch.from_numpy(codes).to(_dev())
    Cd = device.update_codebooks_chain(tX, tc, h)
    torch.cuda.synchronize()
    assert _same_bits(Cd.cpu().numpy(), C1)
    Cl, elapsed = rq.update_codebooks_chain_bin(X, codes.astype(np.int16) + 1, h)
    assert len(Cl) == m and _same_bits(np.stack(Cl), C1) and elapsed > 0
    tc[5, 2] = h            # a code >= h is refused by the device entry
    with pytest.raises(rq.RayuelaHipError):
        device.update_codebooks_chain(tX, tc, h)


# ---- train_chainq ----------------------------------------------------------------------------------------------------------
def _composed(X, codes0, Rimg, h, niter):
    """train_chainq's steps through the public device entries (src/ChainQ.jl:393-426)."""
    import torch
    from rayuela_jl_amd import device
    n, d = X.shape
    tX = torch.from_numpy(X).to(_dev())
    B = torch.from_numpy(codes0).to(_dev())
    R = torch.from_numpy(Rimg).to(_dev())
    RX = device.rotate_T(R, tX)
    C = device.update_codebooks_chain(RX, B, h)
    B = device.quantize_chainq(RX, C)
    obj = []
    for _ in range(niter + 1):
        CB = device.reconstruct_aq(B, C)
        obj.append(device.qerror(RX, CB))
        G = device.gram(tX, CB)
        Rsq, ok, _ = device.polar_factor(G)
        assert ok
        R = Rsq.t().contiguous()               # back to the memory image
        RX = device.rotate_T(R, tX)
        C = device.update_codebooks_chain(RX, B, h)
        B = device.quantize_chainq(RX, C)
    torch.cuda.synchronize()
    return C.cpu().numpy(), B.cpu().numpy(), R.cpu().numpy(), np.array(obj)


def _rotation(d, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return q.astype(np.float32)


@pytest.mark.parametrize("rot", ["identity", "seeded"])
def test_train_chainq_equals_composed_steps(rq, rot):
    from rayuela_jl_amd.ChainQ import train_chainq_u8
    X, B0, R0, h = train_case()
    n, d = X.shape
    m = B0.shape[1]
    if rot == "seeded":
        R0 = _rotation(d, 5)
    C, codes, R, obj = train_chainq_u8(X, B0, m, h, R0, TRAIN_NITER)
    Cc, codes_c, Rc, obj_c = _composed(X, B0, R0, h, TRAIN_NITER)
    assert np.array_equal(codes, codes_c)
    assert _same_bits(C, Cc) and _same_bits(R, Rc)
    assert _same_bits(obj, obj_c)
    C2, codes2, R2, obj2 = train_chainq_u8(X, B0, m, h, R0, TRAIN_NITER)
    assert np.array_equal(codes2, codes) and _same_bits(C2, C) and _same_bits(R2, R) and _same_bits(obj2, obj)


def test_train_chainq_objective_codes_and_rotation(rq):
    """The input falls by more than 1 % per round in the restatement (tests/test_chain_oracle.py checks that), so the
    device's sequence must fall strictly."""
    from rayuela_jl_amd.ChainQ import last_chainq_timing
    X, B0, R0, h = train_case()
    m = B0.shape[1]
    B1 = B0.astype(np.int16) + 1
    C, B, R, obj = rq.train_chainq(X, m, h, R0, B1, None, TRAIN_NITER)
    print("obj", obj)
    assert obj.shape == (TRAIN_NITER + 1,) and obj.dtype == np.float32
    assert (obj[1:] < obj[:-1]).all()
    assert B.dtype == np.int16 and B.shape == B1.shape and B.min() >= 1 and B.max() <= h
    assert np.array_equal(B1, B0.astype(np.int16) + 1)          # the start codes are left alone
    R64 = R.astype(np.float64)
    assert np.abs(R64 @ R64.T - np.eye(R.shape[0])).max() < 1e-5
    assert len(C) == m and all(c.shape == (h, X.shape[1]) for c in C) and _zero_outside(np.stack(C))
    t = last_chainq_timing()
    assert all(v >= 0 for v in t.values())
    assert t["unary_ms"] > 0 and t["viterbi_ms"] > 0 and t["update_ms"] > 0 and t["rotation_ms"] > 0 and t["tables_ms"] > 0
    # the final codes are the Viterbi codes of the final (R, C)
    RX = rq.rotate(R, X)
    assert np.array_equal(rq.quantize_chainq(RX, C)[0], B)
    t = last_chainq_timing()              # the clock now shows that encode alone
    assert t["update_ms"] == 0 and t["rotation_ms"] == 0 and t["viterbi_ms"] > 0


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_device_work(rq):
    import torch
    from rayuela_jl_amd import _lib, device
    L = _lib.lib()
    tX = torch.zeros((4, 8), dtype=torch.float32, device=_dev())
    tB = torch.zeros((4, 2), dtype=torch.uint8, device=_dev())
    out = torch.full((4, 2), 9, dtype=torch.uint8, device=_dev())
    s = torch.cuda.current_stream().cuda_stream

    def enc(m, h, C):
        return L.rq_dev_quantize_chainq(out.data_ptr(), tX.data_ptr(), C.data_ptr(), 4, 8, m, h, 1, s)
    tC = torch.zeros((17 * 257 * 8,), dtype=torch.float32, device=_dev())
    for m, h, word in [(0, 4, b"m=0"), (17, 4, b"m=17"), (2, 257, b"h=257"), (2, 1, b"h=1")]:
        assert enc(m, h, tC) == -1 and word in L.rq_last_error()
    torch.cuda.synchronize()
    assert int(out.min()) == 9                              # nothing ran
    with pytest.raises(ValueError):
        device.update_codebooks_chain(tX, tB[:, :1].contiguous(), 4)             # update with m = 1
    with pytest.raises(ValueError):
        device.update_codebooks_chain(tX, tB[:3].contiguous(), 4)                # wrong shape
    with pytest.raises(ValueError):
        device.quantize_chainq(tX, torch.zeros((2, 4, 7), dtype=torch.float32, device=_dev()))
    with pytest.raises(rq.RayuelaHipError):
        device.update_codebooks_chain(tX, tB + 4, 4)                             # codes >= h
    Cout = np.full((2, 4, 8), 7, np.float32)
    X = np.zeros((4, 8), np.float32)
    B = np.full((4, 2), 4, np.uint8)
    assert L.rq_update_codebooks_chain(Cout.ctypes.data, X.ctypes.data, B.ctypes.data, 4, 8, 2, 4, 1e-4) == -1
    assert b">= h" in L.rq_last_error() and (Cout == 7).all()
