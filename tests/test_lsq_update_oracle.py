"""CPU: the LSQ codebook update restatement (tests/lsq_update_oracle.py) against a literal transcription of the
reference's loops (src/codebook_update.jl:96-170), the Python mirror's argument checks, the C entries' argument checks and
the generated code of rq_lsq.hip (no scratch)."""
import os
import re
import subprocess

import numpy as np
import pytest

import lsq_update_oracle as lo
from conftest import ROOT


def literal_fast_bin_matmul(X, B, h, rho=1e-4):
    """src/codebook_update.jl:96-170 loop for loop.  X is Julia's d-by-n matrix, B its m-by-n one-based Int16 codes."""
    d, n = X.shape
    m = B.shape[0]
    BTB = [[None] * m for _ in range(m)]
    hi = np.zeros(h, np.float32)
    for i in range(m):                                           # :118-131
        hi[:] = 0
        for j in range(n):
            hi[B[i, j] - 1] += np.float32(1)
        BTB[i][i] = np.diag(hi).astype(np.float32)
    for i in range(m):                                           # :134-149
        for j in range(i + 1, m):
            cij = np.zeros((h, h), np.float32)
            for k in range(n):
                cij[B[j, k] - 1, B[i, k] - 1] += np.float32(1)
            BTB[i][j] = cij
            BTB[j][i] = cij.T.copy()
    # hvcat(m, BTB...) (:152): splatting the column-major Matrix{Matrix} yields BTB[1,1], BTB[2,1], ..., BTB[m,1],
    # BTB[1,2], ...; hvcat lays them out m per block row
    blocks = [BTB[r][c] for c in range(m) for r in range(m)]
    BTBc = np.vstack([np.hstack(blocks[q * m:(q + 1) * m]) for q in range(m)])
    BXT = []
    for i in range(m):                                           # :154-164
        BXTi = np.zeros((d, h))
        for j in range(n):
            BXTi[:, B[i, j] - 1] += X[:, j].astype(np.float64)
        BXT.append(BXTi)
    b = np.hstack(BXT).T                                         # hcat(BXT...)'
    A = BTBc.astype(np.float64) + rho * np.eye(m * h)            # Float32 + Float64 I promotes; diagonal fl64(count + rho)
    return A, b


@pytest.mark.parametrize("n,d,m,h,seed", [(40, 5, 3, 4, 0), (64, 3, 4, 6, 1), (17, 7, 1, 5, 2), (0, 4, 2, 3, 3),
                                          (200, 9, 2, 16, 4)])
def test_restatement_equals_the_reference_loops(n, d, m, h, seed):
    rng = np.random.default_rng(seed)
    # non-integer values over 2^-30 .. 2^30: their f64 sums round, so the summation order shows in the bits
    X = (rng.standard_normal((n, d)) * np.exp2(rng.integers(-30, 31, size=(n, d)))).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m))
    A0, b0 = literal_fast_bin_matmul(X.T.copy(), (codes.T + 1).astype(np.int16), h)
    A, b = lo.normal_eq(X, codes, h)
    assert np.array_equal(A.view(np.uint64), A0.view(np.uint64))
    assert np.array_equal(b.view(np.uint64), b0.view(np.uint64))


def test_hvcat_orientation_gives_the_true_gram_matrix():
    """The transposes of BTB[i,j] = cij (indexed [code_j, code_i]) and of the column-major splat cancel: B'B exactly."""
    rng = np.random.default_rng(5)
    n, m, h = 300, 3, 5
    codes = rng.integers(0, h, size=(n, m))
    onehot = np.zeros((n, m * h))
    onehot[np.arange(n)[:, None], codes + np.arange(m)[None, :] * h] = 1
    A0, _ = literal_fast_bin_matmul(np.zeros((1, n), np.float32), (codes.T + 1).astype(np.int16), h, rho=0.5)
    assert np.array_equal(A0, onehot.T @ onehot + 0.5 * np.eye(m * h))
    # asymmetric pair counts, so a transposed block would show
    assert not np.array_equal(A0[:h, h:2 * h], A0[:h, h:2 * h].T)


def test_summation_order_is_ascending_rows():
    """b's bits are those of a left-to-right f64 sum; a pairwise or reversed sum differs on this data."""
    X = np.array([[1e16], [1.0], [-1e16], [1.0]], dtype=np.float32)
    _, b = lo.normal_eq(X, np.zeros((4, 1), np.int64), 2)
    want = 0.0
    for v in X[:, 0].astype(np.float64):
        want = want + v
    assert b[0, 0] == want == 1.0
    assert b[1, 0] == 0.0


def test_unused_codes_get_zero_codewords_and_normal_equations_hold():
    rng = np.random.default_rng(6)
    n, d, m, h, rho = 500, 6, 3, 16, 1e-4
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, 8, size=(n, m))                      # codes 8..15 unused
    C, C64 = lo.update(X, codes, h, rho)
    assert (C[:, 8:] == 0).all() and (C64.reshape(m, h, d)[:, 8:] == 0).all()
    onehot = np.zeros((n, m * h))
    onehot[np.arange(n)[:, None], codes + np.arange(m)[None, :] * h] = 1
    resid = onehot.T @ (onehot @ C64 - X.astype(np.float64)) + rho * C64
    assert np.abs(resid).max() <= 1e-9 * max(1.0, np.abs(onehot.T @ X.astype(np.float64)).max())


def _args(n=10, d=8, m=4, h=256):
    rng = np.random.default_rng(2)
    return (rng.standard_normal((n, d)).astype(np.float32), rng.integers(1, h + 1, size=(n, m)).astype(np.int16))


def test_python_argument_checks_run_before_the_library(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd.LSQ import train_lsq_u8
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    X, B = _args()
    bad = [
        lambda: rq.update_codebooks_fast_bin(X, B, 256, rho=0.0),                      # rho <= 0
        lambda: rq.update_codebooks_fast_bin(X, B, 256, rho=float("inf")),            # rho not finite
        lambda: rq.update_codebooks_fast_bin(X, B, 1),                                 # h < 2
        lambda: rq.update_codebooks_fast_bin(X, B, 257),                               # h > 256
        lambda: rq.update_codebooks_fast_bin(X, np.where(B == B[0, 0], 0, B).astype(np.int16), 256),  # a code 0
        lambda: rq.update_codebooks_fast_bin(X, B[:5], 256),                           # n mismatch
        lambda: rq.update_codebooks_fast_bin(*_args(m=17), 256),                       # m > 16
        lambda: rq.update_codebooks_fast_bin(X, B, 100),                               # codes > h
        lambda: rq.update_codebooks(X, B, 256, False, "lsqr"),                         # unsupported method, named
        lambda: rq.update_codebooks(X, B, 256, False, "bogus"),                        # unknown method
        lambda: rq.train_lsq(X, 4, 256, None, B.copy(), None, -1, 1, 1, True, 1),      # niter < 0
        lambda: rq.train_lsq(X, 4, 256, None, B.copy(), None, 1, 1, 1, True, 5),       # npert > m
        lambda: rq.train_lsq(X, 4, 64, None, B.copy(), None, 1, 1, 1, True, 1),       # cpp with h != 256
        lambda: rq.train_lsq(X, 4, 256, np.eye(4, dtype=np.float32), B.copy(), None, 1, 1, 1, True, 1),  # R shape
        lambda: rq.train_lsq_cuda(X, 4, 256, None, B, None, 1, 1, 1, True, 1, nsplits=0),               # nsplits
        lambda: train_lsq_u8(X, B - 1, 5, 256, None, 1, 1, 1, True, 1),               # m mismatch
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError, match="lsqr"):
        rq.update_codebooks(X, B, 256, False, "lsqr")
    with pytest.raises(TypeError):
        rq.train_lsq(X, 4, 256, None, B.astype(np.int32), None, 1, 1, 1, True, 1)      # B must be Int16


def test_c_abi_argument_checks(rq):
    """Every new entry refuses bad arguments through rq_last_error before any device work (no GPU needed)."""
    import ctypes
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    X = np.zeros((4, 8), np.float32)
    B = np.zeros((4, 2), np.uint8)
    C = np.zeros((2, 4, 8), np.float32)
    A = np.zeros((8, 8))
    b = np.zeros((8, 8))
    obj = np.zeros(2)
    p = lambda a: a.ctypes.data                                   # noqa: E731
    cases = [(dict(m=17), b"m=17"), (dict(m=0), b"m=0"), (dict(h=1), b"h=1"), (dict(h=257), b"h=257"),
             (dict(d=0), b"d=0"), (dict(n=-1), b"n=-1"), (dict(n=1 << 32), b"n="), (dict(rho=0.0), b"rho"),
             (dict(rho=-1.0), b"rho"), (dict(rho=float("nan")), b"rho"), (dict(rho=float("inf")), b"rho"),
             (dict(X=None), b"null"), (dict(codes=None), b"null"), (dict(out=None), b"null")]
    for kw, word in cases:
        a = dict(n=4, d=8, m=2, h=4, rho=1e-4, X=p(X), codes=p(B), out=p(C))
        a.update(kw)
        assert L.rq_update_codebooks_lsq(a["out"], a["X"], a["codes"], a["n"], a["d"], a["m"], a["h"], a["rho"]) == -1
        assert word in L.rq_last_error(), (kw, L.rq_last_error())
        assert L.rq_dev_update_codebooks_lsq(a["out"], a["X"], a["codes"], a["n"], a["d"], a["m"], a["h"], a["rho"],
                                             None) == -1
        assert word in L.rq_last_error(), (kw, L.rq_last_error())
        outA = None if kw.get("out", 1) is None else p(A)
        assert L.rq_dev_lsq_normal_eq(outA, p(b), a["X"], a["codes"], a["n"], a["d"], a["m"], a["h"], a["rho"],
                                      None) == -1
        assert word in L.rq_last_error(), (kw, L.rq_last_error())
    # host entry: a code >= h
    assert L.rq_update_codebooks_lsq(p(C), p(X), p(B + 4), 4, 8, 2, 4, 1e-4) == -1 and b">= h" in L.rq_last_error()

    def train(**kw):
        a = dict(C=p(C), codes=p(B), obj=p(obj), X=p(X), n=4, d=8, m=2, h=4, niter=2, ils=1, icm=1, npert=1, ns=1)
        a.update(kw)
        return L.rq_train_lsq(a["C"], a["codes"], a["obj"], a["X"], None, a["n"], a["d"], a["m"], a["h"], a["niter"],
                              a["ils"], a["icm"], a["npert"], 1, 0, a["ns"])
    for kw, word in [(dict(m=17), b"m=17"), (dict(h=1), b"h=1"), (dict(niter=-1), b"niter"), (dict(obj=None), b"obj"),
                     (dict(npert=3), b"npert=3"), (dict(ils=-1), b"negative"), (dict(ns=0), b"nsplits"),
                     (dict(codes=p(B + 4)), b">= h"), (dict(C=None), b"null"), (dict(codes=None), b"null"),
                     (dict(X=None), b"null"), (dict(ils=1 << 30), b"overflows")]:
        assert train(**kw) == -1, kw
        assert word in L.rq_last_error(), (kw, L.rq_last_error())
    out = (ctypes.c_double * 7)()
    assert L.rq_last_lsq_timing(None, 7) == -1
    assert L.rq_last_lsq_timing(ctypes.cast(out, ctypes.c_void_p), 7) == 0


@pytest.fixture(scope="module")
def lsq_asm(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("lsq") / "rq_lsq.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                           "--cuda-device-only", os.path.join(ROOT, "rayuela.jl_amd", "csrc", "rq_lsq.hip"), "-o",
                           str(out)], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_lsq_kernels_use_no_scratch(lsq_asm):
    """Every kernel of rq_lsq.hip: no private segment, no VGPR spills, no scratch instructions, no float atomics."""
    metas = re.findall(r"\.name:\s+(\S+)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)", lsq_asm, flags=re.S)
    names = [n for n, _ in metas if "lsq_" in n]
    for k in ("lsq_pair_kernel", "lsq_bsum_kernel", "lsq_scatter_kernel", "lsq_chol_diag_kernel", "lsq_gemm_sub_kernel",
              "lsq_trsv_block_kernel", "lsq_assemble_kernel"):
        assert any(k in n for n in names), k
    for name, meta in metas:
        if "lsq_" not in name:
            continue
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), name
    assert not re.search(r"^\s*scratch_|buffer_store_dword\s.*off(set)?.*s\[0:3\]", lsq_asm, flags=re.M)
    assert not re.search(r"^\s*(global|flat|buffer|ds)_atomic_(add|pk_add|min|max)_f(32|64)", lsq_asm, flags=re.M)
