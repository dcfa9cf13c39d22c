"""CPU: the chain quantization restatement (tests/chain_oracle.py) against fixtures whose codes are the reference's own
`viterbi_encoding` (tests/gen_chain_golden.py), the optimality of the Viterbi codes and of the chain codebook update, the
training sequence the GPU test relies on, the Python mirror's argument checks and the generated code of rq_chain.hip."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import chain_oracle as co
import lsq_update_oracle as lo
from conftest import GOLDEN, ROOT, golden

CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("chain_") and f.endswith(".npz"))

# The input of the training tests (here and in tests/test_gpu_chainq.py): Gaussian X, uniform random start codes, identity R
TRAIN_SHAPE = (4000, 24, 4, 64)      # n, d, m, h
TRAIN_NITER = 2                      # obj has niter + 1 = 3 entries


def train_case():
    n, d, m, h = TRAIN_SHAPE
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, d)).astype(np.float32)
    B = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    return X, B, np.eye(d, dtype=np.float32), h


def test_fixtures_exist():
    assert len(CASES) >= 6
    assert {"chain_m4_gauss", "chain_m8_gauss", "chain_m5_uneven", "chain_m4_ties", "chain_m2", "chain_m4_dense"} <= set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_reference_viterbi_fixtures(oracle, name):
    g = golden(name)
    codes = co.viterbi(oracle, g["X"], g["C"])
    assert np.array_equal(codes, g["codes"]), "rows differ: %d" % int((codes != g["codes"]).any(axis=1).sum())


def test_ties_fixture_has_ties(oracle):
    """The integer-valued case is there for the lowest-index rule: its final costs do tie."""
    g = golden("chain_m4_ties")
    U, T = co.tables(oracle, g["X"], g["C"])
    assert (np.sort(U[0], axis=1)[:, 0] == np.sort(U[0], axis=1)[:, 1]).any()


def test_viterbi_reaches_the_brute_force_minimum(oracle):
    rng = np.random.default_rng(7)
    n, d, m, h = 40, 6, 3, 4
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = rng.standard_normal((m, h, d)).astype(np.float32)
    U, T = co.tables(oracle, X, C)
    codes = co.viterbi_tables(U, T)
    best = np.full(n, np.inf)
    for c in itertools.product(range(h), repeat=m):
        best = np.minimum(best, co.energy(U, T, np.tile(np.array(c, dtype=np.uint8), (n, 1))))
    got = co.energy(U, T, codes)
    assert np.all(got <= best + 1e-5 * np.abs(best).max())      # f32 path sums against the f64 energy


def test_single_codebook_is_the_argmin_of_the_unary(oracle):
    rng = np.random.default_rng(8)
    X = rng.standard_normal((30, 5)).astype(np.float32)
    C = rng.standard_normal((1, 9, 5)).astype(np.float32)
    U, _ = co.tables(oracle, X, C)
    assert np.array_equal(co.viterbi(oracle, X, C)[:, 0], np.argmin(U[0], axis=1))


@pytest.mark.parametrize("d,m", [(30, 5), (24, 4), (7, 2), (16, 16)])
def test_get_cbdims_chain(rq, d, m):
    dims = rq.get_cbdims_chain(d, m)
    assert [list(r) for r in dims] == [list(r) for r in co.cbdims(d, m)]
    parts = rq.splitarray(range(d), m - 1)
    assert list(dims[0]) == list(parts[0]) and list(dims[-1]) == list(parts[-1])
    for i in range(1, m - 1):
        assert list(dims[i]) == list(parts[i - 1]) + list(parts[i])


def test_get_cbdims_chain_matches_the_reference_example(rq):
    # splitarray(1:30, 4) = 1:8, 9:16, 17:23, 24:30  ->  1:8, 1:16, 9:23, 17:30, 24:30 (one-based)
    assert [(r[0] + 1, r[-1] + 1) for r in rq.get_cbdims_chain(30, 5)] == [(1, 8), (1, 16), (9, 23), (17, 30), (24, 30)]


def test_chain_update_structure_and_optimality():
    rng = np.random.default_rng(9)
    n, d, m, h = 3000, 14, 4, 16
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    C, _ = co.chain_update(X, codes, h)
    mask = np.zeros((m, d), dtype=bool)
    for i, dims in enumerate(co.cbdims(d, m)):
        mask[i, dims[0]:dims[-1] + 1] = True
    assert (C[~np.broadcast_to(mask[:, None, :], C.shape)] == 0).all()
    q = lo.qerror(X, C, codes)
    step = 0.01 * float(np.abs(C).max())
    for _ in range(20):
        P = C + (rng.choice([-step, step], size=C.shape) * mask[:, None, :]).astype(np.float32)
        assert q <= lo.qerror(X, P, codes)


def test_training_input_falls_by_more_than_one_percent_per_round(oracle):
    """The condition the GPU training test needs of its input: the restated sequence falls by more than 1 % per round,
    with and without the rotation step, so rounding, rho and polar-vs-SVD cannot turn a step around."""
    X, B, R, h = train_case()
    for rotate in (False, True):
        _, codes, Rn, obj = co.train(oracle, X, B, R, h, TRAIN_NITER, rotate=rotate)
        print("rotate=%s obj %s" % (rotate, obj))
        assert obj.shape == (TRAIN_NITER + 1,)
        assert (obj[1:] < 0.99 * obj[:-1]).all()
        assert np.abs(Rn.astype(np.float64) @ Rn.astype(np.float64).T - np.eye(R.shape[0])).max() < 1e-5


def _args(n=10, d=8, m=4, h=256):
    rng = np.random.default_rng(2)
    return (rng.standard_normal((n, d)).astype(np.float32), rng.integers(1, h + 1, size=(n, m)).astype(np.int16),
            [rng.standard_normal((h, d)).astype(np.float32) for _ in range(m)])


def test_python_argument_checks_run_before_the_library(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd.ChainQ import quantize_chainq_u8
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    X, B, C = _args()
    R = np.eye(8, dtype=np.float32)
    X17, B17, C17 = _args(m=17, d=20)
    Xh, Bh, Ch = _args(h=1)
    bad = [
        lambda: rq.quantize_chainq(X[:, :4], C),                                   # d mismatch
        lambda: rq.quantize_chainq(X, []),                                         # m = 0
        lambda: rq.quantize_chainq(X17, C17),                                      # m = 17
        lambda: rq.quantize_chainq(X, [np.zeros((257, 8), np.float32)] * 2),       # h = 257
        lambda: rq.quantize_chainq(Xh, Ch),                                        # h = 1
        lambda: quantize_chainq_u8(X, C, nsplits=0),                               # nsplits < 1
        lambda: rq.update_codebooks_chain_bin(X, B[:, :1], 256),                   # update with m = 1
        lambda: rq.update_codebooks_chain_bin(X, B17, 256),                        # m = 17
        lambda: rq.update_codebooks_chain_bin(X, B, 257),                          # h = 257
        lambda: rq.update_codebooks_chain_bin(X, B, 100),                          # codes >= h
        lambda: rq.update_codebooks_chain_bin(X, np.zeros_like(B), 256),           # zero-based codes
        lambda: rq.update_codebooks_chain_bin(X, B[:5], 256),                      # wrong shape
        lambda: rq.update_codebooks_chain_bin(X, B, 256, rho=0.0),                 # rho
        lambda: rq.update_codebooks_chain_bin(X[:, :2], B, 256),                   # d < m - 1
        lambda: rq.train_chainq(X, 4, 100, R, B, None, 1),                         # codes >= h
        lambda: rq.train_chainq(X, 4, 256, R[:4], B, None, 1),                     # R shape
        lambda: rq.train_chainq(X, 4, 256, R, B, None, -1),                        # niter
        lambda: rq.train_chainq(X, 3, 256, R, B, None, 1),                         # m against the codes
        lambda: rq.get_cbdims_chain(8, 1),
        lambda: rq.get_cbdims_chain(2, 4),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d raised nothing" % k)
    with pytest.raises(TypeError):
        rq.quantize_chainq(X.astype(np.float64), C)
    with pytest.raises(TypeError):
        rq.train_chainq(X, 4, 256, R, B.astype(np.int32), None, 1)
    # good arguments pass the checks and reach the (patched) library
    for f in (lambda: rq.quantize_chainq(X, C, True, True), lambda: rq.update_codebooks_chain_bin(X, B, 256),
              lambda: rq.train_chainq(X, 4, 256, R, B, None, 1)):
        with pytest.raises(AssertionError, match="library touched"):
            f()


def test_c_abi_argument_checks(rq):
    """The C entries refuse bad arguments through rq_last_error before any device work (no GPU needed)."""
    import ctypes
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    X = np.zeros((4, 8), np.float32)
    C = np.zeros((2, 4, 8), np.float32)
    B = np.zeros((4, 2), np.uint8)
    R = np.eye(8, dtype=np.float32)
    obj = np.zeros(2)
    p = lambda a: a.ctypes.data     # noqa: E731

    def enc(m=2, h=4, d=8, n=4, ns=1):
        return L.rq_quantize_chainq(p(B), p(X), p(C), n, d, m, h, ns)

    def upd(m=2, h=4, d=8, rho=1e-4, codes=B):
        return L.rq_update_codebooks_chain(p(C), p(X), p(codes), 4, d, m, h, rho)

    def trn(m=2, h=4, niter=1, codes=B, n=4):
        return L.rq_train_chainq(p(C), p(codes), p(R), p(obj), p(X), n, 8, m, h, niter)
    for call, word in [(lambda: enc(m=0), b"m=0"), (lambda: enc(m=17), b"m=17"), (lambda: enc(h=257), b"h=257"),
                       (lambda: enc(h=1), b"h=1"), (lambda: enc(d=0), b"d=0"), (lambda: enc(n=-1), b"negative"),
                       (lambda: enc(ns=0), b"nsplits"), (lambda: upd(m=1), b"m=1"), (lambda: upd(m=17), b"m=17"),
                       (lambda: upd(h=257), b"h=257"), (lambda: upd(rho=0.0), b"rho"), (lambda: upd(codes=B + 4), b">= h"),
                       (lambda: upd(m=4, d=2), b"m - 1"), (lambda: trn(m=1), b"m=1"), (lambda: trn(niter=-1), b"niter"),
                       (lambda: trn(codes=B + 4), b">= h"), (lambda: trn(n=0), b"n=0")]:
        assert call() == -1
        assert word in L.rq_last_error(), L.rq_last_error()
    lo_, hi_ = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
    assert L.rq_chain_dims(30, 5, ctypes.cast(lo_, ctypes.c_void_p), ctypes.cast(hi_, ctypes.c_void_p)) == 0
    assert list(zip(lo_, hi_)) == [(r[0], r[-1] + 1) for r in co.cbdims(30, 5)]
    assert L.rq_chain_dims(30, 1, ctypes.cast(lo_, ctypes.c_void_p), ctypes.cast(hi_, ctypes.c_void_p)) == -1


@pytest.fixture(scope="module")
def chain_asm(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("chain") / "rq_chain.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                           "--cuda-device-only", os.path.join(ROOT, "rayuela.jl_amd", "csrc", "rq_chain.hip"), "-o",
                           str(out)], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_chain_kernels_use_no_scratch(chain_asm):
    """Every kernel of rq_chain.hip: no private segment, no VGPR or SGPR spills, no scratch instructions."""
    metas = re.findall(r"\.name:\s+(\S+)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)", chain_asm, flags=re.S)
    names = [n for n, _ in metas if "chain_" in n]
    assert any("chain_forward_kernel" in n for n in names) and any("chain_pair_kernel" in n for n in names)
    assert sum("chain_backtrace_kernel" in n for n in names) == 4
    for name, meta in metas:
        if "chain_" not in name:
            continue
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), name
        assert re.search(r"\.sgpr_spill_count:\s+0\b", meta), name
    assert not re.search(r"^\s*scratch_|buffer_store_dword\s.*off(set)?.*s\[0:3\]", chain_asm, flags=re.M)
