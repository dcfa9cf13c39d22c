"""CPU: the LSQ encoding restatement (tests/icm_oracle.py) against fixtures whose conditioning steps are the
reference's own `condition` (tests/gen_icm_golden.py), its random streams, the Python mirror's argument checks and the
generated code of the ILS kernel (no scratch)."""
import os
import re
import subprocess

import numpy as np
import pytest

import icm_oracle as io
from conftest import GOLDEN, ROOT, golden

CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("icm_") and f.endswith(".npz"))


def test_fixtures_exist():
    assert len(CASES) >= 6


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_reference_condition_fixtures(oracle, name):
    g = golden(name)
    ils, icm, npert, randord, seed, t0 = [int(v) for v in g["params"]]
    B, cost = io.ils(oracle, g["X"], g["C"], g["B0"], ils, icm, npert, bool(randord), seed=seed, t0=t0)
    assert np.array_equal(B, g["codes"])
    assert np.array_equal(cost.view(np.uint32), g["cost"].view(np.uint32))
    if name.endswith("all_rejected"):
        assert np.array_equal(B, g["B0"])


def test_subset_of_rows_equals_the_whole(oracle):
    g = golden("icm_m8_rand_pert")
    ils, icm, npert, randord, seed, t0 = [int(v) for v in g["params"]]
    rows = np.array([3, 50, 51, 190])
    B, _ = io.ils(oracle, g["X"][rows], g["C"], g["B0"][rows], ils, icm, npert, bool(randord), seed=seed, t0=t0,
                  rows=rows)
    assert np.array_equal(B, g["codes"][rows])


def test_splitmix64_known_answer():
    assert io.z(0) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("m,npert", [(1, 0), (1, 1), (4, 2), (8, 0), (8, 3), (8, 8), (16, 5)])
def test_perturbation_takes_exactly_npert_distinct_positions(m, npert):
    take, vals = io.perturbation(7, 3, np.arange(5000), m, 100, npert)
    assert (take.sum(axis=1) == npert).all()
    assert vals.min() >= 0 and vals.max() < 100
    if 0 < npert < m:   # every position gets picked sometimes
        assert take.any(axis=0).all()


def test_random_stream_known_answers():
    assert io.visit_order(0, 3, 8, True) == [6, 7, 1, 5, 3, 2, 4, 0]
    assert io.visit_order(0, 3, 8, False) == list(range(8))
    take, vals = io.perturbation(1, 2, np.arange(3), 8, 256, 3)
    assert take.astype(int).tolist() == [[0, 0, 1, 0, 1, 0, 1, 0], [1, 0, 1, 0, 0, 0, 0, 1], [1, 1, 0, 0, 0, 0, 0, 1]]
    assert vals[0].tolist() == [186, 108, 251, 57, 100, 84, 55, 145]


@pytest.mark.parametrize("m", [1, 2, 5, 16])
def test_visit_order_is_a_permutation(m):
    for t in range(50):
        assert sorted(io.visit_order(9, t, m, True)) == list(range(m))
    if m >= 5:
        assert len({tuple(io.visit_order(9, t, m, True)) for t in range(50)}) > 1


def test_cost_never_increases(oracle):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((300, 24)).astype(np.float32)
    C = (rng.standard_normal((6, 64, 24)) * 0.5).astype(np.float32)
    B = rng.integers(0, 64, size=(300, 6)).astype(np.uint8)
    tabs = io.tables(oracle, X, C)
    cost = io.veccost(X, B, C)
    for t in range(4):
        B, c = io.ils(oracle, X, C, B, 1, 2, 2, True, seed=3, t0=t, tabs=tabs)
        assert (c <= cost).all()
        assert np.array_equal(c.view(np.uint32), io.veccost(X, B, C).view(np.uint32))
        cost = c


def test_veccost_butterfly_matches_float64_closely():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((50, 130)).astype(np.float32)
    C = rng.standard_normal((3, 16, 130)).astype(np.float32)
    B = rng.integers(0, 16, size=(50, 3)).astype(np.uint8)
    rec = C[np.arange(3)[None, :], B.astype(np.int64)].astype(np.float64).sum(axis=1)
    want = ((rec - X) ** 2).sum(axis=1)
    np.testing.assert_allclose(io.veccost(X, B, C), want, rtol=1e-5)


def _args(n=10, d=8, m=4, h=256):
    rng = np.random.default_rng(2)
    return (rng.standard_normal((n, d)).astype(np.float32), rng.integers(1, h + 1, size=(n, m)).astype(np.int16),
            [rng.standard_normal((h, d)).astype(np.float32) for _ in range(m)])


def test_python_argument_checks_run_before_the_library(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    X, B, C = _args()
    bad = [
        lambda: rq.encoding_icm(X, B.copy(), C, 1, 1, True, 5),                        # npert > m
        lambda: rq.encoding_icm(X, B.copy(), C, -1, 1, True, 1),                       # negative ilsiter
        lambda: rq.encoding_icm(X, B.copy(), C, 1, -1, True, 1),                       # negative icmiter
        lambda: rq.encoding_icm(X, np.zeros_like(B), C, 1, 1, True, 1),                # zero-based codes
        lambda: rq.encoding_icm(X, B.copy(), [c[:64] for c in C], 1, 1, True, 1),      # cpp with h != 256
        lambda: rq.encoding_icm(X[:, :4], B.copy(), C, 1, 1, True, 1),                 # d mismatch
        lambda: rq.encode_icm_cuda(X, B, C, [2], 1, 1, True, nsplits=0),               # nsplits < 1
        lambda: rq.encode_icm_cuda(X, B, C, [0], 1, 1, True),                          # no iterations
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    X17, B17, C17 = _args(m=17)
    with pytest.raises(ValueError):
        rq.encoding_icm(X17, B17, C17, 1, 1, True, 1)                                   # m > 16
    Xh, Bh, Ch = _args(h=1)
    with pytest.raises(ValueError):
        rq.encoding_icm(Xh, Bh, Ch, 1, 1, False, 1, cpp=False)                          # h < 2
    with pytest.raises(TypeError):
        rq.encoding_icm(X, B.astype(np.int32), C, 1, 1, True, 1)                        # oldB must be Int16
    # cpp=False lifts the h = 256 requirement: the check passes and the (patched) library is reached
    Xs, Bs, Cs = _args(h=64)
    with pytest.raises(AssertionError, match="library touched"):
        rq.encoding_icm(Xs, Bs, Cs, 1, 1, True, 1, cpp=False)


def test_c_abi_argument_checks(rq):
    """The C entry refuses bad arguments through rq_last_error before any device work (no GPU needed)."""
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    X = np.zeros((4, 8), np.float32)
    C = np.zeros((2, 4, 8), np.float32)
    B = np.zeros((4, 2), np.uint8)
    out = np.zeros_like(B)

    def call(m=2, h=4, npert=1, ils=1, icm=1, t0=0, ns=1, codes=B):
        return L.rq_encode_icm(out.ctypes.data, codes.ctypes.data, None, X.ctypes.data, C.ctypes.data, 4, 8, m, h,
                               ils, icm, npert, 1, 0, t0, ns)
    for kw, word in [(dict(m=17), b"m=17"), (dict(h=1), b"h=1"), (dict(npert=3), b"npert=3"), (dict(ils=-1), b"negative"),
                     (dict(ns=0), b"nsplits"), (dict(t0=-1), b"negative"), (dict(codes=B + 4), b">= h")]:
        assert call(**kw) == -1
        assert word in L.rq_last_error()


@pytest.fixture(scope="module")
def icm_asm(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("icm") / "rq_icm.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                           "--cuda-device-only", os.path.join(ROOT, "rayuela.jl_amd", "csrc", "rq_icm.hip"), "-o",
                           str(out)], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_icm_kernels_use_no_scratch(icm_asm):
    """Every kernel of rq_icm.hip: no private segment, no VGPR spills, no scratch instructions.  (SGPR spills of
    loop-invariant scalars at m > 4 go to VGPR lanes, never to memory.)"""
    metas = re.findall(r"\.name:\s+(\S+)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)", icm_asm, flags=re.S)
    names = [n for n, _ in metas if "icm_" in n]
    assert sum("icm_ils_kernel" in n for n in names) == 12 and any("icm_unary_kernel" in n for n in names)
    for name, meta in metas:
        if "icm_" not in name:
            continue
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), name
    assert not re.search(r"^\s*scratch_|buffer_store_dword\s.*off(set)?.*s\[0:3\]", icm_asm, flags=re.M)
