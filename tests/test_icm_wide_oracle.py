"""CPU: the LSQ encoding restatement over int16 codes (tests/icm_wide_oracle.py) against tests/icm_oracle.py and a literal
scalar-loop conditioning step, rq_icm_wide_plan's known answers, the argument checks of rq_encode_icm_wide and of the Python
mirrors (no device), and the generated code of rq_icm_h16.hip (no scratch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import icm_oracle as io
import icm_wide_oracle as wo
from conftest import GOLDEN, ROOT, golden

CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("icm_") and f.endswith(".npz"))
RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_wide_oracle_equals_the_byte_oracle_on_the_fixtures(oracle, name):
    g = golden(name)
    ils, icm, npert, randord, seed, t0 = [int(v) for v in g["params"]]
    B, cost = wo.ils(oracle, g["X"], g["C"], g["B0"], ils, icm, npert, bool(randord), seed=seed, t0=t0)
    B0, cost0 = io.ils(oracle, g["X"], g["C"], g["B0"], ils, icm, npert, bool(randord), seed=seed, t0=t0)
    assert B.dtype == np.int16 and np.array_equal(B, B0) and np.array_equal(B, g["codes"])
    assert np.array_equal(cost.view(np.uint32), cost0.view(np.uint32))
    assert np.array_equal(cost.view(np.uint32), g["cost"].view(np.uint32))


def test_blocked_dots_equal_the_padded_square(oracle):
    rng = np.random.default_rng(0)
    for na, nb, d in [(70, 9, 5), (33, 40, 37), (300, 7, 16)]:
        A = rng.standard_normal((na, d)).astype(np.float32)
        Bm = rng.standard_normal((nb, d)).astype(np.float32)
        assert np.array_equal(wo.dots(oracle, A, Bm).view(np.uint32), io._dots(oracle, A, Bm).view(np.uint32))


def test_one_conditioning_step_equals_the_literal_loops_at_h300(oracle):
    rng = np.random.default_rng(1)
    n, d, m, h = 3, 8, 3, 300
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    C[1, 299] = C[1, 7]                                   # a tie between two codewords: the first index wins
    U, binT = wo.tables(oracle, X, C)
    assert np.array_equal(binT[2, 0], binT[0, 2].T) and not binT[1, 1].any()
    B = rng.integers(256, h, size=(n, m)).astype(np.int16)
    for j in (1, 0, 2):
        a, b = B.copy(), B.copy()
        io.condition(a, U, binT, j)
        wo.condition_literal(b, U, binT, j)
        assert np.array_equal(a, b)
        assert (a[:, 1] != 299).all()
        B = a


def test_codes_past_255_survive_the_whole_encode(oracle):
    rng = np.random.default_rng(2)
    n, d, m, h = 40, 8, 2, 300
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    B0 = rng.integers(0, h, size=(n, m)).astype(np.int16)
    B, cost = wo.ils(oracle, X, C, B0, 2, 2, 1, True, seed=3)
    assert B.max() > 255 and B.max() < h and B.min() >= 0
    assert (cost <= io.veccost(X, B0, C)).all()
    assert np.array_equal(cost.view(np.uint32), io.veccost(X, B, C).view(np.uint32))


# ---- rq_icm_wide_plan: the shape rule and the row chunks, no device ----------------------------------------------------------------
def _plan(rq, n, d, m, h, nsplits, cap=5):
    from rayuela_jl_amd import _lib
    out = (ctypes.c_int64 * 5)(*([-7] * 5))
    rc = _lib.lib().rq_icm_wide_plan(n, d, m, h, nsplits, ctypes.cast(out, ctypes.c_void_p), cap)
    return rc, list(out)


def test_plan_known_answers(rq):
    G = 2 << 30
    assert _plan(rq, 1000, 16, 8, 1024, 1) == (0, [1024, 268435456 + 32768, 32768, 1000, 1])
    assert _plan(rq, 1000, 16, 1, 257, 1) == (0, [320, 257 * 320 * 4 + 257 * 4, 1280, 1000, 1])
    assert _plan(rq, 1000, 16, 8, 256, 1)[1][:3] == [256, 8 * 8 * 256 * 256 * 4 + 8 * 256 * 4, 8 * 256 * 4]
    # nsplits is the minimum number of chunks ...
    assert _plan(rq, 1000, 16, 8, 1024, 3)[1][3:] == [334, 3]
    assert _plan(rq, 1000, 16, 8, 1024, 7)[1][3:] == [143, 7]
    assert _plan(rq, 5, 16, 8, 1024, 7)[1][3:] == [1, 5]
    # ... and the scratch left beside the tables the maximum chunk: (8, 2048) and (16, 1024) hold 1 GiB of tables
    for m, h in ((8, 2048), (16, 1024)):
        rc, (HS, tab, row, chunk, chunks) = _plan(rq, 10_000_000, 128, m, h, 1)
        assert rc == 0 and HS == h and tab == (1 << 30) + m * h * 4 and row == m * h * 4
        assert chunk == (G - tab) // row and chunks == -(-10_000_000 // chunk) and chunks > 1
    assert _plan(rq, 0, 16, 8, 1024, 2) == (0, [1024, 268435456 + 32768, 32768, 0, 0])
    assert _plan(rq, 1000, 16, 8, 1024, 1, cap=2)[1] == [1024, 268435456 + 32768, -7, -7, -7]


def test_plan_refusals(rq):
    L = rq.lib()
    rc, out = _plan(rq, 1000, 16, 16, 2048, 1)
    assert rc == RQ_EUNSUPPORTED and out == [-7] * 5 and b"h=2048" in L.rq_last_error()
    assert _plan(rq, 1000, 16, 2, 16384, 1)[0] == RQ_EUNSUPPORTED
    # around the largest h of every m: exactly the rule of the header, in C and in the Python mirror
    def fits(m, h):
        HS = 64 * -(-h // 64)
        return m * m * h * HS * 4 + m * h * 4 + 4 * (m * HS * 4) <= 2 << 30

    for m in (1, 2, 3, 4, 8, 16):
        hmax = max(h for h in range(2, 32768) if fits(m, h))
        for h in range(hmax - 70, min(hmax + 70, 32768)):
            assert (_plan(rq, 10, 4, m, h, 1)[0] == 0) == fits(m, h) == rq.LSQ.wide_fits(m, h), (m, h)
        assert _plan(rq, 10, 4, m, hmax + 1, 1)[0] == RQ_EUNSUPPORTED
    assert fits(8, 2048) and fits(16, 1024) and not fits(16, 2048)
    for args, word in [((10, 4, 17, 300, 1), b"m=17"), ((10, 4, 0, 300, 1), b"m=0"), ((10, 4, 2, 1, 1), b"h=1"),
                       ((10, 4, 2, 32768, 1), b"h=32768"), ((10, 0, 2, 300, 1), b"d=0"), ((-1, 4, 2, 300, 1), b"negative"),
                       ((10, 4, 2, 300, 0), b"nsplits")]:
        rc, out = _plan(rq, *args)
        assert rc == RQ_EINVAL and out == [-7] * 5 and word in L.rq_last_error(), args


# ---- rq_encode_icm_wide refuses bad arguments before any device work -----------------------------------------------------------------
def test_c_abi_argument_checks(rq):
    L = rq.lib()
    X = np.zeros((4, 8), np.float32)
    C = np.zeros((2, 300, 8), np.float32)
    B = np.full((4, 2), 299, np.int16)
    out = np.full_like(B, -5)
    cost = np.full(4, -5.0, np.float32)

    def call(m=2, h=300, npert=1, ils=1, icm=1, t0=0, ns=1, codes=B, base=0, n=4, d=8, Cp=C.ctypes.data):
        return L.rq_encode_icm_wide(out.ctypes.data, codes.ctypes.data, cost.ctypes.data, X.ctypes.data, Cp, n, d, m, h,
                                    ils, icm, npert, 1, 0, t0, ns, base)
    for kw, word in [(dict(m=17), b"m=17"), (dict(h=1), b"h=1"), (dict(npert=3), b"npert=3"), (dict(ils=-1), b"negative"),
                     (dict(icm=-1), b"negative"), (dict(n=-1), b"negative"), (dict(t0=-1), b"negative"),
                     (dict(ns=0), b"nsplits"), (dict(base=2), b"code_base"), (dict(d=0), b"d=0"),
                     (dict(codes=B + 1), b"outside 0..299"), (dict(codes=B - 300), b"outside 0..299"),
                     (dict(base=1, codes=B - 299), b"outside 1..300"), (dict(Cp=None), b"null")]:
        assert call(**kw) == RQ_EINVAL, kw
        assert word in L.rq_last_error(), (kw, L.rq_last_error())
    assert call(m=16, h=2048) == RQ_EUNSUPPORTED and b"h=2048" in L.rq_last_error()
    assert (out == -5).all() and (cost == -5.0).all()                 # no output byte is written on error
    assert call(n=0) == 0                                             # nothing to do: no device needed


# ---- the Python mirrors check before the library is touched ---------------------------------------------------------------------------
def _args(n=6, d=4, m=2, h=300):
    rng = np.random.default_rng(2)
    return (rng.standard_normal((n, d)).astype(np.float32), rng.integers(1, h + 1, size=(n, m)).astype(np.int16),
            [np.zeros((h, d), np.float32) for _ in range(m)])


def test_python_argument_checks_run_before_the_library(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd.LSQ import encode_icm_u16, encode_icm_u8
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    X, B, C = _args()
    B[0, 0], B[0, 1] = 300, 1                           # both ends of the one-based range
    bad = [
        lambda: rq.encoding_icm(X, B.copy(), C, 1, 1, True, 1),                              # cpp=True keeps requiring h = 256
        lambda: rq.encoding_icm(X, B.copy(), C, 1, 1, True, 3, cpp=False),                   # npert > m
        lambda: rq.encoding_icm(X, B + 1, C, 1, 1, True, 1, cpp=False),                      # a code past h
        lambda: rq.encoding_icm(X, B - 1, C, 1, 1, True, 1, cpp=False),                      # zero-based codes
        lambda: rq.encode_icm_cuda(X, B, C, [2], 1, 1, True, nsplits=0),                     # nsplits < 1
        lambda: rq.veccost(X, B + 1, C),
        lambda: rq.qerror(X[:, :3], B, C),                                                   # d mismatch
        lambda: encode_icm_u16(X, B - 1, C, -1, 1, 1, True),                                 # negative ilsiter
        lambda: encode_icm_u16(X, B, C, 1, 1, 1, True),                                      # one-based codes: 300 >= h
        lambda: encode_icm_u16(X, B - 1, C, 1, 1, 1, True, t0=-1),
        lambda: encode_icm_u8(X, (B - 1).astype(np.uint8), C, 1, 1, 1, True),                # the byte entry keeps refusing h > 256
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
    # the fit rule, restated in Python: (16, 2048) is refused, (8, 2048) reaches the library
    h = 2048
    Xf = np.zeros((1, 2), np.float32)
    with pytest.raises(ValueError, match="do not fit"):
        encode_icm_u16(Xf, np.zeros((1, 16), np.int16), np.zeros((16, h, 2), np.float32), 1, 1, 1, True)
    with pytest.raises(ValueError, match="do not fit"):
        rq.veccost(Xf, np.ones((1, 16), np.int16), np.zeros((16, h, 2), np.float32))
    with pytest.raises(ValueError):
        encode_icm_u16(Xf, np.zeros((1, 1), np.int16), np.zeros((1, 32768, 2), np.float32), 1, 1, 1, True)
    with pytest.raises(AssertionError, match="library touched"):
        encode_icm_u16(Xf, np.zeros((1, 8), np.int16), np.zeros((8, h, 2), np.float32), 1, 1, 1, True)
    # h > 256 passes every mirror's checks and reaches the (patched) library
    for f in (lambda: rq.encoding_icm(X, B.copy(), C, 1, 1, True, 1, cpp=False),
              lambda: rq.encode_icm_cuda(X, B, C, [1], 1, 1, True),
              lambda: rq.veccost(X, B, C), lambda: rq.qerror(X, B, C),
              lambda: encode_icm_u16(X, B - 1, C, 1, 1, 1, True)):
        with pytest.raises(AssertionError, match="library touched"):
            f()


def test_mirrors_route_by_h(rq, monkeypatch):
    """h <= 256 keeps the byte entry, h > 256 takes the wide one; both see zero-based codes of their own width."""
    from rayuela_jl_amd import LSQ
    seen = []

    def fake(name, dtype):
        def fn(X, codes0, Cs, ilsiter, icmiter, npert, randord, seed=0, t0=0, nsplits=1, with_cost=False):
            assert codes0.dtype == dtype and codes0.min() >= 0 and codes0.max() == Cs.shape[1] - 1
            seen.append(name)
            out = np.array(codes0, dtype=dtype)
            return (out, np.zeros(len(out), np.float32)) if with_cost else out
        return fn
    monkeypatch.setattr(LSQ, "encode_icm_u8", fake("u8", np.uint8))
    monkeypatch.setattr(LSQ, "encode_icm_u16", fake("u16", np.int16))
    for h, want in ((256, "u8"), (257, "u16")):
        X, B, C = _args(h=h)
        B[0, 0] = h
        oldB = B.copy()
        out = rq.encoding_icm(X, oldB, C, 1, 1, True, 1, cpp=False)
        assert out.dtype == np.int16 and np.array_equal(out, B) and np.array_equal(oldB, B)
        Bs, objs = rq.encode_icm_cuda(X, B, C, [1, 2], 1, 1, True)
        assert all(b.dtype == np.int16 and np.array_equal(b, B) for b in Bs) and Bs[0] is not Bs[1]
        rq.veccost(X, B, C)
        assert seen == [want] * 4
        del seen[:]


# ---- the generated code -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def icm_h16_asm(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("icm_h16") / "rq_icm_h16.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                           "--cuda-device-only", os.path.join(ROOT, "rayuela.jl_amd", "csrc", "rq_icm_h16.hip"), "-o",
                           str(out)], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_wide_icm_kernels_use_no_scratch(icm_h16_asm):
    """Every kernel of rq_icm_h16.hip, by its metadata: no private segment and no VGPR spills, whatever h is at run time."""
    metas = re.findall(r"\.name:\s+(\S+)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)", icm_h16_asm, flags=re.S)
    metas = [(n, meta) for n, meta in metas if "_kernel" in n]
    names = [n for n, _ in metas]
    assert sum("icm_ils_h16_kernel" in n for n in names) == 3 and sum("icm_pair_h16_kernel" in n for n in names) == 1
    assert len(names) == 4
    for name, meta in metas:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), name
