"""CPU: the LSQ codebook update restatement over int16 codes (tests/lsq_wide_oracle.py) against tests/lsq_update_oracle.py,
rq_lsq_wide_plan's known answers, the argument checks of rq_update_codebooks_lsq_wide / rq_lsq_normal_eq_wide / rq_train_lsq_wide
and of the Python mirrors (no device), and the generated code of rq_lsq.hip (no scratch in any instantiation)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lsq_update_oracle as lo
import lsq_wide_oracle as wo
from conftest import ROOT

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2


def _wide(rng, n, d):
    """values over 2^-30 .. 2^30: their f64 sums round, so the summation order shows in the bits"""
    return (rng.standard_normal((n, d)) * np.exp2(rng.integers(-30, 31, size=(n, d)))).astype(np.float32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,m,h,seed", [(40, 5, 3, 4, 0), (500, 7, 4, 100, 1), (300, 3, 2, 256, 2), (17, 7, 1, 5, 3),
                                          (0, 4, 2, 3, 4)])
def test_wide_restatement_equals_the_byte_restatement(n, d, m, h, seed):
    rng = np.random.default_rng(seed)
    X = _wide(rng, n, d)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    A0, b0 = lo.normal_eq(X, codes, h)
    for base in (0, 1):
        A, b, cnt = wo.normal_eq(X, codes.astype(np.int16) + base, h, code_base=base)
        assert np.array_equal(A.view(np.uint64), A0.view(np.uint64))
        assert np.array_equal(b.view(np.uint64), b0.view(np.uint64))
        assert cnt.dtype == np.uint32 and cnt.shape == (m, h) and cnt.sum() == n * m
        assert np.array_equal(A[np.arange(m * h), np.arange(m * h)], cnt.reshape(-1) + 1e-4)
    _, b1, cnt1 = wo.normal_eq(X, codes.astype(np.int16), h, with_A=False)
    assert np.array_equal(b1.view(np.uint64), b0.view(np.uint64)) and np.array_equal(cnt1, cnt)


def test_wide_restatement_keeps_codes_past_255_apart():
    """Codes 0 and 256, 255 and 511 share their low byte: every one keeps its own row of b and its own count."""
    X = np.arange(1, 7, dtype=np.float32).reshape(6, 1)
    codes = np.array([[256], [0], [511], [255], [256], [0]], np.int16)
    A, b, cnt = wo.normal_eq(X, codes, 512)
    assert [int(cnt[0, a]) for a in (0, 255, 256, 511)] == [2, 1, 2, 1] and cnt.sum() == 6
    assert [float(b[a, 0]) for a in (0, 255, 256, 511)] == [2 + 6, 4, 1 + 5, 3]
    C, C64 = wo.update_one_codebook(X, codes, 512)
    assert np.allclose(C64, wo.solve(A, b), rtol=1e-12, atol=0)        # a diagonal A: the solve is this division
    assert C[0, 256, 0] == np.float32(6 / (2 + 1e-4)) and (C[0, 1:255] == 0).all()


# ---- rq_lsq_wide_plan: the shape rule and the sizes, no device ---------------------------------------------------------------------
def _plan(rq, n, d, m, h, cap=7):
    out = (ctypes.c_int64 * 7)(*([-7] * 7))
    rc = rq.lib().rq_lsq_wide_plan(n, d, m, h, ctypes.cast(out, ctypes.c_void_p), cap)
    return rc, list(out)


@pytest.mark.parametrize("m,h", [(8, 1024), (16, 1024), (4, 4096), (1, 16384)])
def test_plan_known_answers(rq, m, h):
    n, d = 100_000, 128
    mh = m * h
    rc, out = _plan(rq, n, d, m, h)
    assert rc == 0
    assert out == [mh, mh * mh * 8, mh * mh * 4, wo.sort_scratch_bytes(n, m, h), 25, mh // 64, 1]
    assert out[1] <= 2 << 30 and out[2] <= 1 << 30                 # A within the per-slot scratch figure, the pair counts in half
    assert _plan(rq, n, d, m, h, cap=2)[1] == [mh, mh * mh * 8] + [-7] * 5
    assert _plan(rq, 0, d, m, h)[1][3:6] == [wo.sort_scratch_bytes(0, m, h), 1, mh // 64]


def test_plan_small_shapes_and_refusals(rq):
    L = rq.lib()
    # h <= 256: one sort pass, no per-code counts; a partial last Cholesky block counts as a step
    assert _plan(rq, 5000, 7, 2, 256)[1] == [512, 512 * 512 * 8, 512 * 512 * 4, wo.sort_scratch_bytes(5000, 2, 256), 2, 8, 1]
    assert _plan(rq, 30000, 8, 1, 4097)[1][4:] == [8, 65, 1]
    assert wo.sort_scratch_bytes(5000, 2, 256) == 2 * 256 * 2 * 4 + 2304 + 2 * 5000 * 4
    for m, h in ((16, 2048), (2, 16384), (1, 16385), (16, 1025)):
        rc, out = _plan(rq, 1000, 16, m, h)
        assert rc == RQ_EUNSUPPORTED and out == [-7] * 7 and b"exceeds 16384" in L.rq_last_error(), (m, h)
    for args, word in [((10, 4, 17, 300), b"m=17"), ((10, 4, 0, 300), b"m=0"), ((10, 4, 2, 1), b"h=1"),
                       ((10, 4, 2, 32768), b"h=32768"), ((10, 0, 2, 300), b"d=0"), ((-1, 4, 2, 300), b"n=-1"),
                       ((1 << 32, 4, 2, 300), b"n=4294967296")]:
        rc, out = _plan(rq, *args)
        assert rc == RQ_EINVAL and out == [-7] * 7 and word in L.rq_last_error(), args
    assert _plan(rq, (1 << 32) - 1, 4, 2, 300)[0] == 0


# ---- the C entries refuse bad arguments before any device work, and leave their outputs alone ----------------------------------------
def test_c_abi_argument_checks(rq):
    L = rq.lib()
    n, d, m, h = 4, 8, 2, 300
    X = np.zeros((n, d), np.float32)
    B = np.full((n, m), h - 1, np.int16)
    C = np.full((m, h, d), -5.0, np.float32)
    A = np.full((m * h, m * h), -5.0)
    b = np.full((m * h, d), -5.0)
    cnt = np.full((m, h), 77, np.uint32)
    obj = np.full(2, -5.0)
    codes_io = B.copy()
    p = lambda a: None if a is None else a.ctypes.data             # noqa: E731

    def update(**kw):
        a = dict(n=n, d=d, m=m, h=h, rho=1e-4, X=X, codes=B, out=C, base=0)
        a.update(kw)
        return L.rq_update_codebooks_lsq_wide(p(a["out"]), p(a["X"]), p(a["codes"]), a["n"], a["d"], a["m"], a["h"], a["rho"],
                                              a["base"])

    def normal(A_=A, **kw):
        a = dict(n=n, d=d, m=m, h=h, rho=1e-4, X=X, codes=B, out=b, base=0)
        a.update(kw)
        return L.rq_lsq_normal_eq_wide(p(A_), p(a["out"]), p(cnt), p(a["X"]), p(a["codes"]), a["n"], a["d"], a["m"], a["h"],
                                       a["rho"], a["base"])

    def train(**kw):
        a = dict(n=n, d=d, m=m, h=h, X=X, codes=codes_io, out=C, base=0, obj=obj, niter=2, ils=1, icm=1, npert=1, ns=1)
        a.update(kw)
        return L.rq_train_lsq_wide(p(a["out"]), p(a["codes"]), p(a["obj"]), p(a["X"]), None, a["n"], a["d"], a["m"], a["h"],
                                   a["niter"], a["ils"], a["icm"], a["npert"], 1, 0, a["ns"], a["base"])

    shared = [(dict(h=32768), b"h=32768"), (dict(h=1), b"h=1"), (dict(m=17), b"m=17"), (dict(m=0), b"m=0"), (dict(d=0), b"d=0"),
              (dict(n=-1), b"n=-1"), (dict(n=1 << 32), b"n=4294967296"), (dict(X=None), b"null"), (dict(codes=None), b"null"),
              (dict(out=None), b"null"), (dict(base=2), b"code_base"), (dict(base=-1), b"code_base"),
              (dict(codes=B + 1), b"code 300 at [0][0] is outside 0..299"), (dict(codes=B - h), b"code -1 at [0][0]"),
              (dict(codes=B - (h - 1), base=1), b"code 0 at [0][0] is outside 1..300"),
              (dict(codes=B + 2, base=1), b"code 301 at [0][0] is outside 1..300")]
    rhos = [(dict(rho=0.0), b"rho"), (dict(rho=-1.0), b"rho"), (dict(rho=float("nan")), b"rho"), (dict(rho=float("inf")), b"rho")]
    for fn, cases in ((update, shared + rhos), (normal, shared + rhos),
                      (train, shared + [(dict(niter=-1), b"niter"), (dict(obj=None), b"obj"), (dict(npert=3), b"npert=3"),
                                        (dict(ils=-1), b"negative"), (dict(icm=-1), b"negative"), (dict(ns=0), b"nsplits"),
                                        (dict(ils=1 << 30), b"overflows")])):
        for kw, word in cases:
            assert fn(**kw) == RQ_EINVAL, (fn.__name__, kw)
            assert word in L.rq_last_error(), (fn.__name__, kw, L.rq_last_error())
        for mm, hh in ((16, 2048), (2, 16384)):
            big = np.zeros((n, mm), np.int16)
            assert fn(m=mm, h=hh, codes=big) == RQ_EUNSUPPORTED, (fn.__name__, mm, hh)
            assert fn is train or b"exceeds 16384" in L.rq_last_error()      # train: the encoder's table rule may speak first
    # without A the m * h limit does not apply: the call passes every check and only then asks for a device
    if L.rq_device_count() <= 0:
        assert normal(A_=None, m=16, h=2048, codes=np.zeros((n, 16), np.int16), out=np.zeros((16 * 2048, d))) not in (
            0, RQ_EINVAL, RQ_EUNSUPPORTED)
    # no output byte was written by any refusal
    assert (C == -5.0).all() and (A == -5.0).all() and (b == -5.0).all() and (cnt == 77).all() and (obj == -5.0).all()
    assert np.array_equal(codes_io, B)


# ---- the Python mirrors check before the library is touched, and route by h ---------------------------------------------------------
def _args(n=6, d=4, m=2, h=300):
    rng = np.random.default_rng(2)
    B = rng.integers(1, h + 1, size=(n, m)).astype(np.int16)
    B[0, 0], B[0, 1] = h, 1                               # both ends of the one-based range
    return rng.standard_normal((n, d)).astype(np.float32), B


def test_python_argument_checks_run_before_the_library(rq, monkeypatch):
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd.LSQ import train_lsq_u16
    from rayuela_jl_amd.codebook_update import update_codebooks_u16
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    X, B = _args()
    big = np.ones((6, 16), np.int16)
    bad = [
        lambda: rq.update_codebooks(X, B + 1, 300),                                        # a code past h
        lambda: rq.update_codebooks(X, B - 1, 300),                                        # zero-based codes
        lambda: rq.update_codebooks(X, B, 32768),                                          # h past the Int16 limit
        lambda: rq.update_codebooks(X, big, 2048),                                         # m * h > 16384
        lambda: rq.update_codebooks(X, B[:5], 300),                                        # n mismatch
        lambda: rq.update_codebooks(X, B, 300, False, "lsqr"),                             # still fastbin only
        lambda: update_codebooks_u16(X, B, 300),                                           # one-based codes: 300 >= h
        lambda: update_codebooks_u16(X, B - 1, 300, rho=0.0),
        lambda: update_codebooks_u16(X, B - 1, 300, rho=float("nan")),
        lambda: rq.train_lsq(X, 2, 300, None, B.copy(), None, 1, 1, 1, True, 1),           # cpp=True keeps requiring h = 256
        lambda: rq.train_lsq(X, 2, 300, None, B.copy(), None, -1, 1, 1, True, 1, cpp=False),   # niter < 0
        lambda: rq.train_lsq(X, 2, 300, None, B.copy(), None, 1, 1, 1, True, 3, cpp=False),    # npert > m
        lambda: rq.train_lsq(X, 2, 300, None, B + 1, None, 1, 1, 1, True, 1, cpp=False),       # a code past h
        lambda: rq.train_lsq(X, 2, 32768, None, B.copy(), None, 1, 1, 1, True, 1, cpp=False),
        lambda: rq.train_lsq(X, 16, 2048, None, big, None, 1, 1, 1, True, 1, cpp=False),       # m * h > 16384
        lambda: rq.train_lsq(X, 2, 300, np.eye(3, dtype=np.float32), B.copy(), None, 1, 1, 1, True, 1, cpp=False),  # R shape
        lambda: rq.train_lsq_cuda(X, 2, 300, None, B, None, 1, 1, 1, True, 1, nsplits=0),
        lambda: train_lsq_u16(X, B - 1, 3, 300, None, 1, 1, 1, True, 1),                       # m mismatch
        lambda: train_lsq_u16(X, B, 2, 300, None, 1, 1, 1, True, 1),                           # one-based codes
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(TypeError):
        rq.train_lsq(X, 2, 300, None, B.astype(np.int32), None, 1, 1, 1, True, 1, cpp=False)
    # h > 256 passes every mirror's checks and reaches the (patched) library; so does the largest h of one codebook
    for f in (lambda: rq.update_codebooks(X, B, 300), lambda: update_codebooks_u16(X, B - 1, 300),
              lambda: rq.update_codebooks(X, B[:, :1], 16384),
              lambda: rq.train_lsq(X, 2, 300, None, B.copy(), None, 1, 1, 1, True, 1, cpp=False),
              lambda: rq.train_lsq_cuda(X, 2, 300, None, B, None, 1, 1, 1, True, 1),
              lambda: train_lsq_u16(X, B - 1, 2, 300, None, 1, 1, 1, True, 1)):
        with pytest.raises(AssertionError, match="library touched"):
            f()


def test_mirrors_route_by_h(rq, monkeypatch):
    """h <= 256 keeps the byte entries, h > 256 takes the wide ones; both see zero-based codes of their own width, and the
    caller gets one-based Int16 codes back (train_lsq also in B, train_lsq_cuda not)."""
    from rayuela_jl_amd import LSQ, codebook_update
    seen = []

    def fake_update(name, dtype):
        def fn(X, codes, h, rho=1e-4):
            assert codes.dtype == dtype and codes.min() == 0 and codes.max() == h - 1
            seen.append(name)
            return np.zeros((codes.shape[1], h, X.shape[1]), np.float32)
        return fn

    def fake_train(name, dtype):
        def fn(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, seed=0, nsplits=1):
            assert codes0.dtype == dtype and codes0.min() == 0 and codes0.max() == h - 1
            seen.append(name)
            return np.zeros((m, h, X.shape[1]), np.float32), np.array(codes0[::-1], dtype=dtype), np.zeros(niter)
        return fn
    monkeypatch.setattr(codebook_update, "update_codebooks_u8", fake_update("u8", np.uint8))
    monkeypatch.setattr(codebook_update, "update_codebooks_u16", fake_update("u16", np.int16))
    monkeypatch.setattr(LSQ, "train_lsq_u8", fake_train("t8", np.uint8))
    monkeypatch.setattr(LSQ, "train_lsq_u16", fake_train("t16", np.int16))
    for h, up, tr in ((256, "u8", "t8"), (257, "u16", "t16")):
        X, B = _args(h=h)
        C = rq.update_codebooks(X, B, h)
        assert len(C) == 2 and C[0].shape == (h, 4)
        keep = B.copy()
        Cn, Bn, obj = rq.train_lsq(X, 2, h, None, B, None, 2, 1, 1, True, 1, cpp=False, V=False)
        assert Bn.dtype == np.int16 and np.array_equal(Bn, keep[::-1]) and np.array_equal(B, Bn) and obj.dtype == np.float32
        B = keep.copy()
        Cn, Bn, obj = rq.train_lsq_cuda(X, 2, h, None, B, None, 2, 1, 1, True, 1)
        assert Bn.dtype == np.int16 and np.array_equal(Bn, keep[::-1]) and np.array_equal(B, keep)
        assert seen == [up, tr, tr]
        del seen[:]


# ---- the generated code -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lsq_asm(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("lsq_wide") / "rq_lsq.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                           "--cuda-device-only", os.path.join(ROOT, "rayuela.jl_amd", "csrc", "rq_lsq.hip"), "-o",
                           str(out)], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_wide_lsq_kernels_use_no_scratch(lsq_asm):
    """Every kernel of rq_lsq.hip the int16 path adds, by its metadata: no private segment, no VGPR spills -- read as
    tests/test_lsq_update_oracle.py reads the byte kernels -- and the file as a whole no scratch instruction and no float atomic."""
    metas = re.findall(r"\.name:\s+(\S+)(.*?)(?=\n\s+- \.|\n\s*\.end_amdgpu_metadata)", lsq_asm, flags=re.S)
    metas = [(n, meta) for n, meta in metas if "lsq_" in n]
    names = [n for n, _ in metas]
    # the sort trio per code type and pass, the pair counts per code type, the two kernels of the segment bounds
    for k, count in (("lsq_tile_hist_kernel", 3), ("lsq_scatter_kernel", 3), ("lsq_scan_kernel", 2), ("lsq_pair_kernel", 2),
                     ("lsq_code_hist_kernel", 1), ("lsq_segs_scan_kernel", 1)):
        assert sum(k in n for n in names) == count, (k, names)
    # Itanium mangling: `s` = short (int16_t), `h` = unsigned char; the int16 instantiations are there by type
    for k in ("lsq_tile_hist_kernelIsLi0E", "lsq_tile_hist_kernelIsLi1E", "lsq_scatter_kernelIsLi0E", "lsq_scatter_kernelIsLi1E",
              "lsq_pair_kernelIsE", "lsq_tile_hist_kernelIhLi0E", "lsq_scatter_kernelIhLi0E", "lsq_pair_kernelIhE"):
        assert any(k in n for n in names), (k, names)
    for name, meta in metas:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), name
    assert not re.search(r"^\s*scratch_|buffer_store_dword\s.*off(set)?.*s\[0:3\]", lsq_asm, flags=re.M)
    assert not re.search(r"^\s*(global|flat|buffer|ds)_atomic_(add|pk_add|min|max)_f(32|64)", lsq_asm, flags=re.M)
