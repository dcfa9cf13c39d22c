"""GPU: the non-finite contract of the PQ / OPQ encode at h <= 256, of the rotation and of the training loops built on them
(include/rayuela_hip.h, "Non-finite inputs").

Encode, every kernel the dispatch can choose (each case asserts rq_last_encode_kernel, so a silent re-dispatch cannot hide a
kernel), at the smallest shape that selects it and with one codebook size below 28 and one of 256 per family:
  1. the call returns RQ_OK and every code is below h (1 .. h in the one-based forms);
  2. rows are independent: a finite row has the oracle's codes, bit for bit, and the codes it has when the poisoned rows hold
     zeros instead;
  3. sub-quantizers are independent: a non-finite codeword of codebook i leaves every other column equal to the oracle's;
  4. a sub-vector that holds a NaN coordinate (every distance NaN) gets code 0 -- the oracle's answer.
The inputs are tests/nonfinite_encode_cases.py; tests/test_nonfinite_encode_ref.py holds the oracle to the same contract on
the CPU.  The ONLY cells excused from bit-equality with the oracle are the poisoned sub-vectors (their number is asserted)
and the poisoned codebook's column.  Decision per case, contract point 4's exception: sub-vectors with an Inf or a 3e38
coordinate (|x|^2 = +Inf; the inner products +-Inf or NaN by the codeword's sign) are held to "in range" only, in every
kernel -- the f32-MFMA kernels skip NaN distances where the oracle clamps them to 0, and pinning the cases where both happen
to agree would pin an accident of the codebook's signs.

Before this contract a lane whose 16 distances of the winning tile were all NaN answered position 27 + 4 hi of that tile
(rq_encode_split.h, argmin_finish): code 27 at h = 16, an index the RVQ epilogue, update_centers and the ERVQ increment
then used past their tables.  The h < 28 cases here are the ones that see it."""
import ctypes as C

import numpy as np
import pytest

import nonfinite_encode_cases as nc
import nonfinite_ref as nf
from switch_table import switches

pytestmark = pytest.mark.gpu

N = nc.N
_REF = {}


def _L():
    from rayuela_jl_amd import _lib
    return _lib


def _kernel():
    return (_L().lib().rq_last_encode_kernel() or b"").decode()


def _dev(a, offset4=False):
    """a on the device; offset4: at an address that is 4 bytes past a 16-byte boundary"""
    import torch
    a = np.array(a, order="C")               # a writable copy: the shared cases are read-only arrays
    if not offset4:
        return torch.from_numpy(a).cuda()
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = flat[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _encode(X, Ccat, m, h, offset4=False):
    """rq_dev_encode_pq into a buffer filled with 0xEE: an unwritten cell shows as 238"""
    import torch
    from rayuela_jl_amd import device as rqd
    out = torch.full((X.shape[0], m), 0xEE, dtype=torch.uint8, device="cuda")
    rqd.encode_pq(_dev(X, offset4), _dev(Ccat), m, h, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _oracle_bad(oracle, d, m, h):
    key = (d, m, h)
    if key not in _REF:
        c = nc.case(N, d, m, h)
        _REF[key] = oracle.encode_pq(c["Xbad"], c["Ccat"], m, h)
        _REF[key].setflags(write=False)
    return _REF[key]


def _check_codes(got, zero, ref, c, h, what):
    """contract points 1, 2 and 4 on one pair of runs (poisoned rows / the same rows zeroed) against the oracle's codes"""
    assert got.dtype == np.uint8 and int(got.max()) < h, (what, "code out of range", int(got.max()))
    assert int(zero.max()) < h, what
    changed = np.flatnonzero((got[c["clean"]] != zero[c["clean"]]).any(axis=1))
    assert changed.size == 0, (what, "%d finite rows changed their codes" % changed.size)
    ex = c["excused"]
    wrong = np.argwhere((got != ref) & ~ex)
    assert wrong.size == 0, (what, "%d finite cells differ from the oracle, first (row, i) = %s" % (len(wrong), wrong[:1]))
    assert (got[c["nan_cells"]] == 0).all(), (what, "NaN sub-vector without code 0", np.argwhere(c["nan_cells"] & (got != 0))[:3])


def _check_case(oracle, d, m, h, kernel, sw, offset4=False, rows=True, books=True):
    c = nc.case(N, d, m, h)
    assert int(c["excused"].sum()) == nc.excused_count(N, d, m)          # the excuse cannot grow
    what = (kernel, d, m, h, sw)
    with switches(**sw):
        if rows:
            got = _encode(c["Xbad"], c["Ccat"], m, h, offset4)
            assert _kernel() == kernel, (what, _kernel())
            zero = _encode(c["Xzero"], c["Ccat"], m, h, offset4)
            _check_codes(got, zero, _oracle_bad(oracle, d, m, h), c, h, what)
        for kind in nc.CODEWORD_POISONS if books else ():
            _, Ccat, i = nc.poisoned_codebooks(c, kind, d, m, h)
            got = _encode(c["X"], Ccat, m, h, offset4)
            assert _kernel() == kernel, (what, kind, _kernel())
            assert int(got.max()) < h, (what, kind, int(got.max()))
            other = np.arange(m) != i                                      # column i: in range, otherwise unspecified
            ref = oracle.encode_pq(c["X"], Ccat, m, h)
            assert np.array_equal(got[:, other], ref[:, other]), (what, kind, int((got[:, other] != ref[:, other]).sum()))


# ---- the shipped path: bf16 filter + exact pass (sub-space widths 6 packed, 8, 16, 2) -------------------------------------
@pytest.mark.parametrize("d,m,h,waves", [
    (24, 4, 16, 0), (24, 4, 256, 8),
    (32, 4, 16, 8), (32, 4, 27, 12), (32, 4, 28, 0), (32, 4, 33, 8), (32, 4, 256, 12),
    (64, 4, 16, 12), (64, 4, 27, 0), (64, 4, 256, 8),
    (16, 8, 16, 0), (16, 8, 33, 12), (16, 8, 256, 8),
])
def test_filter_kernel_and_exact_pass(oracle, d, m, h, waves):
    _check_case(oracle, d, m, h, "encode_pq_filter_kernel", dict(ENC_SPLIT_WAVES=waves))


@pytest.mark.parametrize("d,m,h,waves", [(24, 4, 17, 8), (24, 4, 256, 12), (64, 4, 17, 16), (64, 4, 256, 8)])
def test_one_pass_split_kernel(oracle, d, m, h, waves):
    _check_case(oracle, d, m, h, "encode_pq_split_kernel", dict(ENC_SPLIT=2, ENC_SPLIT_WAVES=waves))


@pytest.mark.parametrize("d,m,h,waves", [
    (32, 4, 16, 8), (32, 4, 27, 16), (32, 4, 64, 8), (32, 4, 256, 16),
    (96, 1, 16, 16), (96, 1, 256, 8),
    (128, 1, 27, 8), (128, 1, 64, 16),
])
def test_direct_kernel(oracle, d, m, h, waves):
    _check_case(oracle, d, m, h, "encode_pq_direct_kernel", dict(ENC_SPLIT=0, ENC_WAVES=waves))


@pytest.mark.parametrize("d,m,h,offset4", [(32, 4, 17, True), (32, 4, 33, True), (50, 7, 17, False), (50, 7, 33, False),
                                           (32, 4, 256, True)])
def test_lds_staged_kernel(oracle, d, m, h, offset4):
    """rows that are not 8-byte aligned, and an uneven split (widths 8, 7, 7, 7, 7, 7, 7)"""
    _check_case(oracle, d, m, h, "encode_pq_kernel", dict(ENC_SPLIT=0), offset4=offset4)


@pytest.mark.parametrize("d,m,h", [(131, 1, 17), (131, 1, 33), (240, 2, 17), (240, 2, 256)])
def test_wide_kernel(oracle, d, m, h):
    _check_case(oracle, d, m, h, "encode_wide_kernel", {})


@pytest.mark.parametrize("d,m,h", [(32, 4, 16), (32, 4, 256), (24, 4, 16), (24, 4, 256)])
def test_byte_filter_kernel(oracle, d, m, h):
    """Byte rows are finite: the codebook poisons, and a non-finite R (the call returns, the codes are in range)."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(d + h)
    Xb = rng.integers(0, 256, (N, d), dtype=np.uint8)
    Xf = Xb.astype(np.float32)
    w = d // m
    books = [(rng.standard_normal((h, w)) * 40 + 128).astype(np.float32) for _ in range(m)]
    for kind in nc.CODEWORD_POISONS:
        i, k, col, bits = nc.codeword_poison(kind, d, m, h)
        Cl = [b.copy() for b in books]
        nf.put_bits(Cl[i], (k, col), bits)
        Ccat = np.concatenate([b.reshape(-1) for b in Cl])
        out = torch.full((N, m), 0xEE, dtype=torch.uint8, device="cuda")
        rqd.encode_pq(torch.from_numpy(Xb).cuda(), _dev(Ccat), m, h, out=out)
        torch.cuda.synchronize()
        assert _kernel() == "encode_pq_filter_bytes_kernel", _kernel()
        got, ref = out.cpu().numpy(), oracle.encode_pq(Xf, Ccat, m, h)
        other = np.arange(m) != i
        assert int(got.max()) < h and np.array_equal(got[:, other], ref[:, other]), (kind, int(got.max()))
    Ccat = np.concatenate([b.reshape(-1) for b in books])
    for bits in (nf.NAN_POS, 0x7F800000):
        R = synth.rotation(d, seed=3).copy()
        nf.put_bits(R, (1, 2), bits)
        out = torch.full((N, m), 0xEE, dtype=torch.uint8, device="cuda")
        rqd.encode_opq(torch.from_numpy(Xb).cuda(), _dev(R), _dev(Ccat), m, h, out=out)
        torch.cuda.synchronize()
        assert int(out.max()) < h, (hex(bits), int(out.max()))


# ---- the host-pointer forms, once each, into pre-filled outputs ----------------------------------------------------------------
def test_host_forms_once_each(rq, oracle):
    import rayuela_jl_amd.synth as synth
    d, m, h = 32, 4, 16
    c = nc.case(N, d, m, h)
    L = _L()
    lib = L.lib()
    ref = _oracle_bad(oracle, d, m, h)
    R = synth.rotation(d, seed=11)
    ref_o = oracle.encode_opq(c["Xbad"], R, c["Ccat"], m, h)
    zero_o = oracle.encode_opq(c["Xzero"], R, c["Ccat"], m, h)
    assert np.array_equal(ref_o[c["clean"]], zero_o[c["clean"]])
    nan_rows = np.flatnonzero(c["nan_cells"].any(axis=1))                    # a NaN coordinate makes the whole rotated row NaN

    def check_pq(got, zero, what):
        _check_codes(got, zero, ref, c, h, what)

    def check_opq(got, what):
        assert int(got.max()) < h, (what, int(got.max()))
        assert np.array_equal(got[c["clean"]], ref_o[c["clean"]]), what
        assert (got[nan_rows] == 0).all(), what

    Xbad, Xzero, Ccat = c["Xbad"], c["Xzero"], c["Ccat"]
    u8 = lambda: np.full((N, m), 0xEE, dtype=np.uint8)                      # noqa: E731
    i16 = lambda: np.full((N, m), -7, dtype=np.int16)                       # noqa: E731
    a, b = u8(), u8()
    L.check(lib.rq_encode_pq(a.ctypes.data, Xbad.ctypes.data, Ccat.ctypes.data, N, d, m, h))
    assert _kernel() == "encode_pq_filter_kernel"
    L.check(lib.rq_encode_pq(b.ctypes.data, Xzero.ctypes.data, Ccat.ctypes.data, N, d, m, h))
    check_pq(a, b, "rq_encode_pq")
    a, b = i16(), i16()
    L.check(lib.rq_encode_pq_i16(a.ctypes.data, Xbad.ctypes.data, Ccat.ctypes.data, N, d, m, h))
    L.check(lib.rq_encode_pq_i16(b.ctypes.data, Xzero.ctypes.data, Ccat.ctypes.data, N, d, m, h))
    assert int(a.min()) >= 1 and int(a.max()) <= h and int(b.min()) >= 1
    check_pq((a - 1).astype(np.uint8), (b - 1).astype(np.uint8), "rq_encode_pq_i16")
    a = u8()
    L.check(lib.rq_encode_opq(a.ctypes.data, Xbad.ctypes.data, R.ctypes.data, Ccat.ctypes.data, N, d, m, h))
    check_opq(a, "rq_encode_opq")
    a = i16()
    L.check(lib.rq_encode_opq_i16(a.ctypes.data, Xbad.ctypes.data, R.ctypes.data, Ccat.ctypes.data, N, d, m, h))
    assert int(a.min()) >= 1 and int(a.max()) <= h
    check_opq((a - 1).astype(np.uint8), "rq_encode_opq_i16")
    ds = lib.rq_dataset_upload(Xbad.ctypes.data, N, d)
    assert ds, lib.rq_last_error()
    try:
        a, a1 = u8(), i16()
        L.check(lib.rq_dataset_encode(ds, a.ctypes.data, a1.ctypes.data, None, Ccat.ctypes.data, m, h))
        assert np.array_equal(a1, a.astype(np.int16) + 1)
        dz = lib.rq_dataset_upload(Xzero.ctypes.data, N, d)
        assert dz, lib.rq_last_error()
        try:
            b = u8()
            L.check(lib.rq_dataset_encode(dz, b.ctypes.data, None, None, Ccat.ctypes.data, m, h))
        finally:
            lib.rq_dataset_free(dz)
        check_pq(a, b, "rq_dataset_encode")
        a = u8()
        L.check(lib.rq_dataset_encode(ds, a.ctypes.data, None, R.ctypes.data, Ccat.ctypes.data, m, h))
        check_opq(a, "rq_dataset_encode + R")
    finally:
        lib.rq_dataset_free(ds)


# ---- rotation (contract point 5) and OPQ encode on top of it (point 6) ----------------------------------------------------------
NR = 1013


def _same_or_both_nan(got, ref, what):
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, "NaN pattern", np.argwhere(gn != rn)[:3])
    assert np.array_equal(got.view(np.uint32)[~rn], ref.view(np.uint32)[~rn]), (what, np.argwhere((got != ref) & ~rn)[:3])


@pytest.mark.parametrize("legacy", [False, True], ids=["default", "ROT_V2=0,ROT_WIDE2=0"])
@pytest.mark.parametrize("d", [10, 33, 96, 128, 130])
def test_rotation(rq, oracle, d, legacy):
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    c = nc.case(NR, d, 1, 16)
    R = synth.rotation(d, seed=d)
    ref = oracle.rotate_T(R, c["Xbad"])
    fin = oracle.rotate_T(R, c["X"])
    assert np.array_equal(ref[c["clean"]].view(np.uint32), fin[c["clean"]].view(np.uint32)) and np.isnan(ref).any() and np.isinf(ref).any()
    with switches(**(dict(ROT_V2=0, ROT_WIDE2=0) if legacy else {})):
        got = rqd.rotate_T(_dev(R), _dev(c["Xbad"]), out=torch.full((NR, d), 7.0, device="cuda")).cpu().numpy()
        _same_or_both_nan(got, ref, ("rq_dev_rotate_T", d))
        assert np.array_equal(got[c["clean"]].view(np.uint32), fin[c["clean"]].view(np.uint32))
        _same_or_both_nan(rq.rotate(R, c["Xbad"]), ref, ("rq_rotate_T", d))
        # a non-finite R: the calls return
        Rbad = R.copy()
        nf.put_bits(Rbad, (d - 1, 0), nf.NAN_NEG)
        nf.put_bits(Rbad, (0, d - 1), 0xFF800000)
        rq.rotate(Rbad, c["X"])
        rqd.rotate_T(_dev(Rbad), _dev(c["X"]))
        rqd.rotate_T(_dev(Rbad), torch.from_numpy(np.random.default_rng(d).integers(0, 256, (NR, d), dtype=np.uint8)).cuda())
        torch.cuda.synchronize()


@pytest.mark.parametrize("d,m,h", [(32, 4, 16), (96, 16, 256)])
def test_opq_encode(oracle, d, m, h):
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    c = nc.case(N, d, m, h)
    R = synth.rotation(d, seed=d + 1)
    ref = oracle.encode_opq(c["Xbad"], R, c["Ccat"], m, h)
    nan_rows = np.flatnonzero(c["nan_cells"].any(axis=1))
    bad_rows = np.flatnonzero(~c["clean"])
    assert len(bad_rows) == len(nc.row_poisons(N, d)) and (ref[nan_rows] == 0).all()
    Rd, Cd = _dev(R), _dev(c["Ccat"])

    def run(X):
        out = torch.full((N, m), 0xEE, dtype=torch.uint8, device="cuda")
        rqd.encode_opq(_dev(X), Rd, Cd, m, h, out=out)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    got, zero = run(c["Xbad"]), run(c["Xzero"])
    assert _kernel() == "encode_pq_filter_kernel", _kernel()
    assert int(got.max()) < h and int(zero.max()) < h, int(got.max())
    # a poisoned row is poisoned in every rotated coordinate: its m cells are the excused ones, m * 8 in all
    assert np.array_equal(got[c["clean"]], ref[c["clean"]]) and np.array_equal(got[c["clean"]], zero[c["clean"]])
    assert (got[nan_rows] == 0).all(), got[nan_rows]


# ---- training on a base with one non-finite row --------------------------------------------------------------------------------
NT = 3000
TRAIN_POISONS = {"nan": nf.NAN_POS, "pinf": 0x7F800000, "2e19": int(np.array([2e19], dtype=np.float32).view(np.uint32)[0])}
# rq_kmpp_seeds(seed = 5) on _train_base(16): the seeds of the parent commit on the finite base, recorded on an MI355X.  The
# seeding kernel's fallback decision moved into a register (rq_train.hip, kmpp_select_kernel); a finite base never takes it.
KMPP_SEEDS_D16_M2_H16 = [[2288, 2623, 1554, 849, 2373, 1200, 1808, 1346, 1571, 1288, 494, 1926, 2440, 2039, 2650, 185],
                         [244, 1494, 386, 881, 149, 1567, 2153, 133, 2993, 1797, 1770, 1202, 1335, 769, 1605, 1648]]


def _train_base(d):
    X = np.random.default_rng(40 + d).standard_normal((NT, d)).astype(np.float32)
    X.setflags(write=False)
    return X


def _poisoned_base(d, poison, avoid):
    """One row that is not a first seed: poisoned in coordinate 1 (and, for the magnitude 2e19, throughout: |x|^2 ~ 1e40)."""
    X = _train_base(d).copy()
    row = next(r for r in range(NT // 2, NT) if r not in avoid)
    if poison == "2e19":
        X[row] = 2e19
    else:
        nf.put_bits(X, (row, 1), TRAIN_POISONS[poison])
    return X, row


def _status(st):
    """True: RQ_OK.  False: a clean error -- one of the library's own negative codes with a message.  A positive status is a
    hipError_t (a fault on the device stays with the process, and two such calls would look "the same twice"): never clean."""
    msg = (_L().lib().rq_last_error() or b"").decode("utf-8", "replace")
    assert st <= 0, (st, msg)
    assert st == 0 or len(msg) > 0, st
    return st == 0


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrays]


@pytest.mark.parametrize("poison", list(TRAIN_POISONS))
def test_kmpp_seeds(rq, poison):
    d, m, h = 16, 2, 16
    seeds0, _ = rq.kmpp_seeds(_train_base(d), m, h, seed=5)
    assert seeds0.min() >= 0 and seeds0.max() < NT
    assert seeds0.tolist() == KMPP_SEEDS_D16_M2_H16
    X, row = _poisoned_base(d, poison, set(seeds0[:, 0].tolist()))
    lib = _L().lib()
    runs = []
    for _ in range(2):
        seeds = np.full((m, h), -99, dtype=np.int64)
        Ccat = np.zeros(h * d, dtype=np.float32)
        ok = _status(lib.rq_kmpp_seeds(seeds.ctypes.data, Ccat.ctypes.data, X.ctypes.data, NT, d, m, h, 5))
        if ok:
            assert seeds.min() >= 0 and seeds.max() < NT, (poison, seeds)
            assert np.array_equal(seeds[:, 0], seeds0[:, 0])                # the first seed is drawn before any cost exists
            # the seed sub-vectors are the rows the seeds name
            w = d // m
            for i in range(m):
                assert np.array_equal(Ccat[i * h * w:(i + 1) * h * w].reshape(h, w).view(np.uint32),
                                      X[seeds[i], i * w:(i + 1) * w].view(np.uint32)), (poison, i)
        runs.append((ok, _bits(seeds, Ccat)))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), poison


@pytest.mark.parametrize("poison", list(TRAIN_POISONS))
@pytest.mark.parametrize("d,m,h", [(32, 4, 16), (30, 5, 17)])
def test_train_pq(rq, d, m, h, poison):
    seeds0, _ = rq.kmpp_seeds(_train_base(d), m, h, seed=5)
    X, _ = _poisoned_base(d, poison, set(seeds0[:, 0].tolist()))
    lib = _L().lib()
    runs = []
    for _ in range(2):
        Ccat = np.zeros(h * d, dtype=np.float32)
        B = np.full((NT, m), -7, dtype=np.int16)
        err = C.c_double(0.0)
        ok = _status(lib.rq_train_pq(Ccat.ctypes.data, B.ctypes.data, C.cast(C.byref(err), C.c_void_p), X.ctypes.data, NT, d, m, h, 3, 5))
        if ok:
            assert int(B.min()) >= 1 and int(B.max()) <= h, (poison, int(B.min()), int(B.max()))
        runs.append((ok, _bits(Ccat, B, np.array([err.value]))))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), poison


def test_train_pq_with_an_odd_number_of_counters(rq):
    """Finite data at m * h = 85: the Lloyd loop keeps a 64-bit change counter behind its m * h 32-bit cluster counts and
    adds to it atomically; with m * h odd it sat 4 bytes off an 8-byte boundary and the first iteration that changed a code
    faulted (found by test_train_pq[30-5-17-*])."""
    X = _train_base(30)
    a = rq.train_pq(X, 5, 17, niter=4, seed=5)
    b = rq.train_pq(X, 5, 17, niter=4, seed=5)
    assert np.array_equal(a[1], rq.quantize_pq(X, a[0])) and int(a[1].min()) >= 1 and int(a[1].max()) <= 17
    assert np.array_equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[2] == b[2]
    assert np.isfinite(a[2]) and a[2] < float((X.astype(np.float64) ** 2).sum(axis=1).mean())


@pytest.mark.parametrize("poison", list(TRAIN_POISONS))
def test_train_rvq_then_ervq(rq, poison):
    d, m, h = 24, 3, 16
    seeds0, _ = rq.kmpp_seeds(_train_base(d), 1, h, seed=5)
    X, _ = _poisoned_base(d, poison, set(seeds0[:, 0].tolist()))
    lib = _L().lib()
    runs = []
    for _ in range(2):
        Cs = np.zeros((m, h, d), dtype=np.float32)
        B = np.full((NT, m), -7, dtype=np.int16)
        err = C.c_double(0.0)
        ok = _status(lib.rq_train_rvq(Cs.ctypes.data, B.ctypes.data, C.cast(C.byref(err), C.c_void_p), X.ctypes.data, NT, d, m, h, 3, 5))
        out = [Cs, B, np.array([err.value])]
        if ok:
            assert int(B.min()) >= 1 and int(B.max()) <= h, (poison, int(B.min()), int(B.max()))
            # the stage counts of an encode with the trained (possibly non-finite) codebooks: every row once per stage
            codes, counts, _ = rq.quantize_rvq_u8(X, [Cs[i] for i in range(m)], with_extras=True)
            assert int(codes.max()) < h and (counts.sum(axis=1) == NT).all(), (poison, counts.sum(axis=1))
            # ERVQ from that state (the increment indexes the codebooks by these codes)
            C2, B2 = Cs.copy(), B.copy()
            obj = np.zeros(2 * m + 1, dtype=np.float64)
            err2 = C.c_double(0.0)
            ok2 = _status(lib.rq_train_ervq(C2.ctypes.data, B2.ctypes.data, C.cast(C.byref(err2), C.c_void_p), obj.ctypes.data,
                                            X.ctypes.data, NT, d, m, h, 2, 5))
            if ok2:
                assert int(B2.min()) >= 1 and int(B2.max()) <= h, (poison, int(B2.min()), int(B2.max()))
            # one codebook update alone, with in-range codes
            C3 = Cs.copy()
            cnt = np.zeros(h, dtype=np.uint32)
            u8 = np.ascontiguousarray((B - 1).astype(np.uint8))
            if _status(lib.rq_ervq_update_codebook(C3.ctypes.data, cnt.ctypes.data, X.ctypes.data, u8.ctypes.data, NT, d, m, h, 1)):
                assert int(cnt.sum()) == NT and np.array_equal(cnt, np.bincount(u8[:, 1], minlength=h)), poison
            out += [np.array([ok2]), C2, B2, obj, C3, cnt]
        runs.append((ok, _bits(*out)))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), poison


@pytest.mark.parametrize("poison", list(TRAIN_POISONS))
@pytest.mark.parametrize("given", [False, True], ids=["natural", "R0-C0"])
def test_train_opq(rq, poison, given):
    import rayuela_jl_amd.synth as synth
    d, m, h = 32, 4, 16
    seeds0, C0 = rq.kmpp_seeds(_train_base(d), m, h, seed=5)
    X, _ = _poisoned_base(d, poison, set(seeds0[:, 0].tolist()))
    R0 = synth.rotation(d, seed=9) if given else None
    c0 = np.concatenate([c.reshape(-1) for c in C0]) if given else None
    lib = _L().lib()
    runs = []
    for _ in range(2):
        Ccat = np.zeros(h * d, dtype=np.float32)
        B = np.full((NT, m), -7, dtype=np.int16)
        R = np.zeros((d, d), dtype=np.float32)
        obj = np.zeros(4, dtype=np.float32)
        ok = _status(lib.rq_train_opq(Ccat.ctypes.data, B.ctypes.data, R.ctypes.data, obj.ctypes.data, X.ctypes.data, NT, d, m, h, 3,
                                      0, 5, None if R0 is None else R0.ctypes.data, None if c0 is None else c0.ctypes.data))
        if ok:
            assert int(B.min()) >= 1 and int(B.max()) <= h, (poison, int(B.min()), int(B.max()))
        runs.append((ok, _bits(Ccat, B, R, obj)))
    assert runs[0][0] == runs[1][0] and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), poison
