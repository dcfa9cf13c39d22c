"""GPU: the non-finite contract of training (include/rayuela_hip.h, "Non-finite inputs of training") at
h > 256 and for LSQ / chain / SR; inputs and restatements in tests/nonfinite_train_cases.py, which
tests/test_nonfinite_train_ref.py holds to the existing oracles on the CPU.

A. Reductions: a poisoned coordinate (row r, column c) stays in column c.
   rq_dev_update_centers / _wide   counts exact; every column != c bit-equal to the exact restatement; codes without rows keep
                                   their start bits in every column; the same bits twice (uint32: NaN payloads included).  Column
                                   c is unspecified.  centers_mfma_kernel was read for this (rq_train.hip): a one-hot product
                                   meets 0 x NaN in every code of column c and in no other column, and the ones-column that counts
                                   never sees X -- the code agrees with both points.  That NaN pattern is what shows WHICH kernel
                                   ran (the library names no centre kernel): under the default a NaN / Inf poison reaches codes
                                   other than its row's; under TRAIN_CENTERS_MFMA = 0 (owner threads, byte kernel) every cell but
                                   (code of row r, column c) is the restatement's.  At h > 256 the counts of codes past 255 are
                                   the byte kernel's impossibility.
   rq_dev_reconstruct_wide         the gather bit for bit with NaN, +-Inf and denormal entries in C; zeros for out-of-range codes.
   Excused: the poisoned column(s) -- h cells per column, asserted from the poison table; 1 / d of C, which is what a column is
   (below 1 % only at d > 100; the training cases below excuse one row of 3000).
B. Training loops on a base with one poisoned row: status 0 or a negative code with a message, never a hipError_t; codes in
   range; the same bits twice; a finite run of the same shape right afterwards gives its known-good bits.
Every buffer a poisoned code could index is the test's own, with guard words around counts and centres."""
import ctypes as C

import numpy as np
import pytest

import kmeans_oracle as ko
import nonfinite_ref as nf
import nonfinite_train_cases as tc
import train_wide_oracle as two
import wide_oracle as wo
from switch_table import switches

pytestmark = pytest.mark.gpu

GUARD = 64                                  # words before and behind every guarded buffer
GUARD_F, GUARD_I = -7.0, -3
_MEANS = {}


def _L():
    from rayuela_jl_amd import _lib
    return _lib


def _status(st):
    """True: RQ_OK.  False: one of the library's negative codes with a message.  A positive status is a hipError_t: never clean."""
    msg = (_L().lib().rq_last_error() or b"").decode("utf-8", "replace")
    assert st <= 0, (st, msg)
    assert st == 0 or len(msg) > 0, st
    return st == 0


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrays]


def _same_twice(runs, what):
    assert runs[0][0] == runs[1][0], what
    assert len(runs[0][1]) == len(runs[1][1]) and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1])), what


def _guarded(values, dtype, fill):
    """(whole, inner): a device buffer with GUARD words of `fill` on both sides of a copy of `values`."""
    import torch
    v = torch.from_numpy(np.ascontiguousarray(values)).to(dtype).reshape(-1)
    whole = torch.full((v.numel() + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    inner = whole[GUARD:GUARD + v.numel()]
    inner.copy_(v)
    return whole, inner


def _guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def _update(X, codes, C0, m, h, wide):
    """(C list, counts (m, h) int64) of rq_dev_update_centers[_wide] between guard words; counts start from a sentinel."""
    import torch
    n, d = X.shape
    Cw, Ci = _guarded(two.cat(C0), torch.float32, GUARD_F)
    cw, ci = _guarded(np.full(m * h, 12345, np.int32), torch.int32, GUARD_I)
    dX = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    dcodes = torch.from_numpy(np.ascontiguousarray(codes.astype(np.int16 if wide else np.uint8))).cuda()
    lib = _L().lib()
    f = lib.rq_dev_update_centers_wide if wide else lib.rq_dev_update_centers
    st = f(Ci.data_ptr(), ci.data_ptr(), dX.data_ptr(), dcodes.data_ptr(), n, d, m, h, None)
    torch.cuda.synchronize()
    assert st == 0, (st, lib.rq_last_error())
    assert _guards_intact(Cw, GUARD_F) and _guards_intact(cw, GUARD_I)
    return wo.sub_codebooks(Ci.cpu().numpy(), d, m, h)[0], ci.cpu().numpy().astype(np.int64).reshape(m, h)


def _clean_means(shape):
    if shape not in _MEANS:
        n, d, m, h = shape
        c = tc.centre_case(n, d, m, h)
        _MEANS[shape] = two.exact_means(c["X"], c["C0"], c["codes"], m, h)
    return _MEANS[shape]


def _check_centres(shape, wide, owner_threads):
    n, d, m, h = shape
    c = tc.centre_case(n, d, m, h)
    off, sub = c["off"], tc.sub_of(d, m)
    want, cnt = _clean_means(shape)                  # == tc.means outside the poisoned columns (tests/test_nonfinite_train_ref.py)
    assert np.array_equal(cnt, np.stack([np.bincount(c["codes"][:, i], minlength=h) for i in range(m)]))
    spread = 0
    for case in tc.poison_table(n, d, m):
        keep = tc.keep_mask(case, d)
        assert tc.excused_cells(case, d, m, h) == h * int((~keep).sum()) == h * len(case)          # the excuse cannot grow
        Xbad = tc.poisoned(c["X"], case)
        got, gcnt = _update(Xbad, c["codes"], c["C0"], m, h, wide)
        assert np.array_equal(gcnt, cnt), case                                                     # the poisoned row is counted
        for i in range(m):
            k = keep[off[i]:off[i + 1]]
            bad = np.argwhere(got[i][:, k].view(np.uint32) != want[i][:, k].view(np.uint32))
            assert bad.size == 0, (case, i, "%d cells outside the poisoned column differ" % len(bad), bad[:3])
            empty = cnt[i] == 0
            assert empty.sum() >= 2
            assert np.array_equal(got[i][empty].view(np.uint32), c["C0"][i][empty].view(np.uint32)), (case, i)
        again, acnt = _update(Xbad, c["codes"], c["C0"], m, h, wide)
        assert two.same_bits(again, got) and np.array_equal(acnt, gcnt), case
        for r, col, kind in case:
            i, s = int(sub[col]), col - off[int(sub[col])]
            own = int(c["codes"][r, i])
            others = (np.arange(h) != own) & (cnt[i] > 0)
            if owner_threads:                        # the scatter: ONE cell may differ from the restatement
                assert np.array_equal(got[i][others, s].view(np.uint32), want[i][others, s].view(np.uint32)), \
                    (case, "not the owner-thread kernel")
            elif kind != "3e38":                     # the one-hot product: 0 x NaN in the other codes of the column
                assert np.isnan(got[i][others, s]).any(), (case, "not the matrix-core kernel")
                spread += 1
    return spread


@pytest.mark.parametrize("shape", tc.SHAPES_WIDE)
def test_update_centers_wide_keeps_a_poison_in_its_column(rq, shape):
    n, d, m, h = shape
    c = tc.centre_case(n, d, m, h)
    assert (c["codes"] >= 256).any() and _clean_means(shape)[1][:, 256:].sum() > 0      # counts past 255: centers_mfma_kernel<., int16_t>
    assert _check_centres(shape, True, False) >= 6


@pytest.mark.parametrize("mfma", [1, 0], ids=["mfma", "owner-threads"])
@pytest.mark.parametrize("shape", tc.SHAPES_BYTE)
def test_update_centers_keeps_a_poison_in_its_column(rq, shape, mfma):
    with switches(TRAIN_CENTERS_MFMA=mfma):
        spread = _check_centres(shape, False, mfma == 0)
    assert spread == (0 if mfma == 0 else 8)          # six single NaN / Inf poisons and the two of the double case


@pytest.mark.parametrize("shape", tc.SHAPES_WIDE + tc.SHAPES_BYTE[:1])
def test_reconstruct_wide_copies_non_finite_codewords(rq, shape):
    import torch
    n, d, m, h = shape
    c = tc.centre_case(n, d, m, h)
    Cbad, cells = tc.poisoned_codebooks(c["C0"], d, m, h)
    codes = np.array(c["codes"]).astype(np.int16)
    for j, (i, k, s) in enumerate(cells):
        codes[100 + j, i] = k                        # every poisoned entry is gathered at least once
    bad_rows = np.arange(1, n, 7)                    # out-of-range codes, also in the rows and sub-spaces next to a poisoned codeword
    last = cells[2][0]
    codes[bad_rows, last] = np.array([-1, h, 32767], dtype=np.int16)[np.arange(bad_rows.size) % 3]
    want = two.reconstruct(Cbad, np.where((codes < 0) | (codes >= h), 0, codes), c["off"], d)
    want[bad_rows, c["off"][last]:c["off"][last + 1]] = 0.0
    assert np.isnan(want).any() and np.isinf(want).any()
    whole, inner = _guarded(np.full(n * d, 3.0, np.float32), torch.float32, GUARD_F)
    dcodes, dC = torch.from_numpy(codes).cuda(), torch.from_numpy(two.cat(Cbad)).cuda()
    st = _L().lib().rq_dev_reconstruct_wide(inner.data_ptr(), dcodes.data_ptr(), dC.data_ptr(), n, d, m, h, None)
    torch.cuda.synchronize()
    assert st == 0 and _guards_intact(whole, GUARD_F)
    got = inner.cpu().numpy().reshape(n, d)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:3]


# ---- B.1 the wide training loops on a base with one poisoned row -----------------------------------------------------------------
def _pq_wide(X, m, h, base, niter=3):
    n, d = X.shape
    Ccat, B, err = np.zeros(h * d, np.float32), np.full((n, m), -7, np.int16), C.c_double(0.0)
    st = _L().lib().rq_train_pq_wide(Ccat.ctypes.data, B.ctypes.data, C.cast(C.byref(err), C.c_void_p), X.ctypes.data, n, d, m, h,
                                     niter, tc.TRAIN_SEED, base)
    return st, [Ccat, B, np.array([err.value])]


def _rvq_wide(X, m, h, base, niter=3):
    n, d = X.shape
    Cs, B, err = np.zeros((m, h, d), np.float32), np.full((n, m), -7, np.int16), C.c_double(0.0)
    st = _L().lib().rq_train_rvq_wide(Cs.ctypes.data, B.ctypes.data, C.cast(C.byref(err), C.c_void_p), X.ctypes.data, n, d, m, h,
                                      niter, tc.TRAIN_SEED, base)
    return st, [Cs, B, np.array([err.value])]


def _opq_wide(X, m, h, base, R0=None, C0=None, niter=3):
    n, d = X.shape
    Ccat, B = np.zeros(h * d, np.float32), np.full((n, m), -7, np.int16)
    R, obj = np.zeros((d, d), np.float32), np.zeros(niter + 1, np.float32)
    st = _L().lib().rq_train_opq_wide(Ccat.ctypes.data, B.ctypes.data, R.ctypes.data, obj.ctypes.data, X.ctypes.data, n, d, m, h, niter,
                                      0, tc.TRAIN_SEED, None if R0 is None else R0.ctypes.data, None if C0 is None else C0.ctypes.data,
                                      base)
    return st, [Ccat, B, R, obj]


def _in_range(B, h, base, what):
    assert B.dtype == np.int16 and int(B.min()) >= base and int(B.max()) <= h - 1 + base < 32767, (what, int(B.min()), int(B.max()))


def _reductions_on_returned_codes(X, Ccat, codes0, m, h, what):
    """rq_dev_update_centers_wide and rq_dev_reconstruct_wide with the codes a poisoned training run returned (zero-based)."""
    import torch
    n, d = X.shape
    start = wo.sub_codebooks(np.full(h * d, 2.0, np.float32), d, m, h)[0]
    _, cnt = _update(X, codes0, start, m, h, True)
    assert np.array_equal(cnt, np.stack([np.bincount(codes0[:, i], minlength=h) for i in range(m)])), what
    assert (cnt.sum(axis=1) == n).all(), what
    whole, inner = _guarded(np.zeros(n * d, np.float32), torch.float32, GUARD_F)
    dcodes, dC = torch.from_numpy(np.ascontiguousarray(codes0)).cuda(), torch.from_numpy(Ccat).cuda()
    assert _L().lib().rq_dev_reconstruct_wide(inner.data_ptr(), dcodes.data_ptr(), dC.data_ptr(), n, d, m, h, None) == 0
    torch.cuda.synchronize()
    assert _guards_intact(whole, GUARD_F)
    Cl, off = wo.sub_codebooks(Ccat, d, m, h)
    assert np.array_equal(inner.cpu().numpy().reshape(n, d).view(np.uint32), two.reconstruct(Cl, codes0, off, d).view(np.uint32)), what


PQ_SHAPES = [(32, 4, 300), (30, 5, 257)]           # m * h = 1285 is odd: the counter alignment at 16-bit width
_GOOD = {}


def _known_good(key, run):
    """The finite run of a shape, made once before any poisoned run of it: (status, bits)."""
    if key not in _GOOD:
        st, out = run()
        assert st == 0
        _GOOD[key] = _bits(*out)
    return _GOOD[key]


@pytest.mark.parametrize("poison", list(tc.TRAIN_POISONS))
@pytest.mark.parametrize("d,m,h", PQ_SHAPES)
def test_train_pq_wide(rq, d, m, h, poison):
    X, row = tc.poisoned_base(d, m, h, poison)
    Xf = tc.train_base(d)
    for base in (0, 1):
        good = _known_good(("pq", d, m, h, base), lambda: _pq_wide(Xf, m, h, base))
        runs = []
        for _ in range(2):
            st, out = _pq_wide(X, m, h, base)
            ok = _status(st)
            if ok:
                _in_range(out[1], h, base, (poison, base))
            runs.append((ok, _bits(*out)))
        _same_twice(runs, (poison, base))
        print("train_pq_wide d=%d m=%d h=%d %s base %d: RQ_OK %s" % (d, m, h, poison, base, runs[0][0]))
        if runs[0][0]:
            Ccat, B = out[0], out[1]
            _reductions_on_returned_codes(X, Ccat, B - base, m, h, (poison, base))
            Bq = rq.quantize_pq(X, wo.sub_codebooks(Ccat, d, m, h)[0])               # centres that may be non-finite
            _in_range(Bq, h, 1, (poison, "quantize_pq"))
        st, out = _pq_wide(Xf, m, h, base)                                           # no device state was left behind
        assert st == 0 and all(np.array_equal(a, b) for a, b in zip(_bits(*out), good)), (poison, base)


@pytest.mark.parametrize("poison", list(tc.TRAIN_POISONS))
def test_train_pq_wide_at_256_codewords_is_the_byte_loop(rq, poison):
    d, m, h = 32, 4, 256
    X, _ = tc.poisoned_base(d, m, h, poison)
    n = X.shape[0]
    runs = []
    for wide in (False, True):
        if wide:
            st, out = _pq_wide(X, m, h, 1)
        else:
            Ccat, B, err = np.zeros(h * d, np.float32), np.full((n, m), -7, np.int16), C.c_double(0.0)
            st = _L().lib().rq_train_pq(Ccat.ctypes.data, B.ctypes.data, C.cast(C.byref(err), C.c_void_p), X.ctypes.data, n, d, m, h,
                                        3, tc.TRAIN_SEED)
            out = [Ccat, B, np.array([err.value])]
        ok = _status(st)
        if ok:
            _in_range(out[1], h, 1, poison)
        runs.append((ok, _bits(*out)))
    _same_twice(runs, poison)                                                        # the widening adds nothing


@pytest.mark.parametrize("poison", list(tc.TRAIN_POISONS))
@pytest.mark.parametrize("given", [False, True], ids=["natural", "R0-C0"])
@pytest.mark.parametrize("d,m,h", PQ_SHAPES)
def test_train_opq_wide(rq, d, m, h, given, poison):
    import rayuela_jl_amd.synth as synth
    X, _ = tc.poisoned_base(d, m, h, poison)
    Xf = tc.train_base(d)
    R0 = synth.rotation(d, seed=9) if given else None
    off = wo.splitarray(d, m)
    rows = np.random.default_rng(h).permutation(tc.NT // 2)[:h]                     # distinct finite rows as start centres
    C0 = two.cat([Xf[rows, off[i]:off[i + 1]] for i in range(m)]) if given else None
    for base in (0, 1):
        good = _known_good(("opq", d, m, h, base, given), lambda: _opq_wide(Xf, m, h, base, R0, C0))
        runs = []
        for _ in range(2):
            st, out = _opq_wide(X, m, h, base, R0, C0)
            ok = _status(st)
            if ok:
                _in_range(out[1], h, base, (poison, base))
                assert out[3].shape == (4,)
            runs.append((ok, _bits(*out)))
        _same_twice(runs, (poison, base))
        print("train_opq_wide d=%d m=%d h=%d %s base %d: RQ_OK %s" % (d, m, h, poison, base, runs[0][0]))
        if runs[0][0]:
            _reductions_on_returned_codes(X, out[0], out[1] - base, m, h, (poison, base))
            Bq = rq.quantize_opq(X, out[2], wo.sub_codebooks(out[0], d, m, h)[0])     # R and centres that may be non-finite
            _in_range(Bq, h, 1, (poison, "quantize_opq"))
        st, out = _opq_wide(Xf, m, h, base, R0, C0)
        assert st == 0 and all(np.array_equal(a, b) for a, b in zip(_bits(*out), good)), (poison, base)


@pytest.mark.parametrize("poison", list(tc.TRAIN_POISONS))
def test_train_rvq_wide(rq, poison):
    d, m, h = 24, 3, 300
    X, _ = tc.poisoned_base(d, m, h, poison)
    Xf = tc.train_base(d)
    n = X.shape[0]
    for base in (0, 1):
        good = _known_good(("rvq", d, m, h, base), lambda: _rvq_wide(Xf, m, h, base))
        runs = []
        for _ in range(2):
            st, out = _rvq_wide(X, m, h, base)
            ok = _status(st)
            extra = []
            if ok:
                _in_range(out[1], h, base, (poison, base))
                # an encode with the trained (possibly non-finite) codebooks: in range, every row once per stage
                codes, counts, _ = rq.quantize_rvq_u16(X, [out[0][i] for i in range(m)], with_extras=True)
                assert int(codes.max()) < h and (counts.sum(axis=1) == n).all(), (poison, counts.sum(axis=1))
                assert np.array_equal(counts, np.stack([np.bincount(codes[:, i], minlength=h) for i in range(m)]))
                extra = [codes, counts]
            runs.append((ok, _bits(*(out + extra))))
        _same_twice(runs, (poison, base))
        print("train_rvq_wide %s base %d: RQ_OK %s" % (poison, base, runs[0][0]))
        if runs[0][0]:                       # the stage codes as PQ codes of width d / m: the centre update counts every row once
            _reductions_on_returned_codes(X, out[0][0].reshape(-1), out[1] - base, m, h, (poison, base))
        st, out = _rvq_wide(Xf, m, h, base)
        assert st == 0 and all(np.array_equal(a, b) for a, b in zip(_bits(*out), good)), (poison, base)


def test_train_pq_wide_with_an_odd_number_of_counters(rq):
    """Finite data at m * h = 1285 through the 16-bit loop: the 64-bit change counter behind m * h 32-bit counts must sit on an
    8-byte boundary here as in the byte loop (test_train_pq_with_an_odd_number_of_counters)."""
    X = tc.train_base(30)
    a = rq.train_pq(X, 5, 257, niter=4, seed=5)
    b = rq.train_pq(X, 5, 257, niter=4, seed=5)
    assert np.array_equal(a[1], rq.quantize_pq(X, a[0])) and int(a[1].min()) >= 1 and int(a[1].max()) <= 257
    assert np.array_equal(a[1], b[1]) and two.same_bits(a[0], b[0]) and a[2] == b[2]
    assert np.isfinite(a[2]) and a[2] < float((X.astype(np.float64) ** 2).sum(axis=1).mean())


# ---- B.2 the mass refill by itself ------------------------------------------------------------------------------------------------
def test_mass_refill_walk(rq, oracle):
    """Finite data first: 285 of 300 centres empty in iteration 1 and are re-drawn, by cost and then uniformly; every step of
    the library equals the restatement bit for bit (train_wide_oracle.telescope) and the figures are those the CPU test derives.
    Then the same walk with one NaN row: it returns, in range, the same bits twice."""
    from test_nonfinite_train_ref import REFILL_WALK
    X, m, h, seed = tc.refill_fixture()
    stats = two.new_stats()
    with switches(TRAIN_KMPP=0):
        rows, rng = two.start_rows(X, m, h, seed, ko.SALT_PQ, False)

        def train(k):
            Cl, B, _ = rq.train_pq(X, m, h, niter=k, seed=seed)
            return Cl, B

        K, C_K, B_K = two.telescope(train, rq.quantize_pq, oracle, X, m, h, rng, rows, stats)
        empty1 = int((np.bincount(train(0)[1][:, 0] - 1, minlength=h) == 0).sum())
        assert (K, stats["cost"], stats["uniform"], stats["wide"], empty1) == REFILL_WALK, (K, stats, empty1)
        Xn = tc.refill_fixture_nan()
        n, d = Xn.shape
        runs = []
        for _ in range(2):
            Ccat, B, err = np.zeros(h * d, np.float32), np.full((n, m), -7, np.int16), C.c_double(0.0)
            st = _L().lib().rq_train_pq_wide(Ccat.ctypes.data, B.ctypes.data, C.cast(C.byref(err), C.c_void_p), Xn.ctypes.data, n, d,
                                             m, h, K + 1, seed, 1)
            ok = _status(st)
            if ok:
                _in_range(B, h, 1, "nan row")
            runs.append((ok, _bits(Ccat, B, np.array([err.value]))))
        _same_twice(runs, "nan row")
        again = train(K)
        assert two.same_bits(again[0], C_K) and np.array_equal(again[1], B_K)


# ---- B.4 the wide encode, the assignment step of those loops ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tc.WIDE_ENCODE_SHAPES)
def test_wide_encode_non_finite_rows_and_codewords(rq, oracle, shape):
    import torch
    from rayuela_jl_amd import device
    n, d, m, h = shape
    X, Ccat = tc.wide_encode_case(n, d, m, h)
    ref = wo.encode_pq_wide(oracle, X, Ccat, m, h)
    got = device.encode_pq_wide(torch.from_numpy(X).cuda(), torch.from_numpy(Ccat).cuda(), m, h)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert (_L().lib().rq_last_encode_kernel() or b"").decode() == "encode_h16_kernel"
    assert got.min() >= 0 and got.max() < h
    assert np.array_equal(got, ref), "rows differ: %d of %d" % (int((got != ref).any(axis=1).sum()), n)
    out = np.full((n, m), -7, np.int16)
    assert _L().lib().rq_encode_pq_wide(out.ctypes.data, X.ctypes.data, Ccat.ctypes.data, n, d, m, h, 0) == 0
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("h", [257, 300])
def test_wide_rvq_encode_non_finite_rows_and_codewords(rq, oracle, h):
    """rq_dev_encode_rvq_wide with counts into guarded buffers: codes, counts and the residual of the finite rows are the
    restatement's (tests/wide_oracle.py::encode_rvq_wide, the oracle's own chains stage by stage)."""
    import torch
    import rayuela_jl_amd.synth as synth
    n, d, m = 1000, 24, 3
    X = np.array(synth.sift_like(n, d, seed=h))
    rng = np.random.default_rng(h)
    Cs = np.stack([X[rng.integers(0, n, h)] / (2.0 ** i) for i in range(m)]).astype(np.float32)
    X[3, 5] = np.nan
    X[10, 0] = np.inf
    X[20, d - 1] = -np.inf
    X[n - 1, 17] = np.nan
    Cs[1, h - 1, 2] = np.inf                          # h = 257: the one live codeword of the last block
    ref, rcounts, rres = wo.encode_rvq_wide(oracle, X, Cs)
    assert ref.max() < h and (rcounts.sum(axis=1) == n).all()
    cw, ci = _guarded(np.zeros(m * h, np.int32), torch.int32, GUARD_I)
    codes = torch.full((n, m), -7, dtype=torch.int16, device="cuda")
    dC = torch.from_numpy(Cs).cuda()
    Xw, Xr = _guarded(X.reshape(-1), torch.float32, GUARD_F)              # X on entry, the final residual on return
    st = _L().lib().rq_dev_encode_rvq_wide(codes.data_ptr(), Xr.data_ptr(), dC.data_ptr(), n, d, m, h, ci.data_ptr(), None)
    torch.cuda.synchronize()
    assert _guards_intact(Xw, GUARD_F)
    assert st == 0 and _guards_intact(cw, GUARD_I)
    got = codes.cpu().numpy()
    assert got.min() >= 0 and got.max() < h
    assert np.array_equal(got, ref), "rows differ: %d of %d" % (int((got != ref).any(axis=1).sum()), n)
    assert np.array_equal(ci.cpu().numpy().reshape(m, h).astype(np.int64), rcounts.astype(np.int64))
    fin = np.isfinite(rres).all(axis=1)
    assert fin.sum() > n // 4
    assert np.array_equal(Xr.cpu().numpy().reshape(n, d)[fin].view(np.uint32), rres[fin].view(np.uint32))


# ---- A.3 rq_dev_lsq_normal_eq -----------------------------------------------------------------------------------------------------
def _dev_f32(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


@pytest.mark.parametrize("m,h", tc.LSQ_SHAPES)
def test_lsq_normal_equations(rq, m, h):
    """A is bit-equal to the restatement (it depends on the codes alone); b equals the restatement's f64 sums on the poisoned
    rows at EVERY entry: NaN where it is NaN, the same bits elsewhere -- b is a segmented sum, so even inside column c only the
    m cells of the poisoned row's codes are touched (tests/test_nonfinite_train_ref.py counts them)."""
    import torch
    import lsq_update_oracle as lo
    X, codes = tc.lsq_case(m, h)
    n, d = X.shape
    mh = m * h
    dcodes = torch.from_numpy(np.array(codes)).cuda()
    for case in tc.lsq_poisons(d, m):
        Xbad = tc.poisoned(X, case)
        with np.errstate(all="ignore"):
            A0, b0 = lo.normal_eq(Xbad, codes, h)
        Aw, A = _guarded(np.zeros(mh * mh), torch.float64, GUARD_F)
        bw, b = _guarded(np.zeros(mh * d), torch.float64, GUARD_F)
        st = _L().lib().rq_dev_lsq_normal_eq(A.data_ptr(), b.data_ptr(), _dev_f32(Xbad).data_ptr(), dcodes.data_ptr(), n, d, m, h,
                                             1e-4, None)
        torch.cuda.synchronize()
        assert st == 0 and _guards_intact(Aw, GUARD_F) and _guards_intact(bw, GUARD_F)
        A, b = A.cpu().numpy().reshape(mh, mh), b.cpu().numpy().reshape(mh, d)
        assert np.array_equal(A.view(np.uint64), A0.view(np.uint64)), case
        nan = np.isnan(b0)
        assert np.array_equal(np.isnan(b), nan), case
        assert np.array_equal(b.view(np.uint64)[~nan], b0.view(np.uint64)[~nan]), (case, int((b != b0)[~nan].sum()))


# ---- A.4 the codebook updates -------------------------------------------------------------------------------------------------------
_NUMPY_SOLVE = {}


def _numpy_update(kind, m, h, d):
    """numpy's f64 solve on the CLEAN rows, once per shape: column k of the solution depends on column k of X alone, so outside
    the poisoned columns it is the solve of the zeroed rows."""
    import chain_oracle as co
    import lsq_update_oracle as lo
    key = (kind, m, h, d)
    if key not in _NUMPY_SOLVE:
        X, codes = tc.lsq_case(m, h, d)
        _NUMPY_SOLVE[key] = (lo.update(X, codes, h)[1].reshape(m, h, d) if kind == "lsq" else co.chain_update(X, codes, h)[1])
    return _NUMPY_SOLVE[key]


def _dev_update(kind, X, codes, m, h):
    """(status ok, C (m, h, d)) of the device entry, C between guard words."""
    import torch
    n, d = X.shape
    Cw, Cd = _guarded(np.full(m * h * d, 5.0, np.float32), torch.float32, GUARD_F)
    lib = _L().lib()
    f = lib.rq_dev_update_codebooks_lsq if kind == "lsq" else lib.rq_dev_update_codebooks_chain
    dX, dcodes = _dev_f32(X), torch.from_numpy(np.array(codes)).cuda()
    st = f(Cd.data_ptr(), dX.data_ptr(), dcodes.data_ptr(), n, d, m, h, 1e-4, None)
    torch.cuda.synchronize()
    ok = _status(st)
    assert _guards_intact(Cw, GUARD_F)
    return ok, Cd.cpu().numpy().reshape(m, h, d)


def _host_update(kind, X, codes, m, h):
    n, d = X.shape
    Ch = np.full((m, h, d), 5.0, np.float32)
    lib = _L().lib()
    f = lib.rq_update_codebooks_lsq if kind == "lsq" else lib.rq_update_codebooks_chain
    Xc, cc = np.ascontiguousarray(X), np.ascontiguousarray(codes)
    return _status(f(Ch.ctypes.data, Xc.ctypes.data, cc.ctypes.data, n, d, m, h, 1e-4)), Ch


def _check_update(kind, m, h, d):
    import lsq_update_oracle as lo
    X, codes = tc.lsq_case(m, h, d)
    Cn = _numpy_update(kind, m, h, d)
    scale = float(np.abs(Cn).max())
    for case in tc.lsq_poisons(d, m):
        keep = tc.keep_mask(case, d)
        assert (~keep).sum() == len(case) and len(case) / d < 0.1            # the excused columns, from the poison table
        Xbad, Xz = tc.poisoned(X, case), tc.zeroed(X, case)
        ok, Cb = _dev_update(kind, Xbad, codes, m, h)
        okz, Cz = _dev_update(kind, Xz, codes, m, h)
        assert okz
        if not ok:
            continue
        # the solve does not mix right-hand-side columns: changing column c of X changes column c of C alone
        assert np.array_equal(Cb[:, :, keep].view(np.uint32), Cz[:, :, keep].view(np.uint32)), case
        # and those columns are the f64 solve's within the finite-data tolerances of DESIGN.md section 2
        cw = np.abs(Cb[:, :, keep].astype(np.float64) - Cn[:, :, keep]).max()
        rec = np.abs(lo.reconstruct(Cb[:, :, keep], codes) - lo.reconstruct(Cn[:, :, keep], codes)).max()
        print("%s m=%d h=%d d=%d %s: reconstruction %.3e, codeword %.3e (x max|C| = %.3e)"
              % (kind, m, h, d, case, rec / scale, cw / scale, scale))
        assert rec <= 1e-5 * scale and cw <= 1e-4 * scale, case
        okh, Ch = _host_update(kind, Xbad, codes, m, h)
        assert okh and np.array_equal(Ch.view(np.uint32), Cb.view(np.uint32)), case          # host == device, NaN payloads included
        ok2, C2 = _dev_update(kind, Xbad, codes, m, h)
        assert ok2 and np.array_equal(C2.view(np.uint32), Cb.view(np.uint32)), case


@pytest.mark.parametrize("m,h", tc.LSQ_SHAPES)
def test_update_codebooks_lsq_keeps_a_poison_in_its_column(rq, m, h):
    _check_update("lsq", m, h, tc.LSQ_D)


@pytest.mark.parametrize("d", [24, 23])
@pytest.mark.parametrize("m,h", tc.LSQ_SHAPES)
def test_update_codebooks_chain_keeps_a_poison_in_its_column(rq, m, h, d):
    _check_update("chain", m, h, d)


# ---- A.5 rq_sr_std and rq_sr_perturb ---------------------------------------------------------------------------------------------------
def test_sr_std_and_perturb(rq):
    import sr_oracle as so
    from rayuela_jl_amd.SR import sr_perturb, sr_std
    n, d = tc.LSQ_N, tc.LSQ_D
    rng = np.random.default_rng(n + d)
    X = (rng.standard_normal((n, d)) * rng.uniform(0.1, 100, size=d) + rng.uniform(-50, 50, size=d)).astype(np.float32)
    assert np.array_equal(sr_std(X).view(np.uint32), tc.sr_sigma(X).view(np.uint32))         # the restatement is the device's bits
    for case in tc.poison_table(n, d, 4):
        Xbad = tc.poisoned(X, case)
        keep = tc.keep_mask(case, d)
        got, want = sr_std(Xbad), tc.sr_sigma(Xbad)
        assert np.array_equal(got.view(np.uint32)[keep], want.view(np.uint32)[keep]), case
        assert np.array_equal(got.view(np.uint32)[keep], tc.sr_sigma(X).view(np.uint32)[keep]), case
        for r, c, kind in case:                                         # column c: the restated arithmetic's answer
            assert (np.isnan(got[c]) and np.isnan(want[c])) or got[c] == want[c], (case, got[c], want[c])
            assert np.isnan(got[c]) == (kind != "3e38")
        assert np.array_equal(sr_std(Xbad).view(np.uint32), got.view(np.uint32))
    sigma = rng.uniform(0.5, 30.0, size=d).astype(np.float32)
    for kind, name in ((so.SR_C, "SR_C"), (so.SR_D, "SR_D")):
        for c, bits in ((0, nf.NAN_POS), (d - 1, 0x7F800000), (7, 0xFF800000)):
            sg = sigma.copy()
            nf.put_bits(sg, c, bits)
            Y = sr_perturb(X, sg, 0.25, name, seed=3, call=2)
            with np.errstate(all="ignore"):
                Y0 = so.perturb(X, sg, 0.25, kind, 3, 2)
            other = np.arange(d) != c
            assert np.array_equal(Y[:, other].view(np.uint32), Y0[:, other].view(np.uint32)), (name, c)
            assert not np.isfinite(Y[:, c]).any(), (name, c)
            assert np.array_equal(Y[:, other].view(np.uint32), so.perturb(X, sigma, 0.25, kind, 3, 2)[:, other].view(np.uint32))
    L = _L().lib()
    Y = np.full((n, d), GUARD_F, np.float32)
    for scale in (float("nan"), float("inf"), float("-inf")):           # still refused, nothing written
        assert L.rq_sr_perturb(Y.ctypes.data, X.ctypes.data, sigma.ctypes.data, scale, n, d, 0, 3, 0, 0) == -1
    assert (Y == GUARD_F).all()


# ---- B.3 rq_train_lsq, rq_train_sr, rq_train_chainq on a base with one poisoned row ----------------------------------------------------
def _rotation(d, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return q.astype(np.float32)


def _train_lsq(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, nsplits, seed=9):
    n, d = X.shape
    Cs, codes, obj = np.zeros((m, h, d), np.float32), np.array(codes0, dtype=np.uint8, order="C"), np.full(niter, -7.0)
    st = _L().lib().rq_train_lsq(Cs.ctypes.data, codes.ctypes.data, obj.ctypes.data, X.ctypes.data, R.ctypes.data, n, d, m, h, niter,
                                 ilsiter, icmiter, npert, 1, seed, nsplits)
    return st, [Cs, codes, obj]


def _train_sr(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, nsplits, method, clean, seed=9):
    n, d = X.shape
    Cs, codes, obj = np.zeros((m, h, d), np.float32), np.array(codes0, dtype=np.uint8, order="C"), np.full(niter + 1, -7.0)
    st = _L().lib().rq_train_sr(Cs.ctypes.data, codes.ctypes.data, obj.ctypes.data, X.ctypes.data, R.ctypes.data, n, d, m, h, niter,
                                ilsiter, icmiter, npert, 1, method, 1, 0.5, clean, seed, nsplits)
    return st, [Cs, codes, obj]


def _train_chainq(X, codes0, m, h, R0, niter):
    n, d = X.shape
    Cs, codes, obj = np.zeros((m, h, d), np.float32), np.array(codes0, dtype=np.uint8, order="C"), np.full(niter + 1, -7.0)
    R = np.array(R0, dtype=np.float32, order="C")
    st = _L().lib().rq_train_chainq(Cs.ctypes.data, codes.ctypes.data, R.ctypes.data, obj.ctypes.data, X.ctypes.data, n, d, m, h, niter)
    return st, [Cs, codes, R, obj]


def _bar(run, run_finite, h, what, after_ok=None):
    """The common bar: a known-good finite run, the poisoned run twice (status, range, the same bits), the finite run again."""
    st, good = run_finite()
    assert st == 0, what
    good = _bits(*good)
    runs, out = [], None
    for _ in range(2):
        st, out = run()
        ok = _status(st)
        if ok:
            assert out[1].dtype == np.uint8 and int(out[1].max()) <= h - 1, (what, int(out[1].max()))   # (h = 256: the type's range)
            assert (out[-1] != -7.0).all(), what                                  # obj: every documented entry was written
            if after_ok is not None:
                after_ok(out)
        runs.append((ok, _bits(*out)))
    _same_twice(runs, what)
    st, again = run_finite()
    assert st == 0 and all(np.array_equal(a, b) for a, b in zip(_bits(*again), good)), what
    return runs[0][0], out


@pytest.mark.parametrize("poison", list(tc.TRAIN_POISONS))
@pytest.mark.parametrize("m,h", tc.LSQ_SHAPES)
def test_train_lsq(rq, m, h, poison):
    from test_gpu_lsq_train import _composed
    X, Xbad, codes0 = tc.train_aq_case(m, h, poison)
    R = _rotation(X.shape[1], 6)
    statuses, composed = [], 0
    for npert, nsplits in ((0, 1), (2, 2), (2, 1), (0, 2)):
        ok, out = _bar(lambda: _train_lsq(Xbad, codes0, m, h, R, 2, 2, 2, npert, nsplits),
                       lambda: _train_lsq(X, codes0, m, h, R, 2, 2, 2, npert, nsplits), h, (poison, npert, nsplits))
        assert out[2].shape == (2,)
        statuses.append(ok)
        if ok and nsplits == 1:
            # the public steps composed (update, rotate back, encode_icm), as the finite test composes them: the same codes
            try:
                Cc, codes_c, _ = _composed(Xbad, codes0, m, h, R, 2, 2, 2, npert, True, 9)
            except rq.RayuelaHipError:
                continue                                                  # a public step refuses what the fused loop accepts
            assert np.array_equal(out[1], codes_c), (poison, npert)
            composed += 1
    print("train_lsq m=%d h=%d %s: RQ_OK %s, %d runs compared with the composed steps" % (m, h, poison, statuses, composed))


@pytest.mark.parametrize("poison", list(tc.TRAIN_POISONS))
@pytest.mark.parametrize("method", [0, 1], ids=["SR_C", "SR_D"])
@pytest.mark.parametrize("m,h", tc.LSQ_SHAPES)
def test_train_sr(rq, m, h, method, poison):
    from test_gpu_sr import _composed
    X, Xbad, codes0 = tc.train_aq_case(m, h, poison)
    R = _rotation(X.shape[1], 6)
    statuses, composed = [], 0
    for clean in (0, 1):
        for npert, nsplits in ((0, 1), (2, 2)):
            what = (poison, method, clean, npert, nsplits)
            ok, out = _bar(lambda: _train_sr(Xbad, codes0, m, h, R, 2, 2, 2, npert, nsplits, method, clean),
                           lambda: _train_sr(X, codes0, m, h, R, 2, 2, 2, npert, nsplits, method, clean), h, what)
            assert out[2].shape == (3,)
            statuses.append(ok)
            if ok and nsplits == 1:
                try:
                    _, codes_c, _ = _composed(Xbad, codes0, m, h, R, 2, 2, 2, npert, True, 9, ("SR_C", "SR_D")[method], 1, 0.5,
                                              bool(clean))
                except (rq.RayuelaHipError, ValueError):
                    continue
                assert np.array_equal(out[1], codes_c), what
                composed += 1
    print("train_sr m=%d h=%d method=%d %s: RQ_OK %s, %d runs compared with the composed steps"
          % (m, h, method, poison, statuses, composed))


@pytest.mark.parametrize("poison", list(tc.TRAIN_POISONS))
def test_train_chainq(rq, poison):
    m, h, niter = 4, 16, 2
    X, Xbad, codes0 = tc.train_aq_case(m, h, poison)
    d = X.shape[1]
    R0 = _rotation(d, 6)

    def after_ok(out):
        Cs, codes, R, obj = out
        assert obj.shape == (niter + 1,)
        if np.isfinite(R).all():                                          # never "finite but not orthonormal"
            R64 = R.astype(np.float64)
            assert np.abs(R64 @ R64.T - np.eye(d)).max() < 1e-5, poison
        else:
            assert np.isnan(R).any(), poison
        # the final codes are the Viterbi codes of the final (R, C), as the finite test asserts
        from rayuela_jl_amd.ChainQ import quantize_chainq_u8
        assert np.array_equal(quantize_chainq_u8(rq.rotate(R, Xbad), Cs), codes), poison

    ok, _ = _bar(lambda: _train_chainq(Xbad, codes0, m, h, R0, niter), lambda: _train_chainq(X, codes0, m, h, R0, niter), h,
                 poison, after_ok)
    print("train_chainq %s: RQ_OK %s" % (poison, ok))
    if not ok:            # the refusal: the polar factor of X CB' gives up on a non-finite Gram matrix, and nothing was written
        st, (Cs, codes, R, obj) = _train_chainq(Xbad, codes0, m, h, R0, niter)
        msg = (_L().lib().rq_last_error() or b"").decode()
        assert st == -2 and "polar factor" in msg, (st, msg)
        assert (Cs == 0).all() and np.array_equal(codes, codes0) and np.array_equal(R, R0) and (obj == -7.0).all()
