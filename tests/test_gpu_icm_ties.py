"""GPU: the two tie rules of the LSQ encoding contract on the device, for both ICM kernels: the code of a
conditioning step is the first index of the minimum under strict `<`, and a perturbed solution replaces the old one only if its
cost is strictly smaller.  The cases are those of tests/icm_tie_cases.py (bit-identical copies of codewords, start codes that
reconstruct X exactly from the highest copies, small integers), each compared bit for bit, codes and per-row cost, with the
restatement; tests/test_icm_tie_cases.py shows on the CPU that a last-index argmin or a `<=` accept test fails them.  Then the six
reference-derived fixtures tests/golden/icm_*.npz through both entries, and what cannot matter (nsplits, the entry, code_base) on
tie data.

Measured on the MI355X, in a run of the whole suite: the 56 tests of this file take 0.9 s together, the restatement's tables
included; the slowest is wide-m2-h4096-P2048-low at 0.2 s, every other one takes under 0.1 s.  Run first in a process, the first
test adds 1.7 s of loading the library."""
import os

import numpy as np
import pytest

import icm_tie_cases as tc
from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("icm_") and f.endswith(".npz"))


def _gpu(wide, X, C, B0, args, seed=tc.ILS_SEED, t0=0, nsplits=1):
    from rayuela_jl_amd.LSQ import encode_icm_u16, encode_icm_u8
    if wide:
        return encode_icm_u16(X, B0.astype(np.int16), C, *args, seed=seed, t0=t0, nsplits=nsplits, with_cost=True)
    return encode_icm_u8(X, B0.astype(np.uint8), C, *args, seed=seed, t0=t0, nsplits=nsplits, with_cost=True)


def _assert_same(got, want):
    (b1, c1), (b0, c0) = got, want
    bad = np.flatnonzero((b1 != b0).any(axis=1))
    assert bad.size == 0, "%d rows differ, first %d: gpu %s oracle %s" % (bad.size, bad[0], b1[bad[0]], b0[bad[0]])
    assert np.array_equal(c1.view(np.uint32), c0.view(np.uint32)), "per-row costs differ"


def _run(case):
    X, C, B0, codes, cost = tc.expected(case)
    got = _gpu(case.wide, X, C, B0, case.args)
    assert got[0].dtype == codes.dtype
    return got, (X, C, B0, codes, cost)


# ---- a. the lowest copy wins ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.BYTE_LOW + tc.WIDE_LOW, ids=tc.case_id)
def test_lowest_copy_wins(rq, case):
    got, (X, C, B0, codes, cost) = _run(case)
    # without the oracle: B0 is below P, every position is conditioned, and a copy at l + qP never beats l
    assert got[0].min() >= 0 and got[0].max() < case.P, "a higher copy won on %d rows" % int((got[0] >= case.P).any(axis=1).sum())
    if case.P == 1:
        assert ((got[0] == 0) | (got[0] == B0)).all()
    _assert_same(got, (codes, cost))


# ---- b. an equal cost keeps the old codes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.BYTE_KEEP + tc.WIDE_KEEP, ids=tc.case_id)
def test_equal_cost_keeps_the_old_codes(rq, case):
    got, (X, C, B0, codes, cost) = _run(case)
    moved = np.flatnonzero((got[0] != B0).any(axis=1))
    assert moved.size == 0, "%d rows left their start codes at an equal cost, first %d: %s -> %s" % (
        moved.size, moved[0], B0[moved[0]], got[0][moved[0]])
    assert np.array_equal(got[1].view(np.uint32), np.zeros(case.n, np.uint32)), "a cost is not +0.0"
    _assert_same(got, (codes, cost))


def test_high_start_codes_on_gaussian_rows_end_on_the_lowest_copies(rq):
    case = tc.WIDE_HIGH_GAUSS
    got, (X, C, B0, codes, cost) = _run(case)
    assert B0.min() >= case.h - case.P and got[0].max() < case.P
    _assert_same(got, (codes, cost))


# ---- c. different codewords, equal costs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.BYTE_INT + tc.WIDE_INT, ids=tc.case_id)
def test_integer_valued_ties(rq, case):
    got, (X, C, B0, codes, cost) = _run(case)
    assert got[0].min() >= 0 and got[0].max() < case.h
    _assert_same(got, (codes, cost))


# ---- d. the reference's fixtures on the device ----------------------------------------------------------------------------------------
def _fixture(name):
    g = golden(name)
    ils, icm, npert, randord, seed, t0 = [int(v) for v in g["params"]]
    return g, (ils, icm, npert, bool(randord)), seed, t0


def test_fixtures_exist():
    assert len(FIXTURES) >= 6 and {"icm_m4_ties", "icm_m4_all_rejected"} <= set(FIXTURES)


@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_condition_fixtures(rq, name, wide):
    g, args, seed, t0 = _fixture(name)
    got = _gpu(wide, g["X"], g["C"], g["B0"], args, seed=seed, t0=t0)
    _assert_same(got, (g["codes"], g["cost"]))
    if name.endswith("all_rejected"):
        assert np.array_equal(got[0], g["B0"])


def test_reference_ties_fixture_through_the_device_entry(rq):
    import torch
    from rayuela_jl_amd import _lib
    g, (ils, icm, npert, randord), seed, t0 = _fixture("icm_m4_ties")
    n, d = g["X"].shape
    m, h, _ = g["C"].shape
    dev = torch.device("cuda:0")
    tX, tC, tB = (torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("X", "C", "B0"))
    tout = torch.empty_like(tB)
    tcost = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().rq_dev_encode_icm(tout.data_ptr(), tB.data_ptr(), tcost.data_ptr(), tX.data_ptr(), tC.data_ptr(), n, d, m, h,
                                            ils, icm, npert, 1 if randord else 0, seed, t0, 2, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    _assert_same((tout.cpu().numpy(), tcost.cpu().numpy()), (g["codes"], g["cost"]))


# ---- e. what cannot matter, on tie data ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [tc.BYTE_LOW[3], tc.WIDE_LOW[3]], ids=tc.case_id)
def test_nsplits_do_not_change_results(rq, case):
    X, C, B0, codes, cost = tc.expected(case)
    one = _gpu(case.wide, X, C, B0, case.args, nsplits=1)
    _assert_same(_gpu(case.wide, X, C, B0, case.args, nsplits=3), one)
    _assert_same(one, (codes, cost))


@pytest.mark.parametrize("case", tc.BYTE_LOW + tc.BYTE_KEEP, ids=tc.case_id)
def test_wide_entry_equals_byte_entry(rq, case):
    X, C, B0, _, _ = tc.expected(case)
    b8, c8 = _gpu(False, X, C, B0, case.args)
    _assert_same(_gpu(True, X, C, B0, case.args), (b8.astype(np.int16), c8))


def test_code_base_one(rq):
    from rayuela_jl_amd import _lib
    case = tc.WIDE_LOW[4]                                   # (4, 300, 256): copies in the short last piece
    X, C, B0, codes, cost = tc.expected(case)
    n, m = B0.shape
    B1 = np.ascontiguousarray(B0 + 1)
    out, c = np.full((n, m), -3, np.int16), np.full(n, -3.0, np.float32)
    ils, icm, npert, randord = case.args
    rc = _lib.lib().rq_encode_icm_wide(out.ctypes.data, B1.ctypes.data, c.ctypes.data, X.ctypes.data, C.ctypes.data, n, case.d, m,
                                       case.h, ils, icm, npert, 1 if randord else 0, tc.ILS_SEED, 0, 1, 1)
    assert rc == 0 and out.min() >= 1 and out.max() <= case.P
    _assert_same((out - 1, c), (codes, cost))
