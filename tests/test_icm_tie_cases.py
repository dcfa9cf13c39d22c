"""CPU: the cases of tests/test_gpu_icm_ties.py have teeth.  From the restatement alone (tests/icm_oracle.py,
tests/icm_wide_oracle.py and the mutants of tests/icm_tie_cases.py): on every case a conditioning step that takes the last index of
the minimum, or an accept test written `<=`, ends with other codes than the contract's, and the ties fall where each kernel's
layout can get them wrong (inside a lane, across lanes, across the wide kernel's pieces).  These are conditions on the test data,
not measurements of the code under test: a seed or a shape that misses one is changed, never the bound.  Run with -s for the
census and the rows each mutant changes, per case."""
import numpy as np
import pytest

import icm_tie_cases as tc
from conftest import golden


def _count(cen, key):
    return int(cen[key].sum())


@pytest.mark.parametrize("case", tc.ALL_CASES, ids=tc.case_id)
def test_case_tells_the_mutants_from_the_contract(oracle, case):
    s = tc.study(case)
    X, C, B0, codes, cost = s["exp"]
    n, cen = case.n, s["census"]
    assert X.shape == (n, case.d) and C.shape == (case.m, case.h, case.d) and B0.shape == (n, case.m)
    print("%s: %d of %d steps tied (same lane %d, cross lane %d, cross piece %d, two in one lane %d); "
          "equal-cost rejections on %d of %d rows; last-index mutant changes %d rows, <= mutant %d" % (
              tc.case_id(case), _count(cen, "tied"), cen["tied"].size, _count(cen, "same_lane"), _count(cen, "cross_lane"),
              _count(cen, "cross_piece"), _count(cen, "in_lane"), cen["eq_reject_rows"].size, n, s["last_rows"].size, s["le_rows"].size))
    # with no flag the mutant IS the restatement
    assert s["plain"][0].dtype == codes.dtype and np.array_equal(s["plain"][0], codes)
    assert np.array_equal(s["plain"][1].view(np.uint32), cost.view(np.uint32))
    if case.bar is not None:
        assert s["last_rows"].size >= case.bar * n, (s["last_rows"].size, n)
    if case.kind == "dup":
        # every copy ties with its original: every step of every row is tied
        assert cen["tied"].all() or case.h < 2 * case.P
        if case.where == "low":
            assert codes.max() < case.P                         # B0 is below P and every position is conditioned
        if case.P == 1:
            assert ((codes == 0) | (codes == B0)).all()
    if case.kind == "dup" and case.where == "high":
        assert B0.min() >= case.h - case.P and B0.max() == case.h - 1
        if case.exact:
            assert np.array_equal(codes, B0) and np.array_equal(cost.view(np.uint32), np.zeros(n, np.uint32))
            assert s["le_rows"].size >= n / 4, s["le_rows"].size
            assert np.array_equal(s["le_rows"], cen["eq_reject_rows"])
        else:
            assert codes.max() < case.P                         # every row improved once: the lower copies won everywhere
    if case.kind == "int":
        assert _count(cen, "tied") >= 0.10 * cen["tied"].size
        if case.wide:
            assert _count(cen, "cross_piece") >= 1


@pytest.mark.parametrize("wide", [False, True], ids=["byte", "wide"])
def test_ties_fall_inside_lanes_across_lanes_and_across_pieces(oracle, wide):
    cens = [tc.study(c)["census"] for c in (tc.WIDE_CASES if wide else tc.BYTE_CASES)]
    same = sum(_count(c, "same_lane") for c in cens)
    cross = sum(_count(c, "cross_lane") for c in cens)
    both = sum(int((c["same_lane"] & c["cross_piece"]).sum()) for c in cens)
    print("%s family: %d same-lane ties, %d cross-lane ties, %d same-lane cross-piece ties" % ("wide" if wide else "byte", same,
                                                                                                cross, both))
    assert same >= 1 and cross >= 1
    assert sum(_count(c, "in_lane") for c in cens) >= 1
    if wide:
        assert both >= 1                                        # P = 256: a copy sits in the same lane of the next piece


def test_builders():
    X, C, B0 = tc.dup_case(10, 6, 3, 11, 4, where="high", exact=True)
    assert X.dtype == C.dtype == np.float32 and B0.dtype == np.int16
    for l in range(11):
        assert np.array_equal(C[:, l].view(np.uint32), C[:, l % 4].view(np.uint32))
    assert not np.array_equal(C[:, 0], C[:, 1])
    assert ((B0 + 4 > 10) & (B0 <= 10)).all()                   # the highest copy of its class
    Xl, Cl, Bl = tc.dup_case(10, 6, 3, 11, 4, where="low", exact=True)
    assert np.array_equal(Cl, C) and np.array_equal(Bl, B0 % 4) and np.array_equal(Xl.view(np.uint32), X.view(np.uint32))
    assert np.array_equal(tc.io.veccost(X, B0, C).view(np.uint32), np.zeros(10, np.uint32))     # +0.0, bitwise
    # int_case at the generator's shape and seed is the reference-derived fixture itself
    g = golden("icm_m4_ties")
    X, C, B0 = tc.int_case(256, 12, 4, 256, seed=105)
    assert np.array_equal(X, g["X"]) and np.array_equal(C, g["C"]) and np.array_equal(B0, g["B0"])
    assert len({tc.case_id(c) for c in tc.ALL_CASES}) == len(tc.ALL_CASES) == 28
