"""CPU: tests/nonfinite_train_cases.py -- the inputs and restatements tests/test_gpu_nonfinite_train.py holds the training
kernels to -- against the existing oracles (tests/train_wide_oracle.py, tests/kmeans_oracle.py, tests/wide_oracle.py), without a
device.  On the finite part of every case the restatement IS the existing one; what a poison may reach is derived here in
float64 for both formulations of the segment sum (scatter: one cell; one-hot product: the column), and the excuse is counted."""
import numpy as np
import pytest

import kmeans_oracle as ko
import nonfinite_ref as nf
import nonfinite_train_cases as tc
import train_wide_oracle as two
import wide_oracle as wo

# the mass-refill walk (tc.refill_fixture, seed tc.REFILL["seed"]): iterations to convergence, cost-proportional re-draws,
# uniform re-draws, re-draws of centres >= 256, centres without rows in iteration 1 -- derived below, asserted on the library by
# tests/test_gpu_nonfinite_train.py::test_mass_refill_walk
REFILL_WALK = (3, 36, 767, 128, 285)


@pytest.mark.parametrize("shape", tc.SHAPES_WIDE + tc.SHAPES_BYTE)
def test_poison_tables(shape):
    n, d, m, h = shape
    table = tc.poison_table(n, d, m)
    rp = tc.slice_rows(n)
    t = tc.tail_row(n)
    assert t < rp and t >= rp // 64 * 64 and rp % 64                         # inside the ragged tail of slice 0
    assert [case[0][0] for case in table[:7]] == [0, 31, 32, 63, 64, t, n - 1]
    assert {k for case in table for _, _, k in case} == set(tc.KINDS)
    sub = tc.sub_of(d, m)
    (r1, c1, _), (r2, c2, _) = table[7]
    assert r1 != r2 and c1 != c2 and sub[c1] != sub[c2]
    for case in table:
        assert all(0 <= r < n and 0 <= c < d for r, c, _ in case)
        assert tc.excused_cells(case, d, m, h) == h * len(case) == h * int((~tc.keep_mask(case, d)).sum())
        # the excuse is the poisoned column(s) of C: its share is columns / d, the size of a column
        assert tc.excused_cells(case, d, m, h) / (h * d) == len(case) / d
    c = tc.centre_case(n, d, m, h)
    for i in range(m):
        cnt = np.bincount(c["codes"][:, i], minlength=h)
        assert (cnt[list(c["empty"])] == 0).all() and cnt[h - 1] > 0 and (cnt > 0).sum() > h // 2
    if h > 256:
        assert (c["codes"] >= 256).any() and np.bincount(c["codes"][:, 0], minlength=h)[h - 1] > 0


@pytest.mark.parametrize("shape", tc.SHAPES_WIDE + tc.SHAPES_BYTE)
def test_a_poison_stays_in_its_column_in_both_formulations(shape):
    """float64 on the poisoned rows themselves: a scatter-add reaches the one cell (code of row r, column c); a product with
    the one-hot matrix reaches every code of column c (0 x NaN) and no other column.  Everywhere else both are the sums of
    tc.means -- which on a clean input is train_wide_oracle.exact_means itself."""
    n, d, m, h = shape
    c = tc.centre_case(n, d, m, h)
    clean, ccnt = two.exact_means(c["X"], c["C0"], c["codes"], m, h)
    off = c["off"]
    sub = tc.sub_of(d, m)
    for case in tc.poison_table(n, d, m):
        want, cnt = tc.means(c, case, m, h)
        keep = tc.keep_mask(case, d)
        assert np.array_equal(cnt, ccnt)
        for i in range(m):
            k = keep[off[i]:off[i + 1]]
            assert np.array_equal(want[i][:, k].view(np.uint32), clean[i][:, k].view(np.uint32))
            e = np.flatnonzero(cnt[i] == 0)
            assert np.array_equal(want[i][e].view(np.uint32), c["C0"][i][e].view(np.uint32))
        Xbad = tc.poisoned(c["X"], case).astype(np.float64)
        with np.errstate(all="ignore"):
            for i in range(m):
                ci = c["codes"][:, i]
                A = np.zeros((h, n))
                A[ci, np.arange(n)] = 1.0
                prod = A @ Xbad[:, off[i]:off[i + 1]]
                scat = np.zeros((h, off[i + 1] - off[i]))
                np.add.at(scat, ci, Xbad[:, off[i]:off[i + 1]])
                exact = np.stack([np.bincount(ci, weights=c["X"][:, s].astype(np.float64), minlength=h)
                                  for s in range(off[i], off[i + 1])], 1)
                k = keep[off[i]:off[i + 1]]
                assert np.array_equal(prod[:, k], exact[:, k]) and np.array_equal(scat[:, k], exact[:, k])
                for r, col, kind in case:
                    if sub[col] != i:
                        continue
                    s = col - off[i]
                    others = np.arange(h) != ci[r]
                    assert np.array_equal(scat[others, s], exact[others, s])            # scatter: one cell
                    if kind != "3e38":
                        assert not np.isfinite(scat[ci[r], s])
                        assert np.isnan(prod[others, s]).all()                          # product: the whole column


@pytest.mark.parametrize("shape", tc.SHAPES_WIDE)
def test_reconstruct_restatement_keeps_bits(shape):
    n, d, m, h = shape
    c = tc.centre_case(n, d, m, h)
    C, cells = tc.poisoned_codebooks(c["C0"], d, m, h)
    codes = np.array(c["codes"]).astype(np.int16)
    for j, (i, k, s) in enumerate(cells):
        codes[100 + j, i] = k                                                # every poisoned entry is gathered
    CB = two.reconstruct(C, codes, c["off"], d)
    for j, (i, k, s) in enumerate(cells):
        assert CB.view(np.uint32)[100 + j, c["off"][i] + s] == C[i].view(np.uint32)[k, s]
    bits = {int(C[i].view(np.uint32)[k, s]) for i, k, s in cells}
    assert {nf.NAN_POS, nf.NAN_NEG, 0x7F800000, 0xFF800000, 1, 0x80000001} == bits


def test_first_seeds_are_the_restated_first_seeds():
    X = ko.int_data(400, 6, 3)
    for salt in (ko.SALT_PQ, ko.SALT_RVQ):
        assert tc.first_seeds(400, 2, 9, 5, salt) == ko.kmpp_seeds(X, 2, 9, 5, salt=salt)[:, 0].tolist()
    for d, m, h in [(32, 4, 300), (30, 5, 257), (24, 3, 300)]:
        for poison in tc.TRAIN_POISONS:
            X, row = tc.poisoned_base(d, m, h, poison)
            bad = np.flatnonzero(~np.isfinite(X).all(axis=1) | (np.abs(X) > 1e19).any(axis=1))
            assert bad.tolist() == [row] and row not in tc.first_seeds(tc.NT, m, h, tc.TRAIN_SEED, ko.SALT_PQ)
            assert 1 / tc.NT < 0.01                                          # the excused row's share of the base


def test_mass_refill_walk(oracle):
    """The restated Lloyd loop alone on the mass-refill fixture: both repick branches, hundreds of centres at once."""
    X, m, h, seed = tc.refill_fixture()
    assert np.array_equal(X, np.round(X)) and X.min() >= 0 and X.max() <= 255
    assert len({tuple(r) for r in X.tolist()}) <= 41 < h
    K, Cs, codes, rows, st = two.walk(oracle, X, m, h, seed, kmpp=False)
    empty1 = int((np.bincount(codes[0][:, 0], minlength=h) == 0).sum())
    print("mass refill: K = %d, %d cost-proportional, %d uniform, %d of centres >= 256, %d centres empty in iteration 1; "
          "smallest margin %.3g" % (K, st["cost"], st["uniform"], st["wide"], empty1, st["margin"]))
    assert (K, st["cost"], st["uniform"], st["wide"], empty1) == REFILL_WALK
    assert empty1 > 250 and st["cost"] > 0 and st["uniform"] > 0 and st["margin"] > 1e-9
    Xn = tc.refill_fixture_nan()
    assert np.isnan(Xn).sum() == 1 and np.array_equal(np.isnan(Xn).any(axis=1).nonzero()[0], [450])


@pytest.mark.parametrize("shape", tc.WIDE_ENCODE_SHAPES)
def test_wide_encode_cases_reach_their_edges(oracle, shape):
    n, d, m, h = shape
    X, Ccat = tc.wide_encode_case(n, d, m, h)
    ref = wo.encode_pq_wide(oracle, X, Ccat, m, h)
    assert ref.min() >= 0 and ref.max() < h
    assert np.isnan(X).any() and np.isinf(X).any() and np.isinf(Ccat).any()
    nan_cells = [(3, int(tc.sub_of(d, m)[min(5, d - 1)])), (n - 1, int(tc.sub_of(d, m)[d // 2 + 1]))]
    assert all(ref[r, i] == 0 for r, i in nan_cells)                        # every distance NaN: code 0
    if h == 257:
        # the live last codeword wins rows; so does the Inf one (|c|^2 - 2<x, c> = Inf - Inf = NaN, clamped to 0, the oracle's
        # arithmetic), the single live entry of a block whose 255 padded neighbours must never be named
        assert (ref[:, 2] == 256).any() and (ref[:, 1] == 256).any()
    else:
        assert ref[50, 0] == 0 and (ref >= 256).any()


# ---- LSQ / chain / SR ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,h", tc.LSQ_SHAPES)
def test_lsq_normal_equations_keep_a_poison_in_its_cells(m, h):
    """lsq_update_oracle.normal_eq on the poisoned rows: A is that of the clean rows (it depends on the codes alone); b differs
    from the clean b exactly in the cells (i h + code_i(r), c) -- m cells per poison, far below 1 % of b."""
    import lsq_update_oracle as lo
    X, codes = tc.lsq_case(m, h)
    n, d = X.shape
    A0, b0 = lo.normal_eq(X, codes, h)
    for case in tc.lsq_poisons(d, m):
        with np.errstate(all="ignore"):
            A, b = lo.normal_eq(tc.poisoned(X, case), codes, h)
        assert np.array_equal(A, A0)
        cells = {(i * h + int(codes[r, i]), c) for r, c, _ in case for i in range(m)}
        differ = {tuple(x) for x in np.argwhere(b.view(np.uint64) != b0.view(np.uint64)).tolist()}
        assert differ == cells and len(cells) == m * len(case) and len(cells) / b.size < 0.01
        nan = {tuple(x) for x in np.argwhere(np.isnan(b)).tolist()}
        assert nan == {(i * h + int(codes[r, i]), c) for r, c, k in case if k.startswith("nan") for i in range(m)}


@pytest.mark.parametrize("n,d", [(4001, 24), (1024, 5), (1025, 3)])
def test_sr_sigma_restatement(n, d):
    """The restated standard deviation is numpy's f64 one rounded to f32 or a neighbour of it (the bar
    tests/test_gpu_sr.py::test_std_against_numpy holds the device to); a poisoned coordinate changes its own column alone."""
    rng = np.random.default_rng(n + d)
    X = (rng.standard_normal((n, d)) * rng.uniform(0.1, 100, size=d) + rng.uniform(-50, 50, size=d)).astype(np.float32)
    s = tc.sr_sigma(X)
    want = np.std(X.astype(np.float64), axis=0, ddof=1).astype(np.float32)
    assert ((s == want) | (s == np.nextafter(want, np.float32(-np.inf))) | (s == np.nextafter(want, np.float32(np.inf)))).all()
    assert np.array_equal(tc.sr_sigma(X, 3.0), (s.astype(np.float64) / 3.0).astype(np.float32))
    for kind in tc.KINDS:
        Xb = X.copy()
        nf.put_bits(Xb, (n // 2, d - 1), tc.F32[kind])
        sb = tc.sr_sigma(Xb)
        assert np.array_equal(sb[:d - 1].view(np.uint32), s[:d - 1].view(np.uint32))
        assert np.isnan(sb[d - 1]) if kind != "3e38" else np.isfinite(sb[d - 1]) and sb[d - 1] > 1e35
