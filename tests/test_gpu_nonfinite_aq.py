"""GPU: the non-finite contract (include/rayuela_hip.h, "Non-finite inputs") on the additive scans -- linscan_lsq, linscan_cq,
the two *_extra_byte legacy symbols, rq_dev_linscan_aq, rq_lsq_prepare / rq_lsq_search -- whose tables are signed, whose rows
carry a bias, and whose pre-filter has an O(n) preparation pass of its own (rq_scan.hip: cnorm / norm_residual / norm_minmax /
norm_info / norm_quant kernels) that turns the rows' residual norms into ordered keys.

The bar everywhere: ids and distance bits of EVERY query equal tests/nonfinite_ref.py (the contract in plain numpy, pinned to
the C oracle and the compiled reference by tests/test_nonfinite_ref.py), the poisoned queries included.  That the calls
return is checked by the tests finishing.  Every case asserts the path it names: the kernel instantiation
(rq_last_scan_kernel), the planner's slice length against the kernel's own "filter on" condition, the in-call order
(rq_scan_orders_in_call + rq_order_cache_stats), the order plan of a prepared base (rq_order_plan).

LSQ scans that are handed raw pointers keep the arrival order (row_bias and the norm bytes are indexed by position,
rq_api.hip dev_linscan), so "in-call order on / off" exists for the CQ form only; the ordered LSQ path is the prepared base
of rq_lsq_prepare (LsqIndex), which orders rows, norms and norm bytes alike once it holds ORDER_MIN_ROWS rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import nonfinite_ref as nf
from switch_table import switches

pytestmark = pytest.mark.gpu

N, D, H = 200_000, 24, 256
SLOTS = ((3, 1), (9, D - 1), (12, 0))          # (query, coordinate): three different slots of two 8-query groups


def _L():
    from rayuela_jl_amd import _lib
    return _lib


def _kernel():
    return (_L().lib().rq_last_scan_kernel() or b"").decode()


def _plan(n, nq, m, K):
    return _L().scan_plan(n, nq, m, D, K)


def _filter_can_run(n, nq, m, K):
    """The kernel's own condition (rq_scan.hip, filt_on): a work item's rows >= 64 * max(K, 8)."""
    p = _plan(n, nq, m, K)
    return min(n, p["rows_per_slice"]) >= 64 * max(K, 8)


@functools.lru_cache(maxsize=None)
def _base(n, m, nq, ties=False):
    import rayuela_jl_amd.synth as synth
    from oracle import oracle
    rng = np.random.default_rng(100 * m + nq + (7 if ties else 0))
    cb = rng.standard_normal((m * H, D)).astype(np.float32)
    X = rng.standard_normal((nq, D)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=m + nq)
    if ties:                                   # half of the rows drawn from 300 distinct rows: many exact ties
        codes[n // 2:] = codes[rng.integers(0, 300, n - n // 2)]
    xhat = np.zeros((n, D), dtype=np.float64)
    for i in range(m):
        xhat += cb[i * H + codes[:, i].astype(np.int64)]
    nrm = (xhat ** 2).sum(1).astype(np.float32)                             # the true |x_hat|^2
    R = synth.rotation(D, seed=3)
    Qd = oracle.rotate_T(R, X)                 # what the entry points without R are handed
    for a in (cb, X, codes, nrm, R, Qd):
        a.setflags(write=False)
    return cb, X, codes, nrm, R, Qd


def _some_rows(n, part, of=4):
    """~1 % of the rows, disjoint for different `part`."""
    return np.arange(part * 25 + 3, n, 25 * of)


NORM_POISONS = ["nrm_nan_pos", "nrm_nan_neg", "nrm_pinf", "nrm_ninf", "nrm_all", "nrm_wide_one_nan", "nrm_few_left", "nrm_all_nan"]
QUERY_POISONS = ["q_nan_pos", "q_nan_neg", "q_pinf", "q_ninf", "q_3e38", "q_all"]
BOOK_POISONS = ["cb_nan_pos", "cb_nan_neg", "cb_pinf", "cb_ninf", "cb_all", "denormal"]
F32 = {"nan_pos": nf.NAN_POS, "nan_neg": nf.NAN_NEG, "pinf": 0x7F800000, "ninf": 0xFF800000,
       "3e38": int(np.array([3e38], dtype=np.float32).view(np.uint32)[0])}         # finite; 2 * q overflows


def _poisoned(poison, n, m, nq, K):
    """-> dict(codes, cb, nrm, Qd, X, R, rotated_differs): Qd goes to the entry points without a rotation, (X, R) to the others."""
    ties = poison == "nrm_wide_one_nan"
    cb, X, codes, nrm, R, Qd = (a.copy() for a in _base(n, m, nq, ties))
    rotated_differs = False
    if poison.startswith("nrm_"):
        kind = poison[4:]
        if kind in F32:
            nf.put_bits(nrm, _some_rows(n, 0), F32[kind])
        elif kind == "all":
            for part, k in enumerate(("nan_pos", "nan_neg", "pinf", "ninf")):
                nf.put_bits(nrm, _some_rows(n, part), F32[k])
        elif kind == "wide_one_nan":           # non-negative norms 0 .. 1e6 and one clear-sign NaN: the understated-A case
            nrm = (np.random.default_rng(5).random(n) * 1e6).astype(np.float32)
            nrm[::1000] = 0.0
            nf.put_bits(nrm, n // 3, nf.NAN_POS)
        elif kind == "few_left":               # fewer than K rows keep a distance: padded lists
            keep = np.random.default_rng(6).choice(n, size=max(1, (K * 3) // 5), replace=False)
            bad = np.ones(n, bool)
            bad[keep] = False
            nf.put_bits(nrm, np.flatnonzero(bad)[0::2], nf.NAN_POS)
            nf.put_bits(nrm, np.flatnonzero(bad)[1::2], nf.NAN_NEG)
        elif kind == "all_nan":
            nf.put_bits(nrm, np.arange(0, n, 2), nf.NAN_POS)
            nf.put_bits(nrm, np.arange(1, n, 2), nf.NAN_NEG)
        else:
            raise KeyError(poison)
    elif poison.startswith("q_"):
        kind = poison[2:]
        rotated_differs = True                 # a poisoned coordinate of X spreads over the whole rotated query
        for arr in (Qd, X):
            if kind in F32:
                for q, c in SLOTS:
                    nf.put_bits(arr, (q, c), F32[kind])
            else:
                assert kind == "all"
                for (q, c), k in zip(SLOTS + ((5, 7), (10, 2)), ("nan_pos", "pinf", "ninf", "3e38", "nan_neg")):
                    nf.put_bits(arr, (q, c), F32[k])
    elif poison.startswith("cb_"):
        kind = poison[3:]
        entries = {"nan_pos": (2 * H + 77, 1), "nan_neg": (0 * H + 5, D - 1), "pinf": ((m - 1) * H + 3, 0), "ninf": (1 * H + 200, 9)}
        for k in ([kind] if kind in F32 else ["nan_pos", "nan_neg", "pinf", "ninf"]):
            nf.put_bits(cb, entries[k], F32[k])
    else:
        assert poison == "denormal"            # codebooks and queries scaled so that every table entry is a denormal number
        s = np.float32(2e-21)
        cb *= s
        X *= s
        from oracle import oracle
        Qd = oracle.rotate_T(R, X)             # (rotating the scaled queries is not scaling the rotated ones, bit for bit)
        nrm = (nrm * np.float32(1e-42)).astype(np.float32)
        assert (nrm[nrm != 0] < 1.17e-38).all()
    return dict(codes=codes, cb=cb, nrm=nrm, Qd=Qd, X=X, R=R, rotated_differs=rotated_differs)


def _eq(got, ref, what):
    assert nf.same(got[0], got[1], ref), (what, nf.first_difference(got[0], got[1], ref))


def _lsq_kernel_name(m, filt):
    mp = 8 if 4 < m <= 8 else m
    return "adc_scan_kernel<%d, true, %s, %s>" % (mp, "true" if filt else "false", "true" if filt and mp == 8 else "false")


def _check_lsq(rq, oracle, poison, n, m, nq, K, force=None, device=False):
    """One poison through every LSQ entry point, filter on and off; `force`: switches that put the case on its path."""
    c = _poisoned(poison, n, m, nq, K)
    codes, cb, nrm, Qd, X, R = c["codes"], c["cb"], c["nrm"], c["Qd"], c["X"], c["R"]
    Cl = [cb[i * H:(i + 1) * H] for i in range(m)]
    ref = nf.scan("lsq", codes, cb, Qd, K, dbnorms=nrm, id_base=1)
    ref_rot = nf.scan("lsq", codes, cb, oracle.rotate_T(R, X), K, dbnorms=nrm, id_base=1) if c["rotated_differs"] else ref
    if poison == "denormal":
        d = ref[0].view(np.float32)
        assert (d != 0).all() and (np.abs(d) < 1.17e-38).all()          # the distances must keep their denormal bits
    if poison == "nrm_few_left":
        assert ((ref[0] == nf.PAD_BITS).sum(1) == K - max(1, (K * 3) // 5)).all()
    if poison == "nrm_all_nan":
        assert (ref[0] == nf.PAD_BITS).all() and (ref[1] == 0).all()
    has_filter = m in (5, 8, 16)
    with switches(**(force or {})):
        if has_filter:
            assert _filter_can_run(n, nq, m, K), "shape does not reach the pre-filter"
        # the legacy symbol, LSQ form
        _eq(rq.linscan_aqd_query_extra_byte(codes, Qd, cb, nrm, K), ref, (poison, "extra_byte"))
        assert _kernel() == _lsq_kernel_name(m, has_filter), _kernel()
        # linscan_lsq with a real rotation
        _eq(rq.linscan_lsq(codes, X, Cl, nrm, R, K), ref_rot, (poison, "linscan_lsq"))
        # a prepared base, two searches on one handle (the second with the rotation)
        out = (C.c_int * 16)()
        assert _L().lib().rq_order_plan(n, 8 if m == 5 else m, out, 12) == 0
        assert (out[8] > 0) == (n >= 65536)                              # the handle holds its rows (and norms) in bank-aware order
        with rq.LsqIndex(codes, Cl, nrm) as ix:
            _eq(ix.search(Qd, None, K), ref, (poison, "LsqIndex"))
            assert _kernel() == _lsq_kernel_name(m, has_filter), _kernel()
            _eq(ix.search(X, R, K), ref_rot, (poison, "LsqIndex + R"))
        if has_filter:
            with switches(SCAN_FILTER_LSQ=0):
                _eq(rq.linscan_aqd_query_extra_byte(codes, Qd, cb, nrm, K), ref, (poison, "extra_byte, filter off"))
                assert _kernel() == _lsq_kernel_name(m, False), _kernel()
                with rq.LsqIndex(codes, Cl, nrm) as ix:
                    _eq(ix.search(X, R, K), ref_rot, (poison, "LsqIndex + R, filter off"))
        if device:
            _check_device(codes, cb, Qd, nrm, K, poison)


def _check_device(codes, cb, Q, nrm, K, poison, id_offset=1000):
    """rq_dev_linscan_aq: keys out with an id offset (padding must be KEY_MAX exactly), and dists / ids with id_base 1."""
    import torch
    from rayuela_jl_amd import device as rqd
    kind = "cq" if nrm is None else "lsq"
    bits, ids, keys = nf.scan(kind, codes, cb, Q, K, dbnorms=nrm, id_base=1, id_offset=id_offset, want_keys=True)
    cd, bd, qd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (codes, cb, Q))
    nd = None if nrm is None else torch.from_numpy(nrm).cuda()
    got = rqd.linscan_aq(cd, bd, qd, K, dbnorms=nd, id_offset=id_offset, want_keys=True).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, keys), (poison, "keys", np.argwhere(got != keys)[:1])
    assert ((got == nf.KEY_MAX) == (bits == nf.PAD_BITS)).all()
    dd, ii = rqd.linscan_aq(cd, bd, qd, K, dbnorms=nd, id_offset=id_offset, id_base=1)
    _eq((dd.cpu().numpy(), ii.cpu().numpy()), (bits, ids), (poison, "device"))


# ---- LSQ: every poison, m = 8 with K = 1000 and m = 16 with K = 10 (both run the norm pre-filter) ----------------------------
# K = 1000 on 200 000 rows: the planner would cut the base into 5 slices of 40 960 rows, below the filter's 64 K rows per
# item; SCAN_SLICES = 1 keeps the base whole (_filter_can_run asserts it).
CONFIGS = [(8, 29, 1000, {"SCAN_SLICES": 1}), (16, 21, 10, None)]


@pytest.mark.parametrize("m,nq,K,force", CONFIGS, ids=["m8-K1000", "m16-K10"])
@pytest.mark.parametrize("poison", NORM_POISONS + QUERY_POISONS + BOOK_POISONS)
def test_lsq_poisons(rq, oracle, poison, m, nq, K, force):
    _check_lsq(rq, oracle, poison, N, m, nq, K, force=force,
               device=poison in ("nrm_all", "nrm_few_left", "nrm_all_nan", "q_all", "cb_all"))


# ---- the groups together at the other (m, K) pairs, the padded width, the width without the filter, the large-k finish, the short base
@pytest.mark.parametrize("poison", ["nrm_all", "nrm_wide_one_nan", "q_all", "cb_all"])
@pytest.mark.parametrize("n,m,nq,K,force", [
    (N, 8, 29, 10, None),
    (N, 16, 21, 1000, {"SCAN_SLICES": 1}),
    (N, 5, 13, 10, None),                      # padded to the 8-byte tiling: three zero tables
    (N, 4, 13, 10, None),                      # no LSQ pre-filter at this width
], ids=["m8-K10", "m16-K1000", "m5", "m4"])
def test_lsq_poison_groups_other_shapes(rq, oracle, poison, n, m, nq, K, force):
    _check_lsq(rq, oracle, poison, n, m, nq, K, force=force, device=(m == 8))


@pytest.mark.parametrize("poison", ["nrm_all", "nrm_few_left", "q_all", "cb_all"])
def test_lsq_poisons_sample_sort_finish(rq, oracle, poison):
    """K = 4096: the sample-sort finish of the candidate lists (and, with SCAN_SS_MIN_K above it, the bitonic one)."""
    n, m, nq, K = N, 8, 13, 4096
    assert _plan(n, nq, m, K)["bigk"] == 1
    c = _poisoned(poison, n, m, nq, K)
    ref = nf.scan("lsq", c["codes"], c["cb"], c["Qd"], K, dbnorms=c["nrm"], id_base=1)
    _eq(rq.linscan_aqd_query_extra_byte(c["codes"], c["Qd"], c["cb"], c["nrm"], K), ref, (poison, "sample sort"))
    with switches(SCAN_SS_MIN_K=8192):
        assert _plan(n, nq, m, K)["bigk"] == 0
        _eq(rq.linscan_aqd_query_extra_byte(c["codes"], c["Qd"], c["cb"], c["nrm"], K), ref, (poison, "bitonic"))


@pytest.mark.parametrize("poison", ["nrm_all", "nrm_all_nan", "q_all", "cb_all"])
def test_lsq_poisons_short_base(rq, oracle, poison):
    """n = 3000: no sampled threshold (fewer than 32 rows per thread), every row meets tau = +Inf."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, nq, K = 3000, 8, 13, 50
    c = _poisoned(poison, n, m, nq, K)
    ref = nf.scan("lsq", c["codes"], c["cb"], c["Qd"], K, dbnorms=c["nrm"], id_base=1)
    _eq(rq.linscan_aqd_query_extra_byte(c["codes"], c["Qd"], c["cb"], c["nrm"], K), ref, (poison, "extra_byte"))
    Cl = [c["cb"][i * H:(i + 1) * H] for i in range(m)]
    with rq.LsqIndex(c["codes"], Cl, c["nrm"]) as ix:
        _eq(ix.search(c["Qd"], None, K), ref, (poison, "LsqIndex"))
    with switches(SCAN_STATS=1):
        _L().scan_stats()
        cd, bd, qd, nd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["codes"], c["cb"], c["Qd"], c["nrm"]))
        dd, ii = rqd.linscan_aq(cd, bd, qd, K, dbnorms=nd, id_base=1)
        torch.cuda.synchronize()
        assert _L().scan_stats()["sample_rows"] == 0                      # the sampling phase never ran
    _eq((dd.cpu().numpy(), ii.cpu().numpy()), ref, (poison, "device"))


# ---- CQ: queries and codebooks (there are no norms); the pre-filter on / off, the in-call row order on / off ------------------
@pytest.mark.parametrize("m,nq,K,force", [(8, 29, 1000, {"SCAN_SLICES": 1}), (16, 21, 10, None), (4, 13, 10, None)],
                         ids=["m8-K1000", "m16-K10", "m4-K10"])
@pytest.mark.parametrize("poison", QUERY_POISONS + BOOK_POISONS)
def test_cq_poisons(rq, poison, m, nq, K, force):
    c = _poisoned(poison, N, m, nq, K)
    codes, cb, Qd = c["codes"], c["cb"], c["Qd"]
    ref = nf.scan("cq", codes, cb, Qd, K, id_base=1)
    L = _L()
    with switches(**(force or {})):
        assert _filter_can_run(N, nq, m, K)
        assert L.lib().rq_scan_orders_in_call(N, nq, K) == 0
        _eq(rq.linscan_aqd_query_extra_byte(codes, Qd, cb, None, K), ref, (poison, "cq"))
        assert _kernel() == "adc_scan_kernel<%d, false, true, false>" % m, _kernel()
        with switches(SCAN_FILTER=0):
            _eq(rq.linscan_aqd_query_extra_byte(codes, Qd, cb, None, K), ref, (poison, "cq, filter off"))
            assert _kernel() == "adc_scan_kernel<%d, false, false, false>" % m, _kernel()
        # the in-call row order forced on: the call orders a scratch copy of the base and scans that
        L.check(L.lib().rq_release_workspaces())
        with switches(ORDER_MIN_NQ=1):
            assert L.lib().rq_scan_orders_in_call(N, nq, K) == 1
            before = L.order_cache_stats()
            _eq(rq.linscan_cq(codes, Qd, [cb[i * H:(i + 1) * H] for i in range(m)], K), ref, (poison, "cq, in-call order"))
            after = L.order_cache_stats()
            assert after["plain_builds"] + after["balanced_builds"] + after["uncached"] > \
                before["plain_builds"] + before["balanced_builds"] + before["uncached"], (before, after)
            if poison in ("q_all", "cb_all"):
                _check_device(codes, cb, Qd, None, K, poison)
        L.check(L.lib().rq_release_workspaces())


# ---- the encoders' promise: "non-finite inputs give unspecified but in-range codes" (rq_encode_icm, rq_quantize_chainq,
# rq_encode_rvq), and rows are encoded independently of each other -- a clean row gets the code it gets when the poisoned rows
# hold zeros instead (same row count and positions, so the per-row random streams of the ILS perturbations are the same) --------
ENC_N, ENC_D, ENC_H = 4001, 24, 256
BAD_ROWS = {0: ("nan_pos", 3), 17: ("pinf", 0), 63: ("ninf", ENC_D - 1), 64: ("nan_neg", 5), 2000: ("3e38", 7), ENC_N - 1: ("nan_pos", 1)}


def _enc_data(m, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((ENC_N, ENC_D)).astype(np.float32)
    Cs = (rng.standard_normal((m, ENC_H, ENC_D)) * 0.5).astype(np.float32)
    B0 = rng.integers(0, ENC_H, size=(ENC_N, m)).astype(np.uint8)
    Xbad, Xzero = X.copy(), X.copy()
    for row, (kind, col) in BAD_ROWS.items():
        Xzero[row] = 0.0
        Xbad[row] = 0.0
        nf.put_bits(Xbad, (row, col), F32[kind])
    Xbad[64, :] = np.nan                                   # one row that is NaN throughout
    clean = np.ones(ENC_N, bool)
    clean[list(BAD_ROWS)] = False
    return Xbad, Xzero, Cs, B0, clean


def _enc_same(bad, zero, clean, h, what):
    assert bad.dtype == np.uint8 and int(bad.max()) < h, what          # in range (h = 256: by the type; the call returned)
    diff = np.flatnonzero((bad[clean] != zero[clean]).any(axis=1))
    assert diff.size == 0, (what, "%d clean rows changed their codes" % diff.size)


@pytest.mark.parametrize("m", [4, 8])
@pytest.mark.parametrize("npert", [0, 2])
def test_encode_icm_non_finite_rows(rq, m, npert):
    from rayuela_jl_amd.LSQ import encode_icm_u8
    Xbad, Xzero, Cs, B0, clean = _enc_data(m, seed=70 + m)
    args = (2, 2, npert, True)
    bad, cost_bad = encode_icm_u8(Xbad, B0, Cs, *args, seed=5, nsplits=2, with_cost=True)        # check(): RQ_OK
    zero, cost_zero = encode_icm_u8(Xzero, B0, Cs, *args, seed=5, nsplits=2, with_cost=True)
    _enc_same(bad, zero, clean, ENC_H, ("icm", m, npert))
    assert np.array_equal(cost_bad[clean].view(np.uint32), cost_zero[clean].view(np.uint32))


@pytest.mark.parametrize("m", [4, 8])
def test_quantize_chainq_non_finite_rows(rq, m):
    from rayuela_jl_amd.ChainQ import quantize_chainq_u8
    Xbad, Xzero, Cs, _, clean = _enc_data(m, seed=80 + m)
    _enc_same(quantize_chainq_u8(Xbad, Cs, nsplits=2), quantize_chainq_u8(Xzero, Cs, nsplits=2), clean, ENC_H, ("chainq", m))


@pytest.mark.parametrize("m", [4, 8])
def test_quantize_rvq_non_finite_rows(rq, m):
    Xbad, Xzero, Cs, _, clean = _enc_data(m, seed=90 + m)
    C = [Cs[i] for i in range(m)]
    bad, cnt_bad, _ = rq.quantize_rvq_u8(Xbad, C, with_extras=True)
    zero, cnt_zero, res_zero = rq.quantize_rvq_u8(Xzero, C, with_extras=True)
    _enc_same(bad, zero, clean, ENC_H, ("rvq", m))
    assert int(cnt_bad.sum()) == m * ENC_N                 # every row was counted once per stage, the poisoned ones included
    # a smaller codebook: the range is no longer the type's
    C64 = [c[:64] for c in C]
    bad64, cnt64, _ = rq.quantize_rvq_u8(Xbad, C64, with_extras=True)
    _enc_same(bad64, rq.quantize_rvq_u8(Xzero, C64), clean, 64, ("rvq h=64", m))
    assert int(cnt64.sum()) == m * ENC_N


@pytest.mark.parametrize("h", [16, 17, 27])
@pytest.mark.parametrize("m", [4, 8])
def test_quantize_rvq_non_finite_rows_small_h(rq, m, h):
    """h < 28: where a stage encode whose distances are all NaN used to answer 27 (rq_encode_split.h, argmin_finish) and the
    stage epilogue then read the codebook and bumped the counts at that index.  The counts and the codebooks sit inside
    guard-filled device buffers of the test's own, so a stray atomic add or read stays in memory the test owns and shows as
    a changed guard word or a changed code."""
    import torch
    Xbad, Xzero, Cs, _, clean = _enc_data(m, seed=90 + m)
    Ch = np.ascontiguousarray(Cs[:, :h])
    G, GUARD_I, GUARD_F = 4096, 0x5A5A5A5A, 12345.0
    lib = _L().lib()

    def run(X):
        cbuf = torch.full((2 * G + m * h,), GUARD_I, dtype=torch.int32, device="cuda")
        bbuf = torch.full((2 * G + Ch.size,), GUARD_F, dtype=torch.float32, device="cuda")
        bbuf[G:G + Ch.size] = torch.from_numpy(Ch.reshape(-1)).cuda()
        codes = torch.full((ENC_N, m), 0xEE, dtype=torch.uint8, device="cuda")
        Xr = torch.from_numpy(np.ascontiguousarray(X)).cuda()
        _L().check(lib.rq_dev_encode_rvq(codes.data_ptr(), Xr.data_ptr(), bbuf[G:].data_ptr(), ENC_N, ENC_D, m, h,
                                         cbuf[G:].data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert bool((cbuf[:G] == GUARD_I).all()) and bool((cbuf[G + m * h:] == GUARD_I).all()), "a count landed outside [m][h]"
        assert bool((bbuf[:G] == GUARD_F).all()) and bool((bbuf[G + Ch.size:] == GUARD_F).all())
        return codes.cpu().numpy(), cbuf[G:G + m * h].cpu().numpy().reshape(m, h)
    bad, cnt_bad = run(Xbad)
    zero, cnt_zero = run(Xzero)
    _enc_same(bad, zero, clean, h, ("rvq", m, h))
    assert int(cnt_bad.sum()) == m * ENC_N and (cnt_bad.sum(axis=1) == ENC_N).all()
    assert np.array_equal(cnt_bad, np.stack([np.bincount(bad[:, i], minlength=h) for i in range(m)]))
    assert np.array_equal(cnt_zero, np.stack([np.bincount(zero[:, i], minlength=h) for i in range(m)]))
    # the first stage of the row that is NaN throughout: every distance NaN, code 0 (the oracle's answer)
    assert bad[64, 0] == 0
