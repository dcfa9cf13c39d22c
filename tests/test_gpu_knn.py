"""GPU: the exact k-nearest-neighbour entries (rq_knn_f32, rq_knn, rq_knn_bytes, rq_dataset_knn) against
their numpy restatement tests/knn_oracle.py, bit for bit: stage 1 against the (D32, id) order, the ground truth against the
(D64, id) order -- on shapes where the tiling can go wrong (n no multiple of the 128-row tile, nq of the 64-query tile, d of the
32-dimension stage), on near-ties that float32 alone gets wrong, on duplicates, across row chunks, on byte bases at every load
width, on non-finite inputs, and through the experiment drivers.  References are computed once per (d, n) and shared read-only."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_oracle as ko
import nonfinite_ref as nf

gpu = pytest.mark.gpu
DS = (1, 6, 30, 96, 128, 131)
NS = (1, 63, 1000)
NQS = (1, 5, 70)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _data(d, n):
    """Base, 70 queries (the smaller query counts are prefixes) and both distance matrices, made once."""
    rng = np.random.default_rng(100 * d + n)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((70, d)).astype(np.float32)
    return _ro(X, Q, ko.d32(X, Q), ko.d64(X, Q))


def _ks(n):
    return sorted({k for k in (1, 10, n) if k <= n})


def _same64(got, ref):
    """(ids, dists) of groundtruth(one_based=False) against the oracle's (dists, ids), bit for bit."""
    ids, dists = got
    return (dists.dtype == np.float64 and ids.dtype == np.int32 and dists.shape == ref[0].shape and
            np.array_equal(dists.view(np.uint64), ref[0].view(np.uint64)) and np.array_equal(ids.view(np.uint32), ref[1]))


def _first_bad64(got, ref):
    ids, dists = got
    bad = np.argwhere((dists.view(np.uint64) != ref[0].view(np.uint64)) | (ids.view(np.uint32) != ref[1]))
    if bad.size == 0:
        return None
    q, r = (int(x) for x in bad[0])
    return q, r, (float(dists[q, r]), int(ids[q, r])), (float(ref[0][q, r]), int(ref[1][q, r])), int(bad.shape[0])


# ---- 1. stage 1 -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_stage1_equals_the_f32_order_bit_for_bit(rq, d, n, nq):
    X, Q, D32, _ = _data(d, n)
    for k in _ks(n):
        dists, ids = rq.knn_f32(X, Q[:nq], k)
        ref = ko.topk_f32(D32[:nq], k)
        assert nf.same(dists, ids, ref[:2]), (k, nf.first_difference(dists, ids, ref[:2]))
    dists, ids = rq.knn_f32(X, Q[:nq], 1, id_base=1)
    assert nf.same(dists, ids, ko.topk_f32(D32[:nq], 1, id_base=1)[:2])


@gpu
def test_stage1_equals_linscan_cq_over_identity_codes(rq):
    """The second oracle: the base as ONE codebook of n entries, codes 0..n-1 -- linscan_cq's table is D32."""
    X, Q, D32, _ = _data(96, 1000)
    codes = np.arange(1000, dtype=np.uint16).reshape(-1, 1)
    for k in (1, 10, 1000):
        d0, i0 = rq.linscan_cq_u16(codes, Q, [X], k)                 # one-based ids
        d1, i1 = rq.knn_f32(X, Q, k, id_base=1)
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(i0, i1), k


# ---- 2. the ground truth ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_groundtruth_equals_the_f64_order_bit_for_bit(rq, d, n, nq):
    X, Q, _, D64 = _data(d, n)
    for k in _ks(n):
        got = rq.groundtruth(X, Q[:nq], k, one_based=False)
        ref = ko.topk_f64(D64[:nq], k)
        assert _same64(got, ref), (k, _first_bad64(got, ref))
    got = rq.groundtruth(X, Q[:nq], 1)
    assert _same64(got, ko.topk_f64(D64[:nq], 1, id_base=1))


@gpu
@pytest.mark.parametrize("kind", ["sift_like", "deep_like"])
def test_groundtruth_on_synthetic_rows(rq, kind):
    from rayuela_jl_amd import synth
    d = 128 if kind == "sift_like" else 96
    X, Q = getattr(synth, kind)(1000, d, seed=11), getattr(synth, kind)(20, d, seed=12)
    D64 = ko.d64(X, Q)
    for k in (1, 10, 100):
        got = rq.groundtruth(X, Q, k, one_based=False)
        ref = ko.topk_f64(D64, k)
        assert _same64(got, ref), (k, _first_bad64(got, ref))


@gpu
@pytest.mark.parametrize("d", [30, 96, 131])
def test_groundtruth_on_near_ties_widens_and_stays_exact(rq, d):
    X, Q = ko.near_tie(d)
    D32, D64 = ko.d32(X, Q), ko.d64(X, Q)
    k = 10
    got = rq.groundtruth(X, Q, k, one_based=False)
    st = rq.last_knn_stats()
    ref = ko.topk_f64(D64, k)
    assert _same64(got, ref), _first_bad64(got, ref)
    need = [ko.candidates_needed(D32[q], D64[q], k, d) for q in range(Q.shape[0])]
    print("d=%d stats %s; the oracle's widened queries: %d, rounds %d" % (d, st, sum(r > 0 for _, r in need), max(r for _, r in need)))
    assert st["widened"] > 0 and st["host_finished"] == 0 and st["queries"] == Q.shape[0]
    assert st["widened"] == sum(r > 0 for _, r in need) and st["rounds"] == max(r for _, r in need)
    # float32 alone is wrong here: the test is not vacuous
    ids32 = rq.knn_f32(X, Q, k)[1]
    assert int((ids32 != ref[1]).any(axis=1).sum()) * 2 >= Q.shape[0]


# ---- 3. duplicates ------------------------------------------------------------------------------------------------------------------
@gpu
def test_identical_rows_finish_on_the_host_with_the_lowest_ids(rq):
    rng = np.random.default_rng(5)
    X = np.repeat(rng.standard_normal((1, 6)).astype(np.float32), 5000, axis=0)
    Q = rng.standard_normal((3, 6)).astype(np.float32)
    ids, dists = rq.groundtruth(X, Q, 10, one_based=False)
    st = rq.last_knn_stats()
    assert np.array_equal(ids, np.tile(np.arange(10, dtype=np.int32), (3, 1)))
    assert _same64((ids, dists), ko.groundtruth(X, Q, 10))
    assert st["host_finished"] == 3 and st["widened"] == 3, st


@gpu
def test_duplicates_among_random_rows_give_the_lowest_ids(rq):
    rng = np.random.default_rng(6)
    X = rng.standard_normal((1000, 30)).astype(np.float32)
    dup = np.sort(rng.choice(1000, 300, replace=False))
    X[dup] = X[dup[0]]
    Q = np.stack([X[dup[0]], X[dup[0]] + np.float32(1e-3)]).astype(np.float32)
    got = rq.groundtruth(X, Q, 10, one_based=False)
    assert np.array_equal(got[0][0], dup[:10].astype(np.int32)) and np.all(got[1][0] == 0.0)
    assert _same64(got, ko.groundtruth(X, Q, 10))
    assert rq.last_knn_stats()["host_finished"] == 0


# ---- 4. row chunks --------------------------------------------------------------------------------------------------------------------
@gpu
def test_row_chunks_give_the_unchunked_answer(rq):
    from rayuela_jl_amd import knn as K
    X, Q, D32, D64 = _data(30, 1000)
    whole = {k: rq.groundtruth(X, Q, k, one_based=False) for k in (10, 1000)}
    whole32 = {k: rq.knn_f32(X, Q, k) for k in (1, 300, 1000)}
    assert rq.last_knn_stats()["chunks"] == 1
    K.knn_chunk_rows(257)
    try:
        assert K.knn_plan(1000, 70, 30, 10)["chunks"] == 4 and K.knn_plan(1000, 70, 30, 10)["forced"] == 1
        for k, ref in whole.items():
            got = rq.groundtruth(X, Q, k, one_based=False)
            assert rq.last_knn_stats()["chunks"] == 4
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), k
            assert _same64(got, ko.topk_f64(D64, k)), k
        for k, ref in whole32.items():                    # 300 and 1000: more candidates than a chunk has rows
            got = rq.knn_f32(X, Q, k)
            assert rq.last_knn_stats()["chunks"] == 4
            assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1], ref[1]), k
            assert nf.same(got[0], got[1], ko.topk_f32(D32, k)[:2]), k
    finally:
        K.knn_chunk_rows(0)
    assert K.knn_plan(1000, 70, 30, 10)["forced"] == 0


# ---- 5. byte bases ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", [128, 30, 131])             # 4-, 2- and 1-byte loads of an aligned base
@pytest.mark.parametrize("offset", [0, 1])                # ... and a base that starts on an odd address
def test_byte_base_equals_the_widened_rows(rq, d, offset):
    rng = np.random.default_rng(7 + d)
    n, nq, k = 1000, 70, 10
    buf = rng.integers(0, 256, n * d + 1, dtype=np.uint8)
    Xu = buf[offset:offset + n * d].reshape(n, d)
    assert Xu.ctypes.data % 2 == offset % 2
    Q = (rng.integers(0, 256, (nq, d)) + rng.standard_normal((nq, d))).astype(np.float32)
    ref = rq.knn_f64(Xu.astype(np.float32), Q, k)
    got = rq.knn_f64(Xu, Q, k)
    assert np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)) and np.array_equal(got[1], ref[1])
    with rq.Dataset(Xu) as ds:
        res = ds.knn(Q, k)
        ids1, d1 = rq.groundtruth(ds, Q, k)
    assert np.array_equal(res[0].view(np.uint64), ref[0].view(np.uint64)) and np.array_equal(res[1], ref[1])
    assert np.array_equal(ids1.view(np.uint32), ref[1] + 1)
    want = ko.groundtruth(Xu, Q, k)
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1])


@gpu
def test_resident_f32_dataset(rq):
    X, Q, _, D64 = _data(96, 1000)
    with rq.Dataset(X) as ds:
        dists, ids = ds.knn(Q, 10, id_base=1)
    ref = ko.topk_f64(D64, 10, id_base=1)
    assert np.array_equal(dists.view(np.uint64), ref[0].view(np.uint64)) and np.array_equal(ids, ref[1])


# ---- 6. non-finite inputs ---------------------------------------------------------------------------------------------------------------
def _nonfinite_cases():
    rng = np.random.default_rng(8)
    n, d, nq = 200, 6, 5
    X0 = rng.standard_normal((n, d)).astype(np.float32)
    Q0 = rng.standard_normal((nq, d)).astype(np.float32)
    X = X0.copy(); X[3, 2] = np.nan; X[150, 0] = np.nan
    yield "nan_in_rows", X, Q0, 10
    Q = Q0.copy(); Q[1, 4] = np.nan
    yield "nan_in_a_query", X0, Q, 10
    X = X0.copy(); X[7, 1] = np.inf; X[8, 5] = -np.inf; X[9, 0] = np.inf
    Q = Q0.copy(); Q[2, 0] = np.inf                      # Inf - Inf at row 9: a NaN distance
    yield "inf_in_rows", X, Q, 10
    yield "inf_in_rows_full_list", X, Q, n
    X = X0.copy(); X[5:, 3] = np.nan                      # five comparable rows
    yield "k_above_the_comparable_rows", X, Q0, 10
    X = (X0.astype(np.float64) * 1e19).astype(np.float32)
    Q = (Q0.astype(np.float64) * 1e19).astype(np.float32)
    yield "f32_overflow", X, Q, 10
    X = X0.copy(); X[:, :] = np.float32(-0.0)
    yield "negative_zero", X, np.zeros_like(Q0), 10


@gpu
@pytest.mark.parametrize("name", [c[0] for c in _nonfinite_cases()])
def test_non_finite_inputs_follow_the_contract(rq, name):
    X, Q, k = next(c[1:] for c in _nonfinite_cases() if c[0] == name)
    D32, D64 = ko.d32(X, Q), ko.d64(X, Q)
    if name == "f32_overflow":
        assert np.isinf(D32).sum() > D32.size // 2 and np.isfinite(D64).all()
    dists, ids = rq.knn_f32(X, Q, k, id_base=1)
    ref32 = ko.topk_f32(D32, k, id_base=1)
    assert nf.same(dists, ids, ref32[:2]), nf.first_difference(dists, ids, ref32[:2])
    for id_base in (0, 1):
        got = rq.groundtruth(X, Q, k, one_based=bool(id_base))
        ref = ko.topk_f64(D64, k, id_base=id_base)
        assert _same64(got, ref), (id_base, _first_bad64(got, ref))


# ---- 7. errors: checked before any work, no output byte written (no device needed) ----------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched(rq):
    L = rq.lib()
    n, nq, d, k = 40, 3, 6, 5
    X = np.zeros((n, d), np.float32)
    Xu = np.zeros((n, d), np.uint8)
    Q = np.zeros((nq, d), np.float32)
    d64 = np.full((nq, 2048), 7.5, np.float64)
    d32 = np.full((nq, 2048), 7.5, np.float32)
    ids = np.full((nq, 2048), 0xABCDEF01, np.uint32)
    p = lambda a: a.ctypes.data                           # noqa: E731
    EINVAL, EUNSUPPORTED = -1, -2
    entries = [("rq_knn_f32", d32, X), ("rq_knn", d64, X), ("rq_knn_bytes", d64, Xu)]
    for name, dd, base in entries:
        fn = getattr(L, name)
        cases = [
            (EINVAL, (None, p(ids), p(base), p(Q), n, nq, d, k, 0)),
            (EINVAL, (p(dd), None, p(base), p(Q), n, nq, d, k, 0)),
            (EINVAL, (p(dd), p(ids), None, p(Q), n, nq, d, k, 0)),
            (EINVAL, (p(dd), p(ids), p(base), None, n, nq, d, k, 0)),
            (EINVAL, (p(dd), p(ids), p(base), p(Q), n, nq, d, 0, 0)),
            (EINVAL, (p(dd), p(ids), p(base), p(Q), n, nq, d, n + 1, 0)),
            (EINVAL, (p(dd), p(ids), p(base), p(Q), n, nq, d, k, 2)),
            (EINVAL, (p(dd), p(ids), p(base), p(Q), n, nq, d, k, -1)),
            (EINVAL, (p(dd), p(ids), p(base), p(Q), n, nq, 0, k, 0)),
            (EINVAL, (p(dd), p(ids), p(base), p(Q), 1 << 31, nq, d, k, 0)),
            (EINVAL, (p(dd), p(ids), p(base), p(Q), 0, nq, d, k, 0)),
        ]
        if name != "rq_knn_f32":
            cases.append((EUNSUPPORTED, (p(dd), p(ids), p(base), p(Q), 1 << 20, nq, d, 1025, 0)))
        for want, args in cases:
            assert fn(*args) == want, (name, args[4:], L.rq_last_error())
            assert L.rq_last_error() != b""
        assert fn(p(dd), p(ids), p(base), p(Q), n, 0, d, k, 0) == 0          # nq <= 0: nothing to do
        assert fn(None, None, None, None, n, -1, d, k, 0) == 0
    assert L.rq_dataset_knn(None, p(d64), p(ids), p(Q), nq, k, 0) == EINVAL
    assert L.rq_last_knn_stats(None) == EINVAL and L.rq_last_knn_timing(None, 7) == EINVAL
    out = (C.c_int64 * 6)()
    assert L.rq_knn_plan(n, nq, d, k, None, 6) == EINVAL and L.rq_knn_plan(n, nq, d, k, C.cast(out, C.c_void_p), 5) == EINVAL
    assert np.all(d64 == 7.5) and np.all(d32 == 7.5) and np.all(ids == 0xABCDEF01)


def test_plan_is_host_only_and_keeps_one_query_inside_the_budget():
    from rayuela_jl_amd import knn as K
    p = K.knn_plan(1_000_000, 10_000, 128, 100)
    assert p["candidates"] == 132 and p["chunks"] == 1 and p["chunk_rows"] == 1_000_000 and p["forced"] == 0
    assert p["batch"] >= 64 and p["scratch_bytes"] <= 2 << 30
    p = K.knn_plan((1 << 31) - 1, 1000, 128, 1000)
    assert p["candidates"] == 1250 and p["chunks"] > 1 and p["chunk_rows"] * p["chunks"] >= (1 << 31) - 1
    assert p["batch"] >= 64 and p["scratch_bytes"] <= 2 << 30                # no more scratch than a 1e6-row base may take
    assert K.knn_plan(10, 1, 3, 10)["candidates"] == 10                       # k' is capped at n


@gpu
def test_bad_arguments_of_the_resident_form(rq):
    X, Q, _, _ = _data(6, 63)
    d64 = np.full((70, 2048), 7.5, np.float64)
    ids = np.full((70, 2048), 0xABCDEF01, np.uint32)
    L = rq.lib()
    with rq.Dataset(X) as ds:
        for want, (k, id_base, qp) in [(-1, (0, 0, Q.ctypes.data)), (-1, (64, 0, Q.ctypes.data)), (-1, (5, 3, Q.ctypes.data)),
                                       (-1, (5, 0, None))]:
            assert L.rq_dataset_knn(ds._h, d64.ctypes.data, ids.ctypes.data, qp, 70, k, id_base) == want
        assert L.rq_dataset_knn(ds._h, None, ids.ctypes.data, Q.ctypes.data, 70, 5, 0) == -1
    big = np.zeros((1100, 2), np.float32)
    with rq.Dataset(big) as ds:
        assert L.rq_dataset_knn(ds._h, d64.ctypes.data, ids.ctypes.data, big.ctypes.data, 4, 1025, 0) == -2
    assert np.all(d64 == 7.5) and np.all(ids == 0xABCDEF01)


# ---- 8. scratch independence ------------------------------------------------------------------------------------------------------------
@gpu
def test_answer_does_not_depend_on_what_scratch_held(rq):
    from rayuela_jl_amd import _lib
    X, Q = ko.near_tie(30)
    ref = ko.groundtruth(X, Q, 10)
    ref32 = ko.topk_f32(ko.d32(X, Q), 10)
    rq.groundtruth(X, Q, 10)                               # the scratch exists: the fills below reach it
    for value in (0xFF, 0x00):
        assert _lib.fill_scratch(value)["slot_bytes"] > 0
        got = rq.groundtruth(X, Q, 10, one_based=False)
        assert _same64(got, ref), (value, _first_bad64(got, ref))
        _lib.fill_scratch(value)
        dists, ids = rq.knn_f32(X, Q, 10)
        assert nf.same(dists, ids, ref32[:2]), value


# ---- 9. the drivers ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_experiment_pq_computes_the_ground_truth_it_is_not_given(rq):
    from rayuela_jl_amd import synth
    from rayuela_jl_amd.experiments import experiment_pq, experiment_pq_query_base
    Xb = synth.sift_like(2000, 128, seed=21)
    Xq = synth.sift_like(50, 128, seed=22)
    gt = ko.groundtruth(Xb, Xq, 1, id_base=1)[1][:, 0]
    with_gt = experiment_pq(Xb, Xb, Xq, gt, 8, 256, niter=2, knn=100, seed=3)
    without = experiment_pq(Xb, Xb, Xq, None, 8, 256, niter=2, knn=100, seed=3)
    assert np.array_equal(with_gt[-1], without[-1]) and with_gt[-1][-1] > 0.5
    assert np.array_equal(with_gt[3], without[3])
    a = experiment_pq_query_base(Xb, Xq, gt, 8, 256, niter=2, knn=100, seed=3)
    b = experiment_pq_query_base(Xb, Xq, None, 8, 256, niter=2, knn=100, seed=3)
    assert np.array_equal(a[-1], b[-1])


@gpu
def test_recall_of_the_ground_truth_against_itself_is_one(rq):
    from rayuela_jl_amd import synth
    Xb = synth.deep_like(2000, 96, seed=23)
    Xq = synth.deep_like(40, 96, seed=24)
    gt1 = rq.groundtruth(Xb, Xq, 1)[0]
    gt100 = rq.groundtruth(Xb, Xq, 100)[0]
    recall = rq.eval_recall(gt1, gt100, 100, verbose=False)
    assert recall.shape == (100,) and np.all(recall == 1.0)
    assert gt1.min() >= 1 and gt100.max() <= 2000                           # one-based, as ivecs_write stores them
