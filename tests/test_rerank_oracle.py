"""CPU: the restated re-ranking contract (tests/rerank_oracle.py) against the restatements it is built from, and the planner's
arithmetic against the library's (rq_rerank_plan is host code: no device needed)."""
import ctypes as C

import numpy as np
import pytest

import knn_oracle as ko
import nonfinite_ref as nf
import rerank_oracle as ro

N, D, NQ = 300, 7, 6


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(31)
    X = rng.standard_normal((N, D)).astype(np.float32)
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    X[17] = X[4]                                            # equal distances: the ids decide
    X[200, 3] = np.nan                                      # a row that is never a neighbour
    D32 = ko.d32(X, Q)
    for a in (X, Q, D32):
        a.setflags(write=False)
    return X, Q, D32


def _offsets():
    return (0, 5, (1 << 31) - 5, (1 << 32) - 1 - N)


@pytest.mark.parametrize("id_base", [0, 1])
@pytest.mark.parametrize("k", [1, 10, N])
def test_all_ids_give_the_exact_top_k(data, k, id_base):
    X, Q, D32 = data
    cand = np.tile((np.arange(N, dtype=np.int64) + id_base).astype(np.uint32), (NQ, 1))
    bits, ids = ro.rerank_d(D32, cand, N, k, 0, id_base)
    ref = ko.topk_f32(D32, k, id_base)
    assert np.array_equal(bits, ref[0]) and np.array_equal(ids, ref[1])
    rng = np.random.default_rng(k)
    shuffled = np.stack([rng.permutation(row) for row in cand])
    bits2, ids2 = ro.rerank_d(D32, shuffled, N, k, 0, id_base)
    assert np.array_equal(bits2, bits) and np.array_equal(ids2, ids)          # the order of the candidates is no input


def test_the_entry_point_form_computes_the_distances(data):
    X, Q, D32 = data
    cand = np.tile(np.arange(0, N, 3, dtype=np.uint32), (NQ, 1))
    a = ro.rerank(X, Q, cand, cand.shape[1], 9)
    b = ro.rerank_d(D32, cand, cand.shape[1], 9)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    u8 = (np.abs(np.nan_to_num(X)) * 40).astype(np.uint8)
    a = ro.rerank(u8, Q, cand, cand.shape[1], 9)
    b = ro.rerank(u8.astype(np.float32), Q, cand, cand.shape[1], 9)            # byte rows are widened exactly
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_candidate_given_twice_appears_twice(data):
    X, Q, D32 = data
    cand = np.tile(np.array([9, 3, 9, 250, 3, 9], dtype=np.uint32), (NQ, 1))
    bits, ids = ro.rerank_d(D32, cand, 6, 6)
    for q in range(NQ):
        assert sorted(ids[q].tolist()) == [3, 3, 9, 9, 9, 250]
        order = np.lexsort((ids[q], bits[q].view(np.float32)))
        assert np.array_equal(order, np.arange(6))                             # ascending (distance, id), copies adjacent
    bits, ids = ro.rerank_d(D32, cand, 6, 4)                                   # a cut inside a run of copies keeps whole pairs
    full = ro.rerank_d(D32, cand, 6, 6)
    assert np.array_equal(ids, full[1][:, :4]) and np.array_equal(bits, full[0][:, :4])


def test_equal_distances_order_by_id_and_nan_rows_never_appear(data):
    X, Q, D32 = data
    cand = np.tile(np.array([17, 4, 200, 4], dtype=np.uint32), (NQ, 1))
    bits, ids = ro.rerank_d(D32, cand, 4, 4)
    assert np.array_equal(ids, np.tile(np.array([4, 4, 17, M32_PAD(0)], dtype=np.uint32), (NQ, 1)))
    assert np.all(bits[:, 3] == nf.PAD_BITS) and np.all(bits[:, 0] == bits[:, 2])


def M32_PAD(id_base):
    return (0xFFFFFFFF + id_base) & 0xFFFFFFFF


@pytest.mark.parametrize("id_offset", _offsets())
@pytest.mark.parametrize("id_base", [0, 1])
def test_padding_out_of_range_and_wrapped_ids_are_dropped(data, id_base, id_offset):
    X, Q, D32 = data
    rows = np.array([0, 1, N - 1, 40], dtype=np.int64)
    good = (rows + id_offset + id_base) & 0xFFFFFFFF
    junk = np.array([M32_PAD(id_base),                                        # the scans' padding id
                     (N + id_offset + id_base) & 0xFFFFFFFF,                  # the first id behind the base
                     (id_offset + id_base - 1) & 0xFFFFFFFF,                  # the id in front of row 0 (wraps at offset 0, base 0)
                     (id_offset + id_base + (1 << 31)) & 0xFFFFFFFF], dtype=np.int64)
    junk = junk[ro.rows_of(junk, id_offset, id_base) >= N]                    # (2^31 lies inside no base of 300 rows)
    assert junk.size >= 3
    cand = np.tile(np.concatenate([junk[:2], good, junk[2:]]).astype(np.uint32), (NQ, 1))
    kc = cand.shape[1]
    bits, ids = ro.rerank_d(D32, cand, kc, kc, id_offset, id_base)
    ref = ro.rerank_d(D32, np.tile(good.astype(np.uint32), (NQ, 1)), 4, 4, id_offset, id_base)
    assert np.array_equal(ids[:, :4], ref[1]) and np.array_equal(bits[:, :4], ref[0])
    assert np.all(ids[:, 4:] == M32_PAD(id_base)) and np.all(bits[:, 4:] == nf.PAD_BITS)
    assert set(ids[0, :4].tolist()) == set(int(g) for g in good)
    only_junk = np.tile(junk.astype(np.uint32), (NQ, 1))                      # all candidates invalid: all padding
    bits, ids = ro.rerank_d(D32, only_junk, junk.size, 2, id_offset, id_base)
    assert np.all(ids == M32_PAD(id_base)) and np.all(bits == nf.PAD_BITS)


def test_what_lies_behind_kc_is_never_read(data):
    X, Q, D32 = data
    best = np.argmin(np.where(np.isnan(D32), np.inf, D32), axis=1).astype(np.uint32)
    cand = np.full((NQ, 8), 100, dtype=np.uint32)
    cand[:, 5] = best                                                         # would win if it were read
    bits, ids = ro.rerank_d(D32, cand, 5, 1)
    assert np.all(ids[:, 0] == 100)


def test_the_contract_equals_the_scans_contract_on_a_subset(data):
    X, Q, D32 = data
    sub = np.arange(10, 200, 7)
    cand = np.tile(sub.astype(np.uint32) + 1, (NQ, 1))
    bits, ids = ro.rerank_d(D32, cand, sub.size, 5, 0, 1)
    for q in range(NQ):
        b, i, _ = nf.contract(D32[q, sub], 5, id_base=0)
        assert np.array_equal(bits[q], b) and np.array_equal(ids[q], sub[i] + 1)


# ---- the planner through the library ---------------------------------------------------------------------------------------------
PLAN_SHAPES = [(1, 1, 1), (1000, 100, 10), (10_000, 4096, 409), (10_000, 4097, 409), (10_000, 10_000, 1000), (33, 5000, 5000),
               (100_000, 1000, 100), (50_000, 200_000, 200_000), (7, 1 << 24, 1 << 24), (3, (1 << 27) + 5, 10)]


@pytest.mark.parametrize("nq,kc,k", PLAN_SHAPES)
def test_plan_equals_its_restatement(rq, nq, kc, k):
    from rayuela_jl_amd import knn as K
    assert K.rerank_plan(1_000_000, nq, 128, kc, k) == ro.plan(nq, kc, k)


def test_plan_limits_and_hook(rq):
    from rayuela_jl_amd import knn as K
    p = K.rerank_plan(1_000_000, 10_000, 128, 1000, 100)
    assert p["chain"] == 0 and p["batch"] == 10_000 and p["scratch_bytes"] <= ro.BULK_USABLE
    p = K.rerank_plan(1_000_000, 10_000, 128, 10_000, 1000)
    assert p["chain"] == 1 and 1 <= p["batch"] <= 10_000 and p["scratch_bytes"] <= ro.BULK_USABLE
    assert K.rerank_plan(10, 3, 4, (1 << 28), 1)["batch"] == 0                 # one query's keys do not fit: the entry refuses
    assert K.rerank_limits(64, 5) == (0, 0)
    try:
        assert K.rerank_plan(1000, 33, 8, 100, 10) == ro.plan(33, 100, 10, lds_k=64, batch_queries=5)
        p = K.rerank_plan(1000, 33, 8, 100, 10)
        assert p["chain"] == 1 and p["batch"] == 5 and p["forced"] == 1
        assert K.rerank_plan(1000, 33, 8, 64, 10)["chain"] == 0
        assert K.rerank_limits(1 << 20, 0) == (64, 5)                          # never above what LDS holds
        assert K.rerank_plan(1000, 33, 8, 5000, 10)["chain"] == 1 and K.rerank_plan(1000, 33, 8, 4096, 10)["chain"] == 0
    finally:
        K.rerank_limits(0, 0)
    assert K.rerank_limits(0, 0) == (0, 0)
    L = rq.lib()
    out = (C.c_int64 * 5)()
    po = C.cast(out, C.c_void_p)
    assert L.rq_rerank_plan(10, 1, 4, 5, 2, None, 5) == -1 and L.rq_rerank_plan(10, 1, 4, 5, 2, po, 4) == -1
    for bad in [(0, 1, 4, 5, 2), (10, 0, 4, 5, 2), (10, 1, 0, 5, 2), (10, 1, 4, 5, 0), (10, 1, 4, 1, 2), (10, 1, 4, 1 << 31, 2)]:
        assert L.rq_rerank_plan(*bad, po, 5) == -1, bad
    assert L.rq_last_rerank_stats(None) == -1 and L.rq_last_rerank_timing(None, 4) == -1


def test_argument_checks_need_no_device_and_write_nothing(rq):
    """Every refusal that can be decided without a dataset handle: a NULL dataset, and nq <= 0 on one."""
    L = rq.lib()
    dists = np.full((3, 4), 7.5, np.float32)
    ids = np.full((3, 4), 0xABCDEF01, np.uint32)
    Q = np.zeros((3, 6), np.float32)
    cand = np.zeros((3, 8), np.uint32)
    p = lambda a: a.ctypes.data                           # noqa: E731
    assert L.rq_dataset_rerank(None, p(dists), p(ids), p(Q), 3, p(cand), 8, 8, 4, 0, 0) == -1
    assert L.rq_ivf_search_refine(None, None, p(dists), p(ids), p(Q), 3, 1, 4, 8, 0, 0) == -1
    assert np.all(dists == 7.5) and np.all(ids == 0xABCDEF01)
