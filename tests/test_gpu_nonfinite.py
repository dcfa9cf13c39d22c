"""The ADC scan on non-finite inputs (VERDICT r5 Missing #5).  The reference builds the table and the distances in plain f32
(deps/src/linscan_aqd.cpp:66-87) and hands whatever comes out to std::partial_sort on (float, id) pairs (:91-97): +Inf is an
ordinary value there (ties part by id); a NaN makes the pair comparison no strict weak order, so the reference's answer for
that query is unspecified.  What the HIP path guarantees (include/rayuela_hip.h, "Non-finite inputs"):
  * the call returns (no redo / barrier / pacing path spins on a poisoned group);
  * every query without a NaN distance -- the other queries of the same group and of the same launch -- is bit-identical to the
    reference, +Inf / -Inf distances included;
  * a row whose distance to a query is NaN is never a neighbour of that query; the rows with comparable distances are returned
    exactly, in (dist, id) order, and a list that runs out of them ends in (NaN, id 0xFFFFFFFF zero-based = 0 one-based).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _case(seed, n, m, sub, nq):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    return centers, queries, codes


SHAPES = [
    (300_000, 8, 4, 29, 100),      # sampled threshold + byte pre-filter + second estimate, ragged last group
    (300_000, 8, 4, 29, 1000),
    (120_000, 16, 2, 21, 100),     # m = 16: the 1024-thread kernel
    (40_000, 8, 4, 13, 4096),      # large k: sample-sort finish
    (3_000, 8, 4, 13, 50),         # short base: no sampled threshold
    (200_000, 4, 4, 21, 100),      # m = 4: the pre-filter of round 6
]


@pytest.mark.parametrize("n,m,sub,nq,K", SHAPES)
def test_non_finite_queries(rq, oracle, n, m, sub, nq, K):
    centers, queries, codes = _case(41, n, m, sub, nq)
    bad_nan, bad_pinf, bad_ninf = 3, 9, 12          # three different positions of two groups (8 queries per group)
    queries[bad_nan, 1] = np.nan
    queries[bad_pinf, sub * m - 1] = np.inf
    queries[bad_ninf, 0] = -np.inf
    d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    clean = np.ones(nq, bool)
    clean[bad_nan] = False
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries[clean], K)
    # every query but the NaN one -- the +-Inf ones included: all their distances are +Inf, ties part by id -- equals the reference
    assert np.array_equal(i1[clean], i0) and _eq_bits(d1[clean], d0)
    assert np.all(np.isinf(d1[bad_pinf])) and np.array_equal(i1[bad_pinf], np.arange(K, dtype=np.uint32))
    # the NaN query has no comparable distance at all: K times "no row"
    assert np.all(np.isnan(d1[bad_nan])) and np.all(i1[bad_nan] == 0xFFFFFFFF)


@pytest.mark.parametrize("n,m,sub,nq,K", SHAPES)
def test_non_finite_table_entries(rq, oracle, n, m, sub, nq, K):
    centers, queries, codes = _case(43, n, m, sub, nq)
    centers[2, 77, 1] = np.nan           # rows with code 77 in position 2: NaN distance to every query
    centers[m - 3, 3, 0] = np.inf        # rows with code 3 in position m - 3: +Inf distance to every query
    centers[0, 200, sub - 1] = -np.inf
    d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    keep = np.flatnonzero(codes[:, 2] != 77)
    d0, j0 = oracle.linscan_aqd_query(np.ascontiguousarray(codes[keep]), centers, queries, K)
    assert np.array_equal(i1, keep[j0].astype(np.uint32)) and _eq_bits(d1, d0)


def test_a_base_of_nan_rows_only(rq):
    """Fewer comparable rows than k: the comparable ones first, then (NaN, no row)."""
    centers, queries, codes = _case(47, 50_000, 8, 4, 10)
    centers[4, :, 0] = np.nan
    centers[4, 9, 0] = 0.25              # only rows with code 9 in position 4 have a distance
    K = 500
    d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    good = np.flatnonzero(codes[:, 4] == 9)
    assert 0 < good.size < K
    for q in range(queries.shape[0]):
        diff = centers - queries[q].reshape(8, 1, 4)
        lut = diff * diff
        acc = np.zeros(good.size, np.float32)
        for k in range(8):
            t = np.zeros(256, np.float32)
            for s in range(4):
                t = t + lut[k, :, s]
            acc = acc + t[codes[good, k]]
        order = np.lexsort((good, acc))
        assert np.array_equal(i1[q, :good.size], good[order].astype(np.uint32))
        assert _eq_bits(d1[q, :good.size], acc[order])
        assert np.all(np.isnan(d1[q, good.size:])) and np.all(i1[q, good.size:] == 0xFFFFFFFF)


def test_non_finite_inputs_through_linscan_pq_one_based(rq):
    """The Julia-side view (src/Linscan.jl:25: idx .+ 1): "no row" reads 0."""
    centers, queries, codes = _case(53, 20_000, 8, 4, 8)
    queries[5, 7] = np.nan
    C = [centers[i] for i in range(8)]
    d, idx = rq.linscan_pq(codes, queries, C, 64, 10)
    assert np.all(idx[5] == 0) and np.all(np.isnan(d[5]))
    assert np.all(idx[np.arange(8) != 5] >= 1)


# ---- the same contract on the other PQ paths: in-call row order, ordered bases, index handles and their shard merges, host query
# chunks -- against tests/nonfinite_ref.py (the contract in plain numpy; tests/test_nonfinite_ref.py pins it to the oracle), every
# query compared, with NaNs of both signs ------------------------------------------------------------------------------------
import functools                                    # noqa: E402

import nonfinite_ref as nf                          # noqa: E402
from switch_table import switches                   # noqa: E402

PN, PM, PSUB, PNQ = 200_000, 8, 3, 29
POISONS = ["queries", "tables", "both"]


def _L():
    from rayuela_jl_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _poisoned_pq(poison, n=PN, nq=PNQ):
    centers, queries, codes = _case(59, n, PM, PSUB, nq)
    if poison in ("queries", "both"):
        nf.put_bits(queries, (3, 1), nf.NAN_POS)
        nf.put_bits(queries, (10, 5), nf.NAN_NEG)
        queries[9, PSUB * PM - 1] = np.inf
        queries[12, 0] = -np.inf
    if poison in ("tables", "both"):
        nf.put_bits(centers, (2, 77, 1), nf.NAN_POS)       # rows with code 77 in position 2: NaN distance to every query
        nf.put_bits(centers, (5, 9, 0), nf.NAN_NEG)
        centers[PM - 3, 3, 0] = np.inf
        centers[0, 200, PSUB - 1] = -np.inf
    for a in (centers, queries, codes):
        a.setflags(write=False)
    return centers, queries, codes


def _same(got, ref, what):
    assert nf.same(got[0], got[1], ref), (what, nf.first_difference(got[0], got[1], ref))


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]       # (a copy: the cached cases are read-only)


@pytest.mark.parametrize("K", [10, 1000])
@pytest.mark.parametrize("poison", POISONS)
def test_pq_poisons_in_call_order(rq, poison, K):
    """ORDER_MIN_NQ = 1: the call orders a scratch copy of the base (sample blocks first, ids through perm) for 29 queries."""
    from rayuela_jl_amd import device as rqd
    centers, queries, codes = _poisoned_pq(poison)
    ref = nf.scan("pq", codes, centers, queries, K)
    L = _L()
    L.check(L.lib().rq_release_workspaces())
    with switches(ORDER_MIN_NQ=1):
        assert L.lib().rq_scan_orders_in_call(PN, PNQ, K) == 1
        _same(rq.linscan_aqd_query(codes, centers, queries, K), ref, (poison, "host pointers"))
        cd, ce, qd = _cuda(codes, centers, queries)
        for call in range(2):                        # the second call scans the kept order
            dd, ii = rqd.linscan(cd, ce, qd, K)
            _same((dd.cpu().numpy(), ii.cpu().numpy()), ref, (poison, "device", call))
        st = L.order_cache_stats()
        assert st["plain_builds"] + st["balanced_builds"] >= 1 and st["hits"] >= 1, st
    with switches(SCAN_ORDER=0):                     # ... and with no ordering at all
        assert L.lib().rq_scan_orders_in_call(PN, PNQ, K) == 0
        _same(rq.linscan_aqd_query(codes, centers, queries, K), ref, (poison, "arrival order"))
    L.check(L.lib().rq_release_workspaces())


@pytest.mark.parametrize("poison", POISONS)
def test_pq_poisons_ordered_base(rq, poison):
    """rq_dev_order_rows + rq_dev_linscan_ordered: ids and keys carry original row numbers + id_offset, padding is KEY_MAX."""
    from rayuela_jl_amd import device as rqd
    centers, queries, codes = _poisoned_pq(poison)
    cd, ce, qd = _cuda(codes, centers, queries)
    ob = rqd.order_rows(cd)
    assert ob.perm is not None                       # the base was ordered
    for K in (10, 1000):
        bits, ids, keys = nf.scan("pq", codes, centers, queries, K, id_base=1, id_offset=1000, want_keys=True)
        dd, ii = rqd.linscan(ob, ce, qd, K, id_offset=1000, id_base=1)
        _same((dd.cpu().numpy(), ii.cpu().numpy()), (bits, ids), (poison, K))
        got = rqd.linscan(ob, ce, qd, K, id_offset=1000, want_keys=True).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, keys), (poison, K, np.argwhere(got != keys)[:1])


@pytest.mark.parametrize("id_base", [0, 1])
@pytest.mark.parametrize("nshards", [1, 3, 8])
@pytest.mark.parametrize("poison", ["both"])
def test_pq_poisons_index_shards(rq, oracle, poison, nshards, id_base):
    """Index handles over logical shards with id_offset = 1000: the shard lists are merged from packed keys, the padding pair
    must come out of the merge as (0x7FFFFFFF, 0xFFFFFFFF + id_base).  The NaN code 77 is present in one shard only (rows of the
    second third of the base); a second search on the handle rotates the queries first."""
    import rayuela_jl_amd.synth as synth
    centers, queries, codes = _poisoned_pq(poison)
    codes = codes.copy()
    outside = np.ones(PN, bool)
    outside[PN // 3 + 1000:2 * (PN // 3) - 1000] = False
    codes[outside & (codes[:, 2] == 77), 2] = 78
    assert (codes[:, 2] == 77).any()
    C = [centers[i] for i in range(PM)]
    R = synth.rotation(PM * PSUB, seed=3)
    clean = _poisoned_pq("tables")[1]                # queries without poison: rotated, they stay finite
    with rq.Index(C, PM * PSUB, devices=[0] * nshards) as ix:
        ix.set_codes(codes, id_offset=1000)
        info = ix.info()
        assert info["shards"] == nshards and sum(info["rows_per_shard"]) == PN, info
        if nshards == 3:
            lo = np.cumsum([0] + info["rows_per_shard"])
            holds = [bool((codes[lo[s]:lo[s + 1], 2] == 77).any()) for s in range(3)]
            assert holds == [False, True, False], holds
        for K in (10, 1000):
            ref = nf.scan("pq", codes, centers, queries, K, id_base=id_base, id_offset=1000)
            _same(ix.search(queries, K, id_base=id_base), ref, (nshards, id_base, K))
        ref = nf.scan("pq", codes, centers, oracle.rotate_T(R, clean), 100, id_base=id_base, id_offset=1000)
        _same(ix.search(clean, 100, R=R, id_base=id_base), ref, (nshards, id_base, "R"))


def test_pq_poisons_shards_shorter_than_k(rq):
    """8 shards of 375 rows, k = 500: every shard list ends in padding before the merge, the merged list does not (3000 rows,
    a hundredth of them NaN) -- except for the NaN queries, which are padding throughout."""
    centers, queries, codes = _poisoned_pq("both", n=3000)
    C = [centers[i] for i in range(PM)]
    for id_base in (0, 1):
        ref = nf.scan("pq", codes, centers, queries, 500, id_base=id_base, id_offset=1000)
        assert (ref[0][3] == nf.PAD_BITS).all() and not (ref[0][0] == nf.PAD_BITS).any()
        with rq.Index(C, PM * PSUB, devices=[0] * 8) as ix:
            ix.set_codes(codes, id_offset=1000)
            assert max(ix.info()["rows_per_shard"]) < 500
            _same(ix.search(queries, 500, id_base=id_base), ref, id_base)


def test_pq_merge_of_padding_lists_beyond_1024(rq):
    """k = 2000 > 1024 over 8 shards whose lists are mostly padding (only rows with code 9 in position 4 have a distance) or all
    padding (the first shard holds no such row): the merge of KEY_MAX runs."""
    n, K = 40_000, 2000
    centers, queries, codes = (a.copy() for a in _poisoned_pq("queries", n=n))
    centers[4, :, 0] = np.nan
    centers[4, 9, 0] = 0.25
    codes[:n // 8, 4] = 10
    ref = nf.scan("pq", codes, centers, queries, K, id_base=1)
    left = (ref[0] != nf.PAD_BITS).sum(1)
    assert 0 < left.max() < K // 4 and left[3] == 0
    with rq.Index([centers[i] for i in range(PM)], PM * PSUB, devices=[0] * 8) as ix:
        ix.set_codes(codes)
        assert ix.info()["rows_per_shard"][0] == n // 8
        _same(ix.search(queries, K, id_base=1), ref, "merge")
    _same(rq.linscan_pq(codes, queries, [centers[i] for i in range(PM)], 8 * PM, K), ref, "one scan")


def test_pq_nan_query_in_one_host_chunk(rq):
    """600 queries with HOST_CHUNK = 7 (clamped to 256-query chunks: 256 + 256 + 88, scanned on one stream while the other copies):
    the poisoned queries sit in the first chunk, one more NaN query in the second; every other query is untouched."""
    n, nq, K = 10_000, 600, 50
    centers, queries, codes = (a.copy() for a in _poisoned_pq("both", n=n, nq=nq))
    nf.put_bits(queries, (300, 4), nf.NAN_NEG)
    ref = nf.scan("pq", codes, centers, queries, K, id_base=1)
    assert (ref[0][300] == nf.PAD_BITS).all() and (ref[1][300] == 0).all()
    with switches(HOST_CHUNK=7):
        assert nq >= 2 * 256                         # the call is chunked (rq_api.hip scan_and_fetch)
        _same(rq.linscan_pq(codes, queries, [centers[i] for i in range(PM)], 8 * PM, K), ref, "chunked")
    _same(rq.linscan_pq(codes, queries, [centers[i] for i in range(PM)], 8 * PM, K), ref, "one launch")
