"""GPU: the bulk top-k path, k > RQ_MAX_K = 65536 up to k = n (rq_bulk.hip).  Every scan entry point serves it: the host-pointer
calls, the device calls, the legacy symbols, the AQ scans, index handles with logical shards and the merge.  Bar as everywhere:
ids AND distances bit-identical to the compiled reference where it is affordable, otherwise every query certified exactly
(tests/exact_topk.py)."""
import numpy as np
import pytest

import exact_topk as xt

pytestmark = pytest.mark.gpu

RQ_MAX_K = 65536
KEY_MAX = -1          # uint64 0xFFFF...F as int64


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _np(t):
    return t.cpu().numpy()


def _base(n, m, sub, nq, seed, kind="rand"):
    """centers [m][256][sub], queries [nq][m sub], codes [n][m]; kinds "ties" and "dups" as tests/gen_golden.py builds them."""
    import rayuela_jl_amd.synth as synth
    d = m * sub
    if kind == "rand":
        rng = np.random.default_rng(seed)
        centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
        queries = rng.standard_normal((nq, d)).astype(np.float32)
        codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    elif kind == "ties":      # all rows identical: the answer is decided by the ids alone
        centers = (synth.splitmix64(np.arange(m * 256 * sub, dtype=np.uint64) ^ np.uint64(5))
                   % np.uint64(7)).astype(np.float32).reshape(m, 256, sub)
        queries = (synth.splitmix64(np.arange(nq * d, dtype=np.uint64) ^ np.uint64(6))
                   % np.uint64(5)).astype(np.float32).reshape(nq, d)
        codes = np.tile(synth.random_codes(1, m, seed=3), (n, 1))
    elif kind == "dups":      # integer tables, 4 code values per sub-quantizer: massive distance ties
        centers = (synth.splitmix64(np.arange(m * 256 * sub, dtype=np.uint64) ^ np.uint64(8))
                   % np.uint64(3)).astype(np.float32).reshape(m, 256, sub)
        queries = (synth.splitmix64(np.arange(nq * d, dtype=np.uint64) ^ np.uint64(9))
                   % np.uint64(3)).astype(np.float32).reshape(nq, d)
        codes = (synth.random_codes(n, m, seed=4) % 4).astype(np.uint8)
    else:
        raise ValueError(kind)
    return centers, queries, np.ascontiguousarray(codes)


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _kernel():
    from rayuela_jl_amd import _lib
    return (_lib.lib().rq_last_scan_kernel() or b"").decode()


def test_large_k_through_every_pq_entry_point(rq, oracle):
    """k = 65537 and k = n on 70 000 rows: refused with RQ_EUNSUPPORTED before the bulk path (the legacy symbol returned zeros)."""
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq = 70_000, 8, 4, 4
    centers, Q, codes = _base(n, m, sub, nq, seed=1)
    C = [centers[i] for i in range(m)]
    ct, qt, bt = _dev(centers, Q, codes)
    for k in (RQ_MAX_K + 1, n):
        d0, i0 = oracle.ref_linscan_aqd_query(codes, centers, Q, k)
        d1, i1 = rq.linscan_pq(codes, Q, C, 8 * m, k)                   # host pointers, one-based ids
        assert np.array_equal(i1, i0 + 1) and _eq_bits(d1, d0), k
        d2, i2 = rqd.linscan(bt, ct, qt, k)                               # device pointers
        assert _kernel() == "adc_bulk_keys_kernel<8, false>"
        assert np.array_equal(_np(i2).view(np.uint32), i0) and _eq_bits(_np(d2), d0), k
        d3, i3 = rq.linscan_aqd_query(codes, centers, Q, k)               # the void legacy symbol
        assert i3.any() and d3.any(), "legacy symbol returned zeros"
        assert np.array_equal(i3, i0) and _eq_bits(d3, d0), k


def test_boundary_65536_to_65537(rq):
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq = 70_000, 8, 4, 4
    centers, Q, codes = _base(n, m, sub, nq, seed=1)
    ct, qt, bt = _dev(centers, Q, codes)
    d1, i1 = rqd.linscan(bt, ct, qt, RQ_MAX_K)
    assert _kernel().startswith("adc_scan_kernel<8"), _kernel()
    d2, i2 = rqd.linscan(bt, ct, qt, RQ_MAX_K + 1)
    assert _kernel() == "adc_bulk_keys_kernel<8, false>"
    assert np.array_equal(_np(i2)[:, :RQ_MAX_K], _np(i1)) and _eq_bits(_np(d2)[:, :RQ_MAX_K], _np(d1))
    # keys and dists / ids together, id_offset and one-based ids
    keys = rqd.linscan(bt, ct, qt, RQ_MAX_K + 1, id_offset=1000, want_keys=True)
    d3, i3 = rqd.linscan(bt, ct, qt, RQ_MAX_K + 1, id_offset=1000, id_base=1)
    k = _np(keys).view(np.uint64)
    assert np.array_equal((k & 0xFFFFFFFF).astype(np.uint32) + 1, _np(i3).view(np.uint32))
    assert np.array_equal(_np(i3).view(np.uint32), _np(i2).view(np.uint32) + 1001) and _eq_bits(_np(d3), _np(d2))
    assert np.all(k[:, 1:] > k[:, :-1])


SHAPES = [
    (70_001, 4, 4, 9, "rand"),
    (70_000, 5, 4, 9, "rand"),       # m = 5: rows zero-padded to 8 bytes
    (80_000, 16, 2, 1, "rand"),
    (70_000, 32, 4, 9, "rand"),
    (66_000, 64, 2, 3, "rand"),
    (70_000, 8, 4, 9, "ties"),       # every distance equal: ids decide
    (90_000, 4, 2, 9, "dups"),       # heavy duplicates
]


@pytest.mark.parametrize("n,m,sub,nq,kind", SHAPES)
def test_shapes_k_eq_n_and_n_minus_1(rq, oracle, n, m, sub, nq, kind):
    from rayuela_jl_amd import device as rqd
    centers, Q, codes = _base(n, m, sub, nq, seed=n + m, kind=kind)
    ct, qt, bt = _dev(centers, Q, codes)
    for k in (n, n - 1):
        d0, i0 = oracle.ref_linscan_aqd_query(codes, centers, Q, k)
        d1, i1 = rqd.linscan(bt, ct, qt, k)
        assert np.array_equal(_np(i1).view(np.uint32), i0) and _eq_bits(_np(d1), d0), (kind, m, k)
        if k == n:      # a full ranking: every row exactly once
            assert np.array_equal(np.sort(i0, axis=1), np.broadcast_to(np.arange(n, dtype=i0.dtype), i0.shape))


def test_million_rows_k_eq_n_certified(rq):
    """n = 1 000 003, m = 8, 100 queries at k = n and k = n - 1: every query certified."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq = 1_000_003, 8, 4, 100
    centers, Q, codes = _base(n, m, sub, nq, seed=7)
    ct, qt, bt = _dev(centers, Q, codes)
    lut = xt.adc_lut(ct, qt)
    for k in (n, n - 1):
        d1, i1 = rqd.linscan(bt, ct, qt, k)
        assert xt.certify(d1, i1, k, lut, bt, n) == nq
        del d1, i1
        torch.cuda.empty_cache()


def test_opq_lsq_cq_and_legacy_aq_symbols(rq, oracle):
    import rayuela_jl_amd.synth as synth
    n, m, d, nq, K = 75_000, 8, 32, 3, 70_000
    rng = np.random.default_rng(5)
    cb = rng.standard_normal((m * 256, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=17)
    nrm = (rng.random(n) * 50).astype(np.float32)
    C = [cb[k * 256:(k + 1) * 256] for k in range(m)]
    eye = np.eye(d, dtype=np.float32)
    d0, i0 = oracle.linscan_lsq(codes, cb, q, nrm, K, use_ref=True)
    d1, i1 = rq.linscan_lsq(codes, q, C, nrm, eye, K)
    assert np.array_equal(i1.view(np.int32), i0) and _eq_bits(d1, d0)
    d1, i1 = rq.linscan_aqd_query_extra_byte(codes, q, cb, nrm, K)
    assert np.array_equal(i1, i0) and _eq_bits(d1, d0)
    d0, i0 = oracle.linscan_cq(codes, cb, q, K, use_ref=True)
    d1, i1 = rq.linscan_cq(codes, q, C, K)
    assert np.array_equal(i1.view(np.int32), i0) and _eq_bits(d1, d0)
    d1, i1 = rq.linscan_aqd_query_extra_byte(codes, q, cb, None, K)
    assert np.array_equal(i1, i0) and _eq_bits(d1, d0)
    # OPQ: the queries are rotated first (src/Linscan.jl:102)
    centers, Q, pcodes = _base(n, m, 4, nq, seed=6)
    R = synth.rotation(m * 4, seed=3)
    d0, i0 = oracle.ref_linscan_aqd_query(pcodes, centers, oracle.rotate_T(R, Q), K)
    d1, i1 = rq.linscan_opq(pcodes, Q, [centers[i] for i in range(m)], 8 * m, R, K)
    assert np.array_equal(i1, i0 + 1) and _eq_bits(d1, d0)


@pytest.mark.parametrize("nshards", [1, 3, 8])
def test_index_logical_shards_equal_the_single_scan(rq, nshards):
    """Shards of ~8 750 rows (8 shards) are far shorter than k: the merge of P lists of K > RQ_MAX_K runs the bulk select."""
    n, m, sub, nq = 70_000, 8, 4, 5
    centers, Q, codes = _base(n, m, sub, nq, seed=11)
    C = [centers[i] for i in range(m)]
    off = 2 ** 32 - n - 2          # ids up to 2^32 - 2 (+ 1 one-based)
    d0, i0 = rq.linscan_pq(codes, Q, C, 8 * m, n)
    with rq.Index(C, m * sub, devices=[0] * nshards) as ix:
        ix.set_codes(codes, id_offset=off)
        for k in (RQ_MAX_K + 1, n):
            d1, i1 = ix.search(Q, k)
            assert _eq_bits(d1, d0[:, :k]), (nshards, k)
            assert np.array_equal(i1.astype(np.int64), i0[:, :k].astype(np.int64) + off), (nshards, k)


def test_host_calls_stream_results_in_query_chunks(rq):
    """Host-pointer results go through bounded device buffers (256 MiB): 3 query chunks of the host call at k = n = 3e5, and of
    an 8-shard index search (results + gathered + interleaved lists) at k = 70 000."""
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq = 300_000, 8, 4, 230          # 256 MiB / (3e5 x 8 B) = 111 queries per chunk
    centers, Q, codes = _base(n, m, sub, nq, seed=14)
    C = [centers[i] for i in range(m)]
    ct, qt, bt = _dev(centers, Q, codes)
    d1, i1 = rq.linscan_pq(codes, Q, C, 8 * m, n)
    d0, i0 = rqd.linscan(bt, ct, qt, n)
    assert np.array_equal(i1, _np(i0).view(np.uint32) + 1) and _eq_bits(d1, _np(d0))
    del d0, i0, d1, i1
    n, nq, k = 70_000, 60, 70_000                 # 256 MiB / (70 000 x 8 B x 17) = 28 queries per chunk
    centers, Q, codes = _base(n, m, sub, nq, seed=15)
    C = [centers[i] for i in range(m)]
    d0, i0 = rq.linscan_pq(codes, Q, C, 8 * m, k)
    with rq.Index(C, m * sub, devices=[0] * 8) as ix:
        ix.set_codes(codes)
        d1, i1 = ix.search(Q, k)
    assert np.array_equal(i1, i0) and _eq_bits(d1, d0)


def test_env_device_list_large_k(rq, monkeypatch):
    n, m, sub, nq = 70_000, 8, 4, 3
    centers, Q, codes = _base(n, m, sub, nq, seed=12)
    C = [centers[i] for i in range(m)]
    d0, i0 = rq.linscan_pq(codes, Q, C, 8 * m, 68_000)
    monkeypatch.setenv("RAYUELA_HIP_DEVICES", "0,0")
    d1, i1 = rq.linscan_pq(codes, Q, C, 8 * m, 68_000)
    assert np.array_equal(i1, i0) and _eq_bits(d1, d0)


@pytest.mark.parametrize("P", [2, 8])
def test_merge_topk_large_k_equals_a_sort(rq, P):
    """P sorted lists of K = 100 000 keys per query, short lists padded with KEY_MAX; many equal distance words."""
    import torch
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    K, nq = 100_000, 3
    g = torch.Generator().manual_seed(P)
    lists = torch.full((nq, P, K), KEY_MAX, dtype=torch.int64)
    expect = torch.full((nq, K), KEY_MAX, dtype=torch.int64)
    for q in range(nq):
        real = []
        uid = 0
        for p in range(P):
            cnt = K - (p * 37_000) % K if q != 2 else p * 3_000      # query 2: fewer than K real keys in all
            hi = torch.randint(0, 1 << 12 if p % 2 else 1 << 30, (cnt,), generator=g, dtype=torch.int64)
            ids = torch.arange(uid, uid + cnt, dtype=torch.int64)[torch.randperm(cnt, generator=g)]
            uid += cnt
            keys = torch.sort((hi << 32) | ids).values
            lists[q, p, :cnt] = keys
            real.append(keys)
        allk = torch.sort(torch.cat(real)).values[:K]
        expect[q, :allk.numel()] = allk
    kin = lists.cuda()
    out = torch.empty((nq, K), dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().rq_dev_merge_topk(None, None, out.data_ptr(), kin.data_ptr(), nq, P, K, 0, rqd._stream()))
    assert torch.equal(out.cpu(), expect)
    d, i = rqd.merge_topk(kin, K, id_base=1)
    e = expect.numpy().view(np.uint64)
    assert np.array_equal(_np(i).view(np.uint32), ((e & 0xFFFFFFFF) + 1).astype(np.uint32))
    hi = (e >> 32).astype(np.uint32)
    dist = np.where(hi & 0x80000000, hi ^ 0x80000000, ~hi).astype(np.uint32)
    assert np.array_equal(_np(d).view(np.uint32), dist)


def _expect_with_nan(centers, Q, codes, k):
    """(dists, ids) of the contract: rows with a NaN distance never returned, the rest in (dist, id) order, padding
    (NaN, 0xFFFFFFFF) behind them."""
    import torch
    ct, qt, bt = _dev(centers, Q, codes)
    D = xt.distances(xt.adc_lut(ct, qt), bt).cpu()
    nq, n = D.shape
    dd = np.full((nq, k), np.nan, dtype=np.float32)
    dd.view(np.uint32)[:] = 0x7FFFFFFF
    ii = np.full((nq, k), 0xFFFFFFFF, dtype=np.uint32)
    for q in range(nq):
        ok = ~torch.isnan(D[q])
        rows = torch.arange(n)[ok]
        order = torch.sort(D[q][ok], stable=True).indices[:k]
        c = order.numel()
        dd[q, :c] = D[q][ok][order].numpy()
        ii[q, :c] = rows[order].numpy().astype(np.uint32)
    return dd, ii


def test_non_finite_inputs(rq, oracle):
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq, k = 70_000, 8, 4, 5, 70_000
    centers, Q, codes = _base(n, m, sub, nq, seed=13)
    Q[1, 3] = np.nan                 # a NaN query: all padding
    Q[3, :] = np.inf                 # all +Inf: every distance +Inf, ids 0..k-1
    ct, qt, bt = _dev(centers, Q, codes)
    d1, i1 = rqd.linscan(bt, ct, qt, k)
    d1, i1 = _np(d1), _np(i1).view(np.uint32)
    assert np.all(i1[1] == 0xFFFFFFFF) and np.all(d1[1].view(np.uint32) == 0x7FFFFFFF)
    assert np.array_equal(i1[3], np.arange(k, dtype=np.uint32)) and np.all(np.isposinf(d1[3]))
    fin = [0, 2, 4]
    d0, i0 = oracle.ref_linscan_aqd_query(codes, centers, Q[fin], k)
    assert np.array_equal(i1[fin], i0) and _eq_bits(d1[fin], d0)
    # a NaN codebook entry: its rows drop out of every list, the lists end in padding
    centers2 = centers.copy()
    centers2[2, 17, 1] = np.nan
    Q2 = Q[fin]
    c2, q2 = _dev(centers2, Q2)
    d2, i2 = rqd.linscan(bt, c2, q2, k)
    de, ie = _expect_with_nan(centers2, Q2, codes, k)
    nbad = int((codes[:, 2] == 17).sum())
    assert nbad > 0 and np.all(i2.cpu().numpy().view(np.uint32)[:, k - nbad:] == 0xFFFFFFFF)
    assert np.array_equal(_np(i2).view(np.uint32), ie) and _eq_bits(_np(d2), de)


def test_several_batches_equal_one_query_at_a_time(rq):
    """n = 1e6 at k = 65537: the plan's batch (queries per BULK_SCRATCH_BYTES) is ~190 queries; 2 batches + 7 queries run."""
    import torch
    from rayuela_jl_amd import _lib
    from rayuela_jl_amd import device as rqd
    n, m, sub, k = 1_000_000, 8, 4, RQ_MAX_K + 1
    batch = _lib.scan_plan(n, 1000, m, m * sub, k)["cap"]
    assert 16 <= batch < 1000, batch
    nq = 2 * batch + 7
    centers, Q, codes = _base(n, m, sub, nq, seed=21)
    ct, qt, bt = _dev(centers, Q, codes)
    d1, i1 = rqd.linscan(bt, ct, qt, k)
    for q in range(nq):
        d2, i2 = rqd.linscan(bt, ct, qt[q:q + 1].contiguous(), k)
        assert torch.equal(i2[0], i1[q]) and torch.equal(d2[0].view(torch.int32), d1[q].view(torch.int32)), q
    assert xt.certify(d1, i1, k, xt.adc_lut(ct, qt), bt, n) == nq


def test_hundred_million_rows_certified(rq):
    """1e8 rows generated on the device, k = 1e5, 4 queries: two bulk batches of two queries; every query certified."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq, k = 100_000_000, 8, 4, 4, 100_000
    centers, Q, _ = _base(1, m, sub, nq, seed=31)
    ct, qt = _dev(centers, Q)
    bt = rqd.synth_codes(n, m, seed=5)
    d1, i1 = rqd.linscan(bt, ct, qt, k)
    assert _kernel() == "adc_bulk_keys_kernel<8, false>"
    assert xt.certify(d1, i1, k, xt.adc_lut(ct, qt), bt, n) == nq
    del bt
    torch.cuda.empty_cache()
