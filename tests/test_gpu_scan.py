"""GPU parity tests of the ADC scan: HIP path (through the C ABI) vs the reference's golden outputs
and vs the pinned oracle.  Bar: ids AND distances bit-exact (deps/src/linscan_aqd.cpp semantics)."""
import numpy as np
import pytest

import exact_topk as xt
from switch_table import switches

from conftest import golden

pytestmark = pytest.mark.gpu

SCAN_CASES = ["scan_sift_mini", "scan_deep_mini", "scan_all_ties", "scan_dups", "scan_k_eq_n"]


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name", SCAN_CASES)
def test_legacy_symbol_matches_reference_golden(rq, name):
    """The signature-identical linscan_aqd_query symbol (what src/Linscan.jl:19-23 ccalls)."""
    g = golden(name)
    for K in g["Ks"]:
        dists, ids = rq.linscan_aqd_query(g["codes"], g["centers"], g["queries"], int(K))
        assert np.array_equal(ids, g["ids_K%d" % K]), (name, K)
        assert _eq_bits(dists, g["dists_K%d" % K]), (name, K)


@pytest.mark.parametrize("slices", [2, 3, 7])
@pytest.mark.parametrize("name", ["scan_sift_mini", "scan_dups"])
def test_row_slices_merge_to_the_same_answer(rq, name, slices):
    g = golden(name)
    with switches(SCAN_SLICES=slices):
        for K in g["Ks"]:
            if K * slices > g["codes"].shape[0]:
                continue
            dists, ids = rq.linscan_aqd_query(g["codes"], g["centers"], g["queries"], int(K))
            assert np.array_equal(ids, g["ids_K%d" % K]), (name, K, slices)
            assert _eq_bits(dists, g["dists_K%d" % K])


def test_linscan_pq_julia_conventions(rq):
    """linscan_pq(B::Matrix{Int16} one-based, ...) -> one-based UInt32 ids (src/Linscan.jl:25,28-37)."""
    g = golden("scan_sift_mini")
    m = g["codes"].shape[1]
    C = [g["centers"][i] for i in range(m)]
    B1 = g["codes"].astype(np.int16) + 1
    dists, idx = rq.linscan_pq(B1, g["queries"], C, 8 * m, 100)
    assert idx.dtype == np.uint32
    assert np.array_equal(idx, g["ids_K100"] + 1)
    assert _eq_bits(dists, g["dists_K100"])
    d2, i2 = rq.linscan_pq(g["codes"], g["queries"], C, 8 * m, 100)   # UInt8 zero-based overload
    assert np.array_equal(i2, idx) and _eq_bits(d2, dists)


def test_lut_kernel_bit_exact(rq, oracle):
    import torch
    from rayuela_jl_amd import device as rqd
    for name in ["scan_sift_mini", "scan_deep_mini"]:
        g = golden(name)
        lut = rqd.adc_lut(torch.from_numpy(g["centers"]).cuda(), torch.from_numpy(g["queries"]).cuda()).cpu().numpy()
        for q in range(g["queries"].shape[0]):
            assert _eq_bits(lut[q], oracle.adc_lut(g["centers"], g["queries"][q]))


@pytest.mark.parametrize("n,m,sub,nq,K", [
    (200_000, 8, 16, 40, 1000),    # 5 query groups, SIFT shape
    (50_001, 8, 16, 13, 100),      # ragged last group, odd row count
    (30_000, 16, 6, 9, 1000),      # Deep shape: m=16 -> 4 queries per group
    (20_000, 4, 8, 8, 4096),       # k > 2048: big candidate buffers / sort scratch
    (9_000, 2, 3, 5, 1),
    (5_000, 32, 2, 3, 10),
    (1, 8, 4, 2, 1),               # single row
    (70_000, 8, 4, 17, 16384),
    (70_000, 8, 4, 5, 65536),      # RQ_MAX_K: nearly the whole base, exact fallback path (k > rows/16)
    (60_000, 64, 2, 11, 1000),     # PQ64: float2 LUT entries, 2 queries per group
    (10_000, 48, 2, 3, 100),       # padded to 64
])
def test_scan_vs_oracle_random(rq, oracle, n, m, sub, nq, K):
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(n * 31 + m)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=n + 5)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i0, i1)
    assert _eq_bits(d0, d1)


@pytest.mark.parametrize("knob,value", [("SCAN_SAMPLE", 0), ("SCAN_SRANK_MUL", 0), ("SCAN_SLACK", 64)])
def test_threshold_strategies_are_all_exact(rq, oracle, knob, value):
    """The sampled initial threshold is an optimisation only: with sampling off, with a sample that
    is forced to be far too tight (exact fallback path) and with a tiny cut slack (many radix cuts)
    the answer stays bit-identical."""
    import rayuela_jl_amd.synth as synth
    n, m, sub, nq, K = 300_000, 8, 16, 16, 1000
    rng = np.random.default_rng(11)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=123)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    with switches(**{knob: value}):
        d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i0, i1)
    assert _eq_bits(d0, d1)


def test_shard_merge_equals_single_scan(rq, oracle):
    """Row shards scanned separately (global ids via id_offset, packed keys out) and merged on the
    device give the single-scan answer bit for bit -- the multi-GPU data path on one GPU."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq, K = 120_000, 8, 16, 24, 1000
    rng = np.random.default_rng(7)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=99)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    cen, qs = torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    bounds = [0, 30_000, 30_500, 90_001, n]   # uneven shards, one smaller than K
    keys = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        shard = torch.from_numpy(codes[a:b]).cuda()
        kk = min(K, b - a)
        k_sh = rqd.linscan(shard, cen, qs, kk, id_offset=a, want_keys=True)
        if kk < K:  # pad short lists with the maximum key, like a shard with fewer than K rows
            pad = torch.full((nq, K - kk), -1, dtype=torch.int64, device="cuda")
            k_sh = torch.cat([k_sh, pad], dim=1)
        keys.append(k_sh)
    keys = torch.stack(keys, dim=1).contiguous()  # [nq][P][K]
    dists, ids = rqd.merge_topk(keys, K)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), i0)
    assert _eq_bits(dists.cpu().numpy(), d0)


@pytest.mark.parametrize("K", [1025, 3000, 10000])
def test_large_k_sample_sort_paths(rq, oracle, K):
    """K > 1024 finishes with the sample sort (select + sort in global memory): the single-slice
    scan, the sliced scan + merge (slices shorter than K pad their lists with KEY_MAX) and the
    shard merge all give the reference answer bit for bit."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq = 45_000, 8, 16, 19
    rng = np.random.default_rng(K)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=K + 1)
    codes[1000:1400] = codes[7]          # a run of identical rows: equal distances, ordered by id
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    for slices in (0, 1, 3, 8):          # 8 slices of 5625 rows: shorter than K = 10000
        with switches(SCAN_SLICES=slices):
            d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
        assert np.array_equal(i0, i1), (K, slices)
        assert _eq_bits(d0, d1), (K, slices)
    cen, qs = torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    bounds = [0, 20_000, 20_900, n]
    keys = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        kk = min(K, b - a)
        k_sh = rqd.linscan(torch.from_numpy(codes[a:b]).cuda(), cen, qs, kk, id_offset=a, want_keys=True)
        if kk < K:
            k_sh = torch.cat([k_sh, torch.full((nq, K - kk), -1, dtype=torch.int64, device="cuda")], dim=1)
        keys.append(k_sh)
    dists, ids = rqd.merge_topk(torch.stack(keys, dim=1).contiguous(), K)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), i0)
    assert _eq_bits(dists.cpu().numpy(), d0)


@pytest.mark.parametrize("nq,K", [(4196, 10), (4196, 1500), (4600, 100)])
def test_whole_and_sliced_items_in_one_launch(rq, oracle, nq, K):
    """More query groups than resident workgroups with a small remainder: the planner scans the first
    512 groups whole and cuts the remaining ones into two row slices (+ merge) inside the same launch;
    keys-and-dists requests go through the same plan."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    n, m, sub = 50_000, 8, 4
    rng = np.random.default_rng(nq + K)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=nq)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i0, i1)
    assert _eq_bits(d0, d1)
    ct, cen, qs = torch.from_numpy(codes).cuda(), torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    keys = rqd.linscan(ct, cen, qs, K, id_offset=7, want_keys=True).cpu().numpy().view(np.uint64)
    assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), i0 + np.uint32(7))


def test_sharded_index_single_rank_uses_hip_kernels(rq, oracle):
    """ShardedIndex with its default (HIP) scan/merge functions, world size 1: keys out of the scan,
    through rq_dev_merge_topk, equal the direct answer."""
    import torch
    from rayuela_jl_amd.sharded import ShardedIndex
    g = golden("scan_sift_mini")
    codes = torch.from_numpy(g["codes"]).cuda()
    cen = torch.from_numpy(g["centers"]).cuda()
    qs = torch.from_numpy(g["queries"]).cuda()
    ix = ShardedIndex(codes, cen, id_offset=0)
    d, i = ix.search(qs, 100, id_base=0)
    assert np.array_equal(i.cpu().numpy().view(np.uint32), g["ids_K100"])
    assert _eq_bits(d.cpu().numpy(), g["dists_K100"])


def test_linscan_opq_vs_oracle(rq, oracle):
    g = golden("encode_sift_mini")
    import rayuela_jl_amd.synth as synth
    m, d = int(g["m"]), g["X"].shape[1]
    R = g["R"]
    centers = g["C"].reshape(m, 256, d // m)
    codes = g["codes_opq"]
    queries = synth.sift_like(12, d, seed=555)
    RQ = oracle.rotate_T(R, queries)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, RQ, 50)
    d1, i1 = rq.linscan_opq(codes, queries, [centers[i] for i in range(m)], 8 * m, R, 50)
    assert np.array_equal(i1, i0 + 1)
    assert _eq_bits(d1, d0)


def test_index_handle(rq, oracle):
    import ctypes
    g = golden("scan_sift_mini")
    lib = rq.lib()
    n, m = g["codes"].shape
    nq, d = g["queries"].shape
    cen = np.ascontiguousarray(g["centers"])
    ix = lib.rq_index_create(m, d, cen.ctypes.data)
    assert ix
    try:
        codes = np.ascontiguousarray(g["codes"])
        assert lib.rq_index_set_codes(ix, codes.ctypes.data, n, 0) == 0
        K = 100
        dists = np.zeros((nq, K), np.float32)
        ids = np.zeros((nq, K), np.uint32)
        q = np.ascontiguousarray(g["queries"])
        assert lib.rq_index_search(ix, dists.ctypes.data, ids.ctypes.data, q.ctypes.data, nq, K, 0) == 0
        assert np.array_equal(ids, g["ids_K100"]) and _eq_bits(dists, g["dists_K100"])
    finally:
        lib.rq_index_destroy(ctypes.c_void_p(ix))


def test_argument_errors_are_reported(rq):
    g = golden("scan_k_eq_n")
    n = g["codes"].shape[0]
    C = [g["centers"][i] for i in range(g["centers"].shape[0])]
    with pytest.raises(rq.RayuelaHipError):   # k > n is undefined behaviour in the reference
        rq.linscan_pq(g["codes"], g["queries"], C, 8 * len(C), n + 1)


def test_large_base_many_slices(rq, oracle):
    """SIFT1B-shape proxy on one GPU: 2e8 rows (1.6 GB of codes), few queries -> the planner cuts the
    base in row slices and merges them; ids above 2^27; every query certified, the oracle on two."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq, K = 200_000_000, 8, 4, 24, 100
    rng = np.random.default_rng(99)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes_t = rqd.synth_codes(n, m, seed=77)
    cen, qs = torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    dists, ids = rqd.linscan(codes_t, cen, qs, K)
    ids64 = ids.long() & 0xFFFFFFFF
    dd = dists[:, 1:] - dists[:, :-1]
    assert bool((dd >= 0).all())
    assert bool((ids64 < n).all())
    # all 24 queries certified to be exactly the reference's top-k (tests/exact_topk.py)
    assert xt.certify(dists, ids, K, xt.adc_lut(cen, qs), codes_t, n) == nq
    codes = codes_t.cpu().numpy()
    sel = [0, 23]
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries[sel], K)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32)[sel], i0)
    assert _eq_bits(dists.cpu().numpy()[sel], d0)


def test_full_size_sift1m_properties(rq, oracle):
    """BASELINE.json size (n=1e6, m=8, nq=1e4 is the bench; here 512 queries, K=1000): size-independent
    properties and the top-k certificate on everything + the oracle on a few queries."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq, K = 1_000_000, 8, 16, 512, 1000
    rng = np.random.default_rng(2024)
    centers = (rng.standard_normal((m, 256, sub)) * 20).astype(np.float32)
    queries = (rng.standard_normal((nq, m * sub)) * 20).astype(np.float32)
    codes_t = rqd.synth_codes(n, m, seed=synth.SEED_BASE)
    codes = codes_t.cpu().numpy()
    assert np.array_equal(codes[:1000], synth.random_codes(1000, m, seed=synth.SEED_BASE))
    cen, qs = torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    dists, ids = rqd.linscan(codes_t, cen, qs, K)
    ids64 = ids.long() & 0xFFFFFFFF
    # ascending lexicographic (dist, id)
    dd = dists[:, 1:] - dists[:, :-1]
    assert bool((dd >= 0).all())
    tie = dd == 0
    assert bool((ids64[:, 1:][tie] > ids64[:, :-1][tie]).all())
    # ids unique per query and in range
    assert bool((ids64 < n).all())
    assert int((torch.sort(ids64, dim=1).values[:, 1:] == torch.sort(ids64, dim=1).values[:, :-1]).sum()) == 0
    # every reported distance is the sequential-f32 ADC distance of that row
    lut = rqd.adc_lut(cen, qs)                                  # [nq][m][256], bit-exact (tested above)
    rows = codes_t[ids64.reshape(-1)].long().reshape(nq, K, m)
    acc = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
    for k in range(m):
        acc = acc + torch.gather(lut[:, k, :], 1, rows[:, :, k])
    assert torch.equal(acc, dists)
    # all 512 queries certified to be exactly the reference's top-k (tests/exact_topk.py)
    assert xt.certify(dists, ids, K, xt.adc_lut(cen, qs), codes_t, n) == nq
    # oracle on a handful of queries
    sel = [0, 17, 255, 511]
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries[sel], K)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32)[sel], i0)
    assert _eq_bits(dists.cpu().numpy()[sel], d0)


@pytest.mark.parametrize("z", [6, 1, -2, -8])
def test_second_threshold_estimate_and_its_fallback(rq, oracle, z):
    """After 1/8 of a slice the threshold is re-estimated from the candidates collected so far (rank K f + z sigma).
    z = 6 is the shipped setting; smaller and negative z make the new threshold too tight on purpose, so that the
    "fewer than K rows beat it" check must redo the slice exactly.  The answer never changes."""
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(12)
    m, sub, n, nq = 8, 4, 400_000, 24
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=9)
    with switches(SCAN_RETUNE_Z=z):
        for K in (300, 1000, 3000):
            d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
            d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
            assert np.array_equal(i0, i1) and _eq_bits(d0, d1), (z, K)


@pytest.mark.parametrize("z", [6, -2])
@pytest.mark.parametrize("filt", [1, 0])
def test_capacity_cut_after_second_estimate(rq, oracle, filt, z):
    """in round 2 the candidates above a tightened threshold stayed in the buffer; a capacity cut that fired
    AFTER the second estimate, while fewer than K buffered candidates beat it, kept such stale keys, raised the threshold
    to one of them and lost the rows in between that had been scanned in the meantime.  Now the second estimate drops
    the stale candidates at once (retune_tau), so the buffer is always exactly {rows seen with dist <= tau} and every
    cut is exact; a too-tight estimate ends in the end-of-slice shortfall check and the exact redo.  SCAN_SLACK = 1 makes the cut fire that early on ordinary data
    (whole-base items: SCAN_SLICES=1 gives every group the 400 000 rows the second estimate needs).  With the shipped
    z = 6 the tightened threshold still admits the true top-k, so the old code's answer happened to stay right; z = -2
    makes the estimate too tight on purpose (what a base whose row order correlates with distance does), and there the
    round-2 library returned wrong neighbours."""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    rng = np.random.default_rng(77)
    m, sub, n, nq = 8, 4, 400_000, 64
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=21)
    knobs = {"SCAN_SLACK": 1, "SCAN_SLICES": 1, "SCAN_STATS": 1, "SCAN_FILTER": filt, "SCAN_RETUNE_Z": z}
    with switches(**knobs):
        for K in (100, 1000):
            d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
            d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
            st = _lib.scan_stats()
            assert np.array_equal(i0, i1) and _eq_bits(d0, d1), (K, filt, z, st)
            # the path under test ran: in-stream cuts happened; a too-tight estimate was caught and redone exactly
            assert st["n_cuts"] > 0 and (z == 6 or st["n_fallbacks"] > 0), st


@pytest.mark.parametrize("m,sub,K,nq", [(8, 4, 100, 100), (8, 4, 1000, 24), (16, 2, 100, 40), (8, 4, 3000, 16)])
def test_xcd_window_plan_on_a_small_base(rq, oracle, m, sub, K, nq):
    """Big bases are scanned in short row windows handed out per XCD, with per-XCD pacing (plan_for / the item loop of
    adc_scan_kernel).  SCAN_XCD_MIN_MB = 1 and 1 MB windows switch that plan on for a base the oracle can check:
    ragged last window, query groups that do not fill a round, large-k merge of the window lists, strict and no pacing."""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    rng = np.random.default_rng(31 + m + K)
    n = 3_000_017
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=5)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    with switches(SCAN_XCD_MIN_MB=1, SCAN_WINDOW_MB=1):
        plan = _lib.scan_plan(n, nq, m, m * sub, K)
        assert plan["xcd"] == 1 and plan["whole"] == 0 and plan["slices"] >= 16, plan
        for slack in (-1, 0, 1 << 20):
            with switches(SCAN_XCD_SLACK=slack):
                d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
            assert np.array_equal(i0, i1) and _eq_bits(d0, d1), (m, K, slack)
    assert _lib.scan_plan(n, nq, m, m * sub, K)["xcd"] == 0            # 24-48 MB of codes: the ordinary plan


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n,m,sub,nq,K,slices", [
    (300_000, 8, 16, 24, 1000, 0),      # the headline shape: ~1.6 K candidates per query, kept keys in LDS
    (300_000, 8, 16, 24, 1024, 0),      # K = the largest the path takes: kept keys may pass the LDS share
    (200_000, 16, 6, 16, 100, 0),       # 1024-thread workgroups: one of a query's two wavefronts finishes it
    (120_000, 8, 4, 40, 7, 3),          # sliced items: packed-key lists for the merge
    (50_000, 4, 8, 9, 1, 0),
])
def test_bucket_finish_equals_select_and_sort(rq, oracle, mode, n, m, sub, nq, K, slices):
    """K <= 1024 finishes per query through distance buckets (bucket_finish_wave, rq_topk.h): SCAN_BUCKET_FINISH = 1 (default:
    kept keys staged in LDS), 2 (staged in global memory) and 0 (round 1-4: radix select + LDS bitonic sort) must all be the
    reference's answer bit for bit (deps/src/linscan_aqd.cpp:91-97: the K smallest (dist, id) pairs, ascending)."""
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(n + 7 * K)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=n + K)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    with switches(SCAN_BUCKET_FINISH=mode, SCAN_SLICES=slices):
        d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i0, i1)
    assert _eq_bits(d0, d1)


@pytest.mark.parametrize("distinct", [1, 3, 40, 400])
def test_bucket_finish_gives_up_on_mass_ties_and_stays_exact(rq, oracle, distinct):
    """Rows that share their codes share their distance: `distinct` different rows repeated over the base put hundreds of keys
    into ONE distance bucket, where counting ranks is quadratic -- the wavefront gives up before writing anything and the group
    takes the select + sort path; with 400 distinct rows only some queries do.  Ties resolve to the lowest row id either way."""
    n, m, sub, nq, K = 100_000, 8, 16, 16, 1000
    rng = np.random.default_rng(distinct)
    centers = rng.integers(0, 8, (m, 256, sub)).astype(np.float32)
    queries = rng.integers(0, 8, (nq, m * sub)).astype(np.float32)
    pool = rng.integers(0, 256, (distinct, m), dtype=np.uint8)
    codes = np.ascontiguousarray(pool[rng.integers(0, distinct, n)])
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    for mode in (1, 2):
        with switches(SCAN_BUCKET_FINISH=mode):
            d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
        assert np.array_equal(i0, i1), (distinct, mode)
        assert _eq_bits(d0, d1)


@pytest.mark.parametrize("distinct", [0, 1, 50, 3000])
def test_large_k_map_buckets_and_their_splitter_fallback(rq, oracle, distinct):
    """K > 1024 partitions a query's candidates into buckets by a monotone MAP of the distance word (samplesort_topk, rq_topk.h);
    rows that tie in distance share a bucket however many they are, and a crowded bucket sends the query back through sorted
    splitters (whole 64-bit keys, which part ties by id).  distinct = 0: random codes (the map alone); 1 / 50: every candidate
    ties with hundreds of others (splitters); 3000: a mixture.  Ids and distance bits must equal the reference's either way."""
    import rayuela_jl_amd.synth as synth
    n, m, sub, nq, K = 120_000, 8, 16, 16, 3000
    rng = np.random.default_rng(100 + distinct)
    centers = rng.integers(0, 8, (m, 256, sub)).astype(np.float32)
    queries = rng.integers(0, 8, (nq, m * sub)).astype(np.float32)
    if distinct:
        pool = rng.integers(0, 256, (distinct, m), dtype=np.uint8)
        codes = np.ascontiguousarray(pool[rng.integers(0, distinct, n)])
    else:
        codes = synth.random_codes(n, m, seed=77)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    for use_map in (1, 0):
        with switches(SCAN_SS_MAP=use_map):
            d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
        assert np.array_equal(i0, i1), (distinct, use_map)
        assert _eq_bits(d0, d1)
