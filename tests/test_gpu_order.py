"""Bank-aware row order (csrc/rq_order.hip): the ordered base is a permutation of the arrival-order base, and every scan
over it returns the SAME ids and distance bits as the reference semantics (deps/src/linscan_aqd.cpp:85-97: sequential f32
sums, the k smallest (dist, id) pairs) -- ids are original row numbers, ties included."""
import numpy as np
import pytest

from switch_table import switches

pytestmark = pytest.mark.gpu


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _Tuning(rq, **kv):
    """The switches for a `with` block, reset (not restored by value) on exit."""
    return switches(**kv)


def _lds_passes(codes, rpt):
    """LDS-pass model of the byte-table gathers (tools/rowperm_sim.py): mean over lane groups and bytes of the fullest
    slot column's number of distinct addresses."""
    n, m = codes.shape
    tile = 64 * rpt
    g = codes[: n // tile * tile].reshape(-1, 2, 32, rpt, m).transpose(0, 1, 3, 2, 4).reshape(-1, 32, m)
    tot = 0.0
    for k in range(m):
        pres = np.zeros((g.shape[0], 256), dtype=bool)
        pres[np.arange(g.shape[0])[:, None], g[:, :, k]] = True
        tot += pres.reshape(-1, 8, 32).sum(1).max(1).mean()
    return tot / m


@pytest.mark.parametrize("n,m", [(1_000_000, 8), (300_001, 16), (70_000, 4), (200_000, 5), (65_536, 2), (100_003, 32)])
def test_order_rows_is_a_permutation_with_fewer_bank_conflicts(rq, n, m):
    import torch
    from rayuela_jl_amd import device as rqd
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    codes = synth.random_codes(n, m, seed=n + m)
    ob = rqd.order_rows(torch.from_numpy(codes).cuda())
    mp = int(_lib.lib().rq_scan_row_width(m))
    oc, perm = ob.codes.cpu().numpy(), ob.perm.cpu().numpy().view(np.uint32).astype(np.int64)
    assert oc.shape == (n, mp)
    assert np.array_equal(np.sort(perm), np.arange(n))                     # a bijection
    assert np.array_equal(oc[:, :m], codes[perm])                          # ordered row i IS original row perm[i]
    assert not oc[:, m:].any()                                             # zero padding bytes
    if m in (8, 16):
        rpt = 2 if m == 8 else 1
        before, after = _lds_passes(codes, rpt), _lds_passes(oc[:, :m], rpt)
        # n = 1e6, m = 8: 3.15 -> 1.94 passes per gather (5 of 8 byte tables conflict-free)
        # (a sixteenth of the rows -- the arrival-order sample blocks -- keeps the old rate)
        assert after < (0.70 if m == 8 else 0.87) * before, (before, after)


@pytest.mark.parametrize("m", [8, 16])
@pytest.mark.parametrize("kind", ["uniform", "dups", "skew", "clumps"])
def test_greedy_balance_is_a_permutation_and_lowers_the_passes(rq, oracle, kind, m):
    """Round 6: where the key covers 4 tables (8- and 16-byte rows from ~8e5 rows on) the rows of every sort bucket are dealt to
    the bucket's lane groups by a greedy pass over the uncovered tables (order_fine_greedy_kernel).  Whatever it does must be
    a permutation -- the scan's answer then cannot depend on it --; on uniform codes it must beat the plain 15-bit sort in the
    LDS-pass model; hostile bases (60 distinct rows, half of the rows in one bucket, 4096 tight clumps) send coarse buckets
    past the LDS list (plain path) or whole buckets into one window after the other."""
    import torch
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(600 + m)
    n, sub, nq, K = 1_000_000, 2, 8, 100
    if kind == "clumps":
        pool = rng.integers(0, 256, (4096, m), dtype=np.uint8)
        codes = pool[rng.integers(0, 4096, n)]
        codes[:, m - 1] = rng.integers(0, 256, n, dtype=np.uint8)        # ... that differ in their last byte only
    else:
        codes = _hostile_codes(kind, n, m, rng)
    cd = torch.from_numpy(codes).cuda()
    res = {}
    for greedy in (0, 1):
        with _Tuning(rq, ORDER_GREEDY=greedy):
            ob = rqd.order_rows(cd)
        oc, perm = ob.codes.cpu().numpy(), ob.perm.cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(np.sort(perm), np.arange(n)), (kind, m, greedy)
        assert np.array_equal(oc[:, :m], codes[perm]), (kind, m, greedy)
        res[greedy] = (ob, _lds_passes(oc[:, :m], 2 if m == 8 else 1))
    if kind == "uniform":
        # m = 8: 1.94 -> 1.63 passes per gather (tables 4..7: 3.15 -> 2.2 each); m = 16: 2.54 -> 2.14
        assert res[1][1] < 0.90 * res[0][1], (m, res[0][1], res[1][1])
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    d1, i1 = rqd.linscan(res[1][0], torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda(), K)
    assert np.array_equal(i1.cpu().numpy().view(np.uint32), i0) and _eq_bits(d1.cpu().numpy(), d0), (kind, m)


def _hostile_codes(kind, n, m, rng):
    if kind == "uniform":
        return rng.integers(0, 256, (n, m), dtype=np.uint8)
    if kind == "dups":          # 60 distinct rows: massive exact ties across the permutation
        pool = rng.integers(0, 256, (60, m), dtype=np.uint8)
        return pool[rng.integers(0, 60, n)]
    if kind == "lowbits":       # every byte in [0, 8): one sort bucket, ties everywhere
        return rng.integers(0, 8, (n, m), dtype=np.uint8)
    if kind == "skew":          # half of the rows in ONE bucket, the rest uniform
        c = rng.integers(0, 256, (n, m), dtype=np.uint8)
        c[: n // 2] = c[0]
        return c[rng.permutation(n)]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["uniform", "dups", "lowbits", "skew"])
@pytest.mark.parametrize("n,m,sub,nq,K", [(150_000, 8, 4, 24, 1000), (100_003, 8, 4, 9, 1), (90_000, 16, 2, 16, 100),
                                          (70_001, 8, 4, 8, 3000)])
def test_ordered_scan_is_bit_exact(rq, oracle, kind, n, m, sub, nq, K):
    """SCAN_ORDER = 2 forces the in-call ordering at any batch size; ids and distances equal the oracle's."""
    rng = np.random.default_rng(n + m + K)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = _hostile_codes(kind, n, m, rng)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    with _Tuning(rq, SCAN_ORDER=2, ORDER_MIN_ROWS=1):
        d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i0, i1), (kind, n, m, K)
    assert _eq_bits(d0, d1)


@pytest.mark.parametrize("knobs", [dict(SCAN_SRANK_MUL=0), dict(SCAN_SLACK=64, SCAN_SRANK_MUL=0), dict(SCAN_FILTER=0),
                                   dict(SCAN_SLICES=3), dict(SCAN_RETUNE_Z=-8), dict(ORDER_SHUFFLE=0),
                                   dict(ORDER_BITS=9), dict(ORDER_BITS=20), dict(ORDER_GRAN=1024), dict(ORDER_SAMPLE_STRIDE=0),
                                   dict(ORDER_SAMPLE_STRIDE=3)])
def test_ordered_scan_on_every_threshold_path(rq, oracle, knobs):
    """The exact fallback (tau = +inf with capacity cuts: emit_survivors reads perm), the unfiltered loop, row slices +
    merge, a second estimate that is too tight, an unshuffled (sorted) base -- the estimate then misses and the slice is
    redone exactly -- and other key widths / granules: the answer never changes."""
    rng = np.random.default_rng(5)
    n, m, sub, nq = 300_000, 8, 4, 16
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = _hostile_codes("dups", n // 2, m, rng)
    codes = np.concatenate([codes, _hostile_codes("uniform", n - n // 2, m, rng)])[rng.permutation(n)]
    for K in (100, 1000):
        d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
        with _Tuning(rq, SCAN_ORDER=2, ORDER_MIN_ROWS=1, **knobs):
            d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
        assert np.array_equal(i0, i1) and _eq_bits(d0, d1), (knobs, K)


def test_ordered_base_object_with_shards_and_keys(rq, oracle):
    """rq_dev_order_rows + rq_dev_linscan_ordered: shards ordered separately, global ids through id_offset, packed keys
    merged on the device -- the multi-GPU data path over ordered shards."""
    import torch
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(8)
    n, m, sub, nq, K = 260_000, 8, 4, 24, 500
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = _hostile_codes("dups", n, m, rng)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    cen, qs = torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    bounds = [0, 100_000, 100_300, n]        # one shard shorter than K (too small to order: perm is None)
    keys = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        ob = rqd.order_rows(torch.from_numpy(codes[a:b]).cuda())
        assert (ob.perm is None) == (b - a < 1000)
        kk = min(K, b - a)
        ks = rqd.linscan(ob, cen, qs, kk, id_offset=a, want_keys=True)
        if kk < K:
            ks = torch.cat([ks, torch.full((nq, K - kk), -1, dtype=torch.int64, device="cuda")], dim=1)
        keys.append(ks)
    dists, ids = rqd.merge_topk(torch.stack(keys, dim=1).contiguous(), K)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), i0) and _eq_bits(dists.cpu().numpy(), d0)
    # and the (dists, ids) form on one ordered base, one-based ids
    ob = rqd.order_rows(torch.from_numpy(codes).cuda())
    d1, i1 = rqd.linscan(ob, cen, qs, K, id_base=1)
    assert np.array_equal(i1.cpu().numpy().view(np.uint32), i0 + 1) and _eq_bits(d1.cpu().numpy(), d0)


@pytest.mark.parametrize("order", [1, 0])
def test_index_handle_orders_its_shards(rq, oracle, order):
    """rq_index_set_codes orders every shard once (INDEX_ORDER = 1); searches return original ids."""
    rng = np.random.default_rng(3)
    n, m, sub, nq, K = 400_000, 8, 4, 40, 300
    d = m * sub
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    codes = _hostile_codes("skew", n, m, rng)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    with _Tuning(rq, INDEX_ORDER=order):
        for devices in ([0], [0, 0, 0]):
            ix = rq.Index([centers[i] for i in range(m)], d, devices=devices)
            ix.set_codes(codes)
            dd, ii = ix.search(queries, K, id_base=0)
            assert np.array_equal(np.asarray(ii).view(np.uint32), i0) and _eq_bits(dd, d0), (order, devices)
            del ix


def test_auto_order_at_bench_batch_size(rq, oracle):
    """nq >= ORDER_MIN_NQ: rq_dev_linscan / the host-pointer call order the base themselves (default tuning)."""
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(17)
    n, m, sub, nq, K = 200_000, 8, 4, 2048, 100
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=4)
    d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    with _Tuning(rq, SCAN_ORDER=0):
        d2, i2 = rq.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i1, i2) and _eq_bits(d1, d2)
    sel = np.arange(0, nq, 37)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries[sel], K)
    assert np.array_equal(i1[sel], i0) and _eq_bits(d1[sel], d0)


def test_xcd_windows_over_an_ordered_base(rq, oracle):
    """Big-base plan (row windows per XCD) forced on a small ordered base."""
    rng = np.random.default_rng(23)
    n, m, sub, nq, K = 600_000, 8, 4, 64, 100
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = _hostile_codes("dups", n, m, rng)
    d0, i0 = oracle.linscan_aqd_query(codes, centers, queries, K)
    with _Tuning(rq, SCAN_ORDER=2, ORDER_MIN_ROWS=1, SCAN_XCD_MIN_MB=1, SCAN_WINDOW_MB=1):
        d1, i1 = rq.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i0, i1) and _eq_bits(d0, d1)


def test_clumped_base_does_not_fall_back(rq, oracle):
    """1e6 rows from 1024 tight clusters: a query's top-1000 is one cluster = a handful of sort buckets.  On a plainly sorted base
    the second threshold estimate (which takes the first part of a slice for a random sample) missed for half of the whole-base
    items, and the first estimate of sliced items missed with 1024-row shuffle granules; the exact redo made those scans 3x
    slower than in arrival order.  The arrival-order sample blocks and the tile-sized granules keep both estimates honest: no
    fallbacks at any batch size, same answer."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd, _lib
    n, d, m, h, K = 1_000_000, 128, 8, 256, 1000
    X = synth.sift_like(n, d, seed=synth.SEED_BASE)              # ncentres = 1024
    C = synth.codebooks(synth.sift_like(20_000, d, seed=synth.SEED_BASE, row0=3_100_000_000), m, h, seed=synth.SEED_CODEBOOK,
                        iters=5, sample=20000)
    B = rq.quantize_pq_u8(X, C)
    cen = torch.from_numpy(np.stack(C)).cuda()
    ob = rqd.order_rows(torch.from_numpy(B).cuda())
    for nq in (64, 512, 4096):             # sliced items (8 and 2 slices) and whole-base items
        Q = synth.sift_like(nq, d, seed=synth.SEED_QUERY)
        qd = torch.from_numpy(Q).cuda()
        with _Tuning(rq, SCAN_STATS=1):
            _lib.scan_stats()
            d1, i1 = rqd.linscan(ob, cen, qd, K)
            torch.cuda.synchronize()
            st = _lib.scan_stats()
        assert st["n_fallbacks"] == 0, (nq, st)
        sel = np.arange(0, nq, max(1, nq // 32))
        d0, i0 = oracle.linscan_aqd_query(B, np.stack(C), Q[sel], K)
        assert np.array_equal(i1.cpu().numpy().view(np.uint32)[sel], i0) and _eq_bits(d1.cpu().numpy()[sel], d0), nq
    # Round 5: the finish through distance buckets ranks the keys of a bucket against each other -- quadratic in a group of rows
    # that TIE in distance, and this base is full of them (rows of a cluster share their codes).  A 64-key look per query
    # (bf_tie_twins, rq_topk.h) sends such groups to select + sort before any bucket work is done.  What is asserted is the
    # ROUTING (counters of rq_scan_finish_stats), not a clock: nearly every group of this base must be turned away by the look,
    # none may give up half-way (after its histogram), and the answer is the one checked above.  The clock A/B that this guards
    # (bucket finish on / off: 2.13 / 2.10 ms; without the look 2.19 / 2.00) lives in tools/finish_ab.py.
    with _Tuning(rq, SCAN_STATS=1, SCAN_BUCKET_FINISH=1):
        _lib.scan_stats()
        rqd.linscan(ob, cen, qd, K)
        torch.cuda.synchronize()
        st = _lib.scan_stats()
    # (which 64 candidates a query looks at depends on the order its rows were appended in, i.e. on wavefront timing: measured
    # 509-512 of 512 groups turned away by the look, 0-3 giving up after their histogram; the failure this guards -- the look never
    # firing, as in round 5's first version -- reads 0 of 512)
    assert st["bf_items"] == st["n_items"] > 0, st
    assert st["bf_look_skips"] >= 0.97 * st["bf_items"], st
    assert st["bf_select_sort"] - st["bf_look_skips"] <= 0.03 * st["bf_items"], st


def test_tiny_base_of_an_untiled_row_width_through_order_rows(rq, oracle):
    """n < 1024 rows of m = 12 (rows padded to 16 bytes, nothing to order: perm = NULL): order_rows followed by linscan(OrderedBase)
    used to be refused with RQ_EUNSUPPORTED; the pair must always be usable."""
    import torch
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(5)
    n, m, sub, nq, K = 700, 12, 4, 9, 50
    B = rng.integers(0, 256, (n, m), dtype=np.uint8)
    C = rng.standard_normal((m, 256, sub)).astype(np.float32)
    Q = rng.standard_normal((nq, m * sub)).astype(np.float32)
    ob = rqd.order_rows(torch.from_numpy(B).cuda())
    assert ob.perm is None
    d1, i1 = rqd.linscan(ob, torch.from_numpy(C).cuda(), torch.from_numpy(Q).cuda(), K)
    d0, i0 = oracle.linscan_aqd_query(B, C, Q, K)
    assert np.array_equal(i1.cpu().numpy().view(np.uint32), i0) and _eq_bits(d1.cpu().numpy(), d0)
