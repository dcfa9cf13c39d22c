"""GPU: the IVFADC index (rq_ivf_*, rayuela_jl_amd/IVF.py) at the shapes tests/test_gpu_ivf.py does not reach -- every row width
of ivf_keys_kernel<MP> / ivf_place_kernel<MP>, d past one trip of the q' fill and off the multiples of 4, more than 256 lists in a
search, more queries than threads of ivf_scan_kernel and than one batch, batches and queries without a row, k past 65536, ids
at the top of the uint32 range, the scratch refusal, host threads.  DESIGN.md section 4.29 lists which case reaches what.

Every comparison is exact, as in tests/test_gpu_ivf.py: ids, distance bits and padding against tests/ivf_oracle.py, and against
rq_linscan_pq where the exhaustive scan is the same answer (by_residual = 0, every list probed, k <= n).  The shape cases load
their base with set_codes, so that they are about the search kernels; where the encode covers m they also build() and compare
the grouped base."""
import functools
import threading

import numpy as np
import pytest

import ivf_oracle as ivf
from test_gpu_ivf import _bits, _data, _index, _lists_equal, _same

pytestmark = pytest.mark.gpu

RQ_EUNSUPPORTED = -2


@functools.lru_cache(maxsize=None)
def _shape(kind, n, d, m, nlist, nq=9):
    """X, Q (rows of X), centers [m][256][d/m] (sub-vectors of sampled residuals, a little noise), queries; read-only"""
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(d * 1000 + m)
    if kind == "sift":            # integer-valued: exact ties occur
        X, Xq = synth.sift_like(n, d, seed=5, ncentres=64), synth.sift_like(nq, d, seed=6, ncentres=64)
    else:
        X, Xq = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    Q = X[rng.choice(n, nlist, replace=False)].copy()
    R = ivf.residuals(X, Q, ivf.lists_of(X, Q))
    centers = np.stack(synth.codebooks(R, m, 256, seed=9, iters=0, sample=n)).astype(np.float32)
    for a in (X, Q, centers, Xq):
        a.setflags(write=False)
    return X, Q, centers, Xq


def _run_shape(rq, kind, n, d, m, nlist, pairs):
    """A set_codes base of the shape under both by_residual values: lists() gives the unpadded codes back, every (nprobe, k)
    of `pairs` answers as the oracle and, where it is the same answer, as rq_linscan_pq; then build(): the oracle's grouped
    base and the same answers at m <= 32, a refusal that leaves the loaded base alone above."""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    X, Q, centers, Xq = _shape(kind, n, d, m, nlist)
    C = [centers[i] for i in range(m)]
    for by_residual in (True, False):
        if m <= 32:
            grouped, (lists, _, arrival) = ivf.build(X, Q, centers, by_residual)
        else:
            lists, arrival = ivf.lists_of(X, Q), synth.random_codes(n, m, seed=d + m)
            grouped = ivf.group(lists, arrival, nlist)
        rows = {nprobe: ivf.ranked(grouped, Q, centers, by_residual, Xq, nprobe) for nprobe in {p for p, _ in pairs}}
        with _index(rq, Q, centers, by_residual) as ix:
            ix.set_codes(lists, arrival)
            _lists_equal(ix, grouped)
            for nprobe, k in pairs:
                got = ix.search(Xq, nprobe, k)
                _same(got, ivf.take(rows[nprobe], k), (kind, d, m, by_residual, nprobe, k))
                if not by_residual and nprobe == nlist and m <= 32 and k <= n:
                    _same(got, rq.linscan_pq(arrival, Xq, C, 8 * m, k), ("linscan_pq", kind, d, m, k))
            if m <= 32:
                ix.build(X)
                _lists_equal(ix, grouped)
            else:
                with pytest.raises(ValueError):
                    ix.build(X)
                assert _lib.lib().rq_ivf_build(ix._h, X.ctypes.data, n, 0) == RQ_EUNSUPPORTED
                assert b"m <= 32" in _lib.lib().rq_last_error()
                _lists_equal(ix, grouped)
            nprobe, k = pairs[-1]
            _same(ix.search(Xq, nprobe, k), ivf.take(rows[nprobe], k), ("after build", kind, d, m, by_residual))


# ---- 1. row widths ----------------------------------------------------------------------------------------------------------------
# m -> MP: 1, 2 -> 2 (the 16-bit load and copy) | 5 -> 8 | 17, 24, 32 -> 32 | 48, 64 -> 64 (set_codes only; at m = 64 the
# table alone is 64 KiB of LDS, with q' more than a default launch may ask for).  Padded: 1, 5, 17, 24, 48.
WIDTHS = [(32, 1), (32, 2), (40, 5), (34, 17), (96, 24), (96, 32), (96, 48), (64, 64), (128, 64)]


@pytest.mark.parametrize("kind", ["sift", "gauss"])
@pytest.mark.parametrize("d,m", WIDTHS)
def test_every_row_width(rq, d, m, kind):
    n = 1500
    _run_shape(rq, kind, n, d, m, 7, ((1, 10), (3, 100), (7, n), (7, n + 3)))


# ---- 2. d -------------------------------------------------------------------------------------------------------------------------
# 258, 320: a second trip of the 256-thread q' fill | 258, 6, 10, 1: d rounds up to the table's offset | 8 / 8, 1 / 1: sub-spaces
# of one dimension
DIMS = [(258, 2), (320, 4), (6, 3), (10, 2), (8, 8), (1, 1)]


@pytest.mark.parametrize("kind", ["sift", "gauss"])
@pytest.mark.parametrize("d,m", DIMS)
def test_dimensions_past_one_fill_trip_and_off_the_multiples_of_four(rq, d, m, kind):
    n = 700
    _run_shape(rq, kind, n, d, m, 7, ((1, 10), (3, 60), (7, n + 3)))


# ---- 3. more than 256 lists in a search ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _many_lists(nlist):
    """3000 rows over nlist random centroids (most of 32767 stay empty), random codes.  Past 256 lists: centroids 255 and 256
    are identical and both hold rows, queries 0 and 1 sit on them and next to them; from 300 lists on one centroid >= 256 holds
    a NaN and rows."""
    import rayuela_jl_amd.synth as synth
    n, d, m = 3000, 8, 2
    rng = np.random.default_rng(nlist)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nlist, d)).astype(np.float32)
    Xq = rng.standard_normal((9, d)).astype(np.float32)
    centers = rng.standard_normal((m, 256, d // m)).astype(np.float32)
    lists = np.concatenate([ivf.lists_of(X[a:a + 200], Q) for a in range(0, n, 200)])
    nan_list = nlist - 3 if nlist >= 300 else None
    if nlist > 256:
        Q[256] = Q[255]
        lists[(lists == 255) | (lists == 256)] = 0
        lists[0:4], lists[4:8] = 255, 256
        Xq[0] = Q[255]
        Xq[1] = Q[255] + np.float32(1e-3)
    if nan_list is not None:
        Q[nan_list, 5] = np.nan
        lists[8:12] = nan_list
    codes = synth.random_codes(n, m, seed=nlist)
    return Q, centers, Xq, lists, codes, nan_list


@pytest.mark.parametrize("nlist", [256, 257, 300, 512, 32767])
def test_search_over_more_than_256_lists(rq, nlist):
    Q, centers, Xq, lists, codes, nan_list = _many_lists(nlist)
    n = lists.size
    grouped = ivf.group(lists, codes, nlist)
    order = ivf.probe_order(Xq, Q)
    if nlist > 256:                        # the equal pair: the lower index first, across the block boundary of the coarse kernel
        assert order[0, :2].tolist() == [255, 256] and order[1, :2].tolist() == [255, 256]
    if nan_list is not None:               # a NaN value: the last probe of every query
        assert np.all(order[:, -1] == nan_list)
    for by_residual in (True, False):
        with _index(rq, Q, centers, by_residual) as ix:
            ix.set_codes(lists, codes)
            _lists_equal(ix, grouped)
            for nprobe in sorted({min(p, nlist) for p in (1, 255, 256, 257, nlist)}):
                rows = ivf.ranked(grouped, Q, centers, by_residual, Xq, nprobe)
                umin = int(ivf.union_sizes(grouped, Q, Xq, nprobe).min())
                for k in sorted({1, 10, umin + 1}):
                    want = ivf.take(rows, k, 0)
                    for nq in (9, 1):
                        got = ix.search(Xq[:nq], nprobe, k, id_base=0)
                        _same(got, (want[0][:nq], want[1][:nq]), (nlist, by_residual, nprobe, k, nq))
                    if k == umin + 1:
                        assert (_bits(want[0])[:, -1] == ivf.PAD_BITS).any()
                if nlist > 256:            # the probe order, seen through the answers: rows 0..3 are list 255, rows 4..7 list 256
                    ids = ix.search(Xq[:2], min(nprobe, 2), 8, id_base=0)[1]
                    if nprobe == 1:
                        assert np.all(np.sort(ids[:, :4], axis=1) == np.arange(4)) and np.all(ids[:, 4:] == 0xFFFFFFFF)
                    else:
                        assert np.all(np.sort(ids, axis=1) == np.arange(8))
                if nan_list is not None and not by_residual:
                    # rows 8..11 lie in the NaN centroid's list: reached by the last probe alone (with by_residual their
                    # distances are NaN: never neighbours)
                    ids = ix.search(Xq, nprobe, n, id_base=0)[1]
                    assert np.isin(np.arange(8, 12), ids[0]).all() == (nprobe == nlist)


# ---- 4. more queries than threads of the item scan, and than one batch -------------------------------------------------------------
def test_many_queries_ragged_scan_and_two_batches(rq):
    import rayuela_jl_amd.synth as synth
    S, k = 64, 5
    _, Q, centers, _ = _data("sift", nlist=6)
    sizes = [0, 1, S - 1, S, S + 1, 3 * S + 2]
    lists = np.repeat(np.arange(6), sizes)
    lists = lists[np.random.default_rng(1).permutation(lists.size)]
    codes = synth.random_codes(lists.size, centers.shape[0], seed=21)
    grouped = ivf.group(lists, codes, 6, id_offset=17)
    Xd = synth.sift_like(40, Q.shape[1], seed=6, ncentres=64)
    Xd[0] = Q[0]                                       # its nearest list is the empty one
    try:
        rq.set_tuning("IVF_SEGMENT_ROWS", S)
        rq.reset_tuning("IVF_BATCH_QUERIES")
        for by_residual in (True, False):
            with _index(rq, Q, centers, by_residual) as ix:
                ix.set_codes(lists, codes, id_offset=17)
                for nprobe in (1, 2):
                    items = ivf.item_counts(grouped, Q, Xd, nprobe, S)
                    union = ivf.union_sizes(grouped, Q, Xd, nprobe)
                    if nprobe == 1:
                        assert items[0] == 0 and len(set(items.tolist())) >= 3
                    for nq in (1024, 1025, 2500, 16384 + 7):
                        tile = np.random.default_rng(nq).integers(0, 40, nq)
                        tile[:40] = np.arange(40)
                        Xq = np.ascontiguousarray(Xd[tile])
                        want = ivf.search_tiled(grouped, Q, centers, by_residual, Xd, tile, nprobe, k)
                        _same(ix.search(Xq, nprobe, k), want, (by_residual, nprobe, nq))
                        info = ix.info()
                        assert info["batch"] == min(nq, 16384), (nq, info)
                        assert info["items"] == int(items[tile].sum()), (nq, info)
                        assert info["rows_scanned"] == int(union[tile].sum()), (nq, info)
                        assert info["ld"] == max(k, int(union.max())), (nq, info)
    finally:
        rq.reset_tuning("IVF_SEGMENT_ROWS")
        rq.reset_tuning("IVF_BATCH_QUERIES")


# ---- 5. batches and queries without a row ---------------------------------------------------------------------------------------------
def test_empty_probe_sets(rq):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    _, _, centers, _ = _data("sift", nlist=7)
    d, m, n = centers.shape[0] * centers.shape[2], centers.shape[0], 200
    rng = np.random.default_rng(5)
    Q = np.stack([np.zeros(d), np.full(d, 1.0), np.full(d, 100.0)]).astype(np.float32)
    lists = np.full(n, 2)
    codes = synth.random_codes(n, m, seed=13)
    grouped = ivf.group(lists, codes, 3)
    empty = (Q[0] + 0.01 * rng.standard_normal((8, d))).astype(np.float32)      # lists 0, then 1, then 2
    hit = (Q[2] + rng.standard_normal((8, d))).astype(np.float32)               # list 2 first
    assert np.all(ivf.probe_order(empty, Q) == [0, 1, 2]) and np.all(ivf.probe_order(hit, Q)[:, 0] == 2)
    mixed = np.stack([hit[0], empty[0], hit[1], hit[2], empty[1], empty[2], hit[3], empty[3], hit[4]])
    rowless = np.array([0, 1, 0, 0, 1, 1, 0, 1, 0], dtype=bool)

    def sequence(ix, by_residual):
        for nprobe in (1, 2):
            for nq in (8, 1):                          # a whole batch without an item: the fill and the select chain alone
                for k, id_base in ((1, 0), (7, 1), (n + 2, 1)):
                    dists, ids = ix.search(empty[:nq], nprobe, k, id_base)
                    assert np.all(_bits(dists) == ivf.PAD_BITS) and np.all(ids == (0xFFFFFFFF + id_base) & 0xFFFFFFFF)
                    _same((dists, ids), ivf.search(grouped, Q, centers, by_residual, empty[:nq], nprobe, k, id_base))
                    info = ix.info()
                    assert info["items"] == 0 and info["rows_scanned"] == 0 and info["ld"] == k
            for k, id_base in ((1, 0), (7, 1), (n + 2, 1)):
                got = ix.search(mixed, nprobe, k, id_base)
                _same(got, ivf.search(grouped, Q, centers, by_residual, mixed, nprobe, k, id_base), (nprobe, k))
                assert np.all(_bits(got[0])[rowless] == ivf.PAD_BITS) and np.all(_bits(got[0])[~rowless, 0] != ivf.PAD_BITS)
                assert ix.info()["rows_scanned"] == n * int((~rowless).sum())
        got = ix.search(mixed, 3, n + 2)               # the third probe reaches the rows for every query
        _same(got, ivf.search(grouped, Q, centers, by_residual, mixed, 3, n + 2))
        assert np.all(_bits(got[0])[:, n - 1] != ivf.PAD_BITS) and np.all(_bits(got[0])[:, n:] == ivf.PAD_BITS)

    for by_residual in (True, False):
        with _index(rq, Q, centers, by_residual) as ix:
            ix.set_codes(lists, codes)
            sequence(ix, by_residual)
            _lib.fill_scratch(0xA5)
            sequence(ix, by_residual)


# ---- 6. k past 65536, ids at the top of the range, the scratch refusal ---------------------------------------------------------------
def test_k_past_65536(rq):
    import rayuela_jl_amd.synth as synth
    _, _, centers, Xq = _data("sift", nlist=7)
    m, d, n = centers.shape[0], Xq.shape[1], 70000
    C = [centers[i] for i in range(m)]
    rng = np.random.default_rng(6)
    Q = Xq[3:6].copy() + rng.standard_normal((3, d)).astype(np.float32)
    Xq = Xq[:3]
    lists = rng.integers(0, 3, n)
    codes = synth.random_codes(n, m, seed=14)
    grouped = ivf.group(lists, codes, 3)
    for by_residual in (True, False):
        with _index(rq, Q, centers, by_residual) as ix:
            ix.set_codes(lists, codes)
            for nprobe in (2, 3):
                rows = ivf.ranked(grouped, Q, centers, by_residual, Xq, nprobe)
                for k in (65536, 65537, n, n + 1):
                    got = ix.search(Xq, nprobe, k)
                    _same(got, ivf.take(rows, k), (by_residual, nprobe, k))
                    if not by_residual and nprobe == 3 and k <= n:
                        _same(got, rq.linscan_pq(codes, Xq, C, 8 * m, k), ("linscan_pq", k))
            assert np.all(_bits(got[0])[:, n - 1] != ivf.PAD_BITS) and np.all(_bits(got[0])[:, n] == ivf.PAD_BITS)


def test_ids_at_the_top_of_the_range_and_the_scratch_refusal(rq):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    _, Q, centers, Xq = _data("sift", nlist=7)
    m, n = centers.shape[0], 500
    lists = np.random.default_rng(7).integers(0, 7, n)
    codes = synth.random_codes(n, m, seed=15)
    L = _lib.lib()
    for by_residual in (True, False):
        with _index(rq, Q, centers, by_residual) as ix:
            for id_offset in ((1 << 31) - 5, (1 << 32) - 1 - n):
                grouped = ivf.group(lists, codes, 7, id_offset=id_offset)
                ix.set_codes(lists, codes, id_offset=id_offset)
                _lists_equal(ix, grouped)
                for nprobe in (2, 7):
                    rows = ivf.ranked(grouped, Q, centers, by_residual, Xq, nprobe)
                    for id_base in (0, 1):
                        for k in (10, n + 2):
                            got = ix.search(Xq, nprobe, k, id_base)
                            _same(got, ivf.take(rows, k, id_base), (id_offset, nprobe, id_base, k))
                        # (the last search: k = n + 2, so padding is there) a real row and padding never share (dist, id)
                        real = _bits(got[0]) != ivf.PAD_BITS
                        assert np.all(got[1][~real] == (0xFFFFFFFF + id_base) & 0xFFFFFFFF) and (~real).any()
                        top = (got[1] == 0xFFFFFFFF) & real
                        if id_base == 1 and id_offset == (1 << 32) - 1 - n:
                            # row n - 1 carries 0xFFFFFFFF where its list is probed, padding carries 0
                            probed = [int((rows[q][1] == 0xFFFFFFFE).sum()) for q in range(Xq.shape[0])]
                            assert top.sum(axis=1).tolist() == probed and (nprobe < 7 or set(probed) == {1})
                        else:
                            assert not top.any()
            # one query whose keys cannot fit the bulk scratch: refused before anything is written, the base answers as before
            want = ivf.take(rows, 10, 1)
            dists, ids = np.full((1, 1), 7.0, np.float32), np.full((1, 1), 7, np.uint32)
            rc = L.rq_ivf_search(ix._h, dists.ctypes.data, ids.ctypes.data, Xq.ctypes.data, 1, 1, 1 << 30, 1)
            assert rc == RQ_EUNSUPPORTED and b"BULK_SCRATCH_BYTES" in L.rq_last_error()
            assert dists[0, 0] == 7.0 and ids[0, 0] == 7
            _same(ix.search(Xq, 7, 10), want, "after the refusal")
            _lists_equal(ix, grouped)


# ---- 7. host threads ------------------------------------------------------------------------------------------------------------------
def test_searches_a_build_and_the_exact_knn_from_four_host_threads(rq):
    """Two threads search one handle (its mutex, then the device lock), one builds and reads a handle of its own, one runs
    the exact k-nn, which takes the same bulk scratch slot: every answer is the single-threaded one, bit for bit."""
    from rayuela_jl_amd.knn import groundtruth
    X, Q, centers, Xq = _data("sift", nlist=7)
    grouped = ivf.build(X, Q, centers, True)[0]
    small = ivf.build(X[:1000], Q, centers, False, id_offset=5)[0]
    errs = []
    with _index(rq, Q, centers, True) as shared, _index(rq, Q, centers, False) as own:
        shared.build(X)
        want = {pk: shared.search(Xq, *pk) for pk in ((1, 10), (7, X.shape[0]))}
        for pk, w in want.items():
            _same(w, ivf.search(grouped, Q, centers, True, Xq, *pk), pk)
        gt = groundtruth(X, Xq, 10)

        def search(pk):
            _same(shared.search(Xq, *pk), want[pk], pk)

        def build():
            own.build(X[:1000], id_offset=5)
            _lists_equal(own, small)

        def knn():
            ids, dists = groundtruth(X, Xq, 10)
            assert np.array_equal(ids, gt[0]) and np.array_equal(dists.view(np.uint64), gt[1].view(np.uint64))

        jobs = [("search nprobe 1", lambda: search((1, 10))), ("search nprobe 7", lambda: search((7, X.shape[0]))),
                ("build", build), ("groundtruth", knn)]

        def worker(t):
            name, fn = jobs[t]
            try:
                for rnd in range(4):
                    try:
                        fn()
                    except AssertionError as e:
                        errs.append((name, rnd, str(e)[:200]))
            except Exception as e:   # noqa: BLE001
                errs.append((name, repr(e)))

        ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errs, errs[:5]
        for pk in want:                                # and the shared handle still answers
            search(pk)
