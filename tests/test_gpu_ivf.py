"""GPU: the IVFADC index (rq_ivf_*, rayuela_jl_amd/IVF.py) against its restatement (tests/ivf_oracle.py) and against
rq_linscan_pq.  Every comparison is exact: ids, distance bits and padding."""
import functools

import numpy as np
import pytest

import ivf_oracle as ivf

pytestmark = pytest.mark.gpu

N, D, M = 3000, 32, 4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), ("ids", what)
    assert np.array_equal(_bits(got[0]), _bits(want[0])), ("dists", what)


@functools.lru_cache(maxsize=None)
def _data(kind, n=N, d=D, m=M, nlist=7, nq=33):
    """X, Q (rows of X), centers [m][256][d/m] (a few Lloyd steps on residuals of a sample), queries; read-only"""
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(d * 1000 + nlist)
    if kind == "sift":            # integer-valued: exact ties occur
        X, Xq = synth.sift_like(n, d, seed=5, ncentres=64), synth.sift_like(nq, d, seed=6, ncentres=64)
    else:
        X, Xq = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    Q = X[rng.choice(n, nlist, replace=False)].copy()
    R = ivf.residuals(X, Q, ivf.lists_of(X, Q))
    centers = np.stack(synth.codebooks(R, m, 256, seed=9, iters=1, sample=2000)).astype(np.float32)
    for a in (X, Q, centers, Xq):
        a.setflags(write=False)
    return X, Q, centers, Xq


@functools.lru_cache(maxsize=None)
def _oracle_base(kind, by_residual, nlist=7, d=D, m=M, id_offset=0):
    X, Q, centers, _ = _data(kind, d=d, m=m, nlist=nlist)
    return ivf.build(X, Q, centers, by_residual, id_offset)[0]


def _index(rq, Q, centers, by_residual):
    return rq.IvfIndex(Q, [centers[i] for i in range(centers.shape[0])], by_residual=by_residual)


def _lists_equal(ix, want):
    off, ids, codes = ix.lists()
    assert np.array_equal(off, want[0]) and np.array_equal(ids, want[1]) and np.array_equal(codes, want[2])


# ---- build --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sift", "gauss"])
@pytest.mark.parametrize("nlist", [1, 7, 37, 300])           # 300 > 256: the wide coarse encode
def test_build_equals_the_oracle(rq, kind, nlist):
    X, Q, centers, _ = _data(kind, nlist=nlist)
    for by_residual in (True, False):
        with _index(rq, Q, centers, by_residual) as ix:
            for id_offset in (0, 1 << 31):
                ix.build(X, id_offset=id_offset)
                _lists_equal(ix, _oracle_base(kind, by_residual, nlist=nlist, id_offset=id_offset))
            info = ix.info()
            sizes = np.diff(_oracle_base(kind, by_residual, nlist=nlist)[0])
            assert (info["n"], info["nlist"], info["m"], info["d"], info["by_residual"]) == (N, nlist, M, D, int(by_residual))
            assert info["largest_list"] == sizes.max() and info["empty_lists"] == int((sizes == 0).sum())


def test_build_with_equal_centroids_and_more_lists_than_rows(rq):
    X, Q, centers, _ = _data("sift", nlist=7)
    Q = Q.copy()
    Q[4] = Q[1]                                   # the second of two identical centroids stays empty
    with _index(rq, Q, centers, True) as ix:
        ix.build(X)
        want = ivf.build(X, Q, centers, True)[0]
        _lists_equal(ix, want)
        assert want[0][5] == want[0][4] and want[0][2] > want[0][1]
    X5 = np.ascontiguousarray(X[np.arange(N) % 5])              # 5 distinct rows, 37 lists
    _, Q37, _, _ = _data("sift", nlist=37)
    with _index(rq, Q37, centers, True) as ix:
        ix.build(X5)
        want = ivf.build(X5, Q37, centers, True)[0]
        _lists_equal(ix, want)
        assert int((np.diff(want[0]) > 0).sum()) <= 5


def test_build_in_row_chunks_and_sort_pieces(rq):
    X, Q, centers, _ = _data("gauss", nlist=37)
    want = _oracle_base("gauss", True, nlist=37)
    try:
        with _index(rq, Q, centers, True) as ix:
            for rows, piece in ((700, 0), (0, 999), (701, 512)):
                rq.set_tuning("IVF_BUILD_ROWS", rows)
                rq.set_tuning("IVF_SORT_ROWS", piece)
                ix.build(X)
                _lists_equal(ix, want)
    finally:
        rq.reset_tuning("IVF_BUILD_ROWS")
        rq.reset_tuning("IVF_SORT_ROWS")


# ---- search against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_residual", [True, False])
@pytest.mark.parametrize("kind,nlist", [("sift", 7), ("gauss", 37)])
def test_search_equals_the_oracle(rq, kind, nlist, by_residual):
    X, Q, centers, Xq = _data(kind, nlist=nlist)
    grouped = _oracle_base(kind, by_residual, nlist=nlist)
    with _index(rq, Q, centers, by_residual) as ix:
        ix.build(X)
        for nprobe in (1, 3, nlist):
            umin = int(ivf.union_sizes(grouped, Q, Xq, nprobe).min())
            for i, k in enumerate(sorted({1, 10, max(1, umin), umin + 1, N})):
                id_base = i & 1
                want = ivf.search(grouped, Q, centers, by_residual, Xq, nprobe, k, id_base)
                _same(ix.search(Xq, nprobe, k, id_base), want, (nprobe, k))
                if k == umin + 1:                 # the shortest union runs out: padding appears
                    assert (_bits(want[0])[:, -1] == ivf.PAD_BITS).any()
                    assert set(want[1][_bits(want[0]) == ivf.PAD_BITS].tolist()) == {(0xFFFFFFFF + id_base) & 0xFFFFFFFF}
                for nq in (1, 9):
                    got = ix.search(Xq[:nq], nprobe, k, id_base)
                    _same(got, (want[0][:nq], want[1][:nq]), (nprobe, k, nq))
        info = ix.info()
        # the last search: nq = 9, every list probed, k = N + 1 (one more than the union), so one padding slot per row of keys
        assert info["ld"] == N + 1 and info["items"] >= 9 and info["rows_scanned"] == 9 * N


@pytest.mark.parametrize("m", [8, 16, 3, 12])               # 3 and 12: rows padded to 4 and 16 bytes on the device
def test_search_m8_m16_at_d96(rq, m):
    X, Q, centers, Xq = _data("gauss", d=96, m=m, nlist=7)
    for by_residual in (True, False):
        grouped = _oracle_base("gauss", by_residual, nlist=7, d=96, m=m)
        with _index(rq, Q, centers, by_residual) as ix:
            ix.build(X)
            _lists_equal(ix, grouped)
            for nprobe, k in ((3, 10), (7, N), (1, 100)):
                _same(ix.search(Xq, nprobe, k), ivf.search(grouped, Q, centers, by_residual, Xq, nprobe, k), (m, nprobe, k))


# ---- list sizes through set_codes ---------------------------------------------------------------------------------------------------
def test_list_sizes_segments_and_batches(rq):
    import rayuela_jl_amd.synth as synth
    S = 64
    _, Q6, centers, Xq = _data("sift", nlist=6)
    Xq = Xq[:9]
    cases = []
    sizes = [0, 1, S - 1, S, S + 1, 3 * S + 2]
    lists = np.repeat(np.arange(6), sizes)
    lists = lists[np.random.default_rng(1).permutation(lists.size)]
    cases.append((Q6, lists))
    _, Q7, _, _ = _data("sift", nlist=7)
    half = np.where(np.arange(N) % 2 == 0, 2, np.random.default_rng(2).integers(0, 7, N))    # half of all rows in list 2
    cases.append((Q7, half))
    try:
        for Q, lists in cases:
            codes = synth.random_codes(lists.size, M, seed=lists.size)
            grouped = ivf.group(lists, codes, Q.shape[0], id_offset=17)
            for by_residual in (True, False):
                with _index(rq, Q, centers, by_residual) as ix:
                    ix.set_codes(lists, codes, id_offset=17)
                    _lists_equal(ix, grouped)
                    for nprobe, k in ((Q.shape[0], 50), (2, lists.size), (Q.shape[0], lists.size + 5)):
                        want = ivf.search(grouped, Q, centers, by_residual, Xq, nprobe, k)
                        for seg, batch in ((S, 0), (S, 4), (0, 0), (1, 4), (S, 1)):
                            rq.set_tuning("IVF_SEGMENT_ROWS", seg) if seg else rq.reset_tuning("IVF_SEGMENT_ROWS")
                            rq.set_tuning("IVF_BATCH_QUERIES", batch) if batch else rq.reset_tuning("IVF_BATCH_QUERIES")
                            _same(ix.search(Xq, nprobe, k), want, (nprobe, k, seg, batch))
                            info = ix.info()
                            if batch:
                                assert info["batch"] == batch
                            if seg == S and nprobe == Q.shape[0] and batch == 0:
                                per_query = int(np.ceil(np.bincount(lists, minlength=Q.shape[0]) / S).sum())
                                assert info["items"] == per_query * Xq.shape[0]
    finally:
        rq.reset_tuning("IVF_SEGMENT_ROWS")
        rq.reset_tuning("IVF_BATCH_QUERIES")


# ---- equivalence with the exhaustive scan ----------------------------------------------------------------------------------------------
def test_full_probe_without_residual_equals_linscan_pq(rq):
    import rayuela_jl_amd.synth as synth
    _, _, centers, Xq = _data("sift", nlist=7)
    codes = synth.random_codes(N, M, seed=3)
    C = [centers[i] for i in range(M)]
    rng = np.random.default_rng(11)
    for nlist, lists in ((7, rng.integers(0, 7, N)), (5, np.full(N, 3)), (9, (np.arange(N) % 3) * 4)):
        Q = rng.standard_normal((nlist, D)).astype(np.float32)
        with _index(rq, Q, centers, False) as ix:
            ix.set_codes(lists, codes)
            for k in (1, 100, N):
                _same(ix.search(Xq, nlist, k), rq.linscan_pq(codes, Xq, C, 8 * M, k), (nlist, k))


# ---- ties and exact zeros --------------------------------------------------------------------------------------------------------------
def test_duplicate_rows_order_by_id(rq):
    _, Q, centers, Xq = _data("sift", nlist=7)
    n = 600
    codes = np.tile(np.array([[3, 200, 17, 99]], dtype=np.uint8), (n, 1))      # every row the same code
    codes[::7] = [4, 4, 4, 4]
    lists = np.arange(n) % 2 * 3                                               # lists 0 and 3, both probed at nprobe = 7
    grouped = ivf.group(lists, codes, 7)
    with _index(rq, Q, centers, False) as ix:
        ix.set_codes(lists, codes)
        for k in (5, 300, n):
            got = ix.search(Xq[:9], 7, k, id_base=0)
            _same(got, ivf.search(grouped, Q, centers, False, Xq[:9], 7, k, id_base=0), k)
            for q in range(9):                     # equal distances: ascending id, across the two lists
                d, i = _bits(got[0][q]), got[1][q].astype(np.int64)
                assert np.all((d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & (i[1:] > i[:-1])))
    with _index(rq, Q, centers, True) as ix:       # inside one list the residual query is shared: the same rule
        ix.set_codes(lists, codes)
        _same(ix.search(Xq[:9], 7, n, id_base=0), ivf.search(grouped, Q, centers, True, Xq[:9], 7, n, id_base=0))


def test_queries_equal_to_a_centroid_and_a_row_give_zero(rq):
    X, Q, centers, _ = _data("sift", nlist=7)
    centers = centers.copy()
    centers[:, 0, :] = 0                          # codeword 0 of every table is the zero vector
    with _index(rq, Q, centers, True) as ix:
        ix.build(X)                               # the centroids are rows of X: their residual is 0, their codes are all 0
        grouped = ivf.build(X, Q, centers, True)[0]
        _lists_equal(ix, grouped)
        got = ix.search(Q, 1, 3, id_base=0)
        _same(got, ivf.search(grouped, Q, centers, True, Q, 1, 3, id_base=0))
        assert np.all(_bits(got[0])[:, 0] == 0)


# ---- non-finite queries and centroids -----------------------------------------------------------------------------------------------------
def test_nonfinite_queries_and_centroids(rq):
    X, Q, centers, Xq = _data("gauss", nlist=7)
    Xn = Xq[:6].copy()
    Xn[0, 5] = np.nan
    Xn[1, 0] = np.inf
    Xn[2, 31] = -np.inf
    Xn[3, :] = np.nan
    Xn[4, 8:16] = np.inf
    for by_residual in (True, False):
        grouped = _oracle_base("gauss", by_residual, nlist=7)
        with _index(rq, Q, centers, by_residual) as ix:
            ix.build(X)
            for nprobe, k in ((1, 10), (3, 40), (7, N)):
                want = ivf.search(grouped, Q, centers, by_residual, Xn, nprobe, k)
                _same(ix.search(Xn, nprobe, k), want, (by_residual, nprobe, k))
                assert np.all(_bits(want[0])[0] == ivf.PAD_BITS) and np.all(want[1][0] == 0)    # nothing comparable: all padding
        # a centroid holding Inf: its value is +Inf or NaN per query, the residual query of its list is non-finite.  The base comes
        # through set_codes: which list a row takes under a non-finite codebook entry is left open by the encode's contract
        # (include/rayuela_hip.h, "Non-finite inputs of the encode", point 3)
        Qi = Q.copy()
        Qi[2, 7] = np.inf
        lists, _, arrival = ivf.build(X, Q, centers, by_residual)[1]
        grouped = ivf.group(lists, arrival, 7)
        with _index(rq, Qi, centers, by_residual) as ix:
            ix.set_codes(lists, arrival)
            _lists_equal(ix, grouped)
            for nprobe in (2, 7):
                _same(ix.search(Xn, nprobe, 20), ivf.search(grouped, Qi, centers, by_residual, Xn, nprobe, 20), ("inf", nprobe))


# ---- replacement, errors, scratch ------------------------------------------------------------------------------------------------------
def test_replacement_errors_and_stale_scratch(rq):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    X, Q, centers, Xq = _data("sift", nlist=7)
    L = _lib.lib()
    with _index(rq, Q, centers, True) as ix:
        with pytest.raises(rq.RayuelaHipError):            # no base yet: an error code, not a fault
            ix.search(Xq, 1, 1)
        d = np.empty((1, 1), np.float32)
        i = np.empty((1, 1), np.uint32)
        assert L.rq_ivf_search(ix._h, d.ctypes.data, i.ctypes.data, Xq.ctypes.data, 1, 1, 1, 1) == -1
        ix.build(X)
        first = _oracle_base("sift", True, nlist=7)
        _same(ix.search(Xq, 7, N), ivf.search(first, Q, centers, True, Xq, 7, N))          # the larger search
        want = ivf.search(first, Q, centers, True, Xq[:3], 1, 5)
        _same(ix.search(Xq[:3], 1, 5), want, "after a larger search")
        _lib.fill_scratch(0xA5)
        _same(ix.search(Xq[:3], 1, 5), want, "filled scratch")
        # a failed set_codes (list id out of range, past the mirror's own check) leaves the base searchable
        codes = synth.random_codes(500, M, seed=8)
        bad = np.zeros(500, dtype=np.uint32)
        bad[499] = 7
        assert L.rq_ivf_set_codes(ix._h, bad.ctypes.data, codes.ctypes.data, 500, 0) == -1
        assert b"499" in L.rq_last_error()
        _same(ix.search(Xq[:3], 1, 5), want, "after a refused set_codes")
        _lists_equal(ix, first)
        # set_codes replaces the base, a second build replaces it again
        lists = np.arange(500) % 7
        ix.set_codes(lists, codes)
        second = ivf.group(lists, codes, 7)
        _lists_equal(ix, second)
        _same(ix.search(Xq, 3, 600), ivf.search(second, Q, centers, True, Xq, 3, 600))
        ix.build(X[:1000], id_offset=5)
        third = ivf.build(X[:1000], Q, centers, True, id_offset=5)[0]
        _lists_equal(ix, third)
        _same(ix.search(Xq, 2, 10), ivf.search(third, Q, centers, True, Xq, 2, 10))
        assert ix.info()["n"] == 1000
    with pytest.raises(rq.RayuelaHipError):                # n + id_offset past 2^32 - 1, refused by the library too
        with _index(rq, Q, centers, True) as ix:
            _lib.check(L.rq_ivf_build(ix._h, X.ctypes.data, 10, 0xFFFFFFFF))
