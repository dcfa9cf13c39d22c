"""CPU: the restatement of the IVFADC index (tests/ivf_oracle.py) against what the oracle already pins, and the argument checks
of the Python mirror (rayuela_jl_amd/IVF.py), which raise before the library is called.

With by_residual = 0 and nprobe = nlist every row is scanned with the query's own table, so the answer must be the compiled
reference's (the golden files) for ANY assignment of rows to lists: keys (dist, id) are unique and the storage order cannot matter."""
import numpy as np
import pytest

import ivf_oracle as ivf
from conftest import golden


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assignments(n):
    """(name, nlist, lists): random, all rows in one list, round-robin over every fourth list (the others stay empty)"""
    rng = np.random.default_rng(11)
    return [("random", 7, rng.integers(0, 7, n)), ("one_list", 5, np.full(n, 3)), ("round_robin", 9, (np.arange(n) % 3) * 4)]


@pytest.mark.parametrize("name", ["scan_sift_mini", "scan_all_ties"])
def test_full_probe_without_residual_is_the_reference_scan(oracle, name):
    g = golden(name)
    codes, centers, queries = g["codes"], g["centers"], g["queries"]
    n, d = codes.shape[0], queries.shape[1]
    for aname, nlist, lists in _assignments(n):
        Q = np.random.default_rng(nlist).standard_normal((nlist, d)).astype(np.float32)
        grouped = ivf.group(lists, codes, nlist)
        assert grouped[0][-1] == n and np.array_equal(np.sort(grouped[1]), np.arange(n, dtype=np.uint32))
        for K in g["Ks"]:
            dists, ids = ivf.search(grouped, Q, centers, False, queries, nlist, int(K), id_base=0)
            assert np.array_equal(ids, g["ids_K%d" % K]), (name, aname, K)
            assert np.array_equal(_bits(dists), _bits(g["dists_K%d" % K])), (name, aname, K)


def _small(n=400, d=16, m=4, nlist=6, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = X[rng.choice(n, nlist, replace=False)].copy()
    centers = rng.standard_normal((m, 256, d // m)).astype(np.float32)
    Xq = rng.standard_normal((5, d)).astype(np.float32)
    return X, Q, centers, Xq


def test_build_is_encode_pq_and_the_rvq_residual(oracle):
    X, Q, centers, _ = _small()
    lists = ivf.lists_of(X, Q)
    assert np.array_equal(lists, oracle.encode_pq(X, Q, 1, Q.shape[0])[:, 0])
    _, _, Xr = oracle.encode_rvq(X, Q[None], with_extras=True)
    assert np.array_equal(_bits(ivf.residuals(X, Q, lists)), _bits(Xr))
    (offsets, ids, codes), (l2, enc, arrival) = ivf.build(X, Q, centers, True, id_offset=1000)
    assert np.array_equal(l2, lists) and np.array_equal(arrival, oracle.encode_pq(Xr, centers, 4, 256))
    for j in range(Q.shape[0]):                       # grouped by list, ascending id inside a list
        rows = ids[offsets[j]:offsets[j + 1]].astype(np.int64) - 1000
        assert np.array_equal(rows, np.flatnonzero(lists == j))
        assert np.array_equal(codes[offsets[j]:offsets[j + 1]], arrival[rows])


def test_one_list_with_a_zero_centroid_makes_the_modes_equal(oracle):
    X, _, centers, Xq = _small()
    Q = np.zeros((1, X.shape[1]), dtype=np.float32)
    ga, _ = ivf.build(X, Q, centers, True)
    gb, _ = ivf.build(X, Q, centers, False)
    for a, b in zip(ga, gb):
        assert np.array_equal(a, b)
    for k in (1, 10, X.shape[0], X.shape[0] + 3):
        da, ia = ivf.search(ga, Q, centers, True, Xq, 1, k)
        db, ib = ivf.search(gb, Q, centers, False, Xq, 1, k)
        assert np.array_equal(ia, ib) and np.array_equal(_bits(da), _bits(db))
        if k > X.shape[0]:
            assert np.all(_bits(da)[:, X.shape[0]:] == ivf.PAD_BITS) and np.all(ia[:, X.shape[0]:] == 0)   # 0xFFFFFFFF + 1 wraps


def test_probe_order_on_equal_centroids_and_nan():
    X, Q, _, Xq = _small(nlist=8)
    Q[5] = Q[2]                              # identical centroids: the lower index first, and adjacent
    order = ivf.probe_order(Xq, Q)
    for row in order:
        at = int(np.flatnonzero(row == 2)[0])
        assert row[at + 1] == 5
    Q[1, 3] = np.nan                         # a NaN value sorts behind every number, +Inf included
    Q[6, :] = np.float32(3e30)               # |c|^2 overflows: the value is +Inf
    U = ivf.coarse_u(Xq, Q)
    assert np.all(np.isnan(U[:, 1])) and np.all(np.isposinf(U[:, 6]))
    order = ivf.probe_order(Xq, Q)
    assert np.all(order[:, -1] == 1) and np.all(order[:, -2] == 6)
    # ... while the build's argmin reads the NaN as 0 (the encode's clamp): a row goes to the NaN list unless another value is 0 first
    assert np.all(ivf.lists_of(Xq, Q) <= 1)


def test_tiled_search_and_one_ranking_for_every_k_equal_the_plain_search(oracle):
    """The helpers of the GPU tests with many queries or many k: search_tiled on a tiling of distinct queries and take() off one
    ranked() list are the plain search of the tiled queries, padding included; item_counts and union_sizes by hand."""
    X, Q, centers, Xq = _small()
    Xq = Xq.copy()
    Xq[3, 2] = np.nan                        # a query without a comparable row: padding from slot 0
    tile = np.random.default_rng(4).integers(0, Xq.shape[0], 23)
    tile[:5] = np.arange(5)
    for by_residual in (True, False):
        grouped, _ = ivf.build(X, Q, centers, by_residual, id_offset=9)
        for nprobe in (1, 2, 6):
            rows = ivf.ranked(grouped, Q, centers, by_residual, Xq, nprobe)
            for k, id_base in ((1, 0), (7, 1), (X.shape[0] + 2, 1)):
                plain = ivf.search(grouped, Q, centers, by_residual, Xq[tile], nprobe, k, id_base)
                tiled = ivf.search_tiled(grouped, Q, centers, by_residual, Xq, tile, nprobe, k, id_base)
                cut = ivf.take(rows, k, id_base)
                assert np.array_equal(plain[1], tiled[1]) and np.array_equal(_bits(plain[0]), _bits(tiled[0]))
                assert np.array_equal(plain[1], cut[1][tile]) and np.array_equal(_bits(plain[0]), _bits(cut[0][tile]))
                assert np.all(_bits(plain[0])[tile == 3] == ivf.PAD_BITS)
            sizes = np.diff(grouped[0])
            probes = ivf.probe_order(Xq, Q)[:, :nprobe]
            for seg in (1, 7, 4096):
                want = [sum(-(-int(sizes[p]) // seg) for p in probes[q]) for q in range(Xq.shape[0])]
                assert ivf.item_counts(grouped, Q, Xq, nprobe, seg).tolist() == want
            assert ivf.union_sizes(grouped, Q, Xq, nprobe).tolist() == [int(sizes[probes[q]].sum()) for q in range(Xq.shape[0])]


def test_mirror_argument_checks_raise_before_the_library(rq):
    from rayuela_jl_amd.IVF import IvfIndex
    Q = np.zeros((4, 12), dtype=np.float32)
    with pytest.raises(ValueError):          # d % m != 0
        IvfIndex(Q, [np.zeros((256, 2), np.float32)] * 5)
    with pytest.raises(TypeError):           # float64 data never dispatches
        IvfIndex(Q.astype(np.float64), [np.zeros((256, 3), np.float32)] * 4)
    ix = IvfIndex._unbound(nlist=4, d=12, m=4)
    Xq = np.zeros((2, 12), dtype=np.float32)
    with pytest.raises(ValueError):
        ix.search(Xq, 5, 1)                  # nprobe > nlist
    with pytest.raises(ValueError):
        ix.search(Xq, 0, 1)
    with pytest.raises(ValueError):
        ix.search(Xq, 1, 0)
    with pytest.raises(ValueError):
        ix.search(Xq[:, :8], 1, 1)
    B = np.zeros((3, 4), dtype=np.uint8)
    with pytest.raises(ValueError):
        ix.set_codes(np.array([0, 4, 1]), B)          # list id out of range
    with pytest.raises(ValueError):
        ix.set_codes(np.array([0, -1, 1]), B)
    with pytest.raises(ValueError):
        ix.set_codes(np.array([0, 1, 2]), B[:, :3])   # codes of the wrong shape
    with pytest.raises(ValueError):
        ix.set_codes(np.array([0, 1]), B)
    with pytest.raises(ValueError):
        ix.set_codes(np.array([0, 1, 2]), B, id_offset=0xFFFFFFFF)
    with pytest.raises(ValueError):
        ix.build(np.zeros((3, 8), dtype=np.float32))
