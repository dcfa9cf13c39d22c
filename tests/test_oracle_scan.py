"""CPU: pins oracle/rq_oracle.c (scan) against the reference's outputs.

The golden .npz files hold the outputs of the REAL reference scan (oracle/_ref, built by oracle/Makefile from the
reference's deps/src/linscan_aqd.cpp -- see tests/gen_golden.py).  The restatement is also checked on generated inputs
against the reference's answers for them, including the reference's 1e7-row chunked path
(deps/src/linscan_aqd.cpp:52-53,78-92): the answers stored in tests/golden/live_ref.npz, and live as well where oracle/_ref
is built.
"""
import numpy as np
import pytest

from conftest import golden

SCAN_CASES = ["scan_sift_mini", "scan_deep_mini", "scan_all_ties", "scan_dups", "scan_k_eq_n"]


@pytest.mark.parametrize("name", SCAN_CASES)
def test_oracle_scan_matches_reference_golden(oracle, name):
    g = golden(name)
    for K in g["Ks"]:
        dists, ids = oracle.linscan_aqd_query(g["codes"], g["centers"], g["queries"], int(K))
        assert np.array_equal(ids, g["ids_K%d" % K]), (name, K)
        assert np.array_equal(dists.view(np.uint32), g["dists_K%d" % K].view(np.uint32)), (name, K)


def test_all_ties_lowest_ids(oracle):
    g = golden("scan_all_ties")
    K = 17
    assert np.array_equal(g["ids_K%d" % K], np.tile(np.arange(K, dtype=np.uint32), (g["queries"].shape[0], 1)))


def test_oracle_lut_is_unfused_sequential(oracle):
    g = golden("scan_sift_mini")
    centers, q = g["centers"], g["queries"][0]
    lut = oracle.adc_lut(centers, q)
    m, h, sub = centers.shape
    exp = np.zeros((m, h), dtype=np.float32)
    for s in range(sub):
        diff = (centers[:, :, s] - q.reshape(m, sub)[:, s][:, None]).astype(np.float32)
        exp = (exp + (diff * diff).astype(np.float32)).astype(np.float32)
    assert np.array_equal(lut.view(np.uint32), exp.view(np.uint32))
    # distances: sequential f32 sum over sub-quantizers, checked on a few rows
    dist = oracle.adc_distances(g["codes"][:64], centers, q)
    acc = np.zeros(64, dtype=np.float32)
    for k in range(m):
        acc = (acc + lut[k, g["codes"][:64, k]]).astype(np.float32)
    assert np.array_equal(dist.view(np.uint32), acc.view(np.uint32))


LIVE_CASES = [(20000, 8, 16, 5, 1000), (3000, 16, 6, 4, 3000), (100, 4, 2, 7, 1), (1, 8, 4, 2, 1)]


def live_case(n, m, sub, nq, K):
    """inputs of test_oracle_vs_live_reference: (key in live_ref.npz, codes, centers, queries, K)"""
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(n + m)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=n)
    return "scan_%d_%d_%d_%d_%d" % (n, m, sub, nq, K), codes, centers, queries, K


def chunked_case():
    """inputs of test_oracle_vs_reference_chunked_path: n > 1e7 + K rows"""
    import rayuela_jl_amd.synth as synth
    n, m, sub, nq, K = 10_000_000 + 300_123, 2, 2, 2, 50
    centers = (synth.splitmix64(np.arange(m * 256 * sub, dtype=np.uint64)) % np.uint64(4)).astype(np.float32)
    centers = centers.reshape(m, 256, sub)
    queries = np.array([[0, 1, 2, 3], [3, 1, 0, 2]], dtype=np.float32)
    codes = synth.random_codes(n, m, seed=77)
    return "scan_chunked", codes, centers, queries, K


def reference_answer(oracle, key, codes, centers, queries, K):
    """the reference scan's (dists, ids) for these inputs: stored in live_ref.npz (tests/gen_golden.py), and where oracle/_ref
    is built the live reference must give exactly the stored answer"""
    g = golden("live_ref")
    d, i = g[key + "_d"], g[key + "_i"]
    if oracle.ref_available():
        d0, i0 = oracle.ref_linscan_aqd_query(codes, centers, queries, K)
        assert np.array_equal(i0, i) and np.array_equal(d0.view(np.uint32), d.view(np.uint32)), key
    return d, i


@pytest.mark.parametrize("n,m,sub,nq,K", LIVE_CASES)
def test_oracle_vs_live_reference(oracle, n, m, sub, nq, K):
    key, codes, centers, queries, K = live_case(n, m, sub, nq, K)
    d0, i0 = reference_answer(oracle, key, codes, centers, queries, K)
    d1, i1 = oracle.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i0, i1)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


def test_oracle_vs_reference_chunked_path(oracle):
    """n > 1e7 + K exercises the reference's carried-top-K chunking; the restatement (global
    lexicographic top-K) must give the same answer, ties included."""
    key, codes, centers, queries, K = chunked_case()
    d0, i0 = reference_answer(oracle, key, codes, centers, queries, K)
    d1, i1 = oracle.linscan_aqd_query(codes, centers, queries, K)
    assert np.array_equal(i0, i1)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
