"""CPU: pins tests/scan_wide_oracle.py, the restatement of the ADC scan over 16-bit codes, to the committed oracle -- at h = 256
against oracle.linscan_aqd_query on the golden scan fixtures (ties, duplicates and k = n included), and its block-built table
against a direct numpy evaluation above 256 -- and checks what needs no GPU of the new entry points: the argument checks of
linscan_pq_u16 / linscan_opq_u16 and the table placements of rq_scan_wide_plan."""
import ctypes

import numpy as np
import pytest

import scan_wide_oracle as swo
import scan_wide_stream_cases  # noqa: F401  (registers the stream cases of the wide scan entry points)
from conftest import golden

SCAN_CASES = ["scan_sift_mini", "scan_deep_mini", "scan_all_ties", "scan_dups", "scan_k_eq_n"]


@pytest.mark.parametrize("name", SCAN_CASES)
def test_restatement_equals_the_oracle_at_h256(oracle, name):
    g = golden(name)
    codes = g["codes"].astype(np.int16)
    T = swo.tables(oracle, g["centers"], g["queries"])
    for K in g["Ks"]:
        K = int(K)
        d0, i0 = oracle.linscan_aqd_query(g["codes"], g["centers"], g["queries"], K)
        assert np.array_equal(i0, g["ids_K%d" % K]) and np.array_equal(d0.view(np.uint32), g["dists_K%d" % K].view(np.uint32))
        bits, ids, keys = swo.scan_tables(T, codes, K)
        assert np.array_equal(ids, i0), (name, K)
        assert np.array_equal(bits, d0.view(np.uint32)), (name, K)
        assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), i0)
        assert np.array_equal((keys >> np.uint64(32)).astype(np.uint32), swo.nf.ordered_bits(d0))


@pytest.mark.parametrize("m,h,sub", [(3, 257, 6), (2, 1000, 16), (5, 1000, 1)])
def test_block_built_table_equals_the_direct_evaluation(oracle, m, h, sub):
    rng = np.random.default_rng(h + sub)
    centers = rng.standard_normal((m, h, sub)).astype(np.float32)
    queries = rng.standard_normal((4, m * sub)).astype(np.float32)
    T = swo.tables(oracle, centers, queries)
    assert T.shape == (4, m, h)
    assert np.array_equal(T.view(np.uint32), swo.direct_tables(centers, queries).view(np.uint32))


def test_bad_codes_and_short_lists_of_the_restatement(oracle):
    rng = np.random.default_rng(3)
    m, h, sub, n = 2, 300, 2, 50
    centers = rng.standard_normal((m, h, sub)).astype(np.float32)
    queries = rng.standard_normal((2, m * sub)).astype(np.float32)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    codes[7, 1], codes[9, 0], codes[11, 0] = h, -1, 32767
    bits, ids, keys = swo.scan(oracle, codes, centers, queries, n, id_base=1, id_offset=5)
    assert not np.isin(ids[:, :n - 3], [7 + 6, 9 + 6, 11 + 6]).any()
    assert np.all(bits[:, n - 3:] == swo.nf.PAD_BITS) and np.all(ids[:, n - 3:] == 0) and np.all(keys[:, n - 3:] == swo.nf.KEY_MAX)
    assert np.array_equal(np.sort(ids[0, :n - 3]), np.setdiff1d(np.arange(n), [7, 9, 11]) + 6)


def test_linscan_u16_argument_checks(rq):
    C = [np.zeros((300, 2), np.float32)] * 2
    X = np.zeros((1, 4), np.float32)
    with pytest.raises(OverflowError):      # zero-based (uint16) code == h
        rq.linscan_pq_u16(np.array([[0, 300]], dtype=np.uint16), X, C, 1)
    with pytest.raises(OverflowError):      # zero-based int16 code < 0
        rq.linscan_pq_u16(np.array([[0, -1]], dtype=np.int16), X, C, 1)
    with pytest.raises(OverflowError):      # one-based (any other integer dtype) code 0: src/Linscan.jl:35 B .- 1
        rq.linscan_pq_u16(np.array([[0, 1]], dtype=np.int32), X, C, 1)
    with pytest.raises(OverflowError):      # one-based code h + 1
        rq.linscan_opq_u16(np.array([[1, 301]], dtype=np.int64), X, C, np.eye(4, dtype=np.float32), 1)
    with pytest.raises(TypeError):
        rq.linscan_pq_u16(np.zeros((1, 2), np.float32), X, C, 1)
    with pytest.raises(ValueError):         # Cint(d/m) InexactError, src/Linscan.jl:23
        rq.linscan_pq_u16(np.zeros((4, 3), np.uint16), X, [np.zeros((300, 1), np.float32)] * 3, 1)
    with pytest.raises(ValueError):         # codebooks of the wrong width
        rq.linscan_pq_u16(np.zeros((4, 2), np.uint16), X, [np.zeros((300, 3), np.float32)] * 2, 1)
    with pytest.raises(ValueError):         # h beyond what an Int16 code names
        rq.linscan_pq_u16(np.zeros((4, 2), np.uint16), X, [np.zeros((32768, 2), np.float32)] * 2, 1)
    with pytest.raises(ValueError):         # k > n
        rq.linscan_pq_u16(np.zeros((4, 2), np.uint16), X, C, 5)
    with pytest.raises(ValueError):         # R of the wrong shape
        rq.linscan_opq_u16(np.zeros((4, 2), np.uint16), X, C, np.eye(3, dtype=np.float32), 1)


TIERS = [  # (m, h) -> queries per gather, table in LDS, queries per group, LDS bytes
    ((8, 1024), (4, 1, 4, 131072)),
    ((8, 2048), (2, 1, 2, 131072)),
    ((8, 4096), (1, 1, 1, 131072)),
    ((16, 4096), (4, 0, 4, 0)),
    ((1, 1), (4, 1, 4, 16)),
    ((1, 32767), (1, 1, 1, 131072)),      # 131068 bytes of entries, rounded up to whole 16-byte loads
    ((2, 32767), (4, 0, 4, 0)),
    ((32, 257), (2, 1, 2, 65792)),
]


@pytest.mark.parametrize("shape,want", TIERS)
def test_scan_wide_plan_placements(rq, shape, want):
    from rayuela_jl_amd import _lib
    p = _lib.scan_wide_plan(*shape)
    assert (p["qpg"], p["in_lds"], p["qg"], p["lds_bytes"]) == want, p


def test_scan_wide_plan_argument_errors(rq):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 4)(*([-7] * 4))
    ptr = ctypes.cast(out, ctypes.c_void_p)
    assert L.rq_scan_wide_plan(8, 1024, None, 4) == -1 and L.rq_scan_wide_plan(8, 1024, ptr, 3) == -1
    for m, h in ((0, 300), (33, 300), (8, 0), (8, 32768)):
        assert L.rq_scan_wide_plan(m, h, ptr, 4) == -2, (m, h)
    assert list(out) == [-7] * 4
