"""CPU: tests/nonfinite_ref.py -- the plain restatement the GPU tests of the non-finite contract compare with -- pinned bit
for bit to the C oracle (and to the compiled reference where oracle/_ref is built) on inputs on which the reference is
defined (no NaN distance: finite, +-Inf norms, +-Inf in a CQ / PQ query and codebook, a 3e38 query coordinate whose 2 * q
overflows, tables in the denormal range), and to hand-written answers on the NaN rules themselves."""
import numpy as np
import pytest

import nonfinite_ref as nf

N, M, D, NQ, K, H = 20000, 8, 24, 12, 300, 256


def _aq_case(seed):
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((M * H, D)).astype(np.float32)
    q = rng.standard_normal((NQ, D)).astype(np.float32)
    codes = synth.random_codes(N, M, seed=seed)
    codes[N // 2:] = codes[rng.integers(0, 50, N - N // 2)]        # exact ties: the id decides
    nrm = (rng.random(N) * 40).astype(np.float32)
    return codes, cb, q, nrm


def _aq_inputs(kind, name):
    codes, cb, q, nrm = _aq_case(11)
    if name == "finite":
        pass
    elif name == "inf_norms":
        nrm[5::97] = np.inf
        nrm[11::89] = -np.inf
    elif name == "inf_query_and_codebook":       # CQ only: different coordinates, so no Inf - Inf
        q[3, 1] = np.inf
        q[9, D - 1] = -np.inf
        cb[5, 7] = np.inf
        cb[H * 3 + 200, 0] = -np.inf
    elif name == "q3e38":
        q[4, 2] = 3e38                           # 2 * q overflows in the LSQ table; (q - c)^2 overflows in the CQ table
        cb[:, 2] = np.abs(cb[:, 2]) + 0.5        # LSQ: every entry is -Inf then (mixed signs would be NaN rows)
    elif name == "denormal":
        cb *= np.float32(2e-21)                  # table entries ~1e-41: below the smallest normal f32 (1.18e-38)
        q *= np.float32(2e-21)
        nrm = (nrm * np.float32(1e-42)).astype(np.float32)
    else:
        raise KeyError(name)
    return codes, cb, q, (nrm if kind == "lsq" else None)


AQ_CASES = [("lsq", "finite"), ("lsq", "inf_norms"), ("lsq", "q3e38"), ("lsq", "denormal"),
            ("cq", "finite"), ("cq", "inf_query_and_codebook"), ("cq", "q3e38"), ("cq", "denormal")]


@pytest.mark.parametrize("kind,name", AQ_CASES)
def test_restatement_equals_the_oracle_aq(oracle, kind, name):
    codes, cb, q, nrm = _aq_inputs(kind, name)
    ref = nf.scan(kind, codes, cb, q, K, dbnorms=nrm, id_base=1)
    assert not (ref[0] == nf.PAD_BITS).any()                     # defined inputs: no row was dropped
    if name == "denormal":
        d = ref[0].view(np.float32)
        assert (d != 0).all() and (np.abs(d) < 1.17e-38).all()   # the answers themselves are denormal numbers
    variants = [False] + ([True] if oracle.ref_aq_available() else [])
    for use_ref in variants:
        if kind == "lsq":
            d0, i0 = oracle.linscan_lsq(codes, cb, q, nrm, K, use_ref=use_ref)
        else:
            d0, i0 = oracle.linscan_cq(codes, cb, q, K, use_ref=use_ref)
        assert nf.same(d0, i0, ref), (use_ref, nf.first_difference(d0, i0, ref))


@pytest.mark.parametrize("name", ["finite", "inf", "denormal"])
def test_restatement_equals_the_oracle_pq(oracle, name):
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(13)
    sub = 3
    centers = rng.standard_normal((M, 256, sub)).astype(np.float32)
    q = rng.standard_normal((NQ, M * sub)).astype(np.float32)
    codes = synth.random_codes(N, M, seed=13)
    codes[N // 2:] = codes[rng.integers(0, 50, N - N // 2)]
    if name == "inf":
        q[2, 0] = np.inf
        q[7, M * sub - 1] = -np.inf
        centers[1, 77, 1] = np.inf
        centers[M - 1, 3, 1] = -np.inf          # (not the coordinate of the -Inf query: Inf - Inf is a NaN)
    elif name == "denormal":
        centers *= np.float32(2e-21)
        q *= np.float32(2e-21)
    ref = nf.scan("pq", codes, centers, q, K)
    assert not (ref[0] == nf.PAD_BITS).any()
    d0, i0 = oracle.linscan_aqd_query(codes, centers, q, K)
    assert nf.same(d0, i0, ref), nf.first_difference(d0, i0, ref)
    if oracle.ref_available():
        d0, i0 = oracle.ref_linscan_aqd_query(codes, centers, q, K)
        assert nf.same(d0, i0, ref), nf.first_difference(d0, i0, ref)


# ---- the NaN rules on a dozen rows: all-zero codebooks, so a row's LSQ distance IS its norm -------------------------

def _bits(*vals):
    return np.array(vals, dtype=np.float32).view(np.uint32)


def _tiny(norm_bits):
    n = len(norm_bits)
    codes = (np.arange(n * 2).reshape(n, 2) % 4).astype(np.uint8)
    cb = np.zeros((2 * 4, 2), dtype=np.float32)
    q = np.ones((1, 2), dtype=np.float32)
    return codes, cb, q, np.array(norm_bits, dtype=np.uint32).view(np.float32)


def test_nan_rows_are_dropped_and_the_list_is_padded():
    P, Nn = nf.NAN_POS, nf.NAN_NEG
    f = lambda x: int(_bits(x)[0])
    #        row: 0       1   2        3   4       5        6          7   8       9        10  11
    norms = [f(2.0), P, f(-1.0), Nn, f(2.0), f(np.inf), f(-np.inf), P, f(-0.0), f(0.0), Nn, f(1e-40)]
    codes, cb, q, nrm = _tiny(norms)
    assert np.isnan(nrm[[1, 3, 7, 10]]).all() and (nrm.view(np.uint32)[[3, 10]] >> 31 == 1).all()
    # comparable rows in (dist, id) order: -Inf (6), -1 (2), -0 == +0 (8, 9: ties part by id), 1e-40 (11), 2 (0, 4), +Inf (5)
    want_ids = [6, 2, 8, 9, 11, 0, 4, 5]
    want_bits = [f(-np.inf), f(-1.0), f(0.0), f(0.0), f(1e-40), f(2.0), f(2.0), f(np.inf)]
    bits, ids, keys = nf.scan("lsq", codes, cb, q, 12, dbnorms=nrm, id_base=0, want_keys=True)
    assert ids[0].tolist() == want_ids + [0xFFFFFFFF] * 4
    assert bits[0].tolist() == want_bits + [nf.PAD_BITS] * 4              # -0 came back as +0, the padding as 0x7FFFFFFF
    assert keys[0, 8:].tolist() == [nf.KEY_MAX] * 4
    assert np.all(np.diff(keys[0, :8].astype(object)) > 0)               # the packed keys ascend with (dist, id)
    assert int(keys[0, 0]) == (0x007FFFFF << 32) | 6 and int(keys[0, 2]) == (0x80000000 << 32) | 8
    # a list that does not run out: no padding, the NaN rows still never appear
    bits, ids = nf.scan("lsq", codes, cb, q, 5, dbnorms=nrm, id_base=1)
    assert ids[0].tolist() == [i + 1 for i in want_ids[:5]] and bits[0].tolist() == want_bits[:5]
    # one-based padding id is 0 ("no row"); an id offset moves the rows, not the padding; keys stay zero-based
    bits, ids, keys = nf.scan("lsq", codes, cb, q, 10, dbnorms=nrm, id_base=1, id_offset=1000, want_keys=True)
    assert ids[0].tolist() == [i + 1001 for i in want_ids] + [0, 0]
    assert [int(k) & 0xFFFFFFFF for k in keys[0, :8]] == [i + 1000 for i in want_ids]


def test_all_rows_nan_is_all_padding():
    codes, cb, q, nrm = _tiny([nf.NAN_POS, nf.NAN_NEG] * 6)
    for id_base in (0, 1):
        bits, ids, keys = nf.scan("lsq", codes, cb, q, 7, dbnorms=nrm, id_base=id_base, want_keys=True)
        assert (bits == nf.PAD_BITS).all() and (ids == (0xFFFFFFFF + id_base) % 2 ** 32).all() and (keys == nf.KEY_MAX).all()


def test_a_nan_table_entry_drops_the_rows_that_use_it():
    codes, cb, q, _ = _tiny([0] * 12)
    cb[:] = np.arange(16, dtype=np.float32).reshape(8, 2)
    nf.put_bits(cb, (4 + 1, 0), nf.NAN_NEG)                                # code 1 of the second codebook
    for kind in ("cq", "lsq"):
        nrm = np.zeros(12, np.float32) if kind == "lsq" else None
        bits, ids = nf.scan(kind, codes, cb, q, 12, dbnorms=nrm)
        keep = np.flatnonzero(codes[:, 1] != 1)
        assert 0 < keep.size < 12
        assert sorted(ids[0, :keep.size].tolist()) == keep.tolist() and (ids[0, keep.size:] == 0xFFFFFFFF).all()
        d = bits[0, :keep.size].view(np.float32)
        assert not np.isnan(d).any() and np.all(np.diff(d) >= 0)
    # the NaN sign survives put_bits (a float assignment may not keep it) and both signs are NaN to the contract
    assert cb.view(np.uint32)[5, 0] == nf.NAN_NEG
