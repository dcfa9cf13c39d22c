"""CPU: the helper of the additive-quantizer scan over 16-bit codes (tests/aq_wide_oracle.py) pinned against the C oracle and,
where oracle/_ref is built, the compiled reference, at the table widths those take with byte codes (h = 256, 64, 100); the
argument checks of the new Python functions that raise before the library is touched; and the dispatch of the experiment
drivers at h > 256."""
import numpy as np
import pytest

import aq_wide_oracle as awo
import aq_wide_stream_cases  # noqa: F401 -- registers the stream cases of the new `void *stream` entry points
import norms_oracle as no
from conftest import golden


def _against(fn_ref, ref_args, ours, K):
    d0, i0 = fn_ref(*ref_args, K)
    bits, ids, _ = ours(K)
    assert np.array_equal(ids, i0.view(np.uint32)), K
    assert np.array_equal(bits, d0.view(np.uint32)), K


@pytest.mark.parametrize("name", ["aq_mini_m8", "aq_mini_m4"])
def test_helper_equals_the_oracle_on_the_golden_fixtures(oracle, name):
    g = golden(name)
    codes16 = g["codes"].astype(np.int16)
    for K in (int(k) for k in g["Ks"]):
        bits, ids, _ = awo.scan(codes16, g["codebooks"], g["queries"], K, g["dbnorms"], id_base=1)
        assert np.array_equal(ids, g["lsq_i%d" % K].view(np.uint32)) and np.array_equal(bits, g["lsq_d%d" % K].view(np.uint32))
        bits, ids, _ = awo.scan(codes16, g["codebooks"], g["queries"], K, None, id_base=1)
        assert np.array_equal(ids, g["cq_i%d" % K].view(np.uint32)) and np.array_equal(bits, g["cq_d%d" % K].view(np.uint32))


@pytest.mark.parametrize("h", [256, 64, 100])
@pytest.mark.parametrize("integer", [False, True])
def test_helper_equals_the_oracle_on_seeded_data(oracle, h, integer):
    """Gaussian data, and small integers: exact sums, so many rows tie and the (dist, id) order is what is compared."""
    n, m, d, nq = 4001, 5, 30, 3
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 7 * h + integer, integer=integer)
    if integer:
        nrm = np.round(nrm).astype(np.float32)
    cb = C.reshape(m * h, d)
    for K in (1, 100, n):
        for use_ref in ([False, True] if oracle.ref_aq_available() else [False]):
            _against(lambda *a: oracle.linscan_lsq(*a, use_ref=use_ref), (codes.astype(np.uint8), cb, q, nrm),
                     lambda K: awo.scan(codes, C, q, K, nrm, id_base=1), K)
            _against(lambda *a: oracle.linscan_cq(*a, use_ref=use_ref), (codes.astype(np.uint8), cb, q),
                     lambda K: awo.scan(codes, C, q, K, None, id_base=1), K)


def test_helper_rules_beyond_the_reference():
    """A code outside [0, h) makes its row no neighbour; a NaN norm likewise; the short list ends in the padding pair."""
    codes, C, q, nrm = awo.case(40, 3, 300, 5, 2, 3)
    codes[5, 1], codes[6, 0], codes[7, 2] = 300, -1, 32767
    nrm[9] = np.nan
    bits, ids, keys = awo.scan(codes, C, q, 40, nrm)
    assert not np.isin(ids[:, :36], [5, 6, 7, 9]).any()
    assert (ids[:, 36:] == 0xFFFFFFFF).all() and (bits[:, 36:] == 0x7FFFFFFF).all() and (keys[:, 36:] == 0xFFFFFFFFFFFFFFFF).all()
    assert sorted(ids[0, :36].tolist()) == [r for r in range(40) if r not in (5, 6, 7, 9)]


def test_wide_quantize_equals_the_byte_helper_and_the_findmin_loop():
    cases = no.quant_cases()
    for name, (norms, cb) in cases.items():
        assert np.array_equal(awo.quantize(norms, cb), no.quantize(norms, cb).astype(np.int16)), name
    rng = np.random.default_rng(8)
    norms = rng.integers(0, 2000, 300).astype(np.float32)
    cb = rng.permutation(np.repeat(np.arange(0, 2000, 4), 2)).astype(np.float32)      # 1000 entries, every value twice
    got = awo.quantize(norms, cb)
    want = no.findmin_loop(norms[:40], cb[:200])
    assert np.array_equal(awo.quantize(norms[:40], cb[:200]), want.astype(np.int16))
    assert got.dtype == np.int16 and got.max() > 255
    first = {v: int(np.flatnonzero(cb == v)[0]) for v in np.unique(cb)}
    exact = np.isin(norms, cb)
    assert all(got[i] == first[norms[i]] for i in np.flatnonzero(exact))


# ---- the Python mirrors: checks that raise before the library is touched ---------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from rayuela_jl_amd import _lib

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)


def test_u16_scan_argument_checks(no_library):
    from rayuela_jl_amd import Linscan
    rng = np.random.default_rng(0)
    m, h, d, n, nq = 3, 300, 6, 20, 2
    C = [rng.standard_normal((h, d)).astype(np.float32) for _ in range(m)]
    X = rng.standard_normal((nq, d)).astype(np.float32)
    B0 = rng.integers(0, h, (n, m)).astype(np.uint16)
    nrm = np.zeros(n, dtype=np.float32)
    R = np.eye(d, dtype=np.float32)
    for fn, args in ((Linscan.linscan_lsq_u16, (nrm, R)), (Linscan.linscan_cq_u16, ()),
                     (Linscan.linscan_lsq_cbnorms_u16, (np.zeros(7, dtype=np.float32), R))):
        with pytest.raises(OverflowError):                    # zero-based h in a uint16 array
            fn(np.full((n, m), h, dtype=np.uint16), X, C, *args, 5)
        with pytest.raises(OverflowError):                    # one-based 0 in an int64 array
            fn(np.zeros((n, m), dtype=np.int64), X, C, *args, 5)
        with pytest.raises(TypeError):
            fn(B0.astype(np.float32), X, C, *args, 5)
        with pytest.raises(ValueError):                       # k > n
            fn(B0, X, C, *args, n + 1)
        with pytest.raises(ValueError):                       # k < 1
            fn(B0, X, C, *args, 0)
        with pytest.raises(ValueError):                       # one column too many
            fn(np.zeros((n, m + 1), dtype=np.uint16), X, C, *args, 5)
        with pytest.raises(ValueError):                       # codebooks of another dimension
            fn(B0, X[:, :5], C, *args, 5)
        with pytest.raises(ValueError):                       # more codewords than an Int16 names
            fn(B0, X, [np.zeros((32768, d), dtype=np.float32)] * m, *args, 5)
        with pytest.raises(ValueError):                       # more than 32 codebooks
            fn(np.zeros((n, 33), dtype=np.uint16), X, C * 11, *args, 5)
    with pytest.raises(ValueError):
        Linscan.linscan_lsq_u16(B0, X, C, nrm[:-1], R, 5)
    with pytest.raises(ValueError):
        Linscan.linscan_lsq_u16(B0, X, C, None, R, 5)
    with pytest.raises(ValueError):
        Linscan.linscan_lsq_u16(B0, X, C, nrm, np.eye(d + 1, dtype=np.float32), 5)
    with pytest.raises(ValueError):
        Linscan.linscan_lsq_cbnorms_u16(B0, X, C, np.zeros(0, dtype=np.float32), R, 5)
    with pytest.raises(ValueError):
        Linscan.linscan_lsq_cbnorms_u16(B0, X, C, None, R, 5)


def test_norm_helpers_argument_checks(no_library):
    from rayuela_jl_amd import utils
    C = [np.zeros((300, 4), dtype=np.float32)] * 2
    for fn, extra in ((utils.aq_norms, ()), (utils.get_norms_codebook, ()), (utils.quantize_norms, (np.zeros(3, np.float32),))):
        with pytest.raises(ValueError):
            fn(np.full((5, 2), 301, dtype=np.int16), C, *extra)      # one-based codes end at h
        with pytest.raises(ValueError):
            fn(np.zeros((5, 2), dtype=np.int16), C, *extra)
        with pytest.raises(ValueError):
            fn(np.ones((5, 3), dtype=np.int16), C, *extra)
        with pytest.raises(TypeError):
            fn(np.ones((5, 2), dtype=np.float32), C, *extra)
        with pytest.raises(ValueError):
            fn(np.ones((5, 2), dtype=np.int16), [np.zeros((32768, 4), dtype=np.float32)] * 2, *extra)
    codes, Cs = utils._aq_args(np.full((5, 2), 300, dtype=np.int16), C)
    assert codes.dtype == np.int16 and (codes == 299).all()
    codes, _ = utils._aq_args(np.full((5, 2), 256, dtype=np.int16), [np.zeros((256, 4), dtype=np.float32)] * 2)
    assert codes.dtype == np.uint8 and (codes == 255).all()


# ---- the drivers take the scans over 16-bit codes at h > 256 -----------------------------------------------------------------------
@pytest.mark.parametrize("h", [256, 300])
@pytest.mark.parametrize("norms", ["host", "device"])
def test_search_legs_dispatch_on_h(monkeypatch, h, norms):
    from rayuela_jl_amd import Linscan, experiments, utils
    rng = np.random.default_rng(1)
    n, m, d, knn = 50, 2, 4, 7
    B = rng.integers(1, h + 1, (n, m)).astype(np.int16)
    B[0, 0] = h
    C = [rng.standard_normal((h, d)).astype(np.float32) for _ in range(m)]
    Xq = rng.standard_normal((3, d)).astype(np.float32)
    norms_C = rng.random(h).astype(np.float32)
    norms_B = rng.integers(1, h + 1, n)
    called = []

    def record(name):
        def fn(Bs, X, Cs, nrm, R, k):
            called.append((name, np.asarray(Bs), np.asarray(nrm), k))
            return "dists", "idx"
        return fn
    for name in ("linscan_lsq", "linscan_lsq_u16", "linscan_lsq_cbnorms", "linscan_lsq_cbnorms_u16"):
        monkeypatch.setattr(Linscan, name, record(name))
    monkeypatch.setattr(utils, "get_norms_codebook", lambda *a, **k: (norms_B, norms_C))
    monkeypatch.setattr(experiments, "_norms_codebook", lambda *a, **k: (norms_B, norms_C))
    wide = h > 256
    assert experiments._search_base(B, C, h, 0, B, Xq, knn, norms) == ("dists", "idx")
    name, Bs, nrm, k = called.pop()
    assert not called and k == knn
    if norms == "device":
        assert name == ("linscan_lsq_cbnorms_u16" if wide else "linscan_lsq_cbnorms") and np.array_equal(nrm, norms_C)
    else:
        assert name == ("linscan_lsq_u16" if wide else "linscan_lsq") and nrm.shape == (n,) and nrm.dtype == np.float32
    # one-based codes, in a dtype the _u16 functions read as one-based (an int16 array would be taken as zero-based)
    assert np.array_equal(Bs, B) and (Bs.dtype not in (np.int16, np.uint16) if wide else Bs.dtype == B.dtype)
    assert experiments._search_train(B, C, h, 0, Xq, knn, norms) == ("dists", "idx")
    name, Bs, nrm, k = called.pop()
    assert not called and name == ("linscan_lsq_u16" if wide else "linscan_lsq")
    assert np.array_equal(nrm, norms_C[norms_B - 1].astype(np.float32)) and np.array_equal(Bs, B)
    assert Bs.dtype not in (np.int16, np.uint16) if wide else Bs.dtype == B.dtype
