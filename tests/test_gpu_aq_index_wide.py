"""GPU: the additive-quantizer kind of the index handle over 16-bit codes (rq_index_create_aq_wide, rq_index_set_codes_aq_wide;
DESIGN.md section 4.28).  Mirrors tests/test_gpu_aq_index.py: logical shards of the one GPU must return what ONE
rq_linscan_lsq_wide / rq_linscan_cq_wide / rq_linscan_lsq_cbnorms_wide call over the whole base returns (tests/test_gpu_aq_wide.py
pins those to the oracle), ids and distance bits, plus tests/aq_wide_oracle.py directly once.  No tolerances."""
import functools

import numpy as np
import pytest

import aq_wide_oracle as awo
from switch_table import switches

pytestmark = pytest.mark.gpu

RQ_EINVAL = -1
N, NQ, K = 20_001, 5, 100
SHAPES = [(8, 1024, 16), (4, 300, 12)]
SHARDS = (1, 2, 3, 5, 8)


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _same(got, ref, id_shift=0):
    ids = np.ascontiguousarray(ref[1]).view(np.uint32).astype(np.uint64) + id_shift
    return np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32).astype(np.uint64), ids) and _eq_bits(got[0], ref[0])


def _one_call(kind, codes, C3, q, nrm, k, R=None, id_base=1, cbn=None):
    """ONE rq_linscan_{lsq,cq,lsq_cbnorms}_wide over the whole base of zero-based codes (host pointers): (dists f32, ids u32)."""
    from rayuela_jl_amd import _lib
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    cb = np.ascontiguousarray(C3, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    n, m = codes.shape
    nq, d = q.shape
    h = cb.shape[1]
    dists = np.empty((nq, k), dtype=np.float32)
    ids = np.empty((nq, k), dtype=np.uint32)
    L = _lib.lib()
    Rp = None if R is None else np.ascontiguousarray(R, dtype=np.float32)
    Rptr = None if Rp is None else Rp.ctypes.data
    a = (dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, q.ctypes.data, cb.ctypes.data)
    if kind == "cq":
        _lib.check(L.rq_linscan_cq_wide(*a, n, nq, m, h, d, k, 0, id_base))
    elif cbn is None:
        nrm = np.ascontiguousarray(nrm, dtype=np.float32)
        _lib.check(L.rq_linscan_lsq_wide(*a, nrm.ctypes.data, Rptr, n, nq, m, h, d, k, 0, id_base))
    else:
        cbn = np.ascontiguousarray(cbn, dtype=np.float32)
        _lib.check(L.rq_linscan_lsq_cbnorms_wide(*a, cbn.ctypes.data, cbn.shape[0], Rptr, n, nq, m, h, d, k, 0, id_base))
    return dists, ids


@functools.lru_cache(maxsize=None)
def _base(m, h, d, n=N):
    """awo.case with half of the rows (and their norms) copies of 300 rows: ties across shard boundaries.  The references are
    computed once with the package's one-shot calls and shared (never written to)."""
    import rayuela_jl_amd as rq
    codes, C3, q, nrm = awo.case(n, m, h, d, NQ, seed=n + m + h)
    rng = np.random.default_rng(h)
    src = rng.integers(0, 300, n // 2)
    codes[: n // 2] = codes[src]
    nrm[: n // 2] = nrm[src]
    cbn = (rng.standard_normal(777) * 40).astype(np.float32)
    Cl = [C3[i] for i in range(m)]
    k = min(K, n)
    ref = {"lsq": rq.linscan_lsq_u16(codes, q, Cl, nrm, None, k), "cq": rq.linscan_cq_u16(codes, q, Cl, k),
           "cbnorms": rq.linscan_lsq_cbnorms_u16(codes, q, Cl, cbn, None, k)}
    return dict(C=Cl, C3=C3, codes=codes, nrm=nrm, cbn=cbn, q=q, ref=ref, k=k)


def _kind(which):
    return "cq" if which == "cq" else "lsq"


def _norm_kw(which, b):
    return {"lsq": dict(dbnorms=b["nrm"]), "cbnorms": dict(cbnorms=b["cbn"]), "cq": {}}[which]


@pytest.mark.parametrize("which", ["lsq", "cq", "cbnorms"])
@pytest.mark.parametrize("shape", SHAPES)
def test_logical_shards_equal_one_call(rq, shape, which):
    b = _base(*shape)
    for P in SHARDS:
        with rq.AqIndexU16(b["C"], kind=_kind(which), devices=[0] * P) as ix:
            ix.set_codes(b["codes"], **_norm_kw(which, b))
            info = ix.info()
            got = ix.search(b["q"], K)
        assert info["kind"] == _kind(which) and info["wide"] and info["h"] == shape[1]
        assert info["shards"] == P and info["n"] == N and sum(info["rows_per_shard"]) == N
        assert info["ordered"] == [False] * P and info["prepared"] == [False] * P      # wide rows stay in arrival order
        assert _same(got, b["ref"][which]), (shape, which, P)


@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_oracle(rq, shape):
    b = _base(*shape)
    with rq.AqIndexU16(b["C"], devices=[0, 0, 0]) as lsq, rq.AqIndexU16(b["C"], kind="cq", devices=[0, 0, 0]) as cq:
        dl, il = lsq.set_codes(b["codes"], dbnorms=b["nrm"]).search(b["q"], K)
        dc, ic = cq.set_codes(b["codes"]).search(b["q"], K)
    ref = awo.scan(b["codes"], b["C3"], b["q"], K, dbnorms=b["nrm"], id_base=1)
    assert awo.same(dl, il, ref)
    ref = awo.scan(b["codes"], b["C3"], b["q"], K, id_base=1)
    assert awo.same(dc, ic, ref)


def test_default_device_form_and_rotation(rq):
    import rayuela_jl_amd.synth as synth
    m, h, d = SHAPES[0]
    b = _base(m, h, d)
    R = synth.rotation(d, seed=3)
    ref = rq.linscan_lsq_u16(b["codes"], b["q"], b["C"], b["nrm"], R, K)
    with rq.AqIndexU16(b["C"]) as one, rq.AqIndexU16(b["C"], devices=[0] * 3) as many:
        assert one.info()["shards"] == 1
        one.set_codes(b["codes"], dbnorms=b["nrm"])
        many.set_codes(b["codes"], dbnorms=b["nrm"])
        assert _same(one.search(b["q"], K, R=R), ref) and _same(many.search(b["q"], K, R=R), ref)
        assert _same(one.search(b["q"], K), b["ref"]["lsq"]) and _same(many.search(b["q"], K), b["ref"]["lsq"])


@pytest.mark.parametrize("which", ["lsq", "cq", "cbnorms"])
def test_shards_shorter_than_k_and_empty_shards(rq, which):
    """n = 10 over 8 shards (1-2 rows each) with k = 7 > every shard, and n = 5 over 8 shards (3 empty)."""
    b = _base(*SHAPES[0])
    for n, k in [(10, 7), (5, 5)]:
        codes, nrm = b["codes"][N - n:], b["nrm"][N - n:]
        kw = {"lsq": dict(dbnorms=nrm), "cbnorms": dict(cbnorms=b["cbn"]), "cq": {}}[which]
        with rq.AqIndexU16(b["C"], kind=_kind(which), devices=[0] * 8) as ix:
            got = ix.set_codes(codes, **kw).search(b["q"], k)
        ref = _one_call(_kind(which), codes, b["C3"], b["q"], nrm, k, cbn=b["cbn"] if which == "cbnorms" else None)
        assert _same(got, ref), (which, n, k)


def test_bulk_k(rq):
    """k = 65_537 > RQ_MAX_K: the lists of the shards are merged by the bulk select."""
    n, k = 70_000, 65_537
    b = _base(2, 300, 4, n)
    q = b["q"][:2]
    for which in ("lsq", "cq"):
        with rq.AqIndexU16(b["C"], kind=which, devices=[0] * 3) as ix:
            got = ix.set_codes(b["codes"], **_norm_kw(which, b)).search(q, k)
        assert _same(got, _one_call(which, b["codes"], b["C3"], q, b["nrm"], k)), which


def test_rccl_selftest_exchange(rq):
    b = _base(*SHAPES[0])
    with switches(EXCHANGE_SELFTEST=1):
        with rq.AqIndexU16(b["C"], devices=[0, 0, 0, 0]) as ix:
            ix.set_codes(b["codes"], dbnorms=b["nrm"])
            if ix.info()["exchange"] != "rccl":
                pytest.skip("librccl could not be loaded / initialised on this box")
            got = ix.search(b["q"], K)
    assert _same(got, b["ref"]["lsq"])


@pytest.mark.parametrize("chunks", [2, 3])
def test_query_chunks(rq, chunks):
    b = _base(*SHAPES[1])
    with switches(IDX_QCHUNKS=chunks):
        for which in ("lsq", "cq"):
            with rq.AqIndexU16(b["C"], kind=which, devices=[0, 0, 0]) as ix:
                ix.set_codes(b["codes"], **_norm_kw(which, b))
                for _ in range(2):
                    assert _same(ix.search(b["q"], K), b["ref"][which]), (which, chunks)
        # a shard shorter than k (KEY_MAX padding) inside a chunked search
        with rq.AqIndexU16(b["C"], devices=[0] * 7) as ix:
            got = ix.set_codes(b["codes"][:40], dbnorms=b["nrm"][:40]).search(b["q"], 20)
        assert _same(got, _one_call("lsq", b["codes"][:40], b["C3"], b["q"], b["nrm"][:40], 20))


@pytest.mark.parametrize("id_base", [0, 1])
def test_id_offset_past_2_to_31_and_code_bases(rq, id_base):
    b = _base(*SHAPES[1])
    off = 2 ** 31 + 5
    ref = _one_call("lsq", b["codes"], b["C3"], b["q"], b["nrm"], K, id_base=id_base)
    with rq.AqIndexU16(b["C"], devices=[0, 0, 0]) as ix:
        zero = ix.set_codes(b["codes"], dbnorms=b["nrm"], id_offset=off).search(b["q"], K, id_base=id_base)     # int16: zero-based
        one = ix.set_codes(b["codes"].astype(np.int32) + 1, cbnorms=b["cbn"], id_offset=off).search(b["q"], K, id_base=id_base)
        with pytest.raises(rq.RayuelaHipError):
            ix.set_codes(b["codes"], dbnorms=b["nrm"], id_offset=2 ** 32 - N)
        again = ix.search(b["q"], K, id_base=id_base)
    assert zero[1].min() > 2 ** 31 and _same(zero, ref, id_shift=off)
    refc = _one_call("lsq", b["codes"], b["C3"], b["q"], None, K, id_base=id_base, cbn=b["cbn"])
    assert _same(one, refc, id_shift=off) and _same(again, refc, id_shift=off)


def test_a_sliced_shard(rq):
    """The scan's row slices (rq_test_scan_wide_slice_rows) under the index: three shards of 6667 rows in slices of 1000, the norms
    of a slice read at the slice's offset inside the shard's."""
    from rayuela_jl_amd import _lib
    b = _base(*SHAPES[0])
    prev = _lib.lib().rq_test_scan_wide_slice_rows(1000)
    try:
        with rq.AqIndexU16(b["C"], devices=[0, 0, 0]) as ix:
            got = ix.set_codes(b["codes"], dbnorms=b["nrm"]).search(b["q"], K)
        with rq.AqIndexU16(b["C"], kind="cq") as ix:
            one = ix.set_codes(b["codes"]).search(b["q"], K)
    finally:
        _lib.lib().rq_test_scan_wide_slice_rows(prev)
    assert _same(got, b["ref"]["lsq"]) and _same(one, b["ref"]["cq"])


def _raw_set(ix, codes, code_base, dbnorms=None, cbnorms=None, id_offset=0):
    from rayuela_jl_amd import _lib
    codes = np.ascontiguousarray(codes, dtype=np.int16)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (dbnorms, cbnorms)]
    hn = 0 if keep[1] is None else keep[1].shape[0]
    rc = _lib.lib().rq_index_set_codes_aq_wide(ix._h, codes.ctypes.data, *[None if a is None else a.ctypes.data for a in keep], hn,
                                               codes.shape[0], code_base, id_offset)
    return rc, _lib.lib().rq_last_error().decode()


@pytest.mark.parametrize("code_base", [0, 1])
def test_bad_code_is_refused_and_the_loaded_base_keeps_its_norms(rq, code_base):
    m, h, d = SHAPES[0]
    b = _base(m, h, d)
    small, snrm = b["codes"][:5000], (b["nrm"][:5000] * np.float32(2)).astype(np.float32)
    ref = _one_call("lsq", small, b["C3"], b["q"], snrm, K)
    with rq.AqIndexU16(b["C"], devices=[0, 0, 0]) as ix:
        ix.set_codes(small, dbnorms=snrm)
        for row, value in [(17, h), (12_345, -1), (N - 1, 32767)]:      # zero-based values outside [0, h); first, second, last shard
            bad = b["codes"].copy() + np.int16(code_base)
            bad[row, row % m] = min(value + code_base, 32767)
            if row < N - 1:
                bad[N - 1, 0] = -7                                      # a later bad row: the FIRST one is named
            for kw in (dict(dbnorms=b["nrm"]), dict(cbnorms=b["cbn"])):
                rc, msg = _raw_set(ix, bad, code_base, **kw)
                assert rc == RQ_EINVAL and ("row %d " % row) in msg, (row, msg)
                info = ix.info()
                assert info["n"] == 5000 and sum(info["rows_per_shard"]) == 5000
                assert _same(ix.search(b["q"], K), ref), row
        rc, msg = _raw_set(ix, b["codes"] + code_base, 2, dbnorms=b["nrm"])
        assert rc == RQ_EINVAL and "code_base" in msg
        rc, _ = _raw_set(ix, b["codes"] + code_base, code_base, dbnorms=b["nrm"])
        assert rc == 0 and ix.info()["n"] == N
        assert _same(ix.search(b["q"], K), b["ref"]["lsq"])


def test_refused_norm_arguments(rq):
    m, h, d = SHAPES[1]
    b = _base(m, h, d)
    with rq.AqIndexU16(b["C"], devices=[0, 0]) as lsq, rq.AqIndexU16(b["C"], kind="cq", devices=[0, 0]) as cq:
        with pytest.raises(rq.RayuelaHipError):
            cq.search(b["q"], 10)                                   # no codes yet
        lsq.set_codes(b["codes"], dbnorms=b["nrm"])
        cq.set_codes(b["codes"])
        from rayuela_jl_amd import _lib
        L = _lib.lib()
        ci = np.ascontiguousarray(b["codes"])
        big = np.zeros(32768, dtype=np.float32)
        for ix, pn, pc, hn, word in [(lsq, None, None, 0, "exactly one"), (lsq, b["nrm"], b["cbn"], 777, "exactly one"),
                                     (lsq, None, b["cbn"], 0, "hn=0"), (lsq, None, big, 32768, "hn=32768"),
                                     (cq, b["nrm"], None, 0, "no norms"), (cq, None, b["cbn"], 777, "no norms")]:
            rc = L.rq_index_set_codes_aq_wide(ix._h, ci.ctypes.data, None if pn is None else pn.ctypes.data,
                                              None if pc is None else pc.ctypes.data, hn, N, 0, 0)
            assert rc == RQ_EINVAL and word in L.rq_last_error().decode(), (word, L.rq_last_error().decode())
        assert _same(lsq.search(b["q"], K), b["ref"]["lsq"]) and _same(cq.search(b["q"], K), b["ref"]["cq"])


def test_create_limits(rq):
    import ctypes as C
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    cb = np.zeros(33 * 4 * 2, dtype=np.float32)
    dev = C.cast((C.c_int * 1)(0), C.c_void_p)
    for m, h, d, mode in [(0, 4, 2, 1), (33, 4, 2, 1), (4, 0, 2, 1), (4, 32768, 2, 1), (4, 4, 0, 2), (4, 4, 2, 0), (4, 4, 2, 3)]:
        assert not L.rq_index_create_aq_wide(m, h, d, cb.ctypes.data, mode, None, 0), (m, h, d, mode)
        assert L.rq_last_error().decode() != ""
        assert not L.rq_index_create_aq_wide(m, h, d, cb.ctypes.data, mode, dev, 1), (m, h, d, mode)
    assert not L.rq_index_create_aq_wide(4, 4, 2, None, 1, None, 0)
    hnd = L.rq_index_create_aq_wide(32, 4, 2, cb.ctypes.data, 2, None, 0)       # d = 2 < m: no d % m rule for full-dimensional codebooks
    assert hnd
    out = (C.c_int64 * 6)()
    assert L.rq_index_aq_info(hnd, C.cast(out, C.c_void_p), 6) == 0 and list(out)[:4] == [2, 1, 4, 1]
    L.rq_index_destroy(hnd)


def test_h256_equals_the_byte_index(rq):
    n, m, d, nq, k = 20_001, 8, 16, 5, 100
    rng = np.random.default_rng(256)
    Cl = [rng.standard_normal((256, d)).astype(np.float32) for _ in range(m)]
    q = rng.standard_normal((nq, d)).astype(np.float32)
    codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    nrm = (rng.random(n) * 50).astype(np.float32)
    cbn = (rng.random(200) * 30).astype(np.float32)
    for devices in (None, [0, 0, 0]):
        for kind, kw in [("lsq", dict(dbnorms=nrm)), ("lsq", dict(cbnorms=cbn)), ("cq", {})]:
            with rq.AqIndex(Cl, kind=kind, devices=devices) as b8, rq.AqIndexU16(Cl, kind=kind, devices=devices) as b16:
                r8 = b8.set_codes(codes, **kw).search(q, k)
                r16 = b16.set_codes(codes.astype(np.int16), **kw).search(q, k)
            assert _same(r16, r8), (devices, kind, sorted(kw))


def test_two_devices(rq):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    b = _base(*SHAPES[0])
    for which in ("lsq", "cq", "cbnorms"):
        with rq.AqIndexU16(b["C"], kind=_kind(which), devices=[0, 1, 1]) as ix:
            got = ix.set_codes(b["codes"], **_norm_kw(which, b)).search(b["q"], K)
        assert _same(got, b["ref"][which]), which
