"""GPU: the additive-quantizer kind of the index handle over byte codes (rq_index_create_aq, rq_index_set_codes_aq,
rq_index_aq_info).  A base cut into LOGICAL shards of the one GPU must return what ONE rq_linscan_lsq /
rq_linscan_cq call over the whole base returns -- ids and distance bits, so there are no tolerances anywhere in this file.
tests/test_gpu_aq.py pins those calls to the compiled reference, tests/test_gpu_nonfinite_aq.py their non-finite rules."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import golden
from switch_table import switches

pytestmark = pytest.mark.gpu

RQ_EINVAL = -1
N, D, NQ, K = 20_001, 16, 6, 100
SHARDS = (1, 2, 3, 5, 8)


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _same(got, ref, id_shift=0):
    ids = np.ascontiguousarray(ref[1]).view(np.uint32).astype(np.uint64) + id_shift
    return np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32).astype(np.uint64), ids) and _eq_bits(got[0], ref[0])


def _one_call(kind, codes, cb, q, nrm, k, R=None, id_base=1):
    """ONE rq_linscan_lsq / rq_linscan_cq over the whole base (host pointers): (dists f32, ids u32)."""
    from rayuela_jl_amd import _lib
    codes, cb, q = [np.ascontiguousarray(a) for a in (codes, cb, q)]
    n, m = codes.shape
    nq, d = q.shape
    dists = np.empty((nq, k), dtype=np.float32)
    ids = np.empty((nq, k), dtype=np.uint32)
    L = _lib.lib()
    if kind == "lsq":
        nrm = np.ascontiguousarray(nrm, dtype=np.float32)
        Rp = None if R is None else np.ascontiguousarray(R, dtype=np.float32)
        _lib.check(L.rq_linscan_lsq(dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, q.ctypes.data, cb.ctypes.data,
                                    nrm.ctypes.data, None if Rp is None else Rp.ctypes.data, n, nq, m, 256, d, k, id_base))
    else:
        assert R is None
        _lib.check(L.rq_linscan_cq(dists.ctypes.data, ids.ctypes.data, codes.ctypes.data, q.ctypes.data, cb.ctypes.data,
                                   n, nq, m, 256, d, k, id_base))
    return dists, ids


def _true_norms(codes, cb, m, d):
    return ((cb.reshape(m, 256, d)[np.arange(m)[None, :], codes]).sum(1) ** 2).sum(1).astype(np.float32)      # |x_hat|^2


@functools.lru_cache(maxsize=None)
def _base(m, n=N):
    """After test_prepared_lsq_index_equals_linscan_lsq: half of the rows are copies of 300 rows (ties across shard boundaries, a
    live pre-filter), the norms are the true |x_hat|^2.  The references are computed once and shared (never written to)."""
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(n + m)
    Cl = [rng.standard_normal((256, D)).astype(np.float32) for _ in range(m)]
    cb = np.concatenate(Cl)
    codes = synth.random_codes(n, m, seed=n)
    codes[: n // 2] = codes[rng.integers(0, 300, n // 2)]
    nrm = _true_norms(codes, cb, m, D)
    q = rng.standard_normal((NQ, D)).astype(np.float32)
    k = min(K, n)
    eye = np.eye(D, dtype=np.float32)
    ref = {"lsq": rq.linscan_lsq(codes, q, Cl, nrm, eye, k), "cq": rq.linscan_cq(codes, q, Cl, k)}
    assert _same(_one_call("lsq", codes, cb, q, nrm, k), ref["lsq"])      # (the identity rotation is no rotation)
    return dict(C=Cl, cb=cb, codes=codes, nrm=nrm, q=q, ref=ref, k=k)


def _norm_kw(kind, b):
    return dict(dbnorms=b["nrm"]) if kind == "lsq" else {}


# ---- 1. shards against one call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("kind", ["lsq", "cq"])
@pytest.mark.parametrize("m", [8, 16, 5, 4])
def test_logical_shards_equal_one_call(rq, m, kind, ordered):
    """m = 5 is a padded width, m = 4 has no LSQ pre-filter.  Defaults leave shards of this size in arrival order; under
    ORDER_MIN_ROWS = 1 every non-empty shard must be in bank-aware order and, for LSQ at m = 8 and 16, hold its prepared norm
    buffer -- the case in which a norm slice without its row0 offset, or norms not sent through the shard's perm, answers wrong."""
    from rayuela_jl_amd import _lib
    b = _base(m)
    width = _lib.lib().rq_scan_row_width(m)
    assert width == {8: 8, 16: 16, 5: 8, 4: 4}[m]
    with switches(**(dict(ORDER_MIN_ROWS=1) if ordered else {})):
        for P in SHARDS:
            with rq.AqIndex(b["C"], kind=kind, devices=[0] * P) as ix:
                ix.set_codes(b["codes"], **_norm_kw(kind, b))
                info = ix.info()
                got = ix.search(b["q"], b["k"])
            assert info["kind"] == kind and not info["wide"] and info["h"] == 256
            assert info["shards"] == P and info["n"] == N and sum(info["rows_per_shard"]) == N
            assert info["ordered"] == [ordered] * P, (P, info)
            # (the pre-filter goes by the padded row width, as in rq_lsq_prepare: m = 5 is scanned as 8-byte rows)
            assert info["prepared"] == [kind == "lsq" and width in (8, 16)] * P, (P, info)
            assert _same(got, b["ref"][kind]), (m, kind, ordered, P)


def test_default_device_form(rq):
    b = _base(8)
    with rq.AqIndex(b["C"]) as ix:
        got = ix.set_codes(b["codes"], dbnorms=b["nrm"]).search(b["q"], K)
        assert ix.info()["shards"] == 1 and ix.info()["kind"] == "lsq"
    assert _same(got, b["ref"]["lsq"])


# ---- 2. the compiled reference's fixtures through 3 shards ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["aq_mini_m8", "aq_mini_m4"])
def test_reference_golden_through_three_shards(rq, name):
    g = golden(name)
    m = g["codes"].shape[1]
    Cl = [g["codebooks"][i * 256:(i + 1) * 256] for i in range(m)]
    with rq.AqIndex(Cl, kind="lsq", devices=[0, 0, 0]) as lsq, rq.AqIndex(Cl, kind="cq", devices=[0, 0, 0]) as cq:
        lsq.set_codes(g["codes"], dbnorms=g["dbnorms"])
        cq.set_codes(g["codes"])
        for k in g["Ks"]:
            k = int(k)
            d, i = lsq.search(g["queries"], k)
            assert np.array_equal(i.view(np.int32), g["lsq_i%d" % k]) and _eq_bits(d, g["lsq_d%d" % k]), (name, k, "lsq")
            d, i = cq.search(g["queries"], k)
            assert np.array_equal(i.view(np.int32), g["cq_i%d" % k]) and _eq_bits(d, g["cq_d%d" % k]), (name, k, "cq")


# ---- 3. the cbnorms form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hn", [256, 7])
def test_cbnorms_equal_their_dbnorms(rq, hn):
    b = _base(8)
    rng = np.random.default_rng(hn)
    c = (rng.random(hn) * float(b["nrm"].max())).astype(np.float32)
    one_based = b["codes"].astype(np.int16) + 1
    dbn = c[rq.quantize_norms(one_based, b["C"], c)[0].astype(np.int64) - 1]
    with rq.LsqIndex.from_cbnorms(b["codes"], b["C"], c) as whole:
        ref = whole.search(b["q"], None, K)
    with switches(ORDER_MIN_ROWS=1):        # norms computed from the shard's rows, then sent through the shard's perm
        with rq.AqIndex(b["C"], devices=[0, 0, 0]) as ix:
            a = ix.set_codes(b["codes"], cbnorms=c).search(b["q"], K)
            assert ix.info()["ordered"] == [True] * 3
            e = ix.set_codes(b["codes"], dbnorms=dbn).search(b["q"], K)
    with rq.AqIndex(b["C"], devices=[0] * 5) as ix:
        f = ix.set_codes(b["codes"], cbnorms=c).search(b["q"], K)
    assert _same(a, ref) and _same(e, ref) and _same(f, ref)


# ---- 4. short and empty shards ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lsq", "cq"])
def test_shards_shorter_than_k_and_empty_shards(rq, kind):
    """n = 10 over 8 shards (1-2 rows each) with k = 7 > every shard, and n = 5 over 8 shards (3 empty)."""
    b = _base(8)
    for n, k in [(10, 7), (5, 5)]:
        codes, nrm = b["codes"][N - n:], b["nrm"][N - n:]
        with rq.AqIndex(b["C"], kind=kind, devices=[0] * 8) as ix:
            ix.set_codes(codes, **(dict(dbnorms=nrm) if kind == "lsq" else {}))
            assert sorted(ix.info()["rows_per_shard"], reverse=True) == ix.info()["rows_per_shard"] and sum(ix.info()["rows_per_shard"]) == n
            got = ix.search(b["q"], k)
        assert _same(got, _one_call(kind, codes, b["cb"], b["q"], nrm, k)), (kind, n, k)


# ---- 5. bulk k -------------------------------------------------------------------------------------------------------------------
def test_bulk_k(rq):
    """k = 65_537 > RQ_MAX_K: the bulk scan per shard and the bulk merge of the lists."""
    n, m, k = 70_000, 4, 65_537
    b = _base(m, n)
    q = b["q"][:2]
    for kind in ("lsq", "cq"):
        with rq.AqIndex(b["C"], kind=kind, devices=[0] * 3) as ix:
            got = ix.set_codes(b["codes"], **_norm_kw(kind, b)).search(q, k)
        assert _same(got, _one_call(kind, b["codes"], b["cb"], q, b["nrm"], k)), kind


# ---- 6. transport and chunks -----------------------------------------------------------------------------------------------------
def test_rccl_selftest_exchange(rq):
    b = _base(8)
    with switches(EXCHANGE_SELFTEST=1):
        with rq.AqIndex(b["C"], devices=[0, 0, 0, 0]) as ix:
            ix.set_codes(b["codes"], dbnorms=b["nrm"])
            if ix.info()["exchange"] != "rccl":
                pytest.skip("librccl could not be loaded / initialised on this box")
            got = ix.search(b["q"], K)
    assert _same(got, b["ref"]["lsq"])


@pytest.mark.parametrize("chunks", [2, 3])
def test_query_chunks(rq, chunks):
    b = _base(8)
    with switches(IDX_QCHUNKS=chunks):
        for kind in ("lsq", "cq"):
            with rq.AqIndex(b["C"], kind=kind, devices=[0, 0, 0]) as ix:
                ix.set_codes(b["codes"], **_norm_kw(kind, b))
                for _ in range(2):
                    assert _same(ix.search(b["q"], K), b["ref"][kind]), (kind, chunks)
        # a shard shorter than k (KEY_MAX padding) inside a chunked search
        with rq.AqIndex(b["C"], devices=[0] * 7) as ix:
            got = ix.set_codes(b["codes"][:40], dbnorms=b["nrm"][:40]).search(b["q"], 20)
        assert _same(got, _one_call("lsq", b["codes"][:40], b["cb"], b["q"], b["nrm"][:40], 20))


# ---- 7. ids, rotation, replacement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id_base", [0, 1])
def test_id_offset_past_2_to_31(rq, id_base):
    b = _base(8)
    off = 2 ** 31 + 5
    for kind in ("lsq", "cq"):
        ref = _one_call(kind, b["codes"], b["cb"], b["q"], b["nrm"], K, id_base=id_base)
        with rq.AqIndex(b["C"], kind=kind, devices=[0, 0, 0]) as ix:
            got = ix.set_codes(b["codes"], id_offset=off, **_norm_kw(kind, b)).search(b["q"], K, id_base=id_base)
            with pytest.raises(rq.RayuelaHipError):
                ix.set_codes(b["codes"], id_offset=2 ** 32 - N, **_norm_kw(kind, b))
            again = ix.search(b["q"], K, id_base=id_base)      # the refused base changed nothing
        assert got[1].min() > 2 ** 31 and _same(got, ref, id_shift=off) and _same(again, ref, id_shift=off), kind


@pytest.mark.parametrize("nshards", [1, 3])
def test_rotation_given_and_absent(rq, nshards):
    import rayuela_jl_amd.synth as synth
    b = _base(8)
    R = synth.rotation(D, seed=5)
    with rq.AqIndex(b["C"], devices=[0] * nshards) as ix:
        ix.set_codes(b["codes"], dbnorms=b["nrm"])
        for rot in (None, R, None):
            ref = _one_call("lsq", b["codes"], b["cb"], b["q"], b["nrm"], K, R=rot)
            assert _same(ix.search(b["q"], K, R=rot), ref), (nshards, rot is not None)
    assert _same(rq.linscan_lsq(b["codes"], b["q"], b["C"], b["nrm"], R, K), _one_call("lsq", b["codes"], b["cb"], b["q"], b["nrm"], K, R=R))


def test_replacing_the_base_twice(rq):
    b = _base(8)
    with switches(ORDER_MIN_ROWS=1):
        with rq.AqIndex(b["C"], devices=[0, 0, 0]) as ix:
            for n in (N, 777, 12_345):          # ordered and prepared shards, then 259-row shards in arrival order, then ordered again
                codes, nrm = b["codes"][:n], (b["nrm"][:n] + np.float32(n)).astype(np.float32)
                got = ix.set_codes(codes, dbnorms=nrm).search(b["q"], K)
                info = ix.info()
                assert info["n"] == n and sum(info["rows_per_shard"]) == n and info["ordered"] == [n >= 3 * 1024] * 3, info
                assert _same(got, _one_call("lsq", codes, b["cb"], b["q"], nrm, K)), n


# ---- 8. non-finite ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", [False, True])
def test_nonfinite_norms_and_queries(rq, ordered):
    """A NaN and a +Inf norm in rows of the last shard and a NaN query component: the one-shot call's rules, shard by shard."""
    b = _base(8)
    nrm = b["nrm"].copy()
    nrm[N - 5] = np.nan
    nrm[N - 900] = np.inf
    q = b["q"].copy()
    q[2, 3] = np.nan
    ref = _one_call("lsq", b["codes"], b["cb"], q, nrm, K)
    with switches(**(dict(ORDER_MIN_ROWS=1) if ordered else {})):
        with rq.AqIndex(b["C"], devices=[0, 0, 0]) as ix:
            got = ix.set_codes(b["codes"], dbnorms=nrm).search(q, K)
    assert _same(got, ref)
    with rq.AqIndex(b["C"], kind="cq", devices=[0, 0, 0]) as ix:
        got = ix.set_codes(b["codes"]).search(q, K)
    assert _same(got, _one_call("cq", b["codes"], b["cb"], q, None, K))


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def _raw_set(ix, codes, dbnorms, cbnorms, hn, id_offset=0):
    from rayuela_jl_amd import _lib
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (dbnorms, cbnorms)]
    rc = _lib.lib().rq_index_set_codes_aq(ix._h, codes.ctypes.data, *[None if a is None else a.ctypes.data for a in keep], hn,
                                          codes.shape[0], id_offset)
    return rc, _lib.lib().rq_last_error().decode()


def test_refused_norm_arguments_leave_the_base_answering(rq):
    b = _base(8)
    small, snrm = b["codes"][:5000], b["nrm"][:5000]
    cbn = np.linspace(0, 50, 256).astype(np.float32)
    with rq.AqIndex(b["C"], devices=[0, 0, 0]) as lsq, rq.AqIndex(b["C"], kind="cq", devices=[0, 0, 0]) as cq:
        with pytest.raises(rq.RayuelaHipError):
            lsq.search(b["q"], 10)                                  # no codes yet
        lsq.set_codes(small, dbnorms=snrm)
        cq.set_codes(small)
        ref_l = _one_call("lsq", small, b["cb"], b["q"], snrm, K)
        ref_c = _one_call("cq", small, b["cb"], b["q"], None, K)
        for ix, ref, args, word in [(lsq, ref_l, (None, None, 0), "exactly one"),
                                    (lsq, ref_l, (b["nrm"], cbn, 256), "exactly one"),
                                    (lsq, ref_l, (None, cbn, 0), "hn=0"),
                                    (lsq, ref_l, (None, np.zeros(257, np.float32), 257), "hn=257"),
                                    (cq, ref_c, (b["nrm"], None, 0), "no norms"),
                                    (cq, ref_c, (None, cbn, 256), "no norms")]:
            rc, msg = _raw_set(ix, b["codes"], *args)
            assert rc == RQ_EINVAL and word in msg, (args[2], msg)
            info = ix.info()
            assert info["n"] == 5000 and sum(info["rows_per_shard"]) == 5000
            assert _same(ix.search(b["q"], K), ref), word


def test_wrong_kind_calls_are_refused(rq):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    b = _base(8)
    rng = np.random.default_rng(1)
    cpq = [rng.standard_normal((256, D // 8)).astype(np.float32) for _ in range(8)]
    wide_C = [c[:, :] for c in b["C"]]
    small, snrm = b["codes"][:3000], b["nrm"][:3000]
    with rq.Index(cpq, D, devices=[0, 0]) as pq, rq.AqIndex(b["C"], devices=[0, 0]) as aq, \
            rq.AqIndexU16(wide_C, devices=[0, 0]) as aq16:
        pq.set_codes(small)
        aq.set_codes(small, dbnorms=snrm)
        ref_pq = pq.search(b["q"], K)
        ref_aq = aq.search(b["q"], K)
        # the PQ setters on an AQ index
        assert L.rq_index_set_codes(aq._h, small.ctypes.data, 3000, 0) == RQ_EINVAL
        assert "rq_index_set_codes_aq" in L.rq_last_error().decode()
        assert L.rq_index_set_codes_synth(aq._h, 3000, 7, 0) == RQ_EINVAL
        assert "rq_index_set_codes_aq" in L.rq_last_error().decode()
        s16 = small.astype(np.int16)
        assert L.rq_index_set_codes_wide(aq16._h, s16.ctypes.data, 3000, 0, 0) == RQ_EINVAL
        assert "rq_index_set_codes_aq_wide" in L.rq_last_error().decode()
        # the AQ setters on a PQ index, and on an index of the other width
        rc, msg = _raw_set(pq, small, snrm, None, 0)
        assert rc == RQ_EINVAL and "rq_index_set_codes" in msg and "PQ index" in msg
        rc, msg = _raw_set(aq16, small, snrm, None, 0)
        assert rc == RQ_EINVAL and "rq_index_set_codes_aq_wide" in msg
        assert L.rq_index_set_codes_aq_wide(aq._h, s16.ctypes.data, snrm.ctypes.data, None, 0, 3000, 0, 0) == RQ_EINVAL
        assert "rq_index_set_codes_aq" in L.rq_last_error().decode() and "byte" in L.rq_last_error().decode()
        assert _same(pq.search(b["q"], K), ref_pq) and _same(aq.search(b["q"], K), ref_aq)
        out = (C.c_int64 * 8)()
        assert L.rq_index_aq_info(pq._h, C.cast(out, C.c_void_p), 8) == 0 and list(out)[:4] == [0, 0, 256, 2]     # lut_mode 0: PQ
        assert aq16.info()["wide"] and aq16.info()["kind"] == "lsq"


def test_create_limits(rq):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    cb = np.zeros(65 * 256 * 2, dtype=np.float32)
    dev = C.cast((C.c_int * 1)(0), C.c_void_p)
    for m, d, mode in [(0, 2, 1), (65, 2, 1), (4, 0, 1), (4, 2, 0), (4, 2, 3)]:
        assert not L.rq_index_create_aq(m, d, cb.ctypes.data, mode, None, 0), (m, d, mode)
        assert L.rq_last_error().decode() != ""
        assert not L.rq_index_create_aq(m, d, cb.ctypes.data, mode, dev, 1), (m, d, mode)
    assert not L.rq_index_create_aq(4, 2, None, 1, None, 0) and "NULL" in L.rq_last_error().decode()
    assert not L.rq_index_create_aq(4, 2, cb.ctypes.data, 1, dev, 0)
    for mode in (1, 2):
        hnd = L.rq_index_create_aq(64, 2, cb.ctypes.data, mode, None, 0)
        assert hnd
        out = (C.c_int64 * 6)()
        assert L.rq_index_aq_info(hnd, C.cast(out, C.c_void_p), 6) == 0 and list(out)[:4] == [mode, 0, 256, 1]
        L.rq_index_destroy(hnd)


# ---- 10. several GPUs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lsq", "cq"])
def test_two_devices(rq, kind):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    b = _base(8)
    for devices in ([0, 1], [0, 1, 1, 0, 1]):
        with rq.AqIndex(b["C"], kind=kind, devices=devices) as ix:
            got = ix.set_codes(b["codes"], **_norm_kw(kind, b)).search(b["q"], K)
            assert ix.info()["devices"] == 2
        assert _same(got, b["ref"][kind]), devices
