"""GPU: rq_dataset_rerank against its numpy restatement tests/rerank_oracle.py, bit for bit -- u32 views of
the distances, and ids; there are no tolerances.  n = 1000 rows, float32 and uint8 bases: every load width of the row loaders, rows
that are only 4- / 2- / 1-byte aligned, and queries of two and three staged pieces (the kernels stage 1024 floats of the query at a
time: d = 960 is one piece, 1030 and 2052 cross into a second and a third); the slab and sort edges of kc; both select paths
on the same inputs; ragged batches; duplicates, near-ties and non-finite values; scratch and threads; every refusal; bases whose
offsets pass 2^31 elements and 2^32 bytes.  Distance matrices are computed once per (d, kind) and shared read-only."""
import functools
import threading

import numpy as np
import pytest

import knn_oracle as ko
import large_offsets as lo
import nonfinite_ref as nf
import rerank_oracle as ro

gpu = pytest.mark.gpu
N, NQ = 1000, 33
# 12 and 24: the 4- and 8-byte loads of a byte row; 1030 (2-wide loads) and 2052 (4-wide): a second and a third piece of the query
DS = (1, 3, 6, 12, 24, 30, 96, 128, 130, 258, 960, 1030, 2052)
KCS = (1, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 5000)
KINDS = ("f32", "u8")


@functools.lru_cache(maxsize=None)
def _data(d, kind, n=N):
    """Base, 33 queries (smaller query counts are prefixes) and D32, made once."""
    rng = np.random.default_rng(7 * d + (kind == "u8") + n)
    if kind == "u8":
        X = rng.integers(0, 256, (n, d), dtype=np.uint8)
        Q = (128 + 40 * rng.standard_normal((NQ, d))).astype(np.float32)
    else:
        X = rng.standard_normal((n, d)).astype(np.float32)
        Q = rng.standard_normal((NQ, d)).astype(np.float32)
    D32 = ko.d32(X, Q)
    for a in (X, Q, D32):
        a.setflags(write=False)
    return X, Q, D32


@functools.lru_cache(maxsize=None)
def _cands(d, kind, kc, id_offset=0, id_base=1, n=N):
    """cand [33][kc + 3]: random ids over the base and 5 % beyond it, the padding id here and there, copies wherever kc allows;
    the three columns BEHIND kc hold each query's nearest row, which is nowhere in front of kc."""
    D32 = _data(d, kind, n)[2]
    rng = np.random.default_rng(kc + 13 * d)
    rows = rng.integers(0, n + n // 20 + 1, (NQ, kc + 3)).astype(np.int64)
    best = np.argmin(np.where(np.isnan(D32), np.inf, D32), axis=1)
    rows[rows == best[:, None]] = n + 3
    rows[:, kc:] = best[:, None]
    cand = ((rows + id_offset + id_base) & 0xFFFFFFFF).astype(np.uint32)
    pad = rng.random((NQ, kc + 3)) < 0.02
    pad[:, kc:] = False
    cand[pad] = (0xFFFFFFFF + id_base) & 0xFFFFFFFF
    cand.setflags(write=False)
    return cand


_DS_CACHE = {}


def _dataset(rq, d, kind, n=N):
    key = (d, kind, n)
    if key not in _DS_CACHE:
        _DS_CACHE[key] = rq.Dataset(_data(d, kind, n)[0])
    return _DS_CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _free_datasets():
    yield
    for ds in _DS_CACHE.values():
        ds.close()
    _DS_CACHE.clear()


def _check(got, ref, what=""):
    assert nf.same(got[0], got[1], ref), (what, nf.first_difference(got[0], got[1], ref))


def _ks(kc):
    return sorted({1, (kc + 1) // 2, kc})


# ---- 1. row widths and loaders ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DS)
def test_every_row_width(rq, d, kind):
    _, Q, D32 = _data(d, kind)
    ds = _dataset(rq, d, kind)
    for kc, nq in ((257, 7), (4097, 2)):
        cand = _cands(d, kind, kc)
        for k in (1, (kc + 1) // 2):
            got = ds.rerank(Q[:nq], cand[:nq, :kc], k)
            _check(got, ro.rerank_d(D32[:nq], cand[:nq], kc, k, 0, 1), (d, kind, kc, k))


# ---- 2. slab and sort edges ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nq", [1, 7, 33])
@pytest.mark.parametrize("kc", KCS)
def test_slab_and_sort_edges(rq, kc, nq):
    from rayuela_jl_amd import knn as K
    for kind in KINDS:
        _, Q, D32 = _data(30, kind)
        ds = _dataset(rq, 30, kind)
        cand = _cands(30, kind, kc)                      # ldc = kc + 3 > kc: the columns behind kc would change the answer
        for k in _ks(kc):
            got = ds.rerank(Q[:nq], cand[:nq, :kc], k)
            _check(got, ro.rerank_d(D32[:nq], cand[:nq], kc, k, 0, 1), (kind, kc, k, nq))
        st = K.last_rerank_stats()
        valid = int((ro.rows_of(cand[:nq, :kc], 0, 1) < N).sum())
        assert (st["queries"], st["candidates"], st["valid"], st["chain"]) == (nq, nq * kc, valid, int(kc > 4096)), st


@gpu
def test_ids_behind_kc_would_have_changed_the_answer(rq):
    _, Q, D32 = _data(30, "f32")
    cand = _cands(30, "f32", 256)
    short = ro.rerank_d(D32, cand, 256, 1, 0, 1)
    wide = ro.rerank_d(D32, cand, 259, 1, 0, 1)
    assert np.all(short[1] != wide[1])
    _check(_dataset(rq, 30, "f32").rerank(Q, cand[:, :256], 1), short)


@gpu
@pytest.mark.parametrize("id_base", [0, 1])
@pytest.mark.parametrize("id_offset", [0, 5, (1 << 31) - 5, (1 << 32) - 1 - N])
def test_id_offsets_and_bases(rq, id_offset, id_base):
    _, Q, D32 = _data(30, "u8")
    ds = _dataset(rq, 30, "u8")
    for kc in (257, 4097):
        cand = _cands(30, "u8", kc, id_offset, id_base)
        got = ds.rerank(Q, cand[:, :kc], 40, id_offset=id_offset, id_base=id_base)
        _check(got, ro.rerank_d(D32, cand, kc, 40, id_offset, id_base), (kc, id_offset, id_base))


# ---- 3. both select paths, batches -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_both_select_paths_give_the_same_bytes(rq, kind):
    from rayuela_jl_amd import knn as K
    _, Q, D32 = _data(30, kind)
    ds = _dataset(rq, 30, kind)
    for kc in (100, 65, 4096):
        cand = _cands(30, kind, kc)
        for k in _ks(kc):
            ref = ro.rerank_d(D32, cand, kc, k, 0, 1)
            a = ds.rerank(Q, cand[:, :kc], k)
            assert K.last_rerank_stats()["chain"] == 0
            K.rerank_limits(64, 0)
            try:
                b = ds.rerank(Q, cand[:, :kc], k)
                assert K.last_rerank_stats()["chain"] == 1
                c = ds.rerank(Q, cand[:, :64], min(k, 64))
                assert K.last_rerank_stats()["chain"] == 0       # 64 candidates still sort in LDS
            finally:
                K.rerank_limits(0, 0)
            _check(a, ref, (kc, k, "lds"))
            _check(b, ref, (kc, k, "chain"))
            _check(c, ro.rerank_d(D32, cand, 64, min(k, 64), 0, 1), (kc, k, "lds at the limit"))


@gpu
@pytest.mark.parametrize("kc", [100, 4500])
def test_ragged_batches(rq, kc):
    from rayuela_jl_amd import knn as K
    _, Q, D32 = _data(30, "f32")
    ds = _dataset(rq, 30, "f32")
    cand = _cands(30, "f32", kc)
    ref = ro.rerank_d(D32, cand, kc, 50, 0, 1)
    K.rerank_limits(0, 5)
    try:
        got = ds.rerank(Q, cand[:, :kc], 50)
        st = K.last_rerank_stats()
    finally:
        K.rerank_limits(0, 0)
    assert st["batches"] == 7 and st["queries"] == NQ
    _check(got, ref)
    _check(ds.rerank(Q, cand[:, :kc], 50), ref)
    assert K.last_rerank_stats()["batches"] == 1


# ---- 4. inputs that break a wrong kernel -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kc", [600, 5000])
def test_duplicated_base_rows_order_by_id(rq, kc):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 24)).astype(np.float32)
    X[rng.permutation(N)[:700]] = X[:7].repeat(100, axis=0)        # 7 rows, a hundred copies each
    Q = rng.standard_normal((NQ, 24)).astype(np.float32)
    D32 = ko.d32(X, Q)
    cand = rng.integers(1, N + 1, (NQ, kc)).astype(np.uint32)
    with rq.Dataset(X) as ds:
        for k in _ks(kc) + [100, 101]:
            _check(ds.rerank(Q, cand, k), ro.rerank_d(D32, cand, kc, k, 0, 1), (kc, k))


@gpu
@pytest.mark.parametrize("d", [30, 96, 131])
def test_near_ties_keep_the_summation_order(rq, d):
    X, Q = ko.near_tie(d)
    D32 = ko.d32(X, Q)
    n, nq = X.shape[0], Q.shape[0]
    rng = np.random.default_rng(d)
    with rq.Dataset(X) as ds:
        for kc in (n, 700, 4500):
            cand = rng.integers(0, n, (nq, kc)).astype(np.uint32) if kc != n else np.tile(np.arange(n, dtype=np.uint32), (nq, 1))
            for k in (10, kc):
                _check(ds.rerank(Q, cand, k, id_base=0), ro.rerank_d(D32, cand, kc, k, 0, 0), (d, kc, k))


def _nonfinite_cases():
    rng = np.random.default_rng(8)
    n, d, nq = 200, 6, 5
    X0 = rng.standard_normal((n, d)).astype(np.float32)
    Q0 = rng.standard_normal((nq, d)).astype(np.float32)
    X = X0.copy(); X[3, 2] = np.nan; X[150, 0] = np.nan
    yield "nan_in_rows", X, Q0
    Q = Q0.copy(); Q[1, :] = np.nan                       # an all-NaN query: all padding
    yield "all_nan_query", X0, Q
    X = X0.copy(); X[7, 1] = np.inf; X[8, 5] = -np.inf; X[9, 0] = np.inf; X[10, 0] = np.inf
    Q = Q0.copy(); Q[2, 0] = np.inf                       # Inf - Inf at rows 9 and 10: NaN distances
    yield "inf_in_rows", X, Q
    X = X0.copy(); X[5:, 3] = np.nan                      # five comparable rows
    yield "fewer_comparable_rows_than_k", X, Q0
    yield "f32_overflow", (X0.astype(np.float64) * 1e19).astype(np.float32), (Q0.astype(np.float64) * 1e19).astype(np.float32)
    X = X0.copy(); X[:, :] = np.float32(-0.0)
    yield "negative_zero", X, np.zeros_like(Q0)


@gpu
@pytest.mark.parametrize("name", [c[0] for c in _nonfinite_cases()])
def test_non_finite_inputs_follow_the_contract(rq, name):
    X, Q = next(c[1:] for c in _nonfinite_cases() if c[0] == name)
    D32 = ko.d32(X, Q)
    n, nq = X.shape[0], Q.shape[0]
    if name == "f32_overflow":
        assert np.isinf(D32).sum() > D32.size // 2        # +Inf distances order by id
    rng = np.random.default_rng(3)
    with rq.Dataset(X) as ds:
        for kc in (n, 4200):
            cand = rng.integers(1, n + 1, (nq, kc)).astype(np.uint32) if kc != n else np.tile(np.arange(1, n + 1, dtype=np.uint32), (nq, 1))
            for k in (10, kc):
                got = ds.rerank(Q, cand, k)
                _check(got, ro.rerank_d(D32, cand, kc, k, 0, 1), (name, kc, k))
                if name == "all_nan_query":
                    assert np.all(got[1][1] == 0) and np.all(got[0][1].view(np.uint32) == nf.PAD_BITS)


@gpu
@pytest.mark.parametrize("kc", [70, 4100])
def test_invalid_candidates_and_short_lists(rq, kc):
    _, Q, D32 = _data(30, "f32")
    ds = _dataset(rq, 30, "f32")
    junk = np.full((NQ, kc), N + 1, dtype=np.uint32)      # id_base 1: row N, the first one behind the base
    junk[:, ::3] = 0                                      # the padding id 0xFFFFFFFF + 1
    junk[:, 1::3] = 0xFFFFFFFF
    got = ds.rerank(Q, junk, kc)
    assert np.all(got[1] == 0) and np.all(got[0].view(np.uint32) == nf.PAD_BITS)
    few = junk.copy()
    few[:, 5] = 17; few[:, kc - 1] = 3; few[:, 40] = 17   # three valid candidates, one id twice
    got = ds.rerank(Q, few, 10)
    _check(got, ro.rerank_d(D32, few, kc, 10, 0, 1))
    assert np.all(np.sort(got[1][:, :3], axis=1) == np.array([3, 17, 17])) and np.all(got[1][:, 3:] == 0)


# ---- 5. identity with the exact search -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_all_ids_give_the_bytes_of_knn_f32(rq, kind):
    X, Q, D32 = _data(96, kind)
    ds = _dataset(rq, 96, kind)
    cand = np.tile(np.arange(N, dtype=np.uint32), (NQ, 1))
    for k in (1, 10, N):
        got = ds.rerank(Q, cand, k, id_base=0)
        want = rq.knn_f32(X.astype(np.float32), Q, k, id_base=0)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1].view(np.uint32))
        _check(got, ko.topk_f32(D32, k, 0)[:2])


# ---- 6. scratch and threads ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kc", [257, 4500])
def test_answer_does_not_depend_on_what_scratch_held(rq, kc):
    from rayuela_jl_amd import _lib
    _, Q, D32 = _data(30, "u8")
    ds = _dataset(rq, 30, "u8")
    cand = _cands(30, "u8", kc)
    ref = ro.rerank_d(D32, cand, kc, 77, 0, 1)
    ds.rerank(Q, cand[:, :kc], 77)                        # the scratch exists: the fills below reach it
    for value in (0x00, 0xFF):
        assert _lib.fill_scratch(value)["slot_bytes"] > 0
        _check(ds.rerank(Q, cand[:, :kc], 77), ref, value)


@gpu
def test_two_host_threads_on_one_dataset(rq):
    _, Q, D32 = _data(30, "f32")
    ds = _dataset(rq, 30, "f32")
    jobs = [(257, 20), (4500, 300)]
    refs = [ro.rerank_d(D32, _cands(30, "f32", kc), kc, k, 0, 1) for kc, k in jobs]
    out = [None, None]

    def work(i):
        kc, k = jobs[i]
        res = []
        for _ in range(6):
            res.append(ds.rerank(Q, _cands(30, "f32", kc)[:, :kc], k))
        out[i] = res

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for i in range(2):
        assert out[i] is not None and len(out[i]) == 6
        for got in out[i]:
            _check(got, refs[i], jobs[i])


# ---- 7. errors: checked before any work, no output byte written -------------------------------------------------------------------------
@gpu
def test_bad_arguments_leave_the_outputs_untouched(rq):
    from rayuela_jl_amd import knn as K
    _, Q, _ = _data(6, "f32")
    ds = _dataset(rq, 6, "f32")
    L = rq.lib()
    nq, kc, k = 5, 40, 7
    dists = np.full((nq, 64), 7.5, np.float32)
    ids = np.full((nq, 64), 0xABCDEF01, np.uint32)
    cand = np.zeros((nq, 64), np.uint32)
    p = lambda a: a.ctypes.data                           # noqa: E731
    EINVAL, EUNSUPPORTED = -1, -2
    h = ds._h
    cases = [
        (EINVAL, (None, p(dists), p(ids), p(Q), nq, p(cand), kc, 64, k, 0, 0)),
        (EINVAL, (h, None, p(ids), p(Q), nq, p(cand), kc, 64, k, 0, 0)),
        (EINVAL, (h, p(dists), None, p(Q), nq, p(cand), kc, 64, k, 0, 0)),
        (EINVAL, (h, p(dists), p(ids), None, nq, p(cand), kc, 64, k, 0, 0)),
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, None, kc, 64, k, 0, 0)),
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, p(cand), kc, 64, 0, 0, 0)),          # k < 1
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, p(cand), kc, 64, -3, 0, 0)),
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, p(cand), kc, 64, kc + 1, 0, 0)),     # kc < k
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, p(cand), kc, kc - 1, k, 0, 0)),      # ldc < kc
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, p(cand), kc, 64, k, 0, 2)),          # id_base
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, p(cand), kc, 64, k, 0, -1)),
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, p(cand), kc, 64, k, (1 << 32) - N, 0)),      # n + id_offset = 2^32
        (EINVAL, (h, p(dists), p(ids), p(Q), nq, p(cand), 1 << 31, 1 << 31, k, 0, 0)),
        (EUNSUPPORTED, (h, p(dists), p(ids), p(Q), nq, p(cand), 1 << 28, 1 << 28, k, 0, 0)),  # one query's keys: 2 GiB
    ]
    for want, args in cases:
        assert L.rq_dataset_rerank(*args) == want, (args[4:], L.rq_last_error())
        assert L.rq_last_error() != b""
    assert L.rq_dataset_rerank(h, p(dists), p(ids), p(Q), 0, p(cand), kc, 64, k, 0, 0) == 0       # nq <= 0: nothing to do
    assert L.rq_dataset_rerank(h, None, None, None, -1, None, kc, 64, k, 0, 0) == 0
    assert np.all(dists == 7.5) and np.all(ids == 0xABCDEF01)
    assert L.rq_dataset_rerank(h, p(dists), p(ids), p(Q), nq, p(cand), kc, 64, k, (1 << 32) - 1 - N, 0) == 0   # the last offset
    assert K.last_rerank_stats()["valid"] == 0
    with pytest.raises(ValueError):
        ds.rerank(Q[:nq], cand.astype(np.int64), 3)
    with pytest.raises(ValueError):
        ds.rerank(Q[:nq], cand, 65)


# ---- 8. offsets past 2^31 elements and 2^32 bytes -----------------------------------------------------------------------------------------
GB = float(1 << 30)


def _need_host(nbytes):
    with open("/proc/meminfo") as f:
        avail = {ln.split(":")[0]: int(ln.split()[1]) * 1024 for ln in f}["MemAvailable"]
    if avail < 2 * nbytes:
        pytest.skip("needs 2 x %.1f GiB of host memory, %.1f GiB are available" % (nbytes / GB, avail / GB))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_rows_on_both_sides_of_every_crossing(rq, kind):
    """A periodic base (tests/large_offsets.py): u8 past 2^32 bytes -- which crosses 2^31 and 2^32 elements too -- and f32 past
    2^31 elements (and 2^32 bytes on the way).  nq = 4, kc = 64, candidates on both sides of each crossing; the expected answer
    is computed on the period tile."""
    d, nq, kc, k = 128, 4, 64, 64
    itemsize = 1 if kind == "u8" else 4
    marks = lo.thresholds(d, itemsize)
    n = lo.rows_past(marks[1] if kind == "u8" else max(marks[0], marks[1]))
    marks = [m for m in marks if m < n]
    assert len(marks) == (3 if kind == "u8" else 2)
    _need_host(n * d * itemsize)
    rng = np.random.default_rng(11)
    tile = rng.integers(0, 256, (lo.P, d), dtype=np.uint8) if kind == "u8" else rng.standard_normal((lo.P, d)).astype(np.float32)
    Q = (128 + 40 * rng.standard_normal((nq, d))).astype(np.float32) if kind == "u8" else rng.standard_normal((nq, d)).astype(np.float32)
    rows = np.concatenate([[m - 2, m - 1, m, m + 1, m + lo.P - 1] for m in marks] + [[0, n - 1, n, n + 5]]).astype(np.int64)
    rows = np.concatenate([rows, rng.integers(0, n, kc - rows.size)])
    cand = np.stack([rng.permutation(rows) for _ in range(nq)])
    Dt = ko.d32(tile, Q)                                   # row r of the base is row r % P of the tile
    Dfull = np.full((nq, kc), np.nan, dtype=np.float32)
    ok = cand < n
    Dfull[ok] = np.take_along_axis(Dt, np.where(ok, cand % lo.P, 0), axis=1)[ok]
    bits = np.full((nq, k), nf.PAD_BITS, dtype=np.uint32)
    ids = np.zeros((nq, k), dtype=np.uint32)               # padding id with id_base 1
    for q in range(nq):
        r, dv = cand[q][ok[q]], Dfull[q][ok[q]]
        order = np.lexsort((r, dv))
        bits[q, :order.size] = dv[order].view(np.uint32)
        ids[q, :order.size] = r[order] + 1
    X = lo.periodic(tile, n)
    assert X.nbytes > lo.TWO32
    with rq.Dataset(X) as ds:
        del X
        got = ds.rerank(Q, (cand + 1).astype(np.uint32), k)
    _check(got, (bits, ids), kind)
    assert (ids > marks[-1]).any() and (ids[ids > 0] <= marks[0]).any()
