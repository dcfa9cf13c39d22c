"""GPU: rq_ivf_search_refine and the search_refine drivers.  By definition the fused entry equals
rq_dataset_rerank over the ids rq_ivf_search(k = kc) returns; both are held to the restatements (tests/ivf_oracle.py for the
candidates, tests/rerank_oracle.py for their order), bit for bit.  n = 3000, nlist = 37, (d, m) = (32, 8) and (96, 16), residual
and plain codes, float32 and uint8 datasets."""
import functools

import numpy as np
import pytest

import ivf_oracle as ivf
import knn_oracle as ko
import nonfinite_ref as nf
import rerank_oracle as ro
from test_gpu_ivf_shapes import _shape

pytestmark = pytest.mark.gpu
N, NLIST = 3000, 37
SHAPES = [(32, 8), (96, 16)]


@functools.lru_cache(maxsize=None)
def _case(d, m):
    """integer-valued rows in 0..255 (the byte base is the same base), the distance matrix of the 9 queries, made once"""
    X, Q, centers, Xq = _shape("sift", N, d, m, NLIST)
    assert X.min() >= 0 and X.max() <= 255 and np.array_equal(X, np.rint(X))
    D32 = ko.d32(X, Xq)
    D32.setflags(write=False)
    return X, Q, centers, Xq, D32


@functools.lru_cache(maxsize=None)
def _grouped(d, m, by_residual):
    X, Q, centers, _, _ = _case(d, m)
    return ivf.build(X, Q, centers, by_residual)[0]


def _index(rq, Q, centers, by_residual):
    return rq.IvfIndex(Q, [centers[i] for i in range(centers.shape[0])], by_residual=by_residual)


def _same(got, ref, what=""):
    assert nf.same(got[0], got[1], ref), (what, nf.first_difference(got[0], got[1], ref))


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("by_residual", [True, False])
@pytest.mark.parametrize("d,m", SHAPES)
def test_fused_equals_the_two_calls_and_the_oracle(rq, d, m, by_residual, kind):
    X, Q, centers, Xq, D32 = _case(d, m)
    grouped = _grouped(d, m, by_residual)
    base = X.astype(np.uint8) if kind == "u8" else X
    with _index(rq, Q, centers, by_residual) as ix, rq.Dataset(base) as ds:
        ix.build(X)
        for nprobe in (1, 5, 37):
            rows = ivf.ranked(grouped, Q, centers, by_residual, Xq, nprobe)
            union = int(ivf.union_sizes(grouped, Q, Xq, nprobe).max())
            for k in (1, 10):
                for kc in (k, 4 * k, union + 7):
                    for id_base in ((0, 1) if kc == 4 * k else (1,)):
                        before = ix.search(Xq, nprobe, kc, id_base=id_base)
                        fused = ix.search_refine(Xq, ds, nprobe, k, kc, id_base=id_base)
                        two = ds.rerank(Xq, before[1], k, id_base=id_base)
                        what = (nprobe, k, kc, id_base)
                        assert np.array_equal(fused[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(fused[1], two[1]), what
                        cand = ivf.take(rows, kc, id_base)[1]
                        _same(fused, ro.rerank_d(D32, cand, kc, k, 0, id_base), what)
                        after = ix.search(Xq, nprobe, kc, id_base=id_base)       # the search itself is what it was
                        assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("d,m", SHAPES)
def test_every_list_and_every_row_is_the_exact_search(rq, d, m):
    X, Q, centers, Xq, D32 = _case(d, m)
    with _index(rq, Q, centers, True) as ix, rq.Dataset(X) as ds:
        ix.build(X)
        for kc in (N, N + 100, 5000):
            for k in (1, 10):
                got = ix.search_refine(Xq, ds, NLIST, k, kc, id_base=0)
                want = rq.knn_f32(X, Xq, k, id_base=0)
                assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1].view(np.uint32))
                _same(got, ko.topk_f32(D32, k, 0)[:2], (kc, k))


def test_rows_are_placed_by_id_after_an_add_with_a_gap(rq):
    from rayuela_jl_amd import knn as K
    d, m = 32, 8
    X, Q, centers, Xq, _ = _case(d, m)
    id_offset, gap, first = 100, 500, 2000
    base = np.full((N + gap, d), 255, dtype=np.float32)       # row i holds the vector with id i + id_offset; the gap is far away
    base[:first] = X[:first]
    base[first + gap:] = X[first:]
    D32 = ko.d32(base, Xq)
    with _index(rq, Q, centers, True) as ix, rq.Dataset(base) as ds:
        ix.build(X[:first], id_offset=id_offset)
        ix.add(X[first:], id_offset=id_offset + first + gap)
        for nprobe, k, kc in ((5, 10, 40), (37, 10, 4200), (37, 1, 300)):
            cand = ix.search(Xq, nprobe, kc)[1]
            fused = ix.search_refine(Xq, ds, nprobe, k, kc, id_offset=id_offset)
            _same(fused, ro.rerank_d(D32, cand, kc, k, id_offset, 1), (nprobe, k, kc))
            st = K.last_rerank_stats()
            assert st["queries"] == Xq.shape[0] and st["candidates"] == Xq.shape[0] * kc and st["chain"] == int(kc > 4096)
            assert st["valid"] == int((ro.rows_of(cand, id_offset, 1) < base.shape[0]).sum())
            two = ds.rerank(Xq, cand, k, id_offset=id_offset)
            assert np.array_equal(fused[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(fused[1], two[1])
        ids = ix.search_refine(Xq, ds, 37, 10, 300, id_offset=id_offset)[1].astype(np.int64) - 1 - id_offset
        assert ((ids < first) | (ids >= first + gap)).all() and (ids >= first + gap).any()


def test_a_dataset_of_the_wrong_width_is_refused(rq):
    X, Q, centers, Xq, _ = _case(32, 8)
    L = rq.lib()
    with _index(rq, Q, centers, True) as ix, rq.Dataset(np.zeros((N, 33), np.float32)) as wrong, rq.Dataset(X) as ds:
        ix.build(X)
        want = ix.search(Xq, 5, 10)
        dists = np.full((9, 10), 7.5, np.float32)
        ids = np.full((9, 10), 0xABCDEF01, np.uint32)
        p = lambda a: a.ctypes.data                           # noqa: E731
        args = (p(dists), p(ids), p(Xq), 9, 5)
        assert L.rq_ivf_search_refine(ix._h, wrong._h, *args, 10, 40, 0, 1) == -1
        assert b"d=33" in L.rq_last_error()
        for k, kc, id_offset, id_base in ((0, 40, 0, 1), (10, 9, 0, 1), (10, 40, 0, 2), (10, 40, (1 << 32) - N, 1)):
            assert L.rq_ivf_search_refine(ix._h, ds._h, *args, k, kc, id_offset, id_base) == -1, (k, kc, id_offset, id_base)
        assert L.rq_ivf_search_refine(ix._h, None, *args, 10, 40, 0, 1) == -1
        assert L.rq_ivf_search_refine(ix._h, ds._h, p(dists), p(ids), p(Xq), 9, 38, 10, 40, 0, 1) == -1      # nprobe > nlist
        assert np.all(dists == 7.5) and np.all(ids == 0xABCDEF01)
        with pytest.raises(rq.RayuelaHipError):
            ix.search_refine(Xq, wrong, 5, 10, 40)
        got = ix.search(Xq, 5, 10)                            # the loaded base still answers
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("shards", [1, 2])
def test_index_search_refine_is_the_two_call_composition(rq, shards):
    import rayuela_jl_amd.synth as synth
    rng = np.random.default_rng(4)
    n, d, m, nq = 5000, 32, 4, 9
    X = rng.standard_normal((n, d)).astype(np.float32)
    Xq = rng.standard_normal((nq, d)).astype(np.float32)
    D32 = ko.d32(X, Xq)
    C = synth.codebooks(X, m, 256, seed=3, iters=1, sample=n)
    B = rq.quantize_pq(X, C)
    R = synth.rotation(d)
    with rq.Dataset(X) as ds:
        with rq.Index(C, d, devices=[0] * shards) as ix:
            ix.set_codes(B)
            for k, kc, Rq in ((10, 100, None), (1, 4500 if shards == 1 else 64, None), (5, 50, R)):
                cand = ix.search(Xq, k=kc, R=Rq)[1]
                got = ix.search_refine(Xq, ds, k, kc, R=Rq)
                two = ds.rerank(Xq, cand, k)
                assert np.array_equal(got[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(got[1], two[1])
                _same(got, ro.rerank_d(D32, cand, kc, k, 0, 1), (k, kc))         # unrotated queries against the unrotated base
        Cf = [np.ascontiguousarray(np.pad(c, ((0, 0), (i * (d // m), d - (i + 1) * (d // m))))) for i, c in enumerate(C)]
        with rq.AqIndex(Cf, kind="cq", devices=[0] * shards) as aq:
            aq.set_codes(B)
            cand = aq.search(Xq, k=80)[1]
            got = aq.search_refine(Xq, ds, 7, 80)
            two = ds.rerank(Xq, cand, 7)
            assert np.array_equal(got[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(got[1], two[1])
            _same(got, ro.rerank_d(D32, cand, 80, 7, 0, 1))


def test_experiment_ivfpq_reports_the_restated_recall(rq):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.experiments import experiment_ivfpq
    n, d, nq = 4000, 32, 50
    Xb = synth.deep_like(n, d, seed=1)
    Xq = synth.deep_like(nq, d, seed=2)
    plain = experiment_ivfpq(Xb, Xb, Xq, nlist=16, m=4, nprobes=(2, 16), niter=3, knn=100)
    assert len(plain) == 3                                    # the default: today's output
    Q, C, recall, refined = experiment_ivfpq(Xb, Xb, Xq, nlist=16, m=4, nprobes=(2, 16), niter=3, knn=100, refine=400)
    assert np.array_equal(Q, plain[0]) and all(np.array_equal(recall[p], plain[2][p]) for p in (2, 16))
    truth = ko.topk_f64(ko.d64(Xb, Xq), 1, 1)[1][:, 0].astype(np.int64)
    D32 = ko.d32(Xb, Xq)
    with rq.IvfIndex(Q, C) as ix:
        ix.build(Xb)
        for nprobe in (2, 16):
            adc = ix.search(Xq, nprobe, 100)[1].astype(np.int64)
            cand = ix.search(Xq, nprobe, 400)[1]
            ref = ro.rerank_d(D32, cand, 400, 100, 0, 1)[1].astype(np.int64)
            for name, ids in (("adc", adc), ("refined", ref)):
                want = {r: float((ids[:, :r] == truth[:, None]).any(axis=1).mean()) for r in (1, 10, 100)}
                assert refined[nprobe][name] == want, (nprobe, name)
        assert refined[16]["refined"][1] >= refined[16]["adc"][1]
    with pytest.raises(ValueError):
        experiment_ivfpq(Xb, Xb, Xq, nlist=16, m=4, nprobes=(2,), niter=1, knn=100, refine=50)
