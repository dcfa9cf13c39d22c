"""GPU: the two drivers of the IVFADC index, train_ivfpq (rayuela_jl_amd/IVF.py) and experiment_ivfpq
(rayuela_jl_amd/experiments.py), on integer-valued data, where training is exact.

train_ivfpq is a composition, so it is held to its parts bit for bit -- Q to train_pq at m = 1, C to train_pq on the residuals
the restatement (tests/ivf_oracle.py) takes under that Q -- and Q itself to the k-means restatement step by step from the
library's own previous state, with the comparison of tests/test_gpu_kmeans.py on the byte route (nlist <= 256) and of
tests/test_gpu_train_wide.py on the 16-bit route: the chain ends at an oracle.  experiment_ivfpq's recall curves are those of the
restated build and search under the trained Q and C."""
import numpy as np
import pytest

import ivf_oracle as ivf
import kmeans_oracle as ko
import train_wide_oracle as two

pytestmark = pytest.mark.gpu

M, NITER = 4, 3


@pytest.mark.parametrize("nlist", [40, 300])          # the byte route and the 16-bit route of the coarse k-means
def test_train_ivfpq_is_train_pq_on_the_restated_residuals(rq, oracle, nlist):
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(4000, 16, seed=41)
    seed = 2
    Qw = rq.train_pq(X, 1, nlist, NITER, seed=seed)[0][0]
    for by_residual in (True, False):
        Q, C = rq.train_ivfpq(X, nlist, M, niter=NITER, seed=seed, by_residual=by_residual)
        assert Q.dtype == np.float32 and Q.shape == (nlist, 16) and two.same_bits([Q], [Qw])
        Xe = ivf.residuals(X, Q, ivf.lists_of(X, Q)) if by_residual else X
        Cw = rq.train_pq(Xe, M, 256, NITER, seed=seed + 1)[0]
        assert len(C) == M and two.same_bits(C, Cw), by_residual
        with rq.IvfIndex(Q, C, by_residual=by_residual) as ix:      # what the driver returns is what the index takes
            ix.build(X)
            want = ivf.build(X, Q, np.stack(C), by_residual)[0]
            off, ids, codes = ix.lists()
            assert np.array_equal(off, want[0]) and np.array_equal(ids, want[1]) and np.array_equal(codes, want[2])

    # Q against the restated k-means: start rows, then every iteration from the library's previous centres
    def train(k):
        return rq.train_pq(X, 1, nlist, k, seed=seed)[0]

    rows, rng = two.start_rows(X, 1, nlist, seed, ko.SALT_PQ, True)
    C_k = train(0)
    assert two.same_bits(C_k, ko.seed_subvectors(X, 1, rows)), "start rows"
    prev = None
    for k in range(NITER):
        codes = two.encode(oracle, X, C_k, 1, nlist)
        if prev is not None and np.array_equal(codes, prev):
            break                                                   # the restated stopping rule: later iterations change nothing
        C_next, repicked, counts = two.lloyd_step(X, C_k, codes, 1, nlist, rng)
        C_k1 = train(k + 1)
        used = counts[0] > 0
        if nlist > 256:
            assert two.same_bits(C_k1, C_next), k
        else:
            assert np.allclose(C_k1[0][used], C_next[0][used], rtol=1e-5, atol=1e-4), k
            assert np.array_equal(C_k1[0][~used], C_next[0][~used].astype(np.float32)), (k, repicked)
        for (_, _, _, branch, margin) in repicked:
            if branch == "cost":
                assert margin > 1e-9, (k, margin)
        prev, C_k = codes, C_k1
    assert two.same_bits(C_k, [Qw])


def test_train_ivfpq_argument_errors_raise_before_the_library(rq):
    X = np.zeros((400, 16), dtype=np.float32)
    with pytest.raises(ValueError):
        rq.train_ivfpq(X, 40, 3)                      # d % m != 0
    with pytest.raises(ValueError):
        rq.train_ivfpq(X, 0, 4)
    with pytest.raises(ValueError):
        rq.train_ivfpq(X, 32768, 4)


@pytest.mark.parametrize("by_residual", [True, False])
def test_experiment_ivfpq_recall_is_the_restated_search(rq, oracle, by_residual):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.experiments import experiment_ivfpq
    d, nlist, knn, nprobes = 16, 16, 10, (1, 4, 16)
    Xb = synth.sift_like(3000, d, seed=42)
    Xt, Xq = synth.sift_like(2000, d, seed=43), synth.sift_like(33, d, seed=44)
    dd = ((Xq.astype(np.float64)[:, None, :] - Xb.astype(np.float64)[None, :, :]) ** 2).sum(-1)     # integers: exact
    truth = (dd.argmin(1) + 1).astype(np.uint32)      # the first of equal rows, as groundtruth orders ties by id
    for gt in (truth, None):
        Q, C, recall = experiment_ivfpq(Xt, Xb, Xq, gt, nlist=nlist, m=M, nprobes=nprobes, niter=NITER, knn=knn,
                                        by_residual=by_residual, seed=1)
        centers = np.stack(C)
        assert Q.shape == (nlist, d) and centers.shape == (M, 256, d // M) and sorted(recall) == list(nprobes)
        grouped = ivf.build(Xb, Q, centers, by_residual)[0]
        for nprobe in nprobes:
            ids = ivf.search(grouped, Q, centers, by_residual, Xq, nprobe, knn)[1]
            want = rq.eval_recall(truth, ids, knn, verbose=False)
            print("by_residual %d nprobe %2d: recall@1 %.3f @10 %.3f" % (by_residual, nprobe, want[0], want[-1]))
            assert recall[nprobe].shape == (knn,) and np.array_equal(recall[nprobe], want), (gt is None, nprobe)
        last = [recall[nprobe][-1] for nprobe in nprobes]
        assert all(b >= a for a, b in zip(last, last[1:])), last
        if not by_residual:                            # every list probed, the query's own table: the exhaustive scan
            _, idx = rq.linscan_pq(rq.quantize_pq(Xb, C), Xq, C, 8 * M, knn)
            assert np.array_equal(recall[nlist], rq.eval_recall(truth, idx, knn, verbose=False))
