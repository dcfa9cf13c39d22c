"""Training with more than 256 codewords per codebook (rq_train_pq_wide, rq_train_opq_wide, rq_train_rvq_wide and the two
reductions rq_dev_update_centers_wide / rq_dev_reconstruct_wide) against tests/train_wide_oracle.py, the step-by-step
restatement (tests/test_train_wide_oracle.py checks that one, and the fixtures, on the CPU).

Tolerances: bits wherever the data is integer-valued (segment sums below 2^24 are exact in any summation order, so the means
float32(sum) * (float32(1) / float32(count)) are the answer, and so is every centre, code, repick and iteration count of the Lloyd
loop); rtol = atol = 1e-5 on means of unit-variance Gaussian rows (what tests/test_gpu_train.py holds the byte kernel to); for
train_opq the tolerances of test_train_opq_follows_the_oracle_loop, for its reason (two SVDs)."""
import ctypes

import numpy as np
import pytest

import kmeans_oracle as ko
import train_wide_oracle as two
import train_wide_stream_cases  # noqa: F401  (registers the stream cases of the *_wide training reductions)
import wide_oracle as wo
from switch_table import switches

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2
# (n, d, m, h): ragged last tile and h % 16 != 0 | four full blocks | uneven split 3, 3, 2, 2 and a last block of one code |
# the largest h, most codes empty | fewer rows than one 64-row step | more than one 16-dimension block per sub-space, d > 128
SHAPES = [(3001, 32, 4, 300), (2000, 128, 8, 1024), (1000, 10, 4, 257), (40000, 8, 1, 32767), (33, 16, 2, 512),
          (1500, 200, 2, 600)]


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _p(a):
    return a.ctypes.data


def _start_centres(rng, d, m, h):
    off = wo.splitarray(d, m)
    return [rng.standard_normal((h, off[q + 1] - off[q])).astype(np.float32) * 20 for q in range(m)]


def _split(Ccat, d, m, h):
    return wo.sub_codebooks(Ccat, d, m, h)[0]


def _update(X, codes, C0, m, h):
    """(C list, counts (m, h)) of rq_dev_update_centers_wide."""
    import torch
    import rayuela_jl_amd.device as rqd
    dC = torch.from_numpy(two.cat(C0)).cuda()
    counts = rqd.update_centers_wide(dC, torch.from_numpy(X).cuda(), torch.from_numpy(np.ascontiguousarray(codes)).cuda(), m, h)
    torch.cuda.synchronize()
    return _split(dC.cpu().numpy(), X.shape[1], m, h), counts.cpu().numpy().astype(np.int64)


def _check_exact(X, codes, C0, m, h):
    want, cnt = two.exact_means(X, C0, codes, m, h)
    got, gcnt = _update(X, codes, C0, m, h)
    assert np.array_equal(gcnt, cnt)
    for i in range(m):
        assert np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32)), (i, int((got[i] != want[i]).any(axis=1).sum()))
        empty = cnt[i] == 0
        assert np.array_equal(got[i][empty].view(np.uint32), C0[i][empty].view(np.uint32))     # emptied codes keep their bits
    again, acnt = _update(X, codes, C0, m, h)
    assert two.same_bits(again, got) and np.array_equal(acnt, gcnt)
    return cnt


# ---- 1. update_centers_wide ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_update_centers_wide_is_exact_on_integer_data(shape):
    n, d, m, h = shape
    rng = np.random.default_rng(sum(shape))
    X = ko.int_data(n, d, 7 + h)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    cnt = _check_exact(X, codes, _start_centres(rng, d, m, h), m, h)
    if h == 32767:
        assert (cnt == 0).mean() > 0.2
    assert (codes >= 256).any()


@pytest.mark.parametrize("case", ["last_block", "one_row_past_a_pair"])
def test_update_centers_wide_edges(case):
    rng = np.random.default_rng(3)
    if case == "last_block":           # every row's code in the ragged last block of 300 codes: the other blocks sum nothing
        n, d, m, h = 3000, 12, 3, 300
        codes = rng.integers(256, h, (n, m)).astype(np.int16)
    else:                              # n = 65: one row past a pair of 32-row steps
        n, d, m, h = 65, 16, 2, 300
        codes = rng.integers(0, h, (n, m)).astype(np.int16)
    X = ko.int_data(n, d, 19)
    _check_exact(X, codes, _start_centres(rng, d, m, h), m, h)


@pytest.mark.parametrize("shape", [(3001, 32, 4, 300), (2000, 96, 16, 1024)])
def test_update_centers_wide_on_gaussian_rows(shape):
    """Unit-variance Gaussian rows against float64 means at rtol = atol = 1e-5, the tolerance test_update_centers_any_width
    holds the byte kernel to; with uniform codes a code has ~10 (h = 300) or ~2 (h = 1024) rows, fewer than in that test."""
    n, d, m, h = shape
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    C0 = _start_centres(rng, d, m, h)
    got, gcnt = _update(X, codes, C0, m, h)
    off = wo.splitarray(d, m)
    want = two.float_means([c.astype(np.float64) for c in C0], X, codes, off, h)
    for i in range(m):
        cnt = np.bincount(codes[:, i], minlength=h)
        assert np.array_equal(gcnt[i], cnt)
        assert np.allclose(got[i], want[i], rtol=1e-5, atol=1e-5), i
        assert np.array_equal(got[i][cnt == 0].view(np.uint32), C0[i][cnt == 0].view(np.uint32))


# ---- 2. out-of-range codes -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3001, 32, 4, 300), (2000, 16, 2, 512)])
def test_update_centers_wide_ignores_codes_out_of_range(shape):
    n, d, m, h = shape
    rng = np.random.default_rng(5)
    X = ko.int_data(n, d, 23)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    C0 = _start_centres(rng, d, m, h)
    col = 1
    rows = np.arange(0, n, 10)
    bad = codes.copy()
    bad[rows, col] = np.array([-1, h, h + 255, 32767], dtype=np.int16)[np.arange(rows.size) % 4]
    got, gcnt = _update(X, bad, C0, m, h)
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    rest, rcnt = two.exact_means(X[keep], C0, codes[keep], m, h)          # the restatement on the remaining rows
    full, fcnt = two.exact_means(X, C0, codes, m, h)
    for i in range(m):
        w, c = (rest[i], rcnt[i]) if i == col else (full[i], fcnt[i])       # the other columns are unaffected
        assert np.array_equal(gcnt[i], c), i
        assert np.array_equal(got[i].view(np.uint32), w.view(np.uint32)), i
    assert two.same_bits(two.exact_means(X, C0, bad, m, h)[0], got)


# ---- 3. reconstruct_wide -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES + [(65, 16, 2, 300)])
def test_reconstruct_wide_is_the_gather(shape):
    import torch
    import rayuela_jl_amd.device as rqd
    n, d, m, h = shape
    rng = np.random.default_rng(sum(shape) + 1)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    C = _start_centres(rng, d, m, h)
    off = wo.splitarray(d, m)
    CB = rqd.reconstruct_wide(torch.from_numpy(codes).cuda(), torch.from_numpy(two.cat(C)).cuda(), d, h).cpu().numpy()
    assert np.array_equal(CB.view(np.uint32), two.reconstruct(C, codes, off, d).view(np.uint32))
    # a code outside [0, h) is not looked up: its sub-space of the row is zeros (include/rayuela_hip.h)
    bad = codes.copy()
    rows = np.arange(0, n, 7)
    bad[rows, m - 1] = np.array([-1, h, 32767], dtype=np.int16)[np.arange(rows.size) % 3]
    CB2 = rqd.reconstruct_wide(torch.from_numpy(bad).cuda(), torch.from_numpy(two.cat(C)).cuda(), d, h).cpu().numpy()
    want = two.reconstruct(C, codes, off, d)
    want[rows, off[m - 1]:] = 0.0
    assert np.array_equal(CB2.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", sorted(train_wide_stream_cases.TRAIN_WIDE_CASES))
def test_wide_reductions_are_ordered_on_a_side_stream(rq, name):
    """tests/test_gpu_streams.py::test_entry_point_is_ordered_on_a_side_stream runs the cases that are registered when that file
    is collected, which is before this one; the two cases of tests/train_wide_stream_cases.py take the same steps here: once
    without delay (grows the stream's scratch), then behind a delay kernel with poisoned inputs on the null stream's side."""
    import torch
    import stream_cases as sc
    from rayuela_jl_amd import _lib
    from test_gpu_streams import DELAY_CYCLES, _caught, _control_case
    null = torch.cuda.default_stream()
    on_null = _control_case(null)
    stream = None
    for _ in range(16):                 # a side stream on which the harness SEES work misplaced on the null stream
        s = torch.cuda.Stream()
        if s.cuda_stream != null.cuda_stream and _caught(on_null, s, 3) == 3:
            stream = s
            break
    assert stream is not None
    try:
        case = sc.get(name)
        case.check(sc.run_on_side_stream(case, stream, 0))
        case.check(sc.run_on_side_stream(case, stream, DELAY_CYCLES))
    finally:
        torch.cuda.synchronize()
        _lib.check(_lib.lib().rq_release_workspaces())


# ---- 4. h <= 256 through the wide entries: the bits of the byte entry points ---------------------------------------------------

def _train_pq_wide(X, m, h, niter, seed, base):
    n, d = X.shape
    C, B, err = np.empty(h * d, np.float32), np.empty((n, m), np.int16), ctypes.c_double(0)
    st = _L().rq_train_pq_wide(_p(C), _p(B), ctypes.cast(ctypes.byref(err), ctypes.c_void_p), _p(X), n, d, m, h, niter, seed, base)
    assert st == 0
    return C, B, err.value


def _train_rvq_wide(X, m, h, niter, seed, base):
    n, d = X.shape
    C, B, err = np.empty((m, h, d), np.float32), np.empty((n, m), np.int16), ctypes.c_double(0)
    st = _L().rq_train_rvq_wide(_p(C), _p(B), ctypes.cast(ctypes.byref(err), ctypes.c_void_p), _p(X), n, d, m, h, niter, seed, base)
    assert st == 0
    return C, B, err.value


def _train_opq_wide(X, m, h, niter, seed, base):
    n, d = X.shape
    C, B = np.empty(h * d, np.float32), np.empty((n, m), np.int16)
    R, obj = np.empty((d, d), np.float32), np.zeros(niter + 1, np.float32)
    st = _L().rq_train_opq_wide(_p(C), _p(B), _p(R), _p(obj), _p(X), n, d, m, h, niter, 1, seed, None, None, base)
    assert st == 0
    return C, B, R, obj


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("h", [64, 256])
@pytest.mark.parametrize("base", [0, 1])
def test_wide_training_entries_return_the_byte_bits_up_to_256_codewords(rq, h, base):
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(3000, 18, seed=40 + h)
    m, niter, seed = 4, 3, 5                             # d = 18, m = 4: uneven split
    C, B, e = rq.train_pq(X, m, h, niter=niter, seed=seed)
    Cw, Bw, ew = _train_pq_wide(X, m, h, niter, seed, base)
    assert np.array_equal(_bits(Cw), _bits(two.cat(C))) and np.array_equal(Bw, B - 1 + base) and ew == e
    C, B, e = rq.train_rvq(X, 2, h, niter=niter, seed=seed)
    Cw, Bw, ew = _train_rvq_wide(X, 2, h, niter, seed, base)
    assert np.array_equal(_bits(Cw), _bits(np.stack(C))) and np.array_equal(Bw, B - 1 + base) and ew == e
    C, B, R, obj = rq.train_opq(X, m, h, niter, "random", seed=seed)
    Cw, Bw, Rw, objw = _train_opq_wide(X, m, h, niter, seed, base)
    assert np.array_equal(_bits(Cw), _bits(two.cat(C))) and np.array_equal(Bw, B - 1 + base)
    assert np.array_equal(_bits(Rw), _bits(R)) and np.array_equal(_bits(objw), _bits(obj))


def test_update_centers_wide_at_256_codewords_equals_the_byte_kernel():
    import torch
    import rayuela_jl_amd.device as rqd
    n, d, m, h = 5001, 30, 4, 256
    rng = np.random.default_rng(8)
    X = (rng.standard_normal((n, d)) * 20 + 3).astype(np.float32)
    codes = rng.integers(0, h, (n, m)).astype(np.uint8)
    C0 = _start_centres(rng, d, m, h)
    dC = torch.from_numpy(two.cat(C0)).cuda()
    cnt = rqd.update_centers(dC, torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda(), m, h).cpu().numpy()
    got, gcnt = _update(X, codes.astype(np.int16), C0, m, h)
    assert np.array_equal(_bits(two.cat(got)), _bits(dC.cpu().numpy())) and np.array_equal(gcnt, cnt)


# ---- 5. the wide Lloyd loop, step by step --------------------------------------------------------------------------------------

# tests/test_train_wide_oracle.py derives these on the CPU: name -> per seed (K, cost-proportional, uniform, centres >= 256)
WALKS = {
    "crowded_uniform_start": {1: (5, 251, 0, 41), 2: (5, 259, 0, 39), 3: (5, 251, 0, 36)},
    "five_points": {3: (1, 0, 295, 44)},
    "sift": {4: (27, 0, 0, 0)},
    "one_past_a_block": {2: (18, 0, 0, 0)},
}


def _same(a, b):
    return two.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", two.FIXTURES)
def test_wide_lloyd_loop_step_by_step_and_stopping(rq, oracle, name):
    """train(0) is the restated start (kmeans++ / sample_distinct at h > 256); every iteration from the library's own previous
    state: B_k = the wide encode oracle + 1 = quantize_pq(X, C_k), C_{k+1} = the exact restated step bit for bit, repicked
    centres exactly the restated rows; then the stopping rule and the iteration count of rq_train_profile."""
    from rayuela_jl_amd import _lib
    X, m, h, seeds, kmpp = two.lloyd_fixture(name)
    for seed in seeds:
        stats = two.new_stats()
        with switches(**({} if kmpp else dict(TRAIN_KMPP=0))):
            rows, rng = two.start_rows(X, m, h, seed, ko.SALT_PQ, kmpp)

            def train(k):
                C, B, _ = rq.train_pq(X, m, h, niter=k, seed=seed)
                return C, B

            K, C_K, B_K = two.telescope(train, rq.quantize_pq, oracle, X, m, h, rng, rows, stats)
            assert _lib.train_profile()["iterations"] == K              # the last call of the walk was niter = K
            for niter in (K + 1, max(50, K + 7)):
                assert _same(train(niter), (C_K, B_K)), niter
                assert _lib.train_profile()["iterations"] == K, niter
        print("%s seed %d: converged at iteration %d; repicks: %d cost-proportional, %d uniform, %d of centres >= 256; "
              "smallest margin %.3g" % (name, seed, K, stats["cost"], stats["uniform"], stats["wide"], stats["margin"]))
        assert (K, stats["cost"], stats["uniform"], stats["wide"]) == WALKS[name][seed], (seed, K, stats)
        if name != "five_points":          # (five distinct points: the first five centres hold every row)
            assert (B_K > 256).any()


# ---- 6. train_rvq --------------------------------------------------------------------------------------------------------------

def test_train_rvq_wide_one_stage_follows_the_restatement_with_salt_3(rq, oracle):
    X, _, h, (seed,), _ = two.lloyd_fixture("one_past_a_block")
    stats = two.new_stats()
    rows, rng = two.start_rows(X, 1, h, seed, ko.SALT_RVQ, True)

    def train(k):
        C, B, _ = rq.train_rvq(X, 1, h, niter=k, seed=seed)
        return C, B

    K, C_K, B_K = two.telescope(train, lambda X_, C_: rq.quantize_rvq(X_, C_)[0], oracle, X, 1, h, rng, rows, stats)
    assert K == 15                                                      # tests/test_train_wide_oracle.py
    for niter in (K + 1, max(50, K + 7)):
        assert _same(train(niter), (C_K, B_K)), niter
    assert not np.array_equal(rows, two.start_rows(X, 1, h, seed, ko.SALT_PQ, True)[0])


def test_train_rvq_wide_two_stages_seed_from_one_stream(rq, oracle):
    """niter = 0 on integer data: stage 0 is the kmeans++ rows of X, stage 1 the kmeans++ rows of the float32 residual, drawn
    with the NEXT h uniforms of the same stream."""
    n, d, h, seed = 700, 8, 300, 5
    X = ko.int_data(n, d, 61)
    C, B, err = rq.train_rvq(X, 2, h, niter=0, seed=seed)
    rng = ko.Rng(seed, ko.SALT_RVQ)
    s0 = ko.kmpp_seeds(X, 1, h, rng=rng)[0]
    assert np.array_equal(C[0], X[s0])
    b0 = wo.encode_pq_wide(oracle, X, C[0].reshape(-1), 1, h)[:, 0]
    assert np.array_equal(B[:, 0], b0 + 1)
    Xr = X - C[0][b0]
    assert np.abs(Xr).max() <= 255 and np.array_equal(Xr, np.round(Xr))
    s1 = ko.kmpp_seeds(Xr, 1, h, rng=rng)[0]
    assert np.array_equal(C[1], Xr[s1])
    b1 = wo.encode_pq_wide(oracle, Xr, C[1].reshape(-1), 1, h)[:, 0]
    assert np.array_equal(B[:, 1], b1 + 1)
    assert not np.array_equal(s1, ko.kmpp_seeds(Xr, 1, h, seed, salt=ko.SALT_RVQ)[0])   # a restarted stream draws other rows
    assert B.dtype == np.int16 and np.array_equal(B, rq.quantize_rvq(X, C)[0]) and (B > 256).any()
    e0 = float((((Xr - C[1][b1]).astype(np.float64)) ** 2).sum() / n)
    assert abs(err - e0) <= 1e-9 * max(e0, 1.0)


# ---- 7. train_opq --------------------------------------------------------------------------------------------------------------

def test_train_opq_wide_follows_the_restated_loop(rq, oracle):
    import rayuela_jl_amd.synth as synth
    n, d, m, h, niter = 12000, 32, 4, 300, 4
    X = synth.sift_like(n, d, seed=3)
    R0 = synth.rotation(d, seed=5)
    C0 = synth.codebooks(oracle.rotate_T(R0, X), m, h, seed=9, iters=0, sample=2000)
    C, B, R, obj = rq.train_opq(X, m, h, niter, "natural", R0=R0, C0=C0)
    Co, codes_o, Ro, obj_o = two.train_opq(oracle, X, m, h, niter, R0, C0)
    # the two sides take their polar factor from different SVDs (the library's own, LAPACK in numpy), so R -- and with it a
    # handful of near-tie assignments -- agree to float tolerance
    assert obj.shape == (niter + 1,) and B.dtype == np.int16
    print("train_opq wide: obj %s restated %s; assignments differing %.4f" % (obj, obj_o, (B - 1 != codes_o).mean()))
    assert np.allclose(obj, obj_o, rtol=3e-4)
    assert (np.diff(obj) <= 1e-5 * obj[:-1]).all()           # the alternating minimisation never goes up
    assert np.abs(R @ R.T - np.eye(d)).max() < 1e-5          # R stays orthonormal
    assert (B - 1 != codes_o).mean() < 2e-2                  # same assignments up to float near-ties
    assert np.array_equal(B, rq.quantize_opq(X, R, C)) and (B > 256).any()


@pytest.mark.parametrize("d,m", [(8, 2), (9, 3)])
def test_train_opq_wide_starts_from_sample_distinct_with_salt_2(rq, oracle, d, m):
    """train_opq(niter = 0, "natural") without C0 at h = 300: the sampled start C_i = X[sample_distinct(...)] (salt 2, sub-space
    by sub-space; gathered by one kernel per sub-space at h > 256) is pinned through obj[0], the error of the start centres and
    their assignments -- an exact integer sum on integer data, so float32(sum / n) exactly -- and through the returned centres:
    a centre without rows keeps its sampled row exactly."""
    n, h, seed = 900, 300, 8
    X = ko.int_data(n, d, 71)
    off = wo.splitarray(d, m)
    rng = ko.Rng(seed, ko.SALT_OPQ)
    rows = [ko.sample_distinct(rng, n, h) for _ in range(m)]
    C0 = ko.seed_subvectors(X, m, rows)
    codes0 = two.encode(oracle, X, C0, m, h)
    err = 0.0
    for i in range(m):
        err += float(((X[:, off[i]:off[i + 1]].astype(np.float64) - C0[i].astype(np.float64)[codes0[:, i]]) ** 2).sum())
    C, B, R, obj = rq.train_opq(X, m, h, 0, "natural", seed=seed)
    assert obj.shape == (1,) and obj[0] == np.float32(err / n), (obj, err / n)
    other = ko.Rng(seed, ko.SALT_PQ)
    assert [ko.sample_distinct(other, n, h) for _ in range(m)] != rows
    RX = rq.rotate(R, X)
    want = two.float_means(C0, RX, codes0, off, h)
    for i in range(m):
        used = np.bincount(codes0[:, i], minlength=h) > 0
        assert np.allclose(C[i][used], want[i][used], rtol=1e-5, atol=1e-4), i
        assert np.array_equal(C[i][~used], C0[i][~used]), i
    assert np.array_equal(B, rq.quantize_opq(X, R, C))


# ---- 8. landing point against Clustering's rules --------------------------------------------------------------------------------

def test_train_pq_wide_lands_where_clustering_kmeans_rules_land(rq, oracle):
    """The final quantisation error against the restated Clustering.kmeans (kmeans++ seeding, repick proportional to cost, stop
    on |objv - prev| < 1e-6) with the wide assignment, and against it alone.  The data is real-valued, so repicks and near-ties
    differ and the two sides draw from different streams: the library's error on a seed is one more draw from the distribution
    the yardstick's six seeds sample.  It may lie outside their [min, max] by no more than that range's own width."""
    import rayuela_jl_amd.synth as synth
    X = synth.deep_like(8000, 16, seed=1)
    m, h, niter = 2, 300, 25
    eo = [two.train_pq_clustering(oracle, X, m, h, niter, seed)[2] for seed in range(1, 7)]
    lo, hi = min(eo), max(eo)
    eg = []
    for seed in (1, 2, 3):
        C, B, e = rq.train_pq(X, m, h, niter=niter, seed=seed)
        assert np.array_equal(B, rq.quantize_pq(X, C))
        eg.append(e)
    print("train_pq wide: library %s  yardstick min %.6g max %.6g mean %.6g" % (np.round(eg, 6), lo, hi, np.mean(eo)))
    assert hi > lo
    assert all(lo - (hi - lo) <= e <= hi + (hi - lo) for e in eg), (eg, eo)


# ---- statuses: every argument is checked before any work, and no output byte is written ------------------------------------------

def test_wide_training_argument_errors(rq):
    import torch
    L = _L()
    n, d, m, h = 400, 8, 2, 300
    X = ko.int_data(n, d, 3)
    C = np.full(h * d, 7.0, np.float32)
    Cr = np.full((2, h, d), 7.0, np.float32)
    B = np.full((n, m), -3, np.int16)
    R = np.full((d, d), 7.0, np.float32)
    obj = np.full(3, 7.0, np.float32)
    err = ctypes.c_double(7.0)
    pe = ctypes.cast(ctypes.byref(err), ctypes.c_void_p)
    dC = torch.full((h * d,), 7.0, dtype=torch.float32, device="cuda")
    dcnt = torch.full((m, h), 5, dtype=torch.int32, device="cuda")
    dX = torch.from_numpy(X).cuda()
    dcodes = torch.zeros((n, m), dtype=torch.int16, device="cuda")
    dCB = torch.full((n, d), 7.0, dtype=torch.float32, device="cuda")
    t = lambda a: a.data_ptr()      # noqa: E731
    pq = lambda **k: L.rq_train_pq_wide(*[k.get(a, v) for a, v in (("C", _p(C)), ("B", _p(B)), ("e", pe), ("X", _p(X)), ("n", n),  # noqa: E731
                                        ("d", d), ("m", m), ("h", h), ("niter", 2), ("seed", 1), ("base", 1))])
    rv = lambda **k: L.rq_train_rvq_wide(*[k.get(a, v) for a, v in (("C", _p(Cr)), ("B", _p(B)), ("e", pe), ("X", _p(X)), ("n", n),  # noqa: E731
                                         ("d", d), ("m", m), ("h", h), ("niter", 2), ("seed", 1), ("base", 1))])
    op = lambda **k: L.rq_train_opq_wide(*[k.get(a, v) for a, v in (("C", _p(C)), ("B", _p(B)), ("R", _p(R)), ("obj", _p(obj)),  # noqa: E731
                                         ("X", _p(X)), ("n", n), ("d", d), ("m", m), ("h", h), ("niter", 2), ("init", 0), ("seed", 1),
                                         ("R0", None), ("C0", None), ("base", 1))])
    for f in (pq, rv, op):
        assert f(h=32768) == RQ_EUNSUPPORTED and f(h=0) == RQ_EUNSUPPORTED
        assert f(base=2) == RQ_EINVAL and f(base=-1) == RQ_EINVAL
        assert f(niter=-1) == RQ_EINVAL
        assert f(n=h - 1) == RQ_EINVAL                                   # fewer rows than codewords
        assert f(C=None) == RQ_EINVAL and f(B=None) == RQ_EINVAL and f(X=None) == RQ_EINVAL
    assert pq(m=33) == RQ_EUNSUPPORTED and op(m=33) == RQ_EUNSUPPORTED and rv(m=65) == RQ_EUNSUPPORTED
    assert pq(d=1) == RQ_EINVAL and op(d=1) == RQ_EINVAL                  # d < m
    assert op(R=None) == RQ_EINVAL and op(init=2) == RQ_EINVAL
    upd = lambda **k: L.rq_dev_update_centers_wide(*[k.get(a, v) for a, v in (("C", t(dC)), ("cnt", t(dcnt)), ("X", t(dX)),  # noqa: E731
                                                   ("codes", t(dcodes)), ("n", n), ("d", d), ("m", m), ("h", h), ("s", None))])
    rec = lambda **k: L.rq_dev_reconstruct_wide(*[k.get(a, v) for a, v in (("CB", t(dCB)), ("codes", t(dcodes)), ("C", t(dC)),  # noqa: E731
                                                ("n", n), ("d", d), ("m", m), ("h", h), ("s", None))])
    for f in (upd, rec):
        assert f(h=32768) == RQ_EUNSUPPORTED and f(h=0) == RQ_EUNSUPPORTED and f(m=33) == RQ_EUNSUPPORTED
        assert f(d=1) == RQ_EINVAL and f(codes=None) == RQ_EINVAL and f(C=None) == RQ_EINVAL
        assert f(n=0) == 0
    torch.cuda.synchronize()
    assert (C == 7.0).all() and (Cr == 7.0).all() and (B == -3).all() and (R == 7.0).all() and (obj == 7.0).all() and err.value == 7.0
    assert bool((dC == 7.0).all()) and bool((dcnt == 5).all()) and bool((dCB == 7.0).all())
    # the byte entry points keep refusing h = 257
    assert L.rq_train_pq(_p(C), _p(B), pe, _p(X), n, d, m, 257, 2, 1) != 0
    assert L.rq_train_rvq(_p(Cr), _p(B), pe, _p(X), n, d, m, 257, 2, 1) != 0
    assert L.rq_train_opq(_p(C), _p(B), _p(R), _p(obj), _p(X), n, d, m, 257, 2, 0, 1, None, None) != 0
    assert (C == 7.0).all() and (B == -3).all()


def test_experiment_pq_and_opq_end_to_end_at_300_codewords(rq, oracle):
    """experiment_pq / experiment_opq at h > 256: train -> encode -> the scan over 16-bit codes -> recall; the search leg must
    equal the scan of the same (zero-based) codes through linscan_pq_u16 / linscan_opq_u16."""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.experiments import experiment_opq, experiment_pq, experiment_pq_query_base
    d, m, h, knn = 16, 2, 300, 20
    Xb = synth.deep_like(6000, d, seed=1)
    Xt, Xq = Xb[:3000], synth.deep_like(32, d, seed=2)
    dd = ((Xq.astype(np.float64)[:, None, :] - Xb.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    gt = (dd.argmin(1) + 1).astype(np.uint32)
    C, B, e, B_base, recall = experiment_pq(Xt, Xb, Xq, gt, m, h, niter=4, knn=knn)
    assert B_base.dtype == np.int16 and B_base.min() >= 1 and B_base.max() > 256
    assert np.array_equal(B_base, rq.quantize_pq(Xb, C))
    _, idx = rq.linscan_pq_u16((B_base - 1).astype(np.uint16), Xq, C, knn)
    assert np.allclose(recall, rq.eval_recall(gt, idx, knn)) and recall[-1] > 0.5 and (np.diff(recall) >= 0).all()
    C, B, R, obj, B_base, recall = experiment_opq(Xt, Xb, Xq, gt, m, h, "natural", niter=3, knn=knn)
    _, idx = rq.linscan_opq_u16((B_base - 1).astype(np.uint16), Xq, C, R, knn)
    assert np.allclose(recall, rq.eval_recall(gt, idx, knn)) and recall[-1] > 0.5
    gt_t = (((Xq.astype(np.float64)[:, None, :] - Xt.astype(np.float64)[None, :, :]) ** 2).sum(-1).argmin(1) + 1).astype(np.uint32)
    C, B, e, recall = experiment_pq_query_base(Xt, Xq, gt_t, m, h, niter=3, knn=knn)
    assert recall[-1] > 0.5
