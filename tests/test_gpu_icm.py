"""GPU: LSQ encoding (rq_encode_icm / encoding_icm / encode_icm_cuda) bit for bit against the CPU restatement
tests/icm_oracle.py."""
import numpy as np
import pytest

import icm_oracle as io

pytestmark = pytest.mark.gpu


def _data(n, d, m, h, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    B0 = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    return X, C, B0


def _gpu(X, C, B0, ilsiter, icmiter, npert, randord, seed=0, t0=0, nsplits=1):
    from rayuela_jl_amd.LSQ import encode_icm_u8
    return encode_icm_u8(X, B0, C, ilsiter, icmiter, npert, randord, seed=seed, t0=t0, nsplits=nsplits, with_cost=True)


def _assert_same(got, want):
    (b1, c1), (b0, c0) = got, want
    bad = np.flatnonzero((b1 != b0).any(axis=1))
    assert bad.size == 0, "%d rows differ, first %d: gpu %s oracle %s" % (bad.size, bad[0], b1[bad[0]], b0[bad[0]])
    assert np.array_equal(c1.view(np.uint32), c0.view(np.uint32)), "per-row costs differ"


# d = 960 with m > 4 is left to the next test: the oracle's binaries there cost minutes of CPU time
@pytest.mark.parametrize("m,h,d", [(m, h, d) for m in (1, 4, 8, 16) for h in (256, 64) for d in (32, 128, 960)
                                   if d < 960 or m <= 4])
def test_shapes_bit_exact(rq, oracle, m, h, d):
    n = 200 if d < 960 else 96
    X, C, B0 = _data(n, d, m, h, seed=m * 1000 + h + d)
    args = (2, 2, min(2, m), (m + d) % 2 == 0)
    _assert_same(_gpu(X, C, B0, *args, seed=5), io.ils(oracle, X, C, B0, *args, seed=5))


def test_shapes_cover_d960_m16_against_itself(rq):
    """m = 16 at d = 960 (the oracle's binaries are too slow there): in-range codes, costs never above the start."""
    X, C, B0 = _data(64, 960, 16, 256, seed=11)
    b, c = _gpu(X, C, B0, 2, 2, 4, True, seed=1)
    _, c0 = _gpu(X, C, B0, 0, 0, 0, False)
    assert b.max() < 256 and (c <= c0).all() and (c < c0).any()


@pytest.mark.parametrize("icmiter", [0, 1, 4])
@pytest.mark.parametrize("npert", [0, 1, 8])
@pytest.mark.parametrize("randord", [False, True])
def test_iteration_knobs_bit_exact(rq, oracle, icmiter, npert, randord):
    X, C, B0 = _data(256, 32, 8, 256, seed=3)
    args = (3, icmiter, npert, randord)
    _assert_same(_gpu(X, C, B0, *args, seed=9, t0=4), io.ils(oracle, X, C, B0, *args, seed=9, t0=4))


def test_odd_shapes_bit_exact(rq, oracle):
    from rayuela_jl_amd.LSQ import last_timing
    X, C, B0 = _data(77, 37, 5, 100, seed=4)
    got = _gpu(X, C, B0, 3, 2, 3, True, seed=2)
    t = last_timing()                                  # the host entry's clocks (rq_last_icm_timing): the unaries within the call
    assert 0 <= t["unary_ms"] <= t["total_ms"] and t["total_ms"] > 0, t
    _assert_same(got, io.ils(oracle, X, C, B0, 3, 2, 3, True, seed=2))


def test_nsplits_do_not_change_results(rq):
    X, C, B0 = _data(1001, 64, 8, 256, seed=6)
    ref = _gpu(X, C, B0, 3, 2, 2, True, seed=3, nsplits=1)
    for ns in (3, 7):
        _assert_same(_gpu(X, C, B0, 3, 2, 2, True, seed=3, nsplits=ns), ref)


def test_checkpoints_equal_separate_runs(rq):
    X, C, B0 = _data(300, 32, 8, 256, seed=7)
    Bs, objs = rq.encode_icm_cuda(X, B0.astype(np.int16) + 1, list(C), [2, 4, 8], 2, 2, True, nsplits=2, seed=4)
    cur, done = B0, 0
    for B, stop, obj in zip(Bs, [2, 4, 8], objs):
        cur, cost = _gpu(X, C, cur, stop - done, 2, 2, True, seed=4, t0=done)
        done = stop
        assert np.array_equal(B, cur.astype(np.int16) + 1)
        assert obj == np.float32(np.mean(cost, dtype=np.float64))
    one = _gpu(X, C, B0, 8, 2, 2, True, seed=4)
    assert np.array_equal(one[0], cur)


def test_objs_against_the_oracle(rq, oracle):
    X, C, B0 = _data(300, 32, 4, 256, seed=8)
    Bs, objs = rq.encode_icm_cuda(X, B0.astype(np.int16) + 1, list(C), [1, 3], 2, 1, False, seed=2)
    for it, B, obj in zip([1, 3], Bs, objs):
        b0, c0 = io.ils(oracle, X, C, B0, it, 2, 1, False, seed=2)
        assert np.array_equal(B, b0.astype(np.int16) + 1)
        want = np.mean(c0, dtype=np.float64)
        assert abs(obj - want) <= 1e-6 * abs(want)
        assert abs(rq.qerror(X, B, list(C)) - want) <= 1e-6 * abs(want)
        assert np.array_equal(rq.veccost(X, B, list(C)).view(np.uint32), io.veccost(X, b0, C).view(np.uint32))


def test_host_entry_equals_device_entry_and_aliasing(rq):
    import torch
    from rayuela_jl_amd import _lib
    X, C, B0 = _data(500, 64, 8, 64, seed=9)
    want = _gpu(X, C, B0, 2, 2, 2, True, seed=1)
    dev = torch.device("cuda:0")
    tX, tC = torch.from_numpy(X).to(dev), torch.from_numpy(C).to(dev)
    tB = torch.from_numpy(B0).to(dev)
    tout = torch.empty_like(tB)
    tcost = torch.empty(500, dtype=torch.float32, device=dev)
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(L.rq_dev_encode_icm(tout.data_ptr(), tB.data_ptr(), tcost.data_ptr(), tX.data_ptr(), tC.data_ptr(),
                                   500, 64, 8, 64, 2, 2, 2, 1, 1, 0, 1, s))
    torch.cuda.synchronize()
    _assert_same((tout.cpu().numpy(), tcost.cpu().numpy()), want)
    assert np.array_equal(tB.cpu().numpy(), B0)
    # in place on the device (codes_out == codes_in), no cost output
    _lib.check(L.rq_dev_encode_icm(tB.data_ptr(), tB.data_ptr(), None, tX.data_ptr(), tC.data_ptr(),
                                   500, 64, 8, 64, 2, 2, 2, 1, 1, 0, 3, s))
    torch.cuda.synchronize()
    assert np.array_equal(tB.cpu().numpy(), want[0])
    # in place through the host entry
    Bh = B0.copy()
    _lib.check(L.rq_encode_icm(Bh.ctypes.data, Bh.ctypes.data, None, X.ctypes.data, C.ctypes.data,
                               500, 64, 8, 64, 2, 2, 2, 1, 1, 0, 1))
    assert np.array_equal(Bh, want[0])
    # a code >= h is refused by the device entry before any encode work
    tB[3, 2] = 64
    with pytest.raises(rq.RayuelaHipError):
        _lib.check(L.rq_dev_encode_icm(tout.data_ptr(), tB.data_ptr(), None, tX.data_ptr(), tC.data_ptr(),
                                       500, 64, 8, 64, 1, 1, 1, 1, 1, 0, 1, s))


def test_encoding_icm_updates_oldB_and_encode_icm_cuda_leaves_B(rq):
    X, C, B0 = _data(200, 32, 8, 256, seed=10)
    oldB = B0.astype(np.int16) + 1
    B = rq.encoding_icm(X, oldB, list(C), 3, 2, True, 2, seed=6)
    assert B.dtype == np.int16 and B.min() >= 1 and B.max() <= 256
    assert np.array_equal(oldB, B)
    assert np.array_equal(B, _gpu(X, C, B0, 3, 2, 2, True, seed=6)[0].astype(np.int16) + 1)   # Int16 one-based
    Bin = B0.astype(np.int16) + 1
    keep = Bin.copy()
    Bs, _ = rq.encode_icm_cuda(X, Bin, list(C), [3], 2, 2, True, seed=6)
    assert np.array_equal(Bin, keep) and np.array_equal(Bs[0], B)


def test_sift1m_shape_and_end_to_end(rq, oracle):
    """train_rvq codebooks, quantize_rvq start codes, then encoding_icm on 1e6 x 128 (m = 8, ilsiter = 8): every row's
    cost is at most its RVQ cost, 4096 sampled rows equal the oracle run on just those rows, and linscan_lsq on the new
    codes equals the LSQ scan oracle."""
    import rayuela_jl_amd.synth as synth
    n, d, m, h = 1_000_000, 128, 8, 256
    X = synth.sift_like(n, d, seed=21)
    C, _, _ = rq.train_rvq(X[:20000], m, h, niter=4)
    Brvq, _ = rq.quantize_rvq(X, C)
    c_rvq = rq.veccost(X, Brvq, C)
    oldB = Brvq.copy()
    B = rq.encoding_icm(X, oldB, C, 8, 4, True, 4, seed=13)
    c_new = rq.veccost(X, B, C)
    assert (c_new <= c_rvq).all()
    assert (c_new < c_rvq).mean() > 0.5
    rows = np.sort(np.random.default_rng(1).choice(n, 4096, replace=False))
    Cs = np.stack(C)
    b0, _ = io.ils(oracle, X[rows], Cs, (Brvq[rows] - 1).astype(np.uint8), 8, 4, 4, True, seed=13, rows=rows)
    assert np.array_equal(B[rows], b0.astype(np.int16) + 1)
    # the LSQ scan on the new codes
    codes = (B - 1).astype(np.uint8)
    nrm = np.sum(Cs[np.arange(m)[None, :], codes.astype(np.int64)].sum(axis=1) ** 2, axis=1).astype(np.float32)
    Q = synth.sift_like(8, d, seed=22)
    d1, i1 = rq.linscan_lsq(codes, Q, C, nrm, np.eye(d, dtype=np.float32), 100)
    d0, i0 = oracle.linscan_lsq(codes, Cs.reshape(m * h, d), Q, nrm, 100)
    assert np.array_equal(i1.view(np.int32), i0)
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32))
