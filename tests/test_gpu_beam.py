"""GPU: beam-search residual encoding (rq_beam.hip; src/CompetitiveQ.jl:75-135) through the C ABI and its mirrors: codes,
residual and cost bit for bit against the numpy restatement of tests/beam_oracle.py, H = 1 against quantize_rvq, independence
of chunking / pointer form / alignment / stream, the argument checks, the mirrors, the downstream search leg and non-finite
inputs."""
import ctypes

import numpy as np
import pytest

import beam_oracle as bo
import beam_stream_cases as bsc
import stream_cases as sc

pytestmark = pytest.mark.gpu

RQ_EINVAL = -1
PARITY = [(s, H) for s in bo.GPU_SHAPES + ["ties"] for H in bo.BEAMS if H <= (bo.TIE_SHAPE[3] if s == "ties" else s[3])]


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    codes, cost, Xr = got
    assert np.array_equal(codes, want[0]), "rows differ: %d of %d" % (int((codes != want[0]).any(axis=1).sum()), len(codes))
    assert np.array_equal(_bits(Xr), _bits(want[1])) and np.array_equal(_bits(cost), _bits(want[2]))


@pytest.fixture
def side(rq):
    """One side stream per test; its scratch is given back afterwards (a device keeps scratch for at most 8 streams)."""
    import torch
    st = torch.cuda.Stream()
    yield st
    torch.cuda.synchronize()
    assert _L().rq_release_workspaces() == 0


def _dev_call(X, C, H, st, nsplits=1, want=(True, True)):
    """rq_dev_encode_rvq_beam on torch tensors X, C on stream st; sentinel-filled outputs with one spare row -> (codes, cost, Xr)."""
    import torch
    n, d = X.shape
    m, h, _ = C.shape
    codes = torch.full((n + 1, m), sc.SENTINEL, dtype=torch.uint8, device="cuda")
    Xr = torch.full((n + 1, d), -7.0, dtype=torch.float32, device="cuda")
    cost = torch.full((n + 1,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = _L().rq_dev_encode_rvq_beam(codes.data_ptr(), Xr.data_ptr() if want[1] else None, cost.data_ptr() if want[0] else None,
                                     X.data_ptr(), C.data_ptr(), n, d, m, h, H, nsplits, st.cuda_stream)
    assert rc == 0, _L().rq_last_error()
    st.synchronize()
    return codes.cpu().numpy(), cost.cpu().numpy(), Xr.cpu().numpy()


# ---- 1. bit parity with the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,H", PARITY, ids=lambda v: str(v).replace(" ", ""))
def test_codes_residual_and_cost_equal_the_restatement(rq, shape, H):
    X, C, codes, Xr, cost = bo.expected(shape, H)
    _same(rq.quantize_competitiveq_u8(X, list(C), H, with_extras=True), (codes, Xr, cost))


@pytest.mark.parametrize("shape", bo.GPU_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_beam_of_one_is_quantize_rvq(rq, shape):
    X, C = bo.data(*shape)
    c0, _, r0 = rq.quantize_rvq_u8(X, list(C), with_extras=True)
    c1, _, r1 = rq.quantize_competitiveq_u8(X, list(C), 1, with_extras=True)
    assert np.array_equal(c0, c1) and np.array_equal(_bits(r0), _bits(r1))


# ---- 2. chunking, pointer form, alignment, stream -----------------------------------------------------------------------------
@pytest.mark.parametrize("H", [3, 16])
def test_nsplits_and_pointer_form_do_not_change_a_bit(rq, side, H):
    import torch
    shape = bo.GPU_SHAPES[0]
    X, C, codes, Xr, cost = bo.expected(shape, H)
    n = X.shape[0]
    tX, tC = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    for nsplits in (1, 3, 7):
        _same(rq.quantize_competitiveq_u8(X, list(C), H, nsplits=nsplits, with_extras=True), (codes, Xr, cost))
        c, co, r = _dev_call(tX, tC, H, side, nsplits)
        _same((c[:n], co[:n], r[:n]), (codes, Xr, cost))
        assert (c[n] == sc.SENTINEL).all() and co[n] == -7.0 and (r[n] == -7.0).all()       # nothing past row n - 1
        assert np.array_equal(_bits(tX.cpu().numpy()), _bits(X)), "X was overwritten"
    # only what was asked for is filled
    c, co, r = _dev_call(tX, tC, H, side, 3, want=(True, False))
    assert np.array_equal(c[:n], codes) and np.array_equal(_bits(co[:n]), _bits(cost)) and (r == -7.0).all()
    c, co, r = _dev_call(tX, tC, H, side, 3, want=(False, True))
    assert np.array_equal(c[:n], codes) and np.array_equal(_bits(r[:n]), _bits(Xr)) and (co == -7.0).all()
    c, co, r = _dev_call(tX, tC, H, side, 3, want=(False, False))
    assert np.array_equal(c[:n], codes) and (co == -7.0).all() and (r == -7.0).all()
    # the torch mirror
    from rayuela_jl_amd import device as rqd
    out, tcost, tXr = rqd.encode_rvq_beam(tX, tC, H, nsplits=3, want_extras=True)
    torch.cuda.synchronize()
    _same((out.cpu().numpy(), tcost.cpu().numpy(), tXr.cpu().numpy()), (codes, Xr, cost))
    assert rqd.encode_rvq_beam(tX, tC, H).dtype == torch.uint8


@pytest.mark.parametrize("name", sorted(bsc.BEAM_CASES))
def test_device_form_is_ordered_on_a_side_stream(rq, side, name):
    """The harness of tests/test_gpu_streams.py: the call on a side stream behind that file's delay (2e7 cycles), inputs holding
    poison until the stream fills them, outputs consumed on that stream only."""
    import torch
    case = sc.get(name)
    case.check(sc.run_on_side_stream(case, side, 0))                 # grows this stream's scratch outside the delayed run
    case.check(sc.run_on_side_stream(case, side, 20_000_000))


@pytest.mark.parametrize("which", ["X", "C", "both"])
def test_unaligned_device_pointers_give_the_same_bits(rq, side, which):
    import torch
    shape, H = bo.GPU_SHAPES[0], 3
    X, C, codes, Xr, cost = bo.expected(shape, H)
    n = X.shape[0]

    def place(a, shift):
        buf = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
        view = buf[shift:shift + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == (4 * shift) % 16
        return view

    tX = place(X, 1 if which in ("X", "both") else 0)
    tC = place(C, 1 if which in ("C", "both") else 0)
    c, co, r = _dev_call(tX, tC, H, side, 1)
    _same((c[:n], co[:n], r[:n]), (codes, Xr, cost))


# ---- 3. argument checks ---------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_alone(rq):
    import torch
    L = _L()
    n, d, m, h = 40, 16, 3, 16
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = rng.standard_normal((65, 257, d)).astype(np.float32)         # big enough for every (m, h) tried
    bad = [dict(H=0), dict(H=33, h=64), dict(H=17), dict(m=65), dict(h=257), dict(d=0)]
    for kw in bad:
        a = dict(n=n, d=d, m=m, h=h, H=2, nsplits=1)
        a.update(kw)
        codes = np.full((n, 65), sc.SENTINEL, dtype=np.uint8)
        codes16 = np.full((n, 65), -3, dtype=np.int16)
        cost = np.full((n,), -7.0, dtype=np.float32)
        Xr = np.full((n, d), -7.0, dtype=np.float32)
        for fn, out in ((L.rq_encode_rvq_beam, codes), (L.rq_encode_rvq_beam_i16, codes16)):
            rc = fn(out.ctypes.data, X.ctypes.data, C.ctypes.data, a["n"], a["d"], a["m"], a["h"], a["H"], a["nsplits"],
                    cost.ctypes.data, Xr.ctypes.data)
            assert rc == RQ_EINVAL and L.rq_last_error(), (kw, rc)
        assert (codes == sc.SENTINEL).all() and (codes16 == -3).all() and (cost == -7.0).all() and (Xr == -7.0).all(), kw
        tX, tC = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
        tcodes = torch.full((n, 65), sc.SENTINEL, dtype=torch.uint8, device="cuda")
        tcost = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        tXr = torch.full((n, d), -7.0, dtype=torch.float32, device="cuda")
        rc = L.rq_dev_encode_rvq_beam(tcodes.data_ptr(), tXr.data_ptr(), tcost.data_ptr(), tX.data_ptr(), tC.data_ptr(), a["n"],
                                      a["d"], a["m"], a["h"], a["H"], a["nsplits"], None)
        assert rc == RQ_EINVAL and L.rq_last_error(), (kw, rc)
        torch.cuda.synchronize()
        assert bool((tcodes == sc.SENTINEL).all()) and bool((tcost == -7.0).all()) and bool((tXr == -7.0).all()), kw
    # no rows: fine, and nothing is written
    codes = np.full((4, m), sc.SENTINEL, dtype=np.uint8)
    assert L.rq_encode_rvq_beam(codes.ctypes.data, X.ctypes.data, C.ctypes.data, 0, d, m, h, 2, 1, None, None) == 0
    assert L.rq_dev_encode_rvq_beam(None, None, None, None, tC.data_ptr(), 0, d, m, h, 2, 1, None) == 0
    assert (codes == sc.SENTINEL).all()
    t = (ctypes.c_double * 3)()
    assert L.rq_last_beam_timing(ctypes.cast(t, ctypes.c_void_p), 3) == 0 and list(t) == [0.0, 0.0, 0.0]
    with pytest.raises(rq.RayuelaHipError):
        rq.quantize_competitiveq(X, [C[i, :h] for i in range(m)], 17)
    with pytest.raises(TypeError):
        rq.quantize_competitiveq(X.astype(np.float64), [C[i, :h] for i in range(m)], 2)


# ---- 4. mirrors -------------------------------------------------------------------------------------------------------------------
def test_host_mirrors(rq):
    shape, H = bo.GPU_SHAPES[1], 3
    X, C, codes, Xr, cost = bo.expected(shape, H)
    n, d = X.shape
    m, h, _ = C.shape
    B = rq.quantize_competitiveq(X, list(C), H)
    assert B.dtype == np.int16 and B.shape == (n, m) and np.array_equal(B, codes.astype(np.int16) + 1)   # one-based, quantize_rvq's layout
    u8 = rq.quantize_competitiveq_u8(X, list(C), H)
    assert u8.dtype == np.uint8 and np.array_equal(u8, codes)
    for row in (0, 417, n - 1):
        b, r = rq.CompetitiveQ.encode(X[row], list(C), None, m, h, d, H)
        assert b.dtype == np.int16 and b.shape == (m,) and np.array_equal(b, B[row])
        assert r.shape == (d,) and np.array_equal(_bits(r), _bits(Xr[row]))
    t = rq.last_beam_timing()
    assert sorted(t) == ["expand_ms", "other_ms", "stage_ms"] and t["stage_ms"] > 0 and t["expand_ms"] > 0
    assert not hasattr(rq, "train_competitiveq") and not hasattr(rq.CompetitiveQ, "train_competitiveq")


# ---- 5. the codes feed the search leg unchanged, and are better codes ------------------------------------------------------------
def test_beam_codes_search_and_beat_the_greedy_codes(rq):
    import rayuela_jl_amd.synth as synth
    d, m, h, knn = 32, 4, 256, 50                                     # test_experiment_rvq_end_to_end's shape
    Xb = synth.sift_like(20_000, d, seed=5)
    Xq = synth.sift_like(64, d, seed=6)
    C, _, _ = rq.train_rvq(Xb[:8000], m, h, niter=6, seed=0)
    Bg, _ = rq.quantize_rvq(Xb, C)
    Bb = rq.quantize_competitiveq(Xb, C, 16)
    eg, eb = rq.qerror(Xb, Bg, C), rq.qerror(Xb, Bb, C)
    print("qerror: greedy %.6g, beam of 16 %.6g" % (eg, eb))
    assert eb < eg
    _, cbnorms = rq.get_norms_codebook(Bb, C)
    dists, idx = rq.linscan_lsq_cbnorms(Bb, Xq, C, cbnorms, np.eye(d, dtype=np.float32), knn)
    assert idx.shape == (64, knn) and idx.min() >= 1 and idx.max() <= 20_000 and (np.diff(dists, axis=1) >= 0).all()
    dd = ((Xq.astype(np.float64)[:, None, :] - Xb.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    gt = (dd.argmin(1) + 1).astype(np.uint32)
    assert rq.eval_recall(gt, idx, knn)[-1] > 0.5


# ---- 6. non-finite input --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 3, 16])
def test_non_finite_inputs_return_codes_in_range(rq, H):
    shape = bo.GPU_SHAPES[0]
    X, C = bo.data(*shape)
    X, C = X.copy(), C.copy()
    h = C.shape[1]
    X[5, 3], X[70, 0], X[71, 9] = np.nan, np.inf, -np.inf
    C[1, 7, 2], C[2, 60, 5] = np.nan, np.inf
    codes, cost, Xr = rq.quantize_competitiveq_u8(X, list(C), H, with_extras=True)
    assert codes.shape == (shape[0], shape[2]) and int(codes.max()) < h
    assert not np.isnan(cost).any() and (cost >= 0).all()                              # the clamp leaves no NaN in the keys
