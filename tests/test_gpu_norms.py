"""GPU: the database norms of additive-quantizer search (rq_norms.hip): rq_aq_norms / rq_quantize_norms / rq_get_norms_codebook /
rq_lsq_prepare_cbnorms and their device-pointer forms against the numpy restatement of tests/norms_oracle.py bit for bit,
against veccost, rq_train_pq and rq_lsq_prepare, their argument checks, and the LSQ drivers end to end."""
import ctypes

import numpy as np
import pytest

import norms_oracle as no
import norms_stream_cases as nsc
import stream_cases as sc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _host_norms(codes, C):
    n, m = codes.shape
    _, h, d = C.shape
    out = np.full(n, -1.0, dtype=np.float32)
    assert _L().rq_aq_norms(out.ctypes.data, codes.ctypes.data, C.ctypes.data, n, d, m, h) == 0, _L().rq_last_error()
    return out


@pytest.fixture(scope="module")
def restated():
    """The restatement of every norms shape, computed once: (n, d, m, h) -> (codes, C, norms)."""
    out = {}
    for s in no.NORM_SHAPES:
        codes, C = no.norm_case(*s)
        out[s] = (codes, C, no.aq_norms(codes, C))
    return out


# ---- 1. norms bit for bit against the restatement: host pointers, and device pointers on a stream of their own ---------------
@pytest.mark.parametrize("n,d,m,h", no.NORM_SHAPES)
def test_norms_equal_the_restatement(rq, restated, n, d, m, h):
    import torch
    codes, C, want = restated[(n, d, m, h)]
    if n * m == 1:                                           # one cell holds h - 1: entry 0 in a call of its own
        zero = np.zeros((1, 1), dtype=np.uint8)
        assert np.array_equal(_bits(_host_norms(zero, C)), _bits(no.aq_norms(zero, C)))
    else:
        assert (codes == 0).any()
    assert (codes == h - 1).any()
    assert np.array_equal(_bits(_host_norms(codes, C)), _bits(want))
    dev = torch.device("cuda:0")
    tc, tC = torch.from_numpy(codes).to(dev), torch.from_numpy(C).to(dev)
    out = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    assert _L().rq_dev_aq_norms(out.data_ptr(), tc.data_ptr(), tC.data_ptr(), n, d, m, h, st.cuda_stream) == 0
    st.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("name", sorted(nsc.NORMS_CASES))
def test_device_forms_are_ordered_on_a_side_stream(rq, name):
    """The harness of tests/test_gpu_streams.py: the call on a side stream behind that file's delay (2e7 cycles, 8.4 ms), inputs
    holding poison until the stream fills them, outputs consumed on that stream only."""
    import torch
    case = sc.get(name)
    stream = torch.cuda.Stream()
    case.check(sc.run_on_side_stream(case, stream, 0))               # grows this stream's scratch outside the delayed run
    case.check(sc.run_on_side_stream(case, stream, 20_000_000))


# ---- 2. the cross-check against shipped code: veccost of an all-zero X -------------------------------------------------------
@pytest.mark.parametrize("n,d,m,h", [s for s in no.NORM_SHAPES if s[2] <= 16])
def test_norms_equal_veccost_of_zero(rq, restated, n, d, m, h):
    codes, C, _ = restated[(n, d, m, h)]
    cost = rq.veccost(np.zeros((n, d), np.float32), codes.astype(np.int16) + 1, C)
    assert np.array_equal(_bits(_host_norms(codes, C)), _bits(cost))


# ---- 3. integer-valued codebooks: the f64 value exactly ----------------------------------------------------------------------
@pytest.mark.parametrize("n,d,m,h", [s for s in no.NORM_SHAPES if s[2] <= 8 and s[1] <= 128])
def test_integer_codebooks_give_the_f64_value(rq, n, d, m, h):
    codes, C = no.norm_case(n, d, m, h, integer=True)
    assert np.array_equal(_host_norms(codes, C).astype(np.float64), no.norms_f64(codes, C))
    assert np.array_equal(rq.aq_norms(codes.astype(np.int16) + 1, list(C)).astype(np.float64), no.norms_f64(codes, C))


# ---- 4. quantise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(no.quant_cases()))
def test_quantize_equals_the_restatement(rq, name):
    """The device-pointer form on given norms, every n of QUANT_NS: codes bit for bit, dbnorms_out = cbnorms[code]."""
    import torch
    norms, cb = no.quant_cases()[name]
    want = no.quantize(norms, cb)
    dev = torch.device("cuda:0")
    tn, tcb = torch.from_numpy(norms).to(dev), torch.from_numpy(cb).to(dev)
    st = torch.cuda.Stream(device=dev)
    for n in no.QUANT_NS:
        oc = torch.full((max(n, 1),), 255, dtype=torch.uint8, device=dev)
        od = torch.full((max(n, 1),), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        assert _L().rq_dev_quantize_norms(oc.data_ptr(), od.data_ptr(), tn.data_ptr(), tcb.data_ptr(), n, len(cb),
                                          st.cuda_stream) == 0
        st.synchronize()
        assert np.array_equal(oc.cpu().numpy()[:n], want[:n]), (name, n)
        assert np.array_equal(_bits(od.cpu().numpy()[:n]), _bits(cb[want[:n]])), (name, n)
        if n == 0:
            assert oc.item() == 255 and od.item() == -1.0
        assert _L().rq_dev_quantize_norms(oc.data_ptr(), None, tn.data_ptr(), tcb.data_ptr(), n, len(cb), st.cuda_stream) == 0
        st.synchronize()
        assert np.array_equal(oc.cpu().numpy()[:n], want[:n])


@pytest.mark.parametrize("n", no.QUANT_NS)
def test_host_quantize_from_codes(rq, n):
    """rq_quantize_norms on codes and codebooks: norms_out equals rq_aq_norms, the codes the restatement's on those norms, for
    a sorted, an unsorted, a one-entry and a 256-entry norms codebook, one of them far from every norm."""
    d, m, h = 96, 16, 256
    codes, C = no.norm_case(1007, d, m, h)
    codes = np.ascontiguousarray(codes[:n])
    norms = no.aq_norms(codes, C)
    rng = np.random.default_rng(5)
    lo, hi = (norms.min(), norms.max()) if n else (0.0, 1.0)
    for cb in (np.linspace(lo, hi, 16), rng.permutation(np.linspace(lo, hi, 255)), np.array([7.0]),
               rng.standard_normal(256) * 20 + float(np.mean([lo, hi])), np.linspace(hi + 10, hi + 20, 9)):
        cb = np.ascontiguousarray(cb, dtype=np.float32)
        nc = np.full(max(n, 1), 255, dtype=np.uint8)
        no_ = np.full(max(n, 1), -1.0, dtype=np.float32)
        assert _L().rq_quantize_norms(nc.ctypes.data, no_.ctypes.data, codes.ctypes.data, C.ctypes.data, cb.ctypes.data, n, d, m,
                                      h, len(cb)) == 0
        assert np.array_equal(_bits(no_[:n]), _bits(norms)) and np.array_equal(nc[:n], no.quantize(norms, cb))
        if n:
            assert np.array_equal(_bits(no_), _bits(_host_norms(codes, C)))
            B1, nx = rq.quantize_norms(codes.astype(np.int16) + 1, list(C), cb)
            assert B1.dtype == np.int16 and np.array_equal(B1 - 1, nc) and np.array_equal(_bits(nx), _bits(norms))
        assert _L().rq_quantize_norms(nc.ctypes.data, None, codes.ctypes.data, C.ctypes.data, cb.ctypes.data, n, d, m, h,
                                      len(cb)) == 0


# ---- 5. the norms codebook is rq_train_pq(d = 1, m = 1) on resident norms ----------------------------------------------------
@pytest.mark.parametrize("n,hn", [(3000, 16), (3000, 256), (256, 256)])
def test_norms_codebook_equals_train_pq_on_the_norms(rq, n, hn):
    d, m, h, niter, seed = 32, 4, 256, 12, 3
    codes, C = no.norm_case(n, d, m, h)
    norms = _host_norms(codes, C)
    cb0 = np.empty(hn, dtype=np.float32)
    B1 = np.empty((n, 1), dtype=np.int16)
    err = ctypes.c_double(0)
    L = _L()
    assert L.rq_train_pq(cb0.ctypes.data, B1.ctypes.data, ctypes.cast(ctypes.byref(err), ctypes.c_void_p), norms.ctypes.data, n,
                         1, 1, hn, niter, seed) == 0, L.rq_last_error()
    nc = np.full(n, 255, dtype=np.uint8)
    cb = np.full(hn, -1.0, dtype=np.float32)
    nout = np.full(n, -1.0, dtype=np.float32)
    assert L.rq_get_norms_codebook(nc.ctypes.data, cb.ctypes.data, nout.ctypes.data, codes.ctypes.data, C.ctypes.data, n, d, m, h,
                                   hn, niter, seed) == 0, L.rq_last_error()
    assert np.array_equal(_bits(cb), _bits(cb0)) and np.array_equal(nc.astype(np.int16) + 1, B1[:, 0])
    assert np.array_equal(_bits(nout), _bits(norms))
    if hn == h:                                              # the mirror clusters with h centres
        B1m, cbm = rq.get_norms_codebook(codes.astype(np.int16) + 1, list(C), niter, seed)
        assert B1m.dtype == np.int64 and np.array_equal(B1m, B1[:, 0]) and np.array_equal(_bits(cbm), _bits(cb0))


# ---- 6. search from a norms codebook -----------------------------------------------------------------------------------------
def test_prepare_cbnorms_equals_prepare_with_host_norms(rq):
    import rayuela_jl_amd.synth as synth
    n, d, m, nq, k = 4096, 32, 4, 16, 50
    codes, Cs = no.norm_case(n, d, m, 256)
    C = list(Cs)
    norms = no.aq_norms(codes, Cs)
    rng = np.random.default_rng(9)
    cbn = rng.permutation(np.quantile(norms, np.linspace(0, 1, 256))).astype(np.float32)
    dbn = cbn[no.quantize(norms, cbn)]
    q = rng.standard_normal((nq, d)).astype(np.float32)
    R = synth.rotation(d, seed=5)
    with rq.LsqIndex(codes, C, dbn) as ref, rq.LsqIndex.from_cbnorms(codes, C, cbn) as ix:
        for rot in (None, R):
            d0, i0 = ref.search(q, rot, k)
            d1, i1 = ix.search(q, rot, k)
            assert np.array_equal(i1, i0) and np.array_equal(_bits(d1), _bits(d0)), rot is not None
    d2, i2 = rq.linscan_lsq_cbnorms(codes, q, C, cbn, R, k)
    assert np.array_equal(i2, i0) and np.array_equal(_bits(d2), _bits(d0))


# ---- 7. argument errors: a status, a message, outputs as they were -----------------------------------------------------------
def test_argument_errors_leave_the_outputs_alone(rq):
    L = _L()
    n, d, m, h, hn = 300, 8, 3, 16, 16
    codes, C = no.norm_case(n, d, m, h)
    bad = codes.copy()
    bad[217, 1] = h
    cbn = np.linspace(0, 40, 256).astype(np.float32)
    norms = np.full(n, -1.0, dtype=np.float32)
    nc = np.full(n, 255, dtype=np.uint8)
    cbo = np.full(256, -1.0, dtype=np.float32)
    P = lambda a: a.ctypes.data      # noqa: E731

    def failed(status):
        return status != 0 and len(L.rq_last_error()) > 0

    def aq(c=codes, mm=m, hh=h, dd=d, nn=n, out=norms, cc=C):
        return L.rq_aq_norms(None if out is None else P(out), None if c is None else P(c), None if cc is None else P(cc), nn, dd,
                             mm, hh)

    def qn(c=codes, mm=m, hh=h, hh2=hn, nn=n, cb=cbn, out=nc):
        return L.rq_quantize_norms(None if out is None else P(out), P(norms), None if c is None else P(c), P(C),
                                   None if cb is None else P(cb), nn, d, mm, hh, hh2)

    def gc(c=codes, mm=m, hh=h, hh2=hn, nn=n, niter=3, out=cbo):
        return L.rq_get_norms_codebook(P(nc), None if out is None else P(out), P(norms), None if c is None else P(c), P(C), nn, d,
                                       mm, hh, hh2, niter, 0)

    assert failed(aq(c=bad)) and b"code" in L.rq_last_error()
    assert failed(qn(c=bad)) and b"code" in L.rq_last_error()
    assert failed(gc(c=bad)) and b"code" in L.rq_last_error()
    for f in (aq, qn, gc):
        assert failed(f(mm=0)) and failed(f(mm=65)) and failed(f(hh=1)) and failed(f(hh=257)) and failed(f(nn=-1))
        assert failed(f(c=None)) and failed(f(out=None))
    assert failed(aq(dd=0)) and failed(aq(cc=None))
    for f in (qn, gc):
        assert failed(f(hh2=0)) and failed(f(hh2=257))
    assert failed(qn(cb=None))
    assert failed(gc(nn=hn - 1)) and b"fewer" in L.rq_last_error() and failed(gc(niter=-1))
    assert (norms == -1.0).all() and (nc == 255).all() and (cbo == -1.0).all()
    # the device-pointer forms and the prepared search
    import torch
    dev = torch.device("cuda:0")
    tb, tC = torch.from_numpy(bad).to(dev), torch.from_numpy(C).to(dev)
    tn = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
    tnc = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    tcb = torch.from_numpy(cbn).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    assert failed(L.rq_dev_aq_norms(tn.data_ptr(), tb.data_ptr(), tC.data_ptr(), n, d, m, h, s)) and b"code" in L.rq_last_error()
    assert failed(L.rq_dev_aq_norms(tn.data_ptr(), tb.data_ptr(), tC.data_ptr(), n, d, 65, h, s))
    assert failed(L.rq_dev_aq_norms(None, tb.data_ptr(), tC.data_ptr(), n, d, m, h, s))
    for v in (0, 257):
        assert failed(L.rq_dev_quantize_norms(tnc.data_ptr(), tn.data_ptr(), tn.data_ptr(), tcb.data_ptr(), n, v, s))
    assert failed(L.rq_dev_quantize_norms(None, tn.data_ptr(), tn.data_ptr(), tcb.data_ptr(), n, 16, s))
    assert failed(L.rq_dev_quantize_norms(tnc.data_ptr(), tn.data_ptr(), tn.data_ptr(), None, n, 16, s))
    torch.cuda.synchronize()
    assert (tn == -1.0).all().item() and (tnc == 255).all().item()
    c256, C256 = no.norm_case(64, 8, 4, 256)
    for hn_bad in (0, 257):
        assert not L.rq_lsq_prepare_cbnorms(P(c256), P(C256), P(cbn), hn_bad, 64, 4, 256, 8) and len(L.rq_last_error()) > 0
    assert not L.rq_lsq_prepare_cbnorms(P(c256), P(C256), None, 16, 64, 4, 256, 8)
    assert not L.rq_lsq_prepare_cbnorms(P(c256), P(C256), P(cbn), 16, 64, 65, 256, 8)
    assert not L.rq_lsq_prepare_cbnorms(P(c256), P(C256), P(cbn), 16, 64, 4, 16, 8)
    # the mirrors check before the library is reached
    with pytest.raises(ValueError):
        rq.get_norms_codebook(bad.astype(np.int16) + 1, list(C))
    with pytest.raises(ValueError):
        rq.quantize_norms(codes.astype(np.int16), list(C), cbn)          # a zero: not one-based


# ---- 8. the drivers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    import rayuela_jl_amd.synth as synth
    d = 32
    Xb = synth.sift_like(20000, d, seed=5)
    Xt = Xb[:8000]
    Xq = synth.sift_like(64, d, seed=6)

    def nearest(base):
        dd = ((Xq.astype(np.float64)[:, None, :] - base.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        return (dd.argmin(1) + 1).astype(np.uint32)

    return Xt, Xb, Xq, nearest(Xb), nearest(Xt)


def test_experiment_lsq_cuda_end_to_end(rq, oracle, data):
    """experiment_lsq_cuda (src/LSQ_GPU.jl:322-368, :407-436): train_opq -> train_lsq_cuda -> norms codebook -> the base by
    encode_icm_cuda -> quantised norms -> linscan_lsq -> recall; the search leg must equal the oracle's scan with the
    restatement's quantised norms."""
    from rayuela_jl_amd import experiments as ex
    Xt, Xb, Xq, gt, _ = data
    d, m, h, knn = 32, 4, 256, 50
    C, B, R, train_error, B_base, recall = ex.experiment_lsq_cuda(Xt, Xb, Xq, gt, m, h, 1, 2, 4, True, 2, knn, seed=2,
                                                                  niter_init=2)
    assert len(C) == m and C[0].shape == (h, d) and B.shape == (8000, m) and B_base.shape == (20000, m) and R.shape == (d, d)
    assert B.dtype == np.int16 and B_base.dtype == np.int16 and train_error.shape == (1,) and train_error[0] > 0
    assert recall.shape == (knn,) and (np.diff(recall) >= 0).all() and recall[-1] > 0.5
    Cs = np.stack(C)
    codes0 = (B_base - 1).astype(np.uint8)
    _, norms_C = rq.get_norms_codebook(B, C, seed=2)
    dbn = norms_C[no.quantize(no.aq_norms(codes0, Cs), norms_C)]
    d0, i0 = oracle.linscan_lsq(codes0, Cs.reshape(m * h, d), Xq, dbn, knn)
    assert np.allclose(recall, oracle.eval_recall(gt, i0, knn))
    # the method with start codes, codebooks and rotation
    C2, B2, R2, e2, Bb2, rec2 = ex.experiment_lsq_cuda(Xt, B, C, R, Xb, Xq, gt, m, h, 1, 2, 4, True, 2, knn, seed=2)
    assert B2.shape == B.shape and Bb2.shape == B_base.shape and rec2.shape == (knn,) and (np.diff(rec2) >= 0).all()
    assert R2 is R and e2.shape == (1,)


def test_experiment_lsq_cuda_query_base(rq, oracle, data):
    from rayuela_jl_amd import experiments as ex
    Xt, _, Xq, _, gt_t = data
    d, m, h, knn = 32, 4, 256, 50
    (C, B, R, train_error, recall), opq_error = ex.experiment_lsq_cuda_query_base(Xt, Xq, gt_t, m, h, 1, 2, 4, True, 2, "natural",
                                                                                  2, 2, knn, seed=2)
    assert len(C) == m and C[0].shape == (h, d) and B.shape == (8000, m) and B.dtype == np.int16 and R.shape == (d, d)
    assert train_error.shape == (1,) and len(opq_error) == 3 and recall.shape == (knn,)
    assert (np.diff(recall) >= 0).all() and recall[-1] > 0.5
    Cs = np.stack(C)
    norms_B, norms_C = rq.get_norms_codebook(B, C, seed=2)
    d0, i0 = oracle.linscan_lsq((B - 1).astype(np.uint8), Cs.reshape(m * h, d), Xq, norms_C[norms_B - 1], knn)
    assert np.allclose(recall, oracle.eval_recall(gt_t, i0, knn))
    C2, B2, R2, e2, rec2 = ex.experiment_lsq_cuda_query_base(Xt, B, C, R, Xq, gt_t, m, h, 1, 2, 4, True, 2, knn, seed=2)
    assert B2.shape == B.shape and rec2.shape == (knn,) and (np.diff(rec2) >= 0).all() and e2.shape == (1,)


def test_experiment_rvq_with_device_norms(rq, data):
    """norms="device" routes the RVQ driver through get_norms_codebook / rq_lsq_prepare_cbnorms.  The two paths round the norms
    differently, so a handful of rows may change cells: recall at rank knn within
    0.02 -- not a performance claim."""
    from rayuela_jl_amd import experiments as ex
    Xt, Xb, Xq, gt, gt_t = data
    m, h, knn = 4, 256, 50
    Ch, Bh, eh, Bbh, rech = ex.experiment_rvq(Xt, Xb, Xq, gt, m, h, 3, knn, seed=2)
    Cd, Bd, ed, Bbd, recd = ex.experiment_rvq(Xt, Xb, Xq, gt, m, h, 3, knn, seed=2, norms="device")
    assert np.array_equal(Bbd, Bbh) and np.array_equal(Bd, Bh) and ed == eh
    print("recall@%d host %.4f device %.4f" % (knn, rech[-1], recd[-1]))
    assert recd.shape == (knn,) and (np.diff(recd) >= 0).all() and abs(recd[-1] - rech[-1]) <= 0.02
    C3, B3, e3, rec3 = ex.experiment_rvq_query_base(Xt, Xq, gt_t, m, h, 2, knn, seed=2, norms="device")
    assert rec3.shape == (knn,) and (np.diff(rec3) >= 0).all()
    with pytest.raises(ValueError):
        ex.experiment_rvq(Xt, Xb, Xq, gt, m, h, 3, knn, seed=2, norms="gpu")
