"""GPU: quantize_pq / quantize_opq / quantize_rvq with more than 256 codewords per codebook (the *_wide entry points, 16-bit
codes; csrc/rq_encode_h16.hip) against tests/wide_oracle.py.  Every comparison is np.array_equal: codes and counts as integers,
residuals as uint32 views.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import wide_oracle as wo
import wide_stream_cases  # noqa: F401  (registers the stream cases of the *_wide entry points)

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2
KERNEL = "encode_h16_kernel"


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _oracle():
    from oracle import oracle
    oracle.lib()
    return oracle


def _ran():
    return (_L().rq_last_encode_kernel() or b"").decode()


def _p(a):
    return a.ctypes.data


def _sampled_codebooks(X, m, h, seed):
    """Codebooks sampled from the data (with replacement where h > n: duplicated codewords are ties)."""
    n, d = X.shape
    rng = np.random.default_rng(seed)
    off = wo.splitarray(d, m)
    return np.concatenate([X[rng.integers(0, n, h), off[i]:off[i + 1]].reshape(-1) for i in range(m)])


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    import rayuela_jl_amd.synth as synth
    n, d, m, h = shape
    X = (synth.sift_like if kind == "sift" else synth.deep_like)(n, d, seed=sum(shape))
    Ccat = _sampled_codebooks(X, m, h, h + d)
    ref = wo.encode_pq_wide(_oracle(), X, Ccat, m, h)
    for a in (X, Ccat, ref):
        a.setflags(write=False)
    return X, Ccat, ref


def _dev_pq(X, Ccat, m, h):
    import torch
    from rayuela_jl_amd import device
    got = device.encode_pq_wide(torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(Ccat)).cuda(), m, h)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _host_pq(X, Ccat, m, h, code_base):
    n, d = X.shape
    out = np.full((n, m), -7, np.int16)
    st = _L().rq_encode_pq_wide(_p(out), _p(X), _p(Ccat), n, d, m, h, code_base)
    assert st == 0, _L().rq_last_error()
    return out


def _diff(got, ref):
    return "rows differ: %d of %d" % (int((got != ref).any(axis=1).sum()), ref.shape[0])


# 1. PQ against the helper: two blocks with h % 32 != 0 and a ragged last tile; four full blocks; an uneven split (3, 3, 2, 2)
#    with a last block of ONE codeword; the largest h; fewer rows than one workgroup's tiles; a sub-space of 100 (k-chunks times
#    codeword blocks)
PQ_SHAPES = [(3001, 32, 4, 300), (2000, 128, 8, 1024), (1000, 10, 4, 257), (500, 8, 1, 32767), (33, 16, 2, 512),
             (1500, 200, 2, 600)]


@pytest.mark.parametrize("kind", ["sift", "deep"])
@pytest.mark.parametrize("shape", PQ_SHAPES)
def test_pq_equals_the_helper(rq, shape, kind):
    n, d, m, h = shape
    X, Ccat, ref = _case(shape, kind)
    got = _dev_pq(X, Ccat, m, h)
    assert _ran() == KERNEL
    assert np.array_equal(got, ref), _diff(got, ref)
    for base in (0, 1):
        got = _host_pq(X, Ccat, m, h, base)
        assert _ran() == KERNEL
        assert np.array_equal(got, ref + base), (base, _diff(got, ref + base))


# 2. ties across blocks: every codeword again 256 (and 512) places further on -- the lower index wins
@pytest.mark.parametrize("copies", [2, 3])
def test_a_codeword_repeated_in_a_later_block_loses(rq, copies):
    import torch
    from rayuela_jl_amd import device
    n, d, m = 2000, 32, 4
    X, C256, _ = _case((n, d, m, 256), "sift")
    sub = d // m
    Cw = np.concatenate([np.tile(C256[i * 256 * sub:(i + 1) * 256 * sub], copies) for i in range(m)])
    got = _dev_pq(X, Cw, m, 256 * copies)
    assert _ran() == KERNEL
    assert got.max() < 256
    u8 = device.encode_pq(torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(C256)).cuda(), m, 256)
    assert np.array_equal(got, u8.cpu().numpy().astype(np.int16))
    assert np.array_equal(got, wo.encode_pq_wide(_oracle(), X, Cw, m, 256 * copies))


# 3. exact hits: every sub-vector IS a codeword with an index past 255; distance 0 after the clamp, and no other codeword is
#    at distance 0 (the codewords are distinct)
def test_exact_hits_past_the_first_block(rq):
    n, d, m, h = 1000, 32, 4, 600
    rng = np.random.default_rng(3)
    sub = d // m
    C = rng.integers(-50, 50, (m, h, sub)).astype(np.float32)
    C[:, :, 0] = np.arange(h, dtype=np.float32)[None, :]              # distinct codewords
    k = rng.integers(256, h, (n, m))
    X = np.concatenate([C[i][k[:, i]] for i in range(m)], axis=1)
    got = _dev_pq(X, C.reshape(-1), m, h)
    assert _ran() == KERNEL
    assert np.array_equal(got, k.astype(np.int16))
    assert np.array_equal(_host_pq(X, C.reshape(-1), m, h, 1), k.astype(np.int16) + 1)


# 4. non-finite values: the call returns, every code is below h, the codes are the helper's
def test_non_finite_rows_and_codewords(rq):
    n, d, m, h = 1000, 32, 4, 300
    X, Ccat, _ = _case((n, d, m, h), "sift")
    X, Ccat = np.array(X), np.array(Ccat)
    X[3, 5] = np.nan
    X[10, 0] = np.inf
    X[20, 31] = -np.inf
    X[40, 8:16] = np.inf
    X[n - 1, 17] = np.nan
    sub = d // m
    Ccat[1 * h * sub + 270 * sub + 2] = np.inf                       # codeword 270 of sub-quantizer 1
    ref = wo.encode_pq_wide(_oracle(), X, Ccat, m, h)
    got = _dev_pq(X, Ccat, m, h)
    assert _ran() == KERNEL
    assert got.min() >= 0 and got.max() < h
    assert np.array_equal(got, ref), _diff(got, ref)
    got = _host_pq(X, Ccat, m, h, 0)
    assert np.array_equal(got, ref), _diff(got, ref)


# 5. h <= 256 through the wide entries: the codes of rq_dev_encode_pq
@pytest.mark.parametrize("shape", [(2000, 128, 8, 256), (3001, 64, 5, 77)])
def test_up_to_256_codewords_give_the_u8_codes(rq, shape):
    import torch
    from rayuela_jl_amd import device
    n, d, m, h = shape
    X, Ccat, ref = _case(shape, "sift")
    u8 = device.encode_pq(torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(Ccat)).cuda(), m, h).cpu().numpy()
    got = _dev_pq(X, Ccat, m, h)
    assert np.array_equal(got, u8.astype(np.int16)) and np.array_equal(got, ref)
    assert np.array_equal(_host_pq(X, Ccat, m, h, 1), u8.astype(np.int16) + 1)


# 6. OPQ: the helper on the oracle's R'X
@pytest.mark.parametrize("shape", [(2000, 32, 4, 512), (1000, 30, 3, 300)])
def test_opq_equals_the_helper_on_the_rotated_rows(rq, shape):
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device
    n, d, m, h = shape
    X, Ccat, _ = _case(shape, "sift")
    R = synth.rotation(d, seed=d)
    ref = wo.encode_pq_wide(_oracle(), _oracle().rotate_T(R, X), Ccat, m, h)
    got = device.encode_opq_wide(torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(R).cuda(),
                                 torch.from_numpy(np.array(Ccat)).cuda(), m, h).cpu().numpy()
    assert _ran() == KERNEL
    assert np.array_equal(got, ref), _diff(got, ref)
    for base in (0, 1):
        out = np.full((n, m), -7, np.int16)
        assert _L().rq_encode_opq_wide(_p(out), _p(X), _p(R), _p(Ccat), n, d, m, h, base) == 0, _L().rq_last_error()
        assert np.array_equal(out, ref + base), (base, _diff(out, ref + base))


# 7. RVQ: codes, counts [m][h] and the final residual; d % 4 != 0 takes the scalar epilogue
@functools.lru_cache(maxsize=None)
def _rvq_case(shape):
    import rayuela_jl_amd.synth as synth
    n, d, m, h = shape
    X = synth.sift_like(n, d, seed=sum(shape))
    rng = np.random.default_rng(h)
    Cs = np.empty((m, h, d), np.float32)
    Xr = X.copy()
    for i in range(m):                                            # stage codebooks sampled from the running residual
        Cs[i] = Xr[rng.integers(0, n, h)]
        Xr = Xr - Cs[i][rng.integers(0, h, n)] * np.float32(0.5)
    return X, Cs, wo.encode_rvq_wide(_oracle(), X, Cs)


@pytest.mark.parametrize("shape", [(3001, 64, 3, 300), (1000, 30, 2, 257), (2000, 128, 2, 1024)])
def test_rvq_codes_counts_and_residual(rq, shape):
    import torch
    from rayuela_jl_amd import device
    n, d, m, h = shape
    X, Cs, (codes0, counts0, Xr0) = _rvq_case(shape)
    Xr = torch.from_numpy(X.copy()).cuda()
    codes, counts = device.encode_rvq_wide(Xr, torch.from_numpy(Cs).cuda(), want_counts=True)
    torch.cuda.synchronize()
    assert _ran() == KERNEL
    assert np.array_equal(codes.cpu().numpy(), codes0)
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), counts0)
    assert np.array_equal(Xr.cpu().numpy().view(np.uint32), Xr0.view(np.uint32))
    for base in (0, 1):
        out = np.full((n, m), -7, np.int16)
        cnt = np.full((m, h), 0xA5A5A5A5, np.uint32)
        res = np.full((n, d), np.nan, np.float32)
        st = _L().rq_encode_rvq_wide(_p(out), _p(X), _p(Cs), n, d, m, h, base, _p(cnt), _p(res))
        assert st == 0, _L().rq_last_error()
        assert np.array_equal(out, codes0 + base) and np.array_equal(cnt, counts0)
        assert np.array_equal(res.view(np.uint32), Xr0.view(np.uint32))


def test_rvq_singletons_and_null_counts(rq):
    import torch
    from rayuela_jl_amd import device
    shape = (3001, 64, 3, 300)
    n, d, m, h = shape
    X, Cs, (codes0, counts0, Xr0) = _rvq_case(shape)
    B, singletons = rq.quantize_rvq(X, [Cs[i] for i in range(m)])
    assert B.dtype == np.int16 and np.array_equal(B, codes0 + 1)
    assert (counts0 == 0).any()
    for i in range(m):
        unused = int((counts0[i] == 0).sum())
        assert (singletons[i] is None) == (unused == 0)
        if unused:
            assert singletons[i].shape == (unused, d)
    # counts = NULL: host and device forms
    out = np.full((n, m), -7, np.int16)
    assert _L().rq_encode_rvq_wide(_p(out), _p(X), _p(Cs), n, d, m, h, 0, None, None) == 0, _L().rq_last_error()
    assert np.array_equal(out, codes0)
    Xr = torch.from_numpy(X.copy()).cuda()
    codes = device.encode_rvq_wide(Xr, torch.from_numpy(Cs).cuda())
    assert np.array_equal(codes.cpu().numpy(), codes0)
    assert np.array_equal(Xr.cpu().numpy().view(np.uint32), Xr0.view(np.uint32))


# 8. the host path over more than one upload chunk
def test_host_path_over_two_upload_chunks(rq):
    from rayuela_jl_amd import utils
    shape = (35001, 960, 8, 300)
    n, d, m, h = shape
    assert utils.encode_chunk_rows(d) == 34952 < n
    X, Ccat, ref = _case(shape, "sift")
    got = _host_pq(X, Ccat, m, h, 1)
    assert _ran() == KERNEL
    assert np.array_equal(got, ref + 1), _diff(got, ref + 1)


# 9. argument errors leave sentinel-filled outputs untouched
def test_argument_errors_leave_the_outputs_untouched(rq):
    import torch
    L = _L()
    n, d, m, h = 8, 16, 4, 300
    X = np.zeros((n, d), np.float32)
    C = np.zeros(h * d, np.float32)
    Cs = np.zeros((2, h, d), np.float32)
    R = np.eye(d, dtype=np.float32)
    out = np.full((n, 64), -3, np.int16)
    cnt = np.full((65, h), 0xA5A5A5A5, np.uint32)
    res = np.full((n, d), 7.0, np.float32)
    dX, dC, dCs, dR = (torch.from_numpy(a).cuda() for a in (X, C, Cs, R))
    dout = torch.full((n, 64), -3, dtype=torch.int16, device="cuda")
    dcnt = torch.full((65, h), 5, dtype=torch.int32, device="cuda")
    dXr = dX.clone()
    t = lambda a: a.data_ptr()      # noqa: E731
    calls = [
        # h = 32768
        (lambda: L.rq_encode_pq_wide(_p(out), _p(X), _p(C), n, d, m, 32768, 0), RQ_EUNSUPPORTED),
        (lambda: L.rq_encode_opq_wide(_p(out), _p(X), _p(R), _p(C), n, d, m, 32768, 1), RQ_EUNSUPPORTED),
        (lambda: L.rq_encode_rvq_wide(_p(out), _p(X), _p(Cs), n, d, 2, 32768, 0, _p(cnt), _p(res)), RQ_EUNSUPPORTED),
        (lambda: L.rq_dev_encode_pq_wide(t(dout), t(dX), t(dC), n, d, m, 32768, None), RQ_EUNSUPPORTED),
        (lambda: L.rq_dev_encode_opq_wide(t(dout), t(dX), t(dR), t(dC), n, d, m, 32768, None), RQ_EUNSUPPORTED),
        (lambda: L.rq_dev_encode_rvq_wide(t(dout), t(dXr), t(dCs), n, d, 2, 32768, t(dcnt), None), RQ_EUNSUPPORTED),
        # m = 33 (PQ, OPQ), m = 65 (RVQ)
        (lambda: L.rq_encode_pq_wide(_p(out), _p(X), _p(C), 2, 64, 33, 4, 0), RQ_EUNSUPPORTED),
        (lambda: L.rq_encode_opq_wide(_p(out), _p(X), _p(R), _p(C), 2, 64, 33, 4, 0), RQ_EUNSUPPORTED),
        (lambda: L.rq_dev_encode_pq_wide(t(dout), t(dX), t(dC), 2, 64, 33, 4, None), RQ_EUNSUPPORTED),
        (lambda: L.rq_encode_rvq_wide(_p(out), _p(X), _p(Cs), n, d, 65, 4, 0, _p(cnt), _p(res)), RQ_EUNSUPPORTED),
        (lambda: L.rq_dev_encode_rvq_wide(t(dout), t(dXr), t(dCs), n, d, 65, 4, t(dcnt), None), RQ_EUNSUPPORTED),
        # code_base = 2
        (lambda: L.rq_encode_pq_wide(_p(out), _p(X), _p(C), n, d, m, h, 2), RQ_EINVAL),
        (lambda: L.rq_encode_opq_wide(_p(out), _p(X), _p(R), _p(C), n, d, m, h, -1), RQ_EINVAL),
        (lambda: L.rq_encode_rvq_wide(_p(out), _p(X), _p(Cs), n, d, 2, h, 2, _p(cnt), _p(res)), RQ_EINVAL),
        # d < m
        (lambda: L.rq_encode_pq_wide(_p(out), _p(X), _p(C), n, 2, 4, h, 0), RQ_EINVAL),
        (lambda: L.rq_encode_opq_wide(_p(out), _p(X), _p(R), _p(C), n, 2, 4, h, 0), RQ_EINVAL),
        (lambda: L.rq_dev_encode_pq_wide(t(dout), t(dX), t(dC), n, 2, 4, h, None), RQ_EINVAL),
        (lambda: L.rq_dev_encode_opq_wide(t(dout), t(dX), t(dR), t(dC), n, 2, 4, h, None), RQ_EINVAL),
        # NULL pointers
        (lambda: L.rq_encode_pq_wide(None, _p(X), _p(C), n, d, m, h, 0), RQ_EINVAL),
        (lambda: L.rq_encode_pq_wide(_p(out), None, _p(C), n, d, m, h, 0), RQ_EINVAL),
        (lambda: L.rq_encode_pq_wide(_p(out), _p(X), None, n, d, m, h, 0), RQ_EINVAL),
        (lambda: L.rq_encode_opq_wide(_p(out), _p(X), None, _p(C), n, d, m, h, 0), RQ_EINVAL),
        (lambda: L.rq_encode_rvq_wide(_p(out), None, _p(Cs), n, d, 2, h, 0, _p(cnt), _p(res)), RQ_EINVAL),
        (lambda: L.rq_encode_rvq_wide(_p(out), _p(X), None, n, d, 2, h, 0, _p(cnt), _p(res)), RQ_EINVAL),
        (lambda: L.rq_dev_encode_pq_wide(t(dout), None, t(dC), n, d, m, h, None), RQ_EINVAL),
        (lambda: L.rq_dev_encode_opq_wide(t(dout), t(dX), None, t(dC), n, d, m, h, None), RQ_EINVAL),
        (lambda: L.rq_dev_encode_rvq_wide(None, t(dXr), t(dCs), n, d, 2, h, t(dcnt), None), RQ_EINVAL),
        # n = 0: nothing to do
        (lambda: L.rq_encode_pq_wide(_p(out), _p(X), _p(C), 0, d, m, h, 0), 0),
        (lambda: L.rq_encode_opq_wide(_p(out), _p(X), _p(R), _p(C), 0, d, m, h, 1), 0),
        (lambda: L.rq_encode_rvq_wide(_p(out), _p(X), _p(Cs), 0, d, 2, h, 0, _p(cnt), _p(res)), 0),
        (lambda: L.rq_dev_encode_pq_wide(t(dout), t(dX), t(dC), 0, d, m, h, None), 0),
        (lambda: L.rq_dev_encode_opq_wide(t(dout), t(dX), t(dR), t(dC), 0, d, m, h, None), 0),
        (lambda: L.rq_dev_encode_rvq_wide(t(dout), t(dXr), t(dCs), 0, d, 2, h, t(dcnt), None), 0),
    ]
    for i, (call, want) in enumerate(calls):
        st = call()
        assert st == want, (i, st, want, L.rq_last_error())
        if want:
            assert L.rq_last_error(), i
    torch.cuda.synchronize()
    assert (out == -3).all() and (cnt == 0xA5A5A5A5).all() and (res == 7.0).all()
    assert bool((dout == -3).all()) and bool((dcnt == 5).all()) and bool((dXr == 0).all())
    # the u8 and Int16-widening entries keep refusing h = 257
    out8 = np.full((n, m), 0x5A, np.uint8)
    dout8 = torch.full((n, m), 0x5A, dtype=torch.uint8, device="cuda")
    assert L.rq_encode_pq(_p(out8), _p(X), _p(C), n, d, m, 257) == RQ_EUNSUPPORTED
    assert L.rq_encode_pq_i16(_p(out), _p(X), _p(C), n, d, m, 257) == RQ_EUNSUPPORTED
    assert L.rq_encode_opq(_p(out8), _p(X), _p(R), _p(C), n, d, m, 257) == RQ_EUNSUPPORTED
    assert L.rq_encode_opq_i16(_p(out), _p(X), _p(R), _p(C), n, d, m, 257) == RQ_EUNSUPPORTED
    assert L.rq_dev_encode_pq(t(dout8), t(dX), t(dC), n, d, m, 257, None) == RQ_EUNSUPPORTED
    assert L.rq_encode_rvq(_p(out8), _p(X), _p(Cs), n, d, 2, 257, None, None) != 0
    assert L.rq_encode_rvq_i16(_p(out), _p(X), _p(Cs), n, d, 2, 257, None, None) != 0
    torch.cuda.synchronize()
    assert (out8 == 0x5A).all() and (out == -3).all() and bool((dout8 == 0x5A).all())


# 10. the Python mirrors
def test_python_mirrors(rq):
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device
    shape = (3001, 32, 4, 300)
    n, d, m, h = shape
    X, Ccat, ref = _case(shape, "sift")
    C, off = wo.sub_codebooks(Ccat, d, m, h)
    B = rq.quantize_pq(X, C)
    assert B.dtype == np.int16 and np.array_equal(B, ref + 1)
    B0 = rq.quantize_pq_u16(X, C)
    assert B0.dtype == np.uint16 and np.array_equal(B0, ref.astype(np.uint16))
    R = synth.rotation(d, seed=d)
    refo = wo.encode_pq_wide(_oracle(), _oracle().rotate_T(R, X), Ccat, m, h)
    B = rq.quantize_opq(X, R, C)
    assert B.dtype == np.int16 and np.array_equal(B, refo + 1)
    B0 = rq.quantize_opq_u16(X, R, C)
    assert B0.dtype == np.uint16 and np.array_equal(B0, refo.astype(np.uint16))
    Xv, Cs, (codes0, counts0, Xr0) = _rvq_case((3001, 64, 3, 300))
    B, _ = rq.quantize_rvq(Xv, [Cs[i] for i in range(3)])
    assert B.dtype == np.int16 and np.array_equal(B, codes0 + 1)
    B0, cnt, Xr = rq.quantize_rvq_u16(Xv, [Cs[i] for i in range(3)], with_extras=True)
    assert B0.dtype == np.uint16 and np.array_equal(B0, codes0.astype(np.uint16))
    assert np.array_equal(cnt, counts0) and np.array_equal(Xr.view(np.uint32), Xr0.view(np.uint32))
    # the torch wrappers on resident tensors, with out=
    dX, dC, dR = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(Ccat)).cuda(), torch.from_numpy(R).cuda()
    out = torch.full((n, m), -1, dtype=torch.int16, device="cuda")
    assert device.encode_pq_wide(dX, dC, m, h, out=out) is out and np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(device.encode_opq_wide(dX, dR, dC, m, h, out=out).cpu().numpy(), refo)
    dXr = torch.from_numpy(Xv.copy()).cuda()
    out3 = torch.full((3001, 3), -1, dtype=torch.int16, device="cuda")
    codes, counts = device.encode_rvq_wide(dXr, torch.from_numpy(Cs).cuda(), out=out3, want_counts=True)
    assert codes is out3 and np.array_equal(codes.cpu().numpy(), codes0)
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), counts0)
    assert np.array_equal(dXr.cpu().numpy().view(np.uint32), Xr0.view(np.uint32))
