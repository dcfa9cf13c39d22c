"""GPU: beam-search residual encoding with more than 256 codewords per stage (rq_beam.hip, DESIGN.md section 4.21;
src/CompetitiveQ.jl:75-135 on Int16 codes) through rq_encode_rvq_beam_wide / rq_dev_encode_rvq_beam_wide and their mirrors:
codes, residual and cost bit for bit against the numpy restatement of tests/beam_wide_oracle.py, H = 1 against
rq_encode_rvq_wide, h <= 256 against rq_encode_rvq_beam, ties across codeword blocks, independence of chunking / pointer form /
alignment / stream, the argument checks and non-finite inputs."""
import numpy as np
import pytest

import beam_oracle as bo
import beam_wide_oracle as bw
import beam_wide_stream_cases as bwsc
import stream_cases as sc

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2
PARITY = [(s[:5], H) for s in bw.GPU_SHAPES for H in s[5]] + [("big", 32)]
TIES = [(("ties", s), H) for s in bw.TIE_SHAPES for H in bw.TIE_BEAMS]


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _p(a):
    return None if a is None else a.ctypes.data


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    codes, cost, Xr = got
    assert codes.dtype in (np.int16, np.uint16)
    assert np.array_equal(codes.view(np.int16), want[0]), "rows differ: %d of %d" % (
        int((codes.view(np.int16) != want[0]).any(axis=1).sum()), len(codes))
    assert np.array_equal(_bits(Xr), _bits(want[1])) and np.array_equal(_bits(cost), _bits(want[2]))


def _host(X, C, H, nsplits=1, base=0):
    n, d = X.shape
    m, h, _ = C.shape
    codes = np.full((n, m), -3, dtype=np.int16)
    cost, Xr = np.full((n,), -7.0, dtype=np.float32), np.full((n, d), -7.0, dtype=np.float32)
    rc = _L().rq_encode_rvq_beam_wide(_p(codes), _p(X), _p(np.ascontiguousarray(C)), n, d, m, h, H, nsplits, base, _p(cost), _p(Xr))
    assert rc == 0, _L().rq_last_error()
    return codes, cost, Xr


@pytest.fixture(scope="module")
def side(rq):
    """One side stream for the module; its scratch is given back afterwards (a device keeps scratch for at most 8 streams).
    torch hands out the 32 streams of its pool in turn.  The module takes one whole turn and uses the first, so the files that
    run after it meet the pool where they met it before this file existed: tests/test_gpu_streams.py picks its streams by how
    the pool happens to be dealt over the process's hardware queues."""
    import torch
    st = [torch.cuda.Stream() for _ in range(32)][0]
    yield st
    torch.cuda.synchronize()
    assert _L().rq_release_workspaces() == 0


def _dev_call(X, C, H, st, nsplits=1):
    """rq_dev_encode_rvq_beam_wide on torch tensors X, C on stream st; sentinel-filled outputs with one spare row."""
    import torch
    n, d = X.shape
    m, h, _ = C.shape
    codes = torch.full((n + 1, m), -3, dtype=torch.int16, device="cuda")
    Xr = torch.full((n + 1, d), -7.0, dtype=torch.float32, device="cuda")
    cost = torch.full((n + 1,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = _L().rq_dev_encode_rvq_beam_wide(codes.data_ptr(), Xr.data_ptr(), cost.data_ptr(), X.data_ptr(), C.data_ptr(), n, d, m, h, H,
                                          nsplits, st.cuda_stream)
    assert rc == 0, _L().rq_last_error()
    st.synchronize()
    return codes.cpu().numpy(), cost.cpu().numpy(), Xr.cpu().numpy()


# ---- 1. bit parity with the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,H", PARITY + TIES, ids=lambda v: str(v).replace(" ", ""))
def test_codes_residual_and_cost_equal_the_restatement(rq, shape, H):
    X, C, codes, Xr, cost = bw.expected(shape, H)
    _same(rq.quantize_competitiveq_u16(X, list(C), H, with_extras=True), (codes, Xr, cost))


@pytest.mark.parametrize("shape", [s[:5] for s in bw.GPU_SHAPES], ids=lambda v: str(v).replace(" ", ""))
def test_beam_of_one_is_quantize_rvq_wide(rq, shape):
    X, C = bw.data(*shape)
    c0, _, r0 = rq.quantize_rvq_u16(X, list(C), with_extras=True)
    c1, _, r1 = rq.quantize_competitiveq_u16(X, list(C), 1, with_extras=True)
    assert np.array_equal(c0, c1) and np.array_equal(_bits(r0), _bits(r1))


@pytest.mark.parametrize("shape", [(500, 128, 8, 256, "sift"), (3_001, 64, 5, 77, "deep")], ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("H", [1, 3, 32])
def test_up_to_256_codewords_the_wide_entries_give_the_byte_entries_bits(rq, shape, H):
    X, C = bo.data(*shape)
    c8, cost8, r8 = rq.quantize_competitiveq_u8(X, list(C), H, with_extras=True)
    for base in (0, 1):
        c, cost, r = _host(X, C, H, base=base)
        assert np.array_equal(c, c8.astype(np.int16) + base)
        assert np.array_equal(_bits(cost), _bits(cost8)) and np.array_equal(_bits(r), _bits(r8))


# ---- 2. chunking, pointer form, alignment, stream -----------------------------------------------------------------------------
@pytest.mark.parametrize("H", [3, 16])
def test_nsplits_stream_and_pointer_form_do_not_change_a_bit(rq, side, H):
    import torch
    shape = bw.GPU_SHAPES[0][:5]
    X, C, codes, Xr, cost = bw.expected(shape, H)
    n = X.shape[0]
    tX, tC = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    for nsplits in (1, 7):
        c, co, r = _host(X, C, H, nsplits=nsplits, base=1)
        _same((c - 1, co, r), (codes, Xr, cost))
        c, co, r = _dev_call(tX, tC, H, side, nsplits)                 # a stream that is not the default one
        _same((c[:n], co[:n], r[:n]), (codes, Xr, cost))
        assert (c[n] == -3).all() and co[n] == -7.0 and (r[n] == -7.0).all()       # nothing past row n - 1
        assert np.array_equal(_bits(tX.cpu().numpy()), _bits(X)), "X was overwritten"


@pytest.mark.parametrize("name", sorted(bwsc.BEAM_WIDE_CASES))
def test_device_form_is_ordered_on_a_side_stream(rq, side, name):
    """The harness of tests/test_gpu_streams.py: the call on a side stream behind that file's delay (2e7 cycles), inputs holding
    poison until the stream fills them, outputs consumed on that stream only."""
    case = sc.get(name)
    case.check(sc.run_on_side_stream(case, side, 0))                 # grows this stream's scratch outside the delayed run
    case.check(sc.run_on_side_stream(case, side, 20_000_000))


@pytest.mark.parametrize("which", ["X", "C", "both"])
def test_unaligned_device_pointers_give_the_same_bits(rq, side, which):
    import torch
    shape, H = bw.GPU_SHAPES[0][:5], 3
    X, C, codes, Xr, cost = bw.expected(shape, H)
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
    n, d, m, h = 40, 16, 3, 300
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = rng.standard_normal((65 * 300, d)).astype(np.float32)         # big enough for every (m, h) read before a refusal
    bad = [(dict(H=0), RQ_EINVAL), (dict(H=33), RQ_EINVAL), (dict(H=17, h=16), RQ_EINVAL), (dict(m=65), RQ_EUNSUPPORTED),
           (dict(m=0), RQ_EUNSUPPORTED), (dict(h=32768), RQ_EUNSUPPORTED), (dict(h=0), RQ_EINVAL), (dict(d=0), RQ_EINVAL),
           (dict(base=2), RQ_EINVAL), (dict(n=-1), RQ_EINVAL), (dict(nsplits=0), RQ_EINVAL), (dict(X=None), RQ_EINVAL),
           (dict(C=None), RQ_EINVAL), (dict(codes=None), RQ_EINVAL)]
    tX, tC = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    for kw, want in bad:
        a = dict(n=n, d=d, m=m, h=h, H=2, nsplits=1, base=0, X=X, C=C, codes=1)
        a.update(kw)
        codes = np.full((n, 65), -3, dtype=np.int16)
        cost = np.full((n,), -7.0, dtype=np.float32)
        Xr = np.full((n, d), -7.0, dtype=np.float32)
        rc = L.rq_encode_rvq_beam_wide(None if a["codes"] is None else _p(codes), _p(a["X"]), _p(a["C"]), a["n"], a["d"], a["m"],
                                       a["h"], a["H"], a["nsplits"], a["base"], _p(cost), _p(Xr))
        assert rc == want and L.rq_last_error(), (kw, rc)
        assert (codes == -3).all() and (cost == -7.0).all() and (Xr == -7.0).all(), kw
        if "base" in kw:
            continue
        tcodes = torch.full((n, 65), -3, dtype=torch.int16, device="cuda")
        tcost = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        tXr = torch.full((n, d), -7.0, dtype=torch.float32, device="cuda")
        rc = L.rq_dev_encode_rvq_beam_wide(None if a["codes"] is None else tcodes.data_ptr(), tXr.data_ptr(), tcost.data_ptr(),
                                           None if a["X"] is None else tX.data_ptr(), None if a["C"] is None else tC.data_ptr(),
                                           a["n"], a["d"], a["m"], a["h"], a["H"], a["nsplits"], None)
        assert rc == want and L.rq_last_error(), (kw, rc)
        torch.cuda.synchronize()
        assert bool((tcodes == -3).all()) and bool((tcost == -7.0).all()) and bool((tXr == -7.0).all()), kw
    # no rows: fine, and nothing is written
    codes = np.full((4, m), -3, dtype=np.int16)
    assert L.rq_encode_rvq_beam_wide(_p(codes), _p(X), _p(C), 0, d, m, h, 2, 1, 0, None, None) == 0
    assert L.rq_dev_encode_rvq_beam_wide(None, None, None, None, tC.data_ptr(), 0, d, m, h, 2, 1, None) == 0
    assert (codes == -3).all()
    # the byte entries refuse h > 256 as before
    c8 = np.full((n, m), sc.SENTINEL, dtype=np.uint8)
    assert L.rq_encode_rvq_beam(_p(c8), _p(X), _p(C), n, d, m, 257, 2, 1, None, None) == RQ_EINVAL and (c8 == sc.SENTINEL).all()
    with pytest.raises(ValueError):
        rq.quantize_competitiveq(X, [np.zeros((32768, d), np.float32)], 2)


# ---- 4. mirrors -------------------------------------------------------------------------------------------------------------------
def test_host_mirrors_dispatch_on_the_codebook_size(rq):
    shape, H = bw.GPU_SHAPES[0][:5], 3
    X, C, codes, Xr, cost = bw.expected(shape, H)
    n, d = X.shape
    m, h, _ = C.shape
    B = rq.quantize_competitiveq(X, list(C), H)
    assert B.dtype == np.int16 and B.shape == (n, m) and np.array_equal(B, codes + 1)   # one-based, quantize_rvq's layout
    u16 = rq.quantize_competitiveq_u16(X, list(C), H)
    assert u16.dtype == np.uint16 and np.array_equal(u16.view(np.int16), codes)
    for row in (0, 417, n - 1):
        b, r = rq.CompetitiveQ.encode(X[row], list(C), None, m, h, d, H)
        assert b.dtype == np.int16 and b.shape == (m,) and np.array_equal(b, B[row])
        assert r.shape == (d,) and np.array_equal(_bits(r), _bits(Xr[row]))
    t = rq.last_beam_timing()
    assert t["stage_ms"] > 0 and t["expand_ms"] > 0


# ---- 5. non-finite input --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 3, 16])
def test_non_finite_inputs_return_codes_in_range_and_the_same_bits_twice(rq, H):
    shape = bw.GPU_SHAPES[0][:5]
    X, C = bw.data(*shape)
    X, C = X.copy(), C.copy()
    h = C.shape[1]
    X[5, 3], X[70, :], X[71, 9] = np.nan, np.inf, -np.inf               # a NaN row, an Inf row
    C[1, 280, :], C[2, 60, 5] = np.inf, np.nan                          # an Inf codeword in the second block
    a = _host(X, C, H)
    b = _host(X, C, H)
    assert a[0].shape == (shape[0], shape[2]) and int(a[0].min()) >= 0 and int(a[0].max()) < h
    assert not np.isnan(a[1]).any() and (a[1] >= 0).all()               # the clamp leaves no NaN in the keys
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))
