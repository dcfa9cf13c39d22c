"""GPU: quantize_pq / quantize_opq on BYTE data (bvecs: src/xvecs_read.jl:14-52; the reference widens it on the host first,
src/read_datasets.jl:148-167).  The contract is one sentence: for every input the codes -- and with a rotation R'X -- equal,
bit for bit, those of the f32 entry points on X.astype(float32).  Unless noted every check is a three-way equality:
byte path == oracle on the widened array == today's f32 entry point on the widened array."""
import ctypes
import functools

import numpy as np
import pytest

import bytes_stream_cases  # noqa: F401  (the byte entries' cases of tests/test_gpu_streams.py)
import stream_cases as sc
from switch_table import switches

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2
# (d, m, h) the byte filter + exact pass covers: sub 16; sub 6 (packed fragments); sub 8; sub 10 with d % 4 != 0 (rows start at
# every byte parity); sub 2, one tile, h no multiple of 32
FILTER_SHAPES = [(128, 8, 256), (96, 16, 256), (32, 4, 256), (30, 3, 64), (8, 4, 17)]
# shapes that are widened on the device and take the f32 kernels: uneven split 3,3,2,2; sub 32 (direct kernel); the wide
# kernel (with ENC_DIRECT = 0, as tests/stream_cases.py selects it); one odd-width sub-space
FALLBACK_SHAPES = [(10, 4, 256), (128, 4, 256), (96, 1, 256), (17, 1, 5)]
ROWS = [1, 31, 32, 33, 5000]      # the 32-row tile's tail; 5000 rows = several exact-pass workgroups of 1024 rows
NMAX = max(ROWS)
KINDS = ["sift", "ties", "uniform"]


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _kernel():
    return (_L().rq_last_encode_kernel() or b"").decode()


def _splits(d, m):
    per, extra = divmod(d, m)
    return [per + (1 if i < extra else 0) for i in range(m)]


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(X uint8 (NMAX, d), C list of m (h, sub_i) f32, oracle codes of X.astype(f32)) -- computed once, never modified."""
    import rayuela_jl_amd.synth as synth
    from oracle import oracle
    d, m, h = shape
    seed = 1000 + 7 * d + m
    rng = np.random.default_rng(seed)
    if kind == "sift":
        Xf = synth.sift_like(NMAX, d, seed=seed)
        X = Xf.astype(np.uint8)
        assert np.array_equal(X.astype(np.float32), Xf)            # integer-valued 0..255: the cast is exact
        C = synth.codebooks(Xf, m, h, seed=seed + 1, iters=1, sample=2000)
    elif kind == "uniform":
        X = rng.integers(0, 256, (NMAX, d), dtype=np.uint8)
        C = synth.codebooks(X.astype(np.float32), m, h, seed=seed + 1, iters=1, sample=2000)
    else:
        # ties and exact hits: integer codebooks with duplicated centroids, rows that ARE centroids, all-0 and all-255 rows
        C = []
        for sub in _splits(d, m):
            c = rng.integers(0, 256, (h, sub)).astype(np.float32)
            if h >= 4:
                c[0] = 0.0                                             # all-zero and all-255 centroids, each twice:
                c[1] = 255.0
                c[h // 2:] = c[:h - h // 2]                            # every centroid of the upper half repeats a lower one
            C.append(c)
        pick = rng.integers(0, h, (NMAX, m))
        X = np.concatenate([C[i][pick[:, i]] for i in range(m)], axis=1).astype(np.uint8)
        X[::7] = rng.integers(0, 256, (len(X[::7]), d), dtype=np.uint8)
        X[3::50] = 0
        X[4::50] = 255
    C = [np.ascontiguousarray(c, dtype=np.float32) for c in C]
    X.setflags(write=False)
    ref = oracle.encode_pq(X.astype(np.float32), synth.cat_codebooks(C), m, h)
    if kind == "ties" and h >= 4:
        # what the data was built for: an exact hit costs v = 0 after the clamp, and the FIRST of the equal centroids wins
        hit = np.ones(NMAX, bool)
        hit[::7] = False
        hit[3::50] = False
        hit[4::50] = False
        for i in range(m):
            assert (ref[hit, i] <= pick[hit, i]).all() and np.array_equal(C[i][ref[hit, i]], C[i][pick[hit, i]])
            assert h % 2 or (ref[hit, i] < h // 2).all()
        assert (ref[3::50] == 0).all() and (ref[4::50] == 1).all()
    ref.setflags(write=False)
    return X, C, ref


def _cat(C):
    return np.concatenate([c.reshape(-1) for c in C])


def _host(entry, X, C, m, h, R=None, dtype=np.uint8):
    n, d = X.shape
    Cc = _cat(C)
    out = np.full((n, m), 0x5A if dtype == np.uint8 else -3, dtype=dtype)
    args = [out.ctypes.data, X.ctypes.data] + ([R.ctypes.data] if R is not None else []) + [Cc.ctypes.data, n, d, m, h]
    rc = getattr(_L(), entry)(*args)
    assert rc == 0, _L().rq_last_error()
    return out


def _both(X, C, m, h, R=None):
    """(byte entry point on X, f32 entry point on the widened X), host pointers"""
    X = np.ascontiguousarray(X)
    Xf = X.astype(np.float32)
    if R is None:
        return _host("rq_encode_pq_bytes", X, C, m, h), _host("rq_encode_pq", Xf, C, m, h)
    return _host("rq_encode_opq_bytes", X, C, m, h, R), _host("rq_encode_opq", Xf, C, m, h, R)


# ---- 1. the shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=str)
def test_filter_shapes_equal_the_oracle_and_the_f32_path(rq, shape, kind):
    d, m, h = shape
    X, C, ref = _case(shape, kind)
    for n in ROWS:
        got, old = _both(X[:n], C, m, h)
        assert _kernel() == "encode_pq_filter_kernel"                 # (the f32 call ran last)
        assert np.array_equal(old, ref[:n]), (n, "f32 path != oracle")
        assert np.array_equal(got, ref[:n]), (n, "rows differ: %d" % int((got != ref[:n]).any(axis=1).sum()))
    got = _host("rq_encode_pq_bytes", np.ascontiguousarray(X[:33]), C, m, h)
    assert _kernel() == "encode_pq_filter_bytes_kernel" and np.array_equal(got, ref[:33])


@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=str)
def test_device_pieces_of_rows_do_not_change_a_code(rq, shape):
    """ENC_CHUNK_ROWS = 2048 at 5000 rows: three filter + exact-pass launches, the last one a remainder"""
    d, m, h = shape
    X, C, ref = _case(shape, "sift")
    with switches(ENC_CHUNK_ROWS=2048):
        got, old = _both(X, C, m, h)
    assert np.array_equal(old, ref) and np.array_equal(got, ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", FALLBACK_SHAPES, ids=str)
def test_fallback_shapes_equal_the_oracle_and_the_f32_path(rq, shape, kind):
    d, m, h = shape
    X, C, ref = _case(shape, kind)
    want = {(10, 4, 256): "encode_pq_kernel", (128, 4, 256): "encode_pq_direct_kernel", (96, 1, 256): "encode_wide_kernel",
            (17, 1, 5): None}[shape]
    with switches(**(dict(ENC_DIRECT=0) if shape == (96, 1, 256) else {})):
        for n in ROWS:
            Xn = np.ascontiguousarray(X[:n])
            got = _host("rq_encode_pq_bytes", Xn, C, m, h)
            ran = _kernel()
            old = _host("rq_encode_pq", Xn.astype(np.float32), C, m, h)
            assert ran == _kernel() and "bytes" not in ran            # the fallback reports the f32 kernel that ran
            assert want is None or ran == want, ran
            assert np.array_equal(old, ref[:n]) and np.array_equal(got, ref[:n]), n


def test_opq_with_a_wide_rotation(rq, oracle):
    """d = 512, m = 32, n = 257: the rotation is not one rotate_kernel_v2 covers -- widen, f32 rotation, f32 filter"""
    import rayuela_jl_amd.synth as synth
    d, m, h, n = 512, 32, 256, 257
    Xf = synth.sift_like(n, d, seed=77)
    X = Xf.astype(np.uint8)
    assert np.array_equal(X.astype(np.float32), Xf)
    C = synth.codebooks(Xf, m, h, seed=78, iters=1, sample=n)
    R = synth.rotation(d)
    got, old = _both(X, C, m, h, R)
    ref = oracle.encode_opq(Xf, R, _cat(C), m, h)
    assert np.array_equal(old, ref) and np.array_equal(got, ref)


@pytest.mark.parametrize("shape", [(128, 8, 256), (96, 16, 256), (32, 4, 256)], ids=str)
def test_opq_through_the_byte_rotation(rq, oracle, shape):
    import rayuela_jl_amd.synth as synth
    d, m, h = shape
    X, C, _ = _case(shape, "sift")
    R = synth.rotation(d)
    ref = oracle.encode_opq(X.astype(np.float32), R, _cat(C), m, h)
    for n in (1, 33, 5000):
        got, old = _both(X[:n], C, m, h, R)
        assert np.array_equal(old, ref[:n]) and np.array_equal(got, ref[:n]), n
    got16 = _host("rq_encode_opq_bytes_i16", np.ascontiguousarray(X[:33]), C, m, h, R, dtype=np.int16)
    assert np.array_equal(got16, ref[:33].astype(np.int16) + 1)


# ---- 2. device pointers at every byte alignment -------------------------------------------------------------------------------
@pytest.fixture
def side(rq):
    """One side stream per test; its scratch is given back afterwards (a device keeps scratch for at most 8 streams)."""
    import torch
    st = torch.cuda.Stream()
    yield st
    torch.cuda.synchronize()
    assert _L().rq_release_workspaces() == 0


def _at_offset(X, off):
    """X's bytes in a torch buffer, starting `off` bytes after its (256-byte aligned) beginning"""
    import torch
    n, d = X.shape
    buf = torch.zeros(n * d + 32, dtype=torch.uint8, device="cuda")
    view = buf[off:off + n * d].view(n, d)
    view.copy_(torch.from_numpy(np.array(X)))
    assert view.data_ptr() == buf.data_ptr() + off and buf.data_ptr() % 256 == 0
    return buf, view


@pytest.mark.parametrize("shape", [(128, 8, 256), (96, 16, 256), (30, 3, 64)], ids=str)
def test_device_entries_at_every_byte_offset(rq, oracle, side, shape):
    import torch
    import rayuela_jl_amd.synth as synth
    d, m, h = shape
    n = 1000
    X, C, ref = _case(shape, "sift")
    X, ref = X[:n], ref[:n]
    Xf = X.astype(np.float32)
    R = synth.rotation(d)
    ref_rx = oracle.rotate_T(R, Xf)
    ref_opq = oracle.encode_opq(Xf, R, _cat(C), m, h)
    tC, tR = torch.from_numpy(_cat(C)).cuda(), torch.from_numpy(R).cuda()
    for off in (0, 1, 2, 3, 4, 8):
        buf, tX = _at_offset(X, off)
        codes = torch.full((n + 1, m), sc.SENTINEL, dtype=torch.uint8, device="cuda")
        codes_o = torch.full((n + 1, m), sc.SENTINEL, dtype=torch.uint8, device="cuda")
        RX = torch.full((n + 1, d), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s = side.cuda_stream
        assert _L().rq_dev_encode_pq_bytes(codes.data_ptr(), tX.data_ptr(), tC.data_ptr(), n, d, m, h, s) == 0, _L().rq_last_error()
        assert _kernel() == "encode_pq_filter_bytes_kernel"
        assert _L().rq_dev_encode_opq_bytes(codes_o.data_ptr(), tX.data_ptr(), tR.data_ptr(), tC.data_ptr(), n, d, m, h, s) == 0, \
            _L().rq_last_error()
        assert _L().rq_dev_rotate_T_bytes(RX.data_ptr(), tR.data_ptr(), tX.data_ptr(), d, n, s) == 0, _L().rq_last_error()
        side.synchronize()
        c, co, rx = codes.cpu().numpy(), codes_o.cpu().numpy(), RX.cpu().numpy()
        assert np.array_equal(c[:n], ref), (off, int((c[:n] != ref).any(axis=1).sum()))
        assert np.array_equal(co[:n], ref_opq), off
        assert np.array_equal(rx[:n].view(np.uint32), ref_rx.view(np.uint32)), off
        assert (c[n] == sc.SENTINEL).all() and (co[n] == sc.SENTINEL).all() and (rx[n] == -7.0).all(), off   # the spare row
        assert np.array_equal(tX.cpu().numpy(), X) and int(buf[:off].sum()) == 0                         # the input is only read


@pytest.mark.parametrize("d", [32, 64, 96, 128, 512])
def test_rotation_of_bytes_is_bit_equal(rq, oracle, d):
    """rq_dev_rotate_T_bytes against the oracle's rotation of the widened rows; d = 512 takes the widen fallback"""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    n = 1000 if d < 512 else 257
    Xf = synth.sift_like(n, d, seed=90 + d)
    X = Xf.astype(np.uint8)
    assert np.array_equal(X.astype(np.float32), Xf)
    tX = torch.from_numpy(X).cuda()
    for R in (synth.rotation(d), np.eye(d, dtype=np.float32)):
        tR = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float32)).cuda()
        got = rqd.rotate_T(tR, tX).cpu().numpy()
        old = rqd.rotate_T(tR, tX.float()).cpu().numpy()
        ref = oracle.rotate_T(np.ascontiguousarray(R, dtype=np.float32), Xf)
        assert np.array_equal(old.view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got, Xf)          # (R = I last)


# ---- 3. the filter really ran, and decided identically ------------------------------------------------------------------------
def _stats():
    out = (ctypes.c_uint64 * 2)()
    assert _L().rq_last_encode_stats(ctypes.cast(out, ctypes.c_void_p)) == 0
    return int(out[0]), int(out[1])


def test_the_byte_filter_flags_the_same_pairs(rq):
    import torch
    from rayuela_jl_amd import device as rqd
    shape = (128, 8, 256)
    d, m, h = shape
    X, C, ref = _case(shape, "sift")
    tX, tC = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(_cat(C)).cuda()
    with switches(ENC_STATS=1):
        old = rqd.encode_pq(tX.float(), tC, m, h).cpu().numpy()
        pairs, flagged = _stats()
        assert _kernel() == "encode_pq_filter_kernel"
        # a property of the input, established by the f32 kernel: some pairs are settled by the filter, some are not
        assert pairs == NMAX * m and 0 < flagged < pairs, (pairs, flagged)
        got = rqd.encode_pq(tX, tC, m, h).cpu().numpy()
        assert _kernel() == "encode_pq_filter_bytes_kernel"
        assert _stats() == (pairs, flagged)
    assert np.array_equal(old, ref) and np.array_equal(got, ref)
    # ... and a shape the byte filter does not cover names the f32 kernel that ran
    X4, C4, ref4 = _case((128, 4, 256), "sift")
    got = rqd.encode_pq(torch.from_numpy(np.array(X4)).cuda(), torch.from_numpy(_cat(C4)).cuda(), 4, 256).cpu().numpy()
    assert _kernel() == "encode_pq_direct_kernel" and np.array_equal(got, ref4)
    # the one-pass split kernel (ENC_SPLIT = 2) and no filter at all (0) have no byte loaders: widened, same codes
    for v, name in ((2, "encode_pq_split_kernel"), (0, "encode_pq_direct_kernel")):
        with switches(ENC_SPLIT=v):
            got = rqd.encode_pq(tX, tC, m, h).cpu().numpy()
            assert _kernel() == name and np.array_equal(got, ref), v


# ---- 4. the host path across upload chunks ------------------------------------------------------------------------------------
def test_host_path_across_three_upload_chunks(rq, oracle):
    """d = 512, m = 32: 65536 rows per chunk (max(32768, 2^25 / d)), so 150000 rows are three chunks, 77 MB of bytes"""
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.utils import encode_chunk_rows
    d, m, h, n = 512, 32, 256, 150000
    assert encode_chunk_rows(d) == 65536
    # data (a), generated as one block of n / 8 rows and repeated (generating 77e6 values takes 11 s): the period, 18750 rows,
    # shares no multiple with the 65536-row chunk below n, so rows that landed in the wrong place would not go unnoticed
    Xf = np.tile(synth.sift_like(n // 8, d, seed=31), (8, 1))
    X = Xf.astype(np.uint8)
    assert X.shape == (n, d) and np.array_equal(X.astype(np.float32), Xf)
    C = synth.codebooks(Xf[:4096], m, h, seed=32, iters=1, sample=4096)
    old = _host("rq_encode_pq", Xf, C, m, h)              # (pinned to the oracle by the existing tests)
    head = oracle.encode_pq(Xf[:4096], _cat(C), m, h)
    tail = oracle.encode_pq(Xf[-4096:], _cat(C), m, h)
    assert np.array_equal(old[:4096], head) and np.array_equal(old[-4096:], tail)
    del Xf
    for overlap in (1, 0):
        with switches(**({} if overlap else dict(HOST_OVERLAP=0))):
            got = _host("rq_encode_pq_bytes", X, C, m, h)
            assert _kernel() == "encode_pq_filter_bytes_kernel"
            t = rq.last_timing()
            got16 = _host("rq_encode_pq_bytes_i16", X, C, m, h, dtype=np.int16)
        assert np.array_equal(got, old), (overlap, int((got != old).any(axis=1).sum()))
        assert np.array_equal(got16, old.astype(np.int16) + 1), overlap
        assert t["total_ms"] > 0 and t["h2d_ms"] > 0 and t["total_ms"] >= t["h2d_ms"], t


# ---- 5. the mirrors -----------------------------------------------------------------------------------------------------------
def test_python_mirrors_on_uint8(rq, oracle, tmp_path):
    import rayuela_jl_amd.synth as synth
    shape = (128, 8, 256)
    d, m, h = shape
    X, C, ref = _case(shape, "sift")
    X = np.ascontiguousarray(X)
    Xf = X.astype(np.float32)
    R = synth.rotation(d)
    ref_o = oracle.encode_opq(Xf, R, _cat(C), m, h)
    assert np.array_equal(rq.quantize_pq_u8(X, C), ref)
    B = rq.quantize_pq(X, C)
    assert B.dtype == np.int16 and np.array_equal(B, ref.astype(np.int16) + 1) and np.array_equal(B, rq.quantize_pq(Xf, C))
    Bo = rq.quantize_opq(X, R, C)
    assert np.array_equal(Bo, ref_o.astype(np.int16) + 1) and np.array_equal(Bo, rq.quantize_opq(Xf, R, C))
    with rq.Dataset(X) as ds, rq.Dataset(Xf) as df:
        for _ in range(2):                                    # twice: PQ, then OPQ, on the same resident bytes
            assert np.array_equal(ds.quantize(C), df.quantize(C))
            assert np.array_equal(ds.quantize(C, R=R, one_based=False), df.quantize(C, R=R, one_based=False))
        assert np.array_equal(ds.quantize(C, one_based=False), ref)
        assert np.array_equal(ds.quantize(C, R=R, one_based=False), ref_o)
    # bvecs file -> codes: piecewise reads (2048 rows), a middle range of the file
    fn = str(tmp_path / "base.bvecs")
    rq.bvecs_write(X, fn)
    assert np.array_equal(rq.bvecs_read(None, fn), X)
    assert np.array_equal(rq.quantize_bvecs(fn, C, rows_per_read=2048), rq.quantize_pq_u8(X, C))
    got = rq.quantize_bvecs(fn, C, bounds=(1001, 4500), rows_per_read=2048)
    assert np.array_equal(got, rq.quantize_pq_u8(X[1000:4500], C)) and np.array_equal(got, ref[1000:4500])
    got = rq.quantize_bvecs(fn, C, R=R, bounds=(1001, 4500), rows_per_read=2048, one_based=True)
    assert np.array_equal(got, ref_o[1000:4500].astype(np.int16) + 1)


def test_torch_mirrors_on_uint8(rq, oracle):
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    shape = (96, 16, 256)
    d, m, h = shape
    X, C, ref = _case(shape, "uniform")
    R = synth.rotation(d)
    tX, tC, tR = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(_cat(C)).cuda(), torch.from_numpy(R).cuda()
    assert np.array_equal(rqd.encode_pq(tX, tC, m, h).cpu().numpy(), ref)
    ref_o = oracle.encode_opq(X.astype(np.float32), R, _cat(C), m, h)
    assert np.array_equal(rqd.encode_opq(tX, tR, tC, m, h).cpu().numpy(), ref_o)
    assert np.array_equal(rqd.encode_opq(tX.float(), tR, tC, m, h).cpu().numpy(), ref_o)
    with pytest.raises(TypeError):
        rqd.encode_pq(tX.to(torch.int8), tC, m, h)
    torch.cuda.synchronize()


# ---- 6. argument checks -------------------------------------------------------------------------------------------------------
def test_argument_checks_answer_like_the_f32_entries(rq):
    import torch
    L = _L()
    n, d, m, h = 8, 16, 4, 256
    X = np.zeros((n, d), np.uint8)
    Xf = X.astype(np.float32)
    C = np.zeros(300 * d, np.float32)
    R = np.eye(d, dtype=np.float32)
    out = np.full((n, m), 0x5A, np.uint8)
    out16 = np.full((n, m), -3, np.int16)
    p = lambda a: a.ctypes.data        # noqa: E731

    def pair(f32_call, byte_call, want):
        a, b = f32_call(), byte_call()
        assert a == b == want, (a, b, want, L.rq_last_error())

    # R is NULL
    pair(lambda: L.rq_encode_opq(p(out), p(Xf), None, p(C), n, d, m, h),
         lambda: L.rq_encode_opq_bytes(p(out), p(X), None, p(C), n, d, m, h), RQ_EINVAL)
    pair(lambda: L.rq_encode_opq_i16(p(out16), p(Xf), None, p(C), n, d, m, h),
         lambda: L.rq_encode_opq_bytes_i16(p(out16), p(X), None, p(C), n, d, m, h), RQ_EINVAL)
    # n < 1: nothing to do
    for nn in (0, -5):
        pair(lambda: L.rq_encode_pq(p(out), p(Xf), p(C), nn, d, m, h), lambda: L.rq_encode_pq_bytes(p(out), p(X), p(C), nn, d, m, h), 0)
        pair(lambda: L.rq_encode_opq(p(out), p(Xf), p(R), p(C), nn, d, m, h),
             lambda: L.rq_encode_opq_bytes(p(out), p(X), p(R), p(C), nn, d, m, h), 0)
    # h > 256, m > 32, d < m, a zero dimension
    pair(lambda: L.rq_encode_pq(p(out), p(Xf), p(C), n, d, m, 257), lambda: L.rq_encode_pq_bytes(p(out), p(X), p(C), n, d, m, 257),
         RQ_EUNSUPPORTED)
    pair(lambda: L.rq_encode_pq_i16(p(out16), p(Xf), p(C), n, d, m, 257),
         lambda: L.rq_encode_pq_bytes_i16(p(out16), p(X), p(C), n, d, m, 257), RQ_EUNSUPPORTED)
    pair(lambda: L.rq_encode_pq(p(out), p(Xf), p(C), 2, 64, 33, 4), lambda: L.rq_encode_pq_bytes(p(out), p(X), p(C), 2, 64, 33, 4),
         RQ_EUNSUPPORTED)
    pair(lambda: L.rq_encode_pq(p(out), p(Xf), p(C), n, 2, 4, 4), lambda: L.rq_encode_pq_bytes(p(out), p(X), p(C), n, 2, 4, 4),
         RQ_EINVAL)
    pair(lambda: L.rq_encode_pq(p(out), p(Xf), p(C), n, d, 0, h), lambda: L.rq_encode_pq_bytes(p(out), p(X), p(C), n, d, 0, h),
         RQ_EINVAL)
    assert (out == 0x5A).all() and (out16 == -3).all()
    # NULL data pointers: the byte entries refuse them (the f32 entries do not look)
    assert L.rq_encode_pq_bytes(None, p(X), p(C), n, d, m, h) == RQ_EINVAL
    assert L.rq_encode_pq_bytes(p(out), None, p(C), n, d, m, h) == RQ_EINVAL
    assert L.rq_encode_pq_bytes(p(out), p(X), None, n, d, m, h) == RQ_EINVAL
    assert L.rq_encode_opq_bytes_i16(p(out16), None, p(R), p(C), n, d, m, h) == RQ_EINVAL
    assert not L.rq_dataset_upload_bytes(None, n, d) and not L.rq_dataset_upload_bytes(p(X), 0, d)
    assert b"bad arguments" in L.rq_last_error()
    # device entries
    tX, tC, tR = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda(), torch.from_numpy(R).cuda()
    tXf = tX.float()
    tout = torch.full((n, m), sc.SENTINEL, dtype=torch.uint8, device="cuda")
    q = lambda t: t.data_ptr()         # noqa: E731
    pair(lambda: L.rq_dev_encode_pq(q(tout), q(tXf), q(tC), n, d, m, 257, None),
         lambda: L.rq_dev_encode_pq_bytes(q(tout), q(tX), q(tC), n, d, m, 257, None), RQ_EUNSUPPORTED)
    pair(lambda: L.rq_dev_encode_pq(q(tout), q(tXf), q(tC), 0, d, m, h, None),
         lambda: L.rq_dev_encode_pq_bytes(q(tout), q(tX), q(tC), 0, d, m, h, None), 0)
    pair(lambda: L.rq_dev_encode_pq(q(tout), q(tXf), q(tC), n, 2, 4, 4, None),
         lambda: L.rq_dev_encode_pq_bytes(q(tout), q(tX), q(tC), n, 2, 4, 4, None), RQ_EINVAL)
    assert L.rq_dev_encode_opq_bytes(q(tout), q(tX), None, q(tC), n, d, m, h, None) == RQ_EINVAL
    assert L.rq_dev_encode_pq_bytes(q(tout), None, q(tC), n, d, m, h, None) == RQ_EINVAL
    assert L.rq_dev_rotate_T_bytes(None, q(tR), q(tX), d, n, None) == RQ_EINVAL
    assert L.rq_dev_rotate_T_bytes(q(tout), q(tR), q(tX), d, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((tout == sc.SENTINEL).all())
