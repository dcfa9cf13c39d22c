"""GPU: quantize_pq / quantize_opq of BYTE rows and of resident datasets with more than 256 codewords per codebook
(rq_encode_pq_bytes_wide, rq_encode_opq_bytes_wide, rq_dataset_encode_wide).  u8 -> f32 is exact, so the
expected value is rq_encode_{pq,opq}_wide on X.astype(float32) (tests/test_gpu_encode_wide.py pins those to the oracle), bit for
bit; one shape is also checked against the committed encode oracle merged block by block (tests/wide_oracle.py)."""
import numpy as np
import pytest

import wide_oracle as wo

pytestmark = pytest.mark.gpu

RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2
KERNEL = "encode_h16_kernel"
N = 777          # the tile group is 256 rows: three groups, the last partial, its last tile partial (9 rows)


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _p(a):
    return None if a is None else a.ctypes.data


def _ran():
    return (_L().rq_last_encode_kernel() or b"").decode()


def _at_offset(X, off):
    """A copy of X whose first byte lies `off` bytes into a 64-byte aligned buffer."""
    buf = np.zeros(X.size + 64 + off, dtype=np.uint8)
    start = (-buf.ctypes.data) % 64 + off
    view = buf[start:start + X.size].reshape(X.shape)
    view[...] = X
    assert view.ctypes.data % 64 == off and view.flags["C_CONTIGUOUS"]
    return view


def _f32_wide(Xf, R, Ccat, m, h, code_base=0):
    n, d = Xf.shape
    out = np.full((n, m), -7, np.int16)
    if R is None:
        st = _L().rq_encode_pq_wide(_p(out), _p(Xf), _p(Ccat), n, d, m, h, code_base)
    else:
        st = _L().rq_encode_opq_wide(_p(out), _p(Xf), _p(R), _p(Ccat), n, d, m, h, code_base)
    assert st == 0, _L().rq_last_error()
    return out


def _u8_wide(X, R, Ccat, m, h, code_base=0):
    n, d = X.shape
    out = np.full((n, m), -7, np.int16)
    if R is None:
        st = _L().rq_encode_pq_bytes_wide(_p(out), _p(X), _p(Ccat), n, d, m, h, code_base)
    else:
        st = _L().rq_encode_opq_bytes_wide(_p(out), _p(X), _p(R), _p(Ccat), n, d, m, h, code_base)
    assert st == 0, _L().rq_last_error()
    return out


def _codebooks(X, m, h, seed):
    """Sampled from the data (exact hits and, where h > n, duplicated codewords: ties), jittered on every other codeword."""
    n, d = X.shape
    rng = np.random.default_rng(seed)
    off = wo.splitarray(d, m)
    parts = []
    for i in range(m):
        c = X[rng.integers(0, n, h), off[i]:off[i + 1]].astype(np.float32)
        c[1::2] += rng.standard_normal(c[1::2].shape).astype(np.float32) * np.float32(3)
        parts.append(c.reshape(-1))
    return np.concatenate(parts)


def _bytes(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (n, d), dtype=np.uint8)
    X[0], X[1] = 0, 255
    return X


def _diff(got, ref):
    return "rows differ: %d of %d" % (int((got != ref).any(axis=1).sum()), ref.shape[0])


SHAPES = [  # d, m, h
    (128, 8, 257),     # a block with ONE live codeword
    (128, 8, 1024),
    (96, 16, 1024),    # sub = 6: padded dimensions, 2-byte loads
    (30, 4, 300),      # sub 8, 8, 7, 7: odd byte offsets, single-byte loads
    (40, 1, 300),      # three k-chunks: the slice is re-read per codeword block
]


@pytest.mark.parametrize("d,m,h", SHAPES)
def test_pq_bytes_equal_the_widened_rows(rq, d, m, h):
    X = _bytes(N, d, seed=d + m + h)
    Ccat = _codebooks(X, m, h, seed=h)
    ref = _f32_wide(X.astype(np.float32), None, Ccat, m, h)
    assert _ran() == KERNEL
    for off in (0, 1, 3):
        for base in (0, 1):
            got = _u8_wide(_at_offset(X, off), None, Ccat, m, h, base)
            assert _ran() == KERNEL
            assert np.array_equal(got, ref + base), (off, base, _diff(got, ref + base))


def test_against_the_encode_oracle(rq, oracle):
    d, m, h = 30, 4, 300
    X = _bytes(N, d, seed=1)
    Ccat = _codebooks(X, m, h, seed=2)
    ref = wo.encode_pq_wide(oracle, X.astype(np.float32), Ccat, m, h)
    got = _u8_wide(_at_offset(X, 1), None, Ccat, m, h)
    assert np.array_equal(got, ref), _diff(got, ref)


def test_h_up_to_256_equals_the_byte_entry_widened(rq):
    d, m, h = 128, 8, 200
    X = _bytes(N, d, seed=200)
    Ccat = _codebooks(X, m, h, seed=201)
    u8 = np.full((N, m), 0x5A, np.uint8)
    assert _L().rq_encode_pq_bytes(_p(u8), _p(X), _p(Ccat), N, d, m, h) == 0
    byte_kernel = _ran()
    for base in (0, 1):
        got = _u8_wide(X, None, Ccat, m, h, base)
        assert _ran() == byte_kernel != KERNEL
        assert np.array_equal(got, u8.astype(np.int16) + base)
    R = np.linalg.qr(np.random.default_rng(5).standard_normal((d, d)))[0].astype(np.float32)
    assert _L().rq_encode_opq_bytes(_p(u8), _p(X), _p(R), _p(Ccat), N, d, m, h) == 0
    assert np.array_equal(_u8_wide(X, R, Ccat, m, h), u8.astype(np.int16))


def test_a_codeword_duplicated_256_places_on_loses(rq):
    """Byte data gives exact ties: codeword k again at k + 256 (and k + 512), and rows equal to it -- the lower index wins."""
    d, m, h0 = 32, 4, 256
    X = _bytes(N, d, seed=9)
    sub = d // m
    C0 = _codebooks(X, m, h0, seed=10)
    for i in range(m):                                   # rows 2.. are codewords themselves (distance 0 at k and k + 256)
        blk = C0[i * h0 * sub:(i + 1) * h0 * sub].reshape(h0, sub)
        blk[:] = X[2:2 + h0, i * sub:(i + 1) * sub]
    for copies in (2, 3):
        Cw = np.concatenate([np.tile(C0[i * h0 * sub:(i + 1) * h0 * sub], copies) for i in range(m)])
        got = _u8_wide(_at_offset(X, 3), None, Cw, m, h0 * copies)
        assert _ran() == KERNEL
        assert got.max() < 256
        assert np.array_equal(got, _f32_wide(X.astype(np.float32), None, Cw, m, h0 * copies))
        hits = got[2:2 + h0]
        first = np.array([[int(np.flatnonzero((X[2:2 + h0, i * sub:(i + 1) * sub] == X[r, i * sub:(i + 1) * sub]).all(1))[0])
                           for i in range(m)] for r in range(2, 2 + h0)])
        assert np.array_equal(hits, first)


@pytest.mark.parametrize("value", [0, 255])
def test_constant_bases(rq, value):
    d, m, h = 96, 16, 1024
    X = np.full((N, d), value, np.uint8)
    Ccat = _codebooks(_bytes(N, d, seed=3), m, h, seed=4)
    got = _u8_wide(X, None, Ccat, m, h)
    assert np.array_equal(got, _f32_wide(X.astype(np.float32), None, Ccat, m, h))
    assert (got == got[0]).all()


@pytest.mark.parametrize("d,m,h", [(128, 8, 1024), (40, 4, 300)])
def test_opq_bytes(rq, d, m, h):
    """d = 128: the byte-loading rotation; d = 40: widen, then the f32 rotation."""
    X = _bytes(N, d, seed=d)
    Ccat = _codebooks(X, m, h, seed=h + 1)
    R = np.linalg.qr(np.random.default_rng(d).standard_normal((d, d)))[0].astype(np.float32)
    ref = _f32_wide(X.astype(np.float32), R, Ccat, m, h)
    for off, base in [(0, 0), (1, 1), (3, 0)]:
        got = _u8_wide(_at_offset(X, off), R, Ccat, m, h, base)
        assert _ran() == KERNEL
        assert np.array_equal(got, ref + base), (off, base, _diff(got, ref + base))


def test_datasets_of_both_kinds(rq):
    """One upload, two codebooks (and a rotation): rq_dataset_encode_wide on a u8 and on an f32 base equal the host entry."""
    d, m = 128, 8
    X = _bytes(N, d, seed=77)
    Xf = X.astype(np.float32)
    R = np.linalg.qr(np.random.default_rng(7).standard_normal((d, d)))[0].astype(np.float32)
    books = [(h, _codebooks(X, m, h, seed=h)) for h in (1024, 300, 200)]
    L = _L()
    for data, upload in ((X, L.rq_dataset_upload_bytes), (Xf, L.rq_dataset_upload)):
        ds = upload(_p(data), N, d)
        assert ds
        try:
            for h, Ccat in books:
                for Rm in (None, R):
                    for base in (0, 1):
                        out = np.full((N, m), -7, np.int16)
                        assert L.rq_dataset_encode_wide(ds, _p(out), _p(Rm), _p(Ccat), m, h, base) == 0, L.rq_last_error()
                        ref = _u8_wide(X, Rm, Ccat, m, h, base)
                        assert np.array_equal(out, ref), (data.dtype, h, Rm is not None, base, _diff(out, ref))
        finally:
            L.rq_dataset_free(ds)


def test_python_mirrors(rq, tmp_path):
    d, m, h = 30, 4, 300
    X = _bytes(N, d, seed=30)
    Xf = X.astype(np.float32)
    Ccat = _codebooks(X, m, h, seed=31)
    Cs, _ = wo.sub_codebooks(Ccat, d, m, h)
    R = np.linalg.qr(np.random.default_rng(3).standard_normal((d, d)))[0].astype(np.float32)
    pq, opq = rq.quantize_pq_u16(Xf, Cs), rq.quantize_opq_u16(Xf, R, Cs)
    assert pq.dtype == np.uint16
    assert np.array_equal(rq.quantize_pq_u16(X, Cs), pq) and np.array_equal(rq.quantize_opq_u16(X, R, Cs), opq)
    for data in (X, Xf):
        with rq.Dataset(data) as ds:
            assert np.array_equal(ds.quantize_u16(Cs), pq) and np.array_equal(ds.quantize_u16(Cs, R=R), opq)
            one = ds.quantize_u16(Cs, one_based=True)
            assert one.dtype == np.int16 and np.array_equal(one, pq.astype(np.int16) + 1)
    fn = str(tmp_path / "base.bvecs")
    rq.bvecs_write(X, fn)
    out = rq.quantize_bvecs(fn, Cs, rows_per_read=300)
    assert out.dtype == np.int16 and np.array_equal(out, pq.view(np.int16))
    out = rq.quantize_bvecs(fn, Cs, R=R, bounds=(11, 700), rows_per_read=256, one_based=True)
    assert np.array_equal(out, opq.view(np.int16)[10:700] + 1)
    with pytest.raises(ValueError, match="h <= 256"):          # the one-based spellings keep refusing byte rows at h > 256
        rq.quantize_pq(X, Cs)


def test_two_upload_chunks(rq):
    """d = 1024: 32768 rows per chunk, so 32768 + 33 rows (33 MB) run the host entry's chunk loop twice; OPQ also runs the
    device chunk loop of the rotation (d = 1024 takes the widen fallback)."""
    from rayuela_jl_amd.utils import encode_chunk_rows
    d, m, h = 1024, 8, 300
    n = encode_chunk_rows(d) + 33
    assert n == 32768 + 33
    X = _bytes(n, d, seed=1024)
    Ccat = _codebooks(X[:4000], m, h, seed=5)
    Xf = X.astype(np.float32)
    got = _u8_wide(_at_offset(X, 1), None, Ccat, m, h)
    ref = _f32_wide(Xf, None, Ccat, m, h)
    assert np.array_equal(got, ref), _diff(got, ref)
    ds = _L().rq_dataset_upload_bytes(_p(X), n, d)
    assert ds
    try:
        R = np.linalg.qr(np.random.default_rng(1).standard_normal((d, d)))[0].astype(np.float32)
        out = np.full((n, m), -7, np.int16)
        assert _L().rq_dataset_encode_wide(ds, _p(out), _p(R), _p(Ccat), m, h, 0) == 0, _L().rq_last_error()
    finally:
        _L().rq_dataset_free(ds)
    ref = _f32_wide(Xf, R, Ccat, m, h)
    assert np.array_equal(out, ref), _diff(out, ref)


def test_argument_errors_leave_the_output_untouched(rq):
    L = _L()
    n, d, m, h = 64, 16, 4, 300
    X = _bytes(n, d, seed=0)
    C = np.zeros(h * d, np.float32)
    Cbig = np.zeros(1, np.float32)             # never read: the shape is refused first
    R = np.eye(d, dtype=np.float32)
    out = np.full((n, 33), 0x5A5A, np.int16)
    ds = L.rq_dataset_upload_bytes(_p(X), n, d)
    assert ds

    def refused(call, status):
        assert call() == status, (status, L.rq_last_error())
        assert L.rq_last_error() != b"" and (out == 0x5A5A).all()

    def pq(X_, C_, d_, m_, h_, b):
        return L.rq_encode_pq_bytes_wide(_p(out), _p(X_), _p(C_), n, d_, m_, h_, b)

    def opq(X_, C_, d_, m_, h_, b):
        return L.rq_encode_opq_bytes_wide(_p(out), _p(X_), _p(R), _p(C_), n, d_, m_, h_, b)

    def dse(C_, m_, h_, b):
        return L.rq_dataset_encode_wide(ds, _p(out), None, _p(C_), m_, h_, b)

    try:
        for host in (pq, opq):
            refused(lambda: host(None, C, d, m, h, 0), RQ_EINVAL)               # a NULL pointer
            refused(lambda: host(X, None, d, m, h, 0), RQ_EINVAL)
            refused(lambda: host(X, C, d, m, h, 2), RQ_EINVAL)                  # a bad code_base
            refused(lambda: host(X, C, d, m, h, -1), RQ_EINVAL)
            refused(lambda: host(X, C, 3, m, h, 0), RQ_EINVAL)                  # d < m
            refused(lambda: host(X, Cbig, d, m, 32768, 0), RQ_EUNSUPPORTED)     # h > 32767
            refused(lambda: host(X, Cbig, 66, 33, h, 0), RQ_EUNSUPPORTED)       # m = 33
        refused(lambda: dse(None, m, h, 0), RQ_EINVAL)
        refused(lambda: dse(C, m, h, 2), RQ_EINVAL)
        refused(lambda: dse(C, 17, h, 0), RQ_EINVAL)                            # d = 16 < m
        refused(lambda: dse(Cbig, m, 32768, 0), RQ_EUNSUPPORTED)
        refused(lambda: dse(Cbig, 33, h, 0), RQ_EUNSUPPORTED)
        refused(lambda: L.rq_encode_pq_bytes_wide(None, _p(X), _p(C), n, d, m, h, 0), RQ_EINVAL)
        refused(lambda: L.rq_encode_opq_bytes_wide(_p(out), _p(X), None, _p(C), n, d, m, h, 0), RQ_EINVAL)
        refused(lambda: L.rq_dataset_encode_wide(None, _p(out), None, _p(C), m, h, 0), RQ_EINVAL)
        refused(lambda: L.rq_dataset_encode_wide(ds, None, None, _p(C), m, h, 0), RQ_EINVAL)
    finally:
        L.rq_dataset_free(ds)
