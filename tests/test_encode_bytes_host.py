"""CPU: the host side of the byte-input encode (bvecs data, src/xvecs_read.jl:14-52): bvecs_write / bvecs_read, the dtype
dispatch of the mirrors (uint8 -> the *_bytes entry points, float64 still a TypeError) and quantize_bvecs' piecewise reading,
against a recording stand-in for the library (no device is touched)."""
import numpy as np
import pytest

import bytes_stream_cases  # noqa: F401  (completes the table that tests/test_gpu_streams.py checks against the header)


class _Recorder:
    """Stands in for the ctypes library: every rq_* call is recorded and succeeds (an upload returns a non-null handle)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("rq_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 1 if name.startswith("rq_dataset_upload") else 0
        return call

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def fake(monkeypatch, rq):
    from rayuela_jl_amd import _lib
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def _data(n=6, d=8, m=2, h=4, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (n, d), dtype=np.uint8)
    C = [rng.standard_normal((h, d // m)).astype(np.float32) for _ in range(m)]
    R = np.eye(d, dtype=np.float32)
    return X, C, R


def test_bvecs_round_trip_and_bounds(tmp_path, rq):
    rng = np.random.default_rng(1)
    X = rng.integers(0, 256, (37, 13), dtype=np.uint8)
    X[0], X[1] = 0, 255
    fn = str(tmp_path / "x.bvecs")
    rq.bvecs_write(X, fn)
    raw = np.fromfile(fn, dtype=np.uint8)
    assert raw.size == 37 * (4 + 13)                                   # int32 d, then d bytes, per vector
    assert (raw.reshape(37, 17)[:, :4].copy().view("<i4") == 13).all()
    got = rq.bvecs_read(None, fn)
    assert got.dtype == np.uint8 and np.array_equal(got, X)
    assert np.array_equal(rq.bvecs_read(5, fn), X[:5])                 # first n
    assert np.array_equal(rq.bvecs_read((4, 20), fn), X[3:20])         # one-based inclusive range
    assert np.array_equal(rq.bvecs_read((37, 37), fn), X[36:])
    with pytest.raises(EOFError):
        rq.bvecs_read((30, 38), fn)
    with pytest.raises(TypeError):
        rq.bvecs_write(X.astype(np.float32), fn)
    with pytest.raises(TypeError):
        rq.bvecs_write(X[0], fn)


def test_uint8_data_reaches_the_byte_entry_points(fake, rq):
    X, C, R = _data()
    Xf = X.astype(np.float32)
    B = rq.quantize_pq(X, C)
    assert B.dtype == np.int16 and B.shape == (6, 2)
    rq.quantize_pq(Xf, C)
    rq.quantize_pq_u8(X, C)
    rq.quantize_pq_u8(Xf, C)
    rq.quantize_opq(X, R, C)
    rq.quantize_opq(Xf, R, C)
    assert fake.names() == ["rq_encode_pq_bytes_i16", "rq_encode_pq_i16", "rq_encode_pq_bytes", "rq_encode_pq",
                            "rq_encode_opq_bytes_i16", "rq_encode_opq_i16"]
    for name, args in fake.calls:                                      # (..., n, d, m, h)
        assert tuple(args[-4:]) == (6, 8, 2, 4), (name, args)
    # a non-contiguous uint8 view is made contiguous, not widened
    fake.calls.clear()
    rq.quantize_pq_u8(np.asfortranarray(X), C)
    assert fake.names() == ["rq_encode_pq_bytes"]


def test_other_dtypes_are_still_refused(fake, rq):
    X, C, R = _data()
    for bad in (np.float64, np.int8, np.int32, np.uint16, np.float16):
        with pytest.raises(TypeError):      # Float64 data never dispatches in the reference (src/PQ.jl:32)
            rq.quantize_pq(X.astype(bad), C)
        with pytest.raises(TypeError):
            rq.quantize_pq_u8(X.astype(bad), C)
        with pytest.raises(TypeError):
            rq.quantize_opq(X.astype(bad), R, C)
        with pytest.raises(TypeError):
            rq.index.Dataset(X.astype(bad))
    with pytest.raises(TypeError):          # the rotation and the codebooks stay float32
        rq.quantize_opq(X, R.astype(np.uint8), C)
    with pytest.raises(TypeError):
        rq.quantize_pq(X, [c.astype(np.uint8) for c in C])
    assert fake.calls == []


def test_dataset_uploads_bytes_as_bytes(fake, rq):
    X, C, R = _data()
    ds = rq.index.Dataset(X)
    ds.quantize(C)
    ds.quantize(C, R=R, one_based=False)
    ds.close()                              # (while the stand-in is in place: the handle is not a real one)
    df = rq.index.Dataset(X.astype(np.float32))
    df.close()
    assert fake.names() == ["rq_dataset_upload_bytes", "rq_dataset_encode", "rq_dataset_encode", "rq_dataset_free",
                            "rq_dataset_upload", "rq_dataset_free"]
    assert tuple(fake.calls[0][1][1:]) == (6, 8)


def test_quantize_bvecs_reads_and_encodes_piecewise(fake, tmp_path, rq):
    from rayuela_jl_amd import xvecs
    X, C, R = _data(n=50)
    fn = str(tmp_path / "base.bvecs")
    xvecs.bvecs_write(X, fn)
    out = xvecs.quantize_bvecs(fn, C, rows_per_read=16)
    assert out.shape == (50, 2) and out.dtype == np.uint8
    assert [(c[0], c[1][3]) for c in fake.calls] == [("rq_encode_pq_bytes", 16)] * 3 + [("rq_encode_pq_bytes", 2)]
    # every piece lands in its own rows of the result
    assert [c[1][0] - out.ctypes.data for c in fake.calls] == [0, 16 * 2, 32 * 2, 48 * 2]
    fake.calls.clear()
    out = xvecs.quantize_bvecs(fn, C, R=R, bounds=(11, 40), rows_per_read=16, one_based=True)
    assert out.shape == (30, 2) and out.dtype == np.int16
    assert [(c[0], c[1][4]) for c in fake.calls] == [("rq_encode_opq_bytes_i16", 16), ("rq_encode_opq_bytes_i16", 14)]
    fake.calls.clear()
    assert xvecs.quantize_bvecs(fn, C, bounds=7).shape == (7, 2)
    assert [(c[0], c[1][3]) for c in fake.calls] == [("rq_encode_pq_bytes", 7)]
    for bad in ((0, 5), (45, 51), (9, 8)):
        with pytest.raises(ValueError):
            xvecs.quantize_bvecs(fn, C, bounds=bad)
    with pytest.raises(ValueError):
        xvecs.quantize_bvecs(fn, C[:1])                  # codebooks that do not tile d
    with pytest.raises(ValueError):
        xvecs.quantize_bvecs(fn, C, R=np.eye(4, dtype=np.float32))


def test_chunk_row_rule():
    """Rows per upload chunk, bytes and f32 alike: max(32768, 2^25 / d) -- 32 MiB of bytes where f32 moves 128 MiB."""
    from rayuela_jl_amd.utils import encode_chunk_rows
    assert encode_chunk_rows(128) == 262144 and encode_chunk_rows(96) == 349525 and encode_chunk_rows(512) == 65536
    assert encode_chunk_rows(1024) == 32768 and encode_chunk_rows(4096) == 32768 and encode_chunk_rows(1) == 1 << 25
    for d in (1, 3, 30, 96, 128, 960, 5000):
        assert encode_chunk_rows(d) == max(32768, (1 << 27) // (d * 4))          # the f32 path's expression
