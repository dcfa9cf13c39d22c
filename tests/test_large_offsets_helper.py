"""CPU: the periodic-base helper of tests/large_offsets.py cannot pass vacuously -- it accepts a correct array and rejects one
wrong element wherever it is planted (last row, first row of the ragged tail, just past a scaled-down threshold), on the numpy
path and on the torch path (CPU tensors run the code the GPU tests run on the device), for every dtype the GPU tests compare."""
import numpy as np
import pytest

import large_offsets as lo

PERIOD = 13                                # a scaled-down prime period
MARKS = (40, 20, 80)                       # scaled-down thresholds, in the order of an f32 array's: bytes first
N = MARKS[2] + PERIOD + 13                 # 106 rows: 8 periods and a tail of 2, no multiple of 32
DTYPES = ["uint8", "int16", "int32", "float32", "float64"]


def _tile(dtype, width):
    rng = np.random.default_rng(5)
    shape = (PERIOD,) if width == 0 else (PERIOD, width)
    if "float" in dtype:
        return rng.standard_normal(shape).astype(dtype)
    return rng.integers(0, 100, shape).astype(dtype)


def _both(tile):
    import torch
    return [("numpy", tile), ("torch", torch.from_numpy(tile.copy()))]


def _plant(a, row, width):
    """One wrong element in `row`: the lowest bit of its last element flips."""
    flat = a.reshape(a.shape[0], -1)
    col = max(width, 1) - 1
    if lo._is_torch(a):
        v = lo._int_view(flat)
        v[row, col] = v[row, col] ^ 1
    else:
        v = lo._int_view(flat)
        v[row, col] ^= 1


def test_thresholds():
    assert lo.thresholds(128, 4) == (1 << 24, 1 << 23, 1 << 25)
    assert lo.thresholds(128, 1) == (1 << 24, 1 << 25, 1 << 25)
    assert lo.thresholds(960, 4) == (2236963, 1118482, 4473925)
    for d, size in ((128, 4), (128, 1), (960, 4), (30, 4), (7, 2)):
        e31, b32, e32 = lo.thresholds(d, size)
        assert (e31 - 1) * d < lo.TWO31 <= e31 * d
        assert (b32 - 1) * d * size < lo.TWO32 <= b32 * d * size
        assert (e32 - 1) * d < lo.TWO32 <= e32 * d
    assert lo.P == 4099 and lo.P_SHORT == 1031
    for p in (lo.P, lo.P_SHORT, PERIOD):
        assert all(p % q for q in range(2, int(p ** 0.5) + 1)), "%d is not prime" % p
    for t in lo.thresholds(128, 4) + lo.thresholds(960, 4):
        for p in (lo.P, lo.P_SHORT):
            n = lo.rows_past(t, p)
            assert n == t + p + 13 and n % 32 and n % p


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [0, 1, 5])
def test_periodic_repeats_the_tile(dtype, width):
    for kind, tile in _both(_tile(dtype, width)):
        a = lo.periodic(tile, N)
        assert a.shape[0] == N and tuple(a.shape[1:]) == tuple(tile.shape[1:]) and lo._is_torch(a) == (kind == "torch")
        host = a.numpy() if kind == "torch" else a
        ref = tile.numpy() if kind == "torch" else tile
        for i in range(N):
            assert np.array_equal(host[i], ref[i % PERIOD])
        lo.assert_periodic(a, tile, N, MARKS)
        lo.assert_periodic(lo.periodic(tile, 5), tile, 5)                  # fewer rows than one period: tail only


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [0, 1, 5])
@pytest.mark.parametrize("row,beyond", [(N - 1, "2^32 elements"), (N - N % PERIOD, "2^32 elements"), (MARKS[0] + 1, "2^31 elements, 2^32 bytes"),
                                        (MARKS[1], "past 2^32 bytes"),
                                        (MARKS[2], "2^32 elements"), (0, "before every threshold"), (PERIOD, "before every")])
def test_one_wrong_element_is_found(dtype, width, row, beyond):
    for kind, tile in _both(_tile(dtype, width)):
        a = lo.periodic(tile, N)
        _plant(a, row, width)
        with pytest.raises(AssertionError) as e:
            lo.assert_periodic(a, tile, N, MARKS, what=kind)
        msg = str(e.value)
        assert "1 of %d rows" % N in msg and "first wrong row %d " % row in msg and beyond in msg, msg
        if row == MARKS[0] + 1:
            assert "2^32 elements" not in msg, msg                          # not beyond the last threshold


def test_chunked_comparison_finds_errors_in_every_chunk(monkeypatch):
    """With a chunk of one period per step the body loop runs once per repeat: the count and the first row stay right."""
    monkeypatch.setattr(lo, "_CHUNK_ELEMS", 1)
    for kind, tile in _both(_tile("float32", 5)):
        a = lo.periodic(tile, N)
        lo.assert_periodic(a, tile, N)
        for row in (3 * PERIOD + 2, 5 * PERIOD, N - 1):
            _plant(a, row, 5)
        with pytest.raises(AssertionError, match="3 of %d rows differ.*first wrong row %d " % (N, 3 * PERIOD + 2)):
            lo.assert_periodic(a, tile, N)


def test_floats_compare_as_bits():
    for kind, tile in _both(np.zeros((PERIOD, 2), dtype=np.float32)):
        a = lo.periodic(tile, N)
        a[N - 1, 1] = -0.0                                                   # equal as a float, another bit pattern
        with pytest.raises(AssertionError, match="first wrong row %d " % (N - 1)):
            lo.assert_periodic(a, tile, N)
    nan = np.full((PERIOD, 2), np.nan, dtype=np.float32)
    for kind, tile in _both(nan):
        a = lo.periodic(tile, N)
        lo.assert_periodic(a, tile, N)                                      # the same NaN bits are equal
        v = lo._int_view(a)
        v[7, 0] = v[7, 0] ^ 1                                               # another NaN payload
        with pytest.raises(AssertionError, match="first wrong row 7 "):
            lo.assert_periodic(a, tile, N)


def test_shape_and_dtype_mismatches_are_errors():
    tile = _tile("float32", 5)
    a = lo.periodic(tile, N)
    with pytest.raises(AssertionError):
        lo.assert_periodic(a[:N - 1], tile, N)
    with pytest.raises(AssertionError):
        lo.assert_periodic(a.astype(np.float64), tile, N)
    with pytest.raises(AssertionError):
        lo.assert_periodic(a[:, :4], tile, N)


def test_sentinel_row_guard():
    import torch
    for dtype in (torch.uint8, torch.int16, torch.int32, torch.float32, torch.float64):
        out = lo.output(N, (3,), dtype, device="cpu")
        assert out.shape == (N + 1, 3)
        out[:N] = 1
        lo.assert_sentinel(out, N)
        out[N, 2] = 1
        with pytest.raises(AssertionError, match="spare row"):
            lo.assert_sentinel(out, N)
    out = lo.output(N, (), torch.float32, device="cpu")
    lo.assert_sentinel(out, N)
    out[N] = 0.0
    with pytest.raises(AssertionError):
        lo.assert_sentinel(out, N)
