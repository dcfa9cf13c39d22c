"""Periodic bases for tests whose arrays pass 2^31 elements or 2^32 bytes -- a plain helper module: no fixtures, no pytest hooks.

A row-wise operation on an array that repeats a short period of P rows gives, at row i, the result of period row i % P.  The
expected P rows come from a CPU restatement; the n rows of the device (or host) result are then all checked, not a sample.
P = 4099 is prime: the period boundaries drift against every tile, wavefront, block and chunk boundary a kernel has.  Slow
restatements (ICM, Viterbi at d = 960) take the shorter prime P_SHORT = 1031.

  thresholds(d, itemsize)          the first rows whose first element has index >= 2^31, byte offset >= 2^32, index >= 2^32
  rows_past(threshold, P)          n = threshold + P + 13: past the crossing, ragged against P, no multiple of 32
  periodic(tile, n)                the n-row array: torch tensor in, torch tensor (same device) out; numpy in, numpy out
  output(n, tail, dtype, device)   an output of n + 1 rows whose spare last row holds a sentinel
  assert_sentinel(out, n)          the spare row still holds it
  assert_periodic(out, tile, n)    out[i] == tile[i % P] for every i < n, bit for bit (floats as int32 / int64 views)
"""
import numpy as np

P = 4099
P_SHORT = 1031
TWO31 = 1 << 31
TWO32 = 1 << 32
NAMES = ("2^31 elements", "2^32 bytes", "2^32 elements")
_CHUNK_ELEMS = 1 << 27                    # elements compared per step of assert_periodic: bounds its temporaries


def _first_row(limit, per_row):
    return -(-limit // per_row)


def thresholds(d, itemsize):
    """(first row with row * d >= 2^31, first row with row * d * itemsize >= 2^32, first row with row * d >= 2^32)."""
    return _first_row(TWO31, d), _first_row(TWO32, d * itemsize), _first_row(TWO32, d)


def rows_past(threshold, period=P):
    n = threshold + period + 13
    assert n % period and n % 32
    return n


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def periodic(tile, n):
    """tile [P][...] repeated down n rows (the last repeat is cut)."""
    p = tile.shape[0]
    reps, tail = divmod(n, p)
    if not _is_torch(tile):
        return np.resize(np.ascontiguousarray(tile), (n,) + tile.shape[1:])
    import torch
    out = torch.empty((n,) + tuple(tile.shape[1:]), dtype=tile.dtype, device=tile.device)
    if reps:
        out[:reps * p].view((reps,) + tuple(tile.shape)).copy_(tile.unsqueeze(0).expand((reps,) + tuple(tile.shape)))
    if tail:
        out[reps * p:].copy_(tile[:tail])
    return out


def sentinel_of(dtype):
    return -7.0 if "float" in str(dtype) else 0xA5 if "uint8" in str(dtype) else -3


def output(n, tail, dtype, device="cuda"):
    """torch tensor [n + 1][*tail]; rows 0 .. n-1 are uninitialised, row n holds sentinel_of(dtype)."""
    import torch
    out = torch.empty((n + 1,) + tuple(tail), dtype=dtype, device=device)
    out[n:].fill_(sentinel_of(dtype))
    return out


def assert_sentinel(out, n):
    """Nothing was written past row n - 1 of an output(n, ...) buffer."""
    spare = out[n:]
    assert spare.shape[0] == 1, "not an n + 1 row buffer"
    ok = bool((spare == sentinel_of(out.dtype)).all())
    assert ok, "the spare row after row %d was written" % (n - 1)


def _int_view(a):
    """Bit view: floats compare as integers, so NaN payloads and the sign of zero count."""
    name = str(a.dtype).replace("torch.", "")
    if name in ("float32", "float64"):
        if _is_torch(a):
            import torch
            return a.view(torch.int32 if name == "float32" else torch.int64)
        return a.view(np.int32 if name == "float32" else np.int64)
    return a


def _bad_rows(got, want):
    """Row mask of got [..., rows, *tail] != want (broadcast over the leading repeat axis)."""
    ne = got != want
    tail_dims = got.dim() - 2 if _is_torch(got) else got.ndim - 2
    for _ in range(tail_dims):
        ne = ne.any(-1)
    return ne


def assert_periodic(out, tile, n, marks=None, what="output"):
    """out[i] == tile[i % P] for all i in [0, n), bit for bit.  out has at least n rows (a spare sentinel row is ignored); torch
    tensors are compared on their device, numpy arrays in numpy.  marks = thresholds(...) names, in the failure message, the
    thresholds the first wrong row lies at or beyond."""
    p = tile.shape[0]
    assert out.shape[0] >= n and tuple(out.shape[1:]) == tuple(tile.shape[1:]), (tuple(out.shape), tuple(tile.shape), n)
    assert str(out.dtype).replace("torch.", "") == str(tile.dtype).replace("torch.", ""), (out.dtype, tile.dtype)
    torch_side = _is_torch(out)
    if torch_side:
        assert _is_torch(tile) and tile.device == out.device
        assert out.is_contiguous()
    else:
        out = np.ascontiguousarray(out)
    got = _int_view(out[:n]).reshape(n, -1)
    want = _int_view(tile if torch_side else np.ascontiguousarray(tile)).reshape(p, -1)
    width = max(1, got.shape[1])
    reps, tail = divmod(n, p)
    step = max(1, _CHUNK_ELEMS // (p * width))
    nbad, first = 0, None
    for r0 in range(0, reps, step):
        r1 = min(reps, r0 + step)
        bad = _bad_rows(got[r0 * p:r1 * p].reshape(r1 - r0, p, width), want.reshape(1, p, width)).reshape(-1)
        k = int(bad.sum())
        if k:
            nbad += k
            if first is None:
                first = r0 * p + int(bad.nonzero()[0][0] if not torch_side else bad.nonzero()[0, 0])
    if tail:
        bad = _bad_rows(got[reps * p:].reshape(1, tail, width), want[:tail].reshape(1, tail, width)).reshape(-1)
        k = int(bad.sum())
        if k:
            nbad += k
            if first is None:
                first = reps * p + int(bad.nonzero()[0][0] if not torch_side else bad.nonzero()[0, 0])
    if nbad:
        beyond = [] if marks is None else [name for name, row in zip(NAMES, marks) if first >= row]
        where = "at or beyond the first row past " + ", ".join(beyond) if beyond else "before every threshold"
        raise AssertionError("%s: %d of %d rows differ from the period; first wrong row %d (period row %d), %s"
                             % (what, nbad, n, first, first % p, where))
