"""GPU: the encode, rotation, RVQ, beam, ICM, chain, norms and training-reduction kernels on arrays whose element index passes
2^31 and 2^32 and whose byte offset passes 2^32 (tests/large_offsets.py: a short prime period of realistic rows repeated down
the array, so that EVERY output row is checked against the CPU restatement of its period row, bit for bit).

Sizes: n = threshold + P + 13 rows throughout (lo.rows_past), P = 4099, or 1031 where the restatement is slow (d = 960: the
oracle's fmaf chains for beam, Viterbi and ICM).  f32 rows of d = 128, 30, 32 and 960 pass 2^32 elements (17.2 GB); the heavy
per-row kernels at d = 960 pass 2^31 elements, which is 2^33 bytes (8.6 GB); byte rows pass 2^32 bytes (4.3 GB).

Entries whose accepted m cannot bring the codes index row * m + i past 2^31 within 16 GiB of input:
  rq_dev_encode_pq_wide / rq_dev_encode_opq (m <= 32, reached only with d = m = 32 like rq_dev_encode_pq, which is the case
      run here; at d = 128 their row * m stays below 2^29),
  rq_dev_encode_rvq / _rvq_wide / _rvq_beam (m <= 64 full-dimensional stages: 2^31 / 64 rows of d >= 1 floats fit, but a stage
      on d = 1 is no encode; at the d = 128 / 960 run here row * m stays below 2^28),
  rq_dev_quantize_chainq and rq_dev_encode_icm (m <= 16: 2^27 rows; 16 GiB allow that only for d <= 32, where the chain
      parts and the ICM unaries degenerate; run here at d = 960, row * m below 2^24).
rq_dev_aq_norms (m <= 64) and rq_dev_encode_pq (d = m = 32) do pass it and are run past it below.

What the file found: no 32-bit index, but launches of more than 2^32 work-items.  A dispatch that large does not fail, it
wraps and runs the remainder: rq_dev_encode_rvq at d = 30 (one thread per float, n * d = 2^32 + 123 360) returned RQ_OK with
the first 4114 of 143 169 689 rows encoded and the rest untouched.  residual_launch (the RVQ, 16-bit RVQ and ERVQ epilogue),
aq_norms_launch (16 work-items per row: 2^28 rows) and the code-widening kernels now cut their rows into launches of at most
2^31 work-items; test_encode_rvq_scalar_epilogue_all_rows and test_norms_past_the_work_items_of_one_launch pin it.

Section 11 takes the slice planner of the wide centre update (update_centers_launch<int16_t>) to its two caps -- 2^23 rows and 2^30
bytes of X per slice -- and to its refusal; those arrays are 0.5 and 2.1 GB, the limits are the planner's, not an index width.

A GPU test skips only when the device has less free memory than the test needs (never on an MI355X: the file peaks at
32.4 GiB of tensors; 28 tests, 21 s, the slowest 2.9 s)."""
import ctypes

import numpy as np
import pytest

import large_offsets as lo

pytestmark = pytest.mark.gpu

RQ_EINVAL = -1
GB = 1 << 30


def _L():
    from rayuela_jl_amd import _lib
    return _lib.lib()


def _kernel():
    return (_L().rq_last_encode_kernel() or b"").decode()


def _call(name, *args):
    """The C entry `name` on the default stream, then a wait for it.  Tensors pass their pointers, host arrays are uploaded
    first; both stay referenced until the stream has drained (a temporary's block could be handed out again before that)."""
    import torch
    held = [_dev(a) if isinstance(a, np.ndarray) else a for a in args]
    rc = getattr(_L(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in held])
    assert rc == 0, (name, rc, _L().rq_last_error())
    torch.cuda.synchronize()


def _need(nbytes):
    """Skip (with the figures) when the device cannot hold what the test allocates; 1 GiB of slack for the library's scratch."""
    import torch
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes + GB:
        pytest.skip("needs %.1f GiB of device memory, %.1f GiB are free" % ((nbytes + GB) / GB, free / GB))


class _Bases:
    """The periodic bases, one resident at a time: built once per key, dropped when the next key is asked for."""

    def __init__(self):
        self.key, self.val = None, None

    def get(self, key, build):
        import torch
        if self.key != key:
            self.drop()
            self.val = build()
            self.key = key
            torch.cuda.synchronize()
        return self.val

    def drop(self):
        import torch
        self.key, self.val = None, None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def bases(rq):
    import torch
    torch.cuda.reset_peak_memory_stats()
    b = _Bases()
    yield b
    b.drop()
    torch.cuda.synchronize()
    assert _L().rq_release_workspaces() == 0
    torch.cuda.empty_cache()
    print("\npeak device memory of tests/test_gpu_large_offsets.py: %.1f GiB (torch allocator)"
          % (torch.cuda.max_memory_allocated() / GB))


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


_TILES = {}


def _tile(kind, d, period=lo.P):
    """The period rows (host): SIFT-like integer-valued f32, Deep-like f32, or SIFT-like bytes."""
    import rayuela_jl_amd.synth as synth
    key = (kind, d, period)
    if key not in _TILES:
        if kind == "deep":
            _TILES[key] = synth.deep_like(period, d, seed=31)
        else:
            X = synth.sift_like(period, d, seed=31)
            _TILES[key] = X.astype(np.uint8) if kind == "bytes" else X
        _TILES[key].setflags(write=False)
    return _TILES[key]


def _pq_codebooks(tile, m, h, seed=99):
    import rayuela_jl_amd.synth as synth
    return synth.cat_codebooks(synth.codebooks(np.asarray(tile, dtype=np.float32), m, h, seed=seed, iters=1, sample=tile.shape[0]))


def _rvq_codebooks(tile, m, h, seed=99):
    import rayuela_jl_amd.synth as synth
    return synth.rvq_codebooks(np.asarray(tile, dtype=np.float32), m, h, seed=seed, iters=1, sample=min(tile.shape[0], 2048))


def _base(bases, kind, d, n, period=lo.P):
    """Device base of n rows (a longer resident base of the same kind, d and period serves its first n rows)."""
    import torch
    itemsize = 1 if kind == "bytes" else 4
    key = (kind, d, period)
    if bases.key == key and bases.val.shape[0] >= n:
        return bases.val[:n]
    bases.drop()
    _need(n * d * itemsize)
    return bases.get(key, lambda: lo.periodic(_dev(_tile(kind, d, period)), n))[:n]


def _unchanged(X, kind, d, n, marks, period=lo.P):
    lo.assert_periodic(X, _dev(_tile(kind, d, period)), n, marks, what="the input")


# ---- 1. quantize_pq: three kernels, and the codes index past 2^31 -----------------------------------------------------------------
# (d, m, h, period, kernel).  d = 30, m = 3 has even sub-spaces of 10 <= 16 floats: on 8-byte aligned rows the dispatch gives it
# the filter + exact pass like d = 128 (rq_encode.hip: encode_launch), so the LDS-staged kernel is reached by the uneven
# split d = 30, m = 4 (and by d = m = 32) and the streamed-codebook kernel by d = 960.
PQ_SHAPES = [(128, 8, 256, lo.P, "encode_pq_filter_kernel"), (30, 3, 64, lo.P, "encode_pq_filter_kernel"),
             (30, 4, 64, lo.P, "encode_pq_kernel"), (960, 8, 256, lo.P_SHORT, "encode_wide_kernel"),
             (32, 32, 256, lo.P, "encode_pq_kernel")]


def test_pq_shapes_cover_three_kernels():
    assert len({k for _, _, _, _, k in PQ_SHAPES}) == 3


@pytest.mark.parametrize("d,m,h,period,kernel", PQ_SHAPES, ids=lambda v: str(v))
def test_encode_pq_all_rows(rq, oracle, bases, d, m, h, period, kernel):
    """rq_dev_encode_pq; d = m = 32 is the largest m the entry accepts: row * m + i passes 2^31 at row 2^26 and 2^32 at 2^27."""
    import torch
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2], period)
    tile = _tile("sift", d, period)
    C = _pq_codebooks(tile, m, h)
    want = oracle.encode_pq(tile, C, m, h)
    X = _base(bases, "sift", d, n, period)
    _need(n * m + n)
    codes = lo.output(n, (m,), torch.uint8)
    _call("rq_dev_encode_pq", codes, X, C, n, d, m, h, None)
    assert _kernel() == kernel
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_sentinel(codes, n)
    if m == 32:
        assert (n - 1) * m > lo.TWO32                                   # the codes index itself crossed both thresholds
    _unchanged(X, "sift", d, n, marks, period)


# ---- 2. rotation and quantize_opq at d = 128 ------------------------------------------------------------------------------------------
def _opq_case(kind, d=128, m=8, h=256):
    import rayuela_jl_amd.synth as synth
    tile = _tile(kind, d)
    R = synth.rotation(d)
    return tile, R, _pq_codebooks(tile, m, h), m, h


def test_rotate_all_rows(rq, oracle, bases):
    """rq_dev_rotate_T: the 17 GB output crosses the thresholds too."""
    import torch
    d = 128
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    tile, R, _, _, _ = _opq_case("sift")
    want = oracle.rotate_T(R, tile)
    X = _base(bases, "sift", d, n)
    _need((n + 1) * d * 4)
    RX = lo.output(n, (d,), torch.float32)
    _call("rq_dev_rotate_T", RX, R, X, d, n, None)
    lo.assert_periodic(RX, _dev(want), n, marks, what="R'X")
    lo.assert_sentinel(RX, n)
    _unchanged(X, "sift", d, n, marks)


def test_encode_opq_all_rows(rq, oracle, bases):
    import torch
    d = 128
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    tile, R, C, m, h = _opq_case("sift")
    want = oracle.encode_opq(tile, R, C, m, h)
    X = _base(bases, "sift", d, n)
    codes = lo.output(n, (m,), torch.uint8)
    _call("rq_dev_encode_opq", codes, X, R, C, n, d, m, h, None)
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_sentinel(codes, n)
    _unchanged(X, "sift", d, n, marks)


# ---- 3. 16-bit codes ----------------------------------------------------------------------------------------------------------------------
def test_encode_pq_wide_all_rows(rq, oracle, bases):
    """rq_dev_encode_pq_wide, h = 1024: int16 codes out."""
    import torch
    import wide_oracle as wo
    d, m, h = 128, 8, 1024
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    tile = _tile("sift", d)
    C = _pq_codebooks(tile, m, h)
    want = wo.encode_pq_wide(oracle, tile, C, m, h)
    assert int(want.max()) > 255
    X = _base(bases, "sift", d, n)
    codes = lo.output(n, (m,), torch.int16)
    _call("rq_dev_encode_pq_wide", codes, X, C, n, d, m, h, None)
    assert _kernel() == "encode_h16_kernel"
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_sentinel(codes, n)
    _unchanged(X, "sift", d, n, marks)


def _counts_want(tile_codes, h, n):
    """reps x bincount(period) + bincount(tail), per stage, in integers."""
    p, m = tile_codes.shape
    reps, tail = divmod(n, p)
    out = np.zeros((m, h), dtype=np.int64)
    for i in range(m):
        out[i] = reps * np.bincount(tile_codes[:, i].astype(np.int64), minlength=h) \
            + np.bincount(tile_codes[:tail, i].astype(np.int64), minlength=h)
    assert int(out.sum()) == n * m and out.max() < 2 ** 32
    return out


def test_encode_rvq_wide_all_rows(rq, oracle, bases):
    """rq_dev_encode_rvq_wide, m = 2, h = 300: int16 codes, the residual written over X, the per-centre counts."""
    import torch
    import wide_oracle as wo
    d, m, h = 128, 2, 300
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    tile = _tile("sift", d)
    C = _rvq_codebooks(tile, m, h)
    want, _, want_r = wo.encode_rvq_wide(oracle, tile, C)
    assert int(want.max()) > 255
    Xr = _base(bases, "sift", d, n)
    codes = lo.output(n, (m,), torch.int16)
    counts = torch.zeros((m, h), dtype=torch.int32, device="cuda")
    _call("rq_dev_encode_rvq_wide", codes, Xr, C, n, d, m, h, counts, None)
    bases.key = None                                                   # the base now holds the residual: never reused
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_sentinel(codes, n)
    lo.assert_periodic(Xr, _dev(want_r), n, marks, what="residual")
    assert np.array_equal(counts.cpu().numpy().view(np.uint32).astype(np.int64), _counts_want(want, h, n))


def test_encode_rvq_all_rows(rq, oracle, bases):
    """rq_dev_encode_rvq, m = 4, h = 256: codes, the residual written over X, the per-centre counts."""
    import torch
    d, m, h = 128, 4, 256
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    tile = _tile("sift", d)
    C = _rvq_codebooks(tile, m, h)
    want, _, want_r = oracle.encode_rvq(tile, C, with_extras=True)
    Xr = _base(bases, "sift", d, n)
    codes = lo.output(n, (m,), torch.uint8)
    counts = torch.zeros((m, h), dtype=torch.int32, device="cuda")
    _call("rq_dev_encode_rvq", codes, Xr, C, n, d, m, h, counts, None)
    bases.key = None
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_sentinel(codes, n)
    lo.assert_periodic(Xr, _dev(want_r), n, marks, what="residual")
    assert np.array_equal(counts.cpu().numpy().view(np.uint32).astype(np.int64), _counts_want(want, h, n))


@pytest.mark.parametrize("h", [64, 300])
def test_encode_rvq_scalar_epilogue_all_rows(rq, oracle, bases, h):
    """d = 30 is no multiple of 4: the stage epilogue runs one thread per float, n * d = 2^32 + 123 360 of them -- more work-items
    than one launch takes (rq_encode.hip: residual_launch; h = 300: its int16 instantiation).  m = 2."""
    import torch
    import wide_oracle as wo
    d, m = 30, 2
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    assert n * d > lo.TWO32
    tile = _tile("sift", d)
    C = _rvq_codebooks(tile, m, h)
    if h > 256:
        want, _, want_r = wo.encode_rvq_wide(oracle, tile, C)
    else:
        want, _, want_r = oracle.encode_rvq(tile, C, with_extras=True)
    Xr = _base(bases, "sift", d, n)
    codes = lo.output(n, (m,), torch.int16 if h > 256 else torch.uint8)
    counts = torch.zeros((m, h), dtype=torch.int32, device="cuda")
    _call("rq_dev_encode_rvq_wide" if h > 256 else "rq_dev_encode_rvq", codes, Xr, C, n, d, m, h, counts, None)
    bases.key = None
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_sentinel(codes, n)
    lo.assert_periodic(Xr, _dev(want_r), n, marks, what="residual")
    assert np.array_equal(counts.cpu().numpy().view(np.uint32).astype(np.int64), _counts_want(want, h, n))


# ---- 4. byte rows: 2^32 bytes of input, 2^32 elements of rotated output ------------------------------------------------------------------
def test_byte_rows_all_rows(rq, oracle, bases):
    """rq_dev_encode_pq_bytes, rq_dev_encode_opq_bytes and rq_dev_rotate_T_bytes on 2^25 + P + 13 rows of 128 bytes."""
    import torch
    d = 128
    marks = lo.thresholds(d, 1)
    n = lo.rows_past(marks[2])
    tile, R, C, m, h = _opq_case("bytes")
    wide = tile.astype(np.float32)
    X = _base(bases, "bytes", d, n)
    dC, dR = _dev(C), _dev(R)
    codes = lo.output(n, (m,), torch.uint8)
    _call("rq_dev_encode_pq_bytes", codes, X, dC, n, d, m, h, None)
    assert _kernel() == "encode_pq_filter_bytes_kernel"
    lo.assert_periodic(codes, _dev(oracle.encode_pq(wide, C, m, h)), n, marks, what="codes (pq)")
    lo.assert_sentinel(codes, n)
    codes = lo.output(n, (m,), torch.uint8)
    _call("rq_dev_encode_opq_bytes", codes, X, dR, dC, n, d, m, h, None)
    lo.assert_periodic(codes, _dev(oracle.encode_opq(wide, R, C, m, h)), n, marks, what="codes (opq)")
    lo.assert_sentinel(codes, n)
    del codes
    _need((n + 1) * d * 4)
    RX = lo.output(n, (d,), torch.float32)
    _call("rq_dev_rotate_T_bytes", RX, dR, X, d, n, None)
    lo.assert_periodic(RX, _dev(oracle.rotate_T(R, wide)), n, lo.thresholds(d, 4), what="R'X")
    lo.assert_sentinel(RX, n)
    _unchanged(X, "bytes", d, n, marks)


# ---- 5. the heavy per-row kernels at d = 960: past 2^31 elements (and so past 2^32 bytes) ----------------------------------------------------
HEAVY_D = 960


def _heavy(bases):
    marks = lo.thresholds(HEAVY_D, 4)
    n = lo.rows_past(marks[0], lo.P_SHORT)
    assert marks[1] < marks[0] < n
    return marks, n, _tile("sift", HEAVY_D, lo.P_SHORT), _base(bases, "sift", HEAVY_D, n, lo.P_SHORT)


def test_beam_all_rows(rq, bases):
    """rq_dev_encode_rvq_beam, H = 4, m = 2, h = 64: codes, cost and residual; X is only read."""
    import torch
    import beam_oracle as bo
    marks, n, tile, X = _heavy(bases)
    d, m, h, H = HEAVY_D, 2, 64, 4
    C = _rvq_codebooks(tile, m, h)
    want, want_r, want_cost = bo.encode(tile, C, H)
    _need((n + 1) * d * 4)
    codes = lo.output(n, (m,), torch.uint8)
    Xr = lo.output(n, (d,), torch.float32)
    cost = lo.output(n, (), torch.float32)
    _call("rq_dev_encode_rvq_beam", codes, Xr, cost, X, C, n, d, m, h,
                                    H, 1, None)
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_periodic(cost, _dev(want_cost), n, marks, what="cost")
    lo.assert_periodic(Xr, _dev(want_r), n, marks, what="residual")
    for out in (codes, Xr, cost):
        lo.assert_sentinel(out, n)
    _unchanged(X, "sift", d, n, marks, lo.P_SHORT)


def test_chainq_all_rows(rq, oracle, bases):
    """rq_dev_quantize_chainq, m = 4, h = 64, nsplits = 1: the library's own 2 GiB chunking supplies the chunk bases."""
    import torch
    import chain_oracle as co
    marks, n, tile, X = _heavy(bases)
    d, m, h = HEAVY_D, 4, 64
    C = _rvq_codebooks(tile, m, h)
    want = co.viterbi(oracle, tile, C)
    codes = lo.output(n, (m,), torch.uint8)
    _call("rq_dev_quantize_chainq", codes, X, C, n, d, m, h, 1, None)
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_sentinel(codes, n)
    _unchanged(X, "sift", d, n, marks, lo.P_SHORT)


def test_icm_all_rows(rq, oracle, bases):
    """rq_dev_encode_icm with npert = 0, randord = 0, ilsiter = 1, icmiter = 2, nsplits = 1, periodic codes_in.  With npert = 0
    and randord = 0 the kernel draws nothing from its per-row stream (rq_icm.hip: `need` starts at 0, the visit order stays
    the identity), so a row's result is a function of its X row and its start codes alone."""
    import torch
    import icm_oracle as io
    import rayuela_jl_amd.synth as synth
    marks, n, tile, X = _heavy(bases)
    d, m, h = HEAVY_D, 4, 64
    C = _rvq_codebooks(tile, m, h)
    start = (synth.random_codes(lo.P_SHORT, m, seed=5) % h).astype(np.uint8)
    want, want_cost = io.ils(oracle, tile, C, start, 1, 2, 0, 0)
    assert (want != start).any()
    cin = lo.periodic(_dev(start), n)
    codes = lo.output(n, (m,), torch.uint8)
    cost = lo.output(n, (), torch.float32)
    _call("rq_dev_encode_icm", codes, cin, cost, X, C, n, d, m, h,
                               1, 2, 0, 0, 0, 0, 1, None)
    lo.assert_periodic(codes, _dev(want), n, marks, what="codes")
    lo.assert_periodic(cost, _dev(want_cost), n, marks, what="cost")
    lo.assert_sentinel(codes, n)
    lo.assert_sentinel(cost, n)
    lo.assert_periodic(cin, _dev(start), n, marks, what="codes_in")
    _unchanged(X, "sift", d, n, marks, lo.P_SHORT)


# ---- 6. reconstructions: the output crosses the thresholds ----------------------------------------------------------------------------------
def test_reconstruct_all_rows(rq, bases):
    """rq_dev_reconstruct (PQ: sub-vectors side by side) and rq_dev_reconstruct_aq (f32 adds from +0 in codebook order)."""
    import torch
    import rayuela_jl_amd.synth as synth
    from oracle import train_oracle as to
    bases.drop()
    d, m, h = 128, 8, 256
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    tile = _tile("deep", d)
    tcodes = synth.random_codes(lo.P, m, seed=9)
    _need((n + 1) * d * 4 + n * m)
    codes = lo.periodic(_dev(tcodes), n)
    # PQ
    Cl = synth.codebooks(tile, m, h, iters=1, sample=lo.P)
    want = to.reconstruct(Cl, tcodes, to.offsets(d, m), d)
    CB = lo.output(n, (d,), torch.float32)
    _call("rq_dev_reconstruct", CB, codes, synth.cat_codebooks(Cl), n, d, m, h, None)
    lo.assert_periodic(CB, _dev(want), n, marks, what="CB (pq)")
    lo.assert_sentinel(CB, n)
    # additive: full-dimensional codebooks
    C = _rvq_codebooks(tile, m, h)
    want = np.zeros((lo.P, d), dtype=np.float32)
    for i in range(m):
        want = want + C[i][tcodes[:, i].astype(np.int64)]
    CB[n:].fill_(lo.sentinel_of(CB.dtype))
    CB[:n].zero_()
    _call("rq_dev_reconstruct_aq", CB, codes, C, n, d, m, h, None)
    lo.assert_periodic(CB, _dev(want), n, marks, what="CB (aq)")
    lo.assert_sentinel(CB, n)
    lo.assert_periodic(codes, _dev(tcodes), n, what="codes")


# ---- 7. norms: n * m past 2^31 and 2^32 with the largest m --------------------------------------------------------------------------------------
def test_norms_all_rows(rq, bases):
    """rq_dev_aq_norms at m = 64 (its largest), d = 4, h = 16: codes[row * 64 + i] passes 2^31 and 2^32; then
    rq_dev_quantize_norms on those n norms."""
    import torch
    import norms_oracle as no
    import rayuela_jl_amd.synth as synth
    bases.drop()
    d, m, h, hn = 4, 64, 16, 256
    marks = lo.thresholds(m, 1)
    n = lo.rows_past(marks[2])
    assert (n - 1) * m > lo.TWO32
    tcodes = (synth.random_codes(lo.P, m, seed=11) % h).astype(np.uint8)
    C = synth.deep_like(m * h, d, seed=12).reshape(m, h, d)
    want = no.aq_norms(tcodes, C)
    cb = np.ascontiguousarray(np.quantile(want, np.linspace(0, 1, hn))[::-1], dtype=np.float32)      # unsorted (descending)
    wantq = no.quantize(want, cb)
    assert len(np.unique(wantq)) > hn // 2
    _need(n * m + 12 * n)
    codes = lo.periodic(_dev(tcodes), n)
    norms = lo.output(n, (), torch.float32)
    _call("rq_dev_aq_norms", norms, codes, C, n, d, m, h, None)
    lo.assert_periodic(norms, _dev(want), n, marks, what="norms")
    lo.assert_sentinel(norms, n)
    lo.assert_periodic(codes, _dev(tcodes), n, marks, what="codes")
    ncodes = lo.output(n, (), torch.uint8)
    dbn = lo.output(n, (), torch.float32)
    _call("rq_dev_quantize_norms", ncodes, dbn, norms, cb, n, hn, None)
    lo.assert_periodic(ncodes, _dev(wantq), n, marks, what="norm codes")
    lo.assert_periodic(dbn, _dev(cb[wantq.astype(np.int64)]), n, marks, what="dbnorms")
    lo.assert_sentinel(ncodes, n)
    lo.assert_sentinel(dbn, n)


def test_norms_past_the_work_items_of_one_launch(rq, bases):
    """rq_dev_aq_norms runs a wavefront per 4 rows: 16 n work-items, 2^32 of them at n = 2^28 rows -- more than one dispatch
    takes, so the launcher cuts the rows into slices (rq_norms.hip: aq_norms_launch).  m = 4, d = 4, h = 16."""
    import torch
    import norms_oracle as no
    import rayuela_jl_amd.synth as synth
    bases.drop()
    d, m, h = 4, 4, 16
    n = lo.rows_past(1 << 28)
    assert 16 * n > lo.TWO32
    tcodes = (synth.random_codes(lo.P, m, seed=13) % h).astype(np.uint8)
    C = synth.deep_like(m * h, d, seed=14).reshape(m, h, d)
    want = no.aq_norms(tcodes, C)
    _need(n * m + 4 * n)
    codes = lo.periodic(_dev(tcodes), n)
    norms = lo.output(n, (), torch.float32)
    _call("rq_dev_aq_norms", norms, codes, C, n, d, m, h, None)
    lo.assert_periodic(norms, _dev(want), n, (1 << 28, 1 << 28, 1 << 28), what="norms (thresholds: 2^28 rows)")
    lo.assert_sentinel(norms, n)


# ---- 8. reductions, exact by construction --------------------------------------------------------------------------------------------------------
# Integer-valued period rows and codebook entries: every product and every partial sum below is an integer, every f32 partial
# sum stays below 2^24 (asserted from the data, for sums over any set of row slices) and every f64 sum below 2^53, so each
# kernel must return the integer value whatever its summation order; the expected value is integer arithmetic on the period,
# the repeat count and the tail.
RED_D, RED_M, RED_H = 128, 8, 256


def _int_tile(lim, seed, shape):
    import rayuela_jl_amd.synth as synth
    e = np.arange(int(np.prod(shape)), dtype=np.uint64)
    return ((synth.splitmix64(e ^ np.uint64(seed * 7919 + 1)) % np.uint64(2 * lim + 1)).astype(np.int64) - lim).reshape(shape)


def _red_case(xlim):
    """(X period int64 [P][d], codes period uint8 [P][m] with two codes that never occur, C int64 [m][h][sub], CB period)."""
    import rayuela_jl_amd.synth as synth
    d, m, h = RED_D, RED_M, RED_H
    X = _int_tile(xlim, 3, (lo.P, d))
    codes = synth.random_codes(lo.P, m, seed=21).copy()
    codes[codes[:, 0] == 7, 0] = 8                                     # entry 7 of sub-quantizer 0 and entry 200 of 3 stay empty
    codes[codes[:, 3] == 200, 3] = 201
    C = _int_tile(2, 4, (m, h, d // m))
    CB = np.concatenate([C[i][codes[:, i].astype(np.int64)] for i in range(m)], axis=1)
    return X, codes, C, CB


def _total(per_period, per_tail, n):
    return (n // lo.P) * per_period + per_tail


def _f32_sums_stay_exact(sum_period, abs_period, n, what, slices=512):
    """Every f32 partial sum a kernel can form stays an exactly representable integer.  The rows are cut into contiguous
    slices (512 is the most a launch here uses: gram_launch one per CU, gram_codes_launch two per CU at d = 128, 256 CUs);
    a slice sum is whole periods plus at most two partial ones, so the sum over any subset of slices -- and any prefix within
    one -- is at most |reps x period sum| + (2 x slices + 1) x the period's sum of absolute values."""
    reps = n // lo.P
    bound = np.abs(reps * sum_period).max() + (2 * slices + 1) * abs_period.max()
    assert bound < 2 ** 24, "%s: f32 sums may reach %d >= 2^24 (%d repeats)" % (what, bound, reps)


def test_reductions_exact_all_rows(rq, bases):
    """rq_dev_update_centers, rq_dev_qerror, rq_dev_qerror_codes and rq_dev_lsq_normal_eq on X in -8 .. 8 (17.2 GB) and its
    reconstruction CB in -2 .. 2 (17.2 GB)."""
    import torch
    d, m, h = RED_D, RED_M, RED_H
    sub = d // m
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    reps, tail = divmod(n, lo.P)
    Xt, tcodes, C, CBt = _red_case(8)
    bases.drop()
    _need(2 * n * d * 4 + n * m)
    X = lo.periodic(_dev(Xt.astype(np.float32)), n)
    codes = lo.periodic(_dev(tcodes), n)
    Ccat = np.ascontiguousarray(C.astype(np.float32)).reshape(-1)
    ci = tcodes.astype(np.int64)

    # update_centers: exact counts; every non-empty centre is the f32 rounding of the exact quotient (1 ulp allowed: the kernel
    # multiplies by a rounded reciprocal); an empty entry keeps its centre
    cnt = np.stack([_total(np.bincount(ci[:, i], minlength=h), np.bincount(ci[:tail, i], minlength=h), n) for i in range(m)])
    sums = np.zeros((m, h, sub), dtype=np.int64)
    for i in range(m):
        per, tl = np.zeros((h, sub), dtype=np.int64), np.zeros((h, sub), dtype=np.int64)
        np.add.at(per, ci[:, i], Xt[:, i * sub:(i + 1) * sub])
        np.add.at(tl, ci[:tail, i], Xt[:tail, i * sub:(i + 1) * sub])
        sums[i] = _total(per, tl, n)
    assert cnt[0, 7] == 0 and cnt[3, 200] == 0 and (cnt > 0).sum() == m * h - 2 and cnt.sum() == n * m
    assert 2 * 8 * cnt.max() < 2 ** 24                                  # the one-hot product carries 2 x the sums in f32
    Cd = torch.full((m * h * sub,), 99.5, dtype=torch.float32, device="cuda")
    counts = torch.zeros((m, h), dtype=torch.int32, device="cuda")
    _call("rq_dev_update_centers", Cd, counts, X, codes, n, d, m, h, None)
    assert np.array_equal(counts.cpu().numpy().view(np.uint32).astype(np.int64), cnt)
    got = Cd.cpu().numpy().reshape(m, h, sub)
    want = np.where(cnt[:, :, None] > 0, sums / np.maximum(cnt, 1)[:, :, None], 99.5).astype(np.float32)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    ulps[(got == 0) & (want == 0)] = 0
    print("update_centers: %d of %d centre values are 1 ulp from the rounded exact quotient, none further"
          % (int((ulps == 1).sum()), ulps.size))
    assert ulps.max() <= 1, "a centre is %d ulp from the exact mean" % int(ulps.max())
    assert (got[0, 7] == 99.5).all() and (got[3, 200] == 99.5).all()

    # qerror_codes, then reconstruct + qerror: exact
    df2 = ((Xt - CBt) ** 2).sum(axis=1)
    q_want = int(_total(df2.sum(), df2[:tail].sum(), n))
    assert q_want < 2 ** 53
    acc = torch.zeros((1,), dtype=torch.float64, device="cuda")
    _call("rq_dev_qerror_codes", acc, X, codes, Ccat, n, d, m, h, None)
    assert float(acc.item()) == float(q_want), (float(acc.item()), q_want)
    CB = lo.output(n, (d,), torch.float32)
    _call("rq_dev_reconstruct", CB, codes, Ccat, n, d, m, h, None)
    lo.assert_periodic(CB, _dev(CBt.astype(np.float32)), n, marks, what="CB")
    acc.zero_()
    _call("rq_dev_qerror", acc, X, CB, n, d, None)
    assert float(acc.item()) == float(q_want), (float(acc.item()), q_want)
    lo.assert_sentinel(CB, n)
    del CB

    # lsq_normal_eq: A = B'B + rho I (integer counts, the diagonal fl64(count + rho)) and b = B'X, both exact
    rho = 1e-4
    mh = m * h
    onehot = np.zeros((lo.P, mh))
    onehot[np.arange(lo.P)[:, None], ci + np.arange(m)[None, :] * h] = 1.0
    A_want = _total(onehot.T @ onehot, onehot[:tail].T @ onehot[:tail], n)
    b_want = _total(onehot.T @ Xt.astype(np.float64), onehot[:tail].T @ Xt[:tail].astype(np.float64), n)
    assert A_want.max() < 2 ** 32 and np.array_equal(np.diag(A_want).reshape(m, h), cnt)
    A_want[np.arange(mh), np.arange(mh)] = np.diag(A_want) + rho
    A = torch.full((mh, mh), -7.0, dtype=torch.float64, device="cuda")
    b = torch.full((mh, d), -7.0, dtype=torch.float64, device="cuda")
    _call("rq_dev_lsq_normal_eq", A, b, X, codes, n, d, m, h, ctypes.c_double(rho), None)
    assert np.array_equal(A.cpu().numpy(), A_want), "A: %d entries differ" % int((A.cpu().numpy() != A_want).sum())
    assert np.array_equal(b.cpu().numpy(), b_want), "b: %d entries differ" % int((b.cpu().numpy() != b_want).sum())
    lo.assert_periodic(X, _dev(Xt.astype(np.float32)), n, marks, what="X")
    lo.assert_periodic(codes, _dev(tcodes), n, what="codes")


def test_gram_exact_all_rows(rq, bases):
    """rq_dev_gram_codes and rq_dev_gram (f32 matrix-core partial sums per row slice, f32 sums over the slices) on X and CB in
    -2 .. 2: values small enough that every f32 sum of products over 3.4e7 rows stays below 2^24."""
    import torch
    d, m, h = RED_D, RED_M, RED_H
    marks = lo.thresholds(d, 4)
    n = lo.rows_past(marks[2])
    tail = n % lo.P
    Xt, tcodes, C, CBt = _red_case(2)
    G_want = _total(Xt.T @ CBt, Xt[:tail].T @ CBt[:tail], n)
    _f32_sums_stay_exact(Xt.T @ CBt, np.abs(Xt).T @ np.abs(CBt), n, "gram")
    assert np.abs(G_want).max() > 2 ** 16                               # and large enough that the whole array matters
    bases.drop()
    _need(2 * n * d * 4 + n * m)
    X = lo.periodic(_dev(Xt.astype(np.float32)), n)
    codes = lo.periodic(_dev(tcodes), n)
    Ccat = np.ascontiguousarray(C.astype(np.float32)).reshape(-1)
    G = torch.full((d, d), -7.0, dtype=torch.float32, device="cuda")
    _call("rq_dev_gram_codes", G, X, codes, Ccat, n, d, m, h, None)
    got = G.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, G_want), "gram_codes: %d of %d entries differ, worst by %d" % (
        int((got != G_want).sum()), d * d, int(np.abs(got - G_want).max()))
    CB = lo.periodic(_dev(CBt.astype(np.float32)), n)
    G.fill_(-7.0)
    _call("rq_dev_gram", G, X, CB, n, d, None)
    got = G.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, G_want), "gram: %d of %d entries differ, worst by %d" % (
        int((got != G_want).sum()), d * d, int(np.abs(got - G_want).max()))


# ---- 9. host-pointer forms: the chunked upload's pointer arithmetic past 2^32 bytes ------------------------------------------------------------------
def _need_host(nbytes):
    with open("/proc/meminfo") as f:
        avail = {ln.split(":")[0]: int(ln.split()[1]) * 1024 for ln in f}["MemAvailable"]
    if avail < 3 * nbytes:
        pytest.skip("needs 3 x %.1f GiB of host memory, %.1f GiB are available" % (nbytes / GB, avail / GB))


@pytest.mark.parametrize("kind", ["sift", "bytes"])
def test_host_encode_pq_all_rows(rq, oracle, bases, kind):
    """rq_encode_pq (f32 rows) and rq_encode_pq_bytes with n just past the row whose byte offset is 2^32: 4.3 GB of host input."""
    bases.drop()
    d, m, h = 128, 8, 256
    marks = lo.thresholds(d, 1 if kind == "bytes" else 4)
    n = lo.rows_past(marks[1])
    tile = _tile(kind, d)
    _need_host(n * d * tile.itemsize)
    C = _pq_codebooks(tile, m, h)
    want = oracle.encode_pq(tile.astype(np.float32), C, m, h)
    X = lo.periodic(tile, n)
    assert X.nbytes > lo.TWO32 and X.flags.c_contiguous
    codes = np.full((n + 1, m), lo.sentinel_of("uint8"), dtype=np.uint8)
    fn = _L().rq_encode_pq_bytes if kind == "bytes" else _L().rq_encode_pq
    rc = fn(codes.ctypes.data, X.ctypes.data, C.ctypes.data, n, d, m, h)
    assert rc == 0, _L().rq_last_error()
    lo.assert_periodic(codes, want, n, marks, what="codes")
    assert (codes[n] == lo.sentinel_of("uint8")).all()
    lo.assert_periodic(X, tile, n, marks, what="X")


# ---- 10. stated row limits: refused before any access ------------------------------------------------------------------------------------------------------
# The launchers that state a row limit check it ahead of every access to their arrays (read in rq_lsq.hip: lsq_check is the
# first statement of rq_dev_lsq_normal_eq / rq_dev_update_codebooks_lsq; rq_chain.hip: chain_check_update of
# rq_dev_update_codebooks_chain; rq_sr.hip: rq_train_sr and rq_sr_std test n before anything else), so a call at limit + 1 is
# safe on small sentinel-filled arrays.  residual_launch (rq_encode.hip) states no limit: it cuts its rows into
# launches for every caller (a limit inside the launch sequence, behind the host form's upload, could not be pinned).
def test_row_limits_are_refused_before_any_access(rq):
    import torch
    L = _L()
    d, m, h = 8, 2, 4
    over = (1 << 32)                                                   # limit 2^32 - 1 rows (the u32 counters)
    X = torch.full((16, d), -7.0, dtype=torch.float32, device="cuda")
    codes = torch.full((16, m), 0xA5, dtype=torch.uint8, device="cuda")
    A = torch.full((m * h, m * h), -7.0, dtype=torch.float64, device="cuda")
    b = torch.full((m * h, d), -7.0, dtype=torch.float64, device="cuda")
    C = torch.full((m, h, d), -7.0, dtype=torch.float32, device="cuda")
    rho = ctypes.c_double(1e-4)

    def refused(rc, who):
        msg = (L.rq_last_error() or b"").decode()
        assert rc == RQ_EINVAL and who in msg and str(over) in msg, (who, rc, msg)
        torch.cuda.synchronize()
        for t in (A, b, C, X):
            assert bool((t == -7.0).all()), who
        assert bool((codes == 0xA5).all()), who

    refused(L.rq_dev_lsq_normal_eq(A.data_ptr(), b.data_ptr(), X.data_ptr(), codes.data_ptr(), over, d, m, h, rho, None),
            "lsq_normal_eq")
    refused(L.rq_dev_update_codebooks_lsq(C.data_ptr(), X.data_ptr(), codes.data_ptr(), over, d, m, h, rho, None),
            "update_codebooks_lsq")
    refused(L.rq_dev_update_codebooks_chain(C.data_ptr(), X.data_ptr(), codes.data_ptr(), over, d, m, h, rho, None),
            "update_codebooks_chain")
    # host forms
    hX = np.full((16, d), -7.0, dtype=np.float32)
    hcodes = np.full((16, m), 0xA5, dtype=np.uint8)
    hC = np.full((m, h, d), -7.0, dtype=np.float32)
    obj = np.full((3,), -7.0)
    rc = L.rq_train_sr(hC.ctypes.data, hcodes.ctypes.data, obj.ctypes.data, hX.ctypes.data, None, over, d, m, h, 2, 1, 1, 0, 0, 0,
                       1, ctypes.c_double(0.5), 1, 0, 1)
    refused(rc, "train_sr")
    assert (hC == -7.0).all() and (hcodes == 0xA5).all() and (obj == -7.0).all() and (hX == -7.0).all()
    over = (2 ** 31 - 1) * 1024 + 1                                    # rq_sr_std: INT32_MAX blocks of 1024 rows
    sigma = np.full((d,), -7.0, dtype=np.float32)
    refused(L.rq_sr_std(sigma.ctypes.data, hX.ctypes.data, over, d), "sr_std")
    assert (sigma == -7.0).all() and (hX == -7.0).all()


# ---- 11. the slice planner of the wide centre update at its limits ----------------------------------------------------------------------------------
# update_centers_launch<int16_t> (rq_train.hip) cuts the rows into `grid` slices: want = min(ceil(CUs / code blocks), ceil(n / 1024)),
# raised to least = ceil(n / cap) with cap = min(2^23 - 1 rows (f32 counters), 2^30 bytes of X (32-bit buffer offsets)), capped by
# most = the slices whose partial sums ((grid + 1) x (h d + m h) floats, allocated 1.25x) fit 2 GiB; least > most is refused.  The
# library does not name its grid, so the cases below restate the planner and assert that the cap, not `want`, decides.
# The refill of emptied centres needs no case here: refill_cost_kernel and gather_rows_kernel (rq_train.hip) index with a 64-bit
# row throughout (row * d + col0, row * cstride + col and rows[k] * d are int64 / size_t products), so no 32-bit product passes
# 2^31 at any n the *_wide training entries accept.
RQ_EUNSUPPORTED = -2
H16_SCRATCH = 2 << 30


def _h16_plan(n, d, m, h):
    """(want, least, most, grid) of update_centers_launch<int16_t> for the device's CU count."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nblocks = (h + 255) // 256
    stride = h * d + m * h
    cap = min((1 << 23) - 1, (1 << 30) // (d * 4))
    most = (H16_SCRATCH // 5 * 4) // (stride * 4) - 1
    least = -(-n // cap) if cap > 0 else most + 1
    want = min(-(-cus // nblocks), -(-n // 1024))
    return want, least, most, min(max(want, 1, least), most)


def _wide_codes(n, m, h):
    """codes [n][m] int16 on the device: a fixed permutation of (row + 4099 q) % h, so every code has rows (n >= h)."""
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(h + m)
    perm = torch.randperm(h, generator=g).to(torch.int16).cuda()
    rows = torch.arange(n, device="cuda")
    return torch.stack([perm[((rows + 4099 * q) % h)] for q in range(m)], dim=1).contiguous()


def _int_rows(n, d, seed):
    """X [n][d] f32 on the device with integer coordinates in [0, 255]."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, d), generator=g, device="cuda", dtype=torch.int32).to(torch.float32)


def _exact_means_on_device(X, codes, m, h):
    """(C concatenated f32 (numpy), counts [m][h] int64 (numpy)): counts by bincount, sums by an f64 index_add_ on the device
    (exact on integers), centres float32(sum) * (1.0f / float32(count)) -- the kernel's finishing formula -- in numpy."""
    import torch
    n, d = X.shape
    sub = d // m
    assert sub * m == d
    out, counts = [], np.zeros((m, h), dtype=np.int64)
    for q in range(m):
        idx = codes[:, q].long()
        cnt = torch.bincount(idx, minlength=h).cpu().numpy()
        sums = torch.zeros((h, sub), dtype=torch.float64, device="cuda").index_add_(0, idx, X[:, q * sub:(q + 1) * sub].double())
        sums = sums.cpu().numpy()
        assert cnt.min() > 0 and np.array_equal(sums, np.round(sums))
        assert 2 * sums.max() < 2 ** 24 and 2 * cnt.max() < 2 ** 24          # the one-hot product carries 2 x the sums in f32
        out.append((sums.astype(np.float32) * (np.float32(1) / cnt.astype(np.float32))[:, None]).reshape(-1))
        counts[q] = cnt
    return np.concatenate(out), counts


def _wide_update_exact(n, d, m, h, seed):
    import torch
    X, codes = _int_rows(n, d, seed), _wide_codes(n, m, h)
    want, cnt = _exact_means_on_device(X, codes, m, h)
    assert cnt.sum() == n * m
    spare = 64
    Cd = torch.full((h * d + spare,), 99.5, dtype=torch.float32, device="cuda")
    counts = torch.full((m * h + spare,), lo.sentinel_of(torch.int32), dtype=torch.int32, device="cuda")
    _call("rq_dev_update_centers_wide", Cd, counts, X, codes, n, d, m, h, None)
    assert bool((Cd[h * d:] == 99.5).all()) and bool((counts[m * h:] == lo.sentinel_of(torch.int32)).all())
    assert np.array_equal(counts[:m * h].cpu().numpy().astype(np.int64).reshape(m, h), cnt)
    got = Cd[:h * d].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d centre values differ" % int((got != want).sum())
    return X, codes, Cd


def test_update_centers_wide_row_cap_forces_a_third_slice(rq, bases):
    """n = 2 (2^23 - 1) + 4112 rows of d = 8 (0.54 GB), m = 1, h = 32767: 128 code blocks want 2 slices, the 2^23-row cap of the
    f32 counters forces 3.  Counts exact, means bit-equal to float32(sum) * (1.0f / float32(count))."""
    n, d, m, h = 2 * ((1 << 23) - 1) + 4112, 8, 1, 32767
    want, least, most, grid = _h16_plan(n, d, m, h)
    assert (want, least, grid) == (2, 3, 3) and most >= 3 and (1 << 30) // (d * 4) > (1 << 23) - 1      # the ROW cap binds
    bases.drop()
    _need(n * d * 4 + 2 * n * d * 8 + n * m * 2)
    _wide_update_exact(n, d, m, h, 5)


def test_update_centers_wide_byte_cap_forces_a_third_slice(rq, bases):
    """d = 2048, m = 8, h = 32767, n = 2 (2^28 / 2048) + 77 rows (2.1 GB of X, 1.1 GB of partial sums): want 2 slices, the
    2^30-byte rule of the 32-bit buffer offsets forces 3, and 5 would still fit the scratch.  Then rq_dev_reconstruct_wide on the
    same codes: 5.4e8 output elements gathered from h d = 6.7e7 centre values, bit for bit."""
    import torch
    n, d, m, h = 2 * ((1 << 28) // 2048) + 77, 2048, 8, 32767
    want, least, most, grid = _h16_plan(n, d, m, h)
    assert (want, least, most, grid) == (2, 3, 5, 3) and (1 << 30) // (d * 4) < (1 << 23) - 1              # the BYTE cap binds
    bases.drop()
    _need(3 * n * d * 4 + 2 * n * d * 8 // m + 3 * h * d * 4 + (grid + 1) * (h * d + m * h) * 5)
    X, codes, Cd = _wide_update_exact(n, d, m, h, 6)
    del X
    CB = lo.output(n, (d,), torch.float32)
    _call("rq_dev_reconstruct_wide", CB, codes, Cd, n, d, m, h, None)
    sub = d // m
    for q in range(m):
        Cq = Cd[h * sub * q:h * sub * (q + 1)].view(h, sub)
        assert torch.equal(CB[:n, q * sub:(q + 1) * sub].view(torch.int32), Cq[codes[:, q].long()].view(torch.int32)), q
    lo.assert_sentinel(CB, n)


def test_update_centers_wide_refuses_a_slice_that_does_not_fit(rq):
    """d = 8192, m = 1, h = 32767: ONE slice of partial sums is 1.07 GB and the reduced slice behind it as much again, past the
    2 GiB of scratch (most = 0 slices): RQ_EUNSUPPORTED naming the shape.  update_centers_launch<int16_t> makes that test before
    it asks for its workspace or launches anything (read in rq_train.hip), so small sentinel-filled arrays are safe."""
    import torch
    n, d, m, h = 100, 8192, 1, 32767
    want, least, most, grid = _h16_plan(n, d, m, h)
    assert most == 0 and least == 1
    X = torch.full((n, d), -7.0, dtype=torch.float32, device="cuda")
    codes = torch.full((n, m), -3, dtype=torch.int16, device="cuda")
    Cd = torch.full((4096,), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((4096,), -3, dtype=torch.int32, device="cuda")
    L = _L()
    rc = L.rq_dev_update_centers_wide(Cd.data_ptr(), counts.data_ptr(), X.data_ptr(), codes.data_ptr(), n, d, m, h, None)
    msg = (L.rq_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc == RQ_EUNSUPPORTED and "n=%d d=%d h=%d" % (n, d, h) in msg and "partial sums" in msg, (rc, msg)
    assert bool((Cd == -7.0).all()) and bool((counts == -3).all()) and bool((X == -7.0).all()) and bool((codes == -3).all())
