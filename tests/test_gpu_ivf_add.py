"""GPU: adding to a loaded IVFADC base, from float and from byte rows (rq_ivf_add / _add_bytes / _add_codes / _build_bytes,
IvfIndex.add / add_codes, xvecs.ivf_add_bvecs).

The contract: after one build (or set_codes) and any number of adds the loaded base is the one a single build over the concatenated
rows loads.  Every comparison is exact, as in tests/test_gpu_ivf.py: offsets, row ids and code bytes of lists() against the
restatements (tests/ivf_oracle.py, tests/ivf_add_oracle.py) and against the one-call base on the device; ids, distance bits and
padding of a search."""
import functools
import threading

import numpy as np
import pytest

import ivf_add_oracle as ivfa
import ivf_oracle as ivf
from test_gpu_ivf import _bits, _data, _index, _lists_equal, _oracle_base, _same, N, M
from test_gpu_ivf_shapes import _shape

pytestmark = pytest.mark.gpu

LIMIT = 0xFFFFFFFF
RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2


def _lists(ix):
    return ix.lists()


def _equal3(got, want, what=""):
    for g, w, name in zip(got, want, ("offsets", "ids", "codes")):
        assert np.array_equal(g, w), (name, what)


def _probe_pairs(nlist, n):
    return [(p, k) for p in sorted({1, min(3, nlist), nlist}) for k in (1, 10, n + 1)]


# ---- 1. splits ------------------------------------------------------------------------------------------------------------------
SPLITS = [(1, 2), (1500, 2999), (2999, 3000)]


@pytest.mark.parametrize("kind", ["sift", "gauss"])
@pytest.mark.parametrize("nlist", [1, 7, 37, 300])
def test_build_and_two_adds_equal_one_build(rq, kind, nlist):
    X, Q, centers, Xq = _data(kind, nlist=nlist)
    for by_residual in (True, False):
        want = _oracle_base(kind, by_residual, nlist=nlist)
        with _index(rq, Q, centers, by_residual) as whole, _index(rq, Q, centers, by_residual) as ix:
            whole.build(X)
            _lists_equal(whole, want)
            answers = {pk: whole.search(Xq, *pk) for pk in _probe_pairs(nlist, N)}
            for a, b in SPLITS:
                ix.build(X[:a])
                assert ix.info()["next_id"] == a and ix.n == a
                ix.add(X[a:b])
                if b < N:
                    ix.add(X[b:], id_offset=b)
                info = ix.info()
                assert (info["n"], info["next_id"], ix.n, ix.next_id) == (N, N, N, N)
                _lists_equal(ix, want)
                for pk, w in answers.items():
                    _same(ix.search(Xq, *pk), w, (kind, nlist, by_residual, a, b, pk))


def test_add_on_an_empty_handle_is_a_build(rq):
    X, Q, centers, Xq = _data("sift", nlist=7)
    with _index(rq, Q, centers, True) as ix:
        assert ix.info()["next_id"] == 0
        ix.add(X, id_offset=1 << 31)                   # any id_offset: nothing is loaded
        _lists_equal(ix, _oracle_base("sift", True, nlist=7, id_offset=1 << 31))
        assert ix.info()["next_id"] == (1 << 31) + N
        ix.build(X[:10])                               # a build replaces, and the next id follows it down
        assert ix.info()["next_id"] == 10 and ix.info()["n"] == 10
    lists, codes = ivf.build(X, Q, centers, True)[1][0], ivf.build(X, Q, centers, True)[1][2]
    with _index(rq, Q, centers, True) as ix:
        ix.add_codes(lists, codes, id_offset=5)
        _lists_equal(ix, ivf.group(lists, codes, 7, 5))


# ---- 2. empty lists ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlist", [37, 300])
def test_adds_into_empty_and_into_populated_lists(rq, nlist):
    X, Q, centers, Xq = _data("sift", nlist=nlist)
    X5 = np.ascontiguousarray(X[np.arange(N) % 5])            # 5 distinct rows: at most 5 populated lists
    all_lists = ivf.lists_of(X, Q)
    populated = np.unique(ivf.lists_of(X5[:5], Q))
    fresh = np.ascontiguousarray(X[~np.isin(all_lists, populated)][:600])        # rows of lists that hold nothing yet
    again = np.ascontiguousarray(X[np.isin(all_lists, populated)][:400])         # rows of lists that do
    assert fresh.shape[0] == 600 and again.shape[0] >= 5
    pieces = [X5[:1000], X5[1000:2000], fresh, again, X5[2000:]]
    for by_residual in (True, False):
        with _index(rq, Q, centers, by_residual) as ix:
            at = 0
            for i, piece in enumerate(pieces):
                ix.build(piece) if i == 0 else ix.add(piece)
                at += piece.shape[0]
                want = ivf.build(np.concatenate(pieces[:i + 1]), Q, centers, by_residual)[0]
                _lists_equal(ix, want)
                assert ix.info()["next_id"] == at and ix.info()["empty_lists"] == int((np.diff(want[0]) == 0).sum())
                if i == 1:
                    assert int((np.diff(want[0]) > 0).sum()) <= 5          # long runs of equal offsets around the populated lists
            for nprobe, k in ((1, 10), (nlist, at + 1)):
                _same(ix.search(Xq[:9], nprobe, k), ivf.search(want, Q, centers, by_residual, Xq[:9], nprobe, k), (nlist, nprobe, k))


@pytest.mark.parametrize("nlist", [37, 300])
@pytest.mark.parametrize("where", ["last", "first", "middle"])
def test_all_loaded_rows_in_one_list(rq, nlist, where):
    import rayuela_jl_amd.synth as synth
    _, Q, centers, Xq = _data("sift", nlist=nlist)
    only = {"last": nlist - 1, "first": 0, "middle": nlist // 2}[where]
    rng = np.random.default_rng(nlist)
    n0, n1 = 2500, 900          # a workgroup of the carry takes 2048 rows: one lies inside the list, the others end in many lists
    lists = np.concatenate([np.full(n0, only), rng.integers(0, nlist, n1), np.full(50, only)])
    codes = synth.random_codes(lists.size, M, seed=nlist + 1)
    bounds = [0, n0, n0 + n1, lists.size]
    with _index(rq, Q, centers, False) as ix:
        ix.set_codes(lists[:n0], codes[:n0], id_offset=3)
        for lo, hi in zip(bounds[1:-1], bounds[2:]):
            ix.add_codes(lists[lo:hi], codes[lo:hi])
            _lists_equal(ix, ivf.group(lists[:hi], codes[:hi], nlist, 3))
        want = ivf.group(lists, codes, nlist, 3)
        _same(ix.search(Xq[:9], nlist, 20), ivf.search(want, Q, centers, False, Xq[:9], nlist, 20), (nlist, where))


# ---- 3. row widths ----------------------------------------------------------------------------------------------------------------
# m -> MP: 1, 2 -> 2 | 4 -> 4 | 5, 8 -> 8 | 16 -> 16 | 17, 32 -> 32 | 48, 64 -> 64 (add_codes only: the encode covers m <= 32)
WIDTHS = [(32, 1), (32, 2), (32, 4), (40, 5), (96, 8), (96, 16), (34, 17), (96, 32), (96, 48), (64, 64)]


@pytest.mark.parametrize("d,m", WIDTHS)
def test_every_row_width_of_the_carry(rq, d, m):
    import rayuela_jl_amd.synth as synth
    n, nlist = 1500, 7
    X, Q, centers, Xq = _shape("sift", n, d, m, nlist)
    lists, codes = ivf.lists_of(X, Q), synth.random_codes(n, m, seed=d + m)
    with _index(rq, Q, centers, True) as whole, _index(rq, Q, centers, True) as ix:
        whole.set_codes(lists, codes, id_offset=9)
        want = ivf.group(lists, codes, nlist, 9)
        _lists_equal(whole, want)
        for a, b in ((1, 700), (699, 1499)):
            ix.set_codes(lists[:a], codes[:a], id_offset=9)
            ix.add_codes(lists[a:b], codes[a:b])
            ix.add_codes(lists[b:], codes[b:], id_offset=9 + b)
            _lists_equal(ix, want)
        _same(ix.search(Xq, 3, 50), whole.search(Xq, 3, 50), (d, m))
        if m <= 32:
            whole.build(X)
            ix.build(X[:700])
            ix.add(X[700:1499])
            ix.add(X[1499:])
            _equal3(_lists(ix), _lists(whole), (d, m))
            _same(ix.search(Xq, 3, 50), whole.search(Xq, 3, 50), ("build", d, m))


# ---- 4. chunking --------------------------------------------------------------------------------------------------------------------
def test_add_in_row_chunks_and_sort_pieces(rq):
    X, Q, centers, _ = _data("gauss", nlist=37)
    arrival = ivf.build(X, Q, centers, True)[1]
    want = ivfa.chain([(arrival[0][:1000], arrival[2][:1000], 0), (arrival[0], arrival[2], 1000)], 37)[-1]
    try:
        with _index(rq, Q, centers, True) as ix:
            for rows, piece in ((0, 0), (700, 512), (700, 0), (0, 512)):
                rq.set_tuning("IVF_BUILD_ROWS", rows) if rows else rq.reset_tuning("IVF_BUILD_ROWS")
                rq.set_tuning("IVF_SORT_ROWS", piece) if piece else rq.reset_tuning("IVF_SORT_ROWS")
                ix.build(X[:1000])
                ix.add(X)                              # 3000 rows: 5 chunks, 6 sorted pieces, a list's rows spread over them
                _lists_equal(ix, want)
    finally:
        rq.reset_tuning("IVF_BUILD_ROWS")
        rq.reset_tuning("IVF_SORT_ROWS")


# ---- 5. ids ---------------------------------------------------------------------------------------------------------------------------
def test_ids_gaps_limits_and_refusals(rq):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    X, Q, centers, Xq = _data("sift", nlist=7)
    Xq = Xq[:9]
    lists, _, codes = ivf.build(X, Q, centers, True)[1]
    offs = [(1 << 31) - 5, (1 << 31) + 5000, LIMIT - 1000]          # a gap, then a piece that ends exactly at id 2^32 - 2
    bounds = [0, 1000, 2000, 3000]
    bases = ivfa.chain([(lists[lo:hi], codes[lo:hi], off) for lo, hi, off in zip(bounds[:-1], bounds[1:], offs)], 7)
    with _index(rq, Q, centers, True) as ix:
        for i, (lo, hi, off) in enumerate(zip(bounds[:-1], bounds[1:], offs)):
            ix.build(X[lo:hi], id_offset=off) if i == 0 else ix.add(X[lo:hi], id_offset=off)
            _lists_equal(ix, bases[i])
            assert ix.info()["next_id"] == off + 1000 == ivfa.next_id(bases[i]) == ix.next_id
            for id_base in (0, 1):
                _same(ix.search(Xq, 3, 10, id_base), ivf.search(bases[i], Q, centers, True, Xq, 3, 10, id_base), (i, id_base))
        final = bases[-1]
        assert int(final[1].max()) == LIMIT - 1
        answer = ivf.search(final, Q, centers, True, Xq, 7, N + 1, 1)

        def untouched(what):
            _lists_equal(ix, final)
            _same(ix.search(Xq, 7, N + 1, 1), answer, what)
            assert ix.info()["next_id"] == LIMIT and ix.info()["n"] == N and (ix.n, ix.next_id) == (N, LIMIT)

        row = np.ascontiguousarray(X[:1])
        # the index is full at the top: no id is left, every add is refused by the id rule or the id range
        with pytest.raises(ValueError):
            ix.add(row, id_offset=LIMIT - 1)                       # one below the next id
        assert L.rq_ivf_add(ix._h, row.ctypes.data, 1, LIMIT - 1) == RQ_EINVAL
        msg = L.rq_last_error()
        assert str(LIMIT - 1).encode() in msg and str(LIMIT).encode() in msg, msg       # the message names both numbers
        untouched("id below the next id")
        with pytest.raises(ValueError):
            ix.add(row)                                            # id_offset = next id = 2^32 - 1: id_offset + n = 2^32
        assert L.rq_ivf_add(ix._h, row.ctypes.data, 1, LIMIT) == RQ_EINVAL
        assert b"2^32 - 1" in L.rq_last_error()
        untouched("id_offset + n = 2^32")
    with _index(rq, Q, centers, True) as ix:
        ix.build(X[:1000], id_offset=offs[0])
        ix.add(X[1000:2000], id_offset=offs[1])
        loaded, nxt = bases[1], offs[1] + 1000
        answer = ivf.search(loaded, Q, centers, True, Xq, 7, 50, 0)

        def untouched(what):       # noqa: F811
            _lists_equal(ix, loaded)
            _same(ix.search(Xq, 7, 50, 0), answer, what)
            assert ix.info()["next_id"] == nxt and ix.info()["n"] == 2000 and (ix.n, ix.next_id) == (2000, nxt)

        row = np.ascontiguousarray(X[:4])
        with pytest.raises(ValueError):
            ix.add(row, id_offset=nxt - 1)
        assert L.rq_ivf_add(ix._h, row.ctypes.data, 4, nxt - 1) == RQ_EINVAL
        msg = L.rq_last_error()
        assert str(nxt - 1).encode() in msg and str(nxt).encode() in msg, msg
        assert L.rq_ivf_add_bytes(ix._h, row.ctypes.data, 4, nxt - 1) == RQ_EINVAL
        untouched("id below the next id")
        # rows loaded + n past 2^32 - 1 (the argument paths only: the rows are never read)
        ix.n = LIMIT - 2
        with pytest.raises(ValueError):
            ix.add(row, id_offset=nxt)
        ix.n = 2000
        assert L.rq_ivf_add(ix._h, row.ctypes.data, LIMIT - 1999, nxt) == RQ_EINVAL
        lu = lists.astype(np.uint32)
        assert L.rq_ivf_add_codes(ix._h, lu.ctypes.data, codes.ctypes.data, LIMIT - 1999, nxt) == RQ_EINVAL
        assert L.rq_ivf_add(ix._h, row.ctypes.data, 0, nxt) == RQ_EINVAL
        untouched("too many rows")
        # a list id equal to nlist, past the mirror's own check: the message names the row
        bad = np.zeros(500, dtype=np.uint32)
        bad[499] = 7
        assert L.rq_ivf_add_codes(ix._h, bad.ctypes.data, codes.ctypes.data, 500, nxt) == RQ_EINVAL
        assert b"499" in L.rq_last_error()
        with pytest.raises(ValueError):
            ix.add_codes(bad, codes[:500])
        untouched("list id out of range")
        # NULL pointers
        assert L.rq_ivf_add(ix._h, None, 4, nxt) == RQ_EINVAL
        assert L.rq_ivf_add_bytes(ix._h, None, 4, nxt) == RQ_EINVAL
        assert L.rq_ivf_add_codes(ix._h, None, codes.ctypes.data, 4, nxt) == RQ_EINVAL
        assert L.rq_ivf_add_codes(ix._h, bad.ctypes.data, None, 4, nxt) == RQ_EINVAL
        assert L.rq_ivf_add(None, row.ctypes.data, 4, nxt) == RQ_EINVAL
        assert L.rq_ivf_build_bytes(ix._h, None, 4, 0) == RQ_EINVAL
        untouched("NULL")
        ix.add(X[2000:], id_offset=offs[2])                          # and the handle still takes a good add
        _lists_equal(ix, bases[2])


def test_add_of_rows_is_refused_past_32_codebooks(rq):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    n = 600
    X, Q, centers, _ = _shape("sift", 1500, 96, 48, 7)
    lists, codes = ivf.lists_of(X[:n], Q), synth.random_codes(n, 48, seed=1)
    with _index(rq, Q, centers, True) as ix:
        ix.set_codes(lists, codes)
        want = ivf.group(lists, codes, 7)
        with pytest.raises(ValueError):
            ix.add(X[n:])
        assert L.rq_ivf_add(ix._h, X[n:].ctypes.data, 10, n) == RQ_EUNSUPPORTED
        assert b"m <= 32" in L.rq_last_error()
        X8 = X.astype(np.uint8)
        assert L.rq_ivf_add_bytes(ix._h, X8.ctypes.data, 10, n) == RQ_EUNSUPPORTED
        assert L.rq_ivf_build_bytes(ix._h, X8.ctypes.data, 10, 0) == RQ_EUNSUPPORTED
        _lists_equal(ix, want)
        assert ix.info()["next_id"] == n


# ---- 6. bytes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _byte_data(n, d, m, nlist):
    """X8 (uint8; 255 and 0 in every position of some rows), Q (rows of X8 as float), centers, float queries; read-only"""
    import rayuela_jl_amd.synth as synth
    X8 = np.clip(synth.sift_like(n, d, seed=5, ncentres=64), 0, 255).astype(np.uint8)
    X8[3], X8[4] = 255, 0
    X8[5] = np.where(np.arange(d) % 2 == 0, 255, 0)
    X8[n - 1], X8[n - 2] = 0, 255
    Xf = X8.astype(np.float32)
    rng = np.random.default_rng(d * 1000 + nlist)
    Q = Xf[rng.choice(n, nlist, replace=False)].copy()
    R = ivf.residuals(Xf, Q, ivf.lists_of(Xf, Q))
    centers = np.stack(synth.codebooks(R, m, 256, seed=9, iters=0, sample=n)).astype(np.float32)
    Xq = synth.sift_like(9, d, seed=6, ncentres=64)
    for a in (X8, Q, centers, Xq):
        a.setflags(write=False)
    return X8, Q, centers, Xq


# d = 6, 10: rows that are no multiple of 4 bytes (2-byte loads) | d = 1: single bytes | d = 258: a row past 256 bytes, 2-byte loads,
# sub-spaces of 43 | d = 32: 8-byte loads; 300 lists: the 16-bit route of the byte assignment
BYTE_SHAPES = [(3000, 32, 4, 7), (3000, 32, 4, 300), (1500, 6, 3, 7), (1500, 10, 5, 7), (1500, 1, 1, 7), (1000, 258, 6, 7)]


@pytest.mark.parametrize("n,d,m,nlist", BYTE_SHAPES)
def test_byte_rows_are_the_widened_rows(rq, oracle, n, d, m, nlist):
    X8, Q, centers, Xq = _byte_data(n, d, m, nlist)
    Xf = X8.astype(np.float32)
    a, b = n // 3 + 1, n - 1
    for by_residual in (True, False):
        want = ivf.build(Xf, Q, centers, by_residual, id_offset=4)[0]
        with _index(rq, Q, centers, by_residual) as fl, _index(rq, Q, centers, by_residual) as by:
            fl.build(Xf, id_offset=4)
            _lists_equal(fl, want)
            by.build(X8, id_offset=4)
            _lists_equal(by, want)
            assert by.info()["next_id"] == n + 4
            by.build(X8[:a], id_offset=4)
            by.add(X8[a:b])
            by.add(X8[b:])
            _lists_equal(by, want)
            fl.build(Xf[:a], id_offset=4)                # float and byte pieces mix: a byte row IS its widened row
            fl.add(X8[a:b])
            fl.add(Xf[b:])
            _lists_equal(fl, want)
            for nprobe, k in ((min(3, nlist), 10), (nlist, n + 1)):
                _same(by.search(Xq, nprobe, k), fl.search(Xq, nprobe, k), (d, m, by_residual, nprobe, k))


@pytest.mark.parametrize("d,m", [(32, 4), (10, 5)])
def test_byte_rows_at_an_odd_host_address_through_the_c_entries(rq, d, m):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    n = 1500 if d == 10 else 3000
    X8, Q, centers, _ = _byte_data(n, d, m, 7)
    buf = np.zeros(n * d + 64, dtype=np.uint8)
    at = (-buf.ctypes.data) % 64 + 1                       # one byte past a 64-byte boundary
    buf[at:at + n * d] = X8.reshape(-1)
    ptr = buf.ctypes.data + at
    assert ptr % 64 == 1
    a = 701
    for by_residual in (True, False):
        want = ivf.build(X8.astype(np.float32), Q, centers, by_residual)[0]
        with _index(rq, Q, centers, by_residual) as ix:
            _lib.check(L.rq_ivf_build_bytes(ix._h, ptr, n, 0))
            _lists_equal(ix, want)
            _lib.check(L.rq_ivf_build_bytes(ix._h, ptr, a, 0))
            _lib.check(L.rq_ivf_add_bytes(ix._h, ptr + a * d, n - a, a))
            _lists_equal(ix, want)
            assert ix.info()["next_id"] == n


# ---- 7. non-finite --------------------------------------------------------------------------------------------------------------------
def test_nonfinite_rows_and_queries(rq):
    X, Q, centers, Xq = _data("gauss", nlist=7)
    Xn = X.copy()
    Xn[7, 3] = np.nan
    Xn[1600, :] = np.nan
    Xn[1700, 0] = np.inf
    Xn[1800, 31] = -np.inf
    Xn[2999, 8:16] = np.inf
    Xn[2998, 5] = np.nan
    qn = Xq[:6].copy()
    qn[0, 5] = np.nan
    qn[1, 0] = np.inf
    qn[3, :] = np.nan
    for by_residual in (True, False):
        with _index(rq, Q, centers, by_residual) as whole, _index(rq, Q, centers, by_residual) as ix:
            whole.build(Xn)                            # lists and codes of such rows follow the encode's contract: the same kernels
            ix.build(Xn[:1500])
            ix.add(Xn[1500:2999])
            ix.add(Xn[2999:])
            _equal3(_lists(ix), _lists(whole), by_residual)
            _same(ix.search(Xq, 3, 40), whole.search(Xq, 3, 40), by_residual)
            # finite rows, non-finite queries after an add: the restated search
            grouped = _oracle_base("gauss", by_residual, nlist=7)
            ix.build(X[:1234])
            ix.add(X[1234:])
            _lists_equal(ix, grouped)
            for nprobe, k in ((1, 10), (3, 40), (7, N)):
                _same(ix.search(qn, nprobe, k), ivf.search(grouped, Q, centers, by_residual, qn, nprobe, k), (by_residual, nprobe, k))


# ---- 8. file streaming ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_per_read", [1, 999, 3000, 10 ** 6])
def test_ivf_add_bvecs_gives_file_positions_whatever_the_piece(rq, tmp_path, rows_per_read):
    from rayuela_jl_amd import xvecs
    X8, Q, centers, _ = _byte_data(3000, 32, 4, 7)
    path = str(tmp_path / "base.bvecs")
    xvecs.bvecs_write(X8, path)
    Xf = X8.astype(np.float32)
    for bounds, lo, hi in ((None, 0, 3000), ((501, 2500), 500, 2500)):
        want = ivf.build(Xf[lo:hi], Q, centers, True, id_offset=lo)[0]
        with _index(rq, Q, centers, True) as ix:
            assert xvecs.ivf_add_bvecs(ix, path, bounds=bounds, rows_per_read=rows_per_read) == hi - lo
            _lists_equal(ix, want)
            assert ix.info()["next_id"] == hi
            if bounds is not None and rows_per_read == 999:     # the next shard of the file goes behind it
                assert xvecs.ivf_add_bvecs(ix, path, bounds=(2601, 3000), rows_per_read=rows_per_read) == 400
                lists, _, codes = ivf.build(Xf[2600:], Q, centers, True)[1]
                _lists_equal(ix, ivfa.add(want, lists, codes, 7, 2600))


def test_ivf_add_fvecs(rq, tmp_path):
    from rayuela_jl_amd import xvecs
    X, Q, centers, _ = _data("gauss", nlist=7)
    path = str(tmp_path / "base.fvecs")
    xvecs.fvecs_write(X, path)
    with _index(rq, Q, centers, True) as ix:
        assert xvecs.ivf_add_fvecs(ix, path, rows_per_read=999) == N
        _lists_equal(ix, _oracle_base("gauss", True, nlist=7))


# ---- 9. concurrency -------------------------------------------------------------------------------------------------------------------
def test_a_search_sees_the_base_before_or_after_an_add(rq):
    X, Q, centers, Xq = _data("sift", nlist=7)
    lists, _, codes = ivf.build(X, Q, centers, True)[1]
    bounds = [0, 1000, 1700, 2400, N]
    bases = ivfa.chain([(lists[lo:hi], codes[lo:hi], lo) for lo, hi in zip(bounds[:-1], bounds[1:])], 7)
    wants = [ivf.search(g, Q, centers, True, Xq, 3, 10) for g in bases]
    assert len({w[1].tobytes() + _bits(w[0]).tobytes() for w in wants}) == 4           # the four bases answer differently
    got, errs = [], []
    with _index(rq, Q, centers, True) as ix:
        ix.build(X[:1000])

        def searcher():
            try:
                for _ in range(48):
                    got.append(ix.search(Xq, 3, 10))
            except Exception as e:   # noqa: BLE001
                errs.append(repr(e))

        def adder():
            try:
                for lo, hi in zip(bounds[1:-1], bounds[2:]):
                    ix.add(X[lo:hi])
            except Exception as e:   # noqa: BLE001
                errs.append(repr(e))

        ts = [threading.Thread(target=searcher), threading.Thread(target=adder)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errs and len(got) == 48, errs
        seen = []
        for g in got:
            which = [i for i, w in enumerate(wants) if np.array_equal(g[1], w[1]) and np.array_equal(_bits(g[0]), _bits(w[0]))]
            assert len(which) == 1, "an answer that is none of the four bases'"
            seen.append(which[0])
        assert seen == sorted(seen)                     # and never an older base after a newer one
        print("answers per base:", [seen.count(i) for i in range(4)])
        _lists_equal(ix, bases[-1])
        _same(ix.search(Xq, 3, 10), wants[-1])


def test_adds_while_the_exact_knn_runs_on_the_shared_bulk_slot(rq):
    from rayuela_jl_amd.knn import groundtruth
    X, Q, centers, Xq = _data("sift", nlist=7)
    want = _oracle_base("sift", True, nlist=7)
    gt = groundtruth(X, Xq, 10)
    errs = []
    with _index(rq, Q, centers, True) as ix:
        def adds():
            try:
                for _ in range(3):
                    ix.build(X[:500])
                    for lo in range(500, N, 500):
                        ix.add(X[lo:lo + 500])
                    _lists_equal(ix, want)
            except Exception as e:   # noqa: BLE001
                errs.append(("add", repr(e)))

        def knn():
            try:
                for _ in range(4):
                    ids, dists = groundtruth(X, Xq, 10)
                    assert np.array_equal(ids, gt[0]) and np.array_equal(dists.view(np.uint64), gt[1].view(np.uint64))
            except Exception as e:   # noqa: BLE001
                errs.append(("groundtruth", repr(e)))

        ts = [threading.Thread(target=adds), threading.Thread(target=knn)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errs, errs


# ---- 10. scratch ------------------------------------------------------------------------------------------------------------------------
def test_an_add_does_not_depend_on_scratch_content(rq):
    from test_gpu_scratch import _invariance
    X, Q, centers, Xq = _data("sift", nlist=37)
    X8 = X[2500:].astype(np.uint8)                     # sift_like rows are integers in 0 .. 255
    assert np.array_equal(X8.astype(np.float32), X[2500:])
    want = _oracle_base("sift", True, nlist=37)
    answer = ivf.search(want, Q, centers, True, Xq[:9], 3, 10)
    with _index(rq, Q, centers, True) as ix:
        def run():
            ix.build(X[:1500])
            ix.add(X[1500:2500])
            ix.add(X8)
            off, ids, codes = ix.lists()
            dists, idx = ix.search(Xq[:9], 3, 10)
            return {"offsets": off, "ids": ids, "codes": codes, "dists": dists, "idx": idx}

        def check(got):
            _equal3((got["offsets"], got["ids"], got["codes"]), want)
            _same((got["dists"], got["idx"]), answer)

        slots, _ = _invariance("ivf_add", run, check)
        print("build + add + add_bytes + search rewrite:", sorted(slots))
        assert "WS_BULK" in slots


# ---- 11. driver -------------------------------------------------------------------------------------------------------------------------
def test_experiment_ivfpq_in_adds_gives_the_same_curves(rq):
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.experiments import experiment_ivfpq
    d, nlist, knn, nprobes = 16, 16, 10, (1, 4, 16)
    Xb = synth.sift_like(3000, d, seed=42)
    Xt, Xq = synth.sift_like(2000, d, seed=43), synth.sift_like(33, d, seed=44)
    truth = (((Xq.astype(np.float64)[:, None, :] - Xb.astype(np.float64)[None, :, :]) ** 2).sum(-1).argmin(1) + 1).astype(np.uint32)
    for by_residual in (True, False):
        kw = dict(nlist=nlist, m=4, nprobes=nprobes, niter=3, knn=knn, by_residual=by_residual, seed=1)
        Q0, C0, r0 = experiment_ivfpq(Xt, Xb, Xq, truth, **kw)
        Q1, C1, r1 = experiment_ivfpq(Xt, Xb, Xq, truth, add_rows=700, **kw)
        assert np.array_equal(_bits(Q0), _bits(Q1)) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(C0, C1))
        assert sorted(r0) == sorted(r1) == list(nprobes)
        for nprobe in nprobes:
            assert np.array_equal(np.asarray(r0[nprobe]).view(np.uint8), np.asarray(r1[nprobe]).view(np.uint8)), nprobe
    with pytest.raises(ValueError):
        experiment_ivfpq(Xt, Xb, Xq, truth, add_rows=0, **kw)
