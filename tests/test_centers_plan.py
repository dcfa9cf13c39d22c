"""CPU: the slice plan of update_centers and of the ERVQ increment (rq_centers_plan, host code only) against
tests/golden/centers_plan.json.  The number of row slices fixes the order of the float reduction over the partial sums, so it
decides output bits; the table was recorded from the four launchers (bytes / int16, update_centers / increment) as they stood
before they shared one planner, over a thinned cross of CU counts, row counts around the 1024-row and 2^23-row limits,
dimensions, sub-quantizer counts, codebook sizes around the 64 / 128 / 256-code tile steps and code strides -- refused shapes
and the byte fall-back to the owner-thread kernel included."""
import ctypes as C
import json
import os

from switch_table import switches

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "centers_plan.json")
RQ_EINVAL, RQ_EUNSUPPORTED = -1, -2


def _table():
    doc = json.load(open(GOLDEN))
    assert doc["columns"] == ["n", "d", "m", "h", "num_cu", "code_bytes", "cstride", "rc", "path", "slices", "units", "blocks",
                              "full_blocks", "ragged_tiles", "ws_tmp_bytes"]
    return doc["rows"]


def _plan(n, d, m, h, num_cu, code_bytes, cstride):
    from rayuela_jl_amd import _lib
    out = (C.c_int64 * 8)()
    assert _lib.lib().rq_centers_plan(n, d, m, h, num_cu, code_bytes, cstride, C.cast(out, C.c_void_p), 8) == 0
    return list(out)


def test_the_table_covers_the_four_callers_and_their_boundaries():
    rows = _table()
    assert len(rows) > 1500
    for code_bytes in (1, 2):
        for inc in (False, True):
            sub = [r for r in rows if r[5] == code_bytes and (r[6] > 0) == inc]
            assert {r[4] for r in sub} == {1, 64, 256}
            assert {r[0] for r in sub} == {1, 1023, 1024, 1025, 262145, 10**6, 256 * 2**23, 256 * 2**23 + 1, 3 * 10**9}
            assert {r[1] for r in sub} == {1, 16, 17, 20, 128, 960, 8192}
            assert {r[3] for r in sub} == {1, 64, 65, 128, 129, 256, 257, 300, 384, 448, 512, 4096, 32767}
            assert {r[2] for r in sub} == ({1} if inc else {1, 3, 5, 32})
            assert {r[6] for r in sub} == ({1, 4, 64} if inc else {0})
            assert any(r[7] != 0 for r in sub) and any(r[7] == 0 and r[9] > 1 for r in sub)
            assert {r[8] for r in sub if r[7] == 0} == ({1, 2} if (code_bytes, inc) == (1, False) else {1})


def test_every_row_of_the_table_is_what_the_planner_says():
    bad = [(r[:7], r[7:], _plan(*r[:7])) for r in _table() if _plan(*r[:7]) != r[7:]]
    assert not bad, (len(bad), bad[:5])


def test_the_matrix_core_switch_moves_only_the_byte_update():
    """TRAIN_CENTERS_MFMA = 0: update_centers over bytes takes the owner-thread kernel (path 2, no units) with the slices and the
    scratch it had; the int16 form and both increments do not read the switch."""
    rows = [r for r in _table() if r[7] == 0]
    with switches(TRAIN_CENTERS_MFMA=0):
        for r in rows:
            got = _plan(*r[:7])
            if r[5] == 1 and r[6] == 0:
                assert got == [0, 2, r[9], 0, 0, 0, 0, r[14]], (r, got)
            else:
                assert got == r[7:], (r, got)


def test_arguments_of_the_readout():
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    out = (C.c_int64 * 8)()
    ptr = C.cast(out, C.c_void_p)
    assert L.rq_centers_plan(1000, 16, 1, 16, 64, 1, 0, None, 8) == RQ_EINVAL
    assert L.rq_centers_plan(1000, 16, 1, 16, 64, 1, 0, ptr, 7) == RQ_EINVAL
    assert L.rq_centers_plan(1000, 16, 1, 16, 64, 3, 0, ptr, 8) == RQ_EINVAL         # code_bytes
    assert L.rq_centers_plan(1000, 16, 1, 16, 0, 1, 0, ptr, 8) == RQ_EINVAL          # num_cu
    # the launchers' own refusals come back in out[0], with nothing planned
    assert _plan(1000, 16, 1, 257, 64, 1, 0) == [RQ_EUNSUPPORTED] + [0] * 7          # bytes: h <= 256
    assert _plan(1000, 2, 3, 300, 64, 2, 0) == [RQ_EINVAL] + [0] * 7                 # int16: d < m is a bad argument
    assert _plan(1000, 2, 3, 16, 64, 1, 0) == [RQ_EUNSUPPORTED] + [0] * 7            # bytes: the same shape is "not covered"
    assert _plan(1000, 16, 1, 257, 64, 1, 4) == [RQ_EINVAL] + [0] * 7                # byte increment: h <= 256
    assert _plan(0, 16, 1, 16, 64, 2, 0) == [0] * 8 and _plan(0, 16, 1, 16, 64, 2, 1) == [0] * 8
