"""CPU: rq_scan_wide_slices, the host-only planner of the row slices of the scans over 16-bit codes.
The byte counts below restate csrc/rq_scan_h16.hip and csrc/rq_bulk.hip; tests/test_gpu_scan_wide_slices.py runs the slices."""
import pytest

BULK_USABLE_BYTES = (2 << 30) // 5 * 4


def _align256(b):
    return (b + 255) & ~255


def _unsliced_lower_bound(n, nb, m, h, k, plan):
    """h16_scan_bytes without the chain's per-query state: keys + tables + 16 k bytes of select buffers + the 6 * 256 of slack."""
    groups = -(-nb // plan["qg"])
    gstride = (m * h * plan["qpg"] + 3) & ~3
    return _align256(nb * n * 8) + _align256(groups * gstride * 4) + nb * 2 * k * 8 + 6 * 256


def test_a_base_that_fits_is_one_slice(rq):
    from rayuela_jl_amd import _lib
    n, nq, m, h, k = 10 ** 6, 1000, 8, 1024, 100
    p = _lib.scan_wide_slices(n, nq, m, h, k)
    assert (p["rows"], p["slices"], p["forced"]) == (n, 1, 0)
    plan = _lib.scan_wide_plan(m, h)
    assert 1 <= p["batch"] <= nq
    assert _unsliced_lower_bound(n, p["batch"], m, h, k, plan) <= p["bytes"] <= BULK_USABLE_BYTES
    # the 6 * 256 bytes of slack are part of the count, as for the unsliced scan: bytes of nb queries are linear in nb up to them
    one = _lib.scan_wide_slices(n, 1, m, h, k)
    four = _lib.scan_wide_slices(n, 4, m, h, k)
    assert (one["batch"], four["batch"]) == (1, 4)
    per_query_sel = (four["bytes"] - one["bytes"]) // 3 - 8 * n
    fixed = one["bytes"] - 8 * n - per_query_sel - _align256(((m * h * plan["qpg"] + 3) & ~3) * 4)
    assert fixed == 6 * 256
    # the batch is the largest that fits: one more query (its keys, its share of the chain, at most one more table) would not
    assert p["batch"] < nq and p["bytes"] + 8 * n + per_query_sel + (one["bytes"] - 8 * n - per_query_sel - fixed) > BULK_USABLE_BYTES


def test_a_billion_rows_are_sliced(rq):
    from rayuela_jl_amd import _lib
    n, nq, m, h, k = 10 ** 9, 1024, 8, 1024, 100
    p = _lib.scan_wide_slices(n, nq, m, h, k)
    plan = _lib.scan_wide_plan(m, h)
    rows, slices = p["rows"], p["slices"]
    assert slices > 1 and p["forced"] == 0
    assert rows * slices >= n
    assert (rows - 1) * slices < n + slices
    assert p["batch"] >= plan["qpg"] and p["batch"] >= plan["qg"]
    assert 0 < p["bytes"] <= BULK_USABLE_BYTES
    # keys of a slice + tables + the chain's 16 k + the three lists' 32 k per query + the 6 * 256 of slack are all counted
    assert p["bytes"] >= _unsliced_lower_bound(rows, p["batch"], m, h, k, plan) + p["batch"] * 4 * k * 8
    # one slice fewer would not fit a query group
    longer = -(-n // (slices - 1))
    assert _unsliced_lower_bound(longer, plan["qg"], m, h, k, plan) + plan["qg"] * 4 * k * 8 > BULK_USABLE_BYTES


def test_one_query_takes_fewer_slices(rq):
    from rayuela_jl_amd import _lib
    p1 = _lib.scan_wide_slices(10 ** 9, 1, 8, 1024, 100)
    p4 = _lib.scan_wide_slices(10 ** 9, 1024, 8, 1024, 100)
    assert p1["batch"] == 1 and 1 < p1["slices"] < p4["slices"]
    assert 8 * p1["rows"] <= p1["bytes"] <= BULK_USABLE_BYTES


def test_hook_overrides_rows_and_is_reported(rq):
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    prev = L.rq_test_scan_wide_slice_rows(257)
    try:
        assert prev == 0
        p = _lib.scan_wide_slices(20_001, 5, 8, 1024, 100)
        assert (p["rows"], p["slices"], p["batch"], p["forced"]) == (257, 78, 5, 1)
        p = _lib.scan_wide_slices(100, 5, 8, 1024, 100)          # never more rows than the base has
        assert (p["rows"], p["slices"], p["forced"]) == (100, 1, 1)
        assert L.rq_test_scan_wide_slice_rows(-3) == 257          # rows <= 0: the planner's choice again
        assert _lib.scan_wide_slices(20_001, 5, 8, 1024, 100)["forced"] == 0
    finally:
        L.rq_test_scan_wide_slice_rows(0)


def test_argument_checks_and_out_of_memory(rq):
    from rayuela_jl_amd import _lib
    for bad in [(0, 1, 8, 1024, 1), (2 ** 31, 1, 8, 1024, 1), (10, 0, 8, 1024, 1), (10, 1, 0, 1024, 1), (10, 1, 33, 1024, 1),
                (10, 1, 8, 0, 1), (10, 1, 8, 32768, 1), (10, 1, 8, 1024, 0), (10, 1, 8, 1024, 11)]:
        with pytest.raises(_lib.RayuelaHipError):
            _lib.scan_wide_slices(*bad)
    # k so large that the lists of one query alone exceed the budget: the scan's out-of-memory status and wording
    with pytest.raises(_lib.RayuelaHipError, match="one query needs more than the BULK_SCRATCH_BYTES budget"):
        _lib.scan_wide_slices(2 * 10 ** 9, 1, 8, 1024, 10 ** 9)
