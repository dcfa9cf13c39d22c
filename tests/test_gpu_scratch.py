"""GPU: no answer of the library depends on what its scratch holds when a call begins.

Library scratch -- the 20 slots of csrc/rq_internal.h per (device, stream), the device pool and the page-locked pool of the
host-pointer calls -- is allocated with slack, never cleared and shared across families ("What a call may assume about
its scratch").  Every other test runs a call on its own leftovers or on fresh, mostly zero, memory.  Here the test hook
rq_test_fill_scratch makes every byte of that scratch 0x00 (what fresh memory usually is), 0xFF (NaN, the maximum key, UINT_MAX
counters, -1 codes), 0x7F (a finite 3.4e38, a large positive integer) and 0x80 (a tiny negative float, a large unsigned) in turn;
after each fill every case of the stream registry (tests/*stream_cases.py: one small oracle-checked case per internal path of every
`void *stream` entry point) and every host-pointer form (at a shape of its family's test file, checked as that file checks it) must
pass its own check and give, byte for byte, the result of a clean run after rq_release_workspaces.  Neither the number of scratch
allocations nor the two pools may move across the call: a regrowth or a fresh pool buffer would hand it fresh memory.  Then the cases run inside the leftovers of the other users of each slot, and in a seeded shuffle with no release.

What shows that the harness sees what it claims: after a fill rq_test_scratch_report finds no slot differing, after a case it names
the slots the case rewrote (printed per case), and over all cases every slot of the enum -- parsed from the header, so a 21st slot
without a case fails -- is rewritten at least once, each case staying inside the slots DESIGN.md lists for its entry point.

Measured on the MI355X, in a run of the whole suite: the 129 GPU tests of this file take 9.6 s together (66 stream cases, 39 host
forms, 20 slots of leftovers, the shuffle, the controls); the slowest are the two quantize_chainq cases at 0.6 s, then
encode_pq_filter_w and the shuffle at 0.6 s; most take under 0.3 s.  (A case whose reference no earlier file of the run has built
pays for it here: run alone, the adc_lut case takes 1.6 s, nearly all of it on the CPU.)  No dependence on scratch content was
found: every case and form passed under every fill, pairing and order."""
import functools
import os
import random
import re

import numpy as np
import pytest

import stream_cases as sc
import aq_wide_stream_cases  # noqa: F401  (registration is otherwise a side effect of the collection order of other files)
import beam_stream_cases  # noqa: F401
import beam_wide_stream_cases  # noqa: F401
import bytes_stream_cases  # noqa: F401
import norms_stream_cases  # noqa: F401
import scan_wide_stream_cases  # noqa: F401
import train_wide_stream_cases  # noqa: F401
import wide_stream_cases  # noqa: F401

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = (0x00, 0xFF, 0x7F, 0x80)
NAMES = sorted(sc.CASES)


def slot_names():
    """The WS_* names of csrc/rq_internal.h in enum order, WS_SLOTS excluded."""
    src = open(os.path.join(ROOT, "rayuela.jl_amd", "csrc", "rq_internal.h")).read()
    body = re.search(r"enum\s*\{\s*(WS_CAND\s*=\s*0.*?)\}", src, flags=re.S).group(1)
    pairs = [(name, int(val)) for name, val in re.findall(r"(WS_[A-Z0-9_]+)\s*=\s*(\d+)", body)]
    assert pairs[-1][0] == "WS_SLOTS" and [v for _, v in pairs] == list(range(len(pairs))), pairs
    return [name for name, _ in pairs[:-1]]


SLOTS = slot_names()

# DESIGN.md, "What a call may assume about its scratch": the slots the launchers behind each entry point may take.  A case that
# rewrites a slot outside its entry's set fails test_every_slot_is_rewritten_by_some_case: the table is then wrong, or a launcher
# has a new user of shared scratch that nobody read.
_SCAN = {"WS_CAND", "WS_COUNTER", "WS_KEYS", "WS_MERGE", "WS_PAD", "WS_BULK"}
_ENC = {"WS_ENCFLAG", "WS_COUNTER"}
_H16 = _ENC | {"WS_H16_SA", "WS_H16_CODES"}
_LSQ = {"WS_TMP", "WS_LSQ_S", "WS_LSQ_A", "WS_LSQ_B"}
ENTRY_SLOTS = {
    "rq_dev_linscan": _SCAN | {"WS_ORDER", "WS_ORDER_TMP", "WS_ORDER_STATE"},
    "rq_dev_linscan_ordered": _SCAN,
    "rq_dev_linscan_aq": _SCAN | {"WS_NORMB"},
    "rq_dev_order_rows": {"WS_ORDER_TMP", "WS_PAD"},
    "rq_dev_merge_topk": {"WS_MERGE", "WS_BULK"},
    "rq_dev_linscan_wide": {"WS_BULK"},
    "rq_dev_linscan_aq_wide": {"WS_BULK"},
    "rq_dev_encode_pq": _ENC,
    "rq_dev_encode_pq_filter_w": _ENC,
    "rq_dev_encode_opq": _ENC | {"WS_TMP"},
    "rq_dev_encode_rvq": _ENC | {"WS_TMP"},
    "rq_dev_encode_pq_bytes": _ENC | {"WS_TMP"},
    "rq_dev_encode_opq_bytes": _ENC | {"WS_TMP"},
    "rq_dev_rotate_T_bytes": {"WS_TMP"},
    "rq_dev_encode_pq_wide": _H16,
    "rq_dev_encode_opq_wide": _H16 | {"WS_TMP"},
    "rq_dev_encode_rvq_wide": _H16 | {"WS_TMP"},
    "rq_dev_update_centers": {"WS_TMP"},
    "rq_dev_update_centers_wide": {"WS_TMP"},
    "rq_dev_gram": {"WS_TMP"},
    "rq_dev_gram_codes": {"WS_TMP"},
    "rq_dev_qerror": {"WS_MERGE"},
    "rq_dev_qerror_codes": {"WS_MERGE"},
    "rq_dev_encode_icm": {"WS_TMP", "WS_ICM_BIN", "WS_ICM_U"},
    "rq_dev_lsq_normal_eq": _LSQ,
    "rq_dev_update_codebooks_lsq": _LSQ,
    "rq_dev_quantize_chainq": {"WS_ICM_BIN", "WS_ICM_U"},
    "rq_dev_update_codebooks_chain": _LSQ | {"WS_CHAIN"},
    "rq_dev_encode_rvq_beam": {"WS_ICM_BIN", "WS_ICM_U"},
    "rq_dev_encode_rvq_beam_wide": {"WS_ICM_BIN", "WS_ICM_U"},
    "rq_dev_aq_norms": {"WS_TMP"},
    "rq_dev_aq_norms_wide": {"WS_TMP"},
    "rq_dev_reconstruct_aq": {"WS_TMP"},
}      # entries not listed take no scratch


def _L():
    from rayuela_jl_amd import _lib
    return _lib


def _release():
    _L().check(_L().lib().rq_release_workspaces())


def _stream_handle():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _differing(stream=None):
    """(names of the slots of the stream that hold a byte other than the last fill's, {slot: allocated bytes})"""
    nbytes, differs = _L().scratch_report(_stream_handle() if stream is None else stream)
    assert len(nbytes) == len(SLOTS), "the binding's WS_SLOTS and the header's enum disagree"
    return {s for s, d in zip(SLOTS, differs) if d}, {s: b for s, b in zip(SLOTS, nbytes) if b}


def _equal_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _run(case):
    if case.precheck:
        from switch_table import switches
        with switches(**case.switches):
            case.precheck()
    got = sc.run_plain(case)
    if case.after:
        case.after()
    return got


# Outputs that are not a function of the inputs, so no two runs give the same bytes whatever the scratch holds; `check` still holds
# them to their contract after every fill.  order_rows: rows of one sort bucket land in the order of the scatter's atomics
# (stream_cases._ordered_base; csrc/rq_order.hip), so the permutation and the rows moved by it are each run's own.
RUN_DEPENDENT = {"order_rows": {"ordered", "perm"}}

REWRITTEN = {}        # case name -> (slots rewritten, {slot: bytes allocated}) after a run on filled scratch
POOLS = {"device": 0, "pinned": 0}      # most bytes one fill found idle in the device pool / the page-locked pool


def _pools(rep):
    return rep["pool_bytes"], rep["pool_buffers"], rep["pinned_bytes"], rep["pinned_blocks"]


def _note_pools(rep):
    POOLS["device"] = max(POOLS["device"], rep["pool_bytes"])
    POOLS["pinned"] = max(POOLS["pinned"], rep["pinned_bytes"])


def _invariance(name, clean_run, check):
    """release, clean run, then per fill value: fill, run, check, bytes equal to the clean run, no new allocation.  Returns the
    slots the runs rewrote (the union over the fills: a flag that a call resets to 0 shows under 0xFF, not under 0x00)."""
    L = _L()
    _release()
    want = clean_run()
    check(want)
    rep = L.fill_scratch(FILLS[0])
    slots, nbytes = set(), {}
    for i, value in enumerate(FILLS):
        _note_pools(rep)
        assert _differing()[0] == set(), "slots differ from the fill before any call ran"
        gen, pools = rep["ws_gen"], _pools(rep)
        got = clean_run()
        rewritten = _differing()
        slots |= rewritten[0]
        nbytes = rewritten[1]
        # the next fill also tells how many allocations the library has made by now
        rep = L.fill_scratch(FILLS[i + 1] if i + 1 < len(FILLS) else FILLS[0])
        assert rep["ws_gen"] == gen, "%s: scratch regrew across the call on 0x%02X-filled scratch: the trial is void" % (name, value)
        # ... and a host-pointer call that took a fresh device or page-locked buffer leaves one more in its pool afterwards
        assert _pools(rep) == pools, "%s: the pools changed across the call on 0x%02X-filled scratch (%s -> %s): it ran on fresh " \
                                     "buffers and the trial is void" % (name, value, pools, _pools(rep))
        try:
            check(got)
        except AssertionError as e:
            raise AssertionError("%s fails its check on 0x%02X-filled scratch (slots it rewrote: %s): %s"
                                 % (name, value, sorted(rewritten[0]), e)) from e
        assert sorted(got) == sorted(want)
        bad = [k for k in sorted(want) if k not in RUN_DEPENDENT.get(name, ()) and not _equal_bytes(got[k], want[k])]
        assert not bad, "%s: outputs %s differ from the clean run on 0x%02X-filled scratch (slots it rewrote: %s)" % (
            name, bad, value, sorted(rewritten[0]))
    return slots, nbytes


# ---- a. invariance of every `void *stream` case -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_case_does_not_depend_on_scratch_content(rq, name):
    case = sc.get(name)
    REWRITTEN[name] = _invariance(name, lambda: _run(case), case.check)
    slots, nbytes = REWRITTEN[name]
    print("%s rewrites: %s" % (name, ", ".join("%s (%d B)" % (s, nbytes[s]) for s in SLOTS if s in slots) or "no scratch"))


def _slots_of(name):
    """The slots case `name` rewrites (measured by the test above, or here when that one was deselected)."""
    if name not in REWRITTEN:
        case = sc.get(name)
        _release()
        case.check(_run(case))
        slots, nbytes = set(), {}
        for value in (0xFF, 0x00):
            _L().fill_scratch(value)
            case.check(_run(case))
            slots |= _differing()[0]
            nbytes = _differing()[1]
        REWRITTEN[name] = (slots, nbytes)
    return REWRITTEN[name]


# ---- d. the harness sees what it claims ------------------------------------------------------------------------------------------
@gpu
def test_every_slot_is_rewritten_by_some_case(rq):
    assert len(SLOTS) == _L().WS_SLOTS
    seen, outside = {}, []
    for name in NAMES:
        slots, _ = _slots_of(name)
        entry = sc.CASES[name][0]
        for s in sorted(slots):
            seen.setdefault(s, []).append(name)
            if s not in ENTRY_SLOTS.get(entry, set()):
                outside.append("%s (%s) rewrites %s" % (name, entry, s))
    for s in SLOTS:
        print("%s: %s" % (s, ", ".join(seen.get(s, [])) or "-"))
    assert not outside, "users of scratch the slot table of DESIGN.md does not list: " + "; ".join(outside)
    missing = [s for s in SLOTS if s not in seen]
    assert not missing, "no case rewrites %s: add a small case to the matching *_stream_cases.py" % missing


@gpu
def test_report_is_clean_after_a_fill_and_names_what_a_case_wrote(rq):
    """The control of the harness itself: a fill leaves no slot differing, whatever the value and on every stream that holds
    scratch; one case dirties exactly its own stream's slots; an untouched stream stays clean."""
    import torch
    L = _L()
    _release()
    case = sc.get("encode_opq")                 # WS_TMP (the rotated rows) and the encode filter's flags
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        case.check(_run(case))
    case.check(_run(case))
    for value in FILLS:
        rep = L.fill_scratch(value)
        assert rep["slots"] >= 4 and rep["slot_bytes"] >= 2 * case.inputs["X"].nbytes, rep
        assert _differing(0)[0] == set() and _differing(side.cuda_stream)[0] == set()
    case.check(_run(case))
    slots, nbytes = _differing(0)
    assert "WS_TMP" in slots and nbytes["WS_TMP"] >= case.inputs["X"].nbytes + case.inputs["X"].nbytes // 4
    assert _differing(side.cuda_stream)[0] == set(), "a call on the null stream wrote another stream's scratch"
    with pytest.raises(L.RayuelaHipError):
        L.fill_scratch(256)
    torch.cuda.synchronize()
    _release()
    assert _differing(0) == (set(), {}), "a release leaves no scratch to report"


# ---- b. the host-pointer forms: the aux stream pair, the device pool, the page-locked pool -----------------------------------------
# Every form runs at a shape of its family's own test file, on that file's data helper, and `check` is that file's comparison
# with its oracle / restatement.  The references are computed once, before the first release.  Three kinds of reference:
#   oracle      a CPU oracle or restatement of the whole call (encoders, scans, ICM, chain, beam, norms, train_opq, train_ervq);
#   contract    train_pq / train_rvq: the returned codes are the CPU oracle's encode of the returned codebooks and the returned
#               error is their f64 error.  The Lloyd trajectory itself is pinned by tests/test_gpu_kmeans.py and
#               tests/test_gpu_train_wide.py, whose telescoping needs the library's own state after every iteration (k calls);
#   composed    train_lsq, train_sr, train_chainq, get_norms_codebook: their family files have no CPU restatement of the loop at
#               any size; they compare with the same steps taken through the public entry points, and so does `check` here,
#               against a composition run once on clean scratch.
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def _named(names, call):
    def run():
        out = call()
        out = out if isinstance(out, tuple) else (out,)
        assert len(out) == len(names), (len(out), names)
        return {k: (np.array(v) if not isinstance(v, list) else np.stack(v)) for k, v in zip(names, out) if k != "_"}
    return run


@functools.lru_cache(maxsize=None)
def _smoke_data():
    """__graft_entry__.smoke()'s shape: what tests/test_gpu_encode.py and test_gpu_scan.py anchor to the oracle."""
    import rayuela_jl_amd.synth as synth
    g = {}
    n, d, m, h = 20_000, 128, 8, 256
    g["X"] = synth.sift_like(n, d, seed=1)
    g["Xb"] = np.clip(np.rint(g["X"]), 0, 255).astype(np.uint8)
    g["Q"] = synth.sift_like(24, d, seed=2)
    g["Qbig"] = synth.sift_like(1_100, d, seed=4)           # 1100 x 1000 results: 4.4 MB each, page-locked (_lib._PIN_MIN_BYTES)
    g["C"] = synth.codebooks(g["X"], m, h, seed=3, iters=1, sample=4000)
    g["R"] = synth.rotation(d)
    g["codes"] = synth.random_codes(n, m, seed=n)
    return g


def _f_encode(which):
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    g, o = _smoke_data(), _orc()
    cat = synth.cat_codebooks(g["C"])
    if which == "pq":
        ref, call = o.encode_pq(g["X"], cat, 8, 256), lambda: rq.quantize_pq(g["X"], g["C"])
    elif which == "opq":
        ref, call = o.encode_opq(g["X"], g["R"], cat, 8, 256), lambda: rq.quantize_opq(g["X"], g["R"], g["C"])
    else:
        ref, call = o.encode_pq(g["Xb"].astype(np.float32), cat, 8, 256), lambda: rq.quantize_pq(g["Xb"], g["C"])
    ref = ref.astype(np.int16) + 1

    def check(got):
        assert np.array_equal(got["B"], ref), "codes differ from the oracle"
    return _named(("B",), call), check


def _check_scan(d0, i0):
    def check(got):
        assert np.array_equal(got["idx"].astype(np.int64), np.asarray(i0).astype(np.int64)), "ids differ from the oracle"
        assert _same(got["dists"], d0), "distances differ from the oracle"
    return check


def _f_scan(which):
    import rayuela_jl_amd as rq
    g, o = _smoke_data(), _orc()
    cen = np.stack(g["C"])
    if which == "pq":
        d0, i0 = o.linscan_aqd_query(g["codes"], cen, g["Q"], 100)
        call = lambda: rq.linscan_pq(g["codes"], g["Q"], g["C"], 64, 100)              # noqa: E731
    elif which == "pinned":
        d0, i0 = o.linscan_aqd_query(g["codes"], cen, g["Qbig"], 1000)
        call = lambda: rq.linscan_pq(g["codes"], g["Qbig"], g["C"], 64, 1000)          # noqa: E731
    else:
        d0, i0 = o.linscan_aqd_query(g["codes"], cen, o.rotate_T(g["R"], g["Q"]), 100)
        call = lambda: rq.linscan_opq(g["codes"], g["Q"], g["C"], 64, g["R"], 100)     # noqa: E731
    return _named(("dists", "idx"), call), _check_scan(d0, np.asarray(i0).astype(np.int64) + 1)


def _f_scan_aq(lsq):
    """tests/test_gpu_aq.py::test_aq_vs_oracle_random's shape (the one of stream_cases._linscan_aq)."""
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    n, m, d, nq, K = 100_003, 16, 96, 9, 100
    rng = np.random.default_rng(n + m)
    cb = rng.standard_normal((m * 256, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=n)
    nrm = (rng.random(n) * 50).astype(np.float32)
    C = [cb[i * 256:(i + 1) * 256] for i in range(m)]
    o = _orc()
    if lsq:
        d0, i0 = o.linscan_lsq(codes, cb, q, nrm, K)
        return _named(("dists", "idx"), lambda: rq.linscan_lsq(codes, q, C, nrm, np.eye(d, dtype=np.float32), K)), _check_scan(d0, i0)
    d0, i0 = o.linscan_cq(codes, cb, q, K)
    return _named(("dists", "idx"), lambda: rq.linscan_cq(codes, q, C, K)), _check_scan(d0, i0)


def _f_encode_wide(which):
    """tests/test_gpu_encode_wide.py::test_python_mirrors."""
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    import test_gpu_encode_wide as tw
    import wide_oracle as wo
    o = _orc()
    if which == "rvq":
        X, Cs, (codes0, counts0, Xr0) = tw._rvq_case((3001, 64, 3, 300))
        Cl = [Cs[i] for i in range(3)]

        def check(got):
            assert got["B"].dtype == np.uint16 and np.array_equal(got["B"], codes0.astype(np.uint16))
            assert np.array_equal(got["counts"], counts0) and _same(got["Xr"], Xr0)
        return _named(("B", "counts", "Xr"), lambda: rq.quantize_rvq_u16(X, Cl, with_extras=True)), check
    shape = (3001, 32, 4, 300)
    n, d, m, h = shape
    X, Ccat, ref = tw._case(shape, "sift")
    C, _ = wo.sub_codebooks(Ccat, d, m, h)
    if which == "opq":
        R = synth.rotation(d, seed=d)
        ref = wo.encode_pq_wide(o, o.rotate_T(R, X), Ccat, m, h)
        call = lambda: rq.quantize_opq_u16(X, R, C)       # noqa: E731
    else:
        call = lambda: rq.quantize_pq_u16(X, C)           # noqa: E731

    def check(got):
        assert got["B"].dtype == np.uint16 and np.array_equal(got["B"], ref.astype(np.uint16)), "codes differ from the helper"
    return _named(("B",), call), check


def _f_quantize_rvq():
    """tests/test_gpu_beam.py::test_beam_of_one_is_quantize_rvq's shape: the restated beam of one is quantize_rvq."""
    import beam_oracle as bo
    import rayuela_jl_amd as rq
    X, C, codes, Xr, cost = bo.expected(bo.GPU_SHAPES[0], 1)

    def check(got):
        assert np.array_equal(got["B"], codes.astype(np.int16) + 1)
    return _named(("B", "_"), lambda: rq.quantize_rvq(X, list(C))), check


def _f_scan_wide(opq):
    """tests/test_gpu_scan_wide.py::test_host_mirrors_pq_and_opq."""
    import rayuela_jl_amd as rq
    import scan_wide_oracle as swo
    import test_gpu_scan_wide as tsw
    o = _orc()
    n, m, h, sub, nq, k = 20_000, 4, 1000, 4, 11, 500
    codes, centers, queries = tsw._data(n, m, h, sub, nq, seed=21)
    C = [centers[j] for j in range(m)]
    B = codes.view(np.uint16)
    if opq:
        R = np.linalg.qr(np.random.default_rng(4).standard_normal((m * sub, m * sub)))[0].astype(np.float32)
        ref = swo.scan(o, codes, centers, o.rotate_T(R, queries), k, id_base=1)
        call = lambda: rq.linscan_opq_u16(B, queries, C, R, k)        # noqa: E731
    else:
        ref = swo.scan(o, codes, centers, queries, k, id_base=1)
        call = lambda: rq.linscan_pq_u16(B, queries, C, k)            # noqa: E731

    def check(got):
        assert swo.same(got["dists"], got["idx"], ref), swo.first_difference(got["dists"], got["idx"], ref)
    return _named(("dists", "idx"), call), check


def _f_scan_aq_wide(lsq):
    """tests/test_gpu_aq_wide.py::test_host_mirrors."""
    import aq_wide_oracle as awo
    import rayuela_jl_amd as rq
    n, m, h, d, nq, k = 20_000, 4, 1000, 12, 11, 500
    codes, C, q, nrm = awo.case(n, m, h, d, nq, 21)
    Cl = [C[j] for j in range(m)]
    B = codes.view(np.uint16)
    ref = awo.scan(codes, C, q, k, nrm if lsq else None, id_base=1)
    call = (lambda: rq.linscan_lsq_u16(B, q, Cl, nrm, None, k)) if lsq else (lambda: rq.linscan_cq_u16(B, q, Cl, k))

    def check(got):
        assert awo.same(got["dists"], got["idx"], ref)
    return _named(("dists", "idx"), call), check


def _f_encode_icm():
    """tests/test_gpu_icm.py::test_shapes_bit_exact at (m, h, d) = (8, 256, 32)."""
    import icm_oracle as io
    import test_gpu_icm as ti
    m, h, d = 8, 256, 32
    X, C, B0 = ti._data(200, d, m, h, seed=m * 1000 + h + d)
    args = (2, 2, 2, (m + d) % 2 == 0)
    b0, c0 = io.ils(_orc(), X, C, B0, *args, seed=5)

    def check(got):
        ti._assert_same((got["B"], got["cost"]), (b0, c0))
    return _named(("B", "cost"), lambda: ti._gpu(X, C, B0, *args, seed=5, nsplits=2)), check


def _f_encode_icm_wide(ties):
    """rq_encode_icm_wide: the shape of tests/test_gpu_icm_wide.py's `inv` fixture, (101, 16, 4, 300), or the (4, 300, 256) case of
    tests/icm_tie_cases.py, where a copy in the short last piece ties with its original.  The padding of U and binT past h = 300
    keeps the fill."""
    import icm_tie_cases as tc
    import icm_wide_oracle as wo
    import test_gpu_icm_wide as tw
    if ties:
        case = tc.WIDE_LOW[4]
        assert (case.m, case.h, case.P) == (4, 300, 256)
        X, C, B0, b0, c0 = tc.expected(case)
        args, seed = case.args, tc.ILS_SEED
    else:
        X, C, B0 = tw._data(101, 16, 4, 300, seed=6)
        args, seed = (4, 2, 2, True), 3
        b0, c0 = wo.ils(_orc(), X, C, B0, *args, seed=seed)

    def check(got):
        tw._assert_same((got["B"], got["cost"]), (b0, c0))
    return _named(("B", "cost"), lambda: tw._gpu(X, C, B0, *args, seed=seed, nsplits=2)), check


def _f_chainq():
    """tests/test_gpu_chainq.py::test_codes_equal_the_restatement at (8, 256, 128, 257)."""
    import chain_oracle as co
    from rayuela_jl_amd.ChainQ import quantize_chainq_u8
    m, h, d, n = 8, 256, 128, 257
    rng = np.random.default_rng(m * 1000 + h + d + n)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    want = co.viterbi(_orc(), X, C)

    def check(got):
        assert np.array_equal(got["B"], want), "rows differ: %d of %d" % (int((got["B"] != want).any(axis=1).sum()), n)
    return _named(("B",), lambda: quantize_chainq_u8(X, C, nsplits=4)), check


def _f_beam(H, wide):
    """tests/test_gpu_beam.py / test_gpu_beam_wide.py::test_codes_residual_and_cost_equal_the_restatement (their first shape)."""
    import rayuela_jl_amd as rq
    if wide:
        import beam_wide_oracle as bw
        X, C, codes, Xr, cost = bw.expected(bw.GPU_SHAPES[0][:5], H)
        call = lambda: rq.quantize_competitiveq_u16(X, list(C), H, nsplits=3, with_extras=True)      # noqa: E731
    else:
        import beam_oracle as bo
        X, C, codes, Xr, cost = bo.expected(bo.GPU_SHAPES[0], H)
        call = lambda: rq.quantize_competitiveq_u8(X, list(C), H, nsplits=3, with_extras=True)       # noqa: E731

    def check(got):
        assert np.array_equal(got["B"].view(np.int16) if wide else got["B"], codes), "codes differ from the restatement"
        assert _same(got["Xr"], Xr) and _same(got["cost"], cost)
    return _named(("B", "cost", "Xr"), call), check


def _f_norms(which):
    """tests/test_gpu_norms.py::test_host_quantize_from_codes / test_norms_codebook_equals_train_pq_on_the_norms and
    tests/test_gpu_aq_wide.py::test_host_norm_entries."""
    import aq_wide_oracle as awo
    import norms_oracle as no
    import rayuela_jl_amd as rq
    if which == "quantize":
        codes, C = no.norm_case(1007, 96, 16, 256)
        norms = no.aq_norms(codes, C)
        cb = np.ascontiguousarray(np.random.default_rng(5).permutation(np.linspace(norms.min(), norms.max(), 255)), dtype=np.float32)
        B1, want = codes.astype(np.int16) + 1, no.quantize(norms, cb)

        def check(got):
            assert np.array_equal(got["codes"] - 1, want) and _same(got["norms"], norms)
        return _named(("codes", "norms"), lambda: rq.quantize_norms(B1, list(C), cb)), check
    if which == "quantize_wide":
        codes, C, _, _ = awo.case(4096, 2, 300, 16, 1, 71)
        norms = no.aq_norms(codes, C)
        cb = np.random.default_rng(5).permutation(np.linspace(0, 60, 700)).astype(np.float32)
        B1, want = codes + np.int16(1), awo.quantize(norms, cb)

        def check(got):
            assert got["codes"].dtype == np.int16 and np.array_equal(got["codes"].astype(np.int64) - 1, want)
            assert _same(got["norms"], norms)
        return _named(("codes", "norms"), lambda: rq.utils.quantize_norms(B1, [C[j] for j in range(2)], cb)), check
    # the norms codebook is train_pq(d = 1, m = 1, h) on the restated norms: composed once, here
    if which == "codebook":
        (codes, C), h, niter, seed = no.norm_case(3000, 32, 4, 256), 256, 12, 3
        Cl = list(C)
    else:
        codes, C, _, _ = awo.case(4096, 2, 300, 16, 1, 71)
        h, niter, seed, Cl = 300, 7, 3, [C[j] for j in range(2)]
    norms = no.aq_norms(codes, C)
    B1 = codes.astype(np.int16) + 1
    Cn, Bn, _ = rq.train_pq(np.ascontiguousarray(norms.reshape(-1, 1)), 1, h, niter=niter, seed=seed)

    def check(got):
        assert _same(got["cb"], Cn[0][:, 0]) and np.array_equal(got["codes"], Bn[:, 0].astype(np.int64))
    return _named(("codes", "cb"), lambda: rq.utils.get_norms_codebook(B1, Cl, niter=niter, seed=seed)), check


def _f_train_pq(wide):
    """contract.  Fixtures: tests/test_gpu_kmeans.py::_lloyd_fixture("sift"), tests/train_wide_oracle.py::lloyd_fixture("sift")."""
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    import wide_oracle as wo
    o = _orc()
    if wide:
        import train_wide_oracle as two
        X, m, h, (seed,), _ = two.lloyd_fixture("sift")
    else:
        X, m, h, seed = synth.sift_like(6000, 32, seed=31), 4, 32, 4
    n, d = X.shape

    def check(got):
        cat = np.concatenate([c.reshape(-1) for c in got["C"]])
        codes = wo.encode_pq_wide(o, X, cat, m, h) if wide else o.encode_pq(X, cat, m, h)
        assert np.array_equal(got["B"], codes.astype(np.int16) + 1), "B is not the oracle's encode of the returned codebooks"
        sub = d // m
        rec = np.concatenate([got["C"][i][codes[:, i].astype(np.int64)] for i in range(m)], axis=1).astype(np.float64)
        e0 = ((X.astype(np.float64) - rec) ** 2).sum() / n
        assert sub * m == d and abs(float(got["err"]) - e0) <= 1e-6 * e0, (float(got["err"]), e0)
    return _named(("C", "B", "err"), lambda: rq.train_pq(X, m, h, niter=2, seed=seed)), check


def _f_train_rvq(wide):
    """contract.  Shapes: tests/test_gpu_rvq.py::test_train_rvq_contract; tests/train_wide_oracle.py::lloyd_fixture("one_past_a_block")."""
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    import wide_oracle as wo
    o = _orc()
    if wide:
        import train_wide_oracle as two
        X, _, h, (seed,), _ = two.lloyd_fixture("one_past_a_block")
        m = 2
    else:
        X, m, h, seed = synth.sift_like(20_000, 64, seed=21), 4, 64, 3
    n = X.shape[0]

    def check(got):
        Cs = np.ascontiguousarray(got["C"])
        codes = wo.encode_rvq_wide(o, X, Cs)[0] if wide else o.encode_rvq(X, Cs)
        assert np.array_equal(got["B"], np.asarray(codes).astype(np.int16) + 1), "B is not the oracle's encode of the returned codebooks"
        rec = sum(Cs[i][got["B"][:, i].astype(np.int64) - 1].astype(np.float64) for i in range(m))
        e64 = ((X.astype(np.float64) - rec) ** 2).sum() / n
        assert abs(float(got["err"]) - e64) <= 1e-5 * e64, (float(got["err"]), e64)
    return _named(("C", "B", "err"), lambda: rq.train_rvq(X, m, h, niter=2, seed=seed)), check


def _f_train_opq(wide):
    """tests/test_gpu_train.py::test_train_opq_follows_the_oracle_loop / test_gpu_train_wide.py::test_train_opq_wide_follows_the_
    restated_loop, two iterations, their bars."""
    import rayuela_jl_amd as rq
    import rayuela_jl_amd.synth as synth
    o = _orc()
    n, d, m, h, niter = 12000, 32, 4, (300 if wide else 32), 2
    X = synth.sift_like(n, d, seed=3) if wide else synth.sift_like(n, d, seed=4)      # test_gpu_train._setup(seed=3): seed + 1
    R0 = synth.rotation(d, seed=5)
    C0 = synth.codebooks(o.rotate_T(R0, X), m, h, seed=9, iters=0, sample=2000)
    if wide:
        import train_wide_oracle as two
        _, codes_o, _, obj_o = two.train_opq(o, X, m, h, niter, R0, C0)
    else:
        from oracle import train_oracle as to
        _, codes_o, _, obj_o = to.train_opq(X, m, h, niter, R0, C0)

    def check(got):
        obj, R, B = got["obj"], got["R"], got["B"]
        assert obj.shape == (niter + 1,) and np.allclose(obj, obj_o, rtol=3e-4), (obj, obj_o)
        assert (np.diff(obj) <= 1e-5 * obj[:-1]).all() and np.abs(R @ R.T - np.eye(d)).max() < 1e-5
        assert (B - 1 != codes_o).mean() < 2e-2
    return _named(("C", "B", "R", "obj"), lambda: rq.train_opq(X, m, h, niter, "natural", R0=R0, C0=C0)), check


def _f_train_ervq(wide):
    """tests/test_gpu_ervq.py / test_gpu_ervq_wide.py::test_train_ervq*_follows_the_restatement: their fixtures and bars, two
    iterations (a prefix of the byte file's three)."""
    import ervq_oracle as eo
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd.ERVQ import train_ervq_i16
    o = _orc()
    if wide:
        import wide_oracle as wo
        X = synth.sift_like(20000, 32, seed=41)
        C = synth.rvq_codebooks(X, 2, 257, seed=42, sample=20000)

        def enc(X_, C_, with_extras=False):
            out = wo.encode_rvq_wide(o, X_, C_)
            return out if with_extras else out[0]
        bar = 10 * 2.52e-10
    else:
        enc, bar = o.encode_rvq, 10 * 5.342e-10
        X, _, C = eo.fixture(enc)
    codes = enc(X, C)
    Cr, Br, objr = eo.incremental(X, codes, C, 2, enc, np.float32)[:3]
    m, h = C.shape[0], C.shape[1]

    def check(got):
        trace = np.abs(got["obj"] - objr) / objr
        assert trace.max() <= min(bar, 3e-4), trace
        assert float(np.mean((got["B"] - 1) != Br)) == 0.0
    return _named(("C", "B", "err", "obj"), lambda: train_ervq_i16(X, np.asarray(codes).astype(np.int16) + 1, C, m, h, 2)), check


def _f_train_aq(which):
    """composed.  tests/test_gpu_lsq_train.py::test_train_lsq_equals_composed_steps, tests/test_gpu_sr.py::test_train_sr_equals_
    composed_steps (seeded rotation, clean update) and tests/test_gpu_chainq.py::test_train_chainq_equals_composed_steps, at
    their shapes, two iterations."""
    if which == "chainq":
        import test_gpu_chainq as tc
        from rayuela_jl_amd.ChainQ import train_chainq_u8
        from test_chain_oracle import train_case
        X, B0, R0, h = train_case()
        m = B0.shape[1]
        ref = tc._composed(X, B0, R0, h, 2)
        names, call = ("C", "B", "R", "obj"), lambda: train_chainq_u8(X, B0, m, h, R0, 2)       # noqa: E731
    else:
        import test_gpu_sr as ts
        X, codes0, m, h = ts._small()
        R = ts._rotation(X.shape[1], 5)
        niter, ilsiter, icmiter, npert, randord, seed = 2, 2, 2, 2, True, 9
        names = ("C", "B", "obj")
        if which == "lsq":
            import test_gpu_lsq_train as tl
            from rayuela_jl_amd.LSQ import train_lsq_u8
            ref = tl._composed(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, randord, seed)
            call = lambda: train_lsq_u8(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, seed=seed, nsplits=2)    # noqa: E731
        else:
            from rayuela_jl_amd.SR import train_sr_u8
            ref = ts._composed(X, codes0, m, h, R, niter, ilsiter, icmiter, npert, randord, seed, which, 1, 0.5, True)
            call = lambda: train_sr_u8(X, codes0, m, h, R, niter, ilsiter, icmiter, randord, npert, which, 1, 0.5, True,      # noqa: E731
                                       seed=seed, nsplits=2)

    def check(got):
        assert np.array_equal(got["B"], ref[1]) and _same(got["C"], ref[0])
        if which == "chainq":
            assert _same(got["R"], ref[2]) and _same(got["obj"], ref[3])
        else:
            assert np.allclose(got["obj"], ref[2], rtol=1e-12, atol=0)
    return _named(names, call), check


HOST_FORMS = {
    "quantize_pq": lambda: _f_encode("pq"),
    "quantize_opq": lambda: _f_encode("opq"),
    "quantize_pq_bytes": lambda: _f_encode("bytes"),
    "quantize_rvq": _f_quantize_rvq,
    "quantize_pq_u16": lambda: _f_encode_wide("pq"),
    "quantize_opq_u16": lambda: _f_encode_wide("opq"),
    "quantize_rvq_u16": lambda: _f_encode_wide("rvq"),
    "linscan_pq": lambda: _f_scan("pq"),
    "linscan_pq_pinned_results": lambda: _f_scan("pinned"),
    "linscan_opq": lambda: _f_scan("opq"),
    "linscan_lsq": lambda: _f_scan_aq(True),
    "linscan_cq": lambda: _f_scan_aq(False),
    "linscan_pq_u16": lambda: _f_scan_wide(False),
    "linscan_opq_u16": lambda: _f_scan_wide(True),
    "linscan_lsq_u16": lambda: _f_scan_aq_wide(True),
    "linscan_cq_u16": lambda: _f_scan_aq_wide(False),
    "encode_icm": _f_encode_icm,
    "encode_icm_u16": lambda: _f_encode_icm_wide(False),
    "encode_icm_u16_ties": lambda: _f_encode_icm_wide(True),
    "quantize_chainq": _f_chainq,
    "quantize_competitiveq_H1": lambda: _f_beam(1, False),
    "quantize_competitiveq_H4": lambda: _f_beam(4, False),
    "quantize_competitiveq_u16_H4": lambda: _f_beam(4, True),
    "get_norms_codebook": lambda: _f_norms("codebook"),
    "quantize_norms": lambda: _f_norms("quantize"),
    "get_norms_codebook_wide": lambda: _f_norms("codebook_wide"),
    "quantize_norms_wide": lambda: _f_norms("quantize_wide"),
    # the seeded trainers: bit-reproducible per seed (tests/test_gpu_train.py), two iterations each
    "train_pq": lambda: _f_train_pq(False),
    "train_pq_h300": lambda: _f_train_pq(True),
    "train_opq": lambda: _f_train_opq(False),
    "train_opq_h300": lambda: _f_train_opq(True),
    "train_rvq": lambda: _f_train_rvq(False),
    "train_rvq_h257": lambda: _f_train_rvq(True),
    "train_ervq": lambda: _f_train_ervq(False),
    "train_ervq_h257": lambda: _f_train_ervq(True),
    "train_lsq": lambda: _f_train_aq("lsq"),
    "train_chainq": lambda: _f_train_aq("chainq"),
    "train_sr_c": lambda: _f_train_aq("SR_C"),
    "train_sr_d": lambda: _f_train_aq("SR_D"),
}


@functools.lru_cache(maxsize=None)
def _host_form(name):
    return HOST_FORMS[name]()


@gpu
@pytest.mark.parametrize("name", sorted(HOST_FORMS))
def test_host_form_does_not_depend_on_scratch_content(rq, name):
    run, check = _host_form(name)
    slots, nbytes = _invariance(name, run, check)
    print("%s rewrites on the null stream: %s" % (name, ", ".join(s for s in SLOTS if s in slots) or "no scratch"))


@gpu
def test_both_pools_were_filled(rq):
    """The device pool and the page-locked pool each held idle bytes at some fill of the host forms above (when this test runs
    alone: of the two forms it runs itself)."""
    if not (POOLS["device"] and POOLS["pinned"]):
        for name in ("quantize_pq", "linscan_pq_pinned_results"):
            _invariance(name, *_host_form(name))
    print("idle bytes found by one fill: device pool %d, page-locked pool %d" % (POOLS["device"], POOLS["pinned"]))
    assert POOLS["device"] > 0 and POOLS["pinned"] > 0, POOLS


# ---- c. leftovers of another family ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("slot", SLOTS)
def test_case_runs_inside_the_leftovers_of_the_slots_other_users(rq, slot):
    """A: the case with the largest allocation of `slot`.  B: the smallest case of every other entry point that rewrites the slot
    (and, for A's own entry point, behind the largest case of another one).  A then B with no release and no fill in between: B
    runs inside A's leftovers and must pass its check."""
    users = {}
    for name in NAMES:
        slots, nbytes = _slots_of(name)
        if slot in slots:
            users.setdefault(sc.CASES[name][0], []).append((nbytes[slot], name))
    if not users:
        print("%s: no user; see test_every_slot_is_rewritten_by_some_case" % slot)
        return
    ranked = sorted((max(cases), entry) for entry, cases in users.items())
    (_, a1), e1 = ranked[-1]
    pairs = [(a1, min(cases)[1]) for entry, cases in sorted(users.items()) if entry != e1]
    if len(ranked) > 1:
        pairs.append((ranked[-2][0][1], min(users[e1])[1]))
    # two shapes of one entry point: its smallest case inside its largest one's leftovers (the only pair of a slot with one user)
    pairs += [(max(cases)[1], min(cases)[1]) for entry, cases in sorted(users.items()) if max(cases)[1] != min(cases)[1]]
    # A must hold at least B's allocation, or B regrows the slot and runs on fresh memory: keep the pairs that are inside
    sizes = {name: nb for cases in users.values() for nb, name in cases}
    pairs = [(a, b) for a, b in dict.fromkeys(pairs) if sizes[a] >= sizes[b]]
    _release()
    for a, b in pairs:
        ca, cb = sc.get(a), sc.get(b)
        ca.check(_run(ca))
        before = _L().scratch_report(_stream_handle())[0][SLOTS.index(slot)]
        try:
            cb.check(_run(cb))
        except AssertionError as e:
            raise AssertionError("%s fails its check inside the leftovers of %s (shared %s): %s" % (b, a, slot, e)) from e
        after = _L().scratch_report(_stream_handle())[0][SLOTS.index(slot)]
        assert after == before > 0, "%s regrew %s after %s (%d -> %d bytes): it ran on fresh memory, the pair is void" % (
            b, slot, a, before, after)
    print("%s: %d pairs: %s" % (slot, len(pairs), ", ".join("%s -> %s" % p for p in pairs) or "one case only"))


@gpu
def test_seeded_shuffle_of_all_cases_twice_with_no_release(rq):
    order = list(NAMES)
    random.Random(20).shuffle(order)
    _release()
    done = []
    for name in order + order:
        case = sc.get(name)
        try:
            case.check(_run(case))
        except AssertionError as e:
            raise AssertionError("%s fails its check after %s: %s" % (name, done[-6:], e)) from e
        done.append(name)


# ---- e. coverage, without a GPU ----------------------------------------------------------------------------------------------------
def test_every_entry_is_covered_and_both_hooks_are_declared_and_bound():
    from test_cabi import _header_prototypes
    from rayuela_jl_amd import _lib
    assert {sc.CASES[name][0] for name in NAMES} == sc.ENTRIES
    protos = _header_prototypes()
    declared = {name for name, (_, params) in protos.items() if params and params[-1] == ("void *", "stream")}
    assert declared == sc.ENTRIES, (sorted(declared - sc.ENTRIES), sorted(sc.ENTRIES - declared))
    assert set(ENTRY_SLOTS) <= sc.ENTRIES and all(v <= set(SLOTS) for v in ENTRY_SLOTS.values())
    header = open(os.path.join(ROOT, "include", "rayuela_hip.h")).read()
    assert "test hooks: not for callers" in header
    for hook in ("rq_test_fill_scratch", "rq_test_scratch_report"):
        assert hook in protos and hook in _lib.SIGNATURES, hook
        assert ("void *", "stream") not in protos[hook][1], "%s takes no stream to be ordered on" % hook
    assert len(SLOTS) == _lib.WS_SLOTS
