"""GPU: the calling contract of include/rayuela_hip.h around the values -- stream ordering of every `void *stream` entry point,
host threads, the (device, stream) scratch key and the limit of 8 streams per device.

Every other test passes torch's default stream, which on PyTorch-ROCm is the null stream; pool streams are non-blocking.  A
kernel, memset or scratch reset that the library launched on the wrong stream (a forgotten `stream` argument) gives the right
answer there and a race for a caller on a side stream.  Here every entry point runs on a side stream behind a delay
(stream_cases.run_on_side_stream: poison, delay, fill, call, consume, poison) and must give the expected output of its
family's own tests, compared the same way.  (What library scratch holds when a call begins -- a reset that is missing, or that
ran early while nothing dirtied the scratch, a read of an earlier call's intermediates -- is tests/test_gpu_scratch.py's
subject, with these same cases.)  The coverage is derived: test_every_stream_entry_point_has_a_case (no GPU needed)
parses the header for the prototypes that end in `void *stream`.

The delay is an input of the test, not a threshold of the library.  DELAY_CYCLES = 20 000 000 cycles of torch.cuda._sleep,
measured on the MI355X at 8.4 ms (4.18 ms per 1e7 cycles, 41.7 ms per 1e8).  How it was chosen: the control of this file (a
torch copy issued on a second pool stream with no event wait) was caught by the harness in 19 of 20 repetitions with no delay
and in 20 of 20 at 1 000, 1e4, 1e5, 1e6, 1e7, 2e7 and 5e7 cycles, with no false alarm on the correctly ordered copy in any of
the 160 runs; doubling the smallest 20 / 20 delay gives 2 000 cycles, less than a microsecond.  The delay must also outlast the
host time the library needs to queue a whole call, so that work on a wrong stream starts while the right stream still waits:
the slowest asynchronous call of the cases below took 0.51 ms of host time (update_codebooks_chain, h = 256), most 0.01-0.1 ms.
8.4 ms is 16 times that.  (The entries that check their codes with h < 256 synchronise the stream once, and so return after
the delay: 8.4-8.7 ms; what they queue after that check is not behind the delay any more, which is why every such entry has
an h = 256 case too.)  With four plain pool streams the 41 GPU tests of this file took 6 s of the `-m gpu` run; the streams
fixture and the control test have since added about 230 delayed passes of 8.4 ms and a 4 MB copy each, a few seconds more.

Out of scope: hipGraph / torch.cuda.graph capture of these calls (the header does not promise it; the entries allocate and some
synchronise), more than one physical GPU, rq_dev_polar_factor (no stream parameter; device.polar_factor synchronises the
device around it), and stream = NULL while a side stream is current (the wrappers of device.py cannot express it)."""
import threading

import numpy as np
import pytest

import stream_cases as sc

gpu = pytest.mark.gpu

DELAY_CYCLES = 20_000_000


def _release():
    from rayuela_jl_amd import _lib
    _lib.check(_lib.lib().rq_release_workspaces())


def _control_case(second_stream):
    """A stand-in entry point y = x; `second_stream`: the copy is issued there with no event wait -- the bug the harness is for."""
    import torch
    x = np.arange(1, 1 + (1 << 20), dtype=np.float32)

    def run(dev, out):
        with torch.cuda.stream(second_stream or torch.cuda.current_stream()):
            out["y"].copy_(dev["x"])
        return {"y": out["y"]}

    def check(got):
        assert np.array_equal(got["y"], x)

    return sc.Case("control", {"x": x}, run, check, outputs={"y": (x.shape, np.float32)})


def _caught(case, stream, reps):
    n = 0
    for _ in range(reps):
        try:
            case.check(sc.run_on_side_stream(case, stream, DELAY_CYCLES))
        except AssertionError:
            n += 1
    return n


@pytest.fixture(scope="module")
def streams():
    """Four side streams for the whole module; the scratch slots they took are returned at the end.

    Only streams on which the harness SEES work misplaced on the null stream are taken: a process has a few hardware queues
    (4 by default), the runtime deals its streams over them, and a side stream that shares its queue with the null stream runs
    in submission order with it -- a launch on the null stream then waits behind the delay like a correct one."""
    import torch
    null = torch.cuda.default_stream()
    on_null = _control_case(null)
    ss, blind = [], 0
    while len(ss) < 4 and len(ss) + blind < 16:
        s = torch.cuda.Stream()
        if s.cuda_stream != null.cuda_stream and _caught(on_null, s, 3) == 3:
            ss.append(s)
        else:
            blind += 1
    print("side streams: %d taken, %d passed over (they run in order with the null stream)" % (len(ss), blind))
    assert len(ss) == 4, ("only %d of %d pool streams show a launch misplaced on the null stream: a finding about this process's "
                          "hardware queues (GPU_MAX_HW_QUEUES, 4 by default; fewer leave no queue apart from the null stream's) "
                          "and how the runtime deals streams over them, not about the library" % (len(ss), len(ss) + blind))
    assert len({s.cuda_stream for s in ss} | {null.cuda_stream}) == 5
    yield ss
    torch.cuda.synchronize()
    _release()


def test_every_stream_entry_point_has_a_case():
    from test_cabi import _header_prototypes
    declared = {name for name, (_, params) in _header_prototypes().items() if params and params[-1] == ("void *", "stream")}
    assert len(declared) >= 24
    assert declared == sc.ENTRIES, (sorted(declared - sc.ENTRIES), sorted(sc.ENTRIES - declared))


# ---- A. stream ordering --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_entry_point_is_ordered_on_a_side_stream(rq, streams, name):
    case = sc.get(name)
    stream = streams[sorted(sc.CASES).index(name) % len(streams)]
    # once without delay: grows this stream's scratch.  A regrowth synchronises the device inside the call and would end the
    # delay before the launches it is meant to hold back (test_scratch_regrowth_on_a_live_stream looks at regrowth itself)
    case.check(sc.run_on_side_stream(case, stream, 0))
    log = []
    got = sc.run_on_side_stream(case, stream, DELAY_CYCLES, log)
    print("%s: the call took %.2f ms of host time" % log[0])
    case.check(got)


@gpu
def test_harness_reports_a_copy_on_the_wrong_stream(rq, streams):
    """The power of the harness: a wrong answer on harmless data, 20 times of 20 -- for a copy misplaced on another pool stream
    and, on every stream of the module, for one misplaced on the null stream; the correctly placed copy never raises it."""
    import torch
    assert _caught(_control_case(streams[1]), streams[0], 20) == 20
    on_null, good = _control_case(torch.cuda.default_stream()), _control_case(None)
    for s in streams:
        assert _caught(on_null, s, 20) == 20
        assert _caught(good, s, 20) == 0


# ---- B. threads, scratch keys, the limit ------------------------------------------------------------------------------------------
THREAD_CASES = ["encode_pq_split_filter", "linscan_k100", "linscan_k1000_sample_sort", "quantize_chainq_nsplits4",
                "encode_icm_h64_range_check", "update_codebooks_lsq_h256", "rotate_T", "encode_rvq"]


def _host_items(rq):
    """The host-pointer calls of the mix (they run on the library's own stream pair): (name, callable that raises on a mismatch)."""
    from test_gpu_switches import _enc_setup, _scan_setup
    codes, centers, queries, ref = _scan_setup(*sc.SCAN_SHAPE)
    m = centers.shape[0]
    X, Ccat, enc_ref = _enc_setup(128, 8)

    def linscan_pq():
        d1, i1 = rq.linscan_pq(codes, queries, [centers[i] for i in range(m)], 8 * m, 100)
        assert np.array_equal(i1.astype(np.int64) - 1, ref[100][1]) and sc._eq_bits(d1, ref[100][0])

    def quantize_pq():
        B = rq.quantize_pq(X, [Ccat[i] for i in range(8)])
        assert np.array_equal(B, enc_ref.astype(np.int16) + 1)

    return [("rq.linscan_pq", linscan_pq), ("rq.quantize_pq", quantize_pq)]


@gpu
def test_mixed_families_from_four_host_threads(rq, streams):
    import torch
    items = [(name, (lambda c: lambda: c.check(sc.run_plain(c)))(sc.get(name))) for name in THREAD_CASES] + _host_items(rq)
    errs = []

    def worker(t):
        try:
            with torch.cuda.stream(streams[t]):
                for rnd in range(3):
                    for j in range(len(items)):
                        name, fn = items[(j + 3 * t) % len(items)]
                        try:
                            fn()
                        except AssertionError as e:
                            errs.append((t, rnd, name, str(e)[:200]))
        except Exception as e:   # noqa: BLE001
            errs.append((t, repr(e)))

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs[:5]


def _upload(arrays):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}


@gpu
@pytest.mark.parametrize("name", ["linscan_k100", "quantize_chainq_nsplits4"])
def test_two_streams_one_thread_no_synchronisation_in_between(rq, oracle, streams, name):
    """The same entry point queued on two streams back to back with different inputs: the (device, stream) scratch key seen
    from one thread.  The first stream is still behind its delay when the second call is made."""
    import torch
    import chain_oracle as co
    case = sc.get(name)
    second = dict(case.inputs)
    if name == "linscan_k100":
        second["queries"] = np.random.default_rng(99).standard_normal(case.inputs["queries"].shape).astype(np.float32)
        d0, i0 = oracle.linscan_aqd_query(second["codes"], second["centers"], second["queries"], 100)
        check2 = sc._check_scan(d0, i0)
    else:
        second["X"] = np.random.default_rng(99).standard_normal(case.inputs["X"].shape).astype(np.float32)
        want = co.viterbi(oracle, second["X"], second["C"])

        def check2(got):
            assert np.array_equal(got["codes"], want)

    devs = [_upload(case.inputs), _upload(second)]
    outs = [{k: sc._sentinel(*spec) for k, spec in case.outputs.items()} for _ in range(2)]
    torch.cuda.synchronize()
    res = []
    for i, s in enumerate(streams[:2]):
        with torch.cuda.stream(s):
            if i == 0:
                torch.cuda._sleep(DELAY_CYCLES)
            res.append(case.run(devs[i], outs[i]))
    for s in streams[:2]:
        s.synchronize()
    case.check({k: v.cpu().numpy() for k, v in res[0].items()})
    check2({k: v.cpu().numpy() for k, v in res[1].items()})


@gpu
def test_scratch_regrowth_on_a_live_stream(rq, streams):
    """A small call, then without synchronising one whose scratch is larger (the library synchronises the device, frees and
    reallocates that slot), then the small one again: rq_dev_encode_opq keeps n * d * 4 bytes of rotated rows (1 000 and 6 001
    rows: more than the 25 % a slot is over-allocated by, so the second call regrows for certain).  The scan triple (k = 100,
    1000, 100) queues three calls with different plans through one stream's candidate buffers and work counters back to back;
    whether its scratch regrows is the planner's business and is not claimed here."""
    import torch
    _release()
    s = streams[2]
    for names in ([sc.encode_opq_rows(1_000), sc.get("encode_opq"), sc.encode_opq_rows(1_000)],
                  [sc.get("linscan_k100"), sc.get("linscan_k1000_sample_sort"), sc.get("linscan_k100")]):
        devs = [_upload(c.inputs) for c in names]
        outs = [{k: sc._sentinel(*spec) for k, spec in c.outputs.items()} for c in names]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(DELAY_CYCLES)
            res = [c.run(dev, out) for c, dev, out in zip(names, devs, outs)]
        s.synchronize()
        for c, r in zip(names, res):
            c.check({k: v.cpu().numpy() for k, v in r.items()})
        torch.cuda.synchronize()


@gpu
def test_eight_streams_per_device_and_recovery(rq, streams):
    """include/rayuela_hip.h, "Threading": at most 8 distinct streams per device may use the rq_dev_* calls before
    rq_release_workspaces().  rq_dev_encode_opq keeps its rotated rows in library scratch."""
    import torch
    from rayuela_jl_amd import _lib
    L = _lib.lib()
    case = sc.encode_opq_rows(1_000)
    n, d, m, h = 1_000, 128, 8, 256
    nine = list(streams) + [torch.cuda.Stream() for _ in range(5)]
    assert len({s.cuda_stream for s in nine}) == 9 and torch.cuda.default_stream().cuda_stream not in {s.cuda_stream for s in nine}
    dev = _upload(case.inputs)
    outs = [sc._sentinel((n, m), np.uint8) for _ in nine]
    torch.cuda.synchronize()
    _release()

    def call(i):
        with torch.cuda.stream(nine[i]):
            rc = L.rq_dev_encode_opq(outs[i].data_ptr(), dev["X"].data_ptr(), dev["R"].data_ptr(), dev["C"].data_ptr(),
                                     n, d, m, h, nine[i].cuda_stream)
        nine[i].synchronize()
        return rc, outs[i].cpu().numpy()

    for i in range(8):
        rc, codes = call(i)
        assert rc == 0, (i, L.rq_last_error())
        case.check({"codes": codes})
    rc, codes = call(8)
    msg = L.rq_last_error().decode()
    assert rc == -2, (rc, msg)                                     # RQ_EUNSUPPORTED
    assert "8 distinct streams" in msg and "rq_release_workspaces" in msg, msg
    assert (codes == sc.SENTINEL).all(), "the refused call wrote its output"
    rc, codes = call(0)                                            # a stream that has its slot still works
    assert rc == 0
    case.check({"codes": codes})
    _release()
    rc, codes = call(8)
    assert rc == 0, L.rq_last_error()
    case.check({"codes": codes})
