"""Every swept run-time switch of tests/switch_table.py against the oracle ("none of them changes a
result"), and the kernels' unaligned-pointer fallbacks.

Scan, encode, rotation, RVQ and order results are compared bit for bit (ids, distance bits, codes, float32 bits); training
reductions against float64 at the tolerances of tests/test_gpu_train.py.  Where the library says what ran (rq_last_encode_kernel,
rq_scan_plan, rq_order_plan, the permutation itself) the test also asserts that the switch moved the path: a sweep that silently
takes the default proves nothing.  Every switch is reset on exit (switch_table.switches)."""
import ctypes as C
import functools

import numpy as np
import pytest

from switch_table import SWITCHES, switches, swept

pytestmark = pytest.mark.gpu


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _np(t):
    return t.cpu().numpy()


def _enc_kernel():
    from rayuela_jl_amd import _lib
    return (_lib.lib().rq_last_encode_kernel() or b"").decode()


def _order_plan(n, m):
    from rayuela_jl_amd import _lib
    out = (C.c_int * 14)()
    assert _lib.lib().rq_order_plan(n, m, C.cast(out, C.c_void_p), 14) == 0
    return list(out)


def _cases(workload):
    return [(k, v) for k, v, w in swept() if w == workload]


# ---- scan workloads -------------------------------------------------------------------------------------------------------
# "scan" and "scan_big" run the host-pointer call (rq_linscan_pq) and the device call (rqd.linscan).  Each (key, value) runs on a
# baseline where it flips what the readout of its table entry reports (a call orders its base only from ORDER_MIN_NQ queries,
# from ORDER_MIN_ROWS rows, below ORDER_MAX_K, or always with SCAN_ORDER = 2) -- a switch that leaves the default path proves
# nothing.
_SCAN_BASE = {("SCAN_ORDER", 0): dict(ORDER_MIN_NQ=1), ("ORDER_MIN_ROWS", 1): dict(ORDER_MIN_NQ=1),
              ("ORDER_MAX_K", 1): dict(ORDER_MIN_NQ=1), ("ORDER_MAX_SCRATCH_MB", 1): dict(SCAN_ORDER=2),
              ("ORDER_GREEDY_MIN_NQ", 1): dict(SCAN_ORDER=2)}
_SCAN_ROWS = {"ORDER_MIN_ROWS": 50_000}           # below the default ORDER_MIN_ROWS = 65536


@functools.lru_cache(maxsize=None)
def _scan_setup(n, m, sub, nq, seed, style=0, Ks=(100, 1000)):
    import rayuela_jl_amd.synth as synth
    from oracle import oracle
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = synth.random_codes(n, m, seed=seed)
    if style == 3:        # test_gpu_fuzz.py style 3: integer tables -> mass ties
        centers = rng.integers(0, 3, (m, 256, sub)).astype(np.float32)
        queries = rng.integers(0, 3, (nq, m * sub)).astype(np.float32)
    elif style == 4:      # style 4: 50 distinct rows
        codes = codes[rng.integers(0, 50, n)]
    ref = {K: oracle.linscan_aqd_query(codes, centers, queries, K) for K in Ks}
    return codes, centers, queries, ref


def _dev_scan(codes, centers, queries, K):
    import torch
    from rayuela_jl_amd import device as rqd
    dd, idd = rqd.linscan(torch.from_numpy(codes).cuda(), torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda(), K)
    torch.cuda.synchronize()
    return dd, idd


def _scan_both(rq, codes, centers, queries, K):
    m = centers.shape[0]
    dh, ih = rq.linscan_pq(codes, queries, [centers[i] for i in range(m)], 8 * m, K)      # host pointers, one-based ids
    dd, idd = _dev_scan(codes, centers, queries, K)
    return (dh, ih.astype(np.int64) - 1), (_np(dd), _np(idd).view(np.uint32).astype(np.int64))


def _readout(key, setup, K):
    """What the library reports for the scan of `setup` at K under the current switches (the entry's `readout`)."""
    from rayuela_jl_amd import _lib
    codes, centers, queries, _ = setup
    (n, m), nq, sub = codes.shape, queries.shape[0], centers.shape[2]
    kind = SWITCHES[key]["readout"]
    if kind == "orders":
        return _lib.lib().rq_scan_orders_in_call(n, nq, K)
    if kind == "plan":
        return _lib.scan_plan(n, nq, m, m * sub, K)
    if kind == "kernel":
        _dev_scan(codes, centers, queries, K)
        return (_lib.lib().rq_last_scan_kernel() or b"").decode()
    assert kind.startswith("stats:"), kind
    with switches(SCAN_STATS=1):
        _lib.scan_stats()
        _dev_scan(codes, centers, queries, K)
        return _lib.scan_stats()[kind[6:]]


def _check_scan(rq, setup, Ks, tag, kv):
    codes, centers, queries, ref = setup
    for K in Ks:
        d0, i0 = ref[K]
        with switches(**kv):
            for how, (d1, i1) in zip(("host", "device"), _scan_both(rq, codes, centers, queries, K)):
                assert np.array_equal(i1, i0) and _eq_bits(d1, d0), (tag, how, K)


def _check_moved(key, value, setup, K, base):
    """The switch moved the path: its readout differs from the baseline's (entries without a readout say why in the table)."""
    if "readout" not in SWITCHES[key]:
        return None
    with switches(**base):
        before = _readout(key, setup, K)
    with switches(**base, **{key: value}):
        after = _readout(key, setup, K)
    assert before != after, (key, value, K, before)
    return before, after


@pytest.mark.parametrize("key,value", _cases("scan"))
def test_scan_switch(rq, key, value):
    base = _SCAN_BASE.get((key, value), {})
    setup = _scan_setup(_SCAN_ROWS.get(key, 200_000), 8, 4, 12, 41)
    _check_moved(key, value, setup, 100, base)
    _check_scan(rq, setup, (100, 1000), (key, value), {**base, key: value})


@pytest.mark.parametrize("key,value", _cases("scan_big"))
def test_scan_switch_on_a_base_the_balance_orders(rq, key, value):
    """1e6 rows of 8 bytes with SCAN_ORDER = 2: rq_dev_linscan balances its in-call order (ORDER_GREEDY_MIN_NQ = 1: 1 -> 2), or
    skips its scratch copy above ORDER_MAX_SCRATCH_MB (1 -> 0).  The host-pointer call orders into an allocation of its own and
    does not read ORDER_MAX_SCRATCH_MB; both calls must give the oracle's answer."""
    base = _SCAN_BASE[(key, value)]
    setup = _scan_setup(1_000_000, 8, 2, 8, 43, Ks=(100,))
    before, after = _check_moved(key, value, setup, 100, base)
    assert (before, after) == ((1, 0) if key == "ORDER_MAX_SCRATCH_MB" else (1, 2)), (key, before, after)
    _check_scan(rq, setup, (100,), (key, value), {**base, key: value})


@pytest.mark.parametrize("style", [3, 4])
@pytest.mark.parametrize("key,value", _cases("scan_hostile"))
def test_scan_finish_switch_on_hostile_tables(rq, key, value, style):
    """The finish paths around K = 100 / 1000 / 2000 with mass ties: SCAN_SS_MIN_K moves the LDS / sample-sort crossover both
    ways (the planner's bigk flag says which ran); SCAN_BUCKET_FINISH = 0 leaves the bucket finish (its counter reads 0)."""
    from rayuela_jl_amd import _lib
    n, m, sub, nq = 200_000, 8, 2, 11
    setup = _scan_setup(n, m, sub, nq, 70 + style, style, Ks=(100, 1000, 2000))
    if key == "SCAN_SS_MIN_K":
        with switches(**{key: value}):
            for K in (100, 1000, 2000):
                assert _lib.scan_plan(n, nq, m, m * sub, K)["bigk"] == int(K > value), (value, K)
        moved = [K for K in (100, 1000, 2000) if (K > value) != (K > SWITCHES[key]["default"])]
        assert moved, value                                   # every swept value moves at least one K across the crossover
        for K in moved:
            _check_moved(key, value, setup, K, {})
    elif key == "SCAN_BUCKET_FINISH" and value == 0:
        before, after = _check_moved(key, value, setup, 100, {})
        assert before > 0 and after == 0, (before, after)
    _check_scan(rq, setup, (100, 1000, 2000), (key, value, style), {key: value})


@pytest.mark.parametrize("key,value", _cases("scan_xcd"))
def test_scan_switch_on_the_xcd_window_plan(rq, key, value):
    """The small-base XCD plan (SCAN_XCD_MIN_MB = 1, SCAN_WINDOW_MB = 1; 3e5 rows of 64 bytes = 19 windows) with the window
    hand-out switched off, tail slices instead (both: the plan leaves the XCD windows), or pacing rounds of 1 / 3 items (the
    plan stays the XCD plan; the round has no readout)."""
    from rayuela_jl_amd import _lib
    n, m, sub, nq = 300_000, 64, 1, 12
    base = dict(SCAN_XCD_MIN_MB=1, SCAN_WINDOW_MB=1)
    with switches(**base):
        assert _lib.scan_plan(n, nq, m, m * sub, 100)["xcd"] == 1
    with switches(**base, **{key: value}):
        xcd = _lib.scan_plan(n, nq, m, m * sub, 100)["xcd"]
    assert xcd == int(key == "SCAN_XCD_ROUND"), (key, value, xcd)
    _check_scan(rq, _scan_setup(n, m, sub, nq, 47), (100, 1000), (key, value), {**base, key: value})


# ---- host-pointer results path -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_setup():
    import rayuela_jl_amd.synth as synth
    from oracle import oracle
    rng = np.random.default_rng(51)
    n, m, sub, nq = 20_000, 8, 4, 600
    C_ = [rng.standard_normal((256, sub)).astype(np.float32) for _ in range(m)]
    Q = rng.standard_normal((nq, m * sub)).astype(np.float32)
    R = synth.rotation(m * sub, seed=2)
    B = synth.random_codes(n, m, seed=52)
    sel = np.arange(0, nq, 50)
    ref = oracle.linscan_aqd_query(B, np.stack(C_), Q[sel], 100)
    ref_o = oracle.linscan_aqd_query(B, np.stack(C_), oracle.rotate_T(R, Q[sel]), 100)
    return B, C_, Q, R, sel, ref, ref_o


@pytest.mark.parametrize("key,value", _cases("host"))
def test_host_path_switch(rq, key, value):
    """600 queries: HOST_CHUNK cuts them into 256-query chunks, HOST_DIRECT = 0 copies results through device arrays;
    linscan_pq / linscan_opq host -> host equal the default call and the oracle bit for bit."""
    B, C_, Q, R, sel, (d0, i0), (do, io) = _host_setup()
    b = 8 * len(C_)
    dp, ip = rq.linscan_pq(B, Q, C_, b, 100)
    dpo, ipo = rq.linscan_opq(B, Q, C_, b, R, 100)
    with switches(**{key: value}):
        d1, i1 = rq.linscan_pq(B, Q, C_, b, 100)
        d2, i2 = rq.linscan_opq(B, Q, C_, b, R, 100)
    assert np.array_equal(i1, ip) and _eq_bits(d1, dp), key
    assert np.array_equal(i2, ipo) and _eq_bits(d2, dpo), key
    assert np.array_equal(i1[sel].astype(np.int64) - 1, i0) and _eq_bits(d1[sel], d0)
    assert np.array_equal(i2[sel].astype(np.int64) - 1, io) and _eq_bits(d2[sel], do)


# ---- encode / rotation ---------------------------------------------------------------------------------------------------
_ENC_SHAPES = [  # (d, m): the kernel each takes by default
    (128, 8),    # sub 16: split filter + exact pass
    (96, 16),    # sub 6: split
    (128, 4),    # sub 32: direct (X in registers)
    (96, 1),     # a full-width RVQ stage, sub 96: direct wide
    (96, 32),    # sub 3: LDS-staged
]
_ENC_DEFAULT = {(128, 8): "encode_pq_filter_kernel", (96, 16): "encode_pq_filter_kernel", (128, 4): "encode_pq_direct_kernel",
                (96, 1): "encode_pq_direct_kernel", (96, 32): "encode_pq_kernel"}
# what runs instead with the switch set (None: the same kernel, other launch parameters)
_ENC_MOVED = {("ENC_SPLIT", 0): {(128, 8): "encode_pq_direct_kernel", (96, 16): "encode_pq_direct_kernel"},
              ("ENC_SPLIT", 2): {(128, 8): "encode_pq_split_kernel", (96, 16): "encode_pq_split_kernel"},
              ("ENC_DIRECT", 0): {(128, 4): "encode_pq_kernel", (96, 1): "encode_wide_kernel"}}


@functools.lru_cache(maxsize=None)
def _enc_setup(d, m):
    from oracle import oracle
    rng = np.random.default_rng(d * 100 + m)
    X = (rng.standard_normal((6_001, d)) * 10).astype(np.float32)
    Ccat = (rng.standard_normal((m, 256, d // m)) * 10).astype(np.float32)
    return X, Ccat, oracle.encode_pq(X, Ccat, m, 256)


@pytest.mark.parametrize("key,value", _cases("encode"))
def test_encode_switch(rq, key, value):
    import torch
    from rayuela_jl_amd import device as rqd
    for d, m in _ENC_SHAPES:
        X, Ccat, ref = _enc_setup(d, m)
        Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(Ccat).cuda()
        with switches(**{key: value}):
            got = _np(rqd.encode_pq(Xd, Cd, m, 256))
            ran = _enc_kernel()
        assert np.array_equal(got, ref), (key, value, d, m)
        assert ran == _ENC_MOVED.get((key, value), {}).get((d, m), _ENC_DEFAULT[(d, m)]), (key, value, d, m, ran)


_ROT_WIDTHS = {"ROT_V2": (32, 64, 96, 128), "ROT_WIDE2": (200, 784)}


@pytest.mark.parametrize("key,value,d", [(k, v, d) for k, v in _cases("rotate") for d in _ROT_WIDTHS[k]])
def test_rotate_switch(rq, oracle, key, value, d):
    """ROT_V2 = 0: the generic LDS-staged rotate_kernel at d in {32, 64, 96, 128}; ROT_WIDE2 = 0: rotate_wide_kernel at
    d % 4 == 0 above the LDS-resident widths (200, 784) -- only the widths where the switch selects another kernel (the
    library has no rotation readout).  RX = R'X bit for bit with the oracle."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(d)
    X = rng.standard_normal((1_000, d)).astype(np.float32)
    R = synth.rotation(d, seed=d)
    ref = oracle.rotate_T(R, X)
    with switches(**{key: value}):
        got = _np(rqd.rotate_T(torch.from_numpy(R).cuda(), torch.from_numpy(X).cuda()))
    assert _eq_bits(got, ref), (key, value, d)


# ---- row order -------------------------------------------------------------------------------------------------------------
ORDER_SWEEP = [(300_000, 8), (785_000, 8), (790_000, 8), (1_000_000, 8), (4_000_000, 8),
               (300_000, 16), (1_000_000, 16), (4_000_000, 16)]


@pytest.mark.parametrize("n,m", ORDER_SWEEP)
def test_greedy_balance_runs_exactly_where_the_plan_says(rq, n, m):
    """ORDER_GREEDY = 1 against 0 changes the ordered base exactly when rq_order_plan reports the balance (p[12] != 0): the host
    plan and the device launch decide alike.  (Rows of one sort bucket land in atomic order, so the permutations of two runs
    differ anyway; what tells the balance is its effect -- the LDS-pass model of test_gpu_order.py drops by >= 5 %, while two
    plain sorts of one base agree to 1 %.)"""
    import torch
    from rayuela_jl_amd import device as rqd
    from test_gpu_order import _lds_passes
    codes = rqd.synth_codes(n, m, seed=n + m)
    on = _order_plan(n, m)[12] != 0
    passes = {}
    for g in (0, 1):
        with switches(ORDER_GREEDY=g):
            ob = rqd.order_rows(codes)
        perm = ob.perm.view(torch.int32).long()
        assert torch.equal(torch.sort(perm).values, torch.arange(n, device=perm.device)), (n, m, g)
        passes[g] = _lds_passes(_np(ob.codes[:, :m]), 2 if m == 8 else 1)
        del ob, perm
    ratio = passes[1] / passes[0]
    assert (ratio < 0.95) if on else (0.99 < ratio < 1.01), (n, m, on, passes)


@functools.lru_cache(maxsize=None)
def _order_setup(n, m, sub, nq, K):
    """The base (rqd.synth_codes(n, m, seed=9), deterministic), its tables and queries, and the oracle's answer: computed once."""
    from oracle import oracle
    from rayuela_jl_amd import device as rqd
    codes_h = _np(rqd.synth_codes(n, m, seed=9))
    rng = np.random.default_rng(12)
    centers = rng.standard_normal((m, 256, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    return codes_h, centers, queries, oracle.linscan_aqd_query(codes_h, centers, queries, K)


@pytest.mark.parametrize("key,value", _cases("order"))
def test_order_switch(rq, key, value):
    """Each order switch on a 1e6-row base of 8 bytes: still a permutation, rows moved with it, a scan over it equals the
    oracle -- and every switch with a readout (the ones that shape the key) changed rq_order_plan."""
    import torch
    from rayuela_jl_amd import device as rqd
    n, m, sub, nq, K = 1_000_000, 8, 2, 8, 100
    codes_h, centers, queries, (d0, i0) = _order_setup(n, m, sub, nq, K)
    codes = torch.from_numpy(codes_h).cuda()
    with switches(**{key: value}):
        plan = _order_plan(n, m)
        ob = rqd.order_rows(codes)
    perm = ob.perm.view(torch.int32).long()
    assert torch.equal(torch.sort(perm).values, torch.arange(n, device=perm.device)), (key, value)
    assert torch.equal(ob.codes[:, :m], codes[perm]), (key, value)
    if SWITCHES[key].get("readout") == "order_plan":
        assert plan != _order_plan(n, m), (key, value)
    d1, i1 = rqd.linscan(ob, torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda(), K)
    assert np.array_equal(_np(i1).view(np.uint32), i0) and _eq_bits(_np(d1), d0), (key, value)


# ---- training --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,value", _cases("train"))
def test_gram_switch(rq, key, value):
    import torch
    from rayuela_jl_amd import device as rqd
    from oracle import train_oracle as to
    n, d, m, h = 9_000, 128, 8, 256
    rng = np.random.default_rng(5)
    X = (rng.standard_normal((n, d)) * 20 + 3).astype(np.float32)
    codes = rng.integers(0, h, (n, m), dtype=np.uint8)
    off = to.offsets(d, m)
    Cs = [rng.standard_normal((h, off[q + 1] - off[q])).astype(np.float32) * 20 for q in range(m)]
    Ccat = np.concatenate([c.reshape(-1) for c in Cs])
    CB = to.reconstruct(Cs, codes, off, d)
    G0 = X.astype(np.float64).T @ CB.astype(np.float64)
    with switches(**{key: value}):
        G = _np(rqd.gram_codes(torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(Ccat).cuda(), h))
    assert np.allclose(G, G0, rtol=1e-5, atol=1e-5 * np.abs(G0).max()), (key, value)


@pytest.mark.parametrize("key,value", _cases("polar"))
def test_polar_switch(rq, key, value):
    """TRAIN_NS_BIG_D moves d = 96 onto the 64 x 64-tile Newton-Schulz kernel; TRAIN_NS_L0_MICRO changes its first scaling.
    R against LAPACK's U V' in float64 (test_gpu_train.py: 2e-6 for a well-conditioned G)."""
    import torch
    from rayuela_jl_amd import device as rqd
    d = 96
    rng = np.random.default_rng(96)
    G = rng.standard_normal((d, d)).astype(np.float32)
    U, s, Vt = np.linalg.svd(G.astype(np.float64))
    P = U @ Vt
    with switches(**{key: value}):
        R, ok, steps = rqd.polar_factor(torch.from_numpy(G).cuda(), 0)
    R = _np(R).astype(np.float64)
    assert ok, (key, value, steps)
    assert np.abs(R @ R.T - np.eye(d)).max() < 5e-7 * d ** 0.5, (key, value)
    assert np.abs(R - P).max() < max(2e-6, 4e-7 * s[0] / s[-1] * 0.01), (key, value, np.abs(R - P).max())


@pytest.mark.parametrize("key,value", _cases("train_opq"))
def test_train_opq_switch(rq, oracle, key, value):
    """TRAIN_FUSED_CB = 0 (the materialised reconstruction) and TRAIN_DETERMINISTIC = 0 (overlap kept; its factorisation may
    differ bitwise): rq_train_opq's objective curve against the default run and the oracle loop at test_gpu_train.py's
    tolerances."""
    import rayuela_jl_amd.synth as synth
    from oracle import train_oracle as to
    rng = np.random.default_rng(3)
    X = (rng.standard_normal((12_000, 32)) * 10).astype(np.float32)
    R0 = synth.rotation(32, seed=5)
    C0 = synth.codebooks(oracle.rotate_T(R0, X), 4, 32, seed=9, iters=0, sample=2000)
    niter = 3
    _, B, R, obj = rq.train_opq(X, 4, 32, niter, "natural", R0=R0, C0=C0)
    with switches(**{key: value}):
        _, B2, R2, obj2 = rq.train_opq(X, 4, 32, niter, "natural", R0=R0, C0=C0)
    _, _, _, obj_o = to.train_opq(X, 4, 32, niter, R0, C0)
    assert np.allclose(obj2, obj, rtol=1e-4) and np.abs(R2 - R).max() < 2e-2, (key, value)
    assert np.allclose(obj2, obj_o, rtol=3e-4), (key, value)
    assert np.abs(R2 @ R2.T - np.eye(32)).max() < 1e-5


def test_every_swept_switch_has_a_test_here():
    workloads = {"scan", "scan_big", "scan_hostile", "scan_xcd", "host", "encode", "rotate", "order", "train", "polar",
                 "train_opq"}
    assert {w for _, _, w in swept()} <= workloads
    assert all(set(e) <= {"default", "values", "workload", "readout", "tested_in", "reason", "note"} for e in SWITCHES.values())


# ---- unaligned device inputs -----------------------------------------------------------------------------------------------
def _at(t, off_bytes):
    """A contiguous copy of t that starts `off_bytes` past a 256-byte aligned allocation (the view of a flat buffer)."""
    import torch
    es = t.element_size()
    assert off_bytes % es == 0
    buf = torch.full((t.numel() + 64 // es + off_bytes // es,), 0, dtype=t.dtype, device=t.device)
    v = buf[off_bytes // es: off_bytes // es + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 256 == off_bytes % 256
    return v


OFFSETS = [4, 8, 12]


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("d,m", [(128, 8), (96, 16), (32, 16), (64, 32), (200, 25), (784, 28)])
def test_encode_pq_and_opq_at_unaligned_offsets(rq, oracle, off, d, m):
    """X, Ccat, R at 4- / 8- / 12-byte offsets: sub in {2, 6, 16} would take the aligned fast paths (split filter with vec4
    loads, direct); the fallback must give the oracle's codes, and an X that is not 8-byte aligned must leave the split /
    direct kernels."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(d + m)
    X = (rng.standard_normal((3_001, d)) * 10).astype(np.float32)
    Ccat = (rng.standard_normal((m, 256, d // m)) * 10).astype(np.float32)
    R = synth.rotation(d, seed=7)
    ref = oracle.encode_pq(X, Ccat, m, 256)
    Xd, Cd, Rd = torch.from_numpy(X).cuda(), torch.from_numpy(Ccat).cuda(), torch.from_numpy(R).cuda()
    aligned = _np(rqd.encode_pq(Xd, Cd, m, 256))
    got = _np(rqd.encode_pq(_at(Xd, off), _at(Cd, off), m, 256))
    ran = _enc_kernel()
    assert np.array_equal(aligned, ref) and np.array_equal(got, ref), (d, m, off)
    if off % 8:
        assert ran in ("encode_pq_kernel", "encode_wide_kernel"), (d, m, off, ran)
    # OPQ: X, R and C all shifted
    ref_o = oracle.encode_opq(X, R, Ccat, m, 256)
    got_o = _np(rqd.encode_opq(_at(Xd, off), _at(Rd, off), _at(Cd, off), m, 256))
    assert np.array_equal(got_o, ref_o), (d, m, off)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("d", [32, 96, 128, 200, 784])
def test_rotate_at_unaligned_offsets(rq, oracle, off, d):
    """X, R and the output RX at offsets, one at a time and all together: RX = R'X bit for bit."""
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(d)
    X = torch.from_numpy(rng.standard_normal((1_001, d)).astype(np.float32)).cuda()
    R = torch.from_numpy(synth.rotation(d, seed=d)).cuda()
    ref = oracle.rotate_T(_np(R), _np(X))
    for sx, sr, so in ((off, 0, 0), (0, off, 0), (0, 0, off), (off, off, off)):
        out = _at(torch.empty_like(X), so) if so else None
        got = rqd.rotate_T(_at(R, sr) if sr else R, _at(X, sx) if sx else X, out=out)
        assert _eq_bits(_np(got), ref), (d, off, sx, sr, so)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("d", [96, 100])
def test_rvq_at_unaligned_offsets(rq, oracle, off, d):
    """Full-width RVQ stages with Xr and the codebook off 16-byte alignment: the scalar residual kernel on a d % 4 == 0 input
    (and d = 100, whose stage encode is the wide kernel); codes, counts and the final residual bit for bit."""
    import torch
    from rayuela_jl_amd import device as rqd
    rng = np.random.default_rng(d + off)
    n, m, h = 4_001, 3, 256
    X = (rng.standard_normal((n, d)) * 10).astype(np.float32)
    Cs = (rng.standard_normal((m, h, d)) * 5).astype(np.float32)
    codes0, counts0, Xr0 = oracle.encode_rvq(X, Cs, with_extras=True)
    Xr = _at(torch.from_numpy(X).cuda(), off)
    codes, counts = rqd.encode_rvq(Xr, _at(torch.from_numpy(Cs).cuda(), off), want_counts=True)
    assert np.array_equal(_np(codes), codes0), (d, off)
    assert np.array_equal(_np(counts).astype(np.uint32), counts0), (d, off)
    assert _eq_bits(_np(Xr), Xr0), (d, off)


@pytest.mark.parametrize("off", OFFSETS)
def test_training_reductions_at_unaligned_offsets(rq, off):
    """reconstruct (output at an offset), gram, gram_codes, qerror, qerror_codes and update_centers with X, CB and C off
    16-byte alignment: equal to the aligned call and to float64 at test_gpu_train.py's tolerances."""
    import torch
    from rayuela_jl_amd import device as rqd
    from oracle import train_oracle as to
    n, d, m, h = 7_001, 96, 16, 256
    rng = np.random.default_rng(off)
    X = (rng.standard_normal((n, d)) * 20 + 3).astype(np.float32)
    codes = rng.integers(0, h, (n, m), dtype=np.uint8)
    off_ = to.offsets(d, m)
    Cs = [rng.standard_normal((h, off_[q + 1] - off_[q])).astype(np.float32) * 20 for q in range(m)]
    Ccat = np.concatenate([c.reshape(-1) for c in Cs])
    CB0 = to.reconstruct(Cs, codes, off_, d)
    G0 = X.astype(np.float64).T @ CB0.astype(np.float64)
    e0 = ((X.astype(np.float64) - CB0) ** 2).sum() / n
    Xd, cd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(codes).cuda(), torch.from_numpy(Ccat).cuda()
    Xu, Cu = _at(Xd, off), _at(Cd, off)
    CBu = rqd.reconstruct(cd, Cu, d, h, out=_at(torch.empty((n, d), dtype=torch.float32, device="cuda"), off))
    assert np.array_equal(_np(CBu), CB0)
    tol = dict(rtol=1e-5, atol=1e-5 * np.abs(G0).max())
    assert np.allclose(_np(rqd.gram(Xu, CBu)), G0, **tol)
    assert np.allclose(_np(rqd.gram_codes(Xu, cd, Cu, h)), G0, **tol)
    assert np.allclose(_np(rqd.gram_codes(Xd, cd, Cd, h)), _np(rqd.gram_codes(Xu, cd, Cu, h)), **tol)
    assert abs(rqd.qerror(Xu, CBu) - e0) <= 1e-9 * e0
    assert abs(rqd.qerror_codes(Xu, cd, Cu, h) - e0) <= 1e-9 * e0
    Ca, Cb = Cd.clone(), _at(Cd, off)
    ca = rqd.update_centers(Ca, Xd, cd, m, h)
    cb = rqd.update_centers(Cb, Xu, cd, m, h)
    assert torch.equal(ca, cb)
    Cn = to.update_centers(Cs, X, codes, off_, h)
    assert np.allclose(_np(Cb), np.concatenate([c.reshape(-1) for c in Cn]), rtol=1e-5, atol=1e-4)
    assert np.allclose(_np(Cb), _np(Ca), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("off", OFFSETS)
def test_lut_and_scan_with_unaligned_tables_and_queries(rq, oracle, off):
    """adc_lut and linscan with centers and queries off 16-byte alignment: bit for bit with the oracle."""
    import torch
    from rayuela_jl_amd import device as rqd
    codes, centers, queries, ref = _scan_setup(200_000, 8, 4, 12, 41)
    cen, qs = _at(torch.from_numpy(centers).cuda(), off), _at(torch.from_numpy(queries).cuda(), off)
    lut = _np(rqd.adc_lut(cen, qs))
    for q in range(queries.shape[0]):
        assert _eq_bits(lut[q], oracle.adc_lut(centers, queries[q])), (off, q)
    d1, i1 = rqd.linscan(torch.from_numpy(codes).cuda(), cen, qs, 100)
    assert np.array_equal(_np(i1).view(np.uint32), ref[100][1]) and _eq_bits(_np(d1), ref[100][0]), off


def test_scan_codes_alignment(rq):
    """Codes at a 16-byte offset (codes[2:] at m = 8) scan correctly; at any other offset the scan refuses them with
    RayuelaHipError and leaves the output untouched."""
    import torch
    from oracle import oracle
    from rayuela_jl_amd import device as rqd
    codes, centers, queries, _ = _scan_setup(200_000, 8, 4, 12, 41)
    cd = torch.from_numpy(codes).cuda()
    cen, qs = torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    sub = cd[2:]
    assert sub.data_ptr() % 16 == 0
    d0, i0 = oracle.linscan_aqd_query(codes[2:], centers, queries, 100)
    d1, i1 = rqd.linscan(sub, cen, qs, 100)
    assert np.array_equal(_np(i1).view(np.uint32), i0) and _eq_bits(_np(d1), d0)
    flat = cd.reshape(-1)
    for off in (1, 4, 8, 12):
        bad = flat[off: off + 8 * 1000].view(1000, 8)
        dists = torch.full((12, 10), 7.0, device="cuda")
        ids = torch.full((12, 10), 7, dtype=torch.int32, device="cuda")
        with pytest.raises(rq.RayuelaHipError):
            rqd.linscan(bad, cen, qs, 10, out=(dists, ids))
        torch.cuda.synchronize()
        assert bool((dists == 7.0).all()) and bool((ids == 7).all()), off


def test_merge_topk_with_keys_at_an_8_byte_offset(rq):
    import torch
    from rayuela_jl_amd import device as rqd
    codes, centers, queries, _ = _scan_setup(200_000, 8, 4, 12, 41)
    cen, qs = torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    K, bounds = 100, [0, 70_000, 150_000, 200_000]
    keys = torch.stack([rqd.linscan(torch.from_numpy(codes[a:b]).cuda(), cen, qs, K, id_offset=a, want_keys=True)
                        for a, b in zip(bounds[:-1], bounds[1:])], dim=1).contiguous()
    d0, i0 = rqd.merge_topk(keys, K)
    d1, i1 = rqd.merge_topk(_at(keys, 8), K)
    assert torch.equal(i0, i1) and _eq_bits(_np(d0), _np(d1))
    dr, ir = rqd.linscan(torch.from_numpy(codes).cuda(), cen, qs, K)
    assert torch.equal(i1, ir) and _eq_bits(_np(d1), _np(dr))
