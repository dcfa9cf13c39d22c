"""Every query of the scans the project ships, certified complete at full size (tests/exact_topk.py).

The CPU oracle is too slow for these shapes, so the other full-size tests compare with it on sampled queries only.  Here
each answer is proved to be the reference's top-k by the rank certificate: one O(n) pass of plain torch per query batch,
independent of the library.

  * BASELINE config 5 on one GPU (the `scale_anchor_1gpu` line of `bench.py --full`): 1e9 synthetic rows, m = 8, 1024
    queries, k = 100 -- (a) the rows as they arrive, (b) the base put in bank-aware row order (the 24-bit order key),
    (c) the multi-device index as 8 logical shards of 1.25e8 rows; all three equal bit for bit, (a) certified.
  * The bench's scan calls at 1e6 encoded rows, every query certified: the in-call ordering (1e4 queries, k = 1000), its
    greedy balance (16384 queries), k = 10000, m = 16 (Deep shape), m = 4 (the integer pre-filter) and the host-pointer
    call with one-based ids.  Each case asserts the path it claims through the library's own reports, so that a later
    change of thresholds cannot move it off that path unnoticed.
"""
import time

import numpy as np
import pytest

import exact_topk as xt

pytestmark = pytest.mark.gpu


def _eq_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _report(name, **kv):
    print("EXACT_SCALE %s %s" % (name, " ".join("%s=%s" % kv_ for kv_ in kv.items())), flush=True)


_CACHE = {}


def _workload(wl, m):
    """bench.py's generators: (centers [m][256][sub], codebooks as a list, rotated queries [16384][d], codes of 1e6 rows
    encoded on the device).  wl 'opq': SIFT1M shape (d = 128), 'deep': Deep1M shape (d = 96)."""
    key = (wl, m)
    if key in _CACHE:
        return _CACHE[key]
    import torch
    import rayuela_jl_amd.synth as synth
    import rayuela_jl_amd.synth_torch as st
    from rayuela_jl_amd import device as rqd
    dev = torch.device("cuda", 0)
    n, nq, h = 1_000_000, 16384, 256
    d = 96 if wl == "deep" else 128

    def gen(rows, row0):
        if wl == "deep":
            return st.deep_like(rows, d, seed=synth.SEED_BASE, row0=row0, device=dev)
        return st.sift_like(rows, d, seed=synth.SEED_BASE, ncentres=65536, row0=row0, device=dev)
    Q = gen(nq, 3_000_000_000)
    S = gen(20_000, 3_100_000_000)
    R = torch.from_numpy(synth.rotation(d)).to(dev)
    C = synth.codebooks(rqd.rotate_T(R, S).cpu().numpy(), m, h, seed=synth.SEED_CODEBOOK, iters=3, sample=20000)
    Ccat = torch.from_numpy(synth.cat_codebooks(C)).to(dev)
    centers = torch.from_numpy(np.stack(C)).to(dev)
    X = torch.cat([gen(250_000, o) for o in range(0, n, 250_000)], 0)
    codes = rqd.encode_opq(X, R, Ccat, m, h)
    del X
    Qs = rqd.rotate_T(R, Q)
    _CACHE.clear()                              # one workload's tensors at a time
    _CACHE[key] = (centers, C, Qs, codes)
    return _CACHE[key]


def _spread(nq, count, qg=8):
    """`count` queries over the batch: evenly spaced, with the first and the last query group, both ends of each."""
    sel = np.arange(0, nq, max(1, nq // count))
    return np.unique(np.concatenate([sel, np.arange(qg), np.arange(nq - qg, nq)]))


CERT_1E9 = 1024     # certified queries of the 1e9-row scan: all of them (268 took 12.9 s on an MI355X; keep >= 128)


def test_billion_rows_on_one_gpu_config5(rq):
    """1e9 rows x 8 bytes (8 GB of synthetic codes), 1024 queries, k = 100: (a) arrival order, (b) rqd.order_rows (24-bit
    key, byte offsets row * m beyond 2^32), (c) the index as 8 logical shards -- equal bit for bit, (a) certified."""
    import ctypes as C
    import torch
    import rayuela_jl_amd.synth as synth
    from rayuela_jl_amd import device as rqd
    from rayuela_jl_amd import _lib
    torch.cuda.empty_cache()                # free memory as the device sees it, not what torch keeps cached
    free0 = torch.cuda.mem_get_info(0)[0]
    if free0 < 40 << 30:                    # 30 GiB measured at the peak: the base, its ordered copy and the scratch
        pytest.skip("needs 40 GB of free device memory")
    n, m, nq, k = 1_000_000_000, 8, 1024, 100
    L = _lib.lib()
    centers, Cl, Qs, _ = _workload("opq", 8)
    Q = Qs[:nq].contiguous()
    free_min = [free0]

    def mark():
        torch.cuda.synchronize()
        free_min[0] = min(free_min[0], torch.cuda.mem_get_info(0)[0])

    # (a) the rows as they arrive: no in-call ordering at this shape
    assert L.rq_scan_orders_in_call(n, nq, k) == 0
    codes = rqd.synth_codes(n, m, synth.SEED_BASE)
    assert np.array_equal(codes[n - 1000:].cpu().numpy(), synth.random_codes(1000, m, synth.SEED_BASE, row0=n - 1000))
    da, ia = rqd.linscan(codes, centers, Q, k)
    mark()
    sel = torch.from_numpy(_spread(nq, CERT_1E9)).cuda()
    assert {0, nq - 8, nq - 1} <= set(sel.tolist())
    t0 = time.perf_counter()
    lut = xt.adc_lut(centers, Q[sel])
    got = xt.certify(da[sel], ia[sel], k, lut, codes, n)
    mark()
    t_cert = time.perf_counter() - t0
    del lut
    torch.cuda.empty_cache()
    # (b) the base in bank-aware row order: the 24-bit key (2^24 histogram bins)
    out = (C.c_int * 14)()
    assert L.rq_order_plan(n, m, C.cast(out, C.c_void_p), 14) == 0
    assert out[8] == 24, list(out)
    ob = rqd.order_rows(codes)
    mark()
    del codes
    torch.cuda.empty_cache()
    assert ob.perm is not None
    db, ib = rqd.linscan(ob, centers, Q, k)
    mark()
    del ob
    torch.cuda.empty_cache()
    assert torch.equal(ib, ia), "ordered base: ids differ from the arrival-order scan"
    assert torch.equal(db.view(torch.int32), da.view(torch.int32)), "ordered base: distances differ"
    # (c) config 5's 8-way split, on one device
    with rq.Index(Cl, Q.shape[1], devices=[0] * 8) as ix:
        ix.set_codes_synth(n, synth.SEED_BASE)
        assert ix.info()["rows_per_shard"] == [n // 8] * 8
        dc, ic = ix.search(Q.cpu().numpy(), k, id_base=0)
        mark()
    assert np.array_equal(ic, ia.cpu().numpy().view(np.uint32)), "8 logical shards: ids differ"
    assert _eq_bits(dc, da.cpu().numpy()), "8 logical shards: distances differ"
    _report("config5_1e9", certified=got, certify_s=round(t_cert, 1),
            peak_device_gib=round((free0 - free_min[0]) / (1 << 30), 1))


def _plan_ok(n, nq, m, d, k, bigk):
    from rayuela_jl_amd import _lib
    p = _lib.scan_plan(n, nq, m, d, k)
    assert p["whole"] == p["groups"] and p["slices"] == 1 and p["bigk"] == bigk, p


# (workload, m, nq, k, expected rq_scan_orders_in_call, expected kernel prefix)
BENCH_CALLS = [
    ("opq", 8, 10000, 1000, 1, "adc_scan_kernel<8, false, true, false>"),     # the bench call: ordered inside the call
    ("opq", 8, 16384, 1000, 2, "adc_scan_kernel<8, false, true, false>"),     # ... and balanced by the greedy pass
    ("opq", 8, 10000, 10000, 0, "adc_scan_kernel<8, false, true, true>"),     # k = 10000: arrival order, fine tables
    ("deep", 16, 10000, 1000, 1, "adc_scan_kernel<16, false, true, false>"),  # Deep shape, 1024-thread kernel
    ("opq", 4, 10000, 1000, 1, "adc_scan_kernel<4, false, true, false>"),     # m = 4: the integer pre-filter
]


@pytest.mark.parametrize("case", BENCH_CALLS, ids=["%s_m%d_nq%d_k%d" % c[:4] for c in BENCH_CALLS])
def test_bench_scan_calls_every_query_certified(rq, case):
    import torch
    from rayuela_jl_amd import device as rqd
    from rayuela_jl_amd import _lib
    wl, m, nq, k, orders, kernel = case
    centers, _, Qs, codes = _workload(wl, m)
    n, d = codes.shape[0], Qs.shape[1]
    Q = Qs[:nq].contiguous()
    L = _lib.lib()
    assert L.rq_scan_orders_in_call(n, nq, k) == orders
    _plan_ok(n, nq, m, d, k, int(k > 1024))
    dists, ids = rqd.linscan(codes, centers, Q, k)
    assert (L.rq_last_scan_kernel() or b"").decode() == kernel
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = xt.certify(dists, ids, k, xt.adc_lut(centers, Q), codes, n)
    _report("bench_call_%s_m%d_nq%d_k%d" % (wl, m, nq, k), certified=got, certify_s=round(time.perf_counter() - t0, 1))
    assert got == nq


def test_host_pointer_call_every_query_certified(rq):
    """rq_linscan_pq (numpy in, what a Julia `ccall` passes): one-based codes and ids, 1e4 queries, k = 1000, ordered
    inside the call."""
    import torch
    from rayuela_jl_amd import _lib
    centers, Cl, Qs, codes = _workload("opq", 8)
    n, m = codes.shape
    nq, k = 10000, 1000
    assert _lib.lib().rq_scan_orders_in_call(n, nq, k) == 1
    Qn = Qs[:nq].cpu().numpy()
    B1 = codes.cpu().numpy().astype(np.int16) + 1
    dists, idx = rq.linscan_pq(B1, Qn, Cl, 8 * m, k)
    assert idx.dtype == np.uint32 and int(idx.min()) >= 1
    t0 = time.perf_counter()
    got = xt.certify(dists, idx, k, xt.adc_lut(centers, torch.from_numpy(Qn).cuda()), codes, n, id_base=1)
    _report("host_pointer_nq%d_k%d" % (nq, k), certified=got, certify_s=round(time.perf_counter() - t0, 1))
    assert got == nq
