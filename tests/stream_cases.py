"""One case per `void *stream` entry point of include/rayuela_hip.h, and the harness that runs a case on a side stream
(tests/test_gpu_streams.py).  A plain helper module: no fixtures, no pytest hooks.

A case holds its inputs as numpy arrays, harmless poison for each of them (finite floats, codes below h, a valid permutation:
a library that wrongly consumes poison gives a wrong answer, never an out-of-range access), a `run(dev, out)` that calls the
entry point on the CURRENT torch stream and returns {name: result tensor}, and a `check(got)` that compares the results with
the oracle / CPU restatement the family's own test file uses, by the same comparison (bits, or that file's float64 tolerances).
Cases are built lazily (CASES maps a name to (entry point, builder)); ENTRIES needs neither a GPU nor the oracle."""
import functools
import time

import numpy as np

E_K = 2.0 ** -14            # tests/test_gpu_encode_margin.py: the bound the split encode filter rests on
RQ_MAX_K = 65536
SENTINEL = 0xA5             # every byte of an output before the call (float32 0xA5A5A5A5 = -2.9e-16: finite)


class Case:
    def __init__(self, entry, inputs, run, check, outputs=None, poison=None, switches=None, precheck=None, after=None, name=None):
        self.entry, self.inputs, self.run, self.check = entry, inputs, run, check
        self.name = name or entry
        self.outputs = outputs or {}                  # name -> (shape, numpy dtype): allocated by the harness, sentinel-filled
        self.poison = {k: np.zeros_like(v) for k, v in inputs.items()}
        self.poison.update(poison or {})
        self.switches = switches or {}
        self.precheck, self.after = precheck, after   # host-only looks at which path the call takes / took


def _eq_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _L():
    from rayuela_jl_amd import _lib
    return _lib


def _rqd():
    from rayuela_jl_amd import device
    return device


def _oracle():
    from oracle import oracle
    oracle.lib()
    return oracle


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _enc_kernel_is(name):
    def after():
        ran = (_L().lib().rq_last_encode_kernel() or b"").decode()
        assert ran == name, (ran, name)
    return after


def _scan_kernel_starts(prefix):
    def after():
        ran = (_L().lib().rq_last_scan_kernel() or b"").decode()
        assert ran.startswith(prefix), (ran, prefix)
    return after


# ---- encode / rotation / RVQ ------------------------------------------------------------------------------------------------
def _encode_pq(d, m, kernel, switches=None):
    def build():
        from test_gpu_switches import _enc_setup
        X, Ccat, ref = _enc_setup(d, m)

        def run(dev, out):
            return {"codes": _rqd().encode_pq(dev["X"], dev["C"], m, 256, out=out["codes"])}

        def check(got):
            assert np.array_equal(got["codes"], ref), "rows differ: %d" % int((got["codes"] != ref).any(axis=1).sum())

        return Case("rq_dev_encode_pq", {"X": X, "C": Ccat}, run, check, outputs={"codes": (ref.shape, np.uint8)},
                    switches=switches, after=_enc_kernel_is(kernel))
    return build


def _encode_pq_filter_w():
    from test_gpu_switches import _enc_setup
    d, m, h = 128, 8, 256
    X, Ccat, ref = _enc_setup(d, m)
    U = _oracle().pq_distmat(X, Ccat.reshape(-1), m, h).astype(np.float64)             # [n][m][h] canonical distances
    sa = (Ccat.astype(np.float64) ** 2).sum(2)                                         # [m][h]
    sb = (X.astype(np.float64).reshape(-1, m, d // m) ** 2).sum(2)                     # [n][m]

    def run(dev, out):
        codes, W = _rqd().encode_pq_filter_w(dev["X"], dev["C"], m, h)
        return {"codes": codes, "W": W}

    def check(got):
        assert np.array_equal(got["codes"], ref)
        assert not np.isnan(got["W"]).any(), "the split kernel did not run (W untouched)"
        den = sa[None] + sb[:, :, None]
        r = np.abs(got["W"].astype(np.float64) + sb[:, :, None] - np.maximum(U, 0)) / den
        assert r[den > 0].max() <= E_K, r[den > 0].max() / E_K

    return Case("rq_dev_encode_pq_filter_w", {"X": X, "C": Ccat}, run, check)


def _encode_opq(n=None):
    def build():
        import rayuela_jl_amd.synth as synth
        from test_gpu_switches import _enc_setup
        d, m, h = 128, 8, 256
        X, Ccat, _ = _enc_setup(d, m)
        X = X if n is None else np.ascontiguousarray(X[:n])
        R = synth.rotation(d, seed=7)
        ref = _oracle().encode_opq(X, R, Ccat, m, h)

        def run(dev, out):
            return {"codes": _rqd().encode_opq(dev["X"], dev["R"], dev["C"], m, h, out=out["codes"])}

        def check(got):
            assert np.array_equal(got["codes"], ref), "rows differ: %d" % int((got["codes"] != ref).any(axis=1).sum())

        return Case("rq_dev_encode_opq", {"X": X, "R": R, "C": Ccat}, run, check, outputs={"codes": (ref.shape, np.uint8)})
    return build


@functools.lru_cache(maxsize=None)
def encode_opq_rows(n):
    """rq_dev_encode_opq on the first n rows of the encode base: its library scratch is n * d * 4 bytes."""
    case = _encode_opq(n)()
    case.name = "encode_opq_%d_rows" % n
    return case


def _rotate_T():
    import rayuela_jl_amd.synth as synth
    from test_gpu_switches import _enc_setup
    d = 128
    X = _enc_setup(d, 8)[0]
    R = synth.rotation(d, seed=d)
    ref = _oracle().rotate_T(R, X)

    def run(dev, out):
        return {"RX": _rqd().rotate_T(dev["R"], dev["X"], out=out["RX"])}

    def check(got):
        assert _eq_bits(got["RX"], ref)

    return Case("rq_dev_rotate_T", {"R": R, "X": X}, run, check, outputs={"RX": (X.shape, np.float32)})


def _encode_rvq():
    n, d, m, h = 4_001, 96, 3, 256
    rng = np.random.default_rng(d + 4)
    X = (rng.standard_normal((n, d)) * 10).astype(np.float32)
    Cs = (rng.standard_normal((m, h, d)) * 5).astype(np.float32)
    codes0, counts0, Xr0 = _oracle().encode_rvq(X, Cs, with_extras=True)

    def run(dev, out):
        codes, counts = _rqd().encode_rvq(dev["Xr"], dev["C"], out=out["codes"], want_counts=True)
        return {"codes": codes, "counts": counts, "Xr": dev["Xr"]}

    def check(got):
        assert np.array_equal(got["codes"], codes0)
        assert np.array_equal(got["counts"].astype(np.uint32), counts0)
        assert _eq_bits(got["Xr"], Xr0)

    return Case("rq_dev_encode_rvq", {"Xr": X, "C": Cs}, run, check, outputs={"codes": (codes0.shape, np.uint8)})


# ---- scans ------------------------------------------------------------------------------------------------------------------
SCAN_SHAPE = (200_000, 8, 4, 12, 41)          # tests/test_gpu_switches.py::test_scan_switch's base


def _check_scan(d0, i0):
    def check(got):
        assert np.array_equal(got["ids"].view(np.uint32), i0), "ids differ"
        assert _eq_bits(got["dists"], d0), "distances differ"
    return check


def _scan_outputs(nq, K):
    return {"dists": ((nq, K), np.float32), "ids": ((nq, K), np.int32)}


def _run_linscan(K):
    def run(dev, out):
        d, i = _rqd().linscan(dev["codes"], dev["centers"], dev["queries"], K, out=(out["dists"], out["ids"]))
        return {"dists": d, "ids": i}
    return run


def _linscan(K, in_call_order):
    def build():
        from test_gpu_switches import _scan_setup
        codes, centers, queries, ref = _scan_setup(*SCAN_SHAPE)
        (n, m), nq = codes.shape, queries.shape[0]

        def precheck():
            assert _L().lib().rq_scan_orders_in_call(n, nq, K) == int(in_call_order)

        return Case("rq_dev_linscan", {"codes": codes, "centers": centers, "queries": queries}, _run_linscan(K),
                    _check_scan(*ref[K]), outputs=_scan_outputs(nq, K), switches=dict(ORDER_MIN_NQ=1) if in_call_order else None,
                    precheck=precheck, after=_scan_kernel_starts("adc_scan_kernel<8"))
    return build


def _linscan_bulk():
    from test_gpu_bulk_topk import _base
    n, m, sub, nq, K = 100_000, 8, 4, 3, RQ_MAX_K + 1
    centers, queries, codes = _base(n, m, sub, nq, seed=1)
    d0, i0 = _oracle().linscan_aqd_query(codes, centers, queries, K)

    def precheck():
        assert _L().scan_plan(n, nq, m, m * sub, K)["bulk"] == 1

    return Case("rq_dev_linscan", {"codes": codes, "centers": centers, "queries": queries}, _run_linscan(K),
                _check_scan(d0, i0), outputs=_scan_outputs(nq, K), precheck=precheck,
                after=_scan_kernel_starts("adc_bulk_keys_kernel<8"))


def _linscan_padded():
    """m = 5 is no tiled row width: the call first pads the rows to 8 bytes in library scratch (WS_PAD)."""
    from test_gpu_switches import _scan_setup
    n, m, sub, nq, K = 70_001, 5, 4, 5, 100
    codes, centers, queries, ref = _scan_setup(n, m, sub, nq, 31, Ks=(K,))
    return Case("rq_dev_linscan", {"codes": codes, "centers": centers, "queries": queries}, _run_linscan(K),
                _check_scan(*ref[K]), outputs=_scan_outputs(nq, K), after=_scan_kernel_starts("adc_scan_kernel<8"))


def _adc_lut():
    from test_gpu_switches import _scan_setup
    _, centers, queries, _ = _scan_setup(*SCAN_SHAPE)
    oracle = _oracle()
    ref = np.stack([oracle.adc_lut(centers, queries[q]).reshape(centers.shape[0], 256) for q in range(queries.shape[0])])

    def run(dev, out):
        return {"lut": _rqd().adc_lut(dev["centers"], dev["queries"])}

    def check(got):
        assert _eq_bits(got["lut"], ref)

    return Case("rq_dev_adc_lut", {"centers": centers, "queries": queries}, run, check)


def _ordered_base():
    """(codes, ordered rows [n][8], perm [n]) of the scan base, ordered once on the default stream (rows of one sort bucket
    land in atomic order, so the permutation is this run's own)."""
    import torch
    from test_gpu_switches import _scan_setup
    codes = _scan_setup(*SCAN_SHAPE)[0]
    ob = _rqd().order_rows(torch.from_numpy(codes).cuda())
    torch.cuda.synchronize()
    assert ob.perm is not None
    return codes, ob.codes.cpu().numpy().copy(), ob.perm.cpu().numpy().copy()


def _order_rows():
    from test_gpu_switches import _scan_setup
    codes = _scan_setup(*SCAN_SHAPE)[0]
    n, m = codes.shape

    def run(dev, out):
        ob = _rqd().order_rows(dev["codes"])
        assert ob.perm is not None
        return {"ordered": ob.codes, "perm": ob.perm}

    def check(got):
        perm = got["perm"].astype(np.int64)
        assert np.array_equal(np.sort(perm), np.arange(n)), "not a permutation"
        assert np.array_equal(got["ordered"][:, :m], codes[perm]), "rows did not move with the permutation"

    return Case("rq_dev_order_rows", {"codes": codes}, run, check)


def _linscan_ordered():
    from test_gpu_switches import _scan_setup
    codes, centers, queries, ref = _scan_setup(*SCAN_SHAPE)
    _, ordered, perm = _ordered_base()
    n, m = codes.shape
    nq, K = queries.shape[0], 100

    def run(dev, out):
        rqd = _rqd()
        ob = rqd.OrderedBase(None, dev["ordered"], dev["perm"], n, m)
        d, i = rqd.linscan(ob, dev["centers"], dev["queries"], K, out=(out["dists"], out["ids"]))
        return {"dists": d, "ids": i}

    return Case("rq_dev_linscan_ordered", {"ordered": ordered, "perm": perm, "centers": centers, "queries": queries}, run,
                _check_scan(*ref[K]), outputs=_scan_outputs(nq, K),
                poison={"perm": np.arange(n, dtype=perm.dtype)})       # zero rows in the identity order: valid, wrong


def _linscan_aq(lsq):
    def build():
        import rayuela_jl_amd.synth as synth
        n, m, d, nq, K = 100_003, 16, 96, 9, 100          # tests/test_gpu_aq.py::test_aq_vs_oracle_random
        rng = np.random.default_rng(n + m)
        cb = rng.standard_normal((m * 256, d)).astype(np.float32)
        q = rng.standard_normal((nq, d)).astype(np.float32)
        codes = synth.random_codes(n, m, seed=n)
        nrm = (rng.random(n) * 50).astype(np.float32)
        oracle = _oracle()
        d0, i0 = oracle.linscan_lsq(codes, cb, q, nrm, K) if lsq else oracle.linscan_cq(codes, cb, q, K)
        inputs = {"codes": codes, "codebooks": cb, "queries": q}
        if lsq:
            inputs["dbnorms"] = nrm

        def run(dev, out):
            dd, ii = _rqd().linscan_aq(dev["codes"], dev["codebooks"], dev["queries"], K, dbnorms=dev.get("dbnorms"),
                                       id_base=1, out=(out["dists"], out["ids"]))         # the oracles' ids are one-based
            return {"dists": dd, "ids": ii}

        def check(got):
            assert np.array_equal(got["ids"].view(np.int32), i0), "ids differ"
            assert _eq_bits(got["dists"], d0), "distances differ"

        return Case("rq_dev_linscan_aq", inputs, run, check, outputs=_scan_outputs(nq, K))
    return build


def _merge_topk():
    import torch
    from test_gpu_switches import _scan_setup
    codes, centers, queries, ref = _scan_setup(*SCAN_SHAPE)
    K, bounds = 100, [0, 70_000, 150_000, 200_000]
    rqd = _rqd()
    cen, qs = torch.from_numpy(centers).cuda(), torch.from_numpy(queries).cuda()
    keys = torch.stack([rqd.linscan(torch.from_numpy(codes[a:b]).cuda(), cen, qs, K, id_offset=a, want_keys=True)
                        for a, b in zip(bounds[:-1], bounds[1:])], dim=1).contiguous()
    torch.cuda.synchronize()
    keys = keys.cpu().numpy()

    def run(dev, out):
        d, i = rqd.merge_topk(dev["keys"], K, out=(out["dists"], out["ids"]))
        return {"dists": d, "ids": i}

    return Case("rq_dev_merge_topk", {"keys": keys}, run, _check_scan(*ref[K]), outputs=_scan_outputs(queries.shape[0], K))


def _synth_codes():
    import rayuela_jl_amd.synth as synth
    n, m, seed, row0 = 300_001, 8, 77, 12_345
    ref = synth.random_codes(n, m, seed=seed, row0=row0)

    def run(dev, out):
        L = _L()
        L.check(L.lib().rq_dev_synth_codes(out["codes"].data_ptr(), n, m, seed, row0, _stream()))
        return {"codes": out["codes"]}

    def check(got):
        assert np.array_equal(got["codes"], ref)

    return Case("rq_dev_synth_codes", {}, run, check, outputs={"codes": ((n, m), np.uint8)})


# ---- training reductions (tolerances: tests/test_gpu_train.py) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_setup():
    from oracle import train_oracle as to
    n, d, m, h = 7_001, 96, 16, 256             # tests/test_gpu_switches.py::test_training_reductions_at_unaligned_offsets
    rng = np.random.default_rng(4)
    X = (rng.standard_normal((n, d)) * 20 + 3).astype(np.float32)
    codes = rng.integers(0, h, (n, m), dtype=np.uint8)
    off = to.offsets(d, m)
    Cs = [rng.standard_normal((h, off[q + 1] - off[q])).astype(np.float32) * 20 for q in range(m)]
    Ccat = np.concatenate([c.reshape(-1) for c in Cs])
    CB0 = to.reconstruct(Cs, codes, off, d)
    G0 = X.astype(np.float64).T @ CB0.astype(np.float64)
    e0 = ((X.astype(np.float64) - CB0) ** 2).sum() / n
    Cn = np.concatenate([c.reshape(-1) for c in to.update_centers(Cs, X, codes, off, h)])
    return dict(n=n, d=d, m=m, h=h, X=X, codes=codes, Ccat=Ccat, CB0=CB0, G0=G0, e0=e0, Cn=Cn)


def _check_gram(G0):
    def check(got):
        assert np.allclose(got["G"], G0, rtol=1e-5, atol=1e-5 * np.abs(G0).max())
    return check


def _check_qerror(e0, n):
    def check(got):
        assert abs(float(got["acc"][0]) / n - e0) <= 1e-9 * e0, (float(got["acc"][0]) / n, e0)
    return check


def _update_centers():
    s = _train_setup()
    m, h = s["m"], s["h"]

    def run(dev, out):
        counts = _rqd().update_centers(dev["C"], dev["X"], dev["codes"], m, h)
        return {"C": dev["C"], "counts": counts}

    def check(got):
        assert np.allclose(got["C"], s["Cn"], rtol=1e-5, atol=1e-4)
        assert np.array_equal(got["counts"], np.stack([np.bincount(s["codes"][:, i], minlength=h) for i in range(m)]))

    return Case("rq_dev_update_centers", {"C": s["Ccat"], "X": s["X"], "codes": s["codes"]}, run, check)


def _reconstruct():
    s = _train_setup()

    def run(dev, out):
        return {"CB": _rqd().reconstruct(dev["codes"], dev["C"], s["d"], s["h"], out=out["CB"])}

    def check(got):
        assert np.array_equal(got["CB"], s["CB0"])

    return Case("rq_dev_reconstruct", {"codes": s["codes"], "C": s["Ccat"]}, run, check,
                outputs={"CB": ((s["n"], s["d"]), np.float32)})


def _qerror():
    s = _train_setup()

    def run(dev, out):
        L = _L()
        L.check(L.lib().rq_dev_qerror(out["acc"].data_ptr(), dev["X"].data_ptr(), dev["CB"].data_ptr(), s["n"], s["d"], _stream()))
        return {"acc": out["acc"]}

    return Case("rq_dev_qerror", {"X": s["X"], "CB": s["CB0"]}, run, _check_qerror(s["e0"], s["n"]),
                outputs={"acc": ((1,), np.float64)})


def _gram():
    s = _train_setup()

    def run(dev, out):
        return {"G": _rqd().gram(dev["X"], dev["CB"])}

    return Case("rq_dev_gram", {"X": s["X"], "CB": s["CB0"]}, run, _check_gram(s["G0"]))


def _gram_codes():
    s = _train_setup()

    def run(dev, out):
        return {"G": _rqd().gram_codes(dev["X"], dev["codes"], dev["C"], s["h"])}

    return Case("rq_dev_gram_codes", {"X": s["X"], "codes": s["codes"], "C": s["Ccat"]}, run, _check_gram(s["G0"]))


def _qerror_codes():
    s = _train_setup()

    def run(dev, out):
        L = _L()
        L.check(L.lib().rq_dev_qerror_codes(out["acc"].data_ptr(), dev["X"].data_ptr(), dev["codes"].data_ptr(),
                                            dev["C"].data_ptr(), s["n"], s["d"], s["m"], s["h"], _stream()))
        return {"acc": out["acc"]}

    return Case("rq_dev_qerror_codes", {"X": s["X"], "codes": s["codes"], "C": s["Ccat"]}, run,
                _check_qerror(s["e0"], s["n"]), outputs={"acc": ((1,), np.float64)})


# ---- LSQ: ICM encoding and the codebook update ---------------------------------------------------------------------------------
def _encode_icm(n, d, m, h, seed):
    """h < 256: the code range check reads a flag back (and synchronises the stream) before any encode work; h = 256: it does not."""
    def build():
        import icm_oracle as io
        from test_gpu_icm import _data
        X, C, B0 = _data(n, d, m, h, seed=seed)
        args = (2, 2, 2, True)
        b0, c0 = io.ils(_oracle(), X, C, B0, *args, seed=1)

        def run(dev, out):
            L = _L()
            L.check(L.lib().rq_dev_encode_icm(out["codes"].data_ptr(), dev["B0"].data_ptr(), out["cost"].data_ptr(),
                                              dev["X"].data_ptr(), dev["C"].data_ptr(), n, d, m, h, 2, 2, 2, 1, 1, 0, 1, _stream()))
            return {"codes": out["codes"], "cost": out["cost"]}

        def check(got):
            bad = np.flatnonzero((got["codes"] != b0).any(axis=1))
            assert bad.size == 0, "%d rows differ" % bad.size
            assert _eq_bits(got["cost"], c0), "per-row costs differ"

        return Case("rq_dev_encode_icm", {"X": X, "C": C, "B0": B0}, run, check,
                    outputs={"codes": ((n, m), np.uint8), "cost": ((n,), np.float32)})
    return build


def _encode_icm_dup_ties():
    """Every conditioning step tied 64 ways (tests/icm_tie_cases.py, codeword l = codeword l % 4): the lowest copy must win."""
    import icm_tie_cases as tc
    case = tc.BYTE_LOW[2]
    assert (case.m, case.h, case.P) == (4, 256, 4)
    X, C, B0, b0, c0 = tc.expected(case)
    n, d, m, h = case.n, case.d, case.m, case.h
    ils, icm, npert, randord = case.args

    def run(dev, out):
        L = _L()
        L.check(L.lib().rq_dev_encode_icm(out["codes"].data_ptr(), dev["B0"].data_ptr(), out["cost"].data_ptr(), dev["X"].data_ptr(),
                                          dev["C"].data_ptr(), n, d, m, h, ils, icm, npert, 1 if randord else 0, tc.ILS_SEED, 0, 1,
                                          _stream()))
        return {"codes": out["codes"], "cost": out["cost"]}

    def check(got):
        assert got["codes"].max() < case.P, "a higher copy won"
        bad = np.flatnonzero((got["codes"] != b0).any(axis=1))
        assert bad.size == 0, "%d rows differ" % bad.size
        assert _eq_bits(got["cost"], c0), "per-row costs differ"

    return Case("rq_dev_encode_icm", {"X": X, "C": C, "B0": B0}, run, check,
                outputs={"codes": ((n, m), np.uint8), "cost": ((n,), np.float32)})


def _lsq_data(m, h, d, n):
    rng = np.random.default_rng(n + m)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    return X, codes


def _lsq_normal_eq(m, h, d, n):
    def build():
        import lsq_update_oracle as lo
        from test_gpu_lsq_train import _wide
        rng = np.random.default_rng(m * 1000 + h + d + n)
        X = _wide(rng, n, d)                        # summation order shows in the bits
        codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
        A0, b0 = lo.normal_eq(X, codes, h)

        def run(dev, out):
            A, b = _rqd().lsq_normal_eq(dev["X"], dev["codes"], h)
            return {"A": A, "b": b}

        def check(got):
            assert _eq_bits(got["A"], A0), "A differs in %d entries" % int((got["A"] != A0).sum())
            assert _eq_bits(got["b"], b0), "b differs in %d entries" % int((got["b"] != b0).sum())

        return Case("rq_dev_lsq_normal_eq", {"X": X, "codes": codes}, run, check)
    return build


def _update_codebooks_lsq(m, h, d, n):
    def build():
        from test_gpu_lsq_train import _check_against_numpy
        X, codes = _lsq_data(m, h, d, n)

        def run(dev, out):
            return {"C": _rqd().update_codebooks_lsq(dev["X"], dev["codes"], h, out=out["C"])}

        def check(got):
            assert np.isfinite(got["C"]).all()
            _check_against_numpy(X, codes, h, got["C"])

        return Case("rq_dev_update_codebooks_lsq", {"X": X, "codes": codes}, run, check, outputs={"C": ((m, h, d), np.float32)})
    return build


# ---- chain quantization ----------------------------------------------------------------------------------------------------
def chain_data(n, d, m, h, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    C = (rng.standard_normal((m, h, d)) * 0.5).astype(np.float32)
    return X, C


def _quantize_chainq(n, d, m, h, nsplits, seed=18):
    def build():
        import chain_oracle as co
        X, C = chain_data(n, d, m, h, seed)
        want = co.viterbi(_oracle(), X, C)

        def run(dev, out):
            return {"codes": _rqd().quantize_chainq(dev["X"], dev["C"], nsplits=nsplits, out=out["codes"])}

        def check(got):
            assert np.array_equal(got["codes"], want), "rows differ: %d of %d" % (int((got["codes"] != want).any(axis=1).sum()), n)

        return Case("rq_dev_quantize_chainq", {"X": X, "C": C}, run, check, outputs={"codes": ((n, m), np.uint8)})
    return build


def _update_codebooks_chain(m, h, d, n):
    def build():
        from test_gpu_chainq import _check_against_numpy, _zero_outside
        X, codes = _lsq_data(m, h, d, n)

        def run(dev, out):
            return {"C": _rqd().update_codebooks_chain(dev["X"], dev["codes"], h, out=out["C"])}

        def check(got):
            assert np.isfinite(got["C"]).all() and _zero_outside(got["C"])
            _check_against_numpy(X, codes, h, got["C"])

        return Case("rq_dev_update_codebooks_chain", {"X": X, "codes": codes}, run, check, outputs={"C": ((m, h, d), np.float32)})
    return build


def _reconstruct_aq():
    n, d, m, h = 5_003, 96, 8, 256
    rng = np.random.default_rng(23)
    C = rng.standard_normal((m, h, d)).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    ref = np.zeros((n, d), np.float32)          # include/rayuela_hip.h: f32 adds from +0 in codebook order
    for i in range(m):
        ref = ref + C[i][codes[:, i]]

    def run(dev, out):
        return {"CB": _rqd().reconstruct_aq(dev["codes"], dev["C"], out=out["CB"])}

    def check(got):
        assert _eq_bits(got["CB"], ref)

    return Case("rq_dev_reconstruct_aq", {"codes": codes, "C": C}, run, check, outputs={"CB": ((n, d), np.float32)})


# name -> (entry point, builder).  The shapes take the internal paths that differ in what they launch.
CASES = {
    "encode_pq_split_filter": ("rq_dev_encode_pq", _encode_pq(128, 8, "encode_pq_filter_kernel")),
    "encode_pq_direct": ("rq_dev_encode_pq", _encode_pq(128, 4, "encode_pq_direct_kernel")),
    "encode_pq_wide": ("rq_dev_encode_pq", _encode_pq(96, 1, "encode_wide_kernel", switches=dict(ENC_DIRECT=0))),
    "encode_pq_filter_w": ("rq_dev_encode_pq_filter_w", _encode_pq_filter_w),
    "encode_opq": ("rq_dev_encode_opq", _encode_opq()),
    "rotate_T": ("rq_dev_rotate_T", _rotate_T),
    "encode_rvq": ("rq_dev_encode_rvq", _encode_rvq),
    "adc_lut": ("rq_dev_adc_lut", _adc_lut),
    "linscan_k100": ("rq_dev_linscan", _linscan(100, False)),
    "linscan_k100_orders_in_call": ("rq_dev_linscan", _linscan(100, True)),
    "linscan_k1000_sample_sort": ("rq_dev_linscan", _linscan(1000, False)),
    "linscan_bulk_k65537": ("rq_dev_linscan", _linscan_bulk),
    "linscan_m5_padded_rows": ("rq_dev_linscan", _linscan_padded),
    "order_rows": ("rq_dev_order_rows", _order_rows),
    "linscan_ordered": ("rq_dev_linscan_ordered", _linscan_ordered),
    "linscan_aq_lsq": ("rq_dev_linscan_aq", _linscan_aq(True)),
    "linscan_aq_cq": ("rq_dev_linscan_aq", _linscan_aq(False)),
    "merge_topk": ("rq_dev_merge_topk", _merge_topk),
    "synth_codes": ("rq_dev_synth_codes", _synth_codes),
    "update_centers": ("rq_dev_update_centers", _update_centers),
    "reconstruct": ("rq_dev_reconstruct", _reconstruct),
    "qerror": ("rq_dev_qerror", _qerror),
    "gram": ("rq_dev_gram", _gram),
    "gram_codes": ("rq_dev_gram_codes", _gram_codes),
    "qerror_codes": ("rq_dev_qerror_codes", _qerror_codes),
    "encode_icm_h64_range_check": ("rq_dev_encode_icm", _encode_icm(500, 64, 8, 64, 9)),
    "encode_icm_h256": ("rq_dev_encode_icm", _encode_icm(256, 32, 8, 256, 3)),
    "encode_icm_dup_ties": ("rq_dev_encode_icm", _encode_icm_dup_ties),
    "lsq_normal_eq_h100": ("rq_dev_lsq_normal_eq", _lsq_normal_eq(4, 100, 33, 20_000)),
    "lsq_normal_eq_h256": ("rq_dev_lsq_normal_eq", _lsq_normal_eq(2, 256, 32, 20_000)),
    "update_codebooks_lsq_h100_range_check": ("rq_dev_update_codebooks_lsq", _update_codebooks_lsq(4, 100, 33, 20_000)),
    "update_codebooks_lsq_h256": ("rq_dev_update_codebooks_lsq", _update_codebooks_lsq(4, 256, 32, 30_000)),
    "quantize_chainq_one_chunk": ("rq_dev_quantize_chainq", _quantize_chainq(1_500, 32, 8, 256, 1)),
    "quantize_chainq_nsplits4": ("rq_dev_quantize_chainq", _quantize_chainq(1_500, 32, 8, 256, 4)),
    "update_codebooks_chain_h100_range_check": ("rq_dev_update_codebooks_chain", _update_codebooks_chain(5, 100, 30, 20_000)),
    "update_codebooks_chain_h256": ("rq_dev_update_codebooks_chain", _update_codebooks_chain(4, 256, 32, 30_000)),
    "reconstruct_aq": ("rq_dev_reconstruct_aq", _reconstruct_aq),
}
ENTRIES = {entry for entry, _ in CASES.values()}


@functools.lru_cache(maxsize=None)
def get(name):
    entry, build = CASES[name]
    case = build()
    assert case.entry == entry, (name, case.entry, entry)
    case.name = name
    return case


# ---- the harness: poison, delay, fill, call, consume, poison ---------------------------------------------------------------------
def _sentinel(shape, dtype):
    import torch
    t = torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def run_on_side_stream(case, stream, delay_cycles, log=None):
    """Runs `case` on `stream` behind a delay and returns its results {name: numpy array}, consumed on that stream only.

    1. device idle: inputs hold poison, outputs the sentinel;
    2. on `stream`: the delay, the true inputs copied over the poison, the sentinel again over the outputs (so an output written
       during the delay does not survive), the entry point, a clone of every result, poison over the inputs again;
    3. only `stream` is synchronised before the clones are read.
    Work the library puts on another stream without an event dependency runs during the delay.  A misplaced kernel or memset that
    reads a caller's input sees poison, one that writes a caller's output is overwritten or writes after the clone: the clones
    then differ from the expected output.  What library scratch holds when a call begins -- a reset that is missing or misplaced,
    a read of an earlier call's intermediates -- is the subject of tests/test_gpu_scratch.py, which runs these cases on scratch
    filled with four byte values and inside other cases' leftovers.  What the harness does NOT see: for the entries that
    synchronise the stream inside the call (the code range check with h < 256), whatever they queue after that point, which is
    no longer behind the delay."""
    import torch
    from switch_table import switches
    torch.cuda.synchronize()
    true = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.inputs.items()}
    pois = {k: torch.from_numpy(np.ascontiguousarray(case.poison[k])).cuda() for k in case.inputs}
    dev = {k: v.clone() for k, v in pois.items()}
    out = {k: _sentinel(*spec) for k, spec in case.outputs.items()}
    torch.cuda.synchronize()
    with switches(**case.switches), torch.cuda.stream(stream):
        if case.precheck:
            case.precheck()
        torch.cuda._sleep(int(delay_cycles))
        for k in dev:
            dev[k].copy_(true[k])
        for t in out.values():
            t.view(torch.uint8).fill_(SENTINEL)
        t0 = time.perf_counter()
        res = case.run(dev, out)
        t1 = time.perf_counter()
        if case.after:
            case.after()
        clones = {k: v.clone() for k, v in res.items()}
        for k in dev:
            dev[k].copy_(pois[k])
    stream.synchronize()
    got = {k: v.cpu().numpy() for k, v in clones.items()}
    if log is not None:
        log.append((case.name, (t1 - t0) * 1e3))
    torch.cuda.synchronize()          # after the results are on the host: nothing of this case is pending when its tensors are freed
    return got


def run_plain(case, inputs=None):
    """The case on the current stream with its true inputs (or `inputs`), synchronising only that stream: {name: numpy array}."""
    import torch
    from switch_table import switches
    s = torch.cuda.current_stream()
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in (inputs or case.inputs).items()}
    out = {k: _sentinel(*spec) for k, spec in case.outputs.items()}
    with switches(**case.switches):
        res = case.run(dev, out)
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}
