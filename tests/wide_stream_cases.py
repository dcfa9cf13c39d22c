"""The stream cases of the 16-bit encodes (rq_dev_encode_pq_wide, rq_dev_encode_opq_wide, rq_dev_encode_rvq_wide), registered
with the harness of tests/stream_cases.py exactly as tests/bytes_stream_cases.py does -- a plain helper module: no fixtures, no
pytest hooks.  tests/test_gpu_encode_wide.py and tests/test_wide_oracle.py import it, so the table of
tests/test_gpu_streams.py is complete whenever the suite is collected as a whole.  h = 512: the streaming kernel, whose norms
pass, scratch and (RVQ) memset of the counts must sit on the caller's stream as well; one h = 256 case: the byte kernels into
library scratch (WS_H16_CODES), then widened."""
import numpy as np

import stream_cases as sc
import wide_oracle as wo


def _data(n, d, m, h, seed):
    import rayuela_jl_amd.synth as synth
    X = synth.sift_like(n, d, seed=seed)
    rng = np.random.default_rng(seed)
    off = wo.splitarray(d, m)
    C = [np.ascontiguousarray(X[rng.integers(0, n, h), off[i]:off[i + 1]]) for i in range(m)]
    return X, np.concatenate([c.reshape(-1) for c in C])


def _encode_pq_wide(n, d, m, h, kernel="encode_h16_kernel"):
    def build():
        X, Ccat = _data(n, d, m, h, 31)
        ref = wo.encode_pq_wide(sc._oracle(), X, Ccat, m, h)

        def run(dev, out):
            return {"codes": sc._rqd().encode_pq_wide(dev["X"], dev["C"], m, h, out=out["codes"])}

        def check(got):
            assert np.array_equal(got["codes"], ref), "rows differ: %d" % int((got["codes"] != ref).any(axis=1).sum())

        def after():
            ran = (sc._L().lib().rq_last_encode_kernel() or b"").decode()
            assert (ran == kernel) if kernel else (ran != "encode_h16_kernel"), (ran, kernel)

        return sc.Case("rq_dev_encode_pq_wide", {"X": X, "C": Ccat}, run, check, outputs={"codes": (ref.shape, np.int16)},
                       after=after)
    return build


def _encode_opq_wide(n, d, m, h):
    def build():
        import rayuela_jl_amd.synth as synth
        X, Ccat = _data(n, d, m, h, 32)
        R = synth.rotation(d, seed=9)
        ref = wo.encode_pq_wide(sc._oracle(), sc._oracle().rotate_T(R, X), Ccat, m, h)

        def run(dev, out):
            return {"codes": sc._rqd().encode_opq_wide(dev["X"], dev["R"], dev["C"], m, h, out=out["codes"])}

        def check(got):
            assert np.array_equal(got["codes"], ref), "rows differ: %d" % int((got["codes"] != ref).any(axis=1).sum())

        return sc.Case("rq_dev_encode_opq_wide", {"X": X, "R": R, "C": Ccat}, run, check,
                       outputs={"codes": (ref.shape, np.int16)}, after=sc._enc_kernel_is("encode_h16_kernel"))
    return build


def _encode_rvq_wide(n, d, m, h):
    def build():
        rng = np.random.default_rng(d + 5)
        X = (rng.standard_normal((n, d)) * 10).astype(np.float32)
        Cs = (rng.standard_normal((m, h, d)) * 5).astype(np.float32)
        codes0, counts0, Xr0 = wo.encode_rvq_wide(sc._oracle(), X, Cs)

        def run(dev, out):
            codes, counts = sc._rqd().encode_rvq_wide(dev["Xr"], dev["C"], out=out["codes"], want_counts=True)
            return {"codes": codes, "counts": counts, "Xr": dev["Xr"]}

        def check(got):
            assert np.array_equal(got["codes"], codes0)
            assert np.array_equal(got["counts"].astype(np.uint32), counts0)
            assert sc._eq_bits(got["Xr"], Xr0)

        return sc.Case("rq_dev_encode_rvq_wide", {"Xr": X, "C": Cs}, run, check, outputs={"codes": (codes0.shape, np.int16)},
                       after=sc._enc_kernel_is("encode_h16_kernel"))
    return build


WIDE_CASES = {
    "encode_pq_wide": ("rq_dev_encode_pq_wide", _encode_pq_wide(4_001, 64, 4, 512)),
    "encode_pq_wide_chunked": ("rq_dev_encode_pq_wide", _encode_pq_wide(3_000, 80, 2, 512)),
    "encode_pq_wide_h256_byte_kernels": ("rq_dev_encode_pq_wide", _encode_pq_wide(2_001, 64, 4, 256, kernel=None)),
    "encode_opq_wide": ("rq_dev_encode_opq_wide", _encode_opq_wide(4_001, 32, 4, 512)),
    "encode_rvq_wide": ("rq_dev_encode_rvq_wide", _encode_rvq_wide(3_001, 48, 2, 512)),
}
sc.CASES.update(WIDE_CASES)
sc.ENTRIES.update(entry for entry, _ in WIDE_CASES.values())
