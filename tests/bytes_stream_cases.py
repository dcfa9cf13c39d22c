"""The stream cases of the byte-input encode (rq_dev_encode_pq_bytes, rq_dev_encode_opq_bytes, rq_dev_rotate_T_bytes), registered
with the harness of tests/stream_cases.py -- a plain helper module: no fixtures, no pytest hooks.

tests/test_gpu_streams.py derives its coverage from stream_cases.CASES / ENTRIES and requires one case per `void *stream`
prototype of the header.  Importing this module adds the cases below to that table; tests/test_gpu_encode_bytes.py and
tests/test_encode_bytes_host.py import it, so the table is complete whenever the suite is collected as a whole.  Each entry
point has a case on the path with byte loaders and one on the path that widens into library scratch first (whose widening
launch must sit on the caller's stream as well)."""
import numpy as np

import stream_cases as sc


def _data(shape):
    from test_gpu_encode_bytes import _case, _cat
    X, C, ref = _case(shape, "sift")
    return np.array(X), _cat(C), ref          # (a writable copy: the harness hands it to torch)


def _encode_pq_bytes(shape, kernel):
    def build():
        d, m, h = shape
        X, Ccat, ref = _data(shape)

        def run(dev, out):
            return {"codes": sc._rqd().encode_pq(dev["X"], dev["C"], m, h, out=out["codes"])}

        def check(got):
            assert np.array_equal(got["codes"], ref), "rows differ: %d" % int((got["codes"] != ref).any(axis=1).sum())

        return sc.Case("rq_dev_encode_pq_bytes", {"X": X, "C": Ccat}, run, check, outputs={"codes": (ref.shape, np.uint8)},
                       after=sc._enc_kernel_is(kernel))
    return build


def _encode_opq_bytes(shape):
    def build():
        import rayuela_jl_amd.synth as synth
        d, m, h = shape
        X, Ccat, _ = _data(shape)
        R = synth.rotation(d, seed=7)
        ref = sc._oracle().encode_opq(X.astype(np.float32), R, Ccat, m, h)

        def run(dev, out):
            return {"codes": sc._rqd().encode_opq(dev["X"], dev["R"], dev["C"], m, h, out=out["codes"])}

        def check(got):
            assert np.array_equal(got["codes"], ref), "rows differ: %d" % int((got["codes"] != ref).any(axis=1).sum())

        return sc.Case("rq_dev_encode_opq_bytes", {"X": X, "R": R, "C": Ccat}, run, check, outputs={"codes": (ref.shape, np.uint8)})
    return build


def _rotate_T_bytes(shape):
    def build():
        import rayuela_jl_amd.synth as synth
        d = shape[0]
        X = _data(shape)[0]
        R = synth.rotation(d, seed=d)
        ref = sc._oracle().rotate_T(R, X.astype(np.float32))

        def run(dev, out):
            return {"RX": sc._rqd().rotate_T(dev["R"], dev["X"], out=out["RX"])}

        def check(got):
            assert sc._eq_bits(got["RX"], ref)

        return sc.Case("rq_dev_rotate_T_bytes", {"R": R, "X": X}, run, check, outputs={"RX": (X.shape, np.float32)})
    return build


# (128, 8, 256): byte filter, byte rotation.  (128, 4, 256): sub 32, widened, direct kernel.  (30, 3, 64): d = 30 has no byte
# rotation -- widened, generic rotation, then the f32 filter
BYTES_CASES = {
    "encode_pq_bytes_filter": ("rq_dev_encode_pq_bytes", _encode_pq_bytes((128, 8, 256), "encode_pq_filter_bytes_kernel")),
    "encode_pq_bytes_widened": ("rq_dev_encode_pq_bytes", _encode_pq_bytes((128, 4, 256), "encode_pq_direct_kernel")),
    "encode_opq_bytes": ("rq_dev_encode_opq_bytes", _encode_opq_bytes((128, 8, 256))),
    "encode_opq_bytes_widened": ("rq_dev_encode_opq_bytes", _encode_opq_bytes((30, 3, 64))),
    "rotate_T_bytes": ("rq_dev_rotate_T_bytes", _rotate_T_bytes((128, 8, 256))),
    "rotate_T_bytes_widened": ("rq_dev_rotate_T_bytes", _rotate_T_bytes((30, 3, 64))),
}
sc.CASES.update(BYTES_CASES)
sc.ENTRIES.update(entry for entry, _ in BYTES_CASES.values())
