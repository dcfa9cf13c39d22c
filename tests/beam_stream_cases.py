"""The stream case of the beam encoder (rq_dev_encode_rvq_beam), registered with the harness of tests/stream_cases.py -- a plain
helper module: no fixtures, no pytest hooks.

tests/test_gpu_streams.py derives its coverage from stream_cases.CASES / ENTRIES and requires one case per `void *stream`
prototype of the header.  Importing this module adds the case below to that table; tests/test_gpu_beam.py and
tests/test_beam_oracle.py import it, so the table is complete whenever the suite is collected as a whole, and
tests/test_gpu_beam.py runs the same case behind the same delay itself, so it is covered however the files are selected."""
import numpy as np

import beam_oracle as bo
import stream_cases as sc


def _encode_rvq_beam(shape, H, nsplits):
    def build():
        X, C, codes, Xr, cost = bo.expected(shape, H)
        n, d = X.shape
        m = C.shape[0]

        def run(dev, out):
            from rayuela_jl_amd import _lib
            _lib.check(_lib.lib().rq_dev_encode_rvq_beam(out["codes"].data_ptr(), out["Xr"].data_ptr(), out["cost"].data_ptr(),
                                                         dev["X"].data_ptr(), dev["C"].data_ptr(), n, d, m, C.shape[1], H, nsplits,
                                                         sc._stream()))
            return dict(out, X=dev["X"])

        def check(got):
            assert np.array_equal(got["codes"], codes), "rows differ: %d of %d" % (int((got["codes"] != codes).any(axis=1).sum()), n)
            assert sc._eq_bits(got["Xr"], Xr) and sc._eq_bits(got["cost"], cost)
            assert sc._eq_bits(got["X"], X), "X was overwritten"

        return sc.Case("rq_dev_encode_rvq_beam", {"X": X, "C": C}, run, check,
                       outputs={"codes": ((n, m), np.uint8), "Xr": ((n, d), np.float32), "cost": ((n,), np.float32)})
    return build


BEAM_CASES = {
    "encode_rvq_beam_H3_nsplits3": ("rq_dev_encode_rvq_beam", _encode_rvq_beam(bo.GPU_SHAPES[0], 3, 3)),
}
sc.CASES.update(BEAM_CASES)
sc.ENTRIES.update(entry for entry, _ in BEAM_CASES.values())
