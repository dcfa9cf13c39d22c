"""The stream case of the beam encoder over wide codebooks (rq_dev_encode_rvq_beam_wide), registered with the harness of
tests/stream_cases.py in the manner of tests/beam_stream_cases.py -- a plain helper module: no fixtures, no pytest hooks.

tests/test_gpu_streams.py derives its coverage from stream_cases.CASES / ENTRIES and requires one case per `void *stream`
prototype of the header.  Importing this module adds the case below to that table; tests/test_gpu_beam_wide.py and
tests/test_beam_wide_oracle.py import it, so the table is complete whenever the suite is collected as a whole, and
tests/test_gpu_beam_wide.py runs the same case behind the same delay itself."""
import numpy as np

import beam_wide_oracle as bw
import stream_cases as sc


def _encode_rvq_beam_wide(shape, H, nsplits):
    def build():
        X, C, codes, Xr, cost = bw.expected(shape, H)
        n, d = X.shape
        m = C.shape[0]

        def run(dev, out):
            from rayuela_jl_amd import _lib
            _lib.check(_lib.lib().rq_dev_encode_rvq_beam_wide(out["codes"].data_ptr(), out["Xr"].data_ptr(), out["cost"].data_ptr(),
                                                              dev["X"].data_ptr(), dev["C"].data_ptr(), n, d, m, C.shape[1], H,
                                                              nsplits, sc._stream()))
            return dict(out, X=dev["X"])

        def check(got):
            assert np.array_equal(got["codes"], codes), "rows differ: %d of %d" % (int((got["codes"] != codes).any(axis=1).sum()), n)
            assert sc._eq_bits(got["Xr"], Xr) and sc._eq_bits(got["cost"], cost)
            assert sc._eq_bits(got["X"], X), "X was overwritten"

        return sc.Case("rq_dev_encode_rvq_beam_wide", {"X": X, "C": C}, run, check,
                       outputs={"codes": ((n, m), np.int16), "Xr": ((n, d), np.float32), "cost": ((n,), np.float32)})
    return build


BEAM_WIDE_CASES = {
    "encode_rvq_beam_wide_H3_nsplits3": ("rq_dev_encode_rvq_beam_wide", _encode_rvq_beam_wide(bw.GPU_SHAPES[0][:5], 3, 3)),
}
sc.CASES.update(BEAM_WIDE_CASES)
sc.ENTRIES.update(entry for entry, _ in BEAM_WIDE_CASES.values())
