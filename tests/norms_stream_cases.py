"""The stream cases of the database-norms entry points (rq_dev_aq_norms, rq_dev_quantize_norms), registered with the harness of
tests/stream_cases.py -- a plain helper module: no fixtures, no pytest hooks.

tests/test_gpu_streams.py derives its coverage from stream_cases.CASES / ENTRIES and requires one case per `void *stream`
prototype of the header.  Importing this module adds the cases below to that table; tests/test_gpu_norms.py and
tests/test_norms_oracle.py import it, so the table is complete whenever the suite is collected as a whole, and
tests/test_gpu_norms.py runs the same cases behind the same delay itself, so they are covered however the files are selected."""
import numpy as np

import norms_oracle as no
import stream_cases as sc


def _aq_norms(n, d, m, h):
    def build():
        codes, C = no.norm_case(n, d, m, h)
        want = no.aq_norms(codes, C)

        def run(dev, out):
            return {"norms": sc._rqd().aq_norms(dev["codes"], dev["C"], out=out["norms"])}

        def check(got):
            assert sc._eq_bits(got["norms"], want), "norms differ in %d rows" % int((got["norms"] != want).sum())

        return sc.Case("rq_dev_aq_norms", {"codes": codes, "C": C}, run, check, outputs={"norms": ((n,), np.float32)})
    return build


def _quantize_norms():
    norms, cb = no.quant_cases()["hn256"]
    want = no.quantize(norms, cb)
    poison = {"norms": np.full_like(norms, 1e3), "cbnorms": np.arange(len(cb), dtype=np.float32)}

    def run(dev, out):
        codes, dbn = sc._rqd().quantize_norms(dev["norms"], dev["cbnorms"], out=out["codes"], dbnorms=out["dbnorms"])
        return {"codes": codes, "dbnorms": dbn}

    def check(got):
        assert np.array_equal(got["codes"], want) and sc._eq_bits(got["dbnorms"], cb[want])

    return sc.Case("rq_dev_quantize_norms", {"norms": norms, "cbnorms": cb}, run, check, poison=poison,
                   outputs={"codes": (want.shape, np.uint8), "dbnorms": (want.shape, np.float32)})


# the h = 100 case synchronises the stream in its code range check; the h = 256 case keeps every launch behind the delay
NORMS_CASES = {
    "aq_norms_h256": ("rq_dev_aq_norms", _aq_norms(5_003, 96, 16, 256)),
    "aq_norms_h100_range_check": ("rq_dev_aq_norms", _aq_norms(5_003, 130, 5, 100)),
    "quantize_norms": ("rq_dev_quantize_norms", _quantize_norms),
}
sc.CASES.update(NORMS_CASES)
sc.ENTRIES.update(entry for entry, _ in NORMS_CASES.values())
