"""The stream cases of the additive-quantizer entries over 16-bit codes (rq_dev_linscan_aq_wide, rq_dev_aq_lut_wide,
rq_dev_aq_norms_wide, rq_dev_quantize_norms_wide), registered with the harness of tests/stream_cases.py exactly as
tests/scan_wide_stream_cases.py does -- a plain helper module: no fixtures, no pytest hooks.  tests/test_gpu_aq_wide.py and
tests/test_aq_wide_oracle.py import it, so the table of tests/test_gpu_streams.py is complete whenever the suite is collected as a
whole.  Two cases per entry point: the table kernel, the keys kernel with and without the norm, the select chain, the code range
check and the stream's scratch must all sit on the caller's stream."""
import numpy as np

import aq_wide_oracle as awo
import norms_oracle as no
import stream_cases as sc


def _linscan_aq_wide(n, m, h, d, nq, K, lsq, kernel):
    def build():
        codes, C, queries, nrm = awo.case(n, m, h, d, nq, 51)
        bits, ids, _ = awo.scan(codes, C, queries, K, nrm if lsq else None)
        inputs = {"codes": codes, "codebooks": C, "queries": queries}
        if lsq:
            inputs["dbnorms"] = nrm

        def run(dev, out):
            dd, ii = sc._rqd().linscan_aq_wide(dev["codes"], dev["codebooks"], dev["queries"], K, dbnorms=dev.get("dbnorms"),
                                               out=(out["dists"], out["ids"]))
            return {"dists": dd, "ids": ii}

        def check(got):
            assert np.array_equal(got["ids"].view(np.uint32), ids), "ids differ"
            assert np.array_equal(got["dists"].view(np.uint32), bits), "distances differ"

        def after():
            ran = (sc._L().lib().rq_last_scan_kernel() or b"").decode()
            assert ran == kernel, (ran, kernel)

        return sc.Case("rq_dev_linscan_aq_wide", inputs, run, check, outputs=sc._scan_outputs(nq, K), after=after)
    return build


def _aq_lut_wide(m, h, d, nq, lsq):
    def build():
        _, C, queries, _ = awo.case(1, m, h, d, nq, 52)
        ref = awo.tables(lsq, C, queries).reshape(nq, m, h)

        def run(dev, out):
            return {"lut": sc._rqd().aq_lut_wide(dev["codebooks"], dev["queries"], lsq=lsq)}

        def check(got):
            assert sc._eq_bits(got["lut"], ref)

        return sc.Case("rq_dev_aq_lut_wide", {"codebooks": C, "queries": queries}, run, check)
    return build


def _aq_norms_wide(n, d, m, h):
    def build():
        codes, C, _, _ = awo.case(n, m, h, d, 1, 53)
        want = no.aq_norms(codes, C)

        def run(dev, out):
            return {"norms": sc._rqd().aq_norms_wide(dev["codes"], dev["C"], out=out["norms"])}

        def check(got):
            assert sc._eq_bits(got["norms"], want), "norms differ in %d rows" % int((got["norms"] != want).sum())

        return sc.Case("rq_dev_aq_norms_wide", {"codes": codes, "C": C}, run, check, outputs={"norms": ((n,), np.float32)})
    return build


def _quantize_norms_wide(hn):
    def build():
        rng = np.random.default_rng(54 + hn)
        norms = (rng.standard_normal(3_001) * 40 + 300).astype(np.float32)
        cb = rng.permutation(np.linspace(150, 450, hn)).astype(np.float32)
        want = awo.quantize(norms, cb)
        poison = {"norms": np.full_like(norms, 1e3), "cbnorms": np.arange(hn, dtype=np.float32)}

        def run(dev, out):
            codes, dbn = sc._rqd().quantize_norms_wide(dev["norms"], dev["cbnorms"], out=out["codes"], dbnorms=out["dbnorms"])
            return {"codes": codes, "dbnorms": dbn}

        def check(got):
            assert np.array_equal(got["codes"], want) and sc._eq_bits(got["dbnorms"], cb[want])

        return sc.Case("rq_dev_quantize_norms_wide", {"norms": norms, "cbnorms": cb}, run, check, poison=poison,
                       outputs={"codes": (want.shape, np.int16), "dbnorms": (want.shape, np.float32)})
    return build


# the norms entry synchronises the stream in its code range check at every h (int16 codes can always be out of range); the
# quantise cases sit on both sides of the 64 KiB of LDS a kernel gets without asking
AQ_WIDE_CASES = {
    "linscan_aq_wide_lsq_lds4": ("rq_dev_linscan_aq_wide",
                                 _linscan_aq_wide(20_001, 8, 1024, 8, 5, 100, True, "adc_keys_h16_kernel<4, true, true>")),
    "linscan_aq_wide_cq_global": ("rq_dev_linscan_aq_wide",
                                  _linscan_aq_wide(20_001, 8, 4097, 4, 5, 100, False, "adc_keys_h16_kernel<4, false>")),
    "aq_lut_wide_lsq_vec4": ("rq_dev_aq_lut_wide", _aq_lut_wide(4, 1000, 32, 17, True)),
    "aq_lut_wide_cq_scalar": ("rq_dev_aq_lut_wide", _aq_lut_wide(3, 257, 30, 7, False)),
    "aq_norms_wide_h1000": ("rq_dev_aq_norms_wide", _aq_norms_wide(5_003, 96, 8, 1000)),
    "aq_norms_wide_h256": ("rq_dev_aq_norms_wide", _aq_norms_wide(5_003, 130, 5, 256)),
    "quantize_norms_wide_hn1000": ("rq_dev_quantize_norms_wide", _quantize_norms_wide(1000)),
    "quantize_norms_wide_hn20000": ("rq_dev_quantize_norms_wide", _quantize_norms_wide(20_000)),
}
sc.CASES.update(AQ_WIDE_CASES)
sc.ENTRIES.update(entry for entry, _ in AQ_WIDE_CASES.values())
