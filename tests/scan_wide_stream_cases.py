"""The stream cases of the scan over 16-bit codes (rq_dev_linscan_wide, rq_dev_adc_lut_wide), registered with the harness of
tests/stream_cases.py exactly as tests/wide_stream_cases.py does -- a plain helper module: no fixtures, no pytest hooks.
tests/test_gpu_scan_wide.py and tests/test_scan_wide_oracle.py import it, so the table of tests/test_gpu_streams.py is complete
whenever the suite is collected as a whole.  Two cases per entry point, on different table placements: the table kernel, the
keys kernel, the select chain and the stream's scratch must all sit on the caller's stream."""
import numpy as np

import scan_wide_oracle as swo
import stream_cases as sc


def _data(n, m, h, sub, nq, seed):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((m, h, sub)).astype(np.float32)
    queries = rng.standard_normal((nq, m * sub)).astype(np.float32)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    return codes, centers, queries


def _linscan_wide(n, m, h, sub, nq, K, kernel):
    def build():
        codes, centers, queries = _data(n, m, h, sub, nq, 41)
        bits, ids, _ = swo.scan(sc._oracle(), codes, centers, queries, K)

        def run(dev, out):
            d, i = sc._rqd().linscan_wide(dev["codes"], dev["centers"], dev["queries"], K, out=(out["dists"], out["ids"]))
            return {"dists": d, "ids": i}

        def check(got):
            assert np.array_equal(got["ids"].view(np.uint32), ids), "ids differ"
            assert np.array_equal(got["dists"].view(np.uint32), bits), "distances differ"

        def after():
            ran = (sc._L().lib().rq_last_scan_kernel() or b"").decode()
            assert ran == kernel, (ran, kernel)

        return sc.Case("rq_dev_linscan_wide", {"codes": codes, "centers": centers, "queries": queries}, run, check,
                       outputs=sc._scan_outputs(nq, K), after=after)
    return build


def _adc_lut_wide(m, h, sub, nq):
    def build():
        _, centers, queries = _data(1, m, h, sub, nq, 42)
        ref = swo.tables(sc._oracle(), centers, queries)

        def run(dev, out):
            return {"lut": sc._rqd().adc_lut_wide(dev["centers"], dev["queries"])}

        def check(got):
            assert sc._eq_bits(got["lut"], ref)

        return sc.Case("rq_dev_adc_lut_wide", {"centers": centers, "queries": queries}, run, check)
    return build


SCAN_WIDE_CASES = {
    "linscan_wide_lds4": ("rq_dev_linscan_wide", _linscan_wide(20_001, 8, 1024, 2, 5, 100, "adc_keys_h16_kernel<4, true>")),
    "linscan_wide_global": ("rq_dev_linscan_wide", _linscan_wide(20_001, 16, 4096, 2, 5, 100, "adc_keys_h16_kernel<4, false>")),
    "adc_lut_wide_vec4": ("rq_dev_adc_lut_wide", _adc_lut_wide(4, 1000, 4, 7)),
    "adc_lut_wide_scalar": ("rq_dev_adc_lut_wide", _adc_lut_wide(3, 257, 6, 7)),
}
sc.CASES.update(SCAN_WIDE_CASES)
sc.ENTRIES.update(entry for entry, _ in SCAN_WIDE_CASES.values())
