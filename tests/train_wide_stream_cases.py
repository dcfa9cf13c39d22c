"""The stream cases of the training reductions over 16-bit codes (rq_dev_update_centers_wide, rq_dev_reconstruct_wide),
registered with the harness of tests/stream_cases.py exactly as tests/wide_stream_cases.py and tests/scan_wide_stream_cases.py
do -- a plain helper module: no fixtures, no pytest hooks.  tests/test_gpu_train_wide.py and tests/test_train_wide_oracle.py
import it, so the table of tests/test_gpu_streams.py is complete whenever the suite is collected as a whole.  h = 600: three
code blocks, the last one ragged; several row slices, so the reduction of the partial sums and its scratch must sit on the
caller's stream as well."""
import functools

import numpy as np

import kmeans_oracle as ko
import stream_cases as sc
import train_wide_oracle as two
import wide_oracle as wo


@functools.lru_cache(maxsize=None)
def _setup():
    n, d, m, h = 9_001, 40, 4, 600
    X = ko.int_data(n, d, 91)
    rng = np.random.default_rng(17)
    codes = rng.integers(0, h, (n, m)).astype(np.int16)
    off = wo.splitarray(d, m)
    Cs = [rng.standard_normal((h, off[q + 1] - off[q])).astype(np.float32) * 20 for q in range(m)]
    Cn, counts = two.exact_means(X, Cs, codes, m, h)
    return dict(n=n, d=d, m=m, h=h, X=X, codes=codes, Ccat=two.cat(Cs), Cn=two.cat(Cn), counts=counts,
                CB=two.reconstruct(Cs, codes, off, d))


def _update_centers_wide():
    s = _setup()
    m, h = s["m"], s["h"]

    def run(dev, out):
        counts = sc._rqd().update_centers_wide(dev["C"], dev["X"], dev["codes"], m, h)
        return {"C": dev["C"], "counts": counts}

    def check(got):
        assert sc._eq_bits(got["C"], s["Cn"])              # integer rows: exact whatever the tree
        assert np.array_equal(got["counts"], s["counts"])

    return sc.Case("rq_dev_update_centers_wide", {"C": s["Ccat"], "X": s["X"], "codes": s["codes"]}, run, check)


def _reconstruct_wide():
    s = _setup()

    def run(dev, out):
        return {"CB": sc._rqd().reconstruct_wide(dev["codes"], dev["C"], s["d"], s["h"], out=out["CB"])}

    def check(got):
        assert sc._eq_bits(got["CB"], s["CB"])

    return sc.Case("rq_dev_reconstruct_wide", {"codes": s["codes"], "C": s["Ccat"]}, run, check,
                   outputs={"CB": ((s["n"], s["d"]), np.float32)})


TRAIN_WIDE_CASES = {
    "update_centers_wide": ("rq_dev_update_centers_wide", _update_centers_wide),
    "reconstruct_wide": ("rq_dev_reconstruct_wide", _reconstruct_wide),
}
sc.CASES.update(TRAIN_WIDE_CASES)
sc.ENTRIES.update(entry for entry, _ in TRAIN_WIDE_CASES.values())
