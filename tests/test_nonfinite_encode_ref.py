"""CPU: the oracle side of the encode's non-finite contract (include/rayuela_hip.h, "Non-finite inputs")
on the very inputs tests/test_gpu_nonfinite_encode.py hands to the kernels (tests/nonfinite_encode_cases.py), so that the GPU
test's reference is itself under test where no GPU is: rows are independent (the oracle on the poisoned input equals the
oracle on the zeroed input on every finite cell), sub-quantizers are independent (a poisoned codeword moves its own column
only), a sub-vector that holds a NaN gets code 0, every code is below h, and the rotation of a poisoned row leaves the
finite rows alone."""
import numpy as np
import pytest

import nonfinite_encode_cases as nc

SHAPES = [(32, 4), (24, 4), (50, 7), (16, 8), (131, 1)]


@pytest.mark.parametrize("h", [16, 17, 27, 256])
@pytest.mark.parametrize("d,m", SHAPES)
def test_oracle_rows_are_independent_and_nan_gives_code_zero(oracle, d, m, h):
    c = nc.case(nc.N, d, m, h)
    assert int(c["excused"].sum()) == nc.excused_count(nc.N, d, m) and not c["excused"][c["clean"]].any()
    assert c["nan_cells"].any() and not (c["nan_cells"] & ~c["excused"]).any()
    bad = oracle.encode_pq(c["Xbad"], c["Ccat"], m, h)
    zero = oracle.encode_pq(c["Xzero"], c["Ccat"], m, h)
    fin = oracle.encode_pq(c["X"], c["Ccat"], m, h)
    assert bad.dtype == np.uint8 and int(bad.max()) < h and int(zero.max()) < h
    assert np.array_equal(bad[c["clean"]], zero[c["clean"]]) and np.array_equal(bad[c["clean"]], fin[c["clean"]])
    # the finite sub-vectors of a poisoned row are those of the finite input too: a poison stays in its sub-quantizer
    assert np.array_equal(bad[~c["excused"]], fin[~c["excused"]])
    assert (bad[c["nan_cells"]] == 0).all()
    assert (fin[c["nan_cells"]] != 0).any()                # (code 0 is the rule's doing, not the data's)


@pytest.mark.parametrize("kind", nc.CODEWORD_POISONS)
@pytest.mark.parametrize("h", [16, 17, 27, 256])
@pytest.mark.parametrize("d,m", [(32, 4), (50, 7)])
def test_oracle_sub_quantizers_are_independent(oracle, d, m, h, kind):
    c = nc.case(nc.N, d, m, h)
    _, Ccat, i = nc.poisoned_codebooks(c, kind, d, m, h)
    assert int((Ccat.view(np.uint32) != c["Ccat"].view(np.uint32)).sum()) == 1
    got = oracle.encode_pq(c["X"], Ccat, m, h)
    fin = oracle.encode_pq(c["X"], c["Ccat"], m, h)
    other = np.arange(m) != i
    assert int(got.max()) < h
    assert np.array_equal(got[:, other], fin[:, other])
    assert not np.array_equal(got[:, i], fin[:, i])        # (the poisoned codeword does take part in its own column)


@pytest.mark.parametrize("d", [10, 33, 96])
def test_oracle_rotation_keeps_a_poison_in_its_row(oracle, d):
    import rayuela_jl_amd.synth as synth
    n = 1013
    c = nc.case(n, d, 1, 16)
    R = synth.rotation(d, seed=d)
    bad, fin = oracle.rotate_T(R, c["Xbad"]), oracle.rotate_T(R, c["X"])
    assert np.array_equal(bad[c["clean"]].view(np.uint32), fin[c["clean"]].view(np.uint32))
    assert np.isfinite(fin).all()
    assert np.isnan(bad[64]).all() and np.isnan(bad[0]).all()      # NaN throughout; one NaN coordinate under a dense R
    assert np.isinf(bad[31]).all()                                 # one +Inf coordinate: +-Inf everywhere, no NaN
    # OPQ: a finite row keeps its codes
    m, h = (2, 17) if d % 2 == 0 else (3, 17)
    e = nc.case(n, d, m, h)
    codes_bad = oracle.encode_opq(e["Xbad"], R, e["Ccat"], m, h)
    codes_fin = oracle.encode_opq(e["X"], R, e["Ccat"], m, h)
    assert int(codes_bad.max()) < h and np.array_equal(codes_bad[e["clean"]], codes_fin[e["clean"]])
    assert (codes_bad[64] == 0).all()
