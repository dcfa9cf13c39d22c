"""CPU: the numpy restatement of the beam encoding contract (tests/beam_oracle.py) against the oracle's greedy RVQ encoder, a
float64 transcription of src/CompetitiveQ.jl:75-135, a quality check and the tie fixture."""
import numpy as np
import pytest

import beam_oracle as bo
import beam_stream_cases  # noqa: F401  (completes the table that tests/test_gpu_streams.py checks against the header)


# ---- (a) a beam of one is the greedy encoder ------------------------------------------------------------------------------------
# tests/test_gpu_rvq.py's random cases with that file's n, except its 20 000-row case, run on its first 5 000 rows: the
# restatement sorts n * h values per stage, the property is per row, and every (d, m, h) of that file is here
@pytest.mark.parametrize("n,d,m,h,kind", [(min(s[0], 5_000),) + s[1:] for s in bo.RVQ_SHAPES])
def test_beam_of_one_equals_the_rvq_oracle(oracle, n, d, m, h, kind):
    X, C = bo.data(n, d, m, h, kind)
    c0, _, r0 = oracle.encode_rvq(X, C, with_extras=True)
    c1, r1, _ = bo.encode(X, C, 1)
    assert np.array_equal(c0, c1)
    assert np.array_equal(r0.view(np.uint32), r1.view(np.uint32))


# ---- (b) the reference, transcribed in float64 ------------------------------------------------------------------------------------
def reference_encode_f64(x, C, m, h, d, H):
    """src/CompetitiveQ.jl:75-135 line by line for one vector, zero-based: explicit residual matrices (here [h][d], the memory
    image of Julia's d x h), sums of squares, a stable sort, and the new_bs bookkeeping."""
    xrs = x[None, :] - C[0]                                    # :87   all h residuals
    qerrs = (xrs ** 2).sum(axis=1)                             # :88
    sort_idx = np.argsort(qerrs, kind="stable")[:H]            # :89   sortperm is stable
    xrs = xrs[sort_idx]                                        # :90
    new_bs = np.zeros((H * h, m), dtype=np.int16)              # :97
    for i in range(H):                                         # :99-101
        new_bs[i * h:(i + 1) * h, 0] = sort_idx[i]
    for i in range(1, m):                                      # :103
        Ci = C[i]
        new_res, new_qerrs = [], []
        for j in range(H):                                     # :108-114
            new_res.append(xrs[j][None, :] - Ci)
            new_qerrs.append((new_res[j] ** 2).sum(axis=1))
            new_bs[j * h:(j + 1) * h, i] = np.arange(h)
        all_qerrs = np.concatenate(new_qerrs)                  # :117
        sort_idx = np.argsort(all_qerrs, kind="stable")[:H]    # :118
        all_res = np.concatenate(new_res, axis=0)              # :120
        xrs = all_res[sort_idx]                                # :121
        top_bs = new_bs[sort_idx, :i + 1].copy()               # :122
        for j in range(H):                                     # :125-129
            new_bs[j * h:(j + 1) * h, :i + 1] = top_bs[j]
    return new_bs[0], xrs[0]                                   # :133


# synth.deep_like rows with one Lloyd step per stage (tests/test_gpu_rvq.py's generator), at most 600 rows: the transcription is
# a per-vector loop.  The d = 8 input is low-dimensional, where a wider beam gains most.  synth.sift_like does not stay within
# the cap for the restatement alone: its rows are small integers with repeated points, so candidates tie EXACTLY in float64 and
# the f32 roundings of the contract order them otherwise (1 of 600 rows at d = 30, 17 of 400 at d = 32, already at H = 1, where
# the restatement is the RVQ oracle bit for bit); those inputs are left to the bit-parity tests.
F64_INPUTS = [(600, 64, 5, 77, "deep"), (600, 30, 3, 64, "deep"), (33, 16, 2, 16, "deep"), (600, 8, 4, 16, "deep"),
              (400, 32, 4, 64, "deep")]


@pytest.mark.parametrize("n,d,m,h,kind", F64_INPUTS)
def test_contract_agrees_with_the_float64_transcription(n, d, m, h, kind):
    X, C = bo.data(n, d, m, h, kind)
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    for H in (1, 2, 16):
        codes, Xr, _ = bo.encode(X, C, H)
        ref = [reference_encode_f64(X64[r], C64, m, h, d, H) for r in range(n)]
        ref_codes = np.stack([b for b, _ in ref])
        differ = int((ref_codes != codes).any(axis=1).sum())
        e_ref = float(np.mean([(r ** 2).sum() for _, r in ref]))
        e_f32 = float((Xr.astype(np.float64) ** 2).sum(axis=1).mean())
        print("n=%d d=%d m=%d h=%d H=%d: %d rows differ, mean error %.9g (f64 reference) vs %.9g" % (n, d, m, h, H, differ, e_ref, e_f32))
        assert differ <= 1e-3 * n
        assert abs(e_ref - e_f32) <= 1e-6 * e_ref


# ---- (c) a wider beam gives better codes --------------------------------------------------------------------------------------
def test_wider_beam_lowers_the_error():
    X, C = bo.data(2_000, 8, 4, 16, "deep")
    e = {H: bo.qerror(X, C, bo.encode(X, C, H)[0]) for H in (1, 2, 16)}
    print(e)
    assert e[16] < e[1]
    X, C = bo.data(*bo.GPU_SHAPES[0])
    assert bo.qerror(X, C, bo.encode(X, C, 16)[0]) < bo.qerror(X, C, bo.encode(X, C, 1)[0])


# ---- (d) the tie fixture puts ties on the boundary of the beam -----------------------------------------------------------------------
@pytest.mark.parametrize("H", bo.BEAMS)
def test_tie_fixture_has_ties_at_the_beam_boundary(H):
    X, C = bo.tie_fixture()
    for i in range(1, C.shape[0]):
        assert np.array_equal(C[i][9], C[i][5]) and not C[i][20].any() and not C[i][40].any()
    share = bo.boundary_tie_share(X, C, H)
    print("H = %d: %.1f %% of the rows have equal values at ranks H and H + 1 in some stage" % (H, 100 * share))
    assert share >= 0.10


def test_restatement_by_hand():
    """Two stages, two codewords, a beam of two, values small enough to check on paper: the greedy choice of stage 0 is not the
    best pair, and an exact tie is broken by j * h + k."""
    from oracle import oracle
    oracle.lib()
    X = np.array([[1.0, 0.0]], dtype=np.float32)
    C = np.array([[[0.75, 0.0], [1.5, 0.0]], [[0.5, 0.0], [-0.5, 0.0]]], dtype=np.float32)
    # stage 0: v = (0.0625, 0.25) -> greedy keeps codeword 0 (residual 0.25), the beam keeps both (0.25, -0.5)
    # stage 1: parent 0: (0.0625, 0.5625); parent 1: (1, 0) -> best is (parent 1, codeword 1) with residual 0
    c1, r1, v1 = bo.encode(X, C, 1)
    assert c1.tolist() == [[0, 0]] and r1.tolist() == [[-0.25, 0.0]] and v1.tolist() == [0.0625]
    c2, r2, v2 = bo.encode(X, C, 2)
    assert c2.tolist() == [[1, 1]] and r2.tolist() == [[0.0, 0.0]] and v2.tolist() == [0.0]
    # a tie: both codewords of stage 1 equal -> the lower index wins
    C[1][1] = C[1][0]
    assert bo.encode(X, C, 2)[0].tolist() == [[0, 0]]
