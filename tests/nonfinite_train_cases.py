"""The inputs and the CPU restatements of the non-finite contract of TRAINING (include/rayuela_hip.h, "Non-finite inputs of
training"), shared by tests/test_nonfinite_train_ref.py (CPU: the restatements against the existing
oracles) and tests/test_gpu_nonfinite_train.py (the kernels).  A plain helper module in the style of
tests/nonfinite_encode_cases.py: no fixtures, no pytest hooks, no library, no device.

A. Reductions.  One case = integer-valued rows (kmeans_oracle.int_data: everything finite is exact and bit-comparable) with ONE
   poisoned coordinate (row r, column c) -- or two rows poisoned in different columns of different sub-spaces.  The reductions
   are column-wise, so the poison may only reach column c:
     centre update   counts exact with the poisoned row counted; every column k != c bit-equal to train_wide_oracle.exact_means
                     of the rows with column c zeroed (`means`); a code without rows keeps its start bits in EVERY column.
                     What column c may hold was read in centers_mfma_kernel (rq_train.hip): the segment sum is a product with a
                     one-hot matrix A, D[code][col] = sum_row A[code][row] B[row][col]; a non-finite B[r][c] meets 0 x NaN in
                     every code of column c (of every block of 256 codes: all units read all rows) and in no other column -- an
                     idle lane's value is replaced by a select, not multiplied -- and the ones-column Bc that counts is a constant
                     that never sees X.  The owner-thread kernel (TRAIN_CENTERS_MFMA = 0) adds x only into its own row's code:
                     there the poison stays in ONE cell (code of row r, column c).
     reconstruct     a pure copy: non-finite and denormal entries of C arrive bit for bit.
   The excused cells of a case are counted from its poison table (`excused_cells`): the cells of the poisoned columns, h per
   column, so their share of C is (poisoned columns) / d -- 1 / d for a single poison, by the nature of a column, whatever the
   kernel; under the owner-thread kernel the excuse is the single cell and its share is 1 / (h d).
B. Training loops.  A Gaussian base with one poisoned row that is not a first seed, as the byte tests use; the mass-refill
   fixture (`refill_fixture`): integer rows of which all but a handful are identical, under a uniformly sampled start."""
import functools

import numpy as np

import kmeans_oracle as ko
import nonfinite_encode_cases as nc
import nonfinite_ref as nf
import train_wide_oracle as two
import wide_oracle as wo

F32 = nc.F32                                # nan_pos, nan_neg, pinf, ninf, 3e38
KINDS = tuple(F32)
SHAPES_WIDE = [(3001, 32, 4, 300), (1000, 10, 4, 257), (1500, 200, 2, 600)]
SHAPES_BYTE = [(3001, 32, 4, 256), (3001, 30, 5, 17)]
DENORMAL = 0x00000001


def slice_rows(n):
    """Rows of one row slice of the centre kernels at the sizes used here: one slice per 1024 rows (the other terms of the
    planners, compute units / code blocks and the 2^23-row and 2^30-byte caps, bind only far above n = 4129)."""
    g = (n + 1023) // 1024
    return (n + g - 1) // g


def tail_row(n):
    """A row in the ragged tail of slice 0: past its last full pair of 32-row steps."""
    rp = slice_rows(n)
    full = rp // 64 * 64
    assert full < rp
    return full + (rp - full) // 2


def poison_table(n, d, m):
    """-> list of cases, a case = list of (row, column, kind).  Seven single poisons -- rows 0, 31, 32, 63, 64, the ragged tail
    of a slice, the last row; the five kinds in turn; columns at the first, last and inner dimensions of the sub-spaces -- and one
    case of two rows poisoned in different columns of different sub-spaces."""
    off = wo.splitarray(d, m)
    rows = [0, 31, 32, 63, 64, tail_row(n), n - 1]
    cols = [0, d - 1, off[1], off[1] - 1, d // 2, min(1, d - 1), off[m - 1]]
    table = [[(r, c, KINDS[i % len(KINDS)])] for i, (r, c) in enumerate(zip(rows, cols))]
    table.append([(31, off[1] - 1, "pinf"), (64, off[m - 1], "nan_neg")])
    return table


def sub_of(d, m):
    return np.repeat(np.arange(m), np.diff(wo.splitarray(d, m)))


def excused_cells(case, d, m, h):
    """What the excuse adds up to, from the poison table alone: h cells per distinct poisoned column."""
    return h * len({c for _, c, _ in case})


@functools.lru_cache(maxsize=None)
def centre_case(n, d, m, h):
    """-> dict X (finite, integer-valued), codes (n, m) int64 zero-based with (at least) two codes per sub-quantizer left without
    rows, C0 (list of start centres), empty (those two codes); read-only, computed once and shared."""
    rng = np.random.default_rng(n + 7 * d + 11 * m + h)
    X = ko.int_data(n, d, 7 + h)
    empty = (3, h - 2)
    codes = rng.integers(0, h, (n, m))
    for k in empty:
        codes[codes == k] = k + 1
    codes[200:200 + m, :] = h - 1                # the last code (h = 257: the one code of the last block) has rows
    off = wo.splitarray(d, m)
    C0 = [(rng.standard_normal((h, off[i + 1] - off[i])) * 20).astype(np.float32) for i in range(m)]
    for a in [X, codes] + C0:
        a.setflags(write=False)
    return dict(X=X, codes=codes, C0=C0, empty=empty, off=off)


def poisoned(X, case):
    Xbad = np.array(X, copy=True)
    for r, c, kind in case:
        nf.put_bits(Xbad, (r, c), F32[kind])
    return Xbad


def zeroed(X, case):
    Xz = np.array(X, copy=True)
    for _, c, _ in case:
        Xz[:, c] = 0.0
    return Xz


def means(c, case, m, h):
    """(C list, counts (m, h)): the exact restatement on the rows with the poisoned columns zeroed.  Outside those columns it IS
    the restatement of the poisoned input (the sums are column-wise); inside them it is no claim."""
    return two.exact_means(zeroed(c["X"], case), c["C0"], c["codes"], m, h)


def keep_mask(case, d):
    """(d,) bool: the columns held to the restatement."""
    keep = np.ones(d, dtype=bool)
    for _, col, _ in case:
        keep[col] = False
    return keep


def poisoned_codebooks(C, d, m, h):
    """A copy of the centres with NaN (both signs), +-Inf and denormal entries: (C list, [(sub-quantizer, code, column)])."""
    out = [np.array(b, copy=True) for b in C]
    w = [b.shape[1] for b in out]
    cells = [(0, 0, 0, nf.NAN_POS), (0, h - 1, w[0] - 1, nf.NAN_NEG), (m - 1, min(256, h - 1), 0, F32["pinf"]),
             (m - 1, 5, w[m - 1] // 2, F32["ninf"]), (m // 2, 7, 0, DENORMAL), (m // 2, h - 1, w[m // 2] - 1, DENORMAL | 0x80000000)]
    for i, k, s, bits in cells:
        nf.put_bits(out[i], (k, s), bits)
    return out, [(i, k, s) for i, k, s, _ in cells]


# ---- B. training loops ----------------------------------------------------------------------------------------------------------
NT = 3000
TRAIN_POISONS = {"nan": nf.NAN_POS, "pinf": 0x7F800000, "2e19": int(np.array([2e19], dtype=np.float32).view(np.uint32)[0])}
TRAIN_SEED = 5


def first_seeds(n, m, h, seed, salt):
    """The first kmeans++ seed of every sub-space (kmeans_oracle.kmpp_seeds: the m * h uniforms are drawn first, sub-space
    major; the first seed of sub-space i is floor(u[i][0] * n)) -- drawn before any cost exists, so from the stream alone."""
    rng = ko.Rng(seed, salt)
    u = [[rng.uniform() for _ in range(h)] for _ in range(m)]
    return [min(int(u[i][0] * n), n - 1) for i in range(m)]


@functools.lru_cache(maxsize=None)
def train_base(d):
    X = np.random.default_rng(40 + d).standard_normal((NT, d)).astype(np.float32)
    X.setflags(write=False)
    return X


def poisoned_base(d, m, h, poison):
    """(X, row): one row that is no first seed under any of the three salts, poisoned in coordinate 1 (the magnitude 2e19:
    throughout, |x|^2 ~ 1e40)."""
    avoid = set()
    for salt in (ko.SALT_PQ, ko.SALT_OPQ, ko.SALT_RVQ):
        avoid |= set(first_seeds(NT, m, h, TRAIN_SEED, salt)) | set(first_seeds(NT, 1, h, TRAIN_SEED, salt))
    X = np.array(train_base(d), copy=True)
    row = next(r for r in range(NT // 2, NT) if r not in avoid)
    if poison == "2e19":
        X[row] = 2e19
    else:
        nf.put_bits(X, (row, 1), TRAIN_POISONS[poison])
    return X, row


REFILL = dict(n=900, d=4, m=1, h=300, seed=2, heavy=860)


def refill_fixture():
    """860 copies of one integer point and 40 scattered integer rows, permuted; h = 300 centres from a uniformly sampled start
    (TRAIN_KMPP = 0): most start rows are copies of the one point, the first of them keeps every copy and all the later ones
    empty in iteration 1 -- the mass refill.  The scattered rows that were not sampled leave cost, so the first re-draws are
    cost-proportional and the rest, once every distinct row is a centre, uniform."""
    f = REFILL
    X = ko.crowded(n=f["n"], d=f["d"], seed=9, heavy=f["heavy"], npts=1)
    X.setflags(write=False)
    return X, f["m"], f["h"], f["seed"]


def refill_fixture_nan(row=450):
    X = np.array(refill_fixture()[0], copy=True)
    nf.put_bits(X, (row, 1), nf.NAN_POS)
    return X


# ---- B.4 the wide encode at the shapes its one non-finite test does not reach ------------------------------------------------------
WIDE_ENCODE_SHAPES = [(1000, 10, 4, 257), (1000, 80, 2, 300)]


def wide_encode_case(n, d, m, h):
    """(X, Ccat): SIFT-like rows with NaN / Inf coordinates at rows 3, 10, 20, 40, n - 1 (the existing test's rows) and, per
    shape, a codeword poison: h = 257 -- the single live codeword of the second block holds +Inf (a block of one live and 255
    padded codewords, none of which may be named); d = 80 -- a NaN row coordinate and an Inf codeword entry in the LAST of the
    three k-chunks of a 40-wide sub-space."""
    import rayuela_jl_amd.synth as synth
    X = np.array(synth.sift_like(n, d, seed=n + d + m + h))
    rng = np.random.default_rng(h + d)
    off = wo.splitarray(d, m)
    C = [np.array(X[rng.integers(0, n, h), off[i]:off[i + 1]]) for i in range(m)]
    X[3, min(5, d - 1)] = np.nan
    X[10, 0] = np.inf
    X[20, d - 1] = -np.inf
    X[40, off[1]:off[1] + min(8, off[2] - off[1])] = np.inf
    X[n - 1, d // 2 + 1] = np.nan
    if h == 257:
        C[1][256, 0] = np.inf
        C[2][256, :] = X[7, off[2]:off[3]]                  # and a live last codeword that wins a row
    else:
        X[50, off[1] - 1] = np.nan                          # column 39: the third k-chunk of sub-space 0
        C[1][270, off[2] - off[1] - 2] = np.inf
        C[0][299, 35] = -np.inf
    return X, two.cat(C)


# ---- A.3 - A.5 the LSQ / chain normal equations and solves, the SR standard deviation --------------------------------------------
# What was read (rq_lsq.hip, rq_chain.hip, rq_sr.hip): b is a SEGMENTED sum (lsq_bsum_kernel: one thread per (segment, column),
# rows in ascending order), so a poison reaches the cells (i h + code_i(r), c) of b and nothing else, and A never sees X.  The SPD
# solve keeps right-hand-side columns apart: lsq_trsv_block_kernel gives a thread one column, lsq_gemm_sub_kernel forms
# D(i, j) -= sum_k P(i, k) Q(j, k) with j the column (padded columns are selected to 0, not multiplied).  No coupled tiles: the
# confinement is the single column c, for the chain update too (its blocks gather column ranges of the same b).  The standard
# deviation and the perturbation are per column / per element.
LSQ_N, LSQ_D = 4001, 24
LSQ_SHAPES = [(4, 16), (4, 256), (8, 16), (8, 256)]              # (m, h)
LSQ_CASES = (0, 3, 4, 5, 7)                                      # rows of poison_table: nan_pos, ninf, 3e38, the slice tail, two rows
SR_ROWS = 1024


@functools.lru_cache(maxsize=None)
def lsq_case(m, h, d=LSQ_D, n=LSQ_N):
    rng = np.random.default_rng(1000 * m + h + d)
    X = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    X.setflags(write=False)
    codes.setflags(write=False)
    return X, codes


def lsq_poisons(d, m, n=LSQ_N):
    table = poison_table(n, d, m)
    return [table[i] for i in LSQ_CASES]


def sr_sigma(X, div=1.0):
    """rq_sr_std restated operation by operation (sr_colsum_kernel / sr_colfinish_kernel, contraction off): per block of 1024
    rows four interleaved f64 chains (rows g, g + 4, ...), combined (0 + 1) + (2 + 3), the blocks added in ascending order; the
    mean first, then the squared deviations from it; sigma = (float)((double)(float)sqrt(s / (n - 1)) / div)."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    n, d = X64.shape

    def colsum(vals):
        s = np.zeros(d)
        for r0 in range(0, n, SR_ROWS):
            blk = vals[r0:r0 + SR_ROWS]
            red = []
            for g in range(4):
                acc = np.zeros(d)
                for r in range(g, blk.shape[0], 4):
                    acc = acc + blk[r]
                red.append(acc)
            s = s + ((red[0] + red[1]) + (red[2] + red[3]))
        return s
    with np.errstate(all="ignore"):
        mean = colsum(X64) / float(n)
        df = X64 - mean[None, :]
        s = colsum(df * df)
        return (np.sqrt(s / float(n - 1)).astype(np.float32).astype(np.float64) / div).astype(np.float32)


def train_aq_case(m, h, poison, n=NT, d=LSQ_D):
    """(X finite, Xbad, codes0): Gaussian rows, random start codes, row 1700 poisoned as in poisoned_base."""
    rng = np.random.default_rng(77 + m + h)
    X = rng.standard_normal((n, d)).astype(np.float32)
    codes0 = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    Xbad = X.copy()
    if poison == "2e19":
        Xbad[1700] = 2e19
    else:
        nf.put_bits(Xbad, (1700, 1), TRAIN_POISONS[poison])
    return X, Xbad, codes0
