"""The inputs of the non-finite contract of the PQ / OPQ encode at h <= 256 (include/rayuela_hip.h, "Non-finite inputs";
DESIGN.md section 2), shared by tests/test_nonfinite_encode_ref.py (CPU: the oracle side) and
tests/test_gpu_nonfinite_encode.py (the kernels).  A plain helper module, imported by the tests (not a conftest).

One case = finite random rows and codebooks, then
  * ROW poisons: rows of X that carry a non-finite (or overflowing) coordinate -- `Xbad`; `Xzero` holds zeros in those rows
    instead.  Every other coordinate of a poisoned row keeps its finite value, so the row's other sub-vectors stay comparable;
  * CODEWORD poisons: one entry of one sub-codebook made Inf or NaN.
`excused` marks the only cells a kernel may answer differently from the oracle (in range, otherwise unspecified); `nan_cells`
the sub-vectors that hold a NaN coordinate, whose every distance is NaN and whose code is 0 by contract point 4."""
import functools

import numpy as np

import nonfinite_ref as nf

F32 = {"nan_pos": nf.NAN_POS, "nan_neg": nf.NAN_NEG, "pinf": 0x7F800000, "ninf": 0xFF800000,
       "3e38": int(np.array([3e38], dtype=np.float32).view(np.uint32)[0])}         # finite; its square overflows
N = 4129                                   # past one 4096-row chunk of the filter; 129 tiles of 32 rows and one row more


def widths(d, m):
    per, extra = divmod(d, m)              # src/utils.jl:179-203 (splitarray)
    return [per + (1 if i < extra else 0) for i in range(m)]


def row_poisons(n, d):
    """row -> [(kind, column), ...]: first and last row, the half-wave and tile edges 31 / 32 / 63 / 64, a row past the first
    4096-row chunk, and the single row of the ragged last tile (n = 4129: the last row)."""
    run = min(8, d)
    return {
        0: [("nan_pos", min(1, d - 1))],
        31: [("pinf", 0)],
        32: [("ninf", d - 1)],
        63: [("nan_neg", d // 2)],
        64: [("nan_pos", c) for c in range(d)],              # NaN throughout
        min(2000, n // 2): [("3e38", min(3, d - 1))],
        n - 32: [("pinf", c) for c in range(run)],            # 8 consecutive Inf coordinates (row 4097 at n = 4129)
        n - 1: [("nan_pos", d - 1)],
    }


CODEWORD_POISONS = ("cw_first_tile", "cw_last_tile", "cw_zero")


def codeword_poison(kind, d, m, h):
    """-> (sub-quantizer, codeword, column inside the sub-space, bit pattern)"""
    w = widths(d, m)
    i = 1 if m > 1 else 0
    if kind == "cw_first_tile":
        return i, min(3, h - 1), 0, F32["pinf"]
    if kind == "cw_last_tile":             # the last codeword: in a partially padded tile whenever h % 32 != 0
        return i, h - 1, w[i] - 1, F32["nan_neg"]
    assert kind == "cw_zero"
    return m - 1, 0, w[m - 1] // 2, F32["ninf"]


@functools.lru_cache(maxsize=None)
def case(n, d, m, h, seed=0):
    """-> dict: X (finite), Xbad, Xzero, C (list of (h, sub_i)), Ccat, clean (n,) bool, excused (n, m) bool, nan_cells (n, m) bool;
    every array read-only, computed once and shared."""
    rng = np.random.default_rng(1000 * d + 10 * m + h + seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    w = widths(d, m)
    C = [(rng.standard_normal((h, s)) * 0.7).astype(np.float32) for s in w]
    off = np.concatenate([[0], np.cumsum(w)])
    sub_of = np.repeat(np.arange(m), w)
    Xbad, Xzero = X.copy(), X.copy()
    clean = np.ones(n, bool)
    excused = np.zeros((n, m), bool)
    nan_cells = np.zeros((n, m), bool)
    for row, entries in row_poisons(n, d).items():
        clean[row] = False
        Xzero[row] = 0.0
        for kind, col in entries:
            nf.put_bits(Xbad, (row, col), F32[kind])
            excused[row, sub_of[col]] = True
            if kind.startswith("nan"):
                nan_cells[row, sub_of[col]] = True
    Ccat = np.concatenate([c.reshape(-1) for c in C])
    out = dict(X=X, Xbad=Xbad, Xzero=Xzero, C=C, Ccat=Ccat, clean=clean, excused=excused, nan_cells=nan_cells, off=off)
    for a in list(out.values()) + C:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def excused_count(n, d, m):
    """What `excused` must add up to, counted from row_poisons alone: the distinct (row, sub-quantizer) pairs it touches."""
    sub_of = np.repeat(np.arange(m), widths(d, m))
    return len({(row, int(sub_of[col])) for row, entries in row_poisons(n, d).items() for _, col in entries})


def poisoned_codebooks(c, kind, d, m, h):
    """-> (C list, Ccat, sub-quantizer whose column is excused) with one codeword entry poisoned"""
    i, k, col, bits = codeword_poison(kind, d, m, h)
    C = [np.array(b, copy=True) for b in c["C"]]
    nf.put_bits(C[i], (k, col), bits)
    return C, np.concatenate([b.reshape(-1) for b in C]), i
