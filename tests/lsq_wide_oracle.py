"""CPU restatement of the LSQ codebook update contract over int16 codes: the contract of
tests/lsq_update_oracle.py word for word for codes in code_base .. code_base + h - 1 and 2 <= h <= 32767, plus the rows per
(codebook, code).  Plain numpy; A is optional, so b and the counts can be restated at h = 32767 without an (mh, mh) matrix."""
import numpy as np

from lsq_update_oracle import qerror, reconstruct, solve  # noqa: F401  (the yardsticks do not depend on the code width)

MAX_H16 = 32767


def _codes(codes, h, code_base):
    codes = np.asarray(codes)
    assert codes.dtype == np.int16 and codes.ndim == 2, "codes are (n, m) int16"
    assert 2 <= h <= MAX_H16 and code_base in (0, 1)
    c = codes.astype(np.int64) - code_base
    assert c.size == 0 or (c.min() >= 0 and c.max() <= h - 1), "a code outside code_base .. code_base + h - 1"
    return c


def counts(codes, h, code_base=0):
    """(m, h) uint32: the rows of every (codebook, code) segment."""
    c = _codes(codes, h, code_base)
    return np.stack([np.bincount(c[:, i], minlength=h) for i in range(c.shape[1])]).astype(np.uint32)


def normal_eq(X, codes, h, rho=1e-4, code_base=0, with_A=True):
    """X (n, d) f32, codes (n, m) int16 -> (A (mh, mh) f64 or None, b (mh, d) f64, counts (m, h) u32), bit for bit the device's.
    A = B'B + rho I from exact integer counts; b[(i, a), k] = the f64 sum from +0 of (double) X[r, k] over the rows with code a in
    codebook i, in ascending row order."""
    X = np.asarray(X, dtype=np.float32)
    c = _codes(codes, h, code_base)
    n, d = X.shape
    m = c.shape[1]
    mh = m * h
    cnt = counts(codes, h, code_base)
    A = None
    if with_A:
        A = np.zeros((mh, mh))
        for i in range(m):
            idx = i * h + np.arange(h)
            A[idx, idx] = cnt[i].astype(np.float64) + rho
            for j in range(i + 1, m):
                pc = np.zeros((h, h), np.int64)
                np.add.at(pc, (c[:, i], c[:, j]), 1)
                A[i * h:(i + 1) * h, j * h:(j + 1) * h] = pc
                A[j * h:(j + 1) * h, i * h:(i + 1) * h] = pc.T
    b = np.zeros((mh, d))
    X64 = X.astype(np.float64)
    for i in range(m):
        np.add.at(b, c[:, i] + i * h, X64)          # unbuffered, one row after the other: ascending row order
    return A, b, cnt


def update(X, codes, h, rho=1e-4, code_base=0):
    """-> (C (m, h, d) f32, C64 (mh, d)) through numpy's f64 solve"""
    A, b, _ = normal_eq(X, codes, h, rho, code_base)
    C64 = solve(A, b)
    return C64.astype(np.float32).reshape(np.asarray(codes).shape[1], h, -1), C64


def update_one_codebook(X, codes, h, rho=1e-4, code_base=0):
    """m = 1: A is diagonal, so C64 = b / (count + rho) entry by entry in f64 -- no solve, at any h."""
    assert np.asarray(codes).shape[1] == 1
    _, b, cnt = normal_eq(X, codes, h, rho, code_base, with_A=False)
    C64 = b / (cnt[0].astype(np.float64) + rho)[:, None]
    return C64.astype(np.float32).reshape(1, h, -1), C64


def sort_scratch_bytes(n, m, h):
    """What rq_lsq_wide_plan reports as the sort scratch: tile histograms (256 key values at most), the segment bounds, the per-code
    counts and one row list per pass (two passes past 256 codewords), the small tables rounded up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256                        # noqa: E731
    tiles = max(1, -(-n // 4096))
    wide = h > 256
    return m * min(h, 256) * tiles * 4 + up(m * (h + 1) * 4) + (up(m * h * 4) if wide else 0) + m * n * 4 * (2 if wide else 1)
