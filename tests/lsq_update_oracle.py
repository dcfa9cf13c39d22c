"""CPU restatement of the LSQ codebook update contract (src/codebook_update.jl:96-206):
A = B'B + rho I from integer bincounts, b = B'X summed in f64 in ascending row order, C = (float) solve(A, b)."""
import numpy as np


def normal_eq(X, codes, h, rho=1e-4):
    """X (n, d) f32, codes (n, m) zero-based -> (A (mh, mh) f64, b (mh, d) f64), bit for bit the device's."""
    X = np.asarray(X, dtype=np.float32)
    codes = np.asarray(codes).astype(np.int64)
    n, d = X.shape
    m = codes.shape[1]
    mh = m * h
    A = np.zeros((mh, mh))
    for i in range(m):
        idx = i * h + np.arange(h)
        A[idx, idx] = np.bincount(codes[:, i], minlength=h).astype(np.float64) + rho
        for j in range(i + 1, m):
            pc = np.bincount(codes[:, i] * h + codes[:, j], minlength=h * h).reshape(h, h).astype(np.float64)
            A[i * h:(i + 1) * h, j * h:(j + 1) * h] = pc
            A[j * h:(j + 1) * h, i * h:(i + 1) * h] = pc.T
    b = np.zeros((mh, d))
    X64 = X.astype(np.float64)
    for i in range(m):
        np.add.at(b, codes[:, i] + i * h, X64)     # unbuffered, one row after the other: ascending row order
    return A, b


def solve(A, b):
    """numpy's LAPACK solve in f64 (the reference's getrf / getrs)."""
    return np.linalg.solve(A, b)


def update(X, codes, h, rho=1e-4):
    """-> (C (m, h, d) f32, C64 (mh, d))"""
    A, b = normal_eq(X, codes, h, rho)
    C64 = solve(A, b)
    m = np.asarray(codes).shape[1]
    return C64.astype(np.float32).reshape(m, h, -1), C64


def reconstruct(C, codes):
    """sum_i C_i[b_ri] in f64, (n, d)"""
    C = np.asarray(C, dtype=np.float64)
    codes = np.asarray(codes).astype(np.int64)
    return C[np.arange(C.shape[0])[None, :], codes].sum(axis=1)


def qerror(X, C, codes):
    return float(np.mean(((reconstruct(C, codes) - np.asarray(X, np.float64)) ** 2).sum(axis=1)))
