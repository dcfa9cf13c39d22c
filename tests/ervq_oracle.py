"""numpy restatements of train_ervq (src/ERVQ.jl:51-135) for the tests: no library, no device.

`literal` follows the reference line by line (Xd built in f32 with reconstruct's order, the means of
Clustering.update_centers! taken in f64); `incremental` is the library's formulation (the entry plus the mean of the full
residual over its rows) with a selectable accumulation type.  Stage encodes go through `encode`, the oracle's RVQ encode
(oracle.encode_rvq), so codes of the two restatements and of the library are comparable bit for bit.

Layouts: X (n, d) f32, codes (n, m) uint8 zero-based, C (m, h, d) f32.  Entries without rows keep their value in both
restatements (the refill draws from an RNG; the fixtures that compare traces have none)."""
import numpy as np

from rayuela_jl_amd import synth

# The fixture of the restatement and improvement tests (tests/test_ervq_oracle.py shows on the CPU that it improves)
FIX_N, FIX_D, FIX_M, FIX_H, FIX_NITER = 12000, 32, 4, 32, 3


def fixture(encode, n=FIX_N, d=FIX_D, m=FIX_M, h=FIX_H, seed=41):
    """X, start codes and start codebooks: an RVQ built on the CPU (synth.rvq_codebooks) and its encode."""
    X = synth.sift_like(n, d, seed=seed)
    C = synth.rvq_codebooks(X, m, h, seed=seed + 1)
    return X, encode(X, C), C


def qerror(X, codes, C):
    """qerror(X, B, C) (src/qerrors.jl) in f64."""
    rec = np.zeros(X.shape, dtype=np.float64)
    for i in range(C.shape[0]):
        rec += C[i].astype(np.float64)[codes[:, i]]
    return float(((X.astype(np.float64) - rec) ** 2).sum() / X.shape[0])


def class_sums(V, idx, h, acc):
    """sums (h, d) of the rows of V per class in ascending row order, accumulated in `acc`; counts (h,)."""
    sums = np.zeros((h, V.shape[1]), dtype=acc)
    np.add.at(sums, idx, V.astype(acc))
    return sums, np.bincount(idx, minlength=h)


def literal_xd(X, codes, C, j):
    """Xd of step j (src/ERVQ.jl:73-83), f32: Xr = X minus the stages before j - 1 one at a time (:114), then minus
    reconstruct of stage j - 1 and the stages after j (qerrors.jl:6-25: summed in codebook order from zero)."""
    m = C.shape[0]
    Xr = X.astype(np.float32, copy=True)
    for i in range(j - 1):
        Xr -= C[i][codes[:, i]]
    rec = np.zeros_like(Xr)
    for i in ([j - 1] if j >= 1 else []) + list(range(j + 1, m)):
        rec += C[i][codes[:, i]]
    return Xr - rec


def literal_update(X, codes, C, j):
    """The new codebook j in f64 (entries without rows: the old value) and the counts."""
    h = C.shape[1]
    sums, cnt = class_sums(literal_xd(X, codes, C, j), codes[:, j], h, np.float64)
    new = C[j].astype(np.float64)
    used = cnt > 0
    new[used] = sums[used] / cnt[used, None]
    return new, cnt


def literal(X, codes0, C0, niter, encode):
    """-> C, codes, obj (niter * m + 1,), invariant: per iteration, whether codes == encode(X, C)."""
    C, codes = C0.copy(), codes0.copy()
    m = C.shape[0]
    obj, inv = [qerror(X, codes, C)], []
    for _ in range(niter):
        Xr = X.astype(np.float32, copy=True)
        for j in range(m):
            C[j] = literal_update(X, codes, C, j)[0].astype(np.float32)
            if j > 0:
                Xr -= C[j - 1][codes[:, j - 1]]                      # :113-115
            codes[:, j:] = encode(Xr, C[j:])                          # :118
            obj.append(qerror(X, codes, C))
        inv.append(bool(np.array_equal(codes, encode(X, C))))
    return C, codes, np.asarray(obj), inv


def incremental(X, codes0, C0, niter, encode, acc=np.float32):
    """The library's loop: C_j[k] += mean of E over the rows of k; P_j kept as prefix residuals."""
    C, codes = C0.copy(), codes0.copy()
    m, h, _ = C.shape
    E = X.astype(np.float32, copy=True)
    for i in range(m):
        E -= C[i][codes[:, i]]
    obj, inv = [qerror(X, codes, C)], []
    for _ in range(niter):
        P = X.astype(np.float32, copy=True)
        for j in range(m):
            sums, cnt = class_sums(E, codes[:, j], h, acc)
            used = cnt > 0
            if acc == np.float32:
                C[j][used] = C[j][used] + sums[used] / cnt[used, None].astype(np.float32)
            else:
                C[j][used] = (C[j][used].astype(acc) + sums[used] / cnt[used, None]).astype(np.float32)
            part, _, E = encode(P, C[j:], with_extras=True)
            codes[:, j:] = part
            P = P - C[j][codes[:, j]]
            obj.append(qerror(X, codes, C))
        inv.append(bool(np.array_equal(codes, encode(X, C))))
    return C, codes, np.asarray(obj), inv


def spread(a, b):
    """(worst relative difference of the obj traces, worst absolute codebook entry difference, share of differing codes)"""
    Ca, Ba, oa = a[:3]
    Cb, Bb, ob = b[:3]
    return (float(np.max(np.abs(oa - ob) / np.abs(oa))), float(np.max(np.abs(Ca.astype(np.float64) - Cb))),
            float(np.mean(Ba != Bb)))
