"""Expected codes of the *_wide encodes (more than 256 codewords per codebook), from the committed oracle alone -- a plain helper
module: no fixtures, no pytest hooks.

oracle.encode_pq emits bytes, so it cannot name a codeword past 255.  Per sub-space and per block of 256 codewords it is called
with ONE sub-quantizer of hb <= 256 codewords and with_costs=True; the blocks are merged in ascending order under a strict '<'
on the winning clamped value.  That is the first index of the minimum over all k in [0, h) of v_k = (u_k > 0 ? u_k : 0) -- the
oracle's own chains and its own clamp, so uneven splits and non-finite values are covered by construction."""
import numpy as np

BLOCK = 256


def splitarray(d, m):
    per, extra = divmod(d, m)
    off = [0]
    for i in range(m):
        off.append(off[-1] + per + (1 if i < extra else 0))
    return off


def sub_codebooks(C_cat, d, m, h):
    """The m [h][sub_i] blocks of the flat concatenation."""
    Cc = np.ascontiguousarray(np.asarray(C_cat, dtype=np.float32).reshape(-1))
    assert Cc.size == h * d
    off = splitarray(d, m)
    return [Cc[h * off[i]:h * off[i + 1]].reshape(h, off[i + 1] - off[i]) for i in range(m)], off


def encode_pq_wide(oracle, X, C_cat, m, h, with_costs=False):
    """codes [n][m] int16 zero-based (any 1 <= h <= 32767) [, costs [n][m] f32: the winning v]."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    Cs, off = sub_codebooks(C_cat, d, m, h)
    codes = np.zeros((n, m), dtype=np.int64)
    costs = np.zeros((n, m), dtype=np.float32)
    for i in range(m):
        Xs = np.ascontiguousarray(X[:, off[i]:off[i + 1]])
        for k0 in range(0, h, BLOCK):
            hb = min(BLOCK, h - k0)
            cb, vb = oracle.encode_pq(Xs, np.ascontiguousarray(Cs[i][k0:k0 + hb]), 1, hb, with_costs=True)
            cb, vb = cb[:, 0].astype(np.int64) + k0, vb[:, 0]
            if k0 == 0:
                codes[:, i], costs[:, i] = cb, vb
            else:
                better = vb < costs[:, i]                   # strict: the lower block keeps a tie
                codes[better, i] = cb[better]
                costs[better, i] = vb[better]
    assert codes.max(initial=0) < h
    codes = codes.astype(np.int16)
    return (codes, costs) if with_costs else codes


def encode_rvq_wide(oracle, X, C):
    """quantize_rvq (src/RVQ.jl:18-66) for any h: (codes [n][m] int16 zero-based, counts [m][h] uint32, final residual [n][d])."""
    Xr = np.array(X, dtype=np.float32, order="C")
    C = np.ascontiguousarray(C, dtype=np.float32)
    m, h, d = C.shape
    n = Xr.shape[0]
    codes = np.zeros((n, m), dtype=np.int16)
    counts = np.zeros((m, h), dtype=np.uint32)
    for i in range(m):
        ci = encode_pq_wide(oracle, Xr, C[i].reshape(-1), 1, h)[:, 0]
        codes[:, i] = ci
        Xr = (Xr - C[i][ci.astype(np.int64)]).astype(np.float32)          # a plain f32 subtraction
        counts[i] = np.bincount(ci.astype(np.int64), minlength=h).astype(np.uint32)
    return codes, counts, Xr
