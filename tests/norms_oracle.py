"""CPU restatement of the database-norms contract -- test infrastructure.

Every operation is one numpy float32 add, subtract or multiply (one rounding each), in the order of the kernels of
rq_norms.hip:

  aq_norms(codes, C)        norms[i] = |sum_k C_k[b_ik]|^2: CB[t] by adds from +0 in codebook order; lane l sums CB[t]^2 over
                            t = l, l + 64, ... from +0 (multiply and add unfused); the xor butterfly 32, 16, 8, 4, 2, 1 adds the
                            64 partial sums.
  quantize(norms, cb)       first index j minimising fl(fl(norm - cb[j])^2), strict < (findmin, src/utils.jl:50-55).

and the two independent evaluations the restatement is checked against:

  norms_f64 / norms_bound   the f64 value of |sum C_k[b_k]|^2 and the derived bound on the restatement's distance from it.
  findmin_loop              the literal loop of src/utils.jl:50-55 on numpy float32 scalars.
"""
import numpy as np


def aq_norms(codes, C):
    """codes [n][m] zero-based, C [m][h][d] f32 -> [n] f32."""
    C = np.asarray(C, dtype=np.float32)
    codes = np.asarray(codes)
    n = codes.shape[0]
    m, _, d = C.shape
    CB = np.zeros((n, d), dtype=np.float32)
    for i in range(m):
        CB = CB + C[i][codes[:, i].astype(np.int64)]
    sq = CB * CB
    part = np.zeros((n, 64), dtype=np.float32)
    for q in range(0, d, 64):
        cnt = min(64, d - q)
        part[:, :cnt] = part[:, :cnt] + sq[:, q:q + cnt]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ off]
    return part[:, 0].copy()


def quantize(norms, cb):
    """[n] f32, cb [hn] f32 (unsorted) -> zero-based uint8 codes [n]; np.argmin returns the first minimum."""
    norms = np.asarray(norms, dtype=np.float32)
    cb = np.asarray(cb, dtype=np.float32)
    if norms.size == 0:
        return np.zeros(0, dtype=np.uint8)
    df = norms[:, None] - cb[None, :]
    return np.argmin(df * df, axis=1).astype(np.uint8)


def findmin_loop(norms, cb):
    """src/utils.jl:50-55 as written: dists2norm[j] = (ithnorm - cbnorms[j])^2 in f32, then findmin (first minimum)."""
    out = np.zeros(len(norms), dtype=np.uint8)
    for i, v in enumerate(np.asarray(norms, dtype=np.float32)):
        best, bj = None, 0
        for j, c in enumerate(np.asarray(cb, dtype=np.float32)):
            df = np.float32(v - c)
            e = np.float32(df * df)
            if best is None or e < best:
                best, bj = e, j
        out[i] = bj
    return out


def recon_f64(codes, C):
    C = np.asarray(C, dtype=np.float64)
    codes = np.asarray(codes)
    r = np.zeros((codes.shape[0], C.shape[2]), dtype=np.float64)
    for i in range(C.shape[0]):
        r += C[i][codes[:, i].astype(np.int64)]
    return r


def norms_f64(codes, C):
    r = recon_f64(codes, C)
    return (r * r).sum(axis=1)


def _gamma(k):
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def norms_bound(codes, C):
    """|aq_norms - norms_f64| <= gamma_{T+6} sum_j rhat_j^2 + sum_j (2 |r_j| e_j + e_j^2), all in f64.

    r_j the exact component, rhat_j the f32 one: m - 1 rounded adds (the first, to +0, is exact) give
    |rhat_j - r_j| <= e_j = gamma_{m-1} sum_i |c_i[j]|, hence |rhat_j^2 - r_j^2| <= 2 |r_j| e_j + e_j^2.  Each rhat_j^2 then
    passes through one multiply, at most T - 1 rounded adds in its lane (T = ceil(d / 64) terms, the first added to +0) and 6
    butterfly adds: T + 6 roundings, relative to sum_j rhat_j^2 because every term is non-negative."""
    C64 = np.asarray(C, dtype=np.float64)
    codes = np.asarray(codes)
    m, _, d = C64.shape
    T = -(-d // 64)
    r = recon_f64(codes, C)
    a = np.zeros_like(r)
    for i in range(m):
        a += np.abs(C64[i][codes[:, i].astype(np.int64)])
    e = _gamma(m - 1) * a
    C32 = np.asarray(C, dtype=np.float32)
    rh = np.zeros(r.shape, dtype=np.float32)
    for i in range(m):
        rh = rh + C32[i][codes[:, i].astype(np.int64)]
    rh = rh.astype(np.float64)
    return _gamma(T + 6) * (rh * rh).sum(axis=1) + (2.0 * np.abs(r) * e + e * e).sum(axis=1)


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------------------
NORM_SHAPES = [(1, 1, 1, 2), (63, 3, 2, 16), (65, 6, 7, 255), (130, 130, 3, 256), (513, 128, 8, 256), (1007, 96, 16, 256),
               (70, 960, 8, 256), (9, 100, 64, 4)]      # (n, d, m, h)


def norm_case(n, d, m, h, integer=False):
    """Seeded codes (0 and h - 1 present; the single cell of (1, 1, 1, 2) holds h - 1) and codebooks: Gaussian, or integers of
    magnitude <= 31."""
    rng = np.random.default_rng(1000003 * n + 1009 * d + 17 * m + h)
    codes = rng.integers(0, h, size=(n, m)).astype(np.uint8)
    codes[0, 0] = 0
    codes[-1, -1] = h - 1
    if integer:
        C = rng.integers(-31, 32, size=(m, h, d)).astype(np.float32)
    else:
        C = rng.standard_normal((m, h, d)).astype(np.float32)
    return codes, C


QUANT_NS = [0, 1, 64, 65, 1007]


def quant_cases():
    """name -> (norms [1007] f32, cb [hn] f32): slices [:n] of the norms serve every n of QUANT_NS."""
    rng = np.random.default_rng(77)
    out = {}
    ints = rng.integers(0, 64, size=1007).astype(np.float32)
    # duplicate entries: the first of equal values must win
    out["duplicates"] = (ints, np.array([5, 9, 5, 30, 9, 30, 5, 61, 61, 0, 0], dtype=np.float32))
    # exact midpoints on integers: 10 is as far from 8 as from 12 -- listed 12 first, so 12's index wins; same for 3 / 7 around 5
    mid = np.tile(np.array([10, 5, 8, 12, 20, 0, 9, 11], dtype=np.float32), 126)[:1007]
    out["midpoints"] = (mid, np.array([12, 8, 7, 3, 20], dtype=np.float32))
    g = (rng.standard_normal(1007) * 40 + 300).astype(np.float32)
    out["unsorted"] = (g, rng.permutation(np.linspace(150, 450, 37)).astype(np.float32))
    out["hn1"] = (g, np.array([123.5], dtype=np.float32))
    cb256 = (rng.standard_normal(256) * 40 + 300).astype(np.float32)
    out["hn256"] = (g, cb256)
    far = g.copy()
    far[::3] = np.float32(1e6) + far[::3]
    far[1::3] = -far[1::3]
    out["outside_range"] = (far, rng.permutation(np.linspace(250, 350, 16)).astype(np.float32))
    return out
