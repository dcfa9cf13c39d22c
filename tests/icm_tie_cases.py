"""Inputs on which the two tie rules of the LSQ encoding contract decide the answer -- test infrastructure, a
plain helper module: no GPU, no test functions.

Rule 2: the code of a conditioning step is the FIRST index of the minimum under strict `<`.  Rule 3: a perturbed solution replaces
the old one only if `cost_new < cost_old`.  Gaussian data never has two equal costs, so neither rule is reached by it.  Here:

  dup_case   codeword l and every l + qP < h are bit-identical, so their candidates have bit-identical costs in the restatement and
             on the device (the same inputs through the same k-ordered chains, whatever the position): every conditioning step is
             tied P-periodically, and the lowest copy must win.  With `exact` the start codes reconstruct X exactly from the HIGHEST
             copies: the start cost is +0, the encoder finds the lowest copies at the same cost, and must keep the old codes.
  int_case   small integers as float32: every operation is exact, DIFFERENT codewords end with equal costs.
  census     how often, and where in a kernel's lane layout, a run of the restatement is tied.
  ils_mutant the restatement with either rule broken: what a wrong kernel would compute.  tests/test_icm_tie_cases.py shows on the
             CPU that every case of tests/test_gpu_icm_ties.py tells the mutants from the contract.

The layouts.  Byte kernel (rq_icm.hip): lane = idx // E, E = ceil(h / 64) consecutive entries per lane.  Wide kernel
(rq_icm_h16.hip): the row goes by in pieces of 256 floats, piece = idx // 256, lane = (idx % 256) // 4.
"""
import collections

import numpy as np

import icm_oracle as io
import icm_wide_oracle as wo

BUILD_SEED, ILS_SEED, INT_SEED = 7, 3, 105
LOW_ARGS = (3, 2, 2, True)         # (ilsiter, icmiter, npert, randord)
KEEP_ARGS = (3, 2, 1, True)
INT_ARGS = (3, 2, 2, True)

# kind: "dup" or "int"; wide: the int16 entry; P, where, exact: dup_case's; bar: the least share of rows on which the last-index
# mutant must end with other codes (None: exempt)
Case = collections.namedtuple("Case", "kind wide n d m h P where exact args bar")


def _low(wide, m, h, P, n=64, d=16):
    full = h % P == 0
    bar = None if P == 1 else (0.5 if full else 1.0 / n)
    return Case("dup", wide, n, d, m, h, P, "low", False, LOW_ARGS, bar)


# a. lowest copy wins.  Byte: E = 4, 2 and 1; a tie inside a lane, between adjacent lanes, across the butterfly's widest step; the
# three MB instantiations.  Wide: the same lane in the next piece, a copy in the short last piece, the last entry h - 1 alone in
# its 64-block and behind the clamp duplicating entry 0, sixteen pieces, the m = 16 register budget.
BYTE_LOW = [_low(False, *s) for s in [(4, 256, 1), (4, 256, 2), (4, 256, 4), (4, 256, 64), (4, 256, 128), (8, 256, 2), (16, 64, 32),
                                      (5, 100, 50), (5, 100, 1)]]
WIDE_LOW = [_low(True, *s) for s in [(4, 1024, 1), (4, 1024, 4), (4, 1024, 64), (4, 1024, 256), (4, 300, 256), (8, 321, 320)]] + \
           [_low(True, 2, 4096, 2048, n=32), _low(True, 16, 320, 5, n=32, d=8)]


def _keep(wide, m, h, P):
    return Case("dup", wide, 64, 16, m, h, P, "high", True, KEEP_ARGS, None)


# b. an equal cost keeps the old codes; and the same shape on Gaussian X, where the lower copies must win everywhere
BYTE_KEEP = [_keep(False, 4, 256, 128), _keep(False, 4, 256, 4)]
WIDE_KEEP = [_keep(True, 4, 512, 256), _keep(True, 8, 300, 150)]
WIDE_HIGH_GAUSS = Case("dup", True, 64, 16, 8, 300, 150, "high", False, KEEP_ARGS, 0.5)

# c. different codewords, equal costs
BYTE_INT = [Case("int", False, n, d, m, h, 0, "", False, INT_ARGS, None) for n, d, m, h in [(128, 12, 4, 64), (100, 12, 5, 100),
                                                                                            (64, 12, 8, 256)]]
WIDE_INT = [Case("int", True, n, d, m, h, 0, "", False, INT_ARGS, None) for n, d, m, h in [(96, 12, 4, 300), (64, 12, 2, 1000),
                                                                                           (64, 12, 8, 320)]]

BYTE_CASES = BYTE_LOW + BYTE_KEEP + BYTE_INT
WIDE_CASES = WIDE_LOW + WIDE_KEEP + [WIDE_HIGH_GAUSS] + WIDE_INT
ALL_CASES = BYTE_CASES + WIDE_CASES


def case_id(c):
    if c.kind == "int":
        return "%s-int-n%d-m%d-h%d" % ("wide" if c.wide else "byte", c.n, c.m, c.h)
    return "%s-m%d-h%d-P%d-%s%s" % ("wide" if c.wide else "byte", c.m, c.h, c.P, c.where, "-exact" if c.exact else "")


# ---- the builders ---------------------------------------------------------------------------------------------------------------
def dup_case(n, d, m, h, P, where="low", exact=False, seed=BUILD_SEED):
    """(X [n][d] f32, C [m][h][d] f32, B0 [n][m] int16 zero-based) with C[j][l] = base[j][l % P]."""
    assert 1 <= P <= h and where in ("low", "high")
    rng = np.random.default_rng(seed)
    base = (0.5 * rng.standard_normal((m, P, d))).astype(np.float32)
    C = np.ascontiguousarray(base[:, np.arange(h) % P, :])
    draw = rng.integers(0, P, size=(n, m))
    B0 = draw + P * ((h - 1 - draw) // P) if where == "high" else draw
    if exact:      # veccost's CB: adds from +0 in codebook order, so CB - X is +0 in every dimension
        X = np.zeros((n, d), dtype=np.float32)
        for i in range(m):
            X = X + C[i][B0[:, i]]
    else:
        X = rng.standard_normal((n, d)).astype(np.float32)
    return X, C, B0.astype(np.int16)


def int_case(n, d, m, h, seed=INT_SEED):
    """The "ties" kind of tests/gen_icm_golden.py (its rng is default_rng(100 + its seed)): C in {-1, 0, 1}, X in -2..2."""
    rng = np.random.default_rng(seed)
    C = rng.integers(-1, 2, size=(m, h, d)).astype(np.float32)
    X = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    B0 = rng.integers(0, h, size=(n, m)).astype(np.int16)
    return X, C, B0


def build(c):
    if c.kind == "int":
        return int_case(c.n, c.d, c.m, c.h)
    return dup_case(c.n, c.d, c.m, c.h, c.P, c.where, c.exact)


def _mod(wide):
    return wo if wide else io


def _dtype(wide):
    return np.int16 if wide else np.uint8


# ---- the mutants ----------------------------------------------------------------------------------------------------------------
def _costs(B, U, binT, j):
    """io.condition's candidate costs [n][h]: the unary, then the binaries in ascending k, one f32 add each."""
    ub = U[j].copy()
    for k in range(B.shape[1]):
        if k != j:
            ub = ub + binT[j, k][B[:, k].astype(np.int64)]
    return ub


def condition_last(B, U, binT, j):
    """The conditioning step of a kernel that prefers the higher index on equal values."""
    ub = _costs(B, U, binT, j)
    B[:, j] = ub.shape[1] - 1 - np.argmin(ub[:, ::-1], axis=1)


def ils_mutant(oracle, X, C, B0, ilsiter, icmiter, npert, randord, seed=0, t0=0, wide=False, last=False, le=False, tabs=None,
               on_accept=None):
    """icm_oracle.ils / icm_wide_oracle.ils written out again, with the last index of the minimum (`last`) and / or an accept test
    `c <= cost` (`le`).  on_accept(B, nb, cost, c) sees every iteration before the accept test."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.ascontiguousarray(C, dtype=np.float32)
    m, h, _ = C.shape
    rows = np.arange(X.shape[0])
    U, binT = _mod(wide).tables(oracle, X, C) if tabs is None else tabs
    cond = condition_last if last else io.condition
    B = np.array(B0, dtype=_dtype(wide), copy=True)
    cost = io.veccost(X, B, C)
    for it in range(ilsiter):
        t = t0 + it
        perm = io.visit_order(seed, t, m, randord)
        take, vals = io.perturbation(seed, t, rows, m, h, npert)
        nb = B.copy()
        nb[take] = vals[take]
        for _ in range(icmiter):
            for j in perm:
                cond(nb, U, binT, j)
        c = io.veccost(X, nb, C)
        if on_accept is not None:
            on_accept(B, nb, cost, c)
        better = (c <= cost) if le else (c < cost)
        B[better] = nb[better]
        cost[better] = c[better]
    return B, cost


# ---- the census -----------------------------------------------------------------------------------------------------------------
def census(oracle, X, C, B0, args, wide, seed=ILS_SEED, tabs=None):
    """Runs the restatement with a counting conditioning step and returns, per conditioning step and row ([steps][n] arrays):
      tied         the minimum is attained more than once;
      same_lane    tied, and the first and the last attaining index lie in the same lane;
      cross_lane   tied, in different lanes;
      cross_piece  tied, in different pieces of 256 (wide layout only: all False for the byte layout);
      in_lane      some lane holds two attaining indices, wherever the first and the last lie (what the scan inside a lane sees);
    and `eq_reject_rows`: the rows with an equal-cost rejection, some iteration with c == cost and nb != B."""
    C = np.ascontiguousarray(C, dtype=np.float32)
    h = C.shape[1]
    E = -(-h // 64)
    tabs = _mod(wide).tables(oracle, X, C) if tabs is None else tabs
    steps = {k: [] for k in ("tied", "same_lane", "cross_lane", "cross_piece", "in_lane")}
    lane_of = (np.arange(h) % 256) // 4 if wide else np.arange(h) // E
    member = (lane_of[:, None] == np.arange(64)[None, :]).astype(np.int32)          # [h][64]

    def lane(idx):
        return lane_of[idx]

    def cond(B, U, binT, j):
        ub = _costs(B, U, binT, j)
        att = ub == ub.min(axis=1)[:, None]
        first = np.argmax(att, axis=1)
        lastix = h - 1 - np.argmax(att[:, ::-1], axis=1)
        tied = att.sum(axis=1) > 1
        same = lane(first) == lane(lastix)
        steps["tied"].append(tied)
        steps["same_lane"].append(tied & same)
        steps["cross_lane"].append(tied & ~same)
        steps["cross_piece"].append(tied & (first // 256 != lastix // 256) if wide else np.zeros_like(tied))
        steps["in_lane"].append((att.astype(np.int32) @ member).max(axis=1) > 1)
        B[:, j] = first

    got = _mod(wide).ils(oracle, X, C, B0, *args, seed=seed, cond=cond, tabs=tabs)
    rej = np.zeros(X.shape[0], dtype=bool)

    def on_accept(B, nb, cost, c):
        rej[...] |= (c == cost) & (nb != B).any(axis=1)

    again = ils_mutant(oracle, X, C, B0, *args, seed=seed, wide=wide, tabs=tabs, on_accept=on_accept)
    assert np.array_equal(got[0], again[0])
    out = {k: np.array(v) for k, v in steps.items()}
    out["eq_reject_rows"] = np.flatnonzero(rej)
    return out


# ---- what the restatement answers, once per case ------------------------------------------------------------------------------------
_EXPECTED = {}
_STUDY = {}


def _orc():
    from oracle import oracle
    oracle.lib()
    return oracle


def expected(c):
    """(X, C, B0, codes, cost): the case and the restatement's answer to it (ILS seed 3), computed once."""
    if c not in _EXPECTED:
        X, C, B0 = build(c)
        B0 = B0.astype(_dtype(c.wide))
        codes, cost = _mod(c.wide).ils(_orc(), X, C, B0, *c.args, seed=ILS_SEED)
        _EXPECTED[c] = (X, C, B0, codes, cost)
    return _EXPECTED[c]


def study(c):
    """The restatement, the three mutants and the census on one set of tables: a dict of `expected`'s tuple ("exp"), the no-flag
    mutant's answer ("plain"), the rows whose final codes the mutants change ("last_rows", "le_rows") and the census ("census")."""
    if c not in _STUDY:
        o = _orc()
        X, C, B0 = build(c)
        B0 = B0.astype(_dtype(c.wide))
        tabs = _mod(c.wide).tables(o, X, C)
        codes, cost = _mod(c.wide).ils(o, X, C, B0, *c.args, seed=ILS_SEED, tabs=tabs)
        _EXPECTED.setdefault(c, (X, C, B0, codes, cost))
        kw = dict(seed=ILS_SEED, wide=c.wide, tabs=tabs)
        bl, _ = ils_mutant(o, X, C, B0, *c.args, last=True, **kw)
        be, _ = ils_mutant(o, X, C, B0, *c.args, le=True, **kw)
        _STUDY[c] = {"exp": (X, C, B0, codes, cost), "plain": ils_mutant(o, X, C, B0, *c.args, **kw),
                     "last_rows": np.flatnonzero((bl != codes).any(axis=1)), "le_rows": np.flatnonzero((be != codes).any(axis=1)),
                     "census": census(o, X, C, B0, c.args, c.wide, tabs=tabs)}
    return _STUDY[c]
