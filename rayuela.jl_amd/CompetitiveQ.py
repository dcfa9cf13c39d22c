"""Host mirror of src/CompetitiveQ.jl's encoder: beam-search residual encoding (`encode`, :75-135).

`train_competitiveq` (src/CompetitiveQ.jl:138-221) is NOT provided: it is a per-sample SGD whose codebooks change after every
single vector, so its result depends on the sample order and it cannot be batched without becoming a different algorithm.
Train the codebooks with train_rvq / train_ervq and encode with the functions below."""
import ctypes

import numpy as np

from . import _lib
from .RVQ import _stack_codebooks
from .utils import _as_f32, check_wide_h

BEAM_PHASES = ["stage_ms", "expand_ms", "other_ms"]


def _check(X, C, H, nsplits):
    X = _as_f32(X, "X")
    if X.ndim != 2:
        raise ValueError("X must be (n, d)")
    n, d = X.shape
    check_wide_h(np.asarray(C[0]).shape[0])
    Cs = _stack_codebooks(C)
    m, h, d2 = Cs.shape
    if d2 != d:
        raise ValueError("codebooks are %d-dimensional, data is %d-dimensional" % (d2, d))
    return np.ascontiguousarray(X), Cs, n, d, m, h, int(H), int(nsplits)


def quantize_competitiveq(X, C, H, nsplits=1, V=False):
    """`encode` (src/CompetitiveQ.jl:75-135) for every row of X: a beam search of width H over the residual stages.

    X (n, d) float32, C m-long list of (h, d) codebooks (quantize_rvq's layout), 1 <= H <= min(32, h).  Returns B (n, m) int16
    ONE-based, in quantize_rvq's layout; H = 1 gives quantize_rvq's codes.  nsplits: the minimum number of row chunks.
    256 < h <= 32767 codewords per stage take rq_encode_rvq_beam_wide; the return types are the same."""
    X, Cs, n, d, m, h, H, nsplits = _check(X, C, H, nsplits)
    B = np.empty((n, m), dtype=np.int16)
    if check_wide_h(h):
        _lib.check(_lib.lib().rq_encode_rvq_beam_wide(B.ctypes.data, X.ctypes.data, Cs.ctypes.data, n, d, m, h, H, nsplits, 1,
                                                      None, None))
    else:
        _lib.check(_lib.lib().rq_encode_rvq_beam_i16(B.ctypes.data, X.ctypes.data, Cs.ctypes.data, n, d, m, h, H, nsplits,
                                                     None, None))
    if V:
        print("Beam encoding with H = %d on %d codebooks... done" % (H, m))
    return B


def quantize_competitiveq_u8(X, C, H, nsplits=1, with_extras=False):
    """Zero-based uint8 codes (the scan's wire format); with_extras -> (codes, cost (n,), final residual (n, d)): cost is the
    canonical distance of the last stage's choice, the residual is X minus the chosen codewords, subtracted stage by stage."""
    X, Cs, n, d, m, h, H, nsplits = _check(X, C, H, nsplits)
    B = np.empty((n, m), dtype=np.uint8)
    cost = np.empty((n,), dtype=np.float32) if with_extras else None
    Xr = np.empty((n, d), dtype=np.float32) if with_extras else None
    _lib.check(_lib.lib().rq_encode_rvq_beam(B.ctypes.data, X.ctypes.data, Cs.ctypes.data, n, d, m, h, H, nsplits,
                                             None if cost is None else cost.ctypes.data,
                                             None if Xr is None else Xr.ctypes.data))
    return (B, cost, Xr) if with_extras else B


def quantize_competitiveq_u16(X, C, H, nsplits=1, with_extras=False):
    """Zero-based codes viewed as uint16 for any 1 <= h <= 32767 (rq_encode_rvq_beam_wide, code_base 0); with_extras ->
    (codes, cost (n,), final residual (n, d)) as quantize_competitiveq_u8."""
    X, Cs, n, d, m, h, H, nsplits = _check(X, C, H, nsplits)
    B = np.empty((n, m), dtype=np.int16)
    cost = np.empty((n,), dtype=np.float32) if with_extras else None
    Xr = np.empty((n, d), dtype=np.float32) if with_extras else None
    _lib.check(_lib.lib().rq_encode_rvq_beam_wide(B.ctypes.data, X.ctypes.data, Cs.ctypes.data, n, d, m, h, H, nsplits, 0,
                                                  None if cost is None else cost.ctypes.data,
                                                  None if Xr is None else Xr.ctypes.data))
    B = B.view(np.uint16)
    return (B, cost, Xr) if with_extras else B


def encode(x, C, new_res, m, h, d, H):
    """encode(x, C, new_res, m, h, d, H) -> codes, residual          (src/CompetitiveQ.jl:75-135)

    One vector x (d,), C m-long list of (h, d) codebooks; `new_res`, the reference's residual buffer, is accepted and ignored.
    Returns the int16 ONE-based codes (m,) and the residual (d,) of the best beam."""
    x = _as_f32(x, "x")
    if x.ndim != 1 or x.shape[0] != d:
        raise ValueError("x must be a vector of length d = %d" % d)
    if len(C) != m or any(np.shape(c) != (h, d) for c in C):
        raise ValueError("C must hold m = %d codebooks of shape (h, d) = (%d, %d)" % (m, h, d))
    quantize = quantize_competitiveq_u16 if check_wide_h(h) else quantize_competitiveq_u8
    codes, _, Xr = quantize(x[None, :], C, H, with_extras=True)
    return codes[0].astype(np.int16) + 1, Xr[0]


def last_beam_timing():
    """Phase clock of this thread's last beam call (rq_last_beam_timing): stage kernels, expand kernels, other, in ms."""
    out = (ctypes.c_double * 3)()
    _lib.check(_lib.lib().rq_last_beam_timing(ctypes.cast(out, ctypes.c_void_p), 3))
    return dict(zip(BEAM_PHASES, [float(v) for v in out]))
