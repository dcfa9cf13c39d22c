"""Host mirror of the end-to-end drivers: experiment_pq (src/PQ.jl:104-132), experiment_pq_query_base
(:137-159), experiment_opq (src/OPQ.jl:142-171), experiment_opq_query_base (:174-197), experiment_rvq
(src/RVQ.jl:130-175), experiment_rvq_query_base (:163-188), experiment_ervq and experiment_ervq_query_base
(src/ERVQ.jl:151-242), experiment_sr_cuda (src/SR.jl:247-306, :348-373), experiment_sr_cuda_query_base (:308-344, :376-402),
experiment_lsq_cuda and experiment_lsq_cuda_query_base (src/LSQ_GPU.jl:322-467).
train -> encode the base -> ADC search -> recall, every O(n) step on the device.  The norms leg of the additive quantizers
(get_norms_codebook, quantize_norms) runs on the device in the LSQ drivers and, with norms="device", in the RVQ, ERVQ and SR
drivers; their default norms="host" keeps the two numpy helpers below.  Every driver takes gt=None for "compute the ground
truth": the exact nearest neighbour of each query in the set the driver searches (Xb, or Xt in the *_query_base drivers)."""
import numpy as np

from .Linscan import eval_recall, linscan_opq, linscan_opq_u16, linscan_pq, linscan_pq_u16
from .OPQ import quantize_opq, train_opq
from .PQ import quantize_pq, train_pq
from .knn import groundtruth


def _gt(gt, X, Xq):
    """The ground truth of a driver: what the caller read from a file, or (gt=None) the exact nearest row of the searched set
    X per query, one-based, computed on the device (knn.groundtruth; the reference can only read it, src/read_datasets.jl)."""
    if gt is not None:
        return gt
    return groundtruth(X, Xq, 1)[0][:, 0]


def _qerror(X, B, C, R=None):
    """qerror_pq / qerror_opq (src/qerrors.jl:77-100): mean squared reconstruction error."""
    n, d = X.shape
    CB = np.concatenate([np.asarray(C[i])[B[:, i].astype(np.int64) - 1] for i in range(len(C))], axis=1)
    RX = X if R is None else X.astype(np.float64) @ np.asarray(R, dtype=np.float64).T   # R'X in memory-image form
    return float(((RX.astype(np.float64) - CB) ** 2).sum() / n)


def _scan_pq(B, Xq, C, h, m, knn, R=None):
    """The search leg of the PQ / OPQ drivers: linscan_pq / linscan_opq, and above 256 codewords per codebook the scans over
    16-bit codes.  Those read an int16 array as ZERO-based, while train_* and quantize_* return int16 ONE-based codes: the codes
    are converted explicitly."""
    if h > 256:
        B0 = (np.asarray(B) - 1).astype(np.uint16)
        return linscan_pq_u16(B0, Xq, C, knn) if R is None else linscan_opq_u16(B0, Xq, C, R, knn)
    b = int(np.log2(h) * m)
    return linscan_pq(B, Xq, C, b, knn) if R is None else linscan_opq(B, Xq, C, b, R, knn)


def experiment_pq(Xt, Xb, Xq, gt, m, h, niter=25, knn=1000, V=False, seed=0):
    C, B, train_error = train_pq(Xt, m, h, niter, V, seed=seed)
    if V:
        print("Error in training is %e" % train_error)
    B_base = quantize_pq(Xb, C, V)
    base_error = _qerror(Xb, B_base, C)
    if V:
        print("Error in base is %e" % base_error)
    dists, idx = _scan_pq(B_base, Xq, C, h, m, knn)
    recall = eval_recall(_gt(gt, Xb, Xq), idx, knn, verbose=V)
    return C, B, train_error, B_base, recall


def experiment_pq_query_base(Xt, Xq, gt, m, h, niter=25, knn=1000, V=False, seed=0):
    C, B, train_error = train_pq(Xt, m, h, niter, V, seed=seed)
    dists, idx = _scan_pq(B, Xq, C, h, m, knn)
    recall = eval_recall(_gt(gt, Xt, Xq), idx, knn, verbose=V)
    return C, B, train_error, recall


def experiment_opq(Xt, Xb, Xq, gt, m, h, init, niter=25, knn=1000, V=False, seed=0):
    C, B, R, train_error = train_opq(Xt, m, h, niter, init, V, seed=seed)
    if V:
        print("Error in training is %e" % train_error[-1])
    B_base = quantize_opq(Xb, R, C, V)
    base_error = _qerror(Xb, B_base, C, R)
    if V:
        print("Error in base is %e" % base_error)
    dists, idx = _scan_pq(B_base, Xq, C, h, m, knn, R)
    recall = eval_recall(_gt(gt, Xb, Xq), idx, knn, verbose=V)
    return C, B, R, train_error, B_base, recall


def experiment_opq_query_base(Xt, Xq, gt, m, h, init, niter=25, knn=1000, V=False, seed=0):
    C, B, R, train_error = train_opq(Xt, m, h, niter, init, V, seed=seed)
    dists, idx = _scan_pq(B, Xq, C, h, m, knn, R)
    recall = eval_recall(_gt(gt, Xt, Xq), idx, knn, verbose=V)
    return C, B, R, train_error, recall


def experiment_ivfpq(Xt, Xb, Xq, gt=None, nlist=1024, m=8, nprobes=(1, 8, 32), niter=25, knn=100, by_residual=True, V=False,
                     seed=0, add_rows=None, refine=None):
    """IVFADC (IVF.py; no counterpart in the reference): train the coarse centroids and the codebooks on Xt, build the index on
    Xb, search Xq once per nprobe.  Returns Q, C and {nprobe: recall curve of eval_recall} -- recall against the exact nearest
    neighbour, so it is bounded by the share of queries whose neighbour lies in a probed list.  add_rows: load Xb in adds of that
    many rows instead of one build; the loaded base, and so every curve, is the same.  refine=kc: Xb is uploaded as a Dataset and
    every search also runs as search_refine with kc candidates; a fourth return value {nprobe: {"adc": {1: r, 10: r, 100: r},
    "refined": {...}}} then holds recall@1 / 10 / 100 (the share of queries whose exact nearest neighbour is among the first R
    answers) without and with the refinement.  refine=None (the default) returns the three values it always returned."""
    from contextlib import ExitStack
    from .IVF import IvfIndex, train_ivfpq
    from .index import Dataset
    if refine is not None and refine < knn:
        raise ValueError("refine must be at least knn=%d candidates; got %d" % (knn, refine))
    Q, C = train_ivfpq(Xt, nlist, m, niter=niter, seed=seed, by_residual=by_residual)
    truth = _gt(gt, Xb, Xq)
    recall, refined = {}, {}
    with ExitStack() as stack:
        ds = stack.enter_context(Dataset(Xb)) if refine is not None else None
        ix = stack.enter_context(IvfIndex(Q, C, by_residual=by_residual))
        if add_rows is None:
            ix.build(Xb)
        else:
            if add_rows < 1:
                raise ValueError("add_rows must be positive")
            for r0 in range(0, Xb.shape[0], int(add_rows)):
                ix.add(Xb[r0:r0 + int(add_rows)])
        for nprobe in nprobes:
            if V:
                print("nprobe = %d" % nprobe)
            _, idx = ix.search(Xq, nprobe, knn)
            recall[nprobe] = eval_recall(truth, idx, knn, verbose=V)
            if ds is not None:
                _, idr = ix.search_refine(Xq, ds, nprobe, knn, int(refine))
                refined[nprobe] = {"adc": _recall_at(truth, idx, knn), "refined": _recall_at(truth, idr, knn)}
    if refine is not None:
        return Q, C, recall, refined
    return Q, C, recall


def _recall_at(truth, idx, knn, ranks=(1, 10, 100)):
    """{R: share of queries whose exact nearest neighbour (truth, one-based) is among the first R answers}, R <= knn"""
    t = np.asarray(truth).reshape(len(idx), -1)[:, 0].astype(np.int64)
    ids = np.asarray(idx).astype(np.int64)
    return {R: float((ids[:, :R] == t[:, None]).any(axis=1).mean()) for R in ranks if R <= knn}


def _norms_codebook(B, C, h=256, seed=0):
    """get_norms_codebook (src/utils.jl:4-26): norms of the reconstructions, quantised by a 1-D k-means
    (rq_train_pq with d = m = 1).  Returns (norms_codes one-based, norms_codebook (h,))."""
    from .PQ import train_pq
    Cs = np.stack([np.asarray(c, dtype=np.float32) for c in C])
    codes = B.astype(np.int64) - 1
    recon = np.zeros((B.shape[0], Cs.shape[2]), dtype=np.float32)
    for i in range(Cs.shape[0]):
        recon += Cs[i][codes[:, i]]
    dbnorms = (recon ** 2).sum(axis=1, dtype=np.float32).reshape(-1, 1)
    Cn, Bn, _ = train_pq(np.ascontiguousarray(dbnorms), 1, h, niter=25, seed=seed)
    return Bn[:, 0].astype(np.int64), Cn[0][:, 0].copy()


def _quantize_norms(B, C, norms_C):
    """quantize_norms (src/utils.jl:29-60): nearest entry of the norms codebook for every reconstruction."""
    Cs = np.stack([np.asarray(c, dtype=np.float32) for c in C])
    codes = B.astype(np.int64) - 1
    recon = np.zeros((B.shape[0], Cs.shape[2]), dtype=np.float32)
    for i in range(Cs.shape[0]):
        recon += Cs[i][codes[:, i]]
    dbnorms = (recon ** 2).sum(axis=1, dtype=np.float32)
    order = np.argsort(norms_C, kind="stable")
    srt = norms_C[order]
    pos = np.clip(np.searchsorted(srt, dbnorms), 1, len(srt) - 1)
    left = np.abs(dbnorms - srt[pos - 1]) <= np.abs(dbnorms - srt[pos])
    return order[np.where(left, pos - 1, pos)] + 1, dbnorms


def _check_norms_arg(norms):
    if norms not in ("host", "device"):
        raise ValueError('norms must be "host" or "device"; got %r' % (norms,))


def _search_base(B, C, h, seed, B_base, Xq, knn, norms, norms_niter=25):
    """The search leg over an encoded base: norms codebook of the training codes -> quantised norms of the base -> linscan_lsq.
    norms_niter: the k-means iterations of the device path; 25 is what the host helper runs, so that the two paths of the RVQ,
    ERVQ and SR drivers differ in the rounding of the norms alone.  h > 256 (16-bit codes, the RVQ drivers): the same leg through
    linscan_lsq_u16 / linscan_lsq_cbnorms_u16 and the *_wide norm entries."""
    from . import Linscan
    from .utils import get_norms_codebook
    d = Xq.shape[1]
    R = np.eye(d, dtype=np.float32)
    wide = h > 256      # 16-bit codes: the *_u16 scans; the codes are passed one-based in a dtype those read as one-based
    B_scan = np.asarray(B_base).astype(np.int32) if wide else B_base
    if norms == "device":
        _, norms_C = get_norms_codebook(B, C, norms_niter, seed=seed)
        scan = Linscan.linscan_lsq_cbnorms_u16 if wide else Linscan.linscan_lsq_cbnorms
        return scan(B_scan, Xq, C, norms_C, R, knn)
    _, norms_C = _norms_codebook(B, C, h, seed=seed)
    B_base_norms, _ = _quantize_norms(B_base, C, norms_C)
    db_norms = norms_C[B_base_norms - 1].astype(np.float32)
    scan = Linscan.linscan_lsq_u16 if wide else Linscan.linscan_lsq
    return scan(B_scan, Xq, C, db_norms, R, knn)


def _search_train(B, C, h, seed, Xq, knn, norms, norms_niter=25):
    """The search leg of the query-base drivers: the k-means' own assignments of the training codes are their quantised norms."""
    from . import Linscan
    from .utils import get_norms_codebook
    d = Xq.shape[1]
    if norms == "device":
        norms_B, norms_C = get_norms_codebook(B, C, norms_niter, seed=seed)
    else:
        norms_B, norms_C = _norms_codebook(B, C, h, seed=seed)
    db_norms = norms_C[norms_B - 1].astype(np.float32)
    if h > 256:         # 16-bit codes, passed one-based in a dtype linscan_lsq_u16 reads as one-based
        return Linscan.linscan_lsq_u16(np.asarray(B).astype(np.int32), Xq, C, db_norms, np.eye(d, dtype=np.float32), knn)
    return Linscan.linscan_lsq(B, Xq, C, db_norms, np.eye(d, dtype=np.float32), knn)


def _qerror_aq(X, B, C):
    """qerror (src/qerrors.jl) of full-dimensional codebooks: mean squared error of the summed reconstruction."""
    recon = np.zeros(X.shape, dtype=np.float64)
    for i in range(len(C)):
        recon += np.asarray(C[i], dtype=np.float64)[B[:, i].astype(np.int64) - 1]
    return float(((X.astype(np.float64) - recon) ** 2).sum() / X.shape[0])


def experiment_rvq(Xt, Xb, Xq, gt, m, h, niter=25, knn=1000, V=False, seed=0, norms="host"):
    """experiment_rvq (src/RVQ.jl:130-175): train_rvq -> norms codebook -> quantize_rvq of the base ->
    quantised database norms -> linscan_lsq -> eval_recall.  norms="device": the norms leg on the device (get_norms_codebook,
    LsqIndex.from_cbnorms) instead of the numpy helpers."""
    from .RVQ import train_rvq, quantize_rvq
    _check_norms_arg(norms)
    C, B, train_error = train_rvq(Xt, m, h, niter, V, seed=seed)
    B_base, _ = quantize_rvq(Xb, C, V)
    dists, idx = _search_base(B, C, h, seed, B_base, Xq, knn, norms)
    recall = eval_recall(_gt(gt, Xb, Xq), idx, knn, verbose=V)
    return C, B, train_error, B_base, recall


def experiment_rvq_query_base(Xt, Xq, gt, m, h, niter=25, knn=1000, V=False, seed=0, norms="host"):
    """experiment_rvq_query_base (src/RVQ.jl:163-188): train_rvq -> norms codebook -> linscan_lsq over the training codes
    -> eval_recall.  norms as for experiment_rvq."""
    from .RVQ import train_rvq
    _check_norms_arg(norms)
    C, B, train_error = train_rvq(Xt, m, h, niter, V, seed=seed)
    dists, idx = _search_train(B, C, h, seed, Xq, knn, norms)
    recall = eval_recall(_gt(gt, Xt, Xq), idx, knn, verbose=V)
    return C, B, train_error, recall


def experiment_ervq(Xt, *args, V=False, seed=0, norms="host"):
    """experiment_ervq(Xt, B, C, Xb, Xq, gt, m, h, niter=25, knn=1000, V=false)         (src/ERVQ.jl:151-184)
    experiment_ervq(Xt, Xb, Xq, gt, m, h, niter=25, knn=1000, V=false)                (src/ERVQ.jl:214-227)

    train_ervq -> norms codebook -> quantize_ervq of the base -> quantised database norms -> linscan_lsq -> eval_recall.
    The second method starts from train_rvq(Xt, m, h, niter, V).  Returns C, B, train_error, B_base, recall.
    norms as for experiment_rvq."""
    from .ERVQ import train_ervq, quantize_ervq
    from .RVQ import train_rvq
    _check_norms_arg(norms)
    if len(args) >= 7 and np.ndim(args[5]) == 0 and np.ndim(args[6]) == 0 and np.ndim(args[3]) > 0:
        B, C, Xb, Xq, gt, m, h = args[:7]
        rest = list(args[7:])
    elif len(args) >= 5:
        Xb, Xq, gt, m, h = args[:5]
        rest = list(args[5:])
        B = None
    else:
        raise TypeError("experiment_ervq(Xt, [B, C,] Xb, Xq, gt, m, h, niter=25, knn=1000, V=false)")
    niter = int(rest.pop(0)) if rest else 25
    knn = int(rest.pop(0)) if rest else 1000
    V = bool(rest.pop(0)) if rest else V
    if rest:
        raise TypeError("experiment_ervq: too many arguments")
    if B is None:
        C, B, _ = train_rvq(Xt, m, h, niter, V, seed=seed)
    C, B, train_error = train_ervq(Xt, B, C, m, h, niter, V, seed=seed)
    B_base, _ = quantize_ervq(Xb, C, V)
    if V:
        print("Error in base is %e" % _qerror_aq(Xb, B_base, C))
    dists, idx = _search_base(B, C, h, seed, B_base, Xq, knn, norms)
    recall = eval_recall(_gt(gt, Xb, Xq), idx, knn, verbose=V)
    return C, B, train_error, B_base, recall


def experiment_ervq_query_base(Xt, *args, V=False, seed=0, norms="host"):
    """experiment_ervq_query_base(Xt, B, C, Xq, gt, m, h, niter=25, knn=1000, V=false)  (src/ERVQ.jl:187-211)
    experiment_ervq_query_base(Xt, Xq, gt, m, h, niter=25, knn=1000, V=false)         (src/ERVQ.jl:230-242)

    train_ervq -> norms codebook -> linscan_lsq over the training codes -> eval_recall.  Returns C, B, train_error, recall.
    norms as for experiment_rvq."""
    from .ERVQ import train_ervq
    from .RVQ import train_rvq
    _check_norms_arg(norms)
    if len(args) >= 6 and np.ndim(args[4]) == 0 and np.ndim(args[5]) == 0 and np.ndim(args[2]) > 0:
        B, C, Xq, gt, m, h = args[:6]
        rest = list(args[6:])
    elif len(args) >= 4:
        Xq, gt, m, h = args[:4]
        rest = list(args[4:])
        B = None
    else:
        raise TypeError("experiment_ervq_query_base(Xt, [B, C,] Xq, gt, m, h, niter=25, knn=1000, V=false)")
    niter = int(rest.pop(0)) if rest else 25
    knn = int(rest.pop(0)) if rest else 1000
    V = bool(rest.pop(0)) if rest else V
    if rest:
        raise TypeError("experiment_ervq_query_base: too many arguments")
    if B is None:
        C, B, _ = train_rvq(Xt, m, h, niter, V, seed=seed)
    C, B, train_error = train_ervq(Xt, B, C, m, h, niter, V, seed=seed)
    dists, idx = _search_train(B, C, h, seed, Xq, knn, norms)
    recall = eval_recall(_gt(gt, Xt, Xq), idx, knn, verbose=V)
    return C, B, train_error, recall


def _sr_init(Xt, m, h, niter_init, chain, V, seed):
    """The initialisation of the LSQ++ drivers: train_opq "natural" (src/SR.jl:365, :391), then train_chainq (:397) where
    the reference runs it.  Returns C, B, R, opq_error.  h > 256: train_opq and train_chainq both run over 16-bit codes, so the
    start codes exist at any h <= 8192; train_sr_cuda then runs its own loop over 16-bit codes (rq_train_sr_wide) wherever
    m * h <= 16384 and the encoder's tables fit."""
    from .ChainQ import train_chainq
    C, B, R, opq_error = train_opq(Xt, m, h, niter_init, "natural", V, seed=seed)
    if chain:
        C, B, R, _ = train_chainq(Xt, m, h, R, B, C, niter_init, V)
    return C, B, R, opq_error


def experiment_sr_cuda_query_base(Xt, Xq, gt, m, h, niter=25, knn=1000, nsplits_train=1, sr_method="SR_D", V=False,
                                  seed=0, B=None, C=None, R=None, ilsiter=8, icmiter=4, randord=True, npert=4,
                                  schedule=1, p=0.5, niter_init=25, norms="host"):
    """experiment_sr_cuda_query_base (src/SR.jl:308-344, :376-402): train_sr_cuda -> norms codebook -> linscan_lsq over
    the training codes -> eval_recall.  Without B, C, R the start is train_opq "natural" then train_chainq (niter_init
    iterations each, the reference's 25) and the result is ((C, B, R, train_error, recall), opq_error) like the
    reference's six-argument method; with them it is (C, B, R, train_error, recall) like the full method.
    norms as for experiment_rvq."""
    from .SR import train_sr_cuda
    _check_norms_arg(norms)
    opq_error = None
    given = B is not None
    if not given:
        C, B, R, opq_error = _sr_init(Xt, m, h, niter_init, True, V, seed)
    if V:
        print("Running CUDA %s training... " % sr_method)
    C, B, train_error = train_sr_cuda(Xt, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, sr_method, schedule, p,
                                      nsplits_train, V, seed=seed)
    dists, idx = _search_train(B, C, h, seed, Xq, knn, norms)
    recall = eval_recall(_gt(gt, Xt, Xq), idx, knn, verbose=V)
    res = (C, B, R, train_error, recall)
    return res if given else (res, opq_error)


def experiment_sr_cuda(Xt, Xb, Xq, gt, m, h, niter=25, knn=1000, nsplits_train=1, nsplits_base=1, sr_method="SR_D",
                       V=False, seed=0, B=None, C=None, R=None, ilsiter=8, icmiter=4, randord=True, npert=4, schedule=1,
                       p=0.5, niter_init=25, norms="host"):
    """experiment_sr_cuda (src/SR.jl:247-306, :348-373): train_sr_cuda -> norms codebook -> the base encoded by
    encode_icm_cuda with 4 ilsiter iterations from seeded random codes -> quantised database norms -> linscan_lsq ->
    eval_recall.  Without B, C, R the start is train_opq "natural" (the reference leaves train_chainq out here, :369).
    Returns C, B, R, train_error, B_base, recall.  norms as for experiment_rvq."""
    from .LSQ import encode_icm_cuda
    from .SR import train_sr_cuda
    _check_norms_arg(norms)
    if B is None:
        C, B, R, _ = _sr_init(Xt, m, h, niter_init, False, V, seed)
    if V:
        print("Running LSQ++ (%s) with %d codebooks, %d perturbations, %d icm iterations and random order = %s"
              % (sr_method, m, npert, icmiter, bool(randord)))
    C, B, train_error = train_sr_cuda(Xt, m, h, R, B, C, niter, ilsiter, icmiter, randord, npert, sr_method, schedule, p,
                                      nsplits_train, V, seed=seed)
    B_base = np.random.default_rng(seed).integers(1, h + 1, size=(Xb.shape[0], m)).astype(np.int16)
    Bs_base, objs = encode_icm_cuda(Xb, B_base, C, [ilsiter * 4], icmiter, npert, randord, nsplits_base, V, seed=seed)
    B_base = Bs_base[-1]
    if V:
        print("Error in base is %e" % objs[-1])
    dists, idx = _search_base(B, C, h, seed, B_base, Xq, knn, norms)
    recall = eval_recall(_gt(gt, Xb, Xq), idx, knn, verbose=V)
    return C, B, R, train_error, B_base, recall


def experiment_lsq_cuda(Xt, *args, V=False, seed=0, niter_init=25):
    """experiment_lsq_cuda(Xt, B, C, R, Xb, Xq, gt, m, h, niter=25, ilsiter=8, icmiter=4, randord=true, npert=4, knn=1000,
                        nsplits_train=1, nsplits_base=1, V=false)                                  (src/LSQ_GPU.jl:322-368)
    experiment_lsq_cuda(Xt, Xb, Xq, gt, m, h, niter=25, ...the same...)                               (src/LSQ_GPU.jl:407-436)

    train_lsq_cuda -> norms codebook -> the base encoded by encode_icm_cuda with 4 ilsiter iterations from seeded random
    codes -> quantised database norms -> linscan_lsq -> eval_recall; the norms leg runs on the device (get_norms_codebook,
    LsqIndex.from_cbnorms).  The second method starts from train_opq "natural" (niter_init iterations; the reference passes
    niter, :426 -- niter_init defaults to its 25).  Returns C, B, R, train_error, B_base, recall."""
    from .LSQ import encode_icm_cuda, train_lsq_cuda
    if len(args) >= 8 and np.ndim(args[6]) == 0 and np.ndim(args[7]) == 0 and np.ndim(args[3]) > 0:
        B, C, R, Xb, Xq, gt, m, h = args[:8]
        rest = list(args[8:])
    elif len(args) >= 5:
        Xb, Xq, gt, m, h = args[:5]
        rest = list(args[5:])
        B = None
    else:
        raise TypeError("experiment_lsq_cuda(Xt, [B, C, R,] Xb, Xq, gt, m, h, niter=25, ilsiter=8, icmiter=4, randord=true, "
                        "npert=4, knn=1000, nsplits_train=1, nsplits_base=1, V=false)")
    names = ("niter", "ilsiter", "icmiter", "randord", "npert", "knn", "nsplits_train", "nsplits_base", "V")
    if len(rest) > len(names):
        raise TypeError("experiment_lsq_cuda: too many arguments")
    o = dict(niter=25, ilsiter=8, icmiter=4, randord=True, npert=4, knn=1000, nsplits_train=1, nsplits_base=1, V=V)
    o.update(zip(names, rest))
    V = bool(o["V"])
    if B is None:
        C, B, R, _ = train_opq(Xt, m, h, niter_init, "natural", V, seed=seed)
    if V:
        print("Running CUDA LSQ training... ")
    C, B, train_error = train_lsq_cuda(Xt, m, h, R, B, C, o["niter"], o["ilsiter"], o["icmiter"], o["randord"], o["npert"],
                                       o["nsplits_train"], V, seed=seed)
    B_base = np.random.default_rng(seed).integers(1, h + 1, size=(Xb.shape[0], m)).astype(np.int16)
    Bs_base, objs = encode_icm_cuda(Xb, B_base, C, [o["ilsiter"] * 4], o["icmiter"], o["npert"], o["randord"],
                                    o["nsplits_base"], V, seed=seed)
    B_base = Bs_base[-1]
    if V:
        print("Error in base is %e" % objs[-1])
    dists, idx = _search_base(B, C, h, seed, B_base, Xq, int(o["knn"]), "device", 100)
    recall = eval_recall(_gt(gt, Xb, Xq), idx, int(o["knn"]), verbose=V)
    return C, B, R, train_error, B_base, recall


def experiment_lsq_cuda_query_base(Xt, *args, V=False, seed=0, **named):
    """experiment_lsq_cuda_query_base(Xt, B, C, R, Xq, gt, m, h, niter=25, ilsiter=8, icmiter=4, randord=true, npert=4,
                                   knn=1000, nsplits_train=1, V=false)                             (src/LSQ_GPU.jl:370-403)
    experiment_lsq_cuda_query_base(Xt, Xq, gt, m, h, niter=25, ilsiter=8, icmiter=4, randord=true, npert=4, init="natural",
                                   niter_opq=25, niter_chainq=25, knn=1000, nsplits_train=1, V=false)  (src/LSQ_GPU.jl:438-468)

    train_lsq_cuda -> norms codebook on the device -> linscan_lsq over the training codes with the k-means' assignments ->
    eval_recall.  The first method returns (C, B, R, train_error, recall).  The second starts from train_opq(init) then
    train_chainq and returns ((C, B, R, train_error, recall), opq_error).  Deviation: the reference's second method hands
    `niter, knn, nsplits_train, V` positionally to the first (:467), where they land in the slots niter, ilsiter, icmiter,
    randord; here every argument is passed by meaning (ilsiter, icmiter, randord, npert included).  The optional arguments may
    also be given by name.  h > 256: every step runs over 16-bit codes (train_opq, train_chainq, train_lsq_cuda, linscan_lsq_u16)."""
    from .ChainQ import train_chainq
    from .LSQ import train_lsq_cuda
    full = len(args) >= 7 and np.ndim(args[5]) == 0 and np.ndim(args[6]) == 0 and np.ndim(args[2]) > 0
    if full:
        B, C, R, Xq, gt, m, h = args[:7]
        rest = list(args[7:])
        names = ("niter", "ilsiter", "icmiter", "randord", "npert", "knn", "nsplits_train", "V")
    elif len(args) >= 4:
        Xq, gt, m, h = args[:4]
        rest = list(args[4:])
        names = ("niter", "ilsiter", "icmiter", "randord", "npert", "init", "niter_opq", "niter_chainq", "knn",
                 "nsplits_train", "V")
    else:
        raise TypeError("experiment_lsq_cuda_query_base(Xt, [B, C, R,] Xq, gt, m, h, niter=25, ...)")
    if len(rest) > len(names):
        raise TypeError("experiment_lsq_cuda_query_base: too many arguments")
    for key in named:
        if key not in names or key in names[:len(rest)]:
            raise TypeError("experiment_lsq_cuda_query_base: unexpected or repeated argument %r" % key)
    o = dict(niter=25, ilsiter=8, icmiter=4, randord=True, npert=4, init="natural", niter_opq=25, niter_chainq=25, knn=1000,
             nsplits_train=1, V=V)
    o.update(zip(names, rest))
    o.update(named)
    V = bool(o["V"])
    opq_error = None
    if not full:
        C, B, R, opq_error = train_opq(Xt, m, h, o["niter_opq"], o["init"], V, seed=seed)
        C, B, R, _ = train_chainq(Xt, m, h, R, B, C, o["niter_chainq"], V)
    if V:
        print("Running CUDA LSQ training... ")
    C, B, train_error = train_lsq_cuda(Xt, m, h, R, B, C, o["niter"], o["ilsiter"], o["icmiter"], o["randord"], o["npert"],
                                       o["nsplits_train"], V, seed=seed)
    dists, idx = _search_train(B, C, h, seed, Xq, int(o["knn"]), "device", 100)
    recall = eval_recall(_gt(gt, Xt, Xq), idx, int(o["knn"]), verbose=V)
    res = (C, B, R, train_error, recall)
    return res if full else (res, opq_error)
