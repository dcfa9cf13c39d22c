"""rayuela.jl_amd -- MI355X (gfx950) PQ/OPQ encode + ADC linear scan behind Rayuela.jl's API.

Host-side mirror of the reference's operator interface for this path (same names, argument order,
defaults and index bases as src/PQ.jl, src/OPQ.jl, src/Linscan.jl), implemented as thin calls into
the C ABI of librayuela_hip.so (include/rayuela_hip.h).  The Julia drop-in files that bind the same
ABI with `ccall` live in julia/.  No CPU fallback exists: without the HIP library every call raises.
"""
from ._lib import RayuelaHipError, lib, lib_path, set_tuning, reset_tuning, last_timing  # noqa: F401
from .utils import splitarray, cat_codebooks, get_norms_codebook, quantize_norms, aq_norms  # noqa: F401
from .xvecs import (fvecs_read, ivecs_read, bvecs_read, fvecs_write, ivecs_write, bvecs_write,  # noqa: F401
                    quantize_bvecs, ivf_add_bvecs, ivf_add_fvecs)
from .PQ import quantize_pq, quantize_pq_u8, quantize_pq_u16  # noqa: F401
from .OPQ import quantize_opq, quantize_opq_u16, rotate  # noqa: F401
from .RVQ import quantize_rvq, quantize_rvq_u8, quantize_rvq_u16  # noqa: F401


from .PQ import train_pq, kmpp_seeds  # noqa: F401,E402
from .OPQ import train_opq  # noqa: F401,E402
from .RVQ import train_rvq  # noqa: F401,E402
from .ERVQ import quantize_ervq, train_ervq, ervq_update_codebook, last_ervq_timing  # noqa: F401,E402
from .LSQ import encoding_icm, encode_icm_cuda, veccost, qerror, train_lsq, train_lsq_cuda  # noqa: F401,E402
from .SR import apply_schedule, SR_C_perturb, SR_D_perturb, train_sr, train_sr_cuda  # noqa: F401,E402
from .codebook_update import (update_codebooks, update_codebooks_fast_bin, update_codebooks_chain_bin,  # noqa: F401,E402
                              update_codebooks_chain_bin_u16, get_cbdims_chain)
from .ChainQ import quantize_chainq, quantize_chainq_u16, train_chainq, train_chainq_u16  # noqa: F401,E402
from .CompetitiveQ import quantize_competitiveq, quantize_competitiveq_u8, quantize_competitiveq_u16, last_beam_timing  # noqa: F401,E402
from . import CompetitiveQ  # noqa: F401,E402  (CompetitiveQ.encode: the reference's one-vector signature)
from .Linscan import (linscan_pq, linscan_opq, linscan_lsq, linscan_cq, linscan_aqd_query, LsqIndex,  # noqa: F401
                      linscan_aqd_query_extra_byte, eval_recall, linscan_lsq_cbnorms, linscan_pq_u16, linscan_opq_u16,
                      linscan_lsq_u16, linscan_cq_u16, linscan_lsq_cbnorms_u16)

from .index import Index, IndexU16, AqIndex, AqIndexU16, Dataset  # noqa: F401,E402
from .IVF import IvfIndex, train_ivfpq  # noqa: F401,E402
from .knn import groundtruth, knn_f64, knn_f32, knn_plan, last_knn_stats, last_knn_timing  # noqa: F401,E402
from .knn import rerank_plan, last_rerank_stats, last_rerank_timing  # noqa: F401,E402
from . import h5results  # noqa: F401,E402  (libhdf5 is looked up lazily, on first use)
from . import datasets  # noqa: F401,E402

__all__ = ["quantize_pq", "quantize_opq", "linscan_pq", "linscan_opq", "linscan_lsq", "linscan_cq",
           "encoding_icm", "encode_icm_cuda", "train_lsq", "train_lsq_cuda", "train_sr", "train_sr_cuda",
           "apply_schedule", "SR_C_perturb", "SR_D_perturb", "update_codebooks",
           "update_codebooks_fast_bin", "quantize_chainq", "train_chainq", "update_codebooks_chain_bin", "get_cbdims_chain",
           "quantize_competitiveq", "quantize_competitiveq_u8", "quantize_competitiveq_u16",
           "quantize_ervq", "train_ervq", "ervq_update_codebook", "last_ervq_timing",
           "eval_recall", "groundtruth", "knn_f64", "knn_f32", "splitarray", "get_norms_codebook", "quantize_norms"]
