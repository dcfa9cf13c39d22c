"""Every run-time switch the library reads (`tuning("KEY", default)` in rayuela.jl_amd/csrc, env RQ_<KEY> or rq_set_tuning),
with its code default and how the suite covers it.  A plain helper module, imported by the tests (not a conftest).

Each entry of SWITCHES carries `default` and exactly one of
  * `values` + `workload`: tests/test_gpu_switches.py runs that workload with each value set and compares with the oracle;
    `readout` names what the library reports that tells the switched path from the default one (the test asserts it moved:
    "orders" = rq_scan_orders_in_call, "plan" = rq_scan_plan, "kernel" = rq_last_scan_kernel, "stats:<counter>" = the scan's
    counters, "order_plan" = rq_order_plan, "encode_kernel" = rq_last_encode_kernel); a swept entry without one says why in
    `note`;
  * `tested_in`: a test that already sets the switch and compares with the oracle;
  * `reason`: why the switch cannot change a computed value, or cannot be exercised on one GPU.

INTEGRATION.md section 6 promises that no switch changes a result; tests/test_switch_table.py keeps this table equal to the
code's keys and defaults.

`switches(**kv)` sets values for the length of a `with` block and RESETS them on exit (rq_reset_tuning): storing the default back
is not the same -- it would hide RQ_<KEY> from the environment, and SCAN_SAMPLE tells "unset" (-1) from any stored value.
"""
import contextlib

_SCAN = "tests/test_gpu_scan.py"
_ORDER = "tests/test_gpu_order.py"
_FUZZ = "tests/test_gpu_fuzz.py"
_ENC = "tests/test_gpu_encode.py"
_TRAIN = "tests/test_gpu_train.py"
_POOL = "tests/test_gpu_hostpool.py"
_INDEX = "tests/test_gpu_index.py"

SWITCHES = {
    # ---- encode / rotation / RVQ (rq_encode.hip, rq_encode_filter.hip) ----
    "ENC_SPLIT": dict(default=1, values=(0, 2), workload="encode",
                      readout="encode_kernel"),
    "ENC_DIRECT": dict(default=1, values=(0,), workload="encode",
                       readout="encode_kernel"),
    "ENC_WAVES": dict(default=16, values=(8,), workload="encode",
                      note="no readout: the same kernel with 8 wavefronts per workgroup, checked against the oracle only"),
    "ENC_SPLIT_WAVES": dict(default=0, tested_in=_ENC + "::test_split_encode_hostile_inputs"),
    "ENC_SPLIT_DELTA_MILLI": dict(default=3000, tested_in="tests/test_gpu_encode_margin.py::test_filter_error_and_margin_walk_at_full_size"),
    "ENC_CHUNK_ROWS": dict(default=1 << 22, tested_in=_ENC + "::test_encode_in_pieces_of_rows_equals_one_piece"),
    "ENC_STATS": dict(default=0, reason="counts the pairs that take the exact pass (rq_last_encode_stats); codes untouched"),
    "ROT_V2": dict(default=1, values=(0,), workload="rotate",
                   note="no readout of the rotation kernel: swept at d in {32, 64, 96, 128} only, where it selects rotate_kernel"),
    "ROT_WIDE2": dict(default=1, values=(0,), workload="rotate",
                      note="no readout of the rotation kernel: swept at d in {200, 784} only, where it selects rotate_wide_kernel"),
    # ---- row order (rq_order.hip) and when a call orders its base (rq_api.hip) ----
    "SCAN_ORDER": dict(default=1, values=(0, 2), workload="scan",
                       readout="orders"),
    "ORDER_MIN_ROWS": dict(default=65536, values=(1,), workload="scan",
                           readout="orders"),
    "ORDER_MIN_NQ": dict(default=2048, values=(1,), workload="scan",
                         readout="orders"),
    "ORDER_MAX_K": dict(default=8192, values=(1,), workload="scan",
                        readout="orders"),
    "ORDER_MAX_SCRATCH_MB": dict(default=2048, values=(1,), workload="scan_big",
                                 readout="orders", note="rq_scan_orders_in_call answers for rq_dev_linscan; the host-pointer call orders into an allocation of its own and ignores the limit (same answer)"),
    "ORDER_GREEDY": dict(default=1, values=(0,), workload="order",
                         readout="order_plan"),
    "ORDER_GREEDY_MIN_NQ": dict(default=16384, values=(1,), workload="scan_big",
                                readout="orders"),
    "ORDER_TWO_LEVEL": dict(default=1, values=(0,), workload="order",
                            readout="order_plan"),
    "ORDER_CBITS": dict(default=0, values=(2, 4), workload="order",
                        readout="order_plan"),
    "ORDER_BITS": dict(default=0, values=(9, 20), workload="order",
                       readout="order_plan"),
    "ORDER_GRAN": dict(default=0, values=(1024,), workload="order",
                       readout="order_plan"),
    "ORDER_SHUFFLE": dict(default=1, values=(0,), workload="order",
                          note="no readout: moves granules of the ordered base, not its key; permutation + oracle checks only"),
    "ORDER_SAMPLE_STRIDE": dict(default=16, values=(0, 3), workload="order",
                                note="no readout: moves the arrival-order sample blocks, not the key; permutation + oracle checks only"),
    "INDEX_ORDER": dict(default=1, tested_in=_ORDER + "::test_index_handle_orders_its_shards"),
    # ---- scan planner and kernels (rq_scan.hip, rq_topk.h) ----
    "SCAN_SLICES": dict(default=0, values=(3,), workload="scan",
                        readout="plan"),
    "SCAN_MIN_ROWS": dict(default=16384, values=(1024, 1 << 20), workload="scan",
                          readout="plan"),
    "SCAN_TAIL_SLICES": dict(default=0, values=(1, 3), workload="scan_xcd",
                             readout="plan"),
    "SCAN_SPREAD": dict(default=0, values=(1,), workload="scan",
                        note="no readout: one workgroup per CU through the LDS request; the plan's grid only changes above 256 items"),
    "SCAN_SLACK": dict(default=0, values=(64,), workload="scan",
                       readout="plan"),
    "SCAN_SAMPLE": dict(default=-1, values=(0, 256), workload="scan",
                        note="-1 = unset: 16384 rows, the retune samples SCAN_SAMPLE_RT; a value > 0 rules both samples",
                        readout="stats:sample_rows"),
    "SCAN_SAMPLE_RT": dict(default=4096, values=(64, 16384), workload="scan",
                           note="no readout: a parameter inside the scan kernel, checked against the oracle only"),
    "SCAN_SRANK_MUL": dict(default=2, values=(0,), workload="scan",
                           note="no readout: a parameter inside the scan kernel, checked against the oracle only"),
    "SCAN_RETUNE_Z": dict(default=6, values=(-8,), workload="scan",
                          note="no readout: a parameter inside the scan kernel, checked against the oracle only"),
    "SCAN_RETUNE_MIN_K": dict(default=1, values=(1 << 20,), workload="scan",
                              note="no readout: a parameter inside the scan kernel, checked against the oracle only"),
    "SCAN_RETUNE_DIV": dict(default=8, values=(2, 64), workload="scan",
                            note="no readout: a parameter inside the scan kernel, checked against the oracle only"),
    "SCAN_FILTER": dict(default=1, values=(0,), workload="scan",
                        readout="kernel"),
    "SCAN_FILTER_LSQ": dict(default=1, tested_in=_FUZZ + "::test_lsq_prefilter_on_hostile_tables"),
    "SCAN_FINE_MIN_K": dict(default=0, tested_in=_FUZZ + "::test_scan_prefilter_on_hostile_tables"),
    "SCAN_BUCKET_FINISH": dict(default=1, values=(0, 2), workload="scan_hostile",
                               readout="stats:bf_items", note="the counter tells 0 from 1 / 2 only; 2 (kept keys in global memory) has no readout"),
    "SCAN_SS_MAP": dict(default=1, values=(0,), workload="scan_hostile",
                        note="no readout: a parameter inside the scan kernel, checked against the oracle only"),
    "SCAN_SS_MIN_K": dict(default=1024, values=(50, 999, 4096), workload="scan_hostile",
                          readout="plan"),
    "SCAN_XCD": dict(default=1, values=(0,), workload="scan_xcd",
                     readout="plan"),
    "SCAN_XCD_MIN_MB": dict(default=0, tested_in=_SCAN + "::test_xcd_window_plan_on_a_small_base"),
    "SCAN_WINDOW_MB": dict(default=0, tested_in=_SCAN + "::test_xcd_window_plan_on_a_small_base"),
    "SCAN_XCD_SLACK": dict(default=-1, tested_in=_SCAN + "::test_xcd_window_plan_on_a_small_base"),
    "SCAN_XCD_ROUND": dict(default=0, values=(1, 3), workload="scan_xcd",
                           note="no readout: the pacing round of the XCD plan (the plan is asserted to stay the XCD plan)"),
    "SCAN_STATS": dict(default=0, reason="fills the finish / fallback counters of rq_scan_finish_stats; results untouched"),
    # ---- host-pointer calls (rq_api.hip) ----
    "HOST_DIRECT": dict(default=1, values=(0,), workload="host",
                        note="no readout: how results reach the host arrays; compared with the default call and the oracle"),
    "HOST_CHUNK": dict(default=4096, values=(1, 7), workload="host",
                       note="no readout; clamped to >= 256 queries per chunk: 1 and 7 both give 256-query chunks of the 600"),
    "HOST_OVERLAP": dict(default=1, values=(0,), workload="host",
                         note="no readout: how results reach the host arrays; compared with the default call and the oracle"),
    "HOST_DIRECT_MAX_MB": dict(default=0, tested_in=_POOL + "::test_large_results_take_the_chunked_copy_path"),
    "HOST_PIN": dict(default=1, tested_in=_POOL + "::test_large_results_are_pinned_and_correct"),
    "HOST_PIN_MAX_MB": dict(default=0, reason="cap of the page-locked pool; over it an ordinary array is used (same values)"),
    "HOST_PIN_POOL_MB": dict(default=0, reason="idle page-locked bytes kept for reuse: a pool size, not a computation"),
    "HOST_CACHE_MB": dict(default=2048, reason="device cache of uploaded host arrays: a pool size, not a computation"),
    "HOST_CACHE_MAX_MB": dict(default=256, reason="largest array the upload cache keeps: a pool size, not a computation"),
    # ---- index handles, several GPUs (rq_index.hip) ----
    "IDX_QCHUNKS": dict(default=0, tested_in=_INDEX + "::test_query_chunk_pipeline"),
    "EXCHANGE_SELFTEST": dict(default=0, tested_in=_INDEX + "::test_rccl_transport_selftest_on_one_gpu"),
    "EXCHANGE_PEER": dict(default=0, reason="peer copies between GPUs instead of RCCL: needs more than one physical GPU"),
    "EXCHANGE_CHUNK_RCCL": dict(default=0, reason="RCCL chunking of the shard exchange: needs more than one physical GPU"),
    "SHARDED_CACHE": dict(default=1, reason="keeps the stock calls' sharded index between calls: a cache, not a computation"),
    # ---- training (rq_train.hip, rq_train_host.hip) ----
    "TRAIN_FUSED_CB": dict(default=1, values=(0,), workload="train_opq",
                           note="no readout: the training loop materialises the reconstruction instead; tolerance check"),
    "TRAIN_CENTERS_MFMA": dict(default=1, tested_in=_TRAIN + "::test_update_centers_kernels_agree"),
    "GRAM_WAVES_PER_CU": dict(default=8, values=(1, 3), workload="train",
                              note="no readout: the grid of the gram kernel; tolerance check against float64"),
    "TRAIN_NS_BIG_D": dict(default=384, values=(64,), workload="polar",
                           note="no readout: the 64 x 64-tile Newton-Schulz kernel at d = 96; tolerance check against LAPACK"),
    "TRAIN_NS_L0_MICRO": dict(default=1000, values=(100, 100000), workload="polar",
                              note="no readout: the first scaling of Newton-Schulz; tolerance check against LAPACK"),
    "TRAIN_GPU_POLAR": dict(default=1, tested_in=_TRAIN + "::test_train_opq_newton_schulz_and_jacobi_agree"),
    "TRAIN_KMPP": dict(default=1, tested_in=_TRAIN + "::test_train_pq_with_kmeanspp_beats_uniform_seeding_on_clustered_data"),
    "TRAIN_DETERMINISTIC": dict(default=1, values=(0,), workload="train_opq",
                                note="no readout; 0 may give a bitwise different factorisation: tolerance check only"),
    "TRAIN_PROFILE": dict(default=0, reason="per-phase clock of rq_train_profile; one synchronisation per phase, results untouched"),
}


def swept():
    """(key, value, workload) for every value of every swept switch."""
    return [(k, v, e["workload"]) for k, e in sorted(SWITCHES.items()) if "values" in e for v in e["values"]]


def default(key):
    return SWITCHES[key]["default"]


@contextlib.contextmanager
def switches(**kv):
    """Set switches for a block; on exit every one of them is RESET (the environment / code default rules again)."""
    from rayuela_jl_amd import _lib
    unknown = sorted(set(kv) - set(SWITCHES))
    if unknown:
        raise KeyError("not a switch of the library: %s" % unknown)
    try:
        for k, v in kv.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k in kv:
            _lib.reset_tuning(k)
