// rq_scan_cfg.h -- what the two halves of the ADC scan share: the tiling constants (ScanCfg<M>), their run-time view for the
// host (ScanTiling), the per-item LDS state (ScanCtrl) and the kernel's parameter block (ScanParams).
// rq_scan.hip holds the kernel and names its instantiations; rq_scan_plan.hip holds the planner, the launch set-up and the small
// kernels around the scan.
#pragma once
#include "rq_internal.h"
#include "rq_topk.h"

namespace rq {

constexpr int SCAN_THREADS = 512;       // two workgroups per CU (ScanCfg<M>::THREADS is 1024 where one group needs more than half of the LDS)

// Experiments that did not ship (history: git log): 16 queries per 16-byte gather at m = 8 (one
// 1024-thread workgroup per CU; correct and slower: k = 1 2.25 vs 2.01 ms, k = 1000 3.28 vs 2.46 -- a 16-byte entry costs
// four adds, the wider accumulators spill), exact re-evaluation of whole rows instead of (row, query) pairs, all tables in
// LDS (no L1-gathered part), other block / vote periods.
template <int M>
struct ScanCfg {
  // queries per LDS gather: a float4 entry (ds_read_b128) up to m = 32; m = 64 only fits the 160 KiB of
  // LDS with float2 entries (ds_read_b64, 2 queries per gather)
  static constexpr int QPG = (M <= 32) ? 4 : 2;
  static constexpr int QG = (M <= 16) ? 8 : (M <= 32) ? 4 : 2;   // queries per group
  static constexpr int NQUAD = QG / QPG;                         // gathers per code byte
  // rows per thread per sub-step: ~32 gathers' worth, and a whole number of 16-byte code loads
  static constexpr int RPT = (32 / (M * NQUAD)) > (M < 16 ? 16 / M : 1) ? 32 / (M * NQUAD) : (M < 16 ? 16 / M : 1);
  // threads per workgroup: two 512-thread workgroups per CU, or ONE of 1024 where a group's tables take more than half of
  // the LDS (m = 16: 96 KiB of f32 tables + 32 KiB of byte tables; m = 32, 64: 112 KiB of f32 tables) -- the same 16
  // wavefronts per CU either way (m = 32 exact scan 27.1 -> 24.6 ms against one 512-thread workgroup per CU)
  static constexpr int THREADS = (M * QG >= 128) ? 1024 : SCAN_THREADS;
  static constexpr int SUB = THREADS * RPT;    // rows per sub-step (one 16/32-byte load per lane)
  static constexpr int U = (M <= 8) ? 8 : (M <= 16) ? 4 : (M <= 32) ? 2 : 1;  // sub-steps per block: loads of a block fly together
  static constexpr int BLK = SUB * U;               // rows per workgroup block
  // blocks between two capacity votes (the only barrier of the streaming loop): one vote per ~32768 rows.  Measured at
  // SIFT1M shape, votes every 1 / 2 / 4 / 8 blocks: k = 1 2.13 / 2.05 / 2.00 / 1.99 ms, k = 1000 2.62 / 2.62 / 2.46 / 2.44;
  // the candidate buffers grow by 2 * VP * BLK keys (a slow wavefront may still be appending the previous period's rows)
  static constexpr int VP = (32768 / BLK) < 1 ? 1 : (32768 / BLK) > 8 ? 8 : (32768 / BLK);
  static constexpr int LUT_BYTES = M * QG * 1024;   // full table; the LDS part is LUT_LDS_BYTES below
  // The LDS gather pipe is the kernel's bound (~11-12 cycles per 64-lane ds_read_b128 with random
  // slots).  The vector-memory path can gather the same 16 bytes from an L1-resident table in ~29
  // cycles per wavefront (tools/micro/gather_l1.hip) and runs beside the LDS, so the LAST KG
  // sub-quantizers (~25 % of the gathers, <= 16 KiB of table) are looked up through L1 instead.
  static constexpr int KG = (M == 8) ? 2 : (M == 16) ? 4 : (M == 32) ? 4 : (M == 4) ? 1 : 0;   // M = 64: all in LDS
  static constexpr int KL = M - KG;                 // sub-quantizers [0, KL) gather from LDS
  static constexpr int GTAB_F4 = KG * NQUAD * 256;  // entries (float4 for QPG = 4) of the global (L1) table
  static constexpr int LUT_LDS_BYTES = KL * QG * 1024;
  // integer pre-filter (see build_qtab): one byte per (sub-quantizer, code, query); tiled for M = 8 and 16
  static constexpr bool HAS_FILT = (M == 4 || M == 8 || M == 16) && SCAN_THREADS == 512;     // (the default build; m = 4 since round 6: PQ / CQ tables only)
  // byte accumulator sets: 8 sub-quantizers each; m = 8 in FINE mode: two sets of 4 with 6-bit entries (half the step)
  static constexpr int NACC = HAS_FILT ? (M == 8 ? 2 : M >= 8 ? M / 8 : 1) : 1;
  static constexpr int kpa(bool fine) { return (M == 8 && fine) ? 4 : 8; }   // sub-quantizers per accumulator set
  static constexpr int QTAB_BYTES = HAS_FILT ? (M + 1) * 256 * QG : 0;   // + 1: the row-norm table of LSQ scans
  // scratch behind the staged queries: the threshold sample's [QG][THREADS] minima, later the filter table
  static constexpr int AUX_BYTES = (QG * THREADS * 4 > QTAB_BYTES) ? QG * THREADS * 4 : QTAB_BYTES;
  static_assert(RPT >= 1, "M too large for this tiling");
};

template <int QG>
struct ScanCtrl {
  float tau[QG];
  uint32_t cnt[QG];
  uint32_t sel[QG];     // which half of the candidate ping-pong buffer is current
  uint32_t item;
  uint32_t selmask;     // bit q == sel[q] (one LDS word the hot loop reads per block)
  uint32_t pad[2];
  // integer pre-filter (FILT kernels): per-(sub-quantizer, query) table minima and the per-query scale
  float fmin[16][QG];
  float fmax[16][QG];   // LSQ scans: per-(sub-quantizer, query) max |entry| (absolute rounding margins)
  float finv[QG];
  uint32_t fpush;       // rows the pre-filter let through in the item's first block (it is switched off if too many)
  SelState<QG> st;      // st.hist doubles as the per-wavefront queues of rows waiting for the exact evaluation
};

struct ScanParams {
  const uint8_t *codes;     // [n][M]
  const float *centers;     // [M][256][sub]
  const float *queries;     // [nq][d]
  uint32_t n, nq;
  int sub, d, K;
  int m_real;               // sub-quantizers that exist; tables k >= m_real are all-zero padding
  int lut_mode;             // 0 PQ sub-space (c-q)^2 | 1 LSQ -2<q,c> full-dim | 2 CQ (q-c)^2 full-dim
  const float *row_bias;    // LSQ: dbnorms[n], added after the table sum; else nullptr
  const uint8_t *norm_bytes;  // LSQ pre-filter: row norms quantised to 256 lower edges, [n]
  const float *norm_info;     // ... {nmin, nstep, max |.|} of the quantised quantity: norm[row] - sum_k |c_k[b_k]|^2
  const float *cnorm;         // ... |c_k[r]|^2, [M][256]: folded into the filter's tables (see build_qtab)
  const uint32_t *perm;     // bank-aware row order (rq_order.hip): perm[position] = original row, read for survivors only; or nullptr
  uint32_t samp_end;        // ... below this position one block in every samp_stride is an arrival-order sample of the base
  uint32_t samp_stride;     //     (order_sample_rows, rq_order.hip); samp_end == 0: none
  uint32_t id_offset;
  int id_base;
  uint32_t nslices, rows_per_slice, ngroups;
  uint32_t whole;           // query groups [0, whole) are ONE item over all rows (answer written directly);
                            // groups [whole, ngroups) are cut into nslices row slices (key lists -> merge)
  uint32_t xcd_mode;        // 1: big base -- row windows are handed out per XCD (work_counter[0..7]), see the item loop
  uint32_t xcd_slack;       // ... an item may start while at most this many items of the XCD's earlier rounds still run
  uint32_t xcd_round;       // ... items per pacing round (a window's items, or the XCD's resident workgroups)
  uint32_t cap;             // candidate buffer capacity per query (keys)
  uint32_t trigger;         // compact when cnt > trigger  (cap - 2*VP*BLK >= trigger >= K)
  uint32_t p2;              // next_pow2(K)
  uint32_t scratch_keys;    // LDS sort scratch capacity in keys
  uint32_t sample;          // rows sampled per slice to initialise tau (0 = off)
  uint32_t sample_rt;       // ... for slices that get the second estimate (a looser first tau only rules 1/8 of the rows)
  uint32_t srank_mul;       // target survivors per slice = srank_mul * K (3; 0 forces the fallback, tests)
  int retune_z;             // second threshold estimate after 1/8 of the rows: rank = mean + z sigma (6; 0 = off; < 0: tests)
  int retune_min_k;         // ... only for K >= this
  int retune_div;           // ... after rows / retune_div rows (8)
  uint32_t *work_counter;
  float4 *gtab;               // [gridDim][GTAB_F4] L1-gathered part of the LUT
  unsigned long long *stats;  // optional [8]: cycles in lut, sample, stream, cuts, final cut, sort; #cuts; #fallbacks
  uint64_t *cand;           // [gridDim][QG][2][cap]
  uint16_t *bkt;            // [gridDim][cap] bucket ids of the large-K sample sort
  int filter;               // 1: 8-bit lower-bound pre-filter in front of the exact evaluation (FILT kernels)
  int bigk;                 // K > SCAN_SS_MIN_K: finish with samplesort_topk instead of cut + LDS bitonic (1: map buckets first, 2: sorted splitters only)
  int bfin;                 // K <= SCAN_SS_MIN_K: cut + sort per query by one wavefront through distance buckets (SCAN_BUCKET_FINISH)
  // outputs of whole items: dists/ids [nq][K], or packed keys [nq][K] when keys != nullptr;
  // of sliced items: part [(query - whole*QG)][nslices][K] packed keys
  float *dists;
  uint32_t *ids;
  uint64_t *keys;
  uint64_t *part;
};

// LSQ pre-filter, shared by build_qtab (rq_scan_filter.h) and the quantiser of a base's row norms (rq_scan_plan.hip):
// row norm -> its quantisation cell's LOWER edge, with exactly these two rounded operations (the quantiser checks its
// choice against the same expression, so EDGE(byte of a row) <= the row's norm holds in exact arithmetic)
__device__ __forceinline__ float norm_edge(float nmin, float nstep, uint32_t b) {
  const float t = (float)b * nstep;
  return nmin + t;
}

// ScanCfg<M> as values: what the planner, the launch's LDS sizing and the row order read.  CTRL_BYTES: ScanCtrl<QG>, 16-byte padded.
struct ScanTiling {
  int QG, QPG, RPT, THREADS, BLK, VP, LUT_LDS_BYTES, AUX_BYTES, GTAB_F4;
  bool HAS_FILT;
  int CTRL_BYTES;
};

// fn(std::integral_constant<int, M>) for a tiled row width (scan_padded_m); false, and nothing called, for any other mp.
// The only place that spells the widths out: the tiling below and the kernel launch (rq_scan.hip) go through it.
template <class F>
inline bool by_scan_width(int mp, F fn) {
  switch (mp) {
    case 2: fn(std::integral_constant<int, 2>{}); return true;
    case 4: fn(std::integral_constant<int, 4>{}); return true;
    case 8: fn(std::integral_constant<int, 8>{}); return true;
    case 16: fn(std::integral_constant<int, 16>{}); return true;
    case 32: fn(std::integral_constant<int, 32>{}); return true;
    case 64: fn(std::integral_constant<int, 64>{}); return true;
  }
  return false;
}

// (ScanCtrl<ScanCfg<M>::QG> spelled as the kernel's helpers spell it: clang mangles their parameter lists with the FIRST spelling
// of this dependent type it meets, and `Cfg::QG` here would rename every out-of-line device function of the kernel)
template <int M>
constexpr ScanTiling scan_tiling_of() {
  using Cfg = ScanCfg<M>;
  return {Cfg::QG, Cfg::QPG, Cfg::RPT, Cfg::THREADS, Cfg::BLK, Cfg::VP, Cfg::LUT_LDS_BYTES, Cfg::AUX_BYTES, Cfg::GTAB_F4,
          Cfg::HAS_FILT, (int)((sizeof(ScanCtrl<ScanCfg<M>::QG>) + 15) & ~15)};
}
inline bool scan_tiling(int mp, ScanTiling *t) {
  return by_scan_width(mp, [&](auto M) { *t = scan_tiling_of<decltype(M)::value>(); });
}

// rq_scan.hip: picks the adc_scan_kernel instantiation for row width mp and launches it over plan.grid workgroups; fills the
// fields of p that depend on the tiling (samp_end, samp_stride; filter = 0 where the width has no pre-filter)
RQ_LOCAL int scan_kernel_launch(int mp, ScanParams &p, const ScanPlan &plan, hipStream_t stream);

}  // namespace rq
