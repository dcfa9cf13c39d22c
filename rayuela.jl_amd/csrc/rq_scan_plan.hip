// rq_scan_plan.hip -- the host half of the ADC scan and the small kernels around it.
//
// The planner (scan_plan: work items, slices, XCD windows, buffer sizes), the launch set-up (scan_launch: fills ScanParams and
// hands them to scan_kernel_launch of rq_scan.hip, which holds the kernel), the merge of per-slice key lists, the LSQ
// pre-filter's preparation of a base, the tiling the row order has to match, and the pad / LUT / synth helpers.
#include "rq_internal.h"
#include "rq_topk.h"

#include "rq_scan_cfg.h"

namespace rq {

// ------------------------------------------------------------------------------------------
// Merge P sorted key lists per query (slices of one GPU and/or shards of several GPUs).
// One 256-thread workgroup per query: radix-select the K-th key over the P*K keys in global
// memory, pull the K survivors into LDS, sort, write.
// ------------------------------------------------------------------------------------------
constexpr int MERGE_THREADS = 256;

struct MergeParams {
  const uint64_t *keys_in;  // [nq][P][K]
  uint32_t nq, P;
  int K, id_base;
  int use_map;              // large K: buckets from the distance map first (SCAN_SS_MAP)
  uint32_t p2;
  float *dists;
  uint32_t *ids;
  uint64_t *keys_out;
};

struct MergeCtrl {
  SelState<1> st;
};

__global__ __launch_bounds__(MERGE_THREADS) void merge_topk_kernel(MergeParams p) {
  constexpr int CTRL_BYTES = (sizeof(MergeCtrl) + 15) & ~15;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  MergeCtrl *ctrl = reinterpret_cast<MergeCtrl *>(smem);
  uint64_t *a = reinterpret_cast<uint64_t *>(smem + CTRL_BYTES);
  const int tid = threadIdx.x;
  const uint32_t q = blockIdx.x;
  const uint64_t *src = p.keys_in + (size_t)q * p.P * p.K;
  const uint32_t cnt = p.P * (uint32_t)p.K;
  for (uint32_t i = tid; i < p.p2; i += MERGE_THREADS) a[i] = KEY_MAX;
  uint32_t vseq = 0;
  if (tid < 2) ctrl->st.vote[tid] = 0;
  __syncthreads();
  radix_select<1, MERGE_THREADS>(&ctrl->st, src, cnt, (uint32_t)p.K, true, 0, tid, vseq);
  const uint64_t tau = ctrl->st.prefix[0];
  // survivors straight into LDS (padding keys equal to KEY_MAX never survive unless tau is one)
  if (tid == 0) ctrl->st.newcnt[0] = 0;
  __syncthreads();
  {
    const int lane = tid & 63;
    const uint32_t cnt_up = (cnt + 63u) & ~63u;
    for (uint32_t idx = tid; idx < cnt_up; idx += MERGE_THREADS) {
      const uint64_t key = idx < cnt ? src[idx] : KEY_MAX;
      const bool take = idx < cnt && key <= tau && key != KEY_MAX;
      const uint64_t mask = __ballot(take);
      if (mask) {
        const int leader = __ffsll((unsigned long long)mask) - 1;
        uint32_t basep = 0;
        if (lane == leader) basep = atomicAdd(&ctrl->st.newcnt[0], (uint32_t)__popcll(mask));
        basep = __builtin_amdgcn_readlane(basep, leader);
        if (take) {
          const uint32_t pos = basep + __popcll(mask & ((1ull << lane) - 1ull));
          if (pos < p.p2) a[pos] = key;
        }
      }
    }
  }
  __syncthreads();
  bitonic_sort_tiled(a, p.p2, MERGE_THREADS / 64, tid / 64, tid & 63, true);
  for (uint32_t i = tid; i < (uint32_t)p.K; i += MERGE_THREADS) {
    const uint64_t key = a[i];
    if (p.keys_out) p.keys_out[(size_t)q * p.K + i] = key;
    if (p.dists) p.dists[(size_t)q * p.K + i] = key_dist(key);
    if (p.ids) p.ids[(size_t)q * p.K + i] = key_id(key) + (uint32_t)p.id_base;
  }
}

// Large K: the same merge as a sample sort over the P*K keys (no K-sized LDS array).  Persistent
// 512-thread workgroups, each with P*K keys + P*K u16 of global scratch.
__global__ __launch_bounds__(SCAN_THREADS) void merge_topk_big_kernel(MergeParams p, uint64_t *scratch, uint16_t *bkt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t cnt = p.P * (uint32_t)p.K, K = (uint32_t)p.K, tid = threadIdx.x;
  uint64_t *dst = scratch + (size_t)blockIdx.x * cnt;
  uint16_t *b = bkt + (size_t)blockIdx.x * cnt;
  for (uint32_t q = blockIdx.x; q < p.nq; q += gridDim.x) {
    const uint64_t *src = p.keys_in + (size_t)q * cnt;
    uint64_t *ok = p.keys_out ? p.keys_out + (size_t)q * K : nullptr;
    float *od = p.dists ? p.dists + (size_t)q * K : nullptr;
    uint32_t *oi = p.ids ? p.ids + (size_t)q * K : nullptr;
    const uint32_t id_base = (uint32_t)p.id_base;
    auto emit = [ok, od, oi, id_base](uint32_t r, uint64_t key) {
      if (ok) ok[r] = key;
      if (od) od[r] = key_dist(key);
      if (oi) oi[r] = key_id(key) + id_base;
    };
    const uint32_t got = samplesort_topk<SCAN_THREADS>(src, dst, b, cnt, K, smem, emit, nullptr, p.use_map != 0);
    for (uint32_t i = got + tid; i < K; i += SCAN_THREADS) emit(i, KEY_MAX);   // fewer than K real keys
  }
}

// P == 1: the list is already the answer, only unpack it
__global__ void unpack_keys_kernel(MergeParams p) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)p.nq * p.K) return;
  const uint64_t key = p.keys_in[i];
  if (p.keys_out) p.keys_out[i] = key;
  if (p.dists) p.dists[i] = key_dist(key);
  if (p.ids) p.ids[i] = key_id(key) + (uint32_t)p.id_base;
}

// Stand-alone LUT kernel (test aid, rq_dev_adc_lut): lut[q][k][r], one thread per (q,k,r).
__global__ void adc_lut_kernel(float *lut, const float *centers, const float *queries, uint32_t nq,
                               int m, int sub) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per_q = (size_t)m * 256;
  if (e >= per_q * nq) return;
  const size_t q = e / per_q;
  const int t = (int)(e - q * per_q);
  const int k = t >> 8;
  const float *c = centers + (size_t)t * sub;
  const float *qv = queries + q * (size_t)(m * sub) + (size_t)k * sub;
  float acc = 0.0f;
  for (int s = 0; s < sub; ++s) {
    const float diff = c[s] - qv[s];
    const float sq = diff * diff;
    acc = acc + sq;
  }
  lut[e] = acc;
}

// codes [n][m] -> [n][mp] with zero padding bytes (m not one of the tiled widths)
__global__ void pad_codes_kernel(uint8_t *dst, const uint8_t *src, size_t n, int m, int mp) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * (size_t)mp) return;
  const size_t r = e / mp;
  const int k = (int)(e - r * mp);
  dst[e] = k < m ? src[r * m + k] : (uint8_t)0;
}

__global__ void synth_codes_kernel(uint8_t *codes, size_t nbytes, uint64_t seed, uint64_t e0) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i >= nbytes) return;
  uint64_t out = 0;
  const int lim = (int)((nbytes - i) < 8 ? (nbytes - i) : 8);
  for (int b = 0; b < lim; ++b) {
    uint64_t z = ((e0 + i + b) ^ seed) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    out |= (z >> 56) << (8 * b);
  }
  if (lim == 8) *reinterpret_cast<uint64_t *>(codes + i) = out;
  else for (int b = 0; b < lim; ++b) codes[i + b] = (uint8_t)(out >> (8 * b));
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// t: the tiling of row width M (scan_tiling)
static void plan_for(ScanPlan &pl, const ScanTiling &t, int M, int64_t n, int64_t nq, int d, int K, int num_cu, int force_slices) {
  const int CTRL_BYTES = t.CTRL_BYTES;
  pl.qg = t.QG;
  pl.blk = t.BLK;
  pl.ngroups = (uint32_t)((nq + t.QG - 1) / t.QG);
  // slack between cuts: with the sampled tau about 2-3K rows survive a slice, so a slack of 4K means
  // "no cut before the end"; the exact fallback (tau from +inf) cuts every `slack` survivors.
  int slack_i = tuning("SCAN_SLACK", 0);
  if (slack_i <= 0) slack_i = std::max(std::min(std::max(4 * K, 2048), 16384), K + K / 2);
  const uint32_t slack = (uint32_t)slack_i;
  pl.trigger = (uint32_t)K + slack;
  // SCAN_SAMPLE: -1 = unset (16384 rows; the retune samples SCAN_SAMPLE_RT), 0 = no sampled threshold, > 0 rules both samples
  const int sample = tuning("SCAN_SAMPLE", -1);
  pl.sample = sample < 0 ? 16384u : (uint32_t)sample;
  // + 2048: rows waiting in the pre-filter's queues (< 128 per wavefront) are appended outside their block
  pl.cap = pl.trigger + 2 * t.VP * t.BLK + 2048;
  pl.p2 = next_pow2((uint32_t)K);
  // large K finishes with the global-memory sample sort: its LDS need does not grow with K
  pl.bigk = K > tuning("SCAN_SS_MIN_K", 1024);
  // LDS scratch for the final sort: at least one query, at most QG, within 160 KiB total
  const size_t lds_max = 160 * 1024 - CTRL_BYTES;
  size_t want_keys = (size_t)pl.p2 * t.QG;
  size_t base_keys = ((size_t)t.LUT_LDS_BYTES + (size_t)t.QG * d * 4 + t.AUX_BYTES) / 8;
  size_t keys = std::max(base_keys, std::min(want_keys, (size_t)64 * 1024 / 8 * 2));
  keys = std::max(keys, (size_t)pl.p2);
  if (pl.bigk) keys = std::max(base_keys, (size_t)(SS_LDS_BYTES + 7) / 8);
  keys = std::min(keys, lds_max / 8);
  pl.scratch_keys = (uint32_t)keys;
  // workgroups per CU: as many as the LDS request admits (2 x 512 threads when it is <= 80 KiB)
  const size_t lds_req = CTRL_BYTES + std::max<size_t>(base_keys * 8, (size_t)pl.scratch_keys * 8);
  const int wgs = std::max(1, std::min<int>(1024 / t.THREADS, (int)(160 * 1024 / lds_req)));
  // Work items = (8-query group, row range), handed out by an atomic counter to the resident workgroups
  // (2 per CU).  Per item there is a fixed cost (LUT, threshold sample, select + sort, and a merge pass for
  // sliced groups), so whole-base items are best whenever they fill the chip:
  //  * fewer groups than resident workgroups: every group is cut into slots/groups row slices
  //    (1000 queries, K = 1000: 4 slices 1.11 ms; 1, 2, 6, 9 slices 1.85, 1.18, 1.37, 1.64 ms);
  //  * otherwise whole items, except a small last partial round: when the groups beyond a multiple of
  //    num_cu are at most num_cu/2 they are cut in two, so that they occupy twice as many CUs for half
  //    as long (5000 queries: 3.71 -> 3.05 ms, 7000: 4.76 -> 4.10 ms; with a larger remainder, or finer
  //    cuts, the per-item cost wins: 10000 queries 5.80 -> 5.91 ms, so those stay whole).
  int64_t min_rows = std::max<int64_t>(tuning("SCAN_MIN_ROWS", 16384), 32LL * K);
  min_rows = (min_rows + t.BLK - 1) / t.BLK * t.BLK;
  const int64_t max_slices = std::max<int64_t>(1, n / min_rows);
  const int64_t U = num_cu, slots = (int64_t)num_cu * wgs;
  int64_t whole = 0, tail = pl.ngroups, ns = 1;
  if ((int64_t)pl.ngroups < slots) {
    ns = std::min<int64_t>(std::max<int64_t>(1, slots / pl.ngroups), max_slices);
  } else {
    whole = (pl.ngroups / U) * U;
    tail = pl.ngroups - whole;
    if (tail > 0 && 2 * tail <= U && max_slices >= 2) ns = 2;
  }
  const int tail_ns = tuning("SCAN_TAIL_SLICES", 0);           // experiments: slices of the tail groups only
  if (tail_ns > 0 && tail > 0) ns = std::min<int64_t>(tail_ns, max_slices);
  if (force_slices > 0) { ns = force_slices; whole = 0; }   // tests: every group sliced
  // Big bases (code array >= SCAN_XCD_MIN_MB, far beyond the 8 x 4 MiB of L2): short row windows, handed out per XCD
  // (adc_scan_kernel: xcd_mode).  A window is SCAN_WINDOW_MB of codes: small enough that the workgroups of an XCD
  // that started it together are still within L2 reach of each other at its end (their speeds differ by a few percent),
  // large enough that the per-item work (tables, threshold sample, final select + sort) stays around one percent.  Bounds: the per-slice
  // key lists (nq * ns * K * 8 bytes) stay below 1 GiB and a query's merge below 2^20 keys.
  pl.xcd = false;
  // the window hand-out and its pacing are written for the 8 XCDs x 32 CUs of an MI355X in SPX mode (xcd & 7, grid / 8); a
  // partitioned device (CPX / DPX: fewer XCDs behind one agent) takes the plain planner -- results are the same either way
  const bool eight_xcds = num_cu == 256 || tuning("SCAN_XCD", 1) > 1;
  if (force_slices <= 0 && tail_ns <= 0 && tuning("SCAN_XCD", 1) && eight_xcds &&
      (int64_t)n * M >= ((int64_t)(tuning("SCAN_XCD_MIN_MB", 0) > 0 ? tuning("SCAN_XCD_MIN_MB", 0) : 128) << 20)) {
    int64_t wrows = ((int64_t)(tuning("SCAN_WINDOW_MB", 0) > 0 ? tuning("SCAN_WINDOW_MB", 0) : 32) << 20) / M;
    wrows = std::max<int64_t>(wrows, min_rows);
    int64_t nw = (n + wrows - 1) / wrows;
    // per-window key lists: at most 256 MB of scratch per (device, stream) (1 GiB x 8 streams was ~10 GiB hidden)
    const int64_t cap_part = ((int64_t)256 << 20) / std::max<int64_t>(1, nq * (int64_t)K * 8);
    const int64_t cap_merge = ((int64_t)1 << 20) / std::max(1, K);
    nw = std::min(nw, std::min(cap_part, cap_merge));
    if (nw >= 16) { ns = nw; whole = 0; pl.xcd = true; }
  }
  if (ns == 1) whole = pl.ngroups;
  int64_t rps = (n + ns - 1) / ns;
  rps = (rps + t.BLK - 1) / t.BLK * t.BLK;
  ns = (n + rps - 1) / rps;
  if (ns == 1) whole = pl.ngroups;
  if (ns < 16) pl.xcd = false;
  pl.nslices = (uint32_t)ns;
  pl.rows_per_slice = (uint32_t)rps;
  pl.whole = (uint32_t)whole;
  const uint64_t items = (uint64_t)pl.whole + (uint64_t)(pl.ngroups - pl.whole) * pl.nslices;
  // experiment knob: one workgroup per CU (made no difference for small grids -- the dispatcher already
  // spreads them -- and costs 24 % at 4096 queries, so it is off)
  pl.spread = tuning("SCAN_SPREAD", 0) > 0;
  pl.grid = (uint32_t)std::min<uint64_t>(items, (uint64_t)num_cu * (pl.spread ? 1 : wgs));
  pl.cand_bytes = (size_t)pl.grid * t.QG * 2 * pl.cap * sizeof(uint64_t);
  pl.gtab_off = pl.cand_bytes;   // the L1-gathered LUT parts live behind the candidate buffers
  pl.cand_bytes += (size_t)pl.grid * (t.GTAB_F4 > 0 ? t.GTAB_F4 : 1) * sizeof(float4);
  pl.bkt_off = pl.cand_bytes;
  if (pl.bigk) pl.cand_bytes += ((size_t)pl.grid * pl.cap * sizeof(uint16_t) + 15) & ~(size_t)15;
  pl.lds_ok = (pl.bigk || (size_t)pl.p2 * 8 <= lds_max) &&
              ((size_t)t.LUT_LDS_BYTES + (size_t)t.QG * d * 4 + t.AUX_BYTES <= lds_max);
}

int scan_padded_m(int m) {
  for (int mp : {2, 4, 8, 16, 32, 64})
    if (m <= mp) return mp;
  return -1;
}

int scan_plan(ScanPlan &pl, int64_t n, int64_t nq, int m, int d, int K, int num_cu, int force_slices) {
  m = scan_padded_m(m);
  ScanTiling t;
  if (!scan_tiling(m, &t)) return fail(RQ_EUNSUPPORTED, "the ADC scan kernels cover 1 <= m <= 64 sub-quantizers");
  plan_for(pl, t, m, n, nq, d, K, num_cu, force_slices);
  if (!pl.lds_ok) return fail(RQ_EUNSUPPORTED, "k=%d / d=%d does not fit the 160 KiB LDS plan", K, d);
  return RQ_OK;
}

// ---- LSQ pre-filter: the rows' norms as one byte each (the "code" of the row-norm table, see build_qtab) -----------
// info (uint32 view): [0] ordered(min), [1] ordered(max); (float view) [4] nmin, [5] nstep, [6] max |norm|
// rho(row) = norm(row) - sum_k cn[k][b_k], in float64 (exact for f32 inputs up to m = 16) and rounded DOWN to f32
__global__ void norm_residual_kernel(const float *__restrict__ nrm, const uint8_t *__restrict__ codes, uint32_t n, int mrow,
                                     int mreal, const float *__restrict__ cn, float *rho) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    double s = (double)nrm[i];
    for (int k = 0; k < mreal; ++k) s -= (double)cn[k * 256 + codes[(size_t)i * mrow + k]];
    rho[i] = __double2float_rd(s);
  }
}

// Range of the COMPARABLE residual norms.  A NaN rho (a NaN norm of either sign, Inf - Inf, a NaN codebook entry) is left out:
// f2ord is an order for NaN-free inputs only -- a NaN with the sign bit clear would sort above +Inf, one with the sign bit set
// below -Inf.  Such a row's distance is NaN (never a neighbour, whatever the filter says) unless the NaN came from Inf - Inf
// against an infinite |c|^2, which switches the filter off (build_qtab).
__global__ void norm_minmax_kernel(const float *__restrict__ nrm, uint32_t n, uint32_t *info) {
  uint32_t lo = 0xffffffffu, hi = 0u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float v = nrm[i];
    if (v != v) continue;
    const uint32_t o = f2ord(v + 0.0f);
    lo = min(lo, o);
    hi = max(hi, o);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, off));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, off));
  }
  if ((threadIdx.x & 63) == 0) { atomicMin(&info[0], lo); atomicMax(&info[1], hi); }
}

// {nmin, nstep, max |rho|} over the rows norm_minmax_kernel counted.  What build_qtab relies on: nmin <= rho(row) and
// max |rho| >= |rho(row)| for every row with a comparable rho.  An infinite rho makes max |rho| infinite, which switches the
// filter off for every query (build_qtab: A < +Inf); no comparable rho at all (info still holds the start values) gives zeros.
__global__ void norm_info_kernel(uint32_t *info) {
  float *f = reinterpret_cast<float *>(info);
  const bool none = info[0] > info[1];
  const float nmin = none ? 0.0f : ord2f(info[0]), nmax = none ? 0.0f : ord2f(info[1]);
  float nstep = (nmax - nmin) / 255.0f;
  if (!(nstep > 0.0f) || !(nstep < __uint_as_float(0x7f800000u))) nstep = 0.0f;   // constant norms (or not finite): one cell
  f[4] = nmin;
  f[5] = nstep;
  f[6] = fmaxf(fabsf(nmin), fabsf(nmax));
}

__global__ void norm_quant_kernel(const float *__restrict__ nrm, uint32_t n, const uint32_t *info, uint8_t *nb) {
  const float *f = reinterpret_cast<const float *>(info);
  const float nmin = f[4], nstep = f[5];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float v = nrm[i];
    uint32_t b = 0;                 // (a NaN rho stays in cell 0: every comparison below is false)
    if (nstep > 0.0f) {
      const float t = (v - nmin) / nstep;
      b = t >= 255.0f ? 255u : t > 0.0f ? (uint32_t)t : 0u;
      while (b > 0 && !(norm_edge(nmin, nstep, b) <= v)) --b;     // the cell's lower edge must not exceed the norm
    }
    nb[i] = (uint8_t)b;
  }
}

// LSQ pre-filter preprocessing of a base (O(n), independent of the queries): |c|^2 of the codebooks, the rows' cross-term
// norms rho = norm - sum_k |c_k[b_k]|^2 (float64, rounded down), their range and one byte per row.
// norm_buf: [n rounded up to 64] row bytes | 8 words of info | |c|^2 [16][256] f32 | rho [n] f32   (lsq_norm_bytes)
size_t lsq_norm_bytes(int64_t n) { return (((size_t)n + 63) & ~(size_t)63) + 32 + 16 * 256 * 4 + (size_t)n * 4; }

int lsq_norm_prepare(uint8_t *norm_buf, const uint8_t *codes, const float *centers, const float *row_bias, int64_t n,
                     int mp, int m_real, int d, hipStream_t stream) {
  const size_t nb_bytes = ((size_t)n + 63) & ~(size_t)63;
  uint32_t *info = reinterpret_cast<uint32_t *>(norm_buf + nb_bytes);
  float *cn = reinterpret_cast<float *>(info + 8);
  float *rho = cn + 16 * 256;
  RQ_HIP(hipMemsetAsync(info, 0xff, 4, stream));
  RQ_HIP(hipMemsetAsync(info + 1, 0, 4, stream));
  RQ_HIP(hipMemsetAsync(cn, 0, 16 * 256 * 4, stream));       // padding tables (m_real < m): |c|^2 = 0
  const uint32_t grid = (uint32_t)std::min<int64_t>(2048, (n + 255) / 256);
  // |c_k[r]|^2 of the full-dimensional codebooks [m_real][256][d] (any rounding will do: the residual below uses these values)
  RQ_TRY(icm_sqnorm_launch(cn, centers, m_real, 256, d, stream));
  hipLaunchKernelGGL(norm_residual_kernel, dim3(grid), dim3(256), 0, stream, row_bias, codes, (uint32_t)n, mp, m_real, cn, rho);
  hipLaunchKernelGGL(norm_minmax_kernel, dim3(grid), dim3(256), 0, stream, (const float *)rho, (uint32_t)n, info);
  hipLaunchKernelGGL(norm_info_kernel, dim3(1), dim3(1), 0, stream, info);
  hipLaunchKernelGGL(norm_quant_kernel, dim3(grid), dim3(256), 0, stream, (const float *)rho, (uint32_t)n, info, norm_buf);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

int scan_launch(const ScanPlan &pl, const ScanCall &c, hipStream_t stream) {
  const int64_t n = c.n;
  const int d = c.d, K = c.K, lut_mode = c.lut_mode;
  const float *row_bias = c.row_bias;
  uint32_t *work_counter = c.work_counter;
  ScanParams p;
  p.perm = c.perm;
  p.samp_end = 0;           // set per row width (scan_kernel_launch): positions below it hold a sample block in every 16 (order_sample_stride())
  p.codes = c.codes; p.centers = c.centers; p.queries = c.queries;
  p.n = (uint32_t)n; p.nq = (uint32_t)c.nq; p.sub = d / c.m; p.d = d; p.K = K;
  p.m_real = c.m;
  const int m = scan_padded_m(c.m);   // `codes` already has this row width (dev_linscan pads when needed)
  p.lut_mode = lut_mode; p.row_bias = row_bias;
  p.id_offset = c.id_offset; p.id_base = c.id_base;
  p.nslices = pl.nslices; p.rows_per_slice = pl.rows_per_slice; p.ngroups = pl.ngroups; p.whole = pl.whole;
  p.xcd_mode = pl.xcd ? 1u : 0u;
  {
    // pacing round = the items of whole windows, at least as many as the XCD has resident workgroups (fewer would leave
    // workgroups idle); slack = a quarter of a round.  Measured at 1e9 rows x 8 bytes, 1024 queries, k = 100 (128 items per
    // window, 64 workgroups per XCD; round 2's plan: 191.7 ms, 599 GB fetched per launch = 75x the code bytes) and on the
    // 1.25e8-row shard that one of 8 GPUs holds (round 2: 23.85 ms, 60x):
    //   round 128, slack 0 / 8 / 24: 195.8 / 194.7 / 195.1 ms, 6.5x / 7.1x / 7.0x;   slack 32: 185.9 ms, 19x   <- shipped
    //   round  64, slack 0 / 16 / 32: 199.8 / 195.8 / 189.0 ms, 6.0x / 7.0x / 10.7x
    //   no pacing: 185.8 ms, 65x (the pack dissolves after a few windows)
    //   shard: round 128 / slack 32: 23.5 ms, 8.9x;  round 64 / slack 32: 24.5 ms, 7.9x;  slack 0: 24.3 ms, 6.7x
    // Tighter pacing fetches less and costs more idle time than the L2 hits give back; the shipped point is the one that is
    // faster than round 2 at both sizes.
    const uint32_t per_xcd = std::max(1u, pl.grid / 8u);
    const int rd = tuning("SCAN_XCD_ROUND", 0);
    p.xcd_round = rd > 0 ? (uint32_t)rd : pl.ngroups * ((per_xcd + pl.ngroups - 1u) / pl.ngroups);
    const int sl = tuning("SCAN_XCD_SLACK", -1);
    p.xcd_slack = sl >= 0 ? (uint32_t)sl : p.xcd_round / 4u;
  }
  p.cap = pl.cap; p.trigger = pl.trigger; p.p2 = pl.p2; p.scratch_keys = pl.scratch_keys;
  p.sample = pl.sample;
  p.sample_rt = (uint32_t)tuning("SCAN_SAMPLE_RT", 4096);
  if (tuning("SCAN_SAMPLE", -1) > 0) p.sample_rt = pl.sample;     // an explicit SCAN_SAMPLE rules both
  p.srank_mul = (uint32_t)tuning("SCAN_SRANK_MUL", 2);
  p.retune_z = tuning("SCAN_RETUNE_Z", 6);
  p.retune_min_k = tuning("SCAN_RETUNE_MIN_K", 1);
  p.retune_div = std::max(2, tuning("SCAN_RETUNE_DIV", 8));
  p.work_counter = work_counter; p.cand = c.cand;
  p.gtab = reinterpret_cast<float4 *>(reinterpret_cast<char *>(c.cand) + pl.gtab_off);
  p.bkt = reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(c.cand) + pl.bkt_off);
  p.bigk = pl.bigk ? (tuning("SCAN_SS_MAP", 1) ? 1 : 2) : 0;      // 2: sorted splitters only (tests, A/B)
  // the bucket finish needs BF_NB words of LDS per query of the group in the (dead) table space
  // (below k = 16 a query holds a few dozen candidates: select + sort of those costs 2.4 % of a k = 1 scan, the bucket finish's fixed
  // work -- counters, the look, two votes -- 4.0 %)
  p.bfin = (!pl.bigk && K >= 16 && (size_t)pl.scratch_keys * 8 >= (size_t)pl.qg * (BF_NB * 4 + 64)) ? tuning("SCAN_BUCKET_FINISH", 1) : 0;
  p.filter = (lut_mode != LUT_LSQ && !row_bias && tuning("SCAN_FILTER", 1)) ? 1 : 0;
  p.norm_bytes = nullptr; p.norm_info = nullptr; p.cnorm = nullptr;
  if (lut_mode == LUT_LSQ && row_bias && c.norm_buf && (m == 8 || m == 16) && tuning("SCAN_FILTER", 1) &&
      tuning("SCAN_FILTER_LSQ", 1)) {
    // the O(n) preprocessing of the base -- unless the caller holds a prepared base (rq_lsq_prepare: paid once, not per call)
    if (!c.norm_ready) RQ_TRY(lsq_norm_prepare(c.norm_buf, c.codes, c.centers, row_bias, n, m, p.m_real, d, stream));
    const size_t nb_bytes = ((size_t)n + 63) & ~(size_t)63;
    uint32_t *info = reinterpret_cast<uint32_t *>(c.norm_buf + nb_bytes);
    float *cn = reinterpret_cast<float *>(info + 8);
    p.norm_bytes = c.norm_buf;
    p.norm_info = reinterpret_cast<const float *>(info) + 4;
    p.cnorm = cn;
    p.filter = 1;
  }
  p.stats = tuning("SCAN_STATS", 0) ? reinterpret_cast<unsigned long long *>(work_counter + 16) : nullptr;
  p.dists = c.dists; p.ids = c.ids; p.keys = c.keys; p.part = c.part;
  RQ_HIP(hipMemsetAsync(work_counter, 0, p.stats ? 256 : 16 * sizeof(uint32_t), stream));   // [0..7] tickets, [8..15] finished items, per XCD
  return scan_kernel_launch(m, p, pl, stream);
}

int merge_launch(float *dists, uint32_t *ids, uint64_t *keys_out, const uint64_t *keys_in, int64_t nq,
                 int P, int K, int id_base, hipStream_t stream) {
  // K beyond the scan's cap (full rankings over shards): the bulk select + sort of rq_bulk.hip over the P * K keys
  if (P > 1 && K > RQ_MAX_K) return bulk_merge(dists, ids, keys_out, keys_in, nq, P, K, id_base, stream);
  MergeParams p;
  p.keys_in = keys_in; p.nq = (uint32_t)nq; p.P = (uint32_t)P; p.K = K; p.id_base = id_base;
  p.p2 = next_pow2((uint32_t)K);
  p.use_map = tuning("SCAN_SS_MAP", 1);
  p.dists = dists; p.ids = ids; p.keys_out = keys_out;
  if (P == 1) {
    const size_t total = (size_t)nq * K;
    hipLaunchKernelGGL(unpack_keys_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, p);
    RQ_HIP(hipGetLastError());
    return RQ_OK;
  }
  if (K > tuning("SCAN_SS_MIN_K", 1024)) {
    int dev = 0, num_cu = 256;
    RQ_HIP(hipGetDevice(&dev));
    RQ_HIP(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const uint32_t grid = (uint32_t)std::min<int64_t>(nq, 2LL * num_cu);
    const size_t per_wg = (size_t)P * K;
    void *ws = nullptr;
    RQ_TRY(workspace(WS_MERGE, (size_t)grid * per_wg * (sizeof(uint64_t) + sizeof(uint16_t)) + 16, &ws, stream));
    uint64_t *scratch = (uint64_t *)ws;
    uint16_t *bkt = (uint16_t *)(scratch + (size_t)grid * per_wg);
    RQ_LAUNCH_LDS(merge_topk_big_kernel, dim3(grid), dim3(SCAN_THREADS), SS_LDS_BYTES, stream, p, scratch, bkt);
    return RQ_OK;
  }
  constexpr int CTRL_BYTES = (sizeof(MergeCtrl) + 15) & ~15;
  size_t lds = CTRL_BYTES + (size_t)p.p2 * 8;
  RQ_LAUNCH_LDS(merge_topk_kernel, dim3((uint32_t)nq), dim3(MERGE_THREADS), lds, stream, p);
  return RQ_OK;
}

// the row tiling rq_order.hip has to match: rows per lane and sub-step, rows of one wavefront tile (the shuffle granule),
// rows that meet in one LDS gather and the key bits per code byte that make such a gather conflict-free.
// Every LDS read width is served 32 lanes per pass on gfx950 (ds_read_b64: 256 B/clk; a dword gather moves half as much in
// the same passes -- measured again in round 4 with byte tables split into [k][quad][256] dwords read by ds_read2st64_b32
// and a 64-lane / 2-bit row order: 1.55 -> 2.65 ms), so the group is 32 rows and the window 32 values for all of them.
void scan_order_tiling(int mp, OrderTiling *t) {
  int r = 1, g = SCAN_THREADS, bk = SCAN_THREADS;
  ScanTiling c;
  if (scan_tiling(mp, &c)) { r = c.RPT; g = 64 * c.RPT; bk = c.BLK; }
  const int tg = tuning("ORDER_GRAN", 0);
  t->rpt = r;
  t->gran = tg > 0 ? tg : g;
  t->group = 32;
  t->cbits = 3;
  t->blk = bk;
}

int pad_codes_launch(uint8_t *dst, const uint8_t *src, int64_t n, int m, int mp, hipStream_t stream) {
  const size_t total = (size_t)n * mp;
  hipLaunchKernelGGL(pad_codes_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, dst, src,
                     (size_t)n, m, mp);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

int lut_launch(float *lut, const float *centers, const float *queries, int64_t nq, int m, int sub,
               hipStream_t stream) {
  const size_t total = (size_t)nq * m * 256;
  const int threads = 256;
  hipLaunchKernelGGL(adc_lut_kernel, dim3((uint32_t)((total + threads - 1) / threads)), dim3(threads), 0,
                     stream, lut, centers, queries, (uint32_t)nq, m, sub);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

int synth_codes_launch(uint8_t *codes, int64_t n, int m, uint64_t seed, int64_t row0, hipStream_t stream) {
  const size_t nbytes = (size_t)n * m;
  const size_t nthreads = (nbytes + 7) / 8;
  hipLaunchKernelGGL(synth_codes_kernel, dim3((uint32_t)((nthreads + 255) / 256)), dim3(256), 0, stream,
                     codes, nbytes, seed, (uint64_t)row0 * (uint64_t)m);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

}  // namespace rq
