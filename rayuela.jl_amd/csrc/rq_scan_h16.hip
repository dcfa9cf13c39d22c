// rq_scan_h16.hip -- the ADC scan over 16-bit codes: linscan_pq / linscan_opq with 1 <= h <= RQ_MAX_H16 codewords per codebook
// (DESIGN.md section 4.18).  The reference has no such scan (deps/src/linscan_aqd.cpp:58,67 hard-wire 256 entries per table);
// this is its arithmetic (:66-97) with `256` replaced by `h`, exact, for every 1 <= k <= n:
//   1. adc_lut_h16_kernel   T[q][k][r] = sum_s (c[(k h + r) sub + s] - q[k sub + s])^2, sequential f32, product and add rounded
//                           apart (-ffp-contract=off), into global scratch -- QPG queries interleaved per entry for the scan
//   2. adc_keys_h16_kernel  one packed key per (row, query): dist = ((T[0][b0] + T[1][b1]) + ...) + T[m-1][b_{m-1}], the table
//                           of a query group in LDS where it fits 128 KiB, else gathered from the global table through L2;
//                           a NaN distance and a code outside [0, h) give KEY_MAX (the index is clamped, never used raw)
//   3. sel_run              the select -> compact -> sort -> unpack chain of rq_bulk.hip on those keys
// The additive-quantizer scan over 16-bit codes (linscan_lsq / linscan_cq) is the same pipeline with the
// full-dimensional tables of aq_lut_h16_kernel (rq_aq_lut_h16.h) in step 1 and, for LSQ, the row's norm added last in step 2
// (adc_keys_h16_kernel<.., HAS_NORM = true>): deps/src/linscan_aqd_pairwise_byte.cpp:14-94, :97-176 with int16 codes.
// per batch of queries, everything on the caller's stream; the batch is sized so that keys + tables + the chain's scratch fit
// the BULK_SCRATCH_BYTES budget of WS_BULK.
// A base whose 8 n bytes of keys do not fit that budget for one query goes through in ROW SLICES: per
// slice the keys kernel and the select chain give the slice's sorted list of k keys (KEY_MAX behind a slice shorter than k),
// which bulk_merge folds into the running list at P = 2 -- the scheme of knn_stage1 (rq_knn.hip).  Keys are (dist, global id)
// pairs in a total order, so the answer is bit for bit that of the unsliced scan.
#include "rq_internal.h"
#include "rq_aq_lut_h16.h"
#include "rq_topk.h"
#include <atomic>

namespace rq {

constexpr size_t H16_LDS_TABLE_BYTES = 128 * 1024;   // table budget of the 160 KiB of LDS per CU
constexpr int H16_LUT_THREADS = 256;

// where the table of m * h entries lives and how many queries share one gather
struct H16Plan {
  int qpg;            // queries per gather: 4 (16-byte entries), 2 or 1
  bool in_lds;
  int qg;             // queries per group (one gather per code)
  size_t gstride;     // floats of one group's table: m * h * qpg rounded up to whole 16-byte loads
  size_t lds_bytes;
};

static H16Plan h16_plan(int m, int h) {
  const size_t E = (size_t)m * h;
  H16Plan p;
  p.in_lds = true;
  if (16 * E <= H16_LDS_TABLE_BYTES) p.qpg = 4;
  else if (8 * E <= H16_LDS_TABLE_BYTES) p.qpg = 2;
  else if (4 * E <= H16_LDS_TABLE_BYTES) p.qpg = 1;
  else { p.qpg = 4; p.in_lds = false; }      // 16-byte gathers from the global table (L2)
  p.qg = p.qpg;
  p.gstride = (E * p.qpg + 3) & ~(size_t)3;
  p.lds_bytes = p.in_lds ? p.gstride * 4 : 0;
  return p;
}

void scan_h16_plan(int m, int h, int out[4]) {
  const H16Plan p = h16_plan(m, h);
  out[0] = p.qpg;
  out[1] = p.in_lds ? 1 : 0;
  out[2] = p.qg;
  out[3] = (int)p.lds_bytes;
}

// ---- tables ---------------------------------------------------------------------------------------------------------------
// One thread per (query group, entry e = k h + r): lut[(g0 + g) * gstride + e * QPG + j] for the QPG queries of group g0 + g (a
// ragged last group repeats the last query; its entries are never read into a key that is written).  QPG = 1 with
// gstride = m h is the plain [nq][m][h] of rq_dev_adc_lut_wide.  vec4: sub % 4 == 0 and centers 16-byte aligned.
template <int QPG>
__global__ __launch_bounds__(H16_LUT_THREADS) void adc_lut_h16_kernel(float *lut, const float *centers, const float *queries,
                                                                      uint32_t nq, uint32_t g0, uint32_t ngroups, int m, int h,
                                                                      int sub, size_t gstride, int vec4) {
  using V = H16Vec<QPG>;
  const size_t E = (size_t)m * h;
  const size_t t = (size_t)blockIdx.x * H16_LUT_THREADS + threadIdx.x;
  if (t >= (size_t)ngroups * E) return;
  const uint32_t g = g0 + (uint32_t)(t / E);
  const size_t e = t - (size_t)(t / E) * E;
  const int k = (int)(e / (size_t)h);
  const float *c = centers + e * (size_t)sub;
  const size_t d = (size_t)m * sub;
  const float *qv[QPG];
  float acc[QPG];
#pragma unroll
  for (int j = 0; j < QPG; ++j) {
    const uint32_t qq = min(g * (uint32_t)QPG + (uint32_t)j, nq - 1u);
    qv[j] = queries + (size_t)qq * d + (size_t)k * sub;
    acc[j] = 0.0f;
  }
  auto step = [&](float cs, int s) {
#pragma unroll
    for (int j = 0; j < QPG; ++j) {
      const float diff = cs - qv[j][s];
      const float sq = diff * diff;
      acc[j] = acc[j] + sq;
    }
  };
  if (vec4) {
    const float4 *c4 = reinterpret_cast<const float4 *>(c);
    for (int s = 0; s < sub; s += 4) {
      const float4 cv = c4[s >> 2];
      step(cv.x, s); step(cv.y, s + 1); step(cv.z, s + 2); step(cv.w, s + 3);
    }
  } else {
    for (int s = 0; s < sub; ++s) step(c[s], s);
  }
  reinterpret_cast<typename V::type *>(lut + (size_t)g * gstride)[e] = V::make(acc);
}

template <int QPG>
static int lut_h16_groups(float *lut, const float *centers, const float *queries, int64_t nq, int m, int h, int sub,
                          size_t gstride, hipStream_t stream) {
  const int64_t ngroups = (nq + QPG - 1) / QPG;
  const int64_t E = (int64_t)m * h;
  const int vec4 = (sub & 3) == 0 && ((uintptr_t)centers & 15) == 0;
  const int64_t per = std::max<int64_t>(1, LAUNCH_MAX_THREADS / E);     // groups per launch: fewer than 2^31 + m h work-items
  for (int64_t g0 = 0; g0 < ngroups; g0 += per) {
    const int64_t ng = std::min(per, ngroups - g0);
    const int64_t threads = ng * E;
    hipLaunchKernelGGL(adc_lut_h16_kernel<QPG>, dim3((uint32_t)((threads + H16_LUT_THREADS - 1) / H16_LUT_THREADS)),
                       dim3(H16_LUT_THREADS), 0, stream, lut, centers, queries, (uint32_t)nq, (uint32_t)g0, (uint32_t)ng, m, h, sub,
                       gstride, vec4);
    RQ_HIP(hipGetLastError());
  }
  return RQ_OK;
}

int lut_h16_launch(float *lut, const float *centers, const float *queries, int64_t nq, int m, int h, int sub,
                   hipStream_t stream) {
  return lut_h16_groups<1>(lut, centers, queries, nq, m, h, sub, (size_t)m * h, stream);
}

// the tables of the additive-quantizer scan (rq_aq_lut_h16.h) for queries [0, nq) in groups of QPG: codebooks [m * h][d]
template <int QPG, int MODE>
static int aq_lut_h16_mode(float *tab, const float *codebooks, const float *queries, int64_t nq, int m, int h, int d,
                           size_t gstride, hipStream_t stream) {
  const int64_t ngroups = (nq + QPG - 1) / QPG;
  const int64_t E = (int64_t)m * h;
  const int64_t tiles = (nq + AQ_LUT_TQ - 1) / AQ_LUT_TQ;
  const int64_t ex = (E + AQ_LUT_THREADS - 1) / AQ_LUT_THREADS;
  const int vec4 = (d & 3) == 0 && ((uintptr_t)codebooks & 15) == 0;
  // tiles per launch: fewer than LAUNCH_MAX_THREADS work-items, and a grid.y the hardware takes
  const int64_t per = std::max<int64_t>(1, std::min<int64_t>(65535, LAUNCH_MAX_THREADS / (ex * AQ_LUT_THREADS)));
  for (int64_t t0 = 0; t0 < tiles; t0 += per) {
    const int64_t nt = std::min(per, tiles - t0);
    hipLaunchKernelGGL((aq_lut_h16_kernel<QPG, MODE>), dim3((uint32_t)ex, (uint32_t)nt), dim3(AQ_LUT_THREADS), 0, stream, tab,
                       codebooks, queries, (uint32_t)nq, (uint32_t)ngroups, (uint32_t)t0, (uint32_t)E, d, gstride, vec4);
    RQ_HIP(hipGetLastError());
  }
  return RQ_OK;
}

template <int QPG>
static int aq_lut_h16_groups(float *tab, const float *codebooks, const float *queries, int64_t nq, int m, int h, int d,
                             size_t gstride, int lut_mode, hipStream_t stream) {
  if (lut_mode == LUT_LSQ) return aq_lut_h16_mode<QPG, LUT_LSQ>(tab, codebooks, queries, nq, m, h, d, gstride, stream);
  return aq_lut_h16_mode<QPG, LUT_CQ>(tab, codebooks, queries, nq, m, h, d, gstride, stream);
}

int aq_lut_h16_launch(float *lut, const float *codebooks, const float *queries, int64_t nq, int m, int h, int d, int lut_mode,
                      hipStream_t stream) {
  return aq_lut_h16_groups<1>(lut, codebooks, queries, nq, m, h, d, (size_t)m * h, lut_mode, stream);
}

// ---- distances -> keys ----------------------------------------------------------------------------------------------------
struct H16KeyParams {
  const int16_t *codes;     // [n][m], 2-byte aligned at least
  const float *tab;         // [groups][gstride]: entry e of group g holds QPG queries
  const float *dbnorms;     // [n], HAS_NORM only: added to the row's sum last (linscan_aqd_pairwise_byte.cpp:74)
  uint64_t *keys;           // [nb][ld]
  size_t ld;                // keys per query: n, or max(slice rows, k) when the rows go through in slices
  size_t gstride;
  uint32_t n, nb;
  int m, h;
  int vec;                  // bytes per row load: the largest of 16, 8, 4, 2 that divides the row pitch 2 m and the pointer
  uint32_t id_offset;
  uint32_t rows_per_wg;
};

template <int BYTES>
__device__ __forceinline__ void h16_load(uint32_t *w, const unsigned char *p) {
  if constexpr (BYTES == 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else if constexpr (BYTES == 8) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    w[0] = v.x; w[1] = v.y;
  } else if constexpr (BYTES == 4) {
    w[0] = *reinterpret_cast<const uint32_t *>(p);
  } else {
    w[0] = *reinterpret_cast<const uint16_t *>(p);
  }
}

// the row's m table entries summed in order, BYTES of codes per load; returns whether a code lies outside [0, h)
template <int QPG, bool IN_LDS, int BYTES>
__device__ __forceinline__ bool h16_row(float *acc, const unsigned char *rp, int m, uint32_t h,
                                        const typename H16Vec<QPG>::type *lt, const typename H16Vec<QPG>::type *gt) {
  using V = H16Vec<QPG>;
  constexpr int CPL = BYTES / 2;      // codes per load
  bool bad = false;
  uint32_t base = 0;
#pragma unroll 2
  for (int c0 = 0; c0 < m; c0 += CPL) {
    uint32_t w[4];
    h16_load<BYTES>(w, rp + 2 * c0);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const uint32_t code = (w[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;    // a negative int16 is >= 32768 > h
      const bool out = code >= h;
      bad |= out;
      const uint32_t e = base + (out ? 0u : code);                       // clamped: never outside the table
      const typename V::type v = IN_LDS ? lt[e] : gt[e];
#pragma unroll
      for (int q = 0; q < QPG; ++q) acc[q] = acc[q] + V::get(v, q);
      base += h;
    }
  }
  return bad;
}

// blockIdx.y: the group of QPG queries, blockIdx.x: a range of rows.  IN_LDS: the group's table is copied to LDS 16 bytes at a
// time and gathered there with one ds_read of 4 * QPG bytes per code; else the gathers go to the global table.  HAS_NORM (LSQ):
// acc = acc + dbnorms[row] after the m entries, one rounding; a NaN norm makes the row no neighbour like any NaN distance.
template <int QPG, bool IN_LDS, bool HAS_NORM = false>
__global__ __launch_bounds__(1024) void adc_keys_h16_kernel(H16KeyParams p) {
  using V = H16Vec<QPG>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t tid = threadIdx.x, T = blockDim.x;
  const uint32_t q0 = blockIdx.y * QPG;
  const float *gtab = p.tab + (size_t)blockIdx.y * p.gstride;
  if (IN_LDS) {
    float4 *l4 = reinterpret_cast<float4 *>(smem);
    const float4 *g4 = reinterpret_cast<const float4 *>(gtab);
    const uint32_t n4 = (uint32_t)(p.gstride >> 2);
    for (uint32_t i = tid; i < n4; i += T) l4[i] = g4[i];
    __syncthreads();
  }
  const typename V::type *lt = reinterpret_cast<const typename V::type *>(smem);
  const typename V::type *gt = reinterpret_cast<const typename V::type *>(gtab);
  const uint32_t r0 = blockIdx.x * p.rows_per_wg, r1 = min(p.n, r0 + p.rows_per_wg);
  const size_t pitch = (size_t)p.m * 2;
  const unsigned char *cbytes = reinterpret_cast<const unsigned char *>(p.codes);
#pragma unroll 1
  for (uint32_t row = r0 + tid; row < r1; row += T) {
    const unsigned char *rp = cbytes + (size_t)row * pitch;
    float acc[QPG];
#pragma unroll
    for (int q = 0; q < QPG; ++q) acc[q] = 0.0f;
    bool bad;
    if (p.vec == 16) bad = h16_row<QPG, IN_LDS, 16>(acc, rp, p.m, (uint32_t)p.h, lt, gt);
    else if (p.vec == 8) bad = h16_row<QPG, IN_LDS, 8>(acc, rp, p.m, (uint32_t)p.h, lt, gt);
    else if (p.vec == 4) bad = h16_row<QPG, IN_LDS, 4>(acc, rp, p.m, (uint32_t)p.h, lt, gt);
    else bad = h16_row<QPG, IN_LDS, 2>(acc, rp, p.m, (uint32_t)p.h, lt, gt);
    if (HAS_NORM) {
      const float nrm = p.dbnorms[row];
#pragma unroll
      for (int q = 0; q < QPG; ++q) acc[q] = acc[q] + nrm;
    }
    const uint32_t kid = row + p.id_offset;
#pragma unroll
    for (int q = 0; q < QPG; ++q)
      if (q0 + q < p.nb) p.keys[(size_t)(q0 + q) * p.ld + row] = (bad || acc[q] != acc[q]) ? KEY_MAX : make_key(acc[q], kid);
  }
}

// ---- host entries: codes to zero-based, validated on the device ------------------------------------------------------------
__global__ void prepare_codes_h16_kernel(int16_t *codes, unsigned long long *first_bad, size_t e0, size_t nelem, int m, int h,
                                         int base) {
  const size_t i = e0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nelem) return;
  const int c = (int)codes[i] - base;
  if (c < 0 || c >= h) atomicMin(first_bad, (unsigned long long)(i / (size_t)m));
  else if (base) codes[i] = (int16_t)c;
}

int prepare_codes_h16_launch(int16_t *codes, unsigned long long *first_bad, int64_t n, int m, int h, int code_base,
                             hipStream_t stream) {
  RQ_HIP(hipMemsetAsync(first_bad, 0xFF, 8, stream));
  const int64_t nelem = n * m;
  return for_slices(nelem, [&](int64_t e0, int64_t ne) {
    RQ_LAUNCH(prepare_codes_h16_kernel, dim3((uint32_t)((ne + 255) / 256)), dim3(256), 0, stream, codes, first_bad, (size_t)e0,
              (size_t)nelem, m, h, code_base);
    return RQ_OK;
  });
}

// (On the null stream hipMemcpyAsync + hipStreamSynchronize orders exactly as the blocking hipMemcpy the host entries used
// here: both wait for the kernel above, queued on the same stream, and return with the word on the host.)
int check_codes_h16(const char *who, int16_t *codes, unsigned long long *flag, int64_t n, int m, int h, int code_base,
                    hipStream_t stream, const char *suffix) {
  RQ_TRY(prepare_codes_h16_launch(codes, flag, n, m, h, code_base, stream));
  unsigned long long first_bad = 0;
  RQ_HIP(hipMemcpyAsync(&first_bad, flag, 8, hipMemcpyDeviceToHost, stream));
  RQ_HIP(hipStreamSynchronize(stream));
  if (first_bad != ~0ull)
    return fail(RQ_EINVAL, "%s: row %llu holds a code outside [%d, %d]%s", who, first_bad, code_base, h - 1 + code_base, suffix);
  return RQ_OK;
}

// ---- the scan -------------------------------------------------------------------------------------------------------------
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t h16_scan_bytes(const H16Plan &pl, int64_t nb, int64_t n, int k) {
  const size_t groups = (size_t)((nb + pl.qg - 1) / pl.qg);
  return align256((size_t)nb * n * 8) + align256(groups * pl.gstride * 4) + (size_t)nb * sel_bytes_per_query((uint32_t)k) + 6 * 256;
}

// queries per batch (0: one query does not fit the budget)
static int64_t h16_batch(const H16Plan &pl, int64_t nq, int64_t n, int k) {
  const size_t cap = bulk_usable();
  int64_t lo = 0, hi = std::min<int64_t>(nq, BK_MAX_NB);
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (h16_scan_bytes(pl, mid, n, k) <= cap) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ---- row slices -------------------------------------------------------------------------------------------------------------
static std::atomic<int64_t> g_h16_slice_rows{0};     // rq_test_scan_wide_slice_rows: > 0 overrides the planner's slice

struct H16Slices {
  int64_t rows, slices, batch;     // rows per slice (the last may be shorter), slices, queries per batch; batch 0: does not fit
  size_t ld, bytes;                // keys per query of a slice: max(rows, k); WS_BULK bytes of a batch
  int forced, sliced;
};

// WS_BULK of a sliced batch.  The chain's scratch comes FIRST and is exactly what bulk_merge asks of the slot for nb queries:
// the fold lays its own scratch out from the start of the slot, over the slice's select scratch (idle by then) and nothing else.
// Behind it: the slice's keys, the tables, then the running list, the slice's list (adjacent: the interleave reads them as two
// shards) and the interleaved pair -- 32 k bytes of lists per query.
static size_t h16_sliced_front(int64_t nb, int k) { return align256((size_t)nb * sel_bytes_per_query((uint32_t)k) + 6 * 256); }

static size_t h16_sliced_bytes(const H16Plan &pl, int64_t nb, size_t ld, int k) {
  const size_t groups = (size_t)((nb + pl.qg - 1) / pl.qg);
  return h16_sliced_front(nb, k) + align256((size_t)nb * ld * 8) + align256(groups * pl.gstride * 4) +
         2 * align256((size_t)nb * k * 8) + align256((size_t)nb * 2 * k * 8);
}

// Host only.  A call whose whole base fits for one query is not sliced (it launches what it always did) unless the test hook
// forces a slice length.  Else the slice is the longest for which one query group (pl.qg queries: one table gather serves them
// all), or the nq queries if they are fewer, fits the budget, evened out over the slices; the batch is then what fits.
static H16Slices h16_slices(const H16Plan &pl, int64_t n, int64_t nq, int k) {
  H16Slices sl;
  const size_t cap = bulk_usable();
  const int64_t forced = g_h16_slice_rows.load();
  sl.forced = forced > 0;
  if (!sl.forced) {
    const int64_t nb = h16_batch(pl, nq, n, k);
    if (nb >= 1) {
      sl.rows = n; sl.slices = 1; sl.batch = nb; sl.ld = (size_t)n; sl.bytes = h16_scan_bytes(pl, nb, n, k); sl.sliced = 0;
      return sl;
    }
  }
  sl.sliced = 1;
  int64_t rows;
  if (sl.forced) rows = std::min<int64_t>(n, forced);
  else {
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(nq, pl.qg));
    int64_t lo = 0, hi = n;
    while (lo < hi) {         // the bytes do not fall as the slice grows
      const int64_t mid = lo + (hi - lo + 1) / 2;
      if (h16_sliced_bytes(pl, want, (size_t)std::max<int64_t>(mid, k), k) <= cap) lo = mid;
      else hi = mid - 1;
    }
    rows = lo;
  }
  if (rows < 1) { sl.rows = sl.slices = sl.batch = 0; sl.ld = sl.bytes = 0; return sl; }
  sl.slices = (n + rows - 1) / rows;
  if (!sl.forced) rows = (n + sl.slices - 1) / sl.slices;
  sl.rows = rows;
  sl.ld = (size_t)std::max<int64_t>(rows, k);
  int64_t lo = 0, hi = std::min<int64_t>(std::max<int64_t>(nq, 1), BK_MAX_NB);
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (h16_sliced_bytes(pl, mid, sl.ld, k) <= cap) lo = mid;
    else hi = mid - 1;
  }
  sl.batch = lo;
  sl.bytes = lo ? h16_sliced_bytes(pl, lo, sl.ld, k) : 0;
  return sl;
}

int scan_h16_slices(int64_t n, int64_t nq, int m, int h, int k, int64_t out[5]) {
  const H16Slices sl = h16_slices(h16_plan(m, h), n, nq, k);
  out[0] = sl.rows; out[1] = sl.slices; out[2] = sl.batch; out[3] = (int64_t)sl.bytes; out[4] = sl.forced;
  if (sl.batch < 1)
    return fail_hip(hipErrorOutOfMemory, "wide scan: one query needs more than the BULK_SCRATCH_BYTES budget of scratch",
                    __FILE__, __LINE__);
  return RQ_OK;
}

int64_t scan_h16_force_slice_rows(int64_t rows) { return g_h16_slice_rows.exchange(rows > 0 ? rows : 0); }

int linscan_wide_check(const char *who, bool null_arg, int64_t n, int m, int h, int d, int k, uint32_t id_offset, int id_base,
                       bool full_dim) {
  if (null_arg) return fail(RQ_EINVAL, "%s: NULL argument", who);
  if (id_base != 0 && id_base != 1) return fail(RQ_EINVAL, "%s: id_base must be 0 or 1; got %d", who, id_base);
  if (m < 1 || m > 32) return fail(RQ_EUNSUPPORTED, "%s covers 1 <= m <= 32; got m=%d", who, m);
  if (h < 1 || h > RQ_MAX_H16) return fail(RQ_EUNSUPPORTED, "%s scans Int16 codes: 1 <= h <= %d; got h=%d", who, RQ_MAX_H16, h);
  if (full_dim && d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);
  if (!full_dim && (d < m || d % m != 0))
    return fail(RQ_EINVAL, "%s needs d %% m == 0 (src/Linscan.jl:23 Cint(d/m)); got d=%d m=%d", who, d, m);
  if (n < 1 || n >= (1LL << 31)) return fail(RQ_EINVAL, "%s: n=%lld must be in [1, 2^31)", who, (long long)n);
  if (k < 1 || k > n)
    return fail(RQ_EINVAL, "%s: k=%d outside [1, n=%lld] (deps/src/linscan_aqd.cpp:91)", who, k, (long long)n);
  if ((uint64_t)id_offset + (uint64_t)n > 0xFFFFFFFFull) return fail(RQ_EINVAL, "%s: row ids overflow uint32", who);
  return RQ_OK;
}

// lut_mode LUT_PQ: centers [m][h][d/m]; LUT_LSQ / LUT_CQ: `centers` are codebooks [m * h][d], dbnorms [n] for LUT_LSQ
template <int QPG, bool IN_LDS, bool HAS_NORM = false>
static int h16_scan(const H16Plan &pl, float *dists, uint32_t *ids, uint64_t *keys, const int16_t *codes, const float *centers,
                    const float *queries, int64_t n, int64_t nq, int m, int h, int d, int k, uint32_t id_offset, int id_base,
                    int num_cu, hipStream_t stream, int lut_mode = LUT_PQ, const float *dbnorms = nullptr) {
  const H16Slices sl = h16_slices(pl, n, nq, k);
  const int64_t nbmax = sl.batch;
  if (nbmax < 1)
    return fail_hip(hipErrorOutOfMemory, "wide scan: one query needs more than the BULK_SCRATCH_BYTES budget of scratch",
                    __FILE__, __LINE__);
  void *ws = nullptr;
  // (sized once for the whole call: the folds below ask the slot for less and so never move it under these pointers)
  RQ_TRY(workspace(WS_BULK, sl.bytes, &ws, stream));
  char name[64];
  snprintf(name, sizeof(name), "adc_keys_h16_kernel<%d, %s%s>", QPG, IN_LDS ? "true" : "false", HAS_NORM ? ", true" : "");
  set_last_scan_kernel(name);
  void (*kern)(H16KeyParams) = adc_keys_h16_kernel<QPG, IN_LDS, HAS_NORM>;
  if (IN_LDS)
    RQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)pl.lds_bytes));
  // one workgroup per CU where the table takes more than half of the LDS: 1024 threads keep 16 wavefronts there
  const int threads = pl.lds_bytes > 80 * 1024 ? 1024 : 512;
  const uintptr_t al = (uintptr_t)codes | (uintptr_t)(2 * m);
  const int vec = (al & 15) == 0 ? 16 : (al & 7) == 0 ? 8 : (al & 3) == 0 ? 4 : 2;
  if (sl.sliced) {
    const size_t ld = sl.ld;
    for (int64_t q0 = 0; q0 < nq; q0 += nbmax) {
      const int64_t nb = std::min(nbmax, nq - q0);
      const uint32_t gy = (uint32_t)((nb + QPG - 1) / QPG);
      const int64_t want = std::max<int64_t>(1, (2LL * num_cu + gy - 1) / gy);
      unsigned char *at = (unsigned char *)ws;
      unsigned char *const front = at; at += h16_sliced_front(nb, k);
      uint64_t *const kbuf = (uint64_t *)at; at += align256((size_t)nb * ld * 8);
      float *tab = (float *)at; at += align256((size_t)gy * pl.gstride * 4);
      const size_t lstride = align256((size_t)nb * k * 8) / 8;
      uint64_t *const run = (uint64_t *)at, *const part = run + lstride, *const pair = part + lstride;
      if (lut_mode == LUT_PQ) RQ_TRY(lut_h16_groups<QPG>(tab, centers, queries + (size_t)q0 * d, nb, m, h, d / m, pl.gstride, stream));
      else RQ_TRY(aq_lut_h16_groups<QPG>(tab, centers, queries + (size_t)q0 * d, nb, m, h, d, pl.gstride, lut_mode, stream));
      float *const od = dists ? dists + (size_t)q0 * k : nullptr;
      uint32_t *const oi = ids ? ids + (size_t)q0 * k : nullptr;
      uint64_t *const ok = keys ? keys + (size_t)q0 * k : nullptr;
      for (int64_t c = 0; c < sl.slices; ++c) {
        const int64_t r0 = c * sl.rows, nr = std::min(sl.rows, n - r0);
        const bool last = c + 1 == sl.slices;
        const int16_t *cs = codes + (size_t)r0 * m;
        const uintptr_t al = (uintptr_t)cs | (uintptr_t)(2 * m);
        const uint32_t gx = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(want, (nr + threads - 1) / threads));
        H16KeyParams p;
        p.codes = cs;
        p.tab = tab;
        p.dbnorms = dbnorms ? dbnorms + r0 : nullptr;
        p.keys = kbuf;
        p.ld = ld;
        p.gstride = pl.gstride;
        p.n = (uint32_t)nr; p.nb = (uint32_t)nb;
        p.m = m; p.h = h;
        p.vec = (al & 15) == 0 ? 16 : (al & 7) == 0 ? 8 : (al & 3) == 0 ? 4 : 2;
        p.id_offset = id_offset + (uint32_t)r0;
        p.rows_per_wg = (uint32_t)((nr + gx - 1) / gx);
        // a slice shorter than k: the chain reads k keys per query, KEY_MAX from the slice's rows on
        if (nr < k) RQ_HIP(hipMemsetAsync(kbuf, 0xFF, (size_t)nb * ld * 8, stream));
        hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(threads), pl.lds_bytes, stream, p);
        RQ_HIP(hipGetLastError());
        unsigned char *sat = front;
        BulkSel s;
        s.src = kbuf;
        s.ld = ld;
        sel_layout(s, sat, nb, (uint32_t)k);
        uint32_t hx;
        sel_grid(s, (uint32_t)std::max<int64_t>(nr, k), nb, num_cu, &hx);
        BulkOut o;
        const bool direct = c == 0 && last;
        o.dists = direct ? od : nullptr;
        o.ids = direct ? oi : nullptr;
        o.keys = direct ? ok : c == 0 ? run : part;
        o.id_base = direct ? (uint32_t)id_base : 0u;
        RQ_TRY(sel_run(s, hx, nb, o, stream));
        if (c > 0) {
          RQ_TRY(interleave_keys_launch(pair, run, nb, 2, k, lstride, stream));
          if (last) RQ_TRY(bulk_merge(od, oi, ok, pair, nb, 2, k, id_base, stream));
          else RQ_TRY(bulk_merge(nullptr, nullptr, run, pair, nb, 2, k, 0, stream));
        }
      }
    }
    return RQ_OK;
  }
  for (int64_t q0 = 0; q0 < nq; q0 += nbmax) {
    const int64_t nb = std::min(nbmax, nq - q0);
    const uint32_t gy = (uint32_t)((nb + QPG - 1) / QPG);
    const int64_t want = std::max<int64_t>(1, (2LL * num_cu + gy - 1) / gy);
    const uint32_t gx = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(want, (n + threads - 1) / threads));
    unsigned char *at = (unsigned char *)ws;
    H16KeyParams p;
    p.codes = codes;
    p.keys = (uint64_t *)at; at += align256((size_t)nb * n * 8);
    float *tab = (float *)at; at += align256((size_t)gy * pl.gstride * 4);
    p.tab = tab;
    p.dbnorms = dbnorms;
    p.gstride = pl.gstride;
    p.ld = (size_t)n;
    p.n = (uint32_t)n; p.nb = (uint32_t)nb;
    p.m = m; p.h = h; p.vec = vec;
    p.id_offset = id_offset;
    p.rows_per_wg = (uint32_t)((n + gx - 1) / gx);
    if (lut_mode == LUT_PQ) RQ_TRY(lut_h16_groups<QPG>(tab, centers, queries + (size_t)q0 * d, nb, m, h, d / m, pl.gstride, stream));
    else RQ_TRY(aq_lut_h16_groups<QPG>(tab, centers, queries + (size_t)q0 * d, nb, m, h, d, pl.gstride, lut_mode, stream));
    hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(threads), pl.lds_bytes, stream, p);
    RQ_HIP(hipGetLastError());
    BulkSel s;
    s.src = p.keys;
    s.ld = (size_t)n;
    sel_layout(s, at, nb, (uint32_t)k);
    uint32_t hx;
    sel_grid(s, (uint32_t)n, nb, num_cu, &hx);
    BulkOut o;
    o.dists = dists ? dists + (size_t)q0 * k : nullptr;
    o.ids = ids ? ids + (size_t)q0 * k : nullptr;
    o.keys = keys ? keys + (size_t)q0 * k : nullptr;
    o.id_base = (uint32_t)id_base;
    RQ_TRY(sel_run(s, hx, nb, o, stream));
  }
  return RQ_OK;
}

int dev_linscan_wide(float *dists, uint32_t *ids, uint64_t *keys, const int16_t *codes, const float *centers,
                     const float *queries, int64_t n, int64_t nq, int m, int h, int d, int k, uint32_t id_offset, int id_base,
                     hipStream_t stream) {
  if (nq <= 0) return RQ_OK;
  RQ_TRY(linscan_wide_check("rq_dev_linscan_wide", !codes || !centers || !queries || (!keys && (!dists || !ids)), n, m, h, d, k,
                            id_offset, id_base));
  if (((uintptr_t)codes & 1) != 0 || ((uintptr_t)centers & 3) != 0 || ((uintptr_t)queries & 3) != 0)
    return fail(RQ_EINVAL, "rq_dev_linscan_wide: codes must be 2-byte aligned, centers and queries 4-byte aligned");
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock launch_lock;
  const H16Plan pl = h16_plan(m, h);
#define RQ_H16_ARGS pl, dists, ids, keys, codes, centers, queries, n, nq, m, h, d, k, id_offset, id_base, di.num_cu, stream
  if (!pl.in_lds) return h16_scan<4, false>(RQ_H16_ARGS);
  if (pl.qpg == 4) return h16_scan<4, true>(RQ_H16_ARGS);
  if (pl.qpg == 2) return h16_scan<2, true>(RQ_H16_ARGS);
  return h16_scan<1, true>(RQ_H16_ARGS);
#undef RQ_H16_ARGS
}

// linscan_lsq / linscan_cq over one resident shard of 16-bit codes: codebooks [m * h][d] full-dimensional
int dev_linscan_aq_wide(float *dists, uint32_t *ids, uint64_t *keys, const int16_t *codes, const float *codebooks,
                        const float *queries, const float *dbnorms, int64_t n, int64_t nq, int m, int h, int d, int k,
                        int lut_mode, uint32_t id_offset, int id_base, hipStream_t stream) {
  const char *who = "rq_dev_linscan_aq_wide";
  if (nq <= 0) return RQ_OK;
  if (lut_mode != LUT_LSQ && lut_mode != LUT_CQ) return fail(RQ_EINVAL, "%s: lut_mode must be 1 (LSQ) or 2 (CQ)", who);
  RQ_TRY(linscan_wide_check(who, !codes || !codebooks || !queries || (!keys && (!dists || !ids)) || (lut_mode == LUT_LSQ && !dbnorms),
                            n, m, h, d, k, id_offset, id_base, true));
  if (((uintptr_t)codes & 1) != 0 || ((uintptr_t)codebooks & 3) != 0 || ((uintptr_t)queries & 3) != 0 || ((uintptr_t)dbnorms & 3) != 0)
    return fail(RQ_EINVAL, "%s: codes must be 2-byte aligned, codebooks, queries and dbnorms 4-byte aligned", who);
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock launch_lock;
  const H16Plan pl = h16_plan(m, h);
#define RQ_H16_ARGS pl, dists, ids, keys, codes, codebooks, queries, n, nq, m, h, d, k, id_offset, id_base, di.num_cu, stream, lut_mode
  if (lut_mode == LUT_LSQ) {
    if (!pl.in_lds) return h16_scan<4, false, true>(RQ_H16_ARGS, dbnorms);
    if (pl.qpg == 4) return h16_scan<4, true, true>(RQ_H16_ARGS, dbnorms);
    if (pl.qpg == 2) return h16_scan<2, true, true>(RQ_H16_ARGS, dbnorms);
    return h16_scan<1, true, true>(RQ_H16_ARGS, dbnorms);
  }
  if (!pl.in_lds) return h16_scan<4, false>(RQ_H16_ARGS);
  if (pl.qpg == 4) return h16_scan<4, true>(RQ_H16_ARGS);
  if (pl.qpg == 2) return h16_scan<2, true>(RQ_H16_ARGS);
  return h16_scan<1, true>(RQ_H16_ARGS);
#undef RQ_H16_ARGS
}

}  // namespace rq
