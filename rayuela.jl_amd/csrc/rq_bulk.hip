// rq_bulk.hip -- exact top-k for RQ_MAX_K < k <= n: the "bulk" path of every scan entry point and of the merge.
//
// The candidate-buffer scan (rq_scan.hip) keeps ~2.5 k keys per query of a group in every workgroup; at k = 65536 that is
// already ~10 GiB of scratch, so larger k take this path instead.  Per batch of queries (all on the caller's stream, no host
// read-back between the passes):
//   1. adc_bulk_keys_kernel  one packed key ordered(dist) << 32 | id per (row, query), the same table and sum arithmetic as
//                            adc_scan_kernel (build_lut / row_dists of rq_scan_tables.h, then + row_bias); NaN -> KEY_MAX
//   2. bulk_hist / bulk_pick MSB radix select of the k-th smallest key per query: per pass one global 256-bin histogram of
//                            the keys that share the prefix found so far, then one wavefront picks the bin.  A query stops as
//                            soon as the chosen bin is taken whole (rank == population): tau = prefix | all lower bits ones
//   3. bulk_compact          the keys <= tau (KEY_MAX excluded) -- exactly k since keys are unique, fewer only when the k-th is
//                            KEY_MAX (the list runs out of comparable rows; the tail is padded) -- and their OR / AND
//   4. bulk_sort_*           stable LSD radix sort of those keys over the 8-bit windows that cover the bits that vary
//                            (OR & ~AND of the kept keys: the distance range [min, tau] and the id width): per window a
//                            per-tile histogram, a per-query scan, a stable scatter
//   5. bulk_unpack           dists / ids (+ id_base) / keys, KEY_MAX = (NaN, 0xFFFFFFFF + id_base) behind the kept keys
// The merge of P sorted lists with K > RQ_MAX_K (merge_launch) runs steps 2-5 on its P * K input keys directly.
// The scratch of one call is at most BULK_SCRATCH_BYTES per device and stream (rq_internal.h); the query batch is sized to fit.
#include "rq_internal.h"
#include "rq_topk.h"
#include "rq_scan_tables.h"

namespace rq {

constexpr int BK_T = 256;                          // threads of the select / compact / sort kernels
constexpr uint32_t BK_ITEMS = 16;                  // keys per thread of a sort tile
constexpr uint32_t BK_TILE = BK_T * BK_ITEMS;      // keys per sort tile
constexpr uint32_t BK_SPAN = BK_T * 8;             // select / compact: keys per block step (8 loads in flight per thread)
constexpr int BK_WINDOWS = 8;                      // 8-bit windows of a 64-bit key

struct BulkQ {
  unsigned long long prefix;     // select: radix prefix found so far; then tau
  unsigned long long kor, kand;  // OR / AND of the kept keys
  uint32_t krem;                 // rank (1-based) still to resolve inside the chosen bin
  uint32_t done;                 // the select is finished
  uint32_t cnt;                  // kept keys (<= k)
  uint32_t nwin;                 // sort windows; the sorted keys end in buf[nwin & 1]
  uint32_t shift[BK_WINDOWS];
};

__global__ __launch_bounds__(BK_T) void bulk_init_kernel(BulkSel s) {
  const uint32_t q = blockIdx.x;
  if (threadIdx.x == 0) {
    BulkQ &st = s.st[q];
    st.prefix = 0;
    st.kor = 0;
    st.kand = ~0ull;
    st.krem = s.k;
    st.done = 0;
    st.cnt = 0;
    st.nwin = 0;
  }
  s.hist[(size_t)q * 256 + threadIdx.x] = 0;
}

// histogram of digit `pass` (bits [56 - 8 pass, 64 - 8 pass)) over the keys that match the prefix above it
__global__ __launch_bounds__(BK_T) void bulk_hist_kernel(BulkSel s, int pass) {
  __shared__ uint32_t h[256];
  const uint32_t q = blockIdx.y;
  const BulkQ *st = s.st + q;
  if (st->done) return;                      // (uniform over the block)
  h[threadIdx.x] = 0;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const uint64_t pfx = st->prefix;
  const uint64_t *src = s.src + (size_t)q * s.ld;
  const uint32_t beg = blockIdx.x * s.span, end = min(s.cnt, beg + s.span);
#pragma unroll 1
  for (uint32_t i0 = beg; i0 < end; i0 += BK_SPAN) {
    uint64_t key[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t idx = i0 + u * BK_T + threadIdx.x;
      key[u] = idx < end ? src[idx] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool on = i0 + u * BK_T + threadIdx.x < end && (pass == 0 || ((key[u] ^ pfx) >> (shift + 8)) == 0);
      hist_add(h, (uint32_t)(key[u] >> shift) & 255u, on);
    }
  }
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(&s.hist[(size_t)q * 256 + threadIdx.x], c);
}

// one wavefront per query: the bin that holds rank krem; clears the histogram for the next pass
__global__ __launch_bounds__(64) void bulk_pick_kernel(BulkSel s, int pass) {
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x;
  BulkQ *st = s.st + q;
  if (st->done) return;
  uint32_t *h = s.hist + (size_t)q * 256;
  const uint32_t c0 = h[lane * 4 + 0], c1 = h[lane * 4 + 1], c2 = h[lane * 4 + 2], c3 = h[lane * 4 + 3];
  h[lane * 4 + 0] = 0; h[lane * 4 + 1] = 0; h[lane * 4 + 2] = 0; h[lane * 4 + 3] = 0;
  const uint32_t sum = c0 + c1 + c2 + c3;
  const uint32_t incl = wave_incl_scan(sum, lane);
  const uint32_t excl = incl - sum;
  const uint32_t kk = st->krem;
  if (excl < kk && kk <= incl) {             // exactly one lane: the matching keys number >= krem
    uint32_t r = kk - excl, b = 0;
    if (r > c0) { r -= c0; b = 1;
      if (r > c1) { r -= c1; b = 2;
        if (r > c2) { r -= c2; b = 3; } } }
    const uint32_t pop = b == 0 ? c0 : b == 1 ? c1 : b == 2 ? c2 : c3;
    const int shift = 56 - 8 * pass;
    uint64_t pfx = st->prefix | ((uint64_t)(lane * 4 + b) << shift);
    // the whole bin is wanted: every key with this prefix is in, none above -- the keys <= prefix | ones are exactly k
    const bool whole = r == pop;
    if (whole && shift > 0) pfx |= (1ull << shift) - 1ull;
    st->prefix = pfx;
    st->krem = r;
    if (whole || pass == 7) st->done = 1;
  }
}

// keys <= tau (KEY_MAX never) to buf0 in any order; their OR / AND
__global__ __launch_bounds__(BK_T) void bulk_compact_kernel(BulkSel s) {
  const uint32_t q = blockIdx.y;
  BulkQ *st = s.st + q;
  const uint64_t tau = st->prefix;
  const uint64_t *src = s.src + (size_t)q * s.ld;
  uint64_t *out = s.buf0 + (size_t)q * s.k;
  const uint32_t beg = blockIdx.x * s.span, end = min(s.cnt, beg + s.span);
  const int lane = threadIdx.x & 63;
  uint64_t kor = 0, kand = ~0ull;
  bool any = false;
#pragma unroll 1
  for (uint32_t i0 = beg; i0 < end; i0 += BK_SPAN) {
    uint64_t key[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t idx = i0 + u * BK_T + threadIdx.x;
      key[u] = idx < end ? src[idx] : KEY_MAX;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool take = key[u] <= tau && key[u] != KEY_MAX;
      const uint64_t mask = __ballot(take);
      if (mask) {
        const int leader = __ffsll((unsigned long long)mask) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&st->cnt, (uint32_t)__popcll(mask));
        base = __builtin_amdgcn_readlane(base, leader);
        if (take) {
          const uint32_t pos = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
          if (pos < s.k) out[pos] = key[u];
          kor |= key[u];
          kand &= key[u];
          any = true;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    kor |= (uint64_t)__shfl_xor((unsigned long long)kor, off);
    kand &= (uint64_t)__shfl_xor((unsigned long long)kand, off);
  }
  if (__ballot(any) && lane == 0) {
    atomicOr(&st->kor, (unsigned long long)kor);
    atomicAnd(&st->kand, (unsigned long long)kand);
  }
}

// the 8-bit windows of the sort: from the lowest varying bit up, each window starts at the next varying bit
__global__ void bulk_windows_kernel(BulkSel s, uint32_t nb) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nb) return;
  BulkQ &st = s.st[q];
  st.cnt = min(st.cnt, s.k);
  uint64_t v = st.cnt > 1 ? (st.kor & ~st.kand) : 0ull;
  uint32_t nw = 0;
  while (v && nw < (uint32_t)BK_WINDOWS) {
    const uint32_t sh = (uint32_t)__builtin_ctzll(v);
    st.shift[nw++] = sh;
    v = sh + 8 >= 64 ? 0ull : (v >> (sh + 8)) << (sh + 8);
  }
  st.nwin = nw;
}

__device__ __forceinline__ const uint64_t *bulk_src(const BulkSel &s, int j, uint32_t q) {
  return ((j & 1) ? s.buf1 : s.buf0) + (size_t)q * s.k;
}

// sort window j: per tile, the 256-bin histogram of the window's digit
__global__ __launch_bounds__(BK_T) void bulk_sort_hist_kernel(BulkSel s, int j) {
  __shared__ uint32_t h[256];
  const uint32_t q = blockIdx.y, t = blockIdx.x;
  const BulkQ *st = s.st + q;
  const uint32_t cnt = st->cnt;
  if ((uint32_t)j >= st->nwin || t * BK_TILE >= cnt) return;
  const uint32_t shift = st->shift[j];
  const uint64_t *src = bulk_src(s, j, q);
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t t0 = t * BK_TILE;
#pragma unroll 4
  for (uint32_t c = 0; c < BK_ITEMS; ++c) {
    const uint32_t idx = t0 + c * BK_T + threadIdx.x;
    const bool on = idx < cnt;
    const uint64_t key = on ? src[idx] : 0;
    hist_add(h, (uint32_t)(key >> shift) & 255u, on);
  }
  __syncthreads();
  s.th[((size_t)q * 256 + threadIdx.x) * s.tiles + t] = h[threadIdx.x];
}

// sort window j: tile counts -> scatter offsets (digit-major, tiles in order: a stable sort)
__global__ __launch_bounds__(BK_T) void bulk_sort_scan_kernel(BulkSel s, int j) {
  __shared__ uint32_t wt[BK_T / 64];
  const uint32_t q = blockIdx.x;
  const BulkQ *st = s.st + q;
  const uint32_t cnt = st->cnt;
  if ((uint32_t)j >= st->nwin || cnt == 0) return;
  const uint32_t nt = (cnt + BK_TILE - 1) / BK_TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t *row = s.th + ((size_t)q * 256 + tid) * s.tiles;
  uint32_t sum = 0;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t c = row[t];
    row[t] = sum;
    sum += c;
  }
  const uint32_t incl = wave_incl_scan(sum, lane);
  if (lane == 63) wt[wave] = incl;
  __syncthreads();
  uint32_t base = incl - sum;
  for (int w = 0; w < wave; ++w) base += wt[w];
  for (uint32_t t = 0; t < nt; ++t) row[t] += base;
}

// sort window j: every tile scatters its keys, 256 at a time in index order; equal digits keep their order (rank among the
// wavefront's lanes with the same digit, then the earlier wavefronts' counts, then the earlier steps' counts)
__global__ __launch_bounds__(BK_T) void bulk_sort_scatter_kernel(BulkSel s, int j) {
  __shared__ uint32_t run[256];
  __shared__ uint32_t wc[BK_T / 64][256];
  const uint32_t q = blockIdx.y, t = blockIdx.x;
  const BulkQ *st = s.st + q;
  const uint32_t cnt = st->cnt;
  if ((uint32_t)j >= st->nwin || t * BK_TILE >= cnt) return;
  const uint32_t shift = st->shift[j];
  const uint64_t *src = bulk_src(s, j, q);
  uint64_t *dst = ((j & 1) ? s.buf0 : s.buf1) + (size_t)q * s.k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  run[tid] = s.th[((size_t)q * 256 + tid) * s.tiles + t];
#pragma unroll
  for (int w = 0; w < BK_T / 64; ++w) wc[w][tid] = 0;
  __syncthreads();
  const uint32_t t0 = t * BK_TILE;
  const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll 1
  for (uint32_t c = 0; c < BK_ITEMS && t0 + c * BK_T < cnt; ++c) {
    const uint32_t idx = t0 + c * BK_T + tid;
    const bool valid = idx < cnt;
    const uint64_t key = valid ? src[idx] : 0;
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint64_t ones = __ballot((d >> b) & 1u);
      peers &= ((d >> b) & 1u) ? ones : ~ones;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & lt);
    if (valid && rank == 0) wc[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t off = run[d] + rank;
      for (int w = 0; w < wave; ++w) off += wc[w][d];
      if (off < cnt) dst[off] = key;
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (int w = 0; w < BK_T / 64; ++w) { add += wc[w][tid]; wc[w][tid] = 0; }
    run[tid] += add;
    __syncthreads();
  }
}

__global__ __launch_bounds__(BK_T) void bulk_unpack_kernel(BulkSel s, BulkOut o) {
  const uint32_t q = blockIdx.y;
  const uint32_t i = blockIdx.x * BK_T + threadIdx.x;
  if (i >= s.k) return;
  const BulkQ *st = s.st + q;
  const uint64_t key = i < st->cnt ? ((st->nwin & 1) ? s.buf1 : s.buf0)[(size_t)q * s.k + i] : KEY_MAX;
  const size_t e = (size_t)q * s.k + i;
  if (o.keys) o.keys[e] = key;
  if (o.dists) o.dists[e] = key_dist(key);
  if (o.ids) o.ids[e] = key_id(key) + o.id_base;
}

// ---- distances -> keys ---------------------------------------------------------------------------------------------------
struct BulkKeyParams {
  const uint8_t *codes;     // [n][M] (padded row width)
  const float *centers;
  const float *queries;     // [nb][d]: the batch
  const float *row_bias;    // by position, as adc_scan_kernel; or nullptr
  const uint32_t *perm;     // ordered base: perm[position] = row; or nullptr
  uint32_t n, nb;
  int sub, d, m_real, lut_mode;
  uint32_t id_offset;
  uint32_t rows_per_wg;
  float4 *gtab;             // [grid][GTAB_F4]
  uint64_t *keys;           // [nb][n]
};

// blockIdx.y: the group of QG queries, blockIdx.x: a range of rows.  The table is built as adc_scan_kernel builds it
// (LDS part + the L1-gathered part in global memory, same release / acquire around the barrier), every row is summed by
// row_dists and gets the row bias added after the table sum (adc_scan_kernel's BIAS step).
// 512 threads for every width: where the scan runs 1024 (m >= 16) its 128-register budget spills row_dists, so the table is
// built in Cfg::THREADS / 512 strides of build_lut (entry e goes to thread e mod Cfg::THREADS either way).
constexpr int BULK_KEY_THREADS = SCAN_THREADS;
template <int M, bool BIAS>
__global__ __launch_bounds__(BULK_KEY_THREADS) void adc_bulk_keys_kernel(BulkKeyParams p) {
  using Cfg = ScanCfg<M>;
  constexpr int QG = Cfg::QG, T = BULK_KEY_THREADS;
  static_assert(Cfg::THREADS % T == 0, "build_lut stride");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *lut = reinterpret_cast<float *>(smem);
  float *qstage = lut + Cfg::LUT_LDS_BYTES / 4;
  const int tid = threadIdx.x;
  const uint32_t q0 = blockIdx.y * QG;
  float4 *gtab = p.gtab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (Cfg::GTAB_F4 > 0 ? Cfg::GTAB_F4 : 1);
  for (int e = tid; e < QG * p.d; e += T) {
    const int q = e / p.d, c = e - q * p.d;
    const uint32_t qq = min(q0 + (uint32_t)q, p.nb - 1u);   // ragged last group: repeat a query (not written)
    qstage[e] = p.queries[(size_t)qq * p.d + c];
  }
  __syncthreads();
#pragma unroll 1
  for (int part = 0; part < Cfg::THREADS / T; ++part)
    build_lut<M>(lut, gtab, qstage, p.centers, p.sub, p.d, p.lut_mode, p.m_real, tid + part * T);
  if (Cfg::KG > 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (Cfg::KG > 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const float4 *lut4 = reinterpret_cast<const float4 *>(lut);
  const uint32_t r0 = blockIdx.x * p.rows_per_wg, r1 = min(p.n, r0 + p.rows_per_wg);
#pragma unroll 1
  for (uint32_t row = r0 + tid; row < r1; row += T) {
    uint32_t w[(M + 3) / 4];
    load_row<M>(w, p.codes, row);
    float acc[QG];
    row_dists<M>(w, 0, lut4, gtab, acc);
    if (BIAS) {
      const float bias = p.row_bias[row];
#pragma unroll
      for (int q = 0; q < QG; ++q) acc[q] = acc[q] + bias;
    }
    const uint32_t kid = (p.perm ? p.perm[row] : row) + p.id_offset;
#pragma unroll
    for (int q = 0; q < QG; ++q)
      if (q0 + q < p.nb) p.keys[(size_t)(q0 + q) * p.n + row] = acc[q] != acc[q] ? KEY_MAX : make_key(acc[q], kid);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// per-query scratch of the select + sort (the keys themselves excluded)
size_t sel_bytes_per_query(uint32_t k) {
  const size_t tiles = (k + BK_TILE - 1) / BK_TILE;
  return 2 * (size_t)k * 8 + tiles * 256 * 4 + 256 * 4 + sizeof(BulkQ) + 4 * 256;   // (+ alignment slack)
}

// lays the select + sort scratch of nb queries out from `at` (bytes advanced)
void sel_layout(BulkSel &s, unsigned char *&at, int64_t nb, uint32_t k) {
  s.k = k;
  s.tiles = (k + BK_TILE - 1) / BK_TILE;
  s.buf0 = (uint64_t *)at; at += align256((size_t)nb * k * 8);
  s.buf1 = (uint64_t *)at; at += align256((size_t)nb * k * 8);
  s.th = (uint32_t *)at; at += align256((size_t)nb * 256 * s.tiles * 4);
  s.hist = (uint32_t *)at; at += align256((size_t)nb * 256 * 4);
  s.st = (BulkQ *)at; at += align256((size_t)nb * sizeof(BulkQ));
}

// blocks per query of the select / compact passes: ~4 per CU over the batch
void sel_grid(BulkSel &s, uint32_t cnt, int64_t nb, int num_cu, uint32_t *hx) {
  s.cnt = cnt;
  const uint64_t want = std::max<uint64_t>(1, (uint64_t)(4 * num_cu + nb - 1) / (uint64_t)nb);
  const uint64_t steps = ((uint64_t)cnt + BK_SPAN - 1) / BK_SPAN;
  const uint64_t per = (steps + std::min(want, steps) - 1) / std::min(want, steps);
  s.span = (uint32_t)(per * BK_SPAN);
  *hx = (uint32_t)(((uint64_t)cnt + s.span - 1) / s.span);
}

// steps 2-5 for nb queries whose keys are ready in s.src
int sel_run(const BulkSel &s, uint32_t hx, int64_t nb, const BulkOut &o, hipStream_t stream) {
  const uint32_t ub = (uint32_t)nb;
  hipLaunchKernelGGL(bulk_init_kernel, dim3(ub), dim3(BK_T), 0, stream, s);
  for (int pass = 0; pass < 8; ++pass) {
    hipLaunchKernelGGL(bulk_hist_kernel, dim3(hx, ub), dim3(BK_T), 0, stream, s, pass);
    hipLaunchKernelGGL(bulk_pick_kernel, dim3(ub), dim3(64), 0, stream, s, pass);
  }
  hipLaunchKernelGGL(bulk_compact_kernel, dim3(hx, ub), dim3(BK_T), 0, stream, s);
  hipLaunchKernelGGL(bulk_windows_kernel, dim3((ub + 63) / 64), dim3(64), 0, stream, s, ub);
  for (int j = 0; j < BK_WINDOWS; ++j) {
    hipLaunchKernelGGL(bulk_sort_hist_kernel, dim3(s.tiles, ub), dim3(BK_T), 0, stream, s, j);
    hipLaunchKernelGGL(bulk_sort_scan_kernel, dim3(ub), dim3(BK_T), 0, stream, s, j);
    hipLaunchKernelGGL(bulk_sort_scatter_kernel, dim3(s.tiles, ub), dim3(BK_T), 0, stream, s, j);
  }
  hipLaunchKernelGGL(bulk_unpack_kernel, dim3((s.k + BK_T - 1) / BK_T, ub), dim3(BK_T), 0, stream, s, o);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

// the usable part of the budget: workspace() allocates 1.25x the request
size_t bulk_usable() { return BULK_SCRATCH_BYTES / 5 * 4; }

template <int M>
static void bulk_key_grid(int64_t nb, int64_t n, int num_cu, uint32_t *gx, uint32_t *gy) {
  using Cfg = ScanCfg<M>;
  *gy = (uint32_t)((nb + Cfg::QG - 1) / Cfg::QG);
  const int64_t want = std::max<int64_t>(1, (4LL * num_cu + *gy - 1) / *gy);
  *gx = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(want, (n + BULK_KEY_THREADS - 1) / BULK_KEY_THREADS));
}

// workgroups of the distance kernel for any batch of at most nb queries: gx * gy <= 4 num_cu + gy - 1 (bulk_key_grid)
template <int M>
static size_t bulk_key_wgs(int64_t nb, int num_cu) {
  return (size_t)4 * num_cu + (size_t)((nb + ScanCfg<M>::QG - 1) / ScanCfg<M>::QG);
}

template <int M>
static size_t bulk_scan_bytes(int64_t nb, int64_t n, int k, int num_cu) {
  using Cfg = ScanCfg<M>;
  return align256((size_t)nb * n * 8) + align256(bulk_key_wgs<M>(nb, num_cu) * (Cfg::GTAB_F4 > 0 ? Cfg::GTAB_F4 : 1) * sizeof(float4)) +
         (size_t)nb * sel_bytes_per_query((uint32_t)k) + 6 * 256;
}

// queries per batch (0: one query does not fit the budget)
template <int M>
static int64_t bulk_batch(int64_t nq, int64_t n, int k, int num_cu) {
  const size_t cap = bulk_usable();
  int64_t lo = 0, hi = std::min<int64_t>(nq, BK_MAX_NB);
  while (lo < hi) {         // largest nb whose scratch fits
    const int64_t mid = (lo + hi + 1) / 2;
    if (bulk_scan_bytes<M>(mid, n, k, num_cu) <= cap) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <int M>
static int bulk_scan_m(float *dists, uint32_t *ids, uint64_t *keys, const uint8_t *codes, const float *centers,
                       const float *queries, int64_t n, int64_t nq, int m, int d, int k, uint32_t id_offset, int id_base,
                       hipStream_t stream, int lut_mode, const float *row_bias, const uint32_t *perm, int num_cu) {
  using Cfg = ScanCfg<M>;
  const int64_t nbmax = bulk_batch<M>(nq, n, k, num_cu);
  if (nbmax < 1)
    return fail_hip(hipErrorOutOfMemory, "bulk top-k: one query needs more than the BULK_SCRATCH_BYTES budget of scratch",
                    __FILE__, __LINE__);
  void *ws = nullptr;
  RQ_TRY(workspace(WS_BULK, bulk_scan_bytes<M>(nbmax, n, k, num_cu), &ws, stream));
  char name[64];
  snprintf(name, sizeof(name), "adc_bulk_keys_kernel<%d, %s>", M, row_bias ? "true" : "false");
  set_last_scan_kernel(name);
  void (*kern)(BulkKeyParams) = row_bias ? adc_bulk_keys_kernel<M, true> : adc_bulk_keys_kernel<M, false>;
  const size_t lds = (size_t)Cfg::LUT_LDS_BYTES + (size_t)Cfg::QG * d * 4;
  if (lds > 160 * 1024) return fail(RQ_EUNSUPPORTED, "bulk top-k: d=%d does not fit the LDS table plan", d);
  for (int64_t q0 = 0; q0 < nq; q0 += nbmax) {
    const int64_t nb = std::min(nbmax, nq - q0);
    uint32_t gx, gy;
    bulk_key_grid<M>(nb, n, num_cu, &gx, &gy);
    if ((size_t)gx * gy > bulk_key_wgs<M>(nbmax, num_cu)) return fail(RQ_EINVAL, "bulk top-k: grid %u x %u", gx, gy);
    unsigned char *at = (unsigned char *)ws;
    BulkKeyParams p;
    p.codes = codes; p.centers = centers; p.queries = queries + (size_t)q0 * d;
    p.row_bias = row_bias; p.perm = perm;
    p.n = (uint32_t)n; p.nb = (uint32_t)nb;
    p.sub = d / m; p.d = d; p.m_real = m; p.lut_mode = lut_mode;
    p.id_offset = id_offset;
    p.rows_per_wg = (uint32_t)((n + gx - 1) / gx);
    p.keys = (uint64_t *)at; at += align256((size_t)nb * n * 8);
    p.gtab = (float4 *)at; at += align256((size_t)gx * gy * (Cfg::GTAB_F4 > 0 ? Cfg::GTAB_F4 : 1) * sizeof(float4));
    RQ_LAUNCH_LDS(kern, dim3(gx, gy), dim3(BULK_KEY_THREADS), lds, stream, p);
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

int bulk_scan(float *dists, uint32_t *ids, uint64_t *keys, const uint8_t *codes, const float *centers, const float *queries,
              int64_t n, int64_t nq, int m, int d, int k, uint32_t id_offset, int id_base, hipStream_t stream, int lut_mode,
              const float *row_bias, const uint32_t *perm, int num_cu) {
  switch (scan_padded_m(m)) {
#define RQ_BULK_CASE(MP) \
    case MP: return bulk_scan_m<MP>(dists, ids, keys, codes, centers, queries, n, nq, m, d, k, id_offset, id_base, stream, \
                                    lut_mode, row_bias, perm, num_cu);
    RQ_BULK_CASE(2) RQ_BULK_CASE(4) RQ_BULK_CASE(8) RQ_BULK_CASE(16) RQ_BULK_CASE(32) RQ_BULK_CASE(64)
#undef RQ_BULK_CASE
  }
  return fail(RQ_EUNSUPPORTED, "m=%d", m);
}

void bulk_plan(int64_t n, int64_t nq, int m, int k, int num_cu, int64_t *qg, int64_t *groups, int64_t *grid, int64_t *batch) {
  uint32_t gx = 1, gy = 1;
  int64_t nb = 0, g = 1;
  switch (scan_padded_m(m)) {
#define RQ_BULK_CASE(MP)                                                               \
    case MP:                                                                           \
      g = ScanCfg<MP>::QG;                                                             \
      nb = bulk_batch<MP>(nq, n, k, num_cu);                                           \
      bulk_key_grid<MP>(std::max<int64_t>(1, nb), n, num_cu, &gx, &gy);                \
      break;
    RQ_BULK_CASE(2) RQ_BULK_CASE(4) RQ_BULK_CASE(8) RQ_BULK_CASE(16) RQ_BULK_CASE(32) RQ_BULK_CASE(64)
#undef RQ_BULK_CASE
  }
  *qg = g;
  *groups = (nq + g - 1) / g;
  *grid = (int64_t)gx * gy;
  *batch = nb;
}

int bulk_merge(float *dists, uint32_t *ids, uint64_t *keys_out, const uint64_t *keys_in, int64_t nq, int P, int K,
               int id_base, hipStream_t stream) {
  const uint64_t cnt = (uint64_t)P * (uint64_t)K;
  if (cnt >= (1ull << 31)) return fail(RQ_EINVAL, "merge: P*k=%llu keys per query must be below 2^31", (unsigned long long)cnt);
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  const size_t per = sel_bytes_per_query((uint32_t)K);
  const int64_t nbmax = std::min<int64_t>({nq, BK_MAX_NB, (int64_t)((bulk_usable() - 6 * 256) / per)});
  if (nbmax < 1)
    return fail_hip(hipErrorOutOfMemory, "bulk merge: one query needs more than the BULK_SCRATCH_BYTES budget of scratch",
                    __FILE__, __LINE__);
  void *ws = nullptr;
  RQ_TRY(workspace(WS_BULK, (size_t)nbmax * per + 6 * 256, &ws, stream));
  for (int64_t q0 = 0; q0 < nq; q0 += nbmax) {
    const int64_t nb = std::min(nbmax, nq - q0);
    unsigned char *at = (unsigned char *)ws;
    BulkSel s;
    s.src = keys_in + (size_t)q0 * cnt;
    s.ld = (size_t)cnt;
    sel_layout(s, at, nb, (uint32_t)K);
    uint32_t hx;
    sel_grid(s, (uint32_t)cnt, nb, di.num_cu, &hx);
    BulkOut o;
    o.dists = dists ? dists + (size_t)q0 * K : nullptr;
    o.ids = ids ? ids + (size_t)q0 * K : nullptr;
    o.keys = keys_out ? keys_out + (size_t)q0 * K : nullptr;
    o.id_base = (uint32_t)id_base;
    RQ_TRY(sel_run(s, hx, nb, o, stream));
  }
  return RQ_OK;
}

}  // namespace rq
