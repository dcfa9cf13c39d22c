// rq_rerank.hip -- exact re-ranking of search candidates on a resident base.
//
// Every search of this library ranks by a quantized distance; the reference stops there (eval_recall, src/Linscan.jl:196-234,
// takes the ids as they come).  Here the candidates of a search are ordered by D32, the exact f32 distance of rq_knn_f32
// (include/rayuela_hip.h, "exact k-nearest-neighbour"), against a base that is resident on the device:
//   1. rerank_keys_f32_kernel<W> / rerank_keys_u8_kernel<W>   grid (slab of 256 candidates, query): one lane per candidate, its row gathered by id,
//                                     writes make_key(D32, row + id_offset) -- KEY_MAX for an id outside the base or a NaN distance
//                                     -- into keys [nb][ld].  One accumulator per pair walks s = 0..d-1 in order, unfused.  Byte
//                                     rows are streamed by their lane, f32 rows staged through LDS: what each measured faster.
//   2. the k smallest keys            kc <= RERANK_LDS_K: rerank_sort_kernel, one workgroup per query, bitonic sort in LDS;
//                                     above: rerank_cut_kernel, then the select -> compact -> sort chain of rq_bulk.hip, unchanged.
// The chain is written for unique keys: where the k-th smallest key has copies on both sides of rank k it keeps an arbitrary k of
// the keys <= it.  Candidates may repeat (there is no dedupe), so rerank_cut_kernel first finds that key and how many of its copies
// belong to the answer (radix_select of rq_topk.h: after its 8 passes krem is the rank inside the copies) and retires the others to
// KEY_MAX; the chain then meets exactly k keys <= its threshold.  Both paths give the same bytes.
#include "rq_encode_split.h"
#include "rq_internal.h"
#include "rq_topk.h"

#include <string.h>

#include <atomic>

namespace rq {

constexpr int RR_T = 256;                // threads of every kernel here; candidates of a slab
constexpr int RR_QP = 1024;              // floats of the query staged per piece (a multiple of every load width)
constexpr uint32_t RERANK_LDS_K = 4096;  // candidates a workgroup sorts in LDS (32 KiB of keys)

struct RerankKeyParams {
  const void *X;          // the whole base
  const float *Q;         // [nb][d]
  const uint32_t *cand;   // candidate i of query q: cand[q * ldc + i * cstep]; words behind kc are never read
  size_t ldc;             // in words
  uint32_t cstep;         // 1: ids; 2: the low words of packed keys
  uint64_t *keys;         // [nb][ld]
  size_t ld;
  int64_t n;
  uint32_t kc, sub, id_offset; // row = candidate - sub (mod 2^32)
  int d;
};

// W elements of a row at x as floats: f32 rows by dwordx4 / dwordx2 / dword, byte rows by 16 / 8 / 4 / 2 / 1 bytes widened with
// v_cvt_f32_ubyte*.  The host picks W so that every load is aligned (rerank_width).
template <class ROW_T, int W>
__device__ __forceinline__ void rerank_load(const ROW_T *x, float (&v)[W]) {
  if constexpr (sizeof(ROW_T) == 4) {
    if constexpr (W == 4) { const float4 t = *reinterpret_cast<const float4 *>(x); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else if constexpr (W == 2) { const float2 t = *reinterpret_cast<const float2 *>(x); v[0] = t.x; v[1] = t.y; }
    else v[0] = x[0];
  } else {
    uint32_t w[(W + 3) / 4];
    const uint8_t *b = reinterpret_cast<const uint8_t *>(x);
    if constexpr (W == 16) { const uint4 t = *reinterpret_cast<const uint4 *>(b); w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w; }
    else if constexpr (W == 8) { const uint2 t = *reinterpret_cast<const uint2 *>(b); w[0] = t.x; w[1] = t.y; }
    else if constexpr (W == 4) w[0] = *reinterpret_cast<const uint32_t *>(b);
    else if constexpr (W == 2) w[0] = *reinterpret_cast<const uint16_t *>(b);
    else w[0] = b[0];
    bytes_f32<W>(w, v);
  }
}

// Byte rows, the direct loader.  blockIdx.x: slab of RR_T candidates, blockIdx.y: query.  The query goes through LDS in pieces of
// RR_QP floats (every lane reads the same word: a broadcast); a lane streams its own row with U loads of W bytes in flight
// (2 x 16 or 2 x 8 bytes, else 4 loads).  d % W == 0.
template <int W>
__global__ __launch_bounds__(RR_T) void rerank_keys_u8_kernel(RerankKeyParams p) {
  using ROW_T = uint8_t;
  __shared__ __attribute__((aligned(16))) float qs[RR_QP];
  constexpr int U = W >= 8 ? 2 : 4;
  const uint32_t q = blockIdx.y, i = blockIdx.x * RR_T + threadIdx.x;
  const int d = p.d;
  const float *qv = p.Q + (size_t)q * d;
  uint32_t c = 0;
  if (i < p.kc) c = p.cand[(size_t)q * p.ldc + (size_t)i * p.cstep];
  const uint32_t r = c - p.sub;
  const bool valid = i < p.kc && (int64_t)r < p.n;
  const ROW_T *x = reinterpret_cast<const ROW_T *>(p.X) + (size_t)(valid ? r : 0u) * d;
  float acc = 0.0f;
#pragma unroll 1
  for (int s0 = 0; s0 < d; s0 += RR_QP) {
    const int ns = min(RR_QP, d - s0);
    if (s0) __syncthreads();
    for (int s = threadIdx.x; s < ns; s += RR_T) qs[s] = qv[s0 + s];
    __syncthreads();
    if (valid) {
      int s = 0;
#pragma unroll 1
      for (; s + U * W <= ns; s += U * W) {
        float v[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) rerank_load<ROW_T, W>(x + s0 + s + u * W, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int j = 0; j < W; ++j) {
            const float t = v[u][j] - qs[s + u * W + j];
            const float sq = t * t;
            acc = acc + sq;
          }
      }
#pragma unroll 1
      for (; s < ns; s += W) {
        float v[W];
        rerank_load<ROW_T, W>(x + s0 + s, v);
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const float t = v[j] - qs[s + j];
          const float sq = t * t;
          acc = acc + sq;
        }
      }
    }
  }
  if (i < p.kc) p.keys[(size_t)q * p.ld + i] = (!valid || acc != acc) ? KEY_MAX : make_key(acc, r + p.id_offset);
}

// f32 rows, the staged loader.  The rows of a slab go through LDS 32 dimensions at a time: 8 lanes x 4 elements fetch the 32
// elements of one row (a whole 128-byte line per load instruction instead of 16 bytes of each of 64 lines), 32 rows per pass, 8
// passes in flight; xs[s][row] with a pitch of 258 words puts the 8 x 8 (part, row) writes of a wavefront into 64 different
// banks, and lane `row` then reads xs[s][row]: consecutive words.  Any d; W < 4 (d no multiple of 4): pieces of W floats.
constexpr int RR_DS = 32;               // dimensions staged per step
constexpr int RR_XP = RR_T + 2;         // pitch of a staged dimension
template <int W>
__global__ __launch_bounds__(RR_T) void rerank_keys_f32_kernel(RerankKeyParams p) {
  using ROW_T = float;
  __shared__ __attribute__((aligned(16))) float qs[RR_QP];
  __shared__ float xs[RR_DS * RR_XP];
  __shared__ uint32_t rrow[RR_T];
  constexpr int WW = W < 4 ? W : 4;
  const uint32_t q = blockIdx.y, i = blockIdx.x * RR_T + threadIdx.x;
  const int tid = threadIdx.x, d = p.d;
  const float *qv = p.Q + (size_t)q * d;
  uint32_t c = 0;
  if (i < p.kc) c = p.cand[(size_t)q * p.ldc + (size_t)i * p.cstep];
  const uint32_t r = c - p.sub;
  const bool valid = i < p.kc && (int64_t)r < p.n;
  rrow[tid] = valid ? r : 0xFFFFFFFFu;          // (no row has this number: n <= 2^32 - 1)
  const ROW_T *X = reinterpret_cast<const ROW_T *>(p.X);
  const int part = tid & 7, rsub = tid >> 3;
  float acc = 0.0f;
#pragma unroll 1
  for (int s0 = 0; s0 < d; s0 += RR_QP) {
    const int ns = min(RR_QP, d - s0);
    __syncthreads();
    for (int s = tid; s < ns; s += RR_T) qs[s] = qv[s0 + s];
#pragma unroll 1
    for (int t0 = 0; t0 < ns; t0 += RR_DS) {
      __syncthreads();
      const int sb = s0 + t0 + 4 * part;
      const int ne = min(4, d - sb);              // elements of this lane's piece that exist (<= 0: none)
      float v[8][4];
#pragma unroll
      for (int ps = 0; ps < 8; ++ps) {
        const uint32_t row = rrow[ps * 32 + rsub];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[ps][j] = 0.0f;
        if (row != 0xFFFFFFFFu) {
          const ROW_T *x = X + (size_t)row * d + sb;
#pragma unroll
          for (int j = 0; j < 4; j += WW) {
            if (j < ne) {
              float t[WW];
              rerank_load<ROW_T, WW>(x + j, t);
#pragma unroll
              for (int e = 0; e < WW; ++e) v[ps][j + e] = t[e];
            }
          }
        }
      }
#pragma unroll
      for (int ps = 0; ps < 8; ++ps)
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[(4 * part + j) * RR_XP + ps * 32 + rsub] = v[ps][j];
      __syncthreads();
      if (valid) {
        const int nd = min(RR_DS, ns - t0);
        for (int s = 0; s < nd; ++s) {
          const float t = xs[s * RR_XP + tid] - qs[t0 + s];
          const float sq = t * t;
          acc = acc + sq;
        }
      }
    }
  }
  if (i < p.kc) p.keys[(size_t)q * p.ld + i] = (!valid || acc != acc) ? KEY_MAX : make_key(acc, r + p.id_offset);
}

struct RerankSelParams {
  uint64_t *keys;         // [nb][ld]
  size_t ld;
  float *dists;           // [nb][k]
  uint32_t *ids;
  uint32_t kc, k, p2, id_base;
  const uint32_t *cand;   // as RerankKeyParams
  size_t ldc;
  uint32_t cstep, sub;
  int64_t n;
  uint32_t *nvalid;       // [nb] <- candidates of the query inside the base (rq_last_rerank_stats)
};

// One workgroup per query counts its valid candidates: a statistic only, taken here and not in the keys kernel, where one atomic per
// wavefront on a shared counter took as long as the gather itself (1.9 ms of 2.0 at 1e7 candidates).
__device__ __forceinline__ void rerank_count_valid(const RerankSelParams &p, uint32_t q, uint32_t *part) {
  const uint32_t tid = threadIdx.x;
  uint32_t cnt = 0;
  for (uint32_t i = tid; i < p.kc; i += RR_T) cnt += (int64_t)(uint32_t)(p.cand[(size_t)q * p.ldc + (size_t)i * p.cstep] - p.sub) < p.n ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, off);
  if ((tid & 63) == 0) part[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) p.nvalid[q] = part[0] + part[1] + part[2] + part[3];
}

// one workgroup per query, kc <= RERANK_LDS_K: the keys sorted in LDS, the first k unpacked as bulk_unpack_kernel unpacks them
__global__ __launch_bounds__(RR_T) void rerank_sort_kernel(RerankSelParams p) {
  __shared__ uint64_t sk[RERANK_LDS_K];
  __shared__ uint32_t part[RR_T / 64];
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  const uint64_t *src = p.keys + (size_t)q * p.ld;
  rerank_count_valid(p, q, part);
  for (uint32_t i = tid; i < p.p2; i += RR_T) sk[i] = i < p.kc ? src[i] : KEY_MAX;
  bitonic_sort_tiled(sk, p.p2, RR_T / 64, tid >> 6, tid & 63, true);
  for (uint32_t i = tid; i < p.k; i += RR_T) {
    const uint64_t key = sk[i];
    p.dists[(size_t)q * p.k + i] = key_dist(key);
    p.ids[(size_t)q * p.k + i] = key_id(key) + p.id_base;
  }
}

// one workgroup per query, in front of the chain: tau = the k-th smallest key; of its copies only the `krem` that belong to the
// k smallest stay, the others become KEY_MAX.  A select that stopped early took a whole distance bucket (nothing to retire), and
// so did one that ends on KEY_MAX: both leave a low word of ones, which no row's key has (row + id_offset <= 2^32 - 2).
__global__ __launch_bounds__(RR_T) void rerank_cut_kernel(RerankSelParams p) {
  __shared__ SelState<1> st;
  __shared__ uint32_t seen;
  __shared__ uint32_t part[RR_T / 64];
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  uint64_t *keys = p.keys + (size_t)q * p.ld;
  rerank_count_valid(p, q, part);
  uint32_t vseq = 0;
  if (tid < 2) st.vote[tid] = 0;
  if (tid == 0) seen = 0;
  __syncthreads();
  radix_select<1, RR_T>(&st, keys, p.kc, p.k, true, 0, (int)tid, vseq);
  __syncthreads();
  const uint64_t tau = st.prefix[0];
  const uint32_t keep = st.krem[0];
  if ((uint32_t)tau == 0xFFFFFFFFu) return;
  const uint32_t lane = tid & 63;
  const uint32_t cnt_up = (p.kc + RR_T - 1) / RR_T * RR_T;        // whole workgroups in the ballot
  for (uint32_t i = tid; i < cnt_up; i += RR_T) {
    const bool hit = i < p.kc && keys[i] == tau;
    const uint64_t mask = __ballot(hit);
    if (mask) {
      const int leader = __ffsll((unsigned long long)mask) - 1;
      uint32_t base = 0;
      if ((int)lane == leader) base = atomicAdd(&seen, (uint32_t)__popcll(mask));
      base = __builtin_amdgcn_readlane(base, leader);
      if (hit && base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)) >= keep) keys[i] = KEY_MAX;
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static size_t rr_align(size_t b) { return (b + 255) & ~(size_t)255; }

enum { RP_UPLOAD = 0, RP_KEYS, RP_SELECT, RP_DOWNLOAD, RP_N };
static thread_local double g_rr_ms[RP_N] = {0};
static thread_local uint64_t g_rr_stats[8] = {0};

static std::atomic<int64_t> g_rr_lds_k{0};      // rq_test_rerank_limits: > 0 replaces RERANK_LDS_K (never above it)
static std::atomic<int64_t> g_rr_batch{0};      // > 0: queries per batch of rq_dataset_rerank

static uint32_t rerank_lds_limit() {
  const int64_t f = g_rr_lds_k.load();
  return f > 0 ? (uint32_t)std::min<int64_t>(f, RERANK_LDS_K) : RERANK_LDS_K;
}

size_t rerank_scratch_bytes(int64_t nb, int64_t kc, int k, bool chain) {
  const size_t ld = ((size_t)kc + 3) & ~(size_t)3;
  return rr_align((size_t)nb * 4) + rr_align((size_t)nb * ld * 8) + (chain ? (size_t)nb * sel_bytes_per_query((uint32_t)k) + 6 * 256 : 0);
}

struct RerankPlan { int64_t batch; size_t ld, bytes; int chain, forced; };

// queries per batch: the most whose keys and chain scratch fit the bulk budget (0: not even one), or what the hook forces
static RerankPlan rerank_plan(int64_t nq, int64_t kc, int k) {
  RerankPlan pl;
  pl.ld = ((size_t)kc + 3) & ~(size_t)3;
  pl.chain = rerank_chain(kc);           // read ONCE per call: it sizes the scratch here and picks the path in rerank_device
  int64_t lo = 0, hi = std::min<int64_t>(std::max<int64_t>(nq, 1), BK_MAX_NB);
  const int64_t forced = g_rr_batch.load();
  pl.forced = forced > 0;
  if (forced > 0) hi = std::min(hi, forced);
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (rerank_scratch_bytes(mid, kc, k, pl.chain) <= bulk_usable()) lo = mid;
    else hi = mid - 1;
  }
  pl.batch = lo;
  pl.bytes = lo ? rerank_scratch_bytes(lo, kc, k, pl.chain) : 0;
  return pl;
}

// the widest load every row allows: rows begin at X + row * d * esz, so the lowest set bit of (X | d * esz | 16) bytes
static int rerank_width(const void *X, int d, int esz) {
  const uint64_t mix = (uint64_t)(uintptr_t)X | (uint64_t)d * (uint64_t)esz | 16u;
  return (int)((mix & (0 - mix)) / (uint64_t)esz);
}

template <class ROW_T, int W>
static int rerank_keys_launch(const RerankKeyParams &p, uint32_t nb, hipStream_t stream) {
  // the loader that measured faster for the row type: f32 rows staged through LDS, byte rows direct
  const dim3 grid((p.kc + RR_T - 1) / RR_T, nb);
  if constexpr (sizeof(ROW_T) == 4) {
    RQ_LAUNCH(rerank_keys_f32_kernel<W>, grid, dim3(RR_T), 0, stream, p);
  } else {
    RQ_LAUNCH(rerank_keys_u8_kernel<W>, grid, dim3(RR_T), 0, stream, p);
  }
  return RQ_OK;
}

bool rerank_chain(int64_t kc) { return (uint64_t)kc > rerank_lds_limit(); }

void rerank_clear() {
  for (int i = 0; i < RP_N; ++i) g_rr_ms[i] = 0;
  for (int i = 0; i < 8; ++i) g_rr_stats[i] = 0;
}

void rerank_note(int64_t nq, int64_t kc, int64_t batches, unsigned long long valid, int chain) {
  g_rr_stats[0] += (uint64_t)nq;
  g_rr_stats[1] += (uint64_t)nq * (uint64_t)kc;
  g_rr_stats[2] += valid;
  g_rr_stats[3] += (uint64_t)batches;
  g_rr_stats[4] = (uint64_t)chain;
  g_rr_stats[5] = ((uint64_t)kc + 3) & ~(uint64_t)3;
}

void rerank_add_ms(double keys_ms, double select_ms) { g_rr_ms[RP_KEYS] += keys_ms; g_rr_ms[RP_SELECT] += select_ms; }

int rerank_device(const RerankCall &c, hipStream_t stream, PhaseClock &clk, int num_cu) {
  const size_t ld = ((size_t)c.kc + 3) & ~(size_t)3;
  const bool chain = c.chain;
  if (!chain && c.kc > (int64_t)RERANK_LDS_K) return fail(RQ_EINVAL, "rerank: kc=%lld does not sort in LDS", (long long)c.kc);
  unsigned char *at = (unsigned char *)c.scratch;
  RerankKeyParams p;
  uint32_t *nvalid = (uint32_t *)at; at += rr_align((size_t)c.nb * 4);
  p.X = c.base.X; p.Q = c.Q;
  p.cand = c.cand; p.ldc = c.ldc; p.cstep = c.cstep;
  p.keys = (uint64_t *)at; at += rr_align((size_t)c.nb * ld * 8);
  p.ld = ld;
  p.n = c.base.n;
  p.kc = (uint32_t)c.kc;
  p.sub = c.id_offset + (c.cstep == 1 ? (uint32_t)c.id_base : 0u);
  p.id_offset = c.id_offset;
  p.d = c.base.d;
  const uint32_t nb = (uint32_t)c.nb;
  const int w = rerank_width(c.base.X, c.base.d, c.base.esz);
  int rc = RQ_EUNSUPPORTED;
  if (c.base.esz == 4) {
    rc = w >= 4 ? rerank_keys_launch<float, 4>(p, nb, stream) : w == 2 ? rerank_keys_launch<float, 2>(p, nb, stream)
                                                                  : rerank_keys_launch<float, 1>(p, nb, stream);
  } else {
    switch (w) {
      case 16: rc = rerank_keys_launch<uint8_t, 16>(p, nb, stream); break;
      case 8: rc = rerank_keys_launch<uint8_t, 8>(p, nb, stream); break;
      case 4: rc = rerank_keys_launch<uint8_t, 4>(p, nb, stream); break;
      case 2: rc = rerank_keys_launch<uint8_t, 2>(p, nb, stream); break;
      default: rc = rerank_keys_launch<uint8_t, 1>(p, nb, stream); break;
    }
  }
  RQ_TRY(rc);
  clk.mark(c.ph_keys);
  RerankSelParams sp;
  sp.keys = p.keys; sp.ld = ld; sp.dists = c.dists; sp.ids = c.ids;
  sp.kc = (uint32_t)c.kc; sp.k = (uint32_t)c.k; sp.id_base = (uint32_t)c.id_base;
  sp.p2 = std::max<uint32_t>(64u, next_pow2((uint32_t)c.kc));
  sp.cand = p.cand; sp.ldc = p.ldc; sp.cstep = p.cstep; sp.sub = p.sub; sp.n = p.n; sp.nvalid = nvalid;
  if (!chain) {
    RQ_LAUNCH(rerank_sort_kernel, dim3(nb), dim3(RR_T), 0, stream, sp);
  } else {
    RQ_LAUNCH(rerank_cut_kernel, dim3(nb), dim3(RR_T), 0, stream, sp);
    BulkSel s;
    s.src = p.keys;
    s.ld = ld;
    sel_layout(s, at, c.nb, (uint32_t)c.k);
    uint32_t hx;
    sel_grid(s, (uint32_t)c.kc, c.nb, num_cu, &hx);
    BulkOut o;
    o.dists = c.dists; o.ids = c.ids; o.keys = nullptr; o.id_base = (uint32_t)c.id_base;
    RQ_TRY(sel_run(s, hx, c.nb, o, stream));
  }
  clk.mark(c.ph_select);
  RQ_HIP(hipMemcpyAsync(c.nvalid_host, nvalid, (size_t)c.nb * 4, hipMemcpyDeviceToHost, stream));
  return RQ_OK;
}

int rerank_check(const char *who, bool null_arg, int64_t n, int64_t kc, int64_t ldc, int k, uint32_t id_offset, int id_base) {
  if (null_arg) return fail(RQ_EINVAL, "%s: NULL argument", who);
  if (id_base != 0 && id_base != 1) return fail(RQ_EINVAL, "%s: id_base must be 0 or 1; got %d", who, id_base);
  if (k < 1) return fail(RQ_EINVAL, "%s: k=%d < 1", who, k);
  if (kc < (int64_t)k) return fail(RQ_EINVAL, "%s: kc=%lld < k=%d", who, (long long)kc, k);
  if (kc >= (1LL << 31)) return fail(RQ_EINVAL, "%s: kc=%lld must be below 2^31", who, (long long)kc);
  if (ldc < kc) return fail(RQ_EINVAL, "%s: ldc=%lld < kc=%lld", who, (long long)ldc, (long long)kc);
  if ((uint64_t)n + (uint64_t)id_offset > 0xFFFFFFFFull)
    return fail(RQ_EINVAL, "%s: n + id_offset = %llu exceeds 2^32 - 1 (ids are uint32, 0xFFFFFFFF marks padding)", who,
                (unsigned long long)((uint64_t)n + id_offset));
  return RQ_OK;
}

static int rerank_resident(float *dists, uint32_t *ids, const DatasetView &B, const float *queries, int64_t nq,
                           const uint32_t *cand, int64_t kc, int64_t ldc, int k, uint32_t id_offset, int id_base,
                           const RerankPlan &pl) {
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  hipStream_t stream = nullptr;
  const int64_t nbmax = pl.batch;
  Timer tu;
  DevMem dQ, dC, dD, dI;
  RQ_TRY(dQ.alloc((size_t)nq * B.d * 4));
  RQ_TRY(dC.alloc((size_t)nbmax * kc * 4));
  RQ_TRY(dD.alloc((size_t)nbmax * k * 4));
  RQ_TRY(dI.alloc((size_t)nbmax * k * 4));
  RQ_HIP(hipMemcpy(dQ.p, queries, (size_t)nq * B.d * 4, hipMemcpyHostToDevice));
  g_rr_ms[RP_UPLOAD] += tu.ms();
  void *ws = nullptr;
  RQ_TRY(workspace(WS_BULK, pl.bytes, &ws, stream));
  std::vector<float> hd((size_t)nq * k);       // results staged until the call has succeeded
  std::vector<uint32_t> hi((size_t)nq * k), hv((size_t)nbmax);
  PhaseClock clk(stream, g_rr_ms);
  unsigned long long valid = 0;
  int64_t batches = 0;
  for (int64_t q0 = 0; q0 < nq; q0 += nbmax, ++batches) {
    const int64_t nb = std::min(nbmax, nq - q0);
    RQ_HIP(hipMemcpy2D(dC.p, (size_t)kc * 4, cand + (size_t)q0 * ldc, (size_t)ldc * 4, (size_t)kc * 4, (size_t)nb, hipMemcpyHostToDevice));
    clk.mark(RP_UPLOAD);
    RerankCall c;
    c.base = B;
    c.Q = dQ.as<float>() + (size_t)q0 * B.d;
    c.cand = dC.as<uint32_t>(); c.ldc = (size_t)kc; c.cstep = 1;
    c.nb = nb; c.kc = kc; c.k = k; c.id_offset = id_offset; c.id_base = id_base;
    c.dists = dD.as<float>(); c.ids = dI.as<uint32_t>();
    c.scratch = ws;
    c.nvalid_host = hv.data();
    c.chain = pl.chain != 0;
    c.ph_keys = RP_KEYS; c.ph_select = RP_SELECT;
    RQ_TRY(rerank_device(c, stream, clk, di.num_cu));
    RQ_HIP(hipStreamSynchronize(stream));
    for (int64_t b = 0; b < nb; ++b) valid += hv[(size_t)b];
    RQ_HIP(hipMemcpy(hd.data() + (size_t)q0 * k, dD.p, (size_t)nb * k * 4, hipMemcpyDeviceToHost));
    RQ_HIP(hipMemcpy(hi.data() + (size_t)q0 * k, dI.p, (size_t)nb * k * 4, hipMemcpyDeviceToHost));
    clk.mark(RP_DOWNLOAD);
  }
  clk.collect();
  memcpy(dists, hd.data(), hd.size() * 4);
  memcpy(ids, hi.data(), hi.size() * 4);
  rerank_note(nq, kc, batches, valid, pl.chain);
  return RQ_OK;
}

}  // namespace rq

using namespace rq;

extern "C" {

int rq_dataset_rerank(rq_dataset *ds, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, const uint32_t *cand_host,
                      int64_t kc, int64_t ldc, int k, uint32_t id_offset, int id_base) {
  rerank_clear();
  DatasetView v;
  if (!dataset_view(ds, &v)) return fail(RQ_EINVAL, "rq_dataset_rerank: NULL dataset");
  if (nq <= 0) return RQ_OK;
  RQ_TRY(rerank_check("rq_dataset_rerank", !dists || !ids || !queries_host || !cand_host, v.n, kc, ldc, k, id_offset, id_base));
  const RerankPlan pl = rerank_plan(nq, kc, k);
  if (pl.batch < 1)
    return fail(RQ_EUNSUPPORTED, "rq_dataset_rerank: one query's keys (kc=%lld, k=%d) need more than the BULK_SCRATCH_BYTES budget of scratch",
                (long long)kc, k);
  SavedDevice saved;
  RQ_HIP(hipSetDevice(v.device));
  const int rc = rerank_resident(dists, ids, v, queries_host, nq, cand_host, kc, ldc, k, id_offset, id_base, pl);
  if (rc != RQ_OK) (void)hipDeviceSynchronize();     // nothing of the call may still use its buffers when they are freed
  return rc;
}

int rq_last_rerank_stats(uint64_t *out8) {
  if (!out8) return fail(RQ_EINVAL, "rq_last_rerank_stats: null pointer");
  for (int i = 0; i < 8; ++i) out8[i] = g_rr_stats[i];
  return RQ_OK;
}

int rq_last_rerank_timing(double *ms, int cap) {
  if (!ms) return fail(RQ_EINVAL, "rq_last_rerank_timing: null pointer");
  for (int i = 0; i < cap && i < RP_N; ++i) ms[i] = g_rr_ms[i];
  return RQ_OK;
}

int rq_rerank_plan(int64_t n, int64_t nq, int d, int64_t kc, int k, int64_t *out, int cap) {
  if (!out || cap < 5) return fail(RQ_EINVAL, "rq_rerank_plan: out needs 5 entries");
  if (n < 1 || nq < 1 || d < 1 || k < 1 || kc < k || kc >= (1LL << 31)) return fail(RQ_EINVAL, "rq_rerank_plan: bad shape");
  const RerankPlan pl = rerank_plan(nq, kc, k);
  out[0] = pl.batch; out[1] = (int64_t)pl.bytes; out[2] = pl.chain; out[3] = (int64_t)pl.ld; out[4] = pl.forced;
  for (int i = 5; i < cap; ++i) out[i] = 0;
  return RQ_OK;
}

int64_t rq_test_rerank_limits(int64_t lds_kc, int64_t batch_queries) {
  const int64_t a = g_rr_lds_k.exchange(lds_kc > 0 ? lds_kc : 0);
  const int64_t b = g_rr_batch.exchange(batch_queries > 0 ? batch_queries : 0);
  return (a << 32) | (b & 0xFFFFFFFFll);
}

}  // extern "C"
