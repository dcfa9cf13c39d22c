// rq_knn.hip -- exact k-nearest-neighbour ground truth on the device.
//
// The reference never computes ground truth: read_dataset (src/read_datasets.jl) reads it from *_groundtruth.ivecs / gt files and
// eval_recall (src/Linscan.jl:196-234) consumes it.  Here it is made from the vectors themselves, in two stages:
//   1. knn_keys_kernel    one packed key ordered(D32) << 32 | id per (row, query), D32 the unfused f32 chain
//                         acc = acc + (x[s] - q[s]) * (x[s] - q[s]), s = 0..d-1 from +0 (the table arithmetic of linscan_cq,
//                         deps/src/linscan_aqd_pairwise_byte.cpp:124-131); then the select -> compact -> sort chain of rq_bulk.hip
//                         gives the k' smallest keys per query.  The base goes through in row chunks whose keys fit the WS_BULK
//                         budget; a chunk's list is folded into the running one with merge_launch (P = 2).
//   2. knn_rerank_kernel  D64 (the same chain in f64) of the k' candidates of a query, sorted by (D64, id) in LDS, and the
//                         certificate that no other row can enter the list.
//
// Why the answer is exact.  For finite inputs without f32 overflow every term of D32 goes through one subtract, one multiply and
// at most d - 1 adds (the first add, to +0, is exact), each with relative error u = 2^-24 or, where the result is subnormal or
// flushed, absolute error below 2^-126.  A term that stays normal is therefore scaled by (1 + e1)^2 (1 + e2) (1 + e3) ... with at
// most d + 2 factors, and (1 + u)^(d+2) - 1 <= (d + 2) u / (1 - (d + 2) u) < (d + 3) u for every d this library can hold; the
// squared subtract counts twice, which the doubling below absorbs.  Summing over the terms,
//     |D32 - D64| <= gamma D64 + delta,   gamma = 2 (d + 3) 2^-24,   delta = d 2^-125
// (D64's own rounding, (d + 2) 2^-53 relative, disappears in the slack of the doubling; delta is d underflows of at most 2^-126
// each, doubled).  So with T64 the k-th smallest D64 among the candidates and L the D32 of the last candidate, every row that is
// NOT a candidate has D32 >= L, and  L > T64 (1 + gamma) + delta  implies  D64 >= (D32 - delta) / (1 + gamma) > T64: it cannot
// enter the list, not even on an id tie.  D32 = +Inf (an overflow, or an infinite coordinate) is taken as FLT_MAX: the chain
// overflows only where the bound's right-hand side reaches FLT_MAX.  D32 is NaN exactly where D64 is (Inf - Inf or a NaN input;
// the squares and the sums are never negative), and such a pair is no neighbour in either stage.  A query whose certificate
// fails is rerun with four times the candidates; at k' = n there is nothing left to exclude.
#include "rq_encode_split.h"
#include "rq_internal.h"
#include "rq_topk.h"

#include <float.h>
#include <string.h>

#include <atomic>

namespace rq {

typedef float knn_f2 __attribute__((ext_vector_type(2)));

constexpr int KNN_T = 256;            // threads of both kernels
constexpr int KNN_TR = 128;           // rows of a tile: 32 lanes x 4
constexpr int KNN_TQ = 64;            // queries of a tile: 8 lane groups x 8
constexpr int KNN_DS = 32;            // dimensions staged per step
constexpr int KNN_XP = KNN_TR + 4;    // LDS pitch of a staged dimension: the transposing writes spread over the banks, b128 reads stay aligned
constexpr uint32_t KNN_LDS_K = 4096;  // candidates a workgroup sorts in LDS

struct KnnKeyParams {
  const void *X;       // first row of the chunk
  const float *Q;      // [nb][d]
  uint64_t *keys;      // [nb][ld]
  size_t ld;           // a multiple of 4
  uint32_t rows;       // rows of the chunk
  uint32_t cnt;        // keys per query the chain reads: max(rows, k'), KEY_MAX from `rows` on
  uint32_t nb, id0, qtiles;
  int d;
};

// blockIdx.x = row tile * qtiles + query tile (the query tiles of one row tile run together: the rows come from L2).
// Lane (lr, lq) holds rows 4 lr .. + 3 against queries 8 lq .. + 7: per dimension one b128 of rows and two b128 of queries (the
// latter a broadcast) feed 32 (t, t t, acc +) triples, 48 packed f32 instructions.  Every pair walks s = 0..d-1 in order.
template <class ROW_T>
__global__ __launch_bounds__(KNN_T) void knn_keys_kernel(KnnKeyParams p) {
  __shared__ __attribute__((aligned(16))) float xs[KNN_DS * KNN_XP];
  __shared__ __attribute__((aligned(16))) float qs[KNN_DS * KNN_TQ];
  const int tid = threadIdx.x, lr = tid & 31, lq = tid >> 5;
  const uint32_t qt = blockIdx.x % p.qtiles, rt = blockIdx.x / p.qtiles;
  const uint32_t r0 = rt * KNN_TR, q0 = qt * KNN_TQ;
  const int d = p.d;
  const ROW_T *X = reinterpret_cast<const ROW_T *>(p.X);
  knn_f2 acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[r][j] = knn_f2{0.0f, 0.0f};
#pragma unroll 1
  for (int s0 = 0; s0 < d; s0 += KNN_DS) {
    const int ns = min(KNN_DS, d - s0);
    if (s0) __syncthreads();
    if constexpr (sizeof(ROW_T) == 4) {
      for (int e = tid; e < KNN_TR * KNN_DS; e += KNN_T) {
        const int r = e >> 5, s = e & 31;
        const uint32_t row = r0 + (uint32_t)r;
        xs[s * KNN_XP + r] = (row < p.rows && s < ns) ? X[(size_t)row * d + s0 + s] : 0.0f;
      }
    } else {
      const int al = byte_align(X, d, 4);
      for (int e = tid; e < KNN_TR * (KNN_DS / 4); e += KNN_T) {
        const int r = e >> 3, s = 4 * (e & 7);
        const uint32_t row = r0 + (uint32_t)r;
        const int nbytes = row < p.rows ? max(0, min(4, ns - s)) : 0;
        uint32_t w[1];
        float x[4];
        load_bytes<4>(reinterpret_cast<const uint8_t *>(X) + (size_t)(row < p.rows ? row : 0) * d + s0 + s, al, nbytes, w);
        bytes_f32<4>(w, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[(s + j) * KNN_XP + r] = x[j];
      }
    }
    for (int e = tid; e < KNN_TQ * KNN_DS; e += KNN_T) {
      const int q = e >> 5, s = e & 31;
      const uint32_t qq = q0 + (uint32_t)q;
      qs[s * KNN_TQ + q] = (qq < p.nb && s < ns) ? p.Q[(size_t)qq * d + s0 + s] : 0.0f;
    }
    __syncthreads();
#pragma unroll 2
    for (int s = 0; s < ns; ++s) {
      const float4 xv = *reinterpret_cast<const float4 *>(xs + s * KNN_XP + 4 * lr);
      const float4 qa = *reinterpret_cast<const float4 *>(qs + s * KNN_TQ + 8 * lq);
      const float4 qb = *reinterpret_cast<const float4 *>(qs + s * KNN_TQ + 8 * lq + 4);
      const knn_f2 qp[4] = {knn_f2{qa.x, qa.y}, knn_f2{qa.z, qa.w}, knn_f2{qb.x, qb.y}, knn_f2{qb.z, qb.w}};
      const float xr[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const knn_f2 x2 = knn_f2{xr[r], xr[r]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const knn_f2 t = x2 - qp[j];
          const knn_f2 sq = t * t;
          acc[r][j] = acc[r][j] + sq;
        }
      }
    }
  }
  const uint32_t row0 = r0 + 4u * (uint32_t)lr;
  if (row0 >= p.cnt) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t qq = q0 + 8u * (uint32_t)lq + (uint32_t)j;
    if (qq >= p.nb) continue;
    uint64_t key[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = acc[r][j >> 1][j & 1];
      key[r] = (row0 + r >= p.rows || v != v) ? KEY_MAX : make_key(v, row0 + (uint32_t)r + p.id0);
    }
    uint64_t *dst = p.keys + (size_t)qq * p.ld + row0;      // 32-byte aligned: ld and row0 are multiples of 4
    if (row0 + 3 < p.cnt) {
      *reinterpret_cast<ulonglong2 *>(dst) = make_ulonglong2(key[0], key[1]);
      *reinterpret_cast<ulonglong2 *>(dst + 2) = make_ulonglong2(key[2], key[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row0 + r < p.cnt) dst[r] = key[r];
    }
  }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------
struct KnnRerankParams {
  const void *X;          // the whole base
  const float *Q;         // [nb][d]
  const uint64_t *cand;   // [nb][kp] sorted stage-1 keys, KEY_MAX behind the comparable rows
  double *out_d;          // [nb][k]
  uint32_t *out_id;       // [nb][k]
  uint32_t *flag;         // [nb]: 1 certified, 0 not, 2 the host finishes (kp > KNN_LDS_K)
  double *c64;            // [nb][kp] D64 of every candidate (NaN: none) when the host finishes, else null
  uint32_t n, kp, k, p2, id_base;
  int d;
  double gamma1, delta;   // 1 + gamma, delta
};

__device__ __forceinline__ uint64_t knn_d2ord(double v) {
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double knn_ord2d(uint64_t o) {
  const uint64_t u = (o >> 63) ? (o ^ 0x8000000000000000ull) : ~o;
  return __longlong_as_double((long long)u);
}

// one workgroup per query: thread c evaluates candidate c (its row gathered by id), then a bitonic sort of the (D64, id) pairs
template <class ROW_T>
__global__ __launch_bounds__(KNN_T) void knn_rerank_kernel(KnnRerankParams p) {
  __shared__ uint64_t sk[KNN_LDS_K];
  __shared__ uint32_t si[KNN_LDS_K];
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint64_t *cand = p.cand + (size_t)b * p.kp;
  const float *q = p.Q + (size_t)b * p.d;
  const ROW_T *X = reinterpret_cast<const ROW_T *>(p.X);
  const bool in_lds = p.kp <= KNN_LDS_K;
  const uint32_t span = in_lds ? p.p2 : p.kp;
  for (uint32_t c = tid; c < span; c += KNN_T) {
    uint64_t ok = ~0ull;
    uint32_t id = 0xFFFFFFFFu;
    double dv = __longlong_as_double(0x7FF8000000000000ll);
    if (c < p.kp) {
      const uint64_t key = cand[c];
      if (key != KEY_MAX) {
        const uint32_t row = key_id(key);
        const ROW_T *x = X + (size_t)row * p.d;
        double acc = 0.0;
        for (int s = 0; s < p.d; ++s) {
          const double t = __dsub_rn((double)x[s], (double)q[s]);
          acc = __dadd_rn(acc, __dmul_rn(t, t));
        }
        dv = acc;
        if (acc == acc) { ok = knn_d2ord(acc); id = row; }
      }
      if (p.c64) p.c64[(size_t)b * p.kp + c] = dv;
    }
    if (in_lds) { sk[c] = ok; si[c] = id; }
  }
  if (!in_lds) {
    if (tid == 0) p.flag[b] = 2u;
    return;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= p.p2; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t t = tid; t < p.p2 / 2; t += KNN_T) {
        const uint32_t i = 2 * t - (t & (stride - 1)), j = i + stride;
        const uint64_t ka = sk[i], kb = sk[j];
        const uint32_t ia = si[i], ib = si[j];
        const bool gt = ka > kb || (ka == kb && ia > ib);
        if (gt == ((i & size) == 0)) { sk[i] = kb; sk[j] = ka; si[i] = ib; si[j] = ia; }
      }
      __syncthreads();
    }
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  for (uint32_t i = tid; i < p.k; i += KNN_T) {
    const uint64_t ok = sk[i];
    p.out_d[(size_t)b * p.k + i] = ok == ~0ull ? inf : knn_ord2d(ok);
    p.out_id[(size_t)b * p.k + i] = si[i] + p.id_base;
  }
  if (tid == 0) {
    const double t64 = sk[p.k - 1] == ~0ull ? inf : knn_ord2d(sk[p.k - 1]);
    const uint64_t last = cand[p.kp - 1];
    const float l32 = key_dist(last);
    const double l = l32 > FLT_MAX ? (double)FLT_MAX : (double)l32;
    const bool cert = p.kp == p.n || last == KEY_MAX || l > __dadd_rn(__dmul_rn(t64, p.gamma1), p.delta);
    p.flag[b] = cert ? 1u : 0u;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

enum { KP_UPLOAD = 0, KP_KEYS, KP_SELECT, KP_FOLD, KP_RERANK, KP_WIDEN, KP_DOWNLOAD, KP_N };
static thread_local double g_knn_ms[KP_N] = {0};
static thread_local uint64_t g_knn_stats[8] = {0};

static std::atomic<int64_t> g_knn_chunk_rows{0};     // KNN_CHUNK_ROWS (rq_test_knn_chunk_rows): > 0 overrides the planner's chunk

static int64_t knn_first_kp(int64_t n, int k) { return std::min<int64_t>(n, (int64_t)k + std::max(32, k / 4)); }

struct KnnPlan {
  int64_t kp, rows, chunks, batch;
  size_t ld, bytes;      // keys per query of a chunk (a multiple of 4), WS_BULK bytes of a batch
  int forced;
};

static size_t knn_batch_bytes(int64_t nb, size_t ld, int64_t kp) {
  return align256((size_t)nb * ld * 8) + (size_t)nb * sel_bytes_per_query((uint32_t)kp) + 6 * 256;
}

// Row chunks and query batches of one round of stage 1 (host only).  Without the KNN_CHUNK_ROWS override of the test hook a chunk holds the
// whole base while min(nq, 64) queries of it fit the budget, else as many rows as let that many queries fit (never fewer than
// 2^20, or what one query can hold); the batch is then the number of queries whose keys and chain scratch fit.
static KnnPlan knn_plan(int64_t n, int64_t nq, int64_t kp) {
  KnnPlan pl;
  pl.kp = kp;
  const size_t per_sel = sel_bytes_per_query((uint32_t)kp) + 256;
  const size_t usable = bulk_usable() - 6 * 256;
  const int64_t forced = g_knn_chunk_rows.load();
  pl.forced = forced > 0;
  int64_t rows = 0;
  if (forced > 0) rows = std::min<int64_t>(n, forced);
  else if (usable > per_sel + 64) {
    const int64_t want_q = std::max<int64_t>(1, std::min<int64_t>(nq, KNN_TQ));
    const int64_t one = (int64_t)((usable - per_sel) / 8) - 4;
    const int64_t many = usable / want_q > per_sel + 64 ? (int64_t)((usable / want_q - per_sel) / 8) - 4 : 0;
    rows = std::min<int64_t>(n, std::max<int64_t>(many, std::min<int64_t>(one, 1 << 20)));
  }
  if (rows < 1) { pl.rows = pl.chunks = pl.batch = 0; pl.ld = pl.bytes = 0; return pl; }
  pl.chunks = (n + rows - 1) / rows;
  if (!pl.forced) rows = (n + pl.chunks - 1) / pl.chunks;
  pl.rows = rows;
  pl.ld = ((size_t)std::max<int64_t>(rows, kp) + 3) & ~(size_t)3;
  int64_t lo = 0, hi = std::min<int64_t>(std::max<int64_t>(nq, 1), BK_MAX_NB);
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (knn_batch_bytes(mid, pl.ld, kp) <= bulk_usable()) lo = mid;
    else hi = mid - 1;
  }
  pl.batch = lo;
  pl.bytes = lo ? knn_batch_bytes(lo, pl.ld, kp) : 0;
  return pl;
}

struct KnnBase { const void *X; int esz; int64_t n; int d; };

// The kp smallest (D32, id) keys of nb queries (dQ, device) into lists [nb][kp]; lists holds 4 nb kp keys (the running list, the
// chunk's list, the interleaved pair).  `widen`: the call is a rerun, its time goes to that phase.
static int knn_stage1(uint64_t *lists, const KnnBase &B, const float *dQ, int64_t nb, const KnnPlan &pl, int num_cu,
                      PhaseClock &clk, bool widen, hipStream_t stream) {
  const int64_t kp = pl.kp;
  uint64_t *run = lists, *part = lists + (size_t)nb * kp, *pair = lists + 2 * (size_t)nb * kp;
  for (int64_t c = 0; c < pl.chunks; ++c) {
    const int64_t r0 = c * pl.rows, nr = std::min(pl.rows, B.n - r0);
    void *ws = nullptr;    // (looked up per chunk: a fold with k' > RQ_MAX_K runs the bulk merge, which may regrow the slot)
    RQ_TRY(workspace(WS_BULK, pl.bytes, &ws, stream));
    unsigned char *at = (unsigned char *)ws;
    KnnKeyParams p;
    p.X = (const unsigned char *)B.X + (size_t)r0 * B.d * B.esz;
    p.Q = dQ;
    p.keys = (uint64_t *)at; at += align256((size_t)nb * pl.ld * 8);
    p.ld = pl.ld;
    p.rows = (uint32_t)nr;
    p.cnt = (uint32_t)std::max<int64_t>(nr, kp);
    p.nb = (uint32_t)nb;
    p.id0 = (uint32_t)r0;
    p.qtiles = (uint32_t)((nb + KNN_TQ - 1) / KNN_TQ);
    p.d = B.d;
    const uint64_t blocks = (uint64_t)p.qtiles * ((p.cnt + KNN_TR - 1) / KNN_TR);
    if (blocks >= (1ull << 31)) return fail(RQ_EUNSUPPORTED, "knn: %llu tiles in one launch", (unsigned long long)blocks);
    if (B.esz == 1) RQ_LAUNCH(knn_keys_kernel<uint8_t>, dim3((uint32_t)blocks), dim3(KNN_T), 0, stream, p);
    else RQ_LAUNCH(knn_keys_kernel<float>, dim3((uint32_t)blocks), dim3(KNN_T), 0, stream, p);
    clk.mark(widen ? KP_WIDEN : KP_KEYS);
    BulkSel s;
    s.src = p.keys;
    s.ld = pl.ld;
    sel_layout(s, at, nb, (uint32_t)kp);
    uint32_t hx;
    sel_grid(s, p.cnt, nb, num_cu, &hx);
    BulkOut o;
    o.dists = nullptr; o.ids = nullptr; o.keys = c == 0 ? run : part; o.id_base = 0;
    RQ_TRY(sel_run(s, hx, nb, o, stream));
    clk.mark(widen ? KP_WIDEN : KP_SELECT);
    if (c > 0) {
      RQ_TRY(interleave_keys_launch(pair, run, nb, 2, (int)kp, (size_t)nb * kp, stream));
      RQ_TRY(merge_launch(nullptr, nullptr, run, pair, nb, 2, (int)kp, 0, stream));
      clk.mark(widen ? KP_WIDEN : KP_FOLD);
    }
  }
  return RQ_OK;
}

static int knn_check(const char *who, bool null_arg, int64_t n, int d, int k, int id_base, bool f64) {
  if (null_arg) return fail(RQ_EINVAL, "%s: NULL argument", who);
  if (id_base != 0 && id_base != 1) return fail(RQ_EINVAL, "%s: id_base must be 0 or 1; got %d", who, id_base);
  if (d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);
  if (n < 1 || n >= (1LL << 31)) return fail(RQ_EINVAL, "%s: n=%lld must be in [1, 2^31)", who, (long long)n);
  if (k < 1 || k > n) return fail(RQ_EINVAL, "%s: k=%d outside [1, n=%lld]", who, k, (long long)n);
  if (f64 && k > RQ_KNN_MAX_K) return fail(RQ_EUNSUPPORTED, "%s: k=%d above RQ_KNN_MAX_K=%d", who, k, RQ_KNN_MAX_K);
  return RQ_OK;
}

static int knn_oom(const char *who) {
  (void)who;
  return fail_hip(hipErrorOutOfMemory, "knn: one query needs more than the BULK_SCRATCH_BYTES budget of scratch", __FILE__, __LINE__);
}

// stage 1 alone on a resident base; results staged on the host until the call has succeeded
static int knn_f32_resident(float *dists, uint32_t *ids, const KnnBase &B, const float *queries, int64_t nq, int k, int id_base) {
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  hipStream_t stream = nullptr;
  const KnnPlan pl = knn_plan(B.n, nq, k);
  if (pl.batch < 1) return knn_oom("rq_knn_f32");
  g_knn_stats[0] = (uint64_t)nq;
  g_knn_stats[5] = (uint64_t)pl.chunks;
  Timer tu;
  DevMem dQ;
  RQ_TRY(dQ.alloc((size_t)nq * B.d * 4));
  RQ_HIP(hipMemcpy(dQ.p, queries, (size_t)nq * B.d * 4, hipMemcpyHostToDevice));
  g_knn_ms[KP_UPLOAD] += tu.ms();
  const int64_t nbmax = pl.batch;
  void *lists = nullptr, *outs = nullptr;
  RQ_TRY(workspace(WS_KEYS, (size_t)4 * nbmax * k * 8, &lists, stream));
  RQ_TRY(workspace(WS_TMP, (size_t)nbmax * k * 8, &outs, stream));
  float *od = (float *)outs;
  uint32_t *oi = (uint32_t *)(od + (size_t)nbmax * k);
  std::vector<float> hd((size_t)nq * k);
  std::vector<uint32_t> hi((size_t)nq * k);
  PhaseClock clk(stream, g_knn_ms);
  double dl = 0;
  for (int64_t q0 = 0; q0 < nq; q0 += nbmax) {
    const int64_t nb = std::min(nbmax, nq - q0);
    RQ_TRY(knn_stage1((uint64_t *)lists, B, dQ.as<float>() + (size_t)q0 * B.d, nb, pl, di.num_cu, clk, false, stream));
    RQ_TRY(merge_launch(od, oi, nullptr, (const uint64_t *)lists, nb, 1, k, id_base, stream));
    clk.mark(KP_SELECT);
    RQ_HIP(hipStreamSynchronize(stream));
    Timer td;
    RQ_HIP(hipMemcpy(hd.data() + (size_t)q0 * k, od, (size_t)nb * k * 4, hipMemcpyDeviceToHost));
    RQ_HIP(hipMemcpy(hi.data() + (size_t)q0 * k, oi, (size_t)nb * k * 4, hipMemcpyDeviceToHost));
    dl += td.ms();
  }
  clk.collect();
  memcpy(dists, hd.data(), hd.size() * 4);
  memcpy(ids, hi.data(), hi.size() * 4);
  g_knn_ms[KP_DOWNLOAD] += dl;
  return RQ_OK;
}

// the ground truth on a resident base
static int knn_resident(double *dists, uint32_t *ids, const KnnBase &B, const float *queries, int64_t nq, int k, int id_base) {
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  hipStream_t stream = nullptr;
  const int64_t n = B.n;
  const int d = B.d;
  const double gamma = 2.0 * (d + 3) * ldexp(1.0, -24), delta = (double)d * ldexp(1.0, -125);
  const double inf = HUGE_VAL;
  std::vector<double> hd((size_t)nq * k);
  std::vector<uint32_t> hi((size_t)nq * k);
  std::vector<int64_t> todo((size_t)nq), next;
  for (int64_t q = 0; q < nq; ++q) todo[(size_t)q] = q;
  std::vector<float> hq;
  std::vector<uint32_t> hflag;
  std::vector<uint64_t> hkeys;
  std::vector<double> hc64, bd;
  std::vector<uint32_t> bi;
  std::vector<std::pair<double, uint32_t>> v;
  g_knn_stats[0] = (uint64_t)nq;
  DevMem dQ;
  RQ_TRY(dQ.alloc((size_t)nq * d * 4));
  PhaseClock clk(stream, g_knn_ms);
  double dl = 0, ul = 0;
  int64_t kp = knn_first_kp(n, k);
  for (int round = 0; !todo.empty(); ++round) {
    const int64_t nqr = (int64_t)todo.size();
    const bool widen = round > 0;
    const KnnPlan pl = knn_plan(n, nqr, kp);
    if (pl.batch < 1) return knn_oom("rq_knn");
    if (!widen) g_knn_stats[5] = (uint64_t)pl.chunks;
    else {
      g_knn_stats[3] += 1;
      hq.resize((size_t)nqr * d);
      for (int64_t i = 0; i < nqr; ++i) memcpy(hq.data() + (size_t)i * d, queries + (size_t)todo[(size_t)i] * d, (size_t)d * 4);
    }
    Timer tu;
    RQ_HIP(hipMemcpy(dQ.p, widen ? hq.data() : queries, (size_t)nqr * d * 4, hipMemcpyHostToDevice));
    ul += tu.ms();
    const bool on_host = kp > (int64_t)KNN_LDS_K;
    const int64_t nbmax = pl.batch;
    void *lists = nullptr, *outs = nullptr;
    RQ_TRY(workspace(WS_KEYS, (size_t)4 * nbmax * kp * 8, &lists, stream));
    const size_t out_d_bytes = align256((size_t)nbmax * k * 8), out_i_bytes = align256((size_t)nbmax * k * 4);
    const size_t flag_bytes = align256((size_t)nbmax * 4);
    RQ_TRY(workspace(WS_TMP, out_d_bytes + out_i_bytes + flag_bytes + (on_host ? (size_t)nbmax * kp * 8 : 0), &outs, stream));
    KnnRerankParams rp;
    rp.X = B.X;
    rp.cand = (const uint64_t *)lists;
    rp.out_d = (double *)outs;
    rp.out_id = (uint32_t *)((unsigned char *)outs + out_d_bytes);
    rp.flag = (uint32_t *)((unsigned char *)outs + out_d_bytes + out_i_bytes);
    rp.c64 = on_host ? (double *)((unsigned char *)outs + out_d_bytes + out_i_bytes + flag_bytes) : nullptr;
    rp.n = (uint32_t)n; rp.kp = (uint32_t)kp; rp.k = (uint32_t)k; rp.id_base = (uint32_t)id_base;
    rp.p2 = 1;
    while (rp.p2 < rp.kp) rp.p2 <<= 1;
    rp.d = d;
    rp.gamma1 = 1.0 + gamma; rp.delta = delta;
    next.clear();
    for (int64_t q0 = 0; q0 < nqr; q0 += nbmax) {
      const int64_t nb = std::min(nbmax, nqr - q0);
      rp.Q = dQ.as<float>() + (size_t)q0 * d;
      RQ_TRY(knn_stage1((uint64_t *)lists, B, rp.Q, nb, pl, di.num_cu, clk, widen, stream));
      if (B.esz == 1) RQ_LAUNCH(knn_rerank_kernel<uint8_t>, dim3((uint32_t)nb), dim3(KNN_T), 0, stream, rp);
      else RQ_LAUNCH(knn_rerank_kernel<float>, dim3((uint32_t)nb), dim3(KNN_T), 0, stream, rp);
      clk.mark(widen ? KP_WIDEN : KP_RERANK);
      g_knn_stats[1] += (uint64_t)nb * (uint64_t)kp;
      RQ_HIP(hipStreamSynchronize(stream));
      Timer td;
      hflag.resize((size_t)nb);
      if (!on_host) {
        bd.resize((size_t)nb * k);
        bi.resize((size_t)nb * k);
        RQ_HIP(hipMemcpy(hflag.data(), rp.flag, (size_t)nb * 4, hipMemcpyDeviceToHost));
        RQ_HIP(hipMemcpy(bd.data(), rp.out_d, (size_t)nb * k * 8, hipMemcpyDeviceToHost));
        RQ_HIP(hipMemcpy(bi.data(), rp.out_id, (size_t)nb * k * 4, hipMemcpyDeviceToHost));
        for (int64_t b = 0; b < nb; ++b) {
          const int64_t q = todo[(size_t)(q0 + b)];
          if (hflag[(size_t)b] != 1u) { next.push_back(q); continue; }
          memcpy(hd.data() + (size_t)q * k, bd.data() + (size_t)b * k, (size_t)k * 8);
          memcpy(hi.data() + (size_t)q * k, bi.data() + (size_t)b * k, (size_t)k * 4);
        }
      } else {
        // past what a workgroup sorts: the D64 values come back and std::partial_sort on (D64, id) finishes the query
        hkeys.resize((size_t)nb * kp);
        hc64.resize((size_t)nb * kp);
        RQ_HIP(hipMemcpy(hkeys.data(), lists, (size_t)nb * kp * 8, hipMemcpyDeviceToHost));
        RQ_HIP(hipMemcpy(hc64.data(), rp.c64, (size_t)nb * kp * 8, hipMemcpyDeviceToHost));
        for (int64_t b = 0; b < nb; ++b) {
          const int64_t q = todo[(size_t)(q0 + b)];
          const uint64_t *kb = hkeys.data() + (size_t)b * kp;
          const double *cb = hc64.data() + (size_t)b * kp;
          v.clear();
          for (int64_t c = 0; c < kp; ++c)
            if (kb[c] != KEY_MAX && cb[c] == cb[c]) v.push_back({cb[c], (uint32_t)kb[c]});
          const size_t kk = std::min<size_t>((size_t)k, v.size());
          std::partial_sort(v.begin(), v.begin() + kk, v.end());
          const double t64 = v.size() >= (size_t)k ? v[(size_t)k - 1].first : inf;
          const uint64_t last = kb[kp - 1];
          const uint32_t ob = (uint32_t)(last >> 32);
          const uint32_t ub = (ob & 0x80000000u) ? (ob ^ 0x80000000u) : ~ob;
          float l32;
          memcpy(&l32, &ub, 4);
          const double l = l32 > FLT_MAX ? (double)FLT_MAX : (double)l32;
          volatile double rhs = t64 * (1.0 + gamma);      // two roundings, as the kernel's
          rhs = rhs + delta;
          const bool cert = kp == n || last == KEY_MAX || l > rhs;
          if (!cert) { next.push_back(q); continue; }
          g_knn_stats[4] += 1;
          for (size_t i = 0; i < (size_t)k; ++i) {
            hd[(size_t)q * k + i] = i < kk ? v[i].first : inf;
            hi[(size_t)q * k + i] = (i < kk ? v[i].second : 0xFFFFFFFFu) + (uint32_t)id_base;
          }
        }
      }
      dl += td.ms();
    }
    if (!widen) g_knn_stats[2] = (uint64_t)next.size();
    todo.swap(next);
    kp = std::min<int64_t>(n, 4 * kp);
  }
  clk.collect();
  g_knn_ms[KP_UPLOAD] += ul;
  g_knn_ms[KP_DOWNLOAD] += dl;
  memcpy(dists, hd.data(), hd.size() * 8);
  memcpy(ids, hi.data(), hi.size() * 4);
  return RQ_OK;
}

static void knn_clear() {
  for (int i = 0; i < KP_N; ++i) g_knn_ms[i] = 0;
  for (int i = 0; i < 8; ++i) g_knn_stats[i] = 0;
}

// host-pointer forms: the whole base goes up first (esz 4: f32 rows, 1: byte rows)
static int knn_host(const char *who, double *d64, float *d32, uint32_t *ids, const void *base, int esz, const float *queries,
                    int64_t n, int64_t nq, int d, int k, int id_base) {
  knn_clear();
  if (nq <= 0) return RQ_OK;
  RQ_TRY(knn_check(who, (!d64 && !d32) || !ids || !base || !queries, n, d, k, id_base, d64 != nullptr));
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  Timer tu;
  DevMem dX;
  // a byte base keeps its address modulo 16 on the device: the loaders then take the widths they would take on a sub-range of a
  // larger resident base that starts where the caller's rows start
  const size_t shift = esz == 1 ? (size_t)((uintptr_t)base & 15) : 0;
  RQ_TRY(dX.alloc((size_t)n * d * esz + shift));
  void *dbase = (unsigned char *)dX.p + shift;
  RQ_HIP(hipMemcpy(dbase, base, (size_t)n * d * esz, hipMemcpyHostToDevice));
  g_knn_ms[KP_UPLOAD] += tu.ms();
  const KnnBase B{dbase, esz, n, d};
  const int rc = d64 ? knn_resident(d64, ids, B, queries, nq, k, id_base) : knn_f32_resident(d32, ids, B, queries, nq, k, id_base);
  if (rc != RQ_OK) (void)hipDeviceSynchronize();     // nothing of the call may still read dX when it is freed
  return rc;
}

}  // namespace rq

using namespace rq;

extern "C" {

int rq_knn_f32(float *dists, uint32_t *ids, const float *base, const float *queries, int64_t n, int64_t nq, int d, int k,
               int id_base) {
  return knn_host("rq_knn_f32", nullptr, dists, ids, base, 4, queries, n, nq, d, k, id_base);
}

int rq_knn(double *dists, uint32_t *ids, const float *base, const float *queries, int64_t n, int64_t nq, int d, int k,
           int id_base) {
  return knn_host("rq_knn", dists, nullptr, ids, base, 4, queries, n, nq, d, k, id_base);
}

int rq_knn_bytes(double *dists, uint32_t *ids, const uint8_t *base, const float *queries, int64_t n, int64_t nq, int d, int k,
                 int id_base) {
  return knn_host("rq_knn_bytes", dists, nullptr, ids, base, 1, queries, n, nq, d, k, id_base);
}

int rq_dataset_knn(rq_dataset *ds, double *dists, uint32_t *ids, const float *queries, int64_t nq, int k, int id_base) {
  knn_clear();
  DatasetView v;
  if (!dataset_view(ds, &v)) return fail(RQ_EINVAL, "rq_dataset_knn: NULL dataset");
  if (nq <= 0) return RQ_OK;
  RQ_TRY(knn_check("rq_dataset_knn", !dists || !ids || !queries, v.n, v.d, k, id_base, true));
  SavedDevice saved;
  RQ_HIP(hipSetDevice(v.device));
  const KnnBase B{v.X, v.esz, v.n, v.d};
  const int rc = knn_resident(dists, ids, B, queries, nq, k, id_base);
  if (rc != RQ_OK) (void)hipDeviceSynchronize();
  return rc;
}

int rq_last_knn_stats(uint64_t *out8) {
  if (!out8) return fail(RQ_EINVAL, "rq_last_knn_stats: null pointer");
  for (int i = 0; i < 8; ++i) out8[i] = g_knn_stats[i];
  return RQ_OK;
}

int rq_last_knn_timing(double *ms, int cap) {
  if (!ms) return fail(RQ_EINVAL, "rq_last_knn_timing: null pointer");
  for (int i = 0; i < cap && i < KP_N; ++i) ms[i] = g_knn_ms[i];
  return RQ_OK;
}

int64_t rq_test_knn_chunk_rows(int64_t rows) { return g_knn_chunk_rows.exchange(rows > 0 ? rows : 0); }

int rq_knn_plan(int64_t n, int64_t nq, int d, int k, int64_t *out, int cap) {
  if (!out || cap < 6) return fail(RQ_EINVAL, "rq_knn_plan: out needs 6 entries");
  if (n < 1 || n >= (1LL << 31) || nq < 1 || d < 1 || k < 1 || k > n) return fail(RQ_EINVAL, "rq_knn_plan: bad shape");
  const KnnPlan pl = knn_plan(n, nq, knn_first_kp(n, k));
  out[0] = pl.kp; out[1] = pl.rows; out[2] = pl.chunks; out[3] = pl.batch; out[4] = (int64_t)pl.bytes; out[5] = pl.forced;
  for (int i = 6; i < cap; ++i) out[i] = 0;
  return RQ_OK;
}

}  // extern "C"
