// rq_lsq.hip -- LSQ codebook update (src/codebook_update.jl:96-206 fast_bin_matmul / update_codebooks_fast_bin, the
// "fastbin" method of update_codebooks :235-277) and the LSQ training loop (src/LSQ.jl:323-372 train_lsq,
// src/LSQ_GPU.jl:267-319 train_lsq_cuda) on gfx950; contract in DESIGN.md section 2.
//
// The normal equations (B'B + rho I) C = B'X of the one-hot code matrix B:
//   lsq_tile_hist_kernel   per (tile of LSQ_TILE rows, codebook): LDS histogram of the codes (integer atomics)
//   lsq_scan_kernel        per codebook: exclusive scan over (code, tile) -> each tile's first slot per code, and the
//                          segment bounds segs[i][a] (segs[i][a+1] - segs[i][a] = count_i(a))
//   lsq_scatter_kernel     per (tile, codebook): stable counting sort of the row ids by code (ballot match per wavefront)
//   lsq_pair_kernel        pair counts of codebooks i < j into a u32 mh x mh matrix (integer atomics: exact, order-free)
//   lsq_bsum_kernel        b[(i,a)][k] = sum over the rows of segment (i,a), ascending, in f64 from +0, lanes over k
//   lsq_assemble_kernel    A = the full symmetric matrix, fl64(count + rho) on the diagonal
// Past 256 codewords (int16 codes, 2 <= h <= RQ_MAX_H16) the sort is two stable passes of the same trio,
// the low 8 bits of the code and then its high 7 bits over the first pass's list (an LSD radix sort: LDS stays at 256 counters),
// and the segment bounds come from
//   lsq_code_hist_kernel   cnt[i][a] = rows with code a in codebook i (integer atomics)
//   lsq_segs_scan_kernel   per codebook: segs[i][0..h] = the exclusive scan of cnt[i]
// The solve: blocked right-looking Cholesky A = L L' (NB = 64; one-workgroup diagonal factor, a row-per-thread panel
// solve and an f64 SYRK/GEMM update of the trailing matrix), forward and back substitution with d right-hand sides,
// then C = (float) A^-1 b in the [m][h][d] image rq_encode_icm reads.  Every sum runs in a fixed order and no float
// atomic is used, so the result is bitwise reproducible.
#include "rq_internal.h"

#include <math.h>

#include <vector>

namespace rq {

namespace {

constexpr int LSQ_MAX_M = 16;
constexpr int LSQ_TILE = 4096;   // rows per tile of the bucket sort
constexpr int NB = 64;           // Cholesky block
constexpr int GT = 64;           // output tile of the GEMM update
constexpr int KC = 32;           // K chunk of the GEMM update staged in LDS

// ---- counting sort of the row ids by code, per codebook ------------------------------------------------------------
// The sort key of pass PASS: the code's low 8 bits, then its high 7 (a byte code has pass 0 only, and is its own key).
template <int PASS, class Code>
__device__ __forceinline__ int lsq_digit(Code c) {
  return PASS == 0 ? ((int)c & 255) : ((int)c >> 8);
}

// Pass 0 takes the rows in their own order; pass 1 takes position p's row from pass 0's list `in` ([m][n], or null).
// nd = the number of key values of the pass (h when h <= 256, else 256 and then ceil(h / 256)).
template <class Code, int PASS>
__global__ __launch_bounds__(256) void lsq_tile_hist_kernel(uint32_t *th, const Code *codes, const uint32_t *in, int64_t n, int m,
                                                            int nd, int ntiles) {
  __shared__ uint32_t hist[256];
  const int tile = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  const uint32_t *ids = PASS ? in + (size_t)i * n : nullptr;
  const int64_t r0 = (int64_t)tile * LSQ_TILE, r1 = std::min<int64_t>(n, r0 + LSQ_TILE);
  for (int64_t r = r0 + tid; r < r1; r += 256) {
    const int64_t row = PASS ? (int64_t)ids[r] : r;
    atomicAdd(&hist[lsq_digit<PASS>(codes[row * m + i])], 1u);
  }
  __syncthreads();
  if (tid < nd) th[((size_t)i * nd + tid) * ntiles + tile] = hist[tid];
}

// th[i] (h x ntiles, code-major) -> exclusive prefix sums in place; SEGS: segs[i][a] = first slot of code a, segs[i][h] = n
// (the passes of the wide sort scan their key values and leave segs to lsq_segs_scan_kernel)
template <bool SEGS>
__global__ __launch_bounds__(256) void lsq_scan_kernel(uint32_t *th, uint32_t *segs, int64_t n, int h, int ntiles) {
  __shared__ uint32_t part[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  uint32_t *t = th + (size_t)i * h * ntiles;
  const int64_t L = (int64_t)h * ntiles, chunk = (L + 255) / 256;
  const int64_t beg = std::min<int64_t>(L, tid * chunk), end = std::min<int64_t>(L, beg + chunk);
  uint32_t s = 0;
  for (int64_t j = beg; j < end; ++j) s += t[j];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int q = 0; q < 256; ++q) {
      const uint32_t v = part[q];
      part[q] = run;
      run += v;
    }
  }
  __syncthreads();
  uint32_t run = part[tid];
  for (int64_t j = beg; j < end; ++j) {
    const uint32_t v = t[j];
    t[j] = run;
    if (SEGS && j % ntiles == 0) segs[(size_t)i * (h + 1) + j / ntiles] = run;
    run += v;
  }
  if (SEGS && tid == 0) segs[(size_t)i * (h + 1) + h] = (uint32_t)n;
}

// Rows of a tile in passes of 256 (4 wavefronts x 64 lanes, ascending); a lane's slot = the code's running slot + the
// counts of the same code in earlier wavefronts of the pass + its rank among the lanes of its wavefront with that code.
// Stable, so pass 1 over pass 0's list leaves every (codebook, code) segment in ascending row order.
template <class Code, int PASS>
__global__ __launch_bounds__(256) void lsq_scatter_kernel(uint32_t *sorted, const uint32_t *th, const Code *codes,
                                                          const uint32_t *in, int64_t n, int m, int nd, int ntiles) {
  __shared__ uint32_t run[256];
  __shared__ uint32_t wc[4][256];
  const int tile = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  if (tid < nd) run[tid] = th[((size_t)i * nd + tid) * ntiles + tile];
  for (int q = 0; q < 4; ++q) wc[q][tid] = 0;
  __syncthreads();
  uint32_t *out = sorted + (size_t)i * n;
  const uint32_t *ids = PASS ? in + (size_t)i * n : nullptr;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int64_t r0 = (int64_t)tile * LSQ_TILE, r1 = std::min<int64_t>(n, r0 + LSQ_TILE);
  for (int64_t p0 = r0; p0 < r1; p0 += 256) {
    const int64_t p = p0 + tid;
    const bool valid = p < r1;
    const int64_t r = !valid ? 0 : PASS ? (int64_t)ids[p] : p;
    const int c = valid ? lsq_digit<PASS>(codes[r * m + i]) : 0;
    uint64_t mask = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (c >> bit) & 1;
      const uint64_t bb = __ballot(valid && on);
      mask &= on ? bb : ~bb;
    }
    const uint32_t rank = (uint32_t)__popcll(mask & lt);
    if (valid && rank == 0) wc[w][c] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (valid) {
      uint32_t pos = run[c] + rank;
      for (int q = 0; q < w; ++q) pos += wc[q][c];
      out[pos] = (uint32_t)r;
    }
    __syncthreads();
    if (tid < nd) {
      run[tid] += wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
      wc[0][tid] = wc[1][tid] = wc[2][tid] = wc[3][tid] = 0;
    }
    __syncthreads();
  }
}

// ---- the segment bounds past 256 codewords ---------------------------------------------------------------------------
// cnt [m][h], zeroed by the caller; codes in range (checked before any work), so every index is inside cnt
__global__ __launch_bounds__(256) void lsq_code_hist_kernel(uint32_t *cnt, const int16_t *codes, int64_t nelem, int m, int h) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nelem; e += (int64_t)gridDim.x * 256)
    atomicAdd(&cnt[(size_t)(e % m) * h + (int)codes[e]], 1u);
}

// segs[i][a] = the rows of codebook i with a code below a, a = 0..h (segs[i][h] = n): a chunk of the codes per thread
__global__ __launch_bounds__(256) void lsq_segs_scan_kernel(uint32_t *segs, const uint32_t *cnt, int64_t n, int h) {
  __shared__ uint32_t part[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const uint32_t *c = cnt + (size_t)i * h;
  uint32_t *out = segs + (size_t)i * (h + 1);
  const int chunk = (h + 255) / 256, beg = std::min(h, tid * chunk), end = std::min(h, beg + chunk);
  uint32_t s = 0;
  for (int a = beg; a < end; ++a) s += c[a];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int q = 0; q < 256; ++q) {
      const uint32_t v = part[q];
      part[q] = run;
      run += v;
    }
  }
  __syncthreads();
  uint32_t run = part[tid];
  for (int a = beg; a < end; ++a) {
    out[a] = run;
    run += c[a];
  }
  if (tid == 0) out[h] = (uint32_t)n;
}

// ---- A -------------------------------------------------------------------------------------------------------------
template <class Code>
__global__ __launch_bounds__(256) void lsq_pair_kernel(uint32_t *P, const Code *codes, int64_t n, int m, int h) {
  const int mh = m * h;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    int b[LSQ_MAX_M];
#pragma unroll
    for (int i = 0; i < LSQ_MAX_M; ++i) b[i] = i < m ? i * h + (int)codes[r * m + i] : 0;
#pragma unroll
    for (int i = 0; i < LSQ_MAX_M; ++i)
#pragma unroll
      for (int j = i + 1; j < LSQ_MAX_M; ++j)
        if (j < m) atomicAdd(&P[(size_t)b[i] * mh + b[j]], 1u);
  }
}

__global__ __launch_bounds__(256) void lsq_assemble_kernel(double *A, const uint32_t *P, const uint32_t *segs, int m,
                                                           int h, double rho) {
  const int mh = m * h;
  const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (c >= mh) return;
  const int i = r / h, a = r - i * h, j = c / h;
  double v;
  if (i == j) {
    const uint32_t *s = segs + (size_t)i * (h + 1);
    v = (r == c) ? (double)(s[a + 1] - s[a]) + rho : 0.0;
  } else {
    v = (double)(i < j ? P[(size_t)r * mh + c] : P[(size_t)c * mh + r]);
  }
  A[(size_t)r * mh + c] = v;
}

// ---- b -------------------------------------------------------------------------------------------------------------
// one workgroup per (codebook, code) segment; thread t sums dims t, t + blockDim, ... over the segment's rows in order
__global__ __launch_bounds__(256) void lsq_bsum_kernel(double *b, const float *X, const uint32_t *sorted,
                                                       const uint32_t *segs, int64_t n, int d, int h) {
  const int seg = blockIdx.x, i = seg / h, a = seg - i * h;
  const uint32_t beg = segs[(size_t)i * (h + 1) + a], end = segs[(size_t)i * (h + 1) + a + 1];
  const uint32_t *ids = sorted + (size_t)i * n;
  for (int k = threadIdx.x; k < d; k += blockDim.x) {
    double acc = 0.0;
    int64_t j = beg;
    for (; j + 8 <= (int64_t)end; j += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = X[(size_t)ids[j + u] * d + k];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = acc + (double)v[u];
    }
    for (; j < (int64_t)end; ++j) acc = acc + (double)X[(size_t)ids[j] * d + k];
    b[(size_t)seg * d + k] = acc;
  }
}

// ---- the SPD solve -------------------------------------------------------------------------------------------------
// A[k..k+nb) x [k..k+nb) (lower triangle) <- its Cholesky factor; one workgroup, the block in LDS
__global__ __launch_bounds__(256) void lsq_chol_diag_kernel(double *A, int mh, int k, int nb) {
  __shared__ double T[NB][NB + 1];
  const int tid = threadIdx.x;
  for (int e = tid; e < nb * nb; e += 256) {
    const int r = e / nb, c = e - r * nb;
    T[r][c] = c <= r ? A[(size_t)(k + r) * mh + k + c] : 0.0;
  }
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    if (tid == 0) T[j][j] = sqrt(T[j][j]);
    __syncthreads();
    if (tid > j && tid < nb) T[tid][j] = T[tid][j] / T[j][j];
    __syncthreads();
    for (int e = tid; e < nb * nb; e += 256) {
      const int r = e / nb, c = e - r * nb;
      if (c > j && c <= r) T[r][c] = __builtin_fma(-T[r][j], T[c][j], T[r][c]);
    }
    __syncthreads();
  }
  for (int e = tid; e < nb * nb; e += 256) {
    const int r = e / nb, c = e - r * nb;
    if (c <= r) A[(size_t)(k + r) * mh + k + c] = T[r][c];
  }
}

// the panel below the diagonal block: row t of this workgroup solves x L_kk' = a (sequential in the column index)
__global__ __launch_bounds__(64) void lsq_chol_panel_kernel(double *A, int mh, int k, int nb) {
  __shared__ double L[NB][NB];
  __shared__ double PT[NB][64];   // PT[col][row]: lane-consecutive rows, no bank conflicts
  const int t = threadIdx.x;
  const int i0 = k + nb + blockIdx.x * 64;
  for (int e = t; e < nb * nb; e += 64) {
    const int r = e / nb, c = e - r * nb;
    L[r][c] = A[(size_t)(k + r) * mh + k + c];
  }
  const int rows = std::min(64, mh - i0);
  for (int e = t; e < rows * nb; e += 64) {
    const int r = e / nb, c = e - r * nb;
    PT[c][r] = A[(size_t)(i0 + r) * mh + k + c];
  }
  __syncthreads();
  if (t < rows) {
    for (int j = 0; j < nb; ++j) {
      double x = PT[j][t];
      for (int l = 0; l < j; ++l) x = __builtin_fma(-PT[l][t], L[j][l], x);
      PT[j][t] = x / L[j][j];
    }
  }
  __syncthreads();
  for (int e = t; e < rows * nb; e += 64) {
    const int r = e / nb, c = e - r * nb;
    A[(size_t)(i0 + r) * mh + k + c] = PT[c][r];
  }
}

// D(i, j) -= sum_{kk < K} P(i, kk) Q(j, kk), i < M, j < N (lower: j <= i only); P(i, kk) = P[i * ps0 + kk * ps1],
// Q likewise.  64 x 64 outputs per workgroup, 4 x 4 per thread, the K sum in ascending kk from +0, then one subtraction.
__global__ __launch_bounds__(256) void lsq_gemm_sub_kernel(double *D, int64_t ldd, int M, int N, const double *P,
                                                           int64_t ps0, int64_t ps1, const double *Q, int64_t qs0,
                                                           int64_t qs1, int K, int lower) {
  __shared__ double Ps[KC][GT];
  __shared__ double Qs[KC][GT];
  const int i0 = blockIdx.y * GT, j0 = blockIdx.x * GT;
  if (lower && j0 > i0 + GT - 1) return;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  for (int k0 = 0; k0 < K; k0 += KC) {
    for (int e = tid; e < KC * GT; e += 256) {
      int kk, ii;
      if (ps1 == 1) { kk = e % KC; ii = e / KC; } else { ii = e % GT; kk = e / GT; }
      Ps[kk][ii] = (i0 + ii < M && k0 + kk < K) ? P[(int64_t)(i0 + ii) * ps0 + (int64_t)(k0 + kk) * ps1] : 0.0;
      int kq, jj;
      if (qs1 == 1) { kq = e % KC; jj = e / KC; } else { jj = e % GT; kq = e / GT; }
      Qs[kq][jj] = (j0 + jj < N && k0 + kq < K) ? Q[(int64_t)(j0 + jj) * qs0 + (int64_t)(k0 + kq) * qs1] : 0.0;
    }
    __syncthreads();
    const int kn = std::min(KC, K - k0);
    for (int kk = 0; kk < kn; ++kk) {
      double p[4], q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) p[u] = Ps[kk][ty + 16 * u];
#pragma unroll
      for (int v = 0; v < 4; ++v) q[v] = Qs[kk][tx + 16 * v];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = __builtin_fma(p[u], q[v], acc[u][v]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < M && j < N && (!lower || j <= i)) D[(int64_t)i * ldd + j] -= acc[u][v];
    }
}

// Y[k..k+nb) <- L_kk^-1 Y[k..k+nb) (fwd) or L_kk'^-1 Y[k..k+nb) (!fwd); thread t owns column j0 + t
__global__ __launch_bounds__(64) void lsq_trsv_block_kernel(double *Y, const double *A, int mh, int d, int k, int nb,
                                                            int fwd) {
  __shared__ double L[NB][NB];
  __shared__ double Ys[NB][64];
  const int t = threadIdx.x, j = blockIdx.x * 64 + t;
  for (int e = t; e < nb * nb; e += 64) {
    const int r = e / nb, c = e - r * nb;
    L[r][c] = A[(size_t)(k + r) * mh + k + c];
  }
  const bool ok = j < d;
  for (int r = 0; r < nb; ++r) Ys[r][t] = ok ? Y[(size_t)(k + r) * d + j] : 0.0;
  __syncthreads();
  if (fwd) {
    for (int r = 0; r < nb; ++r) {
      double x = Ys[r][t];
      for (int l = 0; l < r; ++l) x = __builtin_fma(-L[r][l], Ys[l][t], x);
      Ys[r][t] = x / L[r][r];
    }
  } else {
    for (int r = nb - 1; r >= 0; --r) {
      double x = Ys[r][t];
      for (int l = r + 1; l < nb; ++l) x = __builtin_fma(-L[l][r], Ys[l][t], x);
      Ys[r][t] = x / L[r][r];
    }
  }
  if (ok)
    for (int r = 0; r < nb; ++r) Y[(size_t)(k + r) * d + j] = Ys[r][t];
}

__global__ __launch_bounds__(256) void lsq_to_f32_kernel(float *C, const double *Y, int64_t cnt) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (int64_t)gridDim.x * 256)
    C[e] = (float)Y[e];
}

// obj = mean of the per-row costs: f64, each thread a strided sum in row order, then a fixed LDS tree
__global__ __launch_bounds__(1024) void lsq_mean_kernel(double *out, const float *cost, int64_t n) {
  __shared__ double part[1024];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t r = tid; r < n; r += 1024) s = s + (double)cost[r];
  part[tid] = s;
  __syncthreads();
  for (int off = 512; off >= 1; off >>= 1) {
    if (tid < off) part[tid] = part[tid] + part[tid + off];
    __syncthreads();
  }
  if (tid == 0) *out = part[0] / (double)n;
}

// hmax: 256 for the byte entries, RQ_MAX_H16 for the entries over int16 codes
int lsq_check(const void *out0, const void *out1, const void *X, const void *codes, int64_t n, int d, int m, int h,
              double rho, const char *who, int hmax = 256) {
  if (m < 1 || m > LSQ_MAX_M) return fail(RQ_EINVAL, "%s: m=%d outside 1..%d", who, m, LSQ_MAX_M);
  if (h < 2 || h > hmax) return fail(RQ_EINVAL, "%s: h=%d outside 2..%d", who, h, hmax);
  if (d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);
  if (n < 0 || n > (int64_t)UINT32_MAX)
    return fail(RQ_EINVAL, "%s: n=%lld outside 0..%u (the u32 counters)", who, (long long)n, UINT32_MAX);
  if (!(rho > 0.0) || !isfinite(rho)) return fail(RQ_EINVAL, "%s: rho=%g must be finite and > 0", who, rho);
  if (!out0 || !out1) return fail(RQ_EINVAL, "%s: null output pointer", who);
  if (n > 0 && (!X || !codes)) return fail(RQ_EINVAL, "%s: null pointer", who);
  return RQ_OK;
}

// Phase clock of the host-pointer entries (which synchronise anyway): hipEvents between the phases of the calling
// thread's last call, read at its end.  The device entries queue no events and leave the clock at zero.
// PH_OTHER: what a training call queues besides the updates and encodes (R'X, the rotation back, the obj means)
enum { PH_COUNT, PH_SORT, PH_B, PH_ASSEMBLE, PH_SOLVE, PH_OTHER, PH_ENCODE, PH_N };
thread_local double g_lsq_ms[PH_N] = {0};

// The limit of the entries over int16 codes: A is then at most 2 GiB of f64 (the library's per-slot scratch figure), the u32 pair
// counts at most 1 GiB.  The byte entries stop at 16 * 256 = 4096.
constexpr int LSQ_MAX_MH = 16384;

// WS_LSQ_S of one call: pair counts | tile histograms | segment bounds | per-code counts (h > 256) | the sorted row lists
struct LsqScratch {
  int ntiles, nd;       // tiles of LSQ_TILE rows; key values of the first sort pass
  size_t pair_bytes, th_bytes, seg_bytes, cnt_bytes, sort_bytes;
  size_t total() const { return pair_bytes + th_bytes + seg_bytes + cnt_bytes + sort_bytes; }
};

// with_A false: b and the segments alone, no mh x mh buffer
LsqScratch lsq_scratch(int64_t n, int m, int h, bool with_A) {
  LsqScratch L;
  const size_t mh = (size_t)m * h;
  L.ntiles = (int)std::max<int64_t>(1, (n + LSQ_TILE - 1) / LSQ_TILE);
  L.nd = std::min(h, 256);
  L.pair_bytes = with_A ? mh * mh * 4 : 0;
  L.th_bytes = (size_t)m * L.nd * L.ntiles * 4;
  L.seg_bytes = ((size_t)m * (h + 1) * 4 + 255) & ~(size_t)255;
  L.cnt_bytes = h > 256 ? (mh * 4 + 255) & ~(size_t)255 : 0;
  L.sort_bytes = (size_t)m * n * 4 * (h > 256 ? 2 : 1);     // h > 256: one list per pass
  return L;
}

// Where the parts of WS_LSQ_S lie for one shape: a function of (n, m, h, with_A) and the buffer's address alone, so a later update
// over the same codes finds the segment bounds and the sorted lists of an earlier one (update_again_dev)
struct LsqLists {
  uint32_t *P, *th, *segs, *cnt, *list0;
  const uint32_t *sorted;   // the final lists [m][n]: list0, or the second pass's past 256 codewords
};

LsqLists lsq_lists(void *ws, const LsqScratch &L, int64_t n, int m, int h) {
  LsqLists Q;
  Q.P = (uint32_t *)ws;
  Q.th = Q.P + L.pair_bytes / 4;
  Q.segs = Q.th + L.th_bytes / 4;
  Q.cnt = Q.segs + L.seg_bytes / 4;
  Q.list0 = Q.cnt + L.cnt_bytes / 4;
  Q.sorted = h > 256 ? Q.list0 + (size_t)m * n : Q.list0;
  return Q;
}

// The part of the normal equations that the codes alone decide, up to the sort: the pair counts (A non-null), the segment bounds
// and the sorted row lists, left in WS_LSQ_S.  Marks PH_COUNT and PH_SORT.
template <class Code>
int normal_eq_codes_dev(LsqLists *out, bool with_A, const Code *codes, int64_t n, int m, int h, hipStream_t s, PhaseClock &clk) {
  const LsqScratch L = lsq_scratch(n, m, h, with_A);
  const int ntiles = L.ntiles;
  void *ws = nullptr;
  RQ_TRY(workspace(WS_LSQ_S, L.total(), &ws, s));
  const LsqLists Q = lsq_lists(ws, L, n, m, h);
  uint32_t *P = Q.P, *th = Q.th, *segs = Q.segs, *cnt = Q.cnt, *sorted = Q.list0;
  if (with_A) RQ_HIP(hipMemsetAsync(P, 0, L.pair_bytes, s));
  RQ_HIP(hipMemsetAsync(th, 0, L.th_bytes, s));
  if (with_A && n > 0 && m > 1) {
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(lsq_pair_kernel<Code>, dim3(grid), dim3(256), 0, s, P, codes, n, m, h);
    RQ_HIP(hipGetLastError());
  }
  if constexpr (std::is_same<Code, int16_t>::value) {
    if (h > 256) {
      RQ_HIP(hipMemsetAsync(cnt, 0, L.cnt_bytes, s));
      const int64_t nelem = n * m;
      if (nelem > 0)
        RQ_LAUNCH(lsq_code_hist_kernel, dim3((unsigned)std::min<int64_t>((nelem + 255) / 256, 8192)), dim3(256), 0, s, cnt, codes,
                  nelem, m, h);
    }
  }
  clk.mark(PH_COUNT);
  if (h <= 256) {
    if (n > 0) {
      hipLaunchKernelGGL((lsq_tile_hist_kernel<Code, 0>), dim3(ntiles, m), dim3(256), 0, s, th, codes, (const uint32_t *)nullptr, n,
                         m, h, ntiles);
      RQ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(lsq_scan_kernel<true>, dim3(m), dim3(256), 0, s, th, segs, n, h, ntiles);
    RQ_HIP(hipGetLastError());
    if (n > 0) {
      hipLaunchKernelGGL((lsq_scatter_kernel<Code, 0>), dim3(ntiles, m), dim3(256), 0, s, sorted, th, codes,
                         (const uint32_t *)nullptr, n, m, h, ntiles);
      RQ_HIP(hipGetLastError());
    }
  } else if constexpr (std::is_same<Code, int16_t>::value) {
    // LSD radix sort: the low 8 bits, then the high 7 over the first list; both passes are stable
    uint32_t *list0 = sorted, *list1 = sorted + (size_t)m * n;
    const int nd1 = (h + 255) >> 8;
    if (n > 0) {
      const uint32_t *none = nullptr;
      RQ_LAUNCH((lsq_tile_hist_kernel<Code, 0>), dim3(ntiles, m), dim3(256), 0, s, th, codes, none, n, m, 256, ntiles);
      RQ_LAUNCH(lsq_scan_kernel<false>, dim3(m), dim3(256), 0, s, th, (uint32_t *)nullptr, n, 256, ntiles);
      RQ_LAUNCH((lsq_scatter_kernel<Code, 0>), dim3(ntiles, m), dim3(256), 0, s, list0, (const uint32_t *)th, codes, none, n, m,
                256, ntiles);
      RQ_LAUNCH((lsq_tile_hist_kernel<Code, 1>), dim3(ntiles, m), dim3(256), 0, s, th, codes, (const uint32_t *)list0, n, m, nd1,
                ntiles);
      RQ_LAUNCH(lsq_scan_kernel<false>, dim3(m), dim3(256), 0, s, th, (uint32_t *)nullptr, n, nd1, ntiles);
      RQ_LAUNCH((lsq_scatter_kernel<Code, 1>), dim3(ntiles, m), dim3(256), 0, s, list1, (const uint32_t *)th, codes,
                (const uint32_t *)list0, n, m, nd1, ntiles);
    }
    RQ_LAUNCH(lsq_segs_scan_kernel, dim3(m), dim3(256), 0, s, segs, (const uint32_t *)cnt, n, h);
  }
  clk.mark(PH_SORT);
  *out = Q;
  return RQ_OK;
}

// b [mh][d] <- the segment sums of X over the sorted lists: the one part of the normal equations that reads X.  Marks PH_B.
int normal_eq_b_dev(double *b, const float *X, const LsqLists &Q, int64_t n, int d, int m, int h, hipStream_t s, PhaseClock &clk) {
  const int bt = d <= 64 ? 64 : d <= 128 ? 128 : 256;
  hipLaunchKernelGGL(lsq_bsum_kernel, dim3(m * h), dim3(bt), 0, s, b, X, Q.sorted, (const uint32_t *)Q.segs, n, d, h);
  RQ_HIP(hipGetLastError());
  clk.mark(PH_B);
  return RQ_OK;
}

// A [mh][mh], b [mh][d] f64 (device pointers; arguments checked, codes in range).  Code: uint8_t (h <= 256) or int16_t
// (zero-based, h <= RQ_MAX_H16; at h <= 256 it queues what the byte instantiation queues).  A null (int16 entries only): b and
// the segments alone.  *segs_out (may be null) <- the segment bounds [m][h + 1] in WS_LSQ_S.
template <class Code>
int normal_eq_dev(double *A, double *b, const float *X, const Code *codes, int64_t n, int d, int m, int h, double rho,
                  hipStream_t s, PhaseClock &clk, const uint32_t **segs_out = nullptr) {
  const int mh = m * h;
  LsqLists Q;
  RQ_TRY(normal_eq_codes_dev(&Q, A != nullptr, codes, n, m, h, s, clk));
  RQ_TRY(normal_eq_b_dev(b, X, Q, n, d, m, h, s, clk));
  if (A) {
    hipLaunchKernelGGL(lsq_assemble_kernel, dim3((mh + 255) / 256, mh), dim3(256), 0, s, A, (const uint32_t *)Q.P,
                       (const uint32_t *)Q.segs, m, h, rho);
    RQ_HIP(hipGetLastError());
  }
  clk.mark(PH_ASSEMBLE);
  if (segs_out) *segs_out = Q.segs;
  return RQ_OK;
}

// A <- its Cholesky factor (lower)
int spd_factor_dev(double *A, int mh, hipStream_t s) {
  for (int k = 0; k < mh; k += NB) {
    const int nb = std::min(NB, mh - k), rest = mh - k - nb;
    RQ_LAUNCH(lsq_chol_diag_kernel, dim3(1), dim3(256), 0, s, A, mh, k, nb);
    if (rest > 0) {
      RQ_LAUNCH(lsq_chol_panel_kernel, dim3((rest + 63) / 64), dim3(64), 0, s, A, mh, k, nb);
      double *pan = A + (size_t)(k + nb) * mh + k;
      const unsigned tiles = (unsigned)((rest + GT - 1) / GT);
      RQ_LAUNCH(lsq_gemm_sub_kernel, dim3(tiles, tiles), dim3(256), 0, s, pan + nb, (int64_t)mh, rest, rest,
                (const double *)pan, (int64_t)mh, (int64_t)1, (const double *)pan, (int64_t)mh, (int64_t)1, nb, 1);
    }
  }
  return RQ_OK;
}

// Y [mh][d] <- (L L')^-1 Y with L the factor spd_factor_dev left in A: forward, then back substitution
int spd_subst_dev(const double *A, double *Y, int mh, int d, hipStream_t s) {
  const unsigned cgrid = (unsigned)((d + 63) / 64), ntile = (unsigned)((d + GT - 1) / GT);
  for (int k = 0; k < mh; k += NB) {   // L y = b
    const int nb = std::min(NB, mh - k), rest = mh - k - nb;
    RQ_LAUNCH(lsq_trsv_block_kernel, dim3(cgrid), dim3(64), 0, s, Y, A, mh, d, k, nb, 1);
    if (rest > 0)
      RQ_LAUNCH(lsq_gemm_sub_kernel, dim3(ntile, (unsigned)((rest + GT - 1) / GT)), dim3(256), 0, s,
                Y + (size_t)(k + nb) * d, (int64_t)d, rest, d, (const double *)(A + (size_t)(k + nb) * mh + k),
                (int64_t)mh, (int64_t)1, (const double *)(Y + (size_t)k * d), (int64_t)1, (int64_t)d, nb, 0);
  }
  for (int k = ((mh - 1) / NB) * NB; k >= 0; k -= NB) {   // L' x = y
    const int nb = std::min(NB, mh - k);
    RQ_LAUNCH(lsq_trsv_block_kernel, dim3(cgrid), dim3(64), 0, s, Y, A, mh, d, k, nb, 0);
    if (k > 0)
      RQ_LAUNCH(lsq_gemm_sub_kernel, dim3(ntile, (unsigned)((k + GT - 1) / GT)), dim3(256), 0, s, Y, (int64_t)d, k, d,
                (const double *)(A + (size_t)k * mh), (int64_t)1, (int64_t)mh, (const double *)(Y + (size_t)k * d),
                (int64_t)1, (int64_t)d, nb, 0);
  }
  return RQ_OK;
}

// A <- its Cholesky factor (lower), Y [mh][d] <- A^-1 Y
int spd_solve_dev(double *A, double *Y, int mh, int d, hipStream_t s) {
  RQ_TRY(spd_factor_dev(A, mh, s));
  return spd_subst_dev(A, Y, mh, d, s);
}

// C [m][h][d] f32 <- the fastbin update of (X, codes) (device pointers; arguments checked, codes in range)
template <class Code>
int update_dev(float *C, const float *X, const Code *codes, int64_t n, int d, int m, int h, double rho, hipStream_t s,
               PhaseClock &clk) {
  const int mh = m * h;
  void *wa = nullptr, *wb = nullptr;
  RQ_TRY(workspace(WS_LSQ_A, (size_t)mh * mh * 8, &wa, s));
  RQ_TRY(workspace(WS_LSQ_B, (size_t)mh * d * 8, &wb, s));
  double *A = (double *)wa, *b = (double *)wb;
  RQ_TRY(normal_eq_dev(A, b, X, codes, n, d, m, h, rho, s, clk));
  RQ_TRY(spd_solve_dev(A, b, mh, d, s));
  const int64_t cnt = (int64_t)mh * d;
  RQ_LAUNCH(lsq_to_f32_kernel, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 8192)), dim3(256), 0, s, C,
            (const double *)b, cnt);
  clk.mark(PH_SOLVE);
  return RQ_OK;
}

// update_dev over int16 codes that also notes where it left the Cholesky factor (WS_LSQ_A) and the segment bounds and sorted
// lists (WS_LSQ_S): what a second update over the SAME codes can start from (update_again_dev)
int update_keep_dev(float *C, const float *X, const int16_t *codes, int64_t n, int d, int m, int h, double rho, hipStream_t s,
                    PhaseClock &clk, LsqKept *kept) {
  *kept = LsqKept();
  RQ_TRY(update_dev(C, X, codes, n, d, m, h, rho, s, clk));
  const size_t mh = (size_t)m * h;
  void *wa = nullptr, *ws = nullptr;
  kept->a_bytes = mh * mh * 8;
  kept->s_bytes = lsq_scratch(n, m, h, true).total();
  RQ_TRY(workspace(WS_LSQ_A, kept->a_bytes, &wa, s));      // the buffers update_dev used: they hold these sizes already
  RQ_TRY(workspace(WS_LSQ_S, kept->s_bytes, &ws, s));
  kept->a = wa;
  kept->s = ws;
  return RQ_OK;
}

// C <- the fastbin update of (X, codes) for the codes of the update that filled `kept`: A = B'B + rho I is that update's, so its
// factor, segment bounds and sorted lists stand; b alone is summed anew, then the two substitution sweeps.  *done = false (and
// nothing queued) when either buffer is no longer the one `kept` names, at its size.
int update_again_dev(bool *done, float *C, const float *X, int64_t n, int d, int m, int h, hipStream_t s, PhaseClock &clk,
                     const LsqKept &kept) {
  *done = false;
  const int mh = m * h;
  const LsqScratch L = lsq_scratch(n, m, h, true);
  if (!kept.a || !kept.s || kept.a_bytes != (size_t)mh * mh * 8 || kept.s_bytes != L.total()) return RQ_OK;
  void *wa = nullptr, *wb = nullptr, *ws = nullptr;
  RQ_TRY(workspace(WS_LSQ_A, kept.a_bytes, &wa, s));
  RQ_TRY(workspace(WS_LSQ_B, (size_t)mh * d * 8, &wb, s));
  RQ_TRY(workspace(WS_LSQ_S, kept.s_bytes, &ws, s));
  if (wa != kept.a || ws != kept.s) return RQ_OK;
  double *b = (double *)wb;
  RQ_TRY(normal_eq_b_dev(b, X, lsq_lists(ws, L, n, m, h), n, d, m, h, s, clk));
  RQ_TRY(spd_subst_dev((const double *)wa, b, mh, d, s));
  const int64_t cnt = (int64_t)mh * d;
  RQ_LAUNCH(lsq_to_f32_kernel, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 8192)), dim3(256), 0, s, C,
            (const double *)b, cnt);
  clk.mark(PH_SOLVE);
  *done = true;
  return RQ_OK;
}

void lsq_clock_reset() {
  for (int q = 0; q < PH_N; ++q) g_lsq_ms[q] = 0;
}

}  // namespace

// The normal equations and the SPD solve for the chain codebook update (rq_chain.hip); no phase clock.
int lsq_normal_eq_launch(double *A, double *b, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h,
                         double rho, hipStream_t s) {
  PhaseClock clk(s, g_lsq_ms, false);
  return normal_eq_dev(A, b, X, codes, n, d, m, h, rho, s, clk);
}

int lsq_spd_solve_launch(double *A, double *Y, int mh, int d, hipStream_t s) { return spd_solve_dev(A, Y, mh, d, s); }

// b [mh][d] and the segment bounds [m][h + 1] (in WS_LSQ_S) alone, over zero-based int16 codes at any h <= RQ_MAX_H16: what the
// chain update past 256 codewords needs of the normal equations (no mh x mh matrix); no phase clock.
int lsq_b_segs_wide_launch(double *b, const uint32_t **segs, const float *X, const int16_t *codes, int64_t n, int d, int m, int h,
                           double rho, hipStream_t s) {
  PhaseClock clk(s, g_lsq_ms, false);
  return normal_eq_dev<int16_t>(nullptr, b, X, codes, n, d, m, h, rho, s, clk, segs);
}

// The fastbin update and the obj mean for the SR training loop (rq_sr.hip), which keeps a phase clock of its own.
int lsq_update_launch(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h, double rho,
                      hipStream_t s) {
  PhaseClock clk(s, g_lsq_ms, false);
  return update_dev(C, X, codes, n, d, m, h, rho, s, clk);
}

// The same over zero-based int16 codes at 2 <= h <= RQ_MAX_H16 (rq_train_sr_wide).  again == false: the full update, and *kept
// <- what it left behind.  again == true: the codes are those of the update that filled *kept, so only b is summed anew
// (update_again_dev); when *kept no longer holds, the full update runs instead.  *reused <- which of the two ran.
int lsq_update_wide_launch(float *C, const float *X, const int16_t *codes, int64_t n, int d, int m, int h, double rho,
                           hipStream_t s, LsqKept *kept, bool again, bool *reused) {
  PhaseClock clk(s, g_lsq_ms, false);
  *reused = false;
  if (again) RQ_TRY(update_again_dev(reused, C, X, n, d, m, h, s, clk, *kept));
  if (*reused) return RQ_OK;
  return update_keep_dev(C, X, codes, n, d, m, h, rho, s, clk, kept);
}

// The shape rule of the training loops over int16 codes (rq_train_lsq_wide, rq_train_sr_wide), no device touched: nsplits and the
// encoder's tables within its scratch (rq_icm_wide_plan's rule), then m * h within LSQ_MAX_MH (RQ_EUNSUPPORTED)
int lsq_train_wide_shape(const char *who, int64_t n, int d, int m, int h, int nsplits) {
  int64_t none = 0;
  RQ_TRY(rq_icm_wide_plan(n, d, m, h, nsplits, &none, 0));
  if (m * h > LSQ_MAX_MH)
    return fail(RQ_EUNSUPPORTED, "%s: m * h = %d * %d exceeds %d (A would take %zu bytes of f64)", who, m, h, LSQ_MAX_MH,
                (size_t)m * h * m * h * 8);
  return RQ_OK;
}

int upload_rotation(DevMem &dR, DevMem &dRX, const float *R, const float *X, int64_t n, int d, int num_cu, hipStream_t s) {
  const size_t rb = (size_t)d * d * 4;
  std::vector<float> Rt((size_t)d * d);
  for (int i = 0; i < d; ++i)
    for (int k = 0; k < d; ++k) Rt[(size_t)i * d + k] = R[(size_t)k * d + i];
  RQ_TRY(dRX.alloc((size_t)n * d * 4));
  RQ_TRY(dR.alloc(rb * 2));
  RQ_HIP(hipMemcpy(dR.p, R, rb, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dR.as<float>() + (size_t)d * d, Rt.data(), rb, hipMemcpyHostToDevice));
  return rotate_launch(dRX.as<float>(), dR.as<float>(), X, d, n, num_cu, s);
}

int lsq_mean_launch(double *out, const float *cost, int64_t n, hipStream_t s) {
  RQ_LAUNCH(lsq_mean_kernel, dim3(1), dim3(1024), 0, s, out, cost, n);
  return RQ_OK;
}

namespace {

// the encoder of a training loop by code type: rq_icm.hip's over bytes, rq_icm_h16.hip's over int16 codes (no phase clock)
int lsq_encode_dev(uint8_t *B, float *cost, const float *X, const float *C, int64_t n, int d, int m, int h, int ilsiter,
                   int icmiter, int npert, int randord, uint64_t seed, int64_t t0, int nsplits, hipStream_t s) {
  return icm_encode_dev(B, B, cost, X, C, n, d, m, h, ilsiter, icmiter, npert, randord, seed, t0, nsplits, s, nullptr);
}
int lsq_encode_dev(int16_t *B, float *cost, const float *X, const float *C, int64_t n, int d, int m, int h, int ilsiter,
                   int icmiter, int npert, int randord, uint64_t seed, int64_t t0, int nsplits, hipStream_t s) {
  return icm_encode_wide_dev(B, B, cost, X, C, n, d, m, h, ilsiter, icmiter, npert, randord, seed, t0, nsplits, s, nullptr);
}

// rq_train_lsq / rq_train_lsq_wide after their argument checks (src/LSQ.jl:345-371).  codes [n][m] on the host, in
// code_base .. code_base + h - 1 (bytes: code_base 0); the loop runs on zero-based codes.
template <class Code>
int train_lsq_host(float *C, Code *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m, int h, int niter,
                   int ilsiter, int icmiter, int npert, int randord, uint64_t seed, int nsplits, int code_base) {
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  const int mh = m * h;
  const size_t xb = (size_t)n * d * 4, cb = (size_t)mh * d * 4, kb = (size_t)n * m * sizeof(Code);
  DevMem dX, dRX, dR, dC, dC2, dcodes, dcost, dobj;
  RQ_TRY(dX.alloc(xb));
  RQ_TRY(dcodes.alloc(kb));
  RQ_TRY(dC.alloc(cb));
  RQ_TRY(dcost.alloc((size_t)n * 4));
  RQ_TRY(dobj.alloc((size_t)(niter + 1) * 8));
  if (n > 0) {
    RQ_HIP(hipMemcpy(dX.p, X, xb, hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(dcodes.p, codes, kb, hipMemcpyHostToDevice));
  }
  const float *Xd = (const float *)dX.p;
  Code *B = (Code *)dcodes.p;
  float *Cd = (float *)dC.p, *cost = (float *)dcost.p;
  double *objd = (double *)dobj.p;
  const hipStream_t s = nullptr;
  lsq_clock_reset();
  PhaseClock clk(s, g_lsq_ms);
  if constexpr (std::is_same<Code, int16_t>::value) {
    if (code_base) {
      RQ_TRY(add_base_codes_launch(B, n * m, -code_base, s));
      clk.mark(PH_OTHER);
    }
  }
  // C = update(R'X, B); C_i <- R C_i   (src/LSQ.jl:345-350)
  if (R) {
    RQ_TRY(upload_rotation(dR, dRX, R, Xd, n, d, di.num_cu, s));
    RQ_TRY(dC2.alloc(cb));
    const float *Rtd = dR.as<float>() + (size_t)d * d;
    clk.mark(PH_OTHER);
    RQ_TRY(update_dev((float *)dC2.p, (const float *)dRX.p, (const Code *)B, n, d, m, h, 1e-4, s, clk));
    RQ_TRY(rotate_launch(Cd, Rtd, (const float *)dC2.p, d, mh, di.num_cu, s));
    clk.mark(PH_OTHER);
  } else {
    RQ_TRY(update_dev(Cd, Xd, (const Code *)B, n, d, m, h, 1e-4, s, clk));
  }
  // encode call e runs ILS iterations e * ilsiter .. (e + 1) * ilsiter - 1 of one stream
  RQ_TRY(lsq_encode_dev(B, cost, Xd, Cd, n, d, m, h, ilsiter, icmiter, npert, randord, seed, 0, nsplits, s));
  clk.mark(PH_ENCODE);
  for (int it = 1; it <= niter; ++it) {
    // obj[iter] = qerror(X, B, C): the mean of the previous encode's per-row costs (NaN when n = 0: a mean of no rows)
    RQ_LAUNCH(lsq_mean_kernel, dim3(1), dim3(1024), 0, s, objd + (it - 1), (const float *)cost, n);
    clk.mark(PH_OTHER);
    RQ_TRY(update_dev(Cd, Xd, (const Code *)B, n, d, m, h, 1e-4, s, clk));
    RQ_TRY(lsq_encode_dev(B, cost, Xd, Cd, n, d, m, h, ilsiter, icmiter, npert, randord, seed, (int64_t)it * ilsiter, nsplits, s));
    clk.mark(PH_ENCODE);
  }
  if constexpr (std::is_same<Code, int16_t>::value) {
    if (code_base) {
      RQ_TRY(add_base_codes_launch(B, n * m, code_base, s));
      clk.mark(PH_OTHER);
    }
  }
  clk.collect();
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(C, Cd, cb, hipMemcpyDeviceToHost));
  if (n > 0) RQ_HIP(hipMemcpy(codes, B, kb, hipMemcpyDeviceToHost));
  if (niter > 0) RQ_HIP(hipMemcpy(obj, objd, (size_t)niter * 8, hipMemcpyDeviceToHost));
  return RQ_OK;
}

// every check of the entries over int16 codes that needs no device: the shape, rho, the pointers and code_base (RQ_EINVAL), then
// -- with_A -- m * h within LSQ_MAX_MH (RQ_EUNSUPPORTED)
int lsq_wide_check(const void *out0, const void *out1, const void *X, const void *codes, int64_t n, int d, int m, int h, double rho,
                   int code_base, bool with_A, const char *who) {
  RQ_TRY(lsq_check(out0, out1, X, codes, n, d, m, h, rho, who, RQ_MAX_H16));
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  if (with_A && m * h > LSQ_MAX_MH)
    return fail(RQ_EUNSUPPORTED, "%s: m * h = %d * %d exceeds %d (A would take %zu bytes of f64)", who, m, h, LSQ_MAX_MH,
                (size_t)m * h * m * h * 8);
  return RQ_OK;
}

// uploads the caller's int16 codes and makes them zero-based
int upload_codes_h16(DevMem &dcodes, const int16_t *codes, int64_t n, int m, int code_base, hipStream_t s) {
  RQ_TRY(dcodes.alloc((size_t)n * m * 2));
  if (n > 0) {
    RQ_HIP(hipMemcpy(dcodes.p, codes, (size_t)n * m * 2, hipMemcpyHostToDevice));
    if (code_base) RQ_TRY(add_base_codes_launch(dcodes.as<int16_t>(), n * m, -code_base, s));
  }
  return RQ_OK;
}

}  // namespace

}  // namespace rq

using namespace rq;

extern "C" int rq_dev_lsq_normal_eq(double *A, double *b, const float *X, const uint8_t *codes, int64_t n, int d, int m,
                                    int h, double rho, void *stream) {
  RQ_TRY(lsq_check(A, b, X, codes, n, d, m, h, rho, "lsq_normal_eq"));
  hipStream_t s = (hipStream_t)stream;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  RQ_TRY(dev_code_range(codes, n, m, h, s, "lsq_normal_eq"));
  lsq_clock_reset();
  PhaseClock clk(s, g_lsq_ms, false);
  RQ_TRY(normal_eq_dev(A, b, X, codes, n, d, m, h, rho, s, clk));
  return RQ_OK;
}

extern "C" int rq_dev_update_codebooks_lsq(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m,
                                           int h, double rho, void *stream) {
  RQ_TRY(lsq_check(C, C, X, codes, n, d, m, h, rho, "update_codebooks_lsq"));
  hipStream_t s = (hipStream_t)stream;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  RQ_TRY(dev_code_range(codes, n, m, h, s, "update_codebooks_lsq"));
  lsq_clock_reset();
  PhaseClock clk(s, g_lsq_ms, false);
  RQ_TRY(update_dev(C, X, codes, n, d, m, h, rho, s, clk));
  return RQ_OK;
}

extern "C" int rq_update_codebooks_lsq(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h,
                                       double rho) {
  RQ_TRY(lsq_check(C, C, X, codes, n, d, m, h, rho, "update_codebooks_lsq"));
  RQ_TRY(host_code_range(codes, n, m, h, "update_codebooks_lsq"));
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  DevMem dX, dcodes, dC;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  RQ_TRY(dcodes.alloc((size_t)n * m));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  if (n > 0) {
    RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(dcodes.p, codes, (size_t)n * m, hipMemcpyHostToDevice));
  }
  lsq_clock_reset();
  PhaseClock clk(nullptr, g_lsq_ms);
  RQ_TRY(update_dev((float *)dC.p, (const float *)dX.p, (const uint8_t *)dcodes.p, n, d, m, h, rho, nullptr, clk));
  clk.collect();
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(C, dC.p, (size_t)m * h * d * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

extern "C" int rq_train_lsq(float *C, uint8_t *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m,
                            int h, int niter, int ilsiter, int icmiter, int npert, int randord, uint64_t seed,
                            int nsplits) {
  RQ_TRY(lsq_check(C, codes ? codes : (const void *)C, X, codes, n, d, m, h, 1e-4, "train_lsq"));
  if (!codes) return fail(RQ_EINVAL, "train_lsq: null codes");
  if (niter < 0) return fail(RQ_EINVAL, "train_lsq: niter=%d < 0", niter);
  if (niter > 0 && !obj) return fail(RQ_EINVAL, "train_lsq: null obj");
  if ((int64_t)ilsiter * ((int64_t)niter + 1) > INT32_MAX)
    return fail(RQ_EINVAL, "train_lsq: ilsiter * (niter + 1) overflows the ILS iteration counter");
  RQ_TRY(icm_check_args(codes, codes, X, C, n, d, m, h, ilsiter, icmiter, npert, 0, nsplits));
  RQ_TRY(host_code_range(codes, n, m, h, "train_lsq"));
  return train_lsq_host<uint8_t>(C, codes, obj, X, R, n, d, m, h, niter, ilsiter, icmiter, npert, randord, seed, nsplits, 0);
}

// ---- 2 <= h <= RQ_MAX_H16 over int16 codes: the int16 instantiations at EVERY h, host pointers --------
extern "C" int rq_lsq_wide_plan(int64_t n, int d, int m, int h, int64_t *out, int cap) {
  if (!out || cap < 0) return fail(RQ_EINVAL, "rq_lsq_wide_plan: null pointer or negative cap");
  RQ_TRY(lsq_wide_check(out, out, out, out, n, d, m, h, 1e-4, 0, true, "rq_lsq_wide_plan"));
  const LsqScratch L = lsq_scratch(n, m, h, true);
  const int64_t mh = (int64_t)m * h;
  int64_t none = 0;
  const int64_t train = rq_icm_wide_plan(n, d, m, h, 1, &none, 0) == RQ_OK ? 1 : 0;
  const int64_t v[7] = {mh, mh * mh * 8, (int64_t)L.pair_bytes, (int64_t)(L.total() - L.pair_bytes), L.ntiles, (mh + NB - 1) / NB,
                        train};
  for (int q = 0; q < cap && q < 7; ++q) out[q] = v[q];
  return RQ_OK;
}

extern "C" int rq_lsq_normal_eq_wide(double *A, double *b, uint32_t *counts, const float *X, const int16_t *codes, int64_t n,
                                     int d, int m, int h, double rho, int code_base) {
  const char *who = "lsq_normal_eq_wide";
  RQ_TRY(lsq_wide_check(b, b, X, codes, n, d, m, h, rho, code_base, A != nullptr, who));
  RQ_TRY(host_code_range(codes, n, m, h, code_base, who));
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  const size_t mh = (size_t)m * h;
  DevMem dX, dcodes, dA, db;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  if (A) RQ_TRY(dA.alloc(mh * mh * 8));
  RQ_TRY(db.alloc(mh * d * 8));
  if (n > 0) RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
  RQ_TRY(upload_codes_h16(dcodes, codes, n, m, code_base, nullptr));
  lsq_clock_reset();
  PhaseClock clk(nullptr, g_lsq_ms);
  const uint32_t *segs = nullptr;
  RQ_TRY(normal_eq_dev(A ? dA.as<double>() : nullptr, db.as<double>(), (const float *)dX.p, (const int16_t *)dcodes.p, n, d, m, h,
                       rho, nullptr, clk, &segs));
  clk.collect();
  RQ_HIP(hipDeviceSynchronize());
  if (A) RQ_HIP(hipMemcpy(A, dA.p, mh * mh * 8, hipMemcpyDeviceToHost));
  RQ_HIP(hipMemcpy(b, db.p, mh * d * 8, hipMemcpyDeviceToHost));
  if (counts) {   // the segment sizes
    std::vector<uint32_t> sg((size_t)m * (h + 1));
    RQ_HIP(hipMemcpy(sg.data(), segs, sg.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < m; ++i)
      for (int a = 0; a < h; ++a) counts[(size_t)i * h + a] = sg[(size_t)i * (h + 1) + a + 1] - sg[(size_t)i * (h + 1) + a];
  }
  return RQ_OK;
}

extern "C" int rq_update_codebooks_lsq_wide(float *C, const float *X, const int16_t *codes, int64_t n, int d, int m, int h,
                                            double rho, int code_base) {
  const char *who = "update_codebooks_lsq_wide";
  RQ_TRY(lsq_wide_check(C, C, X, codes, n, d, m, h, rho, code_base, true, who));
  RQ_TRY(host_code_range(codes, n, m, h, code_base, who));
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  DevMem dX, dcodes, dC;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  if (n > 0) RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
  RQ_TRY(upload_codes_h16(dcodes, codes, n, m, code_base, nullptr));
  lsq_clock_reset();
  PhaseClock clk(nullptr, g_lsq_ms);
  RQ_TRY(update_dev((float *)dC.p, (const float *)dX.p, (const int16_t *)dcodes.p, n, d, m, h, rho, nullptr, clk));
  clk.collect();
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(C, dC.p, (size_t)m * h * d * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

extern "C" int rq_train_lsq_wide(float *C, int16_t *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m,
                                 int h, int niter, int ilsiter, int icmiter, int npert, int randord, uint64_t seed, int nsplits,
                                 int code_base) {
  const char *who = "train_lsq_wide";
  RQ_TRY(lsq_check(C, codes ? codes : (const void *)C, X, codes, n, d, m, h, 1e-4, who, RQ_MAX_H16));
  if (!codes) return fail(RQ_EINVAL, "%s: null codes", who);
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  if (niter < 0) return fail(RQ_EINVAL, "%s: niter=%d < 0", who, niter);
  if (niter > 0 && !obj) return fail(RQ_EINVAL, "%s: null obj", who);
  if (ilsiter < 0 || icmiter < 0) return fail(RQ_EINVAL, "%s: negative count (ilsiter=%d icmiter=%d)", who, ilsiter, icmiter);
  if (npert < 0 || npert > m) return fail(RQ_EINVAL, "%s: npert=%d outside 0..m=%d", who, npert, m);
  if ((int64_t)ilsiter * ((int64_t)niter + 1) > INT32_MAX)
    return fail(RQ_EINVAL, "%s: ilsiter * (niter + 1) overflows the ILS iteration counter", who);
  RQ_TRY(lsq_train_wide_shape(who, n, d, m, h, nsplits));
  RQ_TRY(host_code_range(codes, n, m, h, code_base, who));
  return train_lsq_host<int16_t>(C, codes, obj, X, R, n, d, m, h, niter, ilsiter, icmiter, npert, randord, seed, nsplits,
                                 code_base);
}

extern "C" int rq_last_lsq_timing(double *ms, int cap) {
  if (!ms) return fail(RQ_EINVAL, "rq_last_lsq_timing: null pointer");
  for (int q = 0; q < cap && q < PH_N; ++q) ms[q] = g_lsq_ms[q];
  return RQ_OK;
}
