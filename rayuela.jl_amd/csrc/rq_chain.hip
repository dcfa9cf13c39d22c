// rq_chain.hip -- chain quantization (src/ChainQ.jl) on gfx950: the Viterbi encoder quantize_chainq (:305-348; CUDA path
// quantize_chainq_cuda! :204-285 with its viterbi_forward / vec_add kernels, C++ path deps/src/encode_icm.cpp:63-152
// viterbi_encoding), the chain-structured codebook update update_codebooks_chain_bin (src/codebook_update.jl:280-294,
// 367-412) and the training loop train_chainq (src/ChainQ.jl:373-431).  Contract in DESIGN.md section 2.
//
//   chain_pair_kernel       once per call: the m-1 adjacent-pair tables T_i[b][a] = 2 <c_ia, c_{i+1}b> in both orientations,
//                           Tab[i][a][256] (b contiguous: the forward pass stages slabs of it) and Tba[i][b][HS] (a contiguous:
//                           one row per back-trace step)
//   chain_range_kernel      once per call: per codebook the dimension range outside which it is zero, read from C itself
//   icm_unary_kernel        (rq_icm.hip) per chunk of rows: U[row][i][k] = fl(sa_i[k] - 2 <c_ik, x>), the chain over that
//                           range only (a skipped term is fma(+-0, x, acc) = acc for finite x: the same bits)
//   chain_forward_kernel    per chunk, ONE launch for all m-1 stages: a workgroup owns 32 rows; M_i (32 x h) and a 32-deep
//                           slab of T_i live in LDS, a thread keeps 4 rows x 8 b running minima in registers (add + min
//                           only, no index), M_{i+1} = fl(U_{i+1} + mincost_i) replaces U_{i+1} in place and in LDS
//   chain_backtrace_kernel  per chunk: one wavefront per row; code_{m-1} = first argmin of M_{m-1}, then for each stage the
//                           first a minimising fl(M_i[a] + T_i[code_{i+1}][a]) -- recomputed for the one b the trace needs
// Float min is order-free for finite values and every add is a single f32 add of the contract's two operands, so the
// codes equal the CPU restatement tests/chain_oracle.py (and the reference's strict-`<` scans) bit for bit.
//
// Past 256 codewords (int16 codes, 2 <= h <= RQ_MAX_H16) nothing may grow with h, so the rq_*_wide entries run
//   chain_wide_pair_kernel     64 x 64 tiles of T_i, both orientations with rows of HS = 64 ceil(h / 64) floats
//   chain_wide_forward_kernel  ONE launch per stage: a workgroup owns 32 rows and a 256-wide tile of b and streams a over all of
//                              h in slabs of 32, the slab of M_i (from U in global memory) and of T_i in LDS
//   chain_wide_trace_kernel    one wavefront per row, a running (minimum, first index) per lane over pieces of 256 floats
// and the chain update builds each 2h x 2h block from per-pair u32 counts (chain_wide_count_kernel, chain_wide_block_kernel)
// instead of cutting it from an mh x mh matrix.  The same operands and the same single adds: the same bits at h <= 256.
#include "rq_internal.h"

#include <math.h>

#include <vector>

namespace rq {

namespace {

constexpr int CH_MAX_M = 16;
constexpr size_t CH_SCRATCH_BYTES = (size_t)2 << 30;   // tables + unaries of one chunk, per device and stream
constexpr int VT_ROWS = 32;                            // rows of a forward workgroup
constexpr int VT_KA = 32;                              // depth (a) of the T slab in LDS
constexpr int VT_B = 256;                              // padded b extent of Tab rows

// ---- adjacent-pair tables ----------------------------------------------------------------------------------------------
// block = one (i, b), thread = a: the k-ordered fmaf chain of icm_pair_kernel for (j, k) = (i, i + 1)
__global__ __launch_bounds__(256) void chain_pair_kernel(float *Tab, float *Tba, const float *C, int m, int h, int d,
                                                         int HS) {
  const int b = blockIdx.x % h, i = blockIdx.x / h;
  const int a = threadIdx.x;
  if (a >= h) return;
  const float *ca = C + ((size_t)i * h + a) * d;
  const float *cb = C + ((size_t)(i + 1) * h + b) * d;
  float acc = 0.0f;
  for (int t = 0; t < d; ++t) acc = __builtin_fmaf(ca[t], cb[t], acc);
  const float v = 2.0f * acc;
  Tab[((size_t)i * h + a) * VT_B + b] = v;
  Tba[((size_t)i * h + b) * HS + a] = v;
}

// rng[2i], rng[2i+1] = [lo, hi): codebook i is zero (+-0) outside these dimensions, found from C itself; (d, 0) when it is
// zero everywhere.  block = codebook, thread t scans dimensions t, t + 256, ...
__global__ __launch_bounds__(256) void chain_range_kernel(int *rng, const float *C, int h, int d) {
  __shared__ int slo[256], shi[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float *Ci = C + (size_t)i * h * d;
  int lo = d, hi = 0;
  for (int t = tid; t < d; t += 256) {
    bool nz = false;
    for (int a = 0; a < h && !nz; ++a) nz = Ci[(size_t)a * d + t] != 0.0f;
    if (nz) { lo = min(lo, t); hi = max(hi, t + 1); }
  }
  slo[tid] = lo; shi[tid] = hi;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) { slo[tid] = min(slo[tid], slo[tid + off]); shi[tid] = max(shi[tid], shi[tid + off]); }
    __syncthreads();
  }
  if (tid == 0) { rng[2 * i] = slo[0]; rng[2 * i + 1] = shi[0]; }
}

// ---- forward pass ------------------------------------------------------------------------------------------------------
// thread (tb, tr): rows tr*4 .. tr*4+3 and b in {tb*4 .. tb*4+3} U {128 + tb*4 .. 128 + tb*4+3}.  Per a it reads one float4
// of M (two addresses per wavefront: broadcast) and two float4 of T (32 lanes x 16 B contiguous: conflict-free) for 32 adds and
// 32 mins.  Rows past nrows compute on zeros and store nothing.
__global__ __launch_bounds__(256) void chain_forward_kernel(float *U, const float *Tab, int64_t nrows, int m, int h,
                                                            int HS) {
  __shared__ __attribute__((aligned(16))) float Ms[256][VT_ROWS];   // [a][row]
  __shared__ __attribute__((aligned(16))) float Ts[VT_KA][VT_B];    // [a - a0][b]
  const int tid = threadIdx.x, tb = tid & 31, tr = tid >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * VT_ROWS;
  const size_t rs = (size_t)m * HS;   // floats per row of U
  for (int e = tid; e < VT_ROWS * 256; e += 256) {
    const int r = e >> 8, a = e & 255;
    const int64_t row = row0 + r;
    Ms[a][r] = (a < h && row < nrows) ? U[(size_t)row * rs + a] : 0.0f;
  }
#pragma unroll 1
  for (int i = 0; i + 1 < m; ++i) {
    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_inff();
    const float *Ti = Tab + (size_t)i * h * VT_B;
#pragma unroll 1
    for (int a0 = 0; a0 < h; a0 += VT_KA) {
      const int na = min(VT_KA, h - a0);
      __syncthreads();   // the previous slab's readers are done; Ms of this stage is complete
      const float4 *src = reinterpret_cast<const float4 *>(Ti + (size_t)a0 * VT_B);
      float4 *dst = reinterpret_cast<float4 *>(&Ts[0][0]);
      for (int e = tid; e < na * (VT_B / 4); e += 256) dst[e] = src[e];
      __syncthreads();
#pragma unroll 2
      for (int a = 0; a < na; ++a) {
        const float4 mv = *reinterpret_cast<const float4 *>(&Ms[a0 + a][tr * 4]);
        const float4 t0 = *reinterpret_cast<const float4 *>(&Ts[a][tb * 4]);
        const float4 t1 = *reinterpret_cast<const float4 *>(&Ts[a][128 + tb * 4]);
        const float mr[4] = {mv.x, mv.y, mv.z, mv.w};
        const float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_fminf(acc[r][j], mr[r] + tv[j]);
      }
    }
    __syncthreads();   // every read of M_i is done: M_{i+1} may replace it
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int b0 = g * 128 + tb * 4;
      if (b0 < h) {   // b0 + 3 < HS: HS is a multiple of 64 and >= h
        float o[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = row0 + tr * 4 + r;
          if (row < nrows) {
            float4 *up = reinterpret_cast<float4 *>(U + (size_t)row * rs + (size_t)(i + 1) * HS + b0);
            const float4 u = *up;
            float4 v;
            v.x = u.x + acc[r][g * 4 + 0]; v.y = u.y + acc[r][g * 4 + 1];
            v.z = u.z + acc[r][g * 4 + 2]; v.w = u.w + acc[r][g * 4 + 3];
            *up = v;
            o[r][0] = v.x; o[r][1] = v.y; o[r][2] = v.z; o[r][3] = v.w;
          } else {
            o[r][0] = o[r][1] = o[r][2] = o[r][3] = 0.0f;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float4 w;
          w.x = o[0][j]; w.y = o[1][j]; w.z = o[2][j]; w.w = o[3][j];
          *reinterpret_cast<float4 *>(&Ms[b0 + j][tr * 4]) = w;
        }
      }
    }
  }
}

// ---- back trace --------------------------------------------------------------------------------------------------------
// first index of the minimum over the wavefront: in-lane scan (ascending index), then a (value, index) butterfly
template <int E>
__device__ __forceinline__ int chain_argmin(const float (&v)[E], int lane, int h) {
  float bv = v[0];
  int bi = lane * E;
#pragma unroll
  for (int e = 1; e < E; ++e)
    if (v[e] < bv) { bv = v[e]; bi = lane * E + e; }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  int res = __shfl(bi, 0, 64);
  if (res < 0 || res >= h) res = 0;   // only reachable with NaN costs: keep the code in range
  return res;
}

template <int E>
__global__ __launch_bounds__(256) void chain_backtrace_kernel(uint8_t *codes, const float *M, const float *Tba,
                                                              int64_t nrows, int m, int h, int HS) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const float *Mr = M + (size_t)row * m * HS;
  float v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int a = lane * E + e;
    v[e] = a < h ? Mr[(size_t)(m - 1) * HS + a] : __builtin_inff();
  }
  int b = chain_argmin<E>(v, lane, h);
  if (lane == 0) codes[row * m + (m - 1)] = (uint8_t)b;
#pragma unroll 1
  for (int i = m - 2; i >= 0; --i) {
    const float *Tr = Tba + ((size_t)i * h + b) * HS;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int a = lane * E + e;
      v[e] = a < h ? Mr[(size_t)i * HS + a] + Tr[a] : __builtin_inff();
    }
    b = chain_argmin<E>(v, lane, h);
    if (lane == 0) codes[row * m + i] = (uint8_t)b;
  }
}

// ---- 2 <= h <= RQ_MAX_H16 over int16 codes: LDS and registers do not grow with h -----------------------
// Pair tables: block = the 64 x 64 tile (a0.., b0..) of stage i, thread = 4 a x 4 b, PK dimensions at a time through LDS.  Every
// output is its own fmaf chain over t = 0 .. d-1 in order from +0 (a pad term, t >= d, is fma(0, 0, acc) = acc): the chain of
// chain_pair_kernel.  Both orientations have rows of HS floats, Tab[i][a][b] and Tba[i][b][a]; the tiles cover HS exactly, so
// the pad of every row (index >= h) is written too, as +0.
constexpr int CW_PT = 64, CW_PK = 16;
__global__ __launch_bounds__(256) void chain_wide_pair_kernel(float *Tab, float *Tba, const float *C, int h, int d, int HS) {
  __shared__ __attribute__((aligned(16))) float As[CW_PK][CW_PT + 4], Bs[CW_PK][CW_PT + 4];   // [t][a], [t][b]
  const int i = blockIdx.z, a0 = blockIdx.x * CW_PT, b0 = blockIdx.y * CW_PT;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const float *Ca = C + (size_t)i * h * d, *Cb = C + (size_t)(i + 1) * h * d;
  float acc[4][4];   // [b][a]
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[q][p] = 0.0f;
  for (int t0 = 0; t0 < d; t0 += CW_PK) {
    for (int e = threadIdx.x; e < CW_PT * CW_PK; e += 256) {
      const int r = e / CW_PK, t = e % CW_PK;
      const bool tv = t0 + t < d;
      As[t][r] = (tv && a0 + r < h) ? Ca[(size_t)(a0 + r) * d + t0 + t] : 0.0f;
      Bs[t][r] = (tv && b0 + r < h) ? Cb[(size_t)(b0 + r) * d + t0 + t] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < CW_PK; ++t) {
      const float4 a = *reinterpret_cast<const float4 *>(&As[t][4 * tx]);
      const float4 b = *reinterpret_cast<const float4 *>(&Bs[t][4 * ty]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[q][p] = __builtin_fmaf(av[p], bv[q], acc[q][p]);
    }
    __syncthreads();
  }
  float v[4][4];   // [b][a]
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int p = 0; p < 4; ++p) v[q][p] = (a0 + 4 * tx + p < h && b0 + 4 * ty + q < h) ? 2.0f * acc[q][p] : 0.0f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int b = b0 + 4 * ty + q;
    if (b < h) *reinterpret_cast<float4 *>(Tba + ((size_t)i * h + b) * HS + a0 + 4 * tx) = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int a = a0 + 4 * tx + p;
    if (a < h) *reinterpret_cast<float4 *>(Tab + ((size_t)i * h + a) * HS + b0 + 4 * ty) = make_float4(v[0][p], v[1][p], v[2][p], v[3][p]);
  }
}

// Forward pass, ONE launch per stage i: block (x, y) owns rows 32x .. 32x+31 and the b tile 256y .. 256y+255 and walks a over all
// of h in slabs of VW_KA.  Per slab it stages the slab of M_i for its rows (slot i of U, global memory: a stage reads slot i and
// writes slot i + 1, never what it reads) and the slab of T_i for its tile; the thread layout, the LDS reads and the add + min of
// chain_forward_kernel.  LDS: 36.5 KiB at every h.
constexpr int VW_KA = 32;                  // depth (a) of a slab
constexpr int VW_MP = VT_ROWS + 4;         // padded row extent of the M slab (keeps float4 alignment, spreads the transposing store)
__global__ __launch_bounds__(256) void chain_wide_forward_kernel(float *U, const float *Tab, int64_t nrows, int m, int h, int HS,
                                                                 int i) {
  __shared__ __attribute__((aligned(16))) float Ms[VW_KA][VW_MP];   // [a - a0][row]
  __shared__ __attribute__((aligned(16))) float Ts[VW_KA][VT_B];    // [a - a0][b - b0]
  const int tid = threadIdx.x, tb = tid & 31, tr = tid >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * VT_ROWS;
  const int b0 = blockIdx.y * VT_B;
  const size_t rs = (size_t)m * HS;   // floats per row of U
  const float *Mi = U + (size_t)i * HS;
  const float *Ti = Tab + (size_t)i * h * HS;
  float acc[4][8];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_inff();
#pragma unroll 1
  for (int a0 = 0; a0 < h; a0 += VW_KA) {
    const int na = min(VW_KA, h - a0);
    __syncthreads();   // the previous slab's readers are done
    for (int e = tid; e < VT_ROWS * VW_KA; e += 256) {
      const int r = e >> 5, a = e & 31;
      const int64_t row = row0 + r;
      Ms[a][r] = (a < na && row < nrows) ? Mi[(size_t)row * rs + a0 + a] : 0.0f;
    }
    for (int e = tid; e < na * (VT_B / 4); e += 256) {
      const int a = e >> 6, q = e & 63;
      const int b = b0 + 4 * q;   // b + 3 < HS whenever b < HS: HS is a multiple of 64
      float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (b < HS) t = *reinterpret_cast<const float4 *>(Ti + (size_t)(a0 + a) * HS + b);
      *reinterpret_cast<float4 *>(&Ts[a][4 * q]) = t;
    }
    __syncthreads();
#pragma unroll 2
    for (int a = 0; a < na; ++a) {
      const float4 mv = *reinterpret_cast<const float4 *>(&Ms[a][tr * 4]);
      const float4 t0 = *reinterpret_cast<const float4 *>(&Ts[a][tb * 4]);
      const float4 t1 = *reinterpret_cast<const float4 *>(&Ts[a][128 + tb * 4]);
      const float mr[4] = {mv.x, mv.y, mv.z, mv.w};
      const float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] = __builtin_fminf(acc[r][j], mr[r] + tv[j]);
    }
  }
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int b = b0 + g * 128 + tb * 4;
    if (b >= h) continue;   // b + 3 < HS
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = row0 + tr * 4 + r;
      if (row >= nrows) continue;
      float4 *up = reinterpret_cast<float4 *>(U + (size_t)row * rs + (size_t)(i + 1) * HS + b);
      const float4 u = *up;
      float4 v;
      v.x = u.x + acc[r][g * 4 + 0]; v.y = u.y + acc[r][g * 4 + 1];
      v.z = u.z + acc[r][g * 4 + 2]; v.w = u.w + acc[r][g * 4 + 3];
      *up = v;
    }
  }
}

// Back trace: one wavefront per row.  A lane walks the row in pieces of 64 lanes x 4 floats (ascending index) with a running
// (minimum, first index) under a strict <, then the (value, index) butterfly of chain_argmin.  Entries past h compare as +inf.
// trow: the row T_i[code_{i+1}][.] of Tba, or null for the last codebook (the costs are M_{m-1} themselves).
__device__ __forceinline__ int chain_wide_argmin(const float *mrow, const float *trow, int lane, int h, int HS) {
  float bv = __builtin_inff();
  int bi = 0x7fffffff;
#pragma unroll 1
  for (int i0 = 0; i0 < HS; i0 += 256) {
    const int idx = i0 + lane * 4;
    // a lane past the row's end reads the row's last four floats again: in bounds, and masked below (idx >= HS >= h)
    const int at = idx < HS ? idx : HS - 4;
    const float4 mv = *reinterpret_cast<const float4 *>(mrow + at);
    float v[4] = {mv.x, mv.y, mv.z, mv.w};
    if (trow) {
      const float4 tv = *reinterpret_cast<const float4 *>(trow + at);
      v[0] = v[0] + tv.x; v[1] = v[1] + tv.y; v[2] = v[2] + tv.z; v[3] = v[3] + tv.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float c = idx + e < h ? v[e] : __builtin_inff();
      if (c < bv) { bv = c; bi = idx + e; }
    }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  int res = __shfl(bi, 0, 64);
  if (res < 0 || res >= h) res = 0;   // only reachable with non-finite costs: keep the code in range
  return res;
}

__global__ __launch_bounds__(256) void chain_wide_trace_kernel(int16_t *codes, const float *M, const float *Tba, int64_t nrows,
                                                               int m, int h, int HS) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const float *Mr = M + (size_t)row * m * HS;
  int b = chain_wide_argmin(Mr + (size_t)(m - 1) * HS, nullptr, lane, h, HS);
  if (lane == 0) codes[row * m + (m - 1)] = (int16_t)b;
#pragma unroll 1
  for (int i = m - 2; i >= 0; --i) {
    b = chain_wide_argmin(Mr + (size_t)i * HS, Tba + ((size_t)i * h + b) * HS, lane, h, HS);
    if (lane == 0) codes[row * m + i] = (int16_t)b;
  }
}

// ---- CB = sum_i C_i[b_i]: f32 adds from +0 in codebook order (the CB of src/ChainQ.jl:411-412) ---------------------------------
template <class Code>
__global__ __launch_bounds__(256) void chain_reconstruct_kernel(float *CB, const Code *codes, const float *C, int64_t n,
                                                                int d, int m, int h) {
  const int64_t total = n * d;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / d;
    const int t = (int)(e - r * d);
    float cb = 0.0f;
    for (int i = 0; i < m; ++i) cb = cb + C[((size_t)i * h + codes[r * m + i]) * d + t];
    CB[e] = cb;
  }
}

// ---- chain codebook update: block i of the normal equations ----------------------------------------------------------------
// Ab [2h][2h] <- A[ih .. (i+2)h)^2, Yb [2h][len] <- b[ih .. (i+2)h)[off .. off+len)
__global__ __launch_bounds__(256) void chain_block_gather_kernel(double *Ab, double *Yb, const double *A, const double *b,
                                                                 int mh, int d, int h, int i, int off, int len) {
  const int h2 = 2 * h;
  const int64_t na = (int64_t)h2 * h2, ny = (int64_t)h2 * len;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < na + ny; e += (int64_t)gridDim.x * 256) {
    if (e < na) {
      const int r = (int)(e / h2), c = (int)(e - (int64_t)r * h2);
      Ab[e] = A[(size_t)(i * h + r) * mh + i * h + c];
    } else {
      const int64_t q = e - na;
      const int r = (int)(q / len), c = (int)(q - (int64_t)r * len);
      Yb[q] = b[(size_t)(i * h + r) * d + off + c];
    }
  }
}

// C_i[:, off .. off+len) <- rows 0 .. h-1 of Yb, C_{i+1}[:, off .. off+len) <- rows h .. 2h-1
__global__ __launch_bounds__(256) void chain_block_scatter_kernel(float *C, const double *Yb, int d, int h, int i, int off,
                                                                  int len) {
  const int64_t ny = (int64_t)2 * h * len;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ny; q += (int64_t)gridDim.x * 256) {
    const int r = (int)(q / len), c = (int)(q - (int64_t)r * len);
    C[((size_t)i * h + r) * d + off + c] = (float)Yb[q];   // row r of the block is codeword r of the stacked (C_i, C_{i+1})
  }
}

// ---- the same block past 256 codewords, without the mh x mh matrix -----------------------------------------------------------------
// P [h][h] u32 (zeroed by the caller) += the rows with (codes[.][i], codes[.][i+1]) = (a, b); integer atomics: exact, order-free.
// Codes in range (checked before any work), so every index is inside P.
__global__ __launch_bounds__(256) void chain_wide_count_kernel(uint32_t *P, const int16_t *codes, int64_t n, int m, int h, int i) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256)
    atomicAdd(&P[(size_t)codes[r * m + i] * h + codes[r * m + i + 1]], 1u);
}

// Ab [2h][2h] <- [[diag(cnt_i + rho), P], [P', diag(cnt_{i+1} + rho)]], what chain_block_gather_kernel cuts from lsq_assemble_kernel's
// A bit for bit (fl64(count + rho) on the diagonal, exact integers elsewhere); Yb [2h][len] <- b[ih .. (i+2)h)[off .. off+len)
__global__ __launch_bounds__(256) void chain_wide_block_kernel(double *Ab, double *Yb, const uint32_t *P, const uint32_t *segs,
                                                               const double *b, int d, int h, int i, int off, int len, double rho) {
  const int h2 = 2 * h;
  const int64_t na = (int64_t)h2 * h2, ny = (int64_t)h2 * len;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < na + ny; e += (int64_t)gridDim.x * 256) {
    if (e < na) {
      const int r = (int)(e / h2), c = (int)(e - (int64_t)r * h2);
      const int rj = r >= h, cj = c >= h, ra = r - rj * h, ca = c - cj * h;
      double v;
      if (rj == cj) {
        const uint32_t *s = segs + (size_t)(i + rj) * (h + 1);
        v = (r == c) ? (double)(s[ra + 1] - s[ra]) + rho : 0.0;
      } else {
        v = (double)(rj == 0 ? P[(size_t)ra * h + ca] : P[(size_t)ca * h + ra]);
      }
      Ab[e] = v;
    } else {
      const int64_t q = e - na;
      const int r = (int)(q / len), c = (int)(q - (int64_t)r * len);
      Yb[q] = b[(size_t)(i * h + r) * d + off + c];
    }
  }
}

// part i of splitarray(1:d, parts) (src/utils.jl:179-203), zero-based [lo, hi)
void chain_split(int d, int parts, int i, int *lo, int *hi) {
  const int per = d / parts, xtra = d % parts;
  *lo = i * per + std::min(i, xtra);
  *hi = *lo + per + (i < xtra ? 1 : 0);
}

// phase clock of the host-pointer entries: milliseconds of the calling thread's last call
enum { CP_UNARY, CP_TABLES, CP_VITERBI, CP_UPDATE, CP_ROTATION, CP_N };
thread_local double g_chain_ms[CP_N] = {0};

void chain_clock_reset() {
  for (int q = 0; q < CP_N; ++q) g_chain_ms[q] = 0;
}

// hmax: 256 for the byte entries, RQ_MAX_H16 for the entries over int16 codes
int chain_check_encode(const void *codes, const void *X, const void *C, int64_t n, int d, int m, int h, int nsplits,
                       const char *who, int hmax = 256) {
  if (m < 1 || m > CH_MAX_M) return fail(RQ_EINVAL, "%s: m=%d outside 1..%d", who, m, CH_MAX_M);
  if (h < 2 || h > hmax) return fail(RQ_EINVAL, "%s: h=%d outside 2..%d", who, h, hmax);
  if (d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);
  if (n < 0) return fail(RQ_EINVAL, "%s: negative count n=%lld", who, (long long)n);
  if (nsplits < 1) return fail(RQ_EINVAL, "%s: nsplits=%d < 1", who, nsplits);
  if (!C || (n > 0 && (!codes || !X))) return fail(RQ_EINVAL, "%s: null pointer", who);
  return RQ_OK;
}

int chain_check_update(const void *C, const void *X, const void *codes, int64_t n, int d, int m, int h, double rho,
                       const char *who, int hmax = 256) {
  if (m < 2 || m > CH_MAX_M) return fail(RQ_EINVAL, "%s: m=%d outside 2..%d", who, m, CH_MAX_M);
  if (h < 2 || h > hmax) return fail(RQ_EINVAL, "%s: h=%d outside 2..%d", who, h, hmax);
  if (d < m - 1) return fail(RQ_EINVAL, "%s: d=%d < m - 1 = %d (an empty chain part)", who, d, m - 1);
  if (n < 0 || n > (int64_t)UINT32_MAX)
    return fail(RQ_EINVAL, "%s: n=%lld outside 0..%u (the u32 counters)", who, (long long)n, UINT32_MAX);
  if (!(rho > 0.0) || !isfinite(rho)) return fail(RQ_EINVAL, "%s: rho=%g must be finite and > 0", who, rho);
  if (!C) return fail(RQ_EINVAL, "%s: null output pointer", who);
  if (n > 0 && (!X || !codes)) return fail(RQ_EINVAL, "%s: null pointer", who);
  return RQ_OK;
}

// The device body of the encoder: arguments already checked.
int chain_encode_dev(uint8_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int nsplits,
                     hipStream_t s, PhaseClock &clk) {
  if (n <= 0) return RQ_OK;
  const int E = (h + 63) / 64, HS = 64 * E;
  const size_t tab_bytes = (size_t)(m - 1) * h * VT_B * 4, tba_bytes = (size_t)(m - 1) * h * HS * 4;
  const size_t sa_bytes = (size_t)m * h * 4, row_bytes = (size_t)m * HS * 4;
  const size_t u_budget = CH_SCRATCH_BYTES - tab_bytes - tba_bytes - sa_bytes;   // tables <= 8 MiB of the 2 GiB
  int64_t chunk = (n + nsplits - 1) / nsplits;
  chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(u_budget / row_bytes)));
  void *wt = nullptr, *wu = nullptr;
  RQ_TRY(workspace(WS_ICM_BIN, tab_bytes + tba_bytes + sa_bytes + 256, &wt, s));   // + rng [m][2]
  RQ_TRY(workspace(WS_ICM_U, (size_t)chunk * row_bytes, &wu, s));
  float *Tab = (float *)wt, *Tba = Tab + tab_bytes / 4, *sa = Tba + tba_bytes / 4, *U = (float *)wu;
  int *rng = (int *)(sa + sa_bytes / 4);
  if (m > 1) {
    RQ_HIP(hipMemsetAsync(Tab, 0, tab_bytes + tba_bytes, s));
    RQ_LAUNCH(chain_pair_kernel, dim3((m - 1) * h), dim3(256), 0, s, Tab, Tba, C, m, h, d, HS);
  }
  RQ_TRY(icm_sqnorm_launch(sa, C, m, h, d, s));
  RQ_LAUNCH(chain_range_kernel, dim3(m), dim3(256), 0, s, rng, C, h, d);
  clk.mark(CP_TABLES);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nr = std::min(chunk, n - r0);
    RQ_TRY(icm_unary_launch(U, X + (size_t)r0 * d, C, sa, nr, d, m, h, HS, rng, s));
    clk.mark(CP_UNARY);
    if (m > 1)
      RQ_LAUNCH(chain_forward_kernel, dim3((unsigned)((nr + VT_ROWS - 1) / VT_ROWS)), dim3(256), 0, s, U,
                (const float *)Tab, nr, m, h, HS);
    const dim3 grid((unsigned)((nr + 3) / 4));
    uint8_t *out = codes + (size_t)r0 * m;
    if (E == 1) RQ_LAUNCH((chain_backtrace_kernel<1>), grid, dim3(256), 0, s, out, (const float *)U, (const float *)Tba, nr, m, h, HS);
    else if (E == 2) RQ_LAUNCH((chain_backtrace_kernel<2>), grid, dim3(256), 0, s, out, (const float *)U, (const float *)Tba, nr, m, h, HS);
    else if (E == 3) RQ_LAUNCH((chain_backtrace_kernel<3>), grid, dim3(256), 0, s, out, (const float *)U, (const float *)Tba, nr, m, h, HS);
    else RQ_LAUNCH((chain_backtrace_kernel<4>), grid, dim3(256), 0, s, out, (const float *)U, (const float *)Tba, nr, m, h, HS);
    clk.mark(CP_VITERBI);
  }
  return RQ_OK;
}

// C [m][h][d] f32 <- the chain update of (X, codes): arguments checked, codes in range.  The m-1 blocks are solved one
// after the other (each through the blocked Cholesky of rq_lsq.hip on its own copy: adjacent blocks share a diagonal part).
int chain_update_dev(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h, double rho,
                     hipStream_t s, PhaseClock &clk) {
  const int mh = m * h, h2 = 2 * h;
  void *wa = nullptr, *wb = nullptr, *wc = nullptr;
  RQ_TRY(workspace(WS_LSQ_A, (size_t)mh * mh * 8, &wa, s));
  RQ_TRY(workspace(WS_LSQ_B, (size_t)mh * d * 8, &wb, s));
  int maxlen = 0;
  for (int i = 0; i + 1 < m; ++i) {
    int lo, hi;
    chain_split(d, m - 1, i, &lo, &hi);
    maxlen = std::max(maxlen, hi - lo);
  }
  RQ_TRY(workspace(WS_CHAIN, ((size_t)h2 * h2 + (size_t)h2 * maxlen) * 8, &wc, s));
  double *A = (double *)wa, *b = (double *)wb, *Ab = (double *)wc, *Yb = Ab + (size_t)h2 * h2;
  RQ_TRY(lsq_normal_eq_launch(A, b, X, codes, n, d, m, h, rho, s));
  RQ_HIP(hipMemsetAsync(C, 0, (size_t)mh * d * 4, s));
  for (int i = 0; i + 1 < m; ++i) {
    int lo, hi;
    chain_split(d, m - 1, i, &lo, &hi);
    const int len = hi - lo;
    if (len <= 0) continue;
    const int64_t cnt = (int64_t)h2 * h2 + (int64_t)h2 * len;
    RQ_LAUNCH(chain_block_gather_kernel, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 4096)), dim3(256), 0, s, Ab, Yb,
              (const double *)A, (const double *)b, mh, d, h, i, lo, len);
    RQ_TRY(lsq_spd_solve_launch(Ab, Yb, h2, len, s));
    RQ_LAUNCH(chain_block_scatter_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)h2 * len + 255) / 256, 4096)), dim3(256),
              0, s, C, (const double *)Yb, d, h, i, lo, len);
  }
  clk.mark(CP_UPDATE);
  return RQ_OK;
}

// ---- 2 <= h <= RQ_MAX_H16 over int16 codes: the plan, the encoder and the update ------------------------------------------------
constexpr int CHW_MAX_H2 = 16384;   // 2h of the update: the 2h x 2h f64 block is then at most 2 GiB (LSQ_MAX_MH's figure)

// what rq_chain_wide_plan reports and the wide encoder runs
struct ChainWidePlan {
  int HS;
  size_t table_bytes;   // both orientations of the pair tables + the self-products
  size_t row_bytes;     // unaries of one row
  int64_t chunk, chunks;
};

// shape already checked (chain_check_encode): the tables and 32 rows of unaries within CH_SCRATCH_BYTES, else RQ_EUNSUPPORTED
int chain_wide_plan(ChainWidePlan *pl, int64_t n, int m, int h, int nsplits, const char *who) {
  pl->HS = 64 * ((h + 63) / 64);
  pl->table_bytes = (size_t)2 * (m - 1) * h * pl->HS * 4 + (size_t)m * h * 4;
  pl->row_bytes = (size_t)m * pl->HS * 4;
  if (pl->table_bytes + VT_ROWS * pl->row_bytes > CH_SCRATCH_BYTES)
    return fail(RQ_EUNSUPPORTED, "%s: the tables of m=%d, h=%d take %zu bytes; with %d rows of unaries they must fit %zu", who, m, h,
                pl->table_bytes, VT_ROWS, CH_SCRATCH_BYTES);
  const int64_t fit = (int64_t)((CH_SCRATCH_BYTES - pl->table_bytes) / pl->row_bytes);
  pl->chunk = n == 0 ? 0 : std::max<int64_t>(1, std::min<int64_t>((n + nsplits - 1) / nsplits, fit));
  pl->chunks = n == 0 ? 0 : (n + pl->chunk - 1) / pl->chunk;
  return RQ_OK;
}

// whether the update (and with it training) takes the shape: RQ_EUNSUPPORTED past 2h = CHW_MAX_H2
int chain_wide_update_rule(int h, const char *who) {
  if (2 * h > CHW_MAX_H2)
    return fail(RQ_EUNSUPPORTED, "%s: 2 h = %d exceeds %d (a block would take %zu bytes of f64)", who, 2 * h, CHW_MAX_H2,
                (size_t)4 * h * h * 8);
  return RQ_OK;
}

// The device body of the encoder over zero-based int16 codes: arguments checked, chain_wide_plan passes.
int chain_encode_dev(int16_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int nsplits, hipStream_t s,
                     PhaseClock &clk) {
  if (n <= 0) return RQ_OK;
  ChainWidePlan pl;
  RQ_TRY(chain_wide_plan(&pl, n, m, h, nsplits, "quantize_chainq_wide"));
  const int HS = pl.HS;
  const size_t tab_bytes = (size_t)(m - 1) * h * HS * 4, sa_bytes = (size_t)m * h * 4;
  void *wt = nullptr, *wu = nullptr;
  RQ_TRY(workspace(WS_ICM_BIN, pl.table_bytes + 256, &wt, s));   // + rng [m][2]
  RQ_TRY(workspace(WS_ICM_U, (size_t)pl.chunk * pl.row_bytes, &wu, s));
  float *Tab = (float *)wt, *Tba = Tab + tab_bytes / 4, *sa = Tba + tab_bytes / 4, *U = (float *)wu;
  int *rng = (int *)(sa + sa_bytes / 4);
  if (m > 1)
    RQ_LAUNCH(chain_wide_pair_kernel, dim3((unsigned)(HS / CW_PT), (unsigned)(HS / CW_PT), (unsigned)(m - 1)), dim3(256), 0, s, Tab,
              Tba, C, h, d, HS);
  RQ_TRY(icm_sqnorm_launch(sa, C, m, h, d, s));
  RQ_LAUNCH(chain_range_kernel, dim3(m), dim3(256), 0, s, rng, C, h, d);
  clk.mark(CP_TABLES);
  for (int64_t r0 = 0; r0 < n; r0 += pl.chunk) {
    const int64_t nr = std::min(pl.chunk, n - r0);
    RQ_TRY(icm_unary_launch(U, X + (size_t)r0 * d, C, sa, nr, d, m, h, HS, rng, s));
    clk.mark(CP_UNARY);
    const dim3 fgrid((unsigned)((nr + VT_ROWS - 1) / VT_ROWS), (unsigned)((h + VT_B - 1) / VT_B));
    for (int i = 0; i + 1 < m; ++i)   // stage i reads slot i of U and writes slot i + 1: the launch boundary orders the stages
      RQ_LAUNCH(chain_wide_forward_kernel, fgrid, dim3(256), 0, s, U, (const float *)Tab, nr, m, h, HS, i);
    RQ_LAUNCH(chain_wide_trace_kernel, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, s, codes + (size_t)r0 * m, (const float *)U,
              (const float *)Tba, nr, m, h, HS);
    clk.mark(CP_VITERBI);
  }
  return RQ_OK;
}

// chain_update_dev over zero-based int16 codes (2h <= CHW_MAX_H2): b and the per-code counts from the normal equations without
// their matrix, then per adjacent pair the u32 pair counts, the 2h x 2h block, the solve and the scatter.
// Scratch: WS_LSQ_A the block, WS_LSQ_B b, WS_LSQ_S the sort (lsq_b_segs_wide_launch), WS_CHAIN the pair counts and the right-hand side.
int chain_update_dev(float *C, const float *X, const int16_t *codes, int64_t n, int d, int m, int h, double rho, hipStream_t s,
                     PhaseClock &clk) {
  const int mh = m * h, h2 = 2 * h;
  void *wa = nullptr, *wb = nullptr, *wc = nullptr;
  RQ_TRY(workspace(WS_LSQ_A, (size_t)h2 * h2 * 8, &wa, s));
  RQ_TRY(workspace(WS_LSQ_B, (size_t)mh * d * 8, &wb, s));
  int maxlen = 0;
  for (int i = 0; i + 1 < m; ++i) {
    int lo, hi;
    chain_split(d, m - 1, i, &lo, &hi);
    maxlen = std::max(maxlen, hi - lo);
  }
  const size_t p_bytes = (size_t)h * h * 4;   // a multiple of 8: Yb stays aligned
  RQ_TRY(workspace(WS_CHAIN, p_bytes + (size_t)h2 * maxlen * 8 + 8, &wc, s));
  double *Ab = (double *)wa, *b = (double *)wb;
  uint32_t *P = (uint32_t *)wc;
  double *Yb = (double *)((char *)wc + ((p_bytes + 7) & ~(size_t)7));
  const uint32_t *segs = nullptr;
  RQ_TRY(lsq_b_segs_wide_launch(b, &segs, X, codes, n, d, m, h, rho, s));
  RQ_HIP(hipMemsetAsync(C, 0, (size_t)mh * d * 4, s));
  for (int i = 0; i + 1 < m; ++i) {
    int lo, hi;
    chain_split(d, m - 1, i, &lo, &hi);
    const int len = hi - lo;
    if (len <= 0) continue;
    RQ_HIP(hipMemsetAsync(P, 0, p_bytes, s));
    if (n > 0)
      RQ_LAUNCH(chain_wide_count_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, s, P, codes, n, m, h,
                i);
    const int64_t cnt = (int64_t)h2 * h2 + (int64_t)h2 * len;
    RQ_LAUNCH(chain_wide_block_kernel, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 4096)), dim3(256), 0, s, Ab, Yb,
              (const uint32_t *)P, segs, (const double *)b, d, h, i, lo, len, rho);
    RQ_TRY(lsq_spd_solve_launch(Ab, Yb, h2, len, s));
    RQ_LAUNCH(chain_block_scatter_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)h2 * len + 255) / 256, 4096)), dim3(256),
              0, s, C, (const double *)Yb, d, h, i, lo, len);
  }
  clk.mark(CP_UPDATE);
  return RQ_OK;
}

template <class Code>
int chain_reconstruct_dev(float *CB, const Code *codes, const float *C, int64_t n, int d, int m, int h, hipStream_t s) {
  if (n <= 0) return RQ_OK;
  RQ_LAUNCH(chain_reconstruct_kernel<Code>, dim3((unsigned)std::min<int64_t>((n * d + 255) / 256, 8192)), dim3(256), 0, s, CB,
            codes, C, n, d, m, h);
  return RQ_OK;
}

}  // namespace

}  // namespace rq

using namespace rq;

extern "C" int rq_chain_dims(int d, int m, int *lo, int *hi) {
  if (m < 2 || m > CH_MAX_M) return fail(RQ_EINVAL, "chain_dims: m=%d outside 2..%d", m, CH_MAX_M);
  if (d < m - 1) return fail(RQ_EINVAL, "chain_dims: d=%d < m - 1 = %d (an empty chain part)", d, m - 1);
  if (!lo || !hi) return fail(RQ_EINVAL, "chain_dims: null pointer");
  for (int i = 0; i < m; ++i) {
    int l0, h0, l1, h1;
    chain_split(d, m - 1, std::max(i - 1, 0), &l0, &h0);
    chain_split(d, m - 1, std::min(i, m - 2), &l1, &h1);
    lo[i] = l0;
    hi[i] = h1;
  }
  return RQ_OK;
}

extern "C" int rq_dev_quantize_chainq(uint8_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h,
                                      int nsplits, void *stream) {
  RQ_TRY(chain_check_encode(codes, X, C, n, d, m, h, nsplits, "quantize_chainq"));
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  chain_clock_reset();
  PhaseClock clk((hipStream_t)stream, g_chain_ms, false);
  return chain_encode_dev(codes, X, C, n, d, m, h, nsplits, (hipStream_t)stream, clk);
}

extern "C" int rq_quantize_chainq(uint8_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h,
                                  int nsplits) {
  RQ_TRY(chain_check_encode(codes, X, C, n, d, m, h, nsplits, "quantize_chainq"));
  chain_clock_reset();
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  DevMem dX, dC, dcodes;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  RQ_TRY(dcodes.alloc((size_t)n * m));
  RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dC.p, C, (size_t)m * h * d * 4, hipMemcpyHostToDevice));
  {
    PhaseClock clk(nullptr, g_chain_ms);
    RQ_TRY(chain_encode_dev((uint8_t *)dcodes.p, (const float *)dX.p, (const float *)dC.p, n, d, m, h, nsplits, nullptr, clk));
    clk.collect();
  }
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(codes, dcodes.p, (size_t)n * m, hipMemcpyDeviceToHost));
  return RQ_OK;
}

extern "C" int rq_dev_update_codebooks_chain(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h,
                                             double rho, void *stream) {
  RQ_TRY(chain_check_update(C, X, codes, n, d, m, h, rho, "update_codebooks_chain"));
  hipStream_t s = (hipStream_t)stream;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  RQ_TRY(dev_code_range(codes, n, m, h, s, "update_codebooks_chain"));
  chain_clock_reset();
  PhaseClock clk(s, g_chain_ms, false);
  return chain_update_dev(C, X, codes, n, d, m, h, rho, s, clk);
}

extern "C" int rq_update_codebooks_chain(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h,
                                         double rho) {
  RQ_TRY(chain_check_update(C, X, codes, n, d, m, h, rho, "update_codebooks_chain"));
  RQ_TRY(host_code_range(codes, n, m, h, "update_codebooks_chain"));
  chain_clock_reset();
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
  {
    PhaseClock clk(nullptr, g_chain_ms);
    RQ_TRY(chain_update_dev((float *)dC.p, (const float *)dX.p, (const uint8_t *)dcodes.p, n, d, m, h, rho, nullptr, clk));
    clk.collect();
  }
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(C, dC.p, (size_t)m * h * d * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

extern "C" int rq_dev_reconstruct_aq(float *CB, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h,
                                     void *stream) {
  if (m < 1 || m > CH_MAX_M || h < 2 || h > 256 || d < 1 || n < 0)
    return fail(RQ_EINVAL, "reconstruct_aq: n=%lld d=%d m=%d h=%d", (long long)n, d, m, h);
  if (n > 0 && (!CB || !codes || !C)) return fail(RQ_EINVAL, "reconstruct_aq: null pointer");
  RQ_TRY(dev_code_range(codes, n, m, h, (hipStream_t)stream, "reconstruct_aq"));
  return chain_reconstruct_dev(CB, codes, C, n, d, m, h, (hipStream_t)stream);
}

namespace rq {
namespace {
// rq_train_chainq / rq_train_chainq_wide after their argument checks (src/ChainQ.jl:393-426).  codes [n][m] on the host, in
// code_base .. code_base + h - 1 (bytes: code_base 0).  The byte instantiation queues exactly what rq_train_chainq always has.
template <class Code>
int train_chainq_host(float *C, Code *codes, float *R, double *obj, const float *X, int64_t n, int d, int m, int h, int niter,
                      int code_base, const char *who) {
  chain_clock_reset();
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  const size_t xb = (size_t)n * d * 4, cb = (size_t)m * h * d * 4, kb = (size_t)n * m * sizeof(Code);
  DevMem dX, dRX, dCB, dR, dC, dcodes, dG, dobj, dstat, dns;
  RQ_TRY(dX.alloc(xb)); RQ_TRY(dRX.alloc(xb)); RQ_TRY(dCB.alloc(xb));
  RQ_TRY(dR.alloc((size_t)d * d * 4)); RQ_TRY(dG.alloc((size_t)d * d * 4));
  RQ_TRY(dC.alloc(cb)); RQ_TRY(dcodes.alloc(kb));
  RQ_TRY(dobj.alloc((size_t)(niter + 1) * 8)); RQ_TRY(dstat.alloc(8));
  RQ_TRY(dns.alloc(polar_ns_scratch_bytes(d, di.num_cu)));
  RQ_HIP(hipMemcpy(dX.p, X, xb, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dR.p, R, (size_t)d * d * 4, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dcodes.p, codes, kb, hipMemcpyHostToDevice));
  const float *Xd = (const float *)dX.p;
  float *RX = (float *)dRX.p, *CB = (float *)dCB.p, *Rd = (float *)dR.p, *Cd = (float *)dC.p, *G = (float *)dG.p;
  Code *B = (Code *)dcodes.p;
  double *objd = (double *)dobj.p;
  const hipStream_t s = nullptr;
  {
    PhaseClock clk(s, g_chain_ms);
    if constexpr (std::is_same<Code, int16_t>::value)
      if (code_base) RQ_TRY(add_base_codes_launch(B, n * m, -code_base, s));   // the loop runs on zero-based codes
    // RX = R'X; C = update(RX, B); B = viterbi(RX, C)   (src/ChainQ.jl:393-401)
    RQ_TRY(rotate_launch(RX, Rd, Xd, d, n, di.num_cu, s));
    clk.mark(CP_ROTATION);
    RQ_TRY(chain_update_dev(Cd, RX, B, n, d, m, h, 1e-4, s, clk));
    RQ_TRY(chain_encode_dev(B, RX, Cd, n, d, m, h, 1, s, clk));
    for (int it = 0; it <= niter; ++it) {
      // obj[iter] = qerror(RX, B, C); CB = reconstruct(B, C); R = polar(X CB'); RX = R'X   (:407-419)
      RQ_TRY(chain_reconstruct_dev(CB, B, Cd, n, d, m, h, s));
      RQ_TRY(qerror_launch(objd + it, RX, CB, n, d, di.num_cu, s));
      RQ_TRY(gram_launch(G, Xd, CB, n, d, di.num_cu, s));
      RQ_HIP(hipMemsetAsync(dstat.p, 0, 8, s));
      RQ_TRY(polar_ns_launch(Rd, G, d, (int *)dstat.p, dns.p, di.num_cu, s));
      int st2[2] = {1, 0};
      RQ_HIP(hipMemcpy(st2, dstat.p, 8, hipMemcpyDeviceToHost));
      if (st2[0] != 0)
        return fail(RQ_EUNSUPPORTED, "%s: the polar factor of X CB' did not converge in round %d (rank-deficient)", who, it);
      RQ_TRY(rotate_launch(RX, Rd, Xd, d, n, di.num_cu, s));
      clk.mark(CP_ROTATION);
      RQ_TRY(chain_update_dev(Cd, RX, B, n, d, m, h, 1e-4, s, clk));   // (:423-426)
      RQ_TRY(chain_encode_dev(B, RX, Cd, n, d, m, h, 1, s, clk));
    }
    if constexpr (std::is_same<Code, int16_t>::value)
      if (code_base) RQ_TRY(add_base_codes_launch(B, n * m, code_base, s));
    clk.collect();
  }
  RQ_HIP(hipDeviceSynchronize());
  std::vector<double> acc((size_t)niter + 1);
  RQ_HIP(hipMemcpy(acc.data(), objd, acc.size() * 8, hipMemcpyDeviceToHost));
  for (int it = 0; it <= niter; ++it) obj[it] = acc[it] / (double)n;
  RQ_HIP(hipMemcpy(C, Cd, cb, hipMemcpyDeviceToHost));
  RQ_HIP(hipMemcpy(codes, B, kb, hipMemcpyDeviceToHost));
  RQ_HIP(hipMemcpy(R, Rd, (size_t)d * d * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}
}  // namespace
}  // namespace rq

extern "C" int rq_train_chainq(float *C, uint8_t *codes, float *R, double *obj, const float *X, int64_t n, int d, int m,
                               int h, int niter) {
  RQ_TRY(chain_check_update(C, X, codes, n, d, m, h, 1e-4, "train_chainq"));
  if (n < 1) return fail(RQ_EINVAL, "train_chainq: n=%lld < 1", (long long)n);
  if (niter < 0) return fail(RQ_EINVAL, "train_chainq: niter=%d < 0", niter);
  if (!R || !obj) return fail(RQ_EINVAL, "train_chainq: null R or obj");
  if (d > 1024) return fail(RQ_EUNSUPPORTED, "train_chainq: the device polar factor covers d <= 1024; got %d", d);
  RQ_TRY(host_code_range(codes, n, m, h, "train_chainq"));
  return train_chainq_host<uint8_t>(C, codes, R, obj, X, n, d, m, h, niter, 0, "train_chainq");
}

// ---- 2 <= h <= RQ_MAX_H16 over int16 codes: the int16 kernels at EVERY h, host pointers ------------------
extern "C" int rq_chain_wide_plan(int64_t n, int d, int m, int h, int nsplits, int64_t *out, int cap) {
  const char *who = "rq_chain_wide_plan";
  if (!out || cap < 0) return fail(RQ_EINVAL, "%s: null pointer or negative cap", who);
  RQ_TRY(chain_check_encode(out, out, out, n, d, m, h, nsplits, who, RQ_MAX_H16));
  ChainWidePlan pl;
  RQ_TRY(chain_wide_plan(&pl, n, m, h, nsplits, who));
  const int64_t trains = (m >= 2 && d >= m - 1 && d <= 1024 && 2 * h <= CHW_MAX_H2) ? 1 : 0;
  const int64_t v[7] = {pl.HS, (int64_t)pl.table_bytes, (int64_t)pl.row_bytes, pl.chunk, pl.chunks, (int64_t)4 * h * h * 8, trains};
  for (int q = 0; q < cap && q < 7; ++q) out[q] = v[q];
  return RQ_OK;
}

extern "C" int rq_quantize_chainq_wide(int16_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int nsplits,
                                       int code_base) {
  const char *who = "quantize_chainq_wide";
  RQ_TRY(chain_check_encode(codes, X, C, n, d, m, h, nsplits, who, RQ_MAX_H16));
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  ChainWidePlan pl;
  RQ_TRY(chain_wide_plan(&pl, n, m, h, nsplits, who));
  chain_clock_reset();
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  DevMem dX, dC, dcodes;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  RQ_TRY(dcodes.alloc((size_t)n * m * 2));
  RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dC.p, C, (size_t)m * h * d * 4, hipMemcpyHostToDevice));
  {
    PhaseClock clk(nullptr, g_chain_ms);
    RQ_TRY(chain_encode_dev(dcodes.as<int16_t>(), (const float *)dX.p, (const float *)dC.p, n, d, m, h, nsplits, nullptr, clk));
    if (code_base) RQ_TRY(add_base_codes_launch(dcodes.as<int16_t>(), n * m, code_base, nullptr));
    clk.collect();
  }
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(codes, dcodes.p, (size_t)n * m * 2, hipMemcpyDeviceToHost));
  return RQ_OK;
}

extern "C" int rq_update_codebooks_chain_wide(float *C, const float *X, const int16_t *codes, int64_t n, int d, int m, int h,
                                              double rho, int code_base) {
  const char *who = "update_codebooks_chain_wide";
  RQ_TRY(chain_check_update(C, X, codes, n, d, m, h, rho, who, RQ_MAX_H16));
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  RQ_TRY(chain_wide_update_rule(h, who));
  RQ_TRY(host_code_range(codes, n, m, h, code_base, who));
  chain_clock_reset();
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  DevMem dX, dcodes, dC;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  RQ_TRY(dcodes.alloc((size_t)n * m * 2));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  if (n > 0) {
    RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(dcodes.p, codes, (size_t)n * m * 2, hipMemcpyHostToDevice));
    if (code_base) RQ_TRY(add_base_codes_launch(dcodes.as<int16_t>(), n * m, -code_base, nullptr));
  }
  {
    PhaseClock clk(nullptr, g_chain_ms);
    RQ_TRY(chain_update_dev((float *)dC.p, (const float *)dX.p, (const int16_t *)dcodes.p, n, d, m, h, rho, nullptr, clk));
    clk.collect();
  }
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(C, dC.p, (size_t)m * h * d * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

extern "C" int rq_train_chainq_wide(float *C, int16_t *codes, float *R, double *obj, const float *X, int64_t n, int d, int m, int h,
                                    int niter, int code_base) {
  const char *who = "train_chainq_wide";
  RQ_TRY(chain_check_update(C, X, codes, n, d, m, h, 1e-4, who, RQ_MAX_H16));
  if (n < 1) return fail(RQ_EINVAL, "%s: n=%lld < 1", who, (long long)n);
  if (niter < 0) return fail(RQ_EINVAL, "%s: niter=%d < 0", who, niter);
  if (!R || !obj) return fail(RQ_EINVAL, "%s: null R or obj", who);
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  if (d > 1024) return fail(RQ_EUNSUPPORTED, "%s: the device polar factor covers d <= 1024; got %d", who, d);
  ChainWidePlan pl;
  RQ_TRY(chain_wide_plan(&pl, n, m, h, 1, who));
  RQ_TRY(chain_wide_update_rule(h, who));
  RQ_TRY(host_code_range(codes, n, m, h, code_base, who));
  return train_chainq_host<int16_t>(C, codes, R, obj, X, n, d, m, h, niter, code_base, who);
}

extern "C" int rq_last_chainq_timing(double *ms, int cap) {
  if (!ms) return fail(RQ_EINVAL, "rq_last_chainq_timing: null pointer");
  for (int q = 0; q < cap && q < CP_N; ++q) ms[q] = g_chain_ms[q];
  return RQ_OK;
}
