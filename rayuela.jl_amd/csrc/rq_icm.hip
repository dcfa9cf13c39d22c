// rq_icm.hip -- LSQ encoding (src/LSQ.jl:272-302 encoding_icm, src/LSQ_GPU.jl:218-264 encode_icm_cuda) on gfx950:
// iterated local search (ILS) around iterated conditional modes (ICM), contract in DESIGN.md section 2.
//
//   icm_pair_kernel    once per call: binT[j][k][b][l] = 2 <c_jl, c_kb>  (both orientations, one contiguous row of
//                      HS = 64 * ceil(h / 64) floats per (j, k, b), zero past h) and sa[i][k] = <c_ik, c_ik>.
//   icm_unary_kernel   per chunk of rows: U[row][i][k] = fl(sa_i[k] - 2 <c_ik, x>) on v_mfma_f32_32x32x2_f32 (a k-ordered
//                      fmaf chain, bit for bit, as in rq_encode.hip's rotation).
//   icm_ils_kernel     per chunk of rows, ONE launch for the whole ILS: one wavefront per row, lane l holds entries
//                      l*E .. l*E+E-1 of every unary in registers; a conditioning step is m-1 independent row gathers of
//                      binT (1 KiB dwordx4 per wavefront at h = 256), f32 adds in ascending k, a first-index argmin; the
//                      perturbation (counter-based splitmix64) and the veccost accept test run in the same kernel.
// Every dot product is a k-ordered fmaf chain from +0; adds are unfused (-ffp-contract=off), so the codes equal the CPU
// restatement tests/icm_oracle.py bit for bit.
#include "rq_icm_shared.h"

#include <vector>

namespace rq {

namespace {

// ---- binaries and self-products ----------------------------------------------------------------
// block = one (j, k, b) row, thread = l.  j == k rows are never gathered and stay zero.
__global__ __launch_bounds__(256) void icm_pair_kernel(float *binT, const float *C, int m, int h, int d, int HS) {
  const int row = blockIdx.x;                     // (j * m + k) * h + b
  const int b = row % h, jk = row / h, k = jk % m, j = jk / m;
  const int l = threadIdx.x;
  if (j == k || l >= h) return;
  const float *cj = C + ((size_t)j * h + l) * d;
  const float *ck = C + ((size_t)k * h + b) * d;
  float acc = 0.0f;
  for (int t = 0; t < d; ++t) acc = __builtin_fmaf(cj[t], ck[t], acc);
  binT[(size_t)row * HS + l] = 2.0f * acc;
}

__global__ __launch_bounds__(256) void icm_sqnorm_kernel(float *sa, const float *C, int mh, int d) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= mh) return;
  const float *cc = C + (size_t)c * d;
  float acc = 0.0f;
  for (int t = 0; t < d; ++t) acc = __builtin_fmaf(cc[t], cc[t], acc);
  sa[c] = acc;
}

// ---- unaries: U[row][i][k] = fl(sa[i*h+k] - 2 g), g = <c_ik, x_row> ----------------------------------------------
// A wavefront owns 32 rows x 32 of the m*h codewords (A = codewords, B = rows); lane l feeds k = 2kk + (l >> 5), so the
// chain of every output runs k = 0..d-1 in order (an odd d pads one zero pair: fma(0, 0, acc) = acc).
constexpr int UN_WAVES = 4;
using icm_f32x16 = float __attribute__((ext_vector_type(16)));
// RANGE (the chain encoder, rq_chain.hip): rng[2i], rng[2i+1] = the dimensions [lo, hi) outside which codebook i is zero; the
// chain then runs over the tile's codebooks' ranges only.  A skipped term is fma(+-0, x, acc) = acc for finite x: same bits.
template <bool RANGE>
__global__ __launch_bounds__(UN_WAVES * 64) void icm_unary_kernel(float *U, const float *X, const float *C,
                                                                const float *sa, int64_t nrows, int d, int m, int h,
                                                                int HS, const int *rng) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, hi = lane >> 5;
  const int mh = m * h;
  const int ct = blockIdx.y * UN_WAVES + wave;
  if (ct * 32 >= mh) return;
  const int64_t row0 = (int64_t)blockIdx.x * 32;
  const int cw = ct * 32 + j;
  const bool cw_ok = cw < mh;
  const int64_t r = row0 + j;
  const bool r_ok = r < nrows;
  const float *ap = C + (size_t)(cw_ok ? cw : 0) * d + hi;
  const float *bp = X + (size_t)(r_ok ? r : row0) * d + hi;
  icm_f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  const int KF = d >> 1;   // full k pairs
  int kb = 0, ke = KF;
  bool tail = d & 1;
  if constexpr (RANGE) {
    int lo = d, hi = 0;
    for (int i = (ct * 32) / h; i <= std::min(ct * 32 + 31, mh - 1) / h; ++i) {
      lo = std::min(lo, rng[2 * i]);
      hi = std::max(hi, rng[2 * i + 1]);
    }
    kb = lo >> 1;
    ke = std::min(KF, (hi + 1) >> 1);
    tail = tail && hi > 2 * KF;
  }
#pragma unroll 8
  for (int kk = kb; kk < ke; ++kk) {
    const float a = cw_ok ? ap[2 * kk] : 0.0f;
    const float b = bp[2 * kk];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (tail) {
    const float a = (cw_ok && hi == 0) ? ap[2 * KF] : 0.0f;
    const float b = hi == 0 ? bp[2 * KF] : 0.0f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (!r_ok) return;
  float *o = U + (size_t)r * m * HS;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = ct * 32 + 4 * hi + 8 * (q >> 2) + (q & 3);
    if (c < mh) {
      const int i = c / h, k = c - i * h;
      o[(size_t)i * HS + k] = sa[c] - 2.0f * acc[q];
    }
  }
}

// ---- the fused ILS kernel ----------------------------------------------------------------------------------
struct IcmParams {
  uint8_t *codes_out;        // [nrows][m]   (may alias codes_in)
  const uint8_t *codes_in;   // [nrows][m]
  float *cost_out;           // [nrows] or null
  const float *U;            // [nrows][m][HS]
  const float *binT;         // [m][m][h][HS]
  const float *X;            // [nrows][d]
  const float *C;            // [m][h][d]
  int64_t nrows, row_base, t0;
  uint64_t seed;
  int d, m, h, HS, ilsiter, icmiter, npert, randord;
};

template <int E>
__device__ __forceinline__ void icm_load(float (&v)[E], const float *p) {
  if constexpr (E == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (E == 2) {
    const float2 t = *reinterpret_cast<const float2 *>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = p[e];
  }
}

template <int MB, int E>
__global__ __launch_bounds__(256) void icm_ils_kernel(IcmParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.nrows) return;
  const int m = p.m, h = p.h, HS = p.HS, d = p.d;
  const float *x = p.X + (size_t)row * d;
  int b[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) b[i] = i < m ? (int)p.codes_in[row * m + i] : 0;
  float u[MB][E];
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    if (i < m) {
      icm_load<E>(u[i], p.U + ((size_t)row * m + i) * HS + lane * E);
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (lane * E + e >= h) u[i][e] = __builtin_inff();   // padding never wins
    }
  }
  float cost_old = icm_cost<MB>(b, x, p.C, d, m, h, lane);
  const uint64_t zs = icm_z(p.seed);
  const uint64_t grow = (uint64_t)(p.row_base + row);
#pragma unroll 1
  for (int it = 0; it < p.ilsiter; ++it) {
    const uint64_t t = (uint64_t)(p.t0 + it);
    // visit order pi_t: 4-bit entries packed in one word (no dynamically indexed register array)
    uint64_t perm = 0;
    for (int i = 0; i < m; ++i) perm |= (uint64_t)i << (4 * i);
    if (p.randord) {
      const uint64_t q = icm_z(zs ^ (t | (1ull << 63)));
      for (int i = m - 1; i >= 1; --i) {
        const uint32_t r = icm_scale(icm_z(q + (uint64_t)i), (uint32_t)(i + 1));
        const uint64_t vi = (perm >> (4 * i)) & 15, vr = (perm >> (4 * r)) & 15;
        perm &= ~((15ull << (4 * i)) | (15ull << (4 * r)));
        perm |= (vr << (4 * i)) | (vi << (4 * r));
      }
    }
    // perturbation: selection sampling of npert distinct positions, uniform new values
    int nb[MB];
    const uint64_t base = icm_z(icm_z(zs ^ t) ^ grow);
    int need = p.npert;
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      nb[i] = b[i];
      if (i < m) {
        const uint32_t r = icm_scale(icm_z(base + (uint64_t)i), (uint32_t)(m - i));
        if ((int)r < need) {
          --need;
          nb[i] = (int)icm_scale(icm_z(base + (uint64_t)(m + i)), (uint32_t)h);
        }
      }
    }
#pragma unroll 1
    for (int s = 0; s < p.icmiter; ++s) {
#pragma unroll 1
      for (int jj = 0; jj < m; ++jj) {
        const int j = (int)((perm >> (4 * jj)) & 15);
        float ub[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          ub[e] = u[0][e];
#pragma unroll
          for (int i = 1; i < MB; ++i)
            if (i == j) ub[e] = u[i][e];
        }
        float g[MB][E];
        // 32-bit element offsets (m * m * h * HS < 2^25): the gathers take the SGPR base + VGPR offset form
        const uint32_t oj = (uint32_t)(j * m) * (uint32_t)h;
#pragma unroll
        for (int k = 0; k < MB; ++k)
          if (k < m && k != j)
            icm_load<E>(g[k], p.binT + (((oj + (uint32_t)(k * h) + (uint32_t)nb[k]) * (uint32_t)HS) + (uint32_t)(lane * E)));
#pragma unroll
        for (int k = 0; k < MB; ++k)
          if (k < m && k != j) {
#pragma unroll
            for (int e = 0; e < E; ++e) ub[e] = ub[e] + g[k][e];
          }
        // first index of the minimum: in-lane scan (ascending index), then a (value, index) butterfly
        float bv = ub[0];
        int bi = lane * E;
#pragma unroll
        for (int e = 1; e < E; ++e)
          if (ub[e] < bv) { bv = ub[e]; bi = lane * E + e; }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const float ov = __shfl_xor(bv, off, 64);
          const int oi = __shfl_xor(bi, off, 64);
          if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        int res = __shfl(bi, 0, 64);   // lane 0's winner for every lane (kept in VGPRs: no SGPR pressure)
        if (res < 0 || res >= h) res = 0;   // only reachable with NaN costs: keep the code in range
#pragma unroll
        for (int i = 0; i < MB; ++i)
          if (i == j) nb[i] = res;
      }
    }
    const float c = icm_cost<MB>(nb, x, p.C, d, m, h, lane);
    if (c < cost_old) {   // strict: an equal cost keeps the old codes
      cost_old = c;
#pragma unroll
      for (int i = 0; i < MB; ++i) b[i] = nb[i];
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < MB; ++i)
      if (i < m) p.codes_out[row * m + i] = (uint8_t)b[i];
    if (p.cost_out) p.cost_out[row] = cost_old;
  }
}

template <int MB>
static void launch_ils_e(const IcmParams &p, dim3 grid, hipStream_t stream) {
  const int E = p.HS / 64;
  if (E == 1) hipLaunchKernelGGL((icm_ils_kernel<MB, 1>), grid, dim3(256), 0, stream, p);
  else if (E == 2) hipLaunchKernelGGL((icm_ils_kernel<MB, 2>), grid, dim3(256), 0, stream, p);
  else if (E == 3) hipLaunchKernelGGL((icm_ils_kernel<MB, 3>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((icm_ils_kernel<MB, 4>), grid, dim3(256), 0, stream, p);
}

__global__ __launch_bounds__(256) void icm_code_range_kernel(unsigned int *bad, const uint8_t *codes, int64_t nelem,
                                                             int h) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nelem; i += (int64_t)gridDim.x * 256)
    if (codes[i] >= h) { atomicOr(bad, 1u); return; }
}

}  // namespace

// codes < h on the device: one flag word, read back before any other work is queued
int dev_code_range(const uint8_t *codes, int64_t n, int m, int h, hipStream_t s, const char *who) {
  if (h >= 256 || n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  void *wf = nullptr;
  RQ_TRY(workspace(WS_TMP, 256, &wf, s));
  RQ_HIP(hipMemsetAsync(wf, 0, 4, s));
  const int64_t nelem = n * m;
  const int grid = (int)std::min<int64_t>((nelem + 255) / 256, 4096);
  hipLaunchKernelGGL(icm_code_range_kernel, dim3(grid), dim3(256), 0, s, (unsigned int *)wf, codes, nelem, h);
  RQ_HIP(hipGetLastError());
  unsigned int bad = 0;
  RQ_HIP(hipMemcpyAsync(&bad, wf, 4, hipMemcpyDeviceToHost, s));
  RQ_HIP(hipStreamSynchronize(s));
  if (bad) return fail(RQ_EINVAL, "%s: a code is >= h=%d", who, h);
  return RQ_OK;
}

int host_code_range(const uint8_t *codes, int64_t n, int m, int h, const char *who) {
  if (h >= 256) return RQ_OK;
  for (int64_t e = 0; e < n * m; ++e)
    if (codes[e] >= h)
      return fail(RQ_EINVAL, "%s: code %d at [%lld][%lld] is >= h=%d", who, codes[e], (long long)(e / m), (long long)(e % m), h);
  return RQ_OK;
}

int host_code_range(const int16_t *codes, int64_t n, int m, int h, int code_base, const char *who) {
  for (int64_t e = 0; e < n * m; ++e)
    if (codes[e] < code_base || codes[e] > h - 1 + code_base)
      return fail(RQ_EINVAL, "%s: code %d at [%lld][%lld] is outside %d..%d", who, codes[e], (long long)(e / m), (long long)(e % m),
                  code_base, h - 1 + code_base);
  return RQ_OK;
}

int icm_check_args(const void *codes_out, const void *codes_in, const void *X, const void *C, int64_t n, int d, int m,
                   int h, int ilsiter, int icmiter, int npert, int64_t t0, int nsplits) {
  if (m < 1 || m > ICM_MAX_M) return fail(RQ_EINVAL, "encode_icm: m=%d outside 1..%d", m, ICM_MAX_M);
  if (h < 2 || h > 256) return fail(RQ_EINVAL, "encode_icm: h=%d outside 2..256", h);
  if (d < 1) return fail(RQ_EINVAL, "encode_icm: d=%d < 1", d);
  if (n < 0 || ilsiter < 0 || icmiter < 0 || t0 < 0)
    return fail(RQ_EINVAL, "encode_icm: negative count (n=%lld ilsiter=%d icmiter=%d t0=%lld)", (long long)n, ilsiter,
                icmiter, (long long)t0);
  if (npert < 0 || npert > m) return fail(RQ_EINVAL, "encode_icm: npert=%d outside 0..m=%d", npert, m);
  if (nsplits < 1) return fail(RQ_EINVAL, "encode_icm: nsplits=%d < 1", nsplits);
  if (n > 0 && (!codes_out || !codes_in || !X || !C)) return fail(RQ_EINVAL, "encode_icm: null pointer");
  return RQ_OK;
}

// The device body: arguments already checked, codes already in range.
int icm_encode_dev(uint8_t *codes_out, const uint8_t *codes_in, float *cost_out, const float *X, const float *C,
                   int64_t n, int d, int m, int h, int ilsiter, int icmiter, int npert, int randord, uint64_t seed,
                   int64_t t0, int nsplits, hipStream_t stream, double *unary_ms) {
  if (n <= 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  const int E = (h + 63) / 64, HS = 64 * E;
  const size_t bin_bytes = (size_t)m * m * h * HS * 4, sa_bytes = (size_t)m * h * 4;
  const size_t row_bytes = (size_t)m * HS * 4;
  const size_t u_budget = ICM_SCRATCH_BYTES - bin_bytes - sa_bytes;   // <= 64 MiB + 16 KiB of the 2 GiB
  int64_t chunk = (n + nsplits - 1) / nsplits;
  chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(u_budget / row_bytes)));
  void *wbin = nullptr, *wu = nullptr;
  RQ_TRY(workspace(WS_ICM_BIN, bin_bytes + sa_bytes, &wbin, stream));
  RQ_TRY(workspace(WS_ICM_U, (size_t)chunk * row_bytes, &wu, stream));
  float *binT = (float *)wbin, *sa = binT + bin_bytes / 4, *U = (float *)wu;
  // a zero-iteration encode is a veccost pass: the ILS kernel then uses neither the tables nor the unaries it loads
  const bool tables = ilsiter > 0;
  if (tables) {
    RQ_HIP(hipMemsetAsync(binT, 0, bin_bytes, stream));
    hipLaunchKernelGGL(icm_pair_kernel, dim3(m * m * h), dim3(256), 0, stream, binT, C, m, h, d, HS);
    RQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(icm_sqnorm_kernel, dim3((m * h + 255) / 256), dim3(256), 0, stream, sa, C, m * h, d);
    RQ_HIP(hipGetLastError());
  }
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (unary_ms) {
    *unary_ms = 0;
    RQ_HIP(hipEventCreate(&ev[0]));
    RQ_HIP(hipEventCreate(&ev[1]));
  }
  int rc = RQ_OK;
  for (int64_t r0 = 0; r0 < n && rc == RQ_OK; r0 += chunk) {
    const int64_t nr = std::min(chunk, n - r0);
    const int ctiles = (m * h + 31) / 32;
    if (unary_ms) (void)hipEventRecord(ev[0], stream);
    if (tables) {
      hipLaunchKernelGGL(icm_unary_kernel<false>, dim3((unsigned)((nr + 31) / 32), (ctiles + UN_WAVES - 1) / UN_WAVES),
                         dim3(UN_WAVES * 64), 0, stream, U, X + (size_t)r0 * d, C, sa, nr, d, m, h, HS, (const int *)nullptr);
      if (hipGetLastError() != hipSuccess) { rc = fail(RQ_EINVAL, "encode_icm: unary launch failed"); break; }
    }
    if (unary_ms) {
      (void)hipEventRecord(ev[1], stream);
      (void)hipEventSynchronize(ev[1]);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
      *unary_ms += ms;
    }
    IcmParams p;
    p.codes_out = codes_out + (size_t)r0 * m;
    p.codes_in = codes_in + (size_t)r0 * m;
    p.cost_out = cost_out ? cost_out + r0 : nullptr;
    p.U = U; p.binT = binT; p.X = X + (size_t)r0 * d; p.C = C;
    p.nrows = nr; p.row_base = r0; p.t0 = t0; p.seed = seed;
    p.d = d; p.m = m; p.h = h; p.HS = HS; p.ilsiter = ilsiter; p.icmiter = icmiter; p.npert = npert;
    p.randord = randord ? 1 : 0;
    const dim3 grid((unsigned)((nr + 3) / 4));
    if (m <= 4) launch_ils_e<4>(p, grid, stream);
    else if (m <= 8) launch_ils_e<8>(p, grid, stream);
    else launch_ils_e<16>(p, grid, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = fail_hip(e, "icm_ils_kernel", __FILE__, __LINE__);
  }
  if (ev[0]) (void)hipEventDestroy(ev[0]);
  if (ev[1]) (void)hipEventDestroy(ev[1]);
  return rc;
}

// The unaries of one chunk of rows, and the self-products they need, for the other users of the LSQ encoding contract
// (rq_chain.hip): U [nrows][m][HS] with HS = 64 * ceil(h / 64), sa [m * h]; rng [m][2] (device) or null = every dimension.
int icm_sqnorm_launch(float *sa, const float *C, int m, int h, int d, hipStream_t stream) {
  hipLaunchKernelGGL(icm_sqnorm_kernel, dim3((m * h + 255) / 256), dim3(256), 0, stream, sa, C, m * h, d);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

int icm_unary_launch(float *U, const float *X, const float *C, const float *sa, int64_t nrows, int d, int m, int h, int HS,
                     const int *rng, hipStream_t stream) {
  if (nrows <= 0) return RQ_OK;
  const int ctiles = (m * h + 31) / 32;
  const dim3 grid((unsigned)((nrows + 31) / 32), (ctiles + UN_WAVES - 1) / UN_WAVES);
  if (rng) hipLaunchKernelGGL(icm_unary_kernel<true>, grid, dim3(UN_WAVES * 64), 0, stream, U, X, C, sa, nrows, d, m, h, HS, rng);
  else hipLaunchKernelGGL(icm_unary_kernel<false>, grid, dim3(UN_WAVES * 64), 0, stream, U, X, C, sa, nrows, d, m, h, HS, rng);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

namespace {

thread_local double g_icm_unary_ms = 0, g_icm_total_ms = 0;

}  // namespace

void icm_set_timing(double unary_ms, double total_ms) {
  g_icm_unary_ms = unary_ms;
  g_icm_total_ms = total_ms;
}

}  // namespace rq

using namespace rq;

extern "C" int rq_dev_encode_icm(uint8_t *codes_out, const uint8_t *codes_in, float *cost_out, const float *X,
                                 const float *C, int64_t n, int d, int m, int h, int ilsiter, int icmiter, int npert,
                                 int randord, uint64_t seed, int64_t t0, int nsplits, void *stream) {
  RQ_TRY(icm_check_args(codes_out, codes_in, X, C, n, d, m, h, ilsiter, icmiter, npert, t0, nsplits));
  if (n == 0) return RQ_OK;
  hipStream_t s = (hipStream_t)stream;
  RQ_TRY(dev_code_range(codes_in, n, m, h, s, "encode_icm"));
  return icm_encode_dev(codes_out, codes_in, cost_out, X, C, n, d, m, h, ilsiter, icmiter, npert, randord, seed, t0,
                        nsplits, s, nullptr);
}

extern "C" int rq_encode_icm(uint8_t *codes_out, const uint8_t *codes_in, float *cost_out, const float *X,
                             const float *C, int64_t n, int d, int m, int h, int ilsiter, int icmiter, int npert,
                             int randord, uint64_t seed, int64_t t0, int nsplits) {
  RQ_TRY(icm_check_args(codes_out, codes_in, X, C, n, d, m, h, ilsiter, icmiter, npert, t0, nsplits));
  RQ_TRY(host_code_range(codes_in, n, m, h, "encode_icm"));
  g_icm_unary_ms = g_icm_total_ms = 0;
  if (n == 0) return RQ_OK;
  Timer tt;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  DevMem dX, dC, dcodes, dcost;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  RQ_TRY(dcodes.alloc((size_t)n * m));
  RQ_TRY(dcost.alloc((size_t)n * 4));
  RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dC.p, C, (size_t)m * h * d * 4, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dcodes.p, codes_in, (size_t)n * m, hipMemcpyHostToDevice));
  double un_ms = 0;
  RQ_TRY(icm_encode_dev((uint8_t *)dcodes.p, (const uint8_t *)dcodes.p, cost_out ? (float *)dcost.p : nullptr,
                        (const float *)dX.p, (const float *)dC.p, n, d, m, h, ilsiter, icmiter, npert, randord, seed,
                        t0, nsplits, nullptr, &un_ms));
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(codes_out, dcodes.p, (size_t)n * m, hipMemcpyDeviceToHost));
  if (cost_out) RQ_HIP(hipMemcpy(cost_out, dcost.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  g_icm_unary_ms = un_ms;
  g_icm_total_ms = tt.ms();
  return RQ_OK;
}

extern "C" int rq_last_icm_timing(double *unary_ms, double *total_ms) {
  if (unary_ms) *unary_ms = g_icm_unary_ms;
  if (total_ms) *total_ms = g_icm_total_ms;
  return RQ_OK;
}
