// rq_norms.hip -- the database norms of additive-quantizer search (src/utils.jl:4-26 get_norms_codebook, :29-59
// quantize_norms) on gfx950; contract in DESIGN.md section 4.14.
//
//   aq_norms_kernel       norms[i] = |sum_k C_k[b_ik]|^2 straight from codes and codebooks: one wavefront per row, NR rows in
//                         flight per wavefront, the n x d reconstruction is never written.  The order of the f32 sums is
//                         veccost's (rq_icm.hip icm_cost): CB[t] by adds from +0 in codebook order, lane l sums CB[t]^2 over
//                         t = l, l + 64, ... from +0 (multiply and add unfused: -ffp-contract=off), the xor butterfly
//                         32, 16, 8, 4, 2, 1 adds the 64 partial sums.  So norms == veccost of an all-zero X, bit for bit.
//   quantize_norms_kernel first index j minimising fl(fl(norm - cb[j])^2) (strict <: findmin, src/utils.jl:50-55), the
//                         unsorted codebook of hn <= 256 entries in LDS; optionally the dequantised cb[j] beside the code.
// The 1-D k-means of get_norms_codebook is train_pq_resident (rq_train_host.hip) with d = m = 1 on the resident norms.
// The *_wide entries are the same kernels over int16 codes: aq_norms_kernel<int16_t> for
// 2 <= h <= RQ_MAX_H16, quantize_norms_wide_kernel with the table of hn <= RQ_MAX_H16 entries in dynamic LDS (128 KiB at most)
// and int16 norm codes, train_pq_resident_wide for the k-means (the byte loop, widened, at hn <= 256 like rq_train_pq_wide).
#include "rq_internal.h"

#include <vector>

namespace rq {

namespace {

constexpr int NR = 4, NI = 4;   // rows per wavefront and codebooks per step: NR * NI independent gathers hide the L2 latency

template <class Code>
__global__ __launch_bounds__(256) void aq_norms_kernel(float *norms, const Code *codes, const float *C, int64_t n, int d,
                                                       int m, int h) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * NR;
  if (row0 >= n) return;
  // lane i holds the codebook row (i * h + b_i < m * h <= 2^21) of each of the wavefront's rows (m <= 64), lanes past m row 0;
  // a row past n repeats row n - 1 and is not stored
  int ent[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int64_t row = std::min<int64_t>(row0 + r, n - 1);
    const int b = (int)codes[row * m + std::min(lane, m - 1)];
    ent[r] = lane < m ? lane * h + b : 0;
  }
  float acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.0f;
  for (int t0 = 0; t0 < d; t0 += 64) {            // uniform trip count: the readlanes below are wavefront-uniform
    const int t = t0 + lane, tc = std::min(t, d - 1);      // every gather reads inside the table; `in` selects
    const bool in = t < d;
    float cb[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) cb[r] = 0.0f;
    for (int i0 = 0; i0 < m; i0 += NI) {          // NI * NR gathers issued before the first add needs one
      float v[NI][NR];
#pragma unroll
      for (int u = 0; u < NI; ++u) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const float *p = C + (size_t)__builtin_amdgcn_readlane(ent[r], (i0 + u) & 63) * d;
          const float g = p[tc];
          v[u][r] = in ? g : 0.0f;
        }
      }
#pragma unroll
      for (int u = 0; u < NI; ++u) {
        if (i0 + u < m) {
#pragma unroll
          for (int r = 0; r < NR; ++r) cb[r] = cb[r] + v[u][r];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = acc[r] + cb[r] * cb[r];
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc[r] = acc[r] + __shfl_xor(acc[r], o, 64);
  }
#pragma unroll
  for (int r = 0; r < NR; ++r)
    if (lane == r && row0 + r < n) norms[row0 + r] = acc[r];
}

// the search of one norm over cb [hn] in LDS: first index of the smallest fl(fl(v - cb[j])^2), strict <
__device__ __forceinline__ int nearest_norm(const float *cb, int hn, float v) {
  float df = v - cb[0];
  float best = df * df;
  int bj = 0;
  for (int j = 1; j < hn; ++j) {
    df = v - cb[j];
    const float e = df * df;
    if (e < best) { best = e; bj = j; }
  }
  return bj;
}

// hn <= RQ_MAX_H16: the table in dynamic LDS (4 hn bytes), int16 codes
__global__ __launch_bounds__(256) void quantize_norms_wide_kernel(int16_t *norm_codes, float *dbnorms, const float *norms,
                                                                  const float *cbnorms, int64_t n, int hn) {
  extern __shared__ __attribute__((aligned(16))) float cbw[];
  for (int j = threadIdx.x; j < hn; j += 256) cbw[j] = cbnorms[j];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int bj = nearest_norm(cbw, hn, norms[i]);
    if (norm_codes) norm_codes[i] = (int16_t)bj;
    if (dbnorms) dbnorms[i] = cbw[bj];
  }
}

__global__ __launch_bounds__(256) void quantize_norms_kernel(uint8_t *norm_codes, float *dbnorms, const float *norms,
                                                             const float *cbnorms, int64_t n, int hn) {
  __shared__ float cb[256];
  if ((int)threadIdx.x < hn) cb[threadIdx.x] = cbnorms[threadIdx.x];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int bj = nearest_norm(cb, hn, norms[i]);
    if (norm_codes) norm_codes[i] = (uint8_t)bj;
    if (dbnorms) dbnorms[i] = cb[bj];
  }
}

}  // namespace

template <class Code>
int aq_norms_launch(float *norms, const Code *codes, const float *C, int64_t n, int d, int m, int h, hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  // one wavefront per NR rows, in row slices of at most LAUNCH_MAX_THREADS threads (2^27 rows)
  const int64_t rows = LAUNCH_MAX_THREADS / 64 * NR;
  for (int64_t r0 = 0; r0 < n; r0 += rows) {
    const int64_t nr = std::min(rows, n - r0);
    const int64_t waves = (nr + NR - 1) / NR;
    hipLaunchKernelGGL(aq_norms_kernel<Code>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, norms + r0,
                       codes + (size_t)r0 * m, C, nr, d, m, h);
    RQ_HIP(hipGetLastError());
  }
  return RQ_OK;
}
template int aq_norms_launch(float *, const uint8_t *, const float *, int64_t, int, int, int, hipStream_t);
template int aq_norms_launch(float *, const int16_t *, const float *, int64_t, int, int, int, hipStream_t);

int quantize_norms_launch(int16_t *norm_codes, float *dbnorms, const float *norms, const float *cbnorms, int64_t n, int hn,
                          hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  const size_t lds = (size_t)hn * 4;         // hn <= RQ_MAX_H16: 128 KiB at most
  if (lds > 64 * 1024)
    RQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(quantize_norms_wide_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(quantize_norms_wide_kernel, dim3(grid), dim3(256), lds, stream, norm_codes, dbnorms, norms, cbnorms, n, hn);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

int quantize_norms_launch(uint8_t *norm_codes, float *dbnorms, const float *norms, const float *cbnorms, int64_t n, int hn,
                          hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(quantize_norms_kernel, dim3(grid), dim3(256), 0, stream, norm_codes, dbnorms, norms, cbnorms, n, hn);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

namespace {

// ---- what the entry points below take from the width of a code -------------------------------------------------------------------
// Bytes: 2 <= h <= 256, 1 <= hn <= 256, zero-based codes, their range checked where they arrive (on the host for host pointers,
// by dev_code_range for device pointers).  int16 (the *_wide entries): 2 <= h, 1 <= hn <= RQ_MAX_H16,
// codes made zero-based and checked against [0, h) on the device before any other work (check_codes_h16).
template <class Code> struct NormsWidth;
template <> struct NormsWidth<uint8_t> {
  static constexpr int MAX_H = 256;
  static constexpr bool HN_FIRST = false;
  static int host_range(const char *who, const uint8_t *codes, int64_t n, int m, int h) { return host_code_range(codes, n, m, h, who); }
  static int uploaded_range(const char *, uint8_t *, int64_t, int, int, int) { return RQ_OK; }
  static int dev_range(const char *who, const uint8_t *codes, int64_t n, int m, int h, hipStream_t s) {
    return dev_code_range(codes, n, m, h, s, who);
  }
  static int train(float *dC, uint8_t *dcodes, const float *dX, int64_t n, int hn, int niter, uint64_t seed) {
    return train_pq_resident(dC, dcodes, dX, n, 1, 1, hn, niter, seed);
  }
};
template <> struct NormsWidth<int16_t> {
  static constexpr int MAX_H = RQ_MAX_H16;
  static constexpr bool HN_FIRST = true;
  static int host_range(const char *, const int16_t *, int64_t, int, int) { return RQ_OK; }
  static int uploaded_range(const char *who, int16_t *dcodes, int64_t n, int m, int h, int code_base) {
    DevMem bad;
    RQ_TRY(bad.alloc(8));
    return check_codes_h16(who, dcodes, bad.as<unsigned long long>(), n, m, h, code_base, nullptr);
  }
  // every code in [0, h): one word, read back before any other work is queued (code_base 0: the codes are only read)
  static int dev_range(const char *who, const int16_t *codes, int64_t n, int m, int h, hipStream_t s) {
    if (((uintptr_t)codes & 1) != 0) return fail(RQ_EINVAL, "%s: codes must be 2-byte aligned", who);
    void *wf = nullptr;
    RQ_TRY(workspace(WS_TMP, 256, &wf, s));
    return check_codes_h16(who, const_cast<int16_t *>(codes), (unsigned long long *)wf, n, m, h, 0, s);
  }
  // the byte loop, widened, at hn <= 256 like rq_train_pq_wide
  static int train(float *dC, int16_t *dcodes, const float *dX, int64_t n, int hn, int niter, uint64_t seed) {
    return train_pq_resident_wide(dC, dcodes, dX, n, 1, 1, hn, niter, seed);
  }
};

template <class Code>
int norms_check_hn(const char *who, int hn) {
  constexpr int MAX_H = NormsWidth<Code>::MAX_H;
  if (hn < 1 || hn > MAX_H) return fail(RQ_EINVAL, "%s: hn=%d outside 1..%d", who, hn, MAX_H);
  return RQ_OK;
}

template <class Code>
int norms_check(const char *who, int64_t n, int d, int m, int h, int hn, int code_base) {
  constexpr int MAX_H = NormsWidth<Code>::MAX_H;
  if (m < 1 || m > 64) return fail(RQ_EINVAL, "%s: m=%d outside 1..64", who, m);
  if (h < 2 || h > MAX_H) return fail(RQ_EINVAL, "%s: h=%d outside 2..%d", who, h, MAX_H);
  if (NormsWidth<Code>::HN_FIRST) RQ_TRY(norms_check_hn<Code>(who, hn));   // the int16 entries name a bad hn before a bad d or n,
  if (d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);               // the byte entries after
  if (n < 0) return fail(RQ_EINVAL, "%s: n=%lld < 0", who, (long long)n);
  RQ_TRY(norms_check_hn<Code>(who, hn));
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  return RQ_OK;
}

// codes and codebooks of a host-pointer call on the device, and the norms computed from them
template <class Code>
struct NormsOnDevice {
  DevMem codes, C, norms;
  float *out() { return norms.as<float>(); }
  int run(const char *who, const Code *hcodes, const float *hC, int64_t n, int d, int m, int h, int code_base) {
    const size_t cb = (size_t)n * m * sizeof(Code);
    RQ_TRY(codes.alloc(cb)); RQ_TRY(C.alloc((size_t)m * h * d * 4)); RQ_TRY(norms.alloc((size_t)n * 4));
    RQ_HIP(hipMemcpy(codes.p, hcodes, cb, hipMemcpyHostToDevice));
    RQ_TRY(NormsWidth<Code>::uploaded_range(who, codes.as<Code>(), n, m, h, code_base));
    RQ_HIP(hipMemcpy(C.p, hC, (size_t)m * h * d * 4, hipMemcpyHostToDevice));
    return aq_norms_launch<Code>(norms.as<float>(), codes.as<Code>(), C.as<float>(), n, d, m, h, nullptr);
  }
};

// ---- the five entry points, once; `who` names the extern "C" function, the byte ones pass code_base = 0 ----------------------------
template <class Code>
int dev_aq_norms(const char *who, float *norms, const Code *codes, const float *C, int64_t n, int d, int m, int h, void *stream) {
  RQ_TRY(norms_check<Code>(who, n, d, m, h, 1, 0));
  if (n > 0 && (!norms || !codes || !C)) return fail(RQ_EINVAL, "%s: null pointer", who);
  if (n == 0) return RQ_OK;
  hipStream_t s = (hipStream_t)stream;
  RQ_TRY(NormsWidth<Code>::dev_range(who, codes, n, m, h, s));
  return aq_norms_launch<Code>(norms, codes, C, n, d, m, h, s);
}

template <class Code>
int host_aq_norms(const char *who, float *norms, const Code *codes, const float *C, int64_t n, int d, int m, int h, int code_base) {
  RQ_TRY(norms_check<Code>(who, n, d, m, h, 1, code_base));
  if (n > 0 && (!norms || !codes || !C)) return fail(RQ_EINVAL, "%s: null pointer", who);
  RQ_TRY(NormsWidth<Code>::host_range(who, codes, n, m, h));
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  NormsOnDevice<Code> dv;
  RQ_TRY(dv.run(who, codes, C, n, d, m, h, code_base));
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(norms, dv.norms.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

template <class Code>
int dev_quantize_norms(const char *who, Code *norm_codes, float *dbnorms_out, const float *norms, const float *cbnorms, int64_t n,
                       int hn, void *stream) {
  RQ_TRY(norms_check_hn<Code>(who, hn));
  if (n < 0) return fail(RQ_EINVAL, "%s: n=%lld < 0", who, (long long)n);
  if (!cbnorms || (n > 0 && (!norm_codes || !norms))) return fail(RQ_EINVAL, "%s: null pointer", who);
  return quantize_norms_launch(norm_codes, dbnorms_out, norms, cbnorms, n, hn, (hipStream_t)stream);
}

template <class Code>
int host_quantize_norms(const char *who, Code *norm_codes, float *norms_out, const Code *codes, const float *C, const float *cbnorms,
                        int64_t n, int d, int m, int h, int hn, int code_base) {
  RQ_TRY(norms_check<Code>(who, n, d, m, h, hn, code_base));
  if (!cbnorms || (n > 0 && (!norm_codes || !codes || !C))) return fail(RQ_EINVAL, "%s: null pointer", who);
  RQ_TRY(NormsWidth<Code>::host_range(who, codes, n, m, h));
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  NormsOnDevice<Code> dv;
  DevMem dcb, dnc;
  RQ_TRY(dcb.alloc((size_t)hn * 4)); RQ_TRY(dnc.alloc((size_t)n * sizeof(Code)));
  RQ_HIP(hipMemcpy(dcb.p, cbnorms, (size_t)hn * 4, hipMemcpyHostToDevice));
  RQ_TRY(dv.run(who, codes, C, n, d, m, h, code_base));
  RQ_TRY(quantize_norms_launch(dnc.as<Code>(), nullptr, dv.out(), dcb.as<float>(), n, hn, nullptr));
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(norm_codes, dnc.p, (size_t)n * sizeof(Code), hipMemcpyDeviceToHost));
  if (norms_out) RQ_HIP(hipMemcpy(norms_out, dv.norms.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

template <class Code>
int host_get_norms_codebook(const char *who, Code *norm_codes, float *cbnorms, float *norms_out, const Code *codes, const float *C,
                            int64_t n, int d, int m, int h, int hn, int niter, uint64_t seed, int code_base) {
  RQ_TRY(norms_check<Code>(who, n, d, m, h, hn, code_base));
  if (niter < 0) return fail(RQ_EINVAL, "%s: niter=%d < 0", who, niter);
  if (n < hn) return fail(RQ_EINVAL, "%s: fewer rows (%lld) than norm codebook entries (%d)", who, (long long)n, hn);
  if (!norm_codes || !cbnorms || !codes || !C) return fail(RQ_EINVAL, "%s: null pointer", who);
  RQ_TRY(NormsWidth<Code>::host_range(who, codes, n, m, h));
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  NormsOnDevice<Code> dv;
  DevMem dcb, dnc;
  RQ_TRY(dcb.alloc((size_t)hn * 4)); RQ_TRY(dnc.alloc((size_t)n * sizeof(Code)));
  RQ_TRY(dv.run(who, codes, C, n, d, m, h, code_base));
  RQ_HIP(hipDeviceSynchronize());
  RQ_TRY(NormsWidth<Code>::train(dcb.as<float>(), dnc.as<Code>(), dv.out(), n, hn, niter, seed));
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(cbnorms, dcb.p, (size_t)hn * 4, hipMemcpyDeviceToHost));
  RQ_HIP(hipMemcpy(norm_codes, dnc.p, (size_t)n * sizeof(Code), hipMemcpyDeviceToHost));
  if (norms_out) RQ_HIP(hipMemcpy(norms_out, dv.norms.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

}  // namespace

}  // namespace rq

using namespace rq;

extern "C" {

int rq_dev_aq_norms(float *norms, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h, void *stream) {
  return dev_aq_norms("rq_dev_aq_norms", norms, codes, C, n, d, m, h, stream);
}
int rq_aq_norms(float *norms, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h) {
  return host_aq_norms("rq_aq_norms", norms, codes, C, n, d, m, h, 0);
}
int rq_dev_quantize_norms(uint8_t *norm_codes, float *dbnorms_out, const float *norms, const float *cbnorms, int64_t n,
                          int hn, void *stream) {
  return dev_quantize_norms("rq_dev_quantize_norms", norm_codes, dbnorms_out, norms, cbnorms, n, hn, stream);
}
int rq_quantize_norms(uint8_t *norm_codes, float *norms_out, const uint8_t *codes, const float *C, const float *cbnorms,
                      int64_t n, int d, int m, int h, int hn) {
  return host_quantize_norms("rq_quantize_norms", norm_codes, norms_out, codes, C, cbnorms, n, d, m, h, hn, 0);
}
int rq_get_norms_codebook(uint8_t *norm_codes, float *cbnorms, float *norms_out, const uint8_t *codes, const float *C,
                          int64_t n, int d, int m, int h, int hn, int niter, uint64_t seed) {
  return host_get_norms_codebook("rq_get_norms_codebook", norm_codes, cbnorms, norms_out, codes, C, n, d, m, h, hn, niter, seed, 0);
}

// ---- the same five over int16 codes: 2 <= h <= RQ_MAX_H16, 1 <= hn <= RQ_MAX_H16 ---------------------
int rq_dev_aq_norms_wide(float *norms, const int16_t *codes, const float *C, int64_t n, int d, int m, int h, void *stream) {
  return dev_aq_norms("rq_dev_aq_norms_wide", norms, codes, C, n, d, m, h, stream);
}
int rq_aq_norms_wide(float *norms, const int16_t *codes, const float *C, int64_t n, int d, int m, int h, int code_base) {
  return host_aq_norms("rq_aq_norms_wide", norms, codes, C, n, d, m, h, code_base);
}
int rq_dev_quantize_norms_wide(int16_t *norm_codes, float *dbnorms_out, const float *norms, const float *cbnorms, int64_t n,
                               int hn, void *stream) {
  return dev_quantize_norms("rq_dev_quantize_norms_wide", norm_codes, dbnorms_out, norms, cbnorms, n, hn, stream);
}
int rq_quantize_norms_wide(int16_t *norm_codes, float *norms_out, const int16_t *codes, const float *C, const float *cbnorms,
                           int64_t n, int d, int m, int h, int hn, int code_base) {
  return host_quantize_norms("rq_quantize_norms_wide", norm_codes, norms_out, codes, C, cbnorms, n, d, m, h, hn, code_base);
}
int rq_get_norms_codebook_wide(int16_t *norm_codes, float *cbnorms, float *norms_out, const int16_t *codes, const float *C,
                               int64_t n, int d, int m, int h, int hn, int niter, uint64_t seed, int code_base) {
  return host_get_norms_codebook("rq_get_norms_codebook_wide", norm_codes, cbnorms, norms_out, codes, C, n, d, m, h, hn, niter, seed,
                                 code_base);
}

}  // extern "C"

