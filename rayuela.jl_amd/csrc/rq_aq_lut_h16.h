// rq_aq_lut_h16.h -- the full-dimensional tables of the additive-quantizer scan over 16-bit codes:
// deps/src/linscan_aqd_pairwise_byte.cpp:42-49 (LSQ) and :124-131 (CQ) with h entries per codebook, every operation rounded on
// its own (-ffp-contract=off), the k loop strictly sequential per (entry, query):
//   LUT_LSQ  T[e] = T[e] - (2 q[k]) * c[e][k]           LUT_CQ  T[e] = T[e] + (q[k] - c[e][k]) * (q[k] - c[e][k])
// into the layout adc_keys_h16_kernel reads: tab[group][e][QPG], e = k h + r, `gstride` floats per group of QPG queries.
#pragma once
#include "rq_internal.h"

namespace rq {

template <int QPG> struct H16Vec;
template <> struct H16Vec<4> {
  using type = float4;
  static __device__ __forceinline__ type make(const float *a) { return make_float4(a[0], a[1], a[2], a[3]); }
  static __device__ __forceinline__ float get(const type &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
};
template <> struct H16Vec<2> {
  using type = float2;
  static __device__ __forceinline__ type make(const float *a) { return make_float2(a[0], a[1]); }
  static __device__ __forceinline__ float get(const type &v, int i) { return i == 0 ? v.x : v.y; }
};
template <> struct H16Vec<1> {
  using type = float;
  static __device__ __forceinline__ type make(const float *a) { return a[0]; }
  static __device__ __forceinline__ float get(const type &v, int) { return v; }
};

constexpr int AQ_LUT_THREADS = 256;   // entries per workgroup, one per thread
constexpr int AQ_LUT_TQ = 16;         // queries per workgroup: each codebook row is read once for all of them
constexpr int AQ_LUT_DK = 128;        // coordinates of the query tile staged in LDS at a time (8 KiB)

// one coordinate of one (entry, query): q is 2 q[k] for LUT_LSQ; the product and the sum are rounded apart
template <int MODE>
__device__ __forceinline__ float aq_term(float acc, float q, float c) {
  if (MODE == LUT_LSQ) {
    const float p = q * c;
    return acc - p;
  }
  const float diff = q - c;
  const float sq = diff * diff;
  return acc + sq;
}

// blockIdx.x: a block of AQ_LUT_THREADS entries, blockIdx.y: a tile of AQ_LUT_TQ queries (tile0 + blockIdx.y).  The tile's
// queries sit in LDS (2 q for LUT_LSQ), DK coordinates at a time; every lane reads the same LDS address (a broadcast, no bank
// conflict), 16 bytes per read on the vec4 path, while its own codebook row streams from global memory 16 bytes at a time.
// A query past nq repeats query nq - 1; a group past `ngroups` is not stored.  vec4: d % 4 == 0 and codebooks 16-byte aligned.
template <int QPG, int MODE>
__global__ __launch_bounds__(AQ_LUT_THREADS) void aq_lut_h16_kernel(float *tab, const float *codebooks, const float *queries,
                                                                    uint32_t nq, uint32_t ngroups, uint32_t tile0, uint32_t E,
                                                                    int d, size_t gstride, int vec4) {
  using V = H16Vec<QPG>;
  constexpr int TQ = AQ_LUT_TQ, DK = AQ_LUT_DK;
  __shared__ __attribute__((aligned(16))) float qs[TQ * DK];
  const uint32_t tid = threadIdx.x;
  const uint32_t e = blockIdx.x * AQ_LUT_THREADS + tid;
  const uint32_t q0 = (tile0 + blockIdx.y) * TQ;
  const float *c = codebooks + (size_t)min(e, E - 1u) * (size_t)d;     // a thread past E reads row E - 1 and stores nothing
  float acc[TQ];
#pragma unroll
  for (int t = 0; t < TQ; ++t) acc[t] = 0.0f;
  for (int k0 = 0; k0 < d; k0 += DK) {
    const int kc = min(DK, d - k0);
    __syncthreads();                                 // the previous chunk has been read
    for (int i = (int)tid; i < TQ * kc; i += AQ_LUT_THREADS) {
      const int t = i / kc, kk = i - t * kc;
      const uint32_t qq = min(q0 + (uint32_t)t, nq - 1u);
      const float qv = queries[(size_t)qq * (size_t)d + (size_t)(k0 + kk)];
      qs[t * DK + kk] = MODE == LUT_LSQ ? 2.0f * qv : qv;
    }
    __syncthreads();
    if (vec4) {
      const float4 *c4 = reinterpret_cast<const float4 *>(c + k0);
#pragma unroll 2
      for (int kk = 0; kk < kc; kk += 4) {
        const float4 cv = c4[kk >> 2];
        // coordinate by coordinate: the order of the sums per (entry, query) is k = 0, 1, 2, ...
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
          const float4 qv = *reinterpret_cast<const float4 *>(&qs[t * DK + kk]);
          acc[t] = aq_term<MODE>(acc[t], qv.x, cv.x);
          acc[t] = aq_term<MODE>(acc[t], qv.y, cv.y);
          acc[t] = aq_term<MODE>(acc[t], qv.z, cv.z);
          acc[t] = aq_term<MODE>(acc[t], qv.w, cv.w);
        }
      }
    } else {
      for (int kk = 0; kk < kc; ++kk) {
        const float cv = c[k0 + kk];
#pragma unroll
        for (int t = 0; t < TQ; ++t) acc[t] = aq_term<MODE>(acc[t], qs[t * DK + kk], cv);
      }
    }
  }
  if (e >= E) return;
#pragma unroll
  for (int g = 0; g < TQ / QPG; ++g) {
    const uint32_t grp = q0 / QPG + (uint32_t)g;
    if (grp < ngroups) reinterpret_cast<typename V::type *>(tab + (size_t)grp * gstride)[e] = V::make(&acc[g * QPG]);
  }
}

}  // namespace rq
