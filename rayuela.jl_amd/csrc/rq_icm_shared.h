// rq_icm_shared.h -- what the two LSQ encoders (rq_icm.hip: byte codes, h <= 256; rq_icm_h16.hip: 16-bit codes) share: the limits,
// the counter-based random stream and veccost.  Contract in DESIGN.md section 2.
#pragma once
#include "rq_internal.h"

namespace rq {

constexpr int ICM_MAX_M = 16;                                    // the reference GPU kernel's local_codes[16]
constexpr size_t ICM_SCRATCH_BYTES = (size_t)2 << 30;           // binaries + unaries of one chunk, per device and stream

__host__ __device__ __forceinline__ uint64_t icm_z(uint64_t x) {   // splitmix64 (synth.splitmix64)
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ((w >> 32) * range) >> 32: an integer in [0, range)
__device__ __forceinline__ uint32_t icm_scale(uint64_t w, uint32_t range) {
  return (uint32_t)(((w >> 32) * (uint64_t)range) >> 32);
}

// veccost (src/qerrors.jl:36-66): CB = sum_i C_i[b_i] (f32 adds from +0 in codebook order), then lane l sums (CB - x)^2
// over dims l, l+64, ... in order from +0, and a fixed xor butterfly (32, 16, 8, 4, 2, 1) adds the 64 partial sums.
template <int MB>
__device__ __forceinline__ float icm_cost(const int (&b)[MB], const float *x, const float *C, int d, int m, int h,
                                          int lane) {
  float acc = 0.0f;
  for (int t = lane; t < d; t += 64) {
    float cb = 0.0f;
#pragma unroll
    for (int i = 0; i < MB; ++i)
      if (i < m) cb = cb + C[((size_t)i * h + b[i]) * d + t];
    const float df = cb - x[t];
    acc = acc + df * df;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
  return acc;
}

// rq_last_icm_timing's two numbers for the calling thread (rq_icm.hip)
void icm_set_timing(double unary_ms, double total_ms);

}  // namespace rq
