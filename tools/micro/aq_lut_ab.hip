// aq_lut_ab.hip -- A/B of the table kernel of the additive-quantizer scan over 16-bit codes:
//   A  "port"   the obvious port: adc_lut_h16_kernel's shape with sub := d -- one thread per (query group, entry), each streaming
//               its own codebook row, so the codebooks are read once per query group
//   B  "tiled"  aq_lut_h16_kernel of csrc/rq_aq_lut_h16.h (what the library ships): one entry per thread, 16 queries per workgroup
// both writing tab[group][e][QPG] for one batch of queries, LSQ tables, interleaved in one process, device events around each
// launch, median / min / max of --reps repetitions; the two tables are compared bit for bit first.  One JSON line per shape.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I rayuela.jl_amd/csrc -I include tools/micro/aq_lut_ab.hip -o aq_lut_ab
//   ./aq_lut_ab [reps = 7] [queries per batch = 212]
#include "rq_aq_lut_h16.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace rq;

#define CK(x)                                                                              \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));    \
      exit(1);                                                                             \
    }                                                                                      \
  } while (0)

template <int QPG>
__global__ __launch_bounds__(256) void aq_lut_port_kernel(float *lut, const float *codebooks, const float *queries, uint32_t nq,
                                                          uint32_t ngroups, size_t E, int d, size_t gstride, int vec4) {
  using V = H16Vec<QPG>;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)ngroups * E) return;
  const uint32_t g = (uint32_t)(t / E);
  const size_t e = t - (size_t)g * E;
  const float *c = codebooks + e * (size_t)d;
  const float *qv[QPG];
  float acc[QPG];
#pragma unroll
  for (int j = 0; j < QPG; ++j) {
    qv[j] = queries + (size_t)min(g * (uint32_t)QPG + (uint32_t)j, nq - 1u) * d;
    acc[j] = 0.0f;
  }
  auto step = [&](float cs, int s) {
#pragma unroll
    for (int j = 0; j < QPG; ++j) acc[j] = aq_term<LUT_LSQ>(acc[j], 2.0f * qv[j][s], cs);
  };
  if (vec4) {
    const float4 *c4 = reinterpret_cast<const float4 *>(c);
    for (int s = 0; s < d; s += 4) {
      const float4 cv = c4[s >> 2];
      step(cv.x, s); step(cv.y, s + 1); step(cv.z, s + 2); step(cv.w, s + 3);
    }
  } else {
    for (int s = 0; s < d; ++s) step(c[s], s);
  }
  reinterpret_cast<typename V::type *>(lut + (size_t)g * gstride)[e] = V::make(acc);
}

struct Stat { float med, mn, mx; };
static Stat stat(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return {v[v.size() / 2], v.front(), v.back()};
}

template <int QPG>
static void run(int m, int h, int d, int nb, int reps) {
  const size_t E = (size_t)m * h, gstride = (E * QPG + 3) & ~(size_t)3;
  const uint32_t ngroups = (uint32_t)((nb + QPG - 1) / QPG);
  std::vector<float> hc(E * d), hq((size_t)nb * d);
  uint64_t s = 88172645463325252ull ^ (uint64_t)(E * 131 + d);
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0); };
  for (auto &x : hc) x = rnd();
  for (auto &x : hq) x = rnd();
  float *dc, *dq, *ta, *tb;
  const size_t tbytes = (size_t)ngroups * gstride * 4;
  CK(hipMalloc(&dc, hc.size() * 4)); CK(hipMalloc(&dq, hq.size() * 4)); CK(hipMalloc(&ta, tbytes)); CK(hipMalloc(&tb, tbytes));
  CK(hipMemcpy(dc, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dq, hq.data(), hq.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(ta, 0, tbytes)); CK(hipMemset(tb, 0xFF, tbytes));
  const int vec4 = (d & 3) == 0;
  const size_t pthreads = (size_t)ngroups * E;
  const uint32_t tiles = (uint32_t)((nb + AQ_LUT_TQ - 1) / AQ_LUT_TQ), ex = (uint32_t)((E + AQ_LUT_THREADS - 1) / AQ_LUT_THREADS);
  auto port = [&]() {
    hipLaunchKernelGGL(aq_lut_port_kernel<QPG>, dim3((uint32_t)((pthreads + 255) / 256)), dim3(256), 0, nullptr, ta, dc, dq,
                       (uint32_t)nb, ngroups, E, d, gstride, vec4);
  };
  auto tiled = [&]() {
    hipLaunchKernelGGL((aq_lut_h16_kernel<QPG, LUT_LSQ>), dim3(ex, tiles), dim3(AQ_LUT_THREADS), 0, nullptr, tb, dc, dq, (uint32_t)nb,
                       ngroups, 0u, (uint32_t)E, d, gstride, vec4);
  };
  port(); tiled();
  CK(hipDeviceSynchronize());
  std::vector<float> ha(tbytes / 4), hb(tbytes / 4);
  CK(hipMemcpy(ha.data(), ta, tbytes, hipMemcpyDeviceToHost));
  CK(hipMemcpy(hb.data(), tb, tbytes, hipMemcpyDeviceToHost));
  size_t diff = 0;      // whole groups only: the padding lanes of a ragged last group hold the last query in both
  for (size_t g = 0; g < ngroups; ++g) diff += memcmp(&ha[g * gstride], &hb[g * gstride], E * QPG * 4) != 0;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::vector<float> tp, tt;
  for (int r = 0; r < reps; ++r) {
    float ms;
    CK(hipEventRecord(e0)); port(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
    tp.push_back(ms);
    CK(hipEventRecord(e0)); tiled(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
    tt.push_back(ms);
  }
  const Stat a = stat(tp), b = stat(tt);
  const double ops = 2.0 * nb * (double)E * d;
  printf("{\"m\": %d, \"h\": %d, \"d\": %d, \"queries\": %d, \"qpg\": %d, \"groups_differing\": %zu, "
         "\"port_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, \"tiled_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, "
         "\"port_over_tiled\": %.3f, \"tiled_valu_tops\": %.3f}\n",
         m, h, d, nb, QPG, diff, a.med, a.mn, a.mx, b.med, b.mn, b.mx, a.med / b.med, ops / (b.med * 1e-3) / 1e12);
  fflush(stdout);
  CK(hipFree(dc)); CK(hipFree(dq)); CK(hipFree(ta)); CK(hipFree(tb));
}

int main(int argc, char **argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 7, nb = argc > 2 ? atoi(argv[2]) : 212;
  // the shapes of tools/aq_wide_perf.py with the queries per gather h16_plan gives them
  run<4>(8, 256, 128, nb, reps);
  run<4>(8, 1024, 128, nb, reps);
  run<1>(8, 4096, 128, nb, reps);
  run<4>(4, 16384, 128, nb, reps);
  run<2>(16, 1024, 96, nb, reps);
  return 0;
}
