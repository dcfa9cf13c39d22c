// rq_scan_tables.h -- f32 look-up tables, the exact row evaluation and the survivors' append of the ADC scan kernel
// Device code only, part of the kernel: included by rq_scan.hip alone (through rq_scan_filter.h and rq_scan_select.h too).
// The tiling constants and the kernel's parameter block are in rq_scan_cfg.h.
#pragma once
#include "rq_internal.h"
#include "rq_topk.h"
#include "rq_scan_cfg.h"

namespace rq {

// v_writelane_b32 (no clang builtin in ROCm 7.2): lane `L` of `old` <- wave-uniform `val`
template <class T>
__device__ __forceinline__ uint32_t writelane_u32(uint32_t old, T val, int L) {
  asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(val), "n"(L));
  return old;
}

// LUT entry of QPG queries
template <int QPG> struct LutVec;
template <> struct LutVec<4> {
  using type = float4;
  static __device__ __forceinline__ type make(const float *a) { return make_float4(a[0], a[1], a[2], a[3]); }
  static __device__ __forceinline__ float get(const type &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
};
template <> struct LutVec<2> {
  using type = float2;
  static __device__ __forceinline__ type make(const float *a) { return make_float2(a[0], a[1]); }
  static __device__ __forceinline__ float get(const type &v, int i) { return i == 0 ? v.x : v.y; }
};

constexpr uint32_t FILT_MAX_SHARE_PCT = 60;   // first block: share of rows the pre-filter may let through before it is switched off

// ------------------------------------------------------------------------------------------
// LUT construction, one (k, r) entry at a time for all QG queries of the group; compiled with
// -ffp-contract=off so every product, square and add stays a separately rounded f32 operation
// like the reference's x86-64 builds.
//   mode 0  deps/src/linscan_aqd.cpp:66-74                 T = sum_s (c[s] - q[k*sub+s])^2, s < sub
//   mode 1  deps/src/linscan_aqd_pairwise_byte.cpp:42-49   T = T - (2*q[s])*c[s],            s < d
//   mode 2  deps/src/linscan_aqd_pairwise_byte.cpp:126-133 T = T + (q[s]-c[s])^2,            s < d
// ------------------------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ void build_lut(float *lut, float4 *gtab, const float *qstage,
                                          const float *centers, int sub, int d, int mode, int m_real, int tid) {
  using Cfg = ScanCfg<M>;
  constexpr int QG = Cfg::QG, NQUAD = Cfg::NQUAD;
  const int cdim = mode == 0 ? sub : d;
  for (int e = tid; e < M * 256; e += ScanCfg<M>::THREADS) {
    const int k = e >> 8, r = e & 255;
    const float *c = centers + (size_t)e * cdim;
    const int qoff = mode == 0 ? k * sub : 0;
    float acc[QG];
#pragma unroll
    for (int q = 0; q < QG; ++q) acc[q] = 0.0f;
    if (k >= m_real) {
      // padding sub-quantizer (m rounded up to a supported tile width): T = 0, and x + 0.0f == x
    } else {
      // one table entry per thread, its codebook row streamed 16 bytes at a time (full-dimensional rows
      // are 512 B apart between lanes: scalar loads would touch 64 cache lines per instruction, 4x as often)
      auto step = [&](float cs, int s) {
        if (mode == 1) {
#pragma unroll
          for (int q = 0; q < QG; ++q) {
            const float two_q = 2.0f * qstage[q * d + s];
            const float prod = two_q * cs;
            acc[q] = acc[q] - prod;
          }
        } else {
#pragma unroll
          for (int q = 0; q < QG; ++q) {
            const float diff = cs - qstage[q * d + qoff + s];   // (q-c)^2 has the same bits
            const float sq = diff * diff;
            acc[q] = acc[q] + sq;
          }
        }
      };
      if ((cdim & 3) == 0 && ((uintptr_t)centers & 15) == 0) {
        const float4 *c4 = reinterpret_cast<const float4 *>(c);
#pragma unroll 2
        for (int s4 = 0; s4 < cdim / 4; ++s4) {
          const float4 cv = c4[s4];
          step(cv.x, 4 * s4 + 0);
          step(cv.y, 4 * s4 + 1);
          step(cv.z, 4 * s4 + 2);
          step(cv.w, 4 * s4 + 3);
        }
      } else {
        for (int s = 0; s < cdim; ++s) step(c[s], s);
      }
    }
    using LV = LutVec<Cfg::QPG>;
    using Vec = typename LV::type;
#pragma unroll
    for (int quad = 0; quad < NQUAD; ++quad) {
      const Vec v = LV::make(&acc[quad * Cfg::QPG]);
      if (k < Cfg::KL) reinterpret_cast<Vec *>(lut)[(k * NQUAD + quad) * 256 + r] = v;
      else reinterpret_cast<Vec *>(gtab)[((k - Cfg::KL) * NQUAD + quad) * 256 + r] = v;
    }
  }
}

// ADC distances of row r of the packed byte string w for the QG queries of the group:
// acc_q = ((T_q[0][b0] + T_q[1][b1]) + ...)  -- deps/src/linscan_aqd.cpp:85-87, sequential f32.
template <int M>
__device__ __forceinline__ void row_dists(const uint32_t *w, int r, const float4 *lut4,
                                          const float4 *__restrict__ gtab4, float (&acc)[ScanCfg<M>::QG]) {
  using Cfg = ScanCfg<M>;
  using LV = LutVec<Cfg::QPG>;
  using Vec = typename LV::type;
  constexpr int NQUAD = Cfg::NQUAD, KL = Cfg::KL, QPG = Cfg::QPG;
  const Vec *lutv = reinterpret_cast<const Vec *>(lut4);
  const Vec *__restrict__ gtab = reinterpret_cast<const Vec *>(gtab4);
  // issue the L1 gathers of the last sub-quantizers first: their latency hides under the LDS ones
  Vec tg[(Cfg::KG > 0 ? Cfg::KG : 1) * NQUAD];
  auto load_tg = [&]() {
#pragma unroll
    for (int k = KL; k < M; ++k) {
      const uint32_t byte = (w[(r * M + k) >> 2] >> (8 * ((r * M + k) & 3))) & 0xffu;
#pragma unroll
      for (int quad = 0; quad < NQUAD; ++quad) tg[(k - KL) * NQUAD + quad] = gtab[((k - KL) * NQUAD + quad) * 256 + byte];
    }
  };
  constexpr bool WIDE = M * NQUAD >= 32;     // a row of 32 gathers is summed in two halves (see below)
  if constexpr (!WIDE) load_tg();
#pragma unroll
  for (int k = 0; k < M; ++k) {
    // at most 16 gathers (64 registers of table entries) in flight: a row of 32 (m = 16, 8 queries) is summed in two
    // halves -- the scheduler otherwise hoists all 32 and spills their results (LSQ variant: 160 spilled registers)
    if constexpr (WIDE) {
      if (k * NQUAD == 16) {
        __builtin_amdgcn_sched_barrier(0);
        load_tg();                             // the L1 part belongs to the second half (KL >= M / 2)
      }
    }
    const uint32_t byte = (w[(r * M + k) >> 2] >> (8 * ((r * M + k) & 3))) & 0xffu;
#pragma unroll
    for (int quad = 0; quad < NQUAD; ++quad) {
      const Vec t = k < KL ? lutv[(k * NQUAD + quad) * 256 + byte] : tg[(k - KL) * NQUAD + quad];
#pragma unroll
      for (int c = 0; c < QPG; ++c) {
        if (k == 0) acc[quad * QPG + c] = LV::get(t, c);
        else acc[quad * QPG + c] = acc[quad * QPG + c] + LV::get(t, c);
      }
    }
  }
}

// one row's M code bytes into w[0 .. M/4) (packed like the hot loop's byte string, r = 0)
template <int M>
__device__ __forceinline__ void load_row(uint32_t *w, const uint8_t *codes, uint32_t row) {
  if constexpr (M % 4 == 0) {
#pragma unroll
    for (int i = 0; i < M / 4; ++i) w[i] = reinterpret_cast<const uint32_t *>(codes + (size_t)row * M)[i];
  } else {
#pragma unroll
    for (int i = 0; i < (M + 3) / 4; ++i) w[i] = 0;
#pragma unroll
    for (int k = 0; k < M; ++k) w[k >> 2] |= (uint32_t)codes[(size_t)row * M + k] << (8 * (k & 3));
  }
}

// ------------------------------------------------------------------------------------------
// Survivors of one wave-row-step: lane `lane` holds the exact distances acc[q] of ONE row (key id `kid`) to the
// QG queries; rows with acc[q] <= tau[q] are appended to query q's candidate buffer (INCLUSIVE: tau is a sampled
// distance, and on heavily duplicated codes hundreds of rows share the K-th neighbour's distance exactly -- with a strict
// test they all drop out and the slice has to be redone exactly; 3 % of the groups on 1024-cluster data).  ONE LDS atomic for all QG
// queries: lane q reserves popc(mk[q]) slots of query q.
// ------------------------------------------------------------------------------------------
template <int QG>
__device__ __forceinline__ void emit_survivors(const float (&acc)[QG], const float (&tau)[QG], bool valid, uint32_t row,
                                               const uint32_t *__restrict__ perm, uint32_t id_offset,
                                               uint32_t selmask, ScanCtrl<QG> *ctrl, uint64_t *cand_wg, uint32_t cap,
                                               int lane) {
  uint64_t mk[QG];
  uint64_t any = 0;
#pragma unroll
  for (int q = 0; q < QG; ++q) {
    mk[q] = __ballot(valid && (acc[q] <= tau[q]));
    any |= mk[q];
  }
  if (any) {
    // the key's id: the row's ORIGINAL number (ordered bases: one load per surviving row, never in the common path)
    uint32_t kid = row;
    if (perm && ((any >> lane) & 1ull)) kid = perm[row];
    kid += id_offset;
    uint32_t want = 0;
#pragma unroll
    for (int q = 0; q < QG; ++q)
      want = writelane_u32(want, (uint32_t)__popcll(mk[q]), q);
    uint32_t got = 0;
    if (lane < QG && want) got = atomicAdd(&ctrl->cnt[lane], want);
#pragma unroll
    for (int q = 0; q < QG; ++q) {
      if (mk[q]) {
        const uint32_t basep = __builtin_amdgcn_readlane(got, q);
        if ((mk[q] >> lane) & 1ull) {
          const uint32_t pos = basep + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk[q] >> 32),
                                        __builtin_amdgcn_mbcnt_lo((uint32_t)mk[q], 0u));
          uint64_t *buf = cand_wg + ((size_t)q * 2 + ((selmask >> q) & 1u)) * cap;
          buf[pos] = make_key(acc[q], kid);
        }
      }
    }
  }
}

}  // namespace rq
