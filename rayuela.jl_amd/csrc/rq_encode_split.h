// rq_encode_split.h -- pieces shared by the bf16 matrix-core filter kernels of the PQ encode (rq_encode.hip: the one-pass
// kernel with the exact re-evaluation inside; rq_encode_filter.hip: filter + separate exact pass).
#pragma once
#include "rq_internal.h"

namespace rq {

using f32x16 = float __attribute__((ext_vector_type(16)));
using f32x2 = float __attribute__((ext_vector_type(2)));

struct EncParams {
  const float *X;   // [n][d]
  const float *C;   // concat of [h][sub_i]
  uint8_t *codes;   // [n][m]
  int64_t n;
  int d, m, h, NT;
  int i0, i1;       // sub-quantizers handled by this launch (codebooks of [i0,i1) sit in LDS)
  int off[33];      // splitarray offsets (src/utils.jl:179-203)
  float delta_rel;  // split kernel: candidate margin relative to max|c|^2 + |x|^2 (SplitCfg::DELTA_REL unless tuned, tests)
  float *dbg_w;     // split kernel, tests only: [n][m][h] receives the filter's W values (nullptr in every product call)
  uint32_t *flags;  // filter + exact pass: [n] words, bit (i - i0) set = (row, sub-quantizer i) goes to the exact pass
  unsigned char *image;  // filter + exact pass: the launch's LDS table image (encode_tables_kernel, rq_encode_filter.hip)
  int fix_rows;          // exact pass: rows per workgroup (its per-sub-quantizer LDS lists hold 2 bytes per row)
  unsigned long long *stat;  // tuning ENC_STATS only: [0] += flagged (row, sub-quantizer) pairs (exact pass); nullptr otherwise
};

// lanes 32-63 of a  <->  lanes 0-31 of b   (v_permlane32_swap_b32)
__device__ __forceinline__ void swap32(float &a, float &b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// bf16 round-to-nearest-even of a finite f32 (inf stays inf); returns the 16 payload bits
__device__ __forceinline__ uint32_t bf16_bits(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_val(uint32_t b) { return __uint_as_float(b << 16); }

#ifndef RQ_SPLIT_SINGLE_ACC
#define RQ_SPLIT_SINGLE_ACC 0
#endif
struct SplitCfg {
  static constexpr float DELTA_REL = 3.0f * 6.103515625e-05f;     // 3 * 2^-14
  static constexpr float TINY = 8.673617379884035e-19f;            // 2^-60: below it bf16 flush-to-zero could matter
};

template <int SUB>
struct SplitShape {
  static_assert(SUB >= 2 && SUB <= 16 && SUB % 2 == 0, "split encode: even sub-space widths up to 16");
  static constexpr bool PACK = SUB <= 8;          // hi and lo pieces of -2c share one K = 16 fragment
  static constexpr int NPIECE = PACK ? 1 : 2;     // 16-byte A fragments per (tile, lane)
};

// canonical evaluation of centroid k of sub-quantizer `cb` (oracle/rq_oracle.c:264-328): g = fmaf chain s = 0..sub-1 from
// +0, sa = |c_k|^2 (the same chain, computed once in the prologue: sa_k), v = max(fl(fl(sa + sb) - 2g), 0); then the
// lexicographic (v, index) update.
template <int SUB>
__device__ __forceinline__ void split_exact(const float *__restrict__ cb, int k, const float (&x)[SUB], float sb, float sa,
                                            float &bv, int &bk) {
  float c[SUB];
  if constexpr (SUB % 4 == 0) {
    const float4 *c4 = reinterpret_cast<const float4 *>(cb + (size_t)k * SUB);
#pragma unroll
    for (int s4 = 0; s4 < SUB / 4; ++s4) { const float4 v = c4[s4]; c[4 * s4] = v.x; c[4 * s4 + 1] = v.y; c[4 * s4 + 2] = v.z; c[4 * s4 + 3] = v.w; }
  } else {
    const f32x2 *c2 = reinterpret_cast<const f32x2 *>(cb + (size_t)k * SUB);
#pragma unroll
    for (int s2 = 0; s2 < SUB / 2; ++s2) { const f32x2 v = c2[s2]; c[2 * s2] = v.x; c[2 * s2 + 1] = v.y; }
  }
  float g = 0.0f;
#pragma unroll
  for (int sx = 0; sx < SUB; ++sx) g = __builtin_fmaf(c[sx], x[sx], g);
  const float t = sa + sb;
  const float u = __builtin_fmaf(-2.0f, g, t);
  const float v = __builtin_fmaxf(u, 0.0f);
  if (v < bv || (v == bv && k < bk)) { bv = v; bk = k; }
}

// bit r of the result: v[r] <= thr  (v_cmp + v_addc per value: the carry shifts into the mask).  Only for values that
// were produced by ordinary VALU instructions (see the note at the tile re-run below).
__device__ __forceinline__ uint32_t mask_leq16(const f32x16 &v, float thr) {
  uint32_t cm = 0;
#pragma unroll
  for (int r = 15; r >= 0; --r)
    asm("v_cmp_le_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(cm) : "v"(v[r]), "v"(thr) : "vcc");
  return cm;
}


// ---- canonical evaluation on the f32 matrix cores (direct kernels of rq_encode.hip, exact pass of rq_encode_filter.hip) ----
// One 32-centroid x 32-vector tile of inner products: KS chained 32x32x2 MFMAs (= the fmaf chain
// s = 0..2KS-1 of the oracle; padded k-steps multiply 0 by 0 and leave the chain untouched).
template <int KS>
__device__ __forceinline__ f32x16 tile_dots(const float *cb_tile, const float (&b)[KS]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int kk = 0; kk < KS; ++kk)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cb_tile[kk * 64], b[kk], acc, 0, 0, 0);
  return acc;
}

// Epilogue of one tile on the lane's 16 accumulator registers (16 centroids of ONE vector):
//   u_r = fl(fl(sa_r + sb) - 2 g_r)           (fma(-2, g, t) has the same bits: 2g is exact)
//   the tile's clamped minimum is cm = max(min_r u_r, 0).
// f32 MFMA and f32 VALU share the SIMD's FP32 lanes on gfx950 (measured: busy cycles add up, they
// do not overlap), so every VALU instruction here is paid in full.  Per tile we therefore only
// keep the running best value and, for the lanes that improved (strict '<': the earliest tile wins
// ties), a copy of the tile's 16 u values (one shared mask, 16 v_cndmask).  The first-index search
// runs ONCE per sub-quantizer on that copy (argmin_finish) instead of once per tile.

struct ArgminState {
  float best_v;   // clamped minimum so far
  int best_t;     // tile that holds it
  f32x2 ub[8];    // that tile's 16 u values (register pairs, as the packed ops leave them)
};

__device__ __forceinline__ void tile_argmin(const f32x16 &acc, const float4 *sa4, float sb, int t,
                                            ArgminState &st) {
  // packed f32 arithmetic (v_pk_add_f32 / v_pk_fma_f32): two elements per VALU issue
  f32x2 u[8];
  sa4 = reinterpret_cast<const float4 *>(__builtin_assume_aligned(sa4, 16));
  const f32x2 sb2 = {sb, sb};
  const f32x2 m2 = {-2.0f, -2.0f};
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const float4 sav = sa4[g4];
    const f32x2 s01 = {sav.x, sav.y}, s23 = {sav.z, sav.w};
    const f32x2 g01 = {acc[g4 * 4 + 0], acc[g4 * 4 + 1]}, g23 = {acc[g4 * 4 + 2], acc[g4 * 4 + 3]};
    u[g4 * 2 + 0] = __builtin_elementwise_fma(m2, g01, s01 + sb2);
    u[g4 * 2 + 1] = __builtin_elementwise_fma(m2, g23, s23 + sb2);
  }
  float m01 = __builtin_fminf(__builtin_fminf(u[0].x, u[0].y), u[1].x);
  float m02 = __builtin_fminf(__builtin_fminf(u[1].y, u[2].x), u[2].y);
  float m03 = __builtin_fminf(__builtin_fminf(u[3].x, u[3].y), u[4].x);
  float m04 = __builtin_fminf(__builtin_fminf(u[4].y, u[5].x), u[5].y);
  float m05 = __builtin_fminf(__builtin_fminf(u[6].x, u[6].y), u[7].x);
  float mm = __builtin_fminf(__builtin_fminf(m01, m02), m03);
  mm = __builtin_fminf(__builtin_fminf(mm, m04), m05);
  mm = __builtin_fminf(mm, u[7].y);
  const float cm = __builtin_fmaxf(mm, 0.0f);
  // a real (exec-masked) branch: f32 MFMA and VALU do not overlap on this chip, so there is nothing to
  // interleave the copy with, and under the mask it is 8 64-bit moves instead of 16 selects
  if (cm < st.best_v) {
    st.best_v = cm;
    st.best_t = t;
#pragma unroll
    for (int r = 0; r < 8; ++r) st.ub[r] = u[r];
  }
}

// First index of the clamped minimum inside the winning tile: the first r with u_r <= cm (for
// cm > 0 that is the first minimum; for cm == 0 the first value the reference's max(.,0) clamps).
//
// Non-finite inputs (include/rayuela_hip.h, "Non-finite inputs"; tests/test_gpu_nonfinite_encode.py).  best_v is never NaN
// (fmaxf(NaN, 0) = 0).  A lane's search finds nothing in exactly one case: the 16 u values of its winning tile are ALL NaN
// (fminf skips NaN operands, so a tile with one ordered value has its minimum among them; and a lane that never took a tile
// keeps best_v = +Inf over ub = 0, which finds r = 0).  All NaN means a NaN coordinate, or an Inf one against this lane's
// centroids: mm = NaN, cm = 0 < +Inf, the tile is taken.  The oracle's fmaxf clamps every such distance to 0 and answers with
// the first centroid, so the lane answers 0 -- the sub-quantizer's index 0, not a position inside the tile, which at h < 28
// (27 + 4 hi) or in a tile of zero-padded centroids (k >= h: +Inf norm, 0 * Inf = NaN under an Inf row) lies past h.
// An index that IS found is below h: a padded centroid's u is +Inf (finite row) or NaN, and neither is <= a best_v below +Inf.
// The half-wave merge of the callers keeps the smaller (value, index) pair: an unfound lane carries (0, 0), which no pair
// precedes, and a lane that never took a tile carries (+Inf, 4 hi), which the other half's (<= +Inf, 0 or a found index)
// precedes or ties with a smaller index -- so the merged index is below h as well.  Once per (row, sub-quantizer): one
// compare and one select more than the search itself.
__device__ __forceinline__ int argmin_finish(const ArgminState &st, int hi) {
  int rf = 16;
#pragma unroll
  for (int r = 15; r >= 0; --r) rf = (((r & 1) ? st.ub[r >> 1].y : st.ub[r >> 1].x) <= st.best_v) ? r : rf;
  return rf == 16 ? 0 : st.best_t * 32 + 4 * hi + 8 * (rf >> 2) + (rf & 3);
}

// Prologue: the codebooks of sub-quantizers [i0, i0 + mg) -> LDS in A-fragment order, cbA [mg][NT][KS][64]: lane l of k-step
// kk holds C_i[t*32 + (l & 31)][2kk + (l >> 5)], zero past h and past the sub-space.  SUB > 0: every sub-space is SUB = 2 KS
// wide (constant strides); SUB == 0: the widths of p.off.
template <int KS, int NT, int SUB, int NTHREADS>
__device__ __forceinline__ void stage_codebooks_A(float *cbA, const EncParams &p, int i0, int mg, int tid) {
  const int h = p.h;
  for (int idx = tid; idx < mg * NT * KS * 64; idx += NTHREADS) {
    const int l = idx & 63;
    int rest = idx >> 6;
    const int kk = rest % KS; rest /= KS;
    const int t = rest % NT;
    const int i = i0 + rest / NT;
    const int cen = t * 32 + (l & 31);
    const int s = 2 * kk + (l >> 5);
    if constexpr (SUB > 0) {
      cbA[idx] = cen < h ? p.C[(size_t)h * SUB * i + (size_t)cen * SUB + s] : 0.0f;
    } else {
      const int sub = p.off[i + 1] - p.off[i];
      float v = 0.0f;
      if (cen < h && s < sub) v = p.C[(size_t)h * p.off[i] + (size_t)cen * sub + s];
      cbA[idx] = v;
    }
  }
}

// Prologue: |c_k|^2 (the canonical chain s = 0..sub-1 from +0) of the same sub-quantizers -> LDS in C/D-fragment order,
// saL [mg][NT][2][16], +Inf for the padded centroids k >= h.  SUB as above (the chain unrolls).
template <int NT, int SUB, int NTHREADS>
__device__ __forceinline__ void stage_norms_cd(float *saL, const EncParams &p, int i0, int mg, int tid) {
  const int h = p.h;
  for (int idx = tid; idx < mg * NT * 32; idx += NTHREADS) {
    const int c32 = idx & 31;
    const int t = (idx >> 5) % NT;
    const int il = (idx >> 5) / NT;
    const int i = i0 + il;
    const int cen = t * 32 + c32;
    float sa = __uint_as_float(0x7f800000u);
    if (cen < h) {
      sa = 0.0f;
      if constexpr (SUB > 0) {
        const float *c = p.C + (size_t)h * SUB * i + (size_t)cen * SUB;
#pragma unroll
        for (int s = 0; s < SUB; ++s) sa = __builtin_fmaf(c[s], c[s], sa);
      } else {
        const int sub = p.off[i + 1] - p.off[i];
        const float *c = p.C + (size_t)h * p.off[i] + (size_t)cen * sub;
        for (int s = 0; s < sub; ++s) sa = __builtin_fmaf(c[s], c[s], sa);
      }
    }
    const int hh = (c32 >> 2) & 1;
    const int r = (c32 & 3) + 4 * (c32 >> 3);
    saL[((size_t)(il * NT + t) * 2 + hh) * 16 + r] = sa;
  }
}

// The code bytes of one vector (m <= 32) are gathered in uint64_t cw[4] over the sub-quantizers of a launch and written once
// per tile.  (The gathering stays in the kernels: as a helper, in either of two forms, it moved cw into scratch or changed the
// tile loop's instructions.)
// o: the vector's m code bytes.  whole (m % 8 == 0 and the launch covers all m): 8-byte stores; else the bytes [i0, i1)
__device__ __forceinline__ void codewords_store(const uint64_t (&cw)[4], uint8_t *o, int m, int i0, int i1, bool whole) {
  if (whole) {
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if (w * 8 < m) reinterpret_cast<uint64_t *>(o)[w] = cw[w];
  } else {
    for (int i = i0; i < i1; ++i) o[i] = (uint8_t)(cw[i >> 3] >> (8 * (i & 7)));
  }
}

// ---- building blocks of the rotation kernels (rq_encode.hip) -------------------------------------------------------------
// R [d][d] -> LDS in A-fragment order, RA [NT][KK][64]: lane l of k-step kk holds R[t*32 + (l & 31)][2kk + (l >> 5)], zero
// outside R (PAD_K: the last k-step reaches one dimension past an odd d)
template <bool PAD_K>
__device__ __forceinline__ void stage_rotation_A(float *RA, const float *R, int d, int NT, int KK, int tid, int nthreads) {
  for (int idx = tid; idx < NT * KK * 64; idx += nthreads) {
    const int l = idx & 63;
    const int kk = (idx >> 6) % KK, t = (idx >> 6) / KK;
    const int i = t * 32 + (l & 31), k = 2 * kk + (l >> 5);
    RA[idx] = (i < d && (!PAD_K || k < d)) ? R[(size_t)i * d + k] : 0.0f;
  }
}
// one lane's 16 outputs of a 32 x 32 tile -> o[ibase + 8 g4 .. + 3], g4 = 0..3, as float4 (d % 4 == 0, o 16-byte aligned)
__device__ __forceinline__ void store_rotated_tile(float *o, const f32x16 &acc, int ibase, int d) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const int i0 = ibase + 8 * g4;
    if (i0 < d)
      *reinterpret_cast<float4 *>(o + i0) = make_float4(acc[g4 * 4 + 0], acc[g4 * 4 + 1], acc[g4 * 4 + 2], acc[g4 * 4 + 3]);
  }
}

// ---- byte rows (bvecs are UInt8, src/xvecs_read.jl:14-52; the reference widens them on the host, src/read_datasets.jl:148-167)
// The byte kernels read X as uint8 and widen in registers: u8 -> f32 is exact, so every value the f32 kernels load from the
// widened matrix is reproduced bit for bit, and everything after the loaders is the same code.
// byte_align: the widest power of two (<= 8) that divides the address of EVERY piece a kernel loads, X + row d + i SUB
// (+ 8 hi): the lowest set bit of X | d | SUB | 8.  Uniform over the launch.
__device__ __forceinline__ int byte_align(const void *X, int d, int sub) {
  const uint32_t mix = (uint32_t)(uintptr_t)X | (uint32_t)d | (uint32_t)sub | 8u;
  return (int)(mix & (0u - mix));
}
// w <- the first nb bytes at src (nb <= NB; a multiple of `al`), zero above them, with the widest loads `al` allows;
// nothing outside [src, src + nb) is read
template <int NB>
__device__ __forceinline__ void load_bytes(const uint8_t *src, int al, int nb, uint32_t (&w)[(NB + 3) / 4]) {
#pragma unroll
  for (int q = 0; q < (NB + 3) / 4; ++q) w[q] = 0u;
  if (NB % 8 == 0 && al >= 8) {
#pragma unroll
    for (int q = 0; q < NB / 8; ++q)
      if (8 * q < nb) { const uint2 v = *reinterpret_cast<const uint2 *>(src + 8 * q); w[2 * q] = v.x; w[2 * q + 1] = v.y; }
  } else if (NB % 4 == 0 && al >= 4) {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q)
      if (4 * q < nb) w[q] = *reinterpret_cast<const uint32_t *>(src + 4 * q);
  } else if (NB % 2 == 0 && al >= 2) {
#pragma unroll
    for (int q = 0; q < NB / 2; ++q)
      if (2 * q < nb) w[q >> 1] |= (uint32_t)*reinterpret_cast<const uint16_t *>(src + 2 * q) << (16 * (q & 1));
  } else {
#pragma unroll
    for (int q = 0; q < NB; ++q)
      if (q < nb) w[q >> 2] |= (uint32_t)src[q] << (8 * (q & 3));
  }
}
// byte S of the packed words as f32: the hardware's v_cvt_f32_ubyte0..3, no integer arithmetic on the way
template <int S>
__device__ __forceinline__ float byte_f32(const uint32_t *w) {
  float r;
  if constexpr ((S & 3) == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(r) : "v"(w[S >> 2]));
  else if constexpr ((S & 3) == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(r) : "v"(w[S >> 2]));
  else if constexpr ((S & 3) == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(r) : "v"(w[S >> 2]));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(r) : "v"(w[S >> 2]));
  return r;
}
template <int N, int S = 0>
__device__ __forceinline__ void bytes_f32(const uint32_t *w, float *x) {
  if constexpr (S < N) { x[S] = byte_f32<S>(w); bytes_f32<N, S + 1>(w, x); }
}

// Row loaders of rotate_kernel_v2 (rq_encode.hip): lane (j, hi) keeps the NP = D / 8 pieces X[row][8q + 4hi .. +3] of its row
// in flight.  issue() sends the loads of a row out, piece(q) is piece q as four floats.
template <int D>
struct RowsF32 {                 // 16-byte loads; X 16-byte aligned
  static constexpr int NP = D / 8;
  const float *X;
  float4 nx[NP];
  __device__ __forceinline__ explicit RowsF32(const float *x) : X(x) {}
  __device__ __forceinline__ void issue(int64_t row, int hi) {
    const float4 *src = reinterpret_cast<const float4 *>(X + row * D + 4 * hi);
#pragma unroll
    for (int q = 0; q < NP; ++q) nx[q] = src[2 * q];
  }
  __device__ __forceinline__ float4 piece(int q) const { return nx[q]; }
};
// Byte rows: one register per piece in flight instead of four, widened when the tile's turn comes (u8 -> f32 is exact, so R'X
// is bit for bit that of the widened rows).  The pieces sit at X + row D + 8q + 4hi with D % 8 == 0: 4-byte loads when X is
// 4-byte aligned, else 2-byte or single-byte loads.
template <int D>
struct RowsU8 {
  static constexpr int NP = D / 8;
  const uint8_t *X;
  const int al;
  uint32_t nx[NP];
  __device__ __forceinline__ explicit RowsU8(const float *x) : X(reinterpret_cast<const uint8_t *>(x)), al(byte_align(x, D, 4)) {}
  __device__ __forceinline__ void issue(int64_t row, int hi) {
    const uint8_t *src = X + (size_t)row * D + 4 * hi;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      uint32_t w[1];
      load_bytes<4>(src + 8 * q, al, 4, w);
      nx[q] = w[0];
    }
  }
  __device__ __forceinline__ float4 piece(int q) const {
    return make_float4(byte_f32<0>(&nx[q]), byte_f32<1>(&nx[q]), byte_f32<2>(&nx[q]), byte_f32<3>(&nx[q]));
  }
};

// rq_encode.hip: RX [n][d] <- R' x_j by rotate_kernel_v2, d in {32, 64, 96, 128}; X is f32 rows (16-byte aligned) or, with
// `bytes`, uint8 rows of any alignment
RQ_LOCAL int rotate_v2_launch(float *RX, const float *R, const void *X, bool bytes, int d, int64_t n, int num_cu, hipStream_t stream);
// rq_encode_filter.hip: filter launch + exact pass per group of sub-quantizers that fits LDS (even widths <= 16)
int encode_filter_launch(const EncParams &p, int sub, int nt, int waves, int num_cu, hipStream_t stream);
// the same on byte rows: p.X reinterpreted as uint8 [n][d], any alignment (encode_pq_filter_bytes_kernel)
int encode_filter_bytes_launch(const EncParams &p, int sub, int nt, int waves, int num_cu, hipStream_t stream);
// rq_encode.hip: whether the byte filter covers (d, m) under the current ENC_SPLIT, and its launch (encode_launch's
// set-up; records "encode_pq_filter_bytes_kernel" for rq_last_encode_kernel)
bool encode_filter_bytes_covers(int d, int m);
int encode_filter_bytes(uint8_t *codes, const uint8_t *X, const float *C, int64_t n, int d, int m, int h, int num_cu,
                        hipStream_t stream);

}  // namespace rq
