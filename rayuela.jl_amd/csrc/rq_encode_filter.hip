// rq_encode_filter.hip -- PQ encode (quantize_pq, src/PQ.jl:18-48) as two launches: a bf16 matrix-core FILTER that settles
// every (vector, sub-quantizer) pair whose nearest centroid is beyond doubt, and an EXACT pass over the pairs it leaves.
//
// The arithmetic that defines the answer is the canonical one of oracle/rq_oracle.c:264-328 (g, sa, sb = k-ordered fmaf
// chains from +0, v = max(fl(fl(sa + sb) - 2g), 0), first index of the minimum); see rq_encode.hip for the derivation of
// the filter's margin.  What the filter proves, per (vector, sub-quantizer):
//     W_k = |c_k|^2 - 2<c_k, x>  (bf16 hi/lo pieces on v_mfma_f32_32x32x16_bf16, accumulator pre-loaded with |c_k|^2)
//     |(W_k + |x|^2) - u_k| <= e = 1.02 * 2^-14 (|c_k|^2 + |x|^2)          (measured: tests/test_gpu_encode_margin.py)
//  => the canonical argmin, and everything that ties with it, lies in { k : W_k <= min W + DELTA },
//     DELTA = 3 * 2^-14 (max_k |c_k|^2 + |x|^2).
// If that set has ONE element, it is the argmin and nothing else needs computing (98 % of the pairs on SIFT-like data,
// 99.5 % on Deep-like).  Otherwise the pair's bit is set in flags[row]; encode_pq_fix_kernel then evaluates ALL h
// centroids of such a pair canonically on the VALU and overwrites the code.  Nothing approximate reaches the output.
//
// Why two launches (round 5): with the exact evaluation inside the filter kernel (rq_encode.hip, encode_pq_split_kernel)
// half of the wavefronts walked a divergent candidate loop with L2 latencies in it at 3 wavefronts per SIMD (0.08 ms of
// the 0.41 per 1e6 SIFT vectors), and the `if (improved) copy` of the tile loop cut the loop into basic blocks, so no LDS
// read was ever in flight across an MFMA chain (loads + MFMAs alone: 0.25 ms against floors of 0.08).  Here the tile loop
// is one straight-line block (the copy of the winning tile runs under an exec mask set inside the asm statement), the
// fragments of tile t + 1 are requested before the MFMAs of tile t issue, and the exact pass runs at full occupancy.
#include "rq_encode_split.h"

#include <type_traits>

namespace rq {

// ---- filter --------------------------------------------------------------------------------------------------------
// ub <- a in the lanes of `msk` (a lane mask under the current exec): eight 64-bit moves with exec narrowed INSIDE the
// statement -- no branch, so the tile loop stays one basic block.  `a` holds MFMA results: the statement depends on `msk`,
// which the caller derives from ordinary VALU reads of the same accumulator (tile_min), so the compiler's hazard wait for
// that MFMA precedes it (tests/test_isa.py walks the generated code for exactly this).
__device__ __forceinline__ void copy_lanes(f32x16 &ub, const f32x16 &a, uint64_t msk) {
  f32x2 d0 = {ub[0], ub[1]}, d1 = {ub[2], ub[3]}, d2 = {ub[4], ub[5]}, d3 = {ub[6], ub[7]};
  f32x2 d4 = {ub[8], ub[9]}, d5 = {ub[10], ub[11]}, d6 = {ub[12], ub[13]}, d7 = {ub[14], ub[15]};
  const f32x2 s0 = {a[0], a[1]}, s1 = {a[2], a[3]}, s2 = {a[4], a[5]}, s3 = {a[6], a[7]};
  const f32x2 s4 = {a[8], a[9]}, s5 = {a[10], a[11]}, s6 = {a[12], a[13]}, s7 = {a[14], a[15]};
  uint64_t sv;
  asm("s_mov_b64 %[sv], exec\n\t"
      "s_mov_b64 exec, %[m]\n\t"
      "v_mov_b64 %[d0], %[s0]\n\t"
      "v_mov_b64 %[d1], %[s1]\n\t"
      "v_mov_b64 %[d2], %[s2]\n\t"
      "v_mov_b64 %[d3], %[s3]\n\t"
      "v_mov_b64 %[d4], %[s4]\n\t"
      "v_mov_b64 %[d5], %[s5]\n\t"
      "v_mov_b64 %[d6], %[s6]\n\t"
      "v_mov_b64 %[d7], %[s7]\n\t"
      "s_mov_b64 exec, %[sv]"
      : [d0] "+v"(d0), [d1] "+v"(d1), [d2] "+v"(d2), [d3] "+v"(d3), [d4] "+v"(d4), [d5] "+v"(d5), [d6] "+v"(d6),
        [d7] "+v"(d7), [sv] "=&s"(sv)
      : [m] "s"(msk), [s0] "v"(s0), [s1] "v"(s1), [s2] "v"(s2), [s3] "v"(s3), [s4] "v"(s4), [s5] "v"(s5), [s6] "v"(s6),
        [s7] "v"(s7));
  ub[0] = d0.x; ub[1] = d0.y; ub[2] = d1.x; ub[3] = d1.y; ub[4] = d2.x; ub[5] = d2.y; ub[6] = d3.x; ub[7] = d3.y;
  ub[8] = d4.x; ub[9] = d4.y; ub[10] = d5.x; ub[11] = d5.y; ub[12] = d6.x; ub[13] = d6.y; ub[14] = d7.x; ub[15] = d7.y;
}

// 16 values <= thr, as a bit mask: four independent v_cmp / v_addc chains (one chain of 32 dependent instructions cost
// 0.04 ms per 1e6 SIFT vectors at 3 wavefronts per SIMD).  Only for values ordinary VALU instructions produced (see copy_lanes).
__device__ __forceinline__ uint32_t mask_leq16_4(const f32x16 &v, float thr) {
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 3; r >= 0; --r) {
    asm("v_cmp_le_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(c0) : "v"(v[r]), "v"(thr) : "vcc");
    asm("v_cmp_le_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(c1) : "v"(v[4 + r]), "v"(thr) : "vcc");
    asm("v_cmp_le_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(c2) : "v"(v[8 + r]), "v"(thr) : "vcc");
    asm("v_cmp_le_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(c3) : "v"(v[12 + r]), "v"(thr) : "vcc");
  }
  return c0 | (c1 << 4) | (c2 << 8) | (c3 << 12);
}

__device__ __forceinline__ float min16(const f32x16 &a) {
  const float m1 = __builtin_fminf(__builtin_fminf(a[0], a[1]), a[2]);
  const float m2 = __builtin_fminf(__builtin_fminf(a[3], a[4]), a[5]);
  const float m3 = __builtin_fminf(__builtin_fminf(a[6], a[7]), a[8]);
  const float m4 = __builtin_fminf(__builtin_fminf(a[9], a[10]), a[11]);
  const float m5 = __builtin_fminf(__builtin_fminf(a[12], a[13]), a[14]);
  float mm = __builtin_fminf(__builtin_fminf(m1, m2), m3);
  mm = __builtin_fminf(__builtin_fminf(mm, m4), m5);
  return __builtin_fminf(mm, a[15]);
}

// LDS image of the sub-codebooks of one launch (same layout as encode_pq_split_kernel's), built ONCE per launch in global
// scratch by encode_tables_kernel and copied by every workgroup of the filter with straight 16-byte loads.  (Built inside
// each workgroup -- 8 strided scalar loads per fragment, a dozen dependent round trips to L2 -- the prologue took 50 us of
// the 280 a 1e6-row SIFT-shape launch lasts, and nearly all of a short one.)
//   cbA [mg][NT][NPIECE][64] uint4  bf16 pieces of -2c in the A-fragment order of v_mfma_f32_32x32x16_bf16 (lane l: centroid
//                                   l & 31, K elements 8 (l >> 5) .. + 7; PACK: K 0-7 = hi pieces, 8-15 = lo pieces)
//   saL [mg][NT][2][16] float       |c_k|^2 (canonical chain s = 0..sub-1 from +0) in C/D-fragment order, +inf for k >= h
//   saMax [mg] float                max_k |c_k|^2 over the real centroids (NaN if any norm is NaN), padded to 16 bytes
template <int SUB>
__host__ __device__ constexpr size_t filter_image_bytes(int mg, int NT) {
  return (size_t)mg * NT * SplitShape<SUB>::NPIECE * 64 * 16 + (size_t)mg * NT * 32 * 4 + (((size_t)mg * 4 + 15) & ~(size_t)15);
}

// grid = mg workgroups (one per sub-quantizer of the launch) x 256 threads
template <int SUB, int NT>
__global__ __launch_bounds__(256) void encode_tables_kernel(EncParams p) {
  constexpr bool PACK = SplitShape<SUB>::PACK;
  constexpr int NPIECE = SplitShape<SUB>::NPIECE;
  const int h = p.h, i0 = p.i0, mg = p.i1 - p.i0, il = blockIdx.x;
  uint4 *cbA = reinterpret_cast<uint4 *>(p.image);
  float *saL = reinterpret_cast<float *>(cbA + (size_t)mg * NT * NPIECE * 64);
  float *saMax = saL + (size_t)mg * NT * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ float wmax[4];
  for (int idx = tid; idx < NT * NPIECE * 64; idx += 256) {
    const int l = idx & 63;
    const int piece = (idx >> 6) % NPIECE;
    const int t = (idx >> 6) / NPIECE;
    const int cen = t * 32 + (l & 31);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int sx = PACK ? e : 8 * (l >> 5) + e;            // dimension of this K element
      const bool lo = PACK ? (l >> 5) != 0 : piece != 0;      // which bf16 piece
      uint32_t bits = 0;
      if (cen < h && sx < SUB) {
        const float v = -2.0f * p.C[((size_t)(i0 + il) * h + cen) * SUB + sx];
        const uint32_t hb = bf16_bits(v);
        bits = lo ? bf16_bits(v - bf16_val(hb)) : hb;
      }
      w[e >> 1] |= bits << (16 * (e & 1));
    }
    cbA[(size_t)il * NT * NPIECE * 64 + idx] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  float mx = 0.0f;
  for (int idx = tid; idx < NT * 32; idx += 256) {
    const int c32 = idx & 31, t = idx >> 5;
    const int cen = t * 32 + c32;
    float sa = __uint_as_float(0x7f800000u);
    if (cen < h) {
      const float *c = p.C + ((size_t)(i0 + il) * h + cen) * SUB;
      sa = 0.0f;
#pragma unroll
      for (int sx = 0; sx < SUB; ++sx) sa = __builtin_fmaf(c[sx], c[sx], sa);
      mx = __builtin_fmaxf(mx, sa) + (sa != sa ? sa : 0.0f);    // a NaN norm poisons the bound -> exact pass
    }
    saL[((size_t)(il * NT + t) * 2 + ((c32 >> 2) & 1)) * 16 + (c32 & 3) + 4 * (c32 >> 3)] = sa;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(mx, off);
    mx = (o != o || mx != mx) ? __uint_as_float(0x7fc00000u) : __builtin_fmaxf(mx, o);
  }
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  if (tid == 0) {
    float r = wmax[0];
    for (int w = 1; w < 4; ++w) r = (r != r || wmax[w] != wmax[w]) ? __uint_as_float(0x7fc00000u) : __builtin_fmaxf(r, wmax[w]);
    saMax[il] = r;
  }
}

// ---- exact pass ----------------------------------------------------------------------------------------------------
// One 1024-thread workgroup per chunk of p.fix_rows rows (4096 where the lists fit LDS; fewer for many sub-quantizers).  The flagged rows of the chunk are collected per sub-quantizer in LDS;
// a work item is (sub-quantizer, 32 flagged rows), taken by the wavefronts in turn.  The canonical evaluation is the one of
// the direct kernels (rq_encode.hip): the h x 32 inner products come off v_mfma_f32_32x32x2_f32 -- bit for bit the k-ordered
// fmaf chain of oracle/rq_oracle.c:264-328 -- with the centroids (A fragments) read straight from global memory (the
// sub-codebooks are L2-resident: 16 KiB per item), then tile_argmin / argmin_finish on all h centroids: the first index of
// the minimum of v = max(fl(fl(sa + sb) - 2g), 0), whatever the filter thought of the pair.  (Round 5's first version
// evaluated the centroids on the VALU, four per lane and one row per wavefront at a time: 0.34 ns per pair, 0.1 ms for the
// 2.4 % of the pairs of 1e6 SIFT-like vectors; on the matrix cores it is ~0.1 ns.)
// (Round 5, measured and not kept: the same pass at the END of the filter kernel -- per-workgroup lists of the open pairs, the
// |c|^2 table already in LDS, no flags array, one launch less.  Same speed at 1e6 rows (0.348 / 0.350 vs 0.345 / 0.344 ms at SIFT
// shape, 0.513 / 0.520 vs 0.522 / 0.532 at Deep shape; 41 vs 46 us at 8192 rows): a workgroup's 16 items over 12 wavefronts are two
// rounds of the same dependent chain -- row -> sub-vector from HBM -> centroid rows from L2 -> 64 MFMAs -- behind a barrier all
// its wavefronts reach at different times, and it needs 4 m bytes of list scratch per row instead of 4.)
// Chunk size, measured (rocprofv3, 1e6 rows; flagged pairs 1.5 % / 0.5 %): 1024 rows x 256 threads 46 / 49 us (SIFT / Deep shape),
// 2048 x 512 40 / 37, 4096 x 512 38 / 23, 4096 x 1024 38 / 21.5 -- sparse flags want big chunks (fuller 32-row items).
#ifndef RQ_FIX_ROWS
#define RQ_FIX_ROWS 4096
#endif
#ifndef RQ_FIX_THREADS
#define RQ_FIX_THREADS 1024
#endif
constexpr int FIX_ROWS_MAX = RQ_FIX_ROWS;       // rows per workgroup when the per-sub-quantizer lists (2 bytes per row) fit LDS
constexpr int FIX_THREADS = RQ_FIX_THREADS;

// ---- the kernels ---------------------------------------------------------------------------------------------------
// encode_pq_filter_kernel, exact_item and encode_pq_fix_kernel live in rq_encode_filter_body.inc, which is included twice: for
// f32 rows, and for byte rows (encode_pq_filter_bytes_kernel, exact_item_bytes, encode_pq_fix_bytes_kernel: p.X read as uint8
// [n][d] at any alignment, widened in registers).  Text, not a template, is what the two share: the f32
// kernels' code is walked by tests/test_isa.py and moved when their body became a function template.
#define RQ_ENC_BYTES 0
#include "rq_encode_filter_body.inc"
#undef RQ_ENC_BYTES
#define RQ_ENC_BYTES 1
#include "rq_encode_filter_body.inc"
#undef RQ_ENC_BYTES

static thread_local unsigned long long g_enc_stats[2] = {0, 0};
void last_encode_stats(unsigned long long out[2]) { out[0] = g_enc_stats[0]; out[1] = g_enc_stats[1]; }

template <int SUB, int NT, int NWAVES, bool BYTES>
static int launch_encode_filter(EncParams p, int num_cu, hipStream_t stream) {
  p.NT = NT;
  DeviceLock launch_lock;      // flags scratch (per device and stream) is written by the filter and read by the exact pass
  constexpr int NPIECE = SplitShape<SUB>::NPIECE;
  const size_t per_sub = (size_t)NT * NPIECE * 64 * 16 + (size_t)NT * 32 * sizeof(float) + sizeof(float);
  const size_t budget = 160 * 1024 - 64;
  const int gmax = (int)std::min<size_t>(std::min<size_t>(budget / per_sub, (size_t)p.m), 32);
  if (gmax < 1) return fail(RQ_EUNSUPPORTED, "split encode: one sub-codebook needs %zu B of LDS", per_sub);
  // Rows go through in pieces of ENC_CHUNK_ROWS (4 Mi rows: 16 MiB of flags), so the library's scratch for this path is bounded
  // whatever n is (an encode of 1e8 rows would otherwise keep 400 MB of flags per device and stream); a 1e6-row call is one piece.
  const int64_t rows_all = p.n;
  // rows per workgroup of the exact pass: as many as the LDS lists allow (2 bytes per row and sub-quantizer of the launch group)
  {
    const size_t fixed = (size_t)gmax * NT * 32 * sizeof(float) + 32 * sizeof(uint32_t);
    int64_t fr = ((int64_t)(160 * 1024 - 256) - (int64_t)fixed) / ((int64_t)gmax * 2);
    fr = std::min<int64_t>(FIX_ROWS_MAX, fr / 32 * 32);
    if (p.n < 500000) fr = std::min<int64_t>(fr, FIX_ROWS_MAX / 4);      // short inputs: more, smaller workgroups (latency)
    if (fr < 32) return fail(RQ_EUNSUPPORTED, "split encode: the exact pass's lists do not fit LDS (m=%d)", p.m);
    p.fix_rows = (int)fr;
  }
  const int FIX_ROWS = p.fix_rows;
  const int64_t piece = std::max<int64_t>(FIX_ROWS, (int64_t)tuning("ENC_CHUNK_ROWS", 1 << 22));
  void *fl = nullptr;
  const size_t img_bytes = (filter_image_bytes<SUB>(gmax, NT) + 255) & ~(size_t)255;
  RQ_TRY(workspace(WS_ENCFLAG, img_bytes + (size_t)std::min(rows_all, piece) * sizeof(uint32_t), &fl, stream));
  p.image = static_cast<unsigned char *>(fl);
  p.flags = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(fl) + img_bytes);
  // ENC_STATS = 1 (tests, DESIGN's figures): count the pairs that take the exact pass; costs a synchronous read-back
  p.stat = nullptr;
  const bool want_stats = tuning("ENC_STATS", 0) != 0;
  void *stat_dev = nullptr;
  if (want_stats) {
    RQ_TRY(workspace(WS_COUNTER, WS_COUNTER_BYTES, &stat_dev, stream));
    p.stat = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(stat_dev) + 128);
    RQ_HIP(hipMemsetAsync(p.stat, 0, 8, stream));
  }
  void (*kern)(EncParams);
  void (*fix_kern)(EncParams);
  if constexpr (BYTES) {      // p.X points at uint8 rows
    if (p.dbg_w) return fail(RQ_EUNSUPPORTED, "the filter's W values are recorded on f32 rows only");
    kern = encode_pq_filter_bytes_kernel<SUB, NT, NWAVES, false>;
    fix_kern = encode_pq_fix_bytes_kernel<SUB, NT>;
  } else {
    kern = p.dbg_w ? encode_pq_filter_kernel<SUB, NT, NWAVES, true> : encode_pq_filter_kernel<SUB, NT, NWAVES, false>;
    fix_kern = encode_pq_fix_kernel<SUB, NT>;
  }
  const float *X_all = p.X;
  uint8_t *codes_all = p.codes;
  float *dbg_all = p.dbg_w;
  for (int i0 = 0; i0 < p.m; i0 += gmax) {
    p.i0 = i0;
    p.i1 = std::min(p.m, i0 + gmax);
    const size_t lds = filter_image_bytes<SUB>(p.i1 - p.i0, NT);
    hipLaunchKernelGGL((encode_tables_kernel<SUB, NT>), dim3(p.i1 - p.i0), dim3(256), 0, stream, p);
    RQ_HIP(hipGetLastError());
    RQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const size_t fix_lds = (size_t)(p.i1 - p.i0) * NT * 32 * sizeof(float) + 32 * sizeof(uint32_t) + (size_t)(p.i1 - p.i0) * FIX_ROWS * sizeof(uint16_t);
    RQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fix_kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fix_lds));
    for (int64_t r0 = 0; r0 < rows_all; r0 += piece) {
      p.n = std::min(piece, rows_all - r0);
      if constexpr (BYTES) p.X = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(X_all) + (size_t)r0 * p.d);
      else p.X = X_all + (size_t)r0 * p.d;
      p.codes = codes_all + (size_t)r0 * p.m;
      p.dbg_w = dbg_all ? dbg_all + (size_t)r0 * p.m * p.h : nullptr;
      const int64_t ntiles = (p.n + 31) / 32;
      const int grid = (int)std::min<int64_t>(num_cu, (ntiles + NWAVES - 1) / NWAVES);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(NWAVES * 64), lds, stream, p);
      RQ_HIP(hipGetLastError());
      hipLaunchKernelGGL(fix_kern, dim3((unsigned)((p.n + FIX_ROWS - 1) / FIX_ROWS)), dim3(FIX_THREADS), fix_lds, stream, p);
      RQ_HIP(hipGetLastError());
    }
  }
  p.n = rows_all;
  if (want_stats) {
    unsigned long long fl_pairs = 0;
    RQ_HIP(hipMemcpyAsync(&fl_pairs, p.stat, 8, hipMemcpyDeviceToHost, stream));
    RQ_HIP(hipStreamSynchronize(stream));
    g_enc_stats[0] = (unsigned long long)p.n * (unsigned long long)p.m;
    g_enc_stats[1] = fl_pairs;
  }
  return RQ_OK;
}

template <bool BYTES>
static int encode_filter_dispatch(const EncParams &p, int sub, int nt, int waves, int num_cu, hipStream_t stream) {
#define RQ_FILTER_NT(SUBV, NW)                                                        \
  do {                                                                                \
    if (nt <= 1) return launch_encode_filter<SUBV, 1, NW, BYTES>(p, num_cu, stream);    \
    if (nt <= 2) return launch_encode_filter<SUBV, 2, NW, BYTES>(p, num_cu, stream);    \
    if (nt <= 4) return launch_encode_filter<SUBV, 4, NW, BYTES>(p, num_cu, stream);    \
    return launch_encode_filter<SUBV, 8, NW, BYTES>(p, num_cu, stream);                 \
  } while (0)
#define RQ_FILTER_CASE(SUBV)                                                          \
  if (sub == SUBV) {                                                                  \
    if (waves == 8) RQ_FILTER_NT(SUBV, 8);                                            \
    if (waves == 12 || (waves == 0 && SUBV > 8)) RQ_FILTER_NT(SUBV, 12);              \
    RQ_FILTER_NT(SUBV, 16);                                                           \
  }
  RQ_FILTER_CASE(2) RQ_FILTER_CASE(4) RQ_FILTER_CASE(6) RQ_FILTER_CASE(8)
  RQ_FILTER_CASE(10) RQ_FILTER_CASE(12) RQ_FILTER_CASE(14) RQ_FILTER_CASE(16)
#undef RQ_FILTER_CASE
#undef RQ_FILTER_NT
  return fail(RQ_EUNSUPPORTED, "filter encode covers even sub-space widths up to 16; got %d", sub);
}

int encode_filter_launch(const EncParams &p, int sub, int nt, int waves, int num_cu, hipStream_t stream) {
  return encode_filter_dispatch<false>(p, sub, nt, waves, num_cu, stream);
}
int encode_filter_bytes_launch(const EncParams &p, int sub, int nt, int waves, int num_cu, hipStream_t stream) {
  return encode_filter_dispatch<true>(p, sub, nt, waves, num_cu, stream);
}

}  // namespace rq
