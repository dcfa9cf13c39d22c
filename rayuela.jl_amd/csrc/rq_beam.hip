// rq_beam.hip -- beam-search residual encoding (src/CompetitiveQ.jl:75-135 `encode`) on gfx950; contract in DESIGN.md
// section 2 ("Beam encoding contract"), LDS / occupancy reasoning in section 4.15.
//
// Per chunk of vectors and per stage i the beams live in a double buffer: parent rows R [nvec * H_i][d] with their code
// prefixes P [nvec * H_i][m]; stage 0 reads X itself (H_0 = 1, empty prefix).
//
//   beam_stage_kernel   a workgroup owns VB = 64 / H_i whole vectors = at most 64 parent rows (two 32-row MFMA tiles), so
//                       every candidate of a vector sits in one workgroup.  The codebook C_i and the rows stream through LDS
//                       in slices of 16 dimensions (A-fragment order / padded row-major), double buffered; wavefront w
//                       keeps the accumulators of row tile w & 1 and centroid tiles (w >> 1) + 2u.  v_mfma_f32_32x32x2_f32
//                       IS the k-ordered fmaf chain of the contract; padded dimensions multiply 0 by 0.  The epilogue
//                       stores the clamped v = fl(fl(sa + sb) - 2 g) of every candidate as its f32 bits in LDS (v >= +0
//                       and never NaN, so the bits order as unsigned integers), then one wavefront per vector extracts
//                       the H_{i+1} smallest keys (bits << 32 | j * h + k) in order: lane s owns the strip of candidates
//                       e = s (mod 64) and its current minimum; a round takes the minimum over the lanes, and only the
//                       strip that lost its minimum is scanned again, by all 64 lanes.
//   beam_expand_kernel  one wavefront per survivor: residual fl(r_parent - C_i[k]), prefix = parent's prefix ++ k, written
//                       to the other half of the double buffer; after the last stage only rank 0, straight to the outputs.
//
//
// More than 256 codewords per stage (16-bit codes): the kernels are templates over the code type.  With
// Code = int16_t the stage kernel streams C_i in blocks of 256 codewords, as encode_h16_kernel does: one block's values sit in
// LDS at a time, its at most H_{i+1} smallest keys (now bits << 32 | j * h + k with the GLOBAL k) are extracted as above and
// merged into a running sorted list of H_{i+1} keys per vector, also in LDS.  Keys are distinct, so the H smallest of the union
// are the H smallest of (running list + the block's H smallest): the survivors do not depend on the block size.  A block stops
// extracting at the first key above the running list's largest.  Code = uint8_t compiles to the single-block kernel as it was.
//
// No float atomics; nothing depends on the chunking: a vector's result is a function of its own row and C alone.
#include "rq_internal.h"

#include <atomic>
#include <utility>
#include <vector>

namespace rq {

namespace {

constexpr size_t BEAM_SCRATCH_BYTES = (size_t)2 << 30;   // beams of one chunk, per device and stream (as ICM / ChainQ)
constexpr int BM_MAX_BEAM = 32;
constexpr int BM_ROWS = 64;             // parent rows of a workgroup: two row tiles
constexpr int BM_KC = 8;                // k-steps per staged slice
constexpr int BM_DIMS = 2 * BM_KC;      // dimensions per staged slice
constexpr int BM_XSTR = BM_DIMS + 1;    // padded row stride of the staged rows
constexpr int BM_TPW = 4;               // centroid tiles per wavefront (h <= 256: 8 tiles over 2 wavefront pairs)
using bm_f32x16 = float __attribute__((ext_vector_type(16)));

struct BeamStage {
  const float *R;        // parent rows [nvec * Hi][d]
  const float *Ci;       // [h][d]
  const float *sa;       // [h]
  uint8_t *selP;         // [nvec][Hn]
  void *selK;            // [nvec][Hn] of the code type
  float *selV;
  int64_t nvec;
  int d, h, Hi, Hn, VB, NT;
};

__device__ inline long long bm_wave_min(long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64);
    const int hi = __shfl_xor((int)(v >> 32), o, 64);
    const long long w = ((long long)hi << 32) | (unsigned int)lo;
    v = w < v ? w : v;
  }
  return v;
}

__device__ inline long long bm_shfl64(long long v, int src) {
  const int lo = __shfl((int)(v & 0xffffffffll), src, 64);
  const int hi = __shfl((int)(v >> 32), src, 64);
  return ((long long)hi << 32) | (unsigned int)lo;
}

// bytes of the running lists of a workgroup (Code = int16_t): [VB][Hn] keys, kept a multiple of 16
__host__ __device__ inline size_t bm_run_bytes(int VB, int Hn) { return (((size_t)VB * Hn * 8) + 15) & ~(size_t)15; }

template <bool VEC4, class Code>
__global__ __launch_bounds__(256) void beam_stage_kernel(BeamStage p) {
  constexpr bool WIDE = sizeof(Code) == 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int d = p.d, hall = p.h, Hi = p.Hi, Hn = p.Hn, NT = p.NT;
  const int CHUNK = NT * BM_KC * 64;                       // floats of a staged codebook slice
  long long *runL = reinterpret_cast<long long *>(smem);   // WIDE: [VB][Hn] running keys, sorted
  float *cb0 = reinterpret_cast<float *>(smem + (WIDE ? bm_run_bytes(p.VB, Hn) : 0));   // [2][CHUNK], A-fragment order
  float *xs0 = cb0 + 2 * CHUNK;                            // [2][BM_ROWS][BM_XSTR]
  float *saL = xs0 + 2 * BM_ROWS * BM_XSTR;                // [NT * 32]
  uint32_t *vals = reinterpret_cast<uint32_t *>(saL + NT * 32);   // [VB][NP]: candidate el of a vector at el + (el >> 6)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, hi = lane >> 5;
  const int rt = wave & 1, th = wave >> 1;

  const int64_t vec0 = (int64_t)blockIdx.x * p.VB;
  const int nv = (int)min((int64_t)p.VB, p.nvec - vec0);
  const int rows_blk = nv * Hi;
  const int64_t row0 = vec0 * Hi, last_row = p.nvec * Hi - 1;
  Code *selK = reinterpret_cast<Code *>(p.selK);
  // the codeword block in hand: codewords cbase .. cbase + h - 1 of the stage (the byte kernel: the whole codebook)
  const int nblocks = WIDE ? (hall + 255) >> 8 : 1;
  const int NPS = Hi * min(hall, 256) + ((Hi * min(hall, 256) + 63) >> 6);   // row stride of vals: the largest block's
#pragma unroll 1
  for (int blk = 0; blk < nblocks; ++blk) {
  const int cbase = blk << 8;
  const int h = WIDE ? min(256, hall - cbase) : hall;
  const float *Cb = p.Ci + (size_t)cbase * d;
  const int N = Hi * h, NP = WIDE ? NPS : N + ((N + 63) >> 6);

  for (int e = tid; e < NT * 32; e += 256) saL[e] = e < h ? p.sa[cbase + e] : 0.0f;

  // slice c of the codebook and of the rows, global -> registers -> LDS.  A row past the block's last repeats a valid row
  // and a centroid past h reads as zero: neither is stored.
  float cr[16], xr[4];
  auto load_slice = [&](int c) {
    if (VEC4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = tid + 256 * u, cen = q >> 2, dim = c * BM_DIMS + 4 * (q & 3);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (cen < h && dim < d) v = *reinterpret_cast<const float4 *>(Cb + (size_t)cen * d + dim);
        cr[4 * u] = v.x; cr[4 * u + 1] = v.y; cr[4 * u + 2] = v.z; cr[4 * u + 3] = v.w;
      }
      const int64_t gr = min(row0 + (tid >> 2), last_row);
      const int dim = c * BM_DIMS + 4 * (tid & 3);
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (dim < d) v = *reinterpret_cast<const float4 *>(p.R + (size_t)gr * d + dim);
      xr[0] = v.x; xr[1] = v.y; xr[2] = v.z; xr[3] = v.w;
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u, l = e & 63, kk = (e >> 6) & (BM_KC - 1), t = e >> 9;
        const int cen = t * 32 + (l & 31), dim = c * BM_DIMS + 2 * kk + (l >> 5);
        cr[u] = (t < NT && cen < h && dim < d) ? Cb[(size_t)cen * d + dim] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + 256 * u;
        const int64_t gr = min(row0 + (e >> 4), last_row);
        const int dim = c * BM_DIMS + (e & 15);
        xr[u] = dim < d ? p.R[(size_t)gr * d + dim] : 0.0f;
      }
    }
  };
  auto store_slice = [&](int buf) {
    float *cb = cb0 + buf * CHUNK, *xs = xs0 + buf * BM_ROWS * BM_XSTR;
    if (VEC4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = tid + 256 * u, cen = q >> 2, pc = q & 3;
        if (cen < NT * 32) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            cb[(((cen >> 5) * BM_KC) + 2 * pc + (i >> 1)) * 64 + (i & 1) * 32 + (cen & 31)] = cr[4 * u + i];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) xs[(tid >> 2) * BM_XSTR + 4 * (tid & 3) + i] = xr[i];
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int e = tid + 256 * u;
        if (e < CHUNK) cb[e] = cr[u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = tid + 256 * u;
        xs[(e >> 4) * BM_XSTR + (e & 15)] = xr[u];
      }
    }
  };

  const int nchunks = (d + BM_DIMS - 1) / BM_DIMS;
  load_slice(0);
  store_slice(0);
  __syncthreads();

  bm_f32x16 acc[BM_TPW];
#pragma unroll
  for (int u = 0; u < BM_TPW; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;
  float sb = 0.0f;
#pragma unroll 1
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nchunks;
    if (more) load_slice(c + 1);
    const float *cb = cb0 + buf * CHUNK + lane;
    const float *xw = xs0 + buf * BM_ROWS * BM_XSTR + (rt * 32 + j) * BM_XSTR;
    float b[BM_KC];
#pragma unroll
    for (int kk = 0; kk < BM_KC; ++kk) {
      const float x0 = xw[2 * kk], x1 = xw[2 * kk + 1];
      b[kk] = hi ? x1 : x0;
      sb = __builtin_fmaf(x0, x0, sb);
      sb = __builtin_fmaf(x1, x1, sb);
    }
#pragma unroll
    for (int u = 0; u < BM_TPW; ++u) {
      const int t = th + 2 * u;
      if (t < NT) {
#pragma unroll
        for (int kk = 0; kk < BM_KC; ++kk)
          acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(cb[(t * BM_KC + kk) * 64], b[kk], acc[u], 0, 0, 0);
      }
    }
    if (more) store_slice(buf ^ 1);   // its readers finished before the barrier that ended slice c - 1
    __syncthreads();
  }

  // ---- values of all candidates -> LDS ------------------------------------------------------------------------------
  {
    const int row = rt * 32 + j;
    if (row < rows_blk) {
      const int vl = row / Hi, pj = row - vl * Hi;
      uint32_t *V = vals + (size_t)vl * NP;
#pragma unroll
      for (int u = 0; u < BM_TPW; ++u) {
        const int t = th + 2 * u;
        if (t < NT) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (k < h) {
              const float uu = (saL[k] + sb) - 2.0f * acc[u][r];
              const float v = uu > 0.0f ? uu : 0.0f;
              const int el = pj * h + k;
              V[el + (el >> 6)] = __float_as_uint(v);
            }
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- the Hn smallest (v, j * h + k) of each vector, in order --------------------------------------------------------
  const long long KMAX = 0x7fffffffffffffffll;
  const int L = (N + 63) >> 6;   // longest strip
  for (int vl = wave; vl < nv; vl += 4) {
    const uint32_t *V = vals + (size_t)vl * NP;
    long long mine = KMAX;
    for (int t = 0; t < L; ++t) {
      const int e = lane + 64 * t;
      if (e < N) {
        const long long key = ((long long)V[lane + 65 * t] << 32) | (unsigned int)e;
        mine = key < mine ? key : mine;
      }
    }
    const int64_t out = (vec0 + vl) * Hn;
    // WIDE: the vector's running list (always this wavefront's), the largest key it holds, and in lane s the block's s-th key
    long long *run = runL + (size_t)vl * Hn;
    const long long worst = (WIDE && blk > 0) ? run[Hn - 1] : KMAX;
    long long got = KMAX;
    for (int s = 0; s < Hn; ++s) {
      const long long g = bm_wave_min(mine);
      const int e = (int)(g & 0xffffffffll);
      if constexpr (WIDE) {
        if (g == KMAX) break;                                  // the block holds fewer than Hn candidates
        const int pj = e / h;
        const long long gk = (g & ~0xffffffffll) | (unsigned int)(pj * hall + cbase + (e - pj * h));
        if (gk > worst) break;                                 // and so is every later key of this block
        if (lane == s) got = gk;
      } else {
        if (lane == 0) {
          const int pj = e / h;
          p.selP[out + s] = (uint8_t)pj;
          selK[out + s] = (Code)(e - pj * h);
          p.selV[out + s] = __uint_as_float((uint32_t)(g >> 32));
        }
      }
      if (s + 1 == Hn) break;
      const int so = e & 63;
      long long cand = KMAX;
      for (int t = lane; t < L; t += 64) {
        const int e2 = so + 64 * t;
        if (e2 < N) {
          const long long key = ((long long)V[so + 65 * t] << 32) | (unsigned int)e2;
          if (key > g && key < cand) cand = key;
        }
      }
      cand = bm_wave_min(cand);
      if (lane == so) mine = cand;
    }
    if constexpr (WIDE) {
      // merge: lanes 0..31 hold the block's keys, lanes 32..63 the running list; keys are distinct, so a key's rank in the
      // union is the number of smaller keys, and the Hn smallest go to their ranks (after the last block: to the outputs)
      const long long old = (blk > 0 && lane >= 32 && lane - 32 < Hn) ? run[lane - 32] : KMAX;
      const long long key = lane < 32 ? got : old;
      int rank = 0;
      for (int t = 0; t < Hn; ++t) {
        rank += bm_shfl64(key, t) < key ? 1 : 0;
        rank += bm_shfl64(key, 32 + t) < key ? 1 : 0;
      }
      if (key != KMAX && rank < Hn) {
        if (blk + 1 < nblocks) {
          run[rank] = key;
        } else {
          const int e = (int)(key & 0xffffffffll), pj = e / hall;
          p.selP[out + rank] = (uint8_t)pj;
          selK[out + rank] = (Code)(e - pj * hall);
          p.selV[out + rank] = __uint_as_float((uint32_t)(key >> 32));
        }
      }
    }
  }
  }   // codeword blocks
}

// one wavefront per written row: survivor s < Hout of vector v, chosen by sel[v * Hn + s]
template <class Code>
__global__ __launch_bounds__(256) void beam_expand_kernel(float *Rn, Code *Pn, float *cost, const float *R, const Code *P,
                                                          const float *Ci, const uint8_t *selP, const Code *selK,
                                                          const float *selV, int64_t nvec, int d, int m, int stage, int Hi,
                                                          int Hn, int Hout) {
  const int lane = threadIdx.x & 63;
  const int64_t orow = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (orow >= nvec * Hout) return;
  const int64_t v = orow / Hout;
  const int s = (int)(orow - v * Hout);
  const int64_t si = v * Hn + s;
  const int pj = selP[si], k = selK[si];
  const int64_t prow = v * Hi + pj;
  if (Rn) {
    const float *r = R + (size_t)prow * d, *c = Ci + (size_t)k * d;
    float *o = Rn + (size_t)orow * d;
    for (int t = lane; t < d; t += 64) o[t] = r[t] - c[t];
  }
  Code *po = Pn + (size_t)orow * m;
  if (lane < stage) po[lane] = P[(size_t)prow * m + lane];
  if (lane == stage) po[lane] = (Code)k;
  if (cost && lane == 0) cost[orow] = selV[si];
}

// phase clock: milliseconds of the calling thread's last call {stage kernels, expand kernels, other}
enum { BP_STAGE, BP_EXPAND, BP_OTHER, BP_N };
struct BeamClock {
  hipStream_t s = nullptr;
  hipEvent_t prev = nullptr;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> spans;
  bool on = false, collected = true;
  double ms[BP_N] = {0, 0, 0};
  void clear() {
    if (on) {
      if (spans.empty()) (void)hipEventDestroy(prev);
      else (void)hipEventDestroy(spans.front().second.first);
      for (auto &sp : spans) (void)hipEventDestroy(sp.second.second);
    }
    spans.clear();
    prev = nullptr;
    on = false;
    collected = true;
    for (int q = 0; q < BP_N; ++q) ms[q] = 0;
  }
  void start(hipStream_t st) {
    clear();
    s = st;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return; }
    if (cs != hipStreamCaptureStatusNone) return;   // no timing events inside a captured graph
    if (hipEventCreate(&prev) != hipSuccess) { (void)hipGetLastError(); prev = nullptr; return; }
    (void)hipEventRecord(prev, s);
    on = true;
    collected = false;
  }
  void mark(int phase) {
    if (!on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return; }
    (void)hipEventRecord(e, s);
    spans.push_back({phase, {prev, e}});
    prev = e;
  }
  // waits for the last event of the call
  void collect() {
    if (!on || collected) return;
    collected = true;
    if (spans.empty()) return;
    if (hipEventSynchronize(spans.back().second.second) != hipSuccess) { (void)hipGetLastError(); return; }
    for (auto &sp : spans) {
      float t = 0;
      if (hipEventElapsedTime(&t, sp.second.first, sp.second.second) == hipSuccess) ms[sp.first] += t;
      else (void)hipGetLastError();
    }
  }
};
// never destroyed: events must not be released after the runtime is gone
BeamClock &beam_clock() {
  static thread_local BeamClock *c = new BeamClock();
  return *c;
}

// wide: the int16 entry points -- 1 <= h <= RQ_MAX_H16, and the error codes of the other *_wide encodes (a shape outside what
// the code type or the kernels cover is RQ_EUNSUPPORTED)
int beam_check(const char *who, const void *codes, const void *X, const void *C, int64_t n, int d, int m, int h, int H,
               int nsplits, bool wide = false, int code_base = 0) {
  if (wide) {
    if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
    if (m < 1 || m > 64) return fail(RQ_EUNSUPPORTED, "%s covers 1 <= m <= 64; got m=%d", who, m);
    if (h > RQ_MAX_H16) return fail(RQ_EUNSUPPORTED, "%s emits Int16 codes: 1 <= h <= %d; got h=%d", who, RQ_MAX_H16, h);
    if (h < 1) return fail(RQ_EINVAL, "%s: h=%d < 1", who, h);
  }
  if (m < 1 || m > 64) return fail(RQ_EINVAL, "%s: m=%d outside 1..64", who, m);
  if (!wide && (h < 1 || h > 256)) return fail(RQ_EINVAL, "%s: h=%d outside 1..256", who, h);
  if (H < 1 || H > BM_MAX_BEAM) return fail(RQ_EINVAL, "%s: beam width H=%d outside 1..%d", who, H, BM_MAX_BEAM);
  if (H > h) return fail(RQ_EINVAL, "%s: beam width H=%d exceeds h=%d (the reference takes sortperm(...)[1:H])", who, H, h);
  if (d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);
  if (n < 0) return fail(RQ_EINVAL, "%s: negative count n=%lld", who, (long long)n);
  if (nsplits < 1) return fail(RQ_EINVAL, "%s: nsplits=%d < 1", who, nsplits);
  if (!C || (n > 0 && (!codes || !X))) return fail(RQ_EINVAL, "%s: null pointer", who);
  return RQ_OK;
}

// hb: the codewords whose values are in LDS at a time -- h for the byte kernel, min(h, 256) for the 16-bit kernel, which adds
// the running lists of its VB vectors
size_t beam_stage_lds(int h, int Hi, int Hn, bool wide, int *VB_out, int *NT_out) {
  const int hb = wide ? std::min(h, 256) : h;
  const int NT = (hb + 31) / 32, VB = std::max(1, BM_ROWS / Hi);
  const int N = Hi * hb, NP = N + ((N + 63) >> 6);
  *VB_out = VB;
  *NT_out = NT;
  return ((size_t)2 * NT * BM_KC * 64 + (size_t)2 * BM_ROWS * BM_XSTR + (size_t)NT * 32 + (size_t)VB * NP) * 4 +
         (wide ? bm_run_bytes(VB, Hn) : 0);
}

// hb <= 256 and H_i <= 32 (beam_check): VB * NP <= 64 hb + hb + 64 words, so a workgroup never needs more than 109 KiB of
// slices and values; the 16-bit kernel adds VB * Hn <= 64 * 32 keys of 8 bytes (16 KiB, at H_i = 1): 125 KiB at the very most
static_assert(((size_t)2 * 8 * BM_KC * 64 + (size_t)2 * BM_ROWS * BM_XSTR + 8 * 32 + (64 * 256 + 256 + 64)) * 4 +
                      (size_t)BM_ROWS * BM_MAX_BEAM * 8 <= 160 * 1024,
              "beam stage: LDS of the largest shape");

// the dynamic LDS limit of a kernel variant is raised once per device
template <bool VEC4, class Code>
int beam_stage_attr() {
  static std::atomic<bool> done[64];
  int dev = 0;
  RQ_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !done[dev].load(std::memory_order_acquire)) {
    RQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(beam_stage_kernel<VEC4, Code>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
  }
  return RQ_OK;
}

template <class Code>
int beam_stage_launch(const BeamStage &p, hipStream_t s) {
  int VB, NT;
  const size_t lds = beam_stage_lds(p.h, p.Hi, p.Hn, sizeof(Code) == 2, &VB, &NT);
  BeamStage q = p;
  q.VB = VB;
  q.NT = NT;
  const bool vec4 = q.d % 4 == 0 && (((uintptr_t)q.R | (uintptr_t)q.Ci) & 15) == 0;
  RQ_TRY(vec4 ? (beam_stage_attr<true, Code>()) : (beam_stage_attr<false, Code>()));
  const int64_t grid = (q.nvec + VB - 1) / VB;
  if (vec4) hipLaunchKernelGGL((beam_stage_kernel<true, Code>), dim3((unsigned)grid), dim3(256), lds, s, q);
  else hipLaunchKernelGGL((beam_stage_kernel<false, Code>), dim3((unsigned)grid), dim3(256), lds, s, q);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

// The device body: arguments already checked, n > 0.  X is only read.  Code = uint8_t (h <= 256) or int16_t; codes zero-based.
template <class Code>
int beam_encode_dev(Code *codes, float *Xr_out, float *cost_out, const float *X, const float *C, int64_t n, int d, int m,
                    int h, int H, int nsplits, hipStream_t s, BeamClock &clk) {
  // per vector: two beams of H rows and prefixes, one selection list (4 + sizeof(Code) + 1 bytes per survivor)
  const size_t res_v = (size_t)H * d * 4, pre_v = (size_t)H * m * sizeof(Code), per_v = 2 * res_v + 2 * pre_v + (size_t)H * 8;
  if (per_v > BEAM_SCRATCH_BYTES)
    return fail(RQ_EUNSUPPORTED, "beam encode: the beams of one vector (H=%d, d=%d, m=%d) need %zu B, more than the %zu B of scratch",
                H, d, m, per_v, BEAM_SCRATCH_BYTES);
  int64_t chunk = (n + nsplits - 1) / nsplits;
  chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t)(BEAM_SCRATCH_BYTES / per_v)));
  chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, LAUNCH_MAX_THREADS / 64 / H));   // beam_expand_kernel: a wavefront per beam row
  void *wsa = nullptr, *wb = nullptr;
  RQ_TRY(workspace(WS_ICM_BIN, (size_t)m * h * 4, &wsa, s));
  RQ_TRY(workspace(WS_ICM_U, (size_t)chunk * per_v + 64, &wb, s));
  float *sa = (float *)wsa;
  float *Rb[2] = {(float *)wb, (float *)wb + (size_t)chunk * H * d};
  float *selV = Rb[1] + (size_t)chunk * H * d;
  Code *Pb[2] = {(Code *)(selV + (size_t)chunk * H), nullptr};
  Pb[1] = Pb[0] + (size_t)chunk * H * m;
  Code *selK = Pb[1] + (size_t)chunk * H * m;
  uint8_t *selP = (uint8_t *)(selK + (size_t)chunk * H);
  RQ_TRY(icm_sqnorm_launch(sa, C, m, h, d, s));
  clk.mark(BP_OTHER);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nv = std::min(chunk, n - r0);
    const float *R = X + (size_t)r0 * d;
    const Code *P = nullptr;
    int Hi = 1;
    for (int i = 0; i < m; ++i) {
      const int Hn = (int)std::min<int64_t>(H, (int64_t)Hi * h);
      const float *Ci = C + (size_t)i * h * d;
      BeamStage st;
      st.R = R; st.Ci = Ci; st.sa = sa + (size_t)i * h;
      st.selP = selP; st.selK = selK; st.selV = selV;
      st.nvec = nv; st.d = d; st.h = h; st.Hi = Hi; st.Hn = Hn; st.VB = 0; st.NT = 0;
      RQ_TRY(beam_stage_launch<Code>(st, s));
      clk.mark(BP_STAGE);
      const bool last = i + 1 == m;
      const int Hout = last ? 1 : Hn;
      float *Rn = last ? (Xr_out ? Xr_out + (size_t)r0 * d : nullptr) : Rb[i & 1];
      Code *Pn = last ? codes + (size_t)r0 * m : Pb[i & 1];
      float *cost = last && cost_out ? cost_out + r0 : nullptr;
      const int64_t orows = nv * Hout;
      hipLaunchKernelGGL(beam_expand_kernel<Code>, dim3((unsigned)((orows + 3) / 4)), dim3(256), 0, s, Rn, Pn, cost, R, P, Ci,
                         (const uint8_t *)selP, (const Code *)selK, (const float *)selV, nv, d, m, i, Hi, Hn, Hout);
      RQ_HIP(hipGetLastError());
      clk.mark(BP_EXPAND);
      R = Rn;
      P = Pn;
      Hi = Hn;
    }
  }
  return RQ_OK;
}

}  // namespace

}  // namespace rq

using namespace rq;

extern "C" {

int rq_dev_encode_rvq_beam(uint8_t *codes, float *Xr_out, float *cost_out, const float *X, const float *codebooks, int64_t n,
                           int d, int m, int h, int H, int nsplits, void *stream) {
  RQ_TRY(beam_check("rq_dev_encode_rvq_beam", codes, X, codebooks, n, d, m, h, H, nsplits));
  BeamClock &clk = beam_clock();
  clk.clear();
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  clk.start((hipStream_t)stream);
  return beam_encode_dev(codes, Xr_out, cost_out, X, codebooks, n, d, m, h, H, nsplits, (hipStream_t)stream, clk);
}

static int host_encode_rvq_beam(uint8_t *codes, int16_t *codes1, const float *X, const float *C, int64_t n, int d, int m, int h,
                                int H, int nsplits, float *cost_out, float *Xr_out, const char *who) {
  RQ_TRY(beam_check(who, codes ? (const void *)codes : (const void *)codes1, X, C, n, d, m, h, H, nsplits));
  BeamClock &clk = beam_clock();
  clk.clear();
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  // rows go through the device in chunks of at most 1 GiB of X, as rq_encode_rvq
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (1LL << 30) / ((int64_t)d * 4)));
  DevMem dX, dC, dcodes, d16, dXr, dcost;
  RQ_TRY(dX.alloc((size_t)chunk * d * 4));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  RQ_TRY(dcodes.alloc((size_t)chunk * m));
  if (codes1) RQ_TRY(d16.alloc((size_t)chunk * m * 2));
  if (Xr_out) RQ_TRY(dXr.alloc((size_t)chunk * d * 4));
  if (cost_out) RQ_TRY(dcost.alloc((size_t)chunk * 4));
  RQ_HIP(hipMemcpy(dC.p, C, (size_t)m * h * d * 4, hipMemcpyHostToDevice));
  clk.start(nullptr);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nr = std::min(chunk, n - r0);
    RQ_HIP(hipMemcpy(dX.p, X + (size_t)r0 * d, (size_t)nr * d * 4, hipMemcpyHostToDevice));
    clk.mark(BP_OTHER);
    RQ_TRY(beam_encode_dev(dcodes.as<uint8_t>(), Xr_out ? dXr.as<float>() : nullptr, cost_out ? dcost.as<float>() : nullptr,
                           dX.as<float>(), dC.as<float>(), nr, d, m, h, H, nsplits, nullptr, clk));
    if (codes1) RQ_TRY(widen_codes_launch(d16.as<int16_t>(), dcodes.as<uint8_t>(), nr * m, nullptr));
    RQ_HIP(hipDeviceSynchronize());
    if (codes1) RQ_HIP(hipMemcpy(codes1 + (size_t)r0 * m, d16.p, (size_t)nr * m * 2, hipMemcpyDeviceToHost));
    else RQ_HIP(hipMemcpy(codes + (size_t)r0 * m, dcodes.p, (size_t)nr * m, hipMemcpyDeviceToHost));
    if (Xr_out) RQ_HIP(hipMemcpy(Xr_out + (size_t)r0 * d, dXr.p, (size_t)nr * d * 4, hipMemcpyDeviceToHost));
    if (cost_out) RQ_HIP(hipMemcpy(cost_out + r0, dcost.p, (size_t)nr * 4, hipMemcpyDeviceToHost));
    clk.mark(BP_OTHER);
  }
  clk.collect();
  return RQ_OK;
}

int rq_encode_rvq_beam(uint8_t *codes, const float *X, const float *codebooks, int64_t n, int d, int m, int h, int H,
                       int nsplits, float *cost_out, float *Xr_out) {
  return host_encode_rvq_beam(codes, nullptr, X, codebooks, n, d, m, h, H, nsplits, cost_out, Xr_out, "rq_encode_rvq_beam");
}

int rq_encode_rvq_beam_i16(int16_t *codes1, const float *X, const float *codebooks, int64_t n, int d, int m, int h, int H,
                           int nsplits, float *cost_out, float *Xr_out) {
  return host_encode_rvq_beam(nullptr, codes1, X, codebooks, n, d, m, h, H, nsplits, cost_out, Xr_out,
                              "rq_encode_rvq_beam_i16");
}

// ---- more than 256 codewords per stage: int16 codes, zero-based on the device ------------------------
int rq_dev_encode_rvq_beam_wide(int16_t *codes, float *Xr_out, float *cost_out, const float *X, const float *codebooks, int64_t n,
                                int d, int m, int h, int H, int nsplits, void *stream) {
  RQ_TRY(beam_check("rq_dev_encode_rvq_beam_wide", codes, X, codebooks, n, d, m, h, H, nsplits, true, 0));
  BeamClock &clk = beam_clock();
  clk.clear();
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  clk.start((hipStream_t)stream);
  return beam_encode_dev<int16_t>(codes, Xr_out, cost_out, X, codebooks, n, d, m, h, H, nsplits, (hipStream_t)stream, clk);
}

int rq_encode_rvq_beam_wide(int16_t *codes, const float *X, const float *codebooks, int64_t n, int d, int m, int h, int H,
                            int nsplits, int code_base, float *cost_out, float *Xr_out) {
  RQ_TRY(beam_check("rq_encode_rvq_beam_wide", codes, X, codebooks, n, d, m, h, H, nsplits, true, code_base));
  BeamClock &clk = beam_clock();
  clk.clear();
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  // rows go through the device in chunks of at most 1 GiB of X, as rq_encode_rvq_beam
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (1LL << 30) / ((int64_t)d * 4)));
  DevMem dX, dC, dcodes, dXr, dcost;
  RQ_TRY(dX.alloc((size_t)chunk * d * 4));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  RQ_TRY(dcodes.alloc((size_t)chunk * m * 2));
  if (Xr_out) RQ_TRY(dXr.alloc((size_t)chunk * d * 4));
  if (cost_out) RQ_TRY(dcost.alloc((size_t)chunk * 4));
  RQ_HIP(hipMemcpy(dC.p, codebooks, (size_t)m * h * d * 4, hipMemcpyHostToDevice));
  clk.start(nullptr);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nr = std::min(chunk, n - r0);
    RQ_HIP(hipMemcpy(dX.p, X + (size_t)r0 * d, (size_t)nr * d * 4, hipMemcpyHostToDevice));
    clk.mark(BP_OTHER);
    RQ_TRY(beam_encode_dev<int16_t>(dcodes.as<int16_t>(), Xr_out ? dXr.as<float>() : nullptr,
                                    cost_out ? dcost.as<float>() : nullptr, dX.as<float>(), dC.as<float>(), nr, d, m, h, H,
                                    nsplits, nullptr, clk));
    if (code_base) RQ_TRY(add_base_codes_launch(dcodes.as<int16_t>(), nr * m, code_base, nullptr));
    RQ_HIP(hipDeviceSynchronize());
    RQ_HIP(hipMemcpy(codes + (size_t)r0 * m, dcodes.p, (size_t)nr * m * 2, hipMemcpyDeviceToHost));
    if (Xr_out) RQ_HIP(hipMemcpy(Xr_out + (size_t)r0 * d, dXr.p, (size_t)nr * d * 4, hipMemcpyDeviceToHost));
    if (cost_out) RQ_HIP(hipMemcpy(cost_out + r0, dcost.p, (size_t)nr * 4, hipMemcpyDeviceToHost));
    clk.mark(BP_OTHER);
  }
  clk.collect();
  return RQ_OK;
}

int rq_last_beam_timing(double *ms, int cap) {
  if (!ms) return fail(RQ_EINVAL, "rq_last_beam_timing: null pointer");
  BeamClock &clk = beam_clock();
  clk.collect();
  for (int q = 0; q < cap && q < BP_N; ++q) ms[q] = clk.ms[q];
  return RQ_OK;
}

}  // extern "C"
