// rq_encode_h16.hip -- quantize_pq / quantize_opq / quantize_rvq with MORE than 256 codewords per codebook (16-bit codes).
//
// The reference returns Matrix{Int16} (src/PQ.jl:45-47, src/RVQ.jl:60-62) so that a codebook may hold up to 32767 entries.  The
// kernels of rq_encode.hip keep a whole sub-codebook in LDS, carry the winner as a tile index and pack one byte per code; none
// of that stretches.  encode_h16_kernel streams the codebook instead.  Arithmetic and contract are those at the top of
// rq_encode.hip (oracle/rq_oracle.c:264-328): g, sa, sb k-ordered fmaf chains from +0 -- v_mfma_f32_32x32x2_f32 is that chain --
// u_k = fl(fl(sa_k + sb) - 2 g_k), v_k = u_k > 0 ? u_k : 0 (a NaN u_k becomes 0), code = first index of the minimum, strict '<'.
//
// Work is one flat sequence of positions (tile group, sub-quantizer i, codeword block, k-chunk), the k-chunk innermost:
//   codeword block   256 codewords = NT = 8 tiles of 32: the 128 accumulator registers a wavefront keeps across the k-chunks
//   k-chunk          KC = 8 k-steps (16 dimensions) of the sub-space; its 8 x 8 x 64 floats of the codebook, in A-fragment
//                    order, and the block's 256 norms go to one half of a double-buffered LDS area while the other half feeds
//                    the MFMAs (as encode_wide_kernel of rq_encode.hip does for h <= 256)
//   X                every wavefront stages the 32 x 16 slice of its own tile.  A sub-space of at most 16 dimensions (the PQ
//                    shapes) is one chunk, and the staged slice then serves all codeword blocks: X is read once.  Wider
//                    sub-spaces re-read their slices once per codeword block (h / 256 reads of X, from L2).
//                    Row = uint8_t (bvecs rows): the same slice from BYTES -- lane (row l / 2, dimensions
//                    8 (l & 1) .. + 7) takes one piece of up to 8 bytes with the widest loads X, d and the splitarray offsets
//                    and widths allow (all may be odd: down to single bytes) and widens it in registers (v_cvt_f32_ubyte*,
//                    exact) when the tile is stored.  The staged tile holds the very floats the f32 loader stages from
//                    the widened matrix, and nothing after the tile knows the difference.
// After the last k-chunk of a block the block's winner (clamped value, global index) is folded into the wavefront's running
// pair per vector.  Blocks come in ascending order and the pair is replaced on a strict '<' only, so a codeword duplicated at
// k and k + 256 loses to the lower index; the pair starts at (+Inf, 0), so a row of +Inf values gets index 0.
// Padded codewords (the last tile of the last block; h = 257 leaves a block of ONE live codeword) have zero coordinates and
// norm +Inf, and are masked to +Inf after the clamp: a NaN product of a padded codeword (0 * Inf) must not win through the clamp.
// |c_k|^2 of all m * h codewords is computed once per call into the stream's workspace (WS_H16_SA; 4 MB at m = 32, h = 32767).
#include "rq_internal.h"
#include "rq_encode_split.h"

namespace rq {

struct H16Params {
  const void *X;     // [n][d] float, or uint8_t at any byte alignment (encode_h16_kernel<uint8_t>)
  const float *C;    // concat of [h][sub_i]
  const float *sa;   // [m][h] |c_k|^2
  int16_t *codes;    // [n][m], zero-based
  int64_t n;
  int d, m, h;
  int off[33];       // splitarray offsets (src/utils.jl:179-203)
  int xal;           // byte rows: the load width 8, 4, 2 or 1 (see x_load_bytes)
};

constexpr int H16_NT = 8;      // tiles of 32 codewords per block
constexpr int H16_KC = 8;      // k-steps per chunk
constexpr int H16_NW = 8;      // wavefronts per workgroup
constexpr int H16_BLOCK = H16_NT * 32;

__global__ __launch_bounds__(256) void h16_norms_kernel(float *sa, const float *C, H16Params p) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.m * p.h) return;
  const int i = idx / p.h, k = idx - i * p.h;
  const int sub = p.off[i + 1] - p.off[i];
  const float *c = C + (size_t)p.h * p.off[i] + (size_t)k * sub;
  float acc = 0.0f;
  for (int s = 0; s < sub; ++s) acc = __builtin_fmaf(c[s], c[s], acc);
  sa[idx] = acc;
}

template <class Row>
__global__ __launch_bounds__(H16_NW * 64) void encode_h16_kernel(H16Params p) {
  constexpr bool BYTES = std::is_same<Row, uint8_t>::value;
  static_assert(BYTES || std::is_same<Row, float>::value, "rows are float or uint8_t");
  constexpr int NT = H16_NT, KC = H16_KC, NWAVES = H16_NW;
  constexpr int CHUNK = NT * KC * 64;                  // floats per staged codebook chunk
  constexpr int PER = CHUNK / (NWAVES * 64);           // ... per thread
  constexpr int DIMS = 2 * KC;                         // dimensions per chunk
  constexpr int RPI = 64 / DIMS;                       // rows one wave-wide X load covers
  constexpr int XL = 32 / RPI;                         // X loads per lane per chunk
  constexpr int XSTR = DIMS + 1;                       // padded row stride of the staged X tile
  constexpr int BUF = CHUNK + H16_BLOCK;               // one half of the double buffer: chunk + the block's norms
  static_assert(CHUNK % (NWAVES * 64) == 0 && 64 % DIMS == 0 && NWAVES * 64 >= H16_BLOCK, "chunk split");
  static_assert(!BYTES || DIMS == 16, "the byte loader gives a lane 8 of a row's 16 dimensions");
  __shared__ __attribute__((aligned(16))) float cb0[2 * BUF];
  __shared__ float xs_all[NWAVES * 32 * XSTR];
  const int m = p.m, h = p.h, d = p.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, hi = lane >> 5;
  float *xs = xs_all + wave * 32 * XSTR;
  const int nblocks = (h + H16_BLOCK - 1) / H16_BLOCK;
  const float INF = __uint_as_float(0x7f800000u);

  // element `e` of a staged chunk -> (tile t, k-step kk, lane l): codeword blk*256 + t*32 + (l & 31), dimension 2kk + (l >> 5)
  auto cb_load = [&](int i, int blk, int c, int e) -> float {
    const int l = e & 63;
    const int kk = (e >> 6) % KC;
    const int t = (e >> 6) / KC;
    const int sub = p.off[i + 1] - p.off[i];
    const int cen = blk * H16_BLOCK + t * 32 + (l & 31);
    const int s = c * DIMS + 2 * kk + (l >> 5);
    return (cen < h && s < sub) ? p.C[(size_t)h * p.off[i] + (size_t)cen * sub + s] : 0.0f;
  };
  // norm of codeword blk*256 + tid (threads 0..255), +Inf for a padded one; stored in C/D-fragment order
  auto sa_load = [&](int i, int blk) -> float {
    const int cen = blk * H16_BLOCK + tid;
    return (tid < H16_BLOCK && cen < h) ? p.sa[(size_t)i * h + cen] : INF;
  };
  const int sa_slot = ((tid >> 5) * 2 + ((tid >> 2) & 1)) * 16 + (tid & 3) + 4 * ((tid & 31) >> 3);
  // X slice of (tile group tg, sub-quantizer i, chunk c): lane -> (row u*RPI + lane/DIMS, dimension lane%DIMS);
  // rows past the end repeat the last one (their codes are never written)
  const int xdim = lane % DIMS, xrow_in = lane / DIMS;
  auto x_load = [&](int64_t tg, int i, int c, int u) -> float {
    const int sub = p.off[i + 1] - p.off[i];
    int64_t gr = (tg * NWAVES + wave) * 32 + u * RPI + xrow_in;
    if (gr >= p.n) gr = p.n - 1;
    const int sdim = c * DIMS + xdim;
    return sdim < sub ? static_cast<const float *>(p.X)[gr * d + p.off[i] + sdim] : 0.0f;
  };
  // the same slice of byte rows: lane -> (row lane / 2, dimensions 8 (lane & 1) .. + 7).  The piece starts at
  // X + row d + off_i + 16 c + 8 (lane & 1) and is nb = min(8, what is left of the sub-space) bytes long.  p.xal (host: the
  // largest power of two <= 8 that divides X, d and every sub-space offset and width, so also every piece's address and
  // length) is the load width, uniform over the launch: 1 dwordx2, 2 dwords, 4 ushorts or 8 ubytes, each predicated on lying
  // inside the piece -- nothing outside it is read.  The loads land RAW in r[]: packing and widening wait until the tile is
  // stored, behind the MFMAs, so that no ALU op makes the wavefront wait for them (or for the codebook chunk prefetched with
  // them) before the matrix work.
  const int brow = lane >> 1, bdim = 8 * (lane & 1);
  const int xal = p.xal;
  auto x_load_bytes = [&](int64_t tg, int i, int c, uint32_t (&r)[8]) {
    const int sub = p.off[i + 1] - p.off[i];
    int64_t gr = (tg * NWAVES + wave) * 32 + brow;
    if (gr >= p.n) gr = p.n - 1;
    const int s0 = c * DIMS + bdim;
    const int nb = sub - s0;           // bytes of the piece that exist (<= 0: none; >= 8: all)
    const uint8_t *src = static_cast<const uint8_t *>(p.X) + (size_t)gr * d + p.off[i] + s0;
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = 0u;
    if (xal >= 8) {
      if (nb > 0) { const uint2 v = *reinterpret_cast<const uint2 *>(src); r[0] = v.x; r[1] = v.y; }
    } else if (xal == 4) {
#pragma unroll
      for (int q = 0; q < 2; ++q) if (4 * q < nb) r[q] = *reinterpret_cast<const uint32_t *>(src + 4 * q);
    } else if (xal == 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) if (2 * q < nb) r[q] = *reinterpret_cast<const uint16_t *>(src + 2 * q);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) if (q < nb) r[q] = src[q];
    }
  };
  auto x_store_bytes = [&](const uint32_t (&r)[8]) {
    uint32_t w[2];
    if (xal >= 4) { w[0] = r[0]; w[1] = r[1]; }
    else if (xal == 2) { w[0] = r[0] | (r[1] << 16); w[1] = r[2] | (r[3] << 16); }
    else {
      w[0] = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
      w[1] = r[4] | (r[5] << 8) | (r[6] << 16) | (r[7] << 24);
    }
    float x[8];
    bytes_f32<8>(w, x);
#pragma unroll
    for (int s = 0; s < 8; ++s) xs[brow * XSTR + bdim + s] = x[s];
  };

  const int64_t ntiles = (p.n + 31) / 32;
  const int64_t ngroups = (ntiles + NWAVES - 1) / NWAVES;
  int64_t tg = blockIdx.x;
  int i = 0, blk = 0, c = 0;
  if (tg >= ngroups) return;
#pragma unroll
  for (int u = 0; u < PER; ++u) cb0[tid + u * NWAVES * 64] = cb_load(0, 0, 0, tid + u * NWAVES * 64);
  if (tid < H16_BLOCK) cb0[CHUNK + sa_slot] = sa_load(0, 0);
  if constexpr (BYTES) {
    uint32_t r[8];
    x_load_bytes(tg, 0, 0, r);
    x_store_bytes(r);
  } else {
#pragma unroll
    for (int u = 0; u < XL; ++u) xs[(u * RPI + xrow_in) * XSTR + xdim] = x_load(tg, 0, 0, u);
  }
  __syncthreads();

  f32x16 acc[NT];
  float sb = 0.0f;
  float run_v = INF;     // the vector's best clamped value over the blocks so far, and its global index
  int run_i = 0;
  int buf = 0;
#pragma unroll 1
  for (;;) {
    const int sub = p.off[i + 1] - p.off[i];
    const int nchunks = (sub + DIMS - 1) / DIMS;
    // the position after this one in the flat sequence
    int64_t ntg = tg;
    int ni = i, nblk = blk, nc = c + 1;
    if (nc == nchunks) {
      nc = 0; ++nblk;
      if (nblk == nblocks) { nblk = 0; ++ni; if (ni == m) { ni = 0; ntg += gridDim.x; } }
    }
    const bool more = ntg < ngroups;
    const bool newx = !(ntg == tg && ni == i && nc == c);    // a one-chunk sub-space keeps its staged slice across the blocks
    if (c == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
      sb = 0.0f;
      if (blk == 0) { run_v = INF; run_i = 0; }
    }
    float nxt[PER], xn[XL], nsa = INF;
    uint32_t xw[8];                          // byte rows: the lane's raw loads of the next slice, in place of xn
    if (more) {
#pragma unroll
      for (int u = 0; u < PER; ++u) nxt[u] = cb_load(ni, nblk, nc, tid + u * NWAVES * 64);
      nsa = sa_load(ni, nblk);
      if (newx) {
        if constexpr (BYTES) x_load_bytes(ntg, ni, nc, xw);
        else {
#pragma unroll
          for (int u = 0; u < XL; ++u) xn[u] = x_load(ntg, ni, nc, u);
        }
      }
    }
    const float *cb = cb0 + (size_t)buf * BUF + lane;
    float b[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
      const float x0 = xs[j * XSTR + 2 * kk], x1 = xs[j * XSTR + 2 * kk + 1];
      b[kk] = hi ? x1 : x0;
      sb = __builtin_fmaf(x0, x0, sb);      // chain s = 0..sub-1 (padded dimensions add fma(0, 0, sb) = sb)
      sb = __builtin_fmaf(x1, x1, sb);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int kk = 0; kk < KC; ++kk)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cb[(t * KC + kk) * 64], b[kk], acc[t], 0, 0, 0);
    }
    if (c + 1 == nchunks) {   // the sub-space is complete for this block: its winner, folded into the running pair
      const float4 *sa4 = reinterpret_cast<const float4 *>(cb0 + (size_t)buf * BUF + CHUNK + hi * 16);
      const int kbase = blk * H16_BLOCK;
      float bv = INF;
      int bt = 0;
      f32x2 vb[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) vb[r] = f32x2{0.0f, 0.0f};
      const f32x2 sb2 = {sb, sb}, m2 = {-2.0f, -2.0f}, z2 = {0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x2 v[8];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 sav = sa4[t * 8 + g4];
          const f32x2 s01 = {sav.x, sav.y}, s23 = {sav.z, sav.w};
          const f32x2 g01 = {acc[t][g4 * 4 + 0], acc[t][g4 * 4 + 1]}, g23 = {acc[t][g4 * 4 + 2], acc[t][g4 * 4 + 3]};
          // u = fl(fl(sa + sb) - 2 g)  (fma(-2, g, t) has the same bits: 2g is exact);  v = u > 0 ? u : 0 -- max(NaN, 0) = 0
          v[g4 * 2 + 0] = __builtin_elementwise_max(__builtin_elementwise_fma(m2, g01, s01 + sb2), z2);
          v[g4 * 2 + 1] = __builtin_elementwise_max(__builtin_elementwise_fma(m2, g23, s23 + sb2), z2);
        }
        if (kbase + t * 32 + 32 > h) {     // wave-uniform: the tile holds padded codewords
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = kbase + t * 32 + 4 * hi + 8 * (r >> 2) + (r & 3);
            if (k >= h) { if (r & 1) v[r >> 1].y = INF; else v[r >> 1].x = INF; }
          }
        }
        float m01 = __builtin_fminf(__builtin_fminf(v[0].x, v[0].y), v[1].x);
        float m02 = __builtin_fminf(__builtin_fminf(v[1].y, v[2].x), v[2].y);
        float m03 = __builtin_fminf(__builtin_fminf(v[3].x, v[3].y), v[4].x);
        float m04 = __builtin_fminf(__builtin_fminf(v[4].y, v[5].x), v[5].y);
        float m05 = __builtin_fminf(__builtin_fminf(v[6].x, v[6].y), v[7].x);
        float mm = __builtin_fminf(__builtin_fminf(m01, m02), m03);
        mm = __builtin_fminf(__builtin_fminf(mm, m04), m05);
        mm = __builtin_fminf(mm, v[7].y);
        if (mm < bv) {                      // strict: the earliest tile keeps a tie
          bv = mm;
          bt = t;
#pragma unroll
          for (int r = 0; r < 8; ++r) vb[r] = v[r];
        }
      }
      int rf = 15;
#pragma unroll
      for (int r = 14; r >= 0; --r) rf = (((r & 1) ? vb[r >> 1].y : vb[r >> 1].x) <= bv) ? r : rf;
      int bi = kbase + bt * 32 + 4 * hi + 8 * (rf >> 2) + (rf & 3);
      // the two half-waves hold disjoint codeword subsets of the same vector
      const float ov = __shfl_xor(bv, 32);
      const int oi = __shfl_xor(bi, 32);
      if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      if (bv < run_v) { run_v = bv; run_i = bi; }          // strict: an earlier block keeps a tie
      if (blk + 1 == nblocks) {
        const int64_t row = (tg * NWAVES + wave) * 32 + j;
        if (hi == 0 && row < p.n) p.codes[(size_t)row * m + i] = (int16_t)run_i;
      }
    }
    if (!more) break;
    {
      float *dstb = cb0 + (size_t)(buf ^ 1) * BUF;
#pragma unroll
      for (int u = 0; u < PER; ++u) dstb[tid + u * NWAVES * 64] = nxt[u];
      if (tid < H16_BLOCK) dstb[CHUNK + sa_slot] = nsa;
      if (newx) {                                                                     // this wave's own tile
        if constexpr (BYTES) x_store_bytes(xw);
        else {
#pragma unroll
          for (int u = 0; u < XL; ++u) xs[(u * RPI + xrow_in) * XSTR + xdim] = xn[u];
        }
      }
    }
    __syncthreads();
    buf ^= 1;
    tg = ntg; i = ni; blk = nblk; c = nc;
  }
}

// codes [n][m] int16 zero-based.  h <= 256: the kernels of rq_encode.hip into scratch, widened (the u8 entry points' codes by
// construction); above: the norms pass and encode_h16_kernel.  Everything on `stream`.
int h16_encode_check(int d, int m, int h) {
  if (m < 1 || m > 32) return fail(RQ_EUNSUPPORTED, "wide encode covers 1 <= m <= 32; got m=%d", m);
  if (h < 1 || h > RQ_MAX_H16) return fail(RQ_EUNSUPPORTED, "wide encode emits Int16 codes: 1 <= h <= %d; got h=%d", RQ_MAX_H16, h);
  if (d < m) return fail(RQ_EINVAL, "d=%d < m=%d", d, m);
  return RQ_OK;
}

// the norms pass and encode_h16_kernel<Row> (h > 256) on rows X [n][d] of Row
template <class Row>
static int h16_stream_launch(int16_t *codes, const Row *X, const float *C, int64_t n, int d, int m, int h, int num_cu,
                             hipStream_t stream) {
  H16Params p;
  p.X = X; p.C = C; p.codes = codes; p.n = n; p.d = d; p.m = m; p.h = h;
  split_offsets(p.off, d, m);
  p.xal = 8;
  if (std::is_same<Row, uint8_t>::value) {
    uint32_t mix = (uint32_t)(uintptr_t)X | (uint32_t)d | 8u;
    for (int i = 0; i < m; ++i) mix |= (uint32_t)p.off[i] | (uint32_t)(p.off[i + 1] - p.off[i]);
    p.xal = (int)(mix & (0u - mix));
  }
  void *sa = nullptr;
  RQ_TRY(workspace(WS_H16_SA, (size_t)m * h * sizeof(float), &sa, stream));
  p.sa = (const float *)sa;
  hipLaunchKernelGGL(h16_norms_kernel, dim3((uint32_t)((m * h + 255) / 256)), dim3(256), 0, stream, (float *)sa, C, p);
  RQ_HIP(hipGetLastError());
  const int64_t ngroups = ((n + 31) / 32 + H16_NW - 1) / H16_NW;
  const int grid = (int)std::min<int64_t>(num_cu, ngroups);
  hipLaunchKernelGGL(encode_h16_kernel<Row>, dim3(grid), dim3(H16_NW * 64), 0, stream, p);
  RQ_HIP(hipGetLastError());
  note_encode_h16_kernel();
  return RQ_OK;
}

int encode_h16_launch(int16_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int num_cu,
                      hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  RQ_TRY(h16_encode_check(d, m, h));
  if (h <= 256) {
    void *tmp = nullptr;
    RQ_TRY(workspace(WS_H16_CODES, (size_t)n * m, &tmp, stream));
    RQ_TRY(encode_launch((uint8_t *)tmp, X, C, n, d, m, h, num_cu, stream));
    return convert_codes_launch(codes, (const uint8_t *)tmp, n * m, 0, stream);
  }
  return h16_stream_launch<float>(codes, X, C, n, d, m, h, num_cu, stream);
}

// quantize_pq of BYTE rows at h > 256 (rq_encode_bytes.hip routes h <= 256 and the OPQ chunks): X at any byte alignment
int encode_h16_u8_launch(int16_t *codes, const uint8_t *X, const float *C, int64_t n, int d, int m, int h, int num_cu,
                         hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  RQ_TRY(h16_encode_check(d, m, h));
  if (h <= 256) return fail(RQ_EINVAL, "encode_h16_u8_launch is the h > 256 path; got h=%d", h);
  return h16_stream_launch<uint8_t>(codes, X, C, n, d, m, h, num_cu, stream);
}

// quantize_rvq (src/RVQ.jl:18-66) with 16-bit codes on resident data: stage_codes is n int16 of scratch, counts [m][h] or NULL
int rvq_h16_encode_launch(int16_t *codes, float *Xr, int16_t *stage_codes, unsigned int *counts, const float *C, int64_t n,
                          int d, int m, int h, int num_cu, hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  if (counts) RQ_HIP(hipMemsetAsync(counts, 0, (size_t)m * h * sizeof(unsigned int), stream));
  for (int i = 0; i < m; ++i) {
    const float *Ci = C + (size_t)i * h * d;
    unsigned int *cnt = counts ? counts + (size_t)i * h : nullptr;
    RQ_TRY(encode_h16_launch(stage_codes, Xr, Ci, n, d, 1, h, num_cu, stream));
    RQ_TRY(residual_launch(Xr, Xr, Ci, stage_codes, 1, codes, cnt, n, d, m, i, stream));
  }
  return RQ_OK;
}

}  // namespace rq
