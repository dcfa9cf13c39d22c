// rq_encode_bytes.hip -- quantize_pq / quantize_opq (src/PQ.jl:18-48, src/OPQ.jl:19-27) on BYTE rows.
//
// bvecs files (SIFT1B: bigann_base / learn / query) hold UInt8 vectors (bvecs_read, src/xvecs_read.jl:14-52); the reference
// widens them to Float32 on the host before it encodes (src/read_datasets.jl:148-167).  Here the bytes travel as bytes -- a
// quarter of the PCIe traffic of a host-pointer call, a quarter of the HBM of a resident base -- and are widened in
// registers.  u8 -> f32 is exact, so the answer is DEFINED as the codes (the rotated rows) of the widened matrix, bit for bit,
// and the oracle of the f32 entry points serves unchanged.
//
//   PQ, even sub-space widths <= 16    encode_pq_filter_bytes_kernel + encode_pq_fix_bytes_kernel (rq_encode_filter.hip): the f32
//                                      kernels with byte loaders
//   OPQ, d in {32, 64, 96, 128}        rotate_bytes_kernel_v2 (below: rotate_kernel_v2 of rq_encode.hip with byte loaders) writes
//                                      f32 R'X of a chunk of rows into scratch; the f32 encode reads it
//   everything else                    widen_bytes_kernel writes the f32 rows of a chunk into scratch; the f32 launch follows
// The scratch (WS_TMP of the stream) holds bytes_chunk_rows(d) = max(32768, 2^25 / d) rows -- at most 128 MiB per buffer --
// whatever n is.  All row offsets are size_t: n d exceeds 2^32 for the bases this is for.
#include "rq_encode_split.h"

namespace rq {

int64_t bytes_chunk_rows(int d) { return std::max<int64_t>(32768, (1LL << 25) / std::max(1, d)); }

// ---- u8 -> f32 rows (the fallback) -----------------------------------------------------------------------------------
// one thread per 4 elements; out is library scratch (256-byte aligned), in has any alignment
__global__ __launch_bounds__(256) void widen_bytes_kernel(float *out, const uint8_t *in, size_t nelem) {
  const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= nelem) return;
  uint32_t w[1];
  float x[4];
  if (e + 4 <= nelem) {
    load_bytes<4>(in + e, byte_align(in, 4, 4), 4, w);
    bytes_f32<4>(w, x);
    *reinterpret_cast<float4 *>(out + e) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
    load_bytes<4>(in + e, 1, (int)(nelem - e), w);
    bytes_f32<4>(w, x);
    for (int s = 0; s < (int)(nelem - e); ++s) out[e + s] = x[s];
  }
}

int widen_bytes_launch(float *out, const uint8_t *in, size_t nelem, hipStream_t stream) {
  if (nelem == 0) return RQ_OK;
  const size_t nthreads = (nelem + 3) / 4;
  hipLaunchKernelGGL(widen_bytes_kernel, dim3((uint32_t)((nthreads + 255) / 256)), dim3(256), 0, stream, out, in, nelem);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

// ---- rotation ----------------------------------------------------------------------------------------------------------
struct RotBytesParams {
  const float *R;    // [d][d]  Rc[i][k]
  const uint8_t *X;  // [n][d], any alignment
  float *RX;         // [n][d]
  int64_t n;
};

// rotate_kernel_v2 (rq_encode.hip) on byte rows: the same A fragments of R in LDS, the same chain of 32x32x2 f32 MFMAs over
// k = 0..d-1 from +0 -- so R'X is bit for bit that of the widened rows -- and the same stores.  Only the loads differ: lane
// (j, hi) holds the 4-byte pieces X[j][8q + 4hi .. +3] (one register each in flight instead of four) and widens them when
// the tile's turn comes.  The pieces sit at X + row D + 8q + 4hi with D % 8 == 0: 4-byte loads when X is 4-byte aligned,
// else 2-byte or single-byte loads.
template <int KK, int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void rotate_bytes_kernel_v2(RotBytesParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int D = 2 * KK, NT = (D + 31) / 32, NP = D / 8;   // NP 4-byte pieces per lane
  float *RA = reinterpret_cast<float *>(smem);                 // NT*KK*64
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, hi = lane >> 5;
  for (int idx = tid; idx < NT * KK * 64; idx += NWAVES * 64) {
    const int l = idx & 63;
    const int kk = (idx >> 6) % KK, t = (idx >> 6) / KK;
    const int i = t * 32 + (l & 31), k = 2 * kk + (l >> 5);
    RA[idx] = (i < D) ? p.R[(size_t)i * D + k] : 0.0f;
  }
  __syncthreads();
  const int64_t ntiles = (p.n + 31) / 32;
  const int64_t total_waves = (int64_t)gridDim.x * NWAVES;
  const int64_t tile0 = (int64_t)blockIdx.x * NWAVES + wave;
  const int al = byte_align(p.X, D, 4);
  uint32_t nx[NP];
  auto gload = [&](int64_t tile) {
    int64_t gr = tile * 32 + j;
    if (gr >= p.n) gr = p.n - 1;
    const uint8_t *src = p.X + (size_t)gr * D + 4 * hi;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      uint32_t w[1];
      load_bytes<4>(src + 8 * q, al, 4, w);
      nx[q] = w[0];
    }
  };
  if (tile0 < ntiles) gload(tile0);
  for (int64_t tile = tile0; tile < ntiles; tile += total_waves) {
    const int64_t row0 = tile * 32;
    float b[KK];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      float x = byte_f32<0>(&nx[q]), y = byte_f32<1>(&nx[q]), z = byte_f32<2>(&nx[q]), w = byte_f32<3>(&nx[q]);
      swap32(x, y);   // x: dims (8q, 8q+1) = k-step 4q      y: dims (8q+4, 8q+5) = k-step 4q+2
      swap32(z, w);   // z: dims (8q+2, 8q+3) = k-step 4q+1  w: dims (8q+6, 8q+7) = k-step 4q+3
      b[4 * q + 0] = x; b[4 * q + 1] = z; b[4 * q + 2] = y; b[4 * q + 3] = w;
    }
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      if (t == NT - 1 && tile + total_waves < ntiles) gload(tile + total_waves);
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
      const float *ra = RA + (size_t)t * KK * 64 + lane;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[kk * 64], b[kk], acc, 0, 0, 0);
      if (row0 + j < p.n) {
        float *o = p.RX + (size_t)(row0 + j) * D;
        const int ibase = t * 32 + 4 * hi;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int i0 = ibase + 8 * g4;
          if (i0 < D)
            *reinterpret_cast<float4 *>(o + i0) =
                make_float4(acc[g4 * 4 + 0], acc[g4 * 4 + 1], acc[g4 * 4 + 2], acc[g4 * 4 + 3]);
        }
      }
    }
  }
}

template <int KK>
static int launch_rotate_bytes_v2(const RotBytesParams &p, int num_cu, hipStream_t stream) {
  constexpr int NW = 8;      // as launch_rotate_v2 (rq_encode.hip)
  constexpr int NT = (2 * KK + 31) / 32;
  const size_t lds = (size_t)NT * KK * 64 * sizeof(float);
  auto kern = rotate_bytes_kernel_v2<KK, NW>;
  RQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t ntiles = (p.n + 31) / 32;
  const int grid = (int)std::min<int64_t>(num_cu, (ntiles + NW - 1) / NW);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NW * 64), lds, stream, p);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

// the widths rotate_launch gives to rotate_kernel_v2 (RX is 16-byte aligned there and here: float4 stores)
static bool rotate_bytes_covers(int d) {
  return tuning("ROT_V2", 1) && (d == 32 || d == 64 || d == 96 || d == 128);
}

// RX [n][d] <- R' x_j of n byte rows.  `wide` is f32 scratch of n d floats for the fallback (widen, then rotate_launch); it
// may be null when rotate_bytes_covers(d).
static int rotate_bytes_piece(float *RX, const float *R, const uint8_t *X, int d, int64_t n, int num_cu, hipStream_t stream,
                              float *wide) {
  if (rotate_bytes_covers(d)) {
    RotBytesParams p{R, X, RX, n};
    switch (d) {
      case 32: return launch_rotate_bytes_v2<16>(p, num_cu, stream);
      case 64: return launch_rotate_bytes_v2<32>(p, num_cu, stream);
      case 96: return launch_rotate_bytes_v2<48>(p, num_cu, stream);
      default: return launch_rotate_bytes_v2<64>(p, num_cu, stream);
    }
  }
  RQ_TRY(widen_bytes_launch(wide, X, (size_t)n * d, stream));
  return rotate_launch(RX, R, wide, d, n, num_cu, stream);
}

int rotate_bytes_launch(float *RX, const float *R, const uint8_t *X, int d, int64_t n, int num_cu, hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  if (rotate_bytes_covers(d)) return rotate_bytes_piece(RX, R, X, d, n, num_cu, stream, nullptr);
  const int64_t chunk = std::min<int64_t>(n, bytes_chunk_rows(d));
  void *tmp = nullptr;
  RQ_TRY(workspace(WS_TMP, (size_t)chunk * d * sizeof(float), &tmp, stream));
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nr = std::min(chunk, n - r0);
    RQ_TRY(rotate_bytes_piece(RX + (size_t)r0 * d, R, X + (size_t)r0 * d, d, nr, num_cu, stream, (float *)tmp));
  }
  return RQ_OK;
}

// ---- encode --------------------------------------------------------------------------------------------------------------
int encode_bytes_launch(uint8_t *codes, const uint8_t *X, const float *R, const float *C, int64_t n, int d, int m, int h,
                        int num_cu, hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  // (the checks of encode_launch, so that every path answers a bad shape alike)
  if (m < 1 || m > 32) return fail(RQ_EUNSUPPORTED, "encode covers 1 <= m <= 32; got m=%d", m);
  if (h < 1 || h > 256) return fail(RQ_EUNSUPPORTED, "encode emits uint8 codes: 1 <= h <= 256; got h=%d", h);
  if (d < m) return fail(RQ_EINVAL, "d=%d < m=%d", d, m);
  if (!R && encode_filter_bytes_covers(d, m)) return encode_filter_bytes(codes, X, C, n, d, m, h, num_cu, stream);
  // f32 rows of a chunk in scratch -- R'X, or the widened rows (then also the rotation's input) -- and the f32 launch
  const int64_t chunk = std::min<int64_t>(n, bytes_chunk_rows(d));
  const size_t buf = ((size_t)chunk * d * sizeof(float) + 255) & ~(size_t)255;
  const bool two = R && !rotate_bytes_covers(d);      // the rotation's fallback wants the widened rows AND R'X
  void *tmp = nullptr;
  RQ_TRY(workspace(WS_TMP, buf * (two ? 2 : 1), &tmp, stream));
  float *rows = (float *)tmp;
  float *wide = two ? (float *)((unsigned char *)tmp + buf) : nullptr;
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nr = std::min(chunk, n - r0);
    const uint8_t *xb = X + (size_t)r0 * d;
    if (R) RQ_TRY(rotate_bytes_piece(rows, R, xb, d, nr, num_cu, stream, wide));
    else RQ_TRY(widen_bytes_launch(rows, xb, (size_t)nr * d, stream));
    RQ_TRY(encode_launch(codes + (size_t)r0 * m, rows, C, nr, d, m, h, num_cu, stream));
  }
  return RQ_OK;
}

}  // namespace rq
