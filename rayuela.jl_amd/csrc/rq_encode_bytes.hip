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
//   OPQ, d in {32, 64, 96, 128}        rotate_kernel_v2 of rq_encode.hip with the byte row loader (RowsU8) writes f32 R'X of a
//                                      chunk of rows into scratch; the f32 encode reads it
//   everything else                    widen_bytes_kernel writes the f32 rows of a chunk into scratch; the f32 launch follows
// More than 256 codewords per codebook (16-bit codes, encode_h16_bytes_launch below):
//   PQ                                 encode_h16_kernel<uint8_t> of rq_encode_h16.hip: the streaming kernel with a byte loader
//   OPQ                                R'X of a chunk into scratch as above, then the f32 streaming kernel on that chunk
//   h <= 256 through the wide entries  the byte paths above into scratch, widened: the codes of the uint8 entries bit for bit
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
// the widths rotate_launch gives to rotate_kernel_v2 (RX is 16-byte aligned there and here: float4 stores)
static bool rotate_bytes_covers(int d) {
  return tuning("ROT_V2", 1) && (d == 32 || d == 64 || d == 96 || d == 128);
}

// RX [n][d] <- R' x_j of n byte rows.  `wide` is f32 scratch of n d floats for the fallback (widen, then rotate_launch); it
// may be null when rotate_bytes_covers(d).
static int rotate_bytes_piece(float *RX, const float *R, const uint8_t *X, int d, int64_t n, int num_cu, hipStream_t stream,
                              float *wide) {
  if (rotate_bytes_covers(d)) return rotate_v2_launch(RX, R, X, true, d, n, num_cu, stream);
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

// codes [n][m] int16 zero-based of byte rows, 1 <= h <= RQ_MAX_H16; R null: quantize_pq, else quantize_opq.  On `stream`.
int encode_h16_bytes_launch(int16_t *codes, const uint8_t *X, const float *R, const float *C, int64_t n, int d, int m, int h,
                            int num_cu, hipStream_t stream) {
  if (n <= 0) return RQ_OK;
  RQ_TRY(h16_encode_check(d, m, h));
  if (h <= 256) {
    void *tmp = nullptr;
    RQ_TRY(workspace(WS_H16_CODES, (size_t)n * m, &tmp, stream));
    RQ_TRY(encode_bytes_launch((uint8_t *)tmp, X, R, C, n, d, m, h, num_cu, stream));
    return convert_codes_launch(codes, (const uint8_t *)tmp, n * m, 0, stream);
  }
  if (!R) return encode_h16_u8_launch(codes, X, C, n, d, m, h, num_cu, stream);
  // the chunk loop of encode_bytes_launch: R'X of a chunk in scratch, the f32 wide encode on it
  const int64_t chunk = std::min<int64_t>(n, bytes_chunk_rows(d));
  const size_t buf = ((size_t)chunk * d * sizeof(float) + 255) & ~(size_t)255;
  const bool two = !rotate_bytes_covers(d);
  void *tmp = nullptr;
  RQ_TRY(workspace(WS_TMP, buf * (two ? 2 : 1), &tmp, stream));
  float *rows = (float *)tmp;
  float *wide = two ? (float *)((unsigned char *)tmp + buf) : nullptr;
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nr = std::min(chunk, n - r0);
    RQ_TRY(rotate_bytes_piece(rows, R, X + (size_t)r0 * d, d, nr, num_cu, stream, wide));
    RQ_TRY(encode_h16_launch(codes + (size_t)r0 * m, rows, C, nr, d, m, h, num_cu, stream));
  }
  return RQ_OK;
}

}  // namespace rq
