// rq_icm_h16.hip -- LSQ encoding (encoding_icm, src/LSQ.jl:272-302) with up to RQ_MAX_H16 codewords per codebook: int16 codes,
// the contract of DESIGN.md section 2 at every h, kernel and numbers in DESIGN.md section 4.24.
//
// The byte encoder (rq_icm.hip) keeps a row's m unaries in registers, HS / 64 entries per lane and codebook: that grows with h.
// Here nothing does:
//   icm_pair_h16_kernel  once per call: binT[j][k][b][l] = 2 <c_jl, c_kb>, one row of HS = 64 * ceil(h / 64) floats per (j, k, b);
//                        a block computes a 64 x 64 tile of one (j, k) pair from LDS, every output its own k-ordered fmaf chain.
//                        Entries past h and the j == k rows are never written and never used.
//   icm_unary_launch     per chunk of rows, shared with rq_icm.hip: U[row][i][k] = fl(sa_i[k] - 2 <c_ik, x>).
//   icm_ils_h16_kernel   per chunk of rows, ONE launch for the whole ILS, one wavefront per row; codes, visit order and cost in
//                        registers.  A conditioning step streams the row's unary U[row][j][.] and the m - 1 gathered rows of binT in
//                        pieces of 64 lanes x 4 floats: the m loads of a piece are independent dwordx4 loads issued before the
//                        unfused adds (ascending k), every lane keeps a running (minimum, first index) with a strict < over its
//                        ascending pieces, and the (value, index) butterfly of the byte kernel ends the step.  Entries past h
//                        compare as +inf.  Perturbation, visit order, veccost and the accept test are the byte kernel's.
// The codes equal tests/icm_wide_oracle.py bit for bit, and rq_encode_icm's at h <= 256.
#include "rq_icm_shared.h"

#include <vector>

namespace rq {

namespace {

// block = the 64 x 64 tile (l0.., b0..) of one (j, k) pair, thread = 4 l x 4 b; PK dimensions at a time through LDS.  Every output
// is its own fmaf chain over t = 0 .. d-1 in order; a pad term (t >= d) is fma(0, 0, acc) = acc.
constexpr int PT = 64, PK = 16;
__global__ __launch_bounds__(256) void icm_pair_h16_kernel(float *binT, const float *C, int m, int h, int d, int HS) {
  __shared__ __attribute__((aligned(16))) float As[PK][PT + 4], Bs[PK][PT + 4];   // [t][l], [t][b]
  const int jk = blockIdx.z, k = jk % m, j = jk / m;
  if (j == k) return;
  const int l0 = blockIdx.x * PT, b0 = blockIdx.y * PT;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const float *Cj = C + (size_t)j * h * d, *Ck = C + (size_t)k * h * d;
  float acc[4][4];   // [b][l]
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[q][p] = 0.0f;
  for (int t0 = 0; t0 < d; t0 += PK) {
    for (int e = threadIdx.x; e < PT * PK; e += 256) {
      const int r = e / PK, t = e % PK;
      const bool tv = t0 + t < d;
      As[t][r] = (tv && l0 + r < h) ? Cj[(size_t)(l0 + r) * d + t0 + t] : 0.0f;
      Bs[t][r] = (tv && b0 + r < h) ? Ck[(size_t)(b0 + r) * d + t0 + t] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PK; ++t) {
      const float4 a = *reinterpret_cast<const float4 *>(&As[t][4 * tx]);
      const float4 b = *reinterpret_cast<const float4 *>(&Bs[t][4 * ty]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[q][p] = __builtin_fmaf(av[p], bv[q], acc[q][p]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int b = b0 + 4 * ty + q;
    if (b >= h) continue;
    float *o = binT + ((size_t)jk * h + b) * HS + l0 + 4 * tx;
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (l0 + 4 * tx + p < h) o[p] = 2.0f * acc[q][p];
  }
}

struct IcmWideParams {
  int16_t *codes_out;        // [nrows][m]   (may alias codes_in)
  const int16_t *codes_in;   // [nrows][m]   zero-based, < h
  float *cost_out;           // [nrows] or null
  const float *U;            // [nrows][m][HS]
  const float *binT;         // [m][m][h][HS]
  const float *X;            // [nrows][d]
  const float *C;            // [m][h][d]
  int64_t nrows, row_base, t0;
  uint64_t seed;
  int d, m, h, HS, ilsiter, icmiter, npert, randord;
};

constexpr int PIECE = 256;   // floats of a row one wavefront reads per step: 64 lanes x one dwordx4

template <int MB>
__global__ __launch_bounds__(256) void icm_ils_h16_kernel(IcmWideParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.nrows) return;
  const int m = p.m, h = p.h, HS = p.HS, d = p.d;
  const float *x = p.X + (size_t)row * d;
  const float *urow = p.U + (size_t)row * m * HS;
  int b[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) b[i] = i < m ? (int)p.codes_in[(size_t)row * m + i] : 0;
  float cost_old = icm_cost<MB>(b, x, p.C, d, m, h, lane);
  const uint64_t zs = icm_z(p.seed);
  const uint64_t grow = (uint64_t)(p.row_base + row);
#pragma unroll 1
  for (int it = 0; it < p.ilsiter; ++it) {
    const uint64_t t = (uint64_t)(p.t0 + it);
    // visit order pi_t: 4-bit entries packed in one word (no dynamically indexed register array)
    uint64_t perm = 0;
    for (int i = 0; i < m; ++i) perm |= (uint64_t)i << (4 * i);
    if (p.randord) {
      const uint64_t q = icm_z(zs ^ (t | (1ull << 63)));
      for (int i = m - 1; i >= 1; --i) {
        const uint32_t r = icm_scale(icm_z(q + (uint64_t)i), (uint32_t)(i + 1));
        const uint64_t vi = (perm >> (4 * i)) & 15, vr = (perm >> (4 * r)) & 15;
        perm &= ~((15ull << (4 * i)) | (15ull << (4 * r)));
        perm |= (vr << (4 * i)) | (vi << (4 * r));
      }
    }
    // perturbation: selection sampling of npert distinct positions, uniform new values
    int nb[MB];
    const uint64_t base = icm_z(icm_z(zs ^ t) ^ grow);
    int need = p.npert;
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      nb[i] = b[i];
      if (i < m) {
        const uint32_t r = icm_scale(icm_z(base + (uint64_t)i), (uint32_t)(m - i));
        if ((int)r < need) {
          --need;
          nb[i] = (int)icm_scale(icm_z(base + (uint64_t)(m + i)), (uint32_t)h);
        }
      }
    }
#pragma unroll 1
    for (int s = 0; s < p.icmiter; ++s) {
#pragma unroll 1
      for (int jj = 0; jj < m; ++jj) {
        const int j = (int)((perm >> (4 * jj)) & 15);
        const float *uj = urow + (size_t)j * HS;
        // the m - 1 gathered rows: the codes are the same in every lane, so the 64-bit row bases are scalars
        const float *g[MB];
#pragma unroll
        for (int k = 0; k < MB; ++k) {
          const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((j * m + k) * h + nb[k]);
          g[k] = p.binT + (size_t)r * HS;
        }
        float bv = __builtin_inff();
        int bi = 0x7fffffff;
#pragma unroll 1
        for (int i0 = 0; i0 < HS; i0 += PIECE) {
          const int idx = i0 + lane * 4;
          // a lane past the row's end reads the row's last four floats again: in bounds, and masked below (idx >= HS >= h)
          const int at = idx < HS ? idx : HS - 4;
          const float4 uv = *reinterpret_cast<const float4 *>(uj + at);
          float4 gv[MB];
#pragma unroll
          for (int k = 0; k < MB; ++k)
            if (k < m && k != j) gv[k] = *reinterpret_cast<const float4 *>(g[k] + at);
          float ub[4] = {uv.x, uv.y, uv.z, uv.w};
#pragma unroll
          for (int k = 0; k < MB; ++k)
            if (k < m && k != j) {
              ub[0] = ub[0] + gv[k].x; ub[1] = ub[1] + gv[k].y; ub[2] = ub[2] + gv[k].z; ub[3] = ub[3] + gv[k].w;
            }
          // first index of the minimum within the lane: ascending index, strict <; entries past h never win
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = idx + e < h ? ub[e] : __builtin_inff();
            if (v < bv) { bv = v; bi = idx + e; }
          }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const float ov = __shfl_xor(bv, off, 64);
          const int oi = __shfl_xor(bi, off, 64);
          if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        int res = __shfl(bi, 0, 64);
        if (res < 0 || res >= h) res = 0;   // only reachable with non-finite costs: keep the code in range
#pragma unroll
        for (int i = 0; i < MB; ++i)
          if (i == j) nb[i] = res;
      }
    }
    const float c = icm_cost<MB>(nb, x, p.C, d, m, h, lane);
    if (c < cost_old) {   // strict: an equal cost keeps the old codes
      cost_old = c;
#pragma unroll
      for (int i = 0; i < MB; ++i) b[i] = nb[i];
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < MB; ++i)
      if (i < m) p.codes_out[(size_t)row * m + i] = (int16_t)b[i];
    if (p.cost_out) p.cost_out[row] = cost_old;
  }
}

// what rq_icm_wide_plan reports and icm_encode_wide_dev runs
struct IcmWidePlan {
  int HS;
  size_t table_bytes;   // binaries + self-products
  size_t row_bytes;     // unaries of one row
  int64_t chunk, chunks;
};

// shape and counts in range (RQ_EINVAL), then the tables and four rows of unaries within ICM_SCRATCH_BYTES (RQ_EUNSUPPORTED)
int icm_wide_plan(IcmWidePlan *pl, int64_t n, int d, int m, int h, int nsplits) {
  if (m < 1 || m > ICM_MAX_M) return fail(RQ_EINVAL, "encode_icm_wide: m=%d outside 1..%d", m, ICM_MAX_M);
  if (h < 2 || h > RQ_MAX_H16) return fail(RQ_EINVAL, "encode_icm_wide: h=%d outside 2..%d", h, RQ_MAX_H16);
  if (d < 1) return fail(RQ_EINVAL, "encode_icm_wide: d=%d < 1", d);
  if (n < 0) return fail(RQ_EINVAL, "encode_icm_wide: negative count (n=%lld)", (long long)n);
  if (nsplits < 1) return fail(RQ_EINVAL, "encode_icm_wide: nsplits=%d < 1", nsplits);
  pl->HS = 64 * ((h + 63) / 64);
  pl->table_bytes = (size_t)m * m * h * pl->HS * 4 + (size_t)m * h * 4;
  pl->row_bytes = (size_t)m * pl->HS * 4;
  if (pl->table_bytes + 4 * pl->row_bytes > ICM_SCRATCH_BYTES)
    return fail(RQ_EUNSUPPORTED, "encode_icm_wide: the tables of m=%d, h=%d take %zu bytes; with four rows of unaries they must fit %zu",
                m, h, pl->table_bytes, ICM_SCRATCH_BYTES);
  const int64_t fit = (int64_t)((ICM_SCRATCH_BYTES - pl->table_bytes) / pl->row_bytes);
  pl->chunk = n == 0 ? 0 : std::max<int64_t>(1, std::min<int64_t>((n + nsplits - 1) / nsplits, fit));
  pl->chunks = n == 0 ? 0 : (n + pl->chunk - 1) / pl->chunk;
  return RQ_OK;
}

}  // namespace

// The device body: arguments already checked (icm_wide_plan passes), codes zero-based and in range.  Scratch: WS_ICM_BIN, WS_ICM_U.
// phase_ms (host-pointer callers; null under stream capture): ICM_PH_N milliseconds accumulated per phase, then the stream is idle.
int icm_encode_wide_dev(int16_t *codes_out, const int16_t *codes_in, float *cost_out, const float *X, const float *C, int64_t n,
                        int d, int m, int h, int ilsiter, int icmiter, int npert, int randord, uint64_t seed, int64_t t0,
                        int nsplits, hipStream_t stream, double *phase_ms) {
  if (n <= 0) return RQ_OK;
  IcmWidePlan pl;
  RQ_TRY(icm_wide_plan(&pl, n, d, m, h, nsplits));
  const size_t bin_bytes = pl.table_bytes - (size_t)m * h * 4;
  void *wbin = nullptr, *wu = nullptr;
  RQ_TRY(workspace(WS_ICM_BIN, pl.table_bytes, &wbin, stream));
  RQ_TRY(workspace(WS_ICM_U, (size_t)pl.chunk * pl.row_bytes, &wu, stream));
  float *binT = (float *)wbin, *sa = binT + bin_bytes / 4, *U = (float *)wu;
  // a zero-iteration encode is a veccost pass: the ILS kernel then reads neither the tables nor the unaries
  const bool tables = ilsiter > 0;
  if (tables) {
    const unsigned tiles = (unsigned)((h + PT - 1) / PT);
    RQ_LAUNCH(icm_pair_h16_kernel, dim3(tiles, tiles, (unsigned)(m * m)), dim3(256), 0, stream, binT, C, m, h, d, pl.HS);
    RQ_TRY(icm_sqnorm_launch(sa, C, m, h, d, stream));
  }
  PhaseClock clk(stream, phase_ms, phase_ms != nullptr);
  for (int64_t r0 = 0; r0 < n; r0 += pl.chunk) {
    const int64_t nr = std::min(pl.chunk, n - r0);
    if (tables) RQ_TRY(icm_unary_launch(U, X + (size_t)r0 * d, C, sa, nr, d, m, h, pl.HS, nullptr, stream));
    clk.mark(ICM_PH_UNARY);
    IcmWideParams p;
    p.codes_out = codes_out + (size_t)r0 * m;
    p.codes_in = codes_in + (size_t)r0 * m;
    p.cost_out = cost_out ? cost_out + r0 : nullptr;
    p.U = U; p.binT = binT; p.X = X + (size_t)r0 * d; p.C = C;
    p.nrows = nr; p.row_base = r0; p.t0 = t0; p.seed = seed;
    p.d = d; p.m = m; p.h = h; p.HS = pl.HS; p.ilsiter = ilsiter; p.icmiter = icmiter; p.npert = npert;
    p.randord = randord ? 1 : 0;
    const dim3 grid((unsigned)((nr + 3) / 4));
    if (m <= 4) RQ_LAUNCH(icm_ils_h16_kernel<4>, grid, dim3(256), 0, stream, p);
    else if (m <= 8) RQ_LAUNCH(icm_ils_h16_kernel<8>, grid, dim3(256), 0, stream, p);
    else RQ_LAUNCH(icm_ils_h16_kernel<16>, grid, dim3(256), 0, stream, p);
    clk.mark(ICM_PH_ILS);
  }
  clk.collect();
  return RQ_OK;
}

}  // namespace rq

using namespace rq;

extern "C" int rq_icm_wide_plan(int64_t n, int d, int m, int h, int nsplits, int64_t *out, int cap) {
  if (!out || cap < 0) return fail(RQ_EINVAL, "rq_icm_wide_plan: null pointer or negative cap");
  IcmWidePlan pl;
  RQ_TRY(icm_wide_plan(&pl, n, d, m, h, nsplits));
  const int64_t v[5] = {pl.HS, (int64_t)pl.table_bytes, (int64_t)pl.row_bytes, pl.chunk, pl.chunks};
  for (int q = 0; q < cap && q < 5; ++q) out[q] = v[q];
  return RQ_OK;
}

extern "C" int rq_encode_icm_wide(int16_t *codes_out, const int16_t *codes_in, float *cost_out, const float *X, const float *C,
                                  int64_t n, int d, int m, int h, int ilsiter, int icmiter, int npert, int randord,
                                  uint64_t seed, int64_t t0, int nsplits, int code_base) {
  IcmWidePlan pl;
  RQ_TRY(icm_wide_plan(&pl, n, d, m, h, nsplits));
  if (ilsiter < 0 || icmiter < 0 || t0 < 0)
    return fail(RQ_EINVAL, "encode_icm_wide: negative count (ilsiter=%d icmiter=%d t0=%lld)", ilsiter, icmiter, (long long)t0);
  if (npert < 0 || npert > m) return fail(RQ_EINVAL, "encode_icm_wide: npert=%d outside 0..m=%d", npert, m);
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "encode_icm_wide: code_base must be 0 or 1; got %d", code_base);
  if (n > 0 && (!codes_out || !codes_in || !X || !C)) return fail(RQ_EINVAL, "encode_icm_wide: null pointer");
  const size_t ne = (size_t)n * m;
  for (size_t e = 0; e < ne; ++e)
    if (codes_in[e] < code_base || codes_in[e] > h - 1 + code_base)
      return fail(RQ_EINVAL, "encode_icm_wide: code %d at [%lld][%lld] is outside %d..%d", codes_in[e], (long long)(e / m),
                  (long long)(e % m), code_base, h - 1 + code_base);
  icm_set_timing(0, 0);
  if (n == 0) return RQ_OK;
  Timer tt;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  std::vector<int16_t> hcodes(codes_in, codes_in + ne);   // zero-based on the way in, code_base added on the way out
  if (code_base)
    for (size_t e = 0; e < ne; ++e) hcodes[e] = (int16_t)(hcodes[e] - code_base);
  DevMem dX, dC, dcodes, dcost;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  RQ_TRY(dC.alloc((size_t)m * h * d * 4));
  RQ_TRY(dcodes.alloc(ne * 2));
  RQ_TRY(dcost.alloc((size_t)n * 4));
  RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dC.p, C, (size_t)m * h * d * 4, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dcodes.p, hcodes.data(), ne * 2, hipMemcpyHostToDevice));
  double ph_ms[ICM_PH_N] = {0, 0};
  RQ_TRY(icm_encode_wide_dev(dcodes.as<int16_t>(), dcodes.as<int16_t>(), cost_out ? dcost.as<float>() : nullptr, dX.as<float>(),
                             dC.as<float>(), n, d, m, h, ilsiter, icmiter, npert, randord, seed, t0, nsplits, nullptr, ph_ms));
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(hcodes.data(), dcodes.p, ne * 2, hipMemcpyDeviceToHost));
  for (size_t e = 0; e < ne; ++e) codes_out[e] = (int16_t)(hcodes[e] + code_base);
  if (cost_out) RQ_HIP(hipMemcpy(cost_out, dcost.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  icm_set_timing(ph_ms[ICM_PH_UNARY], tt.ms());
  return RQ_OK;
}
