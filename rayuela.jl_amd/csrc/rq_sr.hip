// rq_sr.hip -- LSQ++ (stochastic relaxations of LSQ) on gfx950: the SR-C / SR-D perturbations (src/SR_perturbations.jl:4-73
// apply_schedule, SR_D_perturb, SR_C_perturb) and the training loop (src/SR.jl:88-176 train_sr_cuda, :4-84 train_sr);
// contract in DESIGN.md section 2 ("SR noise").
//
//   sr_colsum_kernel     per (block of SR_ROWS rows, tile of 64 columns): f64 column sums of x (pass 1) or of (x - mean)^2
//                        (pass 2); 4 row lanes per column, each ascending in the row index, combined (0 + 1) + (2 + 3)
//   sr_colfinish_kernel  per column: the block partials added in ascending block order; pass 1 -> mean = sum / n,
//                        pass 2 -> sigma = (float)(sqrt(sum / (n - 1)) / div)
//   sr_perturb_kernel    Y = (float)((double)X + z * ((double)sigma[j] * scale)), z a counter-based standard normal
//                        variate of the global element index (sr_variate)
// No float atomics: the standard deviation is bitwise reproducible, and every f64 operation of the variate is a
// correctly rounded + - * / sqrt with contraction off, so tests/sr_oracle.py restates it bit for bit.
#include "rq_internal.h"

#include <math.h>

#include <vector>

namespace rq {

namespace {

constexpr int SR_ROWS = 1024;                       // rows per block of the column sums
constexpr uint64_t SR_DOMAIN = 0x53525F4E4F495345ull;   // "SR_NOISE": apart from the ICM streams of the same seed

__host__ __device__ __forceinline__ uint64_t sr_mix(uint64_t x) {   // splitmix64 (synth.splitmix64)
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

uint64_t sr_stream_key(uint64_t seed, int kind, int64_t call) {
  return sr_mix(sr_mix(sr_mix(seed) ^ SR_DOMAIN) ^ (2ull * (uint64_t)call + (uint64_t)kind));
}

// log of a positive normal x: x = f 2^e with f in [sqrt(1/2), sqrt(2)), s = (f - 1) / (f + 1),
// log f = 2 s (1 + s^2/3 + ... + s^20/21) by Horner, plus e ln2
__device__ __forceinline__ double sr_log(double x) {
#pragma clang fp contract(off)
  const uint64_t bits = (uint64_t)__double_as_longlong(x);
  int64_t e = (int64_t)(bits >> 52) - 1022;
  double f = __longlong_as_double((long long)((bits & 0x000FFFFFFFFFFFFFull) | 0x3FE0000000000000ull));
  if (f < 0.7071067811865476) {
    f = f * 2.0;
    e -= 1;
  }
  const double s = (f - 1.0) / (f + 1.0);
  const double s2 = s * s;
  double poly = 1.0 / 21.0;
  poly = poly * s2 + 1.0 / 19.0;
  poly = poly * s2 + 1.0 / 17.0;
  poly = poly * s2 + 1.0 / 15.0;
  poly = poly * s2 + 1.0 / 13.0;
  poly = poly * s2 + 1.0 / 11.0;
  poly = poly * s2 + 1.0 / 9.0;
  poly = poly * s2 + 1.0 / 7.0;
  poly = poly * s2 + 1.0 / 5.0;
  poly = poly * s2 + 1.0 / 3.0;
  poly = poly * s2 + 1.0;
  return (2.0 * s) * poly + (double)e * 0.6931471805599453;
}

// The standard normal variate of the word w: u = (2k + 1) 2^-53 with k the top 52 bits (exact, inside (0, 1), 1 - u
// exact), then P. J. Acklam's rational inverse normal CDF (relative error 1.15e-9).
__device__ __forceinline__ double sr_variate(uint64_t w) {
#pragma clang fp contract(off)
  const double u = (double)((w >> 12) * 2ull + 1ull) * 0x1p-53;
  if (u < 0.02425 || u > 0.97575) {
    const bool upper = u > 0.97575;
    const double t = upper ? 1.0 - u : u;
    const double q = sqrt(-2.0 * sr_log(t));
    double num = -7.784894002430293e-03;
    num = num * q + -3.223964580411365e-01;
    num = num * q + -2.400758277161838e+00;
    num = num * q + -2.549732539343734e+00;
    num = num * q + 4.374664141464968e+00;
    num = num * q + 2.938163982698783e+00;
    double den = 7.784695709041462e-03;
    den = den * q + 3.224671290700398e-01;
    den = den * q + 2.445134137142996e+00;
    den = den * q + 3.754408661907416e+00;
    den = den * q + 1.0;
    const double z = num / den;
    return upper ? -z : z;
  }
  const double q = u - 0.5;
  const double r = q * q;
  double num = -3.969683028665376e+01;
  num = num * r + 2.209460984245205e+02;
  num = num * r + -2.759285104469687e+02;
  num = num * r + 1.383577518672690e+02;
  num = num * r + -3.066479806614716e+01;
  num = num * r + 2.506628277459239e+00;
  double den = -5.447609879822406e+01;
  den = den * r + 1.615858368580409e+02;
  den = den * r + -1.556989798598866e+02;
  den = den * r + 6.680131188771972e+01;
  den = den * r + -1.328068155288572e+01;
  den = den * r + 1.0;
  return (num * q) / den;
}

__device__ __forceinline__ float sr_noisy(float x, float sigma, double scale, uint64_t key, uint64_t e) {
#pragma clang fp contract(off)
  const double amp = (double)sigma * scale;
  const double noise = sr_variate(sr_mix(key ^ e)) * amp;
  return (float)((double)x + noise);
}

// Thread t owns the 4 consecutive elements 4 t .. 4 t + 3 of a pass (one 16-byte access; X and Y are allocations of the
// entry points, so 16-byte aligned); e0 = row0 * d is the global index of element 0.
__global__ __launch_bounds__(256) void sr_perturb_kernel(float *Y, const float *X, const float *sigma, double scale,
                                                         int64_t cnt, int d, uint64_t key, uint64_t e0) {
  const int64_t quads = (cnt + 3) / 4;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < quads; t += (int64_t)gridDim.x * 256) {
    const int64_t e = 4 * t;
    int j = (int)(e % d);
    if (e + 4 <= cnt) {
      const float4 x = *reinterpret_cast<const float4 *>(X + e);
      float v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = sr_noisy(v[q], sigma[j], scale, key, e0 + (uint64_t)(e + q));
        if (++j == d) j = 0;
      }
      *reinterpret_cast<float4 *>(Y + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int q = 0; q < 4 && e + q < cnt; ++q) {
        Y[e + q] = sr_noisy(X[e + q], sigma[j], scale, key, e0 + (uint64_t)(e + q));
        if (++j == d) j = 0;
      }
    }
  }
}

// part[blk][j] = sum over the block's rows of x (mean null) or (x - mean[j])^2
__global__ __launch_bounds__(256) void sr_colsum_kernel(double *part, const float *X, const double *mean, int64_t n,
                                                        int d) {
#pragma clang fp contract(off)
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = blockIdx.y * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.x * SR_ROWS, r1 = std::min<int64_t>(n, r0 + SR_ROWS);
  double acc = 0.0;
  if (j < d) {
    if (mean) {
      const double mu = mean[j];
      for (int64_t r = r0 + g; r < r1; r += 4) {
        const double df = (double)X[(size_t)r * d + j] - mu;
        acc = acc + df * df;
      }
    } else {
      for (int64_t r = r0 + g; r < r1; r += 4) acc = acc + (double)X[(size_t)r * d + j];
    }
  }
  red[g][lane] = acc;
  __syncthreads();
  if (g == 0 && j < d) part[(size_t)blockIdx.x * d + j] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ __launch_bounds__(256) void sr_colfinish_kernel(double *mean, float *sigma, const double *part, int nblk,
                                                           int64_t n, int d, double div) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= d) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s = s + part[(size_t)b * d + j];
  if (sigma) sigma[j] = (float)((double)(float)sqrt(s / (double)(n - 1)) / div);
  else mean[j] = s / (double)n;
}

int sr_blocks(int64_t n) { return (int)((n + SR_ROWS - 1) / SR_ROWS); }
size_t sr_std_scratch_bytes(int64_t n, int d) { return ((size_t)sr_blocks(n) + 1) * d * 8; }

// sigma [d] f32 <- the per-column sample standard deviation of X [n][d] (n >= 2), divided by div in f32 (div a small
// integer: the f64 quotient of two f32 values rounds to f32 as the f32 quotient does); scratch: sr_std_scratch_bytes
int sr_std_dev(float *sigma, const float *X, int64_t n, int d, double div, double *scratch, hipStream_t s) {
  const int nblk = sr_blocks(n);
  double *mean = scratch, *part = scratch + d;
  const dim3 grid((unsigned)nblk, (unsigned)((d + 63) / 64));
  const unsigned fgrid = (unsigned)((d + 255) / 256);
  hipLaunchKernelGGL(sr_colsum_kernel, grid, dim3(256), 0, s, part, X, (const double *)nullptr, n, d);
  RQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(sr_colfinish_kernel, dim3(fgrid), dim3(256), 0, s, mean, (float *)nullptr, (const double *)part,
                     nblk, n, d, 1.0);
  RQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(sr_colsum_kernel, grid, dim3(256), 0, s, part, X, (const double *)mean, n, d);
  RQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(sr_colfinish_kernel, dim3(fgrid), dim3(256), 0, s, mean, sigma, (const double *)part, nblk, n, d,
                     div);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

// Y [n][d] <- X perturbed (device pointers, Y may be X); the rows are rows row0 .. row0 + n - 1 of the call's array
int sr_perturb_dev(float *Y, const float *X, const float *sigma, double scale, int64_t n, int d, int kind, uint64_t seed,
                   int64_t call, int64_t row0, hipStream_t s) {
  const int64_t cnt = n * d;
  if (cnt <= 0) return RQ_OK;
  const int64_t quads = (cnt + 3) / 4;
  const unsigned grid = (unsigned)std::min<int64_t>((quads + 255) / 256, 8192);
  hipLaunchKernelGGL(sr_perturb_kernel, dim3(grid), dim3(256), 0, s, Y, X, sigma, scale, cnt, d,
                     sr_stream_key(seed, kind, call), (uint64_t)row0 * (uint64_t)d);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

int sr_schedule(double *scale, int schedule, int64_t iter, int64_t niter, double p) {
  if (!scale) return fail(RQ_EINVAL, "sr_schedule: null pointer");
  if (schedule < 1 || schedule > 3) return fail(RQ_EINVAL, "sr_schedule: schedule=%d unknown (1, 2 or 3)", schedule);
  if (niter < 1) return fail(RQ_EINVAL, "sr_schedule: niter=%lld < 1", (long long)niter);
  if (iter < 0 || (schedule == 1 && iter > niter))
    return fail(RQ_EINVAL, "sr_schedule: iter=%lld outside 0..niter=%lld", (long long)iter, (long long)niter);
  if (!(p >= 0.0) || !isfinite(p)) return fail(RQ_EINVAL, "sr_schedule: p=%g must be finite and >= 0", p);
  double v;
  if (schedule == 1) v = pow(1.0 - (double)iter / (double)niter, p);
  else if (schedule == 2) v = 1.0 / pow(1.0 + (double)iter, p);
  else v = pow(p, (double)iter / 2.0);
  if (!isfinite(v)) return fail(RQ_EINVAL, "sr_schedule: schedule %d gives a non-finite scale at iter=%lld, p=%g", schedule,
                                (long long)iter, p);
  *scale = v;
  return RQ_OK;
}

int sr_perturb_check(const void *Y, const void *X, const void *sigma, double scale, int64_t n, int d, int kind,
                     int64_t call, int64_t row0) {
  if (n < 0 || d < 1) return fail(RQ_EINVAL, "sr_perturb: n=%lld, d=%d (need n >= 0, d >= 1)", (long long)n, d);
  if (kind != RQ_SR_C && kind != RQ_SR_D) return fail(RQ_EINVAL, "sr_perturb: kind=%d unknown (0 = SR-C, 1 = SR-D)", kind);
  if (call < 0 || row0 < 0) return fail(RQ_EINVAL, "sr_perturb: call=%lld, row0=%lld must be >= 0", (long long)call,
                                        (long long)row0);
  if (row0 > (INT64_MAX / d) - n) return fail(RQ_EINVAL, "sr_perturb: (row0 + n) * d overflows the element index");
  if (!isfinite(scale)) return fail(RQ_EINVAL, "sr_perturb: scale=%g is not finite", scale);
  if (!sigma || (n > 0 && (!Y || !X))) return fail(RQ_EINVAL, "sr_perturb: null pointer");
  return RQ_OK;
}

// Phase clock of rq_train_sr: hipEvents between the phases of the calling thread's last call, read at its end.
enum { SR_STD, SR_PERTURB, SR_UPDATE, SR_ENCODE, SR_OBJ, SR_OTHER, SR_N };
thread_local double g_sr_ms[SR_N] = {0};

// Codebook updates of the calling thread's last training call (rq_last_sr_stats): computed in full, computed from the kept
// Cholesky factor and row sort, skipped outright
enum { SR_UPD_FULL, SR_UPD_REUSED, SR_UPD_SKIPPED, SR_UPD_N };
thread_local int64_t g_sr_upd[SR_UPD_N] = {0};

// the encoder of the loop by code type: rq_icm.hip's over bytes, rq_icm_h16.hip's over int16 codes
int sr_encode_dev(uint8_t *B, float *cost, const float *X, const float *C, int64_t n, int d, int m, int h, int ilsiter, int icmiter,
                  int npert, int randord, uint64_t seed, int64_t t0, int nsplits, hipStream_t s) {
  return icm_encode_dev(B, B, cost, X, C, n, d, m, h, ilsiter, icmiter, npert, randord, seed, t0, nsplits, s, nullptr);
}
int sr_encode_dev(int16_t *B, float *cost, const float *X, const float *C, int64_t n, int d, int m, int h, int ilsiter, int icmiter,
                  int npert, int randord, uint64_t seed, int64_t t0, int nsplits, hipStream_t s) {
  return icm_encode_wide_dev(B, B, cost, X, C, n, d, m, h, ilsiter, icmiter, npert, randord, seed, t0, nsplits, s, nullptr);
}

// The codebook updates of one training call.  Over bytes every update is computed in full.  Over int16 codes (DESIGN.md section
// 4.27) `clean` says that Cd holds update(RX, B) for the codes B as they are now and that `kept` is what that update left
// behind: the trailing clean update sets it, every encode of a step clears it (the obj pass is a zero-iteration encode and
// leaves the codes alone).  The state lives in this object, inside one call and under its DeviceLock.
template <class Code>
struct SrUpdates {
  bool recompute;
  bool clean = false;
  LsqKept kept;
  // C = update(X, B); same_x: X is the RX of the update that set `clean`
  int run(float *C, const float *X, const Code *B, int64_t n, int d, int m, int h, bool same_x, hipStream_t s) {
    if constexpr (std::is_same<Code, uint8_t>::value) {
      g_sr_upd[SR_UPD_FULL] += 1;
      return lsq_update_launch(C, X, B, n, d, m, h, 1e-4, s);
    } else {
      const bool again = clean && !recompute;
      if (again && same_x) {   // the same inputs and a bitwise reproducible update: C holds the result already
        g_sr_upd[SR_UPD_SKIPPED] += 1;
        return RQ_OK;
      }
      bool reused = false;
      RQ_TRY(lsq_update_wide_launch(C, X, B, n, d, m, h, 1e-4, s, &kept, again, &reused));
      g_sr_upd[reused ? SR_UPD_REUSED : SR_UPD_FULL] += 1;
      return RQ_OK;
    }
  }
};

// rq_train_sr / rq_train_sr_wide after their argument checks (src/SR.jl:88-176, :4-84).  codes [n][m] on the host, in code_base ..
// code_base + h - 1 (bytes: code_base 0); the loop runs on zero-based codes.  scale[call]: the noise scale of perturbation call
// `call` (call 0 is SR_C's iter 0 / SR_D's iter 1, call it is iter it).
template <class Code>
int train_sr_host(float *C, Code *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m, int h, int niter,
                  int ilsiter, int icmiter, int npert, int randord, int method, const std::vector<double> &scale, int clean_update,
                  uint64_t seed, int nsplits, int code_base, bool recompute) {
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  const int mh = m * h;
  const size_t xb = (size_t)n * d * 4, cb = (size_t)mh * d * 4, kb = (size_t)n * m * sizeof(Code);
  DevMem dX, dRX, dR, dC, dC2, dnoisy, dcodes, dcost, dobj, dsig, dscr;
  RQ_TRY(dX.alloc(xb));
  RQ_TRY(dcodes.alloc(kb));
  RQ_TRY(dC.alloc(cb));
  RQ_TRY(dcost.alloc((size_t)n * 4));
  RQ_TRY(dobj.alloc((size_t)(niter + 1) * 8));
  RQ_TRY(dsig.alloc((size_t)d * 4));
  RQ_TRY(dscr.alloc(sr_std_scratch_bytes(method == RQ_SR_C ? n : mh, d)));
  if (method == RQ_SR_C) RQ_TRY(dnoisy.alloc(xb));
  const hipStream_t s = nullptr;
  for (int q = 0; q < SR_N; ++q) g_sr_ms[q] = 0;
  for (int q = 0; q < SR_UPD_N; ++q) g_sr_upd[q] = 0;
  PhaseClock clk(s, g_sr_ms);   // SR_OTHER: the uploads, R'X, the rotation back and the code_base shifts
  if (n > 0) {
    RQ_HIP(hipMemcpy(dX.p, X, xb, hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(dcodes.p, codes, kb, hipMemcpyHostToDevice));
  }
  const float *RX = (const float *)dX.p;
  Code *B = (Code *)dcodes.p;
  if constexpr (std::is_same<Code, int16_t>::value) {
    if (code_base) RQ_TRY(add_base_codes_launch(B, n * m, -code_base, s));
  }
  float *Cd = (float *)dC.p, *cost = (float *)dcost.p, *sig = (float *)dsig.p, *noisy = (float *)dnoisy.p;
  double *objd = (double *)dobj.p, *scr = (double *)dscr.p;
  const float *Rtd = nullptr;
  if (R) {   // RX = R'X   (src/SR.jl:115)
    RQ_TRY(upload_rotation(dR, dRX, R, (const float *)dX.p, n, d, di.num_cu, s));
    RQ_TRY(dC2.alloc(cb));
    Rtd = dR.as<float>() + (size_t)d * d;
    RX = (const float *)dRX.p;
  }
  clk.mark(SR_OTHER);
  if (method == RQ_SR_C) {   // RX does not change: one standard deviation serves every call
    RQ_TRY(sr_std_dev(sig, RX, n, d, 1.0, scr, s));
    clk.mark(SR_STD);
  }
  SrUpdates<Code> upd{recompute};
  // perturbation call `call`, then ILS iterations call * ilsiter .. of one `seed` stream   (src/SR.jl:118-134, :151-164)
  auto step = [&](int call) -> int {
    if (method == RQ_SR_C) {
      RQ_TRY(sr_perturb_dev(noisy, RX, sig, scale[call], n, d, RQ_SR_C, seed, call, 0, s));
      clk.mark(SR_PERTURB);
      RQ_TRY(upd.run(Cd, noisy, B, n, d, m, h, false, s));
      clk.mark(SR_UPDATE);
    } else {
      RQ_TRY(upd.run(Cd, RX, B, n, d, m, h, true, s));
      clk.mark(SR_UPDATE);
      RQ_TRY(sr_std_dev(sig, Cd, mh, d, (double)m, scr, s));   // std(cat(C..., dims=2), dims=2) ./ m
      clk.mark(SR_STD);
      RQ_TRY(sr_perturb_dev(Cd, Cd, sig, scale[call], mh, d, RQ_SR_D, seed, call, 0, s));
      clk.mark(SR_PERTURB);
    }
    upd.clean = false;   // the encode moves the codes (and SR_D has perturbed Cd)
    RQ_TRY(sr_encode_dev(B, cost, RX, Cd, n, d, m, h, ilsiter, icmiter, npert, randord, seed, (int64_t)call * ilsiter, nsplits, s));
    clk.mark(SR_ENCODE);
    return RQ_OK;
  };
  // obj = qerror(RX, B, C) against the CURRENT C: a veccost pass (the zero-iteration encode) and its mean
  auto objective = [&](int slot) -> int {
    RQ_TRY(sr_encode_dev(B, cost, RX, Cd, n, d, m, h, 0, 0, 0, 0, seed, 0, nsplits, s));
    RQ_TRY(lsq_mean_launch(objd + slot, cost, n, s));
    clk.mark(SR_OBJ);
    return RQ_OK;
  };
  RQ_TRY(step(0));
  for (int it = 1; it <= niter; ++it) {
    RQ_TRY(objective(it - 1));
    RQ_TRY(step(it));
    if (clean_update) {   // train_sr_cuda's trailing update (src/SR.jl:166); train_sr has none
      RQ_TRY(upd.run(Cd, RX, B, n, d, m, h, true, s));
      clk.mark(SR_UPDATE);
      upd.clean = true;   // Cd = update(RX, B): what the next step opens with, over these codes
    }
  }
  RQ_TRY(objective(niter));
  if constexpr (std::is_same<Code, int16_t>::value) {
    if (code_base) {
      RQ_TRY(add_base_codes_launch(B, n * m, code_base, s));
      clk.mark(SR_OTHER);
    }
  }
  if (R) {   // C_i <- R C_i   (src/SR.jl:172)
    RQ_HIP(hipMemcpyAsync(dC2.p, Cd, cb, hipMemcpyDeviceToDevice, s));
    RQ_TRY(rotate_launch(Cd, Rtd, (const float *)dC2.p, d, mh, di.num_cu, s));
    clk.mark(SR_OTHER);
  }
  clk.collect();
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(C, Cd, cb, hipMemcpyDeviceToHost));
  if (n > 0) RQ_HIP(hipMemcpy(codes, B, kb, hipMemcpyDeviceToHost));
  RQ_HIP(hipMemcpy(obj, objd, (size_t)(niter + 1) * 8, hipMemcpyDeviceToHost));
  return RQ_OK;
}

// the noise scale of every perturbation call: call 0 is SR_C's iter 0 / SR_D's iter 1, call it is iter it
int sr_scales(std::vector<double> &scale, int niter, int method, int schedule, double p) {
  scale.assign((size_t)niter + 1, 0.0);
  for (int it = 0; it <= niter; ++it)
    RQ_TRY(sr_schedule(&scale[it], schedule, it == 0 && method == RQ_SR_D ? 1 : it, niter, p));
  return RQ_OK;
}

}  // namespace

}  // namespace rq

using namespace rq;

extern "C" int rq_sr_schedule(double *scale, int schedule, int64_t iter, int64_t niter, double p) {
  return sr_schedule(scale, schedule, iter, niter, p);
}

extern "C" int rq_sr_std(float *sigma, const float *X, int64_t n, int d) {
  if (d < 1) return fail(RQ_EINVAL, "sr_std: d=%d < 1", d);
  if (n < 2) return fail(RQ_EINVAL, "sr_std: n=%lld < 2 (the sample standard deviation divides by n - 1)", (long long)n);
  if (n > (int64_t)INT32_MAX * SR_ROWS) return fail(RQ_EINVAL, "sr_std: n=%lld is too large", (long long)n);
  if (!sigma || !X) return fail(RQ_EINVAL, "sr_std: null pointer");
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  DevMem dX, dsig, dscr;
  RQ_TRY(dX.alloc((size_t)n * d * 4));
  RQ_TRY(dsig.alloc((size_t)d * 4));
  RQ_TRY(dscr.alloc(sr_std_scratch_bytes(n, d)));
  RQ_HIP(hipMemcpy(dX.p, X, (size_t)n * d * 4, hipMemcpyHostToDevice));
  RQ_TRY(sr_std_dev((float *)dsig.p, (const float *)dX.p, n, d, 1.0, (double *)dscr.p, nullptr));
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(sigma, dsig.p, (size_t)d * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

extern "C" int rq_sr_perturb(float *Y, const float *X, const float *sigma, double scale, int64_t n, int d, int kind,
                             uint64_t seed, int64_t call, int64_t row0) {
  RQ_TRY(sr_perturb_check(Y, X, sigma, scale, n, d, kind, call, row0));
  if (n == 0) return RQ_OK;
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  DevMem dX, dsig;
  const size_t xb = (size_t)n * d * 4;
  RQ_TRY(dX.alloc(xb));
  RQ_TRY(dsig.alloc((size_t)d * 4));
  RQ_HIP(hipMemcpy(dX.p, X, xb, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dsig.p, sigma, (size_t)d * 4, hipMemcpyHostToDevice));
  RQ_TRY(sr_perturb_dev((float *)dX.p, (const float *)dX.p, (const float *)dsig.p, scale, n, d, kind, seed, call, row0,
                        nullptr));
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(Y, dX.p, xb, hipMemcpyDeviceToHost));
  return RQ_OK;
}

extern "C" int rq_train_sr(float *C, uint8_t *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m,
                           int h, int niter, int ilsiter, int icmiter, int npert, int randord, int method, int schedule,
                           double p, int clean_update, uint64_t seed, int nsplits) {
  if (m < 1 || m > 16) return fail(RQ_EINVAL, "train_sr: m=%d outside 1..16", m);
  if (h < 2 || h > 256) return fail(RQ_EINVAL, "train_sr: h=%d outside 2..256", h);
  if (d < 1) return fail(RQ_EINVAL, "train_sr: d=%d < 1", d);
  if (n < 0 || n > (int64_t)UINT32_MAX)
    return fail(RQ_EINVAL, "train_sr: n=%lld outside 0..%u (the u32 counters)", (long long)n, UINT32_MAX);
  if (!C || !codes || !obj) return fail(RQ_EINVAL, "train_sr: null output pointer");
  if (n > 0 && !X) return fail(RQ_EINVAL, "train_sr: null pointer");
  if (method != RQ_SR_C && method != RQ_SR_D) return fail(RQ_EINVAL, "train_sr: SR method %d unknown (0 = SR_C, 1 = SR_D)", method);
  if (niter < 1) return fail(RQ_EINVAL, "train_sr: niter=%d < 1 (schedule 1 divides by it)", niter);
  if (method == RQ_SR_C && n < 2) return fail(RQ_EINVAL, "train_sr: SR_C needs n >= 2 rows for the standard deviation; got %lld", (long long)n);
  if ((int64_t)ilsiter * ((int64_t)niter + 1) > INT32_MAX)
    return fail(RQ_EINVAL, "train_sr: ilsiter * (niter + 1) overflows the ILS iteration counter");
  RQ_TRY(icm_check_args(codes, codes, X, C, n, d, m, h, ilsiter, icmiter, npert, 0, nsplits));
  std::vector<double> scale;
  RQ_TRY(sr_scales(scale, niter, method, schedule, p));
  RQ_TRY(host_code_range(codes, n, m, h, "train_sr"));
  return train_sr_host<uint8_t>(C, codes, obj, X, R, n, d, m, h, niter, ilsiter, icmiter, npert, randord, method, scale, clean_update,
                                seed, nsplits, 0, true);
}

// 2 <= h <= RQ_MAX_H16 over int16 codes: the int16 instantiation at EVERY h, host pointers
extern "C" int rq_train_sr_wide(float *C, int16_t *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m,
                                int h, int niter, int ilsiter, int icmiter, int npert, int randord, int method, int schedule,
                                double p, int clean_update, uint64_t seed, int nsplits, int code_base, int flags) {
  const char *who = "train_sr_wide";
  if (m < 1 || m > 16) return fail(RQ_EINVAL, "%s: m=%d outside 1..16", who, m);
  if (h < 2 || h > RQ_MAX_H16) return fail(RQ_EINVAL, "%s: h=%d outside 2..%d", who, h, RQ_MAX_H16);
  if (d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);
  if (n < 0 || n > (int64_t)UINT32_MAX)
    return fail(RQ_EINVAL, "%s: n=%lld outside 0..%u (the u32 counters)", who, (long long)n, UINT32_MAX);
  if (!C || !codes || !obj) return fail(RQ_EINVAL, "%s: null output pointer", who);
  if (n > 0 && !X) return fail(RQ_EINVAL, "%s: null pointer", who);
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  if (flags & ~RQ_SR_RECOMPUTE) return fail(RQ_EINVAL, "%s: flags=0x%x has an unknown bit (RQ_SR_RECOMPUTE = 1)", who, flags);
  if (method != RQ_SR_C && method != RQ_SR_D) return fail(RQ_EINVAL, "%s: SR method %d unknown (0 = SR_C, 1 = SR_D)", who, method);
  if (niter < 1) return fail(RQ_EINVAL, "%s: niter=%d < 1 (schedule 1 divides by it)", who, niter);
  if (method == RQ_SR_C && n < 2)
    return fail(RQ_EINVAL, "%s: SR_C needs n >= 2 rows for the standard deviation; got %lld", who, (long long)n);
  if (ilsiter < 0 || icmiter < 0) return fail(RQ_EINVAL, "%s: negative count (ilsiter=%d icmiter=%d)", who, ilsiter, icmiter);
  if (npert < 0 || npert > m) return fail(RQ_EINVAL, "%s: npert=%d outside 0..m=%d", who, npert, m);
  if ((int64_t)ilsiter * ((int64_t)niter + 1) > INT32_MAX)
    return fail(RQ_EINVAL, "%s: ilsiter * (niter + 1) overflows the ILS iteration counter", who);
  std::vector<double> scale;
  RQ_TRY(sr_scales(scale, niter, method, schedule, p));
  RQ_TRY(lsq_train_wide_shape(who, n, d, m, h, nsplits));
  RQ_TRY(host_code_range(codes, n, m, h, code_base, who));
  return train_sr_host<int16_t>(C, codes, obj, X, R, n, d, m, h, niter, ilsiter, icmiter, npert, randord, method, scale,
                                clean_update, seed, nsplits, code_base, (flags & RQ_SR_RECOMPUTE) != 0);
}

extern "C" int rq_last_sr_stats(int64_t *out, int cap) {
  if (!out) return fail(RQ_EINVAL, "rq_last_sr_stats: null pointer");
  for (int q = 0; q < cap && q < SR_UPD_N; ++q) out[q] = g_sr_upd[q];
  return RQ_OK;
}

extern "C" int rq_last_sr_timing(double *ms, int cap) {
  if (!ms) return fail(RQ_EINVAL, "rq_last_sr_timing: null pointer");
  for (int q = 0; q < cap && q < SR_N; ++q) ms[q] = g_sr_ms[q];
  return RQ_OK;
}
