// rq_ervq.hip -- Enhanced RVQ / Stacked Quantizers (src/ERVQ.jl, arXiv 1411.2173): train_ervq, device-resident.
//
// The reference (src/ERVQ.jl:51-135) refines m full-dimensional codebooks that train_rvq initialised: for every iteration and
// every codebook j, in this order,
//   1. C_j[k] <- mean over the rows with b_j = k of Xd = X - sum_{i != j} C_i[b_i]      (Clustering.update_centers!, :85-90)
//   2. entries without rows are refilled                                                  (:93-109)
//   3. B[j:end] = quantize_rvq(X - sum_{i < j} C_i[b_i], C[j:end])                         (:113-118)
//   4. qerror(X, B, C) is reported                                                        (:120)
// What runs here is the same loop in another form.  Let E = X - sum_i C_i[b_i], the full residual that step 3 of the previous
// step leaves as the final residual of its quantize_rvq.  Then Xd = E + C_j[b_j], and the mean of Xd over the rows of entry k is
//   C_j[k] + mean_{b_j = k}(E):
// the update is an INCREMENT by the mean residual.  It gathers from no other codebook, and in f32 it lands about ten times closer
// to an f64 evaluation of the reference's formula than the literal form (sums of small residuals instead of sums of data-sized
// values; tests/test_ervq_oracle.py measures both).  The segment sum is update_centers' (rq_train.hip: ervq_increment_launch),
// the stage encode is encode_launch with one sub-quantizer of width d, the error pass qerror_launch on E.
//
// Buffers: X (= P_1, the residual entering stage 1), two prefix buffers that alternate as P_j / P_{j+1}, one working buffer that
// ends every step as E.  Step j encodes stage j on P_j and writes P_{j+1} = P_j - C_j[b_j] OUT OF PLACE into the other prefix
// buffer, stage j + 1 goes from there into the working buffer, the later stages run in place: no n x d copy per step.
//
// Entries without rows, for EVERY j: Clustering.repick_unused_centers' rule (what repick_unused of rq_train_host.hip does for
// train_pq / train_rvq; same costs, same draws) on P_j, the residual entering stage j -- a row drawn with probability
// proportional to |P_j[row] - C_j[b_j]|^2 under the entry values the codes were assigned with, costs lowered after each
// draw, from the library's seeded stream.  The O(n d) parts (the costs, their lowering) run on the device and only the n
// costs come to the host for the draw: an ERVQ step at h = 256 empties entries routinely, and the host form, which
// downloads P_j and loops over n d values per draw, took 7 s of a 35 ms iteration at 1e6 x 128.  The reference takes the
// refill for j >= 2 from quantize_rvq's `singletons` (the same rule with Julia's RNG: other draws) and for j = 1 calls
// repick_unused_centers through a Julia-0.6 `sum(..., 1)` that does not run on Julia >= 0.7; here j = 1 follows the rule of j >= 2.
#include <string.h>

#include <utility>
#include <vector>

#include "rq_internal.h"

// More than 256 codewords per stage: the loop below is ONE template over the code type, as the Lloyd
// loops of rq_train_host.hip (section 4.19).  Code = uint8_t is the loop as it was -- the same launches, draws and bits; Code =
// int16_t (zero-based on the device) takes ervq_increment_launch<int16_t> and encode_launch's int16 overload and nothing else.

namespace rq {

namespace {

// Clustering.repick_unused_centers for the `unused` entries of Cj [h][d]: rows of P drawn with probability proportional to
// their cost under Cold (the entries the codes were assigned with); the drawn row's cost drops to zero and every cost is
// lowered to the distance to the new entry before the next draw.  dtc: n doubles of device scratch.  The costs (f64, one thread
// per row, the d terms in ascending order: the host loop of repick_unused bit for bit) and the draws are refill_unused_launch's
// (rq_train.hip), here on the whole row: columns [0, d).
template <class Code>
int ervq_refill(float *Cj, const float *Cold, const float *P, const Code *codes, int cstride, int col, int64_t n, int d,
                const std::vector<int> &unused, Rng &rng, double *dtc, std::vector<double> &tc, hipStream_t stream) {
  return refill_unused_launch<Code>(Cj, Cold, P, codes, cstride, col, n, d, 0, d, unused, rng, dtc, tc, stream);
}

// E = X - sum_i C_i[b_i] by m in-place epilogues in codebook order (the order quantize_rvq subtracts in)
template <class Code>
int ervq_full_residual(float *E, const float *C, const Code *codes, int64_t n, int d, int m, int h, hipStream_t stream) {
  for (int i = 0; i < m; ++i)
    RQ_TRY(residual_launch<Code>(E, E, C + (size_t)i * h * d, codes + i, m, nullptr, nullptr, n, d, m, i, stream));
  return RQ_OK;
}

int ervq_check_shape(const char *who, int64_t n, int d, int m, int h) {
  if (m < 1 || m > 64) return fail(RQ_EINVAL, "%s: m=%d outside 1..64", who, m);
  if (h < 2 || h > 256) return fail(RQ_EINVAL, "%s: h=%d outside 2..256", who, h);
  if (d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);
  if (n < 0) return fail(RQ_EINVAL, "%s: n=%lld < 0", who, (long long)n);
  return RQ_OK;
}

// the *_wide entries: 2 <= h <= RQ_MAX_H16, and the error codes of the other *_wide entry points
int ervq_check_shape_wide(const char *who, int64_t n, int d, int m, int h, int code_base) {
  if (code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  if (m < 1 || m > 64) return fail(RQ_EUNSUPPORTED, "%s covers 1 <= m <= 64; got m=%d", who, m);
  if (h > RQ_MAX_H16) return fail(RQ_EUNSUPPORTED, "%s takes Int16 codes: 2 <= h <= %d; got h=%d", who, RQ_MAX_H16, h);
  if (h < 2) return fail(RQ_EINVAL, "%s: h=%d < 2", who, h);
  if (d < 1) return fail(RQ_EINVAL, "%s: d=%d < 1", who, d);
  if (n < 0) return fail(RQ_EINVAL, "%s: n=%lld < 0", who, (long long)n);
  return RQ_OK;
}

// every code of B [n][m] (host) in code_base .. code_base + h - 1
int ervq_code_range(const char *who, const int16_t *B, int64_t n, int m, int h, int code_base) {
  for (int64_t e = 0; e < n * m; ++e)
    if (B[e] < code_base || B[e] > h - 1 + code_base)
      return fail(RQ_EINVAL, "%s: code %d at [%lld][%lld] is outside %d..%d", who, (int)B[e], (long long)(e / m),
                  (long long)(e % m), code_base, h - 1 + code_base);
  return RQ_OK;
}

// Phase clock of rq_train_ervq: hipEvents between the phases of the calling thread's last call, read at its end.
enum { EV_INIT, EV_INCREMENT, EV_REFILL, EV_ENCODE, EV_EPILOGUE, EV_ERROR, EV_OTHER, EV_N };
thread_local double g_ervq_ms[EV_N] = {0};

// rq_ervq_update_codebook after its argument checks; codes [n][m] zero-based on the host
template <class Code>
int ervq_update_host(float *C, uint32_t *counts, const float *X, const Code *codes, int64_t n, int d, int m, int h, int j) {
  if (n == 0) {
    memset(counts, 0, (size_t)h * sizeof(uint32_t));
    return RQ_OK;
  }
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  const size_t xb = (size_t)n * d * 4, cb = (size_t)m * h * d * 4, jb = (size_t)h * d * 4, kb = (size_t)n * m * sizeof(Code);
  DevMem dE, dC, dcodes, dcnt;
  RQ_TRY(dE.alloc(xb)); RQ_TRY(dC.alloc(cb)); RQ_TRY(dcodes.alloc(kb)); RQ_TRY(dcnt.alloc((size_t)h * 4));
  RQ_HIP(hipMemcpy(dE.p, X, xb, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dC.p, C, cb, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dcodes.p, codes, kb, hipMemcpyHostToDevice));
  RQ_TRY(ervq_full_residual<Code>(dE.as<float>(), dC.as<float>(), dcodes.as<Code>(), n, d, m, h, nullptr));
  float *Cj = dC.as<float>() + (size_t)j * h * d;
  RQ_TRY(ervq_increment_launch<Code>(Cj, dcnt.as<unsigned int>(), dE.as<float>(), dcodes.as<Code>(), n, d, m, j, h, di.num_cu, nullptr));
  RQ_HIP(hipDeviceSynchronize());
  RQ_HIP(hipMemcpy(C + (size_t)j * h * d, Cj, jb, hipMemcpyDeviceToHost));   // the other blocks are not written
  RQ_HIP(hipMemcpy(counts, dcnt.p, (size_t)h * 4, hipMemcpyDeviceToHost));
  return RQ_OK;
}

// rq_train_ervq after its argument checks: B [n][m] Int16 on the host, in code_base .. code_base + h - 1
template <class Code>
int train_ervq_host(float *C, int16_t *B, double *error, double *obj, const float *X, int64_t n, int d, int m, int h, int niter,
                    uint64_t seed, int code_base) {
  DeviceInfo di;
  RQ_TRY(device_info(&di));
  DeviceLock call_lock;
  const size_t xb = (size_t)n * d * 4, jb = (size_t)h * d * 4, cb = (size_t)m * jb;
  const int nobj = niter * m + 1;
  Rng rng{seed * 0x9E3779B97F4A7C15ull + 4};
  DevMem dX, dP[2], dW, dC, dCold, dcodes, dstage, dcnt, dobj, d16;
  RQ_TRY(dX.alloc(xb)); RQ_TRY(dW.alloc(xb)); RQ_TRY(dC.alloc(cb)); RQ_TRY(dCold.alloc(jb));
  RQ_TRY(dcodes.alloc((size_t)n * m * sizeof(Code))); RQ_TRY(dstage.alloc((size_t)n * sizeof(Code))); RQ_TRY(dcnt.alloc((size_t)h * 4));
  RQ_TRY(dobj.alloc((size_t)nobj * 8)); RQ_TRY(d16.alloc((size_t)n * m * 2));
  if (niter > 0 && m > 1) { RQ_TRY(dP[0].alloc(xb)); RQ_TRY(dP[1].alloc(xb)); }
  const hipStream_t s = nullptr;
  for (int q = 0; q < EV_N; ++q) g_ervq_ms[q] = 0;
  PhaseClock clk(s, g_ervq_ms);
  RQ_HIP(hipMemcpy(dX.p, X, xb, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(dC.p, C, cb, hipMemcpyHostToDevice));
  RQ_HIP(hipMemcpy(d16.p, B, (size_t)n * m * 2, hipMemcpyHostToDevice));
  float *Xd = dX.as<float>(), *W = dW.as<float>(), *Cd = dC.as<float>();
  Code *codes = dcodes.as<Code>(), *stage = dstage.as<Code>();
  double *objd = dobj.as<double>();
  // the caller's Int16 codes -> zero-based codes of the loop's type (the range was checked on the host)
  RQ_TRY(convert_codes_launch(codes, (const int16_t *)d16.as<int16_t>(), n * m, -code_base, s));
  clk.mark(EV_OTHER);
  // E of the caller's codes and codebooks, and its error
  RQ_HIP(hipMemcpyAsync(W, Xd, xb, hipMemcpyDeviceToDevice, s));
  RQ_TRY(ervq_full_residual<Code>(W, Cd, codes, n, d, m, h, s));
  clk.mark(EV_INIT);
  RQ_TRY(qerror_launch(objd, W, nullptr, n, d, di.num_cu, s));
  clk.mark(EV_ERROR);
  std::vector<unsigned int> counts((size_t)h);
  std::vector<int> unused;
  DevMem dtc;                 // the refill's costs: allocated when the first entry without rows turns up
  std::vector<double> tc;
  for (int it = 0; it < niter; ++it) {
    const float *P = Xd;          // P_j: the residual entering stage j under the current codes and codebooks
    for (int j = 0; j < m; ++j) {
      float *Cj = Cd + (size_t)j * h * d;
      // 1. the increment (dCold keeps the entries the codes were assigned with: the refill draws with THOSE costs)
      RQ_HIP(hipMemcpyAsync(dCold.p, Cj, jb, hipMemcpyDeviceToDevice, s));
      RQ_TRY(ervq_increment_launch<Code>(Cj, dcnt.as<unsigned int>(), W, codes, n, d, m, j, h, di.num_cu, s));
      clk.mark(EV_INCREMENT);
      // 2. entries without rows
      RQ_HIP(hipMemcpy(counts.data(), dcnt.p, (size_t)h * 4, hipMemcpyDeviceToHost));
      unused.clear();
      for (int k = 0; k < h; ++k)
        if (counts[k] == 0) unused.push_back(k);
      if (!unused.empty()) {
        if (!dtc.p) RQ_TRY(dtc.alloc((size_t)n * 8));
        RQ_TRY(ervq_refill<Code>(Cj, dCold.as<float>(), P, codes, m, j, n, d, unused, rng, dtc.as<double>(), tc, s));
      }
      clk.mark(EV_REFILL);
      // 3. stages j..m-1 again: P_j -> P_{j+1} (kept for the next step) -> the working buffer, then in place
      float *Pnext = dP[j & 1].as<float>();
      const float *src = P;
      for (int i = j; i < m; ++i) {
        const float *Ci = Cd + (size_t)i * h * d;
        RQ_TRY(encode_launch(stage, src, Ci, n, d, 1, h, di.num_cu, s));
        clk.mark(EV_ENCODE);
        if (i == j && j + 1 < m) {
          RQ_TRY(residual_launch<Code>(Pnext, src, Ci, stage, 1, codes, nullptr, n, d, m, i, s));
          src = Pnext;
        } else if (src != W) {
          RQ_TRY(residual_launch<Code>(W, src, Ci, stage, 1, codes, nullptr, n, d, m, i, s));
          src = W;
        } else {
          RQ_TRY(residual_launch<Code>(W, W, Ci, stage, 1, codes, nullptr, n, d, m, i, s));
        }
        clk.mark(EV_EPILOGUE);
      }
      if (j + 1 < m) P = Pnext;
      // 4. the error of this step
      RQ_TRY(qerror_launch(objd + 1 + (size_t)it * m + j, W, nullptr, n, d, di.num_cu, s));
      clk.mark(EV_ERROR);
    }
  }
  RQ_TRY(convert_codes_launch(d16.as<int16_t>(), (const Code *)codes, n * m, code_base, s));
  clk.mark(EV_OTHER);
  clk.collect();
  RQ_HIP(hipDeviceSynchronize());
  std::vector<double> acc((size_t)nobj);
  RQ_HIP(hipMemcpy(acc.data(), objd, (size_t)nobj * 8, hipMemcpyDeviceToHost));
  for (double &a : acc) a /= (double)n;
  if (obj) memcpy(obj, acc.data(), (size_t)nobj * 8);
  if (error) *error = acc[(size_t)nobj - 1];
  if (niter > 0) {      // niter = 0 returns the inputs as they are
    RQ_HIP(hipMemcpy(C, Cd, cb, hipMemcpyDeviceToHost));
    RQ_HIP(hipMemcpy(B, d16.p, (size_t)n * m * 2, hipMemcpyDeviceToHost));
  }
  return RQ_OK;
}

}  // namespace

}  // namespace rq

using namespace rq;

extern "C" int rq_ervq_update_codebook(float *C, uint32_t *counts, const float *X, const uint8_t *codes, int64_t n, int d, int m,
                                       int h, int j) {
  RQ_TRY(ervq_check_shape("ervq_update_codebook", n, d, m, h));
  if (j < 0 || j >= m) return fail(RQ_EINVAL, "ervq_update_codebook: j=%d outside 0..%d", j, m - 1);
  if (!C || !counts || (n > 0 && (!X || !codes))) return fail(RQ_EINVAL, "ervq_update_codebook: null pointer");
  RQ_TRY(host_code_range(codes, n, m, h, "ervq_update_codebook"));
  return ervq_update_host<uint8_t>(C, counts, X, codes, n, d, m, h, j);
}

extern "C" int rq_train_ervq(float *C, int16_t *B1, double *error, double *obj, const float *X, int64_t n, int d, int m, int h,
                             int niter, uint64_t seed) {
  RQ_TRY(ervq_check_shape("train_ervq", n, d, m, h));
  if (n < 1) return fail(RQ_EINVAL, "train_ervq: n=%lld < 1", (long long)n);
  if (niter < 0 || (int64_t)niter * m + 1 > INT32_MAX) return fail(RQ_EINVAL, "train_ervq: niter=%d", niter);
  if (!C || !B1 || !X) return fail(RQ_EINVAL, "train_ervq: null pointer");
  RQ_TRY(ervq_code_range("train_ervq", B1, n, m, h, 1));
  return train_ervq_host<uint8_t>(C, B1, error, obj, X, n, d, m, h, niter, seed, 1);
}

// ---- 2 <= h <= RQ_MAX_H16 over Int16 codes.  h <= 256 runs the byte instantiation and widens: the bits
// of the two entry points above.
extern "C" int rq_ervq_update_codebook_wide(float *C, uint32_t *counts, const float *X, const int16_t *codes, int64_t n, int d,
                                            int m, int h, int j, int code_base) {
  const char *who = "rq_ervq_update_codebook_wide";
  RQ_TRY(ervq_check_shape_wide(who, n, d, m, h, code_base));
  if (j < 0 || j >= m) return fail(RQ_EINVAL, "%s: j=%d outside 0..%d", who, j, m - 1);
  if (!C || !counts || (n > 0 && (!X || !codes))) return fail(RQ_EINVAL, "%s: null pointer", who);
  RQ_TRY(ervq_code_range(who, codes, n, m, h, code_base));
  const size_t ne = (size_t)std::max<int64_t>(n, 0) * m;
  if (h <= 256) {
    std::vector<uint8_t> c8(ne);
    for (size_t e = 0; e < ne; ++e) c8[e] = (uint8_t)(codes[e] - code_base);
    return ervq_update_host<uint8_t>(C, counts, X, c8.data(), n, d, m, h, j);
  }
  if (code_base == 0) return ervq_update_host<int16_t>(C, counts, X, codes, n, d, m, h, j);
  std::vector<int16_t> c0(ne);
  for (size_t e = 0; e < ne; ++e) c0[e] = (int16_t)(codes[e] - code_base);
  return ervq_update_host<int16_t>(C, counts, X, c0.data(), n, d, m, h, j);
}

extern "C" int rq_train_ervq_wide(float *C, int16_t *B, double *error, double *obj, const float *X, int64_t n, int d, int m, int h,
                                  int niter, uint64_t seed, int code_base) {
  const char *who = "rq_train_ervq_wide";
  RQ_TRY(ervq_check_shape_wide(who, n, d, m, h, code_base));
  if (n < 1) return fail(RQ_EINVAL, "%s: n=%lld < 1", who, (long long)n);
  if (niter < 0 || (int64_t)niter * m + 1 > INT32_MAX) return fail(RQ_EINVAL, "%s: niter=%d", who, niter);
  if (!C || !B || !X) return fail(RQ_EINVAL, "%s: null pointer", who);
  RQ_TRY(ervq_code_range(who, B, n, m, h, code_base));
  if (h <= 256) return train_ervq_host<uint8_t>(C, B, error, obj, X, n, d, m, h, niter, seed, code_base);
  return train_ervq_host<int16_t>(C, B, error, obj, X, n, d, m, h, niter, seed, code_base);
}

extern "C" int rq_last_ervq_timing(double *ms, int cap) {
  if (!ms) return fail(RQ_EINVAL, "rq_last_ervq_timing: null pointer");
  for (int q = 0; q < cap && q < EV_N; ++q) ms[q] = g_ervq_ms[q];
  return RQ_OK;
}

