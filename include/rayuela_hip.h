/*
 * rayuela_hip.h -- C ABI of librayuela_hip.so: MI355X (gfx950) PQ/OPQ encode + ADC linear scan.
 *
 * Drop-in boundary for Rayuela.jl's hot path.  Every entry point names the reference
 * interface it replaces (paths relative to the Rayuela.jl repository):
 *
 *   src/Linscan.jl:19-23  ccall(("linscan_aqd_query", linscan_aqd), ...)  -> linscan_aqd_query
 *   deps/src/linscan_aqd.cpp:105-114 (extern "C" symbol)                  -> linscan_aqd_query
 *   src/Linscan.jl:5-37    linscan_pq                                     -> rq_linscan_pq
 *   src/Linscan.jl:93-115  linscan_opq                                    -> rq_linscan_opq
 *   src/PQ.jl:18-48        quantize_pq                                    -> rq_encode_pq[_i16]
 *   src/OPQ.jl:19-27       quantize_opq  (R'X then quantize_pq)           -> rq_encode_opq[_i16], rq_rotate_T
 *   src/xvecs_read.jl:14-52 + src/read_datasets.jl:148-167  bvecs (UInt8) data, widened before it is encoded
 *                                                                         -> rq_encode_pq_bytes[_i16], rq_encode_opq_bytes[_i16]
 *
 * Array layouts are the C views of the Julia (column-major) arrays, so Julia passes its
 * arrays as they are (zero-copy on the host side):
 *   X, queries   Julia d x n   == C [n][d]   float
 *   R            Julia d x d   == C [d][d]   with Rc[i][k] = R[k,i]
 *   C (PQ)       Vector of m (sub_i x h) matrices, concatenated == C [m][h][sub] when d%m==0
 *                (cat(C...,dims=3), src/Linscan.jl:22); for uneven splits (src/utils.jl:179-203)
 *                the concatenation of the m [h][sub_i] blocks in order
 *   codes        Julia m x n   == C [n][m]   uint8, ZERO-based (the scan's wire format,
 *                src/Linscan.jl:35, demos/experiment_utils.jl:10,17)
 *   dists, ids   Julia k x nq  == C [nq][k]  ascending per query
 *
 * Numerics contract: codes and ids are bit-exact with the CPU oracle; ADC
 * distances are bit-exact with deps/src/linscan_aqd.cpp (unfused f32 LUT, sequential sum,
 * lexicographic (dist,id) top-k).
 *
 * All int-returning functions return 0 on success, a negative RQ_E* code on argument
 * errors and a positive hipError_t on HIP failures; rq_last_error() describes the last
 * failure on the calling thread.  Host-pointer entry points are synchronous and keep no
 * pointer after they return.  The library never falls back to a CPU path.
 */
#ifndef RAYUELA_HIP_H_
#define RAYUELA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RQ_OK 0
#define RQ_EINVAL (-1)      /* bad argument (message in rq_last_error) */
#define RQ_EUNSUPPORTED (-2) /* shape outside what the kernels cover (h>256, LUT > LDS, ...) */
#define RQ_ENODEVICE (-3)   /* no gfx950 device visible */

#define RQ_MAX_H16 32767   /* most codewords per codebook of the *_wide encodes: the largest value a one-based Int16 names */
#define RQ_MAX_K 65536      /* largest k served by the candidate-buffer scan; larger k take the bulk path */

const char *rq_version(void);              /* "rayuela-hip <ver> (gfx950) build <sha1 of the kernel sources, 12 hex digits>" */
const char *rq_last_error(void);
int rq_device_count(void);
/* Select the device used by the calling thread's subsequent calls (hipSetDevice). */
int rq_set_device(int device);

/* ---- legacy symbol: signature-identical to deps/src/linscan_aqd.cpp:107-113 -------------
 * so the stock src/Linscan.jl:19-23 ccall works by pointing `linscan_aqd` at this library.
 * Host pointers; ids zero-based (Julia adds 1, src/Linscan.jl:25).  B = 8*m bits, h = 256.
 * Returns void like the reference; failures are reported on stderr and leave outputs zeroed. */
void linscan_aqd_query(float *dists, unsigned int *res, unsigned char *codes, float *centers,
                       float *queries, int N, unsigned int NQ, int B, int K, int dim1codes,
                       int dim1queries, int subdim);

/* ---- the same scan for non-orthogonal (additive) quantizers ----------------
 * Signature-identical to deps/src/linscan_aqd_pairwise_byte.cpp:179-198 (what src/Linscan.jl:145-153 and
 * :173-181 ccall).  codebooks = hcat(C...) i.e. C [m*h][d], h = 256; ids come back ONE-based like the
 * reference (:76).  LSQ: T = -2<q,c> per entry, dist = sum_k T[k][b_k] + dbnorms[row].  CQ: T = |q-c|^2. */
void linscan_aqd_query_extra_byte(float *dists, int *idx, unsigned char *codes, float *queries,
                                  float *codebooks, float *dbnorms, int nqueries, int ncodes, int m, int h,
                                  int d, int nn);
void linscan_aqd_cq_query_extra_byte(float *dists, int *idx, unsigned char *codes, float *queries,
                                     float *codebooks, int nqueries, int ncodes, int m, int h, int d, int nn);
/* linscan_lsq (src/Linscan.jl:118-157; R may be NULL = no rotation) and linscan_cq (:160-193). */
int rq_linscan_lsq(float *dists, uint32_t *ids, const uint8_t *codes, const float *queries,
                   const float *codebooks, const float *dbnorms, const float *R, int64_t n, int64_t nq,
                   int m, int h, int d, int k, int id_base);
int rq_linscan_cq(float *dists, uint32_t *ids, const uint8_t *codes, const float *queries,
                  const float *codebooks, int64_t n, int64_t nq, int m, int h, int d, int k, int id_base);
/* linscan_lsq over a PREPARED base (round 4): the pre-filter of the LSQ scan needs an O(n) pass over the base
 * (|c|^2 tables, per-row cross-term norms in float64, their range, one byte per row) that rq_linscan_lsq redoes on every
 * call because the ABI of deps/src/linscan_aqd_pairwise_byte.cpp:181-196 has no place to keep it (a cache keyed by the
 * pointers would be unsound: callers rewrite buffers in place).  The handle keeps codes, dbnorms, codebooks and that pass
 * on the device; searches upload queries only.  Same answers as rq_linscan_lsq (R may be NULL), bit for bit. */
typedef struct rq_lsq_index rq_lsq_index;
rq_lsq_index *rq_lsq_prepare(const uint8_t *codes, const float *codebooks, const float *dbnorms, int64_t n, int m,
                             int h, int d);
int rq_lsq_search(rq_lsq_index *ix, float *dists, uint32_t *ids, const float *queries, const float *R, int64_t nq,
                  int k, int id_base);
void rq_lsq_release(rq_lsq_index *ix);
/* The same handle from a norms codebook instead of per-row norms (the search leg of src/LSQ_GPU.jl:357-362, src/RVQ.jl:150-158:
 * quantize_norms, then db_norms = norms_C[B_base_norms]): dbnorms[i] = cbnorms[quantize(|sum_k C_k[b_ik]|^2)] is computed on the
 * device from the uploaded codes and codebooks, with the arithmetic of rq_aq_norms and rq_dev_quantize_norms below, so a base is
 * searched from codes, codebooks and a table of hn <= 256 floats alone.  Equals rq_lsq_prepare given those dbnorms, bit for bit;
 * rq_lsq_search and rq_lsq_release are unchanged.  NULL (message in rq_last_error) on a bad argument. */
rq_lsq_index *rq_lsq_prepare_cbnorms(const uint8_t *codes, const float *codebooks, const float *cbnorms, int hn, int64_t n,
                                     int m, int h, int d);
/* device-pointer form; lut_mode 1 = LSQ (dbnorms required), 2 = CQ */
int rq_dev_linscan_aq(float *dists, uint32_t *ids, uint64_t *keys, const uint8_t *codes,
                      const float *codebooks, const float *queries, const float *dbnorms, int64_t n,
                      int64_t nq, int m, int d, int k, int lut_mode, uint32_t id_offset, int id_base,
                      void *stream);

/* ---- database norms of additive-quantizer search: get_norms_codebook (src/utils.jl:4-26) and quantize_norms (:29-59).  Contract
 * in DESIGN.md section 4.14.  codes [n][m] uint8 zero-based, C [m][h][d] (m full-dimensional codebooks back to back), 1 <= m <= 64,
 * 2 <= h <= 256, d >= 1, 1 <= hn <= 256; n >= 0, and n >= hn for rq_get_norms_codebook.  Every argument (each code being below
 * h included) is checked before any work, errors go through rq_last_error and leave the outputs untouched.  Non-finite
 * codebook entries, norms or cbnorms give unspecified values, as for rq_train_rvq ("Non-finite inputs of the encode" below).
 *
 * rq_aq_norms (src/utils.jl:15-16, :34-48: reconstruct, then sum(CB.^2)): norms[i] = |sum_k C_k[b_ik]|^2 without the n x d
 * reconstruction, in veccost's order of f32 sums: CB[t] by adds from +0 in codebook order, 64 partial sums of CB[t]^2 over
 * t = l, l + 64, ... (multiply and add unfused), added by the xor butterfly 32, 16, 8, 4, 2, 1 -- the veccost of an all-zero X
 * (rq_encode_icm with no iterations), bit for bit. */
int rq_aq_norms(float *norms, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h);
int rq_dev_aq_norms(float *norms, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h, void *stream);
/* quantize_norms (src/utils.jl:29-59): norm_codes[i] = the FIRST index j (zero-based) that minimises fl(fl(norm - cbnorms[j])^2)
 * in f32 -- one subtract, one multiply, strict < like findmin (:50-55); cbnorms [hn] need not be sorted.  norms_out [n] (may be
 * NULL) = the norms themselves, equal to rq_aq_norms (the reference's second return value). */
int rq_quantize_norms(uint8_t *norm_codes, float *norms_out, const uint8_t *codes, const float *C, const float *cbnorms,
                      int64_t n, int d, int m, int h, int hn);
/* device-pointer form on norms already computed; dbnorms_out [n] (may be NULL) = cbnorms[norm_codes[i]], what linscan_lsq takes */
int rq_dev_quantize_norms(uint8_t *norm_codes, float *dbnorms_out, const float *norms, const float *cbnorms, int64_t n, int hn,
                          void *stream);
/* get_norms_codebook (src/utils.jl:4-26): Clustering.kmeans(dbnorms, hn) as the Lloyd loop of rq_train_pq with d = m = 1 on
 * the norms of rq_aq_norms, which stay on the device: cbnorms [hn] and the final assignments equal rq_train_pq(d = 1, m = 1,
 * h = hn) on those norms with the same niter and seed, bit for bit (and the call overwrites rq_train_profile likewise).
 * norm_codes [n] zero-based = the k-means' final assignments, like the reference's dbnormsq.assignments.  They come from the
 * encoder's distance form (|c|^2 - 2 c x, first index on ties), so for a norm near the edge of two cells they can differ from
 * rq_quantize_norms' (norm - c)^2 on the same codebook; a base searched with quantised norms should take rq_quantize_norms'.
 * norms_out [n] may be NULL. */
int rq_get_norms_codebook(uint8_t *norm_codes, float *cbnorms, float *norms_out, const uint8_t *codes, const float *C,
                          int64_t n, int d, int m, int h, int hn, int niter, uint64_t seed);
/* The same five over int16 codes, for the codes of rq_train_rvq_wide / rq_encode_rvq_wide: 1 <= m <= 64,
 * 2 <= h <= RQ_MAX_H16, 1 <= hn <= RQ_MAX_H16, code_base 0 or 1 (the device forms take zero-based codes); norm codes are int16 and
 * zero-based.  Same kernels instantiated for the wider code, same order of sums: at h, hn <= 256 the bits of the byte entries,
 * widened.  A code outside [0, h) (after code_base): RQ_EINVAL before any other work, outputs untouched.
 * rq_aq_norms_wide: src/utils.jl:15-16, :34-48.  rq_quantize_norms_wide: src/utils.jl:29-59, the unsorted table of hn entries in
 * LDS (128 KiB at most).  rq_get_norms_codebook_wide: src/utils.jl:4-26 as the resident Lloyd loop of rq_train_pq_wide with
 * d = m = 1, h = hn -- cbnorms and assignments equal that call on the same norms, niter and seed, bit for bit. */
int rq_aq_norms_wide(float *norms, const int16_t *codes, const float *C, int64_t n, int d, int m, int h, int code_base);
int rq_dev_aq_norms_wide(float *norms, const int16_t *codes, const float *C, int64_t n, int d, int m, int h, void *stream);
int rq_quantize_norms_wide(int16_t *norm_codes, float *norms_out, const int16_t *codes, const float *C, const float *cbnorms,
                           int64_t n, int d, int m, int h, int hn, int code_base);
int rq_dev_quantize_norms_wide(int16_t *norm_codes, float *dbnorms_out, const float *norms, const float *cbnorms, int64_t n,
                               int hn, void *stream);
int rq_get_norms_codebook_wide(int16_t *norm_codes, float *cbnorms, float *norms_out, const int16_t *codes, const float *C,
                               int64_t n, int d, int m, int h, int hn, int niter, uint64_t seed, int code_base);

/* ---- quantize_rvq (src/RVQ.jl:18-66) -----------------------------------------
 * m full-dimensional stages on the running residual: stage i = pairwise SqEuclidean + first-index
 * argmin against C[i] (d x h in Julia = [h][d] here; codebooks = the m matrices back to back), then
 * Xr .-= C[i][:, B[i]] (:56).  Any d.  codes [n][m] uint8 zero-based / Int16 one-based m x n
 * (:60-62).  counts [m][h] (may be NULL) = update_assignments!'s per-centre counts (:43-47): a zero marks
 * an `unused` centre, for which the reference re-picks a singleton with Julia's RNG (:50-53) -- that
 * random re-pick stays on the caller's side.  Xr_out [n][d] (may be NULL) receives the final residual. */
int rq_encode_rvq(uint8_t *codes, const float *X, const float *codebooks, int64_t n, int d, int m, int h,
                  uint32_t *counts, float *Xr_out);
int rq_encode_rvq_i16(int16_t *codes1, const float *X, const float *codebooks, int64_t n, int d, int m, int h,
                      uint32_t *counts, float *Xr_out);
/* train_rvq (src/RVQ.jl:86-127): one k-means of niter Lloyd iterations per stage on the running residual.
 * C [m][h][d] out; B1 [n][m] Int16 one-based out (== quantize_rvq(X, C)); *error = qerror(X, B, C).
 * Seeding: kmeans++ on the running residual like the reference (rq_kmpp_seeds), from the library's seeded
 * stream instead of Julia's global RNG, so results agree in objective, not bit for bit.  One stream serves the
 * whole call: every stage draws its h uniforms where the stage before (its repicks included) left off. */
int rq_train_rvq(float *C, int16_t *B1, double *error, const float *X, int64_t n, int d, int m, int h, int niter,
                 uint64_t seed);
/* device-pointer form: Xr [n][d] holds X on entry and the final residual on return */
int rq_dev_encode_rvq(uint8_t *codes, float *Xr, const float *codebooks, int64_t n, int d, int m, int h,
                      uint32_t *counts, void *stream);

/* ---- Beam-search residual encoding: CompetitiveQ's `encode` (src/CompetitiveQ.jl:75-135).  Contract in DESIGN.md section 2
 * ("Beam encoding contract").  Like quantize_rvq, but the H best partial encodings of each vector survive a stage instead of
 * one: stage i ranks the H_i * h candidates (parent j, codeword k) by (v, j * h + k), v = max(0, fl(fl(sa_k + sb_j) - 2 g_jk))
 * with k-ordered fmaf chains, and keeps the min(H, H_i * h) smallest; the answer is the rank-0 survivor of the last stage.
 * X [n][d], codebooks [m][h][d] as for rq_encode_rvq, codes [n][m] uint8 zero-based (Int16 one-based for _i16), cost_out [n]
 * = the answer's last-stage v and Xr_out [n][d] = its residual (either may be NULL).  1 <= m <= 64, 1 <= h <= 256,
 * 1 <= H <= 32 and H <= h, d >= 1, n >= 0, nsplits >= 1 (the minimum number of row chunks; results do not depend on it).
 * Every argument is checked before any work; a violation returns RQ_EINVAL through rq_last_error and writes no output byte.
 * H = 1 gives rq_encode_rvq's codes and residual bit for bit.  Non-finite inputs: the call returns, codes stay below h, the
 * values are unspecified.  train_competitiveq (src/CompetitiveQ.jl:138-221) is a per-sample SGD and is not provided. */
int rq_encode_rvq_beam(uint8_t *codes, const float *X, const float *codebooks, int64_t n, int d, int m, int h, int H,
                       int nsplits, float *cost_out, float *Xr_out);
/* src/CompetitiveQ.jl:75-135 with the reference's Int16 one-based codes */
int rq_encode_rvq_beam_i16(int16_t *codes1, const float *X, const float *codebooks, int64_t n, int d, int m, int h, int H,
                           int nsplits, float *cost_out, float *Xr_out);
/* src/CompetitiveQ.jl:75-135 on device pointers, queued on `stream`; X is NOT overwritten, scratch comes from the per-stream
 * workspace (at most 2 GiB: rows are chunked); Xr_out and cost_out may be NULL and are then not touched */
int rq_dev_encode_rvq_beam(uint8_t *codes, float *Xr_out, float *cost_out, const float *X, const float *codebooks, int64_t n,
                           int d, int m, int h, int H, int nsplits, void *stream);
/* src/CompetitiveQ.jl:75-135 with up to RQ_MAX_H16 codewords per stage: the contract above with
 * 1 <= h <= 256 replaced by 1 <= h <= RQ_MAX_H16 and nothing else changed; codes [n][m] int16 in code_base .. code_base + h - 1
 * (code_base 0 or 1).  h > RQ_MAX_H16 or m outside 1 .. 64 returns RQ_EUNSUPPORTED, every other violation RQ_EINVAL; no output
 * byte is written on an error.  H = 1 gives rq_encode_rvq_wide's codes and residual bit for bit; at h <= 256 the codes, costs
 * and residuals are rq_encode_rvq_beam's. */
int rq_encode_rvq_beam_wide(int16_t *codes, const float *X, const float *codebooks, int64_t n, int d, int m, int h, int H,
                            int nsplits, int code_base, float *cost_out, float *Xr_out);
/* src/CompetitiveQ.jl:75-135 on device pointers with up to RQ_MAX_H16 codewords per stage: rq_dev_encode_rvq_beam with int16
 * ZERO-based codes; errors as rq_encode_rvq_beam_wide */
int rq_dev_encode_rvq_beam_wide(int16_t *codes, float *Xr_out, float *cost_out, const float *X, const float *codebooks,
                                int64_t n, int d, int m, int h, int H, int nsplits, void *stream);
/* milliseconds of this thread's last beam call (src/CompetitiveQ.jl:75-135) by phase (hipEvents): {stage kernels, expand
 * kernels, other}; cap entries written.  After a device-pointer call it waits for that call's last event. */
int rq_last_beam_timing(double *ms, int cap);

/* ---- Enhanced RVQ / Stacked Quantizers: train_ervq (src/ERVQ.jl:51-135, arXiv 1411.2173).  Contract in DESIGN.md
 * section 2 ("ERVQ").  quantize_ervq IS quantize_rvq (src/ERVQ.jl:19-26): use rq_encode_rvq.  Layouts as for RVQ: X [n][d],
 * C [m][h][d] (m full-dimensional codebooks back to back, one entry per row).  1 <= m <= 64, 2 <= h <= 256, any d >= 1.
 * Every argument (each code's range included) is checked before any work; errors through rq_last_error.  Non-finite input
 * gives unspecified values under the guarantees of "Non-finite inputs of the encode" below (the call returns, codes in range,
 * the same bits twice), as for rq_train_rvq.
 *
 * The codebook update of one step alone (src/ERVQ.jl:85-90, Clustering.update_centers! unweighted): every entry k of block
 * j (zero-based, 0 <= j < m) that has rows becomes the mean of X - sum_{i != j} C_i[b_i] over the rows with b_j = k, computed
 * as C_j[k] + the mean of the full residual X - sum_i C_i[b_i] over those rows (the same value; in f32 closer to an f64
 * evaluation than the literal sum), in a fixed summation order without float atomics: bitwise reproducible.  C in/out: only
 * block j is written, an entry without rows keeps its bits, nothing is refilled.  codes [n][m] uint8 zero-based; counts [h]
 * out = the rows per entry of column j.  n >= 0. */
int rq_ervq_update_codebook(float *C, uint32_t *counts, const float *X, const uint8_t *codes, int64_t n, int d, int m,
                            int h, int j);
/* train_ervq(X, B, C, m, h, niter) (src/ERVQ.jl:51-135), device-resident.  C in: start codebooks, out: trained; B1 [n][m]
 * Int16 one-based in: start codes, out: final codes (== quantize_rvq(X, C) after every complete iteration).  For it = 0 ..
 * niter-1 and j = 0 .. m-1: the update above on codebook j; entries of j without rows are refilled; stages j .. m-1 are
 * encoded again (quantize_rvq on the residual entering stage j); the error is recorded.  obj (may be NULL) has niter*m + 1
 * doubles: obj[0] = qerror of the inputs, obj[1 + it*m + j] = qerror(X, B, C) after step j of iteration it; *error = the
 * last obj entry.  The trace need not fall from step to step: the greedy re-encode may lose what the update won.  niter = 0
 * leaves C and B1 untouched and reports their error.  n >= 1.
 * Entries without rows, for every j: Clustering.repick_unused_centers' rule on the residual entering stage j -- a row drawn
 * with probability proportional to its cost under the entry values the codes were assigned with, costs lowered after each
 * draw -- so a refilled entry is a row of that residual (of X for j = 0) bit for bit.  j = 0 follows the same rule as
 * j >= 1: the reference's own branch for its first codebook (src/ERVQ.jl:93-100) goes through a Julia-0.6 `sum(A, 1)` and
 * does not run on Julia >= 0.7.  The draws come from the library's stream seeded by `seed`, not from Julia's RNG, so
 * refilled entries differ from the reference's; without empty entries the result does not depend on `seed`. */
int rq_train_ervq(float *C, int16_t *B1, double *error, double *obj, const float *X, int64_t n, int d, int m, int h,
                  int niter, uint64_t seed);
/* The codebook update of one ERVQ step (src/ERVQ.jl:85-90) over Int16 codes, 2 <= h <= RQ_MAX_H16:
 * rq_ervq_update_codebook with codes [n][m] int16 in code_base .. code_base + h - 1 (code_base 0 or 1).  h > RQ_MAX_H16 or m
 * outside 1 .. 64 returns RQ_EUNSUPPORTED, every other violation (a code out of range included) RQ_EINVAL, and no output byte is
 * written.  At h <= 256 the result is rq_ervq_update_codebook's bit for bit. */
int rq_ervq_update_codebook_wide(float *C, uint32_t *counts, const float *X, const int16_t *codes, int64_t n, int d, int m,
                                 int h, int j, int code_base);
/* train_ervq (src/ERVQ.jl:51-135) with 2 <= h <= RQ_MAX_H16 entries per codebook: rq_train_ervq's contract at every h, B [n][m]
 * int16 in code_base .. code_base + h - 1 in and out.  Errors as rq_ervq_update_codebook_wide.  At h <= 256 C, B, error and
 * obj are rq_train_ervq's bit for bit (the same draws). */
int rq_train_ervq_wide(float *C, int16_t *B, double *error, double *obj, const float *X, int64_t n, int d, int m, int h,
                       int niter, uint64_t seed, int code_base);
/* milliseconds of this thread's last rq_train_ervq / rq_train_ervq_wide by phase (hipEvents), summed over the call: {initial residual,
 * increments, refills (with the read-back of the counts), stage encodes, epilogues, error passes, other (the uploads,
 * the code conversions)}; cap entries written */
int rq_last_ervq_timing(double *ms, int cap);

/* ---- LSQ encoding: encoding_icm (src/LSQ.jl:272-302) / encode_icm_cuda (src/LSQ_GPU.jl:218-264) -------------------
 * Iterated local search around ICM, contract in DESIGN.md section 2.  X [n][d], C [m][h][d] (m full-dimensional codebooks,
 * one codeword per row), codes [n][m] uint8 zero-based.  1 <= m <= 16, 2 <= h <= 256, d >= 1, 0 <= npert <= m,
 * ilsiter, icmiter, t0 >= 0, nsplits >= 1 (the minimum number of row chunks).  ILS iterations t0 .. t0+ilsiter-1 run, so a
 * checkpointed run continues the same random stream; results depend on neither nsplits nor the chunking.  codes_out may
 * alias codes_in; cost_out [n] (may be NULL) receives each row's final veccost.  Arguments (codes < h included) are checked
 * before any encode work; errors through rq_last_error.  Non-finite inputs give unspecified but in-range codes FOR THEIR OWN
 * ROWS: rows are encoded independently, so every other row keeps its codes and its cost (tests/test_gpu_nonfinite_aq.py; the
 * same holds for rq_quantize_chainq and rq_encode_rvq). */
int rq_encode_icm(uint8_t *codes_out, const uint8_t *codes_in, float *cost_out, const float *X, const float *C,
                  int64_t n, int d, int m, int h, int ilsiter, int icmiter, int npert, int randord, uint64_t seed,
                  int64_t t0, int nsplits);
/* device pointers, queued on `stream` (with h < 256 the code range check reads one flag back first) */
int rq_dev_encode_icm(uint8_t *codes_out, const uint8_t *codes_in, float *cost_out, const float *X, const float *C,
                      int64_t n, int d, int m, int h, int ilsiter, int icmiter, int npert, int randord, uint64_t seed,
                      int64_t t0, int nsplits, void *stream);
/* milliseconds of this thread's last rq_encode_icm / rq_encode_icm_wide: unaries (hipEvent, summed over chunks) and the whole call */
int rq_last_icm_timing(double *unary_ms, double *total_ms);
/* encoding_icm with 2 <= h <= RQ_MAX_H16 codewords per codebook: rq_encode_icm's contract word for word
 * over codes [n][m] int16 in code_base .. code_base + h - 1 (code_base 0 or 1), host pointers.  A kernel of its own whose register
 * use does not grow with h runs at EVERY h; at h <= 256 codes and costs are rq_encode_icm's bit for bit.  The tables must fit the
 * scratch budget: with HS = 64 * ceil(h / 64), m*m*h*HS*4 + m*h*4 bytes of tables plus four rows of unaries (m*HS*4 bytes each)
 * within 2 GiB -- (m, h) = (8, 2048) and (16, 1024) fit, (16, 2048) does not and returns RQ_EUNSUPPORTED.  Every other violation
 * (m outside 1 .. 16, h outside the range above, a code out of range, ...) is RQ_EINVAL; every check runs before any work and no
 * output byte is written on error.  There is no device-pointer form in the C ABI yet. */
int rq_encode_icm_wide(int16_t *codes_out, const int16_t *codes_in, float *cost_out, const float *X, const float *C,
                       int64_t n, int d, int m, int h, int ilsiter, int icmiter, int npert, int randord, uint64_t seed,
                       int64_t t0, int nsplits, int code_base);
/* rq_encode_icm_wide's shape rule and row chunks, no device touched: out[0 .. min(cap, 5) - 1] = {HS, bytes of the tables, bytes
 * of one row's unaries, rows per chunk, chunks} (the last two 0 when n = 0).  Returns what rq_encode_icm_wide would for the shape. */
int rq_icm_wide_plan(int64_t n, int d, int m, int h, int nsplits, int64_t *out, int cap);

/* ---- LSQ codebook update: update_codebooks(X, B, h, V, "fastbin") (src/codebook_update.jl:235-277) ->
 * update_codebooks_fast_bin (:175-206) -> fast_bin_matmul (:96-170).  Contract in DESIGN.md section 2.
 * X [n][d] f32, codes [n][m] uint8 zero-based, 1 <= m <= 16, 2 <= h <= 256, d >= 1, 0 <= n <= 2^32 - 1, rho finite > 0
 * (the reference's default is 1e-4).  A = B'B + rho I is [mh][mh] f64 with row / column i*h + a (exact integer counts;
 * the diagonal is fl64(count + rho)), b = B'X is [mh][d] f64 (each entry an f64 sum from +0 over the rows in ascending
 * order).  C [m][h][d] = (float) A^-1 b, solved in f64 on the device (Cholesky), bitwise reproducible; unused codes get
 * zero codewords.  Arguments (codes < h included) are checked before any other work; errors through rq_last_error. */
int rq_update_codebooks_lsq(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h, double rho);
/* device pointers, queued on `stream` (with h < 256 the code range check reads one flag back first) */
int rq_dev_update_codebooks_lsq(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h,
                                double rho, void *stream);
/* fast_bin_matmul (src/codebook_update.jl:96-170): the normal equations A [mh][mh] and b [mh][d] alone (device) */
int rq_dev_lsq_normal_eq(double *A, double *b, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h,
                         double rho, void *stream);
/* train_lsq (src/LSQ.jl:323-372) / train_lsq_cuda (src/LSQ_GPU.jl:267-319), device-resident: C = update(R'X, codes),
 * C_i <- R C_i, encode; then niter times { obj[iter] = qerror; C = update(X, codes); encode }, rho = 1e-4.  Encode call e
 * (0 = the initial one) runs ILS iterations e*ilsiter .. (e+1)*ilsiter - 1 of one `seed` stream (rq_encode_icm), so the
 * result depends on neither nsplits nor the chunking.  C [m][h][d] out; codes [n][m] in: start codes, out: final codes;
 * obj [niter] f64 out (mean veccost after the previous encode; NaN when n = 0, a mean of no rows); R [d][d] memory image
 * of Julia's R, NULL = identity. */
int rq_train_lsq(float *C, uint8_t *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m, int h,
                 int niter, int ilsiter, int icmiter, int npert, int randord, uint64_t seed, int nsplits);
/* milliseconds of this thread's last rq_update_codebooks_lsq[_wide] / rq_lsq_normal_eq_wide / rq_train_lsq[_wide] by phase
 * (hipEvents; the device entries leave zeros), summed over a training call's updates: {counts, sort, b, assemble A, solve, other
 * training work (R'X, the rotation back, the obj means, the code_base shifts), encodes (training)}; cap entries written */
int rq_last_lsq_timing(double *ms, int cap);

/* ---- the LSQ codebook update and training with 2 <= h <= RQ_MAX_H16 codewords per codebook: the
 * contracts above word for word over codes [n][m] int16 in code_base .. code_base + h - 1 (code_base 0 or 1), host pointers.
 * The int16 kernels run at EVERY h; at h <= 256 A, b, C, obj and the codes are those of the byte entries bit for bit.  The
 * normal equations take m * h <= 16384 (A is then at most 2 GiB of f64, the u32 pair counts 1 GiB): a larger m * h returns
 * RQ_EUNSUPPORTED.  Every other violation (m outside 1 .. 16, h outside the range above, n outside 0 .. 2^32 - 1, rho not finite
 * and > 0, a null pointer, a code out of range, ...) is RQ_EINVAL.  Every check runs before any work and before a device is
 * needed; no output byte is written on error.  There is no device-pointer form in the C ABI yet. */
int rq_update_codebooks_lsq_wide(float *C, const float *X, const int16_t *codes, int64_t n, int d, int m, int h, double rho,
                                 int code_base);
/* fast_bin_matmul alone: A [mh][mh] and b [mh][d] f64 as rq_dev_lsq_normal_eq defines them, and counts [m][h] = the rows per
 * (codebook, code).  A may be NULL: then b and counts alone are produced, no mh x mh buffer is allocated and the m * h limit does
 * not apply (any h <= RQ_MAX_H16 with m <= 16).  counts may be NULL. */
int rq_lsq_normal_eq_wide(double *A, double *b, uint32_t *counts, const float *X, const int16_t *codes, int64_t n, int d, int m,
                          int h, double rho, int code_base);
/* rq_update_codebooks_lsq_wide's shape rule and sizes, no device touched: out[0 .. min(cap, 7) - 1] = {m * h, bytes of A, bytes
 * of the pair counts, bytes of the sort scratch (tile histograms, segment bounds, per-code counts, row lists), tiles of 4096
 * rows, Cholesky block steps (64 wide), 1 when rq_train_lsq_wide can run the shape too (rq_icm_wide_plan passes) else 0}.
 * Returns what rq_update_codebooks_lsq_wide would for the shape; out is written on RQ_OK only. */
int rq_lsq_wide_plan(int64_t n, int d, int m, int h, int64_t *out, int cap);
/* rq_train_lsq over int16 codes: the same steps, the encodes through the encoder of rq_encode_icm_wide (ILS iterations
 * e*ilsiter .. (e+1)*ilsiter - 1 of one `seed` stream for encode call e, so the result depends on neither nsplits nor the
 * chunking).  The shape must pass rq_icm_wide_plan AND m * h <= 16384, else RQ_EUNSUPPORTED.  codes in and out carry code_base. */
int rq_train_lsq_wide(float *C, int16_t *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m, int h,
                      int niter, int ilsiter, int icmiter, int npert, int randord, uint64_t seed, int nsplits, int code_base);

/* ---- LSQ++: stochastic relaxations of LSQ (src/SR.jl, src/SR_perturbations.jl).  Contract in DESIGN.md section 2
 * ("SR noise").  The reference draws from Julia's global randn; here the noise is a counter-based standard normal
 * variate z(seed, kind, call, element index) that tests/sr_oracle.py restates bit for bit, so results depend on
 * neither nsplits, the chunking nor the run. */
#define RQ_SR_C 0           /* noise on the data (SR_C_perturb) */
#define RQ_SR_D 1           /* noise on the codebooks (SR_D_perturb) */
/* Statistics.std(X, dims=2) (src/SR_perturbations.jl:38, :62): sigma [d] = the sample standard deviation (divisor n - 1)
 * of every column of X [n][d]; a two-pass f64 reduction in a fixed order, rounded to f32, bitwise reproducible.  n >= 2
 * (the reference gives NaN below that), d >= 1. */
int rq_sr_std(float *sigma, const float *X, int64_t n, int d);
/* The noise of SR_C_perturb (src/SR_perturbations.jl:67-70) and SR_D_perturb (:41-46):
 * Y[r][j] = (float)((double)X[r][j] + z * ((double)sigma[j] * scale)), z = z(seed, kind, call, (row0 + r) * d + j).
 * X, Y [n][d] (Y may alias X), sigma [d]; kind RQ_SR_C or RQ_SR_D; call >= 0 numbers the perturbation call of a training
 * run; row0 >= 0 is the first row's index in that call's whole array, so a slice gives the same rows; scale finite. */
int rq_sr_perturb(float *Y, const float *X, const float *sigma, double scale, int64_t n, int d, int kind, uint64_t seed,
                  int64_t call, int64_t row0);
/* apply_schedule (src/SR_perturbations.jl:4-25), the factor alone, f64 on the host (no device is touched):
 * schedule 1: (1 - iter/niter)^p, 2: 1/(1 + iter)^p (the reference divides stdev by the power: at most one f64 rounding
 * apart), 3: p^(iter/2); any other schedule is an error.  niter >= 1, iter >= 0 (<= niter for schedule 1), p finite and
 * >= 0; a scale that does not come out finite is an error. */
int rq_sr_schedule(double *scale, int schedule, int64_t iter, int64_t niter, double p);
/* train_sr_cuda (src/SR.jl:88-176; clean_update = 1) / train_sr (:4-84; clean_update = 0, schedule 1), device-resident:
 * RX = R'X; step(0); for it = 1..niter { obj[it-1] = qerror(RX, codes, C); step(it); if clean_update: C = update(RX,
 * codes) }; obj[niter] = qerror; C_i <- R C_i.  step(call) is, for method RQ_SR_C, C = update(perturb(RX)), and for
 * RQ_SR_D, C = perturb(update(RX)) with sigma = rq_sr_std of C as [m h][d], / m in f32; then codes = encode(RX, codes, C)
 * with ILS iterations call * ilsiter .. of one `seed` stream (rq_encode_icm).  The perturbation of call `call` has the
 * scale of schedule iteration `call`, except that RQ_SR_D's call 0 has that of iteration 1 (:127).  update is
 * rq_update_codebooks_lsq with rho = 1e-4; qerror is the mean of a fresh veccost pass against the current C.
 * C [m][h][d] out; codes [n][m] in: start codes, out: final codes; obj [niter + 1] f64 out; R [d][d] memory image of
 * Julia's R, NULL = identity.  Limits of rq_train_lsq, and niter >= 1, n >= 2 for RQ_SR_C.  Every argument is checked
 * before any device work. */
int rq_train_sr(float *C, uint8_t *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m, int h,
                int niter, int ilsiter, int icmiter, int npert, int randord, int method, int schedule, double p,
                int clean_update, uint64_t seed, int nsplits);
/* milliseconds of this thread's last rq_train_sr[_wide] by phase (hipEvents), summed over the call: {standard deviations,
 * perturbations, codebook updates, encodes, obj passes, other (the uploads, R'X, the rotation back, the code_base shifts)}; cap
 * entries written */
int rq_last_sr_timing(double *ms, int cap);
/* ---- LSQ++ with 2 <= h <= RQ_MAX_H16 codewords per codebook: rq_train_sr's contract word for word over
 * codes [n][m] int16 in code_base .. code_base + h - 1 (code_base 0 or 1), host pointers.  The int16 kernels (the update of
 * rq_update_codebooks_lsq_wide, the encoder of rq_encode_icm_wide) run at EVERY h; at h <= 256 C, codes and obj are rq_train_sr's
 * bit for bit.  The shape rule is rq_train_lsq_wide's: it passes rq_icm_wide_plan AND m * h <= 16384, else RQ_EUNSUPPORTED.  Every
 * other violation (m, h, d, n, niter, nsplits, method, schedule, p, code_base, a null pointer, a code out of range, RQ_SR_C with
 * n < 2, the ILS counter overflow, an unknown bit in flags) is RQ_EINVAL.  Every check runs before any work and before a device
 * is needed; no output byte is written on error.  The result depends on neither nsplits nor the chunking.
 * With clean_update = 1 every step after the first opens with an update over the codes of the clean update that closed the step
 * before.  flags = 0 does not repeat that work: RQ_SR_D's opening update has the same inputs, so C holds its result already and it
 * is skipped; RQ_SR_C's has the same matrix B'B + rho I, so the Cholesky factor, the segment bounds and the sorted row lists are
 * kept and only b = B'(noisy RX) and the two substitution sweeps run.  What is kept lives inside the one call.  RQ_SR_RECOMPUTE
 * computes every update from scratch; both settings give the same bits. */
#define RQ_SR_RECOMPUTE 1
int rq_train_sr_wide(float *C, int16_t *codes, double *obj, const float *X, const float *R, int64_t n, int d, int m, int h,
                     int niter, int ilsiter, int icmiter, int npert, int randord, int method, int schedule, double p,
                     int clean_update, uint64_t seed, int nsplits, int code_base, int flags);
/* the codebook updates of this thread's last rq_train_sr[_wide]: out[0 .. min(cap, 3) - 1] = {computed in full, computed from the
 * kept Cholesky factor and row sort, skipped outright}; rq_train_sr computes every update in full */
int rq_last_sr_stats(int64_t *out, int cap);

/* ---- Chain quantization (src/ChainQ.jl).  Contract in DESIGN.md section 2 ("Chain quantization").
 * Layouts as for LSQ: X [n][d], C [m][h][d] (m full-dimensional codebooks, one codeword per row; a trained chain quantizer
 * is zero outside rq_chain_dims, but any C is accepted), codes [n][m] uint8 zero-based.  1 <= m <= 16, 2 <= h <= 256, d >= 1.
 *
 * quantize_chainq (src/ChainQ.jl:305-348; replaces quantize_chainq_cuda! :204-285 with the viterbi_forward / vec_add
 * kernels of src/CudaUtilsModule.jl, and viterbi_encoding, deps/src/encode_icm.cpp:63-152): the exact minimiser of the
 * chain energy sum_i U_i[b_i] + sum_i T_i[b_{i+1}][b_i] by the Viterbi recursion, all in f32, lowest index on ties.  The
 * codes are a pure function of (X, C): they depend on neither nsplits (the minimum number of row chunks, >= 1) nor the
 * chunking.  Arguments are checked before any device work; errors through rq_last_error.  Non-finite inputs give
 * unspecified but in-range codes. */
int rq_quantize_chainq(uint8_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int nsplits);
/* device pointers, queued on `stream`; no n-sized array goes to the host */
int rq_dev_quantize_chainq(uint8_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int nsplits,
                           void *stream);
/* get_cbdims_chain (src/codebook_update.jl:280-294): codebook i of a chain quantizer covers dimensions lo[i] .. hi[i]-1
 * (zero-based, half open; lo, hi hold m ints); part i of splitarray(1:d, m-1) is lo[i+1] .. hi[i]-1.  2 <= m <= 16,
 * d >= m - 1. */
int rq_chain_dims(int d, int m, int *lo, int *hi);
/* update_codebooks_chain_bin (src/codebook_update.jl:367-412): A, b as rq_dev_lsq_normal_eq; for i = 0 .. m-2 the
 * 2h x 2h block A[ih:(i+2)h, ih:(i+2)h] is solved (f64 Cholesky on the device where the reference calls getrf / getrs)
 * against b[ih:(i+2)h, part i]; rows 0..h-1 go to C_i, rows h..2h-1 to C_{i+1}, everything else in C is an exact zero.
 * 2 <= m <= 16, d >= m - 1, rho finite and > 0.  Bitwise reproducible.  Arguments (codes < h included) are checked
 * before any other work. */
int rq_update_codebooks_chain(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h, double rho);
/* device pointers, queued on `stream` (with h < 256 the code range check reads one flag back first) */
int rq_dev_update_codebooks_chain(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h,
                                  double rho, void *stream);
/* CB [n][d] = sum_i C_i[codes[.][i]]: f32 adds from +0 in codebook order (the CB of src/ChainQ.jl:411-412), device pointers */
int rq_dev_reconstruct_aq(float *CB, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h, void *stream);
/* train_chainq (src/ChainQ.jl:373-431), device-resident: RX = R'X; C = chain update(RX, codes); codes = viterbi(RX, C);
 * then niter + 1 rounds { obj[iter] = qerror(RX, codes, C); CB = reconstruct; R = polar factor of X CB' (where the
 * reference takes an SVD); RX = R'X; C = chain update; codes = viterbi }, rho = 1e-4.  No random numbers.  C [m][h][d]
 * out; codes [n][m] in: start codes, out: final codes; R [d][d] memory image of Julia's R, in: start rotation, out: final;
 * obj [niter + 1] f64 out.  n >= 1, 2 <= m <= 16, m - 1 <= d <= 1024 (the device polar factor); a rank-deficient X CB' is
 * reported as RQ_EUNSUPPORTED. */
int rq_train_chainq(float *C, uint8_t *codes, float *R, double *obj, const float *X, int64_t n, int d, int m, int h,
                    int niter);
/* ---- chain quantization with 2 <= h <= RQ_MAX_H16 codewords per codebook: the contracts of
 * rq_quantize_chainq, rq_update_codebooks_chain and rq_train_chainq word for word over codes [n][m] int16 in code_base ..
 * code_base + h - 1 (code_base 0 or 1), host pointers; m as for the byte entries.  The int16 kernels run at EVERY h; at h <= 256
 * the codes, C, R and obj are those of the byte entries bit for bit (on finite inputs; non-finite inputs give unspecified but
 * in-range codes, as there).
 * Shape rule of the encoder: with HS = 64 * ceil(h / 64), the tables take T = 2 * (m - 1) * h * HS * 4 + m * h * 4 bytes (both
 * orientations of the m - 1 pair tables, and the self-products) and one row of unaries m * HS * 4 bytes; T plus 32 rows must fit
 * 2 GiB, else RQ_EUNSUPPORTED; rows per chunk = min(ceil(n / nsplits), (2 GiB - T) / row bytes).  (m, h) = (8, 4096), (16, 2048)
 * and (4, 8192) fit; (2, 16384) does not.  The update and training also need 2 h <= 16384 (one 2h x 2h f64 block is then at
 * most 2 GiB; no (m h)^2 matrix is built), else RQ_EUNSUPPORTED; training keeps d <= 1024 and needs the encoder's rule.  Every
 * other violation (m, h, d, n, nsplits, niter, rho, code_base out of range, a null pointer, a code outside its range) is
 * RQ_EINVAL.  Every check runs before any work and before a device is needed; no output byte is written on error.  There is no
 * device-pointer form of these entries in the C ABI yet. */
int rq_quantize_chainq_wide(int16_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int nsplits,
                            int code_base);
int rq_update_codebooks_chain_wide(float *C, const float *X, const int16_t *codes, int64_t n, int d, int m, int h, double rho,
                                   int code_base);
int rq_train_chainq_wide(float *C, int16_t *codes, float *R, double *obj, const float *X, int64_t n, int d, int m, int h,
                         int niter, int code_base);
/* The shape rule and sizes of the entries above, no device touched: out[0 .. min(cap, 7) - 1] = {HS, table bytes T, bytes of one
 * row's unaries, rows per chunk, chunks (both 0 when n = 0), bytes of the update's 2h x 2h f64 block, 1 when
 * rq_update_codebooks_chain_wide AND rq_train_chainq_wide can run the shape (m >= 2, m - 1 <= d <= 1024, 2 h <= 16384) else 0}.
 * Returns what rq_quantize_chainq_wide would for the shape; out is written on RQ_OK only. */
int rq_chain_wide_plan(int64_t n, int d, int m, int h, int nsplits, int64_t *out, int cap);
/* milliseconds of this thread's last host-pointer chain call (byte or int16 entries) by phase (hipEvents; the device entries
 * leave zeros), summed over a training call: {unaries, pair tables + self-products, forward pass + back trace, codebook updates, rotation work
 * (R'X, reconstruction, qerror, X CB', polar factor)}; cap entries written */
int rq_last_chainq_timing(double *ms, int cap);

/* ---- host-pointer entry points (what the julia/ shims ccall) ----------------------------------
 * rq_encode_*: X is uploaded in ~128 MB chunks while the previous chunk is encoded (the call is PCIe-bound).  With
 * RAYUELA_HIP_DEVICES listing several devices the rows are split over them, one host thread and one PCIe link
 * per device; rq_linscan_* then shard the base (see the index handle below). */
/* linscan_pq (src/Linscan.jl:5-26).  id_base = 1 folds Julia's `res .+= 1` into the kernel.
 * Supported row widths: 1 <= m <= 64 (other widths are zero-padded to 2, 4, 8, 16, 32 or 64).  The integer pre-filter that
 * carries the BASELINE shapes exists for the 4-, 8- and 16-byte tilings (round-6 figures, 1e6 rows x 1e4 queries, k = 1000, resident:
 * m = 8: 1.9 ms, m = 16: 4.6 ms, m = 4: 1.3 ms); m = 2, 32 and 64 run the exact f32 loop (m = 32: 4.9 ms for
 * 5e5 rows x 4096 queries) -- same answers, not tuned. */
int rq_linscan_pq(float *dists, uint32_t *ids, const uint8_t *codes, const float *centers,
                  const float *queries, int64_t n, int64_t nq, int m, int d, int k, int id_base);
/* Non-finite inputs (every scan entry point; tests/test_gpu_nonfinite.py, tests/test_gpu_nonfinite_aq.py; the contract in plain
 * numpy: tests/nonfinite_ref.py, pinned to the oracle by tests/test_nonfinite_ref.py).  The reference builds its table and its distances in
 * plain f32 (deps/src/linscan_aqd.cpp:66-87) and hands the pairs to std::partial_sort (:91-97): +Inf is an ordinary value there
 * (ties part by id), while a NaN breaks the pair comparison's strict weak order -- the reference's answer for such a query is
 * unspecified.  Here:
 *   - the call always returns: no threshold, redo, barrier or pacing path waits on a poisoned query;
 *   - +Inf / -Inf in a query or a codebook behave as in the reference, bit for bit (a query with an infinite coordinate has
 *     distance +Inf to every row and gets the k smallest ids);
 *   - a row whose distance to a query is NaN is never a neighbour of that query (NaN compares false with every threshold).  The
 *     rows with comparable distances are returned exactly, in (dist, id) order; a list that runs out of them ends in the padding
 *     pair (dist = NaN, id = 0xFFFFFFFF + id_base, i.e. 0 on the one-based Julia side: "no row");
 *   - the other queries of the same 8-query group and of the same launch are unaffected, bit for bit (a group that holds a
 *     NaN query takes the exact, un-sampled path: slower, same answer).  No status is raised: the poisoned rows are data.
 * A NaN is a NaN whatever its sign bit (0x7FC00000 as well as the 0xFFC00000 that x86 gives for Inf - Inf) and whatever produced
 * it (a NaN input, Inf - Inf, 0 x Inf inside a table); the padding distance is the bit pattern 0x7FFFFFFF, a packed key KEY_MAX.
 * dbnorms (rq_linscan_lsq, the *_extra_byte symbols, rq_dev_linscan_aq, rq_lsq_prepare) are row data like the codes: a NaN entry
 * takes its row out of every query's answer, a +Inf / -Inf entry gives the row that distance (unless the row's table sum is the
 * opposite infinity: NaN again), exactly as `acc + dbnorms[row]` does in the reference.  The LSQ pre-filter's preparation pass
 * leaves NaN residual norms out of the range it quantises and is switched off by an infinite one; neither changes an answer.
 * Intermediates that overflow (2 * q of the LSQ table at |q| > 1.7e38) are infinities like any other, denormal tables and
 * norms keep their bits (nothing is flushed to zero). */
/* linscan_opq (src/Linscan.jl:93-103): queries are rotated by R' on the device first. */
int rq_linscan_opq(float *dists, uint32_t *ids, const uint8_t *codes, const float *centers,
                   const float *queries, const float *R, int64_t n, int64_t nq, int m, int d,
                   int k, int id_base);
/* Non-finite inputs of the encode at h <= 256 -- rq_encode_pq / rq_encode_opq, their rq_dev_*, _i16, _bytes and
 * rq_dataset_encode forms, rq_rotate_T, every kernel the dispatch can choose (tests/test_gpu_nonfinite_encode.py; the oracle
 * side of it on the same inputs: tests/test_nonfinite_encode_ref.py):
 *   1. the call returns RQ_OK and every code written is below h (1 .. h in the one-based forms);
 *   2. rows are encoded independently: a finite row under finite codebooks has the reference arithmetic's codes, bit for
 *      bit, whatever the other rows of its tile, chunk or launch hold;
 *   3. sub-quantizers are independent: a non-finite entry of codebook i leaves column j != i of every finite row unchanged;
 *      column i is in range and otherwise unspecified;
 *   4. a sub-vector whose every distance is NaN (any NaN coordinate; an Inf coordinate that makes every u_k NaN) gets code 0,
 *      which is what max(NaN, 0) = 0 with a strict `<` gives in the reference arithmetic.  Other poisoned sub-vectors (mixed
 *      Inf / NaN distances, |x|^2 overflowing to +Inf) are in range and otherwise unspecified;
 *   5. rotation: a finite row under a finite R is R'x bit for bit; a poisoned row is NaN exactly where the k-ordered fmaf chain
 *      is NaN and bit-equal where that is finite or +-Inf.  With a non-finite R the call returns, no further claim;
 *   6. the OPQ encode is 5 followed by 1 - 4.
 * Training on a base with non-finite rows (rq_train_pq, rq_train_opq, rq_train_rvq, rq_kmpp_seeds, rq_train_ervq,
 * rq_ervq_update_codebook with in-range codes): the call returns RQ_OK or a negative status with a message, B1 lies in 1 .. h,
 * the seeds in [0, n), every row is counted once per stage, and the same call gives the same bits twice.  Codebooks, R and the
 * objective are unspecified (one non-finite row turns every centre of its sub-space into NaN: the segment sums are matrix
 * products).
 * Non-finite inputs of training -- at h > 256 and of LSQ / chain / SR training (tests/test_gpu_nonfinite_train.py; inputs and CPU
 * restatements in tests/nonfinite_train_cases.py, held to the oracles by tests/test_nonfinite_train_ref.py):
 *   a. the reductions are column-wise -- a non-finite coordinate (row r, column c) of X reaches column c of the result only.
 *      rq_dev_update_centers / rq_dev_update_centers_wide: counts exact, row r counted; every column != c has the bits it has
 *      when column c of X holds zeros; a code without rows keeps its bits in every column; the same bits twice, NaN payloads
 *      included; column c unspecified (the matrix-core kernel meets 0 x NaN in every code of the column, the owner-thread
 *      kernel of TRAIN_CENTERS_MFMA = 0 only in the code of row r).  rq_dev_reconstruct_wide copies NaN, Inf and denormal
 *      entries of C bit for bit.  rq_dev_lsq_normal_eq: A depends on the codes alone; b is NaN exactly where the f64 sums in
 *      ascending row order are NaN and bit-equal elsewhere (a segmented sum: m cells of column c per poisoned row).
 *      rq_[dev_]update_codebooks_lsq / _chain: the solve keeps right-hand-side columns apart (one thread per column in the
 *      triangular solves, one output column per accumulator in the updates; no coupled tiles), so every column != c of C is
 *      bit-equal to the call on X with column c zeroed and within the finite-data tolerances of the f64 solve; the host entry
 *      equals the device entry bit for bit; column c unspecified; RQ_OK or a negative status with a message.  rq_sr_std:
 *      sigma[k], k != c, keeps its bits, sigma[c] is what the f64 two-pass arithmetic gives (NaN for NaN / Inf);
 *      rq_sr_perturb with a NaN / Inf sigma[c]: column c of Y non-finite, every other column unchanged; a non-finite scale
 *      is refused;
 *   b. the training loops -- rq_train_pq_wide, rq_train_opq_wide (with or without R0 / C0), rq_train_rvq_wide, rq_train_lsq,
 *      rq_train_sr (both methods, with and without the clean update), rq_train_chainq -- on a base with a non-finite or
 *      overflowing row: RQ_OK or one of the negative codes with a message, never a hipError_t; on RQ_OK every code in range and
 *      obj of its documented length; the same bits twice on every output; a finite call right afterwards returns its usual bits
 *      (no device state is left behind).  With the returned codes the reductions of (a) count every row once, and an encode
 *      with the returned (possibly non-finite) centres is in range.  rq_train_pq_wide at h <= 256 stays the bits of rq_train_pq.
 *      rq_train_chainq refuses such a base with RQ_EUNSUPPORTED (the polar factor of X CB' does not converge) and writes no
 *      output; were it to return RQ_OK, R is orthonormal to 1e-5 or holds a NaN.  Centres, R and objective unspecified. */
/* quantize_pq (src/PQ.jl:18-48): codes [n][m] uint8 zero-based.  h <= 256. */
int rq_encode_pq(uint8_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h);
/* quantize_opq (src/OPQ.jl:19-27). */
int rq_encode_opq(uint8_t *codes, const float *X, const float *R, const float *C, int64_t n,
                  int d, int m, int h);
/* Same, but emitting Julia's return type directly: Int16, ONE-based, m x n (src/PQ.jl:45-47). */
int rq_encode_pq_i16(int16_t *codes1, const float *X, const float *C, int64_t n, int d, int m,
                     int h);
int rq_encode_opq_i16(int16_t *codes1, const float *X, const float *R, const float *C, int64_t n,
                      int d, int m, int h);
/* ---- more than 256 codewords per codebook: 16-bit codes.  The reference returns Matrix{Int16} from
 * quantize_pq, quantize_opq and quantize_rvq so that a codebook may hold more than 256 entries (src/PQ.jl:45-47,
 * src/RVQ.jl:60-62).  Every entry point above keeps refusing h > 256 (their codes are bytes); these accept 1 <= h <= RQ_MAX_H16.
 * Same arithmetic, wider index: code = first index of the minimum over ALL k in [0, h) of v_k = (u_k > 0 ? u_k : 0),
 * u_k = fl(fl(sa_k + sb) - 2 g_k), strict '<'; a NaN u_k becomes 0 through the clamp, a row of +Inf values gets index 0, a code
 * is always < h.  h <= 256 returns exactly the codes of the u8 entry points (it runs their kernels and widens);
 * rq_last_encode_kernel names "encode_h16_kernel" after a call that ran the streaming kernel.  Layouts of the u8 entry points:
 * codes [n][m] int16, C the m [h][sub_i] blocks back to back, codebooks [m][h][d], counts [m][h] or NULL.  code_base: 0
 * (zero-based) or 1 (Julia's one-based Matrix{Int16}), like id_base of the scans.  n <= 0: RQ_OK.  A NULL pointer, a bad
 * code_base or d < m: RQ_EINVAL; h > RQ_MAX_H16 or m out of range (PQ / OPQ: 1..32, RVQ: 1..64): RQ_EUNSUPPORTED; on any error
 * no output byte is written.  Wide codes are scanned by the *_wide scans below (rq_linscan_pq_wide, rq_dev_linscan_wide); the byte
 * scans stay at h = 256 (deps/src/linscan_aqd.cpp:58,67). */
/* quantize_pq with up to RQ_MAX_H16 codewords per sub-codebook (src/PQ.jl:18-48). */
int rq_encode_pq_wide(int16_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int code_base);
/* quantize_opq with up to RQ_MAX_H16 codewords per sub-codebook (src/OPQ.jl:19-27). */
int rq_encode_opq_wide(int16_t *codes, const float *X, const float *R, const float *C, int64_t n, int d, int m, int h,
                       int code_base);
/* quantize_rvq with up to RQ_MAX_H16 codewords per stage (src/RVQ.jl:18-66); counts and Xr_out as for rq_encode_rvq. */
int rq_encode_rvq_wide(int16_t *codes, const float *X, const float *codebooks, int64_t n, int d, int m, int h, int code_base,
                       uint32_t *counts, float *Xr_out);
/* ---- the ADC scan over 16-bit codes: linscan_pq / linscan_opq for 1 <= h <= RQ_MAX_H16.  The reference has no
 * such scan (deps/src/linscan_aqd.cpp:58,67 hard-wire 256 entries per table); this is its arithmetic with `256` replaced by h:
 * T[k][r] = sum_s (c[(k h + r) sub + s] - q[k sub + s])^2 in sequential f32 (deps/src/linscan_aqd.cpp:66-74), row distance
 * ((T[0][b0] + T[1][b1]) + ...) + T[m-1][b_{m-1}] (:78-87), answer: the k smallest (dist, id) pairs in lexicographic order (:91-97),
 * exact for every 1 <= k <= n -- at h = 256 bit for bit the answer of the byte scans.  One path for every k: a packed key per row
 * and query, then the select / sort chain of the bulk top-k (rq_dev_linscan), in query batches inside the same 2 GiB of scratch
 * per device and stream (8 n + 16 k bytes per query, plus the tables); a base whose keys do not fit for a single query (above
 * about 2.1e8 rows) goes through in row slices whose sorted lists are folded into a running list -- the same answer, bit for
 * bit (rq_scan_wide_slices) -- and the out-of-memory error is left for a k whose lists alone exceed the budget.  The non-finite
 * contract above holds unchanged.  codes [n][m] int16, centers
 * [m][h][d/m], 1 <= m <= 32, d % m == 0, 1 <= k <= n < 2^31.  code_base: 0 (zero-based) or 1 (Julia's Matrix{Int16}), as in the
 * wide encodes.  A code outside [0, h) (after code_base): the host entries validate the codes on the device before any output is
 * written and return RQ_EINVAL naming the first bad row (the reference's InexactError of convert(Matrix{UInt8}, B .- 1),
 * src/Linscan.jl:35); the device entry never makes such a row a neighbour (its key is KEY_MAX for every query, the table index is
 * clamped).  nq <= 0: RQ_OK.  A NULL pointer, a bad code_base or id_base, d % m != 0, k outside [1, n], n >= 2^31: RQ_EINVAL; h
 * outside [1, RQ_MAX_H16] or m outside [1, 32]: RQ_EUNSUPPORTED; on any error no output byte is written.  With several devices in
 * RAYUELA_HIP_DEVICES the host entries use the first.  rq_last_scan_kernel names the distance kernel:
 * "adc_keys_h16_kernel<4, true>" (queries per gather, table in LDS). */
/* linscan_pq over 16-bit codes (src/Linscan.jl:5-37; deps/src/linscan_aqd.cpp:66-97 with h entries per table). */
int rq_linscan_pq_wide(float *dists, uint32_t *ids, const int16_t *codes, const float *centers, const float *queries,
                       int64_t n, int64_t nq, int m, int h, int d, int k, int code_base, int id_base);
/* linscan_opq over 16-bit codes (src/Linscan.jl:93-115): queries are rotated by R' on the device first. */
int rq_linscan_opq_wide(float *dists, uint32_t *ids, const int16_t *codes, const float *centers, const float *queries,
                        const float *R, int64_t n, int64_t nq, int m, int h, int d, int k, int code_base, int id_base);
/* ---- the additive-quantizer scan over 16-bit codes: linscan_lsq / linscan_cq for 1 <= h <= RQ_MAX_H16,
 * what searches the Int16 codes of rq_train_rvq_wide / rq_encode_rvq_wide (src/RVQ.jl:139-158).  The contract is
 * deps/src/linscan_aqd_pairwise_byte.cpp:14-94 (LSQ) and :97-176 (CQ) with `unsigned char *codes` replaced by a zero-based int16
 * -- its arithmetic already takes h at run time (tentry[h*k + code[k]]).  All f32, every operation rounded on its own:
 *   LSQ table  T[j] = T[j] - (2 q[k]) * c[j][k], k = 0..d-1 from +0 (:42-49);  CQ table  T[j] = T[j] + (q[k]-c[j][k]) * (q[k]-c[j][k])
 *   (:124-131);  row distance acc = 0, acc = acc + T[h k + b_k] for k = 0..m-1, then for LSQ acc = acc + dbnorms[row] (:70-74);
 *   answer: the k smallest (dist, id) pairs in lexicographic order, exact for every 1 <= k <= n (:82-88).
 * codes [n][m] int16, codebooks [m*h][d] (m full-dimensional codebooks back to back), 1 <= m <= 32, d >= 1 (no d % m rule),
 * 1 <= k <= n < 2^31, code_base 0 or 1.  "Non-finite inputs" above holds unchanged: a NaN distance -- also one that comes from
 * dbnorms -- is never a neighbour, -0 becomes +0, a short list ends in the padding pair.  A code outside [0, h), statuses, the
 * "no output byte written on error" rule, nq <= 0, scratch and the device used: exactly as for rq_linscan_pq_wide.  At h = 256 the
 * answers are those of rq_linscan_lsq / rq_linscan_cq bit for bit.  rq_last_scan_kernel names the keys kernel:
 * "adc_keys_h16_kernel<4, true, true>" (queries per gather, table in LDS, row norm added; CQ shares the PQ instantiation and its
 * name).  The rq_lsq_prepare handle stays byte-only. */
/* linscan_lsq over 16-bit codes (src/Linscan.jl:118-157; deps/src/linscan_aqd_pairwise_byte.cpp:14-94); R may be NULL */
int rq_linscan_lsq_wide(float *dists, uint32_t *ids, const int16_t *codes, const float *queries, const float *codebooks,
                        const float *dbnorms, const float *R, int64_t n, int64_t nq, int m, int h, int d, int k,
                        int code_base, int id_base);
/* linscan_cq over 16-bit codes (src/Linscan.jl:160-193; deps/src/linscan_aqd_pairwise_byte.cpp:97-176) */
int rq_linscan_cq_wide(float *dists, uint32_t *ids, const int16_t *codes, const float *queries, const float *codebooks,
                       int64_t n, int64_t nq, int m, int h, int d, int k, int code_base, int id_base);
/* The search leg of src/RVQ.jl:147-155 in one call: dbnorms[i] = cbnorms[quantize(|sum_k C_k[b_ik]|^2)] computed on the device from
 * the uploaded codes with the arithmetic of rq_quantize_norms_wide (2 <= h, 1 <= hn <= RQ_MAX_H16), then the scan; equals
 * rq_linscan_lsq_wide given those dbnorms, bit for bit. */
int rq_linscan_lsq_cbnorms_wide(float *dists, uint32_t *ids, const int16_t *codes, const float *queries,
                                const float *codebooks, const float *cbnorms, int hn, const float *R, int64_t n, int64_t nq,
                                int m, int h, int d, int k, int code_base, int id_base);
/* ---- byte rows: quantize_pq / quantize_opq of UInt8 data without widening it on the host.
 * bvecs files (SIFT1B: bigann_base / learn / query) hold UInt8 vectors -- bvecs_read returns Matrix{UInt8},
 * src/xvecs_read.jl:14-52 -- and the reference converts them to Float32 on the host before it encodes them
 * (src/read_datasets.jl:148-167: convert(Matrix{Float32}, X)).  These take X [n][d] uint8 as it lies in the file and
 * return, for every input, byte for byte the codes of the f32 entry point on the widened matrix (u8 -> f32 is exact);
 * a quarter of the bytes cross PCIe (chunks of max(32768, 2^25 / d) rows, as the f32 calls use, double buffered; tuning
 * HOST_OVERLAP = 0: one buffer, no overlap).  Every (d, m, h) the f32 entry points accept is accepted: even sub-space
 * widths <= 16 run the filter + exact pass with byte loaders (rq_last_encode_kernel: "encode_pq_filter_bytes_kernel"),
 * rotations of d in {32, 64, 96, 128} a byte-loading rotation; every other shape is widened on the device into a bounded
 * scratch and takes the f32 kernels (rq_last_encode_kernel then names the f32 kernel).  Statuses, rq_last_timing and
 * rq_last_encode_stats as the f32 entry points; a NULL pointer is RQ_EINVAL. */
/* quantize_pq on UInt8 data (src/xvecs_read.jl:14-52, src/read_datasets.jl:148-167; src/PQ.jl:18-48). */
int rq_encode_pq_bytes(uint8_t *codes, const uint8_t *X, const float *C, int64_t n, int d, int m, int h);
/* quantize_opq on UInt8 data (src/xvecs_read.jl:14-52, src/read_datasets.jl:148-167; src/OPQ.jl:19-27). */
int rq_encode_opq_bytes(uint8_t *codes, const uint8_t *X, const float *R, const float *C, int64_t n,
                        int d, int m, int h);
/* The same with Julia's return type: Int16, ONE-based, m x n (src/xvecs_read.jl:14-52, src/read_datasets.jl:148-167;
 * src/PQ.jl:45-47). */
int rq_encode_pq_bytes_i16(int16_t *codes1, const uint8_t *X, const float *C, int64_t n, int d, int m,
                           int h);
int rq_encode_opq_bytes_i16(int16_t *codes1, const uint8_t *X, const float *R, const float *C, int64_t n,
                            int d, int m, int h);
/* A base set kept on the device: upload X [n][d] once (to the calling thread's current device), encode it as often
 * as needed -- quantize_pq and quantize_opq of the same Xb with different codebooks / rotations pay PCIe once
 * (from host memory quantize_pq is upload-bound: ~9 ms of PCIe against 0.7 ms of kernel per 1e6 x 128).
 * rq_dataset_encode: R == NULL -> quantize_pq (src/PQ.jl:18-48), else quantize_opq (src/OPQ.jl:19-27); codes
 * [n][m] uint8 zero-based and/or codes1 m x n Int16 one-based (either may be NULL). */
typedef struct rq_dataset rq_dataset;
rq_dataset *rq_dataset_upload(const float *X, int64_t n, int d);
/* The same for UInt8 rows (src/xvecs_read.jl:14-52, src/read_datasets.jl:148-167): the base stays n d BYTES on the device
 * (1e9 x 128: 128 GB, which fits one MI355X; as f32 it would not).  rq_dataset_encode / rq_dataset_free work on either
 * kind; R'X of a byte base lives chunk-wise in scratch. */
rq_dataset *rq_dataset_upload_bytes(const uint8_t *X, int64_t n, int d);
int rq_dataset_encode(rq_dataset *ds, uint8_t *codes, int16_t *codes1, const float *R, const float *C, int m, int h);
void rq_dataset_free(rq_dataset *ds);
/* ---- byte rows and resident bases with more than 256 codewords per codebook: the contract of
 * rq_encode_pq_wide / rq_encode_opq_wide -- codes [n][m] int16, code_base 0 or 1, 1 <= h <= RQ_MAX_H16, 1 <= m <= 32, the same
 * statuses, no output byte written on error -- on UInt8 rows as they lie in a bvecs file (src/xvecs_read.jl:14-52; the reference
 * widens on the host, src/read_datasets.jl:148-167).  The codes are bit for bit those of the f32 wide entry on the widened
 * matrix: PQ at h > 256 runs the streaming kernel with a byte loader (X at any byte alignment; rq_last_encode_kernel keeps
 * naming "encode_h16_kernel"), OPQ rotates chunks of max(32768, 2^25 / d) byte rows into scratch and encodes them as f32, and
 * h <= 256 runs the kernels of rq_encode_{pq,opq}_bytes and widens their codes.  The host-pointer entries upload in the double-
 * buffered chunks of the byte calls above. */
/* quantize_pq on UInt8 data, up to RQ_MAX_H16 codewords per sub-codebook (src/xvecs_read.jl:14-52, src/read_datasets.jl:148-167;
 * src/PQ.jl:18-48). */
int rq_encode_pq_bytes_wide(int16_t *codes, const uint8_t *X, const float *C, int64_t n, int d, int m, int h, int code_base);
/* quantize_opq on UInt8 data, up to RQ_MAX_H16 codewords per sub-codebook (src/xvecs_read.jl:14-52, src/read_datasets.jl:148-167;
 * src/OPQ.jl:19-27). */
int rq_encode_opq_bytes_wide(int16_t *codes, const uint8_t *X, const float *R, const float *C, int64_t n, int d, int m, int h,
                             int code_base);
/* rq_dataset_encode with up to RQ_MAX_H16 codewords per sub-codebook, on a resident base of either kind (rq_dataset_upload,
 * rq_dataset_upload_bytes): R == NULL -> quantize_pq (src/PQ.jl:18-48), else quantize_opq (src/OPQ.jl:19-27). */
int rq_dataset_encode_wide(rq_dataset *ds, int16_t *codes, const float *R, const float *C, int m, int h, int code_base);
/* RX = R' * X (src/OPQ.jl:26, src/Linscan.jl:102). */
int rq_rotate_T(float *RX, const float *R, const float *X, int d, int64_t n);

/* ---- exact k-nearest-neighbour ground truth.  There is no reference function: the reference only
 * READS ground truth, from the *_groundtruth.ivecs / gt files of src/read_datasets.jl, and consumes it in eval_recall
 * (src/Linscan.jl:196-234); every experiment_* driver takes it as `gt`.  These entries produce it on the device.
 *
 * Base X [n][d] (f32, or u8 widened exactly), queries Q [nq][d] f32, every operation rounded on its own (no contraction):
 *   D32(i, q): acc = +0; for s = 0..d-1: t = x[s] - q[s]; acc = acc + t * t   in f32 -- the arithmetic of linscan_cq's table
 *              (deps/src/linscan_aqd_pairwise_byte.cpp:124-131) with the base as one codebook of n entries
 *   D64(i, q): the same loop on the values widened to f64, in f64
 * rq_knn_f32 (stage 1 alone): the k smallest (D32, id) pairs in lexicographic order, any 1 <= k <= n, keys packed as the scans pack
 *   them and the scans' "Non-finite inputs" rules unchanged: a NaN distance is never a neighbour, -0 becomes +0, a short list ends
 *   in the padding pair (distance bits 0x7FFFFFFF, id 0xFFFFFFFF + id_base).
 * rq_knn / rq_knn_bytes / rq_dataset_knn (the ground truth): the k smallest (D64, id) pairs in lexicographic order, 1 <= k <=
 *   RQ_KNN_MAX_K, dists f64, ids u32 + id_base; a pair whose D64 is NaN is never a neighbour; a list with fewer than k such rows
 *   ends in the scans' padding id with distance +Inf.  For EVERY input: stage 1 is only a filter with a proven bound,
 *   |D32 - D64| <= gamma D64 + delta, gamma = 2 (d + 3) 2^-24, delta = d 2^-125 (finite inputs, no f32 overflow).  Per query the
 *   k' = min(n, k + max(32, k / 4)) stage-1 candidates are evaluated in f64; with T64 the k-th smallest D64 among them and L the
 *   D32 of the last candidate (+Inf taken as FLT_MAX) the query is certified iff k' == n, or the candidate list ran out of
 *   comparable rows, or L > T64 (1 + gamma) + delta in f64, strictly.  A query that is not certified is rerun with k' <- min(n, 4 k')
 *   until it is; past k' = 4096 the D64 values go to the host and std::partial_sort finishes the query.
 * The host-pointer forms upload the whole base (out-of-memory status if it does not fit); rq_dataset_knn runs in place on a
 * resident base of either kind.  Synchronous on the calling thread's current device.  nq <= 0: RQ_OK.  A NULL pointer, k outside
 * [1, n], a bad id_base, d < 1, n >= 2^31: RQ_EINVAL; k > RQ_KNN_MAX_K in the f64 entries: RQ_EUNSUPPORTED; on any error no output
 * byte is written.
 * rq_last_knn_stats: [0] queries, [1] candidates evaluated in f64, [2] queries widened at least once, [3] widening rounds,
 *   [4] queries finished on the host, [5] row chunks, [6..7] 0.  rq_last_knn_timing: ms of upload, keys, select, fold, rerank,
 *   widen, download of the calling thread's last call.  rq_knn_plan (host only): out[0] k' of the first round, [1] rows per
 *   chunk, [2] row chunks, [3] queries per batch, [4] scratch bytes of a batch, [5] 1 when the test hook rq_test_knn_chunk_rows set [1]. */
#define RQ_KNN_MAX_K 1024
int rq_knn_f32(float *dists, uint32_t *ids, const float *base, const float *queries, int64_t n, int64_t nq, int d, int k,
               int id_base);
int rq_knn(double *dists, uint32_t *ids, const float *base, const float *queries, int64_t n, int64_t nq, int d, int k,
           int id_base);
int rq_knn_bytes(double *dists, uint32_t *ids, const uint8_t *base, const float *queries, int64_t n, int64_t nq, int d, int k,
                 int id_base);
int rq_dataset_knn(rq_dataset *ds, double *dists, uint32_t *ids, const float *queries, int64_t nq, int k, int id_base);
int rq_last_knn_stats(uint64_t *out8);
int rq_last_knn_timing(double *ms, int cap);
int rq_knn_plan(int64_t n, int64_t nq, int d, int k, int64_t *out, int cap);

/* ---- exact re-ranking of search candidates on a resident base.  The reference has no such step: its
 * searches return neighbours ranked by the quantized distance and eval_recall (src/Linscan.jl:196-234) takes them as they come.
 * Faiss calls this step "refine" (IVFADC+R).
 *
 * Base X [n][d] resident (rq_dataset_upload[_bytes]: f32, or u8 widened exactly), queries Q [nq][d] f32 (host), candidates
 * cand [nq][ldc] u32 (host) of which the first kc per query count; ldc >= kc, and what lies behind kc is never read.
 *   row        r = (c - id_base - id_offset) mod 2^32; the candidate is valid iff r < n, everything else is skipped -- so is the
 *              scans' padding id 0xFFFFFFFF + id_base, which is never valid because n + id_offset <= 2^32 - 1 is required
 *   distance   D32(r, q) exactly as the section "exact k-nearest-neighbour" above defines it: one accumulator per pair walks
 *              s = 0..d-1 in order from +0, every operation rounded on its own
 *   answer     per query the k smallest (D32, r) pairs in lexicographic order among the valid candidates, ids r + id_offset +
 *              id_base; the scans' "Non-finite inputs" rules unchanged (a NaN distance is never a neighbour, -0 becomes +0, +Inf
 *              distances order by id); a list with fewer than k such pairs ends in the padding pair (distance bits 0x7FFFFFFF,
 *              id 0xFFFFFFFF + id_base).  A candidate id given twice appears twice: there is NO dedupe.  With cand = all n ids the
 *              answer is rq_knn_f32's.
 *   errors     checked before any work and before any output byte is written: a NULL pointer, k < 1, kc < k, ldc < kc, kc >= 2^31,
 *              a bad id_base, n + id_offset > 2^32 - 1: RQ_EINVAL; one query whose keys (and, past 4096 candidates, select
 *              scratch) do not fit the bulk scratch budget: RQ_EUNSUPPORTED; nq <= 0: RQ_OK.
 * rq_dataset_rerank: the contract above, synchronous on the dataset's device.
 * rq_ivf_search_refine (declared with the rq_ivf entries below): rq_ivf_search with kc in place of k, its sorted top-kc keys
 *   re-ranked on the device against `ds` without a host round trip.  By definition it equals rq_dataset_rerank over the ids
 *   rq_ivf_search(..., k = kc, id_base) returns, bit for bit; id_offset is the id of row 0 of `ds` (the id_offset the rows were
 *   loaded with).  ds on another device than ix, or ds.d != ix.d: RQ_EINVAL.
 * rq_last_rerank_timing: ms of [0] upload, [1] keys, [2] select, [3] download of the calling thread's last call ([1], [2] alone
 *   after rq_ivf_search_refine).  rq_last_rerank_stats: [0] queries, [1] candidates, [2] valid candidates, [3] batches, [4] the
 *   select path (0: one workgroup per query sorts in LDS, kc <= 4096; 1: the select chain of the bulk top-k), [5] keys per query
 *   row, [6..7] 0.  rq_rerank_plan (host only): out[0] queries per batch (0: one query does not fit), [1] scratch bytes of a
 *   batch, [2] the select path, [3] keys per query row, [4] 1 when the test hook rq_test_rerank_limits set the batch. */
int rq_dataset_rerank(rq_dataset *ds, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, const uint32_t *cand_host,
                      int64_t kc, int64_t ldc, int k, uint32_t id_offset, int id_base);
int rq_last_rerank_timing(double *ms, int cap);
int rq_last_rerank_stats(uint64_t *out8);
int rq_rerank_plan(int64_t n, int64_t nq, int d, int64_t kc, int k, int64_t *out, int cap);

/* ---- device-pointer entry points: asynchronous on `stream` (a hipStream_t, NULL = default).
 * All pointers are device pointers on the current device, 16-byte aligned. ------------------ */
int rq_dev_encode_pq(uint8_t *codes, const float *X, const float *C, int64_t n, int d, int m,
                     int h, void *stream);
int rq_dev_rotate_T(float *RX, const float *R, const float *X, int d, int64_t n, void *stream);
/* Name of the kernel the calling thread's last encode call ran ("encode_pq_split_kernel", "encode_pq_direct_kernel", ...):
 * bench.py labels its encode roofline with it instead of guessing from the tuning. */
const char *rq_last_encode_kernel(void);
/* With tuning ENC_STATS = 1 (measurement aid; adds a synchronisation per encode): out2[0] = (vector, sub-quantizer) pairs of the
 * calling thread's last encode through the filter kernels, out2[1] = how many of them the filter could not settle and the exact
 * pass re-evaluated (1.5 % on SIFT-like, 0.5 % on Deep-like bench data).  Zeros when ENC_STATS was off. */
int rq_last_encode_stats(uint64_t *out2);
/* The scan kernel instantiation the calling thread's last linscan launched, spelled as rocprofv3 prints it
 * ("adc_scan_kernel<8, false, true, false>"; the bulk path's distance kernel: "adc_bulk_keys_kernel<8, false>");
 * "" before the first scan.  bench.py replays committed PMC traffic figures
 * only for the very instantiation (and library build) they were measured on. */
const char *rq_last_scan_kernel(void);
/* Test aid (no reference counterpart): rq_dev_encode_pq through the split kernel (even sub-space widths <= 16), which also
 * stores the values its bf16 matrix-core FILTER decides on: W [n][m][h], W_k = |c_k|^2 - 2 <c_k, x> as the MFMAs produced it.
 * tests/test_gpu_encode_margin.py measures |(W_k + |x|^2) - v_k| against the bound the kernel's exactness rests on. */
int rq_dev_encode_pq_filter_w(uint8_t *codes, float *W, const float *X, const float *C, int64_t n, int d, int m,
                              int h, void *stream);
/* Fused rotate+encode is an implementation detail; tmp may be NULL (library workspace). */
int rq_dev_encode_opq(uint8_t *codes, const float *X, const float *R, const float *C, int64_t n,
                      int d, int m, int h, void *stream);
/* Device-pointer forms of the byte entry points (src/xvecs_read.jl:14-52, src/read_datasets.jl:148-167): X uint8 [n][d]
 * at ANY byte alignment (the kernels pick the widest load X, d and the sub-space width allow, down to single bytes);
 * every other pointer 16-byte aligned.  Codes / R'X are bit for bit those of rq_dev_encode_pq / rq_dev_encode_opq /
 * rq_dev_rotate_T on the widened rows.  Scratch: the stream's workspace, bounded by max(32768, 2^25 / d) rows of f32. */
int rq_dev_encode_pq_bytes(uint8_t *codes, const uint8_t *X, const float *C, int64_t n, int d, int m,
                           int h, void *stream);
int rq_dev_encode_opq_bytes(uint8_t *codes, const uint8_t *X, const float *R, const float *C, int64_t n,
                            int d, int m, int h, void *stream);
int rq_dev_rotate_T_bytes(float *RX, const float *R, const uint8_t *X, int d, int64_t n, void *stream);
/* Device-pointer forms of the *_wide entry points: zero-based int16 codes [n][m], everything on `stream` (norms pass, kernels,
 * memsets and the stream's workspace).  quantize_pq (src/PQ.jl:18-48): */
int rq_dev_encode_pq_wide(int16_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, void *stream);
/* quantize_opq (src/OPQ.jl:19-27): R'X into the stream's workspace, then the wide encode. */
int rq_dev_encode_opq_wide(int16_t *codes, const float *X, const float *R, const float *C, int64_t n, int d, int m, int h,
                           void *stream);
/* quantize_rvq (src/RVQ.jl:18-66): Xr [n][d] holds X on entry and the final residual on return. */
int rq_dev_encode_rvq_wide(int16_t *codes, float *Xr, const float *codebooks, int64_t n, int d, int m, int h,
                           uint32_t *counts, void *stream);
/* Per-query ADC look-up tables lut [nq][m][256] (deps/src/linscan_aqd.cpp:66-74); test aid. */
int rq_dev_adc_lut(float *lut, const float *centers, const float *queries, int64_t nq, int m,
                   int subdim, void *stream);
/* The ADC scan + exact top-k over one resident shard of n rows (1 <= m <= 64, h = 256, 1 <= k <= n < 2^31).
 * k <= RQ_MAX_K runs the candidate-buffer scan (adc_scan_kernel); RQ_MAX_K < k <= n the bulk path (rq_bulk.hip: one key per
 * row and query, radix select, radix sort; same answer, bit for bit), whose scratch is at most 2 GiB per device and stream --
 * 8 n + 16 k bytes per query of a batch; a single query that needs more fails with the out-of-memory error.
 *   dists/ids [nq][k] (may both be NULL when keys != NULL)
 *   keys      [nq][k] uint64 or NULL: sorted packed (ordered-dist << 32 | id) per query, the
 *             form exchanged between shards/GPUs and consumed by rq_dev_merge_topk
 *   id_offset added to every row index (global id of the shard's first row)
 *   id_base   0 or 1, added to ids written to `ids` only (keys stay zero-based)           */
int rq_dev_linscan(float *dists, uint32_t *ids, uint64_t *keys, const uint8_t *codes,
                   const float *centers, const float *queries, int64_t n, int64_t nq, int m,
                   int d, int k, uint32_t id_offset, int id_base, void *stream);
/* The ADC scan + exact top-k over one resident shard of n rows of ZERO-based int16 codes (deps/src/linscan_aqd.cpp:66-97 with h
 * entries per table; see rq_linscan_pq_wide).  dists / ids / keys, id_offset and id_base exactly as for rq_dev_linscan, so shards
 * merge through rq_dev_merge_topk unchanged.  codes 2-byte aligned (rows are loaded with the widest load the row pitch 2 m and
 * the pointer allow), centers and queries 4-byte aligned (16 for vector loads of the codebook rows).  Everything runs on
 * `stream`. */
int rq_dev_linscan_wide(float *dists, uint32_t *ids, uint64_t *keys, const int16_t *codes, const float *centers,
                        const float *queries, int64_t n, int64_t nq, int m, int h, int d, int k,
                        uint32_t id_offset, int id_base, void *stream);
/* Per-query ADC look-up tables lut [nq][m][h] of centers [m][h][subdim] (deps/src/linscan_aqd.cpp:66-74 with h entries per
 * table); test aid: the table's bits can be pinned apart from the scan. */
int rq_dev_adc_lut_wide(float *lut, const float *centers, const float *queries, int64_t nq, int m, int h, int subdim,
                        void *stream);
/* linscan_lsq / linscan_cq over one resident shard of ZERO-based int16 codes (deps/src/linscan_aqd_pairwise_byte.cpp:14-94,
 * :97-176 with h entries per codebook; see rq_linscan_lsq_wide): codebooks [m*h][d], lut_mode 1 = LSQ (dbnorms [n] required),
 * 2 = CQ (dbnorms ignored).  dists / ids / keys, id_offset and id_base exactly as for rq_dev_linscan_wide, so shards merge through
 * rq_dev_merge_topk unchanged; a row with a code outside [0, h) is never returned.  codes 2-byte aligned, the float arrays 4-byte
 * aligned (16 and d % 4 == 0 for vector loads of the codebook rows).  Everything runs on `stream`. */
int rq_dev_linscan_aq_wide(float *dists, uint32_t *ids, uint64_t *keys, const int16_t *codes, const float *codebooks,
                           const float *queries, const float *dbnorms, int64_t n, int64_t nq, int m, int h, int d, int k,
                           int lut_mode, uint32_t id_offset, int id_base, void *stream);
/* Per-query tables lut [nq][m][h] of codebooks [m*h][d] (deps/src/linscan_aqd_pairwise_byte.cpp:42-49 for lut_mode 1 = LSQ,
 * :124-131 for 2 = CQ, with h entries per codebook); test aid: the table's bits can be pinned apart from the scan. */
int rq_dev_aq_lut_wide(float *lut, const float *codebooks, const float *queries, int64_t nq, int m, int h, int d,
                       int lut_mode, void *stream);
/* Host-only: where rq_dev_linscan_wide keeps the table of m * h entries (no reference counterpart; the reference's table is a
 * heap array, deps/src/linscan_aqd.cpp:58).  out[0] queries per gather (4, 2 or 1), out[1] 1: the table of a query group is in
 * LDS, 0: gathered from global memory, out[2] queries per group, out[3] LDS bytes.  cap >= 4. */
int rq_scan_wide_plan(int m, int h, int *out, int cap);
/* Host-only: how rq_dev_linscan_wide / rq_dev_linscan_aq_wide (and every entry built on them) take a base of n rows and nq queries
 * through the 2 GiB scratch budget (no reference counterpart: deps/src/linscan_aqd.cpp:78-97 keeps one heap per query on the host).
 * A base whose 8 n bytes of keys fit for one query is one slice and launches what it always did.  A longer one is cut into row
 * slices: per slice the keys kernel and the select chain, then a fold of the slice's sorted list into the running one (P = 2
 * merge); keys are (dist, global id) pairs, so the answer is bit for bit that of an unsliced scan.  The slice is the longest for
 * which one query group (rq_scan_wide_plan's out[2]; the nq queries when fewer) fits, evened out over the slices.
 * out[0] rows per slice (the last may be shorter), [1] slices, [2] queries per batch, [3] scratch bytes of a batch, [4] 1 when
 * the test hook rq_test_scan_wide_slice_rows forced [0].  cap >= 5.  The out-of-memory status is left where one slice of one
 * query group plus 32 k bytes of lists do not fit (very large k); bad shapes: RQ_EINVAL / RQ_EUNSUPPORTED as the scan gives. */
int rq_scan_wide_slices(int64_t n, int64_t nq, int m, int h, int k, int64_t *out, int cap);
/* Bank-aware row order of a resident base (round 4, csrc/rq_order.hip).  No reference counterpart: the reference scans
 * rows in arrival order (deps/src/linscan_aqd.cpp:78-89); the result of the scan -- the k smallest (dist, id) pairs, :91-97
 * -- does not depend on the order rows are visited in, so this is a data-layout choice in HBM, invisible in the answer.
 * The scan's table gathers are LDS-bank-conflict bound; rows sorted by the top 3 bits of their leading code bytes make
 * the 32 lanes of a gather hit 32 distinct bank columns (SIFT1M shape: 2.45 -> 2.1 ms at k = 1000, more on larger bases).
 *   rq_dev_linscan           orders a scratch copy itself when that pays (tuning SCAN_ORDER = 1: from ORDER_MIN_NQ = 2048
 *                            queries and ORDER_MIN_ROWS = 65536 rows on; ~40 us per 1e6 rows, inside the call's time) and
 *                            KEEPS the copy per device and stream: every later call compares its codes, on the device and
 *                            byte for byte, with a snapshot kept next to the copy and orders again only when they differ, so
 *                            codes rewritten in place or re-allocated at the same address are safe; a kept copy is balanced
 *                            on its second use.  Hidden scratch: n * (2 * w + 8) bytes, w = rq_scan_row_width(m), until
 *                            rq_release_workspaces; over ORDER_MAX_SCRATCH_MB without the snapshot's n * w the call orders
 *                            uncached, as before (rq_order_cache_stats counts what happened)
 *   rq_index_set_codes[_synth]  order every shard once, at load time (tuning INDEX_ORDER = 1)
 *   rq_dev_order_rows        the same for callers that keep device-resident codes: `ordered` (rq_order_bytes(n, m) bytes,
 *                            16-byte aligned) receives the permuted rows, padded to rq_scan_row_width(m) bytes each, and
 *                            perm [n] (position -> original row); *codes_out / *perm_out point into it (*perm_out = NULL
 *                            for a base too small to order)
 *   rq_dev_linscan_ordered   rq_dev_linscan over such a pair: ids / keys carry ORIGINAL row numbers (+ id_offset)   */
int rq_scan_row_width(int m);
/* host-only (tests): the key of that order for n rows x m bytes -- out[0..7] bits per leading code byte, [8] total,
 * [9] rows per lane group, [10] rows per shuffle granule, [11] padded row width; cap >= 12.  With cap >= 14 also [12] the number
 * of tables the greedy balance deals the rows of a sort bucket over (round 6: 8- and 16-byte rows from ~7.9e5 rows = ~7.4e5 sorted
 * rows up to ~6e6 (m = 8) / ~4.4e6 (m = 16); the key then covers one table less; 0: plain sort -- the same predicate as the launch) and [13] the wavefronts per workgroup that run it. */
int rq_order_plan(int64_t n, int m, int *out, int cap);
int64_t rq_order_bytes(int64_t n, int m);
int rq_dev_order_rows(void *ordered, const uint8_t **codes_out, const uint32_t **perm_out, const uint8_t *codes,
                      int64_t n, int m, void *stream);
int rq_dev_linscan_ordered(float *dists, uint32_t *ids, uint64_t *keys, const uint8_t *codes_ordered,
                           const uint32_t *perm, const float *centers, const float *queries, int64_t n,
                           int64_t nq, int m, int d, int k, uint32_t id_offset, int id_base, void *stream);
/* Merge P sorted key lists per query: keys_in [nq][P][k] -> dists/ids [nq][k] (and/or
 * keys_out [nq][k]).  Total order on (dist,id) makes the result identical to a single scan. */
int rq_dev_merge_topk(float *dists, uint32_t *ids, uint64_t *keys_out, const uint64_t *keys_in,
                      int64_t nq, int P, int k, int id_base, void *stream);
/* code[i][j] = splitmix64(seed ^ ((row0+i)*m+j)) >> 56 : SIFT1B-shape synthetic shard. */
int rq_dev_synth_codes(uint8_t *codes, int64_t n, int m, uint64_t seed, int64_t row0, void *stream);

/* ---- the reductions of the PQ / OPQ training loops (device pointers) ----------
 * The assignment step of train_pq / train_opq is rq_dev_encode_pq and R'X is rq_dev_rotate_T; these add:
 *   update_centers  Clustering.update_centers! as called at src/OPQ.jl:121: C_i[k] <- mean of the
 *                   sub-vectors with code k; counts [m][h] out; an EMPTY cluster keeps its old centre
 *                   (the reference multiplies by 1/0 there)
 *   reconstruct     CB[j][subdims_i] = C_i[:, b_ji]                        (src/OPQ.jl:101,128)
 *   qerror          *acc = sum_j |X_j - CB_j|^2 in double (divide by n on the host; src/OPQ.jl:108)
 *   gram            G[a][b] = sum_j X[j][a] * CB[j][b], the d x d input of the SVD at src/OPQ.jl:112
 * Float summation orders differ from the reference's sequential loops: tolerance parity (tests/); the order
 * is fixed (one owner thread per (code, dimension), rows ascending), so results are bit-reproducible. */
int rq_dev_update_centers(float *C, uint32_t *counts, const float *X, const uint8_t *codes, int64_t n,
                          int d, int m, int h, void *stream);
int rq_dev_reconstruct(float *CB, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h,
                       void *stream);
int rq_dev_qerror(double *acc, const float *X, const float *CB, int64_t n, int d, void *stream);
int rq_dev_gram(float *G, const float *X, const float *CB, int64_t n, int d, void *stream);
/* The same two reductions with CB given as (codes [n][m] u8, C): CB[j][off_i + s] = C_i[codes[j][i]][s] is gathered inside the
 * kernels instead of being written out by rq_dev_reconstruct first (src/OPQ.jl:101,108,112 without the n x d temporary).
 * Shapes: d % 4 == 0, every sub-space starts on a multiple of 4, h <= 256, gram: d <= 256; RQ_EUNSUPPORTED otherwise. */
int rq_dev_gram_codes(float *G, const float *X, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h, void *stream);
int rq_dev_qerror_codes(double *acc, const float *X, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h, void *stream);

/* train_pq (src/PQ.jl:68-99) and train_opq (src/OPQ.jl:49-139) on host pointers: X [n][d]; outputs
 * C (concat of the m [h][sub_i] codebooks), B1 [n][m] Int16 ONE-based, R [d][d] (memory image of Julia's R),
 * obj [niter+1], *error = qerror_pq of the result.  init: 0 "natural", 1 "random".  R0 / C0 may be NULL;
 * when given they replace the random initialisation.  Every training entry point is bit-reproducible for a
 * given seed / start (segment sums in the matrix cores' fixed order, fixed reduction trees, a reproducible step count of the
 * polar iteration).  `seed` feeds the library's own
 * splitmix64 stream -- the reference uses Julia's global RNG, so equal seeds do not mean equal draws.
 * The k-means of train_pq / train_rvq against Clustering.kmeans (v0.12.2, what src/PQ.jl:86 and src/RVQ.jl:104 call):
 *   seeding      kmeans++ (init=:kmpp), the same law, other draws;
 *   empty centre re-drawn with probability proportional to the points' current cost, costs lowered to the distance to each
 *                new centre before the next draw (Clustering.repick_unused_centers), other draws;
 *   stopping     Clustering: |objv - prev_objv| < 1e-6 absolute on a Float32 sum of costs, or maxiter; here: no assignment
 *                changed, or niter -- the same iteration whenever the objective exceeds ~10 (float32 resolution above 1e-6:
 *                an unchanged rounded objective then means unchanged assignments); data of tiny magnitude (objective below
 *                ~10) stops EARLIER in Clustering than here;
 *   all sub-spaces iterate together and stop together (a sub-space that is stationary early is recomputed to the same bits).
 * tests/test_gpu_train.py holds the final error against oracle/train_oracle.py::train_pq_clustering (those rules) on 3 seeds. */
int rq_train_pq(float *C, int16_t *B1, double *error, const float *X, int64_t n, int d, int m, int h,
                int niter, uint64_t seed);
/* kmeans++ seeding as train_pq / train_rvq use it (Clustering.jl init=:kmpp, call sites src/PQ.jl:86 and
 * src/RVQ.jl:104): per sub-space the first seed is a uniformly drawn row, every further one is drawn with
 * probability proportional to the squared distance to the nearest seed so far.  seeds [m][h] (rows of X, may be
 * NULL), C = concatenation of the m [h][sub_i] seed sub-vectors (may be NULL).  Bit-reproducible for a given
 * `seed` (the library's splitmix64 stream; Julia's RNG draws differ).  tuning TRAIN_KMPP=0 makes the training
 * entry points sample h rows uniformly instead. */
int rq_kmpp_seeds(int64_t *seeds, float *C, const float *X, int64_t n, int d, int m, int h, uint64_t seed);
int rq_train_opq(float *C, int16_t *B1, float *R, float *obj, const float *X, int64_t n, int d, int m,
                 int h, int niter, int init, uint64_t seed, const float *R0, const float *C0);
/* ---- training with more than 256 codewords per codebook: 16-bit codes.  train_pq (src/PQ.jl:68-99),
 * train_opq (src/OPQ.jl:49-139) and train_rvq (src/RVQ.jl:86-127) return Matrix{Int16} codes so that a codebook may hold more than
 * 256 entries; rq_train_pq / rq_train_opq / rq_train_rvq keep refusing h > 256 (their loops run on bytes), these accept
 * 1 <= h <= RQ_MAX_H16.  The SAME loops, instantiated for 16-bit codes: the assignment step is the wide encode (section 4.17), the
 * centres come from rq_dev_update_centers_wide's kernel, emptied centres are re-drawn by Clustering.repick_unused_centers' rule
 * with the costs computed in double on the device (only the n costs come to the host per draw), train_opq reconstructs into an
 * n x d temporary for X'CB and the objective.  The random stream is that of the byte entry points at any h: salts 1 / 2 / 3, the
 * same order of draws.  h <= 256 runs the byte loops and widens: C, R, obj, error and the codes are the bits of rq_train_pq /
 * rq_train_opq / rq_train_rvq for the same arguments.  Layouts are those of the byte entry points; B [n][m] int16 + code_base,
 * code_base 0 (zero-based) or 1 (Julia's one-based Matrix{Int16}), as in the wide encodes.  rq_train_profile describes the last
 * wide call with the same slots.  A NULL C, B, X (or R), a bad code_base, d < m, n < h or niter < 0: RQ_EINVAL; h outside
 * [1, RQ_MAX_H16] or m out of range (PQ / OPQ: 1..32, RVQ: 1..64): RQ_EUNSUPPORTED; on any error no output byte is written.
 * Non-finite rows: the contract of "Non-finite inputs of training" above (point b) holds at every h -- status 0 or a negative
 * code with a message, codes in range, the same bits twice, no device state left behind; centres, R and objective unspecified
 * (tests/test_gpu_nonfinite_train.py, tests/test_nonfinite_train_ref.py). */
int rq_train_pq_wide(float *C, int16_t *B, double *error, const float *X, int64_t n, int d, int m, int h, int niter,
                     uint64_t seed, int code_base);
int rq_train_opq_wide(float *C, int16_t *B, float *R, float *obj, const float *X, int64_t n, int d, int m, int h, int niter,
                      int init, uint64_t seed, const float *R0, const float *C0, int code_base);
int rq_train_rvq_wide(float *C, int16_t *B, double *error, const float *X, int64_t n, int d, int m, int h, int niter,
                      uint64_t seed, int code_base);
/* The two reductions of those loops that read codes, on device pointers, everything on `stream` (kernels, scratch, the reduction
 * of the partial sums): codes [n][m] int16 ZERO-based, read zero-extended; 1 <= h <= RQ_MAX_H16, 1 <= m <= 32, any d >= m, uneven
 * splits (src/utils.jl:179-203), any n.
 *   update_centers  (Clustering.update_centers! as called at src/OPQ.jl:121) C the m [h][sub_i] blocks, counts [m][h]: for each
 *                   (sub-quantizer q, code k, dimension s) the f32 sum of X[row][off_q + s] over the rows with codes[row][q] == k
 *                   in a FIXED order (one-hot products on the matrix cores, row slices combined in a fixed tree; no float
 *                   atomics): two calls on the same input give the same bits.  C = sum * (1.0f / (float)count) for count > 0; a
 *                   code without rows keeps its bits; counts are exact.  On integer-valued X (coordinates in [0, 255]) with fewer
 *                   than 65 793 rows per code every partial sum is an exact integer below 2^24 and the result is
 *                   float32(sum) * (1.0f / float32(count)) bit for bit.  A row whose code lies outside [0, h) (negative ones
 *                   included) is IGNORED in that sub-space: not summed, not counted, never used as an index.  Non-finite X:
 *                   a non-finite coordinate (row r, column c) leaves counts and every column != c exactly as they are with
 *                   column c zeroed; column c is unspecified (0 x NaN reaches every code of it).
 *   reconstruct     (src/OPQ.jl:101,128) CB[j][off_i + s] = C_i[codes[j][i]][s], a pure copy.  A code outside [0, h) is not
 *                   read from C: that sub-space of row j is written as ZEROS.
 * n <= 0: RQ_OK.  A NULL pointer or d < m: RQ_EINVAL; h or m out of range, or a shape whose partial sums do not fit 2 GiB of
 * scratch: RQ_EUNSUPPORTED. */
int rq_dev_update_centers_wide(float *C, uint32_t *counts, const float *X, const int16_t *codes, int64_t n, int d, int m, int h,
                               void *stream);
int rq_dev_reconstruct_wide(float *CB, const int16_t *codes, const float *C, int64_t n, int d, int m, int h, void *stream);
/* Phase clock of the calling thread's last rq_train_pq / rq_train_opq call, milliseconds (measurement aid, bench.py
 * --workload train_opq|train_pq): out[0] X upload, [1] initialisation, [2] qerror, [3] gram X'CB, [4] d x d polar factor
 * incl. its two small copies, [5] rotation, [6] update_centers, [7] encode, [8] reconstruct, [9] convergence check,
 * [10] results D2H, [11] wall time of the iteration loop, [12] iterations run, [13] Jacobi sweeps, [14] Newton-Schulz steps,
 * [15] polar factors taken on the host.  [2]-[9] need tuning TRAIN_PROFILE = 1 (every phase is then bracketed by device
 * synchronisations). */
int rq_train_profile(double *out, int cap);
/* The rotation update of src/OPQ.jl:112-113 (U, S, VV = svd(X * CB'); R = U * VV') as a device call: G [d][d] row-major f32 on
 * the device, Rimg[i * d + k] = R[k][i] (the memory image of Julia's column-major R).  method 0 = scaled Newton-Schulz
 * iteration in double (d <= 1024; what rq_train_opq uses), 1 = one-sided Jacobi SVD (even d <= 128).  status (host, 2 ints):
 * [0] = 0 when Rimg was written, 1 when the method gave up (rank-deficient G); [1] = steps or sweeps.  Synchronous. */
int rq_dev_polar_factor(float *Rimg, const float *G, int d, int method, int *status);

/* ---- device-resident index handle: codes uploaded once, searched many times -- on one device, or
 * row-sharded over the GPUs of a node from ONE host process (what a Julia session is).
 * Replaces, for a resident base, the per-call marshalling of src/Linscan.jl:5-26; the reference has no
 * multi-device path (its only long-axis device is the 1e7-row chunking of deps/src/linscan_aqd.cpp:52-53).
 *   rq_index_create          one shard on the calling thread's current device
 *   rq_index_create_sharded  one shard per entry of devices[0..ndev); a device listed twice holds two
 *                            LOGICAL shards.  Every device scans its rows for all queries on its own
 *                            stream; the per-shard top-k key lists are gathered to devices[0] over xGMI
 *                            (RCCL send/recv on a single-process ncclCommInitAll clique, or
 *                            hipMemcpyPeerAsync when tuning EXCHANGE_PEER=1 / librccl is absent) and merged
 *                            there.  (dist, id) keys are totally ordered and ids are global, so the result
 *                            is bit-identical to one scan of the whole base.  Lists of 128 MB or more per device
 *                            (k x nq x 8 B) travel in up to 4 query chunks -- scan of chunk c+1 | copy of chunk c |
 *                            merge of chunk c-1 on three streams; tuning IDX_QCHUNKS forces the chunk count.
 *   rq_index_set_codes       rows are split into contiguous shards whose sizes differ by at most one;
 *                            ids returned by searches are id_offset + row (+ id_base)
 *   rq_index_set_codes_synth SIFT1B-shape synthetic base generated on the devices:
 *                            code[i][j] = splitmix64(seed ^ (i*m+j)) >> 56
 *   rq_index_search[_opq]    linscan_pq / linscan_opq (src/Linscan.jl:5-26, 93-103) against the resident base;
 *                            host pointers, synchronous, 1 <= k <= n (k > RQ_MAX_K: bulk path, merged across shards by
 *                            the bulk select, queries in chunks whose lists take at most 256 MiB per buffer)
 *   rq_index_info            out[0] shards, [1] distinct devices, [2] exchange (0 none, 1 peer copies, 2 RCCL),
 *                            [3] rows, [4..] rows per shard (as many as fit in cap)
 * The host-pointer calls rq_linscan_pq / rq_linscan_opq / linscan_aqd_query build such an index for the
 * call when the environment variable RAYUELA_HIP_DEVICES lists more than one device ("0,1,2,3" or "all"), so the
 * stock Julia signatures use every GPU without a code change.  That index (RCCL communicator, streams, per-device
 * buffers) is kept for the next call with the same device list, m and d -- only codebooks and code shards are
 * uploaded again -- until rq_release_workspaces(). */
typedef struct rq_index rq_index;
rq_index *rq_index_create(int m, int d, const float *centers_host);
rq_index *rq_index_create_sharded(int m, int d, const float *centers_host, const int *devices, int ndev);
int rq_index_set_codes(rq_index *ix, const uint8_t *codes_host, int64_t n, uint32_t id_offset);
int rq_index_set_codes_synth(rq_index *ix, int64_t n, uint64_t seed, uint32_t id_offset);
int rq_index_search(rq_index *ix, float *dists, uint32_t *ids, const float *queries_host,
                    int64_t nq, int k, int id_base);
int rq_index_search_opq(rq_index *ix, float *dists, uint32_t *ids, const float *queries_host,
                        const float *R_host, int64_t nq, int k, int id_base);
int rq_index_info(rq_index *ix, int64_t *out, int cap);
void rq_index_destroy(rq_index *ix);
/* The index over 16-bit codes: codebooks of 1 <= h <= RQ_MAX_H16 codewords, centers [m][h][d/m], 1 <= m <= 32 (else NULL with
 * rq_last_error set).  The reference has no scan above 256 codewords (deps/src/linscan_aqd.cpp:58,67 hard-wire 256 entries
 * per table); a search is its arithmetic (:66-97) with h entries per table, as rq_linscan_pq_wide states it.
 *   rq_index_create[_sharded]_wide  as rq_index_create[_sharded]; the handle is searched, inspected and destroyed through
 *                                   rq_index_search[_opq], rq_index_info and rq_index_destroy, every shard by the scan of
 *                                   rq_dev_linscan_wide (row slices above the scratch budget, see rq_scan_wide_slices), lists
 *                                   exchanged and merged exactly as for a byte index: the answer is bit for bit that of one
 *                                   rq_dev_linscan_wide over the whole base.  Rows stay in arrival order.
 *   rq_index_set_codes_wide         codes [n][m] int16, code_base 0 or 1 (subtracted on the device).  Every shard is uploaded
 *                                   and checked on the device before the loaded base is replaced: a code outside [0, h) after
 *                                   code_base is RQ_EINVAL naming the first such row, and the index keeps the base it had.
 * rq_index_set_codes_wide on a byte index, rq_index_set_codes[_synth] on a wide one: RQ_EINVAL. */
rq_index *rq_index_create_wide(int m, int h, int d, const float *centers_host);
rq_index *rq_index_create_sharded_wide(int m, int h, int d, const float *centers_host, const int *devices, int ndev);
int rq_index_set_codes_wide(rq_index *ix, const int16_t *codes_host, int64_t n, int code_base, uint32_t id_offset);
/* The additive-quantizer (AQ) kind of the same handle: linscan_lsq / linscan_cq (src/Linscan.jl:118-193) against a resident,
 * row-sharded base, in both code widths.  Searched, inspected and destroyed through rq_index_search[_opq]
 * (linscan_lsq rotates the queries by R first, src/Linscan.jl:126), rq_index_info and rq_index_destroy; lists are exchanged and
 * merged exactly as for a PQ index.  For any shard count the answer is bit for bit that of ONE call over the whole base:
 * rq_linscan_lsq / rq_linscan_cq (byte), rq_linscan_lsq_wide / rq_linscan_cq_wide / rq_linscan_lsq_cbnorms_wide (wide), their
 * rules for NaN norms and non-finite queries and codebooks included.
 *   rq_index_create_aq[_wide]     codebooks [m * h][d] = hcat(C...) as rq_linscan_lsq[_wide] take them (byte: h = 256); lut_mode 1 =
 *                                 LSQ (T = -2<q, c>, plus the row norm), 2 = CQ (T = |q - c|^2), the values of rq_dev_linscan_aq.
 *                                 1 <= m <= 64 (byte) or 32 (wide), 1 <= h <= RQ_MAX_H16, any d >= 1.  devices == NULL with
 *                                 ndev == 0: one shard on the calling thread's current device; else one shard per entry, a
 *                                 repeated device holding several logical shards.  NULL (rq_last_error set) on a bad argument.
 *   rq_index_set_codes_aq[_wide]  replaces the base and its norms (n may differ between calls).  LSQ takes exactly one of dbnorms
 *                                 [n] and cbnorms [hn] (hn <= 256 byte, <= RQ_MAX_H16 wide; wide needs h >= 2): with cbnorms every
 *                                 shard computes dbnorms = cbnorms[quantize_norms(|sum_k C_k[b_k]|^2)] on its own device from its
 *                                 own rows (the arithmetic of rq_lsq_prepare_cbnorms / rq_linscan_lsq_cbnorms_wide).  CQ takes
 *                                 neither.  Anything else is RQ_EINVAL before any work, and the loaded base keeps answering.
 *                                 Byte shards are prepared as rq_lsq_prepare prepares its base: rows padded to a tiled width,
 *                                 bank-aware row order once (tuning INDEX_ORDER), norms by position, the LSQ pre-filter's norm
 *                                 buffer built once; the previous base is freed first.  Wide shards follow
 *                                 rq_index_set_codes_wide: uploaded and checked before the loaded base is replaced, the first bad
 *                                 row named, the base it had (and its norms) kept.  id_offset + n <= 2^32 - 1, a shard < 2^31 rows.
 *   rq_index_aq_info              out[0] lut_mode (0: a PQ index), [1] wide, [2] h, [3] shards, then two slots per shard (as many
 *                                 shards as fit in cap): in bank-aware order, holds a prepared norm buffer.
 * rq_index_set_codes[_wide|_synth] on an AQ index, the AQ setters on a PQ index or one of the other width: RQ_EINVAL naming the
 * entry to call. */
rq_index *rq_index_create_aq(int m, int d, const float *codebooks_host, int lut_mode, const int *devices, int ndev);
rq_index *rq_index_create_aq_wide(int m, int h, int d, const float *codebooks_host, int lut_mode, const int *devices, int ndev);
int rq_index_set_codes_aq(rq_index *ix, const uint8_t *codes_host, const float *dbnorms_host, const float *cbnorms_host,
                          int hn, int64_t n, uint32_t id_offset);
int rq_index_set_codes_aq_wide(rq_index *ix, const int16_t *codes_host, const float *dbnorms_host, const float *cbnorms_host,
                               int hn, int64_t n, int code_base, uint32_t id_offset);
int rq_index_aq_info(rq_index *ix, int64_t *out, int cap);

/* IVFADC (Jegou, Douze, Schmid, PAMI 2011): a coarse quantizer in front of the ADC scan, so that a search reads nprobe lists
 * instead of the whole base.  One device (the calling thread's current one at creation), byte codes with
 * h = 256 tables as rq_linscan_pq, host pointers, synchronous.  The reference has no inverted file; every value is arithmetic this
 * header already pins:
 *   coarse value   v(x, j) = max(fl(fl(sa_j + sb) - 2 g_j), 0) for coarse centroid j, the encode's distance (k-ordered fmaf chains)
 *   list(x)        the first-index argmin of v(x, .): rq_encode_pq_wide with m = 1 and h = nlist (a NaN value counts as 0 there)
 *   probes         the nprobe smallest (v(q, j), j): ties to the lower list, a NaN value behind every number
 *   distance       to a row of probed list p: the table and sum of rq_linscan_pq (deps/src/linscan_aqd.cpp:66-74, 85-87) for the
 *                  query q' = q - Q[p] (one f32 subtraction per element) when by_residual, else q; a NaN distance is no neighbour
 *   answer         the k smallest (dist, id) over the probed lists, ascending; behind them (NaN, 0xFFFFFFFF + id_base)
 * With by_residual = 0 and nprobe = nlist the answer is bit for bit rq_linscan_pq's over the same codes, for any lists.
 *   rq_ivf_create     coarse [nlist][d], centers [m][256][d / m]; d % m == 0, 1 <= m <= 64, 1 <= nlist <= RQ_MAX_H16, by_residual
 *                     0 or 1; NULL (rq_last_error set) otherwise
 *   rq_ivf_build      X [n][d]: assigns, takes residuals (by_residual: x - Q[list(x)], RVQ's stage epilogue), encodes
 *                     (rq_encode_pq; m <= 32) and groups on the device, X in row chunks (tuning IVF_BUILD_ROWS).  Rows are grouped
 *                     by list, inside a list in ascending id; the id of row i is i + id_offset; n + id_offset <= 2^32 - 1.  The
 *                     loaded base is replaced only when the call has succeeded
 *   rq_ivf_set_codes  the same from precomputed lists [n] (each < nlist, else RQ_EINVAL before anything is replaced) and codes
 *                     [n][m] zero-based
 *   rq_ivf_build_bytes  rq_ivf_build on uint8 rows (bvecs).  A byte row MEANS the row widened to float (exact), then everything
 *                     as for float rows: lists, residuals and codes are bit for bit those of the widened matrix.  The bytes
 *                     travel as bytes: lists from rq_encode_pq_wide's byte form, x - Q[list] written as float straight from the
 *                     bytes (by_residual) or the codes from rq_encode_pq_bytes (no float copy of the chunk exists).  X_host at
 *                     any byte alignment, any d; no shape takes another route here (the byte encode's own routing by sub-space
 *                     width applies inside it)
 *   rq_ivf_add, rq_ivf_add_bytes, rq_ivf_add_codes   rq_ivf_build / _build_bytes / _set_codes for a batch that goes BEHIND the
 *                     loaded base instead of replacing it.  After any sequence of one build (or set_codes) and any number of adds,
 *                     the loaded base is the one that a single rq_ivf_build / rq_ivf_set_codes over the concatenated rows would
 *                     load, provided that call gives row i of a piece the id i + id_offset of that piece: the same offsets, the
 *                     same row_ids and the same code bytes in rq_ivf_get_lists, so every search answers with the same bits.
 *                       ids      an add takes its own id_offset, at least the NEXT ID: the largest id loaded plus one (0 for an
 *                                index with no base).  Gaps are allowed (shards of a file carry their file positions); a smaller
 *                                id_offset is RQ_EINVAL and the message names both numbers.  So ids still ascend inside a list,
 *                                which the search contract rests on; added rows go behind the loaded rows of their list
 *                       limits   rows loaded + n <= 2^32 - 1 (offsets are uint32) and id_offset + n <= 2^32 - 1; m <= 32 for the
 *                                row forms, m <= 64 for rq_ivf_add_codes; each refused before any work
 *                       empty    an add on a handle with no base is a build (any id_offset)
 *                       failure  the loaded base is replaced only when the call has succeeded: after a refused argument, a
 *                                failed allocation or a list id >= nlist (RQ_EINVAL naming the row) the old base answers
 *                       cost     one add rewrites the base once (4 + mp bytes per loaded row read and written, mp the tiled row
 *                                width) into fresh allocations; temporaries are sized by the batch.  A search from another
 *                                thread sees the base before or after an add, never a mixture
 *   rq_ivf_search     1 <= nprobe <= nlist, 1 <= k (any k: a short union is padded), id_base 0 or 1; dists / ids [nq][k].  A query
 *                     whose keys (the nprobe largest lists, or k) do not fit the bulk scratch budget: RQ_EUNSUPPORTED.  No base
 *                     loaded: RQ_EINVAL.  Tuning IVF_SEGMENT_ROWS (4096): the longest run of one list a workgroup scans;
 *                     IVF_BATCH_QUERIES: a cap on the query batch; no answer depends on either
 *   rq_ivf_get_lists  offsets [nlist + 1], row_ids [n] (id_offset included) and codes [n][m] in grouped order; NULL skips one
 *   rq_ivf_info       out[0] rows, [1] nlist, [2] m, [3] d, [4] by_residual, [5] the largest list, [6] empty lists; of the last
 *                     search: [7] keys per query (ld), [8] queries per batch, [9] work items, [10] rows scanned; [11] the next id
 *                     (0 with no base)
 *   rq_ivf_last_timing  milliseconds (hipEvents) of the last search: [0] probe selection, [1] item list (with its read-back),
 *                     [2] keys kernel, [3] select chain; of the last successful build / set_codes / add: [4] uploads, assignment
 *                     and encode, [5] grouping (sorts, bounds, offsets), [6] the carry of the loaded rows, [7] placement */
typedef struct rq_ivf rq_ivf;
rq_ivf *rq_ivf_create(int d, int nlist, const float *coarse_host, int m, const float *centers_host, int by_residual);
int rq_ivf_build(rq_ivf *ix, const float *X_host, int64_t n, uint32_t id_offset);
int rq_ivf_set_codes(rq_ivf *ix, const uint32_t *lists_host, const uint8_t *codes_host, int64_t n, uint32_t id_offset);
int rq_ivf_build_bytes(rq_ivf *ix, const uint8_t *X_host, int64_t n, uint32_t id_offset);
int rq_ivf_add(rq_ivf *ix, const float *X_host, int64_t n, uint32_t id_offset);
int rq_ivf_add_bytes(rq_ivf *ix, const uint8_t *X_host, int64_t n, uint32_t id_offset);
int rq_ivf_add_codes(rq_ivf *ix, const uint32_t *lists_host, const uint8_t *codes_host, int64_t n, uint32_t id_offset);
int rq_ivf_search(rq_ivf *ix, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, int nprobe, int k, int id_base);
/* the search with kc candidates per query, re-ranked by the exact distance to the rows of ds ("exact re-ranking" above) */
int rq_ivf_search_refine(rq_ivf *ix, rq_dataset *ds, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, int nprobe,
                         int k, int kc, uint32_t id_offset, int id_base);
int rq_ivf_get_lists(rq_ivf *ix, int64_t *offsets, uint32_t *row_ids, uint8_t *codes);
int rq_ivf_info(rq_ivf *ix, int64_t *out, int cap);
int rq_ivf_last_timing(rq_ivf *ix, double *ms, int cap);
void rq_ivf_destroy(rq_ivf *ix);

/* Threading: every entry point may be called from any host thread.  Library scratch is keyed by
 * (device, stream) and the launch sequences of one device are serialised internally, so concurrent
 * calls on different streams or devices do not interfere; at most 8 distinct streams per device may
 * use the rq_dev_* calls before rq_release_workspaces() (which frees the current device's scratch and the
 * pool of staging buffers the host-pointer calls keep between calls: at most HOST_CACHE_MB = 2048 MB per device,
 * buffers of up to HOST_CACHE_MAX_MB = 256 MB each; HOST_CACHE_MB=0 restores hipMalloc / hipFree per call). */
int rq_release_workspaces(void);

/* Page-locked result buffers for the language shims.  linscan_* return 8 * k * nq bytes; into a freshly allocated
 * pageable array (src/Linscan.jl:16-17 `zeros(Cfloat, k, nq)`, numpy `empty`) the copies back run at the speed of
 * first-touch page faults (18 GB/s on the bench box: 4.4 ms for the 80 MB of the SIFT1M-shape answer, more than the
 * scan).  A shim can instead take its result arrays from rq_host_alloc (hipHostMalloc'ed, pooled), wrap them without
 * copying (Julia `unsafe_wrap` + finalizer, numpy `__array_interface__`) and return them with rq_host_free when the
 * array is collected.  NULL = over the limit (HOST_PIN_MAX_MB = 4096 outstanding) or no device: use an ordinary array.
 * The entry points accept either kind of memory; nothing else changes.  rq_release_workspaces also drops idle buffers. */
void *rq_host_alloc(size_t bytes);
void rq_host_free(void *p);

/* Diagnostic knob used by tests and tuning runs (same effect as env RQ_<KEY>):
 *   SCAN_SLICES  force the number of row slices per shard (0 = automatic)
 *   ENC_WAVES    wavefronts per encode workgroup (8 or 16)
 *   SCAN_FILTER / SCAN_FILTER_LSQ  0 switches the integer pre-filter of the PQ/CQ / LSQ scans off (same results)
 *   SCAN_BUCKET_FINISH / SCAN_SS_MAP  0 switches the bucket finish of K <= 1024 / the map buckets of K > 1024 off (same results)
 *   others (SCAN_SAMPLE, SCAN_SRANK_MUL, SCAN_SLACK, SCAN_SS_MIN_K, SCAN_TAIL_SLICES, SCAN_MIN_ROWS, ENC_DIRECT,
 *   ROT_V2, HOST_OVERLAP, SCAN_STATS) are experiment switches documented where they are read */
int rq_set_tuning(const char *key, int value);
/* Drops the value rq_set_tuning stored for `key` (NULL: for every key): the knob reads env RQ_<KEY> again, else its code default.
 * Storing the default is NOT the same -- it hides the environment, and a few knobs tell "unset" from any stored value. */
int rq_reset_tuning(const char *key);
/* Diagnostics (pure host code): 1 if a raw-pointer PQ scan of n rows (m = 8 wide), nq queries and k neighbours puts a scratch copy
 * of the base into bank-aware row order inside the call (csrc/rq_order.hip: from ORDER_MIN_NQ queries on, below ORDER_MAX_K
 * neighbours, ORDER_MIN_ROWS rows up) -- 2 if that order is also BALANCED (the greedy pass of rq_order.hip, from ORDER_GREEDY_MIN_NQ
 * = 16384 queries on: it costs more than the sort and gains 4-8 % of the scan; bases ordered once always get it) --, 0 if it scans
 * the rows as they arrive.  bench.py times the scan kernel alone on the kind of base the timed call really scans (VERDICT r5 weak
 * #3: at k = 10000 the call scans the arrival order). */
int rq_scan_orders_in_call(int64_t n, int64_t nq, int k);

/* Diagnostics: with tuning SCAN_STATS=1, summed shader-clock cycles (thread 0 of every workgroup) of the
 * last scan: [0] LUT build [1] threshold sample [2] streaming [3] in-stream cuts [4] final cut [5] sort+write,
 * [6] number of in-stream cuts, [7] number of exact fallbacks, [8] the row part of [1], [9..11] sort load / stages /
 * write-out (bucket finish: range + histogram / scan + scatter / rank + write; large K: sample sort or range / bucket search
 * or histogram / scan + scatter), [12] work items, [13] items that kept the integer pre-filter to their end, [14] rows the pre-filter let
 * through in the items' first blocks, [15] rows of those blocks; out has 16 slots. */
int rq_scan_stats(unsigned long long *out16);
/* ... and the finish of that launch (K <= 1024, distance-bucket finish): [0] work items that reached the bucket finish, [1] items
 * the tie look (bf_tie_twins) sent to select + sort before any bucket work, [2] items that took select + sort in the end
 * ([2] - [1] gave up after their histogram); [3..7] reserved (0).  Counts, not clocks: what tests assert on. */
int rq_scan_finish_stats(unsigned long long *out8);
/* Diagnostics: the kept in-call row order (csrc/rq_order.hip) of the current device, summed over its streams, since the last
 * rq_release_workspaces.  A raw-pointer scan that orders a scratch copy of its base keeps that copy and proves on every call, on
 * the device, that it still is the order of the codes it was handed.  [0] calls that consulted the kept copy, [1] hits (the copy
 * was reused as it was), [2] builds of a plain (sorted) copy, [3] builds of a balanced copy, [4] calls that ordered uncached (the
 * snapshot did not fit under ORDER_MAX_SCRATCH_MB), [5] of [3]: upgrades of a plain copy on its first hit, [6..7] reserved (0).
 * [0] = [1] + [2] + [3].  Waits for the device.  Counts, not clocks: what tests assert on. */
int rq_order_cache_stats(unsigned long long *out8);

/* Diagnostics (pure host code, no device needed): the scan planner's decision for a shard of n rows, nq queries,
 * m sub-quantizers, dimension d, k neighbours on a device with num_cu compute units.  out[0] queries per group,
 * [1] groups, [2] groups scanned as whole-base items, [3] row slices of the remaining groups, [4] rows per slice,
 * [5] workgroups launched, [6] candidate capacity per query, [7] bit 0: sample-sort finish (k > 1024), bit 1: big base --
 * row windows handed out per XCD (L2 affinity), bit 2: k > RQ_MAX_K takes the bulk path -- then [2] = [1], [3] = 1, [4] = n,
 * [5] is the distance kernel's grid and [6] the queries per bulk batch (0: one query does not fit the scratch budget). */
int rq_scan_plan(int64_t n, int64_t nq, int m, int d, int k, int num_cu, int64_t *out8);

/* Milliseconds spent in the last host-pointer call on this thread: total wall, H2D, kernels
 * (hipEvent), D2H -- so the PCIe-inclusive and the resident rates can both be reported. */
int rq_last_timing(double *total_ms, double *h2d_ms, double *kernel_ms, double *d2h_ms);

/* ---- test hooks: not for callers --------------------------------------------------------------------------------------------
 * No result of this library depends on what its scratch holds when a call begins; tests/test_gpu_scratch.py pins that with
 * these two.  Both act on the current device as a whole and wait for it, like rq_release_workspaces.
 *
 * rq_test_fill_scratch sets every byte (allocation slack included) of every scratch buffer of every stream, of every idle staging
 * buffer of the host-pointer calls and of every idle page-locked block (rq_host_alloc) to `value` (0..255).  The kept in-call row
 * order starts over as after a fresh allocation (its buffers are filled too), and with it the statistics of
 * rq_order_cache_stats: they read as after rq_release_workspaces.  out7: [0] bytes filled in stream scratch, [1] in
 * idle staging buffers, [2] in idle page-locked blocks, [3] scratch buffers filled, [4] the number of scratch allocations the
 * library has made so far (it moves when a call had to grow a buffer, that is, when it ran on fresh memory instead), [5] idle
 * staging buffers, [6] idle page-locked blocks (either count or its bytes move when a host-pointer call had to take a fresh
 * buffer instead of a filled one).
 *
 * rq_test_scratch_report: for the scratch of stream `of_stream` (NULL: the null stream), per buffer s < 20 (the order of the
 * WS_* enum of csrc/rq_internal.h): bytes[s] allocated (0: none), differs[s] = 1 if any byte is not the value of the last
 * fill.  cap: entries of bytes / differs, at least 20. */
int rq_test_fill_scratch(int value, unsigned long long *out7);
int rq_test_scratch_report(void *of_stream, int64_t *bytes, int *differs, int cap);
/* Host-only, no device: what the segment sum of rq_dev_update_centers[_wide] (cstride == 0) or of the ERVQ codebook increment
 * (cstride > 0: the code stride, one sub-quantizer of width d, m ignored) would launch for n rows on a device of num_cu compute
 * units; code_bytes 1 (uint8 codes) or 2 (int16).  The launchers ask the same planner (csrc/rq_train.hip), and the number of row
 * slices fixes the order of the float reduction, so tests/test_centers_plan.py pins it.  out (cap >= 8 words): [0] the return
 * code the launcher would give (the rest is 0 unless it is RQ_OK), [1] 1: the matrix-core kernel, 2: the owner-thread kernel
 * (then [3..6] are 0), [2] row slices, [3] (sub-quantizer, 16-dimension block) units per block of 256 codes, [4] code blocks,
 * [5] of them launched together with 16 tiles, [6] the tile count (4, 8 or 16) of the ragged last block, 0 if there is none,
 * [7] bytes asked of the WS_TMP scratch slot. */
int rq_centers_plan(int64_t n, int d, int m, int h, int num_cu, int code_bytes, int cstride, int64_t *out, int cap);
/* KNN_CHUNK_ROWS of the ground-truth entries (rq_knn*): rows > 0 makes every later call of this process split the base into
 * chunks of `rows` rows (rq_knn_plan reports it, out[5] = 1), so that a test can run the fold of per-chunk lists on a small base;
 * rows <= 0 gives the planner its choice back.  No answer depends on it (tests/test_gpu_knn.py).  Returns the previous value. */
int64_t rq_test_knn_chunk_rows(int64_t rows);
/* The same for the scans over 16-bit codes: rows > 0 makes every later rq_dev_linscan_wide / rq_dev_linscan_aq_wide of this
 * process (and the host and index entries built on them) cut the base into slices of `rows` rows (rq_scan_wide_slices reports
 * it, out[4] = 1), so that a test can run the fold of per-slice lists on a small base; rows <= 0 gives the planner its choice
 * back.  No answer depends on it (tests/test_gpu_scan_wide_slices.py).  Returns the previous value. */
int64_t rq_test_scan_wide_slice_rows(int64_t rows);
/* The re-ranking entries: lds_kc > 0 makes every later call of this process sort at most lds_kc (<= 4096) candidates per query in
 * LDS and send longer lists through the select chain; batch_queries > 0 caps the queries per batch of rq_dataset_rerank
 * (rq_rerank_plan reports both, out[4] = 1 for the batch).  Values <= 0 give the planner its choice back.  No answer depends on
 * either (tests/test_gpu_rerank.py).  Returns the previous pair as lds_kc * 2^32 + batch_queries. */
int64_t rq_test_rerank_limits(int64_t lds_kc, int64_t batch_queries);

#ifdef __cplusplus
}
#endif
#endif /* RAYUELA_HIP_H_ */
