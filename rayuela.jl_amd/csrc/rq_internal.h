// rq_internal.h -- shared host-side declarations of librayuela_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <math.h>

#include <algorithm>
#include <chrono>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rayuela_hip.h"

namespace rq {

// Records the message for rq_last_error() (thread-local) and returns `code`.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_hip(hipError_t e, const char *what, const char *file, int line);
// The only failure an OPTIONAL step (the bank-aware ordering of a base) may swallow: no memory for its scratch.  fail_hip returns
// the HIP code, so rc == hipErrorOutOfMemory identifies it; forgive_oom() then withdraws the message (the step is skipped, the
// call succeeds).  Launch / synchronisation errors are never forgiven: a device fault must surface where it happened.
inline bool is_oom(int rc) { return rc == (int)hipErrorOutOfMemory; }
void forgive_oom();

#define RQ_HIP(expr)                                                       \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) return ::rq::fail_hip(_e, #expr, __FILE__, __LINE__); \
  } while (0)

#define RQ_TRY(expr)            \
  do {                          \
    int _r = (expr);            \
    if (_r != RQ_OK) return _r; \
  } while (0)

// Host tools that other translation units share but the library does not export: the dynamic symbol table holds the C ABI
// and what it held before them.
#define RQ_LOCAL __attribute__((visibility("hidden")))

// launch a kernel and return the launch error, if any
#define RQ_LAUNCH(...)                \
  do {                                \
    hipLaunchKernelGGL(__VA_ARGS__);  \
    RQ_HIP(hipGetLastError());        \
  } while (0)

// the same for a kernel that needs dynamic LDS: the limit is set on every launch (it is per device and may have been set
// for another LDS size by the previous call)
#define RQ_LAUNCH_LDS(kern, grid, block, lds, stream, ...)                                               \
  do {                                                                                                    \
    RQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                               (int)(lds)));                                                              \
    RQ_LAUNCH(kern, grid, block, lds, stream, __VA_ARGS__);                                               \
  } while (0)

int tuning(const char *key, int dflt);  // env RQ_<KEY> or rq_set_tuning override

// splitarray offsets (src/utils.jl:179-203): sub-space i of m spans dimensions [off[i], off[i + 1]) of d, the first d % m
// one wider than the rest.  Fills off[0..m]; returns the widest sub-space.
inline int split_offsets(int *off, int d, int m) {
  const int per = d / m, extra = d % m;
  int pos = 0;
  for (int i = 0; i < m; ++i) { off[i] = pos; pos += per + (i < extra ? 1 : 0); }
  off[m] = pos;
  return per + (extra ? 1 : 0);
}

struct DeviceInfo {
  int device;
  int num_cu;
  char arch[64];
};
int device_info(DeviceInfo *out);

// Grow-only scratch owned by the library, keyed by (current device, stream): launches on different
// streams never share a buffer.  At most 8 distinct streams per device (release_workspaces() resets).
// A dispatch carries fewer than 2^32 work-items per grid dimension (a 32-bit field of the dispatch packet): a launch of more
// does not fail, it wraps and runs the remainder only.  Launches of one thread or one wavefront per element of an n-sized
// array therefore go in slices of at most LAUNCH_MAX_THREADS work-items (tests/test_gpu_large_offsets.py runs them past it).
constexpr int64_t LAUNCH_MAX_THREADS = 1ll << 31;
// fn(e0, ne) over [0, total) in pieces of at most LAUNCH_MAX_THREADS / per elements (`per` work-items each); stops at the
// first error
template <class F>
inline int for_slices(int64_t total, F fn, int64_t per = 1) {
  const int64_t piece = std::max<int64_t>(1, LAUNCH_MAX_THREADS / per);
  for (int64_t e0 = 0; e0 < total; e0 += piece) RQ_TRY(fn(e0, std::min(piece, total - e0)));
  return RQ_OK;
}
int workspace(int slot, size_t bytes, void **ptr, hipStream_t stream);
int release_workspaces();
int release_stream_workspace(hipStream_t stream);
void *host_pool_alloc(size_t bytes);
void host_pool_free(void *p);
void host_pool_trim();
void sharded_cache_release();
int aux_streams(hipStream_t *compute, hipStream_t *transfer);
// WS_COUNTER, in bytes: [0, 64) work tickets / finished items per XCD, [64, 256) diagnostics (rq_scan_stats; the encode
// filter's two counters at byte 128)
constexpr size_t WS_COUNTER_BYTES = 256;
enum { WS_CAND = 0, WS_COUNTER = 1, WS_KEYS = 2, WS_TMP = 3, WS_PAD = 4, WS_MERGE = 5, WS_NORMB = 6, WS_ORDER = 7, WS_ORDER_TMP = 8, WS_ENCFLAG = 9, WS_BULK = 10, WS_ICM_BIN = 11, WS_ICM_U = 12, WS_LSQ_A = 13, WS_LSQ_B = 14, WS_LSQ_S = 15, WS_CHAIN = 16, WS_ORDER_STATE = 17, WS_H16_SA = 18, WS_H16_CODES = 19, WS_SLOTS = 20 };

// Per-device launch lock (recursive): held while a call looks up scratch, resets the work counter and
// launches, so two host threads cannot interleave those sequences on one device.
class DeviceLock {
 public:
  DeviceLock();
  ~DeviceLock();
  DeviceLock(const DeviceLock &) = delete;
  DeviceLock &operator=(const DeviceLock &) = delete;
 private:
  void *mu_;
};

// The calling thread's current device, restored on every exit path of a call that switches devices.
struct SavedDevice {
  int dev = -1;
  SavedDevice() { if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; } }
  ~SavedDevice() { if (dev >= 0) (void)hipSetDevice(dev); }
  SavedDevice(const SavedDevice &) = delete;
  SavedDevice &operator=(const SavedDevice &) = delete;
};

// Wall clock of the host-pointer calls: milliseconds since it was made.
struct Timer {
  using clock = std::chrono::steady_clock;
  clock::time_point t0 = clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); }
};

// Phase clock of the host-pointer entries (which synchronise anyway): hipEvents between the phases of one call, read at its
// end into the caller's per-phase milliseconds `acc`.  want == false (the device-pointer entries, which may run under stream
// capture) creates and records no event and leaves `acc` alone; so does a clock whose first event cannot be made.
struct RQ_LOCAL PhaseClock {
  bool on = false;
  hipStream_t s;
  double *acc;
  std::vector<std::pair<int, hipEvent_t>> marks;   // (phase ending here, event)
  hipEvent_t first = nullptr;
  PhaseClock(hipStream_t st, double *acc_ms, bool want = true) : s(st), acc(acc_ms) {
    if (want && hipEventCreate(&first) == hipSuccess) on = hipEventRecord(first, s) == hipSuccess;
  }
  PhaseClock(const PhaseClock &) = delete;
  PhaseClock &operator=(const PhaseClock &) = delete;
  // the work queued since the previous mark belongs to `phase`
  void mark(int phase) {
    if (!on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, s);
    marks.push_back({phase, e});
  }
  // accumulate the intervals into acc (interval = previous mark .. this mark)
  void collect() {
    if (!on) return;
    (void)hipStreamSynchronize(s);
    hipEvent_t prev = first;
    for (auto &pe : marks) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, prev, pe.second) == hipSuccess) acc[pe.first] += ms;
      prev = pe.second;
    }
  }
  ~PhaseClock() {
    for (auto &pe : marks) (void)hipEventDestroy(pe.second);
    if (first) (void)hipEventDestroy(first);
  }
};

// Milliseconds reported by rq_last_timing() for the calling thread.
void set_timing(double total_ms, double h2d_ms, double kernel_ms, double d2h_ms);

// ---- ADC scan -------------------------------------------------------------------------------
struct ScanPlan {
  int qg, blk;
  uint32_t ngroups, nslices, rows_per_slice, whole;
  uint32_t cap, trigger, p2, scratch_keys, grid, sample;
  size_t cand_bytes, gtab_off, bkt_off;
  bool lds_ok, bigk, spread;
  bool xcd;        // big base: short row windows handed out per XCD (see plan_for)
};
int scan_plan(ScanPlan &pl, int64_t n, int64_t nq, int m, int d, int K, int num_cu, int force_slices);
enum { LUT_PQ = 0, LUT_LSQ = 1, LUT_CQ = 2 };
// one planned scan of a resident shard: outputs, inputs, shape and scratch (rq_scan_plan.hip)
struct ScanCall {
  float *dists = nullptr;             // whole items: [nq][K] dists / ids, or packed keys [nq][K] when keys != nullptr
  uint32_t *ids = nullptr;
  uint64_t *keys = nullptr;
  uint64_t *part = nullptr;           // sliced items: per-slice key lists for merge_launch
  const uint8_t *codes = nullptr;     // [n][scan_padded_m(m)]
  const float *centers = nullptr, *queries = nullptr;
  int64_t n = 0, nq = 0;
  int m = 0, d = 0, K = 0;
  uint32_t id_offset = 0;
  int id_base = 0;
  uint32_t *work_counter = nullptr;   // WS_COUNTER
  uint64_t *cand = nullptr;           // WS_CAND, pl.cand_bytes
  int lut_mode = LUT_PQ;
  const float *row_bias = nullptr;
  uint8_t *norm_buf = nullptr;        // LSQ pre-filter: lsq_norm_bytes(n), prepared by the call unless norm_ready
  bool norm_ready = false;
  const uint32_t *perm = nullptr;     // ordered base (rq_order.hip)
};
RQ_LOCAL int scan_launch(const ScanPlan &pl, const ScanCall &c, hipStream_t stream);
const char *last_scan_kernel_name();      // which instantiation the calling thread's last scan_launch chose
void set_last_scan_kernel(const char *name);
size_t lsq_norm_bytes(int64_t n);      // LSQ pre-filter: bytes of a base's prepared norm buffer
int lsq_norm_prepare(uint8_t *norm_buf, const uint8_t *codes, const float *centers, const float *row_bias, int64_t n,
                     int mp, int m_real, int d, hipStream_t stream);
// what a caller may know about a resident base beyond its code bytes
struct ScanBase {
  const uint32_t *perm = nullptr;     // rows are in bank-aware order (rq_order.hip): perm[position] = row; implies `padded`
  uint8_t *norm_prepared = nullptr;   // LSQ: the pre-filter's prepared norm buffer (lsq_norm_prepare), else per call
  bool padded = false;                // rows are scan_padded_m(m) bytes wide already
};
// argument checks + planner + launches of one resident shard (rq_dev_linscan's body)
int dev_linscan(float *dists, uint32_t *ids, uint64_t *keys, const uint8_t *codes, const float *centers,
                const float *queries, int64_t n, int64_t nq, int m, int d, int k, uint32_t id_offset,
                int id_base, hipStream_t stream, int lut_mode = LUT_PQ, const float *row_bias = nullptr,
                const ScanBase *base = nullptr);
// One base resident on one device: what survives its preparation.  Every shard of an index handle embeds one (rq_index.hip: PQ and
// AQ, byte and int16 rows) and rq_lsq_prepare holds one.  The arrival-order rows that exist only while an ordered copy is built are
// a local of resident_order, not a member: no pointer here means different allocations on different paths.
struct ResidentBase {
  void *mem = nullptr;              // the ONE rows allocation: the rows as they arrived, or order_base's [ordered rows | perm]
  const void *rowp = nullptr;       // the rows inside mem
  const uint32_t *perm = nullptr;   // inside mem: position -> row when the rows are in bank-aware order (rq_order.hip), else null
  float *norms = nullptr;           // LSQ: [n] row norms -- BY POSITION when perm != nullptr
  uint8_t *normb = nullptr;         // byte LSQ: the pre-filter's prepared norm buffer (lsq_norm_bytes) where the filter applies
  const uint8_t *rows() const { return static_cast<const uint8_t *>(rowp); }
  const int16_t *rows16() const { return static_cast<const int16_t *>(rowp); }   // a wide base: int16 rows, perm null
  void adopt_rows(void *allocation) { mem = allocation; rowp = allocation; perm = nullptr; }   // rows in arrival order
  // the base's device is current and no queued work reads the base
  void free() {
    if (mem) (void)hipFree(mem);
    if (norms) (void)hipFree(norms);
    if (normb) (void)hipFree(normb);
    *this = ResidentBase();
  }
};
// Puts a resident base of [n][mp] byte rows (mp a tiled width) in bank-aware order ONCE, where that pays (INDEX_ORDER /
// order_pays): the rows allocation becomes order_base's, the norms (when the base has any) are gathered through perm, the
// arrival-order rows are freed.  No memory for the ordered copy, the key scratch or the gathered norms leaves the base in arrival
// order -- slower gathers, the same answer -- and the call succeeds (forgive_oom); any other error is returned with the base as it
// was.  The caller holds the DeviceLock and releases the stream's workspace (the key scratch) when it has no further use for it.
int resident_order(ResidentBase *b, int64_t n, int mp, hipStream_t stream);
// One resident base of byte codes of an additive quantizer (h = 256) on the current device, as dev_linscan wants it: rows padded to
// scan_padded_m(m), ordered by resident_order (at every width), the pre-filter's norm buffer prepared once.
// codes [n][m], dbnorms [n] and cbnorms [hn] are HOST arrays, cb [m * 256][d] is on the device.  LSQ (lsq = true) takes dbnorms, or
// (dbnorms null) computes cbnorms[quantize_norms(|sum_k C_k[b_k]|^2)] from the uploaded rows; CQ takes neither.  Launches go to
// `stream`, which is idle when the call returns; on an error *b holds what was allocated so far (b->free()).
int aq_base_prepare(ResidentBase *b, const uint8_t *codes, const float *cb, const float *dbnorms, const float *cbnorms, int hn,
                    int64_t n, int m, int d, bool lsq, hipStream_t stream);
bool order_pays(int64_t n, int64_t nq, int k);                          // SCAN_ORDER / ORDER_MIN_ROWS / ORDER_MIN_NQ / ORDER_MAX_K
size_t order_base_bytes(int64_t n, int mp);
// `batch` of the order planner: the number of queries of the ONE scan the ordering serves (the greedy balance runs only where
// it pays within that call, ORDER_GREEDY_MIN_NQ), or one of
constexpr int64_t ORDER_ONCE = 0;      // a base that is ordered once and scanned many times: always balanced
constexpr int64_t ORDER_PLAIN = -1;    // the plain set: never balanced
RQ_LOCAL int order_base(const uint8_t **out_codes, const uint32_t **out_perm, void *dst, const uint8_t *codes, int64_t n, int mp,
                        int64_t batch, hipStream_t stream);
// ---- bank-aware row order (rq_order.hip) ---------------------------------------------------------
struct OrderTiling { int rpt, gran, group, cbits, blk; };                    // see scan_order_tiling (rq_scan_plan.hip)
void scan_order_tiling(int mp, OrderTiling *t);
RQ_LOCAL bool order_greedy_plan(int64_t n, int mp, int budget, uint32_t out[4], int64_t batch);
RQ_LOCAL bool order_greedy_runs(int64_t n, int mp, const OrderTiling &t, int total, uint32_t gp[4], int64_t batch);  // the launch's balance predicate
RQ_LOCAL int order_key_bits(int64_t n, int mp, const OrderTiling &t, int nb[8], int64_t batch);  // key layout; returns the total bits (0: no ordering)
size_t order_scratch_bytes(int64_t n, int total_bits);
int order_sample_stride();                                               // ORDER_SAMPLE_STRIDE (16; < 2: no sample blocks)
uint32_t order_sample_rows(int64_t n, int blk, uint32_t *sgroups);   // arrival-order sample blocks of an ordered base
int gather_f32_launch(float *dst, const float *src, const uint32_t *perm, int64_t n, hipStream_t stream);
RQ_LOCAL int order_rows_launch(uint8_t *dst, uint32_t *perm, const uint8_t *src, int64_t n, int mp, void *scratch,
                               const OrderTiling &t, int64_t batch, hipStream_t stream);
// The kept order of dev_linscan (rq_order.hip, "the kept order"): the host half of one (device, stream) workspace's cache.  The
// device half -- which key the copy was built for, the verdict of the call's check, the counters -- is WS_ORDER_STATE.
struct OrderCacheHost {
  unsigned char key[768];            // what defines the order (OrderCacheKey); the codes pointer is not part of it
  uint32_t key_id = 0;               // 0: no key yet; the device word must equal it for a hit
  uint32_t epoch = 0;                // number of the call, never 0
  uint64_t order_gen = 0, state_gen = 0;     // allocations of WS_ORDER / WS_ORDER_STATE the cache was set up in
  unsigned long long consulted = 0, uncached = 0;   // rq_order_cache_stats
};
size_t order_cache_state_bytes();
int order_cached_key_bits(int64_t n, int mp, const OrderTiling &t);
// order `src` into dst / perm unless the copy there is proven (on the device, in stream order) to be the order of these bytes
int order_rows_cached(uint8_t *dst, uint32_t *perm, uint8_t *snap, const uint8_t *src, int64_t n, int m, int mp, void *scratch,
                      const OrderTiling &t, int64_t nq, uint32_t *state, OrderCacheHost *h, hipStream_t stream);
int order_cache_stats(unsigned long long *out8);
// [P][nq][k] -> [nq][P][k] (lists gathered shard-major, merged query-major)
int interleave_keys_launch(uint64_t *dst, const uint64_t *src, int64_t nq, int P, int k, size_t pstride, hipStream_t stream);
int scan_padded_m(int m);   // smallest tiled row width >= m (2,4,8,16,32,64) or -1
int pad_codes_launch(uint8_t *dst, const uint8_t *src, int64_t n, int m, int mp, hipStream_t stream);
// ---- bulk top-k (rq_bulk.hip): RQ_MAX_K < k <= n ------------------------------------------------------------------
// Scratch of one bulk call per device and stream (WS_BULK): keys of a query batch + the select / sort buffers.  The batch
// is sized to fit; a query that does not fit alone is an out-of-memory error.
constexpr size_t BULK_SCRATCH_BYTES = (size_t)2 << 30;
// host-pointer calls with k > RQ_MAX_K: device result buffers of at most this many bytes, the queries in chunks
constexpr size_t BULK_HOST_RESULT_BYTES = (size_t)256 << 20;
int bulk_scan(float *dists, uint32_t *ids, uint64_t *keys, const uint8_t *codes, const float *centers, const float *queries,
              int64_t n, int64_t nq, int m, int d, int k, uint32_t id_offset, int id_base, hipStream_t stream, int lut_mode,
              const float *row_bias, const uint32_t *perm, int num_cu);
int bulk_merge(float *dists, uint32_t *ids, uint64_t *keys_out, const uint64_t *keys_in, int64_t nq, int P, int K,
               int id_base, hipStream_t stream);
// rq_scan_plan's view of a bulk call: queries per group, groups, grid of the distance kernel, queries per batch
void bulk_plan(int64_t n, int64_t nq, int m, int k, int num_cu, int64_t *qg, int64_t *groups, int64_t *grid, int64_t *batch);
// The select -> compact -> sort -> unpack chain of rq_bulk.hip (its steps 2-5) on keys that are ready in device memory: shared
// with the scan over 16-bit codes (rq_scan_h16.hip), which writes its own keys and then runs exactly this chain.
constexpr int64_t BK_MAX_NB = 16384;   // queries per batch (grid.y)
struct BulkQ;                          // per-query select / sort state (rq_bulk.hip)
struct BulkSel {
  const uint64_t *src;   // keys of query q: src[q * ld + i], i < cnt
  size_t ld;
  uint32_t cnt, k;
  uint32_t span;         // keys per select / compact block
  uint32_t tiles;        // sort tiles per query: ceil(k / BK_TILE)
  BulkQ *st;             // [nb]
  uint32_t *hist;        // [nb][256]
  uint32_t *th;          // [nb][256][tiles] tile histograms, then scatter offsets
  uint64_t *buf0, *buf1; // [nb][k] sort ping-pong
};
struct BulkOut {
  float *dists;          // [nb][k] (already offset to the batch) or nullptr
  uint32_t *ids;
  uint64_t *keys;
  uint32_t id_base;
};
size_t bulk_usable();                          // the usable part of BULK_SCRATCH_BYTES (workspace() allocates 1.25x the request)
size_t sel_bytes_per_query(uint32_t k);        // scratch of the chain per query, the keys themselves excluded
void sel_layout(BulkSel &s, unsigned char *&at, int64_t nb, uint32_t k);             // lays that scratch out from `at`
void sel_grid(BulkSel &s, uint32_t cnt, int64_t nb, int num_cu, uint32_t *hx);       // blocks per query of select / compact
int sel_run(const BulkSel &s, uint32_t hx, int64_t nb, const BulkOut &o, hipStream_t stream);
int merge_launch(float *dists, uint32_t *ids, uint64_t *keys_out, const uint64_t *keys_in, int64_t nq,
                 int P, int K, int id_base, hipStream_t stream);
// ---- IVFADC (rq_ivf.hip) --------------------------------------------------------------------------------
// The rq_ivf handle shares no entry with other files; it is built from the ones declared here: encode_h16_launch at m = 1 (the
// list of a row), residual_launch (x - Q[list]), encode_launch and pad_codes_launch (the codes), and the chain above (sel_layout /
// sel_grid / sel_run) three times -- as the stable sort that groups rows by list, as the probe selection (k = nprobe over one key
// per list) and as the top-k over the keys of the probed lists.  One item of a search: rows [row0, row0 + nrows) of `list`, scanned
// for batch query q with their keys written from offset koff of the query's row of the key buffer.
struct IvfItem { uint32_t q, list, row0, nrows, koff; };
// ---- ADC scan over 16-bit codes (rq_scan_h16.hip): codes [n][m] int16 zero-based, centers [m][h][d/m] ----
// every argument check of rq_dev_linscan_wide / rq_linscan_*_wide (`who` names the entry point); no device work
// full_dim: the additive-quantizer entries (codebooks [m * h][d], section 4.20) -- any d >= 1 instead of d % m == 0
int linscan_wide_check(const char *who, bool null_arg, int64_t n, int m, int h, int d, int k, uint32_t id_offset, int id_base,
                       bool full_dim = false);
int dev_linscan_wide(float *dists, uint32_t *ids, uint64_t *keys, const int16_t *codes, const float *centers,
                     const float *queries, int64_t n, int64_t nq, int m, int h, int d, int k, uint32_t id_offset, int id_base,
                     hipStream_t stream);
int lut_h16_launch(float *lut, const float *centers, const float *queries, int64_t nq, int m, int h, int sub,
                   hipStream_t stream);                   // plain [nq][m][h]
// host entries: codes -= code_base in place; *first_bad (device) <- the first row with a code outside [0, h), else ~0
int prepare_codes_h16_launch(int16_t *codes, unsigned long long *first_bad, int64_t n, int m, int h, int code_base,
                             hipStream_t stream);
// the int16 code check of every entry that takes such codes from a caller: prepare_codes_h16_launch with `flag` (8 device bytes)
// as its word, the word read back on `stream` before any other work is queued, RQ_EINVAL naming `who`, the first bad row and the
// accepted range [code_base, h - 1 + code_base], `suffix` appended
int check_codes_h16(const char *who, int16_t *codes, unsigned long long *flag, int64_t n, int m, int h, int code_base,
                    hipStream_t stream, const char *suffix = "");
void scan_h16_plan(int m, int h, int out[4]);             // rq_scan_wide_plan
// rq_scan_wide_slices: rows per slice, slices, queries per batch, WS_BULK bytes of a batch, 1 when the hook forced the slice
// (host only; the out-of-memory status when not even one query fits); rq_test_scan_wide_slice_rows: returns the previous value
int scan_h16_slices(int64_t n, int64_t nq, int m, int h, int k, int64_t out[5]);
int64_t scan_h16_force_slice_rows(int64_t rows);
// linscan_lsq / linscan_cq over 16-bit codes: codebooks [m * h][d]; lut_mode LUT_LSQ (dbnorms [n]) or LUT_CQ
int dev_linscan_aq_wide(float *dists, uint32_t *ids, uint64_t *keys, const int16_t *codes, const float *codebooks,
                        const float *queries, const float *dbnorms, int64_t n, int64_t nq, int m, int h, int d, int k,
                        int lut_mode, uint32_t id_offset, int id_base, hipStream_t stream);
int aq_lut_h16_launch(float *lut, const float *codebooks, const float *queries, int64_t nq, int m, int h, int d, int lut_mode,
                      hipStream_t stream);                // plain [nq][m][h]
int lut_launch(float *lut, const float *centers, const float *queries, int64_t nq, int m, int sub,
               hipStream_t stream);
int synth_codes_launch(uint8_t *codes, int64_t n, int m, uint64_t seed, int64_t row0, hipStream_t stream);

// ---- multi-device (rq_index.hip) ---------------------------------------------------------------
int env_devices(int *out, int cap);   // RAYUELA_HIP_DEVICES -> device list (0 entries = unset)
int host_linscan_sharded(float *dists, uint32_t *ids, const uint8_t *codes, const float *centers, const float *queries,
                         const float *R, int64_t n, int64_t nq, int m, int d, int k, int id_base, const int *devices,
                         int ndev);

// ---- encode / rotation ----------------------------------------------------------------------
int encode_launch(uint8_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h,
                  int num_cu, hipStream_t stream, float *dbg_w = nullptr);
const char *last_encode_kernel_name();   // which kernel the calling thread's last encode_launch chose
void last_encode_stats(unsigned long long out[2]);   // tuning ENC_STATS = 1: {pairs, pairs that took the exact pass} of that encode
// Stage epilogue of RVQ / ERVQ (src/RVQ.jl:56  Xr .-= C[i][:, B[i]]): dst[row][:] = src[row][:] - Cj[code][:] with code =
// codes_in[row * in_stride]; codes_out[row * m + stage] = code and counts[code] += 1 (either may be NULL).  dst may be src.
// Code: uint8_t or int16_t (zero-based, read zero-extended).
template <class Code>
RQ_LOCAL int residual_launch(float *dst, const float *src, const float *Cj, const Code *codes_in, int in_stride, Code *codes_out,
                             unsigned int *counts, int64_t n, int d, int m, int stage, hipStream_t stream);
// the in-place stage of quantize_rvq: Xr -= Ci[stage_codes], codes[:, stage] = stage_codes, cnt[code] += 1 (cnt may be NULL)
int rvq_residual_launch(float *Xr, const float *Ci, const uint8_t *stage_codes, uint8_t *codes, unsigned int *cnt,
                        int64_t n, int d, int m, int stage, hipStream_t stream);
int rvq_encode_launch(uint8_t *codes, float *Xr, uint8_t *stage_codes, unsigned int *counts, const float *C,
                      int64_t n, int d, int m, int h, int num_cu, hipStream_t stream);
int rotate_launch(float *RX, const float *R, const float *X, int d, int64_t n, int num_cu,
                  hipStream_t stream);
// out[i] = in[i] + add (uint8_t / int16_t in either place; in place when out == in, then add == 0 launches nothing)
template <class Out, class In>
RQ_LOCAL int convert_codes_launch(Out *out, const In *in, int64_t nelem, int add, hipStream_t stream);
// zero-based bytes -> Julia's one-based Matrix{Int16} (src/PQ.jl:45-47)
int widen_codes_launch(int16_t *out1, const uint8_t *codes, int64_t nelem, hipStream_t stream);
// ---- more than 256 codewords per codebook, 16-bit codes (rq_encode_h16.hip) --------------------------
// codes [n][m] int16 ZERO-based, 1 <= h <= RQ_MAX_H16; h <= 256 runs encode_launch and widens.  Scratch: WS_H16_SA, WS_H16_CODES.
int encode_h16_launch(int16_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int num_cu,
                      hipStream_t stream);
// one overload set with the byte encode, for the loops that are templates over the code type
inline int encode_launch(int16_t *codes, const float *X, const float *C, int64_t n, int d, int m, int h, int num_cu,
                         hipStream_t stream) {
  return encode_h16_launch(codes, X, C, n, d, m, h, num_cu, stream);
}
int rvq_h16_encode_launch(int16_t *codes, float *Xr, int16_t *stage_codes, unsigned int *counts, const float *C, int64_t n,
                          int d, int m, int h, int num_cu, hipStream_t stream);
int add_base_codes_launch(int16_t *codes, int64_t nelem, int base, hipStream_t stream);   // codes += base, in place
// byte rows at 1 <= h <= RQ_MAX_H16: the checks of every wide encode; encode_h16_kernel<uint8_t> (PQ, h > 256
// only); and the router of rq_encode_bytes.hip -- R null: quantize_pq, else quantize_opq through chunks of R'X in WS_TMP; h <= 256:
// the uint8 byte paths widened.  X at any byte alignment, codes zero-based [n][m].
int h16_encode_check(int d, int m, int h);
int encode_h16_u8_launch(int16_t *codes, const uint8_t *X, const float *C, int64_t n, int d, int m, int h, int num_cu,
                         hipStream_t stream);
int encode_h16_bytes_launch(int16_t *codes, const uint8_t *X, const float *R, const float *C, int64_t n, int d, int m, int h,
                            int num_cu, hipStream_t stream);
void note_encode_h16_kernel();          // rq_last_encode_kernel: "encode_h16_kernel"
// ---- byte rows (rq_encode_bytes.hip): X uint8 [n][d] on the device, any alignment ------------------------------------------
int64_t bytes_chunk_rows(int d);      // rows per upload chunk / per piece of f32 scratch: max(32768, 2^25 / d)
int widen_bytes_launch(float *out, const uint8_t *in, size_t nelem, hipStream_t stream);
// codes of the widened rows (R == null: quantize_pq, else quantize_opq with R [d][d] on the device), as encode_launch gives them
int encode_bytes_launch(uint8_t *codes, const uint8_t *X, const float *R, const float *C, int64_t n, int d, int m, int h,
                        int num_cu, hipStream_t stream);
int rotate_bytes_launch(float *RX, const float *R, const uint8_t *X, int d, int64_t n, int num_cu, hipStream_t stream);
// what a resident dataset (rq_dataset_upload[_bytes], rq_api.hip) holds, for the entries of other files (rq_knn.hip)
struct DatasetView { const void *X; int64_t n; int d, esz, device; };   // esz 4: f32 rows, 1: byte rows
RQ_LOCAL bool dataset_view(const rq_dataset *handle, DatasetView *out);
// ---- exact re-ranking of candidates (rq_rerank.hip) ---------------------------------------------------
// One batch of nb queries on the device: candidate i of query q is the word cand[q * ldc + i * cstep] (cstep 1: ids with id_base
// and id_offset on them; cstep 2: the low words of packed keys, id_base 0 on them), its row is that word - id_base - id_offset.
// dists / ids [nb][k] (device) <- the k smallest (D32, row) pairs, ids + id_offset + id_base.  scratch: rerank_scratch_bytes()
// bytes that nothing else uses until the stream has run the call; nvalid_host [nb] <- every query's candidates inside the base,
// once the stream has been waited for.  The clock gets one mark behind the keys (ph_keys) and one behind the selection (ph_select).
struct RerankCall {
  DatasetView base;
  const float *Q = nullptr;
  const uint32_t *cand = nullptr;
  size_t ldc = 0;
  uint32_t cstep = 1;
  int64_t nb = 0, kc = 0;
  int k = 0;
  uint32_t id_offset = 0;
  int id_base = 0;
  float *dists = nullptr;
  uint32_t *ids = nullptr;
  void *scratch = nullptr;
  uint32_t *nvalid_host = nullptr;      // [nb]
  bool chain = false;                   // rerank_chain(kc), read once per call: the scratch was sized with this value
  int ph_keys = 0, ph_select = 0;
};
RQ_LOCAL size_t rerank_scratch_bytes(int64_t nb, int64_t kc, int k, bool chain);
RQ_LOCAL bool rerank_chain(int64_t kc);      // does kc take the select chain (else the LDS sort)?
RQ_LOCAL int rerank_device(const RerankCall &c, hipStream_t stream, PhaseClock &clk, int num_cu);
// every argument check the entries share (`who` names the entry); no device work
RQ_LOCAL int rerank_check(const char *who, bool null_arg, int64_t n, int64_t kc, int64_t ldc, int k, uint32_t id_offset, int id_base);
// rq_last_rerank_stats / rq_last_rerank_timing of the calling thread: start a call, add its keys / select ms, add its counters
RQ_LOCAL void rerank_clear();
RQ_LOCAL void rerank_add_ms(double keys_ms, double select_ms);
RQ_LOCAL void rerank_note(int64_t nq, int64_t kc, int64_t batches, unsigned long long valid, int chain);

// ---- training reductions (rq_train.hip) --------------------------------------------------------
// Code: uint8_t (1 <= h <= 256; reconstruct: any h) or int16_t (zero-based, read zero-extended, 1 <= h <=
// RQ_MAX_H16; a code outside [0, h): update_centers ignores the row in that sub-space, reconstruct writes zeros for it)
template <class Code>
RQ_LOCAL int update_centers_launch(float *C, unsigned int *counts, const float *X, const Code *codes, int64_t n, int d, int m, int h,
                                   int num_cu, hipStream_t stream);
template <class Code>
RQ_LOCAL int reconstruct_launch(float *CB, const Code *codes, const float *C, int64_t n, int d, int m, int h, hipStream_t stream);
// rq_centers_plan: the slice plan of update_centers_launch (cstride == 0) / ervq_increment_launch (cstride > 0), no device work
void centers_plan_readout(int64_t n, int d, int m, int h, int num_cu, int code_bytes, int cstride, int64_t out[8]);
int qerror_launch(double *acc_dev, const float *X, const float *CB, int64_t n, int d, int num_cu,
                  hipStream_t stream);
struct Rng;
// Clustering.repick_unused_centers on the device: the `unused` entries of Csub [h][sub] re-drawn from the rows of P (stride d,
// columns [col0, col0 + sub)); costs under Cold (the entries the codes were assigned with) in f64 on the device, only the n costs
// come to the host per draw (tc); dtc: n doubles of device scratch.  Code: uint8_t or int16_t at codes[row * cstride + col].
template <class Code>
RQ_LOCAL int refill_unused_launch(float *Csub, const float *Cold, const float *P, const Code *codes, int cstride, int col, int64_t n,
                                  int d, int col0, int sub, const std::vector<int> &unused, Rng &rng, double *dtc,
                                  std::vector<double> &tc, hipStream_t stream);
// Csub[k][s] = X[rows[k]][col0 + s], rows on the device
RQ_LOCAL int gather_rows_launch(float *Csub, const float *X, const long long *rows_dev, int h, int d, int col0, int sub, hipStream_t stream);
// kmeans++ seeding of all m sub-spaces (Clustering.jl init=:kmpp): seeds [m][h] rows, C = their sub-vectors;
// mincost [n][m] floats and partial [m][1024] doubles are scratch, u [m][h] uniforms in [0,1) (device pointers)
int kmpp_init_launch(float *C, long long *seeds, float *mincost, double *partial, const double *u, const float *X,
                     int64_t n, int d, int m, int h, hipStream_t stream);
int polar_factor_launch(float *Rimg, const float *G, double *Vw, int warm, int d, int *status, double *scratch, hipStream_t stream);
bool codes_forms_ok(int d, int m, int h, bool for_gram);
int gram_codes_launch(float *G, const float *X, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h, int num_cu,
                      hipStream_t stream);
int qerror_codes_launch(double *acc_dev, const float *X, const uint8_t *codes, const float *C, int64_t n, int d, int m, int h,
                        int num_cu, hipStream_t stream);
size_t polar_ns_scratch_bytes(int d, int num_cu);
int polar_ns_launch(float *Rimg, const float *G, int d, int *status, void *scratch, int num_cu, hipStream_t stream);
int codes_changed_launch(unsigned long long *out, const uint8_t *a, const uint8_t *b, size_t nbytes, hipStream_t stream);
int gram_launch(float *G, const float *X, const float *CB, int64_t n, int d, int num_cu, hipStream_t stream);

// ---- training loops on host pointers (rq_train_host.hip, rq_ervq.hip) --------------------------------------------------------
// the library's seeded stream (splitmix64): every draw of a training call comes from one of these
struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uniform() { return (double)(next() >> 11) / 9007199254740992.0; }
  double normal() {  // Box-Muller
    double u1 = uniform(), u2 = uniform();
    if (u1 < 1e-300) u1 = 1e-300;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
  }
};
struct DevMem {
  void *p = nullptr;
  ~DevMem() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) { RQ_HIP(hipMalloc(&p, bytes ? bytes : 16)); return RQ_OK; }
  template <class T> T *as() { return reinterpret_cast<T *>(p); }
};
// the Lloyd loop of rq_train_pq on a device-resident X [n][d] (rq_train_host.hip): dC [h * d] and dcodes [n][m] (device) out;
// the caller holds the DeviceLock.  Overwrites the calling thread's rq_train_profile like rq_train_pq.
int train_pq_resident(float *dC, uint8_t *dcodes, const float *dX, int64_t n, int d, int m, int h, int niter, uint64_t seed);
// the same for 1 <= h <= RQ_MAX_H16 and zero-based int16 codes: what rq_train_pq_wide runs between its upload and download
int train_pq_resident_wide(float *dC, int16_t *dcodes, const float *dX, int64_t n, int d, int m, int h, int niter, uint64_t seed);
// ---- database norms of additive-quantizer search (rq_norms.hip) -------------------------------------
// Code: uint8_t (2 <= h <= 256) or int16_t (zero-based and in range, 2 <= h <= RQ_MAX_H16)
template <class Code>
RQ_LOCAL int aq_norms_launch(float *norms, const Code *codes, const float *C, int64_t n, int d, int m, int h, hipStream_t stream);
// norm_codes [n] and / or dbnorms [n] = cbnorms[code] (either may be null); cbnorms [hn], unsorted: hn <= 256 for u8 norm codes
// (the table in static LDS), hn <= RQ_MAX_H16 for int16 ones (dynamic LDS)
int quantize_norms_launch(uint8_t *norm_codes, float *dbnorms, const float *norms, const float *cbnorms, int64_t n, int hn,
                          hipStream_t stream);
int quantize_norms_launch(int16_t *norm_codes, float *dbnorms, const float *norms, const float *cbnorms, int64_t n, int hn,
                          hipStream_t stream);
// ---- ERVQ (rq_train.hip: the increment shares update_centers' segment sum; rq_ervq.hip: epilogue and loop) -------------------
// Code: uint8_t (1 <= h <= 256) or int16_t (zero-based, read zero-extended, 1 <= h <= RQ_MAX_H16)
template <class Code>
RQ_LOCAL int ervq_increment_launch(float *Cj, unsigned int *counts, const float *E, const Code *codes, int64_t n, int d, int cstride,
                                   int col, int h, int num_cu, hipStream_t stream);

// ---- LSQ encoding (rq_icm.hip): argument checks, and the device body of rq_dev_encode_icm (codes already in range) -----
int dev_code_range(const uint8_t *codes, int64_t n, int m, int h, hipStream_t stream, const char *who);   // codes [n][m] < h
RQ_LOCAL int host_code_range(const uint8_t *codes, int64_t n, int m, int h, const char *who);   // on host codes; names the first one >= h
// the same on host int16 codes: every code in code_base .. code_base + h - 1; names the first one outside
RQ_LOCAL int host_code_range(const int16_t *codes, int64_t n, int m, int h, int code_base, const char *who);
int icm_check_args(const void *codes_out, const void *codes_in, const void *X, const void *C, int64_t n, int d, int m,
                   int h, int ilsiter, int icmiter, int npert, int64_t t0, int nsplits);
int icm_encode_dev(uint8_t *codes_out, const uint8_t *codes_in, float *cost_out, const float *X, const float *C,
                   int64_t n, int d, int m, int h, int ilsiter, int icmiter, int npert, int randord, uint64_t seed,
                   int64_t t0, int nsplits, hipStream_t stream, double *unary_ms);
// the same at 2 <= h <= RQ_MAX_H16 over zero-based int16 codes (rq_icm_h16.hip), shape already checked by
// rq_icm_wide_plan's rule.  phase_ms: null, or ICM_PH_N milliseconds added per phase (hipEvents; the call then waits for the stream)
enum { ICM_PH_ILS = 0, ICM_PH_UNARY = 1, ICM_PH_N = 2 };
int icm_encode_wide_dev(int16_t *codes_out, const int16_t *codes_in, float *cost_out, const float *X, const float *C, int64_t n,
                        int d, int m, int h, int ilsiter, int icmiter, int npert, int randord, uint64_t seed, int64_t t0,
                        int nsplits, hipStream_t stream, double *phase_ms);

int icm_sqnorm_launch(float *sa,const float *C, int m, int h, int d, hipStream_t stream);                 // sa[i*h+k] = <c_ik, c_ik>
int icm_unary_launch(float *U, const float *X, const float *C, const float *sa, int64_t nrows, int d, int m, int h, int HS,
                     const int *rng, hipStream_t stream);   // U [nrows][m][HS]; rng [m][2]: codebook i is zero outside [lo, hi), or null
// ---- LSQ codebook update (rq_lsq.hip): A [mh][mh], b [mh][d] f64; A <- its Cholesky factor, Y [mh][d] <- A^-1 Y ------------
int lsq_normal_eq_launch(double *A, double *b, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h,
                         double rho, hipStream_t stream);
int lsq_spd_solve_launch(double *A, double *Y, int mh, int d, hipStream_t stream);
// b [mh][d] f64 and *segs <- the segment bounds [m][h + 1] (device, in WS_LSQ_S) over zero-based int16 codes, 2 <= h <= RQ_MAX_H16:
// the normal equations without their matrix, for the chain update past 256 codewords (rq_chain.hip)
RQ_LOCAL int lsq_b_segs_wide_launch(double *b, const uint32_t **segs, const float *X, const int16_t *codes, int64_t n, int d, int m,
                                    int h, double rho, hipStream_t stream);
// C [m][h][d] f32 <- the fastbin update of (X, codes); *out <- the f64 mean of cost [n] (rq_train_lsq's obj); device pointers
int lsq_update_launch(float *C, const float *X, const uint8_t *codes, int64_t n, int d, int m, int h, double rho,
                      hipStream_t stream);
int lsq_mean_launch(double *out, const float *cost, int64_t n, hipStream_t stream);
// What a full update over int16 codes leaves behind, for a second update over the SAME codes inside one call (rq_train_sr_wide;
// DESIGN.md section 4.27): the Cholesky factor in WS_LSQ_A, the segment bounds and sorted row lists in WS_LSQ_S.  It names the two
// buffers and their sizes; lsq_update_wide_launch uses it only while both are still those.
struct LsqKept {
  const void *a = nullptr, *s = nullptr;
  size_t a_bytes = 0, s_bytes = 0;
};
// lsq_update_launch over zero-based int16 codes, 2 <= h <= RQ_MAX_H16.  again: the codes are those of the update that filled
// *kept, so b alone is summed anew and the kept factor solves it (*reused <- true); else, or when *kept no longer holds, the full
// update runs and refills *kept (*reused <- false).  Both give the same bits.
RQ_LOCAL int lsq_update_wide_launch(float *C, const float *X, const int16_t *codes, int64_t n, int d, int m, int h, double rho,
                                    hipStream_t stream, LsqKept *kept, bool again, bool *reused);
// the shape rule of rq_train_lsq_wide / rq_train_sr_wide: rq_icm_wide_plan passes and m * h <= 16384, else its status
RQ_LOCAL int lsq_train_wide_shape(const char *who, int64_t n, int d, int m, int h, int nsplits);
// the rotation of a training call (rq_train_lsq, rq_train_sr): dR <- R | R' ([d][d] each; R on the host), dRX [n][d] <- R'X
RQ_LOCAL int upload_rotation(DevMem &dR, DevMem &dRX, const float *R, const float *X, int64_t n, int d, int num_cu, hipStream_t stream);
}  // namespace rq
