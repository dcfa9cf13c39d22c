// rq_index.hip -- device-resident index handle of the C ABI: codes uploaded once, searched many times,
// on ONE device or row-sharded over the GPUs of a node from a single host process.
//
// The reference has no multi-device path: src/Linscan.jl:5-26 hands the whole code matrix to one
// OpenMP loop over queries (deps/src/linscan_aqd.cpp:55-61), whose only long-axis device is the 1e7-row
// chunking with a carried top-k (:52-53,78-92).  The MI355X analogue behind the same call:
//
//   shard     rows [row0_s, row0_s + n_s) of the base live on device dev_s as resident uint8 codes
//             (rq_index_set_codes splits the caller's matrix; rq_index_set_codes_synth fills the
//             SIFT1B-shape synthetic base on the devices themselves)
//   scan      every device scans its shards for ALL queries on its own stream (queries and codebooks
//             are replicated, 0.5 MB + 128 KiB) and leaves sorted packed keys
//             (ordered(dist) << 32 | GLOBAL row id) per shard                    -- no communication
//   gather    the per-shard key lists (nq*k*8 bytes each) go to the root device over xGMI: RCCL
//             send/recv inside one group on the single-process communicator clique (ncclCommInitAll,
//             /opt/rocm/include/rccl/rccl.h:236), i.e. a gather-to-root over P-1 DISTINCT links -- or
//             hipMemcpyPeerAsync pushes (SDMA engines, no CUs) when RCCL is unavailable or disabled
//             (tuning EXCHANGE_PEER=1); shards that live on the root device write in place
//   merge     merge_topk over the P lists per query on the root.  Keys are totally ordered and ids are
//             global, so the answer is bit-identical to one scan of the whole base.
//
// A device may appear several times in the device list: every occurrence is one LOGICAL shard (that is
// how the sharded path is tested on a one-GPU box, and how a base of >= 2^31 rows fits one device).
// librccl is dlopen()ed on first use, so the library has no link-time dependency on it.
//
// The same handle serves the additive quantizers (rq_index_create_aq[_wide]): full-dimensional codebooks,
// per-shard row norms for linscan_lsq, the shard scans of rq_linscan_lsq / rq_linscan_cq and their forms over 16-bit codes.
//
// What a shard keeps on its device is one ResidentBase (rq_internal.h), freed in one place (its free()) and
// ordered in one place (resident_order, rq_api.hip).  The three setters open alike (set_open: every refusal on the arguments, the
// row split computed without writing the index) and replace the loaded base by one of two rules (index_replace_base):
//   rq_index_set_codes[_synth], _aq     the loaded base is freed FIRST (a base and its replacement need not fit together), then
//                                       the shards are built one by one; an error half-way leaves "index has no codes"
//   rq_index_set_codes_wide, _aq_wide   the new rows (and norms) are validated in fresh allocations first and replace the loaded
//                                       ones together; a refused base leaves the loaded one answering
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "rq_internal.h"
#include "rq_topk.h"

namespace rq {

// ---- RCCL through dlopen ------------------------------------------------------------------------
struct RcclApi {
  void *handle = nullptr;
  bool tried = false;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  bool ok() const { return handle != nullptr; }
};
static RcclApi g_rccl;
static std::mutex g_rccl_mu;

static bool rccl_load() {
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (g_rccl.tried) return g_rccl.ok();
  g_rccl.tried = true;
  const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void *h = nullptr;
  for (const char *nm : names) {
    h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
    if (h) break;
  }
  if (!h) return false;
#define RQ_SYM(field, name)                                                \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name)); \
  if (!g_rccl.field) { dlclose(h); return false; }
  RQ_SYM(CommInitAll, "ncclCommInitAll")
  RQ_SYM(CommDestroy, "ncclCommDestroy")
  RQ_SYM(GroupStart, "ncclGroupStart")
  RQ_SYM(GroupEnd, "ncclGroupEnd")
  RQ_SYM(Send, "ncclSend")
  RQ_SYM(Recv, "ncclRecv")
  RQ_SYM(GetErrorString, "ncclGetErrorString")
#undef RQ_SYM
  g_rccl.handle = h;
  return true;
}

#define RQ_NCCL(expr)                                                                                 \
  do {                                                                                                \
    ncclResult_t _r = (expr);                                                                         \
    if (_r != ncclSuccess) return fail(1000 + (int)_r, "RCCL error %d (%s) in `%s`", (int)_r,         \
                                       g_rccl.GetErrorString ? g_rccl.GetErrorString(_r) : "?", #expr); \
  } while (0)

// ---- [P][nq][k] -> [nq][P][k] ---------------------------------------------------------------------
// pstride = keys between the blocks of two shards (nq_total * k when only a chunk of the queries is interleaved)
__global__ void interleave_keys_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, size_t nq, uint32_t P,
                                       uint32_t k, size_t pstride) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per_q = (size_t)P * k;
  if (i >= nq * per_q) return;
  const size_t q = i / per_q;
  const uint32_t rem = (uint32_t)(i - q * per_q);
  const uint32_t p = rem / k, j = rem - p * k;
  dst[i] = src[(size_t)p * pstride + q * k + j];
}

int interleave_keys_launch(uint64_t *dst, const uint64_t *src, int64_t nq, int P, int k, size_t pstride, hipStream_t stream) {
  const size_t total = (size_t)nq * P * k;
  if (!total) return RQ_OK;
  hipLaunchKernelGGL(interleave_keys_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, dst, src,
                     (size_t)nq, (uint32_t)P, (uint32_t)k, pstride);
  RQ_HIP(hipGetLastError());
  return RQ_OK;
}

// ---- the handle -------------------------------------------------------------------------------------
constexpr int IX_MAX_CHUNKS = 8;

struct IxDev {          // one per DISTINCT device of the index
  int device = 0;
  int num_cu = 0;
  hipStream_t stream = nullptr;     // uploads, rotation, scans
  hipStream_t xstream = nullptr;    // top-k lists towards the root (SDMA peer copies / RCCL send, recv)
  hipStream_t mstream = nullptr;    // root only: interleave + merge of a query chunk
  hipEvent_t ev_scan[IX_MAX_CHUNKS] = {nullptr};   // this device's lists of chunk c are complete
  hipEvent_t ev_xfer[IX_MAX_CHUNKS] = {nullptr};   // ... and have arrived on the root
  float *centers = nullptr;
  float *queries = nullptr, *queries_rot = nullptr, *R = nullptr;
  size_t q_cap = 0;
};

struct IxShard {
  int dev = 0;          // index into devs
  int64_t row0 = 0, n = 0;
  ResidentBase base;    // the shard's rows (a wide index keeps int16 rows, in arrival order), perm, and for an LSQ shard the norms
                        // of rows [row0, row0 + n) and the prepared norm buffer (rq_internal.h)
  uint64_t *keys = nullptr;   // [nq][k] sorted keys of the last search (shards off the root device)
  size_t keys_cap = 0;
  uint64_t *tmp = nullptr;    // [nq][k_local] when the shard holds fewer than k rows
  size_t tmp_cap = 0;
};


static int grow(void **p, size_t *cap, size_t bytes) {
  if (*cap >= bytes && *p) return RQ_OK;
  if (*p) { RQ_HIP(hipDeviceSynchronize()); RQ_HIP(hipFree(*p)); *p = nullptr; *cap = 0; }
  const size_t want = (std::max<size_t>(bytes, 256) + 255) & ~(size_t)255;
  RQ_HIP(hipMalloc(p, want));
  *cap = want;
  return RQ_OK;
}

}  // namespace rq

using namespace rq;

struct rq_index {
  int m = 0, d = 0;
  int h = 256;          // codewords per codebook; wide: int16 codes scanned by dev_linscan_wide
  bool wide = false;
  int lut_mode = LUT_PQ;      // LUT_LSQ / LUT_CQ: an additive-quantizer index (rq_index_create_aq[_wide]) --
                              // `centers` are full-dimensional codebooks [m * h][d], an LSQ shard carries its row norms
  int64_t n = 0;
  uint32_t id_offset = 0;
  std::vector<IxDev> devs;
  std::vector<IxShard> shards;
  // on the root device (devs[0])
  uint64_t *gathered = nullptr, *inter = nullptr;
  size_t gathered_cap = 0, inter_cap = 0;
  float *dd = nullptr;
  uint32_t *di = nullptr;
  size_t dd_cap = 0, di_cap = 0;
  // exchange
  ncclComm_t comms[16] = {nullptr};
  int exchange = 0;     // 0 none (one device), 1 peer copies, 2 RCCL
  bool peer_ok = false;    // every device has a direct path to the root (hipDeviceCanAccessPeer)
  bool selftest = false;   // tuning EXCHANGE_SELFTEST on ONE device: logical shards 1.. travel through RCCL send/recv to self
  std::mutex mu;
};

namespace rq {

static void index_free(rq_index *ix) {
  if (!ix) return;
  SavedDevice saved;
  if (ix->exchange == 2 && g_rccl.ok())
    for (size_t i = 0; i < ix->devs.size(); ++i)
      if (ix->comms[i]) (void)g_rccl.CommDestroy(ix->comms[i]);
  for (auto &s : ix->shards) {
    if (hipSetDevice(ix->devs[s.dev].device) != hipSuccess) continue;
    s.base.free();
    if (s.keys) (void)hipFree(s.keys);
    if (s.tmp) (void)hipFree(s.tmp);
  }
  for (size_t i = 0; i < ix->devs.size(); ++i) {
    IxDev &dv = ix->devs[i];
    if (hipSetDevice(dv.device) != hipSuccess) continue;
    if (i == 0) {
      if (ix->gathered) (void)hipFree(ix->gathered);
      if (ix->inter) (void)hipFree(ix->inter);
      if (ix->dd) (void)hipFree(ix->dd);
      if (ix->di) (void)hipFree(ix->di);
    }
    if (dv.centers) (void)hipFree(dv.centers);
    if (dv.queries) (void)hipFree(dv.queries);
    if (dv.queries_rot) (void)hipFree(dv.queries_rot);
    if (dv.R) (void)hipFree(dv.R);
    for (int c = 0; c < IX_MAX_CHUNKS; ++c) {
      if (dv.ev_scan[c]) (void)hipEventDestroy(dv.ev_scan[c]);
      if (dv.ev_xfer[c]) (void)hipEventDestroy(dv.ev_xfer[c]);
    }
    if (dv.xstream) (void)hipStreamDestroy(dv.xstream);
    if (dv.mstream) { (void)release_stream_workspace(dv.mstream); (void)hipStreamDestroy(dv.mstream); }
    if (dv.stream) { (void)release_stream_workspace(dv.stream); (void)hipStreamDestroy(dv.stream); }
  }
  (void)hipGetLastError();
  delete ix;
}

static int index_build(rq_index *ix, int m, int d, const float *centers_host, const int *devices, int ndev, int h = 256,
                       bool wide = false, int lut_mode = LUT_PQ) {
  if (wide && (m < 1 || m > 32)) return fail(RQ_EUNSUPPORTED, "wide index covers 1 <= m <= 32; got m=%d", m);
  if (wide && (h < 1 || h > RQ_MAX_H16))
    return fail(RQ_EUNSUPPORTED, "wide index holds Int16 codes: 1 <= h <= %d; got h=%d", RQ_MAX_H16, h);
  // (an AQ index has full-dimensional codebooks: any d >= 1, checked by its create entries)
  if (lut_mode == LUT_PQ && (m < 1 || d < m || d % m))
    return fail(RQ_EINVAL, "index: scan needs d %% m == 0 (src/Linscan.jl:23); got d=%d m=%d", d, m);
  if (!centers_host) return fail(RQ_EINVAL, "index: centers is NULL");
  if (ndev < 1 || ndev > 64) return fail(RQ_EINVAL, "index: 1 <= number of shards <= 64, got %d", ndev);
  int visible = 0;
  if (hipGetDeviceCount(&visible) != hipSuccess || visible < 1) { (void)hipGetLastError(); return fail(RQ_ENODEVICE, "no HIP device visible"); }
  ix->m = m; ix->d = d; ix->h = h; ix->wide = wide; ix->lut_mode = lut_mode;
  const size_t ce = (size_t)m * h * (lut_mode == LUT_PQ ? d / m : d) * 4;
  for (int s = 0; s < ndev; ++s) {
    const int dev = devices[s];
    if (dev < 0 || dev >= visible || dev >= 16) return fail(RQ_EINVAL, "index: device %d not in [0, %d)", dev, std::min(visible, 16));
    int di = -1;
    for (size_t i = 0; i < ix->devs.size(); ++i) if (ix->devs[i].device == dev) di = (int)i;
    if (di < 0) {
      IxDev dv;
      dv.device = dev;
      RQ_HIP(hipSetDevice(dev));
      DeviceInfo info;
      RQ_TRY(device_info(&info));
      dv.num_cu = info.num_cu;
      ix->devs.push_back(dv);
      di = (int)ix->devs.size() - 1;
      IxDev &r = ix->devs[di];
      RQ_HIP(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
      RQ_HIP(hipStreamCreateWithFlags(&r.xstream, hipStreamNonBlocking));
      if (di == 0) RQ_HIP(hipStreamCreateWithFlags(&r.mstream, hipStreamNonBlocking));
      for (int c = 0; c < IX_MAX_CHUNKS; ++c) {
        RQ_HIP(hipEventCreateWithFlags(&r.ev_scan[c], hipEventDisableTiming));
        RQ_HIP(hipEventCreateWithFlags(&r.ev_xfer[c], hipEventDisableTiming));
      }
      RQ_HIP(hipMalloc((void **)&r.centers, ce));
      RQ_HIP(hipMemcpy(r.centers, centers_host, ce, hipMemcpyHostToDevice));
    }
    IxShard sh;
    sh.dev = di;
    ix->shards.push_back(sh);
  }
  const int nd = (int)ix->devs.size();
  if (nd == 1 && ix->shards.size() > 1 && tuning("EXCHANGE_SELFTEST", 0) && rccl_load()) {
    // one-GPU boxes: run the RCCL transport anyway (a clique of one, every list but the first sent to self), so
    // that dlopen, communicator, group semantics and datatypes are exercised on real hardware
    int list[1] = {ix->devs[0].device};
    if (g_rccl.CommInitAll(ix->comms, 1, list) == ncclSuccess) { ix->exchange = 2; ix->selftest = true; }
  }
  if (nd > 1) {
    // direct xGMI paths root <-> every other device (a failure only means staged copies)
    const int root = ix->devs[0].device;
    ix->peer_ok = true;
    for (int i = 1; i < nd; ++i) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, root, ix->devs[i].device) != hipSuccess || !can) ix->peer_ok = false;
      if (can) {
        (void)hipSetDevice(root);
        (void)hipDeviceEnablePeerAccess(ix->devs[i].device, 0);
        (void)hipSetDevice(ix->devs[i].device);
        (void)hipDeviceEnablePeerAccess(root, 0);
      }
      (void)hipGetLastError();
    }
    ix->exchange = 1;
    if (!tuning("EXCHANGE_PEER", 0) && rccl_load()) {
      int list[16];
      for (int i = 0; i < nd; ++i) list[i] = ix->devs[i].device;
      const ncclResult_t r = g_rccl.CommInitAll(ix->comms, nd, list);
      if (r == ncclSuccess) ix->exchange = 2;
      else fprintf(stderr, "librayuela_hip: ncclCommInitAll failed (%s); using peer copies for the top-k exchange\n",
                   g_rccl.GetErrorString(r));
    }
  }
  return RQ_OK;
}

// The split of a base of n rows over P shards: shard s holds rows [row0, row0 + n), the first n % P shards one row more than the
// rest.  Nothing of an index is written: a setter commits the bounds (index_replace_base) once it can no longer refuse the call.
struct RowSpan { int64_t row0 = 0, n = 0; };
static std::vector<RowSpan> shard_bounds(size_t P, int64_t n) {
  std::vector<RowSpan> split(P);
  const int64_t per = n / (int64_t)P, extra = n % (int64_t)P;
  int64_t row = 0;
  for (size_t s = 0; s < P; ++s) {
    split[s].row0 = row;
    split[s].n = per + ((int64_t)s < extra ? 1 : 0);
    row += split[s].n;
  }
  return split;
}

// The opening of the three setters: everything a call is refused for on its arguments, with nothing of the index written and no
// device touched.  aq, wide: the kind and the row width of index that the setter serves (the message names the setter of the index
// that was passed); who: the entry's name in its messages -- null for rq_index_set_codes[_synth], which say "index" and have looked
// at their codes themselves.  *split: the rows of every shard.
static int set_open(std::vector<RowSpan> *split, rq_index *ix, const char *who, bool aq, bool wide, const void *codes_host,
                    const float *dbnorms, const float *cbnorms, int hn, int64_t n, uint32_t id_offset, int code_base) {
  if (!ix) return fail(RQ_EINVAL, "index is NULL");
  const bool ix_aq = ix->lut_mode != LUT_PQ;
  if (ix_aq != aq || ix->wide != wide)      // the kind before the width
    return fail(RQ_EINVAL, "%s: %s index takes its codes through rq_index_set_codes%s%s", who ? who : "index",
                ix_aq != aq ? (ix_aq ? "an additive-quantizer" : "a PQ") : (ix->wide ? "a wide" : "a byte"), ix_aq ? "_aq" : "",
                ix->wide ? "_wide" : "");
  if (who && !codes_host) return fail(RQ_EINVAL, "index: codes is NULL");
  // a norm argument that does not fit lut_mode
  if (ix->lut_mode == LUT_CQ && (dbnorms || cbnorms)) return fail(RQ_EINVAL, "%s: a CQ index takes no norms (T = |q - c|^2 holds them)", who);
  if (ix->lut_mode == LUT_LSQ) {
    if (!dbnorms == !cbnorms) return fail(RQ_EINVAL, "%s: an LSQ index takes exactly one of dbnorms [n] and cbnorms [hn]", who);
    const int hn_max = wide ? RQ_MAX_H16 : 256;
    if (cbnorms && (hn < 1 || hn > hn_max)) return fail(RQ_EINVAL, "%s: hn=%d outside 1..%d", who, hn, hn_max);
    if (cbnorms && ix->h < 2) return fail(RQ_EINVAL, "%s: the norms need 2 <= h; got h=%d", who, ix->h);   // (rq_linscan_lsq_cbnorms_wide's rule)
  }
  if (wide && code_base != 0 && code_base != 1) return fail(RQ_EINVAL, "%s: code_base must be 0 or 1; got %d", who, code_base);
  if (n < 1) return fail(RQ_EINVAL, "index: n=%lld must be >= 1", (long long)n);
  // same bound as dev_linscan: the last id must stay below 0xFFFFFFFF (that id is the padding key KEY_MAX's)
  if ((uint64_t)id_offset + (uint64_t)n > 0xFFFFFFFFull) return fail(RQ_EINVAL, "index: row ids overflow uint32 (id_offset + n must be <= 2^32 - 1)");
  *split = shard_bounds(ix->shards.size(), n);
  if (split->front().n >= (1LL << 31))      // (the first shard is a largest one)
    return fail(RQ_EUNSUPPORTED, "index: a shard of %lld rows exceeds 2^31-1; use more shards", (long long)split->front().n);
  return RQ_OK;
}

// The loaded base goes and the new row bounds stand: the index reports "index has no codes" until its setter has seen every shard
// stand and sets ix->n.  fresh == nullptr (the byte setters): the shards are left empty, to be built one by one -- a base and its
// replacement need not fit together, and an error half-way (a device fault, no memory for a shard) leaves the index without codes.
// Else (the wide setter) every shard takes over its validated replacement.
static int index_replace_base(rq_index *ix, const std::vector<RowSpan> &split, std::vector<ResidentBase> *fresh = nullptr) {
  ix->n = 0;
  for (size_t i = 0; i < ix->shards.size(); ++i) {
    IxShard &s = ix->shards[i];
    IxDev &dv = ix->devs[s.dev];
    RQ_HIP(hipSetDevice(dv.device));
    if (s.base.mem) RQ_HIP(hipStreamSynchronize(dv.stream));
    s.base.free();
    s.row0 = split[i].row0;
    s.n = split[i].n;
    if (fresh) std::swap(s.base, (*fresh)[i]);
  }
  return RQ_OK;
}

// rq_index_set_codes[_synth]: every shard's rows are allocated for a base of n rows; fill(rows, row0, n, stream) queues the upload /
// generator of the shard's rows.  Replace rule: index_replace_base's.
template <class Fill>
static int index_set(rq_index *ix, int64_t n, uint32_t id_offset, Fill fill) {
  std::vector<RowSpan> split;
  RQ_TRY(set_open(&split, ix, nullptr, false, false, nullptr, nullptr, nullptr, 0, n, id_offset, 0));
  std::lock_guard<std::mutex> lk(ix->mu);
  SavedDevice saved;
  RQ_TRY(index_replace_base(ix, split));
  for (auto &s : ix->shards) {
    if (s.n == 0) continue;
    IxDev &dv = ix->devs[s.dev];
    RQ_HIP(hipSetDevice(dv.device));
    uint8_t *rows = nullptr;
    RQ_HIP(hipMalloc((void **)&rows, (size_t)s.n * ix->m));
    s.base.adopt_rows(rows);
    RQ_TRY(fill(rows, s.row0, s.n, dv.stream));
    // Rows of a tiled width are ordered once, here; other widths are not padded now: they are padded and ordered per search.
    if (scan_padded_m(ix->m) == ix->m) {
      DeviceLock order_lock;      // scratch lookup + launches of this device, like a scan
      const int rc = resident_order(&s.base, s.n, ix->m, dv.stream);
      // the key scratch (4 bytes per row + the histogram) is not needed again
      if (rc != RQ_OK || s.base.perm) (void)release_stream_workspace(dv.stream);
      RQ_TRY(rc);
    }
  }
  for (auto &dv : ix->devs) {
    RQ_HIP(hipSetDevice(dv.device));
    RQ_HIP(hipStreamSynchronize(dv.stream));
  }
  ix->n = n;
  ix->id_offset = id_offset;
  return RQ_OK;
}

// rq_index_set_codes_aq: every shard is prepared the way rq_lsq_prepare prepares its one base (aq_base_prepare, rq_api.hip) --
// rows padded to a tiled width, bank-aware order once, the shard's norms gathered through the shard's own perm, the LSQ
// pre-filter's norm buffer built once.  Byte codes cannot be out of range, so nothing is refused after the first shard is touched.
// Replace rule: index_replace_base's.
static int index_set_aq(rq_index *ix, const uint8_t *codes_host, const float *dbnorms, const float *cbnorms, int hn, int64_t n,
                        uint32_t id_offset) {
  std::vector<RowSpan> split;
  RQ_TRY(set_open(&split, ix, "rq_index_set_codes_aq", true, false, codes_host, dbnorms, cbnorms, hn, n, id_offset, 0));
  std::lock_guard<std::mutex> lk(ix->mu);
  SavedDevice saved;
  RQ_TRY(index_replace_base(ix, split));
  for (auto &s : ix->shards) {
    if (s.n == 0) continue;
    IxDev &dv = ix->devs[s.dev];
    RQ_HIP(hipSetDevice(dv.device));
    DeviceLock prepare_lock;      // scratch lookup + launches of this device, like a scan
    const int rc = aq_base_prepare(&s.base, codes_host + (size_t)s.row0 * ix->m, dv.centers, dbnorms ? dbnorms + s.row0 : nullptr,
                                   cbnorms, hn, s.n, ix->m, ix->d, ix->lut_mode == LUT_LSQ, dv.stream);
    (void)release_stream_workspace(dv.stream);    // the order's key scratch is not needed again
    if (rc != RQ_OK) { (void)hipStreamSynchronize(dv.stream); s.base.free(); return rc; }
  }
  ix->n = n;
  ix->id_offset = id_offset;
  return RQ_OK;
}

// The wide forms of index_set / index_set_aq: int16 rows, no row order.  Every shard's new rows are uploaded to a fresh allocation
// and checked there (prepare_codes_h16_kernel: zero-based in place, the first row with a code outside [0, h)) BEFORE anything of the
// index is replaced, so a refused base leaves the loaded one answering as before.  Old and new rows are resident together until then.
// `aq`: rq_index_set_codes_aq_wide -- an LSQ shard's norms are uploaded (dbnorms) or computed from the shard's own validated rows on
// the shard's device (cbnorms: aq_norms_launch + quantize_norms_launch, the arithmetic of rq_linscan_lsq_cbnorms_wide) into a fresh
// allocation too, and replace the old ones together with the rows.
static int index_set_wide(rq_index *ix, const int16_t *codes_host, int64_t n, int code_base, uint32_t id_offset, bool aq = false,
                          const float *dbnorms = nullptr, const float *cbnorms = nullptr, int hn = 0) {
  const char *who = aq ? "rq_index_set_codes_aq_wide" : "rq_index_set_codes_wide";
  std::vector<RowSpan> split;
  RQ_TRY(set_open(&split, ix, who, aq, true, codes_host, dbnorms, cbnorms, hn, n, id_offset, code_base));
  std::lock_guard<std::mutex> lk(ix->mu);
  SavedDevice saved;
  const int m = ix->m, h = ix->h;
  const size_t P = ix->shards.size();
  const bool lsq = aq && ix->lut_mode == LUT_LSQ;
  std::vector<ResidentBase> fresh(P);
  auto drop = [&]() {
    for (size_t s = 0; s < P; ++s)
      if (fresh[s].mem && hipSetDevice(ix->devs[ix->shards[s].dev].device) == hipSuccess) fresh[s].free();
    (void)hipGetLastError();
  };
  int rc = RQ_OK;
  for (size_t s = 0; s < P && rc == RQ_OK; ++s) {
    const int64_t sn = split[s].n, row0 = split[s].row0;
    if (sn == 0) continue;
    IxDev &dv = ix->devs[ix->shards[s].dev];
    rc = [&]() -> int {
      RQ_HIP(hipSetDevice(dv.device));
      int16_t *rows = nullptr;
      RQ_HIP(hipMalloc((void **)&rows, (size_t)sn * m * 2));
      fresh[s].adopt_rows(rows);
      DevMem flag;
      RQ_TRY(flag.alloc(8));
      RQ_HIP(hipMemcpyAsync(rows, codes_host + (size_t)row0 * m, (size_t)sn * m * 2, hipMemcpyHostToDevice, dv.stream));
      RQ_TRY(prepare_codes_h16_launch(rows, flag.as<unsigned long long>(), sn, m, h, code_base, dv.stream));
      unsigned long long first_bad = 0;
      RQ_HIP(hipMemcpyAsync(&first_bad, flag.p, 8, hipMemcpyDeviceToHost, dv.stream));
      RQ_HIP(hipStreamSynchronize(dv.stream));
      if (first_bad != ~0ull)      // shards are checked in row order: this is the first bad row of the base
        return fail(RQ_EINVAL, "%s: row %llu holds a code outside [%d, %d]; the index keeps the base it had", who,
                    (unsigned long long)row0 + first_bad, code_base, h - 1 + code_base);
      if (!lsq) return RQ_OK;
      // the shard's norms, from rows that are zero-based and in range by now
      float *nrm = nullptr;
      RQ_HIP(hipMalloc((void **)&nrm, (size_t)sn * 4));
      fresh[s].norms = nrm;
      if (dbnorms) {
        RQ_HIP(hipMemcpyAsync(nrm, dbnorms + row0, (size_t)sn * 4, hipMemcpyHostToDevice, dv.stream));
        RQ_HIP(hipStreamSynchronize(dv.stream));
        return RQ_OK;
      }
      DevMem dcbn;
      RQ_TRY(dcbn.alloc((size_t)hn * 4));
      RQ_HIP(hipMemcpyAsync(dcbn.p, cbnorms, (size_t)hn * 4, hipMemcpyHostToDevice, dv.stream));
      DeviceLock norms_lock;
      RQ_TRY(aq_norms_launch(nrm, rows, dv.centers, sn, ix->d, m, h, dv.stream));
      RQ_TRY(quantize_norms_launch((int16_t *)nullptr, nrm, nrm, dcbn.as<float>(), sn, hn, dv.stream));
      RQ_HIP(hipStreamSynchronize(dv.stream));      // before the table goes back
      return RQ_OK;
    }();
  }
  if (rc == RQ_OK) rc = index_replace_base(ix, split, &fresh);
  if (rc != RQ_OK) { drop(); return rc; }
  ix->n = n;
  ix->id_offset = id_offset;
  return RQ_OK;
}

int index_search(rq_index *ix, float *dists, uint32_t *ids, const float *queries_host, const float *R_host, int64_t nq,
                 int k, int id_base) {
  if (!ix || ix->n < 1) return fail(RQ_EINVAL, "index has no codes");
  if (nq <= 0) return RQ_OK;
  if (k < 1) return fail(RQ_EUNSUPPORTED, "k=%d outside [1, n]", k);
  if (k > ix->n) return fail(RQ_EINVAL, "k=%d > n=%lld (undefined in the reference, deps/src/linscan_aqd.cpp:91)", k, (long long)ix->n);
  if (id_base != 0 && id_base != 1) return fail(RQ_EINVAL, "id_base must be 0 or 1");
  if (!dists || !ids || !queries_host) return fail(RQ_EINVAL, "index search: NULL argument");
  {
    // bulk path (k > RQ_MAX_K): results, gathered and interleaved lists ((2 P + 1) x nq x k x 8 bytes on the root device)
    // are bounded by query chunks of at most BULK_HOST_RESULT_BYTES of each
    const int64_t per_q = (int64_t)k * 8 * (2 * (int64_t)ix->shards.size() + 1);
    const int64_t chunk = std::max<int64_t>(1, (int64_t)BULK_HOST_RESULT_BYTES / per_q);
    if (k > RQ_MAX_K && nq > chunk) {
      Timer tc;
      for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
        const int64_t nqc = std::min(chunk, nq - q0);
        RQ_TRY(index_search(ix, dists + (size_t)q0 * k, ids + (size_t)q0 * k, queries_host + (size_t)q0 * ix->d, R_host, nqc,
                            k, id_base));
      }
      set_timing(tc.ms(), 0, 0, 0);
      return RQ_OK;
    }
  }
  std::lock_guard<std::mutex> lk(ix->mu);
  SavedDevice saved;
  Timer tt;
  const int m = ix->m, d = ix->d;
  const int P = (int)ix->shards.size();
  const size_t qb = (size_t)nq * d * 4, cnt = (size_t)nq * k, ob = cnt * 4;
  IxDev &root = ix->devs[0];

  // ---- queries to every device (and R'q there: linscan_opq rotates the queries first, src/Linscan.jl:102) ----
  Timer t1;
  for (auto &dv : ix->devs) {
    RQ_HIP(hipSetDevice(dv.device));
    if (dv.q_cap < qb) {
      RQ_HIP(hipStreamSynchronize(dv.stream));
      if (dv.queries) RQ_HIP(hipFree(dv.queries));
      if (dv.queries_rot) RQ_HIP(hipFree(dv.queries_rot));
      dv.queries = dv.queries_rot = nullptr;
      dv.q_cap = 0;
      RQ_HIP(hipMalloc((void **)&dv.queries, qb));
      RQ_HIP(hipMalloc((void **)&dv.queries_rot, qb));
      dv.q_cap = qb;
    }
    RQ_HIP(hipMemcpyAsync(dv.queries, queries_host, qb, hipMemcpyHostToDevice, dv.stream));
    if (R_host) {
      if (!dv.R) RQ_HIP(hipMalloc((void **)&dv.R, (size_t)d * d * 4));
      RQ_HIP(hipMemcpyAsync(dv.R, R_host, (size_t)d * d * 4, hipMemcpyHostToDevice, dv.stream));
      RQ_TRY(rotate_launch(dv.queries_rot, dv.R, dv.queries, d, nq, dv.num_cu, dv.stream));
    }
  }
  const double h2d_ms = t1.ms();
  Timer t2;

  RQ_HIP(hipSetDevice(root.device));
  RQ_TRY(grow((void **)&ix->dd, &ix->dd_cap, ob));
  RQ_TRY(grow((void **)&ix->di, &ix->di_cap, ob));
  // one shard's scan on its device's stream (the device is current), by (wide, lut_mode): dists + ids, or sorted keys
  auto scan_shard = [&](IxShard &s, IxDev &dv, float *sd, uint32_t *si, uint64_t *sk, const float *qs, int64_t nqs, int ks,
                        uint32_t id_off, int base) -> int {
    if (ix->wide) {
      const int16_t *c16 = s.base.rows16();
      if (ix->lut_mode != LUT_PQ)
        return dev_linscan_aq_wide(sd, si, sk, c16, dv.centers, qs, s.base.norms, s.n, nqs, m, ix->h, d, ks, ix->lut_mode, id_off, base,
                                   dv.stream);
      return dev_linscan_wide(sd, si, sk, c16, dv.centers, qs, s.n, nqs, m, ix->h, d, ks, id_off, base, dv.stream);
    }
    ScanBase sb;
    sb.perm = s.base.perm;
    if (ix->lut_mode != LUT_PQ) {       // an AQ shard is an aq_base_prepare base: padded rows, the norm buffer where the filter applies
      sb.padded = true;
      sb.norm_prepared = s.base.normb;
    }
    return dev_linscan(sd, si, sk, s.base.rows(), dv.centers, qs, s.n, nqs, m, d, ks, id_off, base, dv.stream, ix->lut_mode,
                       s.base.norms, &sb);
  };
  if (P == 1) {
    RQ_TRY(scan_shard(ix->shards[0], root, ix->dd, ix->di, nullptr, R_host ? root.queries_rot : root.queries, nq, k, ix->id_offset,
                      id_base));
  } else {
    RQ_TRY(grow((void **)&ix->gathered, &ix->gathered_cap, (size_t)P * cnt * 8));
    RQ_TRY(grow((void **)&ix->inter, &ix->inter_cap, (size_t)P * cnt * 8));
    // Query chunks: with several devices and long lists (k x nq x 8 B per shard: 80 MB at SIFT1M shape with k = 1000,
    // 800 MB with the reference's default k = 10000) the exchange is as long as a device's scan of its 1/8 of the rows.
    // The queries are then cut into C chunks and pipelined: scan of chunk c+1 on `stream` | lists of chunk c towards
    // the root on `xstream` | merge of chunk c-1 on the root's `mstream`.  In that mode the lists travel as SDMA peer
    // copies: the persistent scan grid holds every CU and all of the LDS, an RCCL kernel would wait for the scan to
    // drain, the copy engines do not need a CU.  Every extra chunk costs a shard ~0.17 ms of fixed scan overhead
    // (tools/chunk_cost.py: tables, threshold sample, launch tails), an xGMI link moves 64 MB in ~0.42 ms, so a
    // chunk is at least 64 MB.  Unchunked (BASELINE config 5: 0.8 MB per device) the exchange is one RCCL group.
    int C = tuning("IDX_QCHUNKS", 0);
    if (C <= 0) C = (ix->devs.size() > 1) ? (int)std::min<size_t>(cnt * 8 / ((size_t)64 << 20), 4) : 1;
    C = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(C, IX_MAX_CHUNKS), nq));
    const bool use_rccl = ix->exchange == 2 && (C == 1 || ix->selftest || !ix->peer_ok || tuning("EXCHANGE_CHUNK_RCCL", 0));
    auto remote = [&](int si) { return ix->shards[si].dev != 0 || (ix->selftest && si > 0); };

    // ---- buffers first (growing one may synchronise the device) -----------------------------------------
    for (int si = 0; si < P; ++si) {
      IxShard &s = ix->shards[si];
      IxDev &dv = ix->devs[s.dev];
      RQ_HIP(hipSetDevice(dv.device));
      if (remote(si)) RQ_TRY(grow((void **)&s.keys, &s.keys_cap, cnt * 8));
      const int k_local = (int)std::min<int64_t>(k, s.n);
      if (k_local < k && k_local > 0) RQ_TRY(grow((void **)&s.tmp, &s.tmp_cap, (size_t)nq * k_local * 8));
      if (k_local < k)      // KEY_MAX padding: the shard has < k rows
        RQ_HIP(hipMemsetAsync(remote(si) ? s.keys : ix->gathered + (size_t)si * cnt, 0xFF, cnt * 8, dv.stream));
    }
    for (int c = 0; c < C; ++c) {
      const int64_t q0 = nq * c / C, nqc = nq * (c + 1) / C - q0;
      // ---- local scans of this chunk: every device works through its shards on its own stream ------------
      for (int si = 0; si < P; ++si) {
        IxShard &s = ix->shards[si];
        IxDev &dv = ix->devs[s.dev];
        const int k_local = (int)std::min<int64_t>(k, s.n);
        if (k_local == 0) continue;
        RQ_HIP(hipSetDevice(dv.device));
        uint64_t *out = (remote(si) ? s.keys : ix->gathered + (size_t)si * cnt) + (size_t)q0 * k;   // root shards: in place
        uint64_t *dst = k_local < k ? s.tmp + (size_t)q0 * k_local : out;
        const float *qs = (R_host ? dv.queries_rot : dv.queries) + (size_t)q0 * d;
        RQ_TRY(scan_shard(s, dv, nullptr, nullptr, dst, qs, nqc, k_local, (uint32_t)(ix->id_offset + (uint64_t)s.row0), 0));
        if (k_local < k)
          RQ_HIP(hipMemcpy2DAsync(out, (size_t)k * 8, dst, (size_t)k_local * 8, (size_t)k_local * 8, (size_t)nqc,
                                  hipMemcpyDeviceToDevice, dv.stream));
      }
      for (auto &dv : ix->devs) {
        RQ_HIP(hipSetDevice(dv.device));
        RQ_HIP(hipEventRecord(dv.ev_scan[c], dv.stream));
      }
      // ---- the lists of the other devices travel to the root ---------------------------------------------
      RQ_HIP(hipSetDevice(root.device));
      RQ_HIP(hipStreamWaitEvent(root.mstream, root.ev_scan[c], 0));
      if (use_rccl) {
        bool any = false;
        for (size_t i = 0; i < ix->devs.size(); ++i) {
          IxDev &dv = ix->devs[i];
          RQ_HIP(hipSetDevice(dv.device));
          RQ_HIP(hipStreamWaitEvent(dv.xstream, dv.ev_scan[c], 0));
        }
        RQ_NCCL(g_rccl.GroupStart());
        for (int si = 0; si < P; ++si) {
          if (!remote(si)) continue;
          IxShard &s = ix->shards[si];
          IxDev &dv = ix->devs[s.dev];
          any = true;
          RQ_NCCL(g_rccl.Send(s.keys + (size_t)q0 * k, (size_t)nqc * k, ncclUint64, 0, ix->comms[s.dev], dv.xstream));
          RQ_NCCL(g_rccl.Recv(ix->gathered + (size_t)si * cnt + (size_t)q0 * k, (size_t)nqc * k, ncclUint64, s.dev,
                              ix->comms[0], root.xstream));
        }
        RQ_NCCL(g_rccl.GroupEnd());
        if (any) {
          RQ_HIP(hipSetDevice(root.device));
          RQ_HIP(hipEventRecord(root.ev_xfer[c], root.xstream));
          RQ_HIP(hipStreamWaitEvent(root.mstream, root.ev_xfer[c], 0));
        }
      } else {
        for (size_t i = 1; i < ix->devs.size(); ++i) {
          IxDev &dv = ix->devs[i];
          RQ_HIP(hipSetDevice(dv.device));
          RQ_HIP(hipStreamWaitEvent(dv.xstream, dv.ev_scan[c], 0));
          for (int si = 0; si < P; ++si) {
            IxShard &s = ix->shards[si];
            if (s.dev != (int)i) continue;
            RQ_HIP(hipMemcpyPeerAsync(ix->gathered + (size_t)si * cnt + (size_t)q0 * k, root.device,
                                      s.keys + (size_t)q0 * k, dv.device, (size_t)nqc * k * 8, dv.xstream));
          }
          RQ_HIP(hipEventRecord(dv.ev_xfer[c], dv.xstream));
          RQ_HIP(hipStreamWaitEvent(root.mstream, dv.ev_xfer[c], 0));
        }
      }
      // ---- merge of the chunk on the root ------------------------------------------------------------------
      RQ_HIP(hipSetDevice(root.device));
      uint64_t *inter = ix->inter + (size_t)q0 * P * k;
      RQ_TRY(interleave_keys_launch(inter, ix->gathered + (size_t)q0 * k, nqc, P, k, cnt, root.mstream));
      RQ_TRY(merge_launch(ix->dd + (size_t)q0 * k, ix->di + (size_t)q0 * k, nullptr, inter, nqc, P, k, id_base, root.mstream));
    }
  }
  for (size_t i = ix->devs.size(); i-- > 0;) {
    IxDev &dv = ix->devs[i];
    RQ_HIP(hipSetDevice(dv.device));
    RQ_HIP(hipStreamSynchronize(dv.stream));
    RQ_HIP(hipStreamSynchronize(dv.xstream));
    if (dv.mstream) RQ_HIP(hipStreamSynchronize(dv.mstream));
  }
  const double kernel_ms = t2.ms();
  Timer t3;
  RQ_HIP(hipSetDevice(root.device));
  RQ_HIP(hipMemcpy(dists, ix->dd, ob, hipMemcpyDeviceToHost));
  RQ_HIP(hipMemcpy(ids, ix->di, ob, hipMemcpyDeviceToHost));
  set_timing(tt.ms(), h2d_ms, kernel_ms, t3.ms());
  return RQ_OK;
}

// Device list of the host-pointer entry points: env RAYUELA_HIP_DEVICES = "0,1,2,3" | "all" (unset: the current
// device only).  A repeated ordinal is a logical shard.  Returns the number of entries written (0 = unset).
int env_devices(int *out, int cap) {
  const char *v = getenv("RAYUELA_HIP_DEVICES");
  if (!v || !*v) return 0;
  int n = 0;
  if (!strcmp(v, "all")) {
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess) { (void)hipGetLastError(); return 0; }
    for (int i = 0; i < visible && n < cap; ++i) out[n++] = i;
    return n;
  }
  const char *p = v;
  while (*p && n < cap) {
    char *end = nullptr;
    const long x = strtol(p, &end, 10);
    if (end == p) break;
    out[n++] = (int)x;
    p = end;
    while (*p == ',' || *p == ' ') ++p;
  }
  return n;
}

// linscan_pq / linscan_opq on host pointers over several devices (RAYUELA_HIP_DEVICES).  The sharded index behind these
// calls is KEPT between calls with the same device list, m and d: building one costs the RCCL communicator
// (ncclCommInitAll over the clique: hundreds of milliseconds), peer-access setup, streams and events -- a Julia session
// that calls linscan_pq in a loop would pay that every time.  Per call only the codebooks (128 KiB) and the code shards
// are uploaded again.  rq_release_workspaces() drops the cached index (its shards stay allocated until then).
static std::mutex g_shc_mu;
static rq_index *g_shc_ix = nullptr;
static std::vector<int> g_shc_devs;

void sharded_cache_release() {
  std::lock_guard<std::mutex> lk(g_shc_mu);
  if (g_shc_ix) index_free(g_shc_ix);
  g_shc_ix = nullptr;
  g_shc_devs.clear();
}

int host_linscan_sharded(float *dists, uint32_t *ids, const uint8_t *codes, const float *centers, const float *queries,
                         const float *R, int64_t n, int64_t nq, int m, int d, int k, int id_base, const int *devices,
                         int ndev) {
  std::lock_guard<std::mutex> lk(g_shc_mu);      // host-pointer calls over a device set run one at a time
  SavedDevice saved;
  const std::vector<int> devs(devices, devices + ndev);
  int rc = RQ_OK;
  if (g_shc_ix && (g_shc_devs != devs || g_shc_ix->m != m || g_shc_ix->d != d || !tuning("SHARDED_CACHE", 1))) {
    index_free(g_shc_ix);
    g_shc_ix = nullptr;
  }
  if (!g_shc_ix) {
    rq_index *ix = new rq_index();
    rc = index_build(ix, m, d, centers, devices, ndev);
    if (rc != RQ_OK) { index_free(ix); return rc; }
    g_shc_ix = ix;
    g_shc_devs = devs;
  } else {
    const size_t ce = (size_t)m * 256 * (d / m) * 4;      // same shape, new codebooks
    for (auto &dv : g_shc_ix->devs) {
      RQ_HIP(hipSetDevice(dv.device));
      RQ_HIP(hipMemcpy(dv.centers, centers, ce, hipMemcpyHostToDevice));
    }
  }
  rc = rq_index_set_codes(g_shc_ix, codes, n, 0);
  if (rc == RQ_OK) rc = index_search(g_shc_ix, dists, ids, queries, R, nq, k, id_base);
  if (rc != RQ_OK || !tuning("SHARDED_CACHE", 1)) {       // never keep an index that failed half-way
    index_free(g_shc_ix);
    g_shc_ix = nullptr;
    g_shc_devs.clear();
  }
  return rc;
}

}  // namespace rq

extern "C" {

rq_index *rq_index_create_sharded(int m, int d, const float *centers_host, const int *devices, int ndev) {
  if (!devices) { fail(RQ_EINVAL, "index: devices is NULL"); return nullptr; }
  rq_index *ix = new rq_index();
  SavedDevice saved;
  if (index_build(ix, m, d, centers_host, devices, ndev) != RQ_OK) { index_free(ix); return nullptr; }
  return ix;
}

rq_index *rq_index_create_sharded_wide(int m, int h, int d, const float *centers_host, const int *devices, int ndev) {
  if (!devices) { fail(RQ_EINVAL, "index: devices is NULL"); return nullptr; }
  rq_index *ix = new rq_index();
  SavedDevice saved;
  if (index_build(ix, m, d, centers_host, devices, ndev, h, true) != RQ_OK) { index_free(ix); return nullptr; }
  return ix;
}

rq_index *rq_index_create_wide(int m, int h, int d, const float *centers_host) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); fail(RQ_ENODEVICE, "no device"); return nullptr; }
  return rq_index_create_sharded_wide(m, h, d, centers_host, &dev, 1);
}

int rq_index_set_codes_wide(rq_index *ix, const int16_t *codes_host, int64_t n, int code_base, uint32_t id_offset) {
  return index_set_wide(ix, codes_host, n, code_base, id_offset);
}

// rq_index_create_aq[_wide]: devices == NULL with ndev == 0 is one shard on the calling thread's current device
static rq_index *index_create_aq(const char *who, int m, int h, int d, const float *codebooks_host, int lut_mode, const int *devices,
                                 int ndev, bool wide) {
  const int m_max = wide ? 32 : 64;
  if (m < 1 || m > m_max) { fail(RQ_EINVAL, "%s: 1 <= m <= %d; got m=%d", who, m_max, m); return nullptr; }
  if (h < 1 || h > RQ_MAX_H16) { fail(RQ_EINVAL, "%s: 1 <= h <= %d; got h=%d", who, RQ_MAX_H16, h); return nullptr; }
  if (d < 1) { fail(RQ_EINVAL, "%s: d=%d must be >= 1", who, d); return nullptr; }
  if (lut_mode != LUT_LSQ && lut_mode != LUT_CQ) { fail(RQ_EINVAL, "%s: lut_mode must be 1 (LSQ) or 2 (CQ); got %d", who, lut_mode); return nullptr; }
  if (!codebooks_host) { fail(RQ_EINVAL, "%s: codebooks is NULL", who); return nullptr; }
  if ((devices == nullptr) != (ndev == 0)) { fail(RQ_EINVAL, "%s: devices and ndev must be given together", who); return nullptr; }
  int dev = 0;
  if (!devices) {
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); fail(RQ_ENODEVICE, "no device"); return nullptr; }
    devices = &dev;
    ndev = 1;
  }
  rq_index *ix = new rq_index();
  SavedDevice saved;
  if (index_build(ix, m, d, codebooks_host, devices, ndev, h, wide, lut_mode) != RQ_OK) { index_free(ix); return nullptr; }
  return ix;
}

rq_index *rq_index_create_aq(int m, int d, const float *codebooks_host, int lut_mode, const int *devices, int ndev) {
  return index_create_aq("rq_index_create_aq", m, 256, d, codebooks_host, lut_mode, devices, ndev, false);
}

rq_index *rq_index_create_aq_wide(int m, int h, int d, const float *codebooks_host, int lut_mode, const int *devices, int ndev) {
  return index_create_aq("rq_index_create_aq_wide", m, h, d, codebooks_host, lut_mode, devices, ndev, true);
}

int rq_index_set_codes_aq(rq_index *ix, const uint8_t *codes_host, const float *dbnorms_host, const float *cbnorms_host, int hn,
                          int64_t n, uint32_t id_offset) {
  return index_set_aq(ix, codes_host, dbnorms_host, cbnorms_host, hn, n, id_offset);
}

int rq_index_set_codes_aq_wide(rq_index *ix, const int16_t *codes_host, const float *dbnorms_host, const float *cbnorms_host, int hn,
                               int64_t n, int code_base, uint32_t id_offset) {
  return index_set_wide(ix, codes_host, n, code_base, id_offset, true, dbnorms_host, cbnorms_host, hn);
}

int rq_index_aq_info(rq_index *ix, int64_t *out, int cap) {
  if (!ix || !out || cap < 4) return fail(RQ_EINVAL, "rq_index_aq_info: bad arguments");
  out[0] = ix->lut_mode;
  out[1] = ix->wide ? 1 : 0;
  out[2] = ix->h;
  out[3] = (int64_t)ix->shards.size();
  for (size_t s = 0; s < ix->shards.size() && 4 + 2 * (int)s + 1 < cap; ++s) {
    out[4 + 2 * s] = ix->shards[s].base.perm != nullptr;
    out[5 + 2 * s] = ix->shards[s].base.normb != nullptr;
  }
  return RQ_OK;
}

rq_index *rq_index_create(int m, int d, const float *centers_host) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); fail(RQ_ENODEVICE, "no device"); return nullptr; }
  return rq_index_create_sharded(m, d, centers_host, &dev, 1);
}

int rq_index_set_codes(rq_index *ix, const uint8_t *codes_host, int64_t n, uint32_t id_offset) {
  if (!codes_host) return fail(RQ_EINVAL, "index: codes is NULL");
  return index_set(ix, n, id_offset, [&](uint8_t *rows, int64_t row0, int64_t sn, hipStream_t stream) -> int {
    RQ_HIP(hipMemcpyAsync(rows, codes_host + (size_t)row0 * ix->m, (size_t)sn * ix->m, hipMemcpyHostToDevice, stream));
    return RQ_OK;
  });
}

int rq_index_set_codes_synth(rq_index *ix, int64_t n, uint64_t seed, uint32_t id_offset) {
  return index_set(ix, n, id_offset, [&](uint8_t *rows, int64_t row0, int64_t sn, hipStream_t stream) -> int {
    return synth_codes_launch(rows, sn, ix->m, seed, row0, stream);
  });
}

int rq_index_search(rq_index *ix, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, int k,
                    int id_base) {
  return index_search(ix, dists, ids, queries_host, nullptr, nq, k, id_base);
}

int rq_index_search_opq(rq_index *ix, float *dists, uint32_t *ids, const float *queries_host, const float *R_host,
                        int64_t nq, int k, int id_base) {
  if (!R_host) return fail(RQ_EINVAL, "R is NULL");
  return index_search(ix, dists, ids, queries_host, R_host, nq, k, id_base);
}

int rq_index_info(rq_index *ix, int64_t *out, int cap) {
  if (!ix || !out || cap < 4) return fail(RQ_EINVAL, "rq_index_info: bad arguments");
  out[0] = (int64_t)ix->shards.size();
  out[1] = (int64_t)ix->devs.size();
  out[2] = ix->exchange;
  out[3] = ix->n;
  for (size_t s = 0; s < ix->shards.size() && 4 + (int)s < cap; ++s) out[4 + s] = ix->shards[s].n;
  return RQ_OK;
}

void rq_index_destroy(rq_index *ix) { index_free(ix); }

}  // extern "C"
