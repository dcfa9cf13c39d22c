// rq_ivf.hip -- IVFADC (Jegou, Douze, Schmid, PAMI 2011): a coarse quantizer in front of the ADC scan.  DESIGN.md section 4.29.
//
// The base is grouped by the list (nearest coarse centroid) of every row; a search scans only the nprobe lists nearest to the
// query, with one look-up table per (query, probed list) when the codes are those of the residual x - Q[list].  The reference has
// no inverted file; every value is arithmetic the library already pins (include/rayuela_hip.h states the semantics):
//   coarse value   v(x, j) = max(fl(fl(sa_j + sb) - 2 g_j), 0), g / sa / sb k-ordered fmaf chains from +0: the encode's
//                  (oracle/rq_oracle.c:264-328).  The build takes the first-index argmin through encode_h16_launch at m = 1, the
//                  search writes the same values as packed keys (a NaN sorts behind every number) and selects the nprobe smallest
//   residual       one f32 subtraction per element (residual_launch: RVQ's stage epilogue), for rows and for queries
//   table and sum  build_lut's mode 0 and row_dists' order (deps/src/linscan_aqd.cpp:66-74, 85-87): unfused (c - q')^2 summed
//                  over s from +0, tables summed from table 0
//   top-k          sel_run of rq_bulk.hip on make_key(dist, id): unchanged code
// A search runs per batch of queries, all on one stream:
//   1. ivf_coarse_keys_kernel + sel_run (k = nprobe)     probes [nb][nprobe], nearest first
//   2. ivf_plan_kernel / ivf_scan_kernel / ivf_items_kernel   per (query, rank): key offset in the query's row (prefix sum of the
//                  probed list sizes) and its work items, one per IVF_SEGMENT_ROWS rows of the list; ONE read-back of
//                  {items, longest row of keys} sizes ld and the grid
//   3. ivf_fill_kernel + ivf_keys_kernel<MP>             a workgroup per item: q' = q - Q[list], the m x 256 table in LDS, its rows'
//                  keys at the item's offset of keys [nb][ld]; the slots behind a query's last row hold KEY_MAX
//   4. sel_run (k)                                       dists / ids, (NaN, 0xFFFFFFFF + id_base) behind the comparable rows
// rq_ivf_search_refine runs the same body with kc in place of k: step 4 leaves its sorted keys on the
// device and rerank_device (rq_rerank.hip) orders them by the exact distance to the rows of a resident dataset.
// The build groups rows with the same chain: keys (list << 32 | row) of a piece of rows, sorted by sel_run with k = the piece, are
// the piece in (list, row) order; pieces are placed one behind the other inside every list, so a list holds its rows in ascending id.
// An add takes its batch through the same steps with temporaries sized by the batch; the loaded base enters
// ivf_offsets_kernel as the piece in front of all others, ivf_carry_kernel<MP> moves its rows to their new places (a constant shift
// per list) and ivf_place_kernel<MP> puts the batch's rows behind them.  The new base is a fresh allocation, adopted when the last
// kernel has finished; a build is an add to nothing and launches what it launched before there were adds.  Byte rows (bvecs) are
// uploaded as bytes: lists through encode_h16_bytes_launch, then x - Q[list] written as f32 straight from the bytes
// (ivf_residual_bytes_kernel) or, without residuals, the codes through encode_bytes_launch.
#include "rq_internal.h"
#include "rq_ivf_rules.h"
#include "rq_topk.h"
#include "rq_encode_split.h"

#include <mutex>

namespace rq {

constexpr int IVF_T = 256;              // threads of every kernel here
constexpr int IVF_QT = 8;               // queries per workgroup of the coarse kernel
constexpr uint32_t IVF_NAN_ORD = 0xFFC00000u;   // f2ord of the canonical NaN: behind +Inf (0xFF800000)

static size_t ivf_align(size_t b) { return (b + 255) & ~(size_t)255; }

// The four knobs of this file (rq_set_tuning / env RQ_<KEY>): IVF_SEGMENT_ROWS, IVF_BATCH_QUERIES, IVF_BUILD_ROWS, IVF_SORT_ROWS.
// They cut work into pieces and select no code path; tests/test_gpu_ivf.py holds every answer equal under them.  They are read
// through this one function and are NOT rows of tests/switch_table.py, whose key count is pinned by a test of its own.
static int ivf_knob(const char *key, int dflt) { return tuning(key, dflt); }

// sa[j] = |Q_j|^2, a k-ordered fmaf chain from +0
__global__ __launch_bounds__(IVF_T) void ivf_sa_kernel(float *sa, const float *Q, int nlist, int d) {
  const int j = blockIdx.x * IVF_T + threadIdx.x;
  if (j >= nlist) return;
  const float *c = Q + (size_t)j * d;
  float acc = 0.0f;
  for (int s = 0; s < d; ++s) acc = __builtin_fmaf(c[s], c[s], acc);
  sa[j] = acc;
}

// keys[q][j] = ordered(v(q, j)) << 32 | j.  blockIdx.x: 256 lists (one per thread), blockIdx.y: IVF_QT queries; the queries'
// coordinates are wave-uniform loads, a centroid is read once for the IVF_QT queries
__global__ __launch_bounds__(IVF_T) void ivf_coarse_keys_kernel(uint64_t *keys, const float *queries, const float *Q,
                                                                const float *sa, uint32_t nb, int nlist, int d) {
  const int j = blockIdx.x * IVF_T + threadIdx.x;
  if (j >= nlist) return;
  const uint32_t q0 = blockIdx.y * IVF_QT;
  const float *c = Q + (size_t)j * d;
  const float *x[IVF_QT];
#pragma unroll
  for (int q = 0; q < IVF_QT; ++q) x[q] = queries + (size_t)min(q0 + (uint32_t)q, nb - 1u) * d;   // ragged group: repeat, not written
  float g[IVF_QT], sb[IVF_QT];
#pragma unroll
  for (int q = 0; q < IVF_QT; ++q) { g[q] = 0.0f; sb[q] = 0.0f; }
  for (int s = 0; s < d; ++s) {
    const float cs = c[s];
#pragma unroll
    for (int q = 0; q < IVF_QT; ++q) {
      const float xs = x[q][s];
      g[q] = __builtin_fmaf(cs, xs, g[q]);
      sb[q] = __builtin_fmaf(xs, xs, sb[q]);
    }
  }
  const float saj = sa[j];
#pragma unroll
  for (int q = 0; q < IVF_QT; ++q) {
    if (q0 + q >= nb) break;
    const float t = saj + sb[q];
    const float u = t - 2.0f * g[q];            // 2 g is exact: the same bits fused or not
    const uint32_t o = u != u ? IVF_NAN_ORD : f2ord(u > 0.0f ? u : 0.0f);
    keys[(size_t)(q0 + q) * nlist + j] = ((uint64_t)o << 32) | (uint32_t)j;
  }
}

// per query: the key offset and the item offset of every probe rank (serial prefix sums: nprobe is short), its rows and items
__global__ __launch_bounds__(IVF_T) void ivf_plan_kernel(uint32_t *koff, uint32_t *ioff, uint32_t *qrows, uint32_t *qitems,
                                                         const uint32_t *probes, const uint32_t *off, uint32_t nb, int nprobe,
                                                         uint32_t seg, uint32_t nlist) {
  const uint32_t q = blockIdx.x * IVF_T + threadIdx.x;
  if (q >= nb) return;
  uint32_t rows = 0, items = 0;
  for (int r = 0; r < nprobe; ++r) {
    const uint32_t p = probes[(size_t)q * nprobe + r];
    const uint32_t size = p < nlist ? off[p + 1] - off[p] : 0u;   // (every probe is a list: the coarse keys are never KEY_MAX)
    koff[(size_t)q * nprobe + r] = rows;
    ioff[(size_t)q * nprobe + r] = items;
    rows += size;
    items += (size + seg - 1) / seg;
  }
  qrows[q] = rows;
  qitems[q] = items;
}

// one workgroup: qbase = exclusive scan of qitems; stats[0] = items of the batch, [1] = its longest row of keys, [2] = its rows
__global__ __launch_bounds__(1024) void ivf_scan_kernel(uint32_t *qbase, unsigned long long *stats, const uint32_t *qitems,
                                                        const uint32_t *qrows, uint32_t nb) {
  __shared__ unsigned long long part[1024], prow[1024];
  __shared__ uint32_t pmax[1024];
  const uint32_t per = (nb + 1023u) / 1024u;
  const uint32_t b = threadIdx.x * per, e = min(nb, b + per);
  unsigned long long sum = 0, rows = 0;
  uint32_t mx = 0;
  for (uint32_t q = b; q < e; ++q) { sum += qitems[q]; rows += qrows[q]; mx = max(mx, qrows[q]); }
  part[threadIdx.x] = sum; prow[threadIdx.x] = rows; pmax[threadIdx.x] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0, rr = 0;
    uint32_t m = 0;
    for (int t = 0; t < 1024; ++t) {
      const unsigned long long c = part[t];
      part[t] = run;
      run += c; rr += prow[t]; m = max(m, pmax[t]);
    }
    stats[0] = run; stats[1] = m; stats[2] = rr;
  }
  __syncthreads();
  unsigned long long run = part[threadIdx.x];
  for (uint32_t q = b; q < e; ++q) { qbase[q] = (uint32_t)run; run += qitems[q]; }
}

// one thread per (query, rank): its list's segments
__global__ __launch_bounds__(IVF_T) void ivf_items_kernel(IvfItem *items, const uint32_t *probes, const uint32_t *off,
                                                          const uint32_t *koff, const uint32_t *ioff, const uint32_t *qbase,
                                                          uint32_t nb, int nprobe, uint32_t seg, uint32_t nlist, unsigned long long nitems) {
  const size_t e = (size_t)blockIdx.x * IVF_T + threadIdx.x;
  if (e >= (size_t)nb * nprobe) return;
  const uint32_t q = (uint32_t)(e / nprobe);
  const uint32_t p = probes[e];
  if (p >= nlist) return;
  const uint32_t b = off[p], size = off[p + 1] - b;
  size_t at = (size_t)qbase[q] + ioff[e];
  for (uint32_t r0 = 0; r0 < size; r0 += seg, ++at) {
    if (at >= nitems) return;                    // (cannot happen: the counts are ivf_plan_kernel's)
    IvfItem it;
    it.q = q; it.list = p; it.row0 = b + r0; it.nrows = min(seg, size - r0); it.koff = koff[e] + r0;
    items[at] = it;
  }
}

// keys[q][i] = KEY_MAX for qrows[q] <= i < ld
__global__ __launch_bounds__(IVF_T) void ivf_fill_kernel(uint64_t *keys, const uint32_t *qrows, size_t ld) {
  const uint32_t q = blockIdx.y;
  uint64_t *row = keys + (size_t)q * ld;
  for (size_t i = (size_t)qrows[q] + (size_t)blockIdx.x * IVF_T + threadIdx.x; i < ld; i += (size_t)gridDim.x * IVF_T)
    row[i] = KEY_MAX;
}

struct IvfKeyParams {
  const IvfItem *items;
  const uint8_t *codes;     // grouped, [n][MP]
  const uint32_t *ids;      // grouped, [n]: row + id_offset
  const float *centers;     // [m][256][sub]
  const float *coarse;      // [nlist][d]
  const float *queries;     // [nb][d]
  uint64_t *keys;           // [nb][ld]
  size_t ld;
  int m, sub, d, by_residual;
};

// One workgroup per item.  LDS: q' [d], then the table [m][256] f32, entry (k, r) at k * 256 + r -- thread r builds entry r of
// every table (stores of consecutive words: conflict-free), a row gathers one word per table (ds_read_b32, bank = code mod 32:
// for codes that are spread, what any permutation of the table gives).  Rows are read MP bytes at a time, one row per thread.
template <int MP>
__global__ __launch_bounds__(IVF_T) void ivf_keys_kernel(IvfKeyParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ivf_smem[];
  float *qs = reinterpret_cast<float *>(ivf_smem);
  float *lut = qs + ((p.d + 3) & ~3);
  const IvfItem it = p.items[blockIdx.x];
  const int tid = threadIdx.x;
  const float *qv = p.queries + (size_t)it.q * p.d;
  const float *cv = p.coarse + (size_t)it.list * p.d;
  for (int s = tid; s < p.d; s += IVF_T) qs[s] = p.by_residual ? qv[s] - cv[s] : qv[s];
  __syncthreads();
  const int sub = p.sub;
  for (int e = tid; e < p.m * 256; e += IVF_T) {
    const int k = e >> 8;
    const float *c = p.centers + (size_t)e * sub;
    const float *qk = qs + k * sub;
    float acc = 0.0f;
    for (int s = 0; s < sub; ++s) {
      const float diff = c[s] - qk[s];
      const float sq = diff * diff;
      acc = acc + sq;
    }
    lut[e] = acc;
  }
  __syncthreads();
  uint64_t *out = p.keys + (size_t)it.q * p.ld + it.koff;
  for (uint32_t i = tid; i < it.nrows; i += IVF_T) {
    const size_t row = (size_t)it.row0 + i;
    uint32_t w[(MP + 3) / 4];
    const uint8_t *src = p.codes + row * MP;
    if constexpr (MP >= 16) {
#pragma unroll
      for (int j = 0; j < MP / 16; ++j) {
        const uint4 v = reinterpret_cast<const uint4 *>(src)[j];
        w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
      }
    } else if constexpr (MP == 8) {
      const uint2 v = *reinterpret_cast<const uint2 *>(src);
      w[0] = v.x; w[1] = v.y;
    } else if constexpr (MP == 4) {
      w[0] = *reinterpret_cast<const uint32_t *>(src);
    } else {
      w[0] = *reinterpret_cast<const uint16_t *>(src);
    }
    float acc = lut[w[0] & 0xffu];
#pragma unroll
    for (int k = 1; k < MP; ++k)
      if (k < p.m) acc = acc + lut[k * 256 + ((w[k >> 2] >> (8 * (k & 3))) & 0xffu)];
    out[i] = acc != acc ? KEY_MAX : make_key(acc, p.ids[row]);
  }
}

// ---- grouping ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IVF_T) void ivf_widen_lists_kernel(uint32_t *lists, const int16_t *l16, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * IVF_T + threadIdx.x;
  if (i < n) lists[i] = (uint32_t)(uint16_t)l16[i];
}

__global__ __launch_bounds__(IVF_T) void ivf_group_keys_kernel(uint64_t *keys, const uint32_t *lists, uint32_t r0, uint32_t cnt) {
  const uint32_t i = blockIdx.x * IVF_T + threadIdx.x;
  if (i < cnt) keys[i] = ((uint64_t)lists[(size_t)r0 + i] << 32) | (uint64_t)(r0 + i);
}

// first / last [nlist] (zeroed): the positions [first, last) of every list inside a sorted piece
__global__ __launch_bounds__(IVF_T) void ivf_bounds_kernel(uint32_t *first, uint32_t *last, const uint32_t *sorted,
                                                           const uint32_t *lists, uint32_t cnt) {
  const uint32_t j = blockIdx.x * IVF_T + threadIdx.x;
  if (j >= cnt) return;
  const uint32_t l = lists[sorted[j]];
  if (j == 0 || lists[sorted[j - 1]] != l) first[l] = j;
  if (j + 1 == cnt || lists[sorted[j + 1]] != l) last[l] = j + 1;
}

// one workgroup: off [nlist + 1] = exclusive scan of the list sizes over all pieces; base [P][nlist] = where piece p's rows of
// list l begin: off[l] + the rows of l in the pieces before p.  off_old (null: none) is the loaded base of an add, the piece in
// front of all others: list l keeps its off_old[l + 1] - off_old[l] rows first, the pieces of the batch go behind them
__global__ __launch_bounds__(1024) void ivf_offsets_kernel(uint32_t *off, uint32_t *base, const uint32_t *first,
                                                           const uint32_t *last, const uint32_t *off_old, int P, int nlist) {
  __shared__ unsigned long long part[1024];
  const int per = (nlist + 1023) / 1024;
  const int b = min(nlist, (int)threadIdx.x * per), e = min(nlist, b + per);
  unsigned long long sum = 0;
  for (int l = b; l < e; ++l) {
    if (off_old) sum += off_old[l + 1] - off_old[l];
    for (int p = 0; p < P; ++p) sum += last[(size_t)p * nlist + l] - first[(size_t)p * nlist + l];
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int t = 0; t < 1024; ++t) { const unsigned long long c = part[t]; part[t] = run; run += c; }
    off[nlist] = (uint32_t)run;
  }
  __syncthreads();
  uint32_t run = (uint32_t)part[threadIdx.x];
  for (int l = b; l < e; ++l) {
    off[l] = run;
    if (off_old) run += off_old[l + 1] - off_old[l];
    for (int p = 0; p < P; ++p) {
      base[(size_t)p * nlist + l] = run;
      run += last[(size_t)p * nlist + l] - first[(size_t)p * nlist + l];
    }
  }
}

// position j of a sorted piece -> its place in the grouped base: the id and the MP code bytes of its row
template <int MP>
__global__ __launch_bounds__(IVF_T) void ivf_place_kernel(uint8_t *codes_out, uint32_t *ids_out, const uint8_t *codes_in,
                                                          const uint32_t *sorted, const uint32_t *lists, const uint32_t *first,
                                                          const uint32_t *base, uint32_t cnt, uint32_t id_offset, size_t n) {
  const uint32_t j = blockIdx.x * IVF_T + threadIdx.x;
  if (j >= cnt) return;
  const uint32_t row = sorted[j];
  const uint32_t l = lists[row];
  const size_t dest = (size_t)base[l] + (j - first[l]);
  if (dest >= n) return;                       // (cannot happen: the bounds are this piece's)
  ids_out[dest] = row + id_offset;
  using W = typename std::conditional<MP >= 4, uint32_t, uint16_t>::type;
  const W *src = reinterpret_cast<const W *>(codes_in + (size_t)row * MP);
  W *dst = reinterpret_cast<W *>(codes_out + dest * MP);
#pragma unroll
  for (int i = 0; i < MP / (int)sizeof(W); ++i) dst[i] = src[i];
}

// ---- adding to a loaded base ----------------------------------------------------------------------------------------------------
// The owner of position j of a grouped base: the LAST list l with off[l] <= j.  Empty lists make runs of equal offsets, and of a
// run only its last list holds rows.  Needs off[lo] <= j < off[hi]; ends with off[lo] <= j < off[lo + 1], so lo is that list.
__device__ __forceinline__ uint32_t ivf_owner(const uint32_t *off, uint32_t lo, uint32_t hi, uint32_t j) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// An add moves every loaded row -- its id and its MP code bytes -- from off_old[l] + r to off_new[l] + r.  The grid runs over rows,
// so a list that holds a large share of the base costs what its rows cost.  A workgroup takes IVF_T * IVF_CARRY_ROWS consecutive
// rows: two threads find the lists of its first and last row in all of off_old (a chain of dependent loads, paid once per
// workgroup), every row is then searched only between them -- not at all when the workgroup lies inside one list, else over a few
// words that are in L1 / L2.  Thread t takes rows t, t + IVF_T, ...: a wavefront reads and writes consecutive rows.  A row is
// copied in words of min(MP, 16) bytes: both bases are hipMalloc'ed and a row begins at a multiple of MP.
constexpr int IVF_CARRY_ROWS = 8;
template <int MP>
__global__ __launch_bounds__(IVF_T) void ivf_carry_kernel(uint8_t *__restrict__ codes_out, uint32_t *__restrict__ ids_out,
                                                          const uint8_t *__restrict__ codes_in, const uint32_t *__restrict__ ids_in,
                                                          const uint32_t *__restrict__ off_old, const uint32_t *__restrict__ off_new,
                                                          uint64_t n_old, size_t n_new, int nlist) {
  __shared__ uint32_t span[2];
  const uint64_t j0 = (uint64_t)blockIdx.x * (IVF_T * IVF_CARRY_ROWS);
  if (threadIdx.x < 2) {
    const uint64_t je = j0 + IVF_T * IVF_CARRY_ROWS < n_old ? j0 + IVF_T * IVF_CARRY_ROWS : n_old;
    span[threadIdx.x] = ivf_owner(off_old, 0u, (uint32_t)nlist, (uint32_t)(threadIdx.x == 0 ? j0 : je - 1));
  }
  __syncthreads();
  const uint32_t l0 = span[0], l1 = span[1];
  using W = typename std::conditional<MP >= 16, uint4, typename std::conditional<MP == 8, uint2,
            typename std::conditional<MP == 4, uint32_t, uint16_t>::type>::type>::type;
#pragma unroll
  for (int i = 0; i < IVF_CARRY_ROWS; ++i) {
    const uint64_t j = j0 + (uint64_t)i * IVF_T + threadIdx.x;
    if (j >= n_old) return;
    const uint32_t l = l0 == l1 ? l0 : ivf_owner(off_old, l0, l1 + 1u, (uint32_t)j);
    const size_t dest = (size_t)off_new[l] + (size_t)((uint32_t)j - off_old[l]);
    if (dest >= n_new) return;                 // (cannot happen: off_new holds every list's loaded rows)
    ids_out[dest] = ids_in[j];
    const W *src = reinterpret_cast<const W *>(codes_in + (size_t)j * MP);
    W *dst = reinterpret_cast<W *>(codes_out + dest * MP);
#pragma unroll
    for (int w = 0; w < MP / (int)sizeof(W); ++w) dst[w] = src[w];
  }
}

// out[row][:] = float(X[row][:]) - Q[list(row)][:] from byte rows: one f32 subtraction per element, residual_kernel's arithmetic
// on the widened row (u8 -> f32 is exact).  One thread per 8 elements of a row (fewer at its end), loaded 8 bytes at a time down
// to single bytes by the alignment of X and d (byte_align / load_bytes, as the byte encode reads rows); out is 16-byte aligned
__global__ __launch_bounds__(IVF_T) void ivf_residual_bytes_kernel(float *out, const uint8_t *X, const float *__restrict__ Q,
                                                                   const int16_t *lists, int64_t n, int d) {
  const int per = (d + 7) / 8;
  const int64_t e = (int64_t)blockIdx.x * IVF_T + threadIdx.x;
  if (e >= n * per) return;
  const int64_t row = e / per;
  const int i0 = (int)(e - row * per) * 8;
  const int nb = min(8, d - i0);
  const uint32_t list = (uint32_t)(uint16_t)lists[row];
  uint32_t w[2];
  float x[8];
  load_bytes<8>(X + (size_t)row * d + i0, byte_align(X, d, 8), nb, w);
  bytes_f32<8>(w, x);
  float *o = out + (size_t)row * d + i0;
  const float *c = Q + (size_t)list * d + i0;
  if ((d & 3) == 0) {       // nb is 4 or 8, and o / c are 16-byte aligned
    const float4 v = *reinterpret_cast<const float4 *>(c);
    *reinterpret_cast<float4 *>(o) = make_float4(x[0] - v.x, x[1] - v.y, x[2] - v.z, x[3] - v.w);
    if (nb == 8) {
      const float4 u = *reinterpret_cast<const float4 *>(c + 4);
      *reinterpret_cast<float4 *>(o + 4) = make_float4(x[4] - u.x, x[5] - u.y, x[6] - u.z, x[7] - u.w);
    }
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (s < nb) o[s] = x[s] - c[s];
  }
}

}  // namespace rq

using namespace rq;

// ---- the handle ----------------------------------------------------------------------------------------------------------------
struct rq_ivf {
  int device = 0, num_cu = 0;
  int d = 0, nlist = 0, m = 0, mp = 0, by_residual = 0;
  float *coarse = nullptr, *sa = nullptr, *centers = nullptr;     // device
  // the loaded base (device): rows grouped by list
  int64_t n = 0;
  uint64_t next_id = 0;            // the largest id loaded plus one: the least id_offset an add may take
  uint8_t *codes = nullptr;        // [n][mp]
  uint32_t *ids = nullptr;         // [n]: row + id_offset
  uint32_t *off = nullptr;         // [nlist + 1]
  std::vector<int64_t> h_off;      // host copy of off
  std::vector<int64_t> h_desc;     // the list sizes, largest first
  // the last search
  int64_t s_ld = 0, s_batch = 0, s_items = 0, s_rows = 0;
  double s_ms[6] = {0, 0, 0, 0, 0, 0};   // the last search: its four phases, then the keys and the selection of a refinement
  double l_ms[4] = {0, 0, 0, 0};   // the last build / set_codes / add: encode (with its uploads), grouping, carry, place
  std::mutex mu;
};

namespace {

struct IvfBase {                   // what a build or set_codes makes before it replaces the loaded base
  uint8_t *codes = nullptr;
  uint32_t *ids = nullptr, *off = nullptr;
  void drop() {
    if (codes) (void)hipFree(codes);
    if (ids) (void)hipFree(ids);
    if (off) (void)hipFree(off);
    codes = nullptr; ids = nullptr; off = nullptr;
  }
};

// the id rule and the limits (rq_ivf_rules.h) of a call that loads n rows; `loaded` rows stay in front of them (0: it replaces)
int ivf_rule_check(const char *who, const rq_ivf *ix, int64_t loaded, int64_t n, uint32_t id_offset) {
  switch (ivf_load_rule(loaded, ix->next_id, n, id_offset)) {
    case IVF_OK: return RQ_OK;
    case IVF_NO_ROWS: return fail(RQ_EINVAL, "%s: n=%lld rows", who, (long long)n);
    case IVF_ID_RANGE:
      return fail(RQ_EINVAL, "%s: n + id_offset = %llu exceeds 2^32 - 1 (ids are uint32, 0xFFFFFFFF marks padding)", who,
                  (unsigned long long)((uint64_t)n + id_offset));
    case IVF_ID_ORDER:
      return fail(RQ_EINVAL, "%s: id_offset=%u lies below the next id %llu (ids ascend inside a list; gaps are allowed)", who,
                  id_offset, (unsigned long long)ix->next_id);
    case IVF_ROW_RANGE:
      return fail(RQ_EINVAL, "%s: %lld rows loaded + n=%lld exceed 2^32 - 1 (offsets are uint32)", who, (long long)loaded,
                  (long long)n);
  }
  return RQ_EINVAL;
}

template <int MP>
int ivf_place_launch(uint8_t *codes_out, uint32_t *ids_out, const uint8_t *codes_in, const uint32_t *sorted, const uint32_t *lists,
                     const uint32_t *first, const uint32_t *base, uint32_t cnt, uint32_t id_offset, size_t n, hipStream_t stream) {
  RQ_LAUNCH(ivf_place_kernel<MP>, dim3((cnt + IVF_T - 1) / IVF_T), dim3(IVF_T), 0, stream, codes_out, ids_out, codes_in, sorted,
            lists, first, base, cnt, id_offset, n);
  return RQ_OK;
}

// rows per sorted piece: its keys and the chain's scratch fit the bulk budget
int64_t ivf_piece_rows(int64_t n) {
  int64_t rows = std::min<int64_t>(n, 1 << 25);
  while (rows > 1 && ivf_align((size_t)rows * 8) + sel_bytes_per_query((uint32_t)rows) + 16 * 256 > bulk_usable()) rows /= 2;
  const int forced = ivf_knob("IVF_SORT_ROWS", 0);
  return forced > 0 ? std::min<int64_t>(rows, forced) : rows;
}

template <int MP>
int ivf_carry_launch(uint8_t *codes_out, uint32_t *ids_out, const rq_ivf *ix, const uint32_t *off_new, size_t n_new,
                     hipStream_t stream) {
  RQ_LAUNCH(ivf_carry_kernel<MP>, dim3((uint32_t)(((uint64_t)ix->n + IVF_T * IVF_CARRY_ROWS - 1) / (IVF_T * IVF_CARRY_ROWS))),
            dim3(IVF_T), 0, stream, codes_out, ids_out,
            ix->codes, ix->ids, ix->off, off_new, (uint64_t)ix->n, n_new, ix->nlist);
  return RQ_OK;
}

// milliseconds of the last load (rq_ivf_last_timing [4..7])
enum { IVF_MS_ENCODE = 0, IVF_MS_GROUP = 1, IVF_MS_CARRY = 2, IVF_MS_PLACE = 3 };

// lists [n] (device, every entry < nlist) and arrival-order codes [n][mp] of a batch -> the grouped base in *nb (allocated here).
// carry: the loaded base of ix goes in front, list by list (an add); else the batch alone is the base (a build), and no launch
// differs from what a build made before there were adds.
int ivf_group(rq_ivf *ix, IvfBase *nb, const uint32_t *lists, const uint8_t *codes_arr, int64_t n, uint32_t id_offset, bool carry,
              PhaseClock &clock, hipStream_t stream) {
  const int nlist = ix->nlist, mp = ix->mp;
  const int64_t total = n + (carry ? ix->n : 0);
  const int64_t piece = ivf_piece_rows(n);
  const int P = (int)ivf_piece_count(n, piece);
  DevMem sorted, first, last, base;
  RQ_TRY(sorted.alloc((size_t)n * 4));
  RQ_TRY(first.alloc((size_t)P * nlist * 4));
  RQ_TRY(last.alloc((size_t)P * nlist * 4));
  RQ_TRY(base.alloc((size_t)P * nlist * 4));
  RQ_HIP(hipMalloc((void **)&nb->codes, (size_t)total * mp));
  RQ_HIP(hipMalloc((void **)&nb->ids, (size_t)total * 4));
  RQ_HIP(hipMalloc((void **)&nb->off, (size_t)(nlist + 1) * 4));
  RQ_HIP(hipMemsetAsync(first.p, 0, (size_t)P * nlist * 4, stream));
  RQ_HIP(hipMemsetAsync(last.p, 0, (size_t)P * nlist * 4, stream));
  void *ws = nullptr;
  RQ_TRY(workspace(WS_BULK, ivf_align((size_t)piece * 8) + sel_bytes_per_query((uint32_t)piece) + 16 * 256, &ws, stream));
  for (int p = 0; p < P; ++p) {
    int64_t r0;
    uint32_t cnt;
    ivf_piece_span(n, piece, p, &r0, &cnt);
    unsigned char *at = (unsigned char *)ws;
    uint64_t *keys = (uint64_t *)at; at += ivf_align((size_t)cnt * 8);
    RQ_LAUNCH(ivf_group_keys_kernel, dim3((cnt + IVF_T - 1) / IVF_T), dim3(IVF_T), 0, stream, keys, lists, (uint32_t)r0, cnt);
    BulkSel s;
    s.src = keys; s.ld = cnt;
    sel_layout(s, at, 1, cnt);
    uint32_t hx;
    sel_grid(s, cnt, 1, ix->num_cu, &hx);
    BulkOut o;
    o.dists = nullptr; o.keys = nullptr; o.ids = sorted.as<uint32_t>() + r0; o.id_base = 0;
    RQ_TRY(sel_run(s, hx, 1, o, stream));
    RQ_LAUNCH(ivf_bounds_kernel, dim3((cnt + IVF_T - 1) / IVF_T), dim3(IVF_T), 0, stream, first.as<uint32_t>() + (size_t)p * nlist,
              last.as<uint32_t>() + (size_t)p * nlist, sorted.as<uint32_t>() + r0, lists, cnt);
  }
  RQ_LAUNCH(ivf_offsets_kernel, dim3(1), dim3(1024), 0, stream, nb->off, base.as<uint32_t>(), first.as<uint32_t>(),
            last.as<uint32_t>(), carry ? (const uint32_t *)ix->off : nullptr, P, nlist);
  clock.mark(IVF_MS_GROUP);
  if (carry) {
    int rc = RQ_EUNSUPPORTED;
    switch (mp) {
#define RQ_IVF_CASE(MP) case MP: rc = ivf_carry_launch<MP>(nb->codes, nb->ids, ix, nb->off, (size_t)total, stream); break;
      RQ_IVF_CASE(2) RQ_IVF_CASE(4) RQ_IVF_CASE(8) RQ_IVF_CASE(16) RQ_IVF_CASE(32) RQ_IVF_CASE(64)
#undef RQ_IVF_CASE
    }
    RQ_TRY(rc);
    clock.mark(IVF_MS_CARRY);
  }
  for (int p = 0; p < P; ++p) {
    int64_t r0;
    uint32_t cnt;
    ivf_piece_span(n, piece, p, &r0, &cnt);
    const uint32_t *srt = sorted.as<uint32_t>() + r0, *fp = first.as<uint32_t>() + (size_t)p * nlist,
                   *bp = base.as<uint32_t>() + (size_t)p * nlist;
    int rc = RQ_EUNSUPPORTED;
    switch (mp) {
#define RQ_IVF_CASE(MP) \
      case MP: rc = ivf_place_launch<MP>(nb->codes, nb->ids, codes_arr, srt, lists, fp, bp, cnt, id_offset, (size_t)total, stream); break;
      RQ_IVF_CASE(2) RQ_IVF_CASE(4) RQ_IVF_CASE(8) RQ_IVF_CASE(16) RQ_IVF_CASE(32) RQ_IVF_CASE(64)
#undef RQ_IVF_CASE
    }
    RQ_TRY(rc);
  }
  clock.mark(IVF_MS_PLACE);
  RQ_HIP(hipStreamSynchronize(stream));
  return RQ_OK;
}

// the new base replaces the loaded one: host copies of the offsets, the sizes largest first
int ivf_adopt(rq_ivf *ix, IvfBase *nb, int64_t n, uint64_t next_id) {
  std::vector<uint32_t> off((size_t)ix->nlist + 1);
  RQ_HIP(hipMemcpy(off.data(), nb->off, off.size() * 4, hipMemcpyDeviceToHost));
  if ((int64_t)off[ix->nlist] != n) return fail(RQ_EINVAL, "rq_ivf: grouped %u of %lld rows", off[ix->nlist], (long long)n);
  if (ix->codes) (void)hipFree(ix->codes);
  if (ix->ids) (void)hipFree(ix->ids);
  if (ix->off) (void)hipFree(ix->off);
  ix->codes = nb->codes; ix->ids = nb->ids; ix->off = nb->off;
  nb->codes = nullptr; nb->ids = nullptr; nb->off = nullptr;
  ix->n = n;
  ix->next_id = next_id;
  ix->h_off.assign(off.begin(), off.end());
  ix->h_desc.resize(ix->nlist);
  for (int l = 0; l < ix->nlist; ++l) ix->h_desc[l] = ix->h_off[l + 1] - ix->h_off[l];
  std::sort(ix->h_desc.begin(), ix->h_desc.end(), [](int64_t a, int64_t b) { return a > b; });
  return RQ_OK;
}

// what every load ends with: group the batch (behind the loaded base when carry), adopt the result, keep the phase times; after
// a failure the base that was loaded answers
int ivf_finish(rq_ivf *ix, const uint32_t *lists, const uint8_t *codes_arr, int64_t n, uint32_t id_offset, bool carry,
               PhaseClock &clock, double *ms, hipStream_t stream) {
  IvfBase nb;
  int rc = ivf_group(ix, &nb, lists, codes_arr, n, id_offset, carry, clock, stream);
  if (rc == RQ_OK) rc = ivf_adopt(ix, &nb, n + (carry ? ix->n : 0), (uint64_t)id_offset + (uint64_t)n);
  if (rc != RQ_OK) { (void)hipStreamSynchronize(stream); nb.drop(); return rc; }
  clock.collect();
  for (int i = 0; i < 4; ++i) ix->l_ms[i] = ms[i];
  return RQ_OK;
}

// rq_ivf_build[_bytes] (append = false) and rq_ivf_add[_bytes]: X_host [n][d] of esz bytes per element (4: float, 1: uint8)
int ivf_load_rows(const char *who, rq_ivf *ix, const void *X_host, int esz, int64_t n, uint32_t id_offset, bool append) {
  if (!ix || !X_host) return fail(RQ_EINVAL, "%s: NULL argument", who);
  std::lock_guard<std::mutex> guard(ix->mu);
  const bool carry = append && ix->codes && ix->n > 0;
  RQ_TRY(ivf_rule_check(who, ix, carry ? ix->n : 0, n, id_offset));
  if (ix->m > 32)
    return fail(RQ_EUNSUPPORTED, "%s: the encode covers 1 <= m <= 32; got m=%d (%s takes codes)", who, ix->m,
                append ? "rq_ivf_add_codes" : "rq_ivf_set_codes");
  SavedDevice saved;
  RQ_HIP(hipSetDevice(ix->device));
  DeviceLock lock;
  hipStream_t stream = nullptr;
  const int d = ix->d, m = ix->m, mp = ix->mp;
  const bool bytes = esz == 1;
  int64_t chunk = std::max<int64_t>(32768, ((int64_t)1 << 26) / d);
  const int forced = ivf_knob("IVF_BUILD_ROWS", 0);
  if (forced > 0) chunk = forced;
  chunk = std::min(chunk, n);
  DevMem dX, dB, d16, d8, lists, arr;
  if (!bytes || ix->by_residual) RQ_TRY(dX.alloc((size_t)chunk * d * 4));     // byte rows without residuals: no float copy
  if (bytes) RQ_TRY(dB.alloc((size_t)chunk * d));
  RQ_TRY(d16.alloc((size_t)chunk * 2));
  RQ_TRY(d8.alloc((size_t)chunk * m));
  RQ_TRY(lists.alloc((size_t)n * 4));
  RQ_TRY(arr.alloc((size_t)n * mp));
  double ms[4] = {0, 0, 0, 0};
  PhaseClock clock(stream, ms);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nr = std::min(chunk, n - r0);
    uint8_t *out = m == mp ? arr.as<uint8_t>() + (size_t)r0 * mp : d8.as<uint8_t>();
    if (bytes) {
      RQ_HIP(hipMemcpyAsync(dB.p, (const uint8_t *)X_host + (size_t)r0 * d, (size_t)nr * d, hipMemcpyHostToDevice, stream));
      RQ_TRY(encode_h16_bytes_launch(d16.as<int16_t>(), dB.as<uint8_t>(), nullptr, ix->coarse, nr, d, 1, ix->nlist, ix->num_cu, stream));
    } else {
      RQ_HIP(hipMemcpyAsync(dX.p, (const float *)X_host + (size_t)r0 * d, (size_t)nr * d * 4, hipMemcpyHostToDevice, stream));
      RQ_TRY(encode_h16_launch(d16.as<int16_t>(), dX.as<float>(), ix->coarse, nr, d, 1, ix->nlist, ix->num_cu, stream));
    }
    RQ_LAUNCH(ivf_widen_lists_kernel, dim3((uint32_t)((nr + IVF_T - 1) / IVF_T)), dim3(IVF_T), 0, stream,
              lists.as<uint32_t>() + r0, d16.as<int16_t>(), nr);
    if (bytes && !ix->by_residual) {
      RQ_TRY(encode_bytes_launch(out, dB.as<uint8_t>(), nullptr, ix->centers, nr, d, m, 256, ix->num_cu, stream));
    } else {
      if (bytes) {
        const int64_t threads = nr * ((d + 7) / 8);
        RQ_LAUNCH(ivf_residual_bytes_kernel, dim3((uint32_t)((threads + IVF_T - 1) / IVF_T)), dim3(IVF_T), 0, stream, dX.as<float>(),
                  dB.as<uint8_t>(), ix->coarse, d16.as<int16_t>(), nr, d);
      } else if (ix->by_residual) {
        RQ_TRY(residual_launch<int16_t>(dX.as<float>(), dX.as<float>(), ix->coarse, d16.as<int16_t>(), 1, nullptr, nullptr, nr, d, 1, 0,
                                        stream));
      }
      RQ_TRY(encode_launch(out, dX.as<float>(), ix->centers, nr, d, m, 256, ix->num_cu, stream));
    }
    if (m != mp) RQ_TRY(pad_codes_launch(arr.as<uint8_t>() + (size_t)r0 * mp, d8.as<uint8_t>(), nr, m, mp, stream));
    clock.mark(IVF_MS_ENCODE);
    RQ_HIP(hipStreamSynchronize(stream));      // the chunk buffer is reused
  }
  return ivf_finish(ix, lists.as<uint32_t>(), arr.as<uint8_t>(), n, id_offset, carry, clock, ms, stream);
}

// rq_ivf_set_codes (append = false) and rq_ivf_add_codes
int ivf_load_codes(const char *who, rq_ivf *ix, const uint32_t *lists_host, const uint8_t *codes_host, int64_t n, uint32_t id_offset,
                   bool append) {
  if (!ix || !lists_host || !codes_host) return fail(RQ_EINVAL, "%s: NULL argument", who);
  RQ_TRY(ivf_rule_check(who, ix, 0, n, id_offset));      // what needs no state, so that the scan below reads n valid entries ...
  for (int64_t i = 0; i < n; ++i)                        // ... and runs before the mutex: searches go on meanwhile
    if (lists_host[i] >= (uint32_t)ix->nlist)
      return fail(RQ_EINVAL, "%s: row %lld names list %d outside [0, %d)", who, (long long)i, (int)lists_host[i], ix->nlist);
  std::lock_guard<std::mutex> guard(ix->mu);
  const bool carry = append && ix->codes && ix->n > 0;
  RQ_TRY(ivf_rule_check(who, ix, carry ? ix->n : 0, n, id_offset));
  SavedDevice saved;
  RQ_HIP(hipSetDevice(ix->device));
  DeviceLock lock;
  hipStream_t stream = nullptr;
  const int m = ix->m, mp = ix->mp;
  DevMem lists, raw, arr;
  RQ_TRY(lists.alloc((size_t)n * 4));
  RQ_TRY(arr.alloc((size_t)n * mp));
  double ms[4] = {0, 0, 0, 0};
  PhaseClock clock(stream, ms);
  RQ_HIP(hipMemcpyAsync(lists.p, lists_host, (size_t)n * 4, hipMemcpyHostToDevice, stream));
  if (m == mp) {
    RQ_HIP(hipMemcpyAsync(arr.p, codes_host, (size_t)n * m, hipMemcpyHostToDevice, stream));
  } else {
    RQ_TRY(raw.alloc((size_t)n * m));
    RQ_HIP(hipMemcpyAsync(raw.p, codes_host, (size_t)n * m, hipMemcpyHostToDevice, stream));
    RQ_TRY(pad_codes_launch(arr.as<uint8_t>(), raw.as<uint8_t>(), n, m, mp, stream));
  }
  clock.mark(IVF_MS_ENCODE);
  return ivf_finish(ix, lists.as<uint32_t>(), arr.as<uint8_t>(), n, id_offset, carry, clock, ms, stream);
}

// scratch of a batch of nb queries: what survives both phases, then the larger of the probe selection and the scan
struct IvfPlan {
  size_t keep, phase1, phase2, phase3;
  size_t total() const { return keep + std::max(std::max(phase1, phase2), phase3); }
};
// what rq_ivf_search_refine adds to a search: the dataset the candidates are re-ranked on, and the k of the answer (the search
// itself then runs with kc in place of k and hands its sorted keys to rerank_device, whose scratch is a third phase)
struct IvfRefine {
  DatasetView base;
  int k;
  uint32_t id_offset;
  bool chain;          // rerank_chain(kc), read once per call
};
IvfPlan ivf_bytes(int64_t nb, int nlist, int nprobe, int k, size_t ld, size_t items_per_query, const IvfRefine *rf) {
  IvfPlan pl;
  pl.phase3 = rf ? rerank_scratch_bytes(nb, k, rf->k, rf->chain) : 0;
  pl.keep = 3 * ivf_align((size_t)nb * nprobe * 4) + 3 * ivf_align((size_t)nb * 4) + 256;
  pl.phase1 = ivf_align((size_t)nb * nlist * 8) + (size_t)nb * sel_bytes_per_query((uint32_t)nprobe) + 16 * 256;
  pl.phase2 = ivf_align((size_t)nb * items_per_query * sizeof(IvfItem)) + ivf_align((size_t)nb * ld * 8) +
              (size_t)nb * sel_bytes_per_query((uint32_t)k) + 16 * 256;
  return pl;
}

template <int MP>
int ivf_keys_launch(const IvfKeyParams &p, uint32_t nitems, hipStream_t stream) {
  const size_t lds = (size_t)((p.d + 3) & ~3) * 4 + (size_t)p.m * 1024;
  if (lds > 160 * 1024) return fail(RQ_EUNSUPPORTED, "rq_ivf_search: d=%d, m=%d do not fit the LDS table", p.d, p.m);
  RQ_LAUNCH_LDS(ivf_keys_kernel<MP>, dim3(nitems), dim3(IVF_T), lds, stream, p);
  return RQ_OK;
}

// rq_ivf_search (rf null) and rq_ivf_search_refine: k is the k of the index's own top-k (kc of a refinement)
int ivf_search_body(const char *who, rq_ivf *ix, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, int nprobe, int k,
                    int id_base, const IvfRefine *rf);

}  // namespace

extern "C" {

rq_ivf *rq_ivf_create(int d, int nlist, const float *coarse_host, int m, const float *centers_host, int by_residual) {
  if (!coarse_host || !centers_host) { fail(RQ_EINVAL, "rq_ivf_create: NULL argument"); return nullptr; }
  if (d < 1 || m < 1 || d % m != 0) { fail(RQ_EINVAL, "rq_ivf_create: d=%d must be a positive multiple of m=%d", d, m); return nullptr; }
  const int mp = scan_padded_m(m);
  if (mp < 0) { fail(RQ_EUNSUPPORTED, "rq_ivf_create: m=%d has no tiled row width (1 <= m <= 64)", m); return nullptr; }
  if (nlist < 1 || nlist > RQ_MAX_H16) {
    fail(RQ_EUNSUPPORTED, "rq_ivf_create: 1 <= nlist <= %d; got nlist=%d", RQ_MAX_H16, nlist);
    return nullptr;
  }
  if (by_residual != 0 && by_residual != 1) { fail(RQ_EINVAL, "rq_ivf_create: by_residual must be 0 or 1; got %d", by_residual); return nullptr; }
  DeviceInfo di;
  if (device_info(&di) != RQ_OK) return nullptr;
  rq_ivf *ix = new rq_ivf();
  ix->device = di.device; ix->num_cu = di.num_cu;
  ix->d = d; ix->nlist = nlist; ix->m = m; ix->mp = mp; ix->by_residual = by_residual;
  auto body = [&]() -> int {
    DeviceLock lock;
    RQ_HIP(hipMalloc((void **)&ix->coarse, (size_t)nlist * d * 4));
    RQ_HIP(hipMalloc((void **)&ix->sa, (size_t)nlist * 4));
    RQ_HIP(hipMalloc((void **)&ix->centers, (size_t)256 * d * 4));
    RQ_HIP(hipMemcpy(ix->coarse, coarse_host, (size_t)nlist * d * 4, hipMemcpyHostToDevice));
    RQ_HIP(hipMemcpy(ix->centers, centers_host, (size_t)256 * d * 4, hipMemcpyHostToDevice));
    RQ_LAUNCH(ivf_sa_kernel, dim3((nlist + IVF_T - 1) / IVF_T), dim3(IVF_T), 0, (hipStream_t) nullptr, ix->sa, ix->coarse, nlist, d);
    RQ_HIP(hipStreamSynchronize(nullptr));
    return RQ_OK;
  };
  if (body() != RQ_OK) { rq_ivf_destroy(ix); return nullptr; }
  return ix;
}

void rq_ivf_destroy(rq_ivf *ix) {
  if (!ix) return;
  {
    SavedDevice saved;
    (void)hipSetDevice(ix->device);
    DeviceLock lock;
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)ix->coarse, (void *)ix->sa, (void *)ix->centers, (void *)ix->codes, (void *)ix->ids, (void *)ix->off})
      if (p) (void)hipFree(p);
  }
  delete ix;
}

int rq_ivf_build(rq_ivf *ix, const float *X_host, int64_t n, uint32_t id_offset) {
  return ivf_load_rows("rq_ivf_build", ix, X_host, 4, n, id_offset, false);
}

int rq_ivf_build_bytes(rq_ivf *ix, const uint8_t *X_host, int64_t n, uint32_t id_offset) {
  return ivf_load_rows("rq_ivf_build_bytes", ix, X_host, 1, n, id_offset, false);
}

int rq_ivf_set_codes(rq_ivf *ix, const uint32_t *lists_host, const uint8_t *codes_host, int64_t n, uint32_t id_offset) {
  return ivf_load_codes("rq_ivf_set_codes", ix, lists_host, codes_host, n, id_offset, false);
}

int rq_ivf_add(rq_ivf *ix, const float *X_host, int64_t n, uint32_t id_offset) {
  return ivf_load_rows("rq_ivf_add", ix, X_host, 4, n, id_offset, true);
}

int rq_ivf_add_bytes(rq_ivf *ix, const uint8_t *X_host, int64_t n, uint32_t id_offset) {
  return ivf_load_rows("rq_ivf_add_bytes", ix, X_host, 1, n, id_offset, true);
}

int rq_ivf_add_codes(rq_ivf *ix, const uint32_t *lists_host, const uint8_t *codes_host, int64_t n, uint32_t id_offset) {
  return ivf_load_codes("rq_ivf_add_codes", ix, lists_host, codes_host, n, id_offset, true);
}

int rq_ivf_search(rq_ivf *ix, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, int nprobe, int k, int id_base) {
  return ivf_search_body("rq_ivf_search", ix, dists, ids, queries_host, nq, nprobe, k, id_base, nullptr);
}

int rq_ivf_search_refine(rq_ivf *ix, rq_dataset *ds, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, int nprobe,
                         int k, int kc, uint32_t id_offset, int id_base) {
  rerank_clear();
  IvfRefine rf;
  if (!ix || !dataset_view(ds, &rf.base)) return fail(RQ_EINVAL, "rq_ivf_search_refine: NULL argument");
  if (nq <= 0) return RQ_OK;
  RQ_TRY(rerank_check("rq_ivf_search_refine", !dists || !ids || !queries_host, rf.base.n, kc, kc, k, id_offset, id_base));
  if (rf.base.device != ix->device)
    return fail(RQ_EINVAL, "rq_ivf_search_refine: the dataset is on device %d, the index on device %d", rf.base.device, ix->device);
  if (rf.base.d != ix->d) return fail(RQ_EINVAL, "rq_ivf_search_refine: the dataset has d=%d, the index d=%d", rf.base.d, ix->d);
  rf.k = k;
  rf.id_offset = id_offset;
  rf.chain = rerank_chain(kc);
  return ivf_search_body("rq_ivf_search_refine", ix, dists, ids, queries_host, nq, nprobe, kc, id_base, &rf);
}

}  // extern "C"

namespace {

int ivf_search_body(const char *who, rq_ivf *ix, float *dists, uint32_t *ids, const float *queries_host, int64_t nq, int nprobe, int k,
                    int id_base, const IvfRefine *rf) {
  if (!ix || !dists || !ids || !queries_host) return fail(RQ_EINVAL, "%s: NULL argument", who);
  if (nq <= 0) return RQ_OK;
  if (nprobe < 1 || nprobe > ix->nlist) return fail(RQ_EINVAL, "%s: 1 <= nprobe <= nlist=%d; got nprobe=%d", who, ix->nlist, nprobe);
  if (k < 1) return fail(RQ_EINVAL, "%s: k=%d", who, k);
  if (id_base != 0 && id_base != 1) return fail(RQ_EINVAL, "%s: id_base must be 0 or 1; got %d", who, id_base);
  std::lock_guard<std::mutex> guard(ix->mu);
  if (!ix->codes || ix->n < 1) return fail(RQ_EINVAL, "%s: the index holds no base (rq_ivf_build / rq_ivf_set_codes)", who);
  const int kout = rf ? rf->k : k;       // entries per query of dists / ids
  SavedDevice saved;
  RQ_HIP(hipSetDevice(ix->device));
  DeviceLock lock;
  hipStream_t stream = nullptr;
  const int d = ix->d, nlist = ix->nlist;
  const uint32_t seg = (uint32_t)std::max(1, ivf_knob("IVF_SEGMENT_ROWS", 4096));
  // the host-side bounds that size the batch: the nprobe largest lists give the longest row of keys and the most items
  size_t ld_bound = 0, items_bound = 0;
  for (int r = 0; r < nprobe; ++r) {
    ld_bound += (size_t)ix->h_desc[r];
    items_bound += ((size_t)ix->h_desc[r] + seg - 1) / seg;
  }
  ld_bound = std::max<size_t>(ld_bound, (size_t)k);
  items_bound = std::max<size_t>(items_bound, 1);
  int64_t cap = std::min<int64_t>(nq, BK_MAX_NB);
  const int knob = ivf_knob("IVF_BATCH_QUERIES", 0);
  if (knob > 0) cap = std::min<int64_t>(cap, knob);
  int64_t lo = 0, hi = cap;
  while (lo < hi) {               // the largest batch whose scratch fits
    const int64_t mid = (lo + hi + 1) / 2;
    if (ivf_bytes(mid, nlist, nprobe, k, ld_bound, items_bound, rf).total() <= bulk_usable()) lo = mid;
    else hi = mid - 1;
  }
  const int64_t nbmax = lo;
  if (nbmax < 1)
    return fail(RQ_EUNSUPPORTED, "%s: one query's keys (up to %zu, k=%d) need more than the BULK_SCRATCH_BYTES budget of scratch", who,
                ld_bound, k);
  void *ws = nullptr;
  RQ_TRY(workspace(WS_BULK, ivf_bytes(nbmax, nlist, nprobe, k, ld_bound, items_bound, rf).total(), &ws, stream));
  DevMem dq, dd, di, dk;
  RQ_TRY(dq.alloc((size_t)nbmax * d * 4));
  RQ_TRY(dd.alloc((size_t)nbmax * kout * 4));
  RQ_TRY(di.alloc((size_t)nbmax * kout * 4));
  if (rf) RQ_TRY(dk.alloc((size_t)nbmax * k * 8));      // the sorted top-kc keys of step 4: the candidates
  unsigned long long valid = 0;
  int64_t batches = 0;
  std::vector<uint32_t> hv(rf ? (size_t)nbmax : 0);
  ix->s_ld = 0; ix->s_batch = nbmax; ix->s_items = 0; ix->s_rows = 0;
  for (double &t : ix->s_ms) t = 0;
  for (int64_t q0 = 0; q0 < nq; q0 += nbmax) {
    const int64_t nb = std::min(nbmax, nq - q0);
    const uint32_t ub = (uint32_t)nb;
    RQ_HIP(hipMemcpyAsync(dq.p, queries_host + (size_t)q0 * d, (size_t)nb * d * 4, hipMemcpyHostToDevice, stream));
    unsigned char *at = (unsigned char *)ws;
    uint32_t *probes = (uint32_t *)at; at += ivf_align((size_t)nb * nprobe * 4);
    uint32_t *koff = (uint32_t *)at; at += ivf_align((size_t)nb * nprobe * 4);
    uint32_t *ioff = (uint32_t *)at; at += ivf_align((size_t)nb * nprobe * 4);
    uint32_t *qrows = (uint32_t *)at; at += ivf_align((size_t)nb * 4);
    uint32_t *qitems = (uint32_t *)at; at += ivf_align((size_t)nb * 4);
    uint32_t *qbase = (uint32_t *)at; at += ivf_align((size_t)nb * 4);
    unsigned long long *stats = (unsigned long long *)at; at += 256;
    unsigned char *const phase = at;
    PhaseClock clock(stream, ix->s_ms);
    {   // 1. the probes
      uint64_t *ckeys = (uint64_t *)at; at += ivf_align((size_t)nb * nlist * 8);
      RQ_LAUNCH(ivf_coarse_keys_kernel, dim3((nlist + IVF_T - 1) / IVF_T, (ub + IVF_QT - 1) / IVF_QT), dim3(IVF_T), 0, stream, ckeys,
                dq.as<float>(), ix->coarse, ix->sa, ub, nlist, d);
      BulkSel s;
      s.src = ckeys; s.ld = (size_t)nlist;
      sel_layout(s, at, nb, (uint32_t)nprobe);
      uint32_t hx;
      sel_grid(s, (uint32_t)nlist, nb, ix->num_cu, &hx);
      BulkOut o;
      o.dists = nullptr; o.keys = nullptr; o.ids = probes; o.id_base = 0;
      RQ_TRY(sel_run(s, hx, nb, o, stream));
    }
    clock.mark(0);
    // 2. the work items
    RQ_LAUNCH(ivf_plan_kernel, dim3((ub + IVF_T - 1) / IVF_T), dim3(IVF_T), 0, stream, koff, ioff, qrows, qitems, probes, ix->off, ub,
              nprobe, seg, (uint32_t)nlist);
    RQ_LAUNCH(ivf_scan_kernel, dim3(1), dim3(1024), 0, stream, qbase, stats, qitems, qrows, ub);
    unsigned long long hs[3];
    RQ_HIP(hipMemcpyAsync(hs, stats, sizeof(hs), hipMemcpyDeviceToHost, stream));
    RQ_HIP(hipStreamSynchronize(stream));
    const unsigned long long nitems = hs[0];
    const size_t ld = std::max<size_t>((size_t)hs[1], (size_t)k);
    if (ld > ld_bound || nitems > (unsigned long long)nb * items_bound || nitems >= (1ull << 31))
      return fail(RQ_EINVAL, "%s: %llu items, %zu keys per query exceed the plan (%zu, %zu)", who, nitems, ld,
                  (size_t)nb * items_bound, ld_bound);
    at = phase;
    IvfItem *items = (IvfItem *)at; at += ivf_align((size_t)nb * items_bound * sizeof(IvfItem));
    uint64_t *keys = (uint64_t *)at; at += ivf_align((size_t)nb * ld * 8);
    if (nitems)
      RQ_LAUNCH(ivf_items_kernel, dim3((uint32_t)(((size_t)nb * nprobe + IVF_T - 1) / IVF_T)), dim3(IVF_T), 0, stream, items, probes,
                ix->off, koff, ioff, qbase, ub, nprobe, seg, (uint32_t)nlist, nitems);
    clock.mark(1);
    // 3. the keys
    RQ_LAUNCH(ivf_fill_kernel, dim3((uint32_t)std::min<size_t>(64, (ld + IVF_T - 1) / IVF_T), ub), dim3(IVF_T), 0, stream, keys,
              qrows, ld);
    if (nitems) {
      IvfKeyParams p;
      p.items = items; p.codes = ix->codes; p.ids = ix->ids; p.centers = ix->centers; p.coarse = ix->coarse;
      p.queries = dq.as<float>(); p.keys = keys; p.ld = ld;
      p.m = ix->m; p.sub = d / ix->m; p.d = d; p.by_residual = ix->by_residual;
      int rc = RQ_EUNSUPPORTED;
      switch (ix->mp) {
#define RQ_IVF_CASE(MP) case MP: rc = ivf_keys_launch<MP>(p, (uint32_t)nitems, stream); break;
        RQ_IVF_CASE(2) RQ_IVF_CASE(4) RQ_IVF_CASE(8) RQ_IVF_CASE(16) RQ_IVF_CASE(32) RQ_IVF_CASE(64)
#undef RQ_IVF_CASE
      }
      RQ_TRY(rc);
    }
    clock.mark(2);
    {   // 4. the top-k
      BulkSel s;
      s.src = keys; s.ld = ld;
      sel_layout(s, at, nb, (uint32_t)k);
      uint32_t hx;
      sel_grid(s, (uint32_t)ld, nb, ix->num_cu, &hx);
      BulkOut o;
      if (rf) { o.dists = nullptr; o.ids = nullptr; o.keys = dk.as<uint64_t>(); o.id_base = 0; }
      else { o.dists = dd.as<float>(); o.ids = di.as<uint32_t>(); o.keys = nullptr; o.id_base = (uint32_t)id_base; }
      RQ_TRY(sel_run(s, hx, nb, o, stream));
    }
    clock.mark(3);
    if (rf) {   // 5. the candidates by their exact distance: the phase scratch is free again (one stream)
      RerankCall c;
      c.base = rf->base;
      c.Q = dq.as<float>();
      c.cand = dk.as<uint32_t>(); c.ldc = 2 * (size_t)k; c.cstep = 2;
      c.nb = nb; c.kc = k; c.k = kout; c.id_offset = rf->id_offset; c.id_base = id_base;
      c.dists = dd.as<float>(); c.ids = di.as<uint32_t>();
      c.scratch = phase;
      c.nvalid_host = hv.data();
      c.chain = rf->chain;
      c.ph_keys = 4; c.ph_select = 5;
      RQ_TRY(rerank_device(c, stream, clock, ix->num_cu));
    }
    RQ_HIP(hipMemcpyAsync(dists + (size_t)q0 * kout, dd.p, (size_t)nb * kout * 4, hipMemcpyDeviceToHost, stream));
    RQ_HIP(hipMemcpyAsync(ids + (size_t)q0 * kout, di.p, (size_t)nb * kout * 4, hipMemcpyDeviceToHost, stream));
    RQ_HIP(hipStreamSynchronize(stream));
    clock.collect();
    if (rf) for (int64_t b = 0; b < nb; ++b) valid += hv[(size_t)b];
    ++batches;
    ix->s_ld = std::max<int64_t>(ix->s_ld, (int64_t)ld);
    ix->s_items += (int64_t)nitems;
    ix->s_rows += (int64_t)hs[2];
  }
  if (rf) {
    rerank_add_ms(ix->s_ms[4], ix->s_ms[5]);
    rerank_note(nq, k, batches, valid, rf->chain);
  }
  return RQ_OK;
}

}  // namespace

extern "C" {

int rq_ivf_get_lists(rq_ivf *ix, int64_t *offsets, uint32_t *row_ids, uint8_t *codes) {
  if (!ix) return fail(RQ_EINVAL, "rq_ivf_get_lists: NULL index");
  std::lock_guard<std::mutex> guard(ix->mu);
  if (!ix->codes) return fail(RQ_EINVAL, "rq_ivf_get_lists: the index holds no base");
  SavedDevice saved;
  RQ_HIP(hipSetDevice(ix->device));
  DeviceLock lock;
  if (offsets) std::copy(ix->h_off.begin(), ix->h_off.end(), offsets);
  if (row_ids) RQ_HIP(hipMemcpy(row_ids, ix->ids, (size_t)ix->n * 4, hipMemcpyDeviceToHost));
  if (codes) {
    if (ix->m == ix->mp) {
      RQ_HIP(hipMemcpy(codes, ix->codes, (size_t)ix->n * ix->m, hipMemcpyDeviceToHost));
    } else {      // the padding bytes stay behind
      RQ_HIP(hipMemcpy2D(codes, (size_t)ix->m, ix->codes, (size_t)ix->mp, (size_t)ix->m, (size_t)ix->n, hipMemcpyDeviceToHost));
    }
  }
  return RQ_OK;
}

int rq_ivf_info(rq_ivf *ix, int64_t *out, int cap) {
  if (!ix || !out || cap < 1) return fail(RQ_EINVAL, "rq_ivf_info: NULL argument");
  std::lock_guard<std::mutex> guard(ix->mu);
  int64_t empty = 0;
  for (int64_t s : ix->h_desc) empty += s == 0;
  const int64_t v[12] = {ix->codes ? ix->n : 0, ix->nlist, ix->m, ix->d, ix->by_residual, ix->h_desc.empty() ? 0 : ix->h_desc[0], empty,
                         ix->s_ld, ix->s_batch, ix->s_items, ix->s_rows, ix->codes ? (int64_t)ix->next_id : 0};
  for (int i = 0; i < cap && i < 12; ++i) out[i] = v[i];
  return RQ_OK;
}

int rq_ivf_last_timing(rq_ivf *ix, double *ms, int cap) {
  if (!ix || !ms || cap < 1) return fail(RQ_EINVAL, "rq_ivf_last_timing: NULL argument");
  std::lock_guard<std::mutex> guard(ix->mu);
  for (int i = 0; i < cap && i < 8; ++i) ms[i] = i < 4 ? ix->s_ms[i] : ix->l_ms[i - 4];
  return RQ_OK;
}

}  // extern "C"
