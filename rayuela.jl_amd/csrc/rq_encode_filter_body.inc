// rq_encode_filter_body.inc -- the filter kernel, the canonical evaluation of one work item and the exact-pass kernel of
// rq_encode_filter.hip, which includes this text twice: RQ_ENC_BYTES = 0 gives encode_pq_filter_kernel / exact_item /
// encode_pq_fix_kernel on f32 rows, token for token what they were before byte rows existed (tests/test_isa.py walks their
// code, and sharing the body through a function template moved their register allocation); RQ_ENC_BYTES = 1 gives
// encode_pq_filter_bytes_kernel / exact_item_bytes / encode_pq_fix_bytes_kernel, which read p.X as uint8 rows.  Only the
// loaders differ (and the MFMA against the bf16 low piece of x, identically zero for an integer 0..255).
#if RQ_ENC_BYTES
#define RQ_ENC_FILTER_KERNEL encode_pq_filter_bytes_kernel
#define RQ_ENC_EXACT_ITEM exact_item_bytes
#define RQ_ENC_FIX_KERNEL encode_pq_fix_bytes_kernel
#else
#define RQ_ENC_FILTER_KERNEL encode_pq_filter_kernel
#define RQ_ENC_EXACT_ITEM exact_item
#define RQ_ENC_FIX_KERNEL encode_pq_fix_kernel
#endif

template <int SUB, int NT, int NWAVES, bool DBG = false>
__global__ __launch_bounds__(NWAVES * 64) void RQ_ENC_FILTER_KERNEL(EncParams p) {
  using Shape = SplitShape<SUB>;
  constexpr bool PACK = Shape::PACK;
  constexpr int NPIECE = Shape::NPIECE;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int m = p.m, h = p.h, d = p.d;
  const int i0 = p.i0, mg = p.i1 - p.i0;
  uint4 *cbA = reinterpret_cast<uint4 *>(smem);
  float *saL = reinterpret_cast<float *>(cbA + (size_t)mg * NT * NPIECE * 64);
  float *saMax = saL + (size_t)mg * NT * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, hi = lane >> 5;
  {   // the launch's table image, as encode_tables_kernel left it
    const uint4 *src = reinterpret_cast<const uint4 *>(p.image);
    uint4 *dst = reinterpret_cast<uint4 *>(smem);
    const int n16 = (int)(filter_image_bytes<SUB>(mg, NT) / 16);
    for (int idx = tid; idx < n16; idx += NWAVES * 64) dst[idx] = src[idx];
    __syncthreads();
  }

  const int64_t ntiles = (p.n + 31) / 32;
  const int64_t total_waves = (int64_t)gridDim.x * NWAVES;
  const int64_t tile0 = (int64_t)blockIdx.x * NWAVES + wave;
  // the lane's 8 K elements of the sub-vector in flight: dimensions 8 hi .. 8 hi + 7 (PACK: 0 .. 7 in both halves)
  constexpr int NPAIR = PACK ? SUB / 2 : 4;
  const int my_pairs = PACK ? SUB / 2 : (hi ? (SUB - 8) / 2 : 4);
  const bool vec4 = (d % 4 == 0) && (((uintptr_t)p.X & 15) == 0) && (SUB % 4 == 0);
  f32x2 xn[NPAIR];
#if RQ_ENC_BYTES
  // byte rows: the lane's 8 K elements travel as the 8 bytes they are (zero above the lane's share) and are widened
  // when their turn comes; the widest load the addresses X + row d + i SUB + 8 hi allow, down to single bytes
  uint32_t xb[2];
  const int al = byte_align(p.X, d, SUB);
  (void)vec4;
  auto gload = [&](int64_t tile, int il) {
    int64_t gr = tile * 32 + j;
    if (gr >= p.n) gr = p.n - 1;
    load_bytes<8>(reinterpret_cast<const uint8_t *>(p.X) + (size_t)gr * d + (size_t)(i0 + il) * SUB + (PACK ? 0 : 8 * hi), al,
                  2 * my_pairs, xb);
  };
#else
  auto gload = [&](int64_t tile, int il) {
    int64_t gr = tile * 32 + j;
    if (gr >= p.n) gr = p.n - 1;
    const float *src = p.X + gr * d + (size_t)(i0 + il) * SUB + (PACK ? 0 : 8 * hi);
    if (vec4) {
#pragma unroll
      for (int u = 0; u < NPAIR; u += 2) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (u < my_pairs) v = *reinterpret_cast<const float4 *>(src + 2 * u);
        xn[u] = f32x2{v.x, v.y};
        if (u + 1 < NPAIR) xn[u + 1] = f32x2{v.z, v.w};
      }
    } else {
#pragma unroll
      for (int u = 0; u < NPAIR; ++u) xn[u] = u < my_pairs ? *reinterpret_cast<const f32x2 *>(src + 2 * u) : f32x2{0.0f, 0.0f};
    }
  };
#endif
  if (tile0 < ntiles) gload(tile0, 0);
  const int cbase = 4 * hi;          // centroid of (tile t, register r): 32 t + 4 hi + 8 (r >> 2) + (r & 3)

  for (int64_t tile = tile0; tile < ntiles; tile += total_waves) {
    const int64_t row0 = tile * 32;
    uint64_t cw[4] = {0, 0, 0, 0};
    uint32_t fl = 0;                 // bit il: (this row, sub-quantizer i0 + il) goes to the exact pass
    // the tile loop's result for one sub-quantizer, consumed by `settle` (one candidate, or the exact pass)
    struct Pend { f32x16 ub; float b1, delta; int t1, il; uint64_t amb; bool slow; };
    auto settle_v = [&](const f32x16 &q_ub, float q_b1, float q_delta, int q_t1, int q_il, uint64_t q_amb, bool q_slow) {
      const int i = i0 + q_il;
      float bo_a = q_b1, bo_b = q_b1;                              // the other half of this vector's centroids
      swap32(bo_a, bo_b);
      const float bo = hi ? bo_a : bo_b;
      const float thr = __builtin_fminf(q_b1, bo) + q_delta;
      const bool contend = (q_b1 <= thr) && !q_slow;
#if defined(RQ_FILT_ABL) && RQ_FILT_ABL == 5
      uint32_t cm = __float_as_uint(q_ub[3]) & 0xffffu;
#else
      uint32_t cm = mask_leq16_4(q_ub, thr);
#endif
      if (!contend) cm = 0;
      const bool todo = contend && __builtin_amdgcn_inverse_ballot_w64(q_amb);
      const int r1 = __builtin_ctz(cm | 0x10000u);
      const uint32_t kmine = cm != 0u ? (uint32_t)(q_t1 * 32 + cbase + 8 * (r1 >> 2) + (r1 & 3)) : 0xffffu;
      // candidate counts of the two halves add; a flagged tile or an unusable bound in either half shows
      const uint32_t mine_w = ((uint32_t)__builtin_popcount(cm) | (todo ? 0x100u : 0u) | (q_slow ? 0x200u : 0u)) << 16 | kmine;
      float ow_a = __uint_as_float(mine_w), ow_b = __uint_as_float(mine_w);
      swap32(ow_a, ow_b);
      const uint32_t other_w = __float_as_uint(hi ? ow_a : ow_b);
      const bool single = (mine_w >> 16) + (other_w >> 16) == 1u;
      const uint32_t kk = min(mine_w & 0xffffu, other_w & 0xffffu);       // the candidate (single) or any stand-in
      fl |= single ? 0u : (1u << q_il);
      const uint64_t bk = (uint64_t)(kk & 0xffu) << (8 * (i & 7));
      switch (i >> 3) {          // (uniform: one 64-bit shift and OR instead of four selected ones)
        case 0: cw[0] |= bk; break;
        case 1: cw[1] |= bk; break;
        case 2: cw[2] |= bk; break;
        default: cw[3] |= bk; break;
      }
    };
    auto settle = [&](const Pend &q) { settle_v(q.ub, q.b1, q.delta, q.t1, q.il, q.amb, q.slow); };
    Pend pend;
    // One sub-quantizer: B fragments, tile loop.  EPI: the PREVIOUS sub-quantizer's `settle` -- ~80 VALU instructions in
    // dependent chains with two half-wave exchanges, no matrix work of its own -- is placed inside this one's straight-line
    // tile loop, where the scheduler can slide it under the MFMAs (build knob RQ_FILT_PIPE = 1; default: it runs right after its
    // own loop).  MEASURED, round 5: the carried state (16 W values + 6 scalars) costs more than the overlap returns -- 252
    // registers at 8 wavefronts per CU: 0.356 ms per 1e6 SIFT-shape vectors against 0.342 unpipelined at 8 and 0.334 at 12
    // wavefronts (where the pipelined build spills 88 registers: 0.390); Deep shape 0.572 / 0.581 / 0.501.  Not shipped.
    auto unit = [&](int il, auto epi_tag) {
      constexpr bool EPI = decltype(epi_tag)::value;
      const int i = i0 + il;
      // |x|^2 (any order: it only scales the margin) and the B fragments: this lane's 8 K elements of x as bf16 pieces
      f32x2 sel[4];
      f32x2 sq = {0.0f, 0.0f};
#if RQ_ENC_BYTES
      {                                // widen what gload brought (v_cvt_f32_ubyteN: exact)
        float xf[8];
        bytes_f32<8>(xb, xf);
#pragma unroll
        for (int u = 0; u < NPAIR; ++u) xn[u] = f32x2{xf[2 * u], xf[2 * u + 1]};
      }
#endif
#pragma unroll
      for (int u = 0; u < NPAIR; ++u) sq = __builtin_elementwise_fma(xn[u], xn[u], sq);
#pragma unroll
      for (int u = 0; u < 4; ++u) sel[u] = u < NPAIR ? xn[u < NPAIR ? u : 0] : f32x2{0.0f, 0.0f};
#if RQ_ENC_BYTES
      // An integer 0..255 has 8 significant bits and so is its own bf16 high piece: the low piece is identically zero, and
      // the MFMA against it (which would add exact zeros to W) is left out.
      uint32_t bh[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) bh[u] = __builtin_bit_cast(uint32_t, __builtin_convertvector(sel[u], bf16x2_t));
      const bf16x8_t Bh = __builtin_bit_cast(bf16x8_t, make_uint4(bh[0], bh[1], bh[2], bh[3]));
#else
      uint32_t bh[4], bl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bf16x2_t hb = __builtin_convertvector(sel[u], bf16x2_t);
        const f32x2 rest = sel[u] - __builtin_convertvector(hb, f32x2);
        bh[u] = __builtin_bit_cast(uint32_t, hb);
        bl[u] = __builtin_bit_cast(uint32_t, __builtin_convertvector(rest, bf16x2_t));
      }
      if (PACK && hi) { bl[0] = bl[1] = bl[2] = bl[3] = 0; }                // second MFMA: [xl | 0] against [ch | cl]
      const bf16x8_t Bh = __builtin_bit_cast(bf16x8_t, make_uint4(bh[0], bh[1], bh[2], bh[3]));
      const bf16x8_t Bl = __builtin_bit_cast(bf16x8_t, make_uint4(bl[0], bl[1], bl[2], bl[3]));
#endif
      float sb = sq.x + sq.y;
      if constexpr (!PACK) {                               // the other half-wave holds dimensions 8..15
        float sa_ = sb, sb_ = sb;                          // (v_permlane32_swap: no trip through the LDS crossbar)
        swap32(sa_, sb_);
        sb += hi ? sa_ : sb_;
      }
      // the next sub-vector travels while this one is filtered
      if (il + 1 < mg) gload(tile, il + 1);
      else if (tile + total_waves < ntiles) gload(tile + total_waves, 0);
      const float smax = saMax[il];
      const float ssum = smax + sb;
      const float delta = p.delta_rel * ssum;
      // the bound needs finite, non-vanishing magnitudes; otherwise the pair goes to the exact pass
      const bool slow = !(delta < __uint_as_float(0x7f800000u)) || !(ssum >= SplitCfg::TINY);

      float b1 = 0.0f;                           // running minimum of W over this lane's centroids
      int t1 = 0;                                // the tile that holds it (the first one, on ties)
      uint64_t amb = 0;                          // LANE MASK (scalar registers): another tile came within delta of the running
                                                 // minimum and has not been left behind by more than delta since
      f32x16 ub;                                 // the 16 W values of tile t1
      const uint4 *cb_i = cbA + (size_t)il * NT * NPIECE * 64 + lane;
      const float4 *sa_i = reinterpret_cast<const float4 *>(saL + ((size_t)il * NT * 2 + hi) * 16);
      // fragments of one tile: |c|^2 straight into the accumulator registers, the A pieces beside them
      struct Frag { f32x16 acc; uint4 a0, a1; };
      auto fetch = [&](int t) -> Frag {
        Frag f;
        const float4 *s4 = sa_i + (size_t)t * 8;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 v = s4[g4];
          f.acc[g4 * 4 + 0] = v.x; f.acc[g4 * 4 + 1] = v.y; f.acc[g4 * 4 + 2] = v.z; f.acc[g4 * 4 + 3] = v.w;
        }
        f.a0 = cb_i[(size_t)t * NPIECE * 64];
        f.a1 = PACK ? f.a0 : cb_i[(size_t)t * NPIECE * 64 + 64];
        return f;
      };
      auto products = [&](const Frag &f) -> f32x16 {
#if defined(RQ_FILT_ABL) && RQ_FILT_ABL == 1
        { f32x16 a = f.acc; a[0] += __uint_as_float(f.a0.x ^ f.a1.y ^ bh[0] ^ bl[1]); return a; }
#endif
        const bf16x8_t A0 = __builtin_bit_cast(bf16x8_t, f.a0);
        f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, Bh, f.acc, 0, 0, 0);
#if !RQ_ENC_BYTES
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0, Bl, acc, 0, 0, 0);
#endif
        if constexpr (!PACK) {
          const bf16x8_t A1 = __builtin_bit_cast(bf16x8_t, f.a1);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1, Bh, acc, 0, 0, 0);
        }
        return acc;
      };
      auto filter = [&](const f32x16 &a, int t) {
        if constexpr (DBG) {    // tests/test_gpu_encode_margin.py: the very values the filter decides on
          if (row0 + j < p.n) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int k = t * 32 + 4 * hi + 8 * (r >> 2) + (r & 3);
              if (k < h) p.dbg_w[((size_t)(row0 + j) * m + i) * h + k] = a[r];
            }
          }
        }
#if defined(RQ_FILT_ABL) && RQ_FILT_ABL == 2
        b1 = __builtin_fminf(b1, a[t & 15]); return;
#endif
        const float mm = min16(a);
        if (t == 0) {                   // (compile-time: the loop is unrolled)
          b1 = mm;
          ub = a;
          return;
        }
        // Invariant after tile t: b1 = the smallest tile minimum so far, t1 = the first tile that reached it, and -- where
        // `amb` is clear -- every other tile seen so far lies more than delta above b1.  A tile within delta of the running
        // minimum sets the flag, whichever of the two is smaller; a minimum that improves by MORE than delta leaves all
        // earlier tiles out of reach and clears it.  The flag lives in a scalar register pair: two SALU instructions per
        // tile instead of a handful of per-lane selects.
        const bool imp = mm < b1;
        const bool near = __builtin_fabsf(mm - b1) <= delta;       // (NaN: false)
        const uint64_t impm = __builtin_amdgcn_ballot_w64(imp), nearm = __builtin_amdgcn_ballot_w64(near);
        amb = nearm | (amb & ~impm);
#if !defined(RQ_FILT_ABL) || RQ_FILT_ABL != 3
        copy_lanes(ub, a, impm);
#else
        ub[t & 15] += a[t & 15];
#endif
        b1 = __builtin_fminf(b1, mm);
        t1 = imp ? t : t1;
      };
      // straight-line tile loop: fragments of tile t + 1 are requested before the MFMAs of tile t issue, the filter of
      // tile t - 1 runs on the VALU under them
      {
        Frag cur = fetch(0), nxt;
        f32x16 done;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#if defined(RQ_FILT_ABL) && RQ_FILT_ABL == 4
          if (t + 1 < NT) { nxt = cur; nxt.a0.x += t; }
#else
          if (t + 1 < NT) nxt = fetch(t + 1);
#endif
          const f32x16 acc = products(cur);
          if (t > 0) filter(done, t - 1);
          if constexpr (EPI) { if (t == (NT > 2 ? 2 : NT - 1)) settle(pend); }
          done = acc;
          if (t + 1 < NT) cur = nxt;
        }
        filter(done, NT - 1);
      }
#if defined(RQ_FILT_PIPE) && RQ_FILT_PIPE
      pend.ub = ub; pend.b1 = b1; pend.delta = delta; pend.t1 = t1; pend.il = il; pend.amb = amb; pend.slow = slow;
#else
      settle_v(ub, b1, delta, t1, il, amb, slow);       // (directly on the live registers: no copy of the 16 kept values)
#endif
    };

#if defined(RQ_FILT_PIPE) && RQ_FILT_PIPE
    unit(0, std::false_type{});
#pragma unroll 1
    for (int il = 1; il < mg; ++il) unit(il, std::true_type{});
    settle(pend);
#else
#pragma unroll 1
    for (int il = 0; il < mg; ++il) unit(il, std::false_type{});
    (void)settle;
    (void)pend;
#endif
    if (hi == 0 && row0 + j < p.n) {
      uint8_t *o = p.codes + (size_t)(row0 + j) * m;
      if ((m & 7) == 0 && mg == m) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
          if (w * 8 < m) reinterpret_cast<uint64_t *>(o)[w] = cw[w];
      } else {
        for (int i = i0; i < p.i1; ++i) o[i] = (uint8_t)(cw[i >> 3] >> (8 * (i & 7)));
      }
      p.flags[row0 + j] = fl;
    }
  }
}

// The canonical evaluation of one work item -- sub-quantizer i, the rows the 32 lane pairs hold (lane (j, hi): row of lane j) --
// against ALL h centroids on v_mfma_f32_32x32x2_f32; returns the first index of the minimum for the lane's row.  sa_i: this
// sub-quantizer's |c|^2 table in C/D-fragment order, already offset by the lane's half (LDS).
template <int SUB, int NT>
__device__ __forceinline__ int RQ_ENC_EXACT_ITEM(const EncParams &p, int i, int64_t row, const float4 *sa_i) {
  constexpr int KS = SUB / 2;
  const int lane = threadIdx.x & 63, j = lane & 31, hi = lane >> 5;
  const int h = p.h, d = p.d;
  // the row's sub-vector: |x|^2 (canonical chain) and the B fragments (lane: k = 2 kk + hi of vector j)
  float x[SUB];
#if RQ_ENC_BYTES
  {   // byte rows: the SUB bytes with the widest loads the address X + row d + i SUB allows, widened exactly
    uint32_t w[(SUB + 3) / 4];
    load_bytes<SUB>(reinterpret_cast<const uint8_t *>(p.X) + (size_t)row * d + (size_t)i * SUB, byte_align(p.X, d, SUB), SUB, w);
    bytes_f32<SUB>(w, x);
  }
#else
  const float *xs = p.X + (size_t)row * d + (size_t)i * SUB;
  if ((SUB % 4 == 0) && (d % 4 == 0) && (((uintptr_t)p.X & 15) == 0)) {
#pragma unroll
    for (int s4 = 0; s4 < SUB / 4; ++s4) {
      const float4 v = reinterpret_cast<const float4 *>(xs)[s4];
      x[4 * s4] = v.x; x[4 * s4 + 1] = v.y; x[4 * s4 + 2] = v.z; x[4 * s4 + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int s2 = 0; s2 < SUB / 2; ++s2) {
      const f32x2 v = reinterpret_cast<const f32x2 *>(xs)[s2];
      x[2 * s2] = v.x; x[2 * s2 + 1] = v.y;
    }
  }
#endif
  float sb = 0.0f;
#pragma unroll
  for (int s = 0; s < SUB; ++s) sb = __builtin_fmaf(x[s], x[s], sb);
  float b[KS];
#pragma unroll
  for (int kk = 0; kk < KS; ++kk) b[kk] = hi ? x[2 * kk + 1] : x[2 * kk];
  ArgminState st;
  st.best_v = __uint_as_float(0x7f800000u);
  st.best_t = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) st.ub[r] = f32x2{0.0f, 0.0f};
  // A fragments: lane (j, hi) wants C_i[32 t + j][2 kk + hi].  For 8-wide halves (sub = 16) the lane loads floats
  // 8 hi .. 8 hi + 7 of its centroid (two 16-byte loads) and one v_permlane32_swap per register PAIR turns
  // (c[2q] | c[8 + 2q]), (c[2q + 1] | c[9 + 2q]) into the fragments of k-steps q and 4 + q; other widths load the whole
  // row and select.  Four tiles are requested at a time, so an item waits for L2 twice, not once per tile.
  auto cload = [&](int t, float (&a)[KS]) {
    const int cen = t * 32 + j;
    if constexpr (SUB == 16) {
      float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0;
      if (cen < h) {
        const float4 *src = reinterpret_cast<const float4 *>(p.C + ((size_t)i * h + cen) * SUB + 8 * hi);
        v0 = src[0]; v1 = src[1];
      }
      float r[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        swap32(r[2 * q], r[2 * q + 1]);
        a[q] = r[2 * q]; a[4 + q] = r[2 * q + 1];
      }
    } else {
      float c[SUB];
#pragma unroll
      for (int s = 0; s < SUB; ++s) c[s] = 0.0f;
      if (cen < h) {
        const float *src = p.C + ((size_t)i * h + cen) * SUB;
        if constexpr (SUB % 4 == 0) {
#pragma unroll
          for (int s4 = 0; s4 < SUB / 4; ++s4) {
            const float4 v = reinterpret_cast<const float4 *>(src)[s4];
            c[4 * s4] = v.x; c[4 * s4 + 1] = v.y; c[4 * s4 + 2] = v.z; c[4 * s4 + 3] = v.w;
          }
        } else {
#pragma unroll
          for (int s2 = 0; s2 < SUB / 2; ++s2) {
            const f32x2 v = reinterpret_cast<const f32x2 *>(src)[s2];
            c[2 * s2] = v.x; c[2 * s2 + 1] = v.y;
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) a[kk] = hi ? c[2 * kk + 1] : c[2 * kk];
    }
  };
  constexpr int TB = NT < 4 ? NT : (KS >= 8 ? 2 : 4);        // tiles per batch (registers: 128 per lane at 4 wavefronts per SIMD)
#pragma unroll
  for (int t0 = 0; t0 < NT; t0 += TB) {
    float a[TB][KS];
#pragma unroll
    for (int u = 0; u < TB; ++u) cload(t0 + u, a[u]);
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][kk], b[kk], acc, 0, 0, 0);
      tile_argmin(acc, sa_i + (size_t)(t0 + u) * 8, sb, t0 + u, st);
    }
  }
  float best_v = st.best_v;
  int best_i = argmin_finish(st, hi);
  const float ov = __shfl_xor(best_v, 32);
  const int oi = __shfl_xor(best_i, 32);
  if (ov < best_v || (ov == best_v && oi < best_i)) { best_v = ov; best_i = oi; }
  return best_i;
}

template <int SUB, int NT>
__global__ __launch_bounds__(FIX_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void RQ_ENC_FIX_KERNEL(EncParams p) {
  constexpr int KS = SUB / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int mg = p.i1 - p.i0, h = p.h, d = p.d, m = p.m;
  float *saL = reinterpret_cast<float *>(smem);                                   // [mg][NT][2][16] |c|^2, C/D-fragment order
  uint32_t *cnt = reinterpret_cast<uint32_t *>(saL + (size_t)mg * NT * 32);       // [mg]
  uint16_t *list = reinterpret_cast<uint16_t *>(cnt + 32);                        // [mg][fix_rows] flagged rows of the chunk
  const int FIX_ROWS = p.fix_rows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, hi = lane >> 5;
  const int64_t row_base = (int64_t)blockIdx.x * FIX_ROWS;
  if (tid < 32) cnt[tid] = 0;
  __syncthreads();
  uint32_t any = 0;
  for (int r = tid; r < FIX_ROWS && row_base + r < p.n; r += FIX_THREADS) {
    uint32_t fl = p.flags[row_base + r];
    any |= fl;
    while (fl) {
      const int il = __builtin_ctz(fl);
      fl &= fl - 1u;
      list[(size_t)il * FIX_ROWS + atomicAdd(&cnt[il], 1u)] = (uint16_t)r;
    }
  }
  if (!__syncthreads_or(any != 0u)) return;
  if (p.stat && tid < 32 && tid < mg && cnt[tid]) atomicAdd(p.stat, (unsigned long long)cnt[tid]);
  // the norm table (canonical chain s = 0..sub-1 from +0; +inf for centroids >= h) of the launch's table image
  const float *sa_img = reinterpret_cast<const float *>(reinterpret_cast<const uint4 *>(p.image) + (size_t)mg * NT * SplitShape<SUB>::NPIECE * 64);
  for (int idx = tid; idx < mg * NT * 32; idx += FIX_THREADS) saL[idx] = sa_img[idx];
  __syncthreads();

  int item = 0;       // items are numbered sub-quantizer by sub-quantizer; wavefront w takes items w, w + 8, ...
  for (int il = 0; il < mg; ++il) {
    const int ne = (int)cnt[il];
    const int i = p.i0 + il;
    for (int e0 = 0; e0 < ne; e0 += 32, ++item) {
      if ((item & (FIX_THREADS / 64 - 1)) != wave) continue;
      const int e = min(e0 + j, ne - 1);                  // (lanes past the end repeat the last row; nothing is stored for them)
      const int64_t row = row_base + list[(size_t)il * FIX_ROWS + e];
      const int best_i = RQ_ENC_EXACT_ITEM<SUB, NT>(p, i, row, reinterpret_cast<const float4 *>(saL + ((size_t)il * NT * 2 + hi) * 16));
      if (hi == 0 && e0 + j < ne) p.codes[(size_t)row * m + i] = (uint8_t)best_i;
    }
  }
}

#undef RQ_ENC_FILTER_KERNEL
#undef RQ_ENC_EXACT_ITEM
#undef RQ_ENC_FIX_KERNEL
