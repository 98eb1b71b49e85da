// conv_big_body: the LDS-DMA implicit-GEMM tile of conv_big.hip (its header comment describes the
// structure), one template over the element types of conv_tile.h KT<T>: bf16, int8 and fp8.  Internal
// header (anonymous namespace, as conv_tile.h).  The 2:4 tile of conv_sp24.hip keeps its own main loop
// and shares this body's gather pieces through conv_tile.h (profiles/sp24_fold/README.txt).
#pragma once
#include "common.h"
#include "conv_tile.h"

namespace drnmi {
namespace {

// The main-loop schedule is pinned: fragment reads for group q+1 go out before group q's MFMAs
// (sched_barrier between groups) and the next step's DMA pieces are issued without a branch (the
// last steps re-fetch a clamped step into the idle stage).  Without the pins the compiler sinks
// each read next to its MFMAs and waits lgkmcnt(0) on it (no LDS latency hiding).
template <typename T, int KS, int WCO, int WC, int NST, int BK, bool PERSIST, int NWP, bool SPARSE, bool X2 = false,
          bool STRIP = false>
__device__ __forceinline__ void conv_big_body(const drnmi_conv_args& p) {
  using K = KT<T>;
  using C = BigCfg<WCO, WC, NST, BK, NWP, K::ESZ>;
  static_assert(!SPARSE || K::ESZ == 2, "unit skipping: bf16 only");
  // fp8: one MFMA covers a whole row (128 B, or a 64-B row in its low half): one substep per K step
  constexpr bool F8 = kIsF8<T>;
  static_assert(!F8 || (!STRIP && !X2 && !PERSIST), "fp8: the plain per-tap gather");
  constexpr int NSUB = F8 ? 1 : C::SUB;
  static_assert(!STRIP || (KS == 3 && NST == 2 && C::ROWB == 128 && !PERSIST && !SPARSE && !X2 && C::NW == 8),
                "strip mode: the 256 x 256 3x3 instantiations with 128-B rows (bf16 BK 64, int8 BK 128)");
  constexpr int CE = 16 / K::ESZ;   // elements per 16-B chunk
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wc = wave / NWP;        // channel column of the tile
  const int wp = wave % NWP;        // PXW-pixel slice of the tile
  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int nco = (p.cout + C::BCO - 1) / C::BCO;
  const int npx = (M + kBPX - 1) / kBPX;
  const int ntiles = npx * nco;

  const int cin = p.cin;
  const int lc = 31 - __builtin_clz(cin);
  const int H = p.h, W = p.w, dil = p.dil;
  const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
  const T* __restrict__ wt = reinterpret_cast<const T*>(p.wgt);
  const int nk = p.k_pad / BK;
  // fused second input (x2 != NULL: the block's 1x1 downsample folded into this conv, the
  // concatenated-K GEMM [W | W_ds] x [im2col(x) ; x2 sampled at stride2]): the last
  // cin2 / BK K steps read x2 instead of a tap of x
  const T* __restrict__ x2 = reinterpret_cast<const T*>(p.x2);
  const int nk1 = X2 ? (KS * KS * cin) / BK : nk;
  const int fr = lane & 15;       // fragment row (channel or pixel within a 16-block)
  const int fq = lane >> 4;       // 16-B k chunk within a 64-B substep

  // --- DMA assignment.  One wave instruction fills RPI LDS rows (1 KB); lane l fills row
  // RPI*j + l / CPR, slot l % CPR.  Wave w fills A instructions [w*A_INSTR, ...) (weights)
  // and B instructions [w*B_INSTR, ...) (pixels).
  const int lrow = lane / C::CPR;
  const int lslot = lane % C::CPR;
  // weight rows: the swizzle of row (wave*A_INSTR + i)*RPI + lrow depends on i only through its
  // parity, so two offsets + a scalar i*RPI*k_pad cover every piece
  int a_par[2];
  // pixel row i: (ih0, iw0) of tap (0,0) packed as two int16 (ih0 = -16384: no pixel) and the
  // int32 element offset of that tap's chunk (only dereferenced when the tap is inside the
  // image; big_body_shape_ok bounds n*h*w*cin < 2^31 and h, w < 16384)
  uint32_t b_hw[C::B_INSTR];
  int b_off[C::B_INSTR];
  int b2_off[X2 ? C::B_INSTR : 1];   // x2 element offset of the row's chunk (x2 steps)
  const char* zero_src = reinterpret_cast<const char*>(g_zero_page) + lane * 16;
  int s_n = 0, s_oh = 0, s_ow0 = 0;   // STRIP: the tile's image, output row and first column

  auto setup = [&](int px0, int co0) {
    if constexpr (STRIP) {
      s_n = px0 / hw_o;
      const int q = px0 - s_n * hw_o;
      s_oh = q / p.wo;
      s_ow0 = q - s_oh * p.wo;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (wave * C::A_INSTR + i) * C::RPI + lrow;
      a_par[i] = (co0 + r) * p.k_pad + swzb<C::ROWB>(r, lslot) * CE - i * C::RPI * p.k_pad;
    }
    // pixel rows: (ih0, iw0) of tap (0,0) and a base pointer at that tap's chunk (only
    // dereferenced when the tap lies inside the image)
#pragma unroll
    for (int i = 0; i < C::B_INSTR; ++i) {
      const int r = (wave * C::B_INSTR + i) * C::RPI + lrow;
      const int m = px0 + r;
      b_hw[i] = 0xC000C000u;
      b_off[i] = 0;
      if constexpr (X2) b2_off[i] = -1;
      if (m < M) {
        const int n = m / hw_o;
        const int q = m - n * hw_o;
        const int oh = q / p.wo;
        const int ow = q - oh * p.wo;
        const int ih0 = oh * p.stride - p.pad;
        const int iw0 = ow * p.stride - p.pad;
        b_hw[i] = (static_cast<uint32_t>(ih0) << 16) | (static_cast<uint32_t>(iw0) & 0xffffu);
        b_off[i] = ((n * H + ih0) * W + iw0) * cin + swzb<C::ROWB>(r, lslot) * CE;
        if constexpr (X2)
          b2_off[i] = ((n * p.h2 + oh * p.stride2) * p.w2 + ow * p.stride2) * p.cin2 + swzb<C::ROWB>(r, lslot) * CE;
      }
    }
  };

  // K step kt = (channel block cb, tap): taps innermost, so the KS*KS steps that re-read one
  // channel slice of the same pixel neighbourhood run back to back (L2 hits, not MALL).
  struct StepP { int k0, dh, dw; int64_t toff; bool second; };
  auto step_params = [&](int kt) {
    StepP sp;
    sp.second = X2 && kt >= nk1;
    if (sp.second) {                               // x2 step: channels (kt - nk1) * BK of x2
      sp.k0 = KS * KS * cin + (kt - nk1) * BK;
      sp.dh = sp.dw = 0;
      sp.toff = (kt - nk1) * BK;
      return sp;
    }
    const int cb = kt / (KS * KS);
    const int tap = kt - cb * (KS * KS);
    sp.k0 = (tap << lc) + cb * BK;                 // packed weight column: tap * cin + channel
    sp.dh = (tap / KS) * dil;
    sp.dw = (tap - (tap / KS) * KS) * dil;
    sp.toff = (static_cast<int64_t>(sp.dh) * W + sp.dw) * cin + cb * BK;   // uniform over rows
    return sp;
  };
  // one DMA instruction ("piece") of a step: pieces [0, A_INSTR) weights, then pixel rows
  auto issue_piece = [&](const StepP& sp, int stage, int i) {
    if constexpr (STRIP) {                         // A only: B comes as strips
      if (i < C::A_INSTR)
        glds16(wt + (a_par[i & 1] + i * C::RPI * p.k_pad + sp.k0), smem + stage * C::A_BYTES + (wave * C::A_INSTR + i) * 1024);
      return;
    }
    char* sa = smem + stage * C::STAGE;
    if (i < C::A_INSTR) {
      glds16(wt + (a_par[i & 1] + i * C::RPI * p.k_pad + sp.k0), sa + (wave * C::A_INSTR + i) * 1024);
    } else {
      const int j = i - C::A_INSTR;
      const int ih0 = static_cast<int>(b_hw[j]) >> 16;
      const int iw0 = static_cast<int16_t>(b_hw[j] & 0xffffu);
      const bool ok = static_cast<unsigned>(ih0 + sp.dh) < static_cast<unsigned>(H) &&
                      static_cast<unsigned>(iw0 + sp.dw) < static_cast<unsigned>(W);
      const void* src = ok ? static_cast<const void*>(x + (b_off[j] + sp.toff)) : static_cast<const void*>(zero_src);
      if constexpr (X2)
        if (sp.second)
          src = b2_off[j] >= 0 ? static_cast<const void*>(x2 + (b2_off[j] + sp.toff)) : static_cast<const void*>(zero_src);
      glds16(src, sa + C::A_BYTES + (wave * C::B_INSTR + j) * 1024);
    }
  };
  auto issue = [&](int kt, int stage) {
    const StepP sp = step_params(kt);
#pragma unroll
    for (int i = 0; i < C::GLDS; ++i) issue_piece(sp, stage, i);
  };
  // STRIP: share sh (0..4) of the strip of group g = K steps 3g..3g+2 (channel block g / 3, tap
  // row kh = g % 3): strip row R = input pixel (oh - pad + kh dil, ow0 - pad + R), 16-B chunk c
  // at slot c ^ (R & 7) (conflict-free for the 16 consecutive rows of a fragment read at any
  // kw*dil offset)
  const int ngroups = nk / 3;
  auto issue_strip = [&](int g, int sh) {
    const int j = wave + 8 * sh;
    if (j >= kStripPieces) return;                 // wave-uniform
    const int R = j * 8 + lrow;
    const void* src = strip_src<BK, CE>(p, x, g, R, lslot, s_n, s_oh, s_ow0, H, W, cin, dil, zero_src);
    glds16(src, smem + NST * C::A_BYTES + (g & 1) * kStripBytes + j * 1024);
  };


  typename K::acc acc[C::FM][C::FN];
  int tl = blockIdx.x;
  int tile = xcd_remap2(tl, ntiles);
  int px0 = (tile / nco) * kBPX;
  int co0 = (tile % nco) * C::BCO;
  setup(px0, co0);
  // SPARSE: K-step compaction.  A K step whose weight slice (all BCO rows of this tile x BK
  // packed columns) is zero -- a pruned block covering the tile's rows, BlockPruner.py:139-241 --
  // is dropped entirely: no weight DMA, no pixel-row gather, no MFMA.  Lane q holds the K-step
  // id of live position q (lst0) and q + 64 (lst1), built once per tile from two ballots; a
  // position's step is then a readlane (positions are wave-uniform).  nk <= 128 (dispatch).
  int nlive = nk;
  int lst0 = lane, lst1 = lane + 64;
  if constexpr (SPARSE) {
    const int wpr = (p.k_pad + 1023) >> 10;
    auto step_live = [&](int kt) -> bool {
      if (kt >= nk) return false;
      const int u0 = step_params(kt).k0 >> 5;
      bool any = false;
      for (int rb = co0 >> 4; rb < (co0 + C::BCO) >> 4; ++rb)
        any |= ((p.unit_mask[rb * wpr + (u0 >> 5)] >> (u0 & 31)) & ((1u << C::SUB) - 1)) != 0;
      return any;
    };
    const uint64_t b0 = __ballot(step_live(lane)), b1 = __ballot(step_live(lane + 64));
    const int c0 = __popcll(b0), c1 = __popcll(b1);
    nlive = __builtin_amdgcn_readfirstlane(c0 + c1);   // wave-uniform trip count (scalar loop)
    // position q -> K step: the q-th live step of b0, then of b1
    const int q1 = 64 + lane - c0;                       // b1 index of position 64 + lane
    lst0 = lane < c0 ? nth_set_bit(b0, lane) : (lane - c0 < c1 ? 64 + nth_set_bit(b1, lane - c0) : 0);
    lst1 = q1 < c1 ? 64 + nth_set_bit(b1, q1) : 0;
  }
  auto kt_at = [&](int pos) -> int {
    if constexpr (!SPARSE) return pos;
    return pos < 64 ? __builtin_amdgcn_readlane(lst0, pos) : __builtin_amdgcn_readlane(lst1, pos - 64);
  };
  constexpr bool DEFER = NWP < 4;
  if constexpr (K::ESZ == 2) init_tile<C::FM, WCO, C::FN, DEFER>(p, acc, px0, co0, wc, wp, fr, fq);   // residual loads ahead of the DMA
  else zero_tile(acc);
  for (int t = 0; t < NST - 1 && t < nlive; ++t) issue(kt_at(t), t);
  if constexpr (STRIP) {
#pragma unroll
    for (int sh = 0; sh < 5; ++sh) issue_strip(0, sh);
  }

  while (true) {
    // t runs over the (live) K-step positions; kt_at(t) is the K step itself
    for (int t = 0; t < nlive; ++t) {
      const int cur = t % NST;
      // retire step t: the steps issued after it (min(nlive-1, t+NST-2) - t) may stay in flight
      const int newer = ((nlive - 1) < (t + NST - 2) ? (nlive - 1) : (t + NST - 2)) - t;
      if (NST >= 4 && newer >= 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * C::GLDS) : "memory");
      else if (NST >= 3 && newer >= 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(C::GLDS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);

      const char* sa = smem + cur * (STRIP ? C::A_BYTES : C::STAGE);
      const char* sb = STRIP ? smem + NST * C::A_BYTES + ((t / 3) & 1) * kStripBytes : sa + C::A_BYTES;
      const int kwd = STRIP ? (t % 3) * dil : 0;   // STRIP: strip row offset of this step's tap
      // STRIP: this step also issues shares 2 (t % 3), +1 of the next group's strip (clamped: the
      // last group re-fetches its own strip, identical bytes, into the buffer being read)
      const int sg = (t / 3 + 1 < ngroups) ? t / 3 + 1 : ngroups - 1;
      constexpr int GL = STRIP ? C::A_INSTR + 2 : C::GLDS;
      constexpr int NG = NSUB * C::GR;
      constexpr int PPG = (GL + C::GR - 1) / C::GR;   // DMA pieces per group (first substep)
      const StepP sp = step_params(kt_at(t + NST - 1 < nlive ? t + NST - 1 : nlive - 1));
      const int nst = (t + NST - 1) % NST;
      constexpr int PFD = 1;                     // fragment prefetch distance in MFMA groups
      constexpr int NAF = PFD + 1;               // A-fragment ring depth
      typename K::frag af[NAF][C::FPG], bfr[2][C::FN];
      // fp8: the lane group's 32 B of row r -- chunks fq and 4 + fq of a 128-B row, or chunk fq of a
      // 64-B row over zeros (e4m3 +0: those K positions add nothing)
      [[maybe_unused]] auto read_f8 = [&](const char* base, int r) {
        const i32x4 lo = *reinterpret_cast<const i32x4*>(base + r * C::ROWB + swzb<C::ROWB>(r, fq) * 16);
        i32x4 hi = i32x4{0, 0, 0, 0};
        if constexpr (C::ROWB == 128) hi = *reinterpret_cast<const i32x4*>(base + r * C::ROWB + swzb<C::ROWB>(r, 4 + fq) * 16);
        if constexpr (F8) return K::join(lo, hi);
        else return lo;
      };
      auto load_a =[&](typename K::frag (&dst)[C::FPG], int q) {
        const int c = (q / C::GR) * 4 + fq;
#pragma unroll
        for (int h = 0; h < C::FPG; ++h) {
          const int r = wc * WCO + ((q % C::GR) * C::FPG + h) * 16 + fr;
          // unconditional: a branch around an LDS read makes the compiler fall back to lgkmcnt(0)
          if constexpr (F8) dst[h] = read_f8(sa, r);
          else dst[h] = *reinterpret_cast<const typename K::frag*>(sa + r * C::ROWB + swzb<C::ROWB>(r, c) * 16);
        }
      };
      auto load_b = [&](typename K::frag (&dst)[C::FN], int sub) {
        const int c = sub * 4 + fq;
#pragma unroll
        for (int fn = 0; fn < C::FN; ++fn) {
          const int r = wp * C::PXW + fn * 16 + fr;
          if constexpr (F8) {
            dst[fn] = read_f8(sb, r);
          } else if constexpr (STRIP) {
            const int R = r + kwd;
            dst[fn] = *reinterpret_cast<const typename K::frag*>(sb + R * C::ROWB + (c ^ (R & 7)) * 16);
          } else {
            dst[fn] = *reinterpret_cast<const typename K::frag*>(sb + r * C::ROWB + swzb<C::ROWB>(r, c) * 16);
          }
        }
      };
      load_b(bfr[0], 0);
#pragma unroll
      for (int q = 0; q < PFD && q < NG; ++q) {
        load_a(af[q % NAF], q);
        if (q > 0 && q % C::GR == 0) load_b(bfr[(q / C::GR) & 1], q / C::GR);
      }
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        // group q's fragments (issued a group ago) land before the next reads go out, so the
        // compiler's wait in front of the MFMAs does not also cover the fresh reads
        // (s_waitcnt lgkmcnt(0) with vmcnt/expcnt at their maxima: LDS-DMA stays in flight)
        if (q + PFD < NG) {
          load_a(af[(q + PFD) % NAF], q + PFD);
          if ((q + PFD) % C::GR == 0) load_b(bfr[((q + PFD) / C::GR) & 1], (q + PFD) / C::GR);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < C::FPG; ++h) {
#pragma unroll
          for (int fn = 0; fn < C::FN; ++fn)
            acc[(q % C::GR) * C::FPG + h][fn] = K::mma(
                af[q % NAF][h], bfr[(q / C::GR) & 1][fn], acc[(q % C::GR) * C::FPG + h][fn]);
        }
        if (q < C::GR) {
#pragma unroll
          for (int k = 0; k < PPG; ++k)
            if constexpr (STRIP) {
              const int i = q * PPG + k;
              if (i < C::A_INSTR) issue_piece(sp, nst, i);
              else if (i < GL) issue_strip(sg, 2 * (t % 3) + (i - C::A_INSTR));
            } else {
              if (q * PPG + k < C::GLDS) issue_piece(sp, nst, q * PPG + k);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // --- next tile: its first DMA steps go out before this tile's epilogue
    const int cur_px0 = px0, cur_co0 = co0;
    bool more = false;
    if constexpr (PERSIST) {
      tl += gridDim.x;
      more = tl < ntiles;
      if (more) {
        tile = xcd_remap2(tl, ntiles);
        px0 = (tile / nco) * kBPX;
        co0 = (tile % nco) * C::BCO;
        // every wave done with the ring, and the clamped re-fetches have landed
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        setup(px0, co0);
        for (int t = 0; t < NST - 1 && t < nk; ++t) issue(t, t);
      }
    }

    if constexpr (K::ESZ == 2) {
      // whole tile inside a dense bf16 NHWC output: 16-B stores (conv_tile.h store_tile_x4)
      bool x4 = false;
      if constexpr (!DEFER && C::FM % 2 == 0)
        x4 = p.scale == nullptr && p.out_dtype == DRNMI_BF16 && p.y_sc == 1 && p.y_sp == p.cout &&
             p.y_sn == static_cast<int64_t>(p.ho) * p.wo * p.cout && cur_px0 + kBPX <= p.n * p.ho * p.wo &&
             cur_co0 + C::BCO <= p.cout;
      if (x4) store_tile_x4<C::FM, WCO, C::FN>(p, acc, cur_px0, cur_co0, wc, wp, fr, fq);
      else store_tile<C::FM, WCO, C::FN, DEFER>(p, acc, cur_px0, cur_co0, wc, wp, fr, fq);
    } else {
      // whole tile inside a dense 8-bit NHWC output of the code's own type: 16-B pieces.  The terms
      // of q8_dense_x4 with the whole-tile test between them, each code's guard (conv_tile.h Q8,
      // CHECKS_ALIGNMENT) where that code has always evaluated it
      using Q = Q8<T>;
      const bool x4 = C::FM % 4 == 0 && p.out_dtype == Q::OUT && p.y_sc == 1 && p.y_sp == p.cout &&
          p.y_sn == static_cast<int64_t>(p.ho) * p.wo * p.cout &&
          (Q::CHECKS_ALIGNMENT ? ((reinterpret_cast<uintptr_t>(p.y) | reinterpret_cast<uintptr_t>(p.res)) & 15) == 0 : true) &&
          cur_px0 + kBPX <= p.n * p.ho * p.wo && cur_co0 + C::BCO <= p.cout &&
          (Q::CHECKS_ALIGNMENT ? true : (p.res == nullptr || p.cout % 16 == 0));
      if (x4) store_tile_q8_x4<T, C::FM, WCO, C::FN>(p, acc, cur_px0, cur_co0, wc, wp, fr, fq);
      else store_tile_q8<T, C::FM, WCO, C::FN>(p, acc, cur_px0, cur_co0, wc, wp, fr, fq);
    }
    if (!more) break;
    if constexpr (K::ESZ == 2) init_tile<C::FM, WCO, C::FN, DEFER>(p, acc, px0, co0, wc, wp, fr, fq);
    else zero_tile(acc);
  }
}

}  // namespace
}  // namespace drnmi
