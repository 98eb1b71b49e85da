// Three-product split-bf16 NHWC implicit-GEMM convolution ("fp32x2" precision mode, DRNMI_F32X2).
//
// Every fp32 operand is split in two bf16 terms, x = x1 + x2 + r with x1 = bf16(x),
// x2 = bf16(x - x1) and |r| <= 2^-17 |x| (common.h split2), and the product keeps the three terms
// above 2^-16 of the leading one,
//     x*w ~ x1 w2 + x2 w1 + x1 w1         (smallest first, common.h mfma_x3)
// in v_mfma_f32_16x16x32_bf16 with fp32 accumulation: half the MFMA work of conv_x6's six products,
// two weight planes instead of three, about 16 significant bits per product.
//
// Launch contract: conv_x6's (cin >= 32 and a power of two, ks 1 / 2 / 3, any stride / dilation,
// ragged tiles, scale / shift / residual / ReLU in fp32, strided NCHW or row-strided NHWC output,
// split-K through the caller's workspace, BN-statistics partials), on weights [2][cout_pad][k_pad].
//
// What differs from conv_x6 is the pipeline.  With three MFMAs per product the per-step costs that
// do not shrink (the barrier, the DMA issue, the fp32 B rows read from LDS and their split) weigh
// twice as much, so the ring here moves in *pairs* of 32-channel sub-steps:
//   * a ring slot holds SUB sub-stages, each one sub-step's operands: two weight planes (BCO rows
//     x 64 B) and BPX fp32 pixel rows (128 B), swizzled as in conv_x6.  SUB = 2: one barrier, one
//     vmcnt wait and one burst of LDS-DMA issue per 64 input channels.  The two sub-steps of a
//     pair are decoded on their own (tap, channel block), so a pair may straddle a tap (cin 32)
//     and an odd count leaves the last pair half full.  The two-plane A stage is what makes the
//     pair fit: 2 slots x 2 x (16 KB + 16 KB) = 128 KB for the 128 x 128 tile.
//   * the whole next pair is requested right after the barrier, before any LDS read of the current
//     one, so the DMA has a full pair of MFMA time (96 MFMAs per wave) to land; nothing is issued
//     inside the MFMA groups.
//   * per sub-step a wave reads its four B fragments once, splits them once (split2: two
//     conversions and one subtraction per pair) and runs FM x 12 MFMAs on them; the two A planes of
//     fragment fm + 1 are read into a second register pair while fragment fm's twelve MFMAs run.
//   * SUB = 1 forms (one sub-step per slot) are the small-LDS tiles that fit two workgroups per CU.
// Measured, two resident workgroups beat the 64-channel step on every fine-tune shape, so
// the default route takes the SUB = 1 tiles and the SUB = 2 tile is a forced variant.
// Every variant runs each accumulator through the same sequence (sub-steps in K order, mfma_x3's
// order inside one), so all variants are bit-identical, and a split-K partition starts on a
// sub-step boundary whatever SUB is.
#include "conv_xsplit.h"

namespace drnmi {
namespace {

// Tile = BCO = WCO x WC output channels x BPX = 64 x PS pixels; one wave per (channel column,
// 64-pixel slice); SUB sub-steps of 32 channels per ring slot.
template <int WCO, int WC, int PS, int SUB>
struct X3Cfg : XCfg<2, WCO, WC, PS> {
  using B = XCfg<2, WCO, WC, PS>;
  static constexpr int OCC = SUB == 1 ? 2 : 1;      // workgroups per CU the LDS ring is sized for
  static constexpr int SUBST = B::A_BYTES + B::B_BYTES;   // one sub-step's operands
  static constexpr int STAGE = SUB * SUBST;
  static constexpr int NST = (SUB == 1 && 3 * STAGE * OCC <= 160 * 1024) ? 3 : 2;
  static constexpr int LDS = NST * STAGE;
  static_assert(LDS * OCC <= 160 * 1024, "LDS");
  static_assert(SUB == 1 || NST == 2, "a half-full last pair is waited for with vmcnt(0)");
  static_assert(B::GLDS * (NST - 1) < 64, "vmcnt");
};

template <int KS, int WCO, int WC, int PS, int SUB>
__global__ void __launch_bounds__(64 * PS * WC, SUB == 1 ? 2 : 1)   // X3Cfg::OCC
conv_x3_kernel(const drnmi_conv_args p) {
  using C = X3Cfg<WCO, WC, PS, SUB>;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wc = wave / PS;          // channel column of the tile
  const int wp = wave % PS;          // 64-pixel slice of the tile
  const int fr = lane & 15;
  const int fq = lane >> 4;
  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int nco = (p.cout + C::BCO - 1) / C::BCO;
  const int npx = (M + C::BPX - 1) / C::BPX;
  const int tile = xcd_remap(blockIdx.x, npx * nco);
  const int px0 = (tile / nco) * C::BPX;
  const int co0 = (tile % nco) * C::BCO;

  const int cin = p.cin;
  const int lc = 31 - __builtin_clz(cin);
  const int H = p.h, W = p.w, dil = p.dil;
  const float* __restrict__ x = reinterpret_cast<const float*>(p.x);
  const uint16_t* __restrict__ wt = reinterpret_cast<const uint16_t*>(p.wgt);
  const int64_t plane_stride = static_cast<int64_t>(p.cout_pad) * p.k_pad;
  // split-K (gridDim.y > 1, drnmi_conv_args.ws): this workgroup runs sub-steps [s0, s0 + ns)
  const int ns_all = p.k_pad / kBK;
  const int s0 = static_cast<int>(static_cast<int64_t>(ns_all) * blockIdx.y / gridDim.y);
  const int ns = static_cast<int>(static_cast<int64_t>(ns_all) * (blockIdx.y + 1) / gridDim.y) - s0;
  const int nk = (ns + SUB - 1) / SUB;                 // ring steps
  const char* zero_src = reinterpret_cast<const char*>(g_xsplit_zero) + lane * 16;

  // --- A pieces: 16 rows of 64 B each; linear row R = plane * BCO + r
  // element offsets < 2^31: 2 planes x cout_pad x k_pad bf16 (conv_route.cpp x6_route checks)
  int32_t a_off[C::A_PW];
#pragma unroll
  for (int i = 0; i < C::A_PW; ++i) {
    const int R = (wave * C::A_PW + i) * 16 + (lane >> 2);
    const int pl = R / C::BCO, r = R - pl * C::BCO;
    a_off[i] = static_cast<int32_t>(pl * plane_stride + static_cast<int64_t>(co0 + r) * p.k_pad + swz64(r, lane & 3) * 8);
  }
  // --- B pieces: 8 pixel rows of 128 B; (ih0, iw0) of tap (0,0) and the element offset of the
  // row's chunk at that tap (only dereferenced when the tap is inside the image)
  int b_ih[C::B_PW], b_iw[C::B_PW], b_off[C::B_PW];
#pragma unroll
  for (int j = 0; j < C::B_PW; ++j) {
    const int r = (wave * C::B_PW + j) * 8 + (lane >> 3);
    const int m = px0 + r;
    b_ih[j] = -(1 << 28);
    b_iw[j] = -(1 << 28);
    b_off[j] = 0;
    if (m < M) {
      const int n = m / hw_o;
      const int q = m - n * hw_o;
      const int oh = q / p.wo;
      const int ow = q - oh * p.wo;
      b_ih[j] = oh * p.stride - p.pad;
      b_iw[j] = ow * p.stride - p.pad;
      b_off[j] = ((n * H + b_ih[j]) * W + b_iw[j]) * cin + swz128(r, lane & 7) * 4;
    }
  }

  // the DMA of sub-step u of this workgroup into the sub-stage at `sa`
  auto issue_sub = [&](int u, char* sa) {
    const int kt = s0 + u;
    const int cb = kt / (KS * KS);
    const int tap = kt - cb * (KS * KS);
    const int k0 = (tap << lc) + cb * kBK;
    const int dh = (tap / KS) * dil;
    const int dw = (tap - (tap / KS) * KS) * dil;
    const int toff = (dh * W + dw) * cin + cb * kBK;
#pragma unroll
    for (int i = 0; i < C::A_PW; ++i)
      glds16(wt + (static_cast<uint32_t>(a_off[i]) + k0), sa + (wave * C::A_PW + i) * 1024);
#pragma unroll
    for (int j = 0; j < C::B_PW; ++j) {
      const bool ok = static_cast<unsigned>(b_ih[j] + dh) < static_cast<unsigned>(H) &&
                      static_cast<unsigned>(b_iw[j] + dw) < static_cast<unsigned>(W);
      const void* src = ok ? static_cast<const void*>(x + (b_off[j] + toff)) : static_cast<const void*>(zero_src);
      glds16(src, sa + C::A_BYTES + (wave * C::B_PW + j) * 1024);
    }
  };
  // ring step t: its SUB sub-steps (the last one may hold fewer) into slot `slot`
  auto issue = [&](int t, int slot) {
#pragma unroll
    for (int h = 0; h < SUB; ++h)
      if (t * SUB + h < ns) issue_sub(t * SUB + h, smem + slot * C::STAGE + h * C::SUBST);
  };

  f32x4 acc[C::FM][C::FN];
#pragma unroll
  for (int i = 0; i < C::FM; ++i)
#pragma unroll
    for (int j = 0; j < C::FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint32_t a_lane = static_cast<uint32_t>((wc * WCO + fr) * 64 + swz64(fr, fq) * 16);
  const uint32_t b_lane0 = static_cast<uint32_t>(C::A_BYTES + (wp * 64 + fr) * 128 + swz128(fr, 2 * fq) * 16);
  const uint32_t b_lane1 = static_cast<uint32_t>(C::A_BYTES + (wp * 64 + fr) * 128 + swz128(fr, 2 * fq + 1) * 16);

  // one sub-step from the sub-stage at LDS byte `sb`.  The fragment reads are inline-asm
  // ds_read_b128 (common.h ds_rd); each wait names the registers it waits for as in-out operands,
  // so no use of them can move above it.  Rows 16 apart keep both swizzles, so fragment fm / fn
  // is a constant added to the lane's address.
  auto sub_step = [&](uint32_t sb) {
    const uint32_t va = a_lane + sb, vb0 = b_lane0 + sb, vb1 = b_lane1 + sb;
    bf16x8 a[2][2];                     // [register pair][plane]
    f32x4 blo[C::FN], bhi[C::FN];
    ds_rd<0>(a[0][1], va + C::A_PLANE);
    ds_rd<0>(a[0][0], va);
#pragma unroll
    for (int fn = 0; fn < C::FN; ++fn) {
      ds_rd<0>(blo[fn], vb0 + fn * 2048);
      ds_rd<0>(bhi[fn], vb1 + fn * 2048);
    }
    static_assert(C::FN == 4, "four B fragments");
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(blo[0]), "+v"(bhi[0]), "+v"(blo[1]), "+v"(bhi[1]), "+v"(blo[2]), "+v"(bhi[2]), "+v"(blo[3]),
                   "+v"(bhi[3]), "+v"(a[0][0]), "+v"(a[0][1])
                 :
                 : "memory");
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 b[C::FN][2];
#pragma unroll
    for (int fm = 0; fm < C::FM; ++fm) {
      const int cur = fm & 1, nxt = cur ^ 1;
      if (fm + 1 < C::FM) {
        ds_rd<0>(a[nxt][1], va + (fm + 1) * 1024 + C::A_PLANE);
        ds_rd<0>(a[nxt][0], va + (fm + 1) * 1024);
      }
      __builtin_amdgcn_sched_barrier(0);
      // mfma_x3's order per accumulator, issued across the four pixel fragments so that
      // back-to-back MFMAs are independent; fragment 0's first group runs on each B fragment as
      // its split is done, so the split of the next one hides under an MFMA
#pragma unroll
      for (int fn = 0; fn < C::FN; ++fn) {
        if (fm == 0) {
          split2(make_float4(blo[fn].x, blo[fn].y, blo[fn].z, blo[fn].w),
                 make_float4(bhi[fn].x, bhi[fn].y, bhi[fn].z, bhi[fn].w), b[fn][0], b[fn][1]);
        }
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[cur][1], b[fn][0], acc[fm][fn], 0, 0, 0);
        if (fm == 0) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int fn = 0; fn < C::FN; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[cur][0], b[fn][1], acc[fm][fn], 0, 0, 0);
#pragma unroll
      for (int fn = 0; fn < C::FN; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[cur][0], b[fn][0], acc[fm][fn], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (fm + 1 < C::FM) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[nxt][0]), "+v"(a[nxt][1]) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  for (int t = 0; t < C::NST - 1 && t < nk; ++t) issue(t, t);

  for (int t = 0; t < nk; ++t) {
    // the DMA groups in flight are those of steps t .. min(nk - 1, t + NST - 2): step t's has landed
    // once at most the newer ones are outstanding
    const int newer = ((nk - 1) < (t + C::NST - 2) ? (nk - 1) : (t + C::NST - 2)) - t;
    if (C::NST >= 3 && newer >= 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(C::GLDS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // every wave's pieces of step t have landed and every wave has read the last of step t - 1
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (t + C::NST - 1 < nk) issue(t + C::NST - 1, (t + C::NST - 1) % C::NST);   // into step t - 1's slot
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t st_off = static_cast<uint32_t>((t % C::NST) * C::STAGE);
#pragma unroll
    for (int h = 0; h < SUB; ++h)
      if (t * SUB + h < ns) sub_step(st_off + h * C::SUBST);
  }

  // --- split-K: raw fp32 partial sums [split][m][cout]; conv_x6's finish kernel adds them
  if (gridDim.y > 1) {
    float* __restrict__ part = reinterpret_cast<float*>(p.ws) + static_cast<int64_t>(blockIdx.y) * M * p.cout;
#pragma unroll
    for (int fn = 0; fn < C::FN; ++fn) {
      const int m = px0 + wp * 64 + fn * 16 + fr;
      if (m >= M) continue;
#pragma unroll
      for (int fm = 0; fm < C::FM; ++fm) {
        const int co = co0 + wc * WCO + fm * 16 + fq * 4;
        if (co >= p.cout) continue;
        float* q = part + static_cast<int64_t>(m) * p.cout + co;
        if (co + 3 < p.cout) {
          *reinterpret_cast<float4*>(q) = make_float4(acc[fm][fn][0], acc[fm][fn][1], acc[fm][fn][2], acc[fm][fn][3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (co + j < p.cout) q[j] = acc[fm][fn][j];
        }
      }
    }
    return;
  }

  // --- epilogue (conv_x6's contract): lane owns channels co..co+3 of pixel m, fp32
  const float* __restrict__ res = reinterpret_cast<const float*>(p.res);
  const bool nhwc = p.y_sc == 1;
  int64_t ybase_fn[C::FN];          // the lane's output row offsets (-1: past the last pixel)
#pragma unroll
  for (int fn = 0; fn < C::FN; ++fn) {
    const int m = px0 + wp * 64 + fn * 16 + fr;
    const int n = m / hw_o;
    const int q = m - n * hw_o;
    const int64_t qo = p.y_sr != 0 ? static_cast<int64_t>(q / p.wo) * p.y_sr + static_cast<int64_t>(q % p.wo) * p.y_sp
                                   : static_cast<int64_t>(q) * p.y_sp;
    ybase_fn[fn] = m < M ? static_cast<int64_t>(n) * p.y_sn + qo : -1;
  }
  // v = acc * scale + shift (+ res), ReLU, stored; false when the pixel or the channel group lies
  // outside the output
  auto epi = [&](int fm, int fn, float (&v)[4]) -> bool {
    const int m = px0 + wp * 64 + fn * 16 + fr;
    const int co = co0 + wc * WCO + fm * 16 + fq * 4;
    const int64_t ybase = ybase_fn[fn];
    if (ybase < 0 || co >= p.cout) return false;
    const bool full = co + 3 < p.cout;
    const float4 sh = *reinterpret_cast<const float4*>(p.shift + co);   // padded to cout_pad
    const float shv[4] = {sh.x, sh.y, sh.z, sh.w};
    if (p.scale != nullptr) {
      const float4 sc = *reinterpret_cast<const float4*>(p.scale + co);
      const float scv[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = acc[fm][fn][j] * scv[j] + shv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = acc[fm][fn][j] + shv[j];
    }
    if (res != nullptr) {
      const float* rp = res + (p.y_sr != 0 ? ybase : static_cast<int64_t>(m) * p.cout) + co;   // y_sr: y's layout
      if (full) {
        const float4 rv = *reinterpret_cast<const float4*>(rp);
        v[0] += rv.x;
        v[1] += rv.y;
        v[2] += rv.z;
        v[3] += rv.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (co + j < p.cout) v[j] += rp[j];
      }
    }
    if (p.relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    float* y = reinterpret_cast<float*>(p.y);
    if (nhwc && full) {
      *reinterpret_cast<float4*>(y + ybase + co) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (co + j < p.cout) y[ybase + static_cast<int64_t>(co + j) * p.y_sc] = v[j];
    }
    return true;
  };
  if (p.stats == nullptr) {
#pragma unroll
    for (int fn = 0; fn < C::FN; ++fn)
#pragma unroll
      for (int fm = 0; fm < C::FM; ++fm) {
        float v[4];
        epi(fm, fn, v);
      }
    return;
  }
  // BN statistics of the stored values (drnmi_conv_args.stats), conv_x6's layout: row g = this
  // wave's 64-pixel slice, [2][G][cout] (sums, then sums of squares), fp64, fixed order
  const int G = npx * PS;
  const int g = (tile / nco) * PS + wp;
#pragma unroll
  for (int fm = 0; fm < C::FM; ++fm) {
    double a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
#pragma unroll
    for (int fn = 0; fn < C::FN; ++fn) {
      float v[4];
      if (epi(fm, fn, v)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a1[j] += static_cast<double>(v[j]);
          a2[j] += static_cast<double>(v[j]) * v[j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a1[j] = row16_sum(a1[j]);
      a2[j] = row16_sum(a2[j]);
    }
    const int co = co0 + wc * WCO + fm * 16 + fq * 4;
    if (fr == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (co + j < p.cout) {
          p.stats[static_cast<int64_t>(g) * p.cout + co + j] = a1[j];
          p.stats[static_cast<int64_t>(G + g) * p.cout + co + j] = a2[j];
        }
    }
  }
}

}  // namespace

// variants: 0 <K, 64, 2, 2, 2> (128 channels x 128 pixels, 4 waves of 64 x 64, 64-channel ring steps,
// one workgroup per CU; a forced variant), 1 <K, 64, 2, 2, 1> (the same tile on 32-channel steps in
// 64 KB, two workgroups per CU: the default where cout % 128 == 0), 2 <K, 32, 2, 2, 1> (64 x 128, 4 waves
// of 32 x 64, three 24-KB stages, two per CU: the default below, down to the 19-class seg).  step: seconds
// per 32-channel sub-step of one workgroup tile and round of resident workgroups, from the 3x3 512 -> 512
// launch at 2 x 128 x 96 in an earlier run of scripts/x3_micro.py than the committed one: 445 us / (3 rounds x
// 144), 369 / (2 x 144), 494 / (3 x 144); profiles/fp32x2/micro_conv.log has 443 / 349 / 475 us, within 6 %.
#define X3_VARIANT(WCO, WC, PS, SUB, STEP) X_VARIANT(conv_x3_kernel, X3Cfg, STEP, WCO, WC, PS, SUB)
const X6Variant& x3_variant(int v) {
  static const X6Variant k[kNumX3] = {X3_VARIANT(64, 2, 2, 2, 1.0e-6), X3_VARIANT(64, 2, 2, 1, 1.3e-6),
                                      X3_VARIANT(32, 2, 2, 1, 1.15e-6)};
  return k[v];
}
#undef X3_VARIANT

// conv_x6's launch contract under the other dtype code
bool x3_conv_supported(const drnmi_conv_args& p) {
  if (p.dtype != DRNMI_F32X2) return false;
  drnmi_conv_args q = p;
  q.dtype = DRNMI_F32X3;
  return x6_conv_supported(q);
}

}  // namespace drnmi
