// 2:4 weight-sparse NHWC implicit-GEMM convolution, bf16, on v_smfmac_f32_16x16x64_bf16
// (dtype DRNMI_BF16_SP24, include/drnmi.h: inference, opt-in through DRNSeg.set_sparse24).
//
// conv_big.hip's per-tap gather with the sparse MFMA in place of two dense ones: A = weights with at
// most two non-zeros in every four consecutive input channels of a tap, stored compressed (the kept
// values + 2-bit positions, drnmi_sp24_pack), B = pixels, dense.  conv_sp24_body is a main loop of its
// own, written out next to conv_big_body (conv_big_body.h): as one template over a fourth element type the
// sparse kernels lost their schedule (profiles/sp24_fold/README.txt).  From conv_tile.h, one copy for both:
// the swizzles, glds16 / glds4, the XCD-major tile deal, the strip source (strip_src), the strip geometry,
// init_tile / store_tile / store_tile_x4.  Built with VGPR-form MFMAs (build.py).
//
// Operand map of the instruction (measured, tests/test_gpu_sp24.py::test_operand_map), lane = 16 fq + fr:
//   A  lane holds row fr's 8 kept values of dense k 16 fq .. 16 fq + 15: slots (2 g, 2 g + 1) are the
//      kept pair of group g = k 16 fq + 4 g .. + 3, in ascending position;
//   idx bits [2 s + 1 : 2 s] of the 16-bit half ABID selects = slot s's position inside its group;
//   B  lane holds column fr's k 8 fq .. 8 fq + 7 (elements 0-7) and 32 + 8 fq .. + 7 (elements 8-15):
//      two v_mfma_f32_16x16x32_bf16 B fragments side by side;
//   D  as the dense 16x16 MFMAs: lane holds rows 4 fq .. 4 fq + 3 of column fr.
//
// K step = 64 dense channels of one tap.  LDS image of a stage (3 stages):
//   A values  BCO rows x 64 B (32 kept values in channel order), 16-B chunk c of row r at slot
//             swzb<64>(r, c): lane (fr, fq) reads chunk fq, the 64-B-row fragment read of conv_big's
//             BK-32 tiles, conflict-free for the reason given at swzb;
//   A index   BCO / 32 blocks of 64 words: word 16 fq + fr of block f2 holds the 16 index bits of row
//             32 f2 + fr (low half) and of row 32 f2 + 16 + fr (high half) for k 16 fq .. + 15, so a
//             wave reads 64 consecutive words (one ds_read_b32 per fragment pair: no two lanes of a
//             32-lane half on one bank) and the pair's two MFMAs take ABID 0 and 1 of one register;
//   B         256 pixel rows x 128 B with conv_big's 128-B swizzle: lane (fr, fq) reads chunks fq and
//             4 + fq, the dense kernel's two conflict-free substep reads, as one 32-B fragment.
// 256 x 256 tile (8 waves): 16 + 2 + 32 KB per stage; 128 x 256 (4 waves): 8 + 1 + 32 KB.
// The blob (private to this file): the value plane [cout_pad][k_pad / 2] bf16, then the index plane
// [cout_pad / 32][k_pad / 64][64] words in the LDS order above, so a K step's index block of 32 rows
// is one 256-B DMA (global_load_lds_dword) by the wave with that number.
#include "common.h"
#include "conv_tile.h"
#include "kernels.h"

namespace drnmi {
namespace {

typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

template <int WCO, int WC>
struct Sp24Cfg {
  static constexpr int BK = 64;                     // dense channels per K step
  static constexpr int NST = 3;
  static constexpr int BCO = WCO * WC;
  static constexpr int FM = WCO / 16;
  static constexpr int FN = 4;
  static constexpr int NW = 4 * WC;
  static constexpr int THREADS = 64 * NW;
  static constexpr int A_BYTES = BCO * 64;          // kept values: 64-B rows
  static constexpr int I_BYTES = BCO * 8;           // positions: 2 bits per kept value
  static constexpr int B_BYTES = kBPX * 128;
  static constexpr int STAGE = A_BYTES + I_BYTES + B_BYTES;
  static constexpr int A_INSTR = BCO / 16 / NW;     // 1-KB pieces (16 rows) per wave per step
  static constexpr int B_INSTR = kBPX / 8 / NW;     // 1-KB pieces (8 rows)
  static constexpr int GLDS = A_INSTR + 1 + B_INSTR;
  static constexpr int LDS = NST * STAGE;
  static constexpr int GR = FM / 2;                 // MFMA groups per step: one fragment pair each
  static_assert(BCO / 32 == NW, "one 32-row index block per wave");
  static_assert(LDS <= 160 * 1024, "LDS");
};

// STRIP (3x3 stride 1, wo % 256 == 0, the 256 x 256 tile): conv_big's strip-staged B.  The three kw taps
// of one (64-channel block, kh) read one strip of 256 + 2 dil pixel rows at row offset kw * dil, staged
// once per three K steps into one of two strip buffers (conv_tile.h kStripBytes) in five shares per wave;
// A (values + index) rides a two-stage ring and every step waits for all of its DMA, as conv_strip_kernel.
// Same K order and MFMAs as the gather form: bit-identical.
template <int KS, int WCO, int WC, bool STRIP = false>
__device__ __forceinline__ void conv_sp24_body(const drnmi_conv_args& p) {
  using C = Sp24Cfg<WCO, WC>;
  constexpr int NST = STRIP ? 2 : C::NST, BK = C::BK;
  static_assert(!STRIP || (KS == 3 && C::NW == 8), "strip mode: the 256 x 256 3x3 tile");
  constexpr int STAGE = STRIP ? C::A_BYTES + C::I_BYTES : C::STAGE;   // strip: the ring holds A only
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wc = wave / 4;
  const int wp = wave % 4;
  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int nco = (p.cout + C::BCO - 1) / C::BCO;
  const int npx = (M + kBPX - 1) / kBPX;
  const int ntiles = npx * nco;

  const int cin = p.cin;
  const int lc = 31 - __builtin_clz(cin);
  const int H = p.h, W = p.w, dil = p.dil;
  const uint16_t* __restrict__ x = reinterpret_cast<const uint16_t*>(p.x);
  const int kh2 = p.k_pad / 2;                      // kept values per weight row
  const int nk = p.k_pad / BK;
  const uint16_t* __restrict__ vals = reinterpret_cast<const uint16_t*>(p.wgt);
  const uint32_t* __restrict__ idxp = reinterpret_cast<const uint32_t*>(vals + static_cast<int64_t>(p.cout_pad) * kh2);
  const int fr = lane & 15;
  const int fq = lane >> 4;

  const int tile = xcd_remap2(blockIdx.x, ntiles);
  const int px0 = (tile / nco) * kBPX;
  const int co0 = (tile % nco) * C::BCO;

  // --- DMA assignment.  A values: lane l fills row l / 4, slot l % 4 of a 16-row piece; index: the
  // wave's own 32-row block, lane l its word l; pixels: row l / 8, slot l % 8 of an 8-row piece
  int a_off[C::A_INSTR];
#pragma unroll
  for (int i = 0; i < C::A_INSTR; ++i) {
    const int r = (wave * C::A_INSTR + i) * 16 + (lane >> 2);
    a_off[i] = (co0 + r) * kh2 + swzb<64>(r, lane & 3) * 8;
  }
  const int i_off = ((co0 >> 5) + wave) * nk * 64 + lane;
  // pixel rows as conv_big: (ih0, iw0) of tap (0,0) as two int16 and the element offset of that tap's chunk
  uint32_t b_hw[C::B_INSTR];
  int b_off[C::B_INSTR];
  const char* zero_src = reinterpret_cast<const char*>(g_zero_page) + lane * 16;
#pragma unroll
  for (int i = 0; i < C::B_INSTR; ++i) {
    const int r = (wave * C::B_INSTR + i) * 8 + (lane >> 3);
    const int m = px0 + r;
    b_hw[i] = 0xC000C000u;
    b_off[i] = 0;
    if (m < M) {
      const int n = m / hw_o;
      const int q = m - n * hw_o;
      const int oh = q / p.wo;
      const int ow = q - oh * p.wo;
      const int ih0 = oh * p.stride - p.pad;
      const int iw0 = ow * p.stride - p.pad;
      b_hw[i] = (static_cast<uint32_t>(ih0) << 16) | (static_cast<uint32_t>(iw0) & 0xffffu);
      b_off[i] = ((n * H + ih0) * W + iw0) * cin + swzb<128>(r, lane & 7) * 8;
    }
  }

  // K step kt = (channel block cb, tap), taps innermost (conv_big)
  struct StepP { int k0, dh, dw; int64_t toff; };
  auto step_params = [&](int kt) {
    StepP sp;
    const int cb = kt / (KS * KS);
    const int tap = kt - cb * (KS * KS);
    sp.k0 = (tap << lc) + cb * BK;                 // packed weight column: tap * cin + channel
    sp.dh = (tap / KS) * dil;
    sp.dw = (tap - (tap / KS) * KS) * dil;
    sp.toff = (static_cast<int64_t>(sp.dh) * W + sp.dw) * cin + cb * BK;
    return sp;
  };
  // pieces [0, A_INSTR) kept values, A_INSTR the index block, then pixel rows
  auto issue_piece = [&](const StepP& sp, int stage, int i) {
    char* sa = smem + stage * STAGE;
    if (i < C::A_INSTR) {
      glds16(vals + (a_off[i] + (sp.k0 >> 1)), sa + (wave * C::A_INSTR + i) * 1024);
    } else if (i == C::A_INSTR) {
      glds4(idxp + (i_off + (sp.k0 >> 6) * 64), sa + C::A_BYTES + wave * 256);
    } else if constexpr (!STRIP) {
      const int j = i - C::A_INSTR - 1;
      const int ih0 = static_cast<int>(b_hw[j]) >> 16;
      const int iw0 = static_cast<int16_t>(b_hw[j] & 0xffffu);
      const bool ok = static_cast<unsigned>(ih0 + sp.dh) < static_cast<unsigned>(H) &&
                      static_cast<unsigned>(iw0 + sp.dw) < static_cast<unsigned>(W);
      const void* src = ok ? static_cast<const void*>(x + (b_off[j] + sp.toff)) : static_cast<const void*>(zero_src);
      glds16(src, sa + C::A_BYTES + C::I_BYTES + (wave * C::B_INSTR + j) * 1024);
    }
  };

  // STRIP: share sh (0..4) of the strip of group g = K steps 3 g .. 3 g + 2 (channel block g / 3, tap row
  // kh = g % 3): strip row R = input pixel (oh - pad + kh dil, ow0 - pad + R), 16-B chunk c at slot
  // c ^ (R & 7), conv_big's strip image
  const int s_n = px0 / hw_o;
  const int s_oh = (px0 - s_n * hw_o) / p.wo;
  const int s_ow0 = px0 - s_n * hw_o - s_oh * p.wo;
  const int ngroups = nk / 3;
  char* strips = smem + NST * STAGE;
  auto issue_strip = [&](int g, int sh) {
    const int j = wave + 8 * sh;
    if (j >= kStripPieces) return;                 // wave-uniform
    const int R = j * 8 + (lane >> 3);
    const void* src = strip_src<BK, 8>(p, x, g, R, lane & 7, s_n, s_oh, s_ow0, H, W, cin, dil, zero_src);
    glds16(src, strips + (g & 1) * kStripBytes + j * 1024);
  };
  constexpr int GL = STRIP ? C::A_INSTR + 1 + 2 : C::GLDS;   // pieces a wave issues per step (strip: + two strip shares)

  f32x4 acc[C::FM][C::FN];
  init_tile<C::FM, WCO, C::FN>(p, acc, px0, co0, wc, wp, fr, fq);   // shift + residual (scale is NULL)
  for (int t = 0; t < NST - 1 && t < nk; ++t) {
    const StepP sp = step_params(t);
#pragma unroll
    for (int i = 0; i < (STRIP ? C::A_INSTR + 1 : C::GLDS); ++i) issue_piece(sp, t, i);
  }
  if constexpr (STRIP) {
#pragma unroll
    for (int sh = 0; sh < 5; ++sh) issue_strip(0, sh);
  }

  for (int t = 0; t < nk; ++t) {
    const int cur = t % NST;
    // retire step t: the step issued after it may stay in flight
    const int newer = ((nk - 1) < (t + NST - 2) ? (nk - 1) : (t + NST - 2)) - t;
    if (!STRIP && newer >= 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(C::GLDS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);

    const char* sa = smem + cur * STAGE;
    const char* si = sa + C::A_BYTES;
    const char* sb = STRIP ? strips + ((t / 3) & 1) * kStripBytes : si + C::I_BYTES;
    const int kwd = STRIP ? (t % 3) * dil : 0;     // strip row offset of this step's tap
    // STRIP: this step also issues shares 2 (t % 3), + 1 of the next group's strip (clamped: the last group
    // re-fetches its own strip, identical bytes, into the buffer being read)
    const int sg = (t / 3 + 1 < ngroups) ? t / 3 + 1 : ngroups - 1;
    constexpr int PPG = (GL + C::GR - 1) / C::GR;        // DMA pieces per MFMA group
    // the next ring slot's step (clamped: the last steps re-fetch the last step into the idle stage)
    const StepP sp = step_params(t + NST - 1 < nk ? t + NST - 1 : nk - 1);
    const int nst = (t + NST - 1) % NST;
    bf16x8 af[2][2];
    uint32_t ix[2];
    bf16x16 bfr[C::FN];
    auto load_a = [&](bf16x8 (&dst)[2], uint32_t& w, int q) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = wc * WCO + (q * 2 + h) * 16 + fr;
        dst[h] = *reinterpret_cast<const bf16x8*>(sa + r * 64 + swzb<64>(r, fq) * 16);
      }
      w = *reinterpret_cast<const uint32_t*>(si + (wc * (WCO / 32) + q) * 256 + lane * 4);
    };
#pragma unroll
    for (int fn = 0; fn < C::FN; ++fn) {
      const int r = wp * 64 + fn * 16 + fr + kwd;
      const int z = STRIP ? (r & 7) : swzb<128>(r, 0);   // both swizzles are an XOR on the chunk number
      const bf16x8 lo = *reinterpret_cast<const bf16x8*>(sb + r * 128 + (fq ^ z) * 16);
      const bf16x8 hi = *reinterpret_cast<const bf16x8*>(sb + r * 128 + ((4 + fq) ^ z) * 16);
      bfr[fn] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    }
    load_a(af[0], ix[0], 0);
#pragma unroll
    for (int q = 0; q < C::GR; ++q) {
      // group q's fragments were issued a group ago (conv_big's schedule)
      if (q + 1 < C::GR) load_a(af[(q + 1) & 1], ix[(q + 1) & 1], q + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int fn = 0; fn < C::FN; ++fn)
        acc[2 * q][fn] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(af[q & 1][0], bfr[fn], acc[2 * q][fn],
                                                                   static_cast<int>(ix[q & 1]), 0, 0);
#pragma unroll
      for (int fn = 0; fn < C::FN; ++fn)
        acc[2 * q + 1][fn] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(af[q & 1][1], bfr[fn], acc[2 * q + 1][fn],
                                                                       static_cast<int>(ix[q & 1]), 0, 1);
#pragma unroll
      for (int k = 0; k < PPG; ++k) {
        const int i = q * PPG + k;
        if constexpr (STRIP) {
          if (i <= C::A_INSTR) issue_piece(sp, nst, i);
          else if (i < GL) issue_strip(sg, 2 * (t % 3) + (i - C::A_INSTR - 1));
        } else {
          if (i < C::GLDS) issue_piece(sp, nst, i);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // whole tile inside a dense bf16 NHWC output: 16-B stores (conv_tile.h store_tile_x4)
  const bool x4 = p.out_dtype == DRNMI_BF16 && p.y_sc == 1 && p.y_sp == p.cout &&
                  p.y_sn == static_cast<int64_t>(p.ho) * p.wo * p.cout && px0 + kBPX <= M && co0 + C::BCO <= p.cout;
  if (x4) store_tile_x4<C::FM, WCO, C::FN>(p, acc, px0, co0, wc, wp, fr, fq);
  else store_tile<C::FM, WCO, C::FN>(p, acc, px0, co0, wc, wp, fr, fq);
}

template <int KS, int WCO, int WC>
__global__ void __launch_bounds__(256 * WC, 1)
conv_sp24_kernel(const drnmi_conv_args p) {
  conv_sp24_body<KS, WCO, WC>(p);
}

// the strip-staged form of the 256 x 256 3x3 tile: 2 x (16 + 2) KB of A + 2 x 33 KB strips
__global__ void __launch_bounds__(512, 1)
conv_sp24_strip_kernel(const drnmi_conv_args p) {
  conv_sp24_body<3, 128, 2, true>(p);
}

// the three dynamic LDS sizes and the DMA pieces per wave and step (the counted vmcnt), pinned
constexpr int kSp24StripLds = 2 * (Sp24Cfg<128, 2>::A_BYTES + Sp24Cfg<128, 2>::I_BYTES) + 2 * kStripBytes;
static_assert(Sp24Cfg<128, 2>::LDS == 3 * 50 * 1024 && Sp24Cfg<128, 2>::GLDS == 2 + 1 + 4, "256 x 256 gather");
static_assert(Sp24Cfg<128, 1>::LDS == 3 * 41 * 1024 && Sp24Cfg<128, 1>::GLDS == 2 + 1 + 8, "128 x 256 gather");
static_assert(kSp24StripLds == (2 * 18 + 2 * 33) * 1024, "strip form");

template <auto KERNEL>
hipError_t launch_sp24_strip(const drnmi_conv_args& p, hipStream_t s) {
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = (M / kBPX) * ((p.cout + 255) / 256);
  return launch_lds<KERNEL>(dim3(static_cast<unsigned>(blocks)), dim3(512), kSp24StripLds, s, p);
}

template <int KS, int WCO, int WC>
hipError_t launch_sp24(const drnmi_conv_args& p, hipStream_t s) {
  using C = Sp24Cfg<WCO, WC>;
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = ((M + kBPX - 1) / kBPX) * ((p.cout + C::BCO - 1) / C::BCO);
  return launch_lds<&conv_sp24_kernel<KS, WCO, WC>>(dim3(static_cast<unsigned>(blocks)), dim3(C::THREADS), C::LDS, s, p);
}


// One lane per (32-row block, K step, index word): rows rb * 32 + fr and + 16 + fr, dense columns
// kt * 64 + 16 fq .. + 15 -> 2 x 8 kept values (one 16-B store each) and one index word.  A group keeps
// its non-zeros in ascending position; with fewer than two it is filled up from position 3 downwards
// (the values there are the zeros themselves); of more than two (a violation) the first two are kept.
__global__ void __launch_bounds__(256)
sp24_pack_kernel(const uint16_t* __restrict__ w, int rows_pad, int k_pad, uint16_t* __restrict__ vals,
                 uint32_t* __restrict__ idx, int* __restrict__ violations) {
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int nk = k_pad >> 6;
  if (gid >= static_cast<int64_t>(rows_pad >> 5) * nk * 64) return;
  const int l = static_cast<int>(gid & 63);
  const int kt = static_cast<int>((gid >> 6) % nk);
  const int rb = static_cast<int>((gid >> 6) / nk);
  const int fr = l & 15, fq = l >> 4;
  uint32_t word = 0;
  int bad = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = rb * 32 + h * 16 + fr;
    const uint16_t* src = w + static_cast<int64_t>(row) * k_pad + kt * 64 + fq * 16;
    uint16_t kept[8];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      int p0 = -1, p1 = -1, nz = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if ((src[4 * g + j] & 0x7fff) == 0) continue;
        if (nz == 0) p0 = j;
        else if (nz == 1) p1 = j;
        ++nz;
      }
      bad += nz > 2;
      if (nz == 0) {
        p0 = 2;
        p1 = 3;
      } else if (nz == 1) {
        if (p0 == 3) {
          p0 = 2;
          p1 = 3;
        } else {
          p1 = 3;
        }
      }
      kept[2 * g] = src[4 * g + p0];
      kept[2 * g + 1] = src[4 * g + p1];
      word |= static_cast<uint32_t>(p0 | (p1 << 2)) << (16 * h + 4 * g);
    }
    uint4 o;
    o.x = kept[0] | (static_cast<uint32_t>(kept[1]) << 16);
    o.y = kept[2] | (static_cast<uint32_t>(kept[3]) << 16);
    o.z = kept[4] | (static_cast<uint32_t>(kept[5]) << 16);
    o.w = kept[6] | (static_cast<uint32_t>(kept[7]) << 16);
    *reinterpret_cast<uint4*>(vals + static_cast<int64_t>(row) * (k_pad >> 1) + kt * 32 + fq * 8) = o;
  }
  idx[gid] = word;
  if (violations != nullptr && bad != 0) atomicAdd(violations, bad);
}

// one wave, one instruction: the operand-map probe
template <int ABID>
__global__ void __launch_bounds__(64)
sp24_mma_probe_kernel(const bf16x8* __restrict__ a, const bf16x16* __restrict__ b, const uint32_t* __restrict__ idx,
                      f32x4* __restrict__ d) {
  const int l = threadIdx.x;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  d[l] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a[l], b[l], z, static_cast<int>(idx[l]), 0, ABID);
}

// Issue-rate loop (scripts/sp24_micro.py): every wave runs iters x 8 MFMAs on 8 independent accumulators with
// operands in registers, SPARSE: v_smfmac_f32_16x16x64_bf16, else v_mfma_f32_16x16x32_bf16
template <bool SPARSE>
__global__ void __launch_bounds__(256)
sp24_issue_kernel(int iters, float* __restrict__ sink) {
  const int l = threadIdx.x;
  bf16x8 a;
  bf16x16 b;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = static_cast<__bf16>(static_cast<float>((l + j) & 3));
#pragma unroll
  for (int j = 0; j < 16; ++j) b[j] = static_cast<__bf16>(static_cast<float>((l ^ j) & 1));
  const bf16x8 b8 = __builtin_shufflevector(b, b, 0, 1, 2, 3, 4, 5, 6, 7);
  const int idx = 0xEE44EE44;      // positions (0, 1) / (2, 3) alternating
  f32x4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (SPARSE) acc[j] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, b, acc[j], idx, 0, 0);
      else acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b8, acc[j], 0, 0, 0);
    }
  }
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) t += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  sink[blockIdx.x * 256 + l] = t;
}

}  // namespace

const ConvKernel* sp24_kernel(bool tile128, int ks) {
  static const ConvKernel k[2][2] = {
      {DRNMI_KERNEL_ROW(conv_sp24_kernel, launch_sp24, 1, 128, 2), DRNMI_KERNEL_ROW(conv_sp24_kernel, launch_sp24, 3, 128, 2)},
      {DRNMI_KERNEL_ROW(conv_sp24_kernel, launch_sp24, 1, 128, 1), DRNMI_KERNEL_ROW(conv_sp24_kernel, launch_sp24, 3, 128, 1)}};
  return &k[tile128][ks == 3];
}

const ConvKernel* sp24_strip_kernel() {
  static const ConvKernel k = DRNMI_KERNEL_ROW0(conv_sp24_strip_kernel, launch_sp24_strip);
  return &k;
}

// the sparse kernel's shapes: conv_big's with cin >= 64 and a folded scale; no second input, no unit mask
bool sp24_conv_supported(const drnmi_conv_args& p) {
  return p.dtype == DRNMI_BF16_SP24 && p.x2 == nullptr && p.unit_mask == nullptr && p.scale == nullptr &&
         big_body_shape_ok(p, 64) && p.k == p.ks * p.ks * p.cin &&
         static_cast<int64_t>(p.cout_pad) * p.k_pad < (int64_t(1) << 31) &&
         (p.out_dtype == DRNMI_F32 || (p.out_dtype == DRNMI_BF16 && p.y_sc == 1 && p.y_sp == p.cout));
}

}  // namespace drnmi

using namespace drnmi;

extern "C" int64_t drnmi_sp24_pack_bytes(int32_t rows_pad, int32_t k_pad) {
  if (rows_pad <= 0 || rows_pad % 32 != 0 || k_pad <= 0 || k_pad % 64 != 0) return -1;
  return static_cast<int64_t>(rows_pad) * k_pad + static_cast<int64_t>(rows_pad) * k_pad / 8;
}

extern "C" int drnmi_sp24_pack(const void* dense_bf16, int32_t rows_pad, int32_t k_pad, void* out, int32_t* violations,
                               void* stream) {
  if (dense_bf16 == nullptr || out == nullptr || drnmi_sp24_pack_bytes(rows_pad, k_pad) < 0 ||
      (reinterpret_cast<uintptr_t>(out) & 15) != 0)
    return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (violations != nullptr) {
    const hipError_t e = hipMemsetAsync(violations, 0, sizeof(int), s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  uint16_t* vals = reinterpret_cast<uint16_t*>(out);
  uint32_t* idx = reinterpret_cast<uint32_t*>(vals + static_cast<int64_t>(rows_pad) * (k_pad / 2));
  const int64_t lanes = static_cast<int64_t>(rows_pad / 32) * (k_pad / 64) * 64;
  hipLaunchKernelGGL(sp24_pack_kernel, dim3(static_cast<unsigned>((lanes + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const uint16_t*>(dense_bf16), rows_pad, k_pad, vals, idx, violations);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_sp24_mma_probe(const void* a, const void* b, const uint32_t* idx, float* d, int32_t abid, void* stream) {
  if (a == nullptr || b == nullptr || idx == nullptr || d == nullptr || (abid != 0 && abid != 1)) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (abid == 0)
    hipLaunchKernelGGL(sp24_mma_probe_kernel<0>, dim3(1), dim3(64), 0, s, reinterpret_cast<const bf16x8*>(a),
                       reinterpret_cast<const bf16x16*>(b), idx, reinterpret_cast<f32x4*>(d));
  else
    hipLaunchKernelGGL(sp24_mma_probe_kernel<1>, dim3(1), dim3(64), 0, s, reinterpret_cast<const bf16x8*>(a),
                       reinterpret_cast<const bf16x16*>(b), idx, reinterpret_cast<f32x4*>(d));
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_sp24_issue_probe(int32_t sparse, int32_t iters, int32_t blocks, float* sink, void* stream) {
  if (sink == nullptr || iters <= 0 || blocks <= 0) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (sparse) hipLaunchKernelGGL(sp24_issue_kernel<true>, dim3(blocks), dim3(256), 0, s, iters, sink);
  else hipLaunchKernelGGL(sp24_issue_kernel<false>, dim3(blocks), dim3(256), 0, s, iters, sink);
  return static_cast<int>(hipGetLastError());
}
