// 2:4 weight-sparse NHWC implicit-GEMM convolution, int8 (W8A8), on v_smfmac_i32_16x16x128_i8
// (dtype DRNMI_I8_SP24, include/drnmi.h: inference, opt-in through DRNSeg.set_sparse24 at precision "int8").
//
// conv_sp24.hip's main loop at int8: A = int8 weights with at most two non-zeros in every four consecutive
// input channels of a tap, stored compressed (the kept values + 2-bit positions, drnmi_sp24_pack_i8),
// B = int8 pixels, dense, int32 accumulators, and the dense int8 epilogue (conv_tile.h store_tile_q8 /
// store_tile_q8_x4): the DRNMI_I8 contract.  Integer sums are exact, so a launch equals the dense int8
// launch on the same (masked) weights bit for bit.  A file of its own for the reason conv_sp24.hip is one
// (profiles/sp24_fold/README.txt); from conv_tile.h, as they are: the swizzles, glds16 / glds4, the XCD-major
// tile deal, strip_src and the strip geometry, zero_tile and the two 8-bit epilogues.  Built with VGPR-form
// MFMAs (build.py).
//
// Operand map of the instruction (measured, tests/test_gpu_sp24_i8.py::test_operand_map), lane = 16 fq + fr:
//   A  lane holds row fr's 16 kept values of dense k 32 fq .. 32 fq + 31: bytes (2 g, 2 g + 1) are the
//      kept pair of group g = k 32 fq + 4 g .. + 3, in ascending position;
//   idx the whole 32-bit register: bits [2 s + 1 : 2 s] = byte s's position inside its group (ABID unused);
//   B  lane holds column fr's k 16 fq .. 16 fq + 15 (bytes 0-15) and 64 + 16 fq .. + 15 (bytes 16-31):
//      two v_mfma_i32_16x16x64_i8 B fragments side by side;
//   D  as the dense 16x16 MFMAs: lane holds rows 4 fq .. 4 fq + 3 of column fr.
//
// K step = 128 dense channels of one tap (cin >= 128).  LDS image of a stage (3 stages), the bf16 sparse
// kernel's shapes and read patterns:
//   A values  BCO rows x 64 B (64 kept values in channel order), 16-B chunk c of row r at slot
//             swzb<64>(r, c): lane (fr, fq) reads chunk fq;
//   A index   BCO / 16 blocks of 64 words: word 16 fq + fr of block f holds the 32 index bits of row
//             16 f + fr for k 32 fq .. + 31, so a wave reads 64 consecutive words per fragment;
//   B         256 pixel rows x 128 B with the 128-B swizzle: lane (fr, fq) reads chunks fq and 4 + fq
//             as one 32-B fragment.
// 256 x 256 tile (8 waves): 16 + 4 + 32 KB per stage; 128 x 256 (4 waves): 8 + 2 + 32 KB.
// The blob (private to this file): the value plane [cout_pad][k_pad / 2] int8, then the index plane
// [cout_pad / 16][k_pad / 128][64] words in the LDS order above, so a K step's index block of 16 rows
// is one 256-B DMA (global_load_lds_dword); a wave issues the two blocks 2 wave and 2 wave + 1.
#include "common.h"
#include "conv_tile.h"
#include "kernels.h"

namespace drnmi {
namespace {

template <int WCO, int WC>
struct Sp24I8Cfg {
  static constexpr int BK = 128;                    // dense channels per K step
  static constexpr int NST = 3;
  static constexpr int BCO = WCO * WC;
  static constexpr int FM = WCO / 16;
  static constexpr int FN = 4;
  static constexpr int NW = 4 * WC;
  static constexpr int THREADS = 64 * NW;
  static constexpr int A_BYTES = BCO * 64;          // kept values: 64-B rows
  static constexpr int I_BYTES = BCO * 16;          // positions: 2 bits per kept value
  static constexpr int B_BYTES = kBPX * 128;
  static constexpr int STAGE = A_BYTES + I_BYTES + B_BYTES;
  static constexpr int A_INSTR = BCO / 16 / NW;     // 1-KB pieces (16 rows) per wave per step
  static constexpr int I_INSTR = 2;                 // 256-B index blocks (16 rows) per wave per step
  static constexpr int B_INSTR = kBPX / 8 / NW;     // 1-KB pieces (8 rows)
  static constexpr int GLDS = A_INSTR + I_INSTR + B_INSTR;
  static constexpr int LDS = NST * STAGE;
  static constexpr int GR = FM / 2;                 // MFMA groups per step: one fragment pair each
  static_assert(BCO / 16 == I_INSTR * NW, "two 16-row index blocks per wave");
  static_assert(LDS <= 160 * 1024, "LDS");
};

// STRIP (3x3 stride 1, wo % 256 == 0, the 256 x 256 tile): conv_sp24_body's strip mode.  The three kw taps
// of one (128-channel block, kh) read one strip of 256 + 2 dil pixel rows at row offset kw * dil, staged
// once per three K steps into one of two strip buffers (conv_tile.h kStripBytes) in five shares per wave;
// A (values + index) rides a two-stage ring and every step waits for all of its DMA.
// Same K order and MFMAs as the gather form: bit-identical.
template <int KS, int WCO, int WC, bool STRIP = false>
__device__ __forceinline__ void conv_sp24_i8_body(const drnmi_conv_args& p) {
  using C = Sp24I8Cfg<WCO, WC>;
  constexpr int NST = STRIP ? 2 : C::NST, BK = C::BK;
  static_assert(!STRIP || (KS == 3 && C::NW == 8), "strip mode: the 256 x 256 3x3 tile");
  constexpr int STAGE = STRIP ? C::A_BYTES + C::I_BYTES : C::STAGE;   // strip: the ring holds A only
  constexpr int AI = C::A_INSTR + C::I_INSTR;                         // A pieces of a step: values, then index
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
  const int8_t* __restrict__ x = reinterpret_cast<const int8_t*>(p.x);
  const int kh2 = p.k_pad / 2;                      // kept values per weight row
  const int nk = p.k_pad / BK;
  const int8_t* __restrict__ vals = reinterpret_cast<const int8_t*>(p.wgt);
  const uint32_t* __restrict__ idxp = reinterpret_cast<const uint32_t*>(vals + static_cast<int64_t>(p.cout_pad) * kh2);
  const int fr = lane & 15;
  const int fq = lane >> 4;

  const int tile = xcd_remap2(blockIdx.x, ntiles);
  const int px0 = (tile / nco) * kBPX;
  const int co0 = (tile % nco) * C::BCO;

  // --- DMA assignment.  A values: lane l fills row l / 4, slot l % 4 of a 16-row piece; index: the
  // wave's own two 16-row blocks, lane l its word l; pixels: row l / 8, slot l % 8 of an 8-row piece
  int a_off[C::A_INSTR];
#pragma unroll
  for (int i = 0; i < C::A_INSTR; ++i) {
    const int r = (wave * C::A_INSTR + i) * 16 + (lane >> 2);
    a_off[i] = (co0 + r) * kh2 + swzb<64>(r, lane & 3) * 16;
  }
  const int i_off = ((co0 >> 4) + wave * C::I_INSTR) * nk * 64 + lane;
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
      b_off[i] = ((n * H + ih0) * W + iw0) * cin + swzb<128>(r, lane & 7) * 16;
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
  // pieces [0, A_INSTR) kept values, then the two index blocks, then pixel rows
  auto issue_piece = [&](const StepP& sp, int stage, int i) {
    char* sa = smem + stage * STAGE;
    if (i < C::A_INSTR) {
      glds16(vals + (a_off[i] + (sp.k0 >> 1)), sa + (wave * C::A_INSTR + i) * 1024);
    } else if (i < AI) {
      const int j = i - C::A_INSTR;
      glds4(idxp + (i_off + (j * nk + (sp.k0 >> 7)) * 64), sa + C::A_BYTES + (wave * C::I_INSTR + j) * 256);
    } else if constexpr (!STRIP) {
      const int j = i - AI;
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
    const void* src = strip_src<BK, 16>(p, x, g, R, lane & 7, s_n, s_oh, s_ow0, H, W, cin, dil, zero_src);
    glds16(src, strips + (g & 1) * kStripBytes + j * 1024);
  };
  constexpr int GL = STRIP ? AI + 2 : C::GLDS;     // pieces a wave issues per step (strip: + two strip shares)

  i32x4 acc[C::FM][C::FN];
  zero_tile(acc);
  for (int t = 0; t < NST - 1 && t < nk; ++t) {
    const StepP sp = step_params(t);
#pragma unroll
    for (int i = 0; i < (STRIP ? AI : C::GLDS); ++i) issue_piece(sp, t, i);
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
    i32x4 af[2][2];
    uint32_t ix[2][2];
    i32x8 bfr[C::FN];
    auto load_a = [&](i32x4 (&dst)[2], uint32_t (&w)[2], int q) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int f = wc * C::FM + q * 2 + h;
        const int r = f * 16 + fr;
        dst[h] = *reinterpret_cast<const i32x4*>(sa + r * 64 + swzb<64>(r, fq) * 16);
        w[h] = *reinterpret_cast<const uint32_t*>(si + f * 256 + lane * 4);
      }
    };
#pragma unroll
    for (int fn = 0; fn < C::FN; ++fn) {
      const int r = wp * 64 + fn * 16 + fr + kwd;
      const int z = STRIP ? (r & 7) : swzb<128>(r, 0);   // both swizzles are an XOR on the chunk number
      const i32x4 lo = *reinterpret_cast<const i32x4*>(sb + r * 128 + (fq ^ z) * 16);
      const i32x4 hi = *reinterpret_cast<const i32x4*>(sb + r * 128 + ((4 + fq) ^ z) * 16);
      bfr[fn] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    load_a(af[0], ix[0], 0);
#pragma unroll
    for (int q = 0; q < C::GR; ++q) {
      // group q's fragments were issued a group ago (conv_big's schedule)
      if (q + 1 < C::GR) load_a(af[(q + 1) & 1], ix[(q + 1) & 1], q + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int fn = 0; fn < C::FN; ++fn)
          acc[2 * q + h][fn] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(af[q & 1][h], bfr[fn], acc[2 * q + h][fn],
                                                                        static_cast<int>(ix[q & 1][h]), 0, 0);
#pragma unroll
      for (int k = 0; k < PPG; ++k) {
        const int i = q * PPG + k;
        if constexpr (STRIP) {
          if (i < AI) issue_piece(sp, nst, i);
          else if (i < GL) issue_strip(sg, 2 * (t % 3) + (i - AI));
        } else {
          if (i < C::GLDS) issue_piece(sp, nst, i);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // the dense int8 epilogue: whole tiles of a dense int8 NHWC output take the 16-B form (conv_big_body.h)
  const bool x4 = q8_dense_x4<int8_t>(p) && px0 + kBPX <= M && co0 + C::BCO <= p.cout;
  if (x4) store_tile_q8_x4<int8_t, C::FM, WCO, C::FN>(p, acc, px0, co0, wc, wp, fr, fq);
  else store_tile_q8<int8_t, C::FM, WCO, C::FN>(p, acc, px0, co0, wc, wp, fr, fq);
}

template <int KS, int WCO, int WC>
__global__ void __launch_bounds__(256 * WC, 1)
conv_sp24_i8_kernel(const drnmi_conv_args p) {
  conv_sp24_i8_body<KS, WCO, WC>(p);
}

// the strip-staged form of the 256 x 256 3x3 tile: 2 x (16 + 4) KB of A + 2 x 33 KB strips
__global__ void __launch_bounds__(512, 1)
conv_sp24_i8_strip_kernel(const drnmi_conv_args p) {
  conv_sp24_i8_body<3, 128, 2, true>(p);
}

// the three dynamic LDS sizes and the DMA pieces per wave and step (the counted vmcnt), pinned
constexpr int kSp24I8StripLds = 2 * (Sp24I8Cfg<128, 2>::A_BYTES + Sp24I8Cfg<128, 2>::I_BYTES) + 2 * kStripBytes;
static_assert(Sp24I8Cfg<128, 2>::LDS == 3 * 52 * 1024 && Sp24I8Cfg<128, 2>::GLDS == 2 + 2 + 4, "256 x 256 gather");
static_assert(Sp24I8Cfg<128, 1>::LDS == 3 * 42 * 1024 && Sp24I8Cfg<128, 1>::GLDS == 2 + 2 + 8, "128 x 256 gather");
static_assert(kSp24I8StripLds == (2 * 20 + 2 * 33) * 1024, "strip form");

template <auto KERNEL>
hipError_t launch_sp24_i8_strip(const drnmi_conv_args& p, hipStream_t s) {
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = (M / kBPX) * ((p.cout + 255) / 256);
  return launch_lds<KERNEL>(dim3(static_cast<unsigned>(blocks)), dim3(512), kSp24I8StripLds, s, p);
}

template <int KS, int WCO, int WC>
hipError_t launch_sp24_i8(const drnmi_conv_args& p, hipStream_t s) {
  using C = Sp24I8Cfg<WCO, WC>;
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = ((M + kBPX - 1) / kBPX) * ((p.cout + C::BCO - 1) / C::BCO);
  return launch_lds<&conv_sp24_i8_kernel<KS, WCO, WC>>(dim3(static_cast<unsigned>(blocks)), dim3(C::THREADS), C::LDS, s, p);
}

// One lane per (16-row block, K step, index word): row rb * 16 + fr, dense columns kt * 128 + 32 fq .. + 31
// -> 16 kept values (one 16-B store) and one index word.  A group keeps its non-zeros in ascending
// position; with fewer than two it is filled up from position 3 downwards (the values there are the
// zeros themselves); of more than two (a violation) the first two are kept.
__global__ void __launch_bounds__(256)
sp24_pack_i8_kernel(const int8_t* __restrict__ w, int rows_pad, int k_pad, int8_t* __restrict__ vals,
                    uint32_t* __restrict__ idx, int* __restrict__ violations) {
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int nk = k_pad >> 7;
  if (gid >= static_cast<int64_t>(rows_pad >> 4) * nk * 64) return;
  const int l = static_cast<int>(gid & 63);
  const int kt = static_cast<int>((gid >> 6) % nk);
  const int rb = static_cast<int>((gid >> 6) / nk);
  const int fr = l & 15, fq = l >> 4;
  const int row = rb * 16 + fr;
  const int8_t* src = w + static_cast<int64_t>(row) * k_pad + kt * 128 + fq * 32;
  uint32_t word = 0;
  int bad = 0;
  uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    int p0 = -1, p1 = -1, nz = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (src[4 * g + j] == 0) continue;
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
    const uint32_t pair = static_cast<uint8_t>(src[4 * g + p0]) | (static_cast<uint32_t>(static_cast<uint8_t>(src[4 * g + p1])) << 8);
    o[g >> 1] |= pair << (16 * (g & 1));
    word |= static_cast<uint32_t>(p0 | (p1 << 2)) << (4 * g);
  }
  *reinterpret_cast<uint4*>(vals + static_cast<int64_t>(row) * (k_pad >> 1) + kt * 64 + fq * 16) = make_uint4(o[0], o[1], o[2], o[3]);
  idx[gid] = word;
  if (violations != nullptr && bad != 0) atomicAdd(violations, bad);
}

// one wave, one instruction: the operand-map probe
__global__ void __launch_bounds__(64)
sp24_mma_probe_i8_kernel(const i32x4* __restrict__ a, const i32x8* __restrict__ b, const uint32_t* __restrict__ idx,
                         i32x4* __restrict__ d) {
  const int l = threadIdx.x;
  const i32x4 z = {0, 0, 0, 0};
  d[l] = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a[l], b[l], z, static_cast<int>(idx[l]), 0, 0);
}

}  // namespace

const ConvKernel* sp24_i8_kernel(bool tile128, int ks) {
  static const ConvKernel k[2][2] = {
      {DRNMI_KERNEL_ROW(conv_sp24_i8_kernel, launch_sp24_i8, 1, 128, 2), DRNMI_KERNEL_ROW(conv_sp24_i8_kernel, launch_sp24_i8, 3, 128, 2)},
      {DRNMI_KERNEL_ROW(conv_sp24_i8_kernel, launch_sp24_i8, 1, 128, 1), DRNMI_KERNEL_ROW(conv_sp24_i8_kernel, launch_sp24_i8, 3, 128, 1)}};
  return &k[tile128][ks == 3];
}

const ConvKernel* sp24_i8_strip_kernel() {
  static const ConvKernel k = DRNMI_KERNEL_ROW0(conv_sp24_i8_strip_kernel, launch_sp24_i8_strip);
  return &k;
}

// the sparse int8 kernel's shapes: the int8 route's with cin >= 128 (one K step inside a tap); no second
// input, no unit mask
bool sp24_i8_conv_supported(const drnmi_conv_args& p) {
  return p.dtype == DRNMI_I8_SP24 && p.x2 == nullptr && p.unit_mask == nullptr && p.scale != nullptr &&
         big_body_shape_ok(p, 128) && p.k == p.ks * p.ks * p.cin &&
         static_cast<int64_t>(p.cout_pad) * p.k_pad < (int64_t(1) << 31) &&
         (p.out_dtype == DRNMI_F32 || p.out_dtype == DRNMI_BF16 || p.out_dtype == DRNMI_I8);
}

}  // namespace drnmi

using namespace drnmi;

extern "C" int64_t drnmi_sp24_pack_i8_bytes(int32_t rows_pad, int32_t k_pad) {
  if (rows_pad <= 0 || rows_pad % 32 != 0 || k_pad <= 0 || k_pad % 128 != 0) return -1;
  return static_cast<int64_t>(rows_pad) * k_pad / 2 + static_cast<int64_t>(rows_pad) * k_pad / 8;
}

extern "C" int drnmi_sp24_pack_i8(const void* dense_i8, int32_t rows_pad, int32_t k_pad, void* out, int32_t* violations,
                                  void* stream) {
  if (dense_i8 == nullptr || out == nullptr || drnmi_sp24_pack_i8_bytes(rows_pad, k_pad) < 0 ||
      (reinterpret_cast<uintptr_t>(out) & 15) != 0)
    return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (violations != nullptr) {
    const hipError_t e = hipMemsetAsync(violations, 0, sizeof(int), s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  int8_t* vals = reinterpret_cast<int8_t*>(out);
  uint32_t* idx = reinterpret_cast<uint32_t*>(vals + static_cast<int64_t>(rows_pad) * (k_pad / 2));
  const int64_t lanes = static_cast<int64_t>(rows_pad / 16) * (k_pad / 128) * 64;
  hipLaunchKernelGGL(sp24_pack_i8_kernel, dim3(static_cast<unsigned>((lanes + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const int8_t*>(dense_i8), rows_pad, k_pad, vals, idx, violations);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_sp24_mma_probe_i8(const void* a, const void* b, const uint32_t* idx, int32_t* d, void* stream) {
  if (a == nullptr || b == nullptr || idx == nullptr || d == nullptr) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sp24_mma_probe_i8_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const i32x4*>(a),
                     reinterpret_cast<const i32x8*>(b), idx, reinterpret_cast<i32x4*>(d));
  return static_cast<int>(hipGetLastError());
}
