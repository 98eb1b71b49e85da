// Large-channel NHWC implicit-GEMM convolution, bf16, LDS-DMA staged (the MFMA-bound layers).
//
// Serves every bf16 conv of DRN-D with cin >= 32 and ks 1/3: layer3..layer8 3x3 convs
// (dilation 1/2/4, lmodels/drn.py:27-29, :49-65, :201-211), the 1x1 stride-s downsamples
// (:181-186), the Bottleneck convs (:86-106) and the seg 1x1 + bias (lmodels/drnseg.py:278-284).
// In D-22 at 1024x2048 layer5..8 hold ~85 % of the FLOPs at arithmetic intensity
// 750..2150 FLOP/B: MFMA-bound.
//
// Structure (one output tile = BCO channels x 256 pixels per workgroup):
//   * MFMA v_mfma_f32_16x16x32_bf16 with A = weights (rows = output channels), B = pixels,
//     so the accumulator hands each lane 4 consecutive channels of one pixel (8-byte NHWC
//     stores and residual loads).
//   * K step BK (64, or 32 when cin == 32) = one kernel tap x BK input channels.  Both
//     operand tiles go global -> LDS with global_load_lds_dwordx4 (LDS-DMA: no VGPR round
//     trip, no ds_write issue).  Each pixel row of the B tile is gathered from its own NHWC
//     address -- the implicit-GEMM im2col happens in the DMA source addresses; out-of-image
//     taps read a zero page, which is the conv's zero padding.
//   * NST-stage LDS ring, counted vmcnt + raw s_barrier once per step (a __syncthreads()
//     would drain every DMA in flight).
//   * LDS rows are BK*2 bytes; 16-B chunk c of row r sits at slot c ^ f(r) (applied on the
//     DMA source address because the DMA destination is lane-linear, and on the fragment
//     read): the 16x16x32 fragment reads are bank-conflict free (SQ_LDS_BANK_CONFLICT = 0).
//   * Fragment reads run one MFMA group ahead, and the next step's DMA is issued piece by
//     piece between the MFMA groups of the first substep, so DMA issue cost and LDS latency
//     hide under MFMAs (measured +7..10 % over issuing the DMA as one block).
//   * Each wave owns WCO channels x 64 pixels (WCO/16 x 4 fragments).
//   * Tiles are dealt XCD-major (bijective remap) so the channel tiles of a pixel tile and
//     neighbouring pixel rows share an XCD's L2.
//   * PERSIST: one workgroup per CU walks its tiles; the next tile's first DMA steps are
//     issued before the current tile's epilogue, hiding the pipeline fill and the
//     epilogue (a ~10 us fixed cost per tile otherwise).
#include "common.h"
#include "conv_big_body.h"
#include "conv_tile.h"
#include "kernels.h"

namespace drnmi {
namespace {

template <int KS, int WCO, int WC, int NST, int BK, bool PERSIST, int NWP, bool SPARSE, bool X2 = false>
__global__ void __launch_bounds__(64 * NWP * WC, 1)
conv_big_kernel(const drnmi_conv_args p) {
  conv_big_body<uint16_t, KS, WCO, WC, NST, BK, PERSIST, NWP, SPARSE, X2>(p);
}

// Strip-staged B operand (see conv_big_body STRIP): the 256 x 256 3x3 tile for wo % 256 == 0.
__global__ void __launch_bounds__(512, 1)
conv_strip_kernel(const drnmi_conv_args p) {
  conv_big_body<uint16_t, 3, 128, 2, 2, 64, false, 4, false, false, true>(p);
}

// int8 strip-staged B: conv_i8_kernel<3, 128, 2, 2, 128> with the STRIP B path (int8 rows of 128
// channels are 128 B, the bf16 layout): same MFMA order, bit-identical to the per-tap gather.
__global__ void __launch_bounds__(512, 1)
conv_i8_strip_kernel(const drnmi_conv_args p) {
  conv_big_body<int8_t, 3, 128, 2, 2, 128, false, 4, false, false, true>(p);
}

// W8A8 (config C5): the same LDS-DMA pipeline over int8 elements, BK int8 channels per K step
// (128-B LDS rows for cin >= 128, 64-B rows for cin == 64), v_mfma_i32_16x16x64_i8 into int32
// accumulators, store_tile_q8 epilogue.
template <int KS, int WCO, int WC, int NST, int BK>
__global__ void __launch_bounds__(64 * 4 * WC, 1)
conv_i8_kernel(const drnmi_conv_args p) {
  conv_big_body<int8_t, KS, WCO, WC, NST, BK, false, 4, false>(p);
}

// fp8 (DRNMI_F8, OCP e4m3): the same pipeline and LDS image over e4m3 bytes, BK channels per K
// step as the int8 rows, v_mfma_f32_16x16x128_f8f6f4 into fp32 accumulators (one MFMA per fragment
// pair and K step: KT<f8_t>), the same epilogue (conv_tile.h Q8<T>)
template <int KS, int WCO, int WC, int NST, int BK>
__global__ void __launch_bounds__(64 * 4 * WC, 1)
conv_f8_kernel(const drnmi_conv_args p) {
  conv_big_body<f8_t, KS, WCO, WC, NST, BK, false, 4, false>(p);
}

// ... and at two workgroups per CU for the 1x1s, as conv_i8_occ2_kernel (64-B rows: the K-64 step)
template <int KS, int WCO, int WC, int NST, int BK>
__global__ void __launch_bounds__(64 * 4 * WC, 2) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv_f8_occ2_kernel(const drnmi_conv_args p) {
  conv_big_body<f8_t, KS, WCO, WC, NST, BK, false, 4, false>(p);
}

// the same body at two workgroups per CU (register budget 256, 2 x 24 KB of LDS with 64-B rows):
// the 1x1 launches have 1-2 K steps per tile, so one resident tile per CU leaves its loads and
// stores serialised tile after tile; a second tile overlaps them
template <int KS, int WCO, int WC, int NST, int BK>
__global__ void __launch_bounds__(64 * 4 * WC, 2) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv_i8_occ2_kernel(const drnmi_conv_args p) {
  conv_big_body<int8_t, KS, WCO, WC, NST, BK, false, 4, false>(p);
}

// --- Ping-pong 256 x 256 schedule (variant "pp256").
//
// Same tile, LDS image and fragment layout as conv_big_kernel<KS, 128, 2, 2, 64>, but each
// 64-deep K step runs as 4 phases, one per quadrant of the wave's 128 x 64 output block
// (16 MFMAs each), and every phase is {load segment} s_barrier {MFMA segment} s_barrier.
// The two waves of a SIMD (w and w + 4: the two channel halves wc) run one barrier apart,
// so on every SIMD one wave issues its LDS fragment reads and DMA pieces while the other
// one runs its MFMA cluster (cdna_hip_programming.md "256^2 8-phase template", T3-T5).
// The stage is split in halves that free up at different phases: the first half (channel
// rows 0-63 of each wc block, pixel rows 0-31 of each 64-pixel block) is read in phase 0,
// the second half in phases 1-2.  Pieces in flight: phases 0-1 of step s stage the second
// half of step s+1, phases 2-3 the first half of step s+2, so every piece has >= 6
// segments to land, with counted vmcnt waits (never 0 in steady state).
template <int KS>
__global__ void __launch_bounds__(512, 1)
conv_pp_kernel(const drnmi_conv_args p) {
  constexpr int BK = 64, ROWB = 128, A_BYTES = 256 * ROWB, STAGE = 2 * A_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (scalar branches)
  const int wc = wave >> 2;
  const int wp = wave & 3;
  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int nco = p.cout / 256;
  const int npx = (M + kBPX - 1) / kBPX;
  const int ntiles = npx * nco;
  const int tile = xcd_remap2(blockIdx.x, ntiles);
  const int px0 = (tile / nco) * kBPX;
  const int co0 = (tile % nco) * 256;

  const int cin = p.cin;
  const int lc = 31 - __builtin_clz(cin);
  const int H = p.h, W = p.w, dil = p.dil;
  const uint16_t* __restrict__ x = reinterpret_cast<const uint16_t*>(p.x);
  const uint16_t* __restrict__ wt = reinterpret_cast<const uint16_t*>(p.wgt);
  const int nk = p.k_pad / BK;
  const int fr = lane & 15;
  const int fq = lane >> 4;

  // DMA pieces: half h, slot j: weight rows ((2w+j)/8)*128 + h*64 + ((2w+j)%8)*8 .. +8 and
  // pixel rows ((2w+j)/4)*64 + h*32 + ((2w+j)%4)*8 .. +8 (lane -> row + lane/8, chunk lane%8)
  const int lrow = lane >> 3;
  const int lslot = lane & 7;
  int a_off[2][2], a_row0[2][2], b_row0[2][2], b_ih0[2][2], b_iw0[2][2];
  const uint16_t* b_base[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = 2 * wave + j;
      a_row0[h][j] = (q >> 3) * 128 + h * 64 + (q & 7) * 8;
      const int ra = a_row0[h][j] + lrow;
      a_off[h][j] = (co0 + ra) * p.k_pad + swz<BK>(ra, lslot) * 8;
      b_row0[h][j] = (q >> 2) * 64 + h * 32 + (q & 3) * 8;
      const int rb = b_row0[h][j] + lrow;
      const int m = px0 + rb;
      b_ih0[h][j] = -(1 << 28);
      b_iw0[h][j] = -(1 << 28);
      b_base[h][j] = x;
      if (m < M) {
        const int n = m / hw_o;
        const int qq = m - n * hw_o;
        const int oh = qq / p.wo;
        const int ow = qq - oh * p.wo;
        b_ih0[h][j] = oh * p.stride - p.pad;
        b_iw0[h][j] = ow * p.stride - p.pad;
        b_base[h][j] = x + ((static_cast<int64_t>(n) * H + b_ih0[h][j]) * W + b_iw0[h][j]) * cin +
                       swz<BK>(rb, lslot) * 8;
      }
    }
  const char* zero_src = reinterpret_cast<const char*>(g_zero_page) + lane * 16;

  // stage pieces (h, j) of K step kt (one weight piece + one pixel piece)
  auto issue = [&](int kt, int h, int j) {
    const int cb = kt / (KS * KS);                 // channel block outer, tap inner (as conv_big)
    const int tap = kt - cb * (KS * KS);
    const int k0 = (tap << lc) + cb * BK;
    const int dh = (tap / KS) * dil;
    const int dw = (tap - (tap / KS) * KS) * dil;
    const int64_t toff = (static_cast<int64_t>(dh) * W + dw) * cin + cb * BK;
    char* sa = smem + (kt & 1) * STAGE;
    glds16(wt + a_off[h][j] + k0, sa + a_row0[h][j] * ROWB);
    const bool ok = static_cast<unsigned>(b_ih0[h][j] + dh) < static_cast<unsigned>(H) &&
                    static_cast<unsigned>(b_iw0[h][j] + dw) < static_cast<unsigned>(W);
    const void* src = ok ? static_cast<const void*>(b_base[h][j] + toff) : static_cast<const void*>(zero_src);
    glds16(src, sa + A_BYTES + b_row0[h][j] * ROWB);
  };
  auto barrier = [&]() {
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  // fragments: channel half hh (4 fragments x 2 substeps), pixel half g (2 x 2)
  auto load_a = [&](bf16x8 (&dst)[4][2], const char* sa, int hh) {
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int r = wc * 128 + hh * 64 + f * 16 + fr;
        dst[f][sub] = *reinterpret_cast<const bf16x8*>(sa + r * ROWB + swz<BK>(r, sub * 4 + fq) * 16);
      }
  };
  auto load_b = [&](bf16x8 (&dst)[2][2], const char* sa, int g) {
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int r = wp * 64 + g * 32 + f * 16 + fr;
        dst[f][sub] = *reinterpret_cast<const bf16x8*>(sa + A_BYTES + r * ROWB + swz<BK>(r, sub * 4 + fq) * 16);
      }
  };
  f32x4 acc[8][4];
  auto mfma = [&](const bf16x8 (&a)[4][2], const bf16x8 (&b)[2][2], int hh, int g) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int e = 0; e < 2; ++e)
          acc[hh * 4 + f][g * 2 + e] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[f][sub], b[e][sub], acc[hh * 4 + f][g * 2 + e], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  init_tile<8, 128>(p, acc, px0, co0, wc, wp, fr, fq);
  // prologue: step 0 (both halves) and the first half of step 1
  issue(0, 0, 0);
  issue(0, 0, 1);
  issue(0, 1, 0);
  issue(0, 1, 1);
  if (nk > 1) {
    issue(1, 0, 0);
    issue(1, 0, 1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  }
  barrier();
  if (wc == 1) barrier();   // the second channel half runs one barrier behind

  bf16x8 a_f[4][2], b0[2][2], b1[2][2];
  for (int s = 0; s < nk; ++s) {
    const char* sa = smem + (s & 1) * STAGE;
    const bool n1 = s + 1 < nk, n2 = s + 2 < nk;
    // phase 0: quadrant (channels 0-63, pixels 0-31); retire the second half of step s
    load_a(a_f, sa, 0);
    load_b(b0, sa, 0);
    if (n1) {
      issue(s + 1, 1, 0);
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    barrier();
    mfma(a_f, b0, 0, 0);
    barrier();
    // phase 1: (channels 0-63, pixels 32-63)
    load_b(b1, sa, 1);
    if (n1) issue(s + 1, 1, 1);
    barrier();
    mfma(a_f, b1, 0, 1);
    barrier();
    // phase 2: (channels 64-127, pixels 32-63)
    load_a(a_f, sa, 1);
    if (n2) issue(s + 2, 0, 0);
    barrier();
    mfma(a_f, b1, 1, 1);
    barrier();
    // phase 3: (channels 64-127, pixels 0-31); retire the first half of step s+1
    if (n2) {
      issue(s + 2, 0, 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else if (n1) {
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    }
    barrier();
    mfma(a_f, b0, 1, 0);
    barrier();
  }
  if (wc == 0) barrier();   // balance the barrier count of the two halves

  store_tile<8, 128>(p, acc, px0, co0, wc, wp, fr, fq);
}

template <int KS>
hipError_t launch_pp(const drnmi_conv_args& p, hipStream_t s) {
  constexpr int LDS = 2 * 2 * 256 * 128;
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = ((M + kBPX - 1) / kBPX) * (p.cout / 256);
  return launch_lds<&conv_pp_kernel<KS>>(dim3(static_cast<unsigned>(blocks)), dim3(512), LDS, s, p);
}

int g_num_cus = 0;

template <int KS, int WCO, int WC, int NST, int BK, bool PERSIST, int NWP = 4, bool SPARSE = false, bool X2 = false>
hipError_t launch_big(const drnmi_conv_args& p, hipStream_t s) {
  using C = BigCfg<WCO, WC, NST, BK, NWP>;
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  int64_t blocks = ((M + kBPX - 1) / kBPX) * ((p.cout + C::BCO - 1) / C::BCO);
  if (PERSIST) {
    if (g_num_cus == 0) {
      int dev = 0, cus = 0;
      if (hipGetDevice(&dev) != hipSuccess ||
          hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
      g_num_cus = cus;
    }
    const int64_t per_cu = (160 * 1024) / C::LDS;        // resident workgroups per CU (LDS-bound)
    const int64_t cap = g_num_cus * (per_cu > 0 ? per_cu : 1);
    blocks = blocks < cap ? blocks : cap;
  }
  return launch_lds<&conv_big_kernel<KS, WCO, WC, NST, BK, PERSIST, NWP, SPARSE, X2>>(dim3(static_cast<unsigned>(blocks)),
                                                                                      dim3(C::THREADS), C::LDS, s, p);
}

constexpr int kStripLds = 2 * 256 * 128 + 2 * kStripBytes;   // 2 A stages + 2 strips (130 KB)

// conv_strip_kernel / conv_i8_strip_kernel
template <auto KERNEL>
hipError_t launch_strip(const drnmi_conv_args& p, hipStream_t s) {
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = (M / kBPX) * ((p.cout + 255) / 256);
  return launch_lds<KERNEL>(dim3(static_cast<unsigned>(blocks)), dim3(512), kStripLds, s, p);
}

// conv_i8_kernel / conv_f8_kernel, or at OCC2 their two-workgroups-per-CU forms
template <typename T, int KS, int WCO, int WC, int NST, int BK, bool OCC2>
hipError_t launch_q8(const drnmi_conv_args& p, hipStream_t s) {
  using C = BigCfg<WCO, WC, NST, BK, 4, 1>;
  constexpr auto kernel = [] {   // if constexpr: only the kernel picked is instantiated
    if constexpr (kIsF8<T>) {
      if constexpr (OCC2) return &conv_f8_occ2_kernel<KS, WCO, WC, NST, BK>;
      else return &conv_f8_kernel<KS, WCO, WC, NST, BK>;
    } else {
      if constexpr (OCC2) return &conv_i8_occ2_kernel<KS, WCO, WC, NST, BK>;
      else return &conv_i8_kernel<KS, WCO, WC, NST, BK>;
    }
  }();
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = ((M + kBPX - 1) / kBPX) * ((p.cout + C::BCO - 1) / C::BCO);
  return launch_lds<kernel>(dim3(static_cast<unsigned>(blocks)), dim3(C::THREADS), C::LDS, s, p);
}

// one lane per 16 x 32 unit; lanes 0-31 / 32-63 of a wave cover the 32 units of two mask words
template <typename T>
__global__ void __launch_bounds__(256)
unit_mask_kernel(const T* __restrict__ w, int rows_pad, int k_pad, int wpr, uint32_t* __restrict__ mask,
                 int* __restrict__ count) {
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t word = gid >> 5;
  const int bit = static_cast<int>(gid & 31);
  const int rb = static_cast<int>(word / wpr);
  const int ku = static_cast<int>(word % wpr) * 32 + bit;
  const int nku = k_pad >> 5;
  bool nz = false;
  if (rb < rows_pad / 16 && ku < nku) {
    for (int r = 0; r < 16 && !nz; ++r) {
      const T* row = w + static_cast<int64_t>(rb * 16 + r) * k_pad + ku * 32;
      for (int c = 0; c < 32; ++c) {
        if constexpr (sizeof(T) == 2) nz |= (row[c] & 0x7fff) != 0;
        else nz |= (__float_as_uint(row[c]) & 0x7fffffffu) != 0;
      }
    }
  }
  const uint64_t b = __ballot(nz);
  const int lane = threadIdx.x & 63;
  if (rb < rows_pad / 16) {
    if (lane == 0) mask[word] = static_cast<uint32_t>(b & 0xffffffffu);
    if (lane == 32) mask[word] = static_cast<uint32_t>(b >> 32);
  }
  if (count != nullptr && nz) atomicAdd(count, 1);
}

}  // namespace

// conv_big_kernel<KS, WCO, WC, NST, BK, PERSIST, 4, SPARSE, X2>, rows [ks == 3]
#define BIG_ROW(KS, WCO, WC, NST, BK, PERSIST, SPARSE, X2) \
  DRNMI_KERNEL_ROW(conv_big_kernel, launch_big, KS, WCO, WC, NST, BK, PERSIST, 4, SPARSE, X2)
#define BIG_ROWS(...) {BIG_ROW(1, __VA_ARGS__), BIG_ROW(3, __VA_ARGS__)}
#define BIG_NONE {kNoKernel, kNoKernel}
#define BIG_DENSE(WCO, WC, NST, BK, PERSIST) WCO * WC, BK, BIG_ROWS(WCO, WC, NST, BK, PERSIST, false, false)
#define BIG_SPARSE(WCO, WC, NST, BK) BIG_ROWS(WCO, WC, NST, BK, false, true, false)
#define BIG_X2(WCO, WC, NST, BK) BIG_ROWS(WCO, WC, NST, BK, false, false, true)
const BigVariant& big_variant(int v) {
  static const BigVariant k[kNumBigVariants] = {
    {BIG_DENSE(128, 1, 3, 64, false), BIG_SPARSE(128, 1, 3, 64), BIG_X2(128, 1, 3, 64)},   // 128 x 256 tile, 4 waves, 3 x 48 KB
    {BIG_DENSE(128, 2, 2, 64, false), BIG_SPARSE(128, 2, 2, 64), BIG_X2(128, 2, 2, 64)},   // 256 x 256 tile, 8 waves, 2 x 64 KB
    {BIG_DENSE(64, 1, 4, 32, false), BIG_NONE, BIG_NONE},                                  //  64 x 256 tile, 4 waves, 4 x 20 KB
    {BIG_DENSE(64, 1, 2, 64, false), BIG_NONE, BIG_NONE},                                  //  64 x 256 tile, 4 waves, 2 x 40 KB
    {BIG_DENSE(128, 2, 4, 32, false), BIG_SPARSE(128, 2, 4, 32), BIG_NONE},                // 256 x 256 tile, 8 waves, 4 x 32 KB
    {BIG_DENSE(128, 1, 4, 32, false), BIG_SPARSE(128, 1, 4, 32), BIG_NONE},                // 128 x 256 tile, 4 waves, 4 x 24 KB
    {BIG_DENSE(128, 1, 3, 64, true), BIG_NONE, BIG_NONE},                                  // the same six, persistent
    {BIG_DENSE(128, 2, 2, 64, true), BIG_NONE, BIG_NONE},
    {BIG_DENSE(64, 1, 4, 32, true), BIG_NONE, BIG_NONE},
    {BIG_DENSE(64, 1, 2, 64, true), BIG_NONE, BIG_NONE},
    {BIG_DENSE(128, 2, 4, 32, true), BIG_NONE, BIG_NONE},
    {BIG_DENSE(128, 1, 4, 32, true), BIG_NONE, BIG_NONE},
    {256, 64, {DRNMI_KERNEL_ROW(conv_pp_kernel, launch_pp, 1), DRNMI_KERNEL_ROW(conv_pp_kernel, launch_pp, 3)}, BIG_NONE,
     BIG_NONE},
  };
  return k[v];
}

const ConvKernel* strip_kernel(bool i8) {
  static const ConvKernel k[2] = {DRNMI_KERNEL_ROW0(conv_strip_kernel, launch_strip),
                                  DRNMI_KERNEL_ROW0(conv_i8_strip_kernel, launch_strip)};
  return &k[i8];
}

// the 8-bit tiles, one table per code (conv_route.h Q8Variant): KERNEL<KS, ARGS> launched by
// launch_q8<T, KS, ARGS, OCC2>, rows [ks == 3].  (q8_variant sends every 1x1 to the occ2 tile, so the
// KS = 1 rows of tiles 0-3 and the KS = 3 row of the occ2 tile are never picked, for either code.)
#define Q8_ROW(KERNEL, T, OCC2, KS, ...) \
  ConvKernel { #KERNEL "<" #KS ", " #__VA_ARGS__ ">", &launch_unsplit<&launch_q8<T, KS, __VA_ARGS__, OCC2>> }
#define Q8_ROWS(KERNEL, T, OCC2, ...) {Q8_ROW(KERNEL, T, OCC2, 1, __VA_ARGS__), Q8_ROW(KERNEL, T, OCC2, 3, __VA_ARGS__)}
#define Q8_TABLE(KERNEL, OCC2_KERNEL, T)                                                                         \
  {                                                                                                              \
    {256, Q8_ROWS(KERNEL, T, false, 128, 2, 2, 128)},        /* 2 x 64 KB */                                     \
    {128, Q8_ROWS(KERNEL, T, false, 128, 1, 3, 128)},        /* 3 x 48 KB */                                     \
    {256, Q8_ROWS(KERNEL, T, false, 128, 2, 4, 64)},         /* 4 x 32 KB (fp8: K-64 steps on these 64-B rows) */ \
    {128, Q8_ROWS(KERNEL, T, false, 128, 1, 4, 64)},         /* 4 x 24 KB */                                     \
    {128, Q8_ROWS(OCC2_KERNEL, T, true, 128, 1, 2, 64)},     /* 2 x 24 KB, 2 WGs / CU */                         \
  }
const Q8Variant& q8_variant_row(int dtype, int v) {
  static const Q8Variant i8[5] = Q8_TABLE(conv_i8_kernel, conv_i8_occ2_kernel, int8_t);
  static const Q8Variant f8[5] = Q8_TABLE(conv_f8_kernel, conv_f8_occ2_kernel, f8_t);
  return (dtype == DRNMI_F8 ? f8 : i8)[v];
}

// a 256-pixel tile is a run of one output row, the strip of 256 + 2 dil rows fits its buffer
bool strip_ok(const drnmi_conv_args& p) {
  return p.ks == 3 && p.stride == 1 && p.pad == p.dil && p.dil >= 1 && p.dil <= 4 && p.wo % kBPX == 0 &&
         p.x2 == nullptr && p.unit_mask == nullptr && p.cin % 64 == 0 && p.k == 9 * p.cin;
}

// the staggered strip tile (conv_stag.hip): strip geometry, cin % 128 == 0 (an even number of
// 3-step tap groups), optionally with the fused downsample (x2 validated by x2_ok)
bool stag_ok(const drnmi_conv_args& p) {
  const int tco = p.cout <= 128 ? 128 : 256;          // conv_stag128_* / conv_stag_* tile
  return p.ks == 3 && p.stride == 1 && p.pad == p.dil && p.dil >= 1 && p.dil <= 4 && p.wo % kBPX == 0 &&
         p.unit_mask == nullptr && p.cin % 128 == 0 && (p.cout + tco - 1) / tco * tco <= p.cout_pad &&
         (p.x2 == nullptr ? p.k == 9 * p.cin : (p.cin2 % 64 == 0 && p.k == 9 * p.cin + p.cin2));
}

// conv_w1 (conv_w1.hip): the staggered tile's shapes (+ the fused downsample: conv_w1_x2), 256-channel blocks
bool w1_ok(const drnmi_conv_args& p) {
  return stag_ok(p) && p.cout % 256 == 0 && p.scale == nullptr && p.out_dtype == DRNMI_BF16 &&
         p.y_sc == 1 && p.y_sp == p.cout && p.y_sn == static_cast<int64_t>(p.ho) * p.wo * p.cout;
}
// conv_w1h: the same shapes at 128-channel blocks (a 128-pixel run: wo % 128 == 0 follows from stag_ok)
bool w1h_ok(const drnmi_conv_args& p) {
  return stag_ok(p) && p.cout % 128 == 0 && p.scale == nullptr && p.out_dtype == DRNMI_BF16 &&
         p.y_sc == 1 && p.y_sp == p.cout && p.y_sn == static_cast<int64_t>(p.ho) * p.wo * p.cout;
}

// What every conv_big_body tile asks of a launch, whatever its element type (conv_big_body.h): int32 pixel
// offsets and int16 tap coordinates in the row descriptors, a power-of-two cin of at least min_cin (every
// K step inside one tap), whole 128-channel weight blocks, 1x1 or 3x3, no K padding
bool big_body_shape_ok(const drnmi_conv_args& p, int min_cin) {
  return static_cast<int64_t>(p.n) * p.h * p.w * p.cin < (int64_t(1) << 31) && p.h < 16384 && p.w < 16384 &&
         p.cin >= min_cin && (p.cin & (p.cin - 1)) == 0 && p.cout_pad % 128 == 0 && (p.ks == 1 || p.ks == 3) &&
         p.k_pad == p.k;
}

// the 8-bit families' shapes (int8: config C5; fp8: e4m3 bytes): cin >= 64, a non-NULL scale, the
// code's own 8-bit output or bf16 / fp32.  fp8 has no fused second input and no unit skipping and
// refuses them; int8 does not look at those two pointers (its pinned behaviour with them set).
bool q8_conv_supported(const drnmi_conv_args& p) {
  if (p.dtype != DRNMI_I8 && p.dtype != DRNMI_F8) return false;
  if (p.dtype == DRNMI_F8 && (p.x2 != nullptr || p.unit_mask != nullptr)) return false;
  return p.scale != nullptr && big_body_shape_ok(p, 64) && p.k == p.ks * p.ks * p.cin &&
         (p.out_dtype == DRNMI_F32 || p.out_dtype == DRNMI_BF16 || p.out_dtype == p.dtype);
}

// int8 strip-staged B: the 256 x 256 tile with 128-B rows (q8_variant_row 0: cin >= 128, cout % 256 == 0)
bool i8_strip_ok(const drnmi_conv_args& p) {
  return p.cout % 256 == 0 && p.cin % 128 == 0 && strip_ok(p);
}

// 8-bit staggered strip tile (conv_stag.hip, both codes): 128-channel K steps, so cin % 256 == 0
// gives the even number of 3-step tap groups the kernel walks in pairs.  (The fp8 predicate also
// asked cout <= cout_pad: conv_route() refuses cout > cout_pad before any 8-bit route, and both
// routes check rows_exist first, so the term never decided anything.)
bool q8_stag_ok(const drnmi_conv_args& p) {
  return i8_strip_ok(p) && p.cin % 256 == 0 && p.x2 == nullptr;
}

// int8 conv_w1 (conv_w1_i8_kernel): the staggered int8 tile's shapes at 256-channel blocks with a
// dense int8 NHWC output (its 16-B epilogue)
bool i8_w1_ok(const drnmi_conv_args& p) {
  return q8_stag_ok(p) && p.cout % 256 == 0 && p.out_dtype == DRNMI_I8 && p.y_sc == 1 && p.y_sp == p.cout &&
         p.y_sn == static_cast<int64_t>(p.ho) * p.wo * p.cout;
}
// int8 conv_w1h (conv_w1h_i8_kernel: 128 x 128 tiles, two workgroups per CU, odd tap-group counts
// too): whole-row strip geometry, cin % 128 == 0, 128-channel blocks, dense int8 NHWC output
bool i8_w1h_ok(const drnmi_conv_args& p) {
  return strip_ok(p) && p.cin % 128 == 0 && p.cout % 128 == 0 && p.out_dtype == DRNMI_I8 && p.y_sc == 1 &&
         p.y_sp == p.cout && p.y_sn == static_cast<int64_t>(p.ho) * p.wo * p.cout;
}

// second input (fused 1x1 downsample): bf16 NHWC x2 [n][h2][w2][cin2], cin2 a multiple of 64 with
// n*h2*w2*cin2 < 2^31, sampled at (oh*stride2, ow*stride2) inside x2; no residual with it
static bool x2_ok(const drnmi_conv_args& p) {
  if (p.x2 == nullptr) return p.k == p.ks * p.ks * p.cin;
  return p.cin2 >= 64 && p.cin2 % 64 == 0 && p.cin >= 64 && p.res == nullptr && p.unit_mask == nullptr &&
         p.stride2 >= 1 && (p.ho - 1) * p.stride2 < p.h2 && (p.wo - 1) * p.stride2 < p.w2 &&
         static_cast<int64_t>(p.n) * p.h2 * p.w2 * p.cin2 < (int64_t(1) << 31) &&
         p.k == p.ks * p.ks * p.cin + p.cin2;
}

bool big_conv_supported(const drnmi_conv_args& p) {
  return p.dtype == DRNMI_BF16 && big_body_shape_ok(p, kMinCin) && x2_ok(p) &&
         (p.out_dtype == DRNMI_F32 || (p.y_sc == 1 && p.y_sp == p.cout));
}

int weight_unit_mask(const void* wgt, int dtype, int rows_pad, int k_pad, uint32_t* mask, int* count,
                     hipStream_t s) {
  if (wgt == nullptr || mask == nullptr || rows_pad <= 0 || rows_pad % 16 != 0 || k_pad <= 0 || k_pad % 32 != 0)
    return DRNMI_EINVAL;
  const int wpr = (k_pad + 1023) / 1024;
  const int64_t lanes = static_cast<int64_t>(rows_pad / 16) * wpr * 32;
  const unsigned blocks = static_cast<unsigned>((lanes + 255) / 256);
  if (count != nullptr) {
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(int), s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  if (dtype == DRNMI_BF16)
    hipLaunchKernelGGL(unit_mask_kernel<uint16_t>, dim3(blocks), dim3(256), 0, s,
                       reinterpret_cast<const uint16_t*>(wgt), rows_pad, k_pad, wpr, mask, count);
  else if (dtype == DRNMI_F32)
    hipLaunchKernelGGL(unit_mask_kernel<float>, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float*>(wgt),
                       rows_pad, k_pad, wpr, mask, count);
  else
    return DRNMI_EINVAL;
  return static_cast<int>(hipGetLastError());
}

}  // namespace drnmi
extern "C" int drnmi_weight_unit_mask(const void* wgt, int32_t dtype, int32_t rows_pad, int32_t k_pad,
                                      uint32_t* mask, int32_t* nonzero_units, void* stream) {
  return drnmi::weight_unit_mask(wgt, dtype, rows_pad, k_pad, mask, nonzero_units, reinterpret_cast<hipStream_t>(stream));
}
