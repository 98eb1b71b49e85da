// Split-K bf16 implicit-GEMM convolution for grids that leave most CUs idle (the low-latency mode:
// one small frame per call, DRNSeg.set_low_latency; include/drnmi.h drnmi_conv_splitk).
//
// One 300 x 300 frame is 38 x 38 = 1444 pixels at DRN-D layer4..8: on the 256 x 256 tiles of
// conv_big.hip a 512 -> 512 3x3 conv is 12 workgroups, each walking K = 4608 alone on a 256-CU part.
// This kernel cuts the same GEMM the other way:
//   * Tile: 128 output channels x 64 pixels, 4 waves (2 channel halves x 2 pixel halves, 64 x 32 per
//     wave: 4 x 2 accumulator fragments of v_mfma_f32_16x16x32_bf16, A = weights, B = pixels, as
//     conv_big).  Pixels are M = n ho wo flattened, so tiles cross row and image boundaries.
//   * K steps of one tap x 64 channels in the packed order k = (kh ks + kw) cin + ci (step kt is
//     weight columns 64 kt .. 64 kt + 63).  The steps are cut into S contiguous near-equal parts,
//     the remainder steps going to the first parts; the grid is tiles x S workgroups.
//   * Operands go global -> LDS by LDS-DMA (conv_tile.h glds16) into a 3-stage ring of 24 KB stages
//     (16 KB of weight rows, 8 KB of pixel rows, 128-B rows with conv_big's chunk swizzle): 72 KB, two
//     workgroups per CU.  The im2col is in the DMA source addresses; a tap outside the image reads the
//     zero page.  One counted vmcnt wait and one barrier per step; the step after next is issued
//     right after the barrier, into the stage every wave has just left.
//   * Workgroups are dealt XCD-major with the pixel tiles of one (channel tile, K part) adjacent, so
//     the weight slice they share is fetched into one XCD's L2 once.
//
// One launch, no waiting.  With S > 1 each workgroup stores its fp32 partial tile to
// ws[S][M][cout_pad] and then publishes it at agent scope: every wave waits for its stores, the
// workgroup meets at a barrier, and one lane takes the tile's ticket with an agent-scope
// acquire-release atomic add (performed at memory, not in an L2).  Its release is, on gfx950, a
// write-back of the XCD's L2: the partials are then in memory, which is what the L2 of another XCD
// reads.  A workgroup that does not draw ticket S - 1 exits: nobody spins.  The one that does has
// seen S - 1 release sequences on the ticket; its acquire invalidates the CU's L1 and the XCD's L2
// lines another XCD may have written since they were cached (the workspace is reused launch after
// launch, so stale lines are the normal case), and the barrier that hands the ticket to the other
// lanes orders their loads after it.  It adds the S partials in split order 0 .. S - 1,
// its own included and read back like the others, so the sum is a function of (shape, S) alone,
// applies the epilogue (conv_tile.h store_tile: acc * scale + shift, residual, ReLU, bf16 or fp32
// at any output strides) and stores 0 to the ticket for the next launch or graph replay.  S = 1
// touches neither workspace nor ticket.
#include "common.h"
#include "conv_route.h"
#include "conv_tile.h"

namespace drnmi {
namespace {

constexpr int kRowB = kSkBK * 2;                         // bytes per LDS row
constexpr int kABytes = kSkBCO * kRowB, kBBytes = kSkBPX * kRowB, kStage = kABytes + kBBytes;
constexpr int kNST = 3;
constexpr int kLds = kNST * kStage;
constexpr int kAInstr = kSkBCO / 8 / 4, kBInstr = kSkBPX / 8 / 4;   // 1-KB DMA instructions per wave per step
constexpr int kGlds = kAInstr + kBInstr;
constexpr int kFM = 4, kFN = 2, kWCO = 64, kPXW = 32;    // per wave: 64 channels x 32 pixels
static_assert(kRowB == 128 && kLds <= 80 * 1024, "128-B rows; two workgroups per CU");

template <int KS>
__global__ void __launch_bounds__(256, 2)
conv_sk_kernel(const drnmi_conv_args p, const int S, int* __restrict__ tickets, float* part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_ticket;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave >> 1, wp = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int nco = (p.cout + kSkBCO - 1) / kSkBCO;
  const int npx = (M + kSkBPX - 1) / kSkBPX;
  const int H = p.h, W = p.w, cin = p.cin, dil = p.dil;
  const int lc = 31 - __builtin_clz(cin);
  const uint16_t* __restrict__ x = reinterpret_cast<const uint16_t*>(p.x);
  const uint16_t* __restrict__ wt = reinterpret_cast<const uint16_t*>(p.wgt);

  // workgroup -> (pixel tile, channel tile, K part): pixel tiles innermost
  const int lid = xcd_remap2(blockIdx.x, gridDim.x);
  const int grp = lid / npx;
  const int pxt = lid - grp * npx;
  const int split = grp / nco;
  const int cot = grp - split * nco;
  const int tile = pxt * nco + cot;
  const int px0 = pxt * kSkBPX, co0 = cot * kSkBCO;
  const int nsteps = p.k / kSkBK;
  const int base = nsteps / S, rem = nsteps - base * S;
  const int kt0 = split * base + (split < rem ? split : rem);
  const int cnt = base + (split < rem ? 1 : 0);           // >= 1: S <= nsteps (sk_route)

  // DMA assignment: one wave instruction fills 8 LDS rows; lane l fills row 8 j + l / 8, slot l % 8
  const int lrow = lane >> 3, lslot = lane & 7;
  int a_off[kAInstr], b_off[kBInstr], b_ih[kBInstr], b_iw[kBInstr];
#pragma unroll
  for (int i = 0; i < kAInstr; ++i) {
    const int r = (wave * kAInstr + i) * 8 + lrow;
    a_off[i] = (co0 + r) * p.k_pad + swzb<kRowB>(r, lslot) * 8;
  }
#pragma unroll
  for (int i = 0; i < kBInstr; ++i) {
    const int r = (wave * kBInstr + i) * 8 + lrow;
    const int m = px0 + r;
    b_ih[i] = b_iw[i] = -(1 << 20);                       // no pixel: every tap reads zeros
    b_off[i] = 0;
    if (m < M) {
      const int n = m / hw_o;
      const int q = m - n * hw_o;
      const int oh = q / p.wo;
      const int ow = q - oh * p.wo;
      b_ih[i] = oh * p.stride - p.pad;
      b_iw[i] = ow * p.stride - p.pad;
      // (only dereferenced with the tap's offset added and that tap inside the image)
      b_off[i] = ((n * H + b_ih[i]) * W + b_iw[i]) * cin + swzb<kRowB>(r, lslot) * 8;
    }
  }
  const char* zero_src = reinterpret_cast<const char*>(g_zero_page) + lane * 16;

  auto issue = [&](int kt, int stage) {
    const int k0 = kt * kSkBK;
    const int tap = k0 >> lc;
    const int kh = tap / KS, kw = tap - kh * KS;
    const int dh = kh * dil, dw = kw * dil;
    const int toff = (dh * W + dw) * cin + (k0 & (cin - 1));
    char* sa = smem + stage * kStage;
#pragma unroll
    for (int i = 0; i < kAInstr; ++i) glds16(wt + (a_off[i] + k0), sa + (wave * kAInstr + i) * 1024);
#pragma unroll
    for (int i = 0; i < kBInstr; ++i) {
      const bool ok = static_cast<unsigned>(b_ih[i] + dh) < static_cast<unsigned>(H) &&
                      static_cast<unsigned>(b_iw[i] + dw) < static_cast<unsigned>(W);
      const void* src = ok ? static_cast<const void*>(x + (b_off[i] + toff)) : static_cast<const void*>(zero_src);
      glds16(src, sa + kABytes + (wave * kBInstr + i) * 1024);
    }
  };

  f32x4 acc[kFM][kFN];
  zero_tile(acc);
  for (int t = 0; t < kNST - 1 && t < cnt; ++t) issue(kt0 + t, t);

  for (int t = 0; t < cnt; ++t) {
    // retire step t: one newer step may stay in flight
    if (t + 1 < cnt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kGlds) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // every wave has left stage (t - 1) % 3 = (t + 2) % 3
    if (t + kNST - 1 < cnt) issue(kt0 + t + kNST - 1, (t + kNST - 1) % kNST);
    const char* sa = smem + (t % kNST) * kStage;
    const char* sb = sa + kABytes;
#pragma unroll
    for (int sub = 0; sub < kRowB / 64; ++sub) {
      bf16x8 af[kFM], bfr[kFN];
      const int c = sub * 4 + fq;
#pragma unroll
      for (int h = 0; h < kFM; ++h) {
        const int r = wc * kWCO + h * 16 + fr;
        af[h] = *reinterpret_cast<const bf16x8*>(sa + r * kRowB + swzb<kRowB>(r, c) * 16);
      }
#pragma unroll
      for (int fn = 0; fn < kFN; ++fn) {
        const int r = wp * kPXW + fn * 16 + fr;
        bfr[fn] = *reinterpret_cast<const bf16x8*>(sb + r * kRowB + swzb<kRowB>(r, c) * 16);
      }
#pragma unroll
      for (int h = 0; h < kFM; ++h)
#pragma unroll
        for (int fn = 0; fn < kFN; ++fn)
          acc[h][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[h], bfr[fn], acc[h][fn], 0, 0, 0);
    }
  }

  if (S > 1) {
    const int64_t cp = p.cout_pad;
    const int64_t plane = static_cast<int64_t>(M) * cp;
    // lane (fr, fq) holds channels co .. co + 3 of pixel m per fragment: one 16-B piece of the row
    auto piece = [&](int h, int fn) {
      return (static_cast<int64_t>(px0 + wp * kPXW + fn * 16 + fr)) * cp + (co0 + wc * kWCO + h * 16 + fq * 4);
    };
    float* mine = part + split * plane;
#pragma unroll
    for (int fn = 0; fn < kFN; ++fn) {
      if (px0 + wp * kPXW + fn * 16 + fr >= M) continue;
#pragma unroll
      for (int h = 0; h < kFM; ++h)
        *reinterpret_cast<float4*>(mine + piece(h, fn)) = make_float4(acc[h][fn][0], acc[h][fn][1], acc[h][fn][2], acc[h][fn][3]);
    }
    // One agent-scope release and acquire per workgroup, by the lane that takes the ticket: a fence
    // per wave measured 100 us for the 460 workgroups of a 512 -> 512 3x3 on 38 x 38 (each is a
    // write-back or an invalidate of the whole L2).  The other lanes' stores happen before it through
    // the workgroup-scope release / barrier / acquire of __syncthreads() (scopes are inclusive and
    // release is cumulative); in the hardware their stores are in this XCD's L2 once vmcnt is 0, ahead
    // of the barrier, so the one write-back covers them, and the one invalidate ahead of the second
    // barrier covers the L1 and L2 every lane of the workgroup reads through.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(tickets + tile, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != S - 1) return;
    // split order 0 .. S - 1 per element; a part's eight pieces per lane are loaded together
    zero_tile(acc);
    for (int s = 0; s < S; ++s) {
      const float* src = part + s * plane;
#pragma unroll
      for (int fn = 0; fn < kFN; ++fn) {
        if (px0 + wp * kPXW + fn * 16 + fr >= M) continue;
#pragma unroll
        for (int h = 0; h < kFM; ++h) {
          const float4 u = *reinterpret_cast<const float4*>(src + piece(h, fn));
          if (s == 0) acc[h][fn] = f32x4{u.x, u.y, u.z, u.w};     // (not 0 + u: keeps a -0 partial's sign)
          else acc[h][fn] += f32x4{u.x, u.y, u.z, u.w};
        }
      }
    }
    if (tid == 0) __hip_atomic_store(tickets + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  store_tile<kFM, kWCO, kFN, true>(p, acc, px0, co0, wc, wp, fr, fq);
}

template <int KS>
hipError_t launch_sk(const drnmi_conv_args& p, int splits, hipStream_t s) {
  const int64_t tiles = sk_tiles(p);
  int* tickets = reinterpret_cast<int*>(p.ws);
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(p.ws) + sk_ticket_bytes(p));
  return launch_lds<&conv_sk_kernel<KS>>(dim3(static_cast<unsigned>(tiles * splits)), dim3(256), kLds, s, p, splits,
                                         splits > 1 ? tickets : nullptr, splits > 1 ? part : nullptr);
}

}  // namespace

int64_t sk_tiles(const drnmi_conv_args& p) {
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  return ((M + kSkBPX - 1) / kSkBPX) * ((p.cout + kSkBCO - 1) / kSkBCO);
}
// the tickets lead the workspace, one int32 per tile, padded to 256 B; the partials follow
int64_t sk_ticket_bytes(const drnmi_conv_args& p) { return (sk_tiles(p) * 4 + 255) / 256 * 256; }

// The kernel's contract but the pointers that select another form (x2, unit_mask: sk_route) and the
// weight rows (rows_exist): bf16, cin a power of two >= 64 (a K step lies inside one tap), ks 1 / 3,
// k_pad == k, cout_pad % 128 == 0, conv_big's output forms; int32 element offsets into x, the
// weights and one partial plane's rows
bool sk_conv_supported(const drnmi_conv_args& p) {
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  return p.dtype == DRNMI_BF16 && big_body_shape_ok(p, kSkBK) && p.k == p.ks * p.ks * p.cin &&
         static_cast<int64_t>(p.cout_pad) * p.k_pad < (int64_t(1) << 31) && M < (int64_t(1) << 31) - kSkBPX &&
         sk_tiles(p) * kSkMaxSplits < (int64_t(1) << 31) &&
         (p.out_dtype == DRNMI_F32 || (p.out_dtype == DRNMI_BF16 && p.y_sc == 1 && p.y_sp == p.cout));
}

const ConvKernel* sk_kernel(int ks) {
  static const ConvKernel k[2] = {{"conv_sk_kernel<1>", &launch_sk<1>}, {"conv_sk_kernel<3>", &launch_sk<3>}};
  return ks == 1 ? &k[0] : ks == 3 ? &k[1] : nullptr;
}

}  // namespace drnmi
