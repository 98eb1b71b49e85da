// Fused 16-channel BasicBlock (DRN-C layer1: lmodels/drn.py:127-128): conv3x3 16 -> 16 + BN + ReLU,
// conv3x3 16 -> 16 + BN + residual + ReLU, bf16 NHWC, stride 1, dilation 1, on the full-resolution map
// (lmodels/drn.py:27-29 conv3x3, :49-65 BasicBlock.forward; BN folded: eval running stats).
//
// The 16-channel sibling of block64.hip.  Two conv launches move x, t, t, x (the residual) and y
// through HBM: 160 B per pixel; here the intermediate t stays in LDS and the residual is the x row
// already there: 64 B per pixel, which is the bound (the MFMA and LDS-read work is about a third of it).
// One persistent workgroup walks a 254-column strip of a frame down its rows:
//   * waves 0, 1 compute t row j (conv1; 8 of the strip's 16 pixel tiles each) from x rows j-1 .. j+1;
//     waves 2, 3 compute y row j-2 (conv2) from t rows j-3 .. j-1 and add x row j-2 -- the two convs
//     of a step are independent, and one barrier per row step hands t over;
//   * 16 output channels are one v_mfma_f32_16x16x32_bf16 row tile and a K chunk is two taps x 16
//     channels: a conv is 4 chunks and a ninth tap padded with zero weights; a wave keeps its conv's 5
//     A fragments in registers for the whole launch.  B fragments are 16-B LDS reads (pixel fr + tap
//     column, 8 channels): lanes 0-31 read the chunk's first tap, lanes 32-63 its second;
//   * x rows arrive by buffer LDS-DMA one step ahead into a 5-row ring (the oldest row is the
//     residual), t rows live in a 4-row ring; a pixel is 32 B, its two 16-B halves swapped in every
//     second group of 8 pixels (16 consecutive pixels at one half then cover all 64 banks);
//   * the epilogues exchange accumulator halves between two pixel tiles (v_permlane16_swap) so that
//     every lane writes, and reads the residual as, 16 contiguous bytes of one pixel: a wave's y store
//     is 512 contiguous bytes of whole 16-B pieces;
//   * pixels and rows outside the image are zero in both rings (the convs' zero padding);
//   * two workgroups per CU (78 KB of LDS each): one's barrier and DMA waits under the other's work.
#include "common.h"
#include "kernels.h"

#include <cstring>
#include <type_traits>

namespace drnmi {
namespace {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

constexpr int kC = 16;                 // channels (in = mid = out)
constexpr int kOW = 254;               // output columns per strip
constexpr int kTW = 256;               // t columns per strip (16 pixel tiles): image cols c0 - 1 ..
constexpr int kXW = 258;               // x columns per strip: image cols c0 - 2 ..
constexpr int kPixB = 32;              // bytes per pixel (16 bf16)
constexpr int kTileB = 16 * kPixB;     // bytes per 16-pixel tile
constexpr int kXSlot = 9 * 1024;       // 258 pixels (8256 B) padded to whole 1-KB DMA instructions
constexpr int kXRing = 5;              // residual row j-2, conv1 rows j-1 .. j+1, DMA row j+2
constexpr int kTSlot = kTW * kPixB;    // 8192
constexpr int kTRing = 4;
constexpr int kTBase = kXRing * kXSlot;                  // 46080
constexpr int kLds = kTBase + kTRing * kTSlot + 512;     // + slack: conv2 reads t pixels 256, 257 (unstored columns)
constexpr int kChunks = 5;             // K chunks of two taps x 16 channels; the tenth tap is zero weights
constexpr int kTiles = 8;              // pixel tiles per wave
constexpr int kFragB = 16;             // bytes per lane per A fragment
constexpr int kPackW = 2 * kChunks * 64 * kFragB;        // [conv][chunk][lane][8 bf16]
constexpr int kPackBytes = kPackW + 2 * kC * 4;          // + shift1[16], shift2[16]
constexpr unsigned kOob = 0x80000000u;
constexpr int kXPieces = (kXSlot + 1023) / 1024;         // 9 LDS-DMA instructions per x row

struct Block16Params {
  const uint16_t* x;
  const char* pack;
  uint16_t* y;
  int n, h, w, strips, total, per_wg;
};

// which 16-B half of a pixel's 32 B sits first in LDS
__device__ __forceinline__ int hswz(int p) { return (p >> 3) & 1; }

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

template <int OFF>
__device__ __forceinline__ void ds_rd16(u32x4_t& dst, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}

__global__ void __launch_bounds__(256, 2) block16_kernel(const Block16Params a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int role = wave >> 1;          // 0: conv1 (t), 1: conv2 (y)
  const int half = wave & 1;           // pixel tiles 8 half .. + 7 of the strip
  const int fr = lane & 15, fq = lane >> 4;

  // this conv's weight fragments and shift (the accumulator start of the 4 D rows this lane holds)
  u32x4_t wf[kChunks];
  {
    const u32x4_t* pk = reinterpret_cast<const u32x4_t*>(a.pack) + role * kChunks * 64 + lane;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) wf[c] = pk[c * 64];
  }
  f32x4 cinit;
  {
    const float* sh = reinterpret_cast<const float*>(a.pack + kPackW) + role * kC + 4 * fq;
    cinit = f32x4{sh[0], sh[1], sh[2], sh[3]};
  }
  const int H = a.h, W = a.w;
  const __amdgpu_buffer_rsrc_t xs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.x), 0, a.n * H * W * kPixB, 0x00020000);
  const __amdgpu_buffer_rsrc_t ys = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.n * H * W * kPixB, 0x00020000);
  typedef __attribute__((address_space(3))) void lds_t;

  // B fragment of chunk c: this lane's tap is 2 c + (fq >> 1) (the tenth: the ninth again, its
  // weights are zero), channels 8 (fq & 1) .. + 7 of pixel 16 tile + fr + dw in source ring row dh
  int dhc[kChunks];
  uint32_t boff[kChunks];
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const int tap = min(2 * c + (fq >> 1), 8);
    const int dw = tap % 3, p = fr + dw;                 // (bit 3 of the pixel does not depend on the tile)
    dhc[c] = tap / 3;
    boff[c] = half * kTiles * kTileB + p * kPixB + (((fq & 1) ^ hswz(p)) << 4);
  }
  // epilogue pieces after the half exchange: 16 B = channels 8 (fq >> 1) .. + 7 of pixel fr of tile
  // 2 g + (fq & 1) -- conv1: t ring pixel;  conv2: residual = x ring pixel + 2, y = strip column
  const int etile = half * kTiles + (fq & 1);
  const int ep = fr + (role ? 2 : 0);
  const uint32_t eoff = etile * kTileB + ep * kPixB + (((fq >> 1) ^ hswz(ep)) << 4);

  int idx = blockIdx.x * a.per_wg;
  const int end = min(idx + a.per_wg, a.total);
  int ya = 0, yb = 0, n = 0, c0 = 0, img0 = 0;
  // x row DMA (all four waves: instruction i = wave + 4 k of the row's 9)
  auto x_dma = [&](int row) {
    const int slot = ((row % kXRing) + kXRing) % kXRing;
    const bool row_ok = static_cast<unsigned>(row) < static_cast<unsigned>(H);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int i = wave + 4 * k;
      if (i >= kXPieces) break;                        // wave-uniform
      const int byte = i * 1024 + lane * 16;
      const int p = byte >> 5, sl = (byte >> 4) & 1;
      const int col = c0 - 2 + p;
      const bool ok = row_ok && p < kXW && static_cast<unsigned>(col) < static_cast<unsigned>(W);
      const unsigned off = ok ? static_cast<unsigned>(((img0 + row) * W + col) * kPixB + ((sl ^ hswz(p)) << 4)) : kOob;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xs, (lds_t*)(smem + slot * kXSlot + i * 1024), 16, off, 0, 0, 0);
    }
  };
  // next segment: its state and its prologue, x rows ya-2 .. ya (steps start at j = ya - 1; step
  // j issues row j + 2)
  auto begin_segment = [&]() {
    const int seg = idx / H;
    ya = idx - seg * H;
    yb = min(H, ya + (end - idx));
    idx += yb - ya;
    n = seg / a.strips;
    const int s = seg - n * a.strips;
    c0 = kOW * s;                                      // first output column of the strip
    img0 = n * H;
    for (int row = ya - 2; row <= ya; ++row) x_dma(row);
  };
  bool more = idx < end;
  if (more) begin_segment();
  while (more) {
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);

    for (int j = ya - 1; j <= yb + 1; ++j) {
      x_dma(j + 2);
      const int xs_m1 = ((j - 1) % kXRing + kXRing) % kXRing;
      // source rows: conv1 x rows j-1 .. j+1, conv2 t rows j-3 .. j-1
      uint32_t ba[kChunks];
#pragma unroll
      for (int c = 0; c < kChunks; ++c)
        ba[c] = boff[c] + (role == 0 ? static_cast<uint32_t>(((xs_m1 + dhc[c]) % kXRing) * kXSlot)
                                     : static_cast<uint32_t>(kTBase + ((j - 3 + dhc[c]) & 3) * kTSlot));
      f32x4 acc[kTiles];
#pragma unroll
      for (int fn = 0; fn < kTiles; ++fn) acc[fn] = cinit;
      // entries (chunk, pixel tile): one B read, one MFMA; reads run PF entries ahead with counted lgkmcnt
      constexpr int NE = kChunks * kTiles, PF = 4;
      u32x4_t bq[PF + 1];
      auto issue_rd = [&](auto e_c) {
        constexpr int E = decltype(e_c)::value;
        constexpr int KS = E / kTiles, FN = E % kTiles;
        ds_rd16<FN * kTileB>(bq[E % (PF + 1)], ba[KS]);
      };
      static_for<0, PF>(issue_rd);
      auto entry = [&](auto e_c) {
        constexpr int E = decltype(e_c)::value;
        constexpr int KS = E / kTiles, FN = E % kTiles;
        if constexpr (E + PF < NE) issue_rd(std::integral_constant<int, E + PF>{});
        constexpr int AHEAD = (E + PF < NE ? E + PF : NE - 1) - E;
        asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(AHEAD) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        acc[FN] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[KS]),
                                                          __builtin_bit_cast(bf16x8, bq[E % (PF + 1)]), acc[FN], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      };
      static_for<0, NE>(entry);
      if (role == 0) {
        // conv1 epilogue: ReLU -> bf16 into t ring slot j & 3; pixels outside the image (or rows) = 0
        const bool row_ok = static_cast<unsigned>(j) < static_cast<unsigned>(H);
        const uint32_t tb = static_cast<uint32_t>(kTBase + (j & 3) * kTSlot);
#pragma unroll
        for (int g = 0; g < kTiles / 2; ++g) {
          uint4 v;
          {
            const int col = c0 - 1 + (half * kTiles + 2 * g) * 16 + fr;
            const bool ok0 = row_ok && static_cast<unsigned>(col) < static_cast<unsigned>(W);
            const bool ok1 = row_ok && static_cast<unsigned>(col + 16) < static_cast<unsigned>(W);
            const f32x4& a0 = acc[2 * g];
            const f32x4& a1 = acc[2 * g + 1];
            v.x = ok0 ? pk_bf16x2(f32x2_t{fmaxf(a0[0], 0.f), fmaxf(a0[1], 0.f)}) : 0u;
            v.y = ok0 ? pk_bf16x2(f32x2_t{fmaxf(a0[2], 0.f), fmaxf(a0[3], 0.f)}) : 0u;
            v.z = ok1 ? pk_bf16x2(f32x2_t{fmaxf(a1[0], 0.f), fmaxf(a1[1], 0.f)}) : 0u;
            v.w = ok1 ? pk_bf16x2(f32x2_t{fmaxf(a1[2], 0.f), fmaxf(a1[3], 0.f)}) : 0u;
          }
          swap_halves(v);
          *reinterpret_cast<uint4*>(smem + tb + eoff + 2 * g * kTileB) = v;
        }
      } else {
        // conv2 epilogue: + residual (x ring row j - 2), ReLU, bf16 NHWC store (buffer: dropped if not ours)
        const int yrow = j - 2;
        const bool row_ok = yrow >= ya && yrow < yb;
        const uint32_t xb = static_cast<uint32_t>(((yrow % kXRing + kXRing) % kXRing) * kXSlot);
#pragma unroll
        for (int g = 0; g < kTiles / 2; ++g) {
          uint4 rv = *reinterpret_cast<const uint4*>(smem + xb + eoff + 2 * g * kTileB);
          swap_halves(rv);                             // -> channels 4 fq .. + 3 of pixel fr of tiles 2 g, 2 g + 1
          const f32x4& a0 = acc[2 * g];
          const f32x4& a1 = acc[2 * g + 1];
          const f32x2_t r0 = widen_bf16x2(rv.x), r1 = widen_bf16x2(rv.y), r2 = widen_bf16x2(rv.z), r3 = widen_bf16x2(rv.w);
          uint4 v;
          v.x = pk_bf16x2(f32x2_t{fmaxf(a0[0] + r0[0], 0.f), fmaxf(a0[1] + r0[1], 0.f)});
          v.y = pk_bf16x2(f32x2_t{fmaxf(a0[2] + r1[0], 0.f), fmaxf(a0[3] + r1[1], 0.f)});
          v.z = pk_bf16x2(f32x2_t{fmaxf(a1[0] + r2[0], 0.f), fmaxf(a1[1] + r2[1], 0.f)});
          v.w = pk_bf16x2(f32x2_t{fmaxf(a1[2] + r3[0], 0.f), fmaxf(a1[3] + r3[1], 0.f)});
          swap_halves(v);
          const int pc = (etile + 2 * g) * 16 + fr;    // strip column
          const int col = c0 + pc;
          const bool ok = row_ok && pc < kOW && col < W;
          const unsigned ob = ok ? static_cast<unsigned>(((img0 + yrow) * W + col) * kPixB + (fq >> 1) * 16) : kOob;
          __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{v.x, v.y, v.z, v.w}, ys, ob, 0, 0);
        }
      }
      // this wave's DMA pieces of row j + 2 (issued at the start of this step; younger: the conv2
      // waves' 4 stores) must have landed before the barrier hands the t row and the x row over.  In
      // the code the compiler emits they already have: it counts an LDS-DMA as an LDS write and puts
      // s_waitcnt vmcnt(0) before the epilogue's first plain LDS access (the t write, the residual
      // read), so the DMA has the MFMA chain to land, not the epilogue as well, and the conv2 waves
      // drain their previous row's stores there too.  These waits are then free; they stay as the
      // statement of what the barrier needs.
      if (role == 0) asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    more = idx < end;
    if (more) begin_segment();
  }
}

int g_block16_wgs = 0;

}  // namespace
}  // namespace drnmi

using namespace drnmi;

extern "C" int64_t drnmi_block16_pack_bytes(void) { return kPackBytes; }

// OIHW fp32 weights of the block's two 16 -> 16 3x3 convs, eval-BN scale / shift per channel -> the
// kernel's blob: per (conv, chunk c, lane (fr, fq)) the 8 bf16 A[fr][8 fq + e] =
// w[fr][8 (fq & 1) + e][kh][kw] * scale[fr] (RNE) of tap 2 c + (fq >> 1) = 3 kh + kw (tap 9: zeros),
// then the two shift vectors.
extern "C" int drnmi_block16_pack(const float* w1, const float* scale1, const float* shift1, const float* w2,
                                  const float* scale2, const float* shift2, void* out_host) {
  if (w1 == nullptr || scale1 == nullptr || shift1 == nullptr || w2 == nullptr || scale2 == nullptr ||
      shift2 == nullptr || out_host == nullptr)
    return DRNMI_EINVAL;
  char* out = static_cast<char*>(out_host);
  auto bf = [](float v) -> uint16_t {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return static_cast<uint16_t>(u >> 16);
  };
  const float* ws[2] = {w1, w2};
  const float* sc[2] = {scale1, scale2};
  const float* shv[2] = {shift1, shift2};
  uint16_t* o = reinterpret_cast<uint16_t*>(out);
  for (int cv = 0; cv < 2; ++cv)
    for (int c = 0; c < kChunks; ++c)
      for (int ln = 0; ln < 64; ++ln) {
        const int co = ln & 15, fq = ln >> 4;
        const int tap = 2 * c + (fq >> 1), kh = tap / 3, kw = tap % 3;
        for (int e = 0; e < 8; ++e) {
          const int ci = 8 * (fq & 1) + e;
          const float v = tap < 9 ? ws[cv][((co * kC + ci) * 3 + kh) * 3 + kw] * sc[cv][co] : 0.f;
          o[((cv * kChunks + c) * 64 + ln) * 8 + e] = bf(v);
        }
      }
  float* sh = reinterpret_cast<float*>(out + kPackW);
  for (int cv = 0; cv < 2; ++cv)
    for (int c = 0; c < kC; ++c) sh[cv * kC + c] = shv[cv][c];
  return 0;
}

// the buffer resources hold the byte size n * h * w * 32 in 32 bits, and offsets >= 2^31 mark "outside"
extern "C" int drnmi_block16_supported(int32_t n, int32_t h, int32_t w) {
  return n >= 1 && h >= 1 && w >= 1 && static_cast<int64_t>(n) * h * w * kPixB < (int64_t(1) << 31) ? 1 : 0;
}

extern "C" int drnmi_basic_block16(const void* x, const void* pack, void* y, int32_t n, int32_t h, int32_t w,
                                   void* stream) {
  if (x == nullptr || pack == nullptr || y == nullptr || !drnmi_block16_supported(n, h, w)) return DRNMI_EINVAL;
  if (x == y) return DRNMI_EINVAL;                     // the residual is read while y is written
  if (g_block16_wgs == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    g_block16_wgs = 2 * cus;                           // two workgroups per CU
  }
  Block16Params p;
  p.x = static_cast<const uint16_t*>(x);
  p.pack = static_cast<const char*>(pack);
  p.y = static_cast<uint16_t*>(y);
  p.n = n;
  p.h = h;
  p.w = w;
  p.strips = (w + kOW - 1) / kOW;
  p.total = n * p.strips * h;
  p.per_wg = (p.total + g_block16_wgs - 1) / g_block16_wgs;
  const int grid = (p.total + p.per_wg - 1) / p.per_wg;
  return static_cast<int>(launch_lds<&block16_kernel>(dim3(grid), dim3(256), kLds, static_cast<hipStream_t>(stream), p));
}
