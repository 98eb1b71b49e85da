// Block-scaled e4m3 ("mxfp8", dtype DRNMI_MXF8, include/drnmi.h) NHWC implicit-GEMM convolution on the scaled MFMA
// v_mfma_scale_f32_16x16x128_f8f6f4, with the quantiser, its inverse and the weight pack.  This file alone knows
// how an image and a weight blob are laid out.
//
// Storage.  An image of an [m][c] NHWC value: the e4m3 elements uint8 [m][c], then the E8M0 scale bytes uint8
// [m][c / 32] (block b of row r covers channels 32 b .. 32 b + 31), the whole rounded up to 16 bytes.  A weight
// blob of [cout_pad][k_pad]: the elements uint8 [cout_pad][k_pad], then the scale bytes [cout_pad][k_pad / 32].
// With cin a power of two >= 128 the four scale bytes of one K step (128 channels of one tap) are one aligned
// dword of a row, for pixels and weight rows alike.
//
// Tile: 128 output channels x 128 pixels, four waves of 64 x 64 (FM 4, FN 4: 16 scaled MFMAs per K step against
// 16 ds_read_b128 and 8 ds_read_b32), two workgroups per CU.  K step = 128 channels of one tap; steps run
// channel-block-major, taps innermost (the taps of one channel slice re-read the same pixel neighbourhood), on a
// two-stage ring filled by LDS DMA (conv_tile.h glds16 / glds4), one barrier per step.  A stage (33 KB):
//   A    128 weight rows x 128 B, 16-B chunk c of row r at slot c ^ ((r >> 1) & 7) (conv_tile.h swzb<128>);
//   B    128 pixel rows x 128 B likewise; a tap outside the image comes from the zero page (e4m3 +0);
//   SA   128 dwords: the step's four scale bytes of every weight row (DMA'd by waves 0, 1, one 4-B piece each);
//   SB   128 dwords: those of every pixel (waves 2, 3); a tap outside the image reads the zero page: byte 0.
// Operand map of the scaled instruction, measured on gfx950 with one-hot operands (lane = 16 fq + fr): a lane's 32
// bytes are K 16 fq .. 16 fq + 15 (registers 0-3) and K 64 + 16 fq .. + 15 (registers 4-7): the chunks fq and 4 + fq
// of a 128-B row, as the fp8 tiles read them; the scale of K block kb (K 32 kb .. + 31) of row / column fr is
// taken from lane (fr, kb), byte op_sel of its scale register.  So a lane's data lie in two blocks (fq >> 1 and
// 2 + (fq >> 1)) whose scales other lanes supply, and lane (fr, fq) supplies the scale of block fq: byte fq of the
// row's dword, one shift, op_sel 0.  The scale operands are registers, so the instruction keeps its scaled form.
// Epilogue (fp contraction off): v = acc * scale[co] + shift[co]; v += value(res) (a residual image: element x
// 2^(byte - 127), exact); ReLU.  out_dtype DRNMI_F32 / DRNMI_BF16: the strided stores of the 8-bit tiles.
// DRNMI_MXF8: the wave's 64 channels of a pixel are two blocks; a block lies in accumulator fragments 2 b and
// 2 b + 1 of the four lanes (fr, 0..3): the lane's max over its 8 values, two cross-lane steps (lanes ^ 16, ^ 32),
// the shared exponent from the maximum's bits, the 8 values scaled exactly and packed to e4m3, two 4-B stores per
// lane and one byte store of the scale by lane (fr, 0).  All stores are vector stores.
#include <cmath>
#include <string.h>

#include "common.h"
#include "conv_tile.h"
#include "kernels.h"

namespace drnmi {
namespace {

constexpr int kMxBCO = 128, kMxBPX = 128, kMxBK = 128;
constexpr int kMxA = kMxBCO * kMxBK, kMxB = kMxBPX * kMxBK, kMxSA = kMxBCO * 4, kMxSB = kMxBPX * 4;
constexpr int kMxStage = kMxA + kMxB + kMxSA + kMxSB;
constexpr int kMxLds = 2 * kMxStage;
static_assert(2 * kMxLds <= 160 * 1024, "two workgroups per CU");

// The stored scale byte E + 127 of a block whose largest magnitude has the fp32 bits `abs_bits` (include/drnmi.h
// DRNMI_MXF8): amax = m 2^e, E = e - 8 for m <= 1.75 and e - 7 above, clamped to [0, 254]; 0 for amax = 0.
__host__ __device__ inline uint32_t mx_scale_byte(uint32_t abs_bits) {
  const int b = static_cast<int>(abs_bits >> 23) - 8 + ((abs_bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  return static_cast<uint32_t>(b < 0 ? 0 : (b > 254 ? 254 : b));
}
// fp32 bits of 2^-E = 2^(127 - byte)
__host__ __device__ inline uint32_t mx_inv_scale_bits(uint32_t byte) { return (254u - byte) << 23; }

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// four e4m3 bytes of w times 2^e
__device__ __forceinline__ void mx_unpack4(uint32_t w, int e, float (&o)[4]) {
  o[0] = ldexpf(f8_to_f32<0>(w), e);
  o[1] = ldexpf(f8_to_f32<1>(w), e);
  o[2] = ldexpf(f8_to_f32<2>(w), e);
  o[3] = ldexpf(f8_to_f32<3>(w), e);
}

// --- the quantiser: one lane per 32-channel block (64 / 128 B in, 32 B + 1 B out)
template <typename T>
__global__ void __launch_bounds__(256) quantize_mx8_kernel(const T* __restrict__ x, uint8_t* __restrict__ img, int64_t nblk) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  uint8_t* __restrict__ scales = img + nblk * 32;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nblk; i += stride) {
    float f[32];
    uint32_t am = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const Vec8<T> v = Vec8<T>::load(x + i * 32 + g * 8);
      const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f[g * 8 + j] = Elem<T>::to_f32(e[j]);
        const uint32_t b = abs_bits(f[g * 8 + j]);
        am = b > am ? b : am;
      }
    }
    const uint32_t byte = mx_scale_byte(am);
    const float inv = __uint_as_float(mx_inv_scale_bits(byte));
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      w[j] = pk_f8x4(__fmul_rn(f[4 * j], inv), __fmul_rn(f[4 * j + 1], inv), __fmul_rn(f[4 * j + 2], inv), __fmul_rn(f[4 * j + 3], inv));
    *reinterpret_cast<uint4*>(img + i * 32) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint4*>(img + i * 32 + 16) = make_uint4(w[4], w[5], w[6], w[7]);
    scales[i] = static_cast<uint8_t>(byte);
  }
}

__global__ void __launch_bounds__(256) dequantize_mx8_kernel(const uint8_t* __restrict__ img, float* __restrict__ y, int64_t nblk) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const uint8_t* __restrict__ scales = img + nblk * 32;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nblk; i += stride) {
    const uint4 a = *reinterpret_cast<const uint4*>(img + i * 32), b = *reinterpret_cast<const uint4*>(img + i * 32 + 16);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int e = static_cast<int>(scales[i]) - 127;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float o[4];
      mx_unpack4(w[j], e, o);
      *reinterpret_cast<float4*>(y + i * 32 + j * 4) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

// --- the epilogue: lane (fr, fq) holds channels 16 f + 4 fq .. + 3 of pixel fn * 16 + fr of the wave's 64 x 64
__device__ __forceinline__ void mx_store_tile(const drnmi_conv_args& p, const f32x4 (&acc)[4][4], int px0, int co0, int wc,
                                              int wp, int fr, int fq) {
#pragma clang fp contract(off)
  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int cout = p.cout;
  const int c32 = cout >> 5;
  const uint8_t* __restrict__ res = reinterpret_cast<const uint8_t*>(p.res);
  const uint8_t* __restrict__ res_s = res + static_cast<int64_t>(M) * cout;
  uint8_t* __restrict__ yq = reinterpret_cast<uint8_t*>(p.y);
  uint8_t* __restrict__ yq_s = yq + static_cast<int64_t>(M) * cout;
  const bool relu = p.relu != 0;
  const bool out_mx = p.out_dtype == DRNMI_MXF8;
  const bool nhwc16 = p.out_dtype == DRNMI_BF16 && p.y_sc == 1 && (p.y_sp & 3) == 0 && (p.y_sn & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(p.y) & 7) == 0;
  // fp32 NHWC rows, 16-B aligned: a partial 4-channel group is stored whole only into the pixel's own padding
  // (rows exactly round_up(cout, 4) wide), as store_tile_q8 does
  const bool nhwc32 = p.out_dtype == DRNMI_F32 && p.y_sc == 1 && (p.y_sp & 3) == 0 && (p.y_sn & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(p.y) & 15) == 0;
  const bool pad_row = p.y_sp == ((cout + 3) & ~3);
#pragma unroll
  for (int fn = 0; fn < 4; ++fn) {
    const int m = px0 + wp * 64 + fn * 16 + fr;
    const bool inb = m < M;
    const int n = m / hw_o;
    const int q = m - n * hw_o;
    const int64_t ybase = static_cast<int64_t>(n) * p.y_sn + static_cast<int64_t>(q) * p.y_sp;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int cob = co0 + wc * 64 + b * 32;       // the block's first channel
      float v[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int co = cob + h * 16 + fq * 4;
        const float4 sc = *reinterpret_cast<const float4*>(p.scale + co);   // padded to cout_pad
        const float4 sh = *reinterpret_cast<const float4*>(p.shift + co);
        const f32x4 c = acc[2 * b + h][fn];
        v[h][0] = c[0] * sc.x + sh.x;
        v[h][1] = c[1] * sc.y + sh.y;
        v[h][2] = c[2] * sc.z + sh.z;
        v[h][3] = c[3] * sc.w + sh.w;
        if (res != nullptr && inb && co < cout) {   // a residual image: cout % 32 == 0
          const uint32_t rw = *reinterpret_cast<const uint32_t*>(res + static_cast<int64_t>(m) * cout + co);
          float r[4];
          mx_unpack4(rw, static_cast<int>(res_s[static_cast<int64_t>(m) * c32 + (co >> 5)]) - 127, r);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[h][j] = v[h][j] + r[j];
        }
        if (relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[h][j] = fmaxf(v[h][j], 0.f);
        }
      }
      if (out_mx) {
        // the block's largest magnitude: 8 values of this lane, then the lanes (fr, 0..3)
        uint32_t am = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t t = abs_bits(v[h][j]);
            am = t > am ? t : am;
          }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const uint32_t t = static_cast<uint32_t>(__shfl_xor(static_cast<int>(am), o));
          am = t > am ? t : am;
        }
        const uint32_t byte = mx_scale_byte(am);
        const float inv = __uint_as_float(mx_inv_scale_bits(byte));
        if (inb && cob < cout) {                    // an image: dense rows, cout % 32 == 0
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<uint32_t*>(yq + static_cast<int64_t>(m) * cout + cob + h * 16 + fq * 4) =
                pk_f8x4(v[h][0] * inv, v[h][1] * inv, v[h][2] * inv, v[h][3] * inv);
          if (fq == 0) yq_s[static_cast<int64_t>(m) * c32 + (cob >> 5)] = static_cast<uint8_t>(byte);
        }
        continue;
      }
      if (!inb) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int co = cob + h * 16 + fq * 4;
        if (co >= cout) continue;
        const bool full = co + 3 < cout;
        if (nhwc32 && (full || pad_row)) {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + ybase + co) = make_float4(v[h][0], v[h][1], v[h][2], v[h][3]);
        } else if (nhwc16 && full) {
          uint2 o;
          o.x = static_cast<uint32_t>(f32_to_bf16(v[h][0])) | (static_cast<uint32_t>(f32_to_bf16(v[h][1])) << 16);
          o.y = static_cast<uint32_t>(f32_to_bf16(v[h][2])) | (static_cast<uint32_t>(f32_to_bf16(v[h][3])) << 16);
          *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.y) + ybase + co) = o;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (co + j >= cout) break;
            const int64_t off = ybase + static_cast<int64_t>(co + j) * p.y_sc;
            if (p.out_dtype == DRNMI_BF16) reinterpret_cast<uint16_t*>(p.y)[off] = f32_to_bf16(v[h][j]);
            else reinterpret_cast<float*>(p.y)[off] = v[h][j];
          }
        }
      }
    }
  }
}

// --- the conv
template <int KS>
__global__ void __launch_bounds__(256)
conv_mx_kernel(const drnmi_conv_args p) {
  constexpr int TAPS = KS * KS;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wc = wave >> 1;         // 64-channel half of the tile
  const int wp = wave & 1;          // 64-pixel half
  const int fr = lane & 15;
  const int fq = lane >> 4;
  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int nco = (p.cout + kMxBCO - 1) / kMxBCO;
  const int npx = (M + kMxBPX - 1) / kMxBPX;
  const int tile = xcd_remap2(blockIdx.x, npx * nco);
  const int px0 = (tile / nco) * kMxBPX;
  const int co0 = (tile % nco) * kMxBCO;

  const int cin = p.cin, H = p.h, W = p.w, dil = p.dil;
  const int ncb = cin / kMxBK;
  const int nk = TAPS * ncb;
  const int cs32 = cin >> 5;                        // scale bytes per pixel
  const int kp32 = p.k_pad >> 5;                    // ... per weight row
  const uint8_t* __restrict__ wv = reinterpret_cast<const uint8_t*>(p.wgt);
  const uint8_t* __restrict__ ws = wv + static_cast<int64_t>(p.cout_pad) * p.k_pad;
  const uint8_t* __restrict__ x = reinterpret_cast<const uint8_t*>(p.x);
  const uint8_t* __restrict__ xs = x + static_cast<int64_t>(p.n) * H * W * cin;

  // --- DMA assignment.  One 1-KB piece is 8 rows; lane l fills row l / 8, slot l % 8.  Wave w fills pieces
  // 4 w .. 4 w + 3 of the weight rows and of the pixel rows, and one 256-B piece of scale dwords
  int a_off[4], b_off[4];
  uint32_t b_hw[4];                                 // (ih0, iw0) of tap (0, 0) as two int16; ih0 = -16384: no pixel
  const char* zero16 = reinterpret_cast<const char*>(g_zero_page) + lane * 16;
  const char* zero4 = reinterpret_cast<const char*>(g_zero_page) + lane * 4;
  auto pixel = [&](int m, uint32_t& hw) -> int {    // input pixel index of tap (0, 0) (meaningful inside the image only)
    hw = 0xC000C000u;
    if (m >= M) return 0;
    const int n = m / hw_o;
    const int q = m - n * hw_o;
    const int oh = q / p.wo;
    const int ow = q - oh * p.wo;
    const int ih0 = oh - p.pad, iw0 = ow - p.pad;
    hw = (static_cast<uint32_t>(ih0) << 16) | (static_cast<uint32_t>(iw0) & 0xffffu);
    return (n * H + ih0) * W + iw0;
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wave * 4 + i) * 8 + (lane >> 3);
    const int slot = swzb<128>(r, lane & 7) * 16;
    a_off[i] = (co0 + r) * p.k_pad + slot;
    b_off[i] = pixel(px0 + r, b_hw[i]) * cin + slot;
  }
  uint32_t s_hw = 0xC000C000u;
  int s_off;
  if (wave < 2) s_off = (co0 + wave * 64 + lane) * kp32;
  else s_off = pixel(px0 + (wave - 2) * 64 + lane, s_hw) * cs32;

  auto inside = [&](uint32_t hw, int dh, int dw) {
    const int ih0 = static_cast<int>(hw) >> 16;
    const int iw0 = static_cast<int16_t>(hw & 0xffffu);
    return static_cast<unsigned>(ih0 + dh) < static_cast<unsigned>(H) && static_cast<unsigned>(iw0 + dw) < static_cast<unsigned>(W);
  };
  auto issue_step = [&](int kt, int stage) {
    const int cb = kt / TAPS;
    const int tap = kt - cb * TAPS;
    const int dh = (tap / KS) * dil, dw = (tap % KS) * dil;
    const int wcol = tap * cin + cb * kMxBK;        // packed weight column
    const int tpix = dh * W + dw;
    char* sa = smem + stage * kMxStage;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(wv + (a_off[i] + wcol), sa + (wave * 4 + i) * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const void* src = inside(b_hw[i], dh, dw) ? static_cast<const void*>(x + (b_off[i] + tpix * cin + cb * kMxBK))
                                                 : static_cast<const void*>(zero16);
      glds16(src, sa + kMxA + (wave * 4 + i) * 1024);
    }
    if (wave < 2) {
      glds4(ws + (s_off + (wcol >> 5)), sa + kMxA + kMxB + wave * 256);
    } else {
      const void* src = inside(s_hw, dh, dw) ? static_cast<const void*>(xs + (s_off + tpix * cs32 + cb * 4))
                                              : static_cast<const void*>(zero4);
      glds4(src, sa + kMxA + kMxB + kMxSA + (wave - 2) * 256);
    }
  };

  f32x4 acc[4][4];
  zero_tile(acc);
  issue_step(0, 0);
  for (int t = 0; t < nk; ++t) {
    // step t has landed and every wave is done with the other stage
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) issue_step(t + 1, (t + 1) & 1);

    const char* sa = smem + (t & 1) * kMxStage;
    const char* sb = sa + kMxA;
    const char* ssa = sb + kMxB;
    const char* ssb = ssa + kMxSA;
    i32x8 a[4], b[4];
    int sca[4], scb[4];
    auto frag = [&](const char* rows, int r) {     // chunks fq and 4 + fq of row r
      const i32x4 lo = *reinterpret_cast<const i32x4*>(rows + r * 128 + swzb<128>(r, fq) * 16);
      const i32x4 hi = *reinterpret_cast<const i32x4*>(rows + r * 128 + swzb<128>(r, 4 + fq) * 16);
      return KT<f8_t>::join(lo, hi);
    };
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int ra = wc * 64 + f * 16 + fr, rb = wp * 64 + f * 16 + fr;
      a[f] = frag(sa, ra);
      b[f] = frag(sb, rb);
      sca[f] = static_cast<int>(*reinterpret_cast<const uint32_t*>(ssa + ra * 4) >> (8 * fq));
      scb[f] = static_cast<int>(*reinterpret_cast<const uint32_t*>(ssb + rb * 4) >> (8 * fq));
    }
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int fn = 0; fn < 4; ++fn)
        acc[f][fn] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[f], b[fn], acc[f][fn], 0, 0, 0, sca[f], 0, scb[fn]);
  }

  mx_store_tile(p, acc, px0, co0, wc, wp, fr, fq);
}

template <int KS>
hipError_t launch_mx(const drnmi_conv_args& p, hipStream_t s) {
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = ((M + kMxBPX - 1) / kMxBPX) * ((p.cout + kMxBCO - 1) / kMxBCO);
  return launch_lds<&conv_mx_kernel<KS>>(dim3(static_cast<unsigned>(blocks)), dim3(256), kMxLds, s, p);
}

// e4m3fn byte of v: the clamp to +-448, round to nearest even (host; the weights are packed once)
uint8_t e4m3_host(float v) {
  const uint8_t sign = std::signbit(v) ? 0x80 : 0;
  float a = fabsf(v);
  if (a != a) return sign | 0x7f;
  if (a > kF8Max) a = kF8Max;
  if (a < 0.015625f) return sign | static_cast<uint8_t>(nearbyintf(a * 512.f));   // subnormals: steps of 2^-9
  int e;
  frexpf(a, &e);                                   // a = f 2^e, f in [0.5, 1): a in [2^(e-1), 2^e)
  e -= 1;
  const int q = static_cast<int>(nearbyintf(ldexpf(a, 3 - e)));                     // 8 .. 16 (16: carries into e + 1)
  return sign | static_cast<uint8_t>(((e + 7) << 3) + (q - 8));
}

bool mx_image_shape_ok(int64_t m, int64_t c) { return m > 0 && c > 0 && c % 32 == 0 && m * c < (int64_t(1) << 40); }

}  // namespace

const ConvKernel* mx_kernel(int ks) {
  static const ConvKernel k[2] = {DRNMI_KERNEL_ROW(conv_mx_kernel, launch_mx, 1), DRNMI_KERNEL_ROW(conv_mx_kernel, launch_mx, 3)};
  return &k[ks == 3];
}

// the block-scaled kernel's shapes: whole K steps of 128 channels (cin a power of two >= 128), stride 1, any
// dilation and M; a BN scale; no second input, unit mask or forced tile; fp32 / bf16 out at any strides, or an
// image (dense rows of whole blocks); a residual is an image too
bool mx_conv_supported(const drnmi_conv_args& p) {
  if (p.dtype != DRNMI_MXF8 || p.x2 != nullptr || p.unit_mask != nullptr || p.scale == nullptr || p.tile != DRNMI_TILE_AUTO)
    return false;
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  if (!big_body_shape_ok(p, kMxBK) || p.k != p.ks * p.ks * p.cin || p.stride != 1 ||
      static_cast<int64_t>(p.cout_pad) * p.k >= (int64_t(1) << 31) || M >= (int64_t(1) << 31) - kMxBPX ||
      p.h + 2 * p.pad >= 16384 || p.w + 2 * p.pad >= 16384)
    return false;
  if (p.res != nullptr && p.cout % 32 != 0) return false;
  if (p.out_dtype == DRNMI_MXF8)
    return p.cout % 32 == 0 && p.y_sc == 1 && p.y_sp == p.cout && p.y_sn == static_cast<int64_t>(p.ho) * p.wo * p.cout;
  return p.out_dtype == DRNMI_F32 || p.out_dtype == DRNMI_BF16;
}

}  // namespace drnmi

using namespace drnmi;

extern "C" int64_t drnmi_mx8_image_bytes(int64_t m, int32_t c) {
  return mx_image_shape_ok(m, c) ? (m * c / 32 * 33 + 15) / 16 * 16 : -1;
}

extern "C" int drnmi_quantize_mx8(const void* x, int32_t dtype, int64_t m, int32_t c, void* image, void* stream) {
  if (x == nullptr || image == nullptr || !mx_image_shape_ok(m, c) || (dtype != DRNMI_BF16 && dtype != DRNMI_F32) ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(image)) & 15) != 0)
    return DRNMI_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t nblk = m * c / 32;
  uint8_t* img = static_cast<uint8_t*>(image);
  if (dtype == DRNMI_BF16)
    hipLaunchKernelGGL(quantize_mx8_kernel<bf16_t>, dim3(grid_of(nblk)), dim3(256), 0, s, static_cast<const bf16_t*>(x), img, nblk);
  else
    hipLaunchKernelGGL(quantize_mx8_kernel<float>, dim3(grid_of(nblk)), dim3(256), 0, s, static_cast<const float*>(x), img, nblk);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_dequantize_mx8(const void* image, int64_t m, int32_t c, float* y_f32, void* stream) {
  if (image == nullptr || y_f32 == nullptr || !mx_image_shape_ok(m, c) ||
      ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(y_f32)) & 15) != 0)
    return DRNMI_EINVAL;
  const int64_t nblk = m * c / 32;
  hipLaunchKernelGGL(dequantize_mx8_kernel, dim3(grid_of(nblk)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(image), y_f32, nblk);
  return static_cast<int>(hipGetLastError());
}

extern "C" int64_t drnmi_mx8_pack_bytes(int32_t cout_pad, int32_t k_pad) {
  if (cout_pad <= 0 || k_pad <= 0 || cout_pad % 128 != 0 || k_pad % 128 != 0 ||
      static_cast<int64_t>(cout_pad) * k_pad >= (int64_t(1) << 31))
    return -1;
  return static_cast<int64_t>(cout_pad) * k_pad / 32 * 33;
}

extern "C" int drnmi_mx8_pack(const float* w_f32, int32_t cout_pad, int32_t k_pad, void* blob, int64_t nbytes) {
  const int64_t need = drnmi_mx8_pack_bytes(cout_pad, k_pad);
  if (w_f32 == nullptr || blob == nullptr || need < 0 || nbytes < need) return DRNMI_EINVAL;
  const int64_t nblk = static_cast<int64_t>(cout_pad) * k_pad / 32;
  uint8_t* vals = static_cast<uint8_t*>(blob);
  uint8_t* scales = vals + nblk * 32;
  for (int64_t i = 0; i < nblk; ++i) {
    const float* w = w_f32 + i * 32;
    uint32_t am = 0;
    for (int j = 0; j < 32; ++j) {
      uint32_t b;
      memcpy(&b, w + j, 4);
      b &= 0x7fffffffu;
      am = b > am ? b : am;
    }
    const uint32_t byte = mx_scale_byte(am), ib = mx_inv_scale_bits(byte);
    float inv;
    memcpy(&inv, &ib, 4);
    for (int j = 0; j < 32; ++j) vals[i * 32 + j] = e4m3_host(w[j] * inv);
    scales[i] = static_cast<uint8_t>(byte);
  }
  return DRNMI_OK;
}
