// What conv_x6.hip (DRNMI_F32X3: three bf16 planes, six products) and conv_x3.hip (DRNMI_F32X2: two planes,
// three products) share, written once: the device helpers, the zero page, the tile geometry both Cfgs start
// from, the launch and the variant-table macros.  The two files stay two translation units (conv_x3.hip is
// built with one fp32 operation per instruction, drnmi/build.py).  Each keeps its K loop and, written out, the
// prologue and the epilogue around it: shared as one struct and function template, and then piece by piece as
// __forceinline__ helpers, they changed every kernel's text, and conv_x3's `acc * scale + shift` is one fused multiply-add where conv_x6's is a packed
// multiply and a packed add, so the two epilogues are not the same arithmetic (profiles/xsplit_fold).
#pragma once
#include "common.h"
#include "kernels.h"

namespace drnmi {
namespace {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void g_void_t;

__device__ uint4 g_xsplit_zero[64];   // zero-initialised: the source of padded taps / rows (one per translation unit)

constexpr int kBK = 32;     // input channels per K step
static_assert(kBK == kX6BK, "the K step conv_route.cpp plans with");

__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((g_void_t*)src, (lds_void_t*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = bid % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

// swz64 (bf16 A rows, 64 B) is common.h's
__device__ __forceinline__ int swz128(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }   // fp32 B rows

// x from the lane DPP control CTRL selects, as two 32-bit DPP moves
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const int lo = __builtin_amdgcn_mov_dpp(static_cast<int>(u & 0xffffffffu), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(static_cast<int>(u >> 32), CTRL, 0xF, 0xF, false);
  return __builtin_bit_cast(double, (static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo));
}
// sum over the 16 lanes of a DPP row, the same in every lane: quad_perm xor 1, xor 2, then
// row_half_mirror (quads 0 <-> 1) and row_mirror (halves) -- a fixed order, ALU only (the
// ds_bpermute form of __shfl_xor cost the short-K launches ~10 % in their epilogue)
__device__ __forceinline__ double row16_sum(double x) {
  x += dpp_f64<0xB1>(x);    // quad_perm [1, 0, 3, 2]
  x += dpp_f64<0x4E>(x);    // quad_perm [2, 3, 0, 1]
  x += dpp_f64<0x141>(x);   // row_half_mirror
  x += dpp_f64<0x140>(x);   // row_mirror
  return x;
}

// Tile = BCO = WCO x WC output channels x BPX = 64 x PS pixels; one wave per (channel column, 64-pixel
// slice); one K step's operands are PLANES bf16 weight planes and BPX fp32 pixel rows, moved as 1-KB DMA
// pieces.  Each file's Cfg adds its ring: OCC, STAGE, NST, LDS.
template <int PLANES, int WCO, int WC, int PS>
struct XCfg {
  static constexpr int BCO = WCO * WC;
  static constexpr int BPX = 64 * PS;
  static constexpr int FM = WCO / 16;
  static constexpr int FN = 4;
  static constexpr int NW = PS * WC;
  static constexpr int THREADS = 64 * NW;
  static constexpr int A_PLANE = BCO * 64;          // one bf16 plane: BCO rows x 32 K x 2 B
  static constexpr int A_BYTES = PLANES * A_PLANE;
  static constexpr int B_BYTES = BPX * 128;         // BPX pixel rows x 32 ch x 4 B
  static constexpr int A_PW = A_BYTES / 1024 / NW;  // 1-KB DMA pieces per wave per K step
  static constexpr int B_PW = B_BYTES / 1024 / NW;
  static constexpr int GLDS = A_PW + B_PW;
  static_assert(A_PW * NW * 1024 == A_BYTES && B_PW * NW * 1024 == B_BYTES, "DMA split");
};

// one launch of KERNEL on C's tiles, then the split-K finish when the plan splits
template <auto KERNEL, class C>
hipError_t launch_x(const drnmi_conv_args& p, int splits, hipStream_t s) {
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = ((M + C::BPX - 1) / C::BPX) * ((p.cout + C::BCO - 1) / C::BCO);
  const hipError_t e = launch_lds<KERNEL>(dim3(static_cast<unsigned>(blocks), splits), dim3(C::THREADS), C::LDS, s, p);
  if (e != hipSuccess || splits == 1) return e;
  return x6_splitk_finish(p, splits, s);
}

// a variant's table entry: KERNEL is the kernel template's name, CFG its Cfg template; the arguments after
// STEP are the template arguments behind KS, in the order both templates take them
#define X_ROW(KERNEL, CFG, KS, ...) \
  ConvKernel { #KERNEL "<" #KS ", " #__VA_ARGS__ ">", &launch_x<&KERNEL<KS, __VA_ARGS__>, CFG<__VA_ARGS__>> }
#define X_VARIANT(KERNEL, CFG, STEP, ...)                                        \
  {CFG<__VA_ARGS__>::BCO, CFG<__VA_ARGS__>::BPX, CFG<__VA_ARGS__>::OCC, STEP,     \
   {X_ROW(KERNEL, CFG, 1, __VA_ARGS__), X_ROW(KERNEL, CFG, 2, __VA_ARGS__), X_ROW(KERNEL, CFG, 3, __VA_ARGS__)}}

}  // namespace
}  // namespace drnmi
