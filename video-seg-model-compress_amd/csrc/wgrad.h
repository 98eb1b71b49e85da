// Shared between wgrad.hip and wgrad_x3.hip: the launch parameters and the pre pipeline's device helpers
// (moved here unchanged; wgrad.hip's kernels keep their code).
#pragma once
#include "common.h"

namespace drnmi {
namespace {

constexpr int kThreads = 256;

struct WgradP {
  const float* dy;
  const float* x;
  float* ws;
  int dys, cout;
  int n, h, w, cs, ho, wo, ks, stride, pad, dil;
  int K;                 // ks * ks * cs
  int64_t M;
  int64_t pix_per_split;
};

constexpr int kWM = 32;      // pixels per chunk
constexpr int kWLD = kWM + 4;
constexpr int kWT = 64;      // tile rows / cols
constexpr int kWTBig = 128;  // the large tile's; the dy planes' rows are padded to a multiple of it

// A thread's pixel m = (n, oh, ow) advances by one chunk: the coordinates are stepped, not divided
// out of m every chunk (an int64 division per chunk and thread).  On the caller's own variables: as
// a struct copied per load the 128-tile and the pre kernel grew by a dozen instructions.
__device__ __forceinline__ void wgrad_pix_step(const WgradP& p, int64_t& m, int& n, int& oh, int& ow) {
  m += kWM;
  ow += kWM;
  while (ow >= p.wo) {
    ow -= p.wo;
    if (++oh == p.ho) {
      oh = 0;
      ++n;
    }
  }
}

// LDS byte address of a __shared__ object
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) void*)p));
}
// one 16-B-per-lane LDS-DMA (global_load_lds_dwordx4) to the wave-uniform LDS address `lds`
// (M0 holds the LDS address; its previous value is restored, as M0 is reserved to the compiler)
__device__ __forceinline__ void dma16(const void* src, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds) : "memory");
}
// XOR term of the 16-B chunk of a 128-B fp32 B row (the 64-B bf16 A rows take common.h swz64)
__device__ __forceinline__ int pre_swz_b(int row) { return ((row >> 1) & 1) | (row & 4); }
// transposed B write of row RR (0..15) of a thread's 16-row group: w[k] holds the lane address for
// swizzle value k -> (0, 1, 4, 5)
template <int RR>
__device__ __forceinline__ void pre_wr(const uint32_t (&w)[4], float v) {
  constexpr int k = ((RR >> 1) & 1) | (((RR >> 2) & 1) << 1);
  asm volatile("ds_write_b32 %0, %1 offset:%2" :: "v"(w[k]), "v"(v), "i"(RR * 128) : "memory");
}

struct WgradPreP {
  WgradP p;
  const bf16_t* dyt;   // [planes][Cp][Mp]: 3 (drnmi_conv_wgrad_f32x3) or 2 (drnmi_conv_wgrad_f32x2)
  int64_t Mp;
  int Cp;
};

}  // namespace

// wgrad_x3.hip: drnmi_conv_wgrad_f32x2's pre route (dy split into two planes at dyt, then the tile kernel);
// pre_params: the caller's WgradPreP (a type of each translation unit's own, so passed untyped)
void launch_wgrad_x3_pre(const void* pre_params, const float* dy, dim3 split_grid, dim3 grid, hipStream_t s);

}  // namespace drnmi
