// Shared device helpers for the drnmi HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/drnmi.h"

namespace drnmi {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// bf16 stored as raw 16-bit words everywhere in global memory and LDS.
typedef uint16_t bf16_t;

__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
  return __uint_as_float(static_cast<uint32_t>(v) << 16);
}

// Round-to-nearest-even f32 -> bf16 (NaN kept NaN through the plain cast path).
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
  __bf16 b = static_cast<__bf16>(f);
  return __builtin_bit_cast(bf16_t, b);
}

// Exact three-way split of 8 fp32 values into bf16 fragments, x = x1 + x2 + x3 (round to
// nearest even at each step; x - x1 and (x - x1) - x2 are exact in fp32 by Sterbenz): the
// fp32x arithmetic (include/drnmi.h DRNMI_F32X3).  Works on value pairs: one
// v_cvt_pk_bf16_f32 is a fragment dword, and its halves widen back to fp32 by a shift (low)
// and a mask (high), so no per-element register packing is needed.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_bf16x2(f32x2_t v) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ f32x2_t widen_bf16x2(uint32_t h) {
  return f32x2_t{__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};
}
__device__ __forceinline__ void split3(const float4& lo4, const float4& hi4, bf16x8& b1, bf16x8& b2, bf16x8& b3) {
  const f32x2_t x[4] = {f32x2_t{lo4.x, lo4.y}, f32x2_t{lo4.z, lo4.w}, f32x2_t{hi4.x, hi4.y}, f32x2_t{hi4.z, hi4.w}};
  uint32_t u1[4], u2[4], u3[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u1[i] = pk_bf16x2(x[i]);
    const f32x2_t r1 = x[i] - widen_bf16x2(u1[i]);
    u2[i] = pk_bf16x2(r1);
    u3[i] = pk_bf16x2(r1 - widen_bf16x2(u2[i]));
  }
  b1 = __builtin_bit_cast(bf16x8, make_uint4(u1[0], u1[1], u1[2], u1[3]));
  b2 = __builtin_bit_cast(bf16x8, make_uint4(u2[0], u2[1], u2[2], u2[3]));
  b3 = __builtin_bit_cast(bf16x8, make_uint4(u3[0], u3[1], u3[2], u3[3]));
}

// c += a * b on the split3 planes of both operands (a1 + a2 + a3, b1 + b2 + b3, largest first): the
// six products above 2^-24 of the leading one, smallest first.  Every fp32x kernel accumulates in
// this order, which is what makes their sums comparable bit for bit.
__device__ __forceinline__ void mfma_x6(f32x4& c, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
}

// 16-B chunk `chunk` of 64-B LDS row `row` (32 bf16): conflict-free for every ds_read_b128 lane
// group (conv_big.hip swzb<64>)
__device__ __forceinline__ int swz64(int row, int chunk) { return chunk ^ (((row >> 3) & 1) * 3); }

// one ds_read_b128 at LDS byte address base + OFF.  Inline asm: the caller counts lgkmcnt itself
template <int OFF, typename V>
__device__ __forceinline__ void ds_rd(V& dst, uint32_t base) {
  static_assert(sizeof(V) == 16 && OFF >= 0 && OFF < 65536, "ds_read_b128 offset");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(base), "i"(OFF));
}

// OCP e4m3fn bytes (include/drnmi.h DRNMI_F8).  f8_t tags the element type of the fp8 kernels.
struct f8_t { uint8_t v; };
constexpr float kF8Max = 448.f;
__device__ __forceinline__ float f8_clamp(float v) { return fminf(fmaxf(v, -kF8Max), kF8Max); }
// four values -> four e4m3 bytes (byte j = value j): the clamp, then two v_cvt_pk_fp8_f32 (RNE)
__device__ __forceinline__ uint32_t pk_f8x4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(a), f8_clamp(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(c), f8_clamp(d), w, true);
  return static_cast<uint32_t>(w);
}
template <int J>
__device__ __forceinline__ float f8_to_f32(uint32_t w) { return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w), J); }

template <typename T> struct Elem;
template <> struct Elem<float> {
  static constexpr int kDtype = DRNMI_F32;
  __device__ __forceinline__ static float to_f32(float v) { return v; }
};
template <> struct Elem<bf16_t> {
  static constexpr int kDtype = DRNMI_BF16;
  __device__ __forceinline__ static float to_f32(bf16_t v) { return bf16_to_f32(v); }
};

// 8 contiguous elements: 16 B of bf16 or 32 B of fp32.
template <typename T> struct Vec8;
template <> struct Vec8<bf16_t> {
  uint4 v;
  __device__ __forceinline__ static Vec8 zero() { Vec8 r; r.v = make_uint4(0, 0, 0, 0); return r; }
  __device__ __forceinline__ static Vec8 load(const bf16_t* p) {
    Vec8 r; r.v = *reinterpret_cast<const uint4*>(p); return r;
  }
  __device__ __forceinline__ void store(bf16_t* p) const { *reinterpret_cast<uint4*>(p) = v; }
};
template <> struct Vec8<float> {
  float4 a, b;
  __device__ __forceinline__ static Vec8 zero() {
    Vec8 r; r.a = make_float4(0.f, 0.f, 0.f, 0.f); r.b = r.a; return r;
  }
  __device__ __forceinline__ static Vec8 load(const float* p) {
    Vec8 r;
    r.a = reinterpret_cast<const float4*>(p)[0];
    r.b = reinterpret_cast<const float4*>(p)[1];
    return r;
  }
  __device__ __forceinline__ void store(float* p) const {
    reinterpret_cast<float4*>(p)[0] = a;
    reinterpret_cast<float4*>(p)[1] = b;
  }
};

// 16-B row pieces of the MFMA accumulator layout (lane (fr, fq) holds channels 16 fm + 4 fq .. + 3
// of pixel fr): row fq of the 16-lane groups moves chunk s(fq) = (0, 2, 1, 3)[fq] of a 32-channel
// group, and one v_permlane16_swap per dword pair converts (lo: x y, hi: z w) <-> (fragment 2 f2,
// fragment 2 f2 + 1) both ways (conv_tile.h load_residual / store_tile_x4)
__device__ __forceinline__ int chunk_of_row(int fq) { return (fq & 1) * 2 + (fq >> 1); }
__device__ __forceinline__ void swap_halves(uint4& v) {
  const auto a = __builtin_amdgcn_permlane16_swap(v.x, v.z, false, false);
  const auto b = __builtin_amdgcn_permlane16_swap(v.y, v.w, false, false);
  v = make_uint4(a[0], b[0], a[1], b[1]);
}

// int8 rows: lane (fr, fq) holds byte quad fq (channels 4 fq .. + 3) of fragments 4 g + k in r[k];
// this 4 x 4 transpose over (register, 16-lane row) leaves fragment 4 g + fq whole in row fq's four
// registers (16 contiguous bytes), and back (it is its own inverse)
__device__ __forceinline__ void transpose_rows4(uint32_t (&r)[4]) {
  const auto a = __builtin_amdgcn_permlane32_swap(r[0], r[2], false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(r[1], r[3], false, false);
  const auto c = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
  const auto d = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
  r[0] = c[0];
  r[1] = c[1];
  r[2] = d[0];
  r[3] = d[1];
}

// More than 64 KB of dynamic LDS is an opt-in per kernel (hipFuncAttributeMaxDynamicSharedMemorySize).
// allow_lds makes it once per kernel, at the first size asked for; a kernel whose size varies asks for its
// largest first (the wide confusion matrix) or is raised when a later launch needs more (conv_halo's patch
// grows with the dilation).  One flag per kernel, whatever the argument types of the launch.
template <auto KERNEL>
hipError_t allow_lds(int lds) {
  static int attr_lds = 0;
  if (attr_lds < lds) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    attr_lds = lds;
  }
  return hipSuccess;
}
// allow_lds, then the launch with `lds` bytes of dynamic LDS: the first error of the two
template <auto KERNEL, typename... Args>
hipError_t launch_lds(dim3 grid, dim3 block, int lds, hipStream_t s, const Args&... args) {
  const hipError_t e = allow_lds<KERNEL>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(KERNEL, grid, block, lds, s, args...);
  return hipGetLastError();
}

inline int ceil_div(int64_t a, int64_t b) { return static_cast<int>((a + b - 1) / b); }

// workgroups of `per` threads for the n elements of a grid-stride kernel (at least 1, at most 2^20 - 16)
inline unsigned grid_of(int64_t n, int per = 256) {
  const int64_t g = (n + per - 1) / per;
  return static_cast<unsigned>(g < 1 ? 1 : (g > 65535 * 16 ? 65535 * 16 : g));
}

}  // namespace drnmi
