// int8 activation helpers for the W8A8 path (BASELINE config C5).
//
// The reference has no quantisation code: the scheme is ours.
//   * weights: per-output-channel symmetric int8, q = rint(w * 127 / absmax_row) (host packing,
//     drnmi/engine.py), the dequant scale folded into the conv epilogue's per-channel scale;
//   * activations: per-tensor symmetric int8 with a calibrated scale s (absmax / 127 over a
//     calibration batch): q = clamp(rint(x * (1/s)), -127, 127).  The conv that produces an int8
//     activation quantises in its epilogue; this file serves the bf16 -> int8 boundary (the first
//     int8 layer's input), the calibration absmax and the calibration |x| histogram (from which
//     drnmi/calibrate.py derives absmax, percentile or MSE-optimal scales over many batches).
// All three kernels are HBM-bound streams: 16-B loads per lane, grid-stride (no reuse to place).
#include "common.h"
#include "kernels.h"

namespace drnmi {
namespace {

__device__ __forceinline__ int8_t q8(float v, float inv) {
  float r = rintf(__fmul_rn(v, inv));
  r = fminf(fmaxf(r, -127.f), 127.f);
  return static_cast<int8_t>(static_cast<int>(r));
}

// 8 elements per lane per iteration (one 16-B bf16 load -> one 8-B int8 store)
template <typename T>
__global__ void __launch_bounds__(256) quantize_kernel(const T* __restrict__ x, int8_t* __restrict__ y, int64_t n8,
                                                       float inv) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const Vec8<T> v = Vec8<T>::load(x + i * 8);
    const T* e = reinterpret_cast<const T*>(&v);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) lo |= static_cast<uint32_t>(static_cast<uint8_t>(q8(Elem<T>::to_f32(e[j]), inv))) << (8 * j);
#pragma unroll
    for (int j = 0; j < 4; ++j) hi |= static_cast<uint32_t>(static_cast<uint8_t>(q8(Elem<T>::to_f32(e[4 + j]), inv))) << (8 * j);
    *reinterpret_cast<uint2*>(y + i * 8) = make_uint2(lo, hi);
  }
}

// fp8 (include/drnmi.h DRNMI_F8): 16 elements per lane per iteration (16-B loads, one 16-B store),
// x * inv in fp32, the clamp to +-448, packed v_cvt_pk_fp8_f32 (RNE); the last n % 16 elements one
// lane each
template <typename T>
__device__ __forceinline__ uint2 q8_f8(const Vec8<T>& v, float inv) {
  const T* e = reinterpret_cast<const T*>(&v);
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = __fmul_rn(Elem<T>::to_f32(e[j]), inv);
  return make_uint2(pk_f8x4(f[0], f[1], f[2], f[3]), pk_f8x4(f[4], f[5], f[6], f[7]));
}
template <typename T>
__global__ void __launch_bounds__(256) quantize_f8_kernel(const T* __restrict__ x, uint8_t* __restrict__ y, int64_t n,
                                                          float inv) {
  const int64_t n16 = n / 16;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < n16; i += stride) {
    const uint2 a = q8_f8<T>(Vec8<T>::load(x + i * 16), inv), b = q8_f8<T>(Vec8<T>::load(x + i * 16 + 8), inv);
    *reinterpret_cast<uint4*>(y + i * 16) = make_uint4(a.x, a.y, b.x, b.y);
  }
  const int64_t i = n16 * 16 + t0;
  if (i < n) y[i] = static_cast<uint8_t>(pk_f8x4(__fmul_rn(Elem<T>::to_f32(x[i]), inv), 0.f, 0.f, 0.f) & 0xff);
}

// max |x| over n8 * 8 elements into *out (as uint bits: |x| >= 0 orders like its bit pattern;
// NaN (bits above +inf) propagates as the maximum)
template <typename T>
__global__ void __launch_bounds__(256) absmax_kernel(const T* __restrict__ x, int64_t n8, uint32_t* __restrict__ out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  uint32_t m = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const Vec8<T> v = Vec8<T>::load(x + i * 8);
    const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t b = __float_as_uint(Elem<T>::to_f32(e[j])) & 0x7fffffffu;
      m = b > m ? b : m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), o));
    m = t > m ? t : m;
  }
  __shared__ uint32_t red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t r = red[0];
    for (int w = 1; w < 4; ++w) r = red[w] > r ? red[w] : r;
    atomicMax(out, r);
  }
}

unsigned stream_blocks(int64_t n8) {
  const int64_t b = (n8 + 255) / 256;
  return static_cast<unsigned>(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

// Exact |x| histogram: element x adds 1 to bin (bits(float(x)) & 0x7fffffff) >> 16, one bin per
// bf16 magnitude.  The same HBM-bound stream as absmax_kernel, counted in a workgroup-private LDS
// table of DRNMI_HIST_BINS uint32 (128 KiB: one workgroup per CU, hence 1024 lanes in it, each
// with four 16-B loads in flight) and flushed with one 64-bit global atomic per nonzero bin.
//   * the grid is one workgroup per CU at most: the zeroing and the flush of the table are paid
//     once per CU, and a workgroup's share of the elements, with it every LDS counter, stays
//     below 2^32 for n < 2^39;
//   * zeros (more than half of a post-ReLU tensor) never reach the LDS atomics: each lane counts
//     them in a register, a wave adds its sum to bin 0 once;
//   * a lane merges a run of equal bins among its 8 elements into one LDS add (a constant tensor
//     costs one same-address add per lane and load instead of eight).
constexpr int kHistThreads = 1024;
constexpr int kHistUnroll = 4;
constexpr size_t kHistLds = static_cast<size_t>(DRNMI_HIST_BINS) * sizeof(uint32_t);
int g_hist_wgs = 0;                      // workgroups of a full grid (the device's CU count)

template <typename T> __device__ __forceinline__ uint32_t abs_bin(T v);
template <> __device__ __forceinline__ uint32_t abs_bin<bf16_t>(bf16_t v) { return v & 0x7fffu; }
template <> __device__ __forceinline__ uint32_t abs_bin<float>(float v) { return (__float_as_uint(v) & 0x7fffffffu) >> 16; }

template <typename T>
__device__ __forceinline__ void count8(const Vec8<T>& v, uint32_t* bins, uint32_t& zeros) {
  const T* e = reinterpret_cast<const T*>(&v);
  uint32_t cur = 0, run = 0;             // pending run of one nonzero bin (cur == 0: none)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t b = abs_bin<T>(e[j]);
    if (b == 0) {
      ++zeros;
    } else if (b == cur) {
      ++run;
    } else {
      if (cur != 0) atomicAdd(&bins[cur], run);
      cur = b;
      run = 1;
    }
  }
  if (cur != 0) atomicAdd(&bins[cur], run);
}

template <typename T>
__global__ void __launch_bounds__(kHistThreads) abs_histogram_kernel(const T* __restrict__ x, int64_t n8,
                                                                     unsigned long long* __restrict__ hist) {
  extern __shared__ uint32_t bins[];
  for (int b = threadIdx.x * 4; b < DRNMI_HIST_BINS; b += kHistThreads * 4)
    *reinterpret_cast<uint4*>(bins + b) = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint32_t zeros = 0;
  for (; i + (kHistUnroll - 1) * stride < n8; i += kHistUnroll * stride) {
    Vec8<T> v[kHistUnroll];
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) v[u] = Vec8<T>::load(x + (i + u * stride) * 8);
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) count8<T>(v[u], bins, zeros);
  }
  for (; i < n8; i += stride) count8<T>(Vec8<T>::load(x + i * 8), bins, zeros);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) zeros += static_cast<uint32_t>(__shfl_xor(static_cast<int>(zeros), o));
  if ((threadIdx.x & 63) == 0 && zeros != 0) atomicAdd(&bins[0], zeros);
  __syncthreads();
  for (int b = threadIdx.x; b < DRNMI_HIST_BINS; b += kHistThreads) {
    const uint32_t c = bins[b];
    if (c != 0) atomicAdd(&hist[b], static_cast<unsigned long long>(c));
  }
}

template <typename T>
hipError_t launch_abs_histogram(const T* x, int64_t n8, int64_t* hist, hipStream_t s) {
  if (g_hist_wgs == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    g_hist_wgs = cus;
  }
  const int64_t b = (n8 + kHistThreads - 1) / kHistThreads;
  return launch_lds<&abs_histogram_kernel<T>>(dim3(static_cast<unsigned>(b < g_hist_wgs ? b : g_hist_wgs)), dim3(kHistThreads),
                                              static_cast<int>(kHistLds), s, x, n8, reinterpret_cast<unsigned long long*>(hist));
}

}  // namespace
}  // namespace drnmi

using namespace drnmi;

extern "C" int drnmi_quantize_i8(const void* x, int32_t dtype, int8_t* y, int64_t n, float inv_scale, void* stream) {
  if (x == nullptr || y == nullptr || n < 0 || n % 8 != 0 || !(inv_scale > 0.f)) return DRNMI_EINVAL;
  if (n == 0) return DRNMI_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n8 = n / 8;
  if (dtype == DRNMI_BF16)
    hipLaunchKernelGGL(quantize_kernel<bf16_t>, dim3(stream_blocks(n8)), dim3(256), 0, s,
                       static_cast<const bf16_t*>(x), y, n8, inv_scale);
  else if (dtype == DRNMI_F32)
    hipLaunchKernelGGL(quantize_kernel<float>, dim3(stream_blocks(n8)), dim3(256), 0, s,
                       static_cast<const float*>(x), y, n8, inv_scale);
  else
    return DRNMI_EINVAL;
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_quantize_f8(const void* x, int32_t dtype, int64_t n, float inv_scale, uint8_t* y, void* stream) {
  if (x == nullptr || y == nullptr || n <= 0 || !(inv_scale > 0.f) || (dtype != DRNMI_BF16 && dtype != DRNMI_F32))
    return DRNMI_EINVAL;
  // the vector body needs 16-B aligned rows on both sides; torch allocations are
  if ((reinterpret_cast<uintptr_t>(x) & 15) != 0 || (reinterpret_cast<uintptr_t>(y) & 15) != 0) return DRNMI_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned blocks = stream_blocks((n + 15) / 16 * 2);
  if (dtype == DRNMI_BF16)
    hipLaunchKernelGGL(quantize_f8_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, static_cast<const bf16_t*>(x), y, n,
                       inv_scale);
  else
    hipLaunchKernelGGL(quantize_f8_kernel<float>, dim3(blocks), dim3(256), 0, s, static_cast<const float*>(x), y, n,
                       inv_scale);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_abs_histogram(const void* x, int32_t dtype, int64_t n, int64_t* hist, void* stream) {
  if (x == nullptr || hist == nullptr || n < 0 || n % 8 != 0 || (dtype != DRNMI_BF16 && dtype != DRNMI_F32))
    return DRNMI_EINVAL;
  if (n == 0) return DRNMI_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == DRNMI_BF16) return static_cast<int>(launch_abs_histogram(static_cast<const bf16_t*>(x), n / 8, hist, s));
  return static_cast<int>(launch_abs_histogram(static_cast<const float*>(x), n / 8, hist, s));
}

extern "C" int drnmi_absmax(const void* x, int32_t dtype, int64_t n, float* out, void* stream) {
  if (x == nullptr || out == nullptr || n < 0 || n % 8 != 0) return DRNMI_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(out, 0, sizeof(float), s);
  if (e != hipSuccess) return static_cast<int>(e);
  if (n == 0) return DRNMI_OK;
  const int64_t n8 = n / 8;
  uint32_t* o = reinterpret_cast<uint32_t*>(out);
  if (dtype == DRNMI_BF16)
    hipLaunchKernelGGL(absmax_kernel<bf16_t>, dim3(stream_blocks(n8)), dim3(256), 0, s,
                       static_cast<const bf16_t*>(x), n8, o);
  else if (dtype == DRNMI_F32)
    hipLaunchKernelGGL(absmax_kernel<float>, dim3(stream_blocks(n8)), dim3(256), 0, s,
                       static_cast<const float*>(x), n8, o);
  else
    return DRNMI_EINVAL;
  return static_cast<int>(hipGetLastError());
}
