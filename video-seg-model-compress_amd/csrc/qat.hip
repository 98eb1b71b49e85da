// Quantisation-aware fine-tuning: the int8 engine's grids in the fp32 train step.
//
// The train forward of a QAT model reads, wherever the int8 engine would launch W8A8, the values that
// launch would see: activations on their calibrated per-tensor grid and weights on their per-row grid,
// both kept as fp32 ("fake quantisation").  The backward is straight-through.  The reference has no
// quantisation code; what these kernels restate is this project's own scheme:
//   * fake_quant_kernel       restates drnmi_quantize_i8 (quant.hip q8) followed by the dequantising
//                             multiply by the scale: fq(x) = fl(float(q8(x, inv)) * s);
//   * fake_quant_bwd_kernel   is the straight-through estimator of that: the gradient passes where the
//                             level was not clamped (|rint(fl(x * inv))| <= 127), recomputed from x;
//   * fake_quant_rows_kernel  restates engine._pack_q8 / oracle.int8_oracle.quantize_weight_rows on a
//                             row of OIHW weights (one output channel): the same int8 codes, times the
//                             row's scale a / 127.
// One fp32 rounding per step and no multiply feeds an add, so no FMA can form.  The level goes through an
// integer (as the int8 code does), which makes a zero level +0 whatever the sign of x.
// The two activation kernels are HBM-bound streams (two 16-B loads and stores per lane and iteration,
// grid-stride); the row kernel is one workgroup per row, an LDS absmax reduction and a second, cached
// read of the row.
#include "common.h"
#include "kernels.h"

namespace drnmi {
namespace {

constexpr int kQatThreads = 256;
constexpr unsigned kQatMaxBlocks = 2048;     // 8 workgroups per CU; larger tensors grid-stride
constexpr int kFqRowsMaxEntries = 512;

// the int8 level of x as fp32 before the clamp, and clamped (quant.hip q8's arithmetic)
__device__ __forceinline__ float level(float x, float inv) { return rintf(__fmul_rn(x, inv)); }
__device__ __forceinline__ float fq1(float x, float inv, float s) {
  const float r = fminf(fmaxf(level(x, inv), -127.f), 127.f);
  return __fmul_rn(static_cast<float>(static_cast<int>(r)), s);
}
__device__ __forceinline__ bool passes(float x, float inv) { return fabsf(level(x, inv)) <= 127.f; }

__global__ void __launch_bounds__(kQatThreads) fake_quant_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 int64_t n8, float s, float inv) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const Vec8<float> v = Vec8<float>::load(x + i * 8);
    Vec8<float> o;
    o.a = make_float4(fq1(v.a.x, inv, s), fq1(v.a.y, inv, s), fq1(v.a.z, inv, s), fq1(v.a.w, inv, s));
    o.b = make_float4(fq1(v.b.x, inv, s), fq1(v.b.y, inv, s), fq1(v.b.z, inv, s), fq1(v.b.w, inv, s));
    o.store(y + i * 8);
  }
}

template <bool ACC>
__device__ __forceinline__ float ste1(float dq, float x, float inv, float dx) {
  const float g = passes(x, inv) ? dq : 0.f;
  return ACC ? __fadd_rn(dx, g) : g;
}
template <bool ACC>
__device__ __forceinline__ float4 ste4(const float4& dq, const float4& x, float inv, const float4& dx) {
  return make_float4(ste1<ACC>(dq.x, x.x, inv, dx.x), ste1<ACC>(dq.y, x.y, inv, dx.y), ste1<ACC>(dq.z, x.z, inv, dx.z),
                     ste1<ACC>(dq.w, x.w, inv, dx.w));
}
template <bool ACC>
__global__ void __launch_bounds__(kQatThreads) fake_quant_bwd_kernel(const float* __restrict__ dq,
                                                                     const float* __restrict__ x, float* dx, int64_t n8,
                                                                     float inv) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const Vec8<float> g = Vec8<float>::load(dq + i * 8), v = Vec8<float>::load(x + i * 8);
    const Vec8<float> d = ACC ? Vec8<float>::load(dx + i * 8) : Vec8<float>::zero();
    Vec8<float> o;
    o.a = ste4<ACC>(g.a, v.a, inv, d.a);
    o.b = ste4<ACC>(g.b, v.b, inv, d.b);
    o.store(dx + i * 8);
  }
}

unsigned stream_blocks(int64_t n8) {
  const int64_t b = (n8 + kQatThreads - 1) / kQatThreads;
  return static_cast<unsigned>(b < kQatMaxBlocks ? (b > 0 ? b : 1) : kQatMaxBlocks);
}

// One row of `cols` floats by one workgroup: a = max |w| (as bit patterns, which order like the
// magnitudes), then w_q = float(clamp(rint(w * (127 / a)))) * (a / 127); an all-zero row: zeros, scale 1.
// 16-B accesses when the row starts 16-B aligned (cols % 4 == 0), else one float per lane.
__device__ __forceinline__ void fake_quant_row(const float* __restrict__ w, float* __restrict__ wq,
                                               float* __restrict__ scale_out, int cols, uint32_t* red) {
  const int t = threadIdx.x;
  const bool vec = (cols & 3) == 0;
  uint32_t m = 0;
  if (vec) {
    for (int c = t * 4; c < cols; c += kQatThreads * 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(w + c);
      const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t b = e[j] & 0x7fffffffu;
        m = b > m ? b : m;
      }
    }
  } else {
    for (int c = t; c < cols; c += kQatThreads) {
      const uint32_t b = __float_as_uint(w[c]) & 0x7fffffffu;
      m = b > m ? b : m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t u = static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), o));
    m = u > m ? u : m;
  }
  if ((t & 63) == 0) red[t >> 6] = m;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kQatThreads / 64; ++k) m = red[k] > m ? red[k] : m;
  const float a = __uint_as_float(m);
  const bool pos = a > 0.f;
  const float inv = pos ? __fdiv_rn(127.f, a) : 1.f;
  const float s = pos ? __fdiv_rn(a, 127.f) : 1.f;
  if (t == 0) *scale_out = s;
  if (vec) {
    for (int c = t * 4; c < cols; c += kQatThreads * 4) {
      const float4 v = *reinterpret_cast<const float4*>(w + c);
      *reinterpret_cast<float4*>(wq + c) = make_float4(fq1(v.x, inv, s), fq1(v.y, inv, s), fq1(v.z, inv, s), fq1(v.w, inv, s));
    }
  } else {
    for (int c = t; c < cols; c += kQatThreads) wq[c] = fq1(w[c], inv, s);
  }
}

__global__ void __launch_bounds__(kQatThreads) fake_quant_rows_kernel(const float* __restrict__ w, float* __restrict__ wq,
                                                                      float* __restrict__ scale, int64_t rows, int cols) {
  __shared__ uint32_t red[kQatThreads / 64];
  const int64_t r = blockIdx.x;
  if (r >= rows) return;
  fake_quant_row(w + r * cols, wq + r * cols, scale + r, cols, red);
}

// every row of every table entry, one workgroup each: row blockIdx.x belongs to the last entry whose
// first row (word 5, a prefix sum checked on the host) is not above it
__global__ void __launch_bounds__(kQatThreads) fake_quant_rows_batched_kernel(const int64_t* __restrict__ tab, int n,
                                                                              int64_t total) {
  __shared__ uint32_t red[kQatThreads / 64];
  const int64_t r = blockIdx.x;
  if (r >= total) return;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[static_cast<int64_t>(mid) * DRNMI_FQ_ROWS_ENTRY_WORDS + 5] <= r) lo = mid;
    else hi = mid - 1;
  }
  const int64_t* q = tab + static_cast<int64_t>(lo) * DRNMI_FQ_ROWS_ENTRY_WORDS;
  const int64_t local = r - q[5];
  if (local < 0 || local >= q[3]) return;
  const int cols = static_cast<int>(q[4]);
  fake_quant_row(reinterpret_cast<const float*>(q[0]) + local * cols, reinterpret_cast<float*>(q[1]) + local * cols,
                 reinterpret_cast<float*>(q[2]) + local, cols, red);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool positive(float v) { return v > 0.f && v < __builtin_inff(); }

}  // namespace
}  // namespace drnmi

using namespace drnmi;

extern "C" int drnmi_fake_quant_f32(const float* x, int64_t n, float scale, float inv_scale, float* y, void* stream) {
  if (x == nullptr || y == nullptr || !aligned16(x) || !aligned16(y) || n < 0 || n % 8 != 0 || !positive(scale) ||
      !positive(inv_scale))
    return DRNMI_EINVAL;
  if (n == 0) return DRNMI_OK;
  hipLaunchKernelGGL(fake_quant_kernel, dim3(stream_blocks(n / 8)), dim3(kQatThreads), 0, static_cast<hipStream_t>(stream),
                     x, y, n / 8, scale, inv_scale);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_fake_quant_bwd_f32(const float* dq, const float* x, int64_t n, float inv_scale, float* dx,
                                        int32_t accumulate, void* stream) {
  if (dq == nullptr || x == nullptr || dx == nullptr || !aligned16(dq) || !aligned16(x) || !aligned16(dx) || n < 0 ||
      n % 8 != 0 || !positive(inv_scale) || (accumulate != 0 && accumulate != 1))
    return DRNMI_EINVAL;
  if (n == 0) return DRNMI_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (accumulate)
    hipLaunchKernelGGL(fake_quant_bwd_kernel<true>, dim3(stream_blocks(n / 8)), dim3(kQatThreads), 0, s, dq, x, dx, n / 8,
                       inv_scale);
  else
    hipLaunchKernelGGL(fake_quant_bwd_kernel<false>, dim3(stream_blocks(n / 8)), dim3(kQatThreads), 0, s, dq, x, dx, n / 8,
                       inv_scale);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_fake_quant_rows_f32(const float* w, int64_t rows, int32_t cols, float* wq, float* row_scale,
                                         void* stream) {
  if (w == nullptr || wq == nullptr || row_scale == nullptr || !aligned16(w) || !aligned16(wq) ||
      (reinterpret_cast<uintptr_t>(row_scale) & 3) != 0 || rows < 0 || rows >= (int64_t(1) << 31) || cols <= 0)
    return DRNMI_EINVAL;
  if (rows == 0) return DRNMI_OK;
  hipLaunchKernelGGL(fake_quant_rows_kernel, dim3(static_cast<unsigned>(rows)), dim3(kQatThreads), 0,
                     static_cast<hipStream_t>(stream), w, wq, row_scale, rows, cols);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_fake_quant_rows_table_check(const int64_t* t, int32_t n, int64_t* total_rows_out) {
  if (t == nullptr || n <= 0 || n > kFqRowsMaxEntries) return DRNMI_EINVAL;
  int64_t total = 0;
  for (int e = 0; e < n; ++e) {
    const int64_t* q = t + static_cast<int64_t>(e) * DRNMI_FQ_ROWS_ENTRY_WORDS;
    if (q[0] == 0 || q[1] == 0 || q[2] == 0 || ((q[0] | q[1]) & 15) != 0 || (q[2] & 3) != 0) return DRNMI_EINVAL;
    if (q[3] <= 0 || q[4] <= 0 || q[4] >= (int64_t(1) << 31) || q[5] != total) return DRNMI_EINVAL;
    total += q[3];
    if (total >= (int64_t(1) << 31)) return DRNMI_EINVAL;
  }
  if (total_rows_out != nullptr) *total_rows_out = total;
  return DRNMI_OK;
}

extern "C" int drnmi_fake_quant_rows_batched_f32(const int64_t* table, int32_t n, int64_t total_rows, void* stream) {
  if (table == nullptr || n <= 0 || n > kFqRowsMaxEntries || total_rows <= 0 || total_rows >= (int64_t(1) << 31))
    return DRNMI_EINVAL;
  hipLaunchKernelGGL(fake_quant_rows_batched_kernel, dim3(static_cast<unsigned>(total_rows)), dim3(kQatThreads), 0,
                     static_cast<hipStream_t>(stream), table, n, total_rows);
  return static_cast<int>(hipGetLastError());
}
