// The head and the confusion matrix for 33 .. 256 classes (ADE20K has 150): the forms of
//   * up x8 + LogSoftmax + argmax      (ops.hip up8_lsm_kernel, c <= 32: the class vector in registers)
//   * bilinear x8 + LogSoftmax + argmax (ops.hip up8_bilinear_lsm_kernel, likewise)
//   * the confusion matrix              (ops.hip confusion_kernel, n <= 32: a 4 KiB LDS table)
// that do not need the class count to fit a register array or a static LDS table.  256 is what a
// uint8 label map can hold.
#include "kernels.h"

namespace drnmi {
namespace {

// ---------------------------------------------------------------- up x8 + log-softmax + argmax, wide
// up8_lsm_kernel keeps its c <= 32 up-sampled logits v[k] in registers between the max, the sum and
// the log-prob pass.  Here they do not fit, so the classes are swept three times and the four-tap
// value is recomputed in each sweep -- the same mul + 3 fma on the same operands, so the same bits,
// and everything after it (running fmaxf, sum += expf(v - vmax), (v - vmax) - logf(sum), first k
// with lp > best) is up8_lsm_kernel's in the same order: the two kernels agree bit for bit wherever
// both run.  The labels-only form (logprobs == nullptr) runs the same three sweeps without the
// stores; it does not take the argmax of the up-sampled logits, because two classes whose v differ
// by less than half an ulp of the log-sum round to one lp, and then the lower index wins.
//
// A workgroup owns 16 output rows x 64 output columns: rows 8 I0 - 4 .. 8 I0 + 11 (the two tap-row
// windows i1 = I0, I0 + 1, as in up8_labels_tile_kernel) and columns 64 bx .. 64 bx + 63.  The columns
// are not offset by the window's 4 pixels, so a thread's float4 log-prob store and a wave's 256-B row
// segment are aligned.  The tile's taps are rows I0 - 1 .. I0 + 1 and columns 8 bx - 1 .. 8 bx + 8: a
// 3 x 10 patch per class, staged once into LDS class-major (patch[k][3][10], 30 KiB at c = 256, so
// five workgroups fit a CU's 160 KiB and eight at c = 150); the sweeps read nothing else.  A tap
// outside the image is up8_lsm_kernel's clamped read (index 0, weight 0), staged as such.
// A thread owns 4 consecutive pixels of one row (two threads per input cell): thread (r, qx),
// r = tid / 16, qx = tid % 16.  A ds_read_b32 is banked per 32-lane half (2 rows x 16 threads): the
// half reads the 9 consecutive words j1 = 8 bx .. 8 bx + 8 of one patch row -- 9 different banks,
// the lanes of one cell broadcast.
constexpr int kWideMaxClasses = 256;
constexpr int kWideRows = 3, kWideCols = 10, kWidePatch = kWideRows * kWideCols;

template <int LABEL_DTYPE>
__global__ void __launch_bounds__(256)
up8_lsm_wide_kernel(const float* __restrict__ logits, const float* __restrict__ up_w, float* __restrict__ logprobs,
                    void* __restrict__ labels, int c, int h, int w) {
  extern __shared__ __attribute__((aligned(16))) float patch[];   // [c][kWideRows][kWideCols]
  __shared__ float wk[256];
  const int tid = threadIdx.x;
  wk[tid] = up_w[tid];

  const int H = h * 8, W = w * 8;
  const int I0 = blockIdx.y * 2;                     // first tap-row window
  const int JB = blockIdx.x * 8 - 1;                 // input column of patch column 0
  const int n = blockIdx.z;
  const int64_t plane = static_cast<int64_t>(h) * w;
  const float* src = logits + static_cast<int64_t>(n) * c * plane;
  for (int e = tid; e < c * kWidePatch; e += 256) {
    const int k = e / kWidePatch, r = e - k * kWidePatch;
    const int pi = r / kWideCols, pj = r - pi * kWideCols;
    int iy = I0 - 1 + pi, ix = JB + pj;
    iy = (iy < 0 || iy >= h) ? 0 : iy;               // up8_lsm_kernel's ci / cj
    ix = (ix < 0 || ix >= w) ? 0 : ix;
    patch[e] = src[k * plane + static_cast<int64_t>(iy) * w + ix];
  }
  __syncthreads();

  const int row = tid >> 4, qx = tid & 15;
  const int q = blockIdx.x * 16 + qx;                // output columns 4 q .. 4 q + 3
  const int oy = 8 * I0 - 4 + row;
  if (4 * q >= W || oy < 0 || oy >= H) return;

  const int ti = row >> 3;
  const int i1 = I0 + ti, i0 = i1 - 1;               // i1 = (oy + 4) >> 3
  const int ky1 = row & 7, ky0 = ky1 + 8;
  const int j1 = (q + 1) >> 1, j0 = j1 - 1;
  const bool vi0 = i0 >= 0, vi1 = i1 < h, vj0 = j0 >= 0, vj1 = j1 < w;
  float w00[4], w01[4], w10[4], w11[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int kx1 = 4 * q + p + 4 - 8 * j1, kx0 = kx1 + 8;
    w00[p] = (vi0 && vj0) ? wk[ky0 * 16 + kx0] : 0.f;
    w01[p] = (vi0 && vj1) ? wk[ky0 * 16 + kx1] : 0.f;
    w10[p] = (vi1 && vj0) ? wk[ky1 * 16 + kx0] : 0.f;
    w11[p] = (vi1 && vj1) ? wk[ky1 * 16 + kx1] : 0.f;
  }
  // tap (i0, j0) of class k: tp[k * kWidePatch]; (i0, j1): + 1; (i1, j0): + kWideCols; (i1, j1): + kWideCols + 1
  const float* tp = patch + ti * kWideCols + (j0 - JB);
  auto upsampled = [&](int k, float (&a)[4]) {
    const float* t = tp + k * kWidePatch;
    const float s00 = t[0], s01 = t[1], s10 = t[kWideCols], s11 = t[kWideCols + 1];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float v = s00 * w00[p];
      v = fmaf(s01, w01[p], v);
      v = fmaf(s10, w10[p], v);
      v = fmaf(s11, w11[p], v);
      a[p] = v;
    }
  };

  float vmax[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int k = 0; k < c; ++k) {
    float a[4];
    upsampled(k, a);
#pragma unroll
    for (int p = 0; p < 4; ++p) vmax[p] = fmaxf(vmax[p], a[p]);
  }
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < c; ++k) {
    float a[4];
    upsampled(k, a);
#pragma unroll
    for (int p = 0; p < 4; ++p) sum[p] += expf(a[p] - vmax[p]);
  }
  float lse[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) lse[p] = logf(sum[p]);

  const int64_t HW = static_cast<int64_t>(H) * W;
  const int64_t pix = static_cast<int64_t>(oy) * W + 4 * q;
  float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int arg[4] = {0, 0, 0, 0};
  float* out = logprobs != nullptr ? logprobs + static_cast<int64_t>(n) * c * HW + pix : nullptr;
  for (int k = 0; k < c; ++k) {
    float a[4], lp[4];
    upsampled(k, a);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      lp[p] = (a[p] - vmax[p]) - lse[p];
      if (lp[p] > best[p]) { best[p] = lp[p]; arg[p] = k; }
    }
    if (out != nullptr) *reinterpret_cast<float4*>(out + k * HW) = make_float4(lp[0], lp[1], lp[2], lp[3]);
  }
  if (labels != nullptr) {
    if (LABEL_DTYPE == DRNMI_U8) {
      const uint32_t packed = static_cast<uint32_t>(arg[0]) | (static_cast<uint32_t>(arg[1]) << 8) |
                              (static_cast<uint32_t>(arg[2]) << 16) | (static_cast<uint32_t>(arg[3]) << 24);
      *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(labels) + static_cast<int64_t>(n) * HW + pix) = packed;
    } else {
      int64_t* o = reinterpret_cast<int64_t*>(labels) + static_cast<int64_t>(n) * HW + pix;
#pragma unroll
      for (int p = 0; p < 4; ++p) o[p] = arg[p];
    }
  }
}

// ---------------------------------------------------------------- bilinear x8 (use_torch_up), wide
// up8_bilinear_lsm_kernel's per-pixel arithmetic in three sweeps, one pixel per thread.  No shipped
// configuration uses this head, so the four taps come from global memory (L2) in every sweep.  The
// interpolation is one function with contraction off, so the three sweeps cannot round differently.
__device__ __forceinline__ void bilinear_ac_index(int dst, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  const float scale = out > 1 ? static_cast<float>(in - 1) / static_cast<float>(out - 1) : 0.f;
  const float src = scale * static_cast<float>(dst);
  i0 = static_cast<int>(floorf(src));
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - static_cast<float>(i0), 0.f), 1.f);
  l0 = 1.f - l1;
}

__device__ __forceinline__ float bilinear_value(const float* __restrict__ s, int o00, int o01, int o10, int o11,
                                                float wx0, float wx1, float hy0, float hy1) {
#pragma clang fp contract(off)
  const float top = wx0 * s[o00] + wx1 * s[o01];
  const float bot = wx0 * s[o10] + wx1 * s[o11];
  return hy0 * top + hy1 * bot;
}

template <int LABEL_DTYPE>
__global__ void __launch_bounds__(256)
up8_bilinear_lsm_wide_kernel(const float* __restrict__ logits, float* __restrict__ logprobs, void* __restrict__ labels,
                             int c, int h, int w) {
  const int H = h * 8, W = w * 8;
  const int ox = blockIdx.x * blockDim.x + threadIdx.x;
  const int oy = blockIdx.y;
  const int n = blockIdx.z;
  if (ox >= W) return;
  int y0, y1, x0, x1;
  float hy0, hy1, wx0, wx1;
  bilinear_ac_index(oy, h, H, y0, y1, hy0, hy1);
  bilinear_ac_index(ox, w, W, x0, x1, wx0, wx1);
  const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
  const int64_t plane = static_cast<int64_t>(h) * w;
  const float* src = logits + static_cast<int64_t>(n) * c * plane;
  float vmax = -INFINITY;
  for (int k = 0; k < c; ++k)
    vmax = fmaxf(vmax, bilinear_value(src + k * plane, o00, o01, o10, o11, wx0, wx1, hy0, hy1));
  float sum = 0.f;
  for (int k = 0; k < c; ++k)
    sum += expf(bilinear_value(src + k * plane, o00, o01, o10, o11, wx0, wx1, hy0, hy1) - vmax);
  const float lse = logf(sum);
  const int64_t HW = static_cast<int64_t>(H) * W;
  const int64_t pix = static_cast<int64_t>(oy) * W + ox;
  float best = -INFINITY;
  int arg = 0;
  for (int k = 0; k < c; ++k) {
    const float lp = (bilinear_value(src + k * plane, o00, o01, o10, o11, wx0, wx1, hy0, hy1) - vmax) - lse;
    if (logprobs != nullptr) logprobs[(static_cast<int64_t>(n) * c + k) * HW + pix] = lp;
    if (lp > best) { best = lp; arg = k; }
  }
  if (labels != nullptr) {
    if (LABEL_DTYPE == DRNMI_U8) reinterpret_cast<uint8_t*>(labels)[static_cast<int64_t>(n) * HW + pix] = static_cast<uint8_t>(arg);
    else reinterpret_cast<int64_t*>(labels)[static_cast<int64_t>(n) * HW + pix] = arg;
  }
}

// ---------------------------------------------------------------- confusion matrix, wide
// confusion_kernel's counting (workgroup-private uint32 bins in LDS, one 64-bit global atomic per
// non-zero bin per workgroup) with the table in dynamic LDS: n x n counters are 88 KiB at n = 150
// and fit 128 KiB up to n = 181.  Above that the label rows are split into slabs of ceil(n / slabs)
// rows (two slabs of at most 128 x 256 at n = 256), blockIdx.y = slab: every slab's workgroups read
// all the pixels and count the labels of their rows only.  One workgroup per CU fits, so it has
// 1024 threads.  Label maps are spatially coherent: when all the active lanes of a wave hit one bin
// (or none), one lane adds their count instead of 64 serialised LDS atomics on one address.
// Overflow: the grid is at most kHistWideGrid workgroups per slab, each counting at most
// ceil(npix / (kHistWideGrid * 1024)) * 1024 pixels when the grid is at its cap and 8192 below it,
// so no uint32 bin wraps for npix < 2^42 (the entry point refuses more than 2^40).
constexpr int kHistWideBytes = 128 * 1024;
constexpr int kHistWideGrid = 1024;
constexpr int kHistWideThreads = 1024;

template <typename TP, typename TL>
__global__ void __launch_bounds__(kHistWideThreads)
confusion_wide_kernel(const TP* __restrict__ pred, const TL* __restrict__ label, int64_t npix, int n, int rows,
                      unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned int hbins[];            // [rows][n]
  const int row0 = blockIdx.y * rows;
  const int nrow = min(rows, n - row0);
  const int nbins = nrow * n;
  for (int i = threadIdx.x; i < nbins; i += kHistWideThreads) hbins[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kHistWideThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kHistWideThreads + threadIdx.x; i < npix; i += stride) {
    const int64_t l = static_cast<int64_t>(label[i]);
    const int64_t p = static_cast<int64_t>(pred[i]);
    const bool ok = l >= row0 && l < row0 + nrow && p >= 0 && p < n;
    const int bin = ok ? static_cast<int>(l - row0) * n + static_cast<int>(p) : -1;
    const unsigned long long active = __ballot(1);
    const int first = __builtin_amdgcn_readfirstlane(bin);
    if (__ballot(bin != first) == 0) {               // the wave's active lanes agree
      if (first >= 0 && lane == __ffsll(static_cast<long long>(active)) - 1)
        atomicAdd(&hbins[first], static_cast<unsigned int>(__popcll(active)));
    } else if (bin >= 0) {
      atomicAdd(&hbins[bin], 1u);
    }
  }
  __syncthreads();
  unsigned long long* out = hist + static_cast<int64_t>(row0) * n;
  for (int i = threadIdx.x; i < nbins; i += kHistWideThreads)
    if (hbins[i]) atomicAdd(&out[i], static_cast<unsigned long long>(hbins[i]));
}

template <typename TP, typename TL>
int launch_confusion_wide(const void* pred, const void* label, int64_t npix, int n, unsigned long long* hist,
                          hipStream_t s) {
  const int slabs = ceil_div(static_cast<int64_t>(n) * n * 4, kHistWideBytes);
  const int rows = ceil_div(n, slabs);
  const int lds = rows * n * 4;
  static bool attr_set = false;                      // per instantiation: above 64 KiB is opt-in
  if (!attr_set) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&confusion_wide_kernel<TP, TL>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, kHistWideBytes);
    if (e != hipSuccess) return static_cast<int>(e);
    attr_set = true;
  }
  int64_t g = (npix + 8 * kHistWideThreads - 1) / (8 * kHistWideThreads);
  g = g > kHistWideGrid ? kHistWideGrid : g;
  hipLaunchKernelGGL((confusion_wide_kernel<TP, TL>), dim3(static_cast<unsigned>(g), static_cast<unsigned>(slabs)),
                     dim3(kHistWideThreads), lds, s, static_cast<const TP*>(pred), static_cast<const TL*>(label), npix,
                     n, rows, hist);
  return static_cast<int>(hipGetLastError());
}

}  // namespace

int up8_wide_dispatch(const float* logits, const float* up_w, float* logprobs, void* labels, int label_dtype, int n,
                      int c, int h, int w, hipStream_t s) {
  if (logits == nullptr || up_w == nullptr || n <= 0 || h <= 0 || w <= 0) return DRNMI_EINVAL;
  if (c <= 0 || c > kWideMaxClasses) return DRNMI_ENOTSUP;
  if (labels != nullptr && label_dtype != DRNMI_U8 && label_dtype != DRNMI_I64) return DRNMI_EINVAL;
  if (static_cast<int64_t>(h) * 8 > 65535 || n > 65535) return DRNMI_EINVAL;
  // float4 log-prob stores and packed uint8 label stores
  if ((reinterpret_cast<uintptr_t>(logprobs) & 15) != 0) return DRNMI_EINVAL;
  if ((reinterpret_cast<uintptr_t>(labels) & (label_dtype == DRNMI_I64 ? 7 : 3)) != 0) return DRNMI_EINVAL;
  const dim3 grid(static_cast<unsigned>((w + 7) / 8), static_cast<unsigned>(h / 2 + 1), static_cast<unsigned>(n));
  const size_t lds = static_cast<size_t>(c) * kWidePatch * sizeof(float);
  if (label_dtype == DRNMI_I64)
    hipLaunchKernelGGL(up8_lsm_wide_kernel<DRNMI_I64>, grid, dim3(256), lds, s, logits, up_w, logprobs, labels, c, h, w);
  else
    hipLaunchKernelGGL(up8_lsm_wide_kernel<DRNMI_U8>, grid, dim3(256), lds, s, logits, up_w, logprobs, labels, c, h, w);
  return static_cast<int>(hipGetLastError());
}

int up8_bilinear_wide_dispatch(const float* logits, float* logprobs, void* labels, int label_dtype, int n, int c, int h,
                               int w, hipStream_t s) {
  if (c <= 0 || c > kWideMaxClasses) return DRNMI_ENOTSUP;
  const int W = w * 8;
  const dim3 grid(static_cast<unsigned>((W + 255) / 256), static_cast<unsigned>(h * 8), static_cast<unsigned>(n));
  if (label_dtype == DRNMI_I64)
    hipLaunchKernelGGL(up8_bilinear_lsm_wide_kernel<DRNMI_I64>, grid, dim3(256), 0, s, logits, logprobs, labels, c, h, w);
  else
    hipLaunchKernelGGL(up8_bilinear_lsm_wide_kernel<DRNMI_U8>, grid, dim3(256), 0, s, logits, logprobs, labels, c, h, w);
  return static_cast<int>(hipGetLastError());
}

int confusion_wide_dispatch(const void* pred, int pred_dtype, const void* label, int label_dtype, int64_t npix,
                            int nclass, int64_t* hist, hipStream_t s) {
  if (nclass <= 0 || nclass > kWideMaxClasses) return DRNMI_ENOTSUP;
  if (npix > (static_cast<int64_t>(1) << 40)) return DRNMI_ENOTSUP;
  auto* h = reinterpret_cast<unsigned long long*>(hist);
  if (pred_dtype == DRNMI_U8 && label_dtype == DRNMI_U8)
    return launch_confusion_wide<uint8_t, uint8_t>(pred, label, npix, nclass, h, s);
  if (pred_dtype == DRNMI_U8) return launch_confusion_wide<uint8_t, int64_t>(pred, label, npix, nclass, h, s);
  if (label_dtype == DRNMI_U8) return launch_confusion_wide<int64_t, uint8_t>(pred, label, npix, nclass, h, s);
  return launch_confusion_wide<int64_t, int64_t>(pred, label, npix, nclass, h, s);
}

}  // namespace drnmi

using namespace drnmi;

extern "C" int drnmi_up8_logsoftmax_argmax_wide(const float* logits, const float* up_w, float* logprobs, void* labels,
                                                int32_t label_dtype, int32_t n, int32_t c, int32_t h, int32_t w,
                                                void* stream) {
  return up8_wide_dispatch(logits, up_w, logprobs, labels, label_dtype, n, c, h, w, reinterpret_cast<hipStream_t>(stream));
}
