// Fine-tune data path: the batch the training / validation loop feeds the model, made on the GPU.
//
//   * train ingest: uint8 HWC image + uint8 label -> the crop / reflection pad / flip / ToTensor /
//     Normalize of semantic_seg.py:885-889 (data_transforms.py:9-45, :96-125, :228-253) as fp32 NCHW
//     and an int64 target.  Crop offset, padding and flip arrive as two small index tables per sample
//     (drnmi/data.py index_maps), so the kernel is a gather: per output pixel 3 image bytes, a label
//     byte and a column entry in, 12 B of fp32 and 8 B of target out.
//   * pixel accuracy: eval_score=accuracy (utils.py:267-277) as two device counters, in one pass
//     over the log-prob planes.
//
// Ingest: a thread owns kPx = 4 consecutive x of one (i, y).  Where tw is a multiple of 4 every such
// group starts 16-B aligned in each of the three channel planes and 32-B aligned in the target:
// one 16-B store per plane and two for the target, lane after lane at consecutive addresses.  Any
// other tw (and the groups a 4-B or 8-B aligned buffer leaves) takes scalar stores of the same
// elements.  A flipped sample only reverses the order of the source reads of a row; the stores are
// the same.  Every decoded index is clamped into the image before it is read.
#include "common.h"

namespace drnmi {
namespace {

constexpr int kThreads = 256;
constexpr int kPx = 4;                       // output pixels per thread: 16 B of a channel plane
constexpr int kMaxBlocks = 2048 * 8;         // grid-stride beyond
constexpr int64_t kMaxPixels = 1LL << 40;    // n*h*w and n*th*tw bound: every byte offset fits int64

// table entry -> source index inside [0, size - 1]; pad = the entry marks a padded position
__device__ __forceinline__ int decode(int e, int size, bool& pad) {
  pad = e < 0;
  const int s = pad ? ~e : e;
  return s < 0 ? 0 : (s > size - 1 ? size - 1 : s);
}

struct IngestArgs {
  const uint8_t* images;
  const uint8_t* labels;
  const int32_t* rowmap;
  const int32_t* colmap;
  float* out;
  int64_t* target;
  int h, w, th, tw;
  int groups;            // ceil(tw / kPx)
  int64_t items;         // n * th * groups
  float m[3], s[3];
  int vec_out, vec_tgt;  // 16-B stores allowed (tw % 4 == 0 and the base aligned)
};

__global__ void __launch_bounds__(kThreads) train_ingest_kernel(IngestArgs a) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  const int64_t plane = static_cast<int64_t>(a.th) * a.tw;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; g < a.items; g += stride) {
    int64_t row, i;                                   // row = i * th + y
    int x0, y;
    if (a.items <= 0x7fffffff) {                      // launch-uniform: 32-bit divisions
      const uint32_t g32 = static_cast<uint32_t>(g), row32 = g32 / static_cast<uint32_t>(a.groups);
      const uint32_t i32 = row32 / static_cast<uint32_t>(a.th);
      row = row32;
      i = i32;
      x0 = static_cast<int>(g32 - row32 * a.groups) * kPx;
      y = static_cast<int>(row32 - i32 * a.th);
    } else {
      row = g / a.groups;
      i = row / a.th;
      x0 = static_cast<int>(g - row * a.groups) * kPx;
      y = static_cast<int>(row - i * a.th);
    }
    bool rpad;
    const int r = decode(a.rowmap[row], a.h, rpad);
    const int64_t src_row = (i * a.h + r) * a.w;      // pixel index of the source row's first column
    const int32_t* cm = a.colmap + i * a.tw;
    const int cnt = a.tw - x0 < kPx ? a.tw - x0 : kPx;

    float v[3][kPx];
    int64_t t[kPx] = {};
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
      if (k < cnt) {
        bool cpad;
        const int q = decode(cm[x0 + k], a.w, cpad);
        const int64_t p = src_row + q;
        const uint8_t* px = a.images + p * 3;
        // ToTensor (x / 255) then Normalize (sub_, div_): the op sequence of frame_ingest_kernel
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = (static_cast<float>(px[c]) / 255.0f - a.m[c]) / a.s[c];
        if (a.target != nullptr) t[k] = (rpad || cpad) ? 255 : static_cast<int64_t>(a.labels[p]);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = 0.f;
      }
    }

    const int64_t o = (i * 3 * a.th + y) * a.tw + x0;     // plane 0 of sample i
    if (a.vec_out && cnt == kPx) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(a.out + o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < kPx; ++k)
          if (k < cnt) a.out[o + c * plane + k] = v[c][k];
    }
    if (a.target != nullptr) {
      int64_t* tp = a.target + row * a.tw + x0;
      if (a.vec_tgt && cnt == kPx) {
        typedef long long i64x2 __attribute__((ext_vector_type(2)));
        reinterpret_cast<i64x2*>(tp)[0] = i64x2{t[0], t[1]};
        reinterpret_cast<i64x2*>(tp)[1] = i64x2{t[2], t[3]};
      } else {
#pragma unroll
        for (int k = 0; k < kPx; ++k)
          if (k < cnt) tp[k] = t[k];
      }
    }
  }
}

// ---------------------------------------------------------------- pixel accuracy
// counts[0] += pixels with target != ignore, counts[1] += those whose argmax equals the target.
// A thread takes V consecutive pixels of one sample (V = 4: 16-B loads of every class plane and of
// the target; hw a multiple of 4 and both bases aligned), walks the c planes once, and keeps its
// two counts in registers over the grid-stride loop; then wave shuffle, LDS across the waves, and
// one 64-bit atomic per workgroup and counter.
template <int V>
__global__ void __launch_bounds__(kThreads)
pixel_accuracy_kernel(const float* __restrict__ lp, const int64_t* __restrict__ target, int c, int64_t hw,
                      int64_t items, int64_t ignore, unsigned long long* __restrict__ counts) {
  const int64_t per = hw / V;                        // items per sample (V == 1 or hw % V == 0)
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  unsigned int seen = 0, hit = 0;                    // per thread: at most items / stride * V, far below 2^32
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; g < items; g += stride) {
    const int64_t b = g / per;
    const int64_t p = (g - b * per) * V;
    const float* x = lp + b * c * hw + p;
    float best[V];
    int arg[V];
    if constexpr (V == 4) {
      const float4 f = *reinterpret_cast<const float4*>(x);
      best[0] = f.x; best[1] = f.y; best[2] = f.z; best[3] = f.w;
    } else {
      best[0] = x[0];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) arg[j] = 0;
    for (int k = 1; k < c; ++k) {
      float tv[V];
      if constexpr (V == 4) {
        const float4 f = *reinterpret_cast<const float4*>(x + k * hw);
        tv[0] = f.x; tv[1] = f.y; tv[2] = f.z; tv[3] = f.w;
      } else {
        tv[0] = x[k * hw];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        // first maximum, NaN wins: the rule of argmax_nchw_kernel (torch.max)
        if (tv[j] > best[j] || (tv[j] != tv[j] && best[j] == best[j])) {
          best[j] = tv[j];
          arg[j] = k;
        }
      }
    }
    const int64_t* tp = target + b * hw + p;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t tg = tp[j];
      if (tg != ignore) {
        ++seen;
        hit += tg == static_cast<int64_t>(arg[j]) ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    seen += __shfl_down(seen, off, 64);
    hit += __shfl_down(hit, off, 64);
  }
  __shared__ unsigned int part[2][kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[0][wave] = seen;
    part[1][wave] = hit;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long sum = 0;
#pragma unroll
    for (int wv = 0; wv < kThreads / 64; ++wv) sum += part[threadIdx.x][wv];
    atomicAdd(&counts[threadIdx.x], sum);
  }
}

}  // namespace
}  // namespace drnmi

using namespace drnmi;

extern "C" int drnmi_train_ingest_u8(const uint8_t* images, const uint8_t* labels, int32_t n, int32_t h, int32_t w,
                                     const int32_t* rowmap, const int32_t* colmap, int32_t th, int32_t tw,
                                     const float* mean3, const float* std3, float* out, int64_t* target,
                                     void* stream) {
  if (images == nullptr || rowmap == nullptr || colmap == nullptr || out == nullptr) return DRNMI_EINVAL;
  if (mean3 == nullptr || std3 == nullptr) return DRNMI_EINVAL;
  if ((labels == nullptr) != (target == nullptr)) return DRNMI_EINVAL;
  if (n <= 0 || h <= 0 || w <= 0 || th <= 0 || tw <= 0) return DRNMI_EINVAL;
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0 || (reinterpret_cast<uintptr_t>(target) & 7) != 0)
    return DRNMI_EINVAL;
  // every offset is 64-bit; the element counts are bounded so that no product below can overflow
  const int64_t src_plane = static_cast<int64_t>(h) * w, dst_plane = static_cast<int64_t>(th) * tw;
  if (src_plane > kMaxPixels || n > kMaxPixels / src_plane) return DRNMI_EINVAL;
  if (dst_plane > kMaxPixels || n > kMaxPixels / dst_plane) return DRNMI_EINVAL;

  IngestArgs a;
  a.images = images;
  a.labels = labels;
  a.rowmap = rowmap;
  a.colmap = colmap;
  a.out = out;
  a.target = target;
  a.h = h;
  a.w = w;
  a.th = th;
  a.tw = tw;
  a.groups = (tw + kPx - 1) / kPx;
  a.items = static_cast<int64_t>(n) * th * a.groups;
  for (int c = 0; c < 3; ++c) {
    a.m[c] = mean3[c];
    a.s[c] = std3[c];
  }
  a.vec_out = tw % kPx == 0 ? 1 : 0;                       // out is 16-B aligned (checked above)
  a.vec_tgt = a.vec_out && (reinterpret_cast<uintptr_t>(target) & 15) == 0 ? 1 : 0;
  const int64_t blocks = (a.items + kThreads - 1) / kThreads;
  const dim3 grid(static_cast<unsigned>(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(kThreads);
  hipLaunchKernelGGL(train_ingest_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), a);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_pixel_accuracy_f32(const float* logprobs, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                                        int64_t ignore_index, int64_t* counts, void* stream) {
  if (logprobs == nullptr || target == nullptr || counts == nullptr) return DRNMI_EINVAL;
  if (n <= 0 || c <= 0 || hw <= 0) return DRNMI_EINVAL;
  // n * hw <= 2^40 and c <= 2^20: every element offset of logprobs stays inside int64
  if (hw > kMaxPixels || n > kMaxPixels / hw || c > (1 << 20)) return DRNMI_EINVAL;
  const bool wide = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(logprobs) & 15) == 0;
  const int64_t items = static_cast<int64_t>(n) * (wide ? hw / 4 : hw);
  const int64_t blocks = (items + kThreads - 1) / kThreads;
  const dim3 grid(static_cast<unsigned>(blocks < 2048 ? blocks : 2048)), block(kThreads);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  if (wide)
    hipLaunchKernelGGL(pixel_accuracy_kernel<4>, grid, block, 0, s, logprobs, target, c, hw, items, ignore_index, cnt);
  else
    hipLaunchKernelGGL(pixel_accuracy_kernel<1>, grid, block, 0, s, logprobs, target, c, hw, items, ignore_index, cnt);
  return static_cast<int>(hipGetLastError());
}
