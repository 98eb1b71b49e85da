// Label maps to pictures: palette colouring and overlay onto the input frames.
//
//   * seg_video_old_no_plot.py:166-170: every frame's argmax goes through CITYSCAPE_PALETTE[pred];
//     the seg_video*.py variants draw that over the (resized) input frame with alpha = 0.6.
//   * semantic_seg.py:415-426, :448-452, :539-542: test / test_ms write palettes[pred] per image.
//
// One streaming pass after the head, for every precision and head path: per pixel 1 or 8 label
// bytes and (overlay) 3 frame bytes in, 3 bytes out.  Exact integer arithmetic (include/drnmi.h
// drnmi_render_labels): colour = palette[min(label, P - 1)], out = (f*(256-a) + c*a + 128) >> 8.
//
// Frames and output are both dense [n][oh][ow][3], so they are one flat byte stream with the same
// index: a thread takes kPx = 16 consecutive pixels of it = 48 bytes = three 16-B pieces, aligned
// whatever ow is (ow * 3 is no multiple of 4 for most cropped widths).  A block moves its tile of
// 256 x 48 B through LDS, so that the global loads and stores are 16 B per lane at consecutive
// addresses (measured at 8x1024x2048: colour 20.7 -> 12.6 us, overlay 29.7 -> 26.9 us against
// each thread loading and storing its own 48 B; a second LDS buffer to save a barrier was slower,
// 6 instead of 8 waves per SIMD).  Only the label address depends on the row (lw != ow shifts the
// label rows against the output rows): a cursor walks (x, y) along the 16 pixels, and uint8 labels
// are read a dword at a time wherever 4 pixels stay in one row at a 4-B aligned label address,
// bytes otherwise.  int64 labels are read one by one, 128 B apart between lanes: that path (the
// eval drivers' labels) runs at about 1 TB/s, not at the uint8 path's rate.  The last, partial
// tile and buffers that are not 16-B aligned take the per-thread path, per-pixel bytes at the end.
// The palette is staged once per block in LDS as 256 packed dwords: entries P.. repeat entry
// P - 1 (the clamp then is a plain 8-bit index), already reversed when swap_rb is set.
#include "common.h"

namespace drnmi {
namespace {

constexpr int kThreads = 256;
constexpr int kPx = 16;                      // pixels per thread and step: 48 B of frame / output
constexpr int kTile = kThreads * kPx;        // pixels per block and step
constexpr int kMaxBlocks = 2048;             // grid-stride beyond (256 CUs x 8 blocks)
constexpr int64_t kMaxPixels = 1LL << 40;    // n*lh*lw bound: every byte offset fits int64 with room

// position of one output pixel and of its label: x, y inside the frame, lab = label element index
struct Cursor {
  int x, y;
  int64_t lab;
};

struct Geom {
  int oh, ow, lw;
  int64_t row_skip;      // lw - ow: label elements between the end of a cropped row and the next
  int64_t frame_skip;    // (lh - oh) * lw: label rows below the crop
};

__host__ __device__ __forceinline__ Cursor cursor_at(int64_t p, const Geom& g, int lh) {
  const int64_t r = p / g.ow;
  const int64_t f = r / g.oh;
  Cursor c;
  c.x = static_cast<int>(p - r * g.ow);
  c.y = static_cast<int>(r - f * g.oh);
  c.lab = (f * lh + c.y) * g.lw + c.x;
  return c;
}

// carry after x has been advanced (x <= ow on entry)
__host__ __device__ __forceinline__ void wrap(Cursor& c, const Geom& g) {
  if (c.x == g.ow) {
    c.x = 0;
    c.lab += g.row_skip;
    if (++c.y == g.oh) {
      c.y = 0;
      c.lab += g.frame_skip;
    }
  }
}

template <bool I64>
__host__ __device__ __forceinline__ uint32_t label_at(const void* labels, int64_t i) {
  if (I64) {
    const uint64_t v = static_cast<uint64_t>(reinterpret_cast<const int64_t*>(labels)[i]);
    return v > 255u ? 255u : static_cast<uint32_t>(v);      // negative labels too: the last entry
  }
  return reinterpret_cast<const uint8_t*>(labels)[i];
}

// palette dwords (0x00c2c1c0, c0 the first byte written) of the next 4 pixels; advances the cursor
template <bool I64>
__host__ __device__ __forceinline__ void colours4(const void* labels, const uint32_t* pal, Cursor& c, const Geom& g,
                                                  uint32_t (&col)[4]) {
  const uint8_t* l8 = reinterpret_cast<const uint8_t*>(labels) + c.lab;
  if (!I64 && c.x + 4 <= g.ow && (reinterpret_cast<uintptr_t>(l8) & 3) == 0) {
    const uint32_t l4 = *reinterpret_cast<const uint32_t*>(l8);
#pragma unroll
    for (int i = 0; i < 4; ++i) col[i] = pal[(l4 >> (8 * i)) & 255u];
    c.x += 4;
    c.lab += 4;
    wrap(c, g);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    col[i] = pal[label_at<I64>(labels, c.lab)];
    ++c.x;
    ++c.lab;
    wrap(c, g);
  }
}

// (f*(256-a) + c*a + 128) >> 8 on the four bytes of a dword, two 16-bit lanes at a time (the sum
// is at most 255 * 256 + 128 < 2^16, so the lanes do not carry into each other)
__host__ __device__ __forceinline__ uint32_t blend4(uint32_t f, uint32_t c, uint32_t a) {
  const uint32_t m = 0x00ff00ffu, ia = 256u - a;
  const uint32_t even = ((f & m) * ia + (c & m) * a + 0x00800080u) >> 8;
  const uint32_t odd = ((f >> 8) & m) * ia + ((c >> 8) & m) * a + 0x00800080u;
  return (even & m) | (odd & ~m);
}

__host__ __device__ __forceinline__ uint4 blend16(const uint4& f, const uint4& c, uint32_t a) {
  return make_uint4(blend4(f.x, c.x, a), blend4(f.y, c.y, a), blend4(f.z, c.z, a), blend4(f.w, c.w, a));
}

// the 48 colour bytes of the next kPx pixels; advances the cursor
template <bool I64>
__host__ __device__ __forceinline__ void colours16(const void* labels, const uint32_t* pal, Cursor& c, const Geom& g,
                                                   uint4 (&o)[3]) {
  uint32_t d[12];
#pragma unroll
  for (int q = 0; q < 4; ++q) {           // 4 pixels = 12 bytes = 3 dwords
    uint32_t col[4];
    colours4<I64>(labels, pal, c, g, col);
    d[3 * q + 0] = col[0] | (col[1] << 24);
    d[3 * q + 1] = (col[1] >> 8) | (col[2] << 16);
    d[3 * q + 2] = (col[2] >> 16) | (col[3] << 8);
  }
  o[0] = make_uint4(d[0], d[1], d[2], d[3]);
  o[1] = make_uint4(d[4], d[5], d[6], d[7]);
  o[2] = make_uint4(d[8], d[9], d[10], d[11]);
}

// one thread's step: pixels [ch * kPx, min((ch + 1) * kPx, total)) of the flat output
template <bool I64, bool OVERLAY>
__host__ __device__ __forceinline__ void render_chunk(int64_t ch, const void* labels, const uint8_t* frames,
                                                      const uint32_t* pal, uint32_t alpha, uint8_t* out, int lh,
                                                      const Geom& g, int64_t total, int wide) {
  const int64_t p0 = ch * kPx;
  Cursor c = cursor_at(p0, g, lh);
  if (wide && p0 + kPx <= total) {
    uint4 o[3];
    colours16<I64>(labels, pal, c, g, o);
    uint4* dst = reinterpret_cast<uint4*>(out + p0 * 3);
    if (OVERLAY) {
      const uint4* src = reinterpret_cast<const uint4*>(frames + p0 * 3);
#pragma unroll
      for (int j = 0; j < 3; ++j) o[j] = blend16(src[j], o[j], alpha);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) dst[j] = o[j];
    return;
  }
  const int64_t p1 = p0 + kPx < total ? p0 + kPx : total;
  for (int64_t p = p0; p < p1; ++p) {
    const uint32_t col = pal[label_at<I64>(labels, c.lab)];
    ++c.x;
    ++c.lab;
    wrap(c, g);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      uint32_t v = (col >> (8 * k)) & 255u;
      if (OVERLAY) v = (frames[p * 3 + k] * (256u - alpha) + v * alpha + 128u) >> 8;
      out[p * 3 + k] = static_cast<uint8_t>(v);
    }
  }
}

// palette entry e as the dword the kernel indexes: 0x00c2c1c0, c0 the first byte written
__host__ __device__ __forceinline__ uint32_t pack_entry(const uint8_t* palette, int P, int e, int swap_rb) {
  e = e < P ? e : P - 1;
  const uint32_t r = palette[3 * e], gr = palette[3 * e + 1], b = palette[3 * e + 2];
  return swap_rb ? (b | (gr << 8) | (r << 16)) : (r | (gr << 8) | (b << 16));
}

template <bool I64, bool OVERLAY>
__global__ void __launch_bounds__(kThreads)
render_labels_kernel(const void* __restrict__ labels, const uint8_t* frames, const uint8_t* __restrict__ palette, int P,
                     int swap_rb, uint32_t alpha, uint8_t* out, int lh, Geom g, int64_t total, int wide) {
  __shared__ uint32_t pal[256];
  __shared__ uint4 stage[3 * kThreads];      // one tile's frame / output bytes: 48 B per thread
  const int tid = threadIdx.x;
  pal[tid] = pack_entry(palette, P, tid, swap_rb);      // kThreads == 256 entries
  __syncthreads();
  const int64_t tiles = (total + kTile - 1) / kTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {       // the same trip count for the whole block
    const int64_t ch = t * kThreads + tid;
    if (!wide || (t + 1) * kTile > total) {                       // block-uniform: the last tile, unaligned buffers
      if (ch * kPx < total) render_chunk<I64, OVERLAY>(ch, labels, frames, pal, alpha, out, lh, g, total, wide);
      continue;
    }
    // a full tile moves through LDS, so that the global loads and stores are 16 B per lane at
    // consecutive addresses (4 KiB per instruction and block) where a thread's own 48 B would
    // put the lanes 48 B apart; the 48-B stride of the LDS side is conflict-free for b128
    uint4 f[3] = {};
    if (OVERLAY) {
      const uint4* src = reinterpret_cast<const uint4*>(frames + t * kTile * 3);
#pragma unroll
      for (int j = 0; j < 3; ++j) stage[j * kThreads + tid] = src[j * kThreads + tid];
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 3; ++j) f[j] = stage[3 * tid + j];
      __syncthreads();
    }
    Cursor c = cursor_at(ch * kPx, g, lh);
    uint4 o[3];
    colours16<I64>(labels, pal, c, g, o);
#pragma unroll
    for (int j = 0; j < 3; ++j) stage[3 * tid + j] = OVERLAY ? blend16(f[j], o[j], alpha) : o[j];
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(out + t * kTile * 3);
#pragma unroll
    for (int j = 0; j < 3; ++j) dst[j * kThreads + tid] = stage[j * kThreads + tid];
    __syncthreads();
  }
}

}  // namespace
}  // namespace drnmi

using namespace drnmi;

extern "C" int drnmi_render_labels(const void* labels, int32_t label_dtype, int32_t n, int32_t lh, int32_t lw,
                                   const uint8_t* frames, const uint8_t* palette, int32_t P, int32_t alpha_q8,
                                   int32_t swap_rb, uint8_t* out, int32_t oh, int32_t ow, void* stream) {
  if (labels == nullptr || palette == nullptr || out == nullptr) return DRNMI_EINVAL;
  if (label_dtype != DRNMI_U8 && label_dtype != DRNMI_I64) return DRNMI_EINVAL;
  if (P < 1 || P > 256) return DRNMI_EINVAL;
  if (n <= 0 || lh <= 0 || lw <= 0 || oh <= 0 || ow <= 0 || oh > lh || ow > lw) return DRNMI_EINVAL;
  if (frames != nullptr && (alpha_q8 < 0 || alpha_q8 > 256)) return DRNMI_EINVAL;
  // every offset is 64-bit; the element count is bounded so that no product below can overflow
  const int64_t plane = static_cast<int64_t>(lh) * lw;          // < 2^62
  if (plane > kMaxPixels || n > kMaxPixels / plane) return DRNMI_EINVAL;
  const int64_t total = static_cast<int64_t>(n) * oh * ow;      // <= n * lh * lw <= 2^40

  Geom g;
  g.oh = oh;
  g.ow = ow;
  g.lw = lw;
  g.row_skip = lw - ow;
  g.frame_skip = static_cast<int64_t>(lh - oh) * lw;
  const uintptr_t align = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(frames);
  const int wide = (align & 15) == 0 ? 1 : 0;
  const int64_t blocks64 = ((total + kPx - 1) / kPx + kThreads - 1) / kThreads;
  const dim3 grid(static_cast<unsigned>(blocks64 < kMaxBlocks ? blocks64 : kMaxBlocks)), block(kThreads);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t a = static_cast<uint32_t>(alpha_q8);
  const bool i64 = label_dtype == DRNMI_I64;
#define DRNMI_RENDER(I64, OV)                                                                                      \
  hipLaunchKernelGGL((render_labels_kernel<I64, OV>), grid, block, 0, s, labels, frames, palette, P, swap_rb, a, out, \
                     lh, g, total, wide)
  if (frames != nullptr) {
    if (i64) DRNMI_RENDER(true, true);
    else DRNMI_RENDER(false, true);
  } else {
    if (i64) DRNMI_RENDER(true, false);
    else DRNMI_RENDER(false, false);
  }
#undef DRNMI_RENDER
  return static_cast<int>(hipGetLastError());
}
