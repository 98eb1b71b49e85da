// The head and the confusion matrix for 33 .. 256 classes (ADE20K has 150): the forms of
//   * up x8 + LogSoftmax + argmax      (ops.hip up8_lsm_kernel, c <= 32: the class vector in registers)
//   * bilinear x8 + LogSoftmax + argmax (ops.hip up8_bilinear_lsm_kernel, likewise)
//   * the confusion matrix              (ops.hip confusion_kernel, n <= 32: a 4 KiB LDS table)
// that do not need the class count to fit a register array or a static LDS table, and the
// labels-only video head on NHWC logit rows for any class count (up8_labels_wide_tile_kernel, the
// runtime-class-count form of ops.hip's up8_labels_tile_kernel).  256 is what a uint8 label map can
// hold.
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

// The three sweeps for the 4 pixels of one thread, shared by up8_lsm_wide_kernel and the full path of
// up8_labels_wide_tile_kernel so that the two cannot round differently: class k's four taps are
// t00[k * KS] (i0, j0), t01[k * KS] (i0, j1), t10[k * KS] (i1, j0), t11[k * KS] (i1, j1); the
// up-sampled value is one mul + 3 fma in that order with the pixel's weights (0 for a tap outside
// the image).  out: the 4 pixels' log-prob address in plane 0 (planes HW apart), or nullptr.
template <int KS>
__device__ __forceinline__ void lsm_sweeps4(const float* t00, const float* t01, const float* t10, const float* t11,
                                            const float (&w00)[4], const float (&w01)[4], const float (&w10)[4],
                                            const float (&w11)[4], int c, float* out, int64_t HW, int (&arg)[4]) {
  auto upsampled = [&](int k, float (&a)[4]) {
    const float s00 = t00[k * KS], s01 = t01[k * KS], s10 = t10[k * KS], s11 = t11[k * KS];
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

  float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int p = 0; p < 4; ++p) arg[p] = 0;
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
}

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
  const int64_t HW = static_cast<int64_t>(H) * W;
  const int64_t pix = static_cast<int64_t>(oy) * W + 4 * q;
  int arg[4];
  float* out = logprobs != nullptr ? logprobs + static_cast<int64_t>(n) * c * HW + pix : nullptr;
  lsm_sweeps4<kWidePatch>(tp, tp + 1, tp + kWideCols, tp + kWideCols + 1, w00, w01, w10, w11, c, out, HW, arg);
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

// ---------------------------------------------------------------- labels only, NHWC logits, 1 .. 256 classes
// The runtime-class-count form of ops.hip's up8_labels_tile_kernel (read that comment first): the
// labels-only video head on the seg conv's fp32 NHWC rows [n][h][w][cs] (classes 0 .. c - 1 first;
// the columns c .. cs - 1 are never read into a decision).  The labels are those of the labels-only
// drnmi_up8_logsoftmax_argmax on the same values: the first k with lp > best over
// lp = (v - vmax) - logf(sum), v = one mul + 3 fma over the taps (lsm_sweeps4).
//
// A workgroup owns TI x TJ tap windows (window (i1, j1) = the 8 x 8 output pixels whose taps are the
// 1/8-res pixels (i1 - 1 .. i1, j1 - 1 .. j1)); TI x TJ <= 128 is chosen from c so that the tile's
// (TI + 1) x (TJ + 1) logit vectors fit LDS (wide_tile_shape).
//   1. the tile's vectors to LDS, pixel-major, VS floats apart (VS / 4 odd, so the vectors of
//      neighbouring pixels start in different banks), by float4 row reads; a pixel outside the image
//      is staged as up8_lsm_wide_kernel's clamped read (index 0, and its weight is 0);
//   2. the per-pixel summary, four lanes per pixel over contiguous class ranges and merged in class
//      order: argmax, top-2 margin, |best|, all classes finite;
//   3. one window per thread: the fast path's test exactly as up8_labels_tile_kernel's -- interior
//      window, the four taps share their argmax, every class finite and the smallest top-2 margin is
//      at least
//          guard = 2^-16 / min_phase(sum w) * (1 + 2^-10) + 2^-20 * max_t |L_t[best]|
//      -- then the 64 labels are written with no per-pixel work; the others go to a slow list;
//   4. a slow window per 16 lanes (8 rows x 2 four-pixel halves).  Interior all-finite windows first
//      build their candidate list: class k is kept when max_t L_t[k] >= max_j min_t L_t[j] - guard
//      (guard with max |L| over all taps and classes); a class below that can neither win nor come
//      within 2^-16 of the winner anywhere in the window.  The 4 pixels are decided over the
//      candidates (the same mul + 3 fma), and when the top two candidates of any of them are closer
//      than 2^-16 -- and in border windows (a tap outside the image: clamped tap, zero weight) and
//      windows with a non-finite tap -- lsm_sweeps4 runs over all c classes: the arithmetic of
//      up8_lsm_wide_kernel, from the same function.
// Why 2^-16 still separates argmax v from argmax lp at c <= 256: a pixel decided without the sweeps
// has v_best - v_k >= 2^-16 for every other k (fast path and pruning: the bounds above, whose terms
// -- the weights' sum, the rounding of one mul + 3 fma against max |L| -- do not depend on the class
// count; candidates: tested).  Then v_best = vmax, v_best - vmax = 0 and lp_best = -lse exactly, and
// for the others d = vmax - v_k >= 2^-16 is computed with a relative error of 2^-24 and
// lp_k = fl(-d' - lse) with 0 <= lse <= ln 256 < 8: below 16 in magnitude the ulp of lp_k is at most
// 2^-20 < d', above it is at most 2^-23 (d' + lse) < d', and rounding is monotone, so lp_k < lp_best
// strictly and the first k with lp > best is argmax v.  An exact tie has d = 0 and takes the sweeps.
// Labels are identical to the NCHW head's (tests/test_gpu_wide_labels.py).  Measured on a 150-class
// network's logits, 2 x 1024 x 2048 (scripts/wide_labels_micro.py, profiles/many_classes_video): 208
// us against 426 us for the labels-only up8_lsm_wide_kernel; on random logits 306 against 423 us.
// The tile: 8 x 16 windows up to 32 classes, 4 x 16 up to 80, 4 x 8 above -- at most 29 KiB of
// vectors up to 150 classes and 46 KiB at 256 (plus 7 KiB of static tables), so that four to five
// workgroups share a CU's 160 KiB (two at 256): the slow windows' rounds are chains of dependent LDS
// reads, and other workgroups' waves are what hides them.  Never above 64 KiB: no opt-in is needed.
constexpr int kTileMaxPx = 9 * 17;                   // staged pixels of the largest tile (8 x 16 windows)

__host__ __device__ inline void wide_tile_shape(int c, int& ti, int& tj, int& vs) {
  ti = c <= 32 ? 8 : 4;
  tj = c <= 80 ? 16 : 8;
  vs = 4 * (((c + 3) >> 2) | 1);
}

template <int LABEL_DTYPE>
__device__ __forceinline__ void store_wide_labels4(void* labels, int64_t pix, const int (&arg)[4]) {
  if (LABEL_DTYPE == DRNMI_U8) {
    const uint32_t packed = static_cast<uint32_t>(arg[0]) | (static_cast<uint32_t>(arg[1]) << 8) |
                            (static_cast<uint32_t>(arg[2]) << 16) | (static_cast<uint32_t>(arg[3]) << 24);
    *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(labels) + pix) = packed;
  } else {
    int64_t* o = reinterpret_cast<int64_t*>(labels) + pix;
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = arg[p];
  }
}

// STATS (the test entry): stats[0] += fast windows, [1] += pixels decided over candidates,
// [2] += pixels through the sweeps
template <int LABEL_DTYPE, bool STATS>
__global__ void __launch_bounds__(256)
up8_labels_wide_tile_kernel(const float* __restrict__ logits, const float* __restrict__ up_w, void* __restrict__ labels,
                            int c, int cs, int h, int w, unsigned long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float vec[];     // [(TI + 1) * (TJ + 1)][VS]
  __shared__ float wk[256];
  __shared__ float wstat[1];
  __shared__ float smarg[kTileMaxPx], sabsb[kTileMaxPx];
  __shared__ int sam[kTileMaxPx];                    // argmax | 0x100 when every class is finite
  __shared__ int nslow;
  __shared__ unsigned short slist[128];              // window | 0x8000 when it builds candidates
  __shared__ unsigned char clist[16][kWideMaxClasses];
  __shared__ unsigned int scount[3];
  int TI, TJ, VS;
  wide_tile_shape(c, TI, TJ, VS);
  const int PJ = TJ + 1, NPX = (TI + 1) * PJ, C4 = (c + 3) >> 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  wk[tid] = up_w[tid];
  if (tid == 0) nslow = 0;
  if (tid < 3) scount[tid] = 0;
  __syncthreads();
  if (wave == 0) {                                   // min over the 64 phases of sum w (0 if any w < 0)
    const int ky1 = lane >> 3, kx1 = lane & 7;
    const float a = wk[(ky1 + 8) * 16 + kx1 + 8], b = wk[(ky1 + 8) * 16 + kx1], cc = wk[ky1 * 16 + kx1 + 8],
                d = wk[ky1 * 16 + kx1];
    float lo = fminf(fminf(a, b), fminf(cc, d)) < 0.f ? 0.f : (a + b) + (cc + d);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o));
    if (lane == 0) wstat[0] = lo;
  }
  const int H = h * 8, W = w * 8;
  const int I0 = blockIdx.y * TI, J0 = blockIdx.x * TJ;
  const int n = blockIdx.z;
  const int64_t HW = static_cast<int64_t>(H) * W;
  const float* src = logits + static_cast<int64_t>(n) * h * w * cs;

  // ---- 1. the tile's 1/8-res pixels (tap rows I0 - 1 .. I0 + TI - 1, columns J0 - 1 .. J0 + TJ - 1)
#pragma unroll 4
  for (int e = tid; e < NPX * C4; e += 256) {
    const int px = e / C4, f = e - px * C4;
    int iy = I0 - 1 + px / PJ, ix = J0 - 1 + px % PJ;
    iy = (iy < 0 || iy >= h) ? 0 : iy;               // up8_lsm_wide_kernel's clamped read
    ix = (ix < 0 || ix >= w) ? 0 : ix;
    float4 v = *reinterpret_cast<const float4*>(src + (static_cast<int64_t>(iy) * w + ix) * cs + 4 * f);
    v.y = 4 * f + 1 < c ? v.y : 0.f;                 // the row's padding columns
    v.z = 4 * f + 2 < c ? v.z : 0.f;
    v.w = 4 * f + 3 < c ? v.w : 0.f;
    *reinterpret_cast<float4*>(vec + px * VS + 4 * f) = v;
  }
  __syncthreads();

  // ---- 2. the per-pixel summary: lane s of a quad takes the float4 groups s F .. (s + 1) F - 1
  const int F = (C4 + 3) >> 2;
  for (int e0 = 0; e0 < NPX * 4; e0 += 256) {
    const int px = (e0 + tid) >> 2, s = tid & 3;
    float best = -INFINITY, second = -INFINITY;
    int am = 0;
    bool fin = true;
    if (px < NPX) {
      const int f1 = min((s + 1) * F, C4);
      for (int f = s * F; f < f1; ++f) {
        const float4 v = *reinterpret_cast<const float4*>(vec + px * VS + 4 * f);
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 4 * f + j;
          if (k < c) {
            am = x[j] > best ? k : am;
            second = __builtin_amdgcn_fmed3f(best, second, x[j]);
            best = fmaxf(best, x[j]);
            fin = fin && fabsf(x[j]) < INFINITY;     // false for NaN too
          }
        }
      }
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {               // the quad's ranges in class order: first maximum wins
      const float ob = __shfl_xor(best, o), os = __shfl_xor(second, o);
      const int oa = __shfl_xor(am, o), of = __shfl_xor(static_cast<int>(fin), o);
      const bool upper = (tid & o) != 0;             // this lane holds the higher classes
      const float lo_b = upper ? ob : best, hi_b = upper ? best : ob;
      const int lo_a = upper ? oa : am, hi_a = upper ? am : oa;
      am = hi_b > lo_b ? hi_a : lo_a;
      second = fmaxf(fminf(best, ob), fmaxf(second, os));
      best = fmaxf(best, ob);
      fin = fin && of != 0;
    }
    if (px < NPX && s == 0) {
      smarg[px] = best - second;
      sabsb[px] = fabsf(best);
      sam[px] = am | (fin ? 0x100 : 0);
    }
  }
  __syncthreads();

  // ---- 3. one window per thread
  const float wmin = wstat[0];
  if (tid < TI * TJ) {
    const int ti = tid / TJ, tj = tid - ti * TJ;
    const int i1 = I0 + ti, j1 = J0 + tj;
    if (i1 <= h && j1 <= w) {
      bool fast = false, cand = false;
      int cls = 0;
      if (i1 >= 1 && i1 < h && j1 >= 1 && j1 < w) {
        const int p[4] = {ti * PJ + tj, ti * PJ + tj + 1, (ti + 1) * PJ + tj, (ti + 1) * PJ + tj + 1};
        cls = sam[p[0]] & 0xff;
        bool same = true, finite = true;
        float mmin = INFINITY, amax = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int a = sam[p[t]];
          same = same && (a & 0xff) == cls;
          finite = finite && (a & 0x100) != 0;
          mmin = fminf(mmin, smarg[p[t]]);
          amax = fmaxf(amax, sabsb[p[t]]);
        }
        fast = same && wmin > 0.f && finite && mmin >= 0x1p-16f / wmin * (1.f + 0x1p-10f) + 0x1p-20f * amax;
        cand = !fast && finite && wmin > 0.f;
      }
      if (fast) {
        const int la[4] = {cls, cls, cls, cls};
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int64_t row = static_cast<int64_t>(n) * HW + static_cast<int64_t>(8 * i1 - 4 + r) * W;
          store_wide_labels4<LABEL_DTYPE>(labels, row + 8 * j1 - 4, la);
          store_wide_labels4<LABEL_DTYPE>(labels, row + 8 * j1, la);
        }
        if (STATS) atomicAdd(&scount[0], 1u);
      } else {
        const int at = atomicAdd(&nslow, 1);
        slist[at] = static_cast<unsigned short>(tid | (cand ? 0x8000 : 0));
      }
    }
  }
  __syncthreads();

  // ---- 4. the slow windows, one per 16 lanes per round (every thread runs every round: barriers)
  const int ns = nslow;
  const int g = tid >> 4, l = tid & 15, gsh = 16 * (g & 3);
  for (int e0 = 0; e0 < ns; e0 += 16) {
    const bool act = e0 + g < ns;
    const int wt = act ? slist[e0 + g] : 0;
    const bool cand = (wt & 0x8000) != 0;
    const int ti = (wt & 0x7fff) / TJ, tj = (wt & 0x7fff) - ti * TJ;
    const int i1 = I0 + ti, j1 = J0 + tj;
    const float* t00 = vec + (ti * PJ + tj) * VS;    // taps (i0, j0), (i0, j1), (i1, j0), (i1, j1)
    const float* t01 = t00 + VS;
    const float* t10 = t00 + PJ * VS;
    const float* t11 = t10 + VS;
    // the candidate list: lane l takes the classes l, l + 16, ..
    float lmax = -INFINITY, vabs = 0.f;
    if (cand)
      for (int k = l; k < c; k += 16) {
        const float a0 = t00[k], a1 = t01[k], a2 = t10[k], a3 = t11[k];
        vabs = fmaxf(vabs, fmaxf(fmaxf(fabsf(a0), fabsf(a1)), fmaxf(fabsf(a2), fabsf(a3))));
        lmax = fmaxf(lmax, fminf(fminf(a0, a1), fminf(a2, a3)));
      }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      lmax = fmaxf(lmax, __shfl_xor(lmax, o));
      vabs = fmaxf(vabs, __shfl_xor(vabs, o));
    }
    const float thr = lmax - (0x1p-16f / wmin * (1.f + 0x1p-10f) + 0x1p-20f * vabs);
    int cnt = 0;
    for (int k0 = 0; k0 < c; k0 += 16) {
      const int k = k0 + l;
      bool keep = false;
      if (cand && k < c) keep = fmaxf(fmaxf(t00[k], t01[k]), fmaxf(t10[k], t11[k])) >= thr;
      const unsigned int bits = static_cast<unsigned int>(__ballot(keep) >> gsh) & 0xffffu;
      if (keep) clist[g][cnt + __popc(bits & ((1u << l) - 1u))] = static_cast<unsigned char>(k);
      cnt += __popc(bits);
    }
    __syncthreads();
    const int r = l & 7, hh = l >> 3;
    const int q = 2 * j1 - 1 + hh;                   // output columns 4 q .. 4 q + 3
    const int oy = 8 * i1 - 4 + r;
    if (act && q >= 0 && 4 * q < W && oy >= 0 && oy < H) {
      const bool vi0 = i1 - 1 >= 0, vi1 = i1 < h, vj0 = j1 - 1 >= 0, vj1 = j1 < w;
      const int ky1 = r, ky0 = r + 8;
      float w00[4], w01[4], w10[4], w11[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int kx1 = 4 * hh + p, kx0 = kx1 + 8;   // 4 q + p + 4 - 8 j1
        w00[p] = (vi0 && vj0) ? wk[ky0 * 16 + kx0] : 0.f;
        w01[p] = (vi0 && vj1) ? wk[ky0 * 16 + kx1] : 0.f;
        w10[p] = (vi1 && vj0) ? wk[ky1 * 16 + kx0] : 0.f;
        w11[p] = (vi1 && vj1) ? wk[ky1 * 16 + kx1] : 0.f;
      }
      int arg[4] = {0, 0, 0, 0};
      bool decided = false;
      if (cand) {
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        float second[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < cnt; ++i) {
          const int k = clist[g][i];
          const float s00 = t00[k], s01 = t01[k], s10 = t10[k], s11 = t11[k];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            float v = s00 * w00[p];
            v = fmaf(s01, w01[p], v);
            v = fmaf(s10, w10[p], v);
            v = fmaf(s11, w11[p], v);
            arg[p] = v > best[p] ? k : arg[p];
            second[p] = __builtin_amdgcn_fmed3f(best[p], second[p], v);
            best[p] = fmaxf(best[p], v);
          }
        }
        decided = true;
#pragma unroll
        for (int p = 0; p < 4; ++p) decided = decided && !(best[p] - second[p] < 0x1p-16f);
      }
      if (!decided) lsm_sweeps4<1>(t00, t01, t10, t11, w00, w01, w10, w11, c, nullptr, 0, arg);
      store_wide_labels4<LABEL_DTYPE>(labels, static_cast<int64_t>(n) * HW + static_cast<int64_t>(oy) * W + 4 * q, arg);
      if (STATS) atomicAdd(&scount[decided ? 1 : 2], 4u);
    }
    __syncthreads();
  }
  if (STATS) {
    if (tid < 3 && scount[tid] != 0) atomicAdd(&stats[tid], static_cast<unsigned long long>(scount[tid]));
  }
}

template <int LABEL_DTYPE, bool STATS>
int launch_labels_wide_tile(const float* logits, int cs, const float* up_w, void* labels, int n, int c, int h, int w,
                            int64_t* stats, hipStream_t s) {
  int ti, tj, vs;
  wide_tile_shape(c, ti, tj, vs);
  const size_t lds = static_cast<size_t>((ti + 1) * (tj + 1)) * vs * sizeof(float);
  const dim3 grid(static_cast<unsigned>((w + tj) / tj), static_cast<unsigned>((h + ti) / ti), static_cast<unsigned>(n));
  hipLaunchKernelGGL((up8_labels_wide_tile_kernel<LABEL_DTYPE, STATS>), grid, dim3(256), lds, s, logits, up_w, labels, c,
                     cs, h, w, reinterpret_cast<unsigned long long*>(stats));
  return static_cast<int>(hipGetLastError());
}

template <bool STATS>
int labels_wide_tile_dispatch(const float* logits, int cs, const float* up_w, void* labels, int label_dtype, int n,
                              int c, int h, int w, int64_t* stats, hipStream_t s) {
  if (logits == nullptr || up_w == nullptr || labels == nullptr || (STATS && stats == nullptr)) return DRNMI_EINVAL;
  if (n <= 0 || h <= 0 || w <= 0) return DRNMI_EINVAL;
  if (c <= 0 || c > kWideMaxClasses) return DRNMI_ENOTSUP;
  if (label_dtype != DRNMI_U8 && label_dtype != DRNMI_I64) return DRNMI_EINVAL;
  if (cs < c || cs % 4 != 0 || (reinterpret_cast<uintptr_t>(logits) & 15) != 0) return DRNMI_EINVAL;
  if ((reinterpret_cast<uintptr_t>(labels) & (label_dtype == DRNMI_I64 ? 7 : 3)) != 0) return DRNMI_EINVAL;
  if (STATS && (reinterpret_cast<uintptr_t>(stats) & 7) != 0) return DRNMI_EINVAL;
  if (h > 65535 || w > (1 << 27) || n > 65535) return DRNMI_EINVAL;   // grid.y, grid.z; 8 w in an int
  if (label_dtype == DRNMI_I64)
    return launch_labels_wide_tile<DRNMI_I64, STATS>(logits, cs, up_w, labels, n, c, h, w, stats, s);
  return launch_labels_wide_tile<DRNMI_U8, STATS>(logits, cs, up_w, labels, n, c, h, w, stats, s);
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
  int64_t g = (npix + 8 * kHistWideThreads - 1) / (8 * kHistWideThreads);
  g = g > kHistWideGrid ? kHistWideGrid : g;
  const hipError_t e = allow_lds<&confusion_wide_kernel<TP, TL>>(kHistWideBytes);   // the largest a launch asks for
  if (e != hipSuccess) return static_cast<int>(e);
  return static_cast<int>(launch_lds<&confusion_wide_kernel<TP, TL>>(
      dim3(static_cast<unsigned>(g), static_cast<unsigned>(slabs)), dim3(kHistWideThreads), lds, s,
      static_cast<const TP*>(pred), static_cast<const TL*>(label), npix, n, rows, hist));
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

extern "C" int drnmi_up8_labels_nhwc_wide(const float* logits, int32_t cs, const float* up_w, void* labels,
                                          int32_t label_dtype, int32_t n, int32_t c, int32_t h, int32_t w,
                                          void* stream) {
  return labels_wide_tile_dispatch<false>(logits, cs, up_w, labels, label_dtype, n, c, h, w, nullptr,
                                          reinterpret_cast<hipStream_t>(stream));
}

extern "C" int drnmi_up8_labels_nhwc_wide_stats(const float* logits, int32_t cs, const float* up_w, void* labels,
                                                int32_t label_dtype, int32_t n, int32_t c, int32_t h, int32_t w,
                                                void* stream, int64_t* stats) {
  return labels_wide_tile_dispatch<true>(logits, cs, up_w, labels, label_dtype, n, c, h, w, stats,
                                         reinterpret_cast<hipStream_t>(stream));
}
