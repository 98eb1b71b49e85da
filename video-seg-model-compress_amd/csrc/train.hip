// Fine-tune (train-mode) kernels: the backward half of the DRN-D hot path, fp32.
//
// The reference fine-tunes DRNSeg with train-mode BatchNorm, CrossEntropyLoss on the
// log-probs, SGD(momentum, weight_decay) and Pruner.apply_masks after every step
// (semantic_seg.py:166-230, :817, :963-966; pruners/Pruner.py:17-20).  The convs' forward
// and data-gradient (dgrad) passes reuse the implicit-GEMM conv of conv_igemm.hip (dgrad =
// a stride-1 conv of dy with transposed/flipped weights, after a zero-insert for stride-s
// layers) and the conv weight gradient is wgrad.hip; this file holds everything else:
//
//   pack_conv_weight   OIHW fp32 -> packed [rows_pad][k_pad] (forward or dgrad layout)
//   bn stats / apply   train-mode BatchNorm2d: batch mean / biased var, running-stat update
//                      (momentum, unbiased var), y -> relu(bn(y) [+ res])
//   bn backward        relu mask, dgamma / dbeta, dy, residual-branch gradient
//   channel_sum        per-channel column sums (conv bias gradient)
//   split3_bf16        fp32 -> three bf16 planes: the weight side of the fp32x forward pass
//   zero_insert        dy of a stride-s conv spread onto the input grid (dgrad input)
//   up8_lsm_bwd        LogSoftmax backward + transpose of the fixed bilinear up-conv
//   ce_loss            CrossEntropyLoss(ignore_index) forward / backward on log-probs
//   distill_loss       that CE plus the KL divergence to a teacher's log-probs at a temperature
//                      (knowledge distillation), forward / backward in one pass each
//   sgd_step           torch.optim.SGD step (momentum, dampening, wd, nesterov) with the
//                      pruner mask (bit-packed) applied in the same pass
//
// Every reduction accumulates in fp64 in a fixed order (no atomics), so results are
// bit-reproducible run to run.
#include <cmath>

#include "common.h"

namespace drnmi {
namespace {

constexpr int kThreads = 256;

inline bool aligned16(const void* a, const void* b, const void* c) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

// ------------------------------------------------------------------ weight packing
// mode 0 (forward): out[co][ (kh*ks + kw) * kin_stride + ci ] = w[co][ci][kh][kw] * scale[co]
// mode 1 (dgrad):   out[ci][ (kh'*ks + kw') * kin_stride + co ] = w[co][ci][ks-1-kh'][ks-1-kw']
// Everything else in [rows_pad][k_pad] is zero.
template <typename TO>
__global__ void __launch_bounds__(kThreads)
pack_weight_kernel(const float* __restrict__ w, int cout, int cin, int ks, int kin_stride, int rows_pad,
                   int k_pad, int mode, const float* __restrict__ scale, TO* __restrict__ out) {
  const int64_t total = static_cast<int64_t>(rows_pad) * k_pad;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int row = static_cast<int>(i / k_pad);
    const int k = static_cast<int>(i - static_cast<int64_t>(row) * k_pad);
    const int tap = k / kin_stride;
    const int c = k - tap * kin_stride;
    float v = 0.f;
    if (tap < ks * ks) {
      const int kh = tap / ks, kw = tap - (tap / ks) * ks;
      if (mode == 0) {
        if (row < cout && c < cin) {
          v = w[((static_cast<int64_t>(row) * cin + c) * ks + kh) * ks + kw];
          if (scale != nullptr) v *= scale[row];
        }
      } else {
        // row = ci (dgrad output channel), c = co (dgrad input channel)
        if (row < cin && c < cout)
          v = w[((static_cast<int64_t>(c) * cin + row) * ks + (ks - 1 - kh)) * ks + (ks - 1 - kw)];
      }
    }
    if constexpr (sizeof(TO) == 2) out[i] = f32_to_bf16(v);
    else out[i] = v;
  }
}

// All entries of the table in one launch, as LDS-staged transposes.  An element per thread with the
// OIHW source gathered per element ran at ~1 TB/s (0.61 ms of the fp32x fine-tune step): the dgrad
// layout reads w[co][ci] at stride cin * ks * ks per consecutive output.  Here a tile is 32 output
// rows x CT channel columns x all ks * ks taps.  Its source is CT (dgrad) or 32 (forward) runs of
// contiguous floats -- w[co][ci0 .. ci0 + n)[taps] -- read coalesced into LDS.  The tile is then
// written tap by tap, four consecutive k per thread: 16-B fp32 stores, 8-B stores per bf16 plane.
// 37 KB of LDS per workgroup keeps four workgroups (16 waves) per CU on this memory-bound pass.
// Pure data movement plus split3_kernel's arithmetic: bit-identical to the per-layer calls.
constexpr int kPackRows = 32;
constexpr int kPackMaxEntries = 512;
constexpr int kPackLds = kPackRows * (32 * 9 + 1);        // 3x3 taps x 32 columns, run stride + 1
// columns per tile (a multiple of 4): 32 up to 3x3, 4 up to 7x7 (4 x 49 <= 32 x 9)
__device__ __forceinline__ int pack_cols(int taps) { return taps <= 9 ? 32 : 4; }

__global__ void __launch_bounds__(kThreads)
pack_batched_kernel(const int64_t* __restrict__ tab, int n) {
  __shared__ int first[kPackMaxEntries + 1];              // first tile of each entry (prefix sum)
  __shared__ float L[kPackLds];
  const int t = threadIdx.x;
  for (int e = t; e < n; e += kThreads) {
    const int64_t* q = tab + static_cast<int64_t>(e) * DRNMI_PACK_ENTRY_WORDS;
    const int taps = static_cast<int>(q[5] * q[5]);
    first[e + 1] = static_cast<int>(((q[7] + kPackRows - 1) / kPackRows) * ((q[6] + pack_cols(taps) - 1) / pack_cols(taps)));
  }
  __syncthreads();
  if (t == 0) {
    first[0] = 0;
    for (int e = 0; e < n; ++e) first[e + 1] += first[e];
  }
  __syncthreads();
  const int tiles = first[n];
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int lo = 0, hi = n - 1;                                  // entry: last e with first[e] <= tile
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (first[mid] <= tile) lo = mid;
      else hi = mid - 1;
    }
    const int64_t* q = tab + static_cast<int64_t>(lo) * DRNMI_PACK_ENTRY_WORDS;
    const float* __restrict__ w = reinterpret_cast<const float*>(q[0]);
    float* __restrict__ out = reinterpret_cast<float*>(q[1]);
    bf16_t* __restrict__ pl = reinterpret_cast<bf16_t*>(q[2]);
    const int cout = static_cast<int>(q[3]), cin = static_cast<int>(q[4]), ks = static_cast<int>(q[5]);
    const int kst = static_cast<int>(q[6]), rows_pad = static_cast<int>(q[7]), k_pad = static_cast<int>(q[8]);
    const int mode = static_cast<int>(q[9]);
    const int64_t m = static_cast<int64_t>(rows_pad) * k_pad;
    const int T = ks * ks;
    const int CT = pack_cols(T);
    const int ntc = (kst + CT - 1) / CT;
    const int local = tile - first[lo];
    const int row0 = (local / ntc) * kPackRows;
    const int col0 = (local % ntc) * CT;
    // runs: forward: run r = output row co = row0 + r, its elements ci = col0 + c (c < CT);
    //       dgrad:   run r = column co = col0 + r, its elements ci = row0 + c (c < 32)
    const int nrun = mode == 0 ? kPackRows : CT;
    const int nel = mode == 0 ? CT : kPackRows;
    const int run_co0 = mode == 0 ? row0 : col0;
    const int ci0 = mode == 0 ? col0 : row0;
    const int rlen = nel * T;
    const int rstr = rlen + 1;
    const int nci = cin - ci0 < nel ? cin - ci0 : nel;       // valid elements of a run: nci * T floats
    __syncthreads();                                         // the previous tile's reads of L
    for (int idx = t; idx < nrun * rlen; idx += kThreads) {
      const int r = idx / rlen;
      const int j = idx - r * rlen;
      const int co = run_co0 + r;
      float v = 0.f;
      if (co < cout && j < nci * T) v = w[(static_cast<int64_t>(co) * cin + ci0) * T + j];
      L[r * rstr + j] = v;
    }
    __syncthreads();
    // thread: 4 consecutive columns c4 .. c4 + 3 of (row r, tap); kst % 4 == 0 (table check)
    const int cq = CT / 4;
    for (int idx = t; idx < kPackRows * T * cq; idx += kThreads) {
      const int c4 = (idx % cq) * 4;
      const int rt = idx / cq;
      const int tap = rt % T;
      const int r = rt / T;
      const int row = row0 + r, col = col0 + c4;
      if (row >= rows_pad || col >= kst) continue;
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)   // forward: run r, ci c, tap; dgrad: run c, ci r, flipped tap
        v[u] = mode == 0 ? L[r * rstr + (c4 + u) * T + tap] : L[(c4 + u) * rstr + r * T + (T - 1 - tap)];
      const int64_t o = static_cast<int64_t>(row) * k_pad + tap * kst + col;
      *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
      if (pl != nullptr) {                                   // split3_kernel's arithmetic
        uint16_t h1[4], h2[4], h3[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bf16_t a = f32_to_bf16(v[u]);
          const float rr = v[u] - bf16_to_f32(a);
          const bf16_t b = f32_to_bf16(rr);
          h1[u] = a;
          h2[u] = b;
          h3[u] = f32_to_bf16(rr - bf16_to_f32(b));
        }
        *reinterpret_cast<uint2*>(pl + o) = make_uint2(h1[0] | (uint32_t(h1[1]) << 16), h1[2] | (uint32_t(h1[3]) << 16));
        *reinterpret_cast<uint2*>(pl + m + o) = make_uint2(h2[0] | (uint32_t(h2[1]) << 16), h2[2] | (uint32_t(h2[3]) << 16));
        *reinterpret_cast<uint2*>(pl + 2 * m + o) = make_uint2(h3[0] | (uint32_t(h3[1]) << 16), h3[2] | (uint32_t(h3[3]) << 16));
      }
    }
    // the k tail past the last tap (k_pad > ks * ks * kst) is zero; column tile 0 writes it
    const int tail = k_pad - T * kst;
    if (col0 == 0 && tail > 0) {
      for (int idx = t; idx < kPackRows * tail; idx += kThreads) {
        const int r = idx / tail;
        const int row = row0 + r;
        if (row >= rows_pad) continue;
        const int64_t o = static_cast<int64_t>(row) * k_pad + T * kst + (idx - r * tail);
        out[o] = 0.f;
        if (pl != nullptr) {
          pl[o] = 0;
          pl[m + o] = 0;
          pl[2 * m + o] = 0;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ column reductions
// Rows x C (C = row stride, a power of two >= 4), fp32 in, fp64 partial sums.
// Block: TPR threads per row (4 channels each, float4), RG = 256 / TPR row groups.
// grid = (G splits, C / (4 * TPR) channel chunks).  Partials ws[2][G][C] (S1, S2).
enum { RED_STATS = 0, RED_BNBWD = 1, RED_SUM = 2 };


struct RedArgs {
  const float* a;       // STATS: y ; BNBWD: dz ; SUM: x
  const float* z;       // BNBWD: z (relu mask), or NULL: the mask is bn_value(y) > 0 (below)
  const float* y;       // BNBWD: y (pre-BN conv output)
  int64_t rows;
  int C;
  int G;
  int64_t rows_per_split;
  int relu;
  double* ws;
  const float* mean;    // BNBWD with z == NULL: the forward's BN terms (gamma / beta NULL-able)
  const float* invstd;
  const float* gamma;
  const float* beta;
};

// The train-mode BN output before ReLU, one rounding order everywhere it is formed: bn_act_kernel
// writes relu(bn_value) and the backward of a residual-free BN + ReLU recomputes the mask
// bn_value(y) > 0 from y instead of reading z (one fp32 tensor less per pass, bit-identical mask).
__device__ __forceinline__ float bn_value(float v, float m, float s, float g, float b) {
  return __builtin_fmaf((v - m) * s, g, b);
}
__device__ __forceinline__ float4 ld4_or(const float* p, int c, float dflt) {
  return p != nullptr ? *reinterpret_cast<const float4*>(p + c) : make_float4(dflt, dflt, dflt, dflt);
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) colred_kernel(const RedArgs r) {
  const int tpr = (r.C / 4) < 64 ? (r.C / 4) : 64;
  const int rg = kThreads / tpr;
  const int t = threadIdx.x;
  const int tc = t % tpr;
  const int tr = t / tpr;
  const int c0 = blockIdx.y * 4 * tpr + 4 * tc;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * r.rows_per_split;
  const int64_t r1 = (r0 + r.rows_per_split) < r.rows ? (r0 + r.rows_per_split) : r.rows;
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  // BNBWD without z: the thread's four channels' forward BN terms (mask = bn_value(y) > 0)
  float bm[4] = {0, 0, 0, 0}, bs[4] = {0, 0, 0, 0}, bg[4] = {1, 1, 1, 1}, bb[4] = {0, 0, 0, 0};
  const bool ymask = MODE == RED_BNBWD && r.relu && r.z == nullptr;
  if (ymask) {
    const float4 m4 = ld4_or(r.mean, c0, 0.f), s4 = ld4_or(r.invstd, c0, 0.f);
    const float4 g4 = ld4_or(r.gamma, c0, 1.f), b4 = ld4_or(r.beta, c0, 0.f);
    bm[0] = m4.x; bm[1] = m4.y; bm[2] = m4.z; bm[3] = m4.w;
    bs[0] = s4.x; bs[1] = s4.y; bs[2] = s4.z; bs[3] = s4.w;
    bg[0] = g4.x; bg[1] = g4.y; bg[2] = g4.z; bg[3] = g4.w;
    bb[0] = b4.x; bb[1] = b4.y; bb[2] = b4.z; bb[3] = b4.w;
  }
  // RB rows' loads go out before their (in-order) fp64 accumulation: the same sums, with that many
  // loads in flight per thread instead of one
  constexpr int RB = 4;
  int64_t row = r0 + tr;
  for (; row + (RB - 1) * rg < r1; row += RB * rg) {
    float4 av[RB], zv[RB], yv[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int64_t off = (row + u * rg) * r.C + c0;
      av[u] = *reinterpret_cast<const float4*>(r.a + off);
      if constexpr (MODE == RED_BNBWD) {
        if (r.relu && !ymask) zv[u] = *reinterpret_cast<const float4*>(r.z + off);
        yv[u] = *reinterpret_cast<const float4*>(r.y + off);
      }
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      float a[4] = {av[u].x, av[u].y, av[u].z, av[u].w};
      if constexpr (MODE == RED_STATS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s1[j] += a[j];
          s2[j] += static_cast<double>(a[j]) * a[j];
        }
      } else if constexpr (MODE == RED_BNBWD) {
        const float y[4] = {yv[u].x, yv[u].y, yv[u].z, yv[u].w};
        if (ymask) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = bn_value(y[j], bm[j], bs[j], bg[j], bb[j]) > 0.f ? a[j] : 0.f;
        } else if (r.relu) {
          a[0] = zv[u].x > 0.f ? a[0] : 0.f;
          a[1] = zv[u].y > 0.f ? a[1] : 0.f;
          a[2] = zv[u].z > 0.f ? a[2] : 0.f;
          a[3] = zv[u].w > 0.f ? a[3] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s1[j] += a[j];
          s2[j] += static_cast<double>(a[j]) * y[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) s1[j] += a[j];
      }
    }
  }
  for (; row < r1; row += rg) {
    const int64_t off = row * r.C + c0;
    const float4 av = *reinterpret_cast<const float4*>(r.a + off);
    float a[4] = {av.x, av.y, av.z, av.w};
    if constexpr (MODE == RED_STATS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s1[j] += a[j];
        s2[j] += static_cast<double>(a[j]) * a[j];
      }
    } else if constexpr (MODE == RED_BNBWD) {
      const float4 yv = *reinterpret_cast<const float4*>(r.y + off);
      const float y[4] = {yv.x, yv.y, yv.z, yv.w};
      if (ymask) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = bn_value(y[j], bm[j], bs[j], bg[j], bb[j]) > 0.f ? a[j] : 0.f;
      } else if (r.relu) {
        const float4 zv = *reinterpret_cast<const float4*>(r.z + off);
        a[0] = zv.x > 0.f ? a[0] : 0.f;
        a[1] = zv.y > 0.f ? a[1] : 0.f;
        a[2] = zv.z > 0.f ? a[2] : 0.f;
        a[3] = zv.w > 0.f ? a[3] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s1[j] += a[j];
        s2[j] += static_cast<double>(a[j]) * y[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) s1[j] += a[j];
    }
  }
  __shared__ double sh1[kThreads * 4], sh2[kThreads * 4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sh1[t * 4 + j] = s1[j];
    sh2[t * 4 + j] = s2[j];
  }
  __syncthreads();
  // thread q < 4*tpr sums channel q of the block over the rg row groups, in order
  if (t < 4 * tpr) {
    const int q_tc = t / 4, q_j = t % 4;
    double a1 = 0, a2 = 0;
    for (int g = 0; g < rg; ++g) {
      a1 += sh1[(g * tpr + q_tc) * 4 + q_j];
      a2 += sh2[(g * tpr + q_tc) * 4 + q_j];
    }
    const int c = blockIdx.y * 4 * tpr + t;
    r.ws[static_cast<int64_t>(blockIdx.x) * r.C + c] = a1;
    r.ws[static_cast<int64_t>(r.G + blockIdx.x) * r.C + c] = a2;
  }
}

int red_splits(int64_t rows, int C) {
  const int tpr = (C / 4) < 64 ? (C / 4) : 64;
  const int chunks = C / (4 * tpr);
  const int rg = kThreads / tpr;
  int64_t g = 1024 / chunks;
  const int64_t by_rows = (rows + 16 * rg - 1) / (16 * rg);   // >= 16 rows per thread
  if (g > by_rows) g = by_rows;
  return static_cast<int>(g < 1 ? 1 : g);
}

template <int MODE>
hipError_t launch_colred(RedArgs& r, hipStream_t s) {
  const int tpr = (r.C / 4) < 64 ? (r.C / 4) : 64;
  r.G = red_splits(r.rows, r.C);
  r.rows_per_split = (r.rows + r.G - 1) / r.G;
  hipLaunchKernelGGL(colred_kernel<MODE>, dim3(r.G, r.C / (4 * tpr)), dim3(kThreads), 0, s, r);
  return hipGetLastError();
}

// finalize.  The G split partials of a channel were summed by one thread in split order: up to
// 1024 dependent fp64 adds per channel on a handful of waves (120 us per BN layer in the
// fine-tune profile, profiles/r2e_finetune_kernel_stats.csv).  Here a block owns 16 channels
// (a 128-B row of partials per split, coalesced) and 16 threads per channel sum 16 contiguous
// runs of splits, which are then added run by run: a fixed order, so the statistics stay
// deterministic.
constexpr int kFinCh = 16;
__device__ __forceinline__ bool split_sums(const double* __restrict__ ws, int G, int C, int& c, double& s1,
                                           double& s2) {
  __shared__ double p1[kThreads], p2[kThreads];
  const int t = threadIdx.x, tc = t % kFinCh, tg = t / kFinCh;
  constexpr int NG = kThreads / kFinCh;
  c = blockIdx.x * kFinCh + tc;
  const int gs = (G + NG - 1) / NG;
  const int g0 = tg * gs, g1 = g0 + gs < G ? g0 + gs : G;
  double a1 = 0, a2 = 0;
  if (c < C) {
#pragma unroll 8
    for (int g = g0; g < g1; ++g) {
      a1 += ws[static_cast<int64_t>(g) * C + c];
      a2 += ws[static_cast<int64_t>(G + g) * C + c];
    }
  }
  p1[t] = a1;
  p2[t] = a2;
  __syncthreads();
  if (t >= kFinCh || c >= C) return false;
  s1 = 0;
  s2 = 0;
  for (int j = 0; j < NG; ++j) {
    s1 += p1[j * kFinCh + tc];
    s2 += p2[j * kFinCh + tc];
  }
  return true;
}
inline unsigned fin_grid(int C) { return static_cast<unsigned>((C + kFinCh - 1) / kFinCh); }

__global__ void __launch_bounds__(kThreads)
bn_stats_final_kernel(const double* __restrict__ ws, int G, int C, int64_t rows, float eps, float momentum,
                      float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ rmean,
                      float* __restrict__ rvar, int64_t* __restrict__ nbt) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && nbt != nullptr) nbt[0] += 1;
  int c;
  double s1, s2;
  if (!split_sums(ws, G, C, c, s1, s2)) return;
  const double m = s1 / static_cast<double>(rows);
  double var = s2 / static_cast<double>(rows) - m * m;
  if (var < 0) var = 0;
  const float mf = static_cast<float>(m);
  const float vf = static_cast<float>(var);
  mean[c] = mf;
  invstd[c] = 1.f / sqrtf(vf + eps);
  if (rmean != nullptr) {
    const float unb = rows > 1 ? static_cast<float>(var * static_cast<double>(rows) / static_cast<double>(rows - 1)) : vf;
    rmean[c] = momentum * mf + (1.f - momentum) * rmean[c];
    rvar[c] = momentum * unb + (1.f - momentum) * rvar[c];
  }
}

// The per-element BN passes walk [rows][C] as float4 lanes with a grid whose total thread count x 4
// is a multiple of C (bn_ew_grid): a thread's channel group never changes along its grid-stride
// loop, so its per-channel terms are loaded once instead of with every float4 (four or five extra
// 16-B loads per 16 B of data held them at ~4.5 TB/s), and each thread keeps ~8 float4s in flight.
inline unsigned bn_ew_grid(int64_t n4, int C) {
  int64_t g = (n4 + kThreads * 8 - 1) / (kThreads * 8);
  const int64_t q = C > 4 * kThreads ? C / (4 * kThreads) : 1;   // g * 4 * kThreads % C == 0
  g = (g + q - 1) / q * q;
  return static_cast<unsigned>(g < q ? q : g);
}

// z = relu?(((y - mean) * invstd) * gamma + beta [+ res]) over [rows][C], float4 lanes
__global__ void __launch_bounds__(kThreads)
bn_act_kernel(const float* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ invstd,
              const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ res,
              int relu, int64_t n4, int C, float* __restrict__ z) {
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i0 >= n4) return;
  // per-channel terms as 16-B loads (c % 4 == 0), once: c is the same for every i of the thread
  const int c = static_cast<int>((i0 * 4) & (C - 1));
  const float4 m4 = *reinterpret_cast<const float4*>(mean + c);
  const float4 s4 = *reinterpret_cast<const float4*>(invstd + c);
  const float4 g4 = ld4_or(gamma, c, 1.f), b4 = ld4_or(beta, c, 0.f);
  const float cm[4] = {m4.x, m4.y, m4.z, m4.w}, cs[4] = {s4.x, s4.y, s4.z, s4.w};
  const float cg[4] = {g4.x, g4.y, g4.z, g4.w}, cb[4] = {b4.x, b4.y, b4.z, b4.w};
  for (int64_t i = i0; i < n4; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(y)[i];
    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = bn_value(o[j], cm[j], cs[j], cg[j], cb[j]);
    if (res != nullptr) {
      const float4 rv = reinterpret_cast<const float4*>(res)[i];
      o[0] += rv.x; o[1] += rv.y; o[2] += rv.z; o[3] += rv.w;
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
    }
    reinterpret_cast<float4*>(z)[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// BN backward finalize: dbeta = S1, dgamma = invstd * (S2 - mean * S1) with S2 = sum(dr * y);
// coefficients for dy = a * (dr - b - (y - mean) * d):
//   a = gamma * invstd, b = S1 / rows, d = invstd^2 * (S2 - mean * S1) / rows
__global__ void __launch_bounds__(kThreads)
bn_bwd_final_kernel(const double* __restrict__ ws, int G, int C, int64_t rows, const float* __restrict__ mean,
                    const float* __restrict__ invstd, const float* __restrict__ gamma, float* __restrict__ dgamma,
                    float* __restrict__ dbeta, int accumulate, float* __restrict__ coef) {
  int c;
  double s1, s2;
  if (!split_sums(ws, G, C, c, s1, s2)) return;
  const double is = invstd[c];
  const double sx = s2 - static_cast<double>(mean[c]) * s1;   // sum(dr * (y - mean))
  const float dg = static_cast<float>(is * sx);
  const float db = static_cast<float>(s1);
  if (dgamma != nullptr) dgamma[c] = accumulate ? dgamma[c] + dg : dg;
  if (dbeta != nullptr) dbeta[c] = accumulate ? dbeta[c] + db : db;
  const double g = gamma != nullptr ? gamma[c] : 1.0;
  coef[c] = static_cast<float>(g * is);
  coef[C + c] = static_cast<float>(s1 / static_cast<double>(rows));
  coef[2 * C + c] = static_cast<float>(is * is * sx / static_cast<double>(rows));
}

__global__ void __launch_bounds__(kThreads)
bn_bwd_apply_kernel(const float* dz, const float* __restrict__ z, const float* __restrict__ y,
                    const float* __restrict__ mean, const float* __restrict__ coef, int relu, int64_t n4, int C,
                    float* dy, float* dres, int dres_acc, const float* __restrict__ invstd,
                    const float* __restrict__ gamma, const float* __restrict__ beta) {
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i0 >= n4) return;
  // per-channel terms once (bn_ew_grid: c is the same for every i of the thread); coef's three
  // rows are C floats each
  const int c = static_cast<int>((i0 * 4) & (C - 1));
  const bool ymask = relu && z == nullptr;             // mask recomputed: bn_value(y) > 0
  const float4 m4 = *reinterpret_cast<const float4*>(mean + c);
  const float4 s4 = ymask ? *reinterpret_cast<const float4*>(invstd + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 g4 = ld4_or(ymask ? gamma : nullptr, c, 1.f), bb4 = ld4_or(ymask ? beta : nullptr, c, 0.f);
  const float4 a4 = *reinterpret_cast<const float4*>(coef + c);
  const float4 b4 = *reinterpret_cast<const float4*>(coef + C + c);
  const float4 d4 = *reinterpret_cast<const float4*>(coef + 2 * C + c);
  const float cm[4] = {m4.x, m4.y, m4.z, m4.w}, cs[4] = {s4.x, s4.y, s4.z, s4.w};
  const float cg[4] = {g4.x, g4.y, g4.z, g4.w}, cbb[4] = {bb4.x, bb4.y, bb4.z, bb4.w};
  const float ca[4] = {a4.x, a4.y, a4.z, a4.w}, cb[4] = {b4.x, b4.y, b4.z, b4.w};
  const float cd[4] = {d4.x, d4.y, d4.z, d4.w};
  for (int64_t i = i0; i < n4; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float4 gv = reinterpret_cast<const float4*>(dz)[i];
    float dr[4] = {gv.x, gv.y, gv.z, gv.w};
    const float4 yv = reinterpret_cast<const float4*>(y)[i];
    const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
    if (ymask) {
#pragma unroll
      for (int j = 0; j < 4; ++j) dr[j] = bn_value(yy[j], cm[j], cs[j], cg[j], cbb[j]) > 0.f ? dr[j] : 0.f;
    } else if (relu) {
      const float4 zv = reinterpret_cast<const float4*>(z)[i];
      dr[0] = zv.x > 0.f ? dr[0] : 0.f;
      dr[1] = zv.y > 0.f ? dr[1] : 0.f;
      dr[2] = zv.z > 0.f ? dr[2] : 0.f;
      dr[3] = zv.w > 0.f ? dr[3] : 0.f;
    }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ca[j] * (dr[j] - cb[j] - (yy[j] - cm[j]) * cd[j]);
    if (dres != nullptr) {
      float4 rv = make_float4(dr[0], dr[1], dr[2], dr[3]);
      if (dres_acc) {
        const float4 old = reinterpret_cast<const float4*>(dres)[i];
        rv.x += old.x; rv.y += old.y; rv.z += old.z; rv.w += old.w;
      }
      reinterpret_cast<float4*>(dres)[i] = rv;
    }
    reinterpret_cast<float4*>(dy)[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

__global__ void __launch_bounds__(kThreads)
colsum_final_kernel(const double* __restrict__ ws, int G, int C, int cvalid, float* __restrict__ out, int acc) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cvalid) return;
  double s = 0;
  for (int g = 0; g < G; ++g) s += ws[static_cast<int64_t>(g) * C + c];
  out[c] = acc ? out[c] + static_cast<float>(s) : static_cast<float>(s);
}

// ------------------------------------------------------------------ stride-2 dgrad parity classes
// The data gradient of a stride-2 conv is a stride-1 conv of dy zero-inserted to the input grid
// (zero_insert_kernel below) with the flipped weights: 3/4 of its B rows are zeros.  Split by the
// parity (a, b) of the output pixel, each class is a dense stride-1 conv of dy itself with the
// flipped taps kh' = (pad_d - a) mod 2, + 2, ... (kw' likewise), embedded in a KSC x KSC kernel
// (zero weights where a class has fewer taps in one dimension), written to every other pixel of
// every other row (drnmi_conv_args.y_sr).  Products with the zero rows were exact zeros: the four
// class launches are bit-identical to the zero-inserted conv.  This gathers one class's weight
// planes from the packed dgrad planes ([3][rows][k_pad], k = tap' * kst + co).
__global__ void __launch_bounds__(kThreads)
dgrad_class_planes_kernel(const uint4* __restrict__ in, int rows, int k_pad, int kst, int ks, int kh0, int nh, int kw0,
                          int nw, int ksc, uint4* __restrict__ out, int k_pad_c) {
  const int c8 = kst / 8;
  const int64_t per_plane = static_cast<int64_t>(rows) * ksc * ksc * c8;
  const int64_t total = 3 * per_plane;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int pl = static_cast<int>(i / per_plane);
    int64_t j = i - pl * per_plane;
    const int c = static_cast<int>(j % c8);
    j /= c8;
    const int tc = static_cast<int>(j % (ksc * ksc));
    const int r = static_cast<int>(j / (ksc * ksc));
    const int khc = tc / ksc, kwc = tc - (tc / ksc) * ksc;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (khc < nh && kwc < nw) {
      const int tap = (kh0 + 2 * khc) * ks + (kw0 + 2 * kwc);
      v = in[((static_cast<int64_t>(pl) * rows + r) * k_pad + tap * kst) / 8 + c];
    }
    out[((static_cast<int64_t>(pl) * rows + r) * k_pad_c + tc * kst) / 8 + c] = v;
  }
}

// ------------------------------------------------------------------ zero insert (stride-s dgrad)
__global__ void __launch_bounds__(kThreads)
zero_insert_kernel(const float* __restrict__ dy, int n, int ho, int wo, int c4, int s, int hu, int wu,
                   float* __restrict__ out) {
  const int64_t total = static_cast<int64_t>(n) * hu * wu * c4;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int cv = static_cast<int>(i % c4);
    const int64_t pix = i / c4;
    const int x = static_cast<int>(pix % wu);
    const int y = static_cast<int>((pix / wu) % hu);
    const int b = static_cast<int>(pix / (static_cast<int64_t>(wu) * hu));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y % s == 0 && x % s == 0 && y / s < ho && x / s < wo)
      v = reinterpret_cast<const float4*>(dy)[((static_cast<int64_t>(b) * ho + y / s) * wo + x / s) * c4 + cv];
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

// ------------------------------------------------------------------ head backward
// du[n][c][p] = scale * (g[n][c][p] - exp(lp[n][c][p]) * sum_c' g[n][c'][p])  (LogSoftmax bwd).
// NC > 0: the class count at compile time (19, the seg head), the pixel's values held in registers
// (one read of g instead of two); NC = 0: any c.  Same operations in the same order either way.
template <int NC>
__global__ void __launch_bounds__(kThreads)
lsm_bwd_kernel(const float* __restrict__ g, const float* __restrict__ lp, int nimg, int c, int64_t hw, float scale,
               float* __restrict__ du) {
  const int64_t total = static_cast<int64_t>(nimg) * hw;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t b = i / hw, p = i - b * hw;
    const int64_t base = b * c * hw + p;
    if constexpr (NC > 0) {
      float gv[NC], lv[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        gv[k] = g[base + k * hw];
        lv[k] = lp[base + k * hw];
      }
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k) s += gv[k];
#pragma unroll
      for (int k = 0; k < NC; ++k) du[base + k * hw] = scale * (gv[k] - expf(lv[k]) * s);
    } else {
      float s = 0.f;
      for (int k = 0; k < c; ++k) s += g[base + k * hw];
      for (int k = 0; k < c; ++k) {
        const int64_t o = base + k * hw;
        du[o] = scale * (g[o] - expf(lp[o]) * s);
      }
    }
  }
}

// dlogits[n][c][i][j] = sum_{ky,kx} W[ky][kx] * du[n][c][8i-4+ky][8j-4+kx] (+ gscale * g_logits); the
// transpose of ConvTranspose2d(k16, s8, p4) (lmodels/drnseg.py:285-293).  du == NULL: logits-only
// gradient (no log-prob term).  A workgroup owns UBI x UBJ outputs of one plane and stages the
// (8 UBI + 8) x (8 UBJ + 8) du window they read into LDS once (each du value is read by four
// outputs' 16 x 16 windows); every output then sums its 256 products in the same ky-major order,
// skipping the same out-of-image taps: the same result bits as the per-output global gather.
constexpr int kUbI = 4, kUbJ = 32, kUbThreads = kUbI * kUbJ;   // outputs per workgroup, one per thread
constexpr int kUbRows = 8 * kUbI + 8, kUbCols = 8 * kUbJ + 8;
static_assert(kUbCols % 8 == 0, "16-B staging pieces stay inside one skew group");
// column c of a tile row at c + c / 8: output windows start 8 columns apart, so a wave's 32 lanes
// of one row read 9 apart -- distinct banks
constexpr int kUbPitch = kUbCols + kUbCols / 8 + 1;
__global__ void __launch_bounds__(kUbThreads)
up8_bwd_kernel(const float* __restrict__ du, const float* __restrict__ upw, const float* __restrict__ glog,
               float gscale, int nc, int h, int w, float* __restrict__ dlog) {
  __shared__ float wk[256];
  __shared__ float tile[kUbRows * kUbPitch];
  for (int e = threadIdx.x; e < 256; e += kUbThreads) wk[e] = upw[e];
  const int H = 8 * h, W = 8 * w;
  const int64_t plane = blockIdx.z;
  const int i0 = blockIdx.y * kUbI, j0 = blockIdx.x * kUbJ;
  const int y0 = 8 * i0 - 4, x0 = 8 * j0 - 4;        // du window origin
  if (du != nullptr) {
    // 16-B pieces (W = 8 w and x0 = 8 j0 - 4 are multiples of 4: a piece is wholly inside or outside
    // the image), all of a thread's pieces in flight before their LDS writes
    const float* src = du + plane * H * W;
    constexpr int kP4 = kUbCols / 4, kN4 = kUbRows * kP4;
    constexpr int kB = (kN4 + kUbThreads - 1) / kUbThreads;
    float4 v[kB];
#pragma unroll
    for (int u = 0; u < kB; ++u) {
      const int e = threadIdx.x + u * kUbThreads;
      const int r = e / kP4, x = x0 + 4 * (e - r * kP4), y = y0 + r;
      v[u] = (e < kN4 && static_cast<unsigned>(y) < static_cast<unsigned>(H) &&
              static_cast<unsigned>(x) < static_cast<unsigned>(W))
                 ? *reinterpret_cast<const float4*>(src + static_cast<int64_t>(y) * W + x)
                 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kB; ++u) {
      const int e = threadIdx.x + u * kUbThreads;
      if (e < kN4) {
        const int r = e / kP4, cc = 4 * (e - r * kP4);
        float* t = tile + r * kUbPitch + cc + (cc >> 3);   // the 4 columns share one 8-group
        t[0] = v[u].x;
        t[1] = v[u].y;
        t[2] = v[u].z;
        t[3] = v[u].w;
      }
    }
  }
  __syncthreads();
  const int ii = i0 + threadIdx.x / kUbJ, j = j0 + threadIdx.x % kUbJ;
  if (ii >= h || j >= w) return;
  const float* t0 = tile + 8 * (threadIdx.x / kUbJ) * kUbPitch + 9 * (threadIdx.x % kUbJ);   // (8 ti, 8 tj)
  float s = 0.f;
  for (int ky = 0; ky < 16 && du != nullptr; ++ky) {
    const int y = 8 * ii - 4 + ky;
    if (static_cast<unsigned>(y) >= static_cast<unsigned>(H)) continue;
    const float* row = t0 + ky * kUbPitch;
#pragma unroll
    for (int kx = 0; kx < 16; ++kx) {
      const int x = 8 * j - 4 + kx;
      if (static_cast<unsigned>(x) < static_cast<unsigned>(W)) s += wk[ky * 16 + kx] * row[kx + (kx >> 3)];
    }
  }
  const int64_t i = (plane * h + ii) * w + j;
  if (glog != nullptr) s += gscale * glog[i];   // the logits output's gradient, DDP-averaged like du
  dlog[i] = s;
}

// Transpose of nn.UpsamplingBilinear2d(scale_factor=8) (align_corners=True, lmodels/drnseg.py:
// 285-287): dlogits[i][j] = sum_{oy,ox} wy(oy, i) * wx(ox, j) * du[oy][ox] (+ gscale * g_logits),
// gathered (no atomics, fixed order).  Output row oy touches input rows i0(oy) and i1(oy) with
// i0 non-decreasing in oy, so input row i gathers from the oy window whose i0 is i-1 or i; the
// window is found with the forward's own index arithmetic.
__device__ __forceinline__ void bil_ac(int dst, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  const float scale = out > 1 ? static_cast<float>(in - 1) / static_cast<float>(out - 1) : 0.f;
  const float src = scale * static_cast<float>(dst);
  i0 = static_cast<int>(floorf(src));
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - static_cast<float>(i0), 0.f), 1.f);
  l0 = 1.f - l1;
}

__device__ __forceinline__ float bil_weight(int o, int i, int in, int out) {
  int i0, i1;
  float l0, l1;
  bil_ac(o, in, out, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

__global__ void __launch_bounds__(kThreads)
up8_bilinear_bwd_kernel(const float* __restrict__ du, const float* __restrict__ glog, float gscale, int nc, int h,
                        int w, float* __restrict__ dlog) {
  const int H = 8 * h, W = 8 * w;
  const int64_t total = static_cast<int64_t>(nc) * h * w;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int j = static_cast<int>(i % w);
    const int ii = static_cast<int>((i / w) % h);
    const int64_t plane = i / (static_cast<int64_t>(w) * h);
    float s = 0.f;
    if (du != nullptr) {
      const float* src = du + plane * H * W;
      // candidate windows: o with i0(o) in {i-1, i}, i.e. o*(in-1)/(out-1) in [i-1, i+1), +-2 for
      // rounding; bil_weight() then applies the forward's exact index test
      const float ry = h > 1 ? static_cast<float>(H - 1) / static_cast<float>(h - 1) : static_cast<float>(H);
      const float rx = w > 1 ? static_cast<float>(W - 1) / static_cast<float>(w - 1) : static_cast<float>(W);
      const int oy_lo = max(0, static_cast<int>(floorf((ii - 1) * ry)) - 2);
      const int oy_hi = min(H - 1, static_cast<int>(ceilf((ii + 1) * ry)) + 2);
      const int ox_lo = max(0, static_cast<int>(floorf((j - 1) * rx)) - 2);
      const int ox_hi = min(W - 1, static_cast<int>(ceilf((j + 1) * rx)) + 2);
      for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        const float wy = bil_weight(oy, ii, h, H);
        if (wy == 0.f) continue;
        const float* row = src + static_cast<int64_t>(oy) * W;
        float r = 0.f;
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
          const float wx = bil_weight(ox, j, w, W);
          if (wx != 0.f) r += wx * row[ox];
        }
        s += wy * r;
      }
    }
    if (glog != nullptr) s += gscale * glog[i];
    dlog[i] = s;
  }
}

// ------------------------------------------------------------------ cross entropy
// per pixel: lse(lp) - lp[t] over t != ignore (CrossEntropyLoss applied to log-probs,
// semantic_seg.py:817 + :197-198); block partials (sum, count) in fp64, fixed order.
constexpr int kCeBlocks = 512;

// one pixel's lse(lp) - lp[t]: NC > 0 holds the NC values in registers (one read instead of three),
// NC = 0 walks any c; same operations in the same order
template <int NC>
__device__ __forceinline__ float ce_pixel(const float* v, int c, int64_t hw, int64_t t) {
  if constexpr (NC > 0) {
    float x[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) x[k] = v[k * hw];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < NC; ++k) mx = fmaxf(mx, x[k]);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) se += expf(x[k] - mx);
    const float lse = mx + logf(se);
    float xt = x[0];
#pragma unroll
    for (int k = 1; k < NC; ++k) xt = k == t ? x[k] : xt;
    return lse - xt;
  } else {
    float mx = -INFINITY;
    for (int k = 0; k < c; ++k) mx = fmaxf(mx, v[k * hw]);
    float se = 0.f;
    for (int k = 0; k < c; ++k) se += expf(v[k * hw] - mx);
    const float lse = mx + logf(se);
    return lse - v[t * hw];
  }
}

template <int NC>
__global__ void __launch_bounds__(kThreads)
ce_fwd_kernel(const float* __restrict__ lp, const int64_t* __restrict__ tgt, int nimg, int c, int64_t hw,
              int64_t ignore, double* __restrict__ ws) {
  const int64_t total = static_cast<int64_t>(nimg) * hw;
  double s = 0, cnt = 0, bad = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t t = tgt[i];
    if (t == ignore) continue;
    if (t < 0 || t >= c) { bad += 1; continue; }
    const int64_t b = i / hw, p = i - b * hw;
    s += static_cast<double>(ce_pixel<NC>(lp + b * c * hw + p, c, hw, t));
    cnt += 1;
  }
  __shared__ double sh[3][kThreads];
  sh[0][threadIdx.x] = s;
  sh[1][threadIdx.x] = cnt;
  sh[2][threadIdx.x] = bad;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
      sh[2][threadIdx.x] += sh[2][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ws[blockIdx.x] = sh[0][0];
    ws[kCeBlocks + blockIdx.x] = sh[1][0];
    ws[2 * kCeBlocks + blockIdx.x] = sh[2][0];
  }
}

// the block partials summed in block order by one thread, from LDS (the 64 threads stage them:
// one dependent fp64 add per partial instead of a global load each)
__global__ void __launch_bounds__(64) ce_final_kernel(const double* __restrict__ ws, int blocks, float* __restrict__ loss,
                                                      float* __restrict__ count) {
  __shared__ double sh[3 * kCeBlocks];
  for (int e = threadIdx.x; e < 3 * kCeBlocks; e += 64) sh[e] = ws[e];
  __syncthreads();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0, cnt = 0, bad = 0;
  for (int b = 0; b < blocks; ++b) {
    s += sh[b];
    cnt += sh[kCeBlocks + b];
    bad += sh[2 * kCeBlocks + b];
  }
  // an out-of-range target is an error in the reference (device assert); surface it as NaN
  loss[0] = bad > 0 ? __builtin_nanf("") : static_cast<float>(s / cnt);
  count[0] = static_cast<float>(cnt);
}

// four consecutive pixels per thread as 16-B pieces (NC > 0, hw % 4 == 0); per-pixel arithmetic
// as ce_bwd_kernel
template <int NC>
__global__ void __launch_bounds__(kThreads)
ce_bwd_v4_kernel(const float* __restrict__ lp, const int64_t* __restrict__ tgt, int nimg, int c, int64_t hw,
                 int64_t ignore, const float* __restrict__ dloss, const float* __restrict__ count,
                 float* __restrict__ glp) {
  const float sc = dloss[0] / count[0];
  const int64_t total4 = static_cast<int64_t>(nimg) * hw / 4;
  const int64_t hw4 = hw / 4;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total4;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t b = i / hw4, p4 = i - b * hw4;
    const int64_t base4 = b * c * hw4 + p4;
    const float4* v4 = reinterpret_cast<const float4*>(lp) + base4;
    float x[4][NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const float4 a = v4[k * hw4];
      x[0][k] = a.x;
      x[1][k] = a.y;
      x[2][k] = a.z;
      x[3][k] = a.w;
    }
    float lse[4];
    int64_t tt[4];
    bool live[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tt[e] = tgt[4 * i + e];
      live[e] = !(tt[e] == ignore || tt[e] < 0 || tt[e] >= c);
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < NC; ++k) mx = fmaxf(mx, x[e][k]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k) se += expf(x[e][k] - mx);
      lse[e] = mx + logf(se);
    }
    float4* o4 = reinterpret_cast<float4*>(glp) + base4;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = live[e] ? sc * (expf(x[e][k] - lse[e]) - (k == tt[e] ? 1.f : 0.f)) : 0.f;
      o4[k * hw4] = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int NC>
__global__ void __launch_bounds__(kThreads)
ce_bwd_kernel(const float* __restrict__ lp, const int64_t* __restrict__ tgt, int nimg, int c, int64_t hw,
              int64_t ignore, const float* __restrict__ dloss, const float* __restrict__ count,
              float* __restrict__ glp) {
  const float sc = dloss[0] / count[0];
  const int64_t total = static_cast<int64_t>(nimg) * hw;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t t = tgt[i];
    const int64_t b = i / hw, p = i - b * hw;
    const float* v = lp + b * c * hw + p;
    float* o = glp + b * c * hw + p;
    if (t == ignore || t < 0 || t >= c) {
      for (int k = 0; k < c; ++k) o[k * hw] = 0.f;
      continue;
    }
    if constexpr (NC > 0) {
      float x[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) x[k] = v[k * hw];
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < NC; ++k) mx = fmaxf(mx, x[k]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k) se += expf(x[k] - mx);
      const float lse = mx + logf(se);
#pragma unroll
      for (int k = 0; k < NC; ++k) o[k * hw] = sc * (expf(x[k] - lse) - (k == t ? 1.f : 0.f));
    } else {
      float mx = -INFINITY;
      for (int k = 0; k < c; ++k) mx = fmaxf(mx, v[k * hw]);
      float se = 0.f;
      for (int k = 0; k < c; ++k) se += expf(v[k * hw] - mx);
      const float lse = mx + logf(se);
      for (int k = 0; k < c; ++k) o[k * hw] = sc * (expf(v[k * hw] - lse) - (k == t ? 1.f : 0.f));
    }
  }
}

// ------------------------------------------------------------------ distillation (CE + KL to a teacher)
// The reference's --mc-kd loss (rmbsnn_main.py:192-243) for the segmentation loop, on student and
// teacher log-probs s, t [n][c][hw]: per pixel, with a = s / T and b = t / T,
//   kd = sum_k q[k] * (logq[k] - logp[k]),  logp = a - lse(a), logq = b - lse(b), q = exp(logq)
// over every pixel, and ce_pixel's lse(s) - s[target] over the labelled ones; one pass over both
// tensors.  No T^2 factor (the reference has none).

// one pixel's class values: NC > 0 held in registers (each plane read once), NC = 0 read from the
// planes at every use (any c)
template <int NC>
struct KdRow {
  float x[NC > 0 ? NC : 1];
  const float* v;
  int64_t hw;
  __device__ __forceinline__ float operator[](int k) const {
    if constexpr (NC > 0) return x[k];
    else return v[k * hw];
  }
};

// lse of r[k] * invT.  The student's and the teacher's rows both go through this function and kd_logp,
// with nothing contracted, so bit-equal rows give bit-equal log-probabilities (kd == 0, p - q == 0).
// invT = 1 is ce_pixel's lse: the same operations in the same order.
template <int NC>
__device__ __forceinline__ float kd_lse(const KdRow<NC>& r, int c, float invT) {
#pragma clang fp contract(off)
  const int nc = NC > 0 ? NC : c;
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < nc; ++k) mx = fmaxf(mx, r[k] * invT);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < nc; ++k) se += expf(r[k] * invT - mx);
  return mx + logf(se);
}

template <int NC>
__device__ __forceinline__ float kd_logp(const KdRow<NC>& r, int k, float invT, float lse) {
#pragma clang fp contract(off)
  return r[k] * invT - lse;
}

// r[t], 0 <= t < c, without indexing the registers (ce_pixel's selection).  The row by value: through a
// reference the compiler turns the selects into an indexed load and the row moves to scratch memory
template <int NC>
__device__ __forceinline__ float kd_pick(const KdRow<NC> r, int64_t t) {
  if constexpr (NC > 0) {
    float xt = r.x[0];
#pragma unroll
    for (int k = 1; k < NC; ++k) xt = k == t ? r.x[k] : xt;
    return xt;
  } else {
    return r.v[t * r.hw];
  }
}

// PX consecutive pixels of image b from pixel p on: PX = 4 as one 16-B piece per plane (NC > 0, hw % 4 == 0)
template <int NC, int PX>
__device__ __forceinline__ void kd_load(const float* __restrict__ v, int64_t hw, KdRow<NC> (&r)[PX]) {
  static_assert(PX == 1 || (PX == 4 && NC > 0), "the 16-B form holds its classes in registers");
  if constexpr (PX == 4) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const float4 a = *reinterpret_cast<const float4*>(v + k * hw);
      r[0].x[k] = a.x;
      r[1].x[k] = a.y;
      r[2].x[k] = a.z;
      r[3].x[k] = a.w;
    }
  } else if constexpr (NC > 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) r[0].x[k] = v[k * hw];
  } else {
    r[0].v = v;
    r[0].hw = hw;
  }
}

// block partials (ce sum, count, bad targets, kd sum) in fp64, fixed order; PX pixels per thread,
// consecutive lanes on consecutive pixels (PX = 4: consecutive 16-B pieces) of a plane.  Two waves per
// SIMD (the 16-B form holds 152 class values per lane): one wave's loads run under the other's expf
template <int NC, int PX>
__global__ void __launch_bounds__(kThreads, 2)
distill_fwd_kernel(const float* __restrict__ slp, const float* __restrict__ tlp, const int64_t* __restrict__ tgt,
                   int nimg, int c, int64_t hw, int64_t ignore, float invT, double* __restrict__ ws) {
  const int nc = NC > 0 ? NC : c;
  const int64_t hwq = hw / PX;
  const int64_t total = static_cast<int64_t>(nimg) * hwq;
  double sce = 0, cnt = 0, bad = 0, skd = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t b = i / hwq, p = (i - b * hwq) * PX;
    KdRow<NC> s[PX], t[PX];
    kd_load<NC, PX>(slp + b * c * hw + p, hw, s);
    kd_load<NC, PX>(tlp + b * c * hw + p, hw, t);
#pragma unroll
    for (int e = 0; e < PX; ++e) {
      const float la = kd_lse(s[e], c, invT), lb = kd_lse(t[e], c, invT);
      float kd = 0.f;
#pragma unroll
      for (int k = 0; k < nc; ++k) {
        const float lq = kd_logp(t[e], k, invT, lb);
        kd += expf(lq) * (lq - kd_logp(s[e], k, invT, la));
      }
      skd += static_cast<double>(kd);
      const int64_t tg = tgt[b * hw + p + e];
      if (tg == ignore) continue;
      if (tg < 0 || tg >= c) { bad += 1; continue; }
      sce += static_cast<double>(kd_lse(s[e], c, 1.f) - kd_pick(s[e], tg));
      cnt += 1;
    }
  }
  __shared__ double sh[4][kThreads];
  sh[0][threadIdx.x] = sce;
  sh[1][threadIdx.x] = cnt;
  sh[2][threadIdx.x] = bad;
  sh[3][threadIdx.x] = skd;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sh[j][threadIdx.x] += sh[j][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) ws[threadIdx.x * kCeBlocks + blockIdx.x] = sh[threadIdx.x][0];
}

// the block partials summed in block order by one thread, as ce_final_kernel; out3 = loss, ce, kd
__global__ void __launch_bounds__(64)
distill_final_kernel(const double* __restrict__ ws, int blocks, double kd_div, float student_wt, float distill_wt,
                     float* __restrict__ out3, float* __restrict__ count) {
  __shared__ double sh[4 * kCeBlocks];
  for (int e = threadIdx.x; e < 4 * kCeBlocks; e += 64) sh[e] = ws[e];
  __syncthreads();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0, cnt = 0, bad = 0, skd = 0;
  for (int b = 0; b < blocks; ++b) {
    s += sh[b];
    cnt += sh[kCeBlocks + b];
    bad += sh[2 * kCeBlocks + b];
    skd += sh[3 * kCeBlocks + b];
  }
  const float ce = bad > 0 ? __builtin_nanf("") : static_cast<float>(s / cnt);
  const float kd = static_cast<float>(skd / kd_div);
  out3[0] = student_wt * ce + distill_wt * kd;
  out3[1] = ce;
  out3[2] = kd;
  count[0] = static_cast<float>(cnt);
}

// g_s[k] = dloss * (student_wt / count * (softmax(s)[k] - onehot[k]) on labelled pixels
//                   + kd_scale * (p[k] - q[k])),  kd_scale = distill_wt / (D * T);
// the CE term is ce_bwd_kernel's arithmetic, the teacher gets no gradient
template <int NC, int PX>
__global__ void __launch_bounds__(kThreads, 2)
distill_bwd_kernel(const float* __restrict__ slp, const float* __restrict__ tlp, const int64_t* __restrict__ tgt,
                   int nimg, int c, int64_t hw, int64_t ignore, float invT, float student_wt, float kd_scale,
                   const float* __restrict__ dloss, const float* __restrict__ count, float* __restrict__ gs) {
  const int nc = NC > 0 ? NC : c;
  const float sc_ce = dloss[0] * student_wt / count[0];
  const float sc_kd = dloss[0] * kd_scale;
  const int64_t hwq = hw / PX;
  const int64_t total = static_cast<int64_t>(nimg) * hwq;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t b = i / hwq, p = (i - b * hwq) * PX;
    KdRow<NC> s[PX], t[PX];
    kd_load<NC, PX>(slp + b * c * hw + p, hw, s);
    kd_load<NC, PX>(tlp + b * c * hw + p, hw, t);
    float ls[PX], la[PX], lb[PX];
    int64_t tg[PX];
    bool live[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
      tg[e] = tgt[b * hw + p + e];
      live[e] = !(tg[e] == ignore || tg[e] < 0 || tg[e] >= c);
      ls[e] = kd_lse(s[e], c, 1.f);
      la[e] = kd_lse(s[e], c, invT);
      lb[e] = kd_lse(t[e], c, invT);
    }
    float* o = gs + b * c * hw + p;
#pragma unroll
    for (int k = 0; k < nc; ++k) {
      float g[PX];
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        const float ce = live[e] ? sc_ce * (expf(s[e][k] - ls[e]) - (k == tg[e] ? 1.f : 0.f)) : 0.f;
        g[e] = ce + sc_kd * (expf(kd_logp(s[e], k, invT, la[e])) - expf(kd_logp(t[e], k, invT, lb[e])));
      }
      if constexpr (PX == 4) *reinterpret_cast<float4*>(o + k * hw) = make_float4(g[0], g[1], g[2], g[3]);
      else o[k * hw] = g[0];
    }
  }
}

// ------------------------------------------------------------------ SGD (+ mask)
constexpr int kSgdBatch = 48;
struct SgdBatch {
  float* w[kSgdBatch];
  const float* g[kSgdBatch];
  float* buf[kSgdBatch];
  const uint32_t* mask[kSgdBatch];
  int64_t numel[kSgdBatch];
  int first[kSgdBatch];
};

// torch.optim.SGD (dampening d, nesterov off/on): d_p = g + wd * w;
// buf = first ? d_p : m * buf + (1 - d) * d_p;  d_p = nesterov ? d_p + m * buf : buf;
// w = w - lr * d_p; then w *= mask (Pruner.apply_masks fused, pruners/Pruner.py:17-20).
__global__ void __launch_bounds__(kThreads)
sgd_kernel(const SgdBatch b, float lr, float mom, float damp, float wd, int nesterov) {
  const int t = blockIdx.y;
  float* __restrict__ w = b.w[t];
  const float* __restrict__ g = b.g[t];
  float* __restrict__ buf = b.buf[t];
  const uint32_t* __restrict__ mk = b.mask[t];
  const int64_t n = b.numel[t];
  const int first = b.first[t];
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float d = g[i];
    const float wv = w[i];
    if (wd != 0.f) d = d + wd * wv;
    if (mom != 0.f) {
      float bv;
      if (first) bv = d;
      else bv = mom * buf[i] + (1.f - damp) * d;
      buf[i] = bv;
      d = nesterov ? d + mom * bv : bv;
    }
    float nw = wv - lr * d;
    if (mk != nullptr) nw *= static_cast<float>((mk[i >> 5] >> (i & 31)) & 1u);
    w[i] = nw;
  }
}

}  // namespace
}  // namespace drnmi

using namespace drnmi;

// ================================================================== C-ABI
extern "C" int drnmi_pack_conv_weight(const float* w, int32_t cout, int32_t cin, int32_t ks, int32_t kin_stride,
                                      int32_t rows_pad, int32_t k_pad, int32_t mode, const float* row_scale,
                                      int32_t out_dtype, void* out, void* stream) {
  if (w == nullptr || out == nullptr || cout <= 0 || cin <= 0 || ks <= 0 || kin_stride <= 0 || k_pad <= 0)
    return DRNMI_EINVAL;
  if (mode != 0 && mode != 1) return DRNMI_EINVAL;
  if (k_pad < ks * ks * kin_stride) return DRNMI_EINVAL;
  if (mode == 0 && (rows_pad < cout || kin_stride < cin)) return DRNMI_EINVAL;
  if (mode == 1 && (rows_pad < cin || kin_stride < cout || row_scale != nullptr)) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = static_cast<int64_t>(rows_pad) * k_pad;
  if (out_dtype == DRNMI_F32)
    hipLaunchKernelGGL(pack_weight_kernel<float>, dim3(grid_of(total)), dim3(kThreads), 0, s, w, cout, cin, ks,
                       kin_stride, rows_pad, k_pad, mode, row_scale, reinterpret_cast<float*>(out));
  else if (out_dtype == DRNMI_BF16)
    hipLaunchKernelGGL(pack_weight_kernel<bf16_t>, dim3(grid_of(total)), dim3(kThreads), 0, s, w, cout, cin, ks,
                       kin_stride, rows_pad, k_pad, mode, row_scale, reinterpret_cast<bf16_t*>(out));
  else
    return DRNMI_EINVAL;
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_pack_table_check(const int64_t* t, int32_t n, int64_t* total_out) {
  if (t == nullptr || n <= 0 || n > kPackMaxEntries) return DRNMI_EINVAL;
  int64_t total = 0;
  for (int e = 0; e < n; ++e) {
    const int64_t* q = t + static_cast<int64_t>(e) * DRNMI_PACK_ENTRY_WORDS;
    const int64_t cout = q[3], cin = q[4], ks = q[5], kst = q[6], rows = q[7], kp = q[8], mode = q[9];
    if (q[0] == 0 || q[1] == 0 || cout <= 0 || cin <= 0 || ks <= 0 || ks > 7 || kst <= 0 || rows <= 0 || kp <= 0)
      return DRNMI_EINVAL;
    if ((mode != 0 && mode != 1) || kp < ks * ks * kst || kp >= (int64_t(1) << 31) || rows >= (int64_t(1) << 31)) return DRNMI_EINVAL;
    if (kst % 4 != 0 || kp % 4 != 0 || ((q[1] | q[2]) & 15) != 0) return DRNMI_EINVAL;   // 4-column stores
    if (mode == 0 && (rows < cout || kst < cin)) return DRNMI_EINVAL;
    if (mode == 1 && (rows < cin || kst < cout)) return DRNMI_EINVAL;
    if (q[10] != total || q[11] != 0) return DRNMI_EINVAL;
    total += rows * kp;
  }
  if (total_out != nullptr) *total_out = total;
  return 0;
}

extern "C" int drnmi_pack_conv_weights_batched(const int64_t* table, int32_t n, int64_t total, void* stream) {
  if (table == nullptr || n <= 0 || n > kPackMaxEntries || total <= 0) return DRNMI_EINVAL;
  // grid-stride over the tiles (their count is known on the device only): 8 workgroups per CU
  hipLaunchKernelGGL(pack_batched_kernel, dim3(2048), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), table, n);
  return static_cast<int>(hipGetLastError());
}

static bool pow2_ge4(int c) { return c >= 4 && (c & (c - 1)) == 0; }

extern "C" int64_t drnmi_reduce_workspace_bytes(int64_t rows, int32_t channels) {
  if (rows <= 0 || !pow2_ge4(channels)) return -1;
  // partials (2 x G x C doubles) + 3 x C float coefficients
  return static_cast<int64_t>(2) * red_splits(rows, channels) * channels * 8 + 3LL * channels * 4 + 256;
}

extern "C" int drnmi_bn_stats_f32(const float* y, int64_t rows, int32_t C, float eps, float momentum,
                                  float* mean, float* invstd, float* running_mean, float* running_var,
                                  int64_t* num_batches_tracked, void* ws, void* stream) {
  if (y == nullptr || mean == nullptr || invstd == nullptr || ws == nullptr || rows <= 0 || !pow2_ge4(C))
    return DRNMI_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RedArgs r{};
  r.a = y;
  r.rows = rows;
  r.C = C;
  r.ws = reinterpret_cast<double*>(ws);
  hipError_t e = launch_colred<RED_STATS>(r, s);
  if (e != hipSuccess) return static_cast<int>(e);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(fin_grid(C)), dim3(kThreads), 0, s, r.ws, r.G, C, rows, eps,
                     momentum, mean, invstd, running_mean, running_var, num_batches_tracked);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_dgrad_s2_class_planes(const void* planes, int32_t rows, int32_t k_pad, int32_t kst, int32_t ks,
                                           int32_t pad_d, int32_t a, int32_t b, int32_t ksc, void* out, int32_t k_pad_c,
                                           void* stream) {
  if (planes == nullptr || out == nullptr || rows <= 0 || ks <= 0 || ksc <= 0 || kst <= 0 || kst % 8 != 0 ||
      k_pad % 8 != 0 || k_pad < ks * ks * kst || k_pad_c != ksc * ksc * kst || (a != 0 && a != 1) || (b != 0 && b != 1) ||
      ((reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(out)) & 15))
    return DRNMI_EINVAL;
  const int kh0 = ((pad_d - a) % 2 + 2) % 2, kw0 = ((pad_d - b) % 2 + 2) % 2;
  const int nh = kh0 < ks ? (ks - kh0 + 1) / 2 : 0, nw = kw0 < ks ? (ks - kw0 + 1) / 2 : 0;
  if (nh > ksc || nw > ksc) return DRNMI_EINVAL;
  const int64_t total = 3LL * rows * ksc * ksc * (kst / 8);
  hipLaunchKernelGGL(dgrad_class_planes_kernel, dim3(grid_of(total)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint4*>(planes), rows, k_pad, kst,
                     ks, kh0, nh, kw0, nw, ksc, reinterpret_cast<uint4*>(out), k_pad_c);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_bn_stats_partials_f32(const double* partials, int64_t G, int64_t rows, int32_t C, float eps,
                                           float momentum, float* mean, float* invstd, float* running_mean,
                                           float* running_var, int64_t* num_batches_tracked, void* stream) {
  if (partials == nullptr || mean == nullptr || invstd == nullptr || G <= 0 || G >= (int64_t(1) << 31) || rows <= 0 ||
      !pow2_ge4(C))
    return DRNMI_EINVAL;
  if ((running_mean == nullptr) != (running_var == nullptr)) return DRNMI_EINVAL;
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(fin_grid(C)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     partials, static_cast<int>(G), C, rows, eps, momentum, mean, invstd, running_mean, running_var,
                     num_batches_tracked);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_bn_act_f32(const float* y, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, const float* res, int32_t relu, int64_t rows, int32_t C,
                                float* z, void* stream) {
  if (y == nullptr || mean == nullptr || invstd == nullptr || z == nullptr || rows <= 0 || !pow2_ge4(C))
    return DRNMI_EINVAL;
  // the per-channel vectors are read as 16-B pieces
  if ((reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(invstd) | reinterpret_cast<uintptr_t>(gamma) |
       reinterpret_cast<uintptr_t>(beta)) & 15)
    return DRNMI_EINVAL;
  const int64_t n4 = rows * C / 4;
  hipLaunchKernelGGL(bn_act_kernel, dim3(bn_ew_grid(n4, C)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     y, mean, invstd, gamma, beta, res, relu, n4, C, z);
  return static_cast<int>(hipGetLastError());
}

static int bn_bwd_launch(const float* dz, const float* z, const float* y, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, int32_t relu, int64_t rows, int32_t C, float* dy,
                         float* dres, int32_t dres_accumulate, float* dgamma, float* dbeta, int32_t grad_accumulate,
                         void* ws, void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RedArgs r{};
  r.a = dz;
  r.z = z;
  r.y = y;
  r.rows = rows;
  r.C = C;
  r.relu = relu;
  r.ws = reinterpret_cast<double*>(ws);
  r.mean = mean;
  r.invstd = invstd;
  r.gamma = gamma;
  r.beta = beta;
  hipError_t e = launch_colred<RED_BNBWD>(r, s);
  if (e != hipSuccess) return static_cast<int>(e);
  float* coef = reinterpret_cast<float*>(r.ws + static_cast<int64_t>(2) * r.G * C);
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(fin_grid(C)), dim3(kThreads), 0, s, r.ws, r.G, C, rows, mean, invstd,
                     gamma, dgamma, dbeta, grad_accumulate, coef);
  e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  const int64_t n4 = rows * C / 4;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(bn_ew_grid(n4, C)), dim3(kThreads), 0, s, dz, z, y, mean, coef, relu, n4,
                     C, dy, dres, dres_accumulate, invstd, gamma, beta);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_bn_act_bwd_f32(const float* dz, const float* z, const float* y, const float* mean,
                                    const float* invstd, const float* gamma, int32_t relu, int64_t rows, int32_t C,
                                    float* dy, float* dres, int32_t dres_accumulate, float* dgamma, float* dbeta,
                                    int32_t grad_accumulate, void* ws, void* stream) {
  if (dz == nullptr || y == nullptr || mean == nullptr || invstd == nullptr || dy == nullptr || ws == nullptr ||
      rows <= 0 || !pow2_ge4(C) || (relu && z == nullptr))
    return DRNMI_EINVAL;
  if (reinterpret_cast<uintptr_t>(mean) & 15) return DRNMI_EINVAL;   // read as 16-B pieces
  return bn_bwd_launch(dz, z, y, mean, invstd, gamma, nullptr, relu, rows, C, dy, dres, dres_accumulate, dgamma, dbeta,
                       grad_accumulate, ws, stream);
}

extern "C" int drnmi_bn_relu_bwd_y_f32(const float* dz, const float* y, const float* mean, const float* invstd,
                                       const float* gamma, const float* beta, int64_t rows, int32_t C, float* dy,
                                       float* dgamma, float* dbeta, int32_t grad_accumulate, void* ws, void* stream) {
  if (dz == nullptr || y == nullptr || mean == nullptr || invstd == nullptr || dy == nullptr || ws == nullptr ||
      rows <= 0 || !pow2_ge4(C))
    return DRNMI_EINVAL;
  if ((reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(invstd) | reinterpret_cast<uintptr_t>(gamma) |
       reinterpret_cast<uintptr_t>(beta)) & 15)
    return DRNMI_EINVAL;
  return bn_bwd_launch(dz, nullptr, y, mean, invstd, gamma, beta, 1, rows, C, dy, nullptr, 0, dgamma, dbeta,
                       grad_accumulate, ws, stream);
}

extern "C" int drnmi_channel_sum_f32(const float* x, int64_t rows, int32_t C, int32_t cvalid, float* out,
                                     int32_t accumulate, void* ws, void* stream) {
  if (x == nullptr || out == nullptr || ws == nullptr || rows <= 0 || !pow2_ge4(C) || cvalid <= 0 || cvalid > C)
    return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RedArgs r{};
  r.a = x;
  r.rows = rows;
  r.C = C;
  r.ws = reinterpret_cast<double*>(ws);
  hipError_t e = launch_colred<RED_SUM>(r, s);
  if (e != hipSuccess) return static_cast<int>(e);
  hipLaunchKernelGGL(colsum_final_kernel, dim3(grid_of(cvalid)), dim3(kThreads), 0, s, r.ws, r.G, C, cvalid, out,
                     accumulate);
  return static_cast<int>(hipGetLastError());
}

// fp32 [n] -> bf16 [3][n] planes, w = w1 + w2 + w3 (round to nearest even at each step): the weight
// side of the fp32x arithmetic in one pass (drnmi/engine.py split3_bf16 took six ATen launches per
// weight and step in the fp32x fine-tune)
__global__ void __launch_bounds__(kThreads)
split3_kernel(const float* __restrict__ w, int64_t n, bf16_t* __restrict__ out) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float x = w[i];
    const bf16_t a = f32_to_bf16(x);
    const float r = x - bf16_to_f32(a);
    const bf16_t b = f32_to_bf16(r);
    out[i] = a;
    out[n + i] = b;
    out[2 * n + i] = f32_to_bf16(r - bf16_to_f32(b));
  }
}

extern "C" int drnmi_split3_bf16(const float* w, int64_t n, void* out, void* stream) {
  if (w == nullptr || out == nullptr || n <= 0) return DRNMI_EINVAL;
  hipLaunchKernelGGL(split3_kernel, dim3(grid_of(n)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), w, n,
                     reinterpret_cast<bf16_t*>(out));
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_zero_insert_f32(const float* dy, int32_t n, int32_t ho, int32_t wo, int32_t c, int32_t stride,
                                     int32_t hu, int32_t wu, float* out, void* stream) {
  if (dy == nullptr || out == nullptr || n <= 0 || ho <= 0 || wo <= 0 || c <= 0 || c % 4 != 0 || stride <= 0 ||
      hu <= 0 || wu <= 0)
    return DRNMI_EINVAL;
  const int64_t total = static_cast<int64_t>(n) * hu * wu * (c / 4);
  hipLaunchKernelGGL(zero_insert_kernel, dim3(grid_of(total)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), dy, n, ho, wo, c / 4, stride, hu, wu, out);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_up8_lsm_bwd_f32(const float* g_logprobs, const float* logprobs, const float* g_logits,
                                     const float* up_w, float grad_scale, int32_t n, int32_t c, int32_t h, int32_t w,
                                     float* du_ws, float* dlogits, void* stream) {
  if (up_w == nullptr || dlogits == nullptr || n <= 0 || c <= 0 || h <= 0 || w <= 0) return DRNMI_EINVAL;
  if (g_logprobs != nullptr && (logprobs == nullptr || du_ws == nullptr)) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t hw = static_cast<int64_t>(64) * h * w;
  if (g_logprobs != nullptr) {
    if (c == 19)
      hipLaunchKernelGGL(lsm_bwd_kernel<19>, dim3(grid_of(n * hw)), dim3(kThreads), 0, s, g_logprobs, logprobs, n, c, hw,
                         grad_scale, du_ws);
    else
      hipLaunchKernelGGL(lsm_bwd_kernel<0>, dim3(grid_of(n * hw)), dim3(kThreads), 0, s, g_logprobs, logprobs, n, c, hw,
                         grad_scale, du_ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return static_cast<int>(e);
  } else if (g_logits == nullptr) {   // logits-only gradient: dlogits = grad_scale * g_logits
    return DRNMI_EINVAL;
  }
  if (static_cast<int64_t>(n) * c > 65535) return DRNMI_EINVAL;   // planes on grid z
  hipLaunchKernelGGL(up8_bwd_kernel, dim3((w + kUbJ - 1) / kUbJ, (h + kUbI - 1) / kUbI, n * c), dim3(kUbThreads), 0, s,
                     g_logprobs != nullptr ? du_ws : nullptr, up_w, g_logits, grad_scale, n * c, h, w, dlogits);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_up8_bilinear_lsm_bwd_f32(const float* g_logprobs, const float* logprobs, const float* g_logits,
                                              float grad_scale, int32_t n, int32_t c, int32_t h, int32_t w,
                                              float* du_ws, float* dlogits, void* stream) {
  if (dlogits == nullptr || n <= 0 || c <= 0 || h <= 0 || w <= 0) return DRNMI_EINVAL;
  if (g_logprobs != nullptr && (logprobs == nullptr || du_ws == nullptr)) return DRNMI_EINVAL;
  if (g_logprobs == nullptr && g_logits == nullptr) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t hw = static_cast<int64_t>(64) * h * w;
  if (g_logprobs != nullptr) {
    if (c == 19)
      hipLaunchKernelGGL(lsm_bwd_kernel<19>, dim3(grid_of(n * hw)), dim3(kThreads), 0, s, g_logprobs, logprobs, n, c, hw,
                         grad_scale, du_ws);
    else
      hipLaunchKernelGGL(lsm_bwd_kernel<0>, dim3(grid_of(n * hw)), dim3(kThreads), 0, s, g_logprobs, logprobs, n, c, hw,
                         grad_scale, du_ws);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return static_cast<int>(e);
  }
  hipLaunchKernelGGL(up8_bilinear_bwd_kernel, dim3(grid_of(static_cast<int64_t>(n) * c * h * w)), dim3(kThreads), 0, s,
                     g_logprobs != nullptr ? du_ws : nullptr, g_logits, grad_scale, n * c, h, w, dlogits);
  return static_cast<int>(hipGetLastError());
}

extern "C" int64_t drnmi_ce_workspace_bytes(void) { return 3LL * kCeBlocks * 8; }

extern "C" int drnmi_ce_loss_f32(const float* logprobs, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                                 int64_t ignore_index, float* loss, float* count, void* ws, void* stream) {
  if (logprobs == nullptr || target == nullptr || loss == nullptr || count == nullptr || ws == nullptr || n <= 0 ||
      c <= 0 || hw <= 0)
    return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (c == 19)
    hipLaunchKernelGGL(ce_fwd_kernel<19>, dim3(kCeBlocks), dim3(kThreads), 0, s, logprobs, target, n, c, hw,
                       ignore_index, reinterpret_cast<double*>(ws));
  else
    hipLaunchKernelGGL(ce_fwd_kernel<0>, dim3(kCeBlocks), dim3(kThreads), 0, s, logprobs, target, n, c, hw,
                       ignore_index, reinterpret_cast<double*>(ws));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const double*>(ws), kCeBlocks, loss,
                     count);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_ce_loss_bwd_f32(const float* logprobs, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                                     int64_t ignore_index, const float* dloss, const float* count, float* g_logprobs,
                                     void* stream) {
  if (logprobs == nullptr || target == nullptr || dloss == nullptr || count == nullptr || g_logprobs == nullptr ||
      n <= 0 || c <= 0 || hw <= 0)
    return DRNMI_EINVAL;
  if (c == 19 && hw % 4 == 0 && aligned16(logprobs, g_logprobs, nullptr))
    hipLaunchKernelGGL(ce_bwd_v4_kernel<19>, dim3(grid_of(static_cast<int64_t>(n) * hw / 4)), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), logprobs, target, n, c, hw, ignore_index, dloss, count,
                       g_logprobs);
  else if (c == 19)
    hipLaunchKernelGGL(ce_bwd_kernel<19>, dim3(grid_of(static_cast<int64_t>(n) * hw)), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), logprobs, target, n, c, hw, ignore_index, dloss, count,
                       g_logprobs);
  else
    hipLaunchKernelGGL(ce_bwd_kernel<0>, dim3(grid_of(static_cast<int64_t>(n) * hw)), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), logprobs, target, n, c, hw, ignore_index, dloss, count,
                       g_logprobs);
  return static_cast<int>(hipGetLastError());
}

extern "C" int64_t drnmi_distill_workspace_bytes(void) { return 4LL * kCeBlocks * 8; }

namespace {
// the argument checks the two distillation entry points share (before any HIP call)
bool distill_args_ok(const void* s, const void* t, const void* target, int32_t n, int32_t c, int64_t hw,
                     float student_wt, float distill_wt, float temperature) {
  return s != nullptr && t != nullptr && target != nullptr && n > 0 && c > 0 && hw > 0 && std::isfinite(temperature) &&
         temperature > 0.f && std::isfinite(student_wt) && student_wt >= 0.f && std::isfinite(distill_wt) &&
         distill_wt >= 0.f;
}
// KD = sum kd_i / D: every pixel ("mean"), or the reference's size_average=False / shape[0] ("batchmean")
double distill_div(int32_t n, int64_t hw, int32_t batchmean) {
  return batchmean != 0 ? static_cast<double>(n) : static_cast<double>(n) * static_cast<double>(hw);
}
}  // namespace

extern "C" int drnmi_distill_loss_f32(const float* student_lp, const float* teacher_lp, const int64_t* target,
                                      int32_t n, int32_t c, int64_t hw, int64_t ignore_index, float student_wt,
                                      float distill_wt, float temperature, int32_t batchmean, float* out3,
                                      float* count, void* ws, void* stream) {
  if (!distill_args_ok(student_lp, teacher_lp, target, n, c, hw, student_wt, distill_wt, temperature) ||
      out3 == nullptr || count == nullptr || ws == nullptr)
    return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float invT = 1.f / temperature;
  double* part = reinterpret_cast<double*>(ws);
  if (c == 19 && hw % 4 == 0 && aligned16(student_lp, teacher_lp, nullptr))
    hipLaunchKernelGGL((distill_fwd_kernel<19, 4>), dim3(kCeBlocks), dim3(kThreads), 0, s, student_lp, teacher_lp,
                       target, n, c, hw, ignore_index, invT, part);
  else if (c == 19)
    hipLaunchKernelGGL((distill_fwd_kernel<19, 1>), dim3(kCeBlocks), dim3(kThreads), 0, s, student_lp, teacher_lp,
                       target, n, c, hw, ignore_index, invT, part);
  else
    hipLaunchKernelGGL((distill_fwd_kernel<0, 1>), dim3(kCeBlocks), dim3(kThreads), 0, s, student_lp, teacher_lp,
                       target, n, c, hw, ignore_index, invT, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  hipLaunchKernelGGL(distill_final_kernel, dim3(1), dim3(64), 0, s, part, kCeBlocks, distill_div(n, hw, batchmean),
                     student_wt, distill_wt, out3, count);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_distill_loss_bwd_f32(const float* student_lp, const float* teacher_lp, const int64_t* target,
                                          int32_t n, int32_t c, int64_t hw, int64_t ignore_index, float student_wt,
                                          float distill_wt, float temperature, int32_t batchmean, const float* dloss,
                                          const float* count, float* g_student_lp, void* stream) {
  if (!distill_args_ok(student_lp, teacher_lp, target, n, c, hw, student_wt, distill_wt, temperature) ||
      dloss == nullptr || count == nullptr || g_student_lp == nullptr)
    return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float invT = 1.f / temperature;
  const float kd_scale = static_cast<float>(static_cast<double>(distill_wt) /
                                            (distill_div(n, hw, batchmean) * static_cast<double>(temperature)));
  const int64_t total = static_cast<int64_t>(n) * hw;
  if (c == 19 && hw % 4 == 0 && aligned16(student_lp, teacher_lp, g_student_lp))
    hipLaunchKernelGGL((distill_bwd_kernel<19, 4>), dim3(grid_of(total / 4)), dim3(kThreads), 0, s, student_lp,
                       teacher_lp, target, n, c, hw, ignore_index, invT, student_wt, kd_scale, dloss, count,
                       g_student_lp);
  else if (c == 19)
    hipLaunchKernelGGL((distill_bwd_kernel<19, 1>), dim3(grid_of(total)), dim3(kThreads), 0, s, student_lp,
                       teacher_lp, target, n, c, hw, ignore_index, invT, student_wt, kd_scale, dloss, count,
                       g_student_lp);
  else
    hipLaunchKernelGGL((distill_bwd_kernel<0, 1>), dim3(grid_of(total)), dim3(kThreads), 0, s, student_lp,
                       teacher_lp, target, n, c, hw, ignore_index, invT, student_wt, kd_scale, dloss, count,
                       g_student_lp);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_sgd_step_f32(int32_t ntensors, float* const* params, const float* const* grads,
                                  float* const* momentum_bufs, const int64_t* numels,
                                  const uint32_t* const* mask_bits, const int32_t* first_step, float lr,
                                  float momentum, float dampening, float weight_decay, int32_t nesterov,
                                  void* stream) {
  if (ntensors < 0 || (ntensors > 0 && (params == nullptr || grads == nullptr || numels == nullptr)))
    return DRNMI_EINVAL;
  if (momentum != 0.f && ntensors > 0 && (momentum_bufs == nullptr || first_step == nullptr)) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int t0 = 0; t0 < ntensors; t0 += kSgdBatch) {
    SgdBatch b{};
    const int cnt = ntensors - t0 < kSgdBatch ? ntensors - t0 : kSgdBatch;
    int64_t maxn = 0;
    for (int i = 0; i < cnt; ++i) {
      const int k = t0 + i;
      b.w[i] = params[k];
      b.g[i] = grads[k];
      b.buf[i] = momentum != 0.f ? momentum_bufs[k] : nullptr;
      b.mask[i] = mask_bits != nullptr ? mask_bits[k] : nullptr;
      b.numel[i] = numels[k];
      b.first[i] = momentum != 0.f ? first_step[k] : 0;
      if (b.numel[i] < 0) return DRNMI_EINVAL;
      if (b.numel[i] > 0 && (b.w[i] == nullptr || b.g[i] == nullptr || (momentum != 0.f && b.buf[i] == nullptr)))
        return DRNMI_EINVAL;
      maxn = b.numel[i] > maxn ? b.numel[i] : maxn;
    }
    if (maxn == 0) continue;
    unsigned gx = grid_of(maxn);
    gx = gx > 1024 ? 1024 : gx;
    hipLaunchKernelGGL(sgd_kernel, dim3(gx, cnt), dim3(kThreads), 0, s, b, lr, momentum, dampening, weight_decay,
                       nesterov);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return static_cast<int>(e);
  }
  return DRNMI_OK;
}
