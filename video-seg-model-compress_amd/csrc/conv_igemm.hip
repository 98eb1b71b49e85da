// NHWC implicit-GEMM convolution with a fused BN / bias + residual + ReLU epilogue.
//
// One kernel template covers every convolution of DRN-D (reference lmodels/drn.py):
// the 7x7 stem (layer0, :132-137), the 3x3 dilated convs (conv3x3 :27-29, BasicBlock
// :32-65, _make_conv_layers :201-211), the Bottleneck 1x1/3x3/1x1 (:68-106), the 1x1
// stride-s downsample (:181-186) and the seg 1x1 + bias (lmodels/drnseg.py:278-284).
//
// GEMM view: rows = output pixels (n, oh, ow), cols = output channels, K = (tap, ci)
// with k = tap*cin + ci.  A rows are gathered straight from the NHWC input (each
// 8-channel vector of a pixel is one 16 B / 32 B load; out-of-image taps load zeros,
// which is the conv's zero padding), B rows are the packed weights [cout_pad][k_pad].
// Both operands are register-staged into double-buffered LDS (one barrier per K-step)
// and consumed by MFMA:
//   bf16 mode: v_mfma_f32_16x16x32_bf16, fp32 accumulate (perf mode)
//   fp32 mode: v_mfma_f32_16x16x4_f32 — an exact fp32 fmaf chain (parity mode).  A launch given
//     drnmi_conv_args.ws (the training plan: the fine-tune's forward and data-gradient convs) folds
//     the chain into a second accumulator every 256 k (kFoldSteps) from K = 1024 on: one chain over
//     K = 4608 erred up to 10 x a blocked fp32 sum against float64 (profiles/train_audit), the
//     folded one ~1.5 x.  K = 512 .. 1023 folds every 128 k (kFoldShortSteps): one chain over K = 576
//     errs ~3.5 x on average and was measured at 5.3 x on a D-24 layer3 data gradient, the folded
//     one 0.5 x.  Inference launches (ws = NULL) and K < 512 keep the single chain, bit for bit:
//     the fp32 mode's labels are pinned against the reference in that order.
// The per-lane K permutation (lane holds k = 8*(lane>>4) + j) is identical for A and B,
// so one LDS image and one fragment read serve both MFMA shapes.
//
// Workgroup = 4 waves (256 threads), 64-wide wavefronts; tiles are assigned XCD-major
// (blocks b and b+8 share an XCD) so the blocks that share an input row-band and a
// weight panel run under one L2.
#include "common.h"
#include "kernels.h"

namespace drnmi {

namespace {

constexpr int kBK = 32;
constexpr int kThreads = 256;
constexpr int kFoldSteps = 8;       // fp32 mode: K steps per chain before it is folded (256 k)
constexpr int kFoldLongSteps = 32;  // ... in a training launch of at least this many K steps (K >= 1024);
constexpr int kFoldShortSteps = 4;  // a shorter one folds every 128 k
constexpr int kFoldMinSteps = 16;   // ... from this many K steps on (K >= 512)

template <typename T>
__device__ __forceinline__ void mma_step(f32x4& acc, const T* a, const T* b);

template <>
__device__ __forceinline__ void mma_step<bf16_t>(f32x4& acc, const bf16_t* a, const bf16_t* b) {
  const bf16x8 av = *reinterpret_cast<const bf16x8*>(a);
  const bf16x8 bv = *reinterpret_cast<const bf16x8*>(b);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
}

template <>
__device__ __forceinline__ void mma_step<float>(f32x4& acc, const float* a, const float* b) {
  const float4 a0 = reinterpret_cast<const float4*>(a)[0];
  const float4 a1 = reinterpret_cast<const float4*>(a)[1];
  const float4 b0 = reinterpret_cast<const float4*>(b)[0];
  const float4 b1 = reinterpret_cast<const float4*>(b)[1];
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc, 0, 0, 0);
}

__device__ __forceinline__ void store_out(void* y, int64_t off, float v, int out_dtype) {
  if (out_dtype == DRNMI_BF16) {
    reinterpret_cast<bf16_t*>(y)[off] = f32_to_bf16(v);
  } else {
    reinterpret_cast<float*>(y)[off] = v;
  }
}

// Bijective XCD-major remap of a 1-D grid (cdna_hip_programming.md §5, "XCD swizzle").
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = bid % 8;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + bid / 8;
}

template <typename T, int BM, int BN, int WAVES_M, int WAVES_N, int KS>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 2 : 1)))
conv_igemm_kernel(const drnmi_conv_args p) {
  constexpr int PAD = sizeof(T) == 2 ? 8 : 4;  // breaks the power-of-two row stride
  constexpr int LDK = kBK + PAD;
  constexpr int WTM = BM / WAVES_M;
  constexpr int WTN = BN / WAVES_N;
  constexpr int FM = WTM / 16;
  constexpr int FN = WTN / 16;
  constexpr int AV = BM * (kBK / 8);
  constexpr int BV = BN * (kBK / 8);
  constexpr int APT = (AV + kThreads - 1) / kThreads;
  constexpr int BPT = (BV + kThreads - 1) / kThreads;
  constexpr int BUF = (BM + BN) * LDK;
  static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");
  static_assert(FM >= 1 && FN >= 1, "wave tile at least 16x16");

  __shared__ __attribute__((aligned(16))) T smem[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WAVES_N;
  const int wn = wave % WAVES_N;

  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int mt_count = (M + BM - 1) / BM;
  const int nt_count = (p.cout + BN - 1) / BN;      // column tiles past cout would be all padding
  const int tile = xcd_remap(blockIdx.x, mt_count * nt_count);
  const int bm0 = (tile / nt_count) * BM;
  const int bn0 = (tile % nt_count) * BN;

  const int cin = p.cin;
  const int cmask = cin - 1;
  const int lc = 31 - __builtin_clz(cin);
  const int H = p.h, W = p.w, dil = p.dil;
  const T* __restrict__ x = reinterpret_cast<const T*>(p.x);
  const T* __restrict__ wt = reinterpret_cast<const T*>(p.wgt);

  // Per-thread A rows: pixel coordinates are fixed for the whole K loop.
  int a_ih0[APT], a_iw0[APT], a_c[APT], a_row[APT];
  int64_t a_base[APT];
  bool a_on[APT];
#pragma unroll
  for (int i = 0; i < APT; ++i) {
    const int v = tid + i * kThreads;
    a_on[i] = v < AV;
    a_row[i] = v >> 2;
    a_c[i] = v & 3;
    const int m = bm0 + a_row[i];
    a_ih0[i] = -(1 << 28);
    a_iw0[i] = -(1 << 28);
    a_base[i] = 0;
    if (a_on[i] && m < M) {
      const int n = m / hw_o;
      const int r = m - n * hw_o;
      const int oh = r / p.wo;
      const int ow = r - oh * p.wo;
      a_ih0[i] = oh * p.stride - p.pad;
      a_iw0[i] = ow * p.stride - p.pad;
      a_base[i] = static_cast<int64_t>(n) * H * W * cin;
    }
  }

  Vec8<T> ra[APT];
  Vec8<T> rb[BPT];

  auto load_tiles = [&](int kt) {
#pragma unroll
    for (int i = 0; i < APT; ++i) {
      Vec8<T> v = Vec8<T>::zero();
      if (a_on[i]) {
        const int k0 = kt * kBK + 8 * a_c[i];
        const int tap = k0 >> lc;
        const int ci = k0 & cmask;
        if (tap < KS * KS) {
          const int kh = tap / KS;
          const int kw = tap - kh * KS;
          const int ih = a_ih0[i] + kh * dil;
          const int iw = a_iw0[i] + kw * dil;
          if (static_cast<unsigned>(ih) < static_cast<unsigned>(H) &&
              static_cast<unsigned>(iw) < static_cast<unsigned>(W)) {
            v = Vec8<T>::load(x + a_base[i] + (static_cast<int64_t>(ih) * W + iw) * cin + ci);
          }
        }
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      const int v = tid + i * kThreads;
      if (v < BV) {
        const int row = v >> 2;
        const int c = v & 3;
        rb[i] = Vec8<T>::load(wt + static_cast<int64_t>(bn0 + row) * p.k_pad + kt * kBK + 8 * c);
      }
    }
  };

  auto store_tiles = [&](int buf) {
    T* As = smem + buf * BUF;
    T* Bs = As + BM * LDK;
#pragma unroll
    for (int i = 0; i < APT; ++i) {
      if (a_on[i]) ra[i].store(As + a_row[i] * LDK + 8 * a_c[i]);
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      const int v = tid + i * kThreads;
      if (v < BV) rb[i].store(Bs + (v >> 2) * LDK + 8 * (v & 3));
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr bool kFold = sizeof(T) == 4;
  f32x4 tot[kFold ? FM : 1][kFold ? FN : 1];
#pragma unroll
  for (int i = 0; i < (kFold ? FM : 1); ++i)
#pragma unroll
    for (int j = 0; j < (kFold ? FN : 1); ++j) tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = p.k_pad / kBK;
  const bool fold = kFold && p.ws != nullptr && nk >= kFoldMinSteps;
  const int fold_mask = (nk >= kFoldLongSteps ? kFoldSteps : kFoldShortSteps) - 1;
  load_tiles(0);
  store_tiles(0);
  __syncthreads();

  const int frag_row = lane & 15;
  const int frag_k = 8 * (lane >> 4);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) load_tiles(kt + 1);
    const T* As = smem + cur * BUF;
    const T* Bs = As + BM * LDK;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      const T* ap = As + (wm * WTM + fm * 16 + frag_row) * LDK + frag_k;
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const T* bp = Bs + (wn * WTN + fn * 16 + frag_row) * LDK + frag_k;
        mma_step<T>(acc[fm][fn], ap, bp);
      }
    }
    if constexpr (kFold) {
      if (fold && ((kt & fold_mask) == fold_mask || !more)) {
#pragma unroll
        for (int fm = 0; fm < FM; ++fm)
#pragma unroll
          for (int fn = 0; fn < FN; ++fn) {
            tot[fm][fn] += acc[fm][fn];
            acc[fm][fn] = more ? f32x4{0.f, 0.f, 0.f, 0.f} : tot[fm][fn];
          }
      }
    }
    if (more) store_tiles(cur ^ 1);
    __syncthreads();
  }

  // Epilogue: folded BN (or bias), optional residual, optional ReLU, strided store.
  const T* __restrict__ res = reinterpret_cast<const T*>(p.res);
  const int col_l = lane & 15;
  const int row_q = (lane >> 4) * 4;
#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = bm0 + wm * WTM + fm * 16 + row_q + j;
      if (m >= M) continue;
      const int n = m / hw_o;
      const int q = m - n * hw_o;
      const int64_t ybase = static_cast<int64_t>(n) * p.y_sn + static_cast<int64_t>(q) * p.y_sp;
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int co = bn0 + wn * WTN + fn * 16 + col_l;
        if (co >= p.cout) continue;
        float v = acc[fm][fn][j] * (p.scale != nullptr ? p.scale[co] : 1.f) + p.shift[co];
        if (res != nullptr) v += Elem<T>::to_f32(res[static_cast<int64_t>(m) * p.cout + co]);
        if (p.relu) v = fmaxf(v, 0.f);
        store_out(p.y, ybase + static_cast<int64_t>(co) * p.y_sc, v, p.out_dtype);
      }
    }
  }
}

template <typename T, int BM, int BN, int WM, int WN, int KS>
hipError_t launch_conv(const drnmi_conv_args& p, hipStream_t stream) {
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = ((M + BM - 1) / BM) * ((p.cout + BN - 1) / BN);   // (as the kernel's nt_count)
  hipLaunchKernelGGL((conv_igemm_kernel<T, BM, BN, WM, WN, KS>), dim3(static_cast<unsigned>(blocks)),
                     dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

// the element types as the kernel names spell them
using bf16 = bf16_t;
using f32 = float;
#define IGEMM_TILES(T, KS)                                                 \
  {DRNMI_KERNEL_ROW(conv_igemm_kernel, launch_conv, T, 128, 128, 2, 2, KS), \
   DRNMI_KERNEL_ROW(conv_igemm_kernel, launch_conv, T, 128, 64, 2, 2, KS),  \
   DRNMI_KERNEL_ROW(conv_igemm_kernel, launch_conv, T, 256, 32, 4, 1, KS),  \
   DRNMI_KERNEL_ROW(conv_igemm_kernel, launch_conv, T, 256, 16, 4, 1, KS)}
// [bf16][ks 1 / 3 / 7][tile]
}  // namespace

const ConvKernel* igemm_kernel(int dtype, int tile, int ks) {
  static const ConvKernel kIgemm[2][3][4] = {{IGEMM_TILES(f32, 1), IGEMM_TILES(f32, 3), IGEMM_TILES(f32, 7)},
                                             {IGEMM_TILES(bf16, 1), IGEMM_TILES(bf16, 3), IGEMM_TILES(bf16, 7)}};
  const int k = ks == 1 ? 0 : ks == 3 ? 1 : ks == 7 ? 2 : -1;
  return k < 0 ? nullptr : &kIgemm[dtype == DRNMI_BF16][k][tile];
}

}  // namespace drnmi
