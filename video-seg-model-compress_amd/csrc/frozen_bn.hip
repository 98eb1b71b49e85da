// Fine-tuning with frozen BatchNorm statistics (DRNSeg.freeze_bn).
//
// With the running statistics frozen a BN node is a per-channel affine of its conv:
//   z = relu?(conv(x, s o w) + t [+ res]),  s = gamma * rsqrt(running_var + eps),  t = beta - running_mean * s
// so the forward folds s into the packed weights and puts t, the residual and the ReLU into the conv
// epilogue (train.hip's packs take the scale; no kernel here runs per element in the forward), and
// the backward needs the conv output y nowhere:
//   dr     = relu ? (z > 0 ? dz : 0) : dz          consumed by the weight and data gradients
//   dbeta  = sum_rows dr
//   G      = wgrad(dr, x) = dL/d(s o w)            the existing weight-gradient kernels, into a scratch
//   dw     = s o G
//   dgamma = rsqrt(running_var + eps) * (<G[c,:], w[c,:]> - running_mean * dbeta)
// The last line is sum_rows(dr * xhat) with xhat = (y - running_mean) * rsqrt(...), through the identity
// sum_rows(dr * y)[c] = <wgrad(dr, x)[c,:], w[c,:]> (y is linear in w): a dot product over a weight row
// instead of a second pass over the activations.
//
//   frozen_prepare_kernel     s, t and rsqrt(running_var + eps) of every BN node of the network, one
//                             workgroup per node (a device table), one launch per step
//   frozen_act_bwd_kernel     one pass over [rows][C]: dr in place over dz, dres stored or accumulated,
//                             and the per-channel sums of dr.  A lane owns four consecutive channels
//                             (one 16-B access) and walks rows, so its channels never change; the
//                             workgroup's row groups are combined through LDS in row-group order and one
//                             fp64 partial per channel and workgroup goes to the workspace ([G][C]).
//   frozen_dbeta_final_kernel sums the G partials of a channel in a fixed order
//   frozen_unfold_kernel      dw and dgamma from G: one wave per output channel while a weight row is
//                             short (four channels per workgroup), the whole workgroup on one channel
//                             from 2048 floats per row; the dot product in fp64, lanes combined by a
//                             fixed xor tree, the four waves in wave order through LDS
// No atomics anywhere: two runs give the same bits.
#include <cmath>

#include "common.h"

namespace drnmi {
namespace {

constexpr int kFzThreads = 256;
constexpr int kFzWaves = kFzThreads / 64;
constexpr int kFzMaxNodes = 1024;
constexpr int64_t kFzWideRow = 2048;     // floats per weight row from which a workgroup owns one channel

__global__ void __launch_bounds__(kFzThreads) frozen_prepare_kernel(const int64_t* __restrict__ tab) {
  const int64_t* q = tab + static_cast<int64_t>(blockIdx.x) * DRNMI_FROZEN_BN_ENTRY_WORDS;
  const float* __restrict__ gamma = reinterpret_cast<const float*>(q[0]);
  const float* __restrict__ beta = reinterpret_cast<const float*>(q[1]);
  const float* __restrict__ rmean = reinterpret_cast<const float*>(q[2]);
  const float* __restrict__ rvar = reinterpret_cast<const float*>(q[3]);
  float* __restrict__ s = reinterpret_cast<float*>(q[4]);
  float* __restrict__ t = reinterpret_cast<float*>(q[5]);
  float* __restrict__ rstd = reinterpret_cast<float*>(q[6]);
  const int C = static_cast<int>(q[7]), cpad = static_cast<int>(q[8]);
  const float eps = __int_as_float(static_cast<int>(q[9]));
  for (int c = threadIdx.x; c < cpad; c += kFzThreads) {
    float sv = 0.f, tv = 0.f, rv = 0.f;                  // the pad channels: a zero weight row, a zero shift
    if (c < C) {
      rv = 1.f / sqrtf(__fadd_rn(rvar[c], eps));
      sv = __fmul_rn(gamma != nullptr ? gamma[c] : 1.f, rv);
      tv = __fsub_rn(beta != nullptr ? beta[c] : 0.f, __fmul_rn(rmean[c], sv));
    }
    s[c] = sv;
    t[c] = tv;
    rstd[c] = rv;
  }
}

struct FzBwdArgs {
  float* dz;            // in: dz, out: dr (written only with relu: without it dr is dz)
  const float* z;       // relu: the forward's output
  float* dres;          // NULL-able
  int64_t rows;
  int64_t rows_per_split;
  int C;
  double* ws;           // [G][C] partial sums of dr
};

// lanes per row (four channels each) and the row splits: train.hip's red_splits rule, which is what
// drnmi_reduce_workspace_bytes sizes the workspace by.  C = 16 at full resolution: 4 lanes per row, 64
// row groups, 1024 workgroups; C = 512 at 1/8 resolution: 2 channel chunks x 384 splits.
inline int fz_tpr(int C) { return (C / 4) < 64 ? (C / 4) : 64; }
inline int fz_splits(int64_t rows, int C) {
  const int tpr = fz_tpr(C);
  const int rg = kFzThreads / tpr;
  int64_t g = 1024 / (C / (4 * tpr));
  const int64_t by_rows = (rows + 16 * rg - 1) / (16 * rg);   // >= 16 rows per lane
  if (g > by_rows) g = by_rows;
  return static_cast<int>(g < 1 ? 1 : g);
}

__device__ __forceinline__ float sel(float z, float g) { return z > 0.f ? g : 0.f; }

// DRES: 0 no residual branch, 1 dres = dr, 2 dres += dr
template <bool RELU, int DRES>
__global__ void __launch_bounds__(kFzThreads) frozen_act_bwd_kernel(const FzBwdArgs a) {
  const int tpr = (a.C / 4) < 64 ? (a.C / 4) : 64;
  const int rg = kFzThreads / tpr;
  const int t = threadIdx.x;
  const int tc = t % tpr, tr = t / tpr;
  const int c0 = blockIdx.y * 4 * tpr + 4 * tc;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * a.rows_per_split;
  const int64_t r1 = (r0 + a.rows_per_split) < a.rows ? (r0 + a.rows_per_split) : a.rows;
  double s[4] = {0, 0, 0, 0};
  auto one = [&](int64_t off, const float4& g, const float4& zv, const float4& old) {
    float4 d = g;
    if constexpr (RELU) {
      d = make_float4(sel(zv.x, g.x), sel(zv.y, g.y), sel(zv.z, g.z), sel(zv.w, g.w));
      *reinterpret_cast<float4*>(a.dz + off) = d;
    }
    if constexpr (DRES == 1) *reinterpret_cast<float4*>(a.dres + off) = d;
    if constexpr (DRES == 2)
      *reinterpret_cast<float4*>(a.dres + off) = make_float4(__fadd_rn(old.x, d.x), __fadd_rn(old.y, d.y),
                                                              __fadd_rn(old.z, d.z), __fadd_rn(old.w, d.w));
    s[0] += d.x;
    s[1] += d.y;
    s[2] += d.z;
    s[3] += d.w;
  };
  // RB rows' loads go out before their stores and (in-order) fp64 sums
  constexpr int RB = 4;
  int64_t row = r0 + tr;
  for (; row + (RB - 1) * rg < r1; row += RB * rg) {
    float4 g[RB], zv[RB], old[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const int64_t off = (row + u * rg) * a.C + c0;
      g[u] = *reinterpret_cast<const float4*>(a.dz + off);
      if constexpr (RELU) zv[u] = *reinterpret_cast<const float4*>(a.z + off);
      if constexpr (DRES == 2) old[u] = *reinterpret_cast<const float4*>(a.dres + off);
    }
#pragma unroll
    for (int u = 0; u < RB; ++u) one((row + u * rg) * a.C + c0, g[u], zv[u], old[u]);
  }
  for (; row < r1; row += rg) {
    const int64_t off = row * a.C + c0;
    float4 zv = make_float4(0.f, 0.f, 0.f, 0.f), old = zv;
    const float4 g = *reinterpret_cast<const float4*>(a.dz + off);
    if constexpr (RELU) zv = *reinterpret_cast<const float4*>(a.z + off);
    if constexpr (DRES == 2) old = *reinterpret_cast<const float4*>(a.dres + off);
    one(off, g, zv, old);
  }
  __shared__ double sh[kFzThreads * 4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sh[t * 4 + j] = s[j];
  __syncthreads();
  // thread q < 4 * tpr sums channel q of the workgroup over the rg row groups, in order
  if (t < 4 * tpr) {
    double acc = 0;
    for (int g = 0; g < rg; ++g) acc += sh[(g * tpr + t / 4) * 4 + (t % 4)];
    a.ws[static_cast<int64_t>(blockIdx.x) * a.C + blockIdx.y * 4 * tpr + t] = acc;
  }
}

// A workgroup owns 16 channels (a 128-B row of partials per split); 16 threads per channel sum 16
// contiguous runs of splits, which thread tc then adds run by run.
constexpr int kFzFinCh = 16;
__global__ void __launch_bounds__(kFzThreads)
frozen_dbeta_final_kernel(const double* __restrict__ ws, int G, int C, double* __restrict__ sum_out,
                          float* __restrict__ dbeta, int accumulate) {
  __shared__ double p[kFzThreads];
  const int t = threadIdx.x, tc = t % kFzFinCh, tg = t / kFzFinCh;
  constexpr int NG = kFzThreads / kFzFinCh;
  const int c = blockIdx.x * kFzFinCh + tc;
  const int gs = (G + NG - 1) / NG;
  const int g0 = tg * gs, g1 = g0 + gs < G ? g0 + gs : G;
  double acc = 0;
  if (c < C)
    for (int g = g0; g < g1; ++g) acc += ws[static_cast<int64_t>(g) * C + c];
  p[t] = acc;
  __syncthreads();
  if (t >= kFzFinCh || c >= C) return;
  double sum = 0;
  for (int j = 0; j < NG; ++j) sum += p[j * kFzFinCh + tc];
  if (sum_out != nullptr) sum_out[c] = sum;
  if (dbeta != nullptr) {
    const float v = static_cast<float>(sum);
    dbeta[c] = accumulate ? __fadd_rn(dbeta[c], v) : v;
  }
}

struct FzUnfoldArgs {
  const float* g;        // [cout][K]: wgrad(dr, x) = dL/d(s o w)
  const float* w;        // [cout][K]: the weights the forward folded
  const float* s;
  const float* rstd;
  const float* rmean;
  const double* dbeta_sum;
  float* dw;             // NULL-able
  float* dgamma;         // NULL-able
  int64_t K;
  int cout;
  int dw_acc, dgamma_acc;
};

// WPC waves per channel (1: four channels per workgroup, 4: one); VEC: rows as 16-B pieces
template <int WPC, bool VEC>
__global__ void __launch_bounds__(kFzThreads) frozen_unfold_kernel(const FzUnfoldArgs a) {
  __shared__ double part[kFzWaves];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int c = blockIdx.x * (kFzWaves / WPC) + wave / WPC;
  const int sub = wave % WPC;
  double dot = 0;
  if (c < a.cout) {
    const float sc = a.s[c];
    const int64_t base = static_cast<int64_t>(c) * a.K;
    if constexpr (VEC) {
      const int64_t k4 = a.K / 4;
#pragma unroll 2
      for (int64_t i = sub * 64 + lane; i < k4; i += 64 * WPC) {
        const float4 gv = *reinterpret_cast<const float4*>(a.g + base + 4 * i);
        if (a.dgamma != nullptr) {
          const float4 wv = *reinterpret_cast<const float4*>(a.w + base + 4 * i);
          dot += static_cast<double>(gv.x) * wv.x;
          dot += static_cast<double>(gv.y) * wv.y;
          dot += static_cast<double>(gv.z) * wv.z;
          dot += static_cast<double>(gv.w) * wv.w;
        }
        if (a.dw != nullptr) {
          float4 o = make_float4(__fmul_rn(sc, gv.x), __fmul_rn(sc, gv.y), __fmul_rn(sc, gv.z), __fmul_rn(sc, gv.w));
          float4* q = reinterpret_cast<float4*>(a.dw + base + 4 * i);
          if (a.dw_acc) {
            const float4 old = *q;
            o = make_float4(__fadd_rn(old.x, o.x), __fadd_rn(old.y, o.y), __fadd_rn(old.z, o.z), __fadd_rn(old.w, o.w));
          }
          *q = o;
        }
      }
    } else {
      for (int64_t i = sub * 64 + lane; i < a.K; i += 64 * WPC) {
        const float gv = a.g[base + i];
        if (a.dgamma != nullptr) dot += static_cast<double>(gv) * a.w[base + i];
        if (a.dw != nullptr) {
          const float o = __fmul_rn(sc, gv);
          a.dw[base + i] = a.dw_acc ? __fadd_rn(a.dw[base + i], o) : o;
        }
      }
    }
  }
  if (a.dgamma == nullptr) return;                        // uniform over the grid
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) dot += __shfl_xor(dot, off, 64);
  if constexpr (WPC > 1) {
    if (lane == 0) part[wave] = dot;
    __syncthreads();
    dot = 0;
    for (int j = 0; j < WPC; ++j) dot += part[j];
  }
  if (lane == 0 && sub == 0 && c < a.cout) {
    const double sx = dot - static_cast<double>(a.rmean[c]) * a.dbeta_sum[c];   // sum(dr * (y - running_mean))
    const float dg = static_cast<float>(static_cast<double>(a.rstd[c]) * sx);
    a.dgamma[c] = a.dgamma_acc ? __fadd_rn(a.dgamma[c], dg) : dg;
  }
}

inline bool pow2_ge4(int c) { return c >= 4 && (c & (c - 1)) == 0; }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool RELU>
void launch_act_bwd(const FzBwdArgs& a, int G, int dres_mode, hipStream_t s) {
  const dim3 grid(G, a.C / (4 * fz_tpr(a.C)));
  if (dres_mode == 0) hipLaunchKernelGGL((frozen_act_bwd_kernel<RELU, 0>), grid, dim3(kFzThreads), 0, s, a);
  else if (dres_mode == 1) hipLaunchKernelGGL((frozen_act_bwd_kernel<RELU, 1>), grid, dim3(kFzThreads), 0, s, a);
  else hipLaunchKernelGGL((frozen_act_bwd_kernel<RELU, 2>), grid, dim3(kFzThreads), 0, s, a);
}

template <int WPC>
void launch_unfold(const FzUnfoldArgs& a, bool vec, hipStream_t s) {
  const int per = kFzWaves / WPC;
  const dim3 grid((a.cout + per - 1) / per);
  if (vec) hipLaunchKernelGGL((frozen_unfold_kernel<WPC, true>), grid, dim3(kFzThreads), 0, s, a);
  else hipLaunchKernelGGL((frozen_unfold_kernel<WPC, false>), grid, dim3(kFzThreads), 0, s, a);
}

}  // namespace
}  // namespace drnmi

using namespace drnmi;

extern "C" int drnmi_frozen_bn_table_check(const int64_t* t, int32_t n) {
  if (t == nullptr || n <= 0 || n > kFzMaxNodes) return DRNMI_EINVAL;
  for (int e = 0; e < n; ++e) {
    const int64_t* q = t + static_cast<int64_t>(e) * DRNMI_FROZEN_BN_ENTRY_WORDS;
    if (q[2] == 0 || q[3] == 0 || q[4] == 0 || q[5] == 0 || q[6] == 0) return DRNMI_EINVAL;
    if (q[7] <= 0 || q[8] < q[7] || q[8] >= (int64_t(1) << 24)) return DRNMI_EINVAL;
    for (int j = 0; j < 7; ++j)
      if (q[j] & 3) return DRNMI_EINVAL;
    const float eps = __builtin_bit_cast(float, static_cast<int32_t>(q[9]));
    if (!(eps >= 0.f) || !std::isfinite(eps) || q[9] != static_cast<int64_t>(static_cast<int32_t>(q[9]))) return DRNMI_EINVAL;
  }
  return 0;
}

extern "C" int drnmi_frozen_bn_prepare_f32(const int64_t* table, int32_t n, void* stream) {
  if (table == nullptr || n <= 0 || n > kFzMaxNodes) return DRNMI_EINVAL;
  hipLaunchKernelGGL(frozen_prepare_kernel, dim3(n), dim3(kFzThreads), 0, reinterpret_cast<hipStream_t>(stream), table);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_frozen_bn_act_bwd_f32(float* dz, const float* z, int32_t relu, int64_t rows, int32_t C, float* dres,
                                           int32_t dres_accumulate, float* dbeta, int32_t dbeta_accumulate,
                                           double* dbeta_sum, void* ws, void* stream) {
  if (dz == nullptr || ws == nullptr || rows <= 0 || !pow2_ge4(C) || (relu && z == nullptr)) return DRNMI_EINVAL;
  if (rows >= (int64_t(1) << 40) || !al16(dz) || !al16(z) || !al16(dres) || (reinterpret_cast<uintptr_t>(ws) & 7) ||
      (reinterpret_cast<uintptr_t>(dbeta_sum) & 7))
    return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int G = fz_splits(rows, C);
  // the workspace is the caller's, sized by drnmi_reduce_workspace_bytes: the partials must fit it
  if (static_cast<int64_t>(G) * C * 8 > drnmi_reduce_workspace_bytes(rows, C)) return DRNMI_EINVAL;
  FzBwdArgs a{};
  a.dz = dz;
  a.z = z;
  a.dres = dres;
  a.rows = rows;
  a.rows_per_split = (rows + G - 1) / G;
  a.C = C;
  a.ws = reinterpret_cast<double*>(ws);
  const int mode = dres == nullptr ? 0 : (dres_accumulate ? 2 : 1);
  if (relu) launch_act_bwd<true>(a, G, mode, s);
  else launch_act_bwd<false>(a, G, mode, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || (dbeta == nullptr && dbeta_sum == nullptr)) return static_cast<int>(e);
  hipLaunchKernelGGL(frozen_dbeta_final_kernel, dim3((C + kFzFinCh - 1) / kFzFinCh), dim3(kFzThreads), 0, s, a.ws, G, C,
                     dbeta_sum, dbeta, dbeta_accumulate);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_frozen_bn_unfold_f32(const float* g, const float* w, const float* s, const float* rstd,
                                          const float* running_mean, const double* dbeta_sum, int32_t cout, int64_t K,
                                          float* dw, int32_t dw_accumulate, float* dgamma, int32_t dgamma_accumulate,
                                          void* stream) {
  if (g == nullptr || s == nullptr || cout <= 0 || K <= 0 || K >= (int64_t(1) << 31) || (dw == nullptr && dgamma == nullptr))
    return DRNMI_EINVAL;
  if (dgamma != nullptr && (w == nullptr || rstd == nullptr || running_mean == nullptr || dbeta_sum == nullptr))
    return DRNMI_EINVAL;
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dw)) & 3) return DRNMI_EINVAL;
  if (reinterpret_cast<uintptr_t>(dbeta_sum) & 7) return DRNMI_EINVAL;
  FzUnfoldArgs a{};
  a.g = g;
  a.w = w;
  a.s = s;
  a.rstd = rstd;
  a.rmean = running_mean;
  a.dbeta_sum = dbeta_sum;
  a.dw = dw;
  a.dgamma = dgamma;
  a.K = K;
  a.cout = cout;
  a.dw_acc = dw_accumulate;
  a.dgamma_acc = dgamma_accumulate;
  const bool vec = K % 4 == 0 && al16(g) && al16(w) && al16(dw);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (K >= kFzWideRow) launch_unfold<kFzWaves>(a, vec, st);
  else launch_unfold<1>(a, vec, st);
  return static_cast<int>(hipGetLastError());
}
