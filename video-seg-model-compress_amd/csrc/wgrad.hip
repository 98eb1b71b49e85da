// The convolution weight gradient of the fine-tune step, fp32 and fp32x (split-bf16).
//
// dW[co][tap][ci] = sum_m dy[m][co] * x[pix(m, tap)][ci]: C = A * B with A = dy^T (co x m),
// B = im2col(x) (m x k), the pixel range cut into splits whose partial sums ws[z][co][k] a second
// kernel adds in split order.  No atomics and a fixed order everywhere: dw is bit-reproducible.
//
//   wgrad_kernel<T, X6>        the LDS tile: <64, false> exact fp32 (v_mfma_f32_16x16x4f32),
//                              <64, true> and <128, true> split-bf16 (six v_mfma_f32_16x16x32_bf16
//                              per product, common.h mfma_x6)
//   wgrad_dy_split_kernel      dy -> three transposed bf16 planes, once per launch, for
//   wgrad_x6_pre_kernel        the 128-tile that stages them by LDS-DMA and splits only x (K >= 1024)
//   wgrad_x6_direct_kernel     cout <= 32: operands from global memory into registers, no LDS
//   wgrad_reduce*_kernel       dw (+)= sum over the splits, into OIHW
//
// The LDS tiles share the stepped pixel walk (wgrad_pix_step); every split-bf16 kernel takes the
// six-product order from common.h mfma_x6.  The k-column decode and the partial-sum epilogue are
// written out in wgrad_kernel and in wgrad_x6_pre_kernel: as helpers (a struct, reference
// parameters, a per-fragment store) each one changed the register assignment of the 128-tile and
// of the pre kernel, whose code is kept instruction for instruction (profiles/wgrad_fold).
// The host side has one routing decision (wgrad_route) on one workspace layout (wgrad_layout) that
// the size queries, the plan query and the launch read.
#include "common.h"

namespace drnmi {
namespace {

constexpr int kThreads = 256;

struct WgradP {
  const float* dy;
  const float* x;
  float* ws;
  int dys, cout;
  int n, h, w, cs, ho, wo, ks, stride, pad, dil;
  int K;                 // ks * ks * cs
  int64_t M;
  int64_t pix_per_split;
};

constexpr int kWM = 32;      // pixels per chunk
constexpr int kWLD = kWM + 4;
constexpr int kWT = 64;      // tile rows / cols
constexpr int kWTBig = 128;  // the large tile's; the dy planes' rows are padded to a multiple of it

// A thread's pixel m = (n, oh, ow) advances by one chunk: the coordinates are stepped, not divided
// out of m every chunk (an int64 division per chunk and thread).  On the caller's own variables: as
// a struct copied per load the 128-tile and the pre kernel grew by a dozen instructions.
__device__ __forceinline__ void wgrad_pix_step(const WgradP& p, int64_t& m, int& n, int& oh, int& ow) {
  m += kWM;
  ow += kWM;
  while (ow >= p.wo) {
    ow -= p.wo;
    if (++oh == p.ho) {
      oh = 0;
      ++n;
    }
  }
}

// Tile T co x T k per workgroup: 4 waves of T/2 x T/2, F x F fragments each (F = T / 32), K loop
// over 32-pixel chunks of the block's pixel split.  Operand tiles go to LDS transposed ([row][m]).
//   fp32 (X6 = false, T = 64): one ds_read_b128 feeds 4 v_mfma_f32_16x16x4f32: lane l reads
// m = mm + 4*(l/16) + {0..3}; MFMA j consumes element j of both operands, so the pairing of A and B
// over m is identical and the 4 MFMAs together cover 16 pixels.
//   X6 (fp32x fine-tune): the same tiles and chunks, each 32-pixel chunk one K step of
// v_mfma_f32_16x16x32_bf16 on the exact 3-way bf16 splits of both operands (common.h split3), the
// six products above 2^-24 in conv_x6's order -- fp32-class accuracy at the bf16 MFMA rate
// (2.5 PF / 6 = 417 TF against the 157 TF of the f32 MFMA).  Lane (fr, fq) takes pixels
// 8 fq .. 8 fq + 7 of the chunk for its A row and its B column alike, so the pairing over m holds.
//   T = 128 (cout and K >= 128): every staged byte feeds twice the MFMAs of the 64 x 64 tile, and
// the split of a B fragment is done once per chunk and reused by the wave's four row blocks.  Two
// workgroups per CU (2 x 2 x 128 x 36 floats of LDS each) against four of the 64-tile.  It is at
// the register limit (256 VGPRs), so the skip of row fragments past cout (16- and 32-channel
// layers) stays a property of the 64-tile.
template <int T, bool X6>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(T == 64 ? 4 : 2))) wgrad_kernel(const WgradP p) {
  static_assert(T == 64 || (T == 128 && X6), "64-tile in both arithmetics, 128-tile split-bf16 only");
  constexpr int CPT = T / 8;      // columns (A: channels) a thread stages per pixel
  constexpr int F = T / 32;       // 16 x 16 fragments per wave and dimension
  constexpr int WT = T / 2;       // wave tile
  __shared__ __attribute__((aligned(16))) float As[2][T][kWLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][T][kWLD];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int wr = wave >> 1, wcn = wave & 1;
  const int co0 = blockIdx.y * T;
  const int kc0 = blockIdx.x * T;
  const int64_t m_begin = static_cast<int64_t>(blockIdx.z) * p.pix_per_split;
  int64_t m_end = m_begin + p.pix_per_split;
  if (m_end > p.M) m_end = p.M;
  // the transposed LDS writes As[CPT lv + j][lm] hit bank (4 j + lm) % 32 whatever lv is (rows are
  // 36 floats, 8 rows = 288 = 0 mod 32): with 8 pixels x 8 column groups per wave every write was
  // 8-way conflicted; 32 pixels per 32-lane half (lm = t % 32) makes them conflict-free, at 64 B
  // per pixel per load instruction pair instead of 256 B
  const int lm = t & 31;      // pixel row of the chunk this thread loads
  const int lv = t >> 5;      // CPT-column group
  // B column group: (tap, ci) fixed for the whole loop; CPT consecutive k stay in one tap (cs % 8 == 0
  // always, cs % 16 == 0 on the 128-tile: wgrad_big_ok)
  const int kcol = kc0 + CPT * lv;
  const int tap = kcol / p.cs;
  const int ci = kcol - tap * p.cs;
  const bool kval = kcol < p.K && tap < p.ks * p.ks;
  const int kh = kval ? tap / p.ks : 0;
  const int kw = kval ? tap - kh * p.ks : 0;
  const int co = co0 + CPT * lv;

  // The thread's pixel advances by kWM per chunk, and two register sets keep two chunks of global
  // loads in flight (chunk c + 2 loads while chunk c computes and chunk c + 1 is staged).  16-B
  // registers: as float[CPT] the 128-tile spilled more
  const int hw = p.ho * p.wo;
  int64_t m_cur = m_begin + lm;
  int p_n = 0, p_oh = 0, p_ow = 0;
  {
    const int mi = static_cast<int>(m_cur < p.M ? m_cur : 0);   // M < 2^31 (wgrad_check rejects larger)
    p_n = mi / hw;
    const int q = mi - p_n * hw;
    p_oh = q / p.wo;
    p_ow = q - p_oh * p.wo;
  }
  auto load = [&](float4 (&ra)[CPT / 4], float4 (&rb)[CPT / 4]) {
    const int64_t m = m_cur;
    const int nn = p_n, oh = p_oh, ow = p_ow;
    wgrad_pix_step(p, m_cur, p_n, p_oh, p_ow);
#pragma unroll
    for (int j = 0; j < CPT / 4; ++j) {
      ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      rb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (m >= m_end) return;
    const float* dr = p.dy + m * p.dys;
    if (co + CPT <= p.dys && co + CPT <= p.cout) {
#pragma unroll
      for (int j = 0; j < CPT / 4; ++j) ra[j] = *reinterpret_cast<const float4*>(dr + co + 4 * j);
    } else {
      float v[CPT];
#pragma unroll
      for (int j = 0; j < CPT; ++j) v[j] = co + j < p.cout ? dr[co + j] : 0.f;
#pragma unroll
      for (int j = 0; j < CPT / 4; ++j) ra[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    }
    if (kval) {
      const int ih = oh * p.stride - p.pad + kh * p.dil;
      const int iw = ow * p.stride - p.pad + kw * p.dil;
      if (static_cast<unsigned>(ih) < static_cast<unsigned>(p.h) && static_cast<unsigned>(iw) < static_cast<unsigned>(p.w)) {
        const float* xr = p.x + ((static_cast<int64_t>(nn) * p.h + ih) * p.w + iw) * p.cs + ci;
#pragma unroll
        for (int j = 0; j < CPT / 4; ++j) rb[j] = *reinterpret_cast<const float4*>(xr + 4 * j);
      }
    }
  };
  auto store = [&](int buf, const float4 (&ra)[CPT / 4], const float4 (&rb)[CPT / 4]) {
#pragma unroll
    for (int j = 0; j < CPT / 4; ++j) {
      const float av[4] = {ra[j].x, ra[j].y, ra[j].z, ra[j].w};
      const float bv[4] = {rb[j].x, rb[j].y, rb[j].z, rb[j].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        As[buf][CPT * lv + 4 * j + e][lm] = av[e];
        Bs[buf][CPT * lv + 4 * j + e][lm] = bv[e];
      }
    }
  };

  f32x4 acc[F][F];
#pragma unroll
  for (int i = 0; i < F; ++i)
#pragma unroll
    for (int j = 0; j < F; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15;
  const int fq = lane >> 4;
  auto compute = [&](int buf) {
    if constexpr (X6) {
      // B splits first, then one A row block at a time (fewer live split registers: the 64-tile
      // fits 128 VGPRs, four waves per SIMD, without spilling); same MFMA order per accumulator
      bf16x8 b[F][3];
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const float* br = &Bs[buf][wcn * WT + f * 16 + fr][8 * fq];
        split3(*reinterpret_cast<const float4*>(br), *reinterpret_cast<const float4*>(br + 4), b[f][0], b[f][1], b[f][2]);
      }
#pragma unroll
      for (int fi = 0; fi < F; ++fi) {
        if constexpr (T == 64)
          if (co0 + wr * WT + fi * 16 >= p.cout) continue;   // rows past cout (16- and 32-channel layers)
        bf16x8 a[3];
        const float* ar = &As[buf][wr * WT + fi * 16 + fr][8 * fq];
        split3(*reinterpret_cast<const float4*>(ar), *reinterpret_cast<const float4*>(ar + 4), a[0], a[1], a[2]);
#pragma unroll
        for (int fj = 0; fj < F; ++fj) mfma_x6(acc[fi][fj], a, b[fj]);
      }
    } else {
#pragma unroll
      for (int mm = 0; mm < kWM; mm += 16) {
        float4 a4[F], b4[F];
#pragma unroll
        for (int f = 0; f < F; ++f) {
          a4[f] = *reinterpret_cast<const float4*>(&As[buf][wr * WT + f * 16 + fr][mm + 4 * fq]);
          b4[f] = *reinterpret_cast<const float4*>(&Bs[buf][wcn * WT + f * 16 + fr][mm + 4 * fq]);
        }
#pragma unroll
        for (int fi = 0; fi < F; ++fi) {
          if (co0 + wr * WT + fi * 16 >= p.cout) continue;
#pragma unroll
          for (int fj = 0; fj < F; ++fj) {
            acc[fi][fj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[fi].x, b4[fj].x, acc[fi][fj], 0, 0, 0);
            acc[fi][fj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[fi].y, b4[fj].y, acc[fi][fj], 0, 0, 0);
            acc[fi][fj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[fi].z, b4[fj].z, acc[fi][fj], 0, 0, 0);
            acc[fi][fj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[fi].w, b4[fj].w, acc[fi][fj], 0, 0, 0);
          }
        }
      }
    }
  };

  // chunk c computes from LDS buffer c & 1; set X holds chunk c + 1 (staged after the compute),
  // set Y receives chunk c + 2 (its loads fly across the compute of c and the staging of c + 1)
  float4 r0a[CPT / 4], r0b[CPT / 4], r1a[CPT / 4], r1b[CPT / 4];
  load(r0a, r0b);
  store(0, r0a, r0b);
  load(r0a, r0b);                                   // chunk 1
  __syncthreads();
  for (int64_t mc = m_begin; mc < m_end; mc += 2 * kWM) {
    load(r1a, r1b);                                 // chunk c + 2 (zeros past the end)
    compute(0);
    if (mc + kWM < m_end) store(1, r0a, r0b);
    __syncthreads();
    if (mc + kWM >= m_end) break;
    load(r0a, r0b);                                 // chunk c + 3
    compute(1);
    if (mc + 2 * kWM < m_end) store(0, r1a, r1b);
    __syncthreads();
  }
  float* out = p.ws + static_cast<int64_t>(blockIdx.z) * p.cout * p.K;
#pragma unroll
  for (int fi = 0; fi < F; ++fi)
#pragma unroll
    for (int fj = 0; fj < F; ++fj) {
      const int k = kc0 + wcn * WT + fj * 16 + fr;
      if (k >= p.K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = co0 + wr * WT + fi * 16 + 4 * fq + r;
        if (c < p.cout) out[static_cast<int64_t>(c) * p.K + k] = acc[fi][fj][r];
      }
    }
}

// ---- fp32x weight gradient, dy pre-split -----------------------------------------------------
// The 128 x 128 tile above splits every dy and x value in each of the two waves that read it
// (~4.4 VALU instructions per MFMA: VALU-bound, MFMA busy 0.31, profiles/r5r_wgrad_pmc).  Here dy
// is split once per launch into three transposed bf16 planes [plane][co][m] (one HBM pass,
// wgrad_dy_split_kernel) that the tile stages with LDS-DMA like conv_x6's weight planes: the
// kernel splits only x.  Same split3 (RNE) of the same values and the same MFMA order per
// accumulator as wgrad_kernel<128, true>, so the partial sums are bit-identical to it.
__device__ float4 g_wgrad_zero[4];   // zero-initialised: the B source outside the image

// LDS byte address of a __shared__ object
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) void*)p));
}
// one 16-B-per-lane LDS-DMA (global_load_lds_dwordx4) to the wave-uniform LDS address `lds`
// (M0 holds the LDS address; its previous value is restored, as M0 is reserved to the compiler)
__device__ __forceinline__ void dma16(const void* src, uint32_t lds) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds) : "memory");
}
// XOR term of the 16-B chunk of a 128-B fp32 B row (the 64-B bf16 A rows take common.h swz64)
__device__ __forceinline__ int pre_swz_b(int row) { return ((row >> 1) & 1) | (row & 4); }
// transposed B write of row RR (0..15) of a thread's 16-row group: w[k] holds the lane address for
// swizzle value k -> (0, 1, 4, 5)
template <int RR>
__device__ __forceinline__ void pre_wr(const uint32_t (&w)[4], float v) {
  constexpr int k = ((RR >> 1) & 1) | (((RR >> 2) & 1) << 1);
  asm volatile("ds_write_b32 %0, %1 offset:%2" :: "v"(w[k]), "v"(v), "i"(RR * 128) : "memory");
}

__global__ void __launch_bounds__(kThreads)
wgrad_dy_split_kernel(const float* __restrict__ dy, int dys, int cout, int64_t M, int64_t Mp, int Cp,
                      bf16_t* __restrict__ out) {
  // thread: channel co = 64-channel block + t / 4, pixels 8 (t % 4) .. +7 of a 32-pixel group:
  // four lanes write one channel's 64-B row piece per plane; each read instruction is 16
  // consecutive channels (64 B) of 4 pixels
  const int t = threadIdx.x;
  const int64_t ngroups = Mp / 32;
  const int cblocks = Cp / 64;
  const int64_t total = ngroups * cblocks;
  const int64_t pstride = static_cast<int64_t>(Cp) * Mp;
  for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const int cb = static_cast<int>(b % cblocks);
    const int64_t g = b / cblocks;
    const int co = cb * 64 + (t >> 2);
    const int64_t m0 = g * 32 + 8 * (t & 3);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = (co < cout && m0 + j < M) ? dy[(m0 + j) * dys + co] : 0.f;
    bf16x8 h1, h2, h3;
    split3(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), h1, h2, h3);
    bf16_t* o = out + static_cast<int64_t>(co) * Mp + m0;
    *reinterpret_cast<bf16x8*>(o) = h1;
    *reinterpret_cast<bf16x8*>(o + pstride) = h2;
    *reinterpret_cast<bf16x8*>(o + 2 * pstride) = h3;
  }
}

struct WgradPreP {
  WgradP p;
  const bf16_t* dyt;   // [3][Cp][Mp]
  int64_t Mp;
  int Cp;
};

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) wgrad_x6_pre_kernel(const WgradPreP q) {
  const WgradP& p = q.p;
  // A: [buf][plane][128 rows][64 B] bf16 (16-B chunks swizzled), B: [buf][128 rows][32 floats]
  // (16-B chunks swizzled): 2 x (24 + 16) KB, two workgroups per CU
  __shared__ __attribute__((aligned(16))) char Ab[2][3 * kWTBig * 64];
  __shared__ __attribute__((aligned(16))) float Bs[2][kWTBig * 32];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int wr = wave >> 1, wcn = wave & 1;
  const int co0 = blockIdx.y * kWTBig;
  const int kc0 = blockIdx.x * kWTBig;
  const int64_t m_begin = static_cast<int64_t>(blockIdx.z) * p.pix_per_split;
  int64_t m_end = m_begin + p.pix_per_split;
  if (m_end > p.M) m_end = p.M;
  const int lm = t & 31;
  const int lv = t >> 5;
  const int hw = p.ho * p.wo;
  const int kcol = kc0 + 16 * lv;
  const int tap = kcol / p.cs;
  const int ci = kcol - tap * p.cs;
  const bool kval = kcol < p.K && tap < p.ks * p.ks;
  const int kh = kval ? tap / p.ks : 0;
  const int kw = kval ? tap - kh * p.ks : 0;

  // A DMA: 24 pieces of 1 KB per chunk, 6 per wave; piece gi = plane * 8 + 16-row block.  Sources
  // as element offsets from the block's first row (< 2^31: 3 x 128 rows x Mp), not 64-bit pointers
  // (six of those spilled to scratch, and the reload waited on every load in flight)
  const int64_t plane_stride = static_cast<int64_t>(q.Cp) * q.Mp;
  const bf16_t* a_base = q.dyt + static_cast<int64_t>(co0) * q.Mp;
  int32_t a_off[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int gi = wave * 6 + i;
    const int pl = gi >> 3;
    const int r = (gi & 7) * 16 + (lane >> 2);
    const int c = swz64(r, lane & 3);
    a_off[i] = static_cast<int32_t>(pl * plane_stride + static_cast<int64_t>(r) * q.Mp + 8 * c);
  }
  // as inline asm: hipcc models the LDS-DMA builtin's address registers as pending until vmcnt(0)
  // and drained the B loads in flight the first time it reused one
  const uint32_t a_dst = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(lds_addr(&Ab[0][wave * 6 * 1024]))));
  auto dma_a = [&](int buf, int64_t m) {
    const bf16_t* src = a_base + m;
#pragma unroll
    for (int i = 0; i < 6; ++i) dma16(src + a_off[i], a_dst + buf * static_cast<uint32_t>(sizeof(Ab[0])) + i * 1024);
  };

  int64_t m_cur = m_begin + lm;
  int p_n = 0, p_oh = 0, p_ow = 0;
  {
    const int mi = static_cast<int>(m_cur < p.M ? m_cur : 0);
    p_n = mi / hw;
    const int qq = mi - p_n * hw;
    p_oh = qq / p.wo;
    p_ow = qq - p_oh * p.wo;
  }
  // exactly four 16-B loads per call (the zero page outside the image / past the split), so that
  // the chunk-end wait below can leave them in flight with a fixed vmcnt
  auto load = [&](float4 (&rb)[4]) {
    const int64_t m = m_cur;
    const int nn = p_n, oh = p_oh, ow = p_ow;
    wgrad_pix_step(p, m_cur, p_n, p_oh, p_ow);
    const float* xr = reinterpret_cast<const float*>(g_wgrad_zero);
    const int ih = oh * p.stride - p.pad + kh * p.dil;
    const int iw = ow * p.stride - p.pad + kw * p.dil;
    if (m < m_end && kval && static_cast<unsigned>(ih) < static_cast<unsigned>(p.h) &&
        static_cast<unsigned>(iw) < static_cast<unsigned>(p.w))
      xr = p.x + ((static_cast<int64_t>(nn) * p.h + ih) * p.w + iw) * p.cs + ci;
#pragma unroll
    for (int j = 0; j < 4; ++j) rb[j] = *reinterpret_cast<const float4*>(xr + 4 * j);
  };
  // transposed B writes as inline asm as well (a C++ LDS store made hipcc wait vmcnt(0) for the
  // DMA in flight); row 16 lv + 4 j + e: its swizzle depends on 4 j + e only
  const uint32_t bs_w = lds_addr(&Bs[0][0]) + static_cast<uint32_t>(16 * lv * 128 + 4 * (lm & 3));
  auto store = [&](int buf, const float4 (&rb)[4]) {
    const uint32_t base = bs_w + buf * static_cast<uint32_t>(sizeof(Bs[0]));
    // one lane address per swizzle value (0, 1, 4, 5); the row is the instruction's offset
    const uint32_t w[4] = {base + 16u * ((lm >> 2) ^ 0), base + 16u * ((lm >> 2) ^ 1), base + 16u * ((lm >> 2) ^ 4),
                           base + 16u * ((lm >> 2) ^ 5)};
    pre_wr<0>(w, rb[0].x); pre_wr<1>(w, rb[0].y); pre_wr<2>(w, rb[0].z); pre_wr<3>(w, rb[0].w);
    pre_wr<4>(w, rb[1].x); pre_wr<5>(w, rb[1].y); pre_wr<6>(w, rb[1].z); pre_wr<7>(w, rb[1].w);
    pre_wr<8>(w, rb[2].x); pre_wr<9>(w, rb[2].y); pre_wr<10>(w, rb[2].z); pre_wr<11>(w, rb[2].w);
    pre_wr<12>(w, rb[3].x); pre_wr<13>(w, rb[3].y); pre_wr<14>(w, rb[3].z); pre_wr<15>(w, rb[3].w);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15;
  const int fq = lane >> 4;
  // Fragment reads as inline-asm ds_read_b128 with hand-counted lgkmcnt waits: hipcc cannot tell
  // that the LDS-DMA in flight targets the other buffer, and put a vmcnt(0) before the first C++
  // read of the chunk (draining the B loads issued for two chunks ahead).  The swizzles depend on
  // row bits the fragment offsets (16 rows apart) do not change, so one lane address per operand.
  const uint32_t ab_lds = lds_addr(&Ab[0][0]), bs_lds = lds_addr(&Bs[0][0]);
  uint32_t b_lane[2], a_lane;
  {
    const int rb = wcn * 64 + fr;
    b_lane[0] = bs_lds + static_cast<uint32_t>(rb * 128 + 16 * ((2 * fq) ^ pre_swz_b(rb)));
    b_lane[1] = bs_lds + static_cast<uint32_t>(rb * 128 + 16 * ((2 * fq + 1) ^ pre_swz_b(rb)));
    const int ra = wr * 64 + fr;
    a_lane = ab_lds + static_cast<uint32_t>(ra * 64 + 16 * swz64(ra, fq));
  }
  static_assert(sizeof(Bs[0]) == kWTBig * 128 && sizeof(Ab[0]) == 3 * kWTBig * 64, "LDS buffer strides");
  auto compute = [&](int buf) {
    const uint32_t vb0 = b_lane[0] + buf * static_cast<uint32_t>(sizeof(Bs[0]));
    const uint32_t vb1 = b_lane[1] + buf * static_cast<uint32_t>(sizeof(Bs[0]));
    const uint32_t va = a_lane + buf * static_cast<uint32_t>(sizeof(Ab[0]));
    float4 blo[4], bhi[4];
    ds_rd<0>(blo[0], vb0); ds_rd<0>(bhi[0], vb1);
    ds_rd<2048>(blo[1], vb0); ds_rd<2048>(bhi[1], vb1);
    ds_rd<4096>(blo[2], vb0); ds_rd<4096>(bhi[2], vb1);
    ds_rd<6144>(blo[3], vb0); ds_rd<6144>(bhi[3], vb1);
    bf16x8 a[3];
    ds_rd<0>(a[0], va); ds_rd<kWTBig * 64>(a[1], va); ds_rd<2 * kWTBig * 64>(a[2], va);
    // the reads are asm: their results are valid only after the counted wait, and a
    // sched_barrier after each wait keeps the scheduler from hoisting their uses above it
    asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 b[4][3];
#pragma unroll
    for (int f = 0; f < 4; ++f) split3(blo[f], bhi[f], b[f][0], b[f][1], b[f][2]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int fi = 0; fi < 4; ++fi) {
      bf16x8 an[3];
      // the next fragment's three planes (rows 16 apart: +1 KB), read under this one's MFMAs
      switch (fi) {
        case 0: ds_rd<1024>(an[0], va); ds_rd<1024 + kWTBig * 64>(an[1], va); ds_rd<1024 + 2 * kWTBig * 64>(an[2], va); break;
        case 1: ds_rd<2048>(an[0], va); ds_rd<2048 + kWTBig * 64>(an[1], va); ds_rd<2048 + 2 * kWTBig * 64>(an[2], va); break;
        case 2: ds_rd<3072>(an[0], va); ds_rd<3072 + kWTBig * 64>(an[1], va); ds_rd<3072 + 2 * kWTBig * 64>(an[2], va); break;
        default: break;
      }
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) mfma_x6(acc[fi][fj], a, b[fj]);
      if (fi < 3) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        a[0] = an[0];
        a[1] = an[1];
        a[2] = an[2];
      }
    }
  };

  // Chunk c computes from buffers c & 1.  At the start of its phase the B registers of chunk c + 1
  // (loaded during the previous phase) are written to the other buffer, chunk c + 1's A DMA goes to
  // it as well, then chunk c + 2's B loads are issued into the same registers -- so hipcc's wait for
  // those registers (it cannot count LDS-DMA and waits vmcnt(0)) drains nothing else.  The phase
  // ends with vmcnt(4) (the DMA landed, the four B loads stay in flight across the barrier) +
  // lgkmcnt(0) + s_barrier.  Compiler barriers keep the DMA ahead of the B loads in issue order.
  float4 rb[4];
  dma_a(0, m_begin);
  load(rb);                                        // chunk 0
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  store(0, rb);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  load(rb);                                        // chunk 1
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  int cur = 0;
  for (int64_t mc = m_begin; mc < m_end; mc += kWM, cur ^= 1) {
    store(cur ^ 1, rb);                            // chunk c + 1 (zeros past the split, never read)
    if (mc + kWM < m_end) dma_a(cur ^ 1, mc + kWM);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    load(rb);                                      // chunk c + 2 (the zero page past the split)
    __builtin_amdgcn_sched_barrier(0);
    compute(cur);
    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  float* out = p.ws + static_cast<int64_t>(blockIdx.z) * p.cout * p.K;
#pragma unroll
  for (int fi = 0; fi < 4; ++fi)
#pragma unroll
    for (int fj = 0; fj < 4; ++fj) {
      const int k = kc0 + wcn * 64 + fj * 16 + fr;
      if (k >= p.K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = co0 + wr * 64 + fi * 16 + 4 * fq + r;
        if (c < p.cout) out[static_cast<int64_t>(c) * p.K + k] = acc[fi][fj][r];
      }
    }
}

// ---- fp32x weight gradient of the small-cout convs (cout <= 32: stem, layer1, layer2) ----------
// The 64 x 64 tile left 3/4 of its rows idle at cout 16, and the stem's 8-channel input stride left
// 5/8 of its k columns zero (cin 3): 474 us for 20 GFLOP of the fine-tune step.  Here the MFMA
// operands come straight from global memory into registers -- no LDS, no barriers: lane (fr, fq)
// loads dy[m][16 fm + fr] and x[pix(m, tap)][ci] of its 8 pixels m = m0 + 8 fq + j, as the
// 16x16x32 bf16 A / B layouts ask -- and the k columns are the dense (tap, ci < cin) pairs only
// (147 at the stem instead of 392).  Each wave owns FN 16-column fragments and a contiguous range of
// 32-pixel chunks (one output row segment each: wo % 32 == 0) and writes its own partial sums,
// reduced in split order by wgrad_reduce*_kernel; same split3 and six-product order per
// accumulator as wgrad_kernel<64, true>.
constexpr int kDirFN = 4;
static bool wgrad_direct_ok(const drnmi_wgrad_args& a) {
  return a.cout <= 32 && a.wo % 32 == 0 && a.ks * a.ks * a.cin <= 4096;
}
static int wgrad_direct_tiles(const drnmi_wgrad_args& a) {
  return (a.ks * a.ks * a.cin + 16 * kDirFN - 1) / (16 * kDirFN);
}
// wave splits: ~2048 waves in all (8 per CU), whole workgroups of 4, <= one chunk per wave
static int wgrad_direct_splits(const drnmi_wgrad_args& a) {
  const int64_t chunks = static_cast<int64_t>(a.n) * a.ho * a.wo / 32;
  int64_t s = 2048 / wgrad_direct_tiles(a);
  if (s > chunks) s = chunks;
  s = (s + 3) / 4 * 4;
  return static_cast<int>(s < 4 ? 4 : s);
}

template <int FM>
__global__ void __launch_bounds__(kThreads) wgrad_x6_direct_kernel(const WgradP p, int cin) {
  const int lane = threadIdx.x & 63;
  const int z = blockIdx.y * 4 + (threadIdx.x >> 6);        // this wave's split
  const int nz = gridDim.y * 4;
  const int fr = lane & 15, fq = lane >> 4;
  const int hw = p.ho * p.wo;
  const int chunks = static_cast<int>(p.M / 32);
  const int c_begin = static_cast<int>(static_cast<int64_t>(chunks) * z / nz);
  const int c_end = static_cast<int>(static_cast<int64_t>(chunks) * (z + 1) / nz);
  const int kdense = p.ks * p.ks * cin;
  // the lane's B column of each fragment: dense column kv -> (tap, ci) -> tap offsets
  int b_dh[kDirFN], b_dw[kDirFN], b_ci[kDirFN];
  bool b_ok[kDirFN];
#pragma unroll
  for (int f = 0; f < kDirFN; ++f) {
    const int kv = (blockIdx.x * kDirFN + f) * 16 + fr;
    b_ok[f] = kv < kdense;
    const int tap = b_ok[f] ? kv / cin : 0;
    b_ci[f] = b_ok[f] ? kv - tap * cin : 0;
    const int kh = tap / p.ks;
    b_dh[f] = kh * p.dil - p.pad;
    b_dw[f] = (tap - kh * p.ks) * p.dil - p.pad;
  }
  f32x4 acc[FM][kDirFN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < kDirFN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = c_begin; c < c_end; ++c) {
    const int m0 = c * 32;
    const int n = m0 / hw;
    const int q = m0 - n * hw;
    const int oh = q / p.wo;
    const int ow = q - oh * p.wo + 8 * fq;                 // the lane's first pixel (same row)
    const int64_t mrow = static_cast<int64_t>(m0 + 8 * fq) * p.dys;
    float av[FM][8], bv[kDirFN][8];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      const int co = 16 * fm + fr;
#pragma unroll
      for (int j = 0; j < 8; ++j) av[fm][j] = co < p.cout ? p.dy[mrow + static_cast<int64_t>(j) * p.dys + co] : 0.f;
    }
#pragma unroll
    for (int f = 0; f < kDirFN; ++f) {
      const int ih = oh * p.stride + b_dh[f];
      const bool row_ok = b_ok[f] && static_cast<unsigned>(ih) < static_cast<unsigned>(p.h);
      const float* xr = p.x + (static_cast<int64_t>(n) * p.h + (row_ok ? ih : 0)) * p.w * p.cs + b_ci[f];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int iw = (ow + j) * p.stride + b_dw[f];
        bv[f][j] = row_ok && static_cast<unsigned>(iw) < static_cast<unsigned>(p.w) ? xr[static_cast<int64_t>(iw) * p.cs] : 0.f;
      }
    }
    bf16x8 b[kDirFN][3];
#pragma unroll
    for (int f = 0; f < kDirFN; ++f)
      split3(make_float4(bv[f][0], bv[f][1], bv[f][2], bv[f][3]), make_float4(bv[f][4], bv[f][5], bv[f][6], bv[f][7]),
             b[f][0], b[f][1], b[f][2]);
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      bf16x8 a[3];
      split3(make_float4(av[fm][0], av[fm][1], av[fm][2], av[fm][3]),
             make_float4(av[fm][4], av[fm][5], av[fm][6], av[fm][7]), a[0], a[1], a[2]);
#pragma unroll
      for (int f = 0; f < kDirFN; ++f) mfma_x6(acc[fm][f], a, b[f]);
    }
  }
  // C[row = 16 fm + 4 fq + r][col = 16 f + fr] -> ws[z][co][tap * cs + ci] (the reduce skips ci >= cin)
  float* out = p.ws + static_cast<int64_t>(z) * p.cout * p.K;
#pragma unroll
  for (int f = 0; f < kDirFN; ++f) {
    if (!b_ok[f]) continue;
    const int kv = (blockIdx.x * kDirFN + f) * 16 + fr;
    const int tap = kv / cin;
    const int k = tap * p.cs + (kv - tap * cin);
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = 16 * fm + 4 * fq + r;
        if (co < p.cout) out[static_cast<int64_t>(co) * p.K + k] = acc[fm][f][r];
      }
  }
}

// dw[co][ci][kh][kw] (+)= sum_z ws[z][co][(kh*ks + kw)*cs + ci]
__global__ void __launch_bounds__(kThreads)
wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int cout, int cin, int cs, int ks, int K,
                    float* __restrict__ dw, int acc) {
  // threads walk the partials' own [co][k] order (k = tap * cs + ci), so each of the `splits`
  // reads is coalesced (walking dw's OIHW order read them ks*ks*... apart); dw is written once
  const int64_t total = static_cast<int64_t>(cout) * K;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int co = static_cast<int>(i / K);
    const int k = static_cast<int>(i - static_cast<int64_t>(co) * K);
    const int tap = k / cs;
    const int ci = k - tap * cs;
    if (ci >= cin) continue;
    // eight splits' loads in flight at a time, summed in split order (one load per add serialised
    // the chain on its latency)
    float s = 0.f;
    const int64_t zs = static_cast<int64_t>(cout) * K;
    int z = 0;
    for (; z + 8 <= splits; z += 8) {
      float a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = ws[(z + u) * zs + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += a[u];
    }
    for (; z < splits; ++z) s += ws[z * zs + i];
    const int64_t o = (static_cast<int64_t>(co) * cin + ci) * ks * ks + tap;   // tap = kh * ks + kw
    dw[o] = acc ? dw[o] + s : s;
  }
}

// Few outputs over many splits (the stem's 16 x 392 partials over 432 splits): one thread per
// output walked its splits as a chain of dependent loads on 18 workgroups (125 us).  Here 8
// threads share an output, each sums a contiguous eighth of the splits (8 loads in flight), and
// the eighths are added in order: a fixed order, so dw stays bit-reproducible.
constexpr int kRedOut = 32;
constexpr int kRedGrp = kThreads / kRedOut;

__global__ void __launch_bounds__(kThreads)
wgrad_reduce_grouped_kernel(const float* __restrict__ ws, int splits, int cout, int cin, int cs, int ks, int K,
                            float* __restrict__ dw, int acc) {
  __shared__ float part[kRedGrp][kRedOut];
  const int t = threadIdx.x;
  const int oi = t % kRedOut, g = t / kRedOut;
  const int64_t total = static_cast<int64_t>(cout) * K;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kRedOut + oi;
  const int z0 = static_cast<int>(static_cast<int64_t>(splits) * g / kRedGrp);
  const int z1 = static_cast<int>(static_cast<int64_t>(splits) * (g + 1) / kRedGrp);
  float s = 0.f;
  if (i < total) {
    const float* p = ws + i;
#pragma unroll 8
    for (int z = z0; z < z1; ++z) s += p[static_cast<int64_t>(z) * total];
  }
  part[g][oi] = s;
  __syncthreads();
  if (g != 0 || i >= total) return;
  const int co = static_cast<int>(i / K);
  const int k = static_cast<int>(i - static_cast<int64_t>(co) * K);
  const int tap = k / cs;
  const int ci = k - tap * cs;
  if (ci >= cin) return;
  float v = part[0][oi];
#pragma unroll
  for (int j = 1; j < kRedGrp; ++j) v += part[j][oi];
  const int64_t o = (static_cast<int64_t>(co) * cin + ci) * ks * ks + tap;
  dw[o] = acc ? dw[o] + v : v;
}

// ------------------------------------------------------------------ host: plan, layout, route
static bool wgrad_big_ok(const drnmi_wgrad_args& a) {
  const int K = a.ks * a.ks * a.cin_stride;
  return a.cout >= kWTBig && K >= kWTBig && a.cin_stride % 16 == 0;
}
// the dy split pass costs ~10 B of HBM per dy element against 2 K flops per element of the tile:
// it pays where K >= 1024 (layer7.0: 3.78 -> 2.72 ms; a 1x1 256 -> 1024 wgrad: 128 -> 234 us)
static bool wgrad_pre_ok(const drnmi_wgrad_args& a) {
  return wgrad_big_ok(a) && a.ks * a.ks * a.cin_stride >= 1024;
}

// The pixel range is split so that the launch fills the chip: at least two rounds of the resident
// workgroup slots, and among lo .. 4 lo splits the count whose last round is fullest (the first
// rule alone put D-54 layer7.0's 576 big tiles on 512 slots at one split: 1.125 rounds, the
// second round 1/8 full, 4.6 ms of a 52.8 ms fine-tune step).  Every split holds >= 512 pixels.
struct WgradSplit {
  int splits;
  int64_t per;           // pixels per split, whole 32-pixel chunks
};
static WgradSplit wgrad_plan(const drnmi_wgrad_args& a, int tile) {
  const int K = a.ks * a.ks * a.cin_stride;
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  }
  const int64_t slots = (tile == kWTBig ? 2 : 4) * static_cast<int64_t>(cus);   // resident workgroups: LDS 73.7 / 36.9 KB
  const int64_t M = static_cast<int64_t>(a.n) * a.ho * a.wo;
  const int64_t tiles = static_cast<int64_t>((a.cout + tile - 1) / tile) * ((K + tile - 1) / tile);
  int64_t smax = (M + 511) / 512;
  if (smax > 512) smax = 512;
  if (smax < 1) smax = 1;
  int64_t lo = (2 * slots + tiles - 1) / tiles;
  if (lo > smax) lo = smax;
  int64_t hi = 4 * lo < smax ? 4 * lo : smax;
  WgradSplit best{0, 0};
  double best_eff = -1.0;
  for (int64_t s = lo; s <= hi; ++s) {
    int64_t pp = (M + s - 1) / s;
    pp = (pp + kWM - 1) / kWM * kWM;
    const int64_t sa = (M + pp - 1) / pp;
    const int64_t wgs = tiles * sa;
    const int64_t rounds = (wgs + slots - 1) / slots;
    const double eff = static_cast<double>(wgs) / static_cast<double>(rounds * slots);
    if (eff > best_eff + 0.02) {     // a larger split count only for a clearly fuller last round
      best_eff = eff;
      best = WgradSplit{static_cast<int>(sa), pp};
    }
  }
  return best;
}

// The workspace of one geometry, whichever kernel runs on it: the partials [splits][cout][K] fp32,
// then (128-tile geometries with K >= 1024) the dy planes [3][Cp][Mp] bf16 of the pre kernel.
// `splits` sizes the partials for the largest of the 64-tile plan, the 128-tile plan and the direct
// kernel's wave splits, so the planes start at one offset for every route; the size queries, the
// route and the launch all read this one value.
struct WgradLayout {
  WgradSplit t64, t128;      // t128.splits = 0 where the 128-tile does not apply
  int direct_splits;         // 0 where the direct kernel does not apply
  int splits;
  int64_t partials_bytes;    // = the offset of the dy planes
  int64_t Mp;                // dy planes: pixels and rows padded to whole chunks / tiles
  int Cp;
  int64_t planes_bytes;      // 0 where the pre kernel does not apply
};
static int64_t wgrad_partials_bytes(const drnmi_wgrad_args& a, int splits) {
  return (static_cast<int64_t>(splits) * a.cout * a.ks * a.ks * a.cin_stride * 4 + 255) / 256 * 256;
}
static WgradLayout wgrad_layout(const drnmi_wgrad_args& a) {
  WgradLayout l{};
  l.t64 = wgrad_plan(a, kWT);
  if (wgrad_big_ok(a)) l.t128 = wgrad_plan(a, kWTBig);
  if (wgrad_direct_ok(a)) l.direct_splits = wgrad_direct_splits(a);
  l.splits = l.t64.splits;
  if (l.t128.splits > l.splits) l.splits = l.t128.splits;
  if (l.direct_splits > l.splits) l.splits = l.direct_splits;
  l.partials_bytes = wgrad_partials_bytes(a, l.splits);
  const int64_t M = static_cast<int64_t>(a.n) * a.ho * a.wo;
  l.Mp = (M + kWM - 1) / kWM * kWM;
  l.Cp = (a.cout + kWTBig - 1) / kWTBig * kWTBig;
  if (wgrad_pre_ok(a)) l.planes_bytes = 3 * l.Cp * l.Mp * 2;
  return l;
}

// The one launch decision of a weight gradient: wgrad_launch runs it and drnmi_conv_wgrad_plan
// reports it.  kernel: DRNMI_WGRAD_* (include/drnmi.h).
struct WgradRoute {
  int kernel;
  int splits;
  int64_t per;
  int reduce;        // 0 wgrad_reduce_kernel, 1 wgrad_reduce_grouped_kernel
};
static WgradRoute wgrad_route(const drnmi_wgrad_args& a, bool x6, const WgradLayout& l) {
  WgradRoute r{};
  const bool big = x6 && l.t128.splits > 0;
  const WgradSplit& s = big ? l.t128 : l.t64;
  r.splits = s.splits;
  r.per = s.per;
  if (x6 && !big && l.direct_splits > 0) {
    r.kernel = DRNMI_WGRAD_DIRECT;
    r.splits = l.direct_splits;
  } else if (big) {
    r.kernel = l.planes_bytes > 0 ? DRNMI_WGRAD_PRE : DRNMI_WGRAD_BIG;
  } else {
    r.kernel = x6 ? DRNMI_WGRAD_X6 : DRNMI_WGRAD_F32;
  }
  const int64_t total = static_cast<int64_t>(a.cout) * a.ks * a.ks * a.cin_stride;
  // the grouped form where one thread per output would leave the chip mostly idle on a long chain
  r.reduce = (r.splits >= 4 * kRedGrp && total <= 2048 * kThreads) ? 1 : 0;
  return r;
}

}  // namespace
}  // namespace drnmi

using namespace drnmi;

static int wgrad_check(const drnmi_wgrad_args* a) {
  if (a == nullptr) return DRNMI_EINVAL;
  if (a->n <= 0 || a->h <= 0 || a->w <= 0 || a->ho <= 0 || a->wo <= 0 || a->cout <= 0 || a->cin <= 0) return DRNMI_EINVAL;
  if (a->cin_stride < 8 || (a->cin_stride & (a->cin_stride - 1)) != 0 || a->cin > a->cin_stride) return DRNMI_EINVAL;
  if (a->dy_stride < a->cout || a->ks <= 0 || a->stride <= 0 || a->dil <= 0 || a->pad < 0) return DRNMI_EINVAL;
  if (a->ho != (a->h + 2 * a->pad - a->dil * (a->ks - 1) - 1) / a->stride + 1 ||
      a->wo != (a->w + 2 * a->pad - a->dil * (a->ks - 1) - 1) / a->stride + 1)
    return DRNMI_EINVAL;
  // pixel indices are int32 inside the kernels (m_cur, m / hw)
  if (static_cast<int64_t>(a->n) * a->ho * a->wo >= (int64_t(1) << 31)) return DRNMI_EINVAL;
  return DRNMI_OK;
}

// the exact-f32 kernel's own partials (the f32x3 query below holds every plan and the dy planes)
extern "C" int64_t drnmi_conv_wgrad_f32_workspace_bytes(const drnmi_wgrad_args* a) {
  if (wgrad_check(a) != DRNMI_OK) return -1;
  return wgrad_partials_bytes(*a, wgrad_layout(*a).t64.splits);
}

// room for either arithmetic (f32 or f32x3)
extern "C" int64_t drnmi_conv_wgrad_workspace_bytes(const drnmi_wgrad_args* a) {
  if (wgrad_check(a) != DRNMI_OK) return -1;
  const WgradLayout l = wgrad_layout(*a);
  return l.partials_bytes + l.planes_bytes;
}

extern "C" int drnmi_conv_wgrad_plan(const drnmi_wgrad_args* a, int32_t x6, int32_t* kernel, int32_t* splits,
                                     int64_t* pix_per_split, int32_t* reduce) {
  const int rc = wgrad_check(a);
  if (rc != DRNMI_OK) return rc;
  const WgradRoute r = wgrad_route(*a, x6 != 0, wgrad_layout(*a));
  if (kernel != nullptr) *kernel = r.kernel;
  if (splits != nullptr) *splits = r.splits;
  if (pix_per_split != nullptr) *pix_per_split = r.per;
  if (reduce != nullptr) *reduce = r.reduce;
  return DRNMI_OK;
}

static int wgrad_launch(const drnmi_wgrad_args* a, bool x6, void* stream) {
  const int rc = wgrad_check(a);
  if (rc != DRNMI_OK) return rc;
  if (a->dy == nullptr || a->x == nullptr || a->dw == nullptr || a->ws == nullptr) return DRNMI_EINVAL;
  const WgradLayout l = wgrad_layout(*a);
  if (a->ws_bytes < (x6 ? l.partials_bytes + l.planes_bytes : wgrad_partials_bytes(*a, l.t64.splits))) return DRNMI_EINVAL;
  // 16-B loads of dy / x; the dy bf16 planes in ws are LDS-DMA'd and stored as 16-B pieces
  if ((reinterpret_cast<uintptr_t>(a->dy) | reinterpret_cast<uintptr_t>(a->x) | reinterpret_cast<uintptr_t>(a->ws)) & 15)
    return DRNMI_EINVAL;
  if (a->dy_stride % 4 != 0) return DRNMI_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  WgradP p{};
  p.dy = a->dy;
  p.x = a->x;
  p.ws = reinterpret_cast<float*>(a->ws);
  p.dys = a->dy_stride;
  p.cout = a->cout;
  p.n = a->n; p.h = a->h; p.w = a->w; p.cs = a->cin_stride;
  p.ho = a->ho; p.wo = a->wo; p.ks = a->ks; p.stride = a->stride; p.pad = a->pad; p.dil = a->dil;
  p.K = a->ks * a->ks * a->cin_stride;
  p.M = static_cast<int64_t>(a->n) * a->ho * a->wo;
  const WgradRoute r = wgrad_route(*a, x6, l);
  const int splits = r.splits;
  p.pix_per_split = r.per;
  const dim3 grid((p.K + kWT - 1) / kWT, (a->cout + kWT - 1) / kWT, splits);
  const dim3 g2((p.K + kWTBig - 1) / kWTBig, (a->cout + kWTBig - 1) / kWTBig, splits);
  if (r.kernel == DRNMI_WGRAD_DIRECT) {
    const dim3 gd(static_cast<unsigned>(wgrad_direct_tiles(*a)), static_cast<unsigned>(splits / 4));
    if (a->cout <= 16) hipLaunchKernelGGL(wgrad_x6_direct_kernel<1>, gd, dim3(kThreads), 0, s, p, a->cin);
    else hipLaunchKernelGGL(wgrad_x6_direct_kernel<2>, gd, dim3(kThreads), 0, s, p, a->cin);
  } else if (r.kernel == DRNMI_WGRAD_PRE) {
    WgradPreP q{};
    q.p = p;
    q.Mp = l.Mp;
    q.Cp = l.Cp;
    bf16_t* dyt = reinterpret_cast<bf16_t*>(reinterpret_cast<char*>(a->ws) + l.partials_bytes);
    q.dyt = dyt;
    const int64_t blocks = (q.Mp / 32) * (q.Cp / 64);
    hipLaunchKernelGGL(wgrad_dy_split_kernel, dim3(static_cast<unsigned>(blocks < 8192 ? blocks : 8192)), dim3(kThreads),
                       0, s, a->dy, a->dy_stride, a->cout, p.M, q.Mp, q.Cp, dyt);
    hipLaunchKernelGGL(wgrad_x6_pre_kernel, g2, dim3(kThreads), 0, s, q);
  } else if (r.kernel == DRNMI_WGRAD_BIG) {
    hipLaunchKernelGGL((wgrad_kernel<kWTBig, true>), g2, dim3(kThreads), 0, s, p);
  } else if (r.kernel == DRNMI_WGRAD_X6) {
    hipLaunchKernelGGL((wgrad_kernel<kWT, true>), grid, dim3(kThreads), 0, s, p);
  } else {
    hipLaunchKernelGGL((wgrad_kernel<kWT, false>), grid, dim3(kThreads), 0, s, p);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  const int64_t total = static_cast<int64_t>(a->cout) * p.K;
  if (r.reduce)
    hipLaunchKernelGGL(wgrad_reduce_grouped_kernel, dim3(static_cast<unsigned>((total + kRedOut - 1) / kRedOut)),
                       dim3(kThreads), 0, s, p.ws, splits, a->cout, a->cin, a->cin_stride, a->ks, p.K, a->dw,
                       a->accumulate);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_of(total)), dim3(kThreads), 0, s, p.ws, splits, a->cout, a->cin,
                       a->cin_stride, a->ks, p.K, a->dw, a->accumulate);
  return static_cast<int>(hipGetLastError());
}

extern "C" int drnmi_conv_wgrad_f32(const drnmi_wgrad_args* a, void* stream) { return wgrad_launch(a, false, stream); }
extern "C" int drnmi_conv_wgrad_f32x3(const drnmi_wgrad_args* a, void* stream) { return wgrad_launch(a, true, stream); }
