// The fp32x2 weight gradient (drnmi_conv_wgrad_f32x2): wgrad.hip's pre pipeline on two planes and three
// products.  Its own translation unit: built with one fp32 operation per instruction (drnmi/build.py).
#include "wgrad.h"

namespace drnmi {
namespace {

__device__ float4 g_wgrad_x3_zero[4];   // zero-initialised: the B source outside the image

// ---- fp32x2 weight gradient: the pre pipeline on two planes and three products ------------------
// drnmi_conv_wgrad_f32x2's form of wgrad.hip's wgrad_dy_split_kernel and wgrad_x6_pre_kernel (the K >= 1024 launches): dy is split once
// into two transposed bf16 planes [2][Cp][Mp] (common.h split2), the tile stages them by LDS-DMA (16
// 1-KB pieces per chunk instead of 24, 64 KB of LDS instead of 80), splits x in registers with split2
// and runs mfma_x3 per accumulator: half the MFMAs of wgrad_x6_pre_kernel per chunk on the same ring
// (pixel walk, B staging, vmcnt(4) phase end).  The other routes keep six products under fp32x2.
__global__ void __launch_bounds__(kThreads)
wgrad_dy_split2_kernel(const float* __restrict__ dy, int dys, int cout, int64_t M, int64_t Mp, int Cp,
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
    bf16x8 h1, h2;
    split2(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), h1, h2);
    bf16_t* o = out + static_cast<int64_t>(co) * Mp + m0;
    *reinterpret_cast<bf16x8*>(o) = h1;
    *reinterpret_cast<bf16x8*>(o + pstride) = h2;
  }
}

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) wgrad_x3_pre_kernel(const WgradPreP q) {
  const WgradP& p = q.p;
  // A: [buf][2 planes][128 rows][64 B] bf16, B: [buf][128 rows][32 floats]: 2 x (16 + 16) KB
  __shared__ __attribute__((aligned(16))) char Ab[2][2 * kWTBig * 64];
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

  // A DMA: 16 pieces of 1 KB per chunk, 4 per wave; piece gi = plane * 8 + 16-row block
  const int64_t plane_stride = static_cast<int64_t>(q.Cp) * q.Mp;
  const bf16_t* a_base = q.dyt + static_cast<int64_t>(co0) * q.Mp;
  int32_t a_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gi = wave * 4 + i;
    const int pl = gi >> 3;
    const int r = (gi & 7) * 16 + (lane >> 2);
    const int c = swz64(r, lane & 3);
    a_off[i] = static_cast<int32_t>(pl * plane_stride + static_cast<int64_t>(r) * q.Mp + 8 * c);
  }
  // as inline asm: hipcc models the LDS-DMA builtin's address registers as pending until vmcnt(0)
  // and drained the B loads in flight the first time it reused one
  const uint32_t a_dst = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(lds_addr(&Ab[0][wave * 4 * 1024]))));
  auto dma_a = [&](int buf, int64_t m) {
    const bf16_t* src = a_base + m;
#pragma unroll
    for (int i = 0; i < 4; ++i) dma16(src + a_off[i], a_dst + buf * static_cast<uint32_t>(sizeof(Ab[0])) + i * 1024);
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
    const float* xr = reinterpret_cast<const float*>(g_wgrad_x3_zero);
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
  static_assert(sizeof(Bs[0]) == kWTBig * 128 && sizeof(Ab[0]) == 2 * kWTBig * 64, "LDS buffer strides");
  auto compute = [&](int buf) {
    const uint32_t vb0 = b_lane[0] + buf * static_cast<uint32_t>(sizeof(Bs[0]));
    const uint32_t vb1 = b_lane[1] + buf * static_cast<uint32_t>(sizeof(Bs[0]));
    const uint32_t va = a_lane + buf * static_cast<uint32_t>(sizeof(Ab[0]));
    float4 blo[4], bhi[4];
    ds_rd<0>(blo[0], vb0); ds_rd<0>(bhi[0], vb1);
    ds_rd<2048>(blo[1], vb0); ds_rd<2048>(bhi[1], vb1);
    ds_rd<4096>(blo[2], vb0); ds_rd<4096>(bhi[2], vb1);
    ds_rd<6144>(blo[3], vb0); ds_rd<6144>(bhi[3], vb1);
    bf16x8 a[2];
    ds_rd<0>(a[0], va); ds_rd<kWTBig * 64>(a[1], va);
    // the reads are asm: their results are valid only after the counted wait, and a
    // sched_barrier after each wait keeps the scheduler from hoisting their uses above it
    asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 b[4][2];
#pragma unroll
    for (int f = 0; f < 4; ++f) split2(blo[f], bhi[f], b[f][0], b[f][1]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int fi = 0; fi < 4; ++fi) {
      bf16x8 an[2];
      // the next fragment's two planes (rows 16 apart: +1 KB), read under this one's MFMAs
      switch (fi) {
        case 0: ds_rd<1024>(an[0], va); ds_rd<1024 + kWTBig * 64>(an[1], va); break;
        case 1: ds_rd<2048>(an[0], va); ds_rd<2048 + kWTBig * 64>(an[1], va); break;
        case 2: ds_rd<3072>(an[0], va); ds_rd<3072 + kWTBig * 64>(an[1], va); break;
        default: break;
      }
#pragma unroll
      for (int fj = 0; fj < 4; ++fj) mfma_x3(acc[fi][fj], a, b[fj]);
      if (fi < 3) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        a[0] = an[0];
        a[1] = an[1];
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

}  // namespace

void launch_wgrad_x3_pre(const void* pre_params, const float* dy, dim3 split_grid, dim3 grid, hipStream_t s) {
  const WgradPreP& q = *static_cast<const WgradPreP*>(pre_params);
  hipLaunchKernelGGL(wgrad_dy_split2_kernel, split_grid, dim3(kThreads), 0, s, dy, q.p.dys, q.p.cout, q.p.M, q.Mp, q.Cp,
                     const_cast<bf16_t*>(q.dyt));
  hipLaunchKernelGGL(wgrad_x3_pre_kernel, grid, dim3(kThreads), 0, s, q);
}

}  // namespace drnmi
