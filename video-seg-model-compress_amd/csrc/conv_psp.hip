// Period-sparse NHWC implicit-GEMM convolution (dtype DRNMI_BF16_PSP, include/drnmi.h: bf16 inference, opt-in
// through DRNSeg.set_srmb_sparse) for weights masked by SRMBRepMasker: the MFMAs run on the live input
// channels only, 1 / (1 - isp) fewer of them than the dense tiles issue.
//
// What the mask gives (drnmi_psp_pack checks it on the weights' zeros, nothing is taken on trust):
//   classes  output rows fall into classes with one zero support each; every class has a multiple of 16 rows,
//            so after a row permutation every 16-row MFMA fragment holds rows of one class;
//   periods  for a (class, tap) the live input channels repeat with period P (32 / 64), d (16 / 8) of them
//            per period, one per residue mod d: live channel v of period q is q P + v + d s_v with
//            s_v in 0 .. G - 1, G = P / d (2, 4 or 8: the MFMA saving).
// Weights are stored compacted, [row][tap][cin / G] (element q d + v of a tap = channel q P + v + d s_v), in
// permuted row order.  v_mfma_f32_16x16x32_bf16, fp32 accumulation; ks 1 / 3, stride 1, any dilation.
//
// Tile: 128 (permuted) output rows x 128 pixels, four waves of 32 pixels x all 128 rows (FM 8, FN 2): a wave
// owns every class of the tile, so what it reads of the pixels is reused by all of them.
// K step = 32 compacted elements of one tap = S = 32 G source channels; steps run tap-major (kt = tap ncb + cb)
// on a two-stage ring filled by LDS DMA (global_load_lds, conv_tile.h glds16), one barrier per step.
// LDS image of a stage:
//   A   128 rows x 64 B of compacted weights, 16-B chunk c of row r at slot swzb<64>(r, c) (conv_big's BK-32 read);
//   B   128 pixel rows x 2 S B in SOURCE channel order, staged once and shared by all classes; chunk c of row
//       r at slot c ^ swz(r) (swz: (r >> 1) & 7 for 128-B rows, r & 15 for 256- / 512-B rows).
// Per step a lane (fr, fq) -- MFMA k slots 8 fq .. 8 fq + 7, i.e. period ql = 8 fq / d, residues vb = 8 fq % d
// .. + 7 -- reads for each of its two pixel fragments the G candidate chunks (channels ql P + vb + d s .. + 7,
// s = 0 .. G - 1) into registers ONCE: 2 G ds_read_b128.  For each of the 8 fragments it then forms the
// compacted B fragment from those registers: dword t = (element 2 t from candidate s_{vb + 2 t}, element
// 2 t + 1 from candidate s_{vb + 2 t + 1}) = OR over candidate pairs i of v_perm_b32(R[2 i + 1], R[2 i], sel_i)
// with zero-filling selector bytes for the halves the pair does not supply: G / 2 v_perm_b32 and G / 2 - 1 ORs
// per dword, one MFMA where the dense tile issues G.  The selectors depend on (fragment, tap, fq's half of a
// 16-residue period) only; the workgroup builds them once from the blob's s table into LDS
// ([fragment][tap][half][pair] x 16 B) and a lane reads G / 2 x 16 B of them per fragment and step.
// Epilogue: the accumulators go through LDS ([pixel][132] fp32); a thread then takes 8 positions that are
// consecutive in TRUE channel order (the blob's per-tile `order`), adds shift[channel] and the residual,
// applies ReLU and writes one 16-B piece of the NHWC row where the 8 channels are one aligned run (always so
// when the tile's classes are 8 consecutive residues), element stores otherwise and for fp32 / strided outputs.
// No scalar memory writes anywhere: the tables are read-only and LDS is written by vector stores and DMA.
//
// The blob (drnmi_psp_pack; private to this file and the unpacking test): 16 int32 of header {magic, rows, cin,
// ks, P, d, G, kc = ks ks cin / G, 0...}, int32 perm[rows] (position -> true channel), int32 order[rows] (per
// 128-row tile, its positions sorted by true channel), uint8 s[rows / 16][ks ks][d] padded to 16 B, then the
// bf16 values [rows][kc].
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "conv_tile.h"
#include "kernels.h"

namespace drnmi {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kPspMagic = 0x31505350;     // "PSP1"
constexpr int kPspHeader = 64;
constexpr int kPspBCO = 128, kPspBPX = 128;
// tile id (enum drnmi_psp_tile) -> period and live channels per period
constexpr int kPspP[4] = {32, 64, 64, 32};
constexpr int kPspD[4] = {16, 16, 8, 8};

constexpr int64_t psp_s_bytes(int rows, int ks, int d) { return (static_cast<int64_t>(rows / 16) * ks * ks * d + 15) / 16 * 16; }
constexpr int64_t psp_vals_off(int rows, int ks, int d) { return kPspHeader + 8 * static_cast<int64_t>(rows) + psp_s_bytes(rows, ks, d); }

template <int KS, int G>
struct PspCfg {
  static constexpr int TAPS = KS * KS;
  static constexpr int S = 32 * G;                  // source channels per K step
  static constexpr int ROWB = 2 * S;                // bytes of a pixel row
  static constexpr int CPR = ROWB / 16;             // 16-B chunks per pixel row
  static constexpr int RPI = 1024 / ROWB;           // pixel rows per 1-KB DMA piece
  static constexpr int NW = 4, THREADS = 256, FM = 8, FN = 2;
  static constexpr int A_BYTES = kPspBCO * 64;
  static constexpr int B_BYTES = kPspBPX * ROWB;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  static constexpr int A_INSTR = A_BYTES / 1024 / NW;
  static constexpr int B_INSTR = B_BYTES / 1024 / NW;
  static constexpr int SEL_BYTES = FM * TAPS * 2 * (G / 2) * 16;
  static constexpr int EPI_LD = kPspBCO + 4;        // floats per pixel row of the epilogue image
  static constexpr int EPI_BYTES = kPspBPX * EPI_LD * 4;
  static constexpr int LDS = SEL_BYTES + (2 * STAGE > EPI_BYTES ? 2 * STAGE : EPI_BYTES);
  static_assert(LDS <= 160 * 1024, "LDS");
};

template <int CPR>
__device__ __forceinline__ int psp_swz(int row) { return CPR == 8 ? (row >> 1) & 7 : row & 15; }

template <int KS, int G, int D>
__global__ void __launch_bounds__(256)
conv_psp_kernel(const drnmi_conv_args p) {
  using C = PspCfg<KS, G>;
  constexpr int P = G * D, TAPS = C::TAPS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sel_lds = smem;
  char* const ring = smem + C::SEL_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int fr = lane & 15;
  const int fq = lane >> 4;
  const int M = p.n * p.ho * p.wo;
  const int hw_o = p.ho * p.wo;
  const int nco = p.cout / kPspBCO;
  const int npx = (M + kPspBPX - 1) / kPspBPX;
  const int tile = xcd_remap2(blockIdx.x, npx * nco);
  const int px0 = (tile / nco) * kPspBPX;
  const int co0 = (tile % nco) * kPspBCO;

  const int cin = p.cin, H = p.h, W = p.w, dil = p.dil;
  const int ncb = cin / C::S;                       // channel blocks per tap
  const int nk = TAPS * ncb;
  const int kc = nk * 32;                           // compacted columns per weight row
  const char* __restrict__ blob = reinterpret_cast<const char*>(p.wgt);
  const int* __restrict__ perm = reinterpret_cast<const int*>(blob + kPspHeader);
  const int* __restrict__ order = perm + p.cout_pad;
  const uint8_t* __restrict__ stab = reinterpret_cast<const uint8_t*>(order + p.cout_pad);
  const uint16_t* __restrict__ vals = reinterpret_cast<const uint16_t*>(blob + psp_vals_off(p.cout_pad, KS, D));
  const uint16_t* __restrict__ x = reinterpret_cast<const uint16_t*>(p.x);

  // --- the selector table: entry (f, tap, half, pair i, dword t) for elements v0 = vb + 2 t, v0 + 1
  for (int e = tid; e < C::SEL_BYTES / 4; e += C::THREADS) {
    const int t = e & 3;
    int r = e >> 2;
    const int i = r % (G / 2);
    r /= G / 2;
    const int half = r & 1;
    r >>= 1;
    const int tap = r % TAPS;
    const int f = r / TAPS;
    const uint8_t* sv = stab + ((co0 / 16 + f) * TAPS + tap) * D + (D == 16 ? 8 * half : 0) + 2 * t;
    const int s0 = sv[0], s1 = sv[1];
    // v_perm_b32(S0 = R[2 i + 1], S1 = R[2 i]): bytes 0-3 of S1, 4-7 of S0, 0x0c = zero
    const uint32_t lo = (s0 >> 1) != i ? 0x0c0cu : (s0 & 1) ? 0x0504u : 0x0100u;
    const uint32_t hi = (s1 >> 1) != i ? 0x0c0cu : (s1 & 1) ? 0x0706u : 0x0302u;
    reinterpret_cast<uint32_t*>(sel_lds)[e] = lo | (hi << 16);
  }

  // --- DMA assignment.  A: lane l fills row l / 4, slot l % 4 of a 16-row piece; pixels: row l / CPR, slot
  // l % CPR of an RPI-row piece
  int a_off[C::A_INSTR];
#pragma unroll
  for (int i = 0; i < C::A_INSTR; ++i) {
    const int r = (wave * C::A_INSTR + i) * 16 + (lane >> 2);
    a_off[i] = (co0 + r) * kc + swzb<64>(r, lane & 3) * 8;
  }
  uint32_t b_hw[C::B_INSTR];
  int b_off[C::B_INSTR];
  const char* zero_src = reinterpret_cast<const char*>(g_zero_page) + lane * 16;
#pragma unroll
  for (int i = 0; i < C::B_INSTR; ++i) {
    const int r = (wave * C::B_INSTR + i) * C::RPI + lane / C::CPR;
    const int m = px0 + r;
    b_hw[i] = 0xC000C000u;                          // a row past M: no tap is inside the image
    b_off[i] = 0;
    if (m < M) {
      const int n = m / hw_o;
      const int q = m - n * hw_o;
      const int oh = q / p.wo;
      const int ow = q - oh * p.wo;
      const int ih0 = oh - p.pad, iw0 = ow - p.pad;
      b_hw[i] = (static_cast<uint32_t>(ih0) << 16) | (static_cast<uint32_t>(iw0) & 0xffffu);
      b_off[i] = ((n * H + ih0) * W + iw0) * cin + ((lane % C::CPR) ^ psp_swz<C::CPR>(r)) * 8;
    }
  }
  auto issue_step = [&](int kt, int stage) {
    const int tap = kt / ncb;
    const int cb = kt - tap * ncb;
    const int dh = (tap / KS) * dil, dw = (tap % KS) * dil;
    const int toff = (dh * W + dw) * cin + cb * C::S;
    char* sa = ring + stage * C::STAGE;
#pragma unroll
    for (int i = 0; i < C::A_INSTR; ++i) glds16(vals + (a_off[i] + kt * 32), sa + (wave * C::A_INSTR + i) * 1024);
#pragma unroll
    for (int i = 0; i < C::B_INSTR; ++i) {
      const int ih0 = static_cast<int>(b_hw[i]) >> 16;
      const int iw0 = static_cast<int16_t>(b_hw[i] & 0xffffu);
      const bool ok = static_cast<unsigned>(ih0 + dh) < static_cast<unsigned>(H) &&
                      static_cast<unsigned>(iw0 + dw) < static_cast<unsigned>(W);
      const void* src = ok ? static_cast<const void*>(x + (b_off[i] + toff)) : static_cast<const void*>(zero_src);
      glds16(src, sa + C::A_BYTES + (wave * C::B_INSTR + i) * 1024);
    }
  };

  // the lane's period and residues inside a K step, and its candidate chunks
  const int ql = (8 * fq) / D, vb = (8 * fq) % D;
  const int half = D == 16 ? (fq & 1) : 0;
  const int chunk0 = (ql * P + vb) / 8;             // candidate s: chunk0 + s D / 8

  f32x4 acc[C::FM][C::FN];
#pragma unroll
  for (int f = 0; f < C::FM; ++f)
#pragma unroll
    for (int fn = 0; fn < C::FN; ++fn) acc[f][fn] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue_step(0, 0);
  for (int t = 0; t < nk; ++t) {
    // step t has landed and every wave is done with the other stage (and, at t = 0, the table is written)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) issue_step(t + 1, (t + 1) & 1);

    const char* sa = ring + (t & 1) * C::STAGE;
    const char* sb = sa + C::A_BYTES;
    const int tap = t / ncb;
    u32x4 R[C::FN][G];
#pragma unroll
    for (int fn = 0; fn < C::FN; ++fn) {
      const int r = wave * 32 + fn * 16 + fr;
      const int z = psp_swz<C::CPR>(r);
#pragma unroll
      for (int s = 0; s < G; ++s)
        R[fn][s] = *reinterpret_cast<const u32x4*>(sb + r * C::ROWB + ((chunk0 + s * (D / 8)) ^ z) * 16);
    }
#pragma unroll
    for (int f = 0; f < C::FM; ++f) {
      const int r = f * 16 + fr;
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(sa + r * 64 + swzb<64>(r, fq) * 16);
      u32x4 sel[G / 2];
#pragma unroll
      for (int i = 0; i < G / 2; ++i)
        sel[i] = *reinterpret_cast<const u32x4*>(sel_lds + (((f * TAPS + tap) * 2 + half) * (G / 2) + i) * 16);
#pragma unroll
      for (int fn = 0; fn < C::FN; ++fn) {
        u32x4 b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t w = __builtin_amdgcn_perm(R[fn][1][j], R[fn][0][j], sel[0][j]);
#pragma unroll
          for (int i = 1; i < G / 2; ++i) w |= __builtin_amdgcn_perm(R[fn][2 * i + 1][j], R[fn][2 * i][j], sel[i][j]);
          b[j] = w;
        }
        acc[f][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf16x8, b), acc[f][fn], 0, 0, 0);
      }
    }
  }

  // --- epilogue through LDS: accumulator layout (rows 4 fq .. + 3 of fragment f, pixel fr) -> [pixel][position]
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  float* epi = reinterpret_cast<float*>(ring);
#pragma unroll
  for (int fn = 0; fn < C::FN; ++fn)
#pragma unroll
    for (int f = 0; f < C::FM; ++f)
      *reinterpret_cast<f32x4*>(epi + (wave * 32 + fn * 16 + fr) * C::EPI_LD + f * 16 + fq * 4) = acc[f][fn];
  __syncthreads();

  // a thread's 8 positions: consecutive in true channel order
  int pos[8], ch[8];
  float sh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    pos[k] = order[co0 + (tid & 15) * 8 + k];
    ch[k] = perm[co0 + pos[k]];
    sh[k] = p.shift[ch[k]];
  }
  const uint16_t* __restrict__ res = reinterpret_cast<const uint16_t*>(p.res);
  const bool run = ch[7] == ch[0] + 7 && (ch[0] & 7) == 0;
  const bool y16 = run && p.out_dtype == DRNMI_BF16 && p.y_sc == 1 && (p.y_sp & 7) == 0 && (p.y_sn & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(p.y) & 15) == 0;
  const bool r16 = run && (p.cout & 7) == 0 && (reinterpret_cast<uintptr_t>(p.res) & 15) == 0;
  const bool relu = p.relu != 0;
#pragma unroll 1
  for (int it = 0; it < kPspBPX / 16; ++it) {
    const int px = it * 16 + (tid >> 4);
    const int m = px0 + px;
    if (m >= M) continue;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = epi[px * C::EPI_LD + pos[k]] + sh[k];
    if (res != nullptr) {
      const uint16_t* rp = res + static_cast<int64_t>(m) * p.cout;
      if (r16) {
        const uint4 rv = *reinterpret_cast<const uint4*>(rp + ch[0]);
        const uint32_t w[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[2 * k] += bf16_to_f32(static_cast<uint16_t>(w[k] & 0xffff));
          v[2 * k + 1] += bf16_to_f32(static_cast<uint16_t>(w[k] >> 16));
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += bf16_to_f32(rp[ch[k]]);
      }
    }
    if (relu) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
    }
    const int n = m / hw_o;
    const int q = m - n * hw_o;
    const int64_t ybase = static_cast<int64_t>(n) * p.y_sn + static_cast<int64_t>(q) * p.y_sp;
    if (y16) {
      uint32_t o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = static_cast<uint32_t>(f32_to_bf16(v[2 * k])) | (static_cast<uint32_t>(f32_to_bf16(v[2 * k + 1])) << 16);
      *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(p.y) + ybase + ch[0]) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t off = ybase + static_cast<int64_t>(ch[k]) * p.y_sc;
        if (p.out_dtype == DRNMI_BF16) reinterpret_cast<uint16_t*>(p.y)[off] = f32_to_bf16(v[k]);
        else reinterpret_cast<float*>(p.y)[off] = v[k];
      }
    }
  }
}

template <int KS, int G, int D>
hipError_t launch_psp(const drnmi_conv_args& p, hipStream_t s) {
  using C = PspCfg<KS, G>;
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int64_t blocks = ((M + kPspBPX - 1) / kPspBPX) * (p.cout / kPspBCO);
  return launch_lds<&conv_psp_kernel<KS, G, D>>(dim3(static_cast<unsigned>(blocks)), dim3(C::THREADS), C::LDS, s, p);
}

// --- the pack (host only).  nz [rows][k] -> the most compact (H, tile id) under which the zeros have the
// structure above; the failures of the nearest attempt otherwise
struct PspPlan {
  int variant = -1, violations = 0;
  std::vector<int> perm;            // position -> true row
  std::vector<uint8_t> s;           // [rows / 16][taps][d]
};

PspPlan psp_analyze(const uint16_t* w, int rows, int cin, int ks) {
  const int taps = ks * ks, K = taps * cin;
  PspPlan best;
  best.violations = INT32_MAX;
  for (int H = 8; H <= 64; H *= 2) {
    if (rows % H != 0) continue;
    // supports of the residues mod H, merged into classes of equal support
    std::vector<std::vector<uint8_t>> supp(H, std::vector<uint8_t>(K, 0));
    for (int r = 0; r < rows; ++r) {
      uint8_t* sp = supp[r % H].data();
      const uint16_t* wr = w + static_cast<int64_t>(r) * K;
      for (int k = 0; k < K; ++k) sp[k] |= (wr[k] & 0x7fff) != 0;
    }
    std::vector<int> cls(H, -1), rep;
    for (int a = 0; a < H; ++a) {
      for (size_t c = 0; c < rep.size() && cls[a] < 0; ++c)
        if (supp[rep[c]] == supp[a]) cls[a] = static_cast<int>(c);
      if (cls[a] < 0) {
        cls[a] = static_cast<int>(rep.size());
        rep.push_back(a);
      }
    }
    int size_fail = 0;
    for (size_t c = 0; c < rep.size(); ++c) {
      const int members = static_cast<int>(std::count(cls.begin(), cls.end(), static_cast<int>(c)));
      size_fail += (members * (rows / H)) % 16 != 0;
    }
    for (int v = 0; v < 4; ++v) {
      const int P = kPspP[v], d = kPspD[v];
      int fails = size_fail + (cin % (32 * P / d) != 0);
      std::vector<uint8_t> sv(rep.size() * taps * d, 0);
      if (cin % P == 0) {
        for (size_t c = 0; c < rep.size(); ++c)
          for (int tap = 0; tap < taps; ++tap) {
            const uint8_t* L = supp[rep[c]].data() + tap * cin;
            bool ok = true;
            for (int ci = P; ci < cin && ok; ++ci) ok = L[ci] == L[ci % P];
            int live = 0;
            std::vector<int> seen(d, -1);
            for (int ci = 0; ci < P && ok; ++ci) {
              if (!L[ci]) continue;
              ++live;
              if (seen[ci % d] >= 0) ok = false;
              else seen[ci % d] = ci / d;
            }
            ok = ok && live == d;
            if (!ok) {
              ++fails;
              continue;
            }
            for (int u = 0; u < d; ++u) sv[(c * taps + tap) * d + u] = static_cast<uint8_t>(seen[u]);
          }
      } else {
        fails += static_cast<int>(rep.size()) * taps;
      }
      if (fails == 0) {
        // of the (H, tile id) that fit, the most compact one (smallest d / P), then the smallest H: a coarser H
        // can fit too, with the union of several classes' supports and their zeros stored as weights
        if (best.variant >= 0 && d * kPspP[best.variant] >= kPspD[best.variant] * P) continue;
        PspPlan pl;
        pl.variant = v;
        // classes in the order of their smallest residue, a class's rows ascending
        std::vector<int> frag_cls;
        for (size_t c = 0; c < rep.size(); ++c) {
          const size_t first = pl.perm.size();
          for (int r = 0; r < rows; ++r)
            if (cls[r % H] == static_cast<int>(c)) pl.perm.push_back(r);
          for (size_t f = 0; f < (pl.perm.size() - first) / 16; ++f) frag_cls.push_back(static_cast<int>(c));
        }
        pl.s.resize(static_cast<size_t>(rows / 16) * taps * d);
        for (size_t f = 0; f < frag_cls.size(); ++f)
          memcpy(pl.s.data() + f * taps * d, sv.data() + static_cast<size_t>(frag_cls[f]) * taps * d, static_cast<size_t>(taps) * d);
        best = pl;
        continue;
      }
      if (best.variant < 0 && fails < best.violations) best.violations = fails;
    }
  }
  if (best.variant < 0 && best.violations == INT32_MAX) best.violations = 1;
  return best;
}

bool psp_pack_shape_ok(int rows, int cin, int ks) {
  return rows > 0 && rows % kPspBCO == 0 && cin >= 64 && (cin & (cin - 1)) == 0 && (ks == 1 || ks == 3) &&
         static_cast<int64_t>(rows) * ks * ks * cin < (int64_t(1) << 31);
}

}  // namespace

const ConvKernel* psp_kernel(int variant, int ks) {
#define PSP_ROW(...) DRNMI_KERNEL_ROW(conv_psp_kernel, launch_psp, __VA_ARGS__)
  static const ConvKernel k[4][2] = {{PSP_ROW(1, 2, 16), PSP_ROW(3, 2, 16)},
                                     {PSP_ROW(1, 4, 16), PSP_ROW(3, 4, 16)},
                                     {PSP_ROW(1, 8, 8), PSP_ROW(3, 8, 8)},
                                     {PSP_ROW(1, 4, 8), PSP_ROW(3, 4, 8)}};
  return variant >= 0 && variant < 4 ? &k[variant][ks == 3] : nullptr;
}

// the period-sparse kernel's shapes: tile names the blob's (P, d); stride 1, whole 128-row tiles of real
// channels, whole K steps; a folded scale, no second input, no unit mask; fp32 or bf16 out at any strides
bool psp_conv_supported(const drnmi_conv_args& p) {
  if (p.dtype != DRNMI_BF16_PSP || p.tile < 0 || p.tile >= 4) return false;
  const int step = 32 * kPspP[p.tile] / kPspD[p.tile];
  return p.x2 == nullptr && p.unit_mask == nullptr && p.scale == nullptr && big_body_shape_ok(p, 64) &&
         p.k == p.ks * p.ks * p.cin && p.stride == 1 && p.cin % step == 0 && p.cout == p.cout_pad &&
         static_cast<int64_t>(p.cout_pad) * p.k < (int64_t(1) << 31) && p.h + 2 * p.pad < 16384 && p.w + 2 * p.pad < 16384 &&
         (p.out_dtype == DRNMI_F32 || p.out_dtype == DRNMI_BF16);
}

}  // namespace drnmi

using namespace drnmi;

extern "C" int64_t drnmi_psp_pack_bytes(int32_t rows, int32_t cin, int32_t ks, int32_t variant) {
  if (!psp_pack_shape_ok(rows, cin, ks) || variant < 0 || variant >= 4 || cin % (32 * kPspP[variant] / kPspD[variant]) != 0)
    return -1;
  const int d = kPspD[variant], G = kPspP[variant] / d;
  return psp_vals_off(rows, ks, d) + static_cast<int64_t>(rows) * (ks * ks * cin / G) * 2;
}

extern "C" int drnmi_psp_pack(const void* dense_bf16, int32_t rows, int32_t cin, int32_t ks, void* out, int64_t out_bytes,
                              int32_t* variant, int32_t* violations) {
  if (dense_bf16 == nullptr || variant == nullptr || violations == nullptr || !psp_pack_shape_ok(rows, cin, ks)) return DRNMI_EINVAL;
  const uint16_t* w = reinterpret_cast<const uint16_t*>(dense_bf16);
  const PspPlan pl = psp_analyze(w, rows, cin, ks);
  *variant = pl.variant;
  *violations = pl.violations;
  if (pl.variant < 0 || out == nullptr) return DRNMI_OK;
  const int64_t need = drnmi_psp_pack_bytes(rows, cin, ks, pl.variant);
  if (need < 0 || out_bytes < need) return DRNMI_EINVAL;
  const int P = kPspP[pl.variant], d = kPspD[pl.variant], G = P / d, taps = ks * ks, kc = taps * cin / G;
  char* o = reinterpret_cast<char*>(out);
  memset(o, 0, static_cast<size_t>(psp_vals_off(rows, ks, d)));
  const int32_t hdr[8] = {kPspMagic, rows, cin, ks, P, d, G, kc};
  memcpy(o, hdr, sizeof(hdr));
  int32_t* perm = reinterpret_cast<int32_t*>(o + kPspHeader);
  int32_t* order = perm + rows;
  memcpy(perm, pl.perm.data(), sizeof(int32_t) * rows);
  for (int t0 = 0; t0 < rows; t0 += kPspBCO) {
    for (int i = 0; i < kPspBCO; ++i) order[t0 + i] = i;
    std::sort(order + t0, order + t0 + kPspBCO, [&](int a, int b) { return perm[t0 + a] < perm[t0 + b]; });
  }
  memcpy(order + rows, pl.s.data(), pl.s.size());
  uint16_t* vals = reinterpret_cast<uint16_t*>(o + psp_vals_off(rows, ks, d));
  for (int pos = 0; pos < rows; ++pos) {
    const uint16_t* wr = w + static_cast<int64_t>(perm[pos]) * taps * cin;
    const uint8_t* sv = pl.s.data() + static_cast<size_t>(pos / 16) * taps * d;
    uint16_t* vr = vals + static_cast<int64_t>(pos) * kc;
    for (int tap = 0; tap < taps; ++tap)
      for (int q = 0; q < cin / P; ++q)
        for (int v = 0; v < d; ++v) vr[tap * (cin / G) + q * d + v] = wr[tap * cin + q * P + v + d * sv[tap * d + v]];
  }
  return DRNMI_OK;
}
