// The one routing decision per conv launch (host code only).  conv_route() validates a
// drnmi_conv_args, decodes its tile id, applies the auto policy and returns the kernel row to
// launch; drnmi_conv2d_bn_act launches that row and drnmi_conv_kernel_name / drnmi_conv_status
// report it, so the three cannot disagree.  seg_route() does the same for drnmi_conv_stag_seg.
// The kernel files own their rows (name + launcher), geometry predicates and launch attributes
// (conv_route.h).  Routing is fixed (no environment switches); the forced tile ids stay reachable
// for the bit-identity tests.
#include "conv_route.h"

namespace drnmi {
namespace {

struct TileDesc {
  int id, bm, bn;
  const char* name;
};

constexpr TileDesc kTiles[] = {
    {DRNMI_TILE_IGEMM_128X128, 128, 128, "128x128"},
    {DRNMI_TILE_IGEMM_128X64, 128, 64, "128x64"},
    {DRNMI_TILE_IGEMM_256X32, 256, 32, "256x32"},
    {DRNMI_TILE_IGEMM_256X16, 256, 16, "256x16"},
    // conv_big.hip (bf16, LDS-DMA implicit GEMM, cin >= 32, ks 1/3): cout tile x 256 pixels
    {DRNMI_TILE_DMA128, 128, 128, "dma128"}, {DRNMI_TILE_DMA256, 256, 256, "dma256"},
    {DRNMI_TILE_DMA64K32, 64, 64, "dma64k32"}, {DRNMI_TILE_DMA64, 32, 32, "dma32"},
    {DRNMI_TILE_DMA256K32, 256, 256, "dma256k32"}, {DRNMI_TILE_DMA128K32, 128, 128, "dma128k32"},
    {DRNMI_TILE_DMA128P, 128, 128, "dma128p"}, {DRNMI_TILE_DMA256P, 256, 256, "dma256p"},
    {DRNMI_TILE_DMA64K32P, 64, 64, "dma64k32p"}, {DRNMI_TILE_DMA64P, 32, 32, "dma32p"},
    {DRNMI_TILE_DMA256K32P, 256, 256, "dma256k32p"}, {DRNMI_TILE_DMA128K32P, 128, 128, "dma128k32p"},   // p = persistent
    {DRNMI_TILE_PP256, 256, 256, "pp256"},
    {DRNMI_TILE_HALO, 128, 128, "halo"},
    {DRNMI_TILE_STRIP, 256, 256, "strip256"},
    {DRNMI_TILE_STAG, 256, 256, "stag256"},
    {DRNMI_TILE_S2ROW, 64, 64, "s2row"},
    {DRNMI_TILE_S1X2ROW, 64, 64, "s1x2row"},
    {DRNMI_TILE_W1, 256, 256, "w1stag256"},
    {DRNMI_TILE_W1H, 128, 128, "w1h128"},
};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);
constexpr bool tiles_in_enum_order() {
  for (int i = 0; i < kNumTiles; ++i)
    if (kTiles[i].id != i) return false;
  return kNumTiles == DRNMI_TILE_COUNT;
}
static_assert(tiles_in_enum_order(), "kTiles[i] describes enum drnmi_tile value i");
static_assert(DRNMI_TILE_PP256 - DRNMI_TILE_DMA128 + 1 == kNumBigVariants,
              "big_variant(tile - DRNMI_TILE_DMA128)");

constexpr int kBK = 32;     // conv_igemm's K step

ConvRoute refuse(int status) { return {status, nullptr, 1}; }
ConvRoute take(const ConvKernel* k, int splits = 1) {
  return k != nullptr && k->name != nullptr ? ConvRoute{0, k, splits} : refuse(DRNMI_ENOTSUP);
}

// every weight row a tile's DMA reads must exist: ceil(cout / BCO) * BCO <= cout_pad
bool rows_exist(const drnmi_conv_args& p, int bco) { return (p.cout + bco - 1) / bco * bco <= p.cout_pad; }

bool conv_geometry(const drnmi_conv_args& p) {
  return p.ho == (p.h + 2 * p.pad - p.dil * (p.ks - 1) - 1) / p.stride + 1 &&
         p.wo == (p.w + 2 * p.pad - p.dil * (p.ks - 1) - 1) / p.stride + 1;
}

// --- conv_igemm: tile by cout
int auto_tile(int cout) {
  if (cout > 64) return DRNMI_TILE_IGEMM_128X128;
  if (cout > 32) return DRNMI_TILE_IGEMM_128X64;
  if (cout > 16) return DRNMI_TILE_IGEMM_256X32;
  return DRNMI_TILE_IGEMM_256X16;
}

// --- the bf16 LDS-DMA kernels
int auto_variant(const drnmi_conv_args& p) {
  if (p.cin < 64) return p.cout % 256 == 0 ? DRNMI_TILE_DMA256K32 : p.cout % 128 == 0 ? DRNMI_TILE_DMA128K32 : DRNMI_TILE_DMA64K32;   // K steps of 32
  // cout <= 32 (the seg 1x1) also takes the 64-wide BK-32 tile: 57 vs 66 us on the D-22 seg conv
  // at batch 8 (scripts/conv_micro.py) — two workgroups fit per CU where the 32-wide 3 x 36 KB ring fits one
  // 64 -> 128 (D-22 layer4.0 conv1 / downsample, stride 2): the 64-wide BK-32 tile too, two
  // workgroups per CU against one for the 128 x 256 x 3-stage ring: 98 vs 116 us (3x3), 50 vs
  // 75 us (1x1) at batch 8 (scripts/conv_micro.py); the fused-x2 instantiations are DMA128 / DMA256
  if (p.cin <= 64 && p.cout % 256 != 0 && p.x2 == nullptr) {
    // cin == 64 3x3 (D-22 layer4.0 conv1, stride 2): the 64-wide tile with 64-channel K steps on a
    // 2 x 40 KB ring halves the K steps of the BK-32 tile at the same DMA bytes: 93.6 vs 102 us
    // at batch 8 (profiles/r3k_tile_64w_bk64_ab.txt)
    if (p.cin == 64 && p.ks == 3) return DRNMI_TILE_DMA64;
    return DRNMI_TILE_DMA64K32;
  }
  return p.cout % 256 == 0 ? DRNMI_TILE_DMA256 : p.cout % 128 == 0 ? DRNMI_TILE_DMA128 : DRNMI_TILE_DMA64K32;
}

// conv_w1 is auto-routed where it measured no slower inside the network (same-box interleaved
// bench A/B, profiles/r10m_w1_ab): the long-K residual-free launches (D-22 layer6.1 conv1,
// layer7).  At cin 128 / 256 (18 / 36 K steps) and with a residual its per-tile prologue and
// epilogue, issued by 4 waves instead of 8, cost more than the loop saves (layer5.0 conv1 145 vs
// 130 us)
bool w1_auto(const drnmi_conv_args& p) { return w1_ok(p) && p.x2 == nullptr && p.cin >= 512 && p.res == nullptr; }
bool w1h_auto(const drnmi_conv_args& p) { return w1h_ok(p) && p.cout <= 128; }

// 128-channel convs (D-22 layer4) go to the staggered 128-channel tile instead of the halo
// kernel when both apply (88-96 vs 102-107 us, profiles/r4c_stag128_vs_halo)
bool halo_preferred(const drnmi_conv_args& p) { return !(big_conv_supported(p) && stag_ok(p)); }

// s2row_auto / s1x2row_auto: the row-walk kernels are routed by default wherever they apply.
// Auto-picked strip launches run conv_w1_kernel on the long-K residual-free launches (w1_auto),
// conv_w1h_kernel at cout <= 128, else conv_stag_kernel when cin % 128 == 0 (5-6 % faster than the
// strip tile, bit-identical), else conv_strip_kernel.
ConvRoute big_route(const drnmi_conv_args& p) {
  int tile = p.tile;
  const bool auto_pick = tile < 0;
  if (tile == DRNMI_TILE_S2ROW || (auto_pick && s2row_conv_supported(p)))
    return s2row_conv_supported(p) ? take(s2row_kernel(p.cin)) : refuse(DRNMI_ENOTSUP);
  if (tile == DRNMI_TILE_S1X2ROW || (auto_pick && s1x2row_conv_supported(p)))
    return s1x2row_conv_supported(p) ? take(s1x2row_kernel()) : refuse(DRNMI_ENOTSUP);
  if ((tile == DRNMI_TILE_W1 || tile == DRNMI_TILE_W1H) &&
      (!big_conv_supported(p) || !(tile == DRNMI_TILE_W1 ? w1_ok(p) : w1h_ok(p))))
    return refuse(DRNMI_ENOTSUP);
  // the halo kernel (cin/cout 64-128) stays dense: it beats unit skipping on those shapes
  if (tile == DRNMI_TILE_HALO || (auto_pick && halo_conv_supported(p) && halo_preferred(p)))
    return halo_conv_supported(p) ? take(halo_kernel(p.cin, p.cout)) : refuse(DRNMI_ENOTSUP);
  if (!big_conv_supported(p)) return refuse(DRNMI_ENOTSUP);
  if (auto_pick) {
    tile = auto_variant(p);
    if (w1_auto(p)) tile = DRNMI_TILE_W1;
    else if (w1h_auto(p)) tile = DRNMI_TILE_W1H;
    else if (stag_ok(p)) tile = DRNMI_TILE_STAG;
    else if (tile == DRNMI_TILE_DMA256 && strip_ok(p)) tile = DRNMI_TILE_STRIP;
  }
  if (tile == DRNMI_TILE_W1) return take(w1_kernel(false, p.x2 != nullptr));
  if (tile == DRNMI_TILE_W1H) return take(w1h_kernel(false, p.x2 != nullptr));
  if (tile == DRNMI_TILE_STAG) return stag_ok(p) ? take(stag_kernel(DRNMI_BF16, p.cout <= 128, p.x2 != nullptr)) : refuse(DRNMI_ENOTSUP);
  if (tile == DRNMI_TILE_STRIP) {
    if (!strip_ok(p) || p.cin < 64) return refuse(DRNMI_ENOTSUP);
    return rows_exist(p, 256) ? take(strip_kernel(false)) : refuse(DRNMI_EINVAL);
  }
  if (tile > DRNMI_TILE_PP256) return refuse(DRNMI_ENOTSUP);
  const BigVariant& v = big_variant(tile - DRNMI_TILE_DMA128);
  if (p.cin < v.bk) return refuse(DRNMI_ENOTSUP);                            // a K step must fit in one tap
  if (!rows_exist(p, v.bco)) return refuse(DRNMI_EINVAL);
  const int ks3 = p.ks == 3;
  if (tile == DRNMI_TILE_PP256 && p.cout % 256 != 0) return refuse(DRNMI_ENOTSUP);
  if (p.x2 != nullptr) return take(&v.x2[ks3]);        // fused second input: its own instantiation (DMA128 / DMA256)
  if (p.unit_mask != nullptr && v.sparse[ks3].name != nullptr && p.k_pad / v.bk <= 128) return take(&v.sparse[ks3]);
  return take(&v.dense[ks3]);
}

// --- the 8-bit families (DRNMI_I8: W8A8; DRNMI_F8: e4m3), one route
int q8_variant(const drnmi_conv_args& p) {
  const int wide = p.cout % 256 == 0 ? 0 : 1;
  // 1x1: the two-workgroups-per-CU tile (71.6-73.5 vs 86.7-86.9 us for layer5.0 / layer6.0's
  // downsample, 65.6-67.0 for the seg conv: profiles/r6_int8_fusions/occ2_ab.txt).  Its 128 rows
  // always divide cout_pad (q8_conv_supported: cout_pad % 128 == 0), for either code
  return p.ks == 1 && p.cout_pad % q8_variant_row(p.dtype, kQ8Occ2).bco == 0 ? kQ8Occ2 : (p.cin >= 128 ? 0 : 2) + wide;
}
// conv_w1h_i8_kernel is auto-routed at cin, cout <= 256 (D-22 layer4.1, layer5 in int8 nets:
// profiles/r11_int8_layer4)
bool i8_w1h_pick(const drnmi_conv_args& p) {
  return p.tile == DRNMI_TILE_W1H ||
         (p.tile < 0 && i8_w1h_ok(p) && (p.cout <= 128 || p.cin == 128 || (p.cin <= 256 && p.cout <= 256)));
}

// Both codes run conv_{i8,f8}_kernel on the same five tiles (128-B rows at cin >= 128, the 64-B rows
// -- fp8: the K-64 step shape -- at cin == 64) and the strip-staged conv_{i8,f8}_stag_kernel on the
// row-aligned 3x3 launches q8_stag_ok admits.  What fp8 lacks is stated where int8 takes it: the
// one-wave-per-SIMD tiles (W1, W1H), the strip tile and the seg-fused form (seg_route).
ConvRoute q8_route(const drnmi_conv_args& p) {
  if (!q8_conv_supported(p)) return refuse(DRNMI_ENOTSUP);
  const bool f8 = p.dtype == DRNMI_F8;
  if (f8 && (p.tile == DRNMI_TILE_W1 || p.tile == DRNMI_TILE_W1H)) return refuse(DRNMI_ENOTSUP);   // no fp8 form
  const Q8Variant& v = q8_variant_row(p.dtype, q8_variant(p));
  if (!rows_exist(p, v.bco)) return refuse(DRNMI_EINVAL);
  const int ks3 = p.ks == 3;
  if (!f8 && ks3 && i8_w1h_pick(p)) return i8_w1h_ok(p) ? take(w1h_kernel(true, false)) : refuse(DRNMI_ENOTSUP);
  if (ks3 && q8_stag_ok(p)) {
    // DRNMI_TILE_W1 forces the one-wave-per-SIMD int8 tile (the bit-identity tests); else the
    // staggered one: on the long-K residual-free int8 launches conv_w1_i8_kernel measured no faster
    // inside the network (profiles/r11_w1i8: layer6.1 conv1 460 vs 450 us); the seg-fused layer8
    // launch (drnmi_conv_stag_seg) takes its SEGF form (431 vs 456 us)
    if (p.tile != DRNMI_TILE_W1) return take(stag_kernel(p.dtype, false, false));
    return i8_w1_ok(p) ? take(w1_kernel(true, false)) : refuse(DRNMI_ENOTSUP);
  }
  // fp8: DRNMI_TILE_STAG forces the staggered tile and refuses the shapes it does not admit (int8
  // ignores the id there); and no fp8 strip tile
  if (f8 && p.tile == DRNMI_TILE_STAG) return refuse(DRNMI_ENOTSUP);
  if (!f8 && ks3 && i8_strip_ok(p)) return take(strip_kernel(true));
  return take(&v.k[ks3]);
}

// --- the 2:4 weight-sparse bf16 tiles (DRNMI_BF16_SP24, conv_sp24.hip).  tile is this dtype's own
// variant (enum drnmi_sp24_tile).  The strip-staged form takes conv_strip_kernel's geometry on the
// 256 x 256 tile and is a forced variant only: with the MFMA time of a K step halved, its two-stage ring
// that waits for all of a step's DMA measured slower than the gather's three counted stages at
// cin 512 (758 vs 707 us) and equal at cin 256 (profiles/sp24), so auto is the gather everywhere
ConvRoute sp24_route(const drnmi_conv_args& p) {
  if (p.tile != DRNMI_TILE_AUTO && p.tile != DRNMI_SP24_GATHER && p.tile != DRNMI_SP24_STRIP) return refuse(DRNMI_EINVAL);
  if (!sp24_conv_supported(p)) return refuse(DRNMI_ENOTSUP);
  const bool tile128 = p.cout_pad % 256 != 0 || p.cout <= 128;
  const bool strip = !tile128 && strip_ok(p);
  if (p.tile == DRNMI_SP24_STRIP && !strip) return refuse(DRNMI_ENOTSUP);
  if (p.tile == DRNMI_SP24_STRIP) return take(sp24_strip_kernel());
  if (!rows_exist(p, tile128 ? 128 : 256)) return refuse(DRNMI_EINVAL);
  return take(sp24_kernel(tile128, p.ks));
}

// --- the 2:4 weight-sparse int8 tiles (DRNMI_I8_SP24, conv_sp24_i8.hip): sp24_route's decisions on the
// int8 contract (a non-NULL scale, the 8-bit epilogue).  Auto is the gather; the strip-staged form is a
// forced variant (profiles/sp24_i8/README.txt)
ConvRoute sp24_i8_route(const drnmi_conv_args& p) {
  if (p.tile != DRNMI_TILE_AUTO && p.tile != DRNMI_SP24_GATHER && p.tile != DRNMI_SP24_STRIP) return refuse(DRNMI_EINVAL);
  if (!sp24_i8_conv_supported(p)) return refuse(DRNMI_ENOTSUP);
  const bool tile128 = p.cout_pad % 256 != 0 || p.cout <= 128;
  const bool strip = !tile128 && strip_ok(p);
  if (p.tile == DRNMI_SP24_STRIP && !strip) return refuse(DRNMI_ENOTSUP);
  if (!rows_exist(p, tile128 ? 128 : 256)) return refuse(DRNMI_EINVAL);
  if (p.tile == DRNMI_SP24_STRIP) return take(sp24_i8_strip_kernel());
  return take(sp24_i8_kernel(tile128, p.ks));
}

// --- conv_x6.  A drnmi_conv_args.tile >= 0 forces variant tile % 6 and, when tile >= 6, tile / 6
// split-K partitions (tests, micro-benchmarks; split-K only with a caller workspace).
// 128-channel layers take the two-per-CU 128 x 128 tile: D-22 layer4's five launches 1631-1649 ->
// 1510-1568 us against the 8-wave 128 x 256 tile, same box, three interleaved runs each
// (profiles/r9_x6_v5/v4_ab.txt; the 8-wave tile had beaten the 4-wave one, 492 vs 511 us,
// profiles/r7_x6).  64-channel
// layers (and the 19-class seg) take the two-per-CU 64 x 128 tile (eight waves per CU instead of
// four): D-22 layer3 3x3 750 -> 660 us at batch 8, the fine-tune's 1x1 256 -> 64 49 -> 37 us, the
// seg 1x1 512 -> 19 153 -> 142 us (profiles/r9_x6_v5)
int x6_auto_variant(const drnmi_conv_args& p) {
  return p.cout % 256 == 0 ? 0 : p.cout % 128 == 0 ? 4 : p.cout <= 64 ? 5 : 2;
}

int x6_num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  }
  return cus;
}

// Launch plan (variant, split-K count); split_ok: the launch has (drnmi_conv_args.ws) or is sizing
// (drnmi_conv_workspace_bytes) a caller workspace.  Inference launches (none) take the auto variant
// unsplit.  The fp32x training path (a workspace) picks among the 256- / 128-channel tiles
// and S = 1..4 by a cost model: rounds of resident workgroups x K steps per workgroup x the
// variant's step time, plus the split partials' HBM round trip (S x M x cout fp32 written and
// read) and the output (+ residual) stream.  The default (auto variant, S = 1) is kept unless the
// best plan is >= 5 % faster.  The model is within a few % of the SPLITS sweep (512 -> 512 d4 at
// 2 x 128 x 96: 631 / 580 us modelled for S = 1 / 4, 627 / 580 measured).
struct X6Plan { int v, S; };
X6Plan x6_plan(const drnmi_conv_args& p, bool split_ok) {
  // the partials are [split][m][cout] rows written as float4: only cout % 4 == 0 splits
  if (p.cout % 4 != 0) split_ok = false;
  if (p.tile >= 0) {
    const int v = p.tile % kNumX6;
    int S = p.tile / kNumX6;
    if (!split_ok || S < 1) S = 1;
    if (S > p.k_pad / kX6BK) S = p.k_pad / kX6BK;
    return {v, S};
  }
  const int v0 = x6_auto_variant(p);
  if (!split_ok) return {v0, 1};
  const int cus = x6_num_cus();
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  const int nk = p.k_pad / kX6BK;
  const double out_s = static_cast<double>(M) * p.cout * 4.0 * (p.res != nullptr ? 2 : 1) / 4.5e12;
  auto tiles_of = [&](const X6Variant& x) { return ((M + x.bpx - 1) / x.bpx) * ((p.cout + x.bco - 1) / x.bco); };
  auto cost = [&](const X6Variant& x, int S) {
    const int64_t slots = static_cast<int64_t>(cus) * x.occ;
    const int64_t rounds = (tiles_of(x) * S + slots - 1) / slots;
    double t = static_cast<double>(rounds) * ((nk + S - 1) / S) * x.step + out_s;
    if (S > 1) t += 2.0 * S * static_cast<double>(M) * p.cout * 4.0 / 4e12 + 4e-6;
    return t;
  };
  // Only the auto variant's split counts: with the two-per-CU 128 x 128 tile as a candidate (<= two
  // rounds of it) the plan moved 1/3 of the step's conv_x6 launches onto it and the step's conv_x6
  // time did not move (19.52 -> 19.57 ms, profiles/r8_finetune/x6_plan_v4.txt); variant 4 stays a
  // forced tile for A/B runs.
  const X6Variant& x = x6_variant(v0);
  const double c0 = cost(x, 1);
  X6Plan best{v0, 1};
  double bc = c0;
  if (!rows_exist(p, x.bco)) return best;
  for (int S = 1; S <= 4 && (S == 1 || nk / S >= 8); ++S) {
    if (x.occ == 2 && tiles_of(x) * S > 2 * 2 * static_cast<int64_t>(cus)) continue;
    const double c = cost(x, S);
    if (c < 0.95 * c0 && c < bc) {
      best = {v0, S};
      bc = c;
    }
  }
  return best;
}
// the workspace a training launch of this geometry needs (its plan with splits allowed); a plan
// that differs from the inference default without splitting asks for a token 256 B, since a
// launch takes the training plan exactly when it is given a workspace
int64_t x6_workspace_bytes(const drnmi_conv_args& p) {
  const X6Plan pl = x6_plan(p, true);
  if (pl.S > 1) return static_cast<int64_t>(pl.S) * p.n * p.ho * p.wo * p.cout * 4;
  return pl.v != x6_plan(p, false).v ? 256 : 0;
}

// rows of BN-statistics partials a launch with these arguments writes (0: it cannot -- split K)
int64_t x6_stats_rows(const drnmi_conv_args& p) {
  if (!x6_conv_supported(p)) return 0;
  const X6Plan pl = x6_plan(p, p.ws != nullptr);
  if (pl.S > 1) return 0;
  const int bpx = x6_variant(pl.v).bpx;
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  return (M + bpx - 1) / bpx * (bpx / 64);
}

ConvRoute x6_route(const drnmi_conv_args& p) {
  if (!x6_conv_supported(p)) return refuse(DRNMI_ENOTSUP);
  const X6Plan pl = x6_plan(p, p.ws != nullptr);
  const X6Variant& v = x6_variant(pl.v);
  if (!rows_exist(p, v.bco)) return refuse(DRNMI_EINVAL);      // ... in each plane
  if (3 * static_cast<int64_t>(p.cout_pad) * p.k_pad >= (int64_t(1) << 31)) return refuse(DRNMI_EINVAL);
  const int S = pl.S;
  if (S > 1 && p.stats != nullptr) return refuse(DRNMI_EINVAL);   // statistics only from an unsplit launch
  if (p.stats != nullptr && (reinterpret_cast<uintptr_t>(p.stats) & 7) != 0) return refuse(DRNMI_EINVAL);
  if (S > 1 && p.ws_bytes < x6_workspace_bytes(p)) return refuse(DRNMI_EINVAL);
  if (S > 1 && (reinterpret_cast<uintptr_t>(p.ws) & 15) != 0) return refuse(DRNMI_EINVAL);
  return take(&v.k[p.ks - 1], S);       // ks 2: the 2x2 parity-class kernels of a stride-2 conv's data gradient
}

}  // namespace

ConvRoute conv_route(const drnmi_conv_args& p) {
  // BN-statistics partials and output row strides: conv_x6 only
  if (p.stats != nullptr && (p.algo != DRNMI_ALGO_IGEMM || x6_stats_rows(p) <= 0)) return refuse(DRNMI_EINVAL);
  if (p.y_sr != 0 && (p.algo != DRNMI_ALGO_IGEMM || p.dtype != DRNMI_F32X3 || p.y_sc != 1 || p.y_sr < 0 ||
                      !x6_conv_supported(p)))
    return refuse(DRNMI_EINVAL);
  if (p.algo == DRNMI_ALGO_PATCH) {
    if (p.dtype == DRNMI_BF16_SP24 || p.dtype == DRNMI_I8_SP24) return refuse(DRNMI_EINVAL);
    if (p.x2 != nullptr) return refuse(DRNMI_ENOTSUP);     // fused second input: LDS-DMA kernels only
    if (p.n <= 0 || p.h <= 0 || p.w <= 0 || p.cout > p.cout_pad || !conv_geometry(p)) return refuse(DRNMI_EINVAL);
    return take(patch_kernel(p));
  }
  if (p.algo != DRNMI_ALGO_IGEMM || p.src_u8) return refuse(DRNMI_EINVAL);
  // 2:4 sparse: no fused second input, unit mask or unfolded scale
  if (p.dtype == DRNMI_BF16_SP24 && (p.x2 != nullptr || p.unit_mask != nullptr || p.scale != nullptr)) return refuse(DRNMI_ENOTSUP);
  // 2:4 sparse int8: no fused second input or unit mask; the int8 contract's scale
  if (p.dtype == DRNMI_I8_SP24 && (p.x2 != nullptr || p.unit_mask != nullptr || p.scale == nullptr)) return refuse(DRNMI_ENOTSUP);
  const bool pow2 = p.cin >= 8 && (p.cin & (p.cin - 1)) == 0;
  if (!pow2 || p.n <= 0 || p.h <= 0 || p.w <= 0 || p.ho <= 0 || p.wo <= 0) return refuse(DRNMI_EINVAL);
  if (p.cout <= 0 || p.cout > p.cout_pad || p.k != p.ks * p.ks * p.cin + (p.x2 != nullptr ? p.cin2 : 0))
    return refuse(DRNMI_EINVAL);
  if (p.k_pad < p.k || p.k_pad % kBK != 0 || p.stride <= 0 || p.dil <= 0 || p.pad < 0) return refuse(DRNMI_EINVAL);
  if (p.dtype == DRNMI_I8 || p.dtype == DRNMI_F8) {       // 8-bit: the code's own type, bf16 or fp32
    if (p.out_dtype != p.dtype && p.out_dtype != DRNMI_BF16 && p.out_dtype != DRNMI_F32) return refuse(DRNMI_EINVAL);
  } else if (p.dtype == DRNMI_I8_SP24) {                  // the int8 route's outputs
    if (p.out_dtype != DRNMI_I8 && p.out_dtype != DRNMI_BF16 && p.out_dtype != DRNMI_F32) return refuse(DRNMI_EINVAL);
  } else if (p.dtype == DRNMI_F32X3) {
    if (p.out_dtype != DRNMI_F32) return refuse(DRNMI_EINVAL);
  } else if ((p.dtype != DRNMI_BF16 && p.dtype != DRNMI_F32 && p.dtype != DRNMI_BF16_SP24) ||
             (p.out_dtype != DRNMI_BF16 && p.out_dtype != DRNMI_F32)) {
    return refuse(DRNMI_EINVAL);
  }
  // Output geometry must be the conv's: ho = (h + 2 pad - dil (ks-1) - 1) / stride + 1 -- except for
  // the row-strided (y_sr) class launches of a stride-2 data gradient, whose taps past the input's
  // bottom / right edge read zeros (an asymmetric pad; conv_x6 bounds-checks every tap)
  if (p.y_sr == 0 && !conv_geometry(p)) return refuse(DRNMI_EINVAL);
  if (p.dtype == DRNMI_I8 || p.dtype == DRNMI_F8) return q8_route(p);       // 8-bit: one kernel family
  if (p.dtype == DRNMI_F32X3) return x6_route(p);
  if (p.dtype == DRNMI_BF16_SP24) return sp24_route(p);
  if (p.dtype == DRNMI_I8_SP24) return sp24_i8_route(p);
  if (p.tile >= DRNMI_TILE_DMA128 || (p.tile < 0 && (big_conv_supported(p) || halo_conv_supported(p)))) return big_route(p);
  if (p.x2 != nullptr) return refuse(DRNMI_ENOTSUP);          // fused second input: LDS-DMA kernels only
  const int tile = p.tile < 0 ? auto_tile(p.cout) : p.tile;
  if (p.cout_pad % kTiles[tile].bn != 0) return refuse(DRNMI_EINVAL);
  const int64_t M = static_cast<int64_t>(p.n) * p.ho * p.wo;
  if (M >= (int64_t(1) << 31) / 2) return refuse(DRNMI_EINVAL);
  return take(igemm_kernel(p.dtype, tile, p.ks));
}

namespace {

struct SegRoute {
  int status;
  const SegKernel* k;
};

// The conv-side checks of drnmi_conv_stag_seg (those that do not involve seg_w, seg_k_pad,
// seg_rows, partials): the conv it replaces must take the staggered tile.  The launch runs on the
// one-wave-per-SIMD tile (conv_w1_seg_kernel / conv_w1_i8_seg_kernel); DRNMI_TILE_STAG forces the
// staggered one (the same partial logits, bit for bit: the bit-identity test).
SegRoute seg_route(const drnmi_conv_args& p) {
  if (p.algo != DRNMI_ALGO_IGEMM || p.src_u8) return {DRNMI_EINVAL, nullptr};
  if (p.dtype == DRNMI_F8 || p.dtype == DRNMI_BF16_SP24 || p.dtype == DRNMI_I8_SP24) return {DRNMI_ENOTSUP, nullptr};   // no seg-fused fp8 / 2:4 form
  const bool i8 = p.dtype == DRNMI_I8;
  // int8 nets: the conv's int8 output (out_dtype I8, quantised with out_scale) feeds int8 seg
  // weights; int32 partials
  if (i8 ? (p.out_dtype != DRNMI_I8 || p.scale == nullptr) : (p.dtype != DRNMI_BF16 || p.out_dtype != DRNMI_BF16))
    return {DRNMI_EINVAL, nullptr};
  if (!conv_geometry(p)) return {DRNMI_EINVAL, nullptr};
  const bool stag = i8 ? q8_conv_supported(p) && p.ks == 3 && q8_stag_ok(p)
                       : big_conv_supported(p) && stag_ok(p) && p.x2 == nullptr && p.scale == nullptr;
  if (!stag || p.res != nullptr || p.cout % 256 != 0 || p.cout_pad < p.cout) return {DRNMI_ENOTSUP, nullptr};
  return {0, p.tile == DRNMI_TILE_STAG ? stag_seg_kernel(i8) : w1_seg_kernel(i8)};
}

int launch_status(hipError_t e) { return e == hipErrorInvalidValue ? DRNMI_ENOTSUP : static_cast<int>(e); }

}  // namespace
}  // namespace drnmi

using namespace drnmi;

extern "C" int drnmi_conv_num_tiles(void) { return kNumTiles; }

extern "C" const char* drnmi_conv_tile_name(int tile) {
  return (tile >= 0 && tile < kNumTiles) ? kTiles[tile].name : nullptr;
}

extern "C" int drnmi_conv2d_bn_act(const drnmi_conv_args* a, void* stream) {
  if (a == nullptr || a->x == nullptr || a->wgt == nullptr || a->shift == nullptr || a->y == nullptr) return DRNMI_EINVAL;
  const ConvRoute r = conv_route(*a);
  if (r.status != 0) return r.status;
  return launch_status(r.k->launch(*a, r.splits, reinterpret_cast<hipStream_t>(stream)));
}

extern "C" int drnmi_conv_status(const drnmi_conv_args* a) { return a == nullptr ? DRNMI_EINVAL : conv_route(*a).status; }

extern "C" const char* drnmi_conv_kernel_name(const drnmi_conv_args* a) {
  return a == nullptr ? nullptr : conv_route(*a).name();
}

extern "C" int64_t drnmi_conv_workspace_bytes(const drnmi_conv_args* a) {
  if (a == nullptr) return -1;
  return a->dtype == DRNMI_F32X3 && a->algo == DRNMI_ALGO_IGEMM && x6_conv_supported(*a) ? x6_workspace_bytes(*a) : 0;
}

extern "C" int64_t drnmi_conv_stats_rows(const drnmi_conv_args* a) {
  if (a == nullptr) return -1;
  return a->dtype == DRNMI_F32X3 && a->algo == DRNMI_ALGO_IGEMM ? x6_stats_rows(*a) : 0;
}

// The labels-only video path's last 3x3 conv (D-22 layer8) with the seg classifier folded into its
// epilogue (conv_stag.hip SEGF): same launch geometry and MFMA work as conv_stag_kernel, the
// activation is never stored.  Validated like the conv it replaces plus the seg operands.
extern "C" int drnmi_conv_stag_seg(const drnmi_conv_args* a, const void* seg_w, int32_t seg_k_pad, int32_t seg_rows,
                                   void* partials, void* stream) {
  if (a == nullptr || seg_w == nullptr || partials == nullptr) return DRNMI_EINVAL;
  const drnmi_conv_args& p = *a;
  if (p.x == nullptr || p.wgt == nullptr || p.shift == nullptr) return DRNMI_EINVAL;
  const SegRoute r = seg_route(p);
  if (r.status == DRNMI_EINVAL) return DRNMI_EINVAL;
  // seg weight rows: whole 16-B pieces of int8 / bf16 columns
  if (seg_k_pad < p.cout || seg_k_pad % (p.dtype == DRNMI_I8 ? 16 : 8) != 0 || seg_rows < 32 ||
      (reinterpret_cast<uintptr_t>(partials) & 15) != 0)
    return DRNMI_EINVAL;
  if (r.status != 0) return r.status;
  return launch_status(r.k->launch(p, seg_w, seg_k_pad, partials, reinterpret_cast<hipStream_t>(stream)));
}

extern "C" const char* drnmi_conv_stag_seg_kernel_name(const drnmi_conv_args* a) {
  if (a == nullptr) return nullptr;
  const SegRoute r = seg_route(*a);
  return r.status == 0 ? r.k->name : nullptr;
}
