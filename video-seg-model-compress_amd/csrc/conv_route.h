// The conv routing interface between the kernel translation units and conv_route.cpp (host code
// only: no device declarations, so the host-only route can include it).
//
// Each kernel file exports one ConvKernel row per instantiation (the name the profiler shows and
// the launcher, written once by DRNMI_KERNEL_ROW so the string cannot drift from the template
// arguments) and the geometry predicates only it knows.  conv_route.cpp is the only place that
// decodes drnmi_conv_args.tile, applies the auto policy and picks a row.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/drnmi.h"

namespace drnmi {

struct ConvKernel {
  const char* name;     // nullptr: no such instantiation
  hipError_t (*launch)(const drnmi_conv_args& p, int splits, hipStream_t s);   // splits: conv_x6's split-K count
};
template <hipError_t (*LAUNCH)(const drnmi_conv_args&, hipStream_t)>
hipError_t launch_unsplit(const drnmi_conv_args& p, int, hipStream_t s) {
  return LAUNCH(p, s);
}
// KERNEL<ARGS> launched by LAUNCH<ARGS>(p, s)
#define DRNMI_KERNEL_ROW(KERNEL, LAUNCH, ...) \
  ConvKernel { #KERNEL "<" #__VA_ARGS__ ">", &launch_unsplit<&LAUNCH<__VA_ARGS__>> }
// a kernel that is no template, launched by LAUNCH<&KERNEL>(p, s)
#define DRNMI_KERNEL_ROW0(KERNEL, LAUNCH) \
  ConvKernel { #KERNEL, &launch_unsplit<&LAUNCH<&KERNEL>> }
constexpr ConvKernel kNoKernel{nullptr, nullptr};

// the seg-fused launches (drnmi_conv_stag_seg): the conv's arguments plus the classifier's
struct SegKernel {
  const char* name;
  hipError_t (*launch)(const drnmi_conv_args& p, const void* seg_w, int seg_k_pad, void* part, hipStream_t s);
};
#define DRNMI_SEG_ROW(KERNEL, LAUNCH) \
  SegKernel { #KERNEL, &LAUNCH<&KERNEL> }

struct ConvRoute {
  int status;               // 0, DRNMI_EINVAL or DRNMI_ENOTSUP
  const ConvKernel* k;      // status == 0: what to launch
  int splits;               // conv_x6's split-K count (1 elsewhere)
  const char* name() const { return status == 0 ? k->name : nullptr; }
};
// Every check of drnmi_conv2d_bn_act except the null checks of x, wgt, shift, y (routing reads the
// other pointers only for presence or alignment).
ConvRoute conv_route(const drnmi_conv_args& p);

// conv_igemm.hip: register-staged implicit GEMM, tiles 0..3 (128x128, 128x64, 256x32, 256x16), ks 1 / 3 / 7
const ConvKernel* igemm_kernel(int dtype, int tile, int ks);     // nullptr: no such kernel size

// conv_big.hip: bf16 LDS-DMA implicit GEMM for cin >= 32, cout_pad % 128 == 0; rows [ks == 3]
struct BigVariant {
  int bco, bk;              // output channels per tile, channels per K step
  ConvKernel dense[2], sparse[2], x2[2];
};
constexpr int kNumBigVariants = 13;
const BigVariant& big_variant(int v);            // tile ids DRNMI_TILE_DMA128 + v .. DRNMI_TILE_PP256
const ConvKernel* strip_kernel(bool i8);
// The 8-bit families (dtype DRNMI_I8: W8A8, config C5; DRNMI_F8: e4m3) share their tiles.  Variants:
// 0 = 256 x 256 tile / 128-B rows, 1 = 128 x 256 / 128-B, 2 = 256 x 256 / 64-B, 3 = 128 x 256 / 64-B
// (K steps of 128 or 64 channels), 4 = 128 x 256 / 64-B rows, 2 stages, two workgroups per CU
struct Q8Variant {
  int bco;
  ConvKernel k[2];
};
const Q8Variant& q8_variant_row(int dtype, int v);
constexpr int kQ8Occ2 = 4;
bool q8_conv_supported(const drnmi_conv_args& p);      // dtype DRNMI_I8 / DRNMI_F8, cin >= 64, scale non-NULL
bool q8_stag_ok(const drnmi_conv_args& p);
bool big_conv_supported(const drnmi_conv_args& p);
bool strip_ok(const drnmi_conv_args& p);
bool stag_ok(const drnmi_conv_args& p);
bool w1_ok(const drnmi_conv_args& p);
bool w1h_ok(const drnmi_conv_args& p);
bool i8_strip_ok(const drnmi_conv_args& p);
bool i8_w1_ok(const drnmi_conv_args& p);
bool i8_w1h_ok(const drnmi_conv_args& p);

// conv_stag.hip: the strip tile with staggered SIMD partners: 3x3 stride-1, wo % 256 == 0, cin % 128 == 0
const ConvKernel* stag_kernel(int dtype, bool tile128, bool x2);     // DRNMI_I8 / DRNMI_F8: the 256-channel tile, no x2
const SegKernel* stag_seg_kernel(bool i8);
// conv_w1.hip: the same tile as 4 waves of 128 x 128 (one per SIMD), and as 128 x 128 tiles of 4
// waves of 64 x 64 (two workgroups per CU); bit-identical to conv_stag_kernel
const ConvKernel* w1_kernel(bool i8, bool x2);          // i8: no x2 form
const ConvKernel* w1h_kernel(bool i8, bool x2);
const SegKernel* w1_seg_kernel(bool i8);

// conv_sp24.hip: the 2:4 weight-sparse bf16 tiles (dtype DRNMI_BF16_SP24), 256 x 256 or 128 x 256
bool sp24_conv_supported(const drnmi_conv_args& p);
// conv_big.hip: the size and shape terms common to big_conv_supported, q8_conv_supported and sp24_conv_supported
bool big_body_shape_ok(const drnmi_conv_args& p, int min_cin);
const ConvKernel* sp24_kernel(bool tile128, int ks);
const ConvKernel* sp24_strip_kernel();           // 3x3 stride 1, wo % 256 == 0, the 256 x 256 tile (strip_ok)
// conv_sp24_i8.hip: the 2:4 weight-sparse int8 tiles (dtype DRNMI_I8_SP24), cin >= 128, the same two tiles
bool sp24_i8_conv_supported(const drnmi_conv_args& p);
const ConvKernel* sp24_i8_kernel(bool tile128, int ks);
const ConvKernel* sp24_i8_strip_kernel();        // strip_ok on the 256 x 256 tile, as sp24_strip_kernel

// conv_halo.hip: halo-patch 3x3 stride-1 conv, cin / cout 64 or 128
bool halo_conv_supported(const drnmi_conv_args& p);
const ConvKernel* halo_kernel(int cin, int cout);

// conv_s2row.hip: row-walking stride-2 3x3 conv, 32 -> 64 / 64 -> 128, bit-identical to conv_big's
// BK-32 / BK-64 tiles; and the stride-1 3x3 64 -> 64 + folded 1x1 stride-2 downsample from 32
// channels, bit-identical to conv_halo's x2 form
bool s2row_conv_supported(const drnmi_conv_args& p);
bool s1x2row_conv_supported(const drnmi_conv_args& p);
const ConvKernel* s2row_kernel(int cin);
const ConvKernel* s1x2row_kernel();

// conv_x6.hip: fp32-accurate 6-product split-bf16 implicit GEMM: dtype DRNMI_F32X3, cin >= 32;
// rows k[ks - 1]
constexpr int kX6BK = 32;     // input channels per K step
struct X6Variant {
  int bco, bpx, occ;          // tile: channels x pixels, workgroups per CU
  double step;                // seconds per K step of one workgroup tile
  ConvKernel k[3];
};
constexpr int kNumX6 = 6;
const X6Variant& x6_variant(int v);
bool x6_conv_supported(const drnmi_conv_args& p);

// patch_conv.hip / patch_f32.hip: the small-channel LDS-patch convs (DRNMI_ALGO_PATCH); the row
// for these arguments, or nullptr (not supported)
const ConvKernel* patch_kernel(const drnmi_conv_args& p);
const ConvKernel* patch_f32_kernel_row(const drnmi_conv_args& p);

}  // namespace drnmi
