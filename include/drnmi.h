/*
 * drnmi.h — C-ABI of the MI355X-native DRN-D segmentation hot path.
 *
 * Every entry point takes device pointers, plain sizes and a hipStream_t (passed
 * as void*), launches asynchronously on that stream and returns 0 on success or
 * a negative drnmi_status on a rejected argument / a positive hipError_t on a
 * launch failure.  No torch or C++ types cross this boundary; the Python host
 * layer (drnmi/_lib.py) binds it with ctypes, and any other FFI (cgo, JNI,
 * N-API) can bind it the same way.
 *
 * The reference (thejasvi-konduru/video-seg-model-compress) has no native code
 * and no FFI: its hot path is PyTorch ATen ops called from Python.  Each entry
 * point below names the reference code it replaces (file:line in the reference).
 *
 * Layouts: activations are NHWC with a power-of-two channel stride >= 8;
 * weights are packed [cout_pad][k_pad] with k = (kh*ks + kw)*cin + ci.
 * dtype codes: DRNMI_F32 (fp32 parity mode), DRNMI_BF16 (bf16 perf mode).
 */
#ifndef DRNMI_H
#define DRNMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of the argument structs below (drnmi_conv_args, drnmi_wgrad_args).  The structs
 * have grown by appended fields (x2.. in version 2, ws / ws_bytes in version 3); a caller built
 * against another header must not pass them: check drnmi_abi_version() == DRNMI_ABI_VERSION and
 * drnmi_conv_args_size() == sizeof(drnmi_conv_args) once after loading the library (drnmi/_lib.py
 * does, and refuses a mismatched library). */
#define DRNMI_ABI_VERSION 7
int32_t drnmi_abi_version(void);
int64_t drnmi_conv_args_size(void);

enum drnmi_dtype { DRNMI_F32 = 0, DRNMI_BF16 = 1, DRNMI_U8 = 2, DRNMI_I64 = 3, DRNMI_I8 = 4, DRNMI_F32X3 = 5,
                   DRNMI_F8 = 6, DRNMI_BF16_SP24 = 7, DRNMI_I8_SP24 = 8 };
/* DRNMI_F32X3 (conv dtype only, the "fp32x" precision mode): x, res and y are fp32 NHWC as in
 * DRNMI_F32, wgt is three bf16 planes [3][cout_pad][k_pad] with w = w1 + w2 + w3 (an exact split
 * of the fp32 weight), and the conv runs fp32-accurate arithmetic on the bf16 MFMA pipe: each
 * fp32 activation is split the same way in registers and the six products above 2^-24 are
 * accumulated in fp32 (csrc/conv_x6.hip).  Requires cin >= 32 (power of two), ks 1 or 3,
 * out_dtype DRNMI_F32. */
/* DRNMI_F8 (the "fp8" precision mode; version 6): OCP e4m3fn bytes (maximum 448, no infinities,
 * round to nearest even).  The arithmetic, stated once for the kernels and for tests/fp8_ref.py:
 *   element    e4m3(v) = the e4m3fn value nearest to clamp(v, -448, 448), ties to even; the clamp is
 *              done in fp32 before the conversion, so saturation does not depend on the conversion
 *              instruction's mode (torch: v.clamp(-448, 448).to(torch.float8_e4m3fn)).
 *   weights    per output channel: a = absmax(row), q = e4m3(w * 448 / a), s_w = a / 448 (1 for an
 *              all-zero row); packed [cout_pad][k_pad], k = (kh*ks + kw)*cin + ci.
 *   activations per tensor.  A calibrated scale s (DRNSeg._act_scales, "clip = 127 s", shared with
 *              int8) gives the fp8 scale s8 = s * 127 / 448: q = e4m3(x * (1 / s8)).
 *   launch     dtype = DRNMI_F8: x, wgt, res are e4m3 bytes; scale non-NULL = s_w * s8_x * bn_scale.
 *              acc = fp32 sum of the exact products (v_mfma_f32_16x16x128_f8f6f4, K in steps of 128);
 *              v = acc * scale[co] + shift[co] (fmul then fadd, no contraction);
 *              v += f32(res) * res_scale (residual, if any); ReLU (if set);
 *              out_dtype DRNMI_F8 stores e4m3(v * out_scale), DRNMI_BF16 / DRNMI_F32 store v with
 *              the strided forms of the int8 launches (NCHW logits, NHWC rows with y_sp = cs).
 *              drnmi_conv_args does not grow: scale, res_scale and out_scale are reused.
 *   kernels    cin >= 64 (power of two), ks 1 or 3, cout_pad % 128 == 0, k_pad == k: conv_f8_kernel
 *              (any stride / dilation / ragged tiles; the 1x1s on its two-workgroups-per-CU form
 *              conv_f8_occ2_kernel); whole 256-pixel output rows of a stride-1 3x3
 *              with cin % 256 == 0 and cout % 256 == 0 take the strip-staged conv_f8_stag_kernel
 *              (DRNMI_TILE_STAG forces it).  DRNMI_TILE_W1 / DRNMI_TILE_W1H, drnmi_conv_stag_seg, a
 *              unit mask and a fused second input have no fp8 form: DRNMI_ENOTSUP. */

/* DRNMI_BF16_SP24 (conv dtype only; version 7; inference, opt-in: DRNSeg.set_sparse24): a bf16 launch
 * whose weights have at most two non-zeros in every group of four consecutive packed columns (a
 * group is 4 consecutive input channels of one tap: k = (kh*ks + kw)*cin + ci, cin % 4 == 0), run on
 * the 2:4 structured-sparse MFMA v_smfmac_f32_16x16x64_bf16 (csrc/conv_sp24.hip: its own main loop on
 * the gather pieces and epilogues of csrc/conv_tile.h, as the dense tiles of csrc/conv_big_body.h).  x, res and y are
 * as in a DRNMI_BF16 launch; wgt is the blob drnmi_sp24_pack wrote (0.5625 x the dense bytes: the
 * kept values and their 2-bit positions; its layout is private to the kernel); scale must be NULL
 * (folded into the weights before packing).
 *   shapes   cin a power of two >= 64, ks 1 or 3 at any stride / dilation, any M, cout_pad % 128 == 0
 *            (256 x 256 tiles when cout_pad % 256 == 0, else 128 x 256), k_pad == k, out_dtype
 *            DRNMI_BF16 (NHWC rows) or DRNMI_F32 (any strides), residual and ReLU.
 *   refused  DRNMI_ENOTSUP: x2, unit_mask, a non-NULL scale, drnmi_conv_stag_seg; DRNMI_EINVAL: cin not
 *            a power of two and whatever every launch is refused for.
 *   tile     read as this dtype's own variant: DRNMI_SP24_GATHER (the per-tap gather, every shape above),
 *            DRNMI_SP24_STRIP (strip-staged pixels: 3x3, stride 1, pad == dil <= 4, wo % 256 == 0, on
 *            the 256-channel tile; DRNMI_ENOTSUP elsewhere; measured no faster than the gather, kept for
 *            A/B runs) or DRNMI_TILE_AUTO (the gather).  The two forms add in the same order:
 *            bit-identical.
 * Operand map of the instruction, measured on gfx950 (tests/test_gpu_sp24.py::test_operand_map;
 * lane = 16 fq + fr, D = A x B with A 16 x 64 sparse, B 64 x 16 dense):
 *   A    8 bf16 per lane: row fr, the kept values of dense k 16 fq .. 16 fq + 15; elements 2 g and
 *        2 g + 1 are the kept pair of group g (k 16 fq + 4 g .. + 3), lower position first;
 *   idx  one 32-bit register per lane; ABID (0 / 1) selects its low / high 16 bits; bits
 *        [2 s + 1 : 2 s] of that half are the position (0..3) of A element s inside its group.  A
 *        group with fewer than two non-zeros still names two positions (zeros are kept there);
 *   B    16 bf16 per lane: column fr, elements 0-7 = k 8 fq .. 8 fq + 7, elements 8-15 = k 32 + 8 fq ..
 *        + 7 (two v_mfma_f32_16x16x32_bf16 B fragments side by side);
 *   D    4 fp32 per lane: rows 4 fq .. 4 fq + 3 of column fr, as the dense 16x16 MFMAs. */
enum drnmi_sp24_tile { DRNMI_SP24_GATHER = 0, DRNMI_SP24_STRIP = 1 };

/* DRNMI_I8_SP24 (conv dtype only; inference, opt-in: DRNSeg.set_sparse24 at precision "int8"): a DRNMI_I8
 * launch whose weights are 2:4 along the input channels of a tap (the groups of DRNMI_BF16_SP24), run on
 * v_smfmac_i32_16x16x128_i8 (csrc/conv_sp24_i8.hip).  Added under ABI version 7: a new enum value and
 * three new symbols, drnmi_conv_args unchanged, so callers built against the earlier version-7 header
 * keep working (backward compatible).  The contract is DRNMI_I8's exactly: x and res int8 NHWC, scale
 * non-NULL, res_scale, ReLU, out_scale, output DRNMI_I8 (NHWC), DRNMI_BF16 or DRNMI_F32 at any strides;
 * wgt is the blob drnmi_sp24_pack_i8 wrote (0.625 x the dense bytes).  int32 accumulation is exact, so
 * the output equals the DRNMI_I8 launch on the dense weights bit for bit.
 *   shapes   cin a power of two >= 128 (a K step is 128 dense channels of one tap), ks 1 or 3 at any
 *            stride / dilation, any M, cout_pad % 128 == 0 (the 256 x 256 tile when cout_pad % 256 == 0
 *            and cout > 128, else 128 x 256), k_pad == k == ks*ks*cin.
 *   refused  DRNMI_ENOTSUP: x2, unit_mask, a NULL scale, cin 64, drnmi_conv_stag_seg; DRNMI_EINVAL: cin
 *            not a power of two and whatever every launch is refused for.
 *   tile     enum drnmi_sp24_tile as for DRNMI_BF16_SP24: DRNMI_TILE_AUTO is the gather; DRNMI_SP24_STRIP
 *            (3x3, stride 1, pad == dil <= 4, wo % 256 == 0, the 256-channel tile) is bit-identical.
 * Operand map of the instruction, measured on gfx950 (tests/test_gpu_sp24_i8.py::test_operand_map;
 * lane = 16 fq + fr, D = A x B with A 16 x 128 sparse, B 128 x 16 dense):
 *   A    16 int8 per lane: row fr, the kept values of dense k 32 fq .. 32 fq + 31; bytes 2 g and 2 g + 1
 *        are the kept pair of group g (k 32 fq + 4 g .. + 3), lower position first;
 *   idx  the whole 32-bit register: bits [2 s + 1 : 2 s] = byte s's position in its group; ABID unused;
 *   B    32 int8 per lane: column fr, bytes 0-15 = k 16 fq .. 16 fq + 15, bytes 16-31 = k 64 + 16 fq ..
 *        + 15 (two v_mfma_i32_16x16x64_i8 B fragments side by side);
 *   D    4 int32 per lane: rows 4 fq .. 4 fq + 3 of column fr, as the dense 16x16 MFMAs. */

enum drnmi_status {
  DRNMI_OK = 0,
  DRNMI_EINVAL = -1,     /* bad shape / stride / dtype combination */
  DRNMI_ENOTSUP = -2,    /* no kernel instantiated for this configuration */
};

/* One fused convolution: y = act(conv(x, w) * scale + shift [+ res]).
 * Replaces conv3x3 + BatchNorm2d + ReLU (+ residual add) of the reference:
 *   lmodels/drn.py:27-29   conv3x3
 *   lmodels/drn.py:49-65   BasicBlock.forward (conv-bn-relu, conv-bn, += residual, relu)
 *   lmodels/drn.py:86-106  Bottleneck.forward (1x1 / 3x3 / 1x1 + residual)
 *   lmodels/drn.py:132-137 layer0 (7x7 stem) ; :181-186 downsample (1x1 stride s + BN)
 *   lmodels/drn.py:201-211 _make_conv_layers (conv-bn-relu stacks, layer1/2/7/8)
 *   lmodels/drnseg.py:278-284 seg (1x1 conv + bias, scale = 1, shift = bias)
 * Output addressing: y[img*y_sn + pixel*y_sp + c*y_sc] (pixel = oh*wo + ow), so
 * the same kernel writes NHWC activations or the NCHW fp32 logits tensor. */
typedef struct drnmi_conv_args {
  const void* x;       /* NHWC input [n][h][w][cin]                                   */
  const void* wgt;     /* packed weights [cout_pad][k_pad]                            */
  const float* scale;  /* [cout_pad] folded BN scale, or NULL = 1 (scale pre-folded    */
                       /* into wgt; lets the bf16 kernels start from shift + res)    */
  const float* shift;  /* [cout_pad] folded BN shift (or conv bias)                   */
  const void* res;     /* optional NHWC residual [n*ho*wo][cout] in x's dtype, or NULL */
  void* y;             /* output                                                      */
  int64_t y_sn, y_sp, y_sc; /* output strides in elements                          */
  int32_t n, h, w, cin;     /* cin: channel stride of x, power of two >= 8          */
  int32_t ho, wo, cout, cout_pad;
  int32_t ks, stride, pad, dil;
  int32_t k, k_pad;         /* k = ks*ks*cin ; k_pad = round_up(k, 32)              */
  int32_t relu;             /* 1: ReLU after the (optional) residual add            */
  int32_t dtype;            /* DRNMI_BF16 or DRNMI_F32: x, w, res                   */
  int32_t out_dtype;        /* DRNMI_BF16 or DRNMI_F32: y                           */
  int32_t tile;             /* enum drnmi_tile (below), DRNMI_TILE_AUTO = -1        */
  int32_t algo;             /* DRNMI_ALGO_IGEMM or DRNMI_ALGO_PATCH (see below)     */
  int32_t src_u8;           /* PATCH only: x is uint8 HWC3 frames, normalised on load */
  int32_t bgr;              /* src_u8: swap channel 0 and 2 on read                  */
  float mean[3], std[3];    /* src_u8: (u8 / 255 - mean[c]) / std[c], fp32          */
  const uint32_t* unit_mask; /* optional block-sparsity map of wgt (drnmi_weight_unit_mask):  */
                             /* bit (rb, ku) = 0 -> rows 16rb..16rb+15 x packed K columns   */
                             /* 32ku..32ku+31 are all zero and their MFMAs are skipped      */
                             /* (bf16 LDS-DMA kernels; NULL = dense).  Results are bit-     */
                             /* identical to the dense kernel on the same weights.          */
  /* W8A8 (dtype DRNMI_I8: x, wgt, res int8; per-tensor symmetric activations, per-channel  */
  /* weights; BASELINE config C5).  acc = int32 sum; v = float(acc) * scale[c] + shift[c];  */
  /* v += float(res) * res_scale; ReLU; out_dtype DRNMI_I8 stores                           */
  /* clamp(rint(v * out_scale), -127, 127), BF16 / F32 store v.  Each step is one fp32        */
  /* rounding (no fused multiply-add), so a scalar restatement reproduces it bit for bit.  */
  /* scale must be non-NULL for int8.  Ignored for other dtypes.                             */
  float res_scale;
  float out_scale;            /* 1 / (scale of the int8 output activation)                */
  /* Fused second input (bf16 LDS-DMA kernels, x2 != NULL): y = act(conv(x, w) + conv1x1_s(x2, w2)
   * * scale + shift) as ONE implicit GEMM over the concatenated K [ks*ks*cin | cin2]; wgt rows hold
   * [w | w2] (k = ks*ks*cin + cin2).  This folds a BasicBlock / Bottleneck 1x1 downsample
   * (lmodels/drn.py:181-186, its BN scale folded into w2, shifts summed) into the block's last
   * conv, so the residual branch is never written to HBM.  x2: NHWC [n][h2][w2][cin2], sampled at
   * (oh*stride2, ow*stride2); res must be NULL.  x2 = NULL: unused.  Two accepted forms:
   *   conv_big (cin >= 256 tiles): cin2 % 64 == 0 and k_pad == k;
   *   conv_halo (stride-1 3x3 with cin = cout 64 or 128, layer3/layer4): cin2 == 32 or 64,
   *     k_pad = round_up(k, 64) with zero columns after w2, scale == NULL (BN scales folded
   *     into the weights, shifts summed in shift).  Other combinations return
   *     DRNMI_ENOTSUP.                                                                       */
  const void* x2;
  int32_t cin2, h2, w2, stride2;
  /* Optional fp32 scratch (16-B aligned) of the F32X3 kernel (conv_x6): a launch given one takes
   * the training plan -- a tile variant and split-K count chosen for grids that leave CUs idle
   * (the K range split over gridDim.y workgroups per tile, their partial sums land here and a
   * second kernel adds them in split order and applies the epilogue).  Size:
   * drnmi_conv_workspace_bytes (0 = the plan is the inference one: pass NULL).  ws = NULL keeps
   * the inference plan (the inference engine's launches).  DRNMI_F32 launches of the implicit GEMM
   * read only whether it is set: with one (any 16-B aligned pointer, nothing is written) a conv of
   * K >= 1024 sums K in chains of 256 (K = 512 .. 1023: of 128) folded into a second fp32 accumulator, which keeps its
   * error against float64 at that of a blocked fp32 sum; without, K is one fmaf chain, the order
   * the fp32 inference parity is pinned in.  Other dtypes ignore it. */
  void* ws;
  int64_t ws_bytes;
  /* Optional train-mode BN statistics of the stored output (F32X3 conv_x6 launches that do not
   * split K: drnmi_conv_stats_rows(args) > 0): the epilogue writes per-channel fp64 partial sums
   * of y and y^2, one row per 64-pixel wave slice, as [2][rows][cout] (sums, then sums of
   * squares), in a fixed order.  drnmi_bn_stats_partials_f32 turns them into the batch mean /
   * invstd with the same finalize as drnmi_bn_stats_f32 (mean, biased variance, invstd, running-
   * stat update; semantic_seg.py:166-230's train-mode BatchNorm2d after the conv), without reading
   * y again.  The fp64 sums are added in a different fixed order than drnmi_bn_stats_f32's row
   * splits, so the two agree to fp32 rounding, not bit for bit.  NULL: off. */
  double* stats;
  /* Optional output row stride in elements (F32X3 conv_x6 launches only): y(n, oh, ow, c) =
   * y[n*y_sn + oh*y_sr + ow*y_sp + c*y_sc]; a residual then has y's layout.  0 = rows packed
   * (oh*wo*y_sp).  A stride-2 conv's data gradient runs as four of these launches, one per output
   * parity class, writing every other pixel of every other row (drnmi_dgrad_s2_class_planes).  With
   * y_sr != 0 the output size is free (ho x wo need not follow the conv formula): taps past the
   * input's edges read zeros. */
  int64_t y_sr;
} drnmi_conv_args;

/* Algorithms behind drnmi_conv2d_bn_act:
 *  DRNMI_ALGO_IGEMM  NHWC implicit GEMM (any power-of-two cin >= 8, any ks/stride/dil; bf16 or
 *                    fp32), on the tile drnmi_conv_args.tile names (enum drnmi_tile below).
 *  DRNMI_ALGO_PATCH  bf16-only small-channel direct conv for the full-resolution layers
 *                    (lmodels/drn.py:132-137 layer0, :201-211 layer1/layer2): the input tile
 *                    plus halo is staged once in LDS and reused by all ks*ks taps; weights stay
 *                    in registers; the MFMA puts output channels on rows so each lane stores 4
 *                    contiguous channels (coalesced NHWC stores).  Supports dil = 1,
 *                    (cin, cout, ks, stride) in {(8,16,7,1), (16,16,3,1), (16,32,3,2), (32,64,3,2)},
 *                    no residual, packed NHWC output; and the
 *                    fused stem src_u8 = 1 with (cin = 4, cout = 16, ks = 7, stride = 1): weights
 *                    packed [cout_pad][224] with k = kh*32 + kw*4 + c (kw < 8, c < 4; kw = 7 and
 *                    c = 3 are zero), which also replaces the frame-ingest kernel. */
enum drnmi_algo { DRNMI_ALGO_IGEMM = 0, DRNMI_ALGO_PATCH = 1 };

/* drnmi_conv_args.tile of a DRNMI_ALGO_IGEMM launch, in the order of drnmi_conv_tile_name.
 * DRNMI_TILE_AUTO picks the bf16 LDS-DMA kernel (DMA128 / DMA256 / DMA64K32 / DMA64: 128 / 256 /
 * 64 / 64 output channels x 256 pixels, 64-channel K steps but DMA64K32's 32; cin >= 32, ks 1 or
 * 3) when it applies, else a register-staged tile IGEMM_* by cout.  Whole 256-pixel output rows
 * (3x3, stride 1, cin % 128 == 0) route to the strip tiles: STAG (256 / 128 channels, 8 waves
 * with staggered SIMD partners), W1 (the same tile as 4 waves of 128 x 128, one per SIMD; auto at
 * cin >= 512 without residual), W1H (128 x 128 tiles, two workgroups per CU; auto at cout 128) --
 * all with the same K order, so bit-identical.  int8 (dtype DRNMI_I8) takes STAG / W1 / W1H as its
 * int8 forms (auto: W1H at cin, cout <= 256, else STAG) and ignores the other ids.  The forced ids
 * exist for the bit-identity tests and A/B runs.  DRNMI_F32X3 (conv_x6) reads tile >= 0 in its own
 * encoding instead: tile % 6 is the conv_x6 variant and, when tile >= 6, tile / 6 the split-K
 * count (only with a workspace). */
enum drnmi_tile {
  DRNMI_TILE_AUTO = -1,
  DRNMI_TILE_IGEMM_128X128 = 0, DRNMI_TILE_IGEMM_128X64 = 1, DRNMI_TILE_IGEMM_256X32 = 2, DRNMI_TILE_IGEMM_256X16 = 3,
  DRNMI_TILE_DMA128 = 4, DRNMI_TILE_DMA256 = 5, DRNMI_TILE_DMA64K32 = 6, DRNMI_TILE_DMA64 = 7,
  DRNMI_TILE_DMA256K32 = 8, DRNMI_TILE_DMA128K32 = 9,
  DRNMI_TILE_DMA128P = 10, DRNMI_TILE_DMA256P = 11, DRNMI_TILE_DMA64K32P = 12, DRNMI_TILE_DMA64P = 13,
  DRNMI_TILE_DMA256K32P = 14, DRNMI_TILE_DMA128K32P = 15,      /* the same six, persistent */
  DRNMI_TILE_PP256 = 16,           /* ping-pong 4-phase schedule */
  DRNMI_TILE_HALO = 17,            /* conv_halo: 4 x 64 pixel blocks, cin / cout 64 or 128 */
  DRNMI_TILE_STRIP = 18,           /* strip-staged B (3x3, wo % 256 == 0) */
  DRNMI_TILE_STAG = 19,
  DRNMI_TILE_S2ROW = 20,           /* stride-2 3x3 32 -> 64 / 64 -> 128 row walk */
  DRNMI_TILE_S1X2ROW = 21,         /* stride-1 3x3 64 -> 64 + 1x1 stride-2 downsample from 32 channels */
  DRNMI_TILE_W1 = 22,
  DRNMI_TILE_W1H = 23,
  DRNMI_TILE_COUNT = 24            /* drnmi_conv_num_tiles() */
};

int drnmi_conv2d_bn_act(const drnmi_conv_args* args, void* stream);

/* The status drnmi_conv2d_bn_act would refuse these arguments with (DRNMI_EINVAL / DRNMI_ENOTSUP),
 * or 0 when it would launch; no launch is made and x, wgt, shift, y are not looked at.
 * drnmi_conv_kernel_name(args) is NULL exactly when this is not 0. */
int drnmi_conv_status(const drnmi_conv_args* args);

/* Rows of the args->stats partials this launch writes (4 per 256-pixel tile), or 0 when it
 * cannot produce them (not conv_x6, or a split-K plan: compute the statistics from y). */
int64_t drnmi_conv_stats_rows(const drnmi_conv_args* args);

/* Bytes of args->ws the training plan of these arguments needs (0: the inference plan; 256: a
 * different tile variant, no split; else S x M x cout x 4 for S split-K partitions; -1: NULL).
 * Only DRNMI_F32X3 implicit-GEMM launches use it (drnmi/train.py passes it for the fp32x
 * fine-tune); the plan depends on the geometry alone, so a size queried once per layer holds for
 * every step. */
int64_t drnmi_conv_workspace_bytes(const drnmi_conv_args* args);

/* Fused stem + layer1 (bf16, csrc/patch_conv.hip stem_l1_kernel): replaces the two launches
 *   drnmi_conv2d_bn_act(stem); drnmi_conv2d_bn_act(next)
 * of lmodels/drn.py:132-137 (layer0 7x7 3->16 + BN + ReLU on the uint8 frame) and :201-211
 * (layer1 3x3 16->16 + BN + ReLU) with one, bit-identical to them; the stem output is never
 * written (stem->y is ignored).  stem: the src_u8 = 1 PATCH contract above (cin 4, cout 16,
 * ks 7, pad 3, k = k_pad = 224); next: cin 16, cout 16, ks 3, stride 1, pad 1, dil 1,
 * k = 144, k_pad >= 160, no residual, packed NHWC bf16 output, same n/h/w as the stem.
 * DRNMI_EINVAL for anything else.  drnmi_stem_layer1_kernel_name: "stem_l1_kernel" or NULL. */
int drnmi_stem_layer1(const drnmi_conv_args* stem, const drnmi_conv_args* next, void* stream);
const char* drnmi_stem_layer1_kernel_name(const drnmi_conv_args* stem, const drnmi_conv_args* next);

/* Fused video front (bf16 perf mode, csrc/front.hip front_kernel): uint8 HWC3 frames -> layer0
 * (7x7 3->16 + BN + ReLU, lmodels/drn.py:132-137, on the normalised frame of data_transforms.py:
 * 109-125, 256-281) -> layer1 (3x3 16->16 + BN + ReLU, drn.py:201-211) -> layer2 (3x3 stride 2
 * 16->32 + BN + ReLU) in one launch: neither the 16-channel full-resolution stem output nor
 * layer1's is ever written; the layer2 output y is NHWC bf16 [n][(h+1)/2][(w+1)/2][32].
 * Arithmetic: the stem runs f16 MFMAs on the exact frame bytes (1024 + u8 is exact in f16) with the
 * normalisation and the stem's BN scale folded into f16 weights w * scale / (255 std[c]); the
 * offset 1024 and the mean term are subtracted through a per-border-case shift (the reference
 * zero-pads in normalised space, so the shift depends on which taps fall inside the image);
 * layer1 / layer2 are bf16 MFMAs (BN scale folded into bf16 weights) on bf16 activations.
 *   drnmi_front_pack: HOST function, no GPU: packs the three convs' OIHW fp32 weights (w0
 *     [16][3][7][7], w1 [16][16][3][3], w2 [32][16][3][3]), their folded BN scale/shift
 *     (scale*: NULL = 1), mean/std (3 each, per model channel) and bgr into a host buffer of
 *     drnmi_front_pack_bytes() bytes that the caller copies to the device once.
 *   drnmi_video_front_u8: frames [n][h][w][3] uint8 (bgr as packed), pack = the device copy;
 *     requires w % 4 == 0, h >= 8, w >= 8, n*h*w*3 < 2^31 (DRNMI_EINVAL otherwise).
 *   drnmi_front_supported: 1 if drnmi_video_front_u8 takes (n, h, w).
 * Replaces ToTensorVideoImage + Normalize + layer0 + layer1 + layer2 of the seg_video loop
 * (seg_video_old_no_plot.py:157-169 -> lmodels/drnseg.py:295-299 -> drn.py:213-259). */
int64_t drnmi_front_pack_bytes(void);
int drnmi_front_pack(const float* w0, const float* scale0, const float* shift0, const float* w1, const float* scale1,
                     const float* shift1, const float* w2, const float* scale2, const float* shift2,
                                      const float* mean3, const float* std3, int32_t bgr, void* out_host);
int drnmi_front_supported(int32_t n, int32_t h, int32_t w);

/* Fused 64-channel BasicBlock (lmodels/drn.py:49-65 with inplanes = planes = 64, stride 1,
 * dilation 1, no downsample: DRN-D-22 layer3.1, D-38 layer3.1/3.2):
 *   y = relu(bn2(conv3x3(relu(bn1(conv3x3(x))))) + x), bf16 NHWC [n][h][w][64] in and out, eval BN
 *   (scale folded into the weights, shift added; fp32 accumulation).
 * The intermediate never reaches HBM (csrc/block64.hip).  `pack`: device copy of the blob that the
 * HOST function drnmi_block64_pack(w1, scale1, shift1, w2, scale2, shift2, out) builds from the two
 * convs' OIHW fp32 weights [64][64][3][3] and per-channel BN scale / shift (fp32 [64] each);
 * drnmi_block64_pack_bytes() bytes.  x and y must not alias. */
int64_t drnmi_block64_pack_bytes(void);
int drnmi_block64_pack(const float* w1, const float* scale1, const float* shift1, const float* w2,
                       const float* scale2, const float* shift2, void* out_host);
int drnmi_block64_supported(int32_t n, int32_t h, int32_t w);
int drnmi_basic_block64(const void* x, const void* pack, void* y, int32_t n, int32_t h, int32_t w, void* stream);
int drnmi_video_front_u8(const uint8_t* frames, const void* pack, void* y, int32_t n, int32_t h, int32_t w,
                         void* stream);

/* Fused 16-channel BasicBlock (lmodels/drn.py:49-65 with inplanes = planes = 16, stride 1, dilation 1,
 * no downsample: DRN-C layer1, lmodels/drn.py:127-128):
 *   y = relu(bn2(conv3x3(relu(bn1(conv3x3(x))))) + x), bf16 NHWC [n][h][w][16] in and out, eval BN
 *   (scale folded into the weights, shift added; fp32 accumulation; the intermediate rounded to bf16).
 * The intermediate never reaches HBM (csrc/block16.hip).  `pack`: device copy of the blob that the
 * HOST function drnmi_block16_pack(w1, scale1, shift1, w2, scale2, shift2, out) builds from the two
 * convs' OIHW fp32 weights [16][16][3][3] and per-channel BN scale / shift (fp32 [16] each);
 * drnmi_block16_pack_bytes() bytes.  drnmi_block16_supported: n, h, w >= 1 and n * h * w * 32 < 2^31.
 * x and y must not alias.  Arguments are validated before any HIP call. */
int64_t drnmi_block16_pack_bytes(void);
int drnmi_block16_pack(const float* w1, const float* scale1, const float* shift1, const float* w2,
                       const float* scale2, const float* shift2, void* out_host);
int drnmi_block16_supported(int32_t n, int32_t h, int32_t w);
int drnmi_basic_block16(const void* x, const void* pack, void* y, int32_t n, int32_t h, int32_t w, void* stream);

/* Block-sparsity map of packed weights [rows_pad][k_pad] (dtype F32 or BF16): one bit per
 * 16-row x 32-column unit, bit = 1 iff any element of the unit is nonzero (+-0 count as zero);
 * layout: row-block rb owns words [rb*W, rb*W + W), W = ceil(k_pad / 32 / 32), unit ku at bit
 * ku % 32 of word ku / 32.  mask must hold (rows_pad / 16) * W words; *nonzero_units (device
 * int32, NULL-able) receives the count of nonzero units.  This is how pruner masks reach the
 * MFMA path: MFMA runs only on the dense-within-block sub-tiles (BlockPruner blocks of whole
 * kernels, BlockPruner.py:139-241, with block_width a multiple of 32 input channels map 1:1 to
 * units; narrower blocks skip where neighbouring blocks are both pruned). */
int drnmi_weight_unit_mask(const void* wgt, int32_t dtype, int32_t rows_pad, int32_t k_pad, uint32_t* mask,
                           int32_t* nonzero_units, void* stream);

/* 2:4 packing for DRNMI_BF16_SP24 (csrc/conv_sp24.hip).  dense_bf16: packed bf16 weights
 * [rows_pad][k_pad] (rows_pad % 32 == 0, k_pad % 64 == 0, device memory); out: device buffer of
 * drnmi_sp24_pack_bytes(rows_pad, k_pad) = rows_pad * k_pad * 9 / 8 bytes (-1 for other sizes), 16-B
 * aligned.  For every group of four consecutive packed columns the kernel writes the kept values and
 * their positions in its own layout (private: nothing else reads the blob).  *violations (device int32,
 * NULL-able) receives the number of groups with more than two non-zeros (+-0 count as zero); a blob
 * with violations drops weights (the first two non-zeros of such a group are kept) and must not be
 * launched.
 * drnmi_sp24_mma_probe: one v_smfmac_f32_16x16x64_bf16 on one wave with a zero accumulator, for the
 * operand-map test: a [64][8] bf16, b [64][16] bf16, idx [64] words, d [64][4] fp32 per lane, abid 0 / 1. */
int64_t drnmi_sp24_pack_bytes(int32_t rows_pad, int32_t k_pad);
int drnmi_sp24_pack(const void* dense_bf16, int32_t rows_pad, int32_t k_pad, void* out, int32_t* violations,
                    void* stream);
int drnmi_sp24_mma_probe(const void* a, const void* b, const uint32_t* idx, float* d, int32_t abid, void* stream);
/* Issue-rate loop for scripts/sp24_micro.py: `blocks` workgroups of four waves (one per SIMD), every wave
 * iters x 8 back-to-back MFMAs on 8 accumulators, operands in registers: sparse != 0 runs
 * v_smfmac_f32_16x16x64_bf16, else v_mfma_f32_16x16x32_bf16.  sink: blocks x 256 floats. */
int drnmi_sp24_issue_probe(int32_t sparse, int32_t iters, int32_t blocks, float* sink, void* stream);

/* 2:4 packing for DRNMI_I8_SP24 (csrc/conv_sp24_i8.hip), the rules of drnmi_sp24_pack on int8.  dense_i8:
 * packed int8 weights [rows_pad][k_pad] (rows_pad % 32 == 0, k_pad % 128 == 0, device memory); out: device
 * buffer of drnmi_sp24_pack_i8_bytes(rows_pad, k_pad) = rows_pad * k_pad * 5 / 8 bytes (-1 for other
 * sizes: half the values plus 2 bits per kept value), 16-B aligned, layout private to the kernel.  A zero
 * is the value 0; groups fill up from position 3 downwards; *violations (device int32, NULL-able, reset by
 * every call) counts the groups with more than two non-zeros, and a blob with violations must not be
 * launched.  Arguments are refused (DRNMI_EINVAL) before any HIP call.
 * drnmi_sp24_mma_probe_i8: one v_smfmac_i32_16x16x128_i8 on one wave with a zero accumulator, for the
 * operand-map test: a [64][16] int8, b [64][32] int8, idx [64] words, d [64][4] int32 per lane. */
int64_t drnmi_sp24_pack_i8_bytes(int32_t rows_pad, int32_t k_pad);
int drnmi_sp24_pack_i8(const void* dense_i8, int32_t rows_pad, int32_t k_pad, void* out, int32_t* violations,
                       void* stream);
int drnmi_sp24_mma_probe_i8(const void* a, const void* b, const uint32_t* idx, int32_t* d, void* stream);

/* W8A8 helpers (BASELINE config C5; csrc/quant.hip).  The reference has no quantisation code
 * (SURVEY.md C5 row): the scheme is ours.  Activations are per-tensor symmetric int8.
 *   drnmi_quantize_i8: y[i] = clamp(rint(x[i] * inv_scale), -127, 127) over n elements
 *     (x BF16 or F32, n % 8 == 0; one fp32 multiply, round-half-even) -- the bf16 -> int8
 *     boundary in front of the first int8 conv.
 *   drnmi_absmax: *out = max |x[i]| (device float; calibration of the activation scales).
 *   drnmi_abs_histogram: the exact distribution of |x|, for scales other than absmax / 127 and
 *     for calibration streamed over many batches.  hist is a device array of DRNMI_HIST_BINS
 *     64-bit counters; x[i] (BF16 or F32, n % 8 == 0) adds 1 to bin
 *     (bits((float)x[i]) & 0x7fffffff) >> 16.  For BF16 input that is one bin per representable
 *     magnitude: bin b counts the elements whose |x| has the bf16 pattern b, +0 and -0 both in
 *     bin 0, inf / NaN in bins 0x7f80 and up.  F32 input is binned by TRUNCATION to its top 16
 *     bits (bin b counts |x| in [value(b), value(b + 1))), not by rounding to bf16.  The call
 *     ACCUMULATES and never zeroes hist: zero it once, then stream any number of batches through
 *     (64-bit counters do not wrap).  Percentile and MSE-optimal scales are derived from the
 *     histogram on the host (drnmi/calibrate.py); the scales themselves are plain floats a
 *     deployment stores next to its weights (DRNSeg.int8_state / load_int8_state, and
 *     <checkpoint>.int8.json of drnmi/checkpoint.py), so no calibration frames are needed at
 *     start-up.  NULL pointers, n % 8 != 0 or another dtype: DRNMI_EINVAL before any HIP call;
 *     n == 0: DRNMI_OK, nothing launched. */
#define DRNMI_HIST_BINS 32768
int drnmi_quantize_i8(const void* x, int32_t dtype, int8_t* y, int64_t n, float inv_scale, void* stream);
/* The fp8 sibling (DRNMI_F8 above): y[i] = e4m3(x[i] * inv_scale) over n elements, x BF16 or F32, one
 * fp32 multiply, the clamp to +-448, round to nearest even; any n >= 1 (16 elements per lane, a
 * scalar tail).  NULL pointers, x or y not 16-byte aligned, n <= 0, another dtype or a non-positive
 * inv_scale: DRNMI_EINVAL before any HIP call.  One streaming kernel on the caller's stream, no allocation (graph-capturable). */
int drnmi_quantize_f8(const void* x, int32_t dtype, int64_t n, float inv_scale, uint8_t* y, void* stream);
int drnmi_absmax(const void* x, int32_t dtype, int64_t n, float* out, void* stream);
int drnmi_abs_histogram(const void* x, int32_t dtype, int64_t n, int64_t* hist, void* stream);

/* Name of the kernel (template instance) drnmi_conv2d_bn_act would launch for these
 * arguments, e.g. "conv_big_kernel<3, 128, 2, 2>"; NULL if it would refuse them (the same
 * decision: drnmi_conv_status; x, wgt, shift, y may be NULL).  No launch, no GPU needed.
 * (Used by bench.py to attribute timed launches to kernels as rocprofv3 names them.) */
const char* drnmi_conv_kernel_name(const drnmi_conv_args* args);

/* Name of a tile configuration ("128x128", ...) or NULL; count via drnmi_conv_num_tiles. */
const char* drnmi_conv_tile_name(int tile);
int drnmi_conv_num_tiles(void);

/* Frame ingest: uint8 HWC frames -> normalised NHWC (channel stride 8, c>=3 zero).
 * Replaces ToTensorVideoImage + Normalize (data_transforms.py:256-281, :109-125;
 * constants info.json:1): v = (u8 / 255 - mean[c]) / std[c] in fp32, then cast.
 * bgr != 0 swaps channel order on read (seg_video_old_no_plot.py:125 feeds cv2's
 * BGR frames as "RGB"; bgr = 0 reproduces that quirk when given cv2 frames). */
/* mean3 / std3 are HOST pointers to 3 floats (passed by value to the kernel). */
int drnmi_frame_ingest_u8(const uint8_t* frames, void* out, int32_t n, int32_t h, int32_t w,
                          const float* mean3, const float* std3, int32_t bgr,
                          int32_t out_dtype, void* stream);

/* fp32 NCHW [n][c][h][w] -> NHWC [n][h][w][c_pad] in out_dtype, zero-filling c..c_pad-1.
 * The boundary conversion for DRNSeg.forward(x) (lmodels/drnseg.py:295-299 takes NCHW fp32). */
int drnmi_nchw_to_nhwc(const float* x, void* out, int32_t n, int32_t c, int32_t h, int32_t w,
                       int32_t c_pad, int32_t out_dtype, void* stream);

/* NHWC [n][h][w][c_stride] (first c channels) -> fp32 NCHW [n][c][h][w]. Debug/parity taps. */
int drnmi_nhwc_to_nchw(const void* x, float* out, int32_t n, int32_t c, int32_t h, int32_t w,
                       int32_t c_stride, int32_t in_dtype, void* stream);

/* Fused up x8 + LogSoftmax(dim=1) + argmax over classes.
 * Replaces the depthwise ConvTranspose2d(c, c, 16, stride 8, pad 4, groups=c) with the
 * bilinear fill_up_weights kernel, the LogSoftmax and torch.max(final, 1):
 *   lmodels/drnseg.py:257-266, :285-299 ; semantic_seg.py:445 ; seg_video_old_no_plot.py:166
 * logits: fp32 NCHW [n][c][h][w]; up_w: fp32 [16][16] (one depthwise plane, all planes equal);
 * logprobs: fp32 NCHW [n][c][8h][8w] or NULL; labels: [n][8h][8w] uint8 or int64 (label_dtype)
 * or NULL.  Ties in argmax resolve to the lowest class index.
 * 1 <= c <= 256 (what a uint8 label map holds), else DRNMI_ENOTSUP.  c <= 32 keeps the class vector
 * in registers; 33 <= c <= 256 runs the three-sweep LDS-patch kernel (csrc/head_wide.hip: same
 * per-pixel arithmetic in the same order), which needs logprobs 16-byte and labels 4-byte (uint8)
 * or 8-byte (int64) aligned, else DRNMI_EINVAL. */
int drnmi_up8_logsoftmax_argmax(const float* logits, const float* up_w, float* logprobs,
                                void* labels, int32_t label_dtype, int32_t n, int32_t c,
                                int32_t h, int32_t w, void* stream);

/* The 33 .. 256-class kernel of drnmi_up8_logsoftmax_argmax for any 1 <= c <= 256 (same arguments,
 * same alignment rule): what the tests use to pin it bit for bit against the c <= 32 kernels.
 * Not a faster path: callers use drnmi_up8_logsoftmax_argmax. */
int drnmi_up8_logsoftmax_argmax_wide(const float* logits, const float* up_w, float* logprobs,
                                     void* labels, int32_t label_dtype, int32_t n, int32_t c,
                                     int32_t h, int32_t w, void* stream);

/* Labels-only form of the same head (the video path: no log-prob planes) on NHWC logits: fp32
 * [n][h][w][cs] rows, classes 0..c-1 first (cs % 4 == 0, cs >= c, 16-B aligned), as the seg conv
 * writes them with y_sp = cs, y_sc = 1.  Same per-pixel arithmetic, near-tie fallback and argmax
 * order as drnmi_up8_logsoftmax_argmax: identical labels.  c == 19 (else DRNMI_ENOTSUP); any other
 * class count: drnmi_up8_labels_nhwc_wide. */
int drnmi_up8_labels_nhwc(const float* logits, int32_t cs, const float* up_w, void* labels, int32_t label_dtype,
                          int32_t n, int32_t c, int32_t h, int32_t w, void* stream);

/* The same labels-only head for any 1 <= c <= 256 (else DRNMI_ENOTSUP), c == 19 included: the
 * runtime-class-count form of the 19-class tiled kernel (csrc/head_wide.hip
 * up8_labels_wide_tile_kernel).  A workgroup stages its tile's 1/8-res logit vectors in LDS once;
 * an 8 x 8 output window whose four taps agree on the best class by more than a guard is written
 * without per-pixel work, the others are decided over the classes that can still win, and a pixel
 * whose top two are closer than 2^-16 takes the three-sweep log-softmax argmax of
 * drnmi_up8_logsoftmax_argmax (the same device function).  Labels are bit-identical to the
 * labels-only drnmi_up8_logsoftmax_argmax on the NCHW form of the same values; the columns
 * c .. cs - 1 of a row are never read into a decision.
 * DRNMI_EINVAL before any HIP call: NULL pointers, a label_dtype other than DRNMI_U8 / DRNMI_I64,
 * cs % 4 != 0, cs < c, non-positive sizes, logits not 16-byte aligned, labels not 4-byte (uint8) or
 * 8-byte (int64) aligned, n or h above 65535, w above 2^27.  No allocation, no host synchronisation. */
int drnmi_up8_labels_nhwc_wide(const float* logits, int32_t cs, const float* up_w, void* labels,
                               int32_t label_dtype, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);

/* drnmi_up8_labels_nhwc_wide with counters, for the tests to prove that each path ran (not a
 * faster path; the shipped kernel is compiled without the counting): the same labels, and
 * stats (device, int64[3], 8-byte aligned, accumulated): [0] += windows written by the fast path
 * (64 pixels each), [1] += pixels decided over the candidate classes, [2] += pixels through the
 * three-sweep fallback. */
int drnmi_up8_labels_nhwc_wide_stats(const float* logits, int32_t cs, const float* up_w, void* labels,
                                     int32_t label_dtype, int32_t n, int32_t c, int32_t h, int32_t w, void* stream,
                                     int64_t* stats);

/* The labels-only video path with the seg classifier (1x1 c_in -> 19 + bias, lmodels/drnseg.py:278-284)
 * folded into the epilogue of the last 3x3 conv (D-22 layer8): `a` is that conv's argument block
 * exactly as for drnmi_conv2d_bn_act (bf16, scale folded, no residual / x2, cout % 256 == 0, a shape
 * the staggered strip tile takes) but its activation is NOT stored (a->y unused); instead each
 * 256-channel block's partial logits go to partials[cout / 256][n*ho*wo][20] (fp32, 16-B aligned):
 * partial_b[m][k] = sum over the block's channels c of seg_w[k][c] * bf16(relu(conv)[m][c]).
 * seg_w: packed bf16 [seg_rows >= 32][seg_k_pad] (rows 19.. zero).  DRNMI_ENOTSUP if the conv does
 * not take the staggered tile.  It runs on the one-wave-per-SIMD tile (conv_w1_seg_kernel /
 * conv_w1_i8_seg_kernel); a->tile == 19 forces the staggered one (the same partials, bit for bit).
 * int8 nets (a->dtype DRNMI_I8, out_dtype DRNMI_I8, the W8A8 epilogue of drnmi_conv2d_bn_act, no
 * residual): seg_w is the int8 seg conv's packed weights and the partials are int32,
 * partial_b[m][k] = sum over the block's channels c of seg_w[k][c] * q8[m][c], q8 = the int8 value
 * the conv would store; the int8 seg conv's fp32 output is then (float)(partial_0 + partial_1) *
 * seg_scale[k] + seg_shift[k] (drnmi_up8_labels_seg2_i8). */
int drnmi_conv_stag_seg(const drnmi_conv_args* a, const void* seg_w, int32_t seg_k_pad, int32_t seg_rows,
                        void* partials, void* stream);
/* The kernel drnmi_conv_stag_seg launches for these arguments (as rocprofv3 names it), or NULL
 * where its checks of the conv arguments refuse them. */
const char* drnmi_conv_stag_seg_kernel_name(const drnmi_conv_args* a);

/* Labels from those partials: logit[k] = (bias[k] + partial_0[k]) + partial_1[k] (bias: >= cs
 * floats), then the labels-only head's arithmetic (drnmi_up8_labels_nhwc).  partials: [2][n][h][w][cs]. */
int drnmi_up8_labels_seg2(const float* partials, int32_t cs, const float* bias, const float* up_w, void* labels,
                          int32_t label_dtype, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);

/* int8 nets: logit[k] = (float)(partial_0[k] + partial_1[k]) * scale[k] + shift[k] (fmul then fadd,
 * the int8 seg conv's epilogue: identical logits), then the same head.  partials: int32
 * [2][n][h][w][cs]; scale, shift: >= cs floats. */
int drnmi_up8_labels_seg2_i8(const int32_t* partials, int32_t cs, const float* scale, const float* shift,
                             const float* up_w, void* labels, int32_t label_dtype, int32_t n, int32_t c, int32_t h,
                             int32_t w, void* stream);

/* Same head for DRNSeg(use_torch_up=True): nn.UpsamplingBilinear2d(scale_factor=8) (bilinear,
 * align_corners=True; lmodels/drnseg.py:285-287) + LogSoftmax + argmax.  Source index and
 * weights follow ATen's CPU kernel: scale = (in-1)/(out-1) in fp32, i0 = floor(scale*dst),
 * i1 = i0 + (i0 < in-1), l1 = scale*dst - i0.  Output [n][c][8h][8w].  1 <= c <= 256, else
 * DRNMI_ENOTSUP; 33 <= c <= 256 recomputes the interpolation in three sweeps over the classes. */
int drnmi_up8_bilinear_logsoftmax_argmax(const float* logits, float* logprobs, void* labels,
                                         int32_t label_dtype, int32_t n, int32_t c, int32_t h, int32_t w,
                                         void* stream);

/* Bilinear resize with Pillow's arithmetic (Image.resize(size, BILINEAR): separable, horizontal
 * pass first, the filter support widened by the downscale factor; coefficient tables computed on
 * the device exactly as Pillow's precompute_coeffs).  Bit-identical to Pillow 12.
 *   drnmi_resize_bilinear_u8: uint8 HWC3 frames [n][h][w][3] -> [n][oh][ow][3]; 8-bit fixed point
 *     with 22 fractional bits and a uint8 intermediate (Pillow's 8bpc path).  Replaces
 *     T.Resize((300, 300)) on each decoded frame (seg_video_old_no_plot.py:126-127).
 *   drnmi_resize_bilinear_f32: fp32 planes [planes][h][w] -> [planes][oh][ow]; fp32 x double
 *     summed in double, fp32 intermediate (Pillow's 'F' mode).  accumulate != 0: dst += result in
 *     fp32.  Replaces resize_4d_tensor + the scale sum of test_ms (semantic_seg.py:471-504, :540).
 *   ws: device workspace of drnmi_resize_workspace_bytes(n or planes, h, w, oh, ow, 3 or 4) bytes.
 *   drnmi_argmax_nchw_f32: labels[n][p] = first index of the max over c of x[n][c][p] (numpy
 *     argmax(axis=1), semantic_seg.py:543), uint8 or int64 labels. */
int64_t drnmi_resize_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t elem_bytes);
int drnmi_resize_bilinear_u8(const uint8_t* src, int32_t n, int32_t h, int32_t w, uint8_t* dst, int32_t oh, int32_t ow,
                             void* ws, int64_t ws_bytes, void* stream);
int drnmi_resize_bilinear_f32(const float* src, int32_t planes, int32_t h, int32_t w, float* dst, int32_t oh,
                              int32_t ow, int32_t accumulate, void* ws, int64_t ws_bytes, void* stream);
int drnmi_argmax_nchw_f32(const float* x, int32_t n, int32_t c, int64_t hw, void* labels, int32_t label_dtype,
                          void* stream);

/* Label maps to pictures (csrc/render.hip): the palette colouring that ends every reference driver
 * (CITYSCAPE_PALETTE[pred], seg_video_old_no_plot.py:166-170; save_colorful_images,
 * semantic_seg.py:415-426) and the overlay of that colour image on the input frame (the
 * seg_video*.py variants, alpha = 0.6).  One streaming kernel on the caller's stream, no
 * allocation (graph-capturable); it serves every precision and head path.
 *   labels: [n][lh][lw] uint8 or int64 (label_dtype, the codes of drnmi_up8_labels_nhwc);
 *   palette: device uint8 [P][3] RGB, 1 <= P <= 256; out: uint8 [n][oh][ow][3], oh <= lh, ow <= lw;
 *   frames: uint8 [n][oh][ow][3], or NULL for the colour image alone (out == frames is allowed).
 * Exact integer arithmetic:
 *   crop    output pixel (y, x) takes label (y, x): the top-left oh x ow of the label map.  The
 *           ConvTranspose2d head (k16, s8, p4) keeps output pixel (y, x) over input pixel (y, x);
 *           the extra rows / columns of a 300 -> 304 map come from the stride ceil chain and have
 *           no source pixel.
 *   colour  c = palette[min(label, P - 1)]: labels at or above P (the ignore value 255 too) and
 *           negative int64 labels take the last entry -- entry 19 of the 20-entry Cityscapes
 *           palette is black, the reference's `color_image[output == 255] = CITYSCAPE_PALETTE[-1]`.
 *           swap_rb != 0 writes the entry as B, G, R (BGR frames going back to a cv2 writer).
 *   overlay per channel out = (f * (256 - a) + c * a + 128) >> 8 with a = alpha_q8 in 0..256:
 *           a = 0 returns the frame, a = 256 the colour, both exactly.  alpha_q8 is ignored when
 *           frames == NULL.  (matplotlib's float compositing is not reproduced; this is the contract.)
 * DRNMI_EINVAL before any HIP call: NULL labels / palette / out, another dtype, P outside 1..256,
 * a non-positive size, oh > lh, ow > lw, alpha_q8 outside 0..256 (with frames), or n * lh * lw above
 * 2^40 elements (the kernel indexes in 64 bits; the bound keeps every byte offset inside them). */
int drnmi_render_labels(const void* labels, int32_t label_dtype, int32_t n, int32_t lh, int32_t lw,
                        const uint8_t* frames, const uint8_t* palette, int32_t P, int32_t alpha_q8, int32_t swap_rb,
                        uint8_t* out, int32_t oh, int32_t ow, void* stream);

/* Multi-tensor in-place mask apply: w[t][i] *= m[t][i] for every tensor t.
 * Replaces Pruner.apply_masks (pruners/Pruner.py:17-20, same body BlockPruner.py:27-30,
 * SRMBRepMasker.py:20-23): one launch for all masked layers instead of one ATen mul_ per
 * layer plus a state_dict() rebuild per layer. */
int drnmi_mask_apply_f32(int32_t ntensors, float* const* weights, const float* const* masks,
                         const int64_t* numels, void* stream);

/* Same, with bit-packed masks: bit i of word i/32 of masks[t] keeps element i. */
int drnmi_mask_apply_bits_f32(int32_t ntensors, float* const* weights,
                              const uint32_t* const* mask_bits, const int64_t* numels,
                              void* stream);

/* Eval: accumulate the nclass x nclass confusion matrix hist[label*nclass + pred] += 1 over the
 * pixels with 0 <= label < nclass and pred < nclass (int64 hist, NOT cleared: accumulates across
 * calls like the reference's running hist).  Replaces fast_hist (semantic_seg.py:293-296) used by
 * test()/val_miou() (:455, :655).  pred/label dtypes: DRNMI_U8 or DRNMI_I64; nclass <= 256
 * (nclass <= 32: a 4 KiB LDS table; above: up to 128 KiB of LDS per workgroup, the label rows in
 * two slabs from nclass = 182; npix <= 2^40 there). */
int drnmi_confusion_matrix(const void* pred, int32_t pred_dtype, const void* label, int32_t label_dtype,
                           int64_t npix, int32_t nclass, int64_t* hist, void* stream);

/* ======================================================================================
 * Fine-tune (train-mode) path, fp32 — csrc/train.hip.
 * Replaces the reference training step (semantic_seg.py:166-230): model.train() forward
 * with batch-statistics BatchNorm (lmodels/drn.py:7), CrossEntropyLoss(ignore_index=255) on
 * the log-probs (semantic_seg.py:817, :197-198), loss.backward(), torch.optim.SGD(momentum,
 * weight_decay) (:963-966, :212) and Pruner.apply_masks (:213-214, pruners/Pruner.py:17-20).
 * Conv forward and data-gradient passes go through drnmi_conv2d_bn_act (fp32): dgrad is a
 * stride-1 conv of dy with weights packed by drnmi_pack_conv_weight(mode = 1), after
 * drnmi_zero_insert_f32 for stride-s convs.  All reductions are fp64, fixed order
 * (bit-reproducible).  Workspaces are caller-provided device buffers of the queried size.
 * ====================================================================================== */

/* OIHW fp32 weights -> packed [rows_pad][k_pad] (out_dtype F32 or BF16), zero elsewhere.
 * mode 0 (forward):  row = co, k = (kh*ks + kw)*kin_stride + ci, value w[co][ci][kh][kw] *
 *                    row_scale[co] (row_scale may be NULL = 1; folds an eval BN scale).
 * mode 1 (dgrad):    row = ci, k = (kh*ks + kw)*kin_stride + co, value
 *                    w[co][ci][ks-1-kh][ks-1-kw] (transposed, spatially flipped).
 * Replaces the host-side permute/pad of the conv weights (lmodels/drn.py:27-29 layout). */
int drnmi_pack_conv_weight(const float* w, int32_t cout, int32_t cin, int32_t ks, int32_t kin_stride,
                           int32_t rows_pad, int32_t k_pad, int32_t mode, const float* row_scale,
                           int32_t out_dtype, void* out, void* stream);

/* Batched form of drnmi_pack_conv_weight (F32 output) + drnmi_split3_bf16 for a whole network:
 * one launch packs every entry of a device-resident table (the fine-tune re-packs all forward
 * and data-gradient weights after each SGD step; per layer that was 4 launches of ~6 us).
 * table: DEVICE memory, n entries of DRNMI_PACK_ENTRY_WORDS int64 each:
 *   [0] w (const float*), [1] out (float* [rows_pad][k_pad]), [2] planes (bf16 [3][rows_pad*k_pad]
 *   or 0), [3] cout, [4] cin, [5] ks, [6] kin_stride, [7] rows_pad, [8] k_pad, [9] mode (0 | 1,
 *   as drnmi_pack_conv_weight, no row scale), [10] first element index of the entry (prefix sum
 *   of rows_pad*k_pad over the entries before it), [11] 0.
 * total = sum of rows_pad*k_pad.  Values are bit-identical to the per-layer calls.
 * Limits: n <= 512, ks <= 7, kin_stride and k_pad multiples of 4, out / planes 16-B aligned.
 * drnmi_pack_table_check validates a HOST copy of the table before it is uploaded. */
#define DRNMI_PACK_ENTRY_WORDS 12
int drnmi_pack_table_check(const int64_t* table_host, int32_t n, int64_t* total_out);
int drnmi_pack_conv_weights_batched(const int64_t* table, int32_t n, int64_t total, void* stream);

/* Workspace bytes for the per-channel reductions over `rows` x `channels` (power of two >= 4). */
int64_t drnmi_reduce_workspace_bytes(int64_t rows, int32_t channels);

/* Train-mode BatchNorm2d statistics over rows of NHWC y [rows][C]: mean, invstd =
 * 1/sqrt(biased_var + eps); if running_mean/var are given: r = (1-momentum)*r + momentum*batch
 * (running_var with the unbiased variance), and *num_batches_tracked += 1 (if non-NULL). */
int drnmi_bn_stats_f32(const float* y, int64_t rows, int32_t C, float eps, float momentum,
                       float* mean, float* invstd, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked, void* ws, void* stream);

/* Weight planes of parity class (a, b) of a stride-2 conv's data gradient (the transpose of
 * lmodels/drn.py's strided conv3x3 / downsample 1x1 in the fine-tune backward): gathered from the
 * dgrad's packed bf16 planes `planes` ([3][rows][k_pad], drnmi_pack_conv_weight mode 1 + split3,
 * k = tap' * kst + co, taps flipped, pad_d = dil*(ks-1) - pad) into `out` [3][rows][k_pad_c] for a
 * ksc x ksc stride-1 conv of dy: tap (khc, kwc) = flipped tap ((pad_d - a) mod 2 + 2 khc, likewise
 * for b), zero where the class has fewer taps.  Launch the class conv with F32X3, x = dy, pad 0,
 * y = dx + (a * W + b) * cs, y_sp = 2 cs, y_sr = 2 W cs, y_sn = H W cs: the four classes together
 * are bit-identical to the conv of the zero-inserted dy (drnmi_zero_insert_f32).  kst % 8 == 0. */
int drnmi_dgrad_s2_class_planes(const void* planes, int32_t rows, int32_t k_pad, int32_t kst, int32_t ks,
                                int32_t pad_d, int32_t a, int32_t b, int32_t ksc, void* out, int32_t k_pad_c,
                                void* stream);

/* drnmi_bn_stats_f32 from the partial sums a conv epilogue wrote (drnmi_conv_args.stats:
 * [2][G][C] fp64, G = drnmi_conv_stats_rows): the same finalize (mean, biased variance, invstd,
 * running-stat update) over `rows` pixels. */
int drnmi_bn_stats_partials_f32(const double* partials, int64_t G, int64_t rows, int32_t C, float eps,
                                float momentum, float* mean, float* invstd, float* running_mean,
                                float* running_var, int64_t* num_batches_tracked, void* stream);

/* z = relu?(((y - mean) * invstd) * gamma + beta [+ res]) over [rows][C]; gamma/beta/res NULL-able.
 * (BasicBlock / Bottleneck tail: lmodels/drn.py:49-65, :86-106.)  mean/invstd/gamma/beta must be
 * 16-byte aligned (DRNMI_EINVAL otherwise). */
int drnmi_bn_act_f32(const float* y, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, const float* res, int32_t relu, int64_t rows, int32_t C,
                     float* z, void* stream);

/* Backward of drnmi_bn_act_f32 (train-mode BN): dr = dz * (relu ? z > 0 : 1);
 * dbeta = sum dr, dgamma = sum dr * xhat; dy = gamma*invstd*(dr - mean(dr) - xhat*mean(dr*xhat));
 * dres (NULL-able) = dr (or += dr with dres_accumulate).  dy may alias dz.
 * grad_accumulate: dgamma/dbeta += instead of =.  mean must be 16-byte aligned. */
int drnmi_bn_act_bwd_f32(const float* dz, const float* z, const float* y, const float* mean,
                         const float* invstd, const float* gamma, int32_t relu, int64_t rows,
                         int32_t C, float* dy, float* dres, int32_t dres_accumulate, float* dgamma,
                         float* dbeta, int32_t grad_accumulate, void* ws, void* stream);

/* drnmi_bn_act_bwd_f32 for a residual-free BN + ReLU (relu = 1, res = NULL, dres = NULL) without z:
 * the mask z > 0 is recomputed from y with the forward's own arithmetic (bn_act's rounding order),
 * so it is bit-identical to reading z and each pass reads one fp32 tensor less.  gamma / beta as
 * given to drnmi_bn_act_f32 (NULL-able); mean/invstd/gamma/beta 16-byte aligned.
 * (semantic_seg.py:166-230 backward through lmodels/drn.py:49-65 / :86-106's bn + relu.) */
int drnmi_bn_relu_bwd_y_f32(const float* dz, const float* y, const float* mean, const float* invstd,
                            const float* gamma, const float* beta, int64_t rows, int32_t C, float* dy,
                            float* dgamma, float* dbeta, int32_t grad_accumulate, void* ws, void* stream);

/* out[c] (+)= sum over rows of x[row][c], c < cvalid (row stride C).  Conv-bias gradient
 * (seg 1x1 + bias, lmodels/drnseg.py:278-284). */
int drnmi_channel_sum_f32(const float* x, int64_t rows, int32_t C, int32_t cvalid, float* out,
                          int32_t accumulate, void* ws, void* stream);

/* Weight gradient of a conv: dw[co][ci][kh][kw] (+)= sum_pixels dy[pix][co] * x[tap(pix)][ci].
 * dy: NHWC [n*ho*wo][dy_stride] (first cout valid), x: NHWC [n][h][w][cin_stride]. */
typedef struct drnmi_wgrad_args {
  const float* dy;
  const float* x;
  float* dw;             /* OIHW [cout][cin][ks][ks] fp32 (the parameter's .grad)          */
  void* ws;              /* workspace, ws_bytes >= drnmi_conv_wgrad_workspace_bytes()      */
  int64_t ws_bytes;
  int32_t n, h, w, cin, cin_stride, ho, wo, cout, dy_stride;
  int32_t ks, stride, pad, dil;
  int32_t accumulate;    /* 1: dw += ; 0: dw =                                            */
} drnmi_wgrad_args;
int64_t drnmi_conv_wgrad_workspace_bytes(const drnmi_wgrad_args* args);    /* room for either kernel */
int64_t drnmi_conv_wgrad_f32_workspace_bytes(const drnmi_wgrad_args* args);/* drnmi_conv_wgrad_f32 only */
int drnmi_conv_wgrad_f32(const drnmi_wgrad_args* args, void* stream);
/* The same weight gradient in fp32-class split-bf16 arithmetic (the fp32x fine-tune: exact 3-way
 * bf16 split of dy and x, the six products above 2^-24 on the bf16 MFMA, fp32 accumulation);
 * same arguments, workspace and errors.  semantic_seg.py:166-230 backward. */
int drnmi_conv_wgrad_f32x3(const drnmi_wgrad_args* args, void* stream);
/* Host-only: the launch drnmi_conv_wgrad_f32 (x6 = 0) or drnmi_conv_wgrad_f32x3 (x6 = 1) makes for
 * these arguments, from the launcher's own decision (no pointer is read, nothing runs).  kernel:
 * DRNMI_WGRAD_*; splits: the pixel splits whose partials the reduce sums (wave splits for the direct
 * kernel); pix_per_split: pixels per split, a multiple of 32 (the last split is ragged when
 * n*ho*wo % pix_per_split != 0; unused by the direct kernel); reduce: 0 = one thread per output,
 * 1 = the grouped reduce (>= 32 splits).  Out pointers may be NULL.  DRNMI_EINVAL on bad geometry. */
#define DRNMI_WGRAD_F32 0     /* wgrad_kernel<64, false>: exact-f32 MFMA, 64 x 64 tile        */
#define DRNMI_WGRAD_X6 1      /* wgrad_kernel<64, true>: split-bf16, 64 x 64 tile             */
#define DRNMI_WGRAD_BIG 2     /* wgrad_kernel<128, true>: split-bf16, 128 x 128 tile          */
#define DRNMI_WGRAD_PRE 3     /* wgrad_dy_split_kernel + wgrad_x6_pre_kernel (K >= 1024)      */
#define DRNMI_WGRAD_DIRECT 4  /* wgrad_x6_direct_kernel: cout <= 32, wo % 32 == 0             */
int drnmi_conv_wgrad_plan(const drnmi_wgrad_args* args, int32_t x6, int32_t* kernel, int32_t* splits,
                          int64_t* pix_per_split, int32_t* reduce);
/* fp32 w[n] -> bf16 out[3][n] with w = out[0] + out[1] + out[2] exactly (round to nearest even at
 * each step): the three weight planes of a DRNMI_F32X3 launch. */
int drnmi_split3_bf16(const float* w, int64_t n, void* out, void* stream);

/* Quantisation-aware fine-tuning (csrc/qat.hip): the int8 engine's grids as fp32
 * values in the train step, straight-through in the backward.  One fp32 rounding per step, no FMA.
 * All four run on the caller's stream and allocate nothing; NULL or misaligned pointers (16 bytes;
 * 4 for row_scale), n % 8 != 0 or a scale that is not a positive finite number: DRNMI_EINVAL before any
 * HIP call; n == 0 / rows == 0: DRNMI_OK, nothing launched.
 *   drnmi_fake_quant_f32: y[i] = float(clamp(rint(x[i] * inv_scale), -127, 127)) * scale -- the code
 *     drnmi_quantize_i8 gives, dequantised; inv_scale is the caller's fp32 rounding of 1 / scale (the
 *     one the int8 plan passes).  A zero level is +0.
 *   drnmi_fake_quant_bwd_f32: the straight-through gradient of that, g = dq[i] where
 *     |rint(x[i] * inv_scale)| <= 127 (the level was not clamped; recomputed from x, no stored mask),
 *     else 0; dx[i] = g, or dx[i] + g (one rounding) with accumulate = 1.
 *   drnmi_fake_quant_rows_f32: per row of w [rows][cols] (an OIHW conv weight: one output channel),
 *     a = max |w|, q = clamp(rint(w * (127 / a)), -127, 127), wq = float(q) * (a / 127),
 *     row_scale = a / 127; an all-zero row gives zeros and scale 1.  q is the int8 code the int8 pack
 *     (drnmi/engine.py _pack_q8) stores for that weight.  cols: any positive count.
 *   drnmi_fake_quant_rows_batched_f32: the same for every entry of a DEVICE table in one launch (one
 *     workgroup per row), n <= 512 entries of DRNMI_FQ_ROWS_ENTRY_WORDS int64 each:
 *     [0] w, [1] wq, [2] row_scale, [3] rows, [4] cols, [5] first row of the entry (prefix sum of rows).
 *     total_rows = sum of rows.  drnmi_fake_quant_rows_table_check validates a HOST copy first. */
#define DRNMI_FQ_ROWS_ENTRY_WORDS 6
int drnmi_fake_quant_f32(const float* x, int64_t n, float scale, float inv_scale, float* y, void* stream);
int drnmi_fake_quant_bwd_f32(const float* dq, const float* x, int64_t n, float inv_scale, float* dx,
                             int32_t accumulate, void* stream);
int drnmi_fake_quant_rows_f32(const float* w, int64_t rows, int32_t cols, float* wq, float* row_scale,
                              void* stream);
int drnmi_fake_quant_rows_table_check(const int64_t* table_host, int32_t n, int64_t* total_rows_out);
int drnmi_fake_quant_rows_batched_f32(const int64_t* table, int32_t n, int64_t total_rows, void* stream);

/* out[n][y][x][c] = dy[n][y/s][x/s][c] where y, x are multiples of s (and inside dy), else 0;
 * out is [n][hu][wu][c] (c % 4 == 0).  Input of the stride-1 dgrad conv of a stride-s conv. */
int drnmi_zero_insert_f32(const float* dy, int32_t n, int32_t ho, int32_t wo, int32_t c, int32_t stride,
                          int32_t hu, int32_t wu, float* out, void* stream);

/* Head backward: du = grad_scale * (g_lp - exp(lp) * sum_c g_lp) (LogSoftmax, dim 1), then
 * dlogits = up^T(du) [+ grad_scale * g_logits] — the transpose of the fixed bilinear ConvTranspose2d(k16,
 * s8, p4) (lmodels/drnseg.py:285-299).  g_logprobs/logprobs/du_ws: NCHW [n][c][8h][8w];
 * dlogits/g_logits: [n][c][h][w]; g_logprobs NULL = logits-only gradient. */
int drnmi_up8_lsm_bwd_f32(const float* g_logprobs, const float* logprobs, const float* g_logits,
                          const float* up_w, float grad_scale, int32_t n, int32_t c, int32_t h,
                          int32_t w, float* du_ws, float* dlogits, void* stream);

/* Head backward of the use_torch_up head (bilinear align_corners=True x8): du as above, then
 * dlogits = bilinear^T(du) [+ grad_scale * g_logits] (a fixed-order gather, no atomics). */
int drnmi_up8_bilinear_lsm_bwd_f32(const float* g_logprobs, const float* logprobs, const float* g_logits,
                                   float grad_scale, int32_t n, int32_t c, int32_t h, int32_t w, float* du_ws,
                                   float* dlogits, void* stream);

/* CrossEntropyLoss(ignore_index) applied to log-probs [n][c][hw] with int64 targets [n][hw]:
 * loss[0] = mean over target != ignore of (logsumexp(lp) - lp[target]) (NaN if a target is out
 * of range), count[0] = number of counted pixels.  Device scalars; ws of drnmi_ce_workspace_bytes. */
int64_t drnmi_ce_workspace_bytes(void);
int drnmi_ce_loss_f32(const float* logprobs, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                      int64_t ignore_index, float* loss, float* count, void* ws, void* stream);
/* g_logprobs = dloss[0] / count[0] * (softmax(lp) - onehot(target)), 0 on ignored pixels. */
int drnmi_ce_loss_bwd_f32(const float* logprobs, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                          int64_t ignore_index, const float* dloss, const float* count,
                          float* g_logprobs, void* stream);

/* Distillation loss (added under ABI version 7: new functions only): the CrossEntropyLoss above on
 * the student's log-probs plus the KL divergence to a teacher's log-probs at a temperature, in one
 * pass over both [n][c][hw] fp32 tensors.  Per pixel, in fp32, with a = s / T and b = t / T:
 *   logp = a - lse(a), logq = b - lse(b), q = exp(logq), kd_i = sum_k q[k] * (logq[k] - logp[k])
 * over EVERY pixel (labelled or not), and ce_i = lse(s) - s[target] over target != ignore_index.
 *   CE = sum ce_i / count;  KD = sum kd_i / D, D = n * hw, or n with batchmean != 0 (F.kl_div's
 *   size_average=False / shape[0]);  loss = student_wt * CE + distill_wt * KD.  No T^2 factor.
 * out3 = {loss, CE, KD}, count[0] = number of labelled pixels: device scalars.  An out-of-range
 * target other than ignore_index makes loss and CE NaN.  Bit-equal s and t give KD == 0 exactly.
 * fp64 block partials in a fixed order: bit-reproducible.  ws of drnmi_distill_workspace_bytes.
 * Asynchronous on the stream, no allocation, no synchronisation.  DRNMI_EINVAL before any HIP call:
 * a NULL pointer, a non-positive size, a temperature not finite and > 0, a weight negative or not
 * finite. */
int64_t drnmi_distill_workspace_bytes(void);
int drnmi_distill_loss_f32(const float* student_lp, const float* teacher_lp, const int64_t* target,
                           int32_t n, int32_t c, int64_t hw, int64_t ignore_index, float student_wt,
                           float distill_wt, float temperature, int32_t batchmean, float* out3,
                           float* count, void* ws, void* stream);
/* g_student_lp = dloss[0] * (student_wt / count[0] * (softmax(s) - onehot(target)) on labelled pixels
 *                            + distill_wt / (D * T) * (exp(logp) - q)); the teacher gets no gradient. */
int drnmi_distill_loss_bwd_f32(const float* student_lp, const float* teacher_lp, const int64_t* target,
                               int32_t n, int32_t c, int64_t hw, int64_t ignore_index, float student_wt,
                               float distill_wt, float temperature, int32_t batchmean, const float* dloss,
                               const float* count, float* g_student_lp, void* stream);

/* Multi-tensor torch.optim.SGD step (semantic_seg.py:963-966, torch semantics: d = g + wd*w;
 * buf = first ? d : momentum*buf + (1-dampening)*d; d = nesterov ? d + momentum*buf : buf;
 * w -= lr*d) with the pruner mask fused: w *= bit (mask_bits[t] NULL-able; NULL array = none).
 * params/grads/momentum_bufs/numels/mask_bits/first_step are HOST arrays of device pointers. */
int drnmi_sgd_step_f32(int32_t ntensors, float* const* params, const float* const* grads,
                       float* const* momentum_bufs, const int64_t* numels,
                       const uint32_t* const* mask_bits, const int32_t* first_step, float lr,
                       float momentum, float dampening, float weight_decay, int32_t nesterov,
                       void* stream);

/* Fine-tune data path (csrc/ingest.hip): the batch of the train() / validate() loop made on the
 * GPU from uint8 images and labels.  Replaces the per-sample PIL / numpy pipeline of
 * semantic_seg.py:885-889 and :918-921: RandomCrop with reflection padding
 * (data_transforms.py:9-45, :128-155), RandomHorizontalFlip (:96-106), ToTensor (:228-253) and
 * Normalize (:109-125).  The random draws and the padding geometry stay on the host
 * (drnmi/data.py); they reach the kernel as two index tables per sample.
 *   images  device uint8 [n][h][w][3];  labels  device uint8 [n][h][w], or NULL with target == NULL;
 *   rowmap  device int32 [n][th], colmap device int32 [n][tw].  An entry e >= 0 is a source row /
 *           column inside the image.  An entry e < 0 marks a padded position: its image source
 *           index is ~e (the reflection) and its label is 255 (the 'constant' pad, :31-32).
 *   mean3 / std3  HOST pointers to 3 floats, as in drnmi_frame_ingest_u8;
 *   out     fp32 NCHW [n][3][th][tw], 16-byte aligned:
 *             out[i][c][y][x] = (float(images[i][r][q][c]) / 255.0f - mean[c]) / std[c]
 *           with r / q the decoded entries of rowmap[i][y] / colmap[i][x]: division, subtraction,
 *           division in fp32, nothing contracted -- the sequence of drnmi_frame_ingest_u8, bit-identical
 *           to img.float().div(255) followed by sub_(m).div_(s);
 *   target  int64 [n][th][tw], 8-byte aligned: 255 where rowmap or colmap is negative, else
 *           labels[i][r][q] (ToTensor's LongTensor, :253).
 * The kernel clamps every decoded index into [0, h-1] / [0, w-1] before it reads: no table content
 * makes it read outside the images.  64-bit indexing, no allocation, no host synchronisation
 * (graph-capturable).  DRNMI_EINVAL before any HIP call: NULL images / rowmap / colmap / out / mean3 /
 * std3, labels and target not both NULL or both set, a non-positive size, out not 16-byte or target
 * not 8-byte aligned, n * h * w or n * th * tw above 2^40. */
int drnmi_train_ingest_u8(const uint8_t* images, const uint8_t* labels, int32_t n, int32_t h, int32_t w,
                          const int32_t* rowmap, const int32_t* colmap, int32_t th, int32_t tw,
                          const float* mean3, const float* std3, float* out, int64_t* target, void* stream);

/* Pixel accuracy, eval_score=accuracy (utils.py:267-277; semantic_seg.py:1072, :1004), in one pass
 * over log-probs [n][c][hw] and int64 targets [n][hw].  counts is device int64[2], accumulated and
 * NOT cleared (like drnmi_confusion_matrix): counts[0] += pixels with target != ignore_index,
 * counts[1] += those whose argmax over c equals the target (a tie takes the lowest index, as in
 * drnmi_argmax_nchw_f32).  A target outside 0..c-1 other than ignore_index counts and is never
 * correct.  DRNMI_EINVAL: NULL pointers, non-positive sizes, n * hw above 2^40 or c above 2^20. */
int drnmi_pixel_accuracy_f32(const float* logprobs, const int64_t* target, int32_t n, int32_t c, int64_t hw,
                             int64_t ignore_index, int64_t* counts, void* stream);

/* Library version string, e.g. "drnmi 0.1.0 gfx950". */
const char* drnmi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DRNMI_H */
