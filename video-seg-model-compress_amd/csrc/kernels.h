// Internal (non-ABI) launchers shared between the kernel translation units.
#pragma once
#include "common.h"
#include "conv_route.h"

namespace drnmi {
// Fused uint8 stem + the 3x3 16->16 conv after it (patch_conv.hip).
bool stem_l1_ok(const drnmi_conv_args& p, const drnmi_conv_args& q);
int stem_l1_dispatch(const drnmi_conv_args& p, const drnmi_conv_args& q, hipStream_t s);
int weight_unit_mask(const void* wgt, int dtype, int rows_pad, int k_pad, uint32_t* mask, int* count, hipStream_t s);
// The heads and the confusion matrix for up to 256 classes (head_wide.hip); the entry points in
// ops.hip route c > 32 / nclass > 32 here after their own argument checks (up8_wide_dispatch, also
// behind drnmi_up8_logsoftmax_argmax_wide, repeats them); they return drnmi_status / hipError_t.
int up8_wide_dispatch(const float* logits, const float* up_w, float* logprobs, void* labels, int label_dtype, int n,
                      int c, int h, int w, hipStream_t s);
int up8_bilinear_wide_dispatch(const float* logits, float* logprobs, void* labels, int label_dtype, int n, int c, int h,
                               int w, hipStream_t s);
int confusion_wide_dispatch(const void* pred, int pred_dtype, const void* label, int label_dtype, int64_t npix,
                            int nclass, int64_t* hist, hipStream_t s);
}  // namespace drnmi
