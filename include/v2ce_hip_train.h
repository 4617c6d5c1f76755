/* v2ce_hip_train.h -- the trainable layers of libv2ce_hip.so: forward and backward of the prediction head UNet.pred.
 *
 * The conventions of v2ce_hip.h hold: device pointers unless stated, entries enqueue on `stream` and do not synchronise,
 * they return V2CE_OK or a negative error code, v2ce_last_error() describes the last failure.  The loss gradients stay
 * in v2ce_hip_grad.h; what turns a gradient with respect to an activation into gradients with respect to parameters
 * (and to the layer's input) lives here. */
#ifndef V2CE_HIP_TRAIN_H
#define V2CE_HIP_TRAIN_H

#include "v2ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The prediction head (csrc/pred_head.hip): ConvLayer3D(32, Cout, 1, activation='relu', norm=None), a 1x1x1 convolution
 * with bias followed by relu, and its backward.
 *   feat, d_feat  V2CE_LAYOUT_C16 with two channel groups: [B][L][2][H][pitch][16] f32, what the last decoder block
 *                 produces; pitch >= W; the columns W .. pitch-1 of a row are never read and never written; 16-byte
 *                 aligned, B * L * 2 * H * pitch * 64 bytes
 *   y, upstream   [B][L][Cout][H][W] f32, dense and contiguous (the output of V2ce3d and the gradient of
 *                 v2ce_voxloss_grads), 4-byte aligned, B * L * Cout * H * W * 4 bytes
 *   weight        [Cout][32] f32, the [Cout, 32, 1, 1, 1] parameter as stored;  bias [Cout];  d_weight, d_bias alike
 *   workspace     >= the *_workspace_bytes value, 8-byte aligned; scratch, nothing is read before it is written
 * 1 <= Cout <= 32 (the limit of the fused inference head), B, L, H, W >= 1, B * L * H * W < 2^31 and
 * B * L * H * pitch < 2^34, else V2CE_ERR_BAD_ARG, as for NULL pointers and a misaligned feat, d_feat or workspace; the
 * *_workspace_bytes queries return 0 for arguments the entry refuses.  A small workspace is V2CE_ERR_WORKSPACE and
 * nothing is written.  Outputs must not overlap inputs or each other.
 *
 * v2ce_pred_head_fwd:  y = max((float)(bias + sum_ci feat[ci] weight[co][ci]), 0), the sum in f64 from the f32 inputs in
 * the order ci = 0 .. 31 starting from the bias, one rounding at the store; a NaN stays a NaN (torch.relu).  Every
 * element of y is written.
 *
 * v2ce_pred_head_grads:  with m = upstream where y > 0, else 0 (torch's relu backward on the result: a NaN in y gives 0,
 * a NaN in upstream propagates),
 *     d_weight[co][ci] = sum_pos m[co] feat[ci]      d_bias[co] = sum_pos m[co]      d_feat[pos][ci] = sum_co m[co] weight[co][ci]
 * y is the forward's output.  d_weight, d_bias and d_feat may each be NULL (its work is skipped), not all three.  Every
 * product and sum is f64 from the f32 inputs; the one rounding to f32 is the store.  No atomics: a workgroup sums a fixed
 * share of the positions into f64 partials in the workspace and a finish kernel adds the partials in a fixed order, so
 * the bytes are identical from run to run, and an output does not depend on which other outputs were asked for. */
size_t v2ce_pred_head_fwd_workspace_bytes(int B, int L, int Cout, int H, int W, int pitch);
int v2ce_pred_head_fwd(const float *feat, const float *weight, const float *bias, int B, int L, int Cout, int H, int W,
                       int pitch, float *y, void *workspace, size_t workspace_bytes, v2ce_stream_t stream);
size_t v2ce_pred_head_grads_workspace_bytes(int B, int L, int Cout, int H, int W, int pitch);
int v2ce_pred_head_grads(const float *feat, const float *y, const float *upstream, const float *weight, int B, int L,
                         int Cout, int H, int W, int pitch, float *d_weight, float *d_bias, float *d_feat,
                         void *workspace, size_t workspace_bytes, v2ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2CE_HIP_TRAIN_H */
