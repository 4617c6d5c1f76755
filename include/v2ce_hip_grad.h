/* v2ce_hip_grad.h -- the training-side entries of libv2ce_hip.so: gradients of the stage-1 voxel losses.
 *
 * The conventions of v2ce_hip.h hold: device pointers unless stated, entries enqueue on `stream` and do not synchronise,
 * they return V2CE_OK or a negative error code, v2ce_last_error() describes the last failure.  Inference-side entries
 * stay in v2ce_hip.h; what only a training step needs lives here. */
#ifndef V2CE_HIP_GRAD_H
#define V2CE_HIP_GRAD_H

#include "v2ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Gradient with respect to pred of the voxel-only terms of ModelInterface.calculate_loss (csrc/voxlossgrads.hip), the
 * backward of what v2ce_voxlosses / v2ce_volume_losses measure.  The loss is a weighted sum of terms that are each a mean
 * of squares of linear window sums (or |.| sums) of pred - gt, a softmax NLL, or a norm; its gradient per element is
 *     a_sq (p - g)
 *   + sum_q a_pyr[q] e_k     e_k = pool_k(p) - pool_k(g) of the element's window, k = 2, 4, 8 (AvgPool3d(k, stride k) of one
 *                            volume); 0 for an element outside the floored extent (D/k k, H/k k, W/k k)
 *   + a_t3 e3 + a_t5 e5      e3: AvgPool1d(3, stride 3, padding 1) along D, window j = (d + 1) / 3 = {3j-1, 3j, 3j+1},
 *                            divisor always 3, only for j <= (D - 1) / 3;  e5: AvgPool1d(5, stride 5), window d / 5 < D / 5
 *   + sign(p) (a_ef[0] E0 + a_ef[1] E1 + a_ef[2] E2 + a_ef[3] E3)     E = sum |pred| - sum |gt| over [0] the 20 channels of
 *                            the element's frame, [1] channels and all frames, [2] the 10 bins of its polarity and frame,
 *                            [3] bins and all frames; sign(0) = 0
 *   + a_comp e / max(cp, 1) if p > 0.01f (f32 compare)     per column (b, l, w) over (c, h): S = sum of v (v > 0.01f),
 *                            c = count, e = Sp / max(cp, 1) - Sg / max(cg, 1)
 *   + a_match (exp(p - logsumexp_l p) - [l == t])     per (b, c, h, w); t = the first argmax over l of gt
 *   + a_l1 sign(p) + a_l2 p
 * The caller folds every constant into the f64 factors: the term's alpha, 2 / n with n the batch-total count of the
 * forward record (v2ce_voxlosses_stats: n, pyr_n, temporal_n, ef_n, comp_n, match_n), 1 / k^3, the / 3 and / 2 of the
 * pyramid and temporal classes, 1 / number of refinement stages, and for a_l2 the 1 / ||pred||_2 of the forward record.
 * A factor of zero switches its term's work off.  struct_size = sizeof(v2ce_voxloss_grad_coeffs). */
typedef struct v2ce_voxloss_grad_coeffs {
    int64_t struct_size;
    double a_sq;
    double a_pyr[3];
    double a_t3, a_t5;
    double a_ef[4];
    double a_comp;
    double a_match;
    double a_l1, a_l2;
} v2ce_voxloss_grad_coeffs;

/* v2ce_voxloss_grads: pred, gt, grad [B][L][C][H][W] f32 (C must be 20, channels (p c)), contiguous, 4-byte aligned,
 * B * L * C * H * W * 4 bytes each; grad must not overlap pred or gt.  v2ce_volume_loss_grads: the same for [N][D][H][W]
 * (what 'b l (p c) h w -> (b p) (l c) h w' hands to Pyramid3dLoss / PyramidTemporalLoss) with a_sq, a_pyr, a_t3, a_t5
 * only: any other non-zero factor is refused.  On the rearranged copy of a 5-D tensor it writes the 5-D entry's
 * gradient, rearranged, bit for bit.
 *   coef      HOST pointer, read before the call returns; coef_struct_size and coef->struct_size must both be
 *             sizeof(v2ce_voxloss_grad_coeffs)
 *   upstream  one f32 on the device, the incoming gradient of the loss, or NULL for 1; read by the kernel, so the
 *             backward needs no host synchronisation
 *   grad      every element is written (zeros included): (float)(sum of the terms in f64 * (double)upstream[0])
 *   workspace >= the *_workspace_bytes value, 8-byte aligned; scratch, nothing is read before it is written
 * Every difference, sum, quotient, exp and log is f64 from the f32 inputs; the one rounding to f32 is the store.  No
 * atomics: the bytes are identical run to run, and for a given coef the gradient of b / n does not depend on what else
 * is in the call.  1 <= B, N <= 65535; a non-zero a_pyr needs min(D, H, W) >= 8 and a non-zero a_t3 / a_t5 D >= 5
 * (D = 10 L for sequences), else V2CE_ERR_BAD_ARG, as for NULL pointers and C != 20; the *_workspace_bytes queries
 * return 0 for arguments the entry refuses.  A small workspace is V2CE_ERR_WORKSPACE and nothing is written. */
size_t v2ce_voxloss_grads_workspace_bytes(int B, int L, int C, int H, int W, const v2ce_voxloss_grad_coeffs *coef,
                                          size_t coef_struct_size);
int v2ce_voxloss_grads(const float *pred, const float *gt, int B, int L, int C, int H, int W,
                       const v2ce_voxloss_grad_coeffs *coef, size_t coef_struct_size, const float *upstream, float *grad,
                       void *workspace, size_t workspace_bytes, v2ce_stream_t stream);
size_t v2ce_volume_loss_grads_workspace_bytes(int N, int D, int H, int W, const v2ce_voxloss_grad_coeffs *coef,
                                              size_t coef_struct_size);
int v2ce_volume_loss_grads(const float *pred, const float *gt, int N, int D, int H, int W,
                           const v2ce_voxloss_grad_coeffs *coef, size_t coef_struct_size, const float *upstream,
                           float *grad, void *workspace, size_t workspace_bytes, v2ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2CE_HIP_GRAD_H */
