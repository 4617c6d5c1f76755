/* v2ce_hip_convdgrad.h -- input gradients of the trunk's convolutions in libv2ce_hip.so: the 3x3x3 Conv3d(32, 32) of the
 * last decoder block (UNet.decoders[3].conv2) on the exact-f32 MFMA.
 *
 * The conventions of v2ce_hip.h hold: device pointers unless stated, entries enqueue on `stream` and do not synchronise,
 * they return V2CE_OK or a negative error code, v2ce_last_error() describes the last failure.
 *
 * v2ce_conv32_dgrad (csrc/convndgrad.hip): the gradient of a stride-1, zero-padded 3x3x3 convolution 32 -> 32 with respect
 * to its input and to a residual added behind it, seen through the relu that follows.
 *   y, upstream, d_x, d_res  V2CE_LAYOUT_C16 with two channel groups: [B][L][2][H][pitch][16] f32, 16-byte aligned, B * L * 2
 *                   * H * pitch * 64 bytes each; pitch >= W.  y is the block's output relu(...), upstream the gradient with
 *                   respect to y.  The columns W .. pitch-1 of a row of y and upstream are never read; in d_x and d_res
 *                   they are written as zeros, so an output has no undefined byte
 *   weight          [32][32][3][3][3] f32 (co, ci, kt, kh, kw: nn.Conv3d's own order), 4-byte aligned, as the caller holds
 *                   it: the entry repacks it into the workspace itself
 *   workspace       >= v2ce_conv32_dgrad_workspace_bytes(...), 8-byte aligned; scratch, nothing is read before it is written
 * With m = upstream where y > 0, else 0 (torch's relu backward on the result: a NaN in y gives 0, a NaN in upstream
 * propagates); y == NULL: m = upstream, the plain input gradient of the convolution:
 *     d_x[ci][b, l, h, w] = sum over co, kt, kh, kw of weight[co][ci][kt][kh][kw] * m[co][b, l - kt + 1, h - kh + 1, w - kw + 1]
 *     d_res               = m
 * where a term whose l - kt + 1, h - kh + 1 or w - kw + 1 falls outside 0 .. L-1, 0 .. H-1 or 0 .. W-1 is zero; nothing
 * leaks across b.  (weight is expected to be finite: a zero of m does not mask a non-finite weight.)  d_x or d_res may be
 * NULL (its work is skipped), not both.  Cin = Cout = 32 is fixed.
 *
 * B, L, H, W >= 1, B * L * H * W < 2^31 and B * L * H * pitch < 2^34, max_workgroups >= 0, else V2CE_ERR_BAD_ARG, as for
 * NULL weight, upstream or workspace and a misaligned y, upstream, d_x, d_res or workspace; the size query returns 0 for
 * arguments the entry refuses and is > 0 otherwise.  A small workspace is V2CE_ERR_WORKSPACE and nothing is written.
 * Outputs must not overlap inputs or each other.
 *
 * Precision contract.  The products and the sums of d_x run on v_mfma_f32_32x32x2_f32, and in plain f32 additions where
 * the four partial accumulators of an element meet.  An element is an f32 sum of V2CE_DGRAD_TERMS = 32 * 27 exact-product
 * terms in a fixed order (terms of the zero padding included, as zeros).  Any order of an n-term f32 sum is within
 * n 2^-24 / (1 - n 2^-24) of its sum of |terms|, so with S = the sum of |terms| of the element
 *     |d_x - exact| <= (V2CE_DGRAD_TERMS + 1) * 2^-24 * S + V2CE_DGRAD_TERMS * 2^-126
 * where the second term covers products and sums flushed below the normal range.  d_res is a copy: its bytes are those of
 * where(y > 0, upstream, 0).
 *
 * Determinism.  There are no atomics.  Every d_x element is produced by one workgroup, in an order that does not depend
 * on the grid: the bytes are identical from run to run, for any max_workgroups and for a base pointer moved by 16 bytes.
 * An output does not depend on whether the other one was asked for.
 *
 * max_workgroups: 0 = the kernel's own choice (one workgroup per tile of 2 x 64 positions, at most 256); n > 0 caps the
 * grid at n workgroups, each walking a contiguous share of the tiles.  The result does not depend on n. */
#ifndef V2CE_HIP_CONVDGRAD_H
#define V2CE_HIP_CONVDGRAD_H

#include "v2ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define V2CE_DGRAD_TERMS 864

size_t v2ce_conv32_dgrad_workspace_bytes(int B, int L, int H, int W, int pitch, int max_workgroups);
int v2ce_conv32_dgrad(const float *weight, const float *y, const float *upstream, int B, int L, int H, int W, int pitch,
                      float *d_x, float *d_res, void *workspace, size_t workspace_bytes, int max_workgroups,
                      v2ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2CE_HIP_CONVDGRAD_H */
