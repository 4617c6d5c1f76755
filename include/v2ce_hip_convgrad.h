/* v2ce_hip_convgrad.h -- weight gradients of the trunk's convolutions in libv2ce_hip.so: the 3x3x3 Conv3d(32, 32) of the
 * last decoder block (UNet.decoders[3].conv2) on the exact-f32 MFMA.
 *
 * The conventions of v2ce_hip.h hold: device pointers unless stated, entries enqueue on `stream` and do not synchronise,
 * they return V2CE_OK or a negative error code, v2ce_last_error() describes the last failure.
 *
 * v2ce_conv32_wgrad (csrc/convnwgrad.hip): the gradient of a stride-1, zero-padded 3x3x3 convolution 32 -> 32 with respect
 * to its weight and to a per-channel shift added behind it, seen through the relu that follows.
 *   x, y, upstream  V2CE_LAYOUT_C16 with two channel groups: [B][L][2][H][pitch][16] f32, 16-byte aligned, B * L * 2 * H *
 *                   pitch * 64 bytes each; pitch >= W; the columns W .. pitch-1 of a row are never read.  x is the
 *                   convolution's input, y the block's output relu(...), upstream the gradient with respect to y
 *   d_weight        [32][32][3][3][3] f32 (co, ci, kt, kh, kw: nn.Conv3d's own order);  d_shift [32]
 *   workspace       >= v2ce_conv32_wgrad_workspace_bytes(...) for the same max_workgroups, 8-byte aligned; scratch, nothing
 *                   is read before it is written
 * With m = upstream where y > 0, else 0 (torch's relu backward on the result: a NaN in y gives 0, a NaN in upstream
 * propagates); y == NULL: m = upstream, the plain weight gradient of the convolution:
 *     d_weight[co][ci][kt][kh][kw] = sum over b, l, h, w of m[co][b, l, h, w] * x[ci][b, l + kt - 1, h + kh - 1, w + kw - 1]
 *     d_shift[co]                  = sum over b, l, h, w of m[co][b, l, h, w]
 * where a term whose l + kt - 1, h + kh - 1 or w + kw - 1 falls outside 0 .. L-1, 0 .. H-1 or 0 .. W-1 is zero; nothing
 * leaks across b.  (x is expected to be finite: a zero of m does not mask a non-finite x.)  d_weight or d_shift may be
 * NULL (its work is skipped), not both.  Cin = Cout = 32 is fixed.
 *
 * B, L, H, W >= 1, B * L * H * W < 2^31 and B * L * H * pitch < 2^34, max_workgroups >= 0, else V2CE_ERR_BAD_ARG, as for
 * NULL x, upstream or workspace and a misaligned x, y, upstream or workspace; the size query returns 0 for arguments the
 * entry refuses.  A small workspace is V2CE_ERR_WORKSPACE and nothing is written.  Outputs must not overlap inputs or each
 * other.
 *
 * Precision contract.  The products and the inner accumulation of d_weight run on v_mfma_f32_32x32x2_f32, bit for bit an
 * f32 fmaf chain over the positions.  One f32 accumulator sums at most V2CE_WGRAD_CHAIN positions; it is then added into
 * an f64 sum and starts again from zero.  Everything above that level is f64: the per-workgroup f64 partial sums in the
 * workspace and the finish kernel that adds them in the order of the workgroups.  d_shift is f64 throughout.  There is one
 * rounding to f32, at the store.  So for an element whose terms have the absolute sum S over N positions
 *     |d_weight - exact| <= ulp32(exact) + V2CE_WGRAD_CHAIN * 2^-24 * S + N * 2^-52 * S
 * and d_shift is within one rounding.  There are no atomics: the bytes are identical from run to run for the same
 * max_workgroups, and an output does not depend on whether the other one was asked for.
 *
 * max_workgroups: 0 = the kernel's own choice (one workgroup per tile of 2 x 64 positions, at most 256); n > 0 caps the
 * grid at n workgroups.  The result depends on n only through the order of the f64 sums: which tiles share a workgroup's
 * f32 chain and in which order the partial sums are added. */
#ifndef V2CE_HIP_CONVGRAD_H
#define V2CE_HIP_CONVGRAD_H

#include "v2ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define V2CE_WGRAD_CHAIN 4096

size_t v2ce_conv32_wgrad_workspace_bytes(int B, int L, int H, int W, int pitch, int max_workgroups);
int v2ce_conv32_wgrad(const float *x, const float *y, const float *upstream, int B, int L, int H, int W, int pitch,
                      float *d_weight, float *d_shift, void *workspace, size_t workspace_bytes, int max_workgroups,
                      v2ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2CE_HIP_CONVGRAD_H */
