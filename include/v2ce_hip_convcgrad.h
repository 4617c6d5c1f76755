/* v2ce_hip_convcgrad.h -- weight and input gradients of the trunk's 3x3x3 convolutions with any of the UNet's channel
 * widths on either side in libv2ce_hip.so, on the exact-f32 MFMA: cin and cout are each one of 32, 64, 128, 256, 512, chosen
 * independently.  UNet.decoders[1].conv2, the Conv3d(128, 128) whose output decoders[2] consumes, is the 128 -> 128 case;
 * decoders[0].conv2 is 256 -> 256, the resblocks' convolutions 512 -> 512.  At cin, cout in {32, 64} the entries restate
 * those of v2ce_hip_convngrad.h byte for byte, hence at 32 -> 32 those of v2ce_hip_convgrad.h and v2ce_hip_convdgrad.h.
 *
 * The conventions of v2ce_hip.h hold: device pointers unless stated, entries enqueue on `stream` and do not synchronise,
 * they return V2CE_OK or a negative error code, v2ce_last_error() describes the last failure.
 *
 * Tensors.  An activation with C channels is V2CE_LAYOUT_C16 with C / 16 planes: [B][L][C / 16][H][pitch][16] f32, 16-byte
 * aligned, B * L * (C / 16) * H * pitch * 64 bytes; pitch >= W.  cin and cout are each 32, 64, 128, 256 or 512; anything
 * else is V2CE_ERR_BAD_ARG.  With m = upstream where y > 0, else 0 (torch's relu backward on the result: a NaN in y gives
 * 0, a NaN in upstream propagates); y == NULL: m = upstream, the plain gradients of the convolution.
 *
 * v2ce_convc_wgrad (csrc/convnwgrad.hip): the gradient of a stride-1, zero-padded 3x3x3 convolution cin -> cout with
 * respect to its weight and to a per-channel shift added behind it, seen through the relu that follows.
 *   x               cin channels, the convolution's input;  y, upstream: cout channels, the layer's output relu(...) and the
 *                   gradient with respect to it.  The columns W .. pitch-1 of a row are never read
 *   d_weight        [cout][cin][3][3][3] f32 (co, ci, kt, kh, kw: nn.Conv3d's own order);  d_shift [cout]
 *   workspace       >= v2ce_convc_wgrad_workspace_bytes(...) for the same cin, cout and max_workgroups, 8-byte aligned;
 *                   scratch, nothing is read before it is written.  It is shares * pairs * (27 * 1024 + 32) f64 rounded up
 *                   to 256 bytes, at most 256 * (27 * 1024 + 32) * 8 bytes = 56.7 MB
 *     d_weight[co][ci][kt][kh][kw] = sum over b, l, h, w of m[co][b, l, h, w] * x[ci][b, l + kt - 1, h + kh - 1, w + kw - 1]
 *     d_shift[co]                  = sum over b, l, h, w of m[co][b, l, h, w]
 * where a term whose l + kt - 1, h + kh - 1 or w + kw - 1 falls outside 0 .. L-1, 0 .. H-1 or 0 .. W-1 is zero; nothing
 * leaks across b.  (x is expected to be finite: a zero of m does not mask a non-finite x.)  d_weight or d_shift may be
 * NULL (its work is skipped), not both.
 *
 * Precision contract of v2ce_convc_wgrad.  The products and the inner accumulation of d_weight run on
 * v_mfma_f32_32x32x2_f32, bit for bit an f32 fmaf chain over the positions.  One f32 accumulator sums at most
 * V2CE_WGRAD_CHAIN positions; it is then added into an f64 sum and starts again from zero.  Everything above that level is
 * f64: the per-workgroup partial sums in the workspace and the finish kernel that adds them in the order of the shares.
 * d_shift is f64 throughout.  There is one rounding to f32, at the store.  So for an element whose terms have the absolute
 * sum S over N positions
 *     |d_weight - exact| <= ulp32(exact) + V2CE_WGRAD_CHAIN * 2^-24 * S + N * 2^-52 * S
 * and d_shift is within one rounding.  There are no atomics: the bytes are identical from run to run for the same
 * max_workgroups, and an output does not depend on whether the other one was asked for.
 *
 * max_workgroups of v2ce_convc_wgrad.  The grid is pairs x shares with pairs = (cout / 32) * (cin / 32) <= 256: one
 * workgroup per (co group, ci group) pair of 32 x 32 channels for every share of the tiles of 2 x 64 positions; d_shift is
 * taken by the pairs with ci group 0.  0 = the kernel's own choice: one share per tile, at most 256 / pairs shares (one
 * share at 512 -> 512).  n > 0 caps the shares at max(n / pairs, 1) (so the grid at n workgroups wherever n >= pairs).  The
 * result depends on n only through the order of the f64 sums: which tiles share a workgroup's f32 chain and in which order
 * the partial sums are added.  For cin, cout in {32, 64} the bytes are those of v2ce_hip_convngrad.h's entry for the
 * same max_workgroups.
 *
 * v2ce_convc_dgrad (csrc/convndgrad.hip): the gradient of the same convolution with respect to its input and to a residual
 * added behind it, seen through the relu that follows.
 *   y, upstream, d_res  cout channels;  d_x: cin channels.  The columns W .. pitch-1 of a row of y and upstream are never
 *                   read; in d_x and d_res they are written as zeros, so an output has no undefined byte
 *   weight          [cout][cin][3][3][3] f32 (nn.Conv3d's own order), 4-byte aligned, as the caller holds it: the entry
 *                   repacks it into the workspace itself
 *   workspace       >= v2ce_convc_dgrad_workspace_bytes(...), 8-byte aligned; scratch, nothing is read before it is written.
 *                   It is 27 * cout * cin f32 rounded up to 256 bytes
 *     d_x[ci][b, l, h, w] = sum over co, kt, kh, kw of weight[co][ci][kt][kh][kw] * m[co][b, l - kt + 1, h - kh + 1, w - kw + 1]
 *     d_res               = m
 * where a term whose l - kt + 1, h - kh + 1 or w - kw + 1 falls outside 0 .. L-1, 0 .. H-1 or 0 .. W-1 is zero; nothing
 * leaks across b.  (weight is expected to be finite: a zero of m does not mask a non-finite weight.)  d_x or d_res may be
 * NULL (its work is skipped), not both.
 *
 * Precision contract of v2ce_convc_dgrad.  The products and the sums of d_x run on v_mfma_f32_32x32x2_f32, and in plain f32
 * additions where the four partial accumulators of an element meet.  One workgroup produces a whole d_x element: each of
 * its four waves runs its taps over co group 0, 1, ..., cout / 32 - 1, in that order, into the same accumulator, and the
 * four partials are added in the order of the waves.  (From cout = 128 on a wave fetches the weights of one co group at a
 * time again per tile; that changes where an operand comes from, not the order of the sum.)  An element is an f32 sum of
 * 27 * cout exact-product terms in an order fixed by cout and the tap split alone (terms of the zero padding included, as
 * zeros).  With S = the sum of |terms|
 *     |d_x - exact| <= (27 * cout + 1) * 2^-24 * S + 27 * cout * 2^-126
 * where the second term covers products and sums flushed below the normal range.  d_res is a copy: its bytes are those of
 * where(y > 0, upstream, 0).
 *
 * Determinism of v2ce_convc_dgrad.  There are no atomics, and an element's order does not depend on the grid: the bytes are
 * identical from run to run, for any max_workgroups and for a base pointer moved by 16 bytes.  An output does not depend
 * on whether the other one was asked for.  For cin, cout in {32, 64} the bytes are those of v2ce_hip_convngrad.h's entry.
 *
 * max_workgroups of v2ce_convc_dgrad.  The grid is (cin / 32) x shares: one workgroup per group of 32 input channels for
 * every share of the tiles of 2 x 64 positions; d_res and the padding columns of d_res are written by the workgroups of ci
 * group 0, for any number of planes.  0 = one share per tile, at most 256 / (cin / 32) shares; n > 0 caps the shares at
 * max(n / (cin / 32), 1).  The result does not depend on n.
 *
 * Refusals of both entries.  B, L, H, W >= 1, B * L * H * W < 2^31 and B * L * H * pitch < 2^34, max_workgroups >= 0, cin
 * and cout in {32, 64, 128, 256, 512}, else V2CE_ERR_BAD_ARG, as for a NULL x / weight, upstream or workspace and a
 * misaligned activation, output or workspace; the size queries return 0 for arguments the entry refuses and are > 0
 * otherwise.  A small workspace is V2CE_ERR_WORKSPACE and nothing is written.  Outputs must not overlap inputs or each
 * other.  The entries of v2ce_hip_convngrad.h keep refusing anything wider than 64 channels. */
#ifndef V2CE_HIP_CONVCGRAD_H
#define V2CE_HIP_CONVCGRAD_H

#include "v2ce_hip.h"
#include "v2ce_hip_convgrad.h" /* V2CE_WGRAD_CHAIN */

#ifdef __cplusplus
extern "C" {
#endif

size_t v2ce_convc_wgrad_workspace_bytes(int cin, int cout, int B, int L, int H, int W, int pitch, int max_workgroups);
int v2ce_convc_wgrad(const float *x, const float *y, const float *upstream, int cin, int cout, int B, int L, int H, int W,
                     int pitch, float *d_weight, float *d_shift, void *workspace, size_t workspace_bytes, int max_workgroups,
                     v2ce_stream_t stream);

size_t v2ce_convc_dgrad_workspace_bytes(int cin, int cout, int B, int L, int H, int W, int pitch, int max_workgroups);
int v2ce_convc_dgrad(const float *weight, const float *y, const float *upstream, int cin, int cout, int B, int L, int H, int W,
                     int pitch, float *d_x, float *d_res, void *workspace, size_t workspace_bytes, int max_workgroups,
                     v2ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2CE_HIP_CONVCGRAD_H */
