/* v2ce_hip_convupndgrad.h -- input gradients of the first half of a decoder block in libv2ce_hip.so: of the 3x3x3
 * Conv3d(c0 + c1, cout) conv1 and of the 1x1x1 Conv3d(c0 + c1, cout) shortcut with respect to the block's two sources, on
 * the exact-f32 MFMA, for c0 in {64, 128}, c1 in {32, 64} and cout in {32, 64}.  UNet.decoders[2].conv1 and
 * .downsample[0] are the 128 + 64 -> 64 case, UNet.decoders[3]'s the 64 + 32 -> 32 case, which v2ce_hip_convupdgrad.h
 * also offers without the channel arguments.  The block's input is the 2x nearest-upsampled output of the decoder in
 * front of it, concatenated with the skip tensor; the gradient goes back through that concat and that upsample without
 * materialising either.
 *
 * The conventions of v2ce_hip.h hold: device pointers unless stated, entries enqueue on `stream` and do not synchronise,
 * they return V2CE_OK or a negative error code, v2ce_last_error() describes the last failure.  The weight gradients of the
 * same two layers are v2ce_hip_convupngrad.h's, the input gradient of the convolution behind them is
 * v2ce_hip_convngrad.h's; this header mirrors their refusals.
 *
 * v2ce_convupn_dgrad (csrc/convupdgrad.hip), with cin = c0 + c1:
 *   weight        [cout][cin][3][3][3] f32 (co, ci, kt, kh, kw: nn.Conv3d's own order);  short_weight [cout][cin] f32.
 *                 Both 4-byte aligned, as the caller holds them: the entry repacks them into the workspace itself
 *   g1, gd        V2CE_LAYOUT_C16 with cout / 16 channel groups: [B][L][cout / 16][H][pitch][16] f32, pitch >= W.  g1 is
 *                 the gradient with respect to conv1's raw output, gd the gradient with respect to the shortcut
 *                 convolution's raw output
 *   d_x1          V2CE_LAYOUT_C16 with c1 / 16 channel groups: [B][L][c1 / 16][H][pitch][16] f32: the gradient with
 *                 respect to the skip tensor
 *   d_x0          V2CE_LAYOUT_C16 with c0 / 16 channel groups at the SOURCE resolution: [B][L][c0 / 16][H0][pitch0][16]
 *                 f32 with H0 = (H + 1) / 2, W0 = (W + 1) / 2, pitch0 >= W0: the gradient with respect to the c0 channels
 *                 the forward upsamples
 *                 All four are 16-byte aligned.  The columns W .. pitch-1 of a row of g1 and gd are never read; in d_x1
 *                 they, and in d_x0 the columns W0 .. pitch0-1, are written as zeros over the whole pitch, so an output
 *                 has no undefined byte
 *   workspace     >= v2ce_convupn_dgrad_workspace_bytes(...), 8-byte aligned; scratch, nothing is read before it is
 *                 written.  It holds the repacked weights: 28 * cout * cin floats, rounded up to 256 bytes
 * With X = cat(nearest_upsample_2x(x0), x1), X[ci][b, l, h, w] = x0[ci][b, l, h >> 1, w >> 1] for ci < c0 and
 * x1[ci - c0][b, l, h, w] for c0 <= ci < cin:
 *     d_X[ci][b, l, h, w]   = sum over co, kt, kh, kw of weight[co][ci][kt][kh][kw] * g1[co][b, l - kt + 1, h - kh + 1, w - kw + 1]
 *                           + sum over co of short_weight[co][ci] * gd[co][b, l, h, w]                    (0 <= ci < cin)
 *     d_x1[c][b, l, h, w]   = d_X[c0 + c][b, l, h, w]                                                      (0 <= c < c1)
 *     d_x0[c][b, l, h0, w0] = sum of d_X[c][b, l, h, w] over the output positions (h, w) with h >> 1 == h0, w >> 1 == w0,
 *                             h < H, w < W                                                                 (0 <= c < c0)
 * where a term whose l - kt + 1, h - kh + 1 or w - kw + 1 falls outside 0 .. L-1, 0 .. H-1 or 0 .. W-1 is zero; nothing
 * leaks across b.  d_X exists at output positions only: with an odd H or W the last source row or column collects ONE
 * output row or column -- the convolution sum at h = H or w = W is not zero, and it is not added.  There is no relu mask
 * in this entry: g1 and gd arrive masked, and masking d_x0 by x0 > 0 is the consumer's business.  (The weights are
 * expected to be finite: a zero of g1 or gd does not mask a non-finite weight.)
 *
 * g1 may be NULL (weight is then unused and may be NULL): the shortcut's share alone.  gd may be NULL (short_weight
 * likewise): conv1's share alone.  Not both.  d_x0 or d_x1 may be NULL (the work of its channel groups is skipped), not
 * both.
 *
 * c0 in {64, 128}, c1 in {32, 64}, cout in {32, 64}, B, L, H, W >= 1, pitch >= W, pitch0 >= (W + 1) / 2, B * L * H * W <
 * 2^31, B * L * H * pitch < 2^34 and B * L * H0 * pitch0 < 2^34, max_workgroups >= 0, else V2CE_ERR_BAD_ARG, as for g1 and
 * gd both NULL, g1 without weight, gd without short_weight, d_x0 and d_x1 both NULL, a NULL workspace, a misaligned g1,
 * gd, d_x0, d_x1 (16 bytes), weight, short_weight (4 bytes) or workspace (8 bytes); the size query returns 0 for arguments
 * the entry refuses and is > 0 otherwise.  A small workspace is V2CE_ERR_WORKSPACE and nothing is written.  Outputs must
 * not overlap inputs or each other.
 *
 * Precision contract.  The products and the sums run on v_mfma_f32_32x32x2_f32, and in plain f32 additions where the four
 * partial accumulators of a position and the up to four positions of a source pixel meet.  A d_x1 element is an f32 sum of
 * V2CE_UPNDGRAD_TERMS(cout) = 28 * cout exact-product terms in an order fixed by cout (27 taps and the shortcut, each over
 * cout output channels, 32 at a time; terms of the zero padding and of a NULL g1 or gd included, as zeros); a d_x0 element
 * is a sum of n = V2CE_UPNDGRAD_TERMS(cout) times the number of its output positions (1, 2 or 4) such terms.  Any order of
 * an n-term f32 sum is within n 2^-24 / (1 - n 2^-24) of its sum of |terms|, so with n the element's term count and S its
 * sum of |terms|
 *     |out - exact| <= (n + 1) * 2^-24 * S + n * 2^-126
 * where the second term covers products and sums flushed below the normal range.
 *
 * Determinism.  There are no atomics.  Every output element is produced by one workgroup -- a tile of 2 x 64 positions
 * starts at an even row and an even column, so the output positions of a source pixel lie in one tile -- in an order
 * fixed by cout, the split of the 28 units over the four waves and (for d_x0) the pool order alone: the bytes are
 * identical from run to run, for any max_workgroups, for base pointers moved by 16 bytes, and whichever other output was
 * asked for.  v2ce_convupn_dgrad(64, 32, 32, ...) returns the bytes of v2ce_hip_convupdgrad.h's entry: both run the same kernel
 * instance.
 *
 * max_workgroups: the grid is one workgroup per requested 32-channel group of X (c0 / 32 for d_x0, c1 / 32 for d_x1) for
 * every share of the tiles.  0 = the kernel's own choice (one share per tile, at most 256 workgroups); n > 0 caps the grid
 * at max(n / groups, 1) shares, each walking a contiguous run of the tiles.  The result does not depend on n. */
#ifndef V2CE_HIP_CONVUPNDGRAD_H
#define V2CE_HIP_CONVUPNDGRAD_H

#include "v2ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define V2CE_UPNDGRAD_TERMS(cout) (28 * (cout))

size_t v2ce_convupn_dgrad_workspace_bytes(int c0, int c1, int cout, int B, int L, int H, int W, int pitch, int pitch0,
                                          int max_workgroups);
int v2ce_convupn_dgrad(const float *weight, const float *short_weight, const float *g1, const float *gd, int c0, int c1, int cout,
                       int B, int L, int H, int W, int pitch, int pitch0, float *d_x0, float *d_x1, void *workspace,
                       size_t workspace_bytes, int max_workgroups, v2ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2CE_HIP_CONVUPNDGRAD_H */
