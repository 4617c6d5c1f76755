/* v2ce_hip_convupngrad.h -- weight gradients of the first half of a decoder block in libv2ce_hip.so with the channel counts
 * as arguments: the 3x3x3 Conv3d(c0 + c1, cout) conv1 and the 1x1x1 Conv3d(c0 + c1, cout) shortcut on the exact-f32 MFMA,
 * both reading the block's input -- the 2x nearest-upsampled output of the decoder in front of it (c0 channels),
 * concatenated with the skip tensor (c1 channels) -- without materialising it.  UNet.decoders[2].conv1 and .downsample[0]
 * are 128 + 64 -> 64; at 64 + 32 -> 32 the entry is that of v2ce_hip_convupgrad.h, byte for byte.
 *
 * The conventions of v2ce_hip.h hold: device pointers unless stated, entries enqueue on `stream` and do not synchronise,
 * they return V2CE_OK or a negative error code, v2ce_last_error() describes the last failure.  This header restates the
 * contract of v2ce_hip_convupgrad.h and shares its V2CE_UPWGRAD_CHAIN.
 *
 * v2ce_convupn_wgrad (csrc/convupnwgrad.hip):
 *   c0, c1, cout  channels of the upsampled source, of the skip tensor and of either convolution's output: c0 in {64, 128},
 *               c1 in {32, 64}, cout in {32, 64}; C = c0 + c1 below
 *   x0          V2CE_LAYOUT_C16 with c0 / 16 channel groups at the SOURCE resolution: [B][L][c0/16][H0][pitch0][16] f32 with
 *               H0 = (H + 1) / 2, W0 = (W + 1) / 2, pitch0 >= W0: the channels the forward upsamples
 *   x1          V2CE_LAYOUT_C16 with c1 / 16 channel groups: [B][L][c1/16][H][pitch][16] f32, pitch >= W: the skip tensor
 *   g1, gd      V2CE_LAYOUT_C16 with cout / 16 channel groups: [B][L][cout/16][H][pitch][16] f32.  g1 is the gradient with
 *               respect to conv1's raw output, gd the gradient with respect to the shortcut convolution's raw output
 *               All four are 16-byte aligned; the columns W .. pitch-1 and W0 .. pitch0-1 of a row are never read.
 *   d_weight    [cout][C][3][3][3] f32 (co, ci, kt, kh, kw: nn.Conv3d's own order);  d_short [cout][C];  d_short_bias [cout]
 *   workspace   >= v2ce_convupn_wgrad_workspace_bytes(...) for the same channel counts and max_workgroups, 8-byte aligned;
 *               scratch, nothing is read before it is written
 * The virtual input is X[ci][b, l, h, w] = x0[ci][b, l, h >> 1, w >> 1] for ci < c0 and x1[ci - c0][b, l, h, w] for
 * c0 <= ci < C (the channel order of cat([upsample(x), skip])):
 *     d_weight[co][ci][kt][kh][kw] = sum over b, l, h, w of g1[co][b, l, h, w] * X[ci][b, l + kt - 1, h + kh - 1, w + kw - 1]
 *     d_short[co][ci]              = sum over b, l, h, w of gd[co][b, l, h, w] * X[ci][b, l, h, w]
 *     d_short_bias[co]             = sum over b, l, h, w of gd[co][b, l, h, w]
 * The zero padding is that of the UPSAMPLED tensor: a term whose l + kt - 1, h + kh - 1 or w + kw - 1 falls outside
 * 0 .. L-1, 0 .. H-1 or 0 .. W-1 is zero, whatever the source range says (with an odd H the last source row is seen through
 * one output row only).  Nothing leaks across b.  There is no relu mask in this entry: g1 and gd arrive masked.  (X is
 * expected to be finite: a zero of g1 or gd does not mask a non-finite X.)
 *
 * Any output may be NULL (its work is skipped), not all three.  d_weight needs g1, d_short and d_short_bias need gd, d_weight
 * and d_short need x0 and x1; an input that no requested output needs may be NULL.
 *
 * c0, c1, cout as above, B, L, H, W >= 1, pitch >= W, pitch0 >= (W + 1) / 2, B * L * H * W < 2^31, B * L * H * pitch < 2^34
 * and B * L * H0 * pitch0 < 2^34, max_workgroups >= 0, else V2CE_ERR_BAD_ARG, as for a NULL needed input or workspace and a
 * misaligned x0, x1, g1, gd (16 bytes) or workspace (8 bytes); the size query returns 0 for arguments the entry refuses.  A
 * small workspace is V2CE_ERR_WORKSPACE and nothing is written.  Outputs must not overlap inputs or each other.
 *
 * Precision contract.  The products and the inner accumulation of d_weight and d_short run on v_mfma_f32_32x32x2_f32, bit
 * for bit an f32 fmaf chain over the positions.  One f32 accumulator sums at most V2CE_UPWGRAD_CHAIN positions; it is then
 * added into an f64 sum and starts again from zero.  Everything above that level is f64: the per-workgroup f64 partial sums
 * in the workspace and the finish kernel that adds a pair's partials in the order of the shares.  d_short_bias is f64
 * throughout.  There is one rounding to f32, at the store.  So for an element of d_weight or d_short whose terms have the
 * absolute sum S over N positions
 *     |out - exact| <= ulp32(exact) + V2CE_UPWGRAD_CHAIN * 2^-24 * S + N * 2^-52 * S
 * and d_short_bias is within one rounding.  There are no atomics: the bytes are identical from run to run for the same
 * max_workgroups; they do not depend on the base pointers nor on which other outputs were asked for.
 *
 * max_workgroups: with pairs = (cout / 32) * (C / 32) the grid is `pairs` workgroups -- one per (32 output channels, 32-channel
 * group of X) -- for every share of the tiles of 2 x 64 positions; the pairs with X group 0 also take d_short_bias.  0 = the
 * kernel's own choice (one share per tile, at most 256 / pairs shares); n > 0 caps the shares at max(n / pairs, 1).  The
 * result depends on n only through the order of the f64 sums: which tiles share a workgroup's f32 chain and in which order
 * the partial sums are added.  At (c0, c1, cout) = (64, 32, 32) these are the rules of v2ce_hip_convupgrad.h's entry (pairs
 * 3, 85 shares) and the outputs are its bytes for the same max_workgroups. */
#ifndef V2CE_HIP_CONVUPNGRAD_H
#define V2CE_HIP_CONVUPNGRAD_H

#include "v2ce_hip.h"
#include "v2ce_hip_convupgrad.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t v2ce_convupn_wgrad_workspace_bytes(int c0, int c1, int cout, int B, int L, int H, int W, int pitch, int pitch0,
                                          int max_workgroups);
int v2ce_convupn_wgrad(const float *x0, const float *x1, const float *g1, const float *gd, int c0, int c1, int cout, int B, int L,
                       int H, int W, int pitch, int pitch0, float *d_weight, float *d_short, float *d_short_bias, void *workspace,
                       size_t workspace_bytes, int max_workgroups, v2ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2CE_HIP_CONVUPNGRAD_H */
