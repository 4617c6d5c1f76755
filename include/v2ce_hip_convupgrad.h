/* v2ce_hip_convupgrad.h -- weight gradients of the first half of the last decoder block in libv2ce_hip.so: the 3x3x3
 * Conv3d(96, 32) conv1 and the 1x1x1 Conv3d(96, 32) shortcut (UNet.decoders[3].conv1 and .downsample[0]) on the exact-f32
 * MFMA, both reading the block's input -- the 2x nearest-upsampled output of the decoder in front of it, concatenated with
 * the skip tensor -- without materialising it.
 *
 * The conventions of v2ce_hip.h hold: device pointers unless stated, entries enqueue on `stream` and do not synchronise,
 * they return V2CE_OK or a negative error code, v2ce_last_error() describes the last failure.  The 32-channel entries of
 * v2ce_hip_convgrad.h and v2ce_hip_convdgrad.h are the layers behind this one; this header mirrors their refusals.
 *
 * v2ce_convup_wgrad (csrc/convupnwgrad.hip):
 *   x0          V2CE_LAYOUT_C16 with four channel groups at the SOURCE resolution: [B][L][4][H0][pitch0][16] f32 with
 *               H0 = (H + 1) / 2, W0 = (W + 1) / 2, pitch0 >= W0: the 64 channels the forward upsamples
 *   x1, g1, gd  V2CE_LAYOUT_C16 with two channel groups: [B][L][2][H][pitch][16] f32, pitch >= W.  x1 is the skip tensor
 *               (32 channels), g1 the gradient with respect to conv1's raw output, gd the gradient with respect to the
 *               shortcut convolution's raw output
 *               All four are 16-byte aligned; the columns W .. pitch-1 and W0 .. pitch0-1 of a row are never read.
 *   d_weight    [32][96][3][3][3] f32 (co, ci, kt, kh, kw: nn.Conv3d's own order);  d_short [32][96];  d_short_bias [32]
 *   workspace   >= v2ce_convup_wgrad_workspace_bytes(...) for the same max_workgroups, 8-byte aligned; scratch, nothing
 *               is read before it is written
 * The virtual input is X[ci][b, l, h, w] = x0[ci][b, l, h >> 1, w >> 1] for ci < 64 and x1[ci - 64][b, l, h, w] for
 * 64 <= ci < 96 (the channel order of cat([upsample(x), skip])):
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
 * B, L, H, W >= 1, pitch >= W, pitch0 >= (W + 1) / 2, B * L * H * W < 2^31, B * L * H * pitch < 2^34 and B * L * H0 * pitch0
 * < 2^34, max_workgroups >= 0, else V2CE_ERR_BAD_ARG, as for a NULL needed input or workspace and a misaligned x0, x1, g1,
 * gd (16 bytes) or workspace (8 bytes); the size query returns 0 for arguments the entry refuses.  A small workspace is
 * V2CE_ERR_WORKSPACE and nothing is written.  Outputs must not overlap inputs or each other.
 *
 * Precision contract.  The products and the inner accumulation of d_weight and d_short run on v_mfma_f32_32x32x2_f32, bit
 * for bit an f32 fmaf chain over the positions.  One f32 accumulator sums at most V2CE_UPWGRAD_CHAIN positions; it is then
 * added into an f64 sum and starts again from zero.  Everything above that level is f64: the per-workgroup f64 partial sums
 * in the workspace and the finish kernel that adds them in a fixed order.  d_short_bias is f64 throughout.  There is one
 * rounding to f32, at the store.  So for an element of d_weight or d_short whose terms have the absolute sum S over N
 * positions
 *     |out - exact| <= ulp32(exact) + V2CE_UPWGRAD_CHAIN * 2^-24 * S + N * 2^-52 * S
 * and d_short_bias is within one rounding.  There are no atomics: the bytes are identical from run to run for the same
 * max_workgroups; they do not depend on the base pointers nor on which other outputs were asked for.
 *
 * max_workgroups: the grid is three workgroups -- one per 32-channel group of X -- for every share of the tiles of 2 x 64
 * positions.  0 = the kernel's own choice (one share per tile, at most 85 shares); n > 0 caps the grid at max(n, 3)
 * workgroups, that is at max(n / 3, 1) shares.  The result depends on n only through the order of the f64 sums: which tiles
 * share a workgroup's f32 chain and in which order the partial sums are added. */
#ifndef V2CE_HIP_CONVUPGRAD_H
#define V2CE_HIP_CONVUPGRAD_H

#include "v2ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define V2CE_UPWGRAD_CHAIN 4096

size_t v2ce_convup_wgrad_workspace_bytes(int B, int L, int H, int W, int pitch, int pitch0, int max_workgroups);
int v2ce_convup_wgrad(const float *x0, const float *x1, const float *g1, const float *gd, int B, int L, int H, int W, int pitch,
                      int pitch0, float *d_weight, float *d_short, float *d_short_bias, void *workspace, size_t workspace_bytes,
                      int max_workgroups, v2ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2CE_HIP_CONVUPGRAD_H */
