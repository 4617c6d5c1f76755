// convupdgrad.hip -- the input gradients of a decoder block's first half on gfx950: of the 3x3x3 Conv3d(c0 + c1, cout) conv1
// and of the 1x1x1 Conv3d(c0 + c1, cout) shortcut with respect to the block's two sources, back through the concat and the 2x
// nearest upsample that the forward never materialises (include/v2ce_hip_convupndgrad.h and, for the 64 + 32 -> 32 entry
// v2ce_convup_dgrad, include/v2ce_hip_convupdgrad.h state the formulas, the tensors and the precision contract).
// UNet.decoders[3] is the 64 + 32 -> 32 case, UNet.decoders[2] the 128 + 64 -> 64 case.
//
// The tile is convndgrad.hip's, once per 32-channel group of X = cat(upsample(x0), x1).  d_X of a group is a GEMM with the
// positions as M, the group's 32 input channels as N and (co group, unit, co) as K = 28 cout: unit u < 27 is tap u of conv1
// on g1,
//   D[pos][ci] += sum_co g1[co][pos - tap + 1] W[co][ci][tap],
// and unit 27 the shortcut on gd at the position itself.  v_mfma_f32_32x32x2_f32 takes two output channels per instruction:
// lane l holds A[pos = l & 31][k = l >> 5] and B[k = l >> 5][ci = l & 31].  A workgroup stages 32 output channels at a time,
// whatever cout is, so the tile, the halo, the LDS and the bank arguments do not depend on the channel counts:
//   B  the weights, [group][unit][co][ci] after the prep kernel: wave v keeps those of the units 7 v .. 7 v + 6 (the shortcut
//      is the last wave's seventh) and of EVERY co group in registers for the whole kernel: 7 x 16 registers per lane and co
//      group, 224 at cout = 64.  With the 64 accumulator registers that is under the 512 a wave may hold at four waves per
//      workgroup (one workgroup per CU: the LDS decides the occupancy anyway)
//   A  sH, the halo of g1 of ONE co group in LDS, channel-major: 3 frames x 4 rows x 66 columns = 792 positions at a plane
//      stride of 800 floats, and sD, gd of the tile and the same co group, channel-major at a plane stride of 160 floats.
//      Both strides are 32 mod 64: the 32 lanes of a half read 32 consecutive columns of one row of one channel plane, the
//      other half the next plane, 32 banks further: one conflict-free ds_read_b32 per MFMA
//
// The grid is groups x shares: workgroup G s + c walks share s of the tiles for the c-th requested group (the groups 0 ..
// c0 / 32 - 1: the channels 32 c .. of x0, asked for through d_x0; the c1 / 32 groups behind them: x1, through d_x1).  A tile
// is 2 rows x 64 columns of one frame and starts at an even row and an even column, so every 2 x 2 pool of the upsample lies
// inside one tile: one workgroup produces a d_x0 element whole, with no atomics, whatever the grid.  Per tile the workgroup
//   1. for co group 0, then co group 1 (cout = 64): stages the group's halo of g1 (zeros outside the frame, the sequence and
//      the row's W columns: the convolution's zero padding) and its tile of gd, and runs its units into the SAME
//      accumulators: 4 independent MFMA chains (the tile's four groups of 32 positions) per wave, 7 x 16 steps each per
//      group.  With the first group it zero-fills the padding columns of its output rows when the tile is the last one of
//      its rows;
//   2. writes the four partial tiles over the halo (sP[wave][position][ci]) and adds them in the order of the waves,
//      ((p0 + p1) + p2) + p3, per position: an x1 group stores that as d_x1; an x0 group adds the up to four positions of a
//      source pixel in the order (0, 0), (0, 1), (1, 0), (1, 1) -- leaving out those at h >= H or w >= W, which are no output
//      positions although their convolution sums are not zero -- and stores 32 source columns of one source row.
// An element's order of summation is fixed by cout, the unit split and the pool order alone: it depends neither on the grid
// nor on the tile walk nor on which other output was asked for.  At cout = 32 there is one co group: a tile is staged once.
#include "convgrad_dev.h"

#include "../../include/v2ce_hip_convupdgrad.h"
#include "../../include/v2ce_hip_convupndgrad.h"

namespace v2ce {
namespace {

constexpr int kUnits = kTaps + 1;                   // the 27 taps of conv1 and the shortcut
constexpr int kUnitsPerWave = 7;
constexpr int kSteps = kC / 2;                      // k-steps of a unit and co group: two output channels per MFMA
constexpr int kMGroups = kTile / 32;                // M groups of a tile: (row, half of the columns)
constexpr int kPlaneD = 160;                        // floats between the channel planes of sD
constexpr int kPos = 36;                            // floats between the positions of a partial tile (32 channels + 4: 16-byte rows)
constexpr size_t kLds = (size_t)kC * (kPlane + kPlaneD) * sizeof(float);        // 120 KB
static_assert(kPlaneD >= kTile && kPlaneD % 64 == 32, "plane stride of the gd tile");
static_assert((size_t)4 * kTile * kPos <= (size_t)kC * kPlane && kPos % 4 == 0, "the partial tiles lie over the halo");
static_assert(kLds <= 160 * 1024, "LDS of one workgroup");
static_assert(V2CE_UPDGRAD_TERMS == kUnits * kC && V2CE_UPNDGRAD_TERMS(64) == kUnits * 64, "terms of an element of d_X");
static_assert(kUnits == 4 * kUnitsPerWave, "every wave owns seven units");
static_assert(kTileH == 2 && kTileW % 2 == 0 && kTileW / 2 * kC / 4 == kThreads, "one thread per four channels of a source pixel");

struct Dims : Extent {
    int c0, c1, cout, g0;                           // g0: groups of 32 channels of x0; those of x1 follow them
    size_t total;
};

// c16_at in d_x0 with its c0 / 16 planes, (h0, w0) at the source resolution
__device__ __forceinline__ long long src_at(const Dims &D, long long f, int g, int h0, int w0) {
    return ((((f * (D.c0 / 16) + g) * D.H0 + h0) * D.pitch0) + w0) * 16;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ((p0 + p1) + p2) + p3 of four channels of a position
__device__ __forceinline__ float4 wave_sum(const float *src) {
    float4 s = *reinterpret_cast<const float4 *>(src);
#pragma unroll
    for (int v = 1; v < 4; ++v) s = add4(s, *reinterpret_cast<const float4 *>(src + v * kTile * kPos));
    return s;
}

// [co][cin][27] and [co][cin] -> [group][unit][co][ci]: what a lane of the main kernel loads as consecutive floats
__global__ __launch_bounds__(kThreads) void updgrad_prep_kernel(const float *__restrict__ weight, const float *__restrict__ short_weight,
                                                                int cin, int cout, float *__restrict__ wt) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= kUnits * cout * cin) return;
    const int ci = e % kC, co = (e / kC) % cout, unit = (e / (kC * cout)) % kUnits, grp = e / (kUnits * cout * kC);
    const int at = co * cin + grp * kC + ci;
    if (unit < kTaps) {
        if (weight) wt[e] = weight[at * kTaps + unit];
    } else if (short_weight) {
        wt[e] = short_weight[at];
    }
}

// kCog: co groups of 32 output channels (cout / 32)
template <int kCog>
__global__ __launch_bounds__(kThreads) void updgrad_kernel(const float *__restrict__ wt, const float *__restrict__ g1,
                                                           const float *__restrict__ gd, Dims D, int grp0, int ngrp,
                                                           float *__restrict__ d_x0, float *__restrict__ d_x1) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sH = smem, *sD = smem + kC * kPlane, *sP = smem;     // the partial tiles lie over the halo once it has been read
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(t / kWave);
    const int grp = grp0 + (int)(blockIdx.x % ngrp);
    const long long share = blockIdx.x / ngrp, shares = gridDim.x / ngrp;
    const long long t0 = share * D.tiles / shares, t1 = (share + 1) * D.tiles / shares;
    const bool doC = g1 != nullptr, doS = gd != nullptr;
    const bool short_wave = wv == kUnits / kUnitsPerWave - 1;
    const bool is_x1 = grp >= D.g0;                  // (uniform)
    const int mplanes = D.cout / 16, x1planes = D.c1 / 16, xg = is_x1 ? grp - D.g0 : grp;
    // this workgroup's two planes of its output: plane 2 xg of d_x1 or of d_x0 is plane 0 of `dst`
    float *const dst = is_x1 ? d_x1 + (long long)xg * 2 * D.H * D.pitch * 16 : d_x0 + (long long)xg * 2 * D.H0 * D.pitch0 * 16;

    // B operands of this wave's units: step s of unit u and co group cg is W[co = 32 cg + 2 s + (lane >> 5)][ci = 32 grp +
    // (lane & 31)][u]
    float wreg[kCog][kUnitsPerWave][kSteps];
    int tapoff[kUnitsPerWave];                      // the tap's shift inside a plane of sH: g1 at pos - tap + 1
#pragma unroll
    for (int j = 0; j < kUnitsPerWave; ++j) {
        const int unit = wv * kUnitsPerWave + j, kt = unit / 9, kh = (unit / 3) % 3, kw = unit % 3;
        const bool live = unit < kTaps ? doC : doS;
        tapoff[j] = unit < kTaps ? ((2 - kt) * kHaloH + (2 - kh)) * kHaloW + (2 - kw) : 0;
#pragma unroll
        for (int cg = 0; cg < kCog; ++cg)
#pragma unroll
            for (int s = 0; s < kSteps; ++s)
                wreg[cg][j][s] = live ? wt[((size_t)(grp * kUnits + unit) * D.cout + cg * kC + 2 * s + (lane >> 5)) * kC + (lane & 31)]
                                      : 0.0f;
    }

    for (long long tile = t0; tile < t1; ++tile) {
        const TileAt ta = tile_at(D, tile);
        const long long f = ta.f;
        const int l = ta.l, h0 = ta.h0, w0 = ta.w0, tw = ta.tw;

        f32x16 acc[kMGroups];
#pragma unroll
        for (int gq = 0; gq < kMGroups; ++gq)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[gq][r] = 0.0f;

#pragma unroll
        for (int cg = 0; cg < kCog; ++cg) {
            __syncthreads();                         // the previous tile's partials / the previous group's halo have been read
            // the group's two planes lie 2 cg planes behind those of group 0: a uniform shift of the base pointers
            const long long cgoff = (long long)cg * 2 * D.H * D.pitch * 16;
            if (doC) {
                // the halo of g1: 2 planes x 792 positions, 64 bytes each; consecutive lanes take consecutive positions
                for (int i = t; i < 2 * kHalo; i += kThreads) {
                    const int g = i / kHalo, hp = i % kHalo;
                    const int dt = hp / (kHaloH * kHaloW), rem = hp % (kHaloH * kHaloW), hh = rem / kHaloW, ww = rem % kHaloW;
                    const int ll = l + dt - 1, h = h0 + hh - 1, w = w0 + ww - 1;
                    float4 v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (ll >= 0 && ll < D.L && h >= 0 && h < D.H && w >= 0 && w < D.W) {
                        const long long at = c16_at(D, mplanes, f + dt - 1, g, h, w);
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float4 *>(g1 + cgoff + at + q * 4);
                    }
                    float *dst = sH + (g * 16) * kPlane + hp;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        dst[(q * 4 + 0) * kPlane] = v[q].x; dst[(q * 4 + 1) * kPlane] = v[q].y;
                        dst[(q * 4 + 2) * kPlane] = v[q].z; dst[(q * 4 + 3) * kPlane] = v[q].w;
                    }
                }
            }
            if (doS) {
                // gd of the tile: 2 planes x 128 positions, one per thread
                const int g = t / kTile, p = t % kTile;
                const int h = h0 + p / kTileW, w = w0 + p % kTileW;
                float4 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (h < D.H && w < D.W) {
                    const long long at = c16_at(D, mplanes, f, g, h, w);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float4 *>(gd + cgoff + at + q * 4);
                }
                float *dst = sD + (g * 16) * kPlaneD + p;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    dst[(q * 4 + 0) * kPlaneD] = v[q].x; dst[(q * 4 + 1) * kPlaneD] = v[q].y;
                    dst[(q * 4 + 2) * kPlaneD] = v[q].z; dst[(q * 4 + 3) * kPlaneD] = v[q].w;
                }
            }
            __syncthreads();

            // group gq = (row gq >> 1, columns 32 (gq & 1) ..): lane's position inside a plane before the tap's shift
            const float *a0 = sH + (lane >> 5) * kPlane + (lane & 31);
            const float *d0 = sD + (lane >> 5) * kPlaneD + (lane & 31);
#pragma unroll
            for (int j = 0; j < kUnitsPerWave; ++j) {
                if (j == kUnitsPerWave - 1 && short_wave) {
                    if (doS) {
#pragma unroll
                        for (int s = 0; s < kSteps; ++s) {
#pragma unroll
                            for (int gq = 0; gq < kMGroups; ++gq) {
                                const float a = d0[2 * s * kPlaneD + gq * 32];
                                acc[gq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wreg[cg][j][s], acc[gq], 0, 0, 0);
                            }
                        }
                    }
                } else if (doC) {
                    const float *aj = a0 + tapoff[j];
#pragma unroll
                    for (int s = 0; s < kSteps; ++s) {
#pragma unroll
                        for (int gq = 0; gq < kMGroups; ++gq) {
                            const float a = aj[2 * s * kPlane + (gq >> 1) * kHaloW + (gq & 1) * 32];
                            acc[gq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wreg[cg][j][s], acc[gq], 0, 0, 0);
                        }
                    }
                }
            }
        }
        __syncthreads();                             // every wave has read the halo

        // C/D map of the 32x32 MFMA: column (ci) = lane & 31, row (position) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int gq = 0; gq < kMGroups; ++gq) {
            float *blk = sP + ((size_t)wv * kTile + gq * 32) * kPos + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) blk[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * kPos] = acc[gq][r];
        }
        __syncthreads();

        // the stores' per-thread address arithmetic is redone per tile: hoisted out of the tile walk it would sit in registers the
        // weights need
        int te = t;
        asm volatile("" : "+v"(te));
        if (tw == D.tiles_w - 1) {
            // the padding columns of the tile's output rows, this workgroup's two planes: a thread keeps its (row, plane,
            // piece of 16 bytes) and walks the columns
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const int piece = te & 3, g = (te >> 2) & 1;
            if (is_x1) {
                const int h = h0 + ((te >> 3) & 1);
                if (h < D.H)
                    for (int col = D.W + (te >> 4); col < D.pitch; col += kThreads / 16)
                        *reinterpret_cast<float4 *>(dst + c16_at(D, x1planes, f, g, h, col) + piece * 4) = zero;
            } else {
                for (int col = D.W0 + (te >> 3); col < D.pitch0; col += kThreads / 8)
                    *reinterpret_cast<float4 *>(dst + src_at(D, f, g, h0 >> 1, col) + piece * 4) = zero;
            }
        }
        if (is_x1) {
            // position p = row * 64 + column of the tile; 8 pieces of four channels each
#pragma unroll
            for (int k = 0; k < kTile * 8 / kThreads; ++k) {
                const int i = te + k * kThreads, piece = i & 3, rest = i >> 2, p = rest % kTile, g = rest / kTile;
                const int h = h0 + p / kTileW, w = w0 + p % kTileW;
                if (h < D.H && w < D.W)
                    *reinterpret_cast<float4 *>(dst + c16_at(D, x1planes, f, g, h, w) + piece * 4) =
                        wave_sum(sP + p * kPos + g * 16 + piece * 4);
            }
        } else {
            // source pixel (h0 / 2, w0 / 2 + col): its output positions are rows h0, h0 + 1 and columns w0 + 2 col, + 1
            const int piece = te & 3, col = (te >> 2) & 31, g = te >> 7;
            const int w = w0 + 2 * col;
            if (w < D.W) {
                const float *src = sP + 2 * col * kPos + g * 16 + piece * 4;
                const bool right = w + 1 < D.W, below = h0 + 1 < D.H;
                float4 s = wave_sum(src);
                if (right) s = add4(s, wave_sum(src + kPos));
                if (below) s = add4(s, wave_sum(src + kTileW * kPos));
                if (below && right) s = add4(s, wave_sum(src + (kTileW + 1) * kPos));
                *reinterpret_cast<float4 *>(dst + src_at(D, f, g, h0 >> 1, (w0 >> 1) + col) + piece * 4) = s;
            }
        }
    }
}

bool make_dims(int c0, int c1, int cout, int B, int L, int H, int W, int pitch, int pitch0, int max_workgroups, Dims &D) {
    if ((c0 != 64 && c0 != 128) || (c1 != 32 && c1 != 64) || (cout != 32 && cout != 64)) return false;
    if (!make_extent(B, L, H, W, pitch, true, pitch0, max_workgroups, D)) return false;
    D.c0 = c0; D.c1 = c1; D.cout = cout; D.g0 = c0 / kC;
    D.total = round256((size_t)kUnits * cout * (c0 + c1) * sizeof(float));  // the repacked weights; the grid needs nothing
    return true;
}

const char *kNeeds = "needs c0 in {64, 128}, c1 and cout in {32, 64}, B, L, H, W >= 1, pitch >= W, pitch0 >= (W + 1) / 2, "
                     "max_workgroups >= 0, B L H W < 2^31, B L H pitch < 2^34 and B L H0 pitch0 < 2^34";

// `entry`: the symbol the caller used; it leads every message
int updgrad(const char *entry, const float *weight, const float *short_weight, const float *g1, const float *gd, int c0, int c1,
            int cout, int B, int L, int H, int W, int pitch, int pitch0, float *d_x0, float *d_x1, void *workspace,
            size_t workspace_bytes, int max_workgroups, v2ce_stream_t stream) {
    clear_error();
    Dims D;
    V2CE_REQUIRE(make_dims(c0, c1, cout, B, L, H, W, pitch, pitch0, max_workgroups, D), V2CE_ERR_BAD_ARG,
                 "%s: c0 %d c1 %d cout %d B %d L %d H %d W %d pitch %d pitch0 %d max_workgroups %d: %s", entry, c0, c1, cout, B, L, H,
                 W, pitch, pitch0, max_workgroups, kNeeds);
    V2CE_REQUIRE(d_x0 || d_x1, V2CE_ERR_BAD_ARG, "%s: no output requested (d_x0 and d_x1 are both null)", entry);
    V2CE_REQUIRE(workspace && (g1 || gd) && (!g1 || weight) && (!gd || short_weight), V2CE_ERR_BAD_ARG,
                 "%s: null pointer (g1 and gd are both null, g1 without weight, gd without short_weight, or no workspace)", entry);
    V2CE_REQUIRE(aligned16(g1, gd, d_x0, d_x1), V2CE_ERR_BAD_ARG, "%s: g1, gd, d_x0 and d_x1 must be 16-byte aligned", entry);
    V2CE_REQUIRE(((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(short_weight)) & 3) == 0, V2CE_ERR_BAD_ARG,
                 "%s: weight and short_weight must be 4-byte aligned", entry);
    if (const int rc = check_workspace(entry, workspace, workspace_bytes, D.total)) return rc;
    // the requested 32-channel groups of X: those of x0 (d_x0) and those of x1 behind them (d_x1)
    const int grp0 = d_x0 ? 0 : D.g0, ngrp = (d_x0 ? D.g0 : 0) + (d_x1 ? c1 / kC : 0);
    const int shares = plan_shares(D.tiles, ngrp, max_workgroups);
    hipStream_t st = as_stream(stream);
    float *wt = static_cast<float *>(workspace);
    const auto kernel = cout == 64 ? updgrad_kernel<2> : updgrad_kernel<1>;
    const int weights = kUnits * cout * (c0 + c1);
    V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
    hipLaunchKernelGGL(updgrad_prep_kernel, dim3((weights + kThreads - 1) / kThreads), dim3(kThreads), 0, st, g1 ? weight : nullptr,
                       gd ? short_weight : nullptr, c0 + c1, cout, wt);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(shares * ngrp)), dim3(kThreads), kLds, st, wt, g1, gd, D, grp0, ngrp, d_x0, d_x1);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_convupn_dgrad_workspace_bytes(int c0, int c1, int cout, int B, int L, int H, int W, int pitch, int pitch0,
                                                     int max_workgroups) {
    Dims D;
    return make_dims(c0, c1, cout, B, L, H, W, pitch, pitch0, max_workgroups, D) ? D.total : 0;
}

extern "C" int v2ce_convupn_dgrad(const float *weight, const float *short_weight, const float *g1, const float *gd, int c0, int c1,
                                  int cout, int B, int L, int H, int W, int pitch, int pitch0, float *d_x0, float *d_x1,
                                  void *workspace, size_t workspace_bytes, int max_workgroups, v2ce_stream_t stream) {
    return updgrad("v2ce_convupn_dgrad", weight, short_weight, g1, gd, c0, c1, cout, B, L, H, W, pitch, pitch0, d_x0, d_x1, workspace,
                   workspace_bytes, max_workgroups, stream);
}

// the 64 + 32 -> 32 entries of include/v2ce_hip_convupdgrad.h: updgrad_kernel<1> with two groups of x0 and one of x1
extern "C" size_t v2ce_convup_dgrad_workspace_bytes(int B, int L, int H, int W, int pitch, int pitch0, int max_workgroups) {
    return v2ce_convupn_dgrad_workspace_bytes(64, 32, 32, B, L, H, W, pitch, pitch0, max_workgroups);
}

extern "C" int v2ce_convup_dgrad(const float *weight, const float *short_weight, const float *g1, const float *gd, int B, int L,
                                 int H, int W, int pitch, int pitch0, float *d_x0, float *d_x1, void *workspace,
                                 size_t workspace_bytes, int max_workgroups, v2ce_stream_t stream) {
    return updgrad("v2ce_convup_dgrad", weight, short_weight, g1, gd, 64, 32, 32, B, L, H, W, pitch, pitch0, d_x0, d_x1, workspace,
                   workspace_bytes, max_workgroups, stream);
}
