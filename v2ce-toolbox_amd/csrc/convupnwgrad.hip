// convupnwgrad.hip -- the weight gradients of a decoder block's first half on gfx950 at any of the decoders' channel counts:
// the 3x3x3 Conv3d(c0 + c1, cout) conv1 and the 1x1x1 Conv3d(c0 + c1, cout) shortcut, both on the virtual tensor
// X = cat(nearest_upsample_2x(x0, c0 channels), x1, c1 channels) (include/v2ce_hip_convupngrad.h and, for the 64 + 32 -> 32
// entry v2ce_convup_wgrad, include/v2ce_hip_convupgrad.h state the formulas, the tensors and the precision contract).
// UNet.decoders[3] is 64 + 32 -> 32, UNet.decoders[2] 128 + 64 -> 64.
//
// The tile is convnwgrad.hip's, run once per pair of a 32-channel group of the outputs and a 32-channel group of X: d_weight
// is (cout / 32) x ((c0 + c1) / 32) blocks of a 32 x 864 GEMM and d_short as many 32 x 32 GEMMs whose K runs over every
// output position; v_mfma_f32_32x32x2_f32 takes two positions per instruction: lane l holds A[co = l & 31][k = l >> 5] and
// B[k = l >> 5][ci = l & 31], so with both operands staged in LDS as [position][32 channels] a wave's A operand of the position
// pair (p, p + 1) is the 64 consecutive floats at p * 32 and its B operand the 64 consecutive floats at (halo position of p
// shifted by the tap) * 32: one conflict-free ds_read_b32 each.
//
// The grid is pairs x shares: workgroup s * pairs + p walks share s of the tiles for pair p = cog * gx + xg, the output
// channels 32 cog .. + 31 (planes 2 cog, 2 cog + 1 of g1 and gd) against group xg of X (xg < c0 / 32: channels 32 xg .. of x0,
// read at (h >> 1, w >> 1); the others: channels 32 (xg - c0 / 32) .. of x1); 64 + 32 -> 32 has three pairs, all of cog = 0.
// A tile is 2 rows x 64 columns of one frame (kTile = 128 positions, convgrad_dev.h).  Per tile the workgroup stages
//   sG  g1 of the tile and its co group, [128][32] f32 (16 KB); positions outside the tensor hold zeros
//   sD  gd of the tile, the same
//   sX  the halo of its group of X, 3 frames x 4 rows x 66 columns, [792][32] f32 (99 KB); positions outside the frame, the
//       sequence or the row's W columns hold zeros -- the zero padding of the UPSAMPLED tensor: a halo position is in range
//       by its own (l, h, w), and an upsampled group then reads x0 at (h >> 1, w >> 1)
// and wave v takes the units 7 v .. 7 v + 6 of 28: unit u < 27 is tap u of d_weight (A from sG), unit 27 -- the last wave's
// seventh -- is d_short: A from sD, B at the centre tap's halo offset, so the staged halo serves both layers.  Per position
// pair two reads for A and one read of sX per unit feed one MFMA per unit, 7 x 16 accumulator registers per lane.  A
// workgroup stages 32 channels of every tensor at a time, whatever the channel counts are.
//
// Chain and flush: an f32 accumulator takes kChainTiles = V2CE_UPWGRAD_CHAIN / 128 tiles; then (and after the last tile) the
// lane that owns it adds it into the workgroup's f64 partial in the workspace (the first flush stores) and clears it.  A
// partial element has one owner for the whole kernel, so no atomics.  d_short_bias (the pairs with xg = 0 only): thread t
// sums channel t & 31 over the 16 positions (t >> 5) * 16 .. + 15 of sD in f64, tile after tile; the eight sums of a channel
// meet at the end in a fixed order.  finish_kernel: one thread per output adds its pair's partials in the order of the shares
// 0 .. shares - 1 and rounds once.  A unit's arithmetic does not depend on which other units run: an output's bytes do not
// depend on which others were asked for.
#include "convgrad_dev.h"

#include "../../include/v2ce_hip_convupngrad.h"

namespace v2ce {
namespace {

constexpr int kUnits = kTaps + 1;                   // 27 taps of d_weight and d_short
constexpr int kUnitsPerWave = 7;
constexpr int kCentre = ((1 * kHaloH + 1) * kHaloW + 1) * kC;   // float offset of the tap (1, 1, 1) inside sX
constexpr int kChainTiles = V2CE_UPWGRAD_CHAIN / kTile;
constexpr int kPartial = kUnits * kC * kC + kC;     // f64 per workgroup: [28][32][32] unit blocks, [32] d_short_bias (xg = 0)
constexpr size_t kLds = (size_t)(2 * kTile + kHalo) * kC * sizeof(float);       // 131 KB
static_assert(kUnits == 4 * kUnitsPerWave, "every wave owns seven units");
static_assert(kChainTiles >= 1 && kChainTiles * kTile <= V2CE_UPWGRAD_CHAIN && V2CE_UPWGRAD_CHAIN <= 4096, "chain length");
static_assert(kLds <= 160 * 1024, "LDS of one workgroup");

struct Dims : Extent {
    int c0, c1, cout, g0, gx, pairs;                // g0: groups of 32 channels of x0; gx: of X; pairs = (cout / 32) gx
    int shares;
    size_t total;
};

// c16_at in the source x0 of the upsampled channels, (h, w) at the output resolution
__device__ __forceinline__ long long up_at(const Dims &D, int planes, long long f, int g, int h, int w) {
    return ((((f * planes + g) * D.H0 + (h >> 1)) * D.pitch0) + (w >> 1)) * 16;
}

__global__ __launch_bounds__(kThreads) void upnwgrad_kernel(const float *__restrict__ x0, const float *__restrict__ x1,
                                                            const float *__restrict__ g1, const float *__restrict__ gd, Dims D,
                                                            int doW, int doS, int doB, double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sG = smem, *sD = smem + kTile * kC, *sX = smem + 2 * kTile * kC;
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(t / kWave);
    const int pair = (int)(blockIdx.x % D.pairs), cog = pair / D.gx, xg = pair % D.gx;
    const long long share = blockIdx.x / D.pairs;
    const long long t0 = share * D.tiles / D.shares, t1 = (share + 1) * D.tiles / D.shares;
    double *mine = partial + (size_t)blockIdx.x * kPartial;
    doB = doB && xg == 0;
    const bool doX = doW || doS;
    if (!doX && !doB) return;                        // (uniform) d_short_bias alone: the other pairs have nothing to add
    const int gplanes = D.cout / 16, planes0 = D.c0 / 16, planes1 = D.c1 / 16;
    const bool from_up = xg < D.g0;
    const int xplane = from_up ? xg * 2 : (xg - D.g0) * 2;      // the group's first plane in x0 or x1
    // wave 3's seventh unit is the shortcut: its A operand comes from sD
    const bool short_wave = wv == kUnits / kUnitsPerWave - 1;
    const int nw = doW ? (short_wave ? kUnitsPerWave - 1 : kUnitsPerWave) : 0;     // this wave's units of d_weight: 0 .. nw - 1
    const bool has_short = short_wave && doS;

    f32x16 acc[kUnitsPerWave];
#pragma unroll
    for (int j = 0; j < kUnitsPerWave; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    int tapoff[kUnitsPerWave];                      // float offset of the unit's shift inside sX
#pragma unroll
    for (int j = 0; j < kUnitsPerWave; ++j) {
        const int tap = wv * kUnitsPerWave + j, kt = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        tapoff[j] = tap < kTaps ? ((kt * kHaloH + kh) * kHaloW + kw) * kC : kCentre;
    }
    double bsum = 0.0;
    int chain = 0;
    bool stored = false;

    for (long long tile = t0; tile < t1; ++tile) {
        const TileAt ta = tile_at(D, tile);
        const long long f = ta.f;
        const int l = ta.l, h0 = ta.h0, w0 = ta.w0;

        __syncthreads();                             // the previous tile has been read
        if (doW) stage_tile(D, g1, nullptr, sG, gplanes, cog * 2, f, h0, w0, t);
        if (doS || doB) stage_tile(D, gd, nullptr, sD, gplanes, cog * 2, f, h0, w0, t);
        if (doX) {
            // the halo of this group of X: 792 positions x 8 pieces
#pragma unroll 5
            for (int i = t; i < kHalo * 8; i += kThreads) {
                const int piece = i & 3, rest = i >> 2, g = rest / kHalo, hp = rest % kHalo;
                const int dt = hp / (kHaloH * kHaloW), rem = hp % (kHaloH * kHaloW);
                const int ll = l + dt - 1, h = h0 + rem / kHaloW - 1, w = w0 + rem % kHaloW - 1;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (ll >= 0 && ll < D.L && h >= 0 && h < D.H && w >= 0 && w < D.W) {
                    const float *at = from_up ? x0 + up_at(D, planes0, f + dt - 1, xplane + g, h, w)
                                              : x1 + c16_at(D, planes1, f + dt - 1, xplane + g, h, w);
                    v = *reinterpret_cast<const float4 *>(at + piece * 4);
                }
                *reinterpret_cast<float4 *>(sX + hp * kC + g * 16 + piece * 4) = v;
            }
        }
        __syncthreads();

        if (nw > 0 || has_short) {
#pragma unroll
            for (int row = 0; row < kTileH; ++row) {
                const float *ag = sG + row * kTileW * kC + lane;
                const float *ad = sD + row * kTileW * kC + lane;
                const float *bx = sX + row * kHaloW * kC + lane;
#pragma unroll 2
                for (int c = 0; c < kTileW; c += 2) {
                    const float a = nw > 0 ? ag[c * kC] : 0.0f;
#pragma unroll
                    for (int j = 0; j < kUnitsPerWave - 1; ++j) {
                        if (j < nw) {
                            const float b = bx[c * kC + tapoff[j]];
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
                        }
                    }
                    if (short_wave ? has_short : nw > 0) {
                        const float a6 = short_wave ? ad[c * kC] : a;
                        const float b = bx[c * kC + tapoff[kUnitsPerWave - 1]];
                        acc[kUnitsPerWave - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a6, b, acc[kUnitsPerWave - 1], 0, 0, 0);
                    }
                }
            }
        }
        if (doB) add_channel_part(sD, t, bsum);

        if (doX && (++chain == kChainTiles || tile + 1 == t1)) {
            // C/D map of the 32x32 MFMA: column (ci) = lane & 31, row (co) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
            for (int j = 0; j < kUnitsPerWave; ++j) {
                const bool active = j < kUnitsPerWave - 1 ? j < nw : (short_wave ? has_short : nw > 0);
                if (active) {
                    double *blk = mine + (size_t)(wv * kUnitsPerWave + j) * (kC * kC);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int co = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        double *e = blk + co * kC + (lane & 31);
                        *e = stored ? *e + (double)acc[j][r] : (double)acc[j][r];
                        acc[j][r] = 0.0f;
                    }
                }
            }
            stored = true;
            chain = 0;
        }
    }

    if (doB) reduce_channel_parts(reinterpret_cast<double *>(smem), t, bsum, mine + kUnits * kC * kC);
}

// one thread per output: e < pairs * 28 * 1024 is (pair, unit, co, ci) of d_weight (unit < 27) or d_short, the others
// d_short_bias, read from the pair (cog, xg = 0)
__global__ __launch_bounds__(kThreads) void upnwgrad_finish_kernel(const double *__restrict__ partial, Dims D, int doW, int doS,
                                                                   int doB, float *__restrict__ d_weight, float *__restrict__ d_short,
                                                                   float *__restrict__ d_short_bias) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    const int nu = D.pairs * kUnits * kC * kC;
    if (e >= nu + D.cout) return;
    if (e >= nu) {
        if (!doB) return;
        const int co = e - nu, pair = (co / kC) * D.gx;
        double s = 0.0;
        for (int sh = 0; sh < D.shares; ++sh) s += partial[((size_t)sh * D.pairs + pair) * kPartial + kUnits * kC * kC + co % kC];
        d_short_bias[co] = (float)s;
        return;
    }
    const int pair = e / (kUnits * kC * kC), in = e % (kUnits * kC * kC);
    const int unit = in / (kC * kC), co = (pair / D.gx) * kC + (in / kC) % kC, ci = (pair % D.gx) * kC + in % kC;
    if (unit < kTaps ? !doW : !doS) return;
    double s = 0.0;
    for (int sh = 0; sh < D.shares; ++sh) s += partial[((size_t)sh * D.pairs + pair) * kPartial + in];
    if (unit < kTaps)
        d_weight[((size_t)co * (D.gx * kC) + ci) * kTaps + unit] = (float)s;
    else
        d_short[(size_t)co * (D.gx * kC) + ci] = (float)s;
}

bool make_dims(int c0, int c1, int cout, int B, int L, int H, int W, int pitch, int pitch0, int max_workgroups, Dims &D) {
    if ((c0 != 64 && c0 != 128) || (c1 != 32 && c1 != 64) || (cout != 32 && cout != 64)) return false;
    if (!make_extent(B, L, H, W, pitch, true, pitch0, max_workgroups, D)) return false;
    D.c0 = c0; D.c1 = c1; D.cout = cout; D.g0 = c0 / kC; D.gx = (c0 + c1) / kC; D.pairs = (cout / kC) * D.gx;
    D.shares = plan_shares(D.tiles, D.pairs, max_workgroups);
    D.total = round256((size_t)D.shares * D.pairs * kPartial * sizeof(double));
    return true;
}

const char *kNeeds = "needs c0 in {64, 128}, c1 and cout in {32, 64}, B, L, H, W >= 1, pitch >= W, pitch0 >= (W + 1) / 2, "
                     "max_workgroups >= 0, B L H W < 2^31, B L H pitch < 2^34 and B L H0 pitch0 < 2^34";

// `entry`: the symbol the caller used; it leads every message
int upnwgrad(const char *entry, const float *x0, const float *x1, const float *g1, const float *gd, int c0, int c1, int cout, int B,
             int L, int H, int W, int pitch, int pitch0, float *d_weight, float *d_short, float *d_short_bias, void *workspace,
             size_t workspace_bytes, int max_workgroups, v2ce_stream_t stream) {
    clear_error();
    Dims D;
    V2CE_REQUIRE(make_dims(c0, c1, cout, B, L, H, W, pitch, pitch0, max_workgroups, D), V2CE_ERR_BAD_ARG,
                 "%s: c0 %d c1 %d cout %d B %d L %d H %d W %d pitch %d pitch0 %d max_workgroups %d: %s", entry, c0, c1, cout, B, L, H,
                 W, pitch, pitch0, max_workgroups, kNeeds);
    V2CE_REQUIRE(d_weight || d_short || d_short_bias, V2CE_ERR_BAD_ARG,
                 "%s: no output requested (d_weight, d_short and d_short_bias are all null)", entry);
    const int doW = d_weight != nullptr, doS = d_short != nullptr, doB = d_short_bias != nullptr;
    V2CE_REQUIRE(workspace && (!(doW || doS) || (x0 && x1)) && (!doW || g1) && (!(doS || doB) || gd), V2CE_ERR_BAD_ARG,
                 "%s: null pointer (d_weight needs x0, x1 and g1; d_short x0, x1 and gd; d_short_bias gd)", entry);
    V2CE_REQUIRE(aligned16(x0, x1, g1, gd), V2CE_ERR_BAD_ARG, "%s: x0, x1, g1 and gd must be 16-byte aligned", entry);
    if (const int rc = check_workspace(entry, workspace, workspace_bytes, D.total)) return rc;
    hipStream_t st = as_stream(stream);
    double *partial = static_cast<double *>(workspace);
    const int outputs = D.pairs * kUnits * kC * kC + D.cout;
    V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(upnwgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kLds));
    hipLaunchKernelGGL(upnwgrad_kernel, dim3((unsigned)(D.shares * D.pairs)), dim3(kThreads), kLds, st, x0, x1, g1, gd, D, doW, doS,
                       doB, partial);
    hipLaunchKernelGGL(upnwgrad_finish_kernel, dim3((outputs + kThreads - 1) / kThreads), dim3(kThreads), 0, st, partial, D, doW,
                       doS, doB, d_weight, d_short, d_short_bias);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_convupn_wgrad_workspace_bytes(int c0, int c1, int cout, int B, int L, int H, int W, int pitch, int pitch0,
                                                     int max_workgroups) {
    Dims D;
    return make_dims(c0, c1, cout, B, L, H, W, pitch, pitch0, max_workgroups, D) ? D.total : 0;
}

extern "C" int v2ce_convupn_wgrad(const float *x0, const float *x1, const float *g1, const float *gd, int c0, int c1, int cout, int B,
                                  int L, int H, int W, int pitch, int pitch0, float *d_weight, float *d_short, float *d_short_bias,
                                  void *workspace, size_t workspace_bytes, int max_workgroups, v2ce_stream_t stream) {
    return upnwgrad("v2ce_convupn_wgrad", x0, x1, g1, gd, c0, c1, cout, B, L, H, W, pitch, pitch0, d_weight, d_short, d_short_bias,
                    workspace, workspace_bytes, max_workgroups, stream);
}

// the 64 + 32 -> 32 entries of include/v2ce_hip_convupgrad.h: three pairs, 85 shares at the most
extern "C" size_t v2ce_convup_wgrad_workspace_bytes(int B, int L, int H, int W, int pitch, int pitch0, int max_workgroups) {
    return v2ce_convupn_wgrad_workspace_bytes(64, 32, 32, B, L, H, W, pitch, pitch0, max_workgroups);
}

extern "C" int v2ce_convup_wgrad(const float *x0, const float *x1, const float *g1, const float *gd, int B, int L, int H, int W,
                                 int pitch, int pitch0, float *d_weight, float *d_short, float *d_short_bias, void *workspace,
                                 size_t workspace_bytes, int max_workgroups, v2ce_stream_t stream) {
    return upnwgrad("v2ce_convup_wgrad", x0, x1, g1, gd, 64, 32, 32, B, L, H, W, pitch, pitch0, d_weight, d_short, d_short_bias,
                    workspace, workspace_bytes, max_workgroups, stream);
}
