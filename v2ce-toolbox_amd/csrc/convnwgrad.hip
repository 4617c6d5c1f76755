// convnwgrad.hip -- the weight gradient of a 3x3x3 Conv3d(cin, cout) with 32, 64, 128, 256 or 512 channels on either side on
// gfx950, seen through the relu behind it (include/v2ce_hip_convcgrad.h; include/v2ce_hip_convngrad.h for the entry that
// stops at 64 channels, v2ce_convn_wgrad, and include/v2ce_hip_convgrad.h for the 32 -> 32 entry v2ce_conv32_wgrad state
// the formulas, the tensors and the precision contract).  UNet.decoders[3].conv2 is the 32 -> 32 case, UNet.decoders[2].conv2
// the 64 -> 64 case, UNet.decoders[1].conv2 the 128 -> 128 case.
//
// d_weight is (cout / 32) x (cin / 32) blocks of a 32 x 864 GEMM whose K runs over every output position, one block per pair
// of channel groups.  Per tap (kt, kh, kw) a 32 x 32 block D[co][ci] += sum_pos m[co][pos] x[ci][pos + tap].
// v_mfma_f32_32x32x2_f32 takes two positions per instruction: lane l holds A[co = l & 31][k = l >> 5] and B[k = l >> 5]
// [ci = l & 31], so with both operands staged in LDS as [position][32 channels] a wave's A operand of the position pair
// (p, p + 1) is the 64 consecutive floats at p * 32 and its B operand the 64 consecutive floats at (halo position of p
// shifted by the tap) * 32: one conflict-free ds_read_b32 each.
//
// The grid is pairs x shares: workgroup s * pairs + p walks share s of the tiles for pair p = cog * (cin / 32) + cig, the
// output channels 32 cog .. + 31 against the input channels 32 cig .. + 31; 32 -> 32 has one pair, and its grid is the
// shares.  A tile is 2 rows x 64 columns of one frame (kTile = 128 positions, convgrad_dev.h).  Per tile the workgroup stages
//   sM  m = y > 0 ? upstream : 0 of its 32 output channels, [128][32] f32 (16 KB); zeros outside the tensor
//   sX  the halo of its 32 input channels of x, 3 frames x 4 rows x 66 columns, [792][32] f32 (99 KB); zeros outside the
//       frame, the sequence or the row's W columns -- the convolution's zero padding
// and wave v takes the taps 7 v .. 7 v + 6 (the last wave six): per position pair one read of sM and one read of sX per tap
// feed one MFMA per tap, 7 x 16 accumulator registers per lane.  LDS traffic is 8 reads per 7 MFMAs of 64 cycles.  A
// workgroup stages 32 channels of either tensor at a time, whatever cin and cout are.
//
// Chain and flush: an f32 accumulator takes kChainTiles = V2CE_WGRAD_CHAIN / 128 tiles; then (and after the last tile) the
// lane that owns it adds it into the workgroup's f64 partial in the workspace (the first flush stores) and clears it.  A
// partial element has one owner for the whole kernel, so no atomics.  d_shift is taken by the pairs with cig = 0: thread t
// sums channel t & 31 over the 16 positions (t >> 5) * 16 .. + 15 of sM in f64, tile after tile; the eight sums of a
// channel meet at the end in a fixed order.  finish_kernel: one thread per output adds its pair's partials in the order of
// the shares 0 .. shares - 1 and rounds once.
#include "convgrad_dev.h"

#include "../../include/v2ce_hip_convcgrad.h"
#include "../../include/v2ce_hip_convngrad.h"

namespace v2ce {
namespace {

constexpr int kTapsPerWave = 7;
constexpr int kChainTiles = V2CE_WGRAD_CHAIN / kTile;
constexpr int kPartial = kTaps * kC * kC + kC;      // f64 per workgroup: [27][32][32] d_weight blocks, [32] d_shift
constexpr size_t kLds = (size_t)(kTile + kHalo) * kC * sizeof(float);   // 115 KB
static_assert(kChainTiles >= 1 && kChainTiles * kTile <= V2CE_WGRAD_CHAIN && V2CE_WGRAD_CHAIN <= 4096, "chain length");
static_assert(kLds <= 160 * 1024, "LDS of one workgroup");

struct Dims : Extent {
    int cin, cout, gi, go, pairs;                   // gi, go: groups of 32 input / output channels; pairs = gi go
    int shares;
    size_t total;
};

__global__ __launch_bounds__(kThreads) void nwgrad_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                          const float *__restrict__ up, Dims D, int doW, int wantB,
                                                          double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sM = smem, *sX = smem + kTile * kC;
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(t / kWave);
    const int pair = blockIdx.x % D.pairs, cog = pair / D.gi, cig = pair % D.gi;
    const long long share = blockIdx.x / D.pairs;
    const long long t0 = share * D.tiles / D.shares, t1 = (share + 1) * D.tiles / D.shares;
    const int doB = wantB && cig == 0;
    if (!doW && !doB) return;                        // (uniform) d_shift alone: the other pairs have nothing to add
    const int xplanes = D.cin / 16, mplanes = D.cout / 16;
    double *mine = partial + (size_t)blockIdx.x * kPartial;

    f32x16 acc[kTapsPerWave];
#pragma unroll
    for (int j = 0; j < kTapsPerWave; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    int tapoff[kTapsPerWave];                       // float offset of the tap's shift inside sX
#pragma unroll
    for (int j = 0; j < kTapsPerWave; ++j) {
        const int tap = wv * kTapsPerWave + j, kt = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        tapoff[j] = tap < kTaps ? ((kt * kHaloH + kh) * kHaloW + kw) * kC : 0;
    }
    const int ntaps = kTaps - wv * kTapsPerWave < kTapsPerWave ? kTaps - wv * kTapsPerWave : kTapsPerWave;
    double bsum = 0.0;
    int chain = 0;
    bool stored = false;

    for (long long tile = t0; tile < t1; ++tile) {
        const TileAt ta = tile_at(D, tile);
        const long long f = ta.f;
        const int l = ta.l, h0 = ta.h0, w0 = ta.w0;

        __syncthreads();                             // the previous tile has been read
        stage_tile(D, up, y, sM, mplanes, cog * 2, f, h0, w0, t);
        if (doW) {
            // the halo of x: 792 positions x 8 pieces
#pragma unroll 5
            for (int i = t; i < kHalo * 8; i += kThreads) {
                const int piece = i & 3, rest = i >> 2, g = rest / kHalo, hp = rest % kHalo;
                const int dt = hp / (kHaloH * kHaloW), rem = hp % (kHaloH * kHaloW);
                const int ll = l + dt - 1, h = h0 + rem / kHaloW - 1, w = w0 + rem % kHaloW - 1;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (ll >= 0 && ll < D.L && h >= 0 && h < D.H && w >= 0 && w < D.W)
                    v = *reinterpret_cast<const float4 *>(x + c16_at(D, xplanes, f + dt - 1, cig * 2 + g, h, w) + piece * 4);
                *reinterpret_cast<float4 *>(sX + hp * kC + g * 16 + piece * 4) = v;
            }
        }
        __syncthreads();

        if (doW) {
#pragma unroll
            for (int row = 0; row < kTileH; ++row) {
                const float *am = sM + row * kTileW * kC + lane;
                const float *bx = sX + row * kHaloW * kC + lane;
#pragma unroll 2
                for (int c = 0; c < kTileW; c += 2) {
                    const float a = am[c * kC];
#pragma unroll
                    for (int j = 0; j < kTapsPerWave; ++j) {
                        if (j < ntaps) {
                            const float b = bx[c * kC + tapoff[j]];
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (doB) add_channel_part(sM, t, bsum);

        if (doW && (++chain == kChainTiles || tile + 1 == t1)) {
            // C/D map of the 32x32 MFMA: column (ci) = lane & 31, row (co) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
            for (int j = 0; j < kTapsPerWave; ++j) {
                if (j < ntaps) {
                    double *blk = mine + (size_t)(wv * kTapsPerWave + j) * (kC * kC);
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

    if (doB) reduce_channel_parts(reinterpret_cast<double *>(smem), t, bsum, mine + kTaps * kC * kC);
}

// one thread per output: e < pairs * 27 * 1024 is d_weight (e = (pair * 27 + tap) * 1024 + co * 32 + ci inside the pair's
// block), the others d_shift
__global__ __launch_bounds__(kThreads) void nwgrad_finish_kernel(const double *__restrict__ partial, Dims D, int doW, int doB,
                                                                 float *__restrict__ d_weight, float *__restrict__ d_shift) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    const int nw = D.pairs * kTaps * kC * kC;
    if (e >= nw + D.cout) return;
    const bool is_w = e < nw;
    if (is_w ? !doW : !doB) return;
    const int pair = is_w ? e / (kTaps * kC * kC) : ((e - nw) / kC) * D.gi;
    const int in = is_w ? e % (kTaps * kC * kC) : kTaps * kC * kC + (e - nw) % kC;
    double s = 0.0;
    for (int sh = 0; sh < D.shares; ++sh) s += partial[((size_t)sh * D.pairs + pair) * kPartial + in];
    if (is_w) {
        const int tap = in / (kC * kC), co = (pair / D.gi) * kC + (in / kC) % kC, ci = (pair % D.gi) * kC + in % kC;
        d_weight[((size_t)co * D.cin + ci) * kTaps + tap] = (float)s;
    } else {
        d_shift[e - nw] = (float)s;
    }
}

// widest: the most channels the calling entry takes on either side (64: v2ce_convn_wgrad and v2ce_conv32_wgrad).  At 512
// -> 512 there are 256 pairs and one share: 256 x kPartial f64 = 56 MB, the most the workspace ever is
bool make_dims(int widest, int cin, int cout, int B, int L, int H, int W, int pitch, int max_workgroups, Dims &D) {
    if (!channels_ok(cin, widest) || !channels_ok(cout, widest)) return false;
    if (!make_extent(B, L, H, W, pitch, false, 0, max_workgroups, D)) return false;
    D.cin = cin; D.cout = cout; D.gi = cin / kC; D.go = cout / kC; D.pairs = D.gi * D.go;
    D.shares = plan_shares(D.tiles, D.pairs, max_workgroups);
    D.total = round256((size_t)D.shares * D.pairs * kPartial * sizeof(double));
    return true;
}

const char *kNeeds = "B, L, H, W >= 1, pitch >= W, max_workgroups >= 0, B L H W < 2^31 and B L H pitch < 2^34";
const char *needs_channels(int widest) { return widest > 64 ? "{32, 64, 128, 256, 512}" : "{32, 64}"; }

// `entry`: the symbol the caller used; it leads every message
int nwgrad(const char *entry, int widest, const float *x, const float *y, const float *upstream, int cin, int cout, int B, int L, int H, int W,
           int pitch, float *d_weight, float *d_shift, void *workspace, size_t workspace_bytes, int max_workgroups,
           v2ce_stream_t stream) {
    clear_error();
    Dims D;
    V2CE_REQUIRE(make_dims(widest, cin, cout, B, L, H, W, pitch, max_workgroups, D), V2CE_ERR_BAD_ARG,
                 "%s: cin %d cout %d B %d L %d H %d W %d pitch %d max_workgroups %d: needs cin, cout in %s, %s", entry, cin, cout, B,
                 L, H, W, pitch, max_workgroups, needs_channels(widest), kNeeds);
    V2CE_REQUIRE(x && upstream && workspace, V2CE_ERR_BAD_ARG, "%s: null pointer", entry);
    V2CE_REQUIRE(d_weight || d_shift, V2CE_ERR_BAD_ARG, "%s: no output requested (d_weight and d_shift are both null)", entry);
    V2CE_REQUIRE(aligned16(x, y, upstream), V2CE_ERR_BAD_ARG, "%s: x, y and upstream must be 16-byte aligned", entry);
    if (const int rc = check_workspace(entry, workspace, workspace_bytes, D.total)) return rc;
    hipStream_t st = as_stream(stream);
    double *partial = static_cast<double *>(workspace);
    const int doW = d_weight != nullptr, doB = d_shift != nullptr;
    const int outputs = D.pairs * kTaps * kC * kC + D.cout;
    V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(nwgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kLds));
    hipLaunchKernelGGL(nwgrad_kernel, dim3((unsigned)(D.shares * D.pairs)), dim3(kThreads), kLds, st, x, y, upstream, D, doW, doB,
                       partial);
    hipLaunchKernelGGL(nwgrad_finish_kernel, dim3((outputs + kThreads - 1) / kThreads), dim3(kThreads), 0, st, partial, D, doW,
                       doB, d_weight, d_shift);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_convn_wgrad_workspace_bytes(int cin, int cout, int B, int L, int H, int W, int pitch, int max_workgroups) {
    Dims D;
    return make_dims(64, cin, cout, B, L, H, W, pitch, max_workgroups, D) ? D.total : 0;
}

extern "C" int v2ce_convn_wgrad(const float *x, const float *y, const float *upstream, int cin, int cout, int B, int L, int H,
                                int W, int pitch, float *d_weight, float *d_shift, void *workspace, size_t workspace_bytes,
                                int max_workgroups, v2ce_stream_t stream) {
    return nwgrad("v2ce_convn_wgrad", 64, x, y, upstream, cin, cout, B, L, H, W, pitch, d_weight, d_shift, workspace, workspace_bytes,
                  max_workgroups, stream);
}

// the entries of include/v2ce_hip_convcgrad.h: every width of the UNet on either side, up to 16 x 16 pairs
extern "C" size_t v2ce_convc_wgrad_workspace_bytes(int cin, int cout, int B, int L, int H, int W, int pitch, int max_workgroups) {
    Dims D;
    return make_dims(kWidest, cin, cout, B, L, H, W, pitch, max_workgroups, D) ? D.total : 0;
}

extern "C" int v2ce_convc_wgrad(const float *x, const float *y, const float *upstream, int cin, int cout, int B, int L, int H,
                                int W, int pitch, float *d_weight, float *d_shift, void *workspace, size_t workspace_bytes,
                                int max_workgroups, v2ce_stream_t stream) {
    return nwgrad("v2ce_convc_wgrad", kWidest, x, y, upstream, cin, cout, B, L, H, W, pitch, d_weight, d_shift, workspace,
                  workspace_bytes, max_workgroups, stream);
}

// the 32 -> 32 entries of include/v2ce_hip_convgrad.h: one pair
extern "C" size_t v2ce_conv32_wgrad_workspace_bytes(int B, int L, int H, int W, int pitch, int max_workgroups) {
    return v2ce_convn_wgrad_workspace_bytes(32, 32, B, L, H, W, pitch, max_workgroups);
}

extern "C" int v2ce_conv32_wgrad(const float *x, const float *y, const float *upstream, int B, int L, int H, int W, int pitch,
                                 float *d_weight, float *d_shift, void *workspace, size_t workspace_bytes, int max_workgroups,
                                 v2ce_stream_t stream) {
    return nwgrad("v2ce_conv32_wgrad", 64, x, y, upstream, 32, 32, B, L, H, W, pitch, d_weight, d_shift, workspace, workspace_bytes,
                  max_workgroups, stream);
}
