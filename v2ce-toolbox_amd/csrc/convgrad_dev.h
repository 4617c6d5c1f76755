// convgrad_dev.h -- what the gradient kernels of the 3x3x3 convolutions share (convnwgrad.hip, convndgrad.hip,
// convupnwgrad.hip, convupdgrad.hip): one tile design -- 2 rows x 64 columns of one frame, a halo of 3 frames x 4 rows x 66
// columns, 32 channels of either side at a time, four waves that split the 27 taps seven apiece -- with its addressing, the
// weight-gradient kernels' tile staging and f64 channel sums, and the host side's extent checks, share plan and workspace
// checks.  Only what at least two of the four files use in the same words is here.
#pragma once
#include "common.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;                       // 4 waves
constexpr int kC = 32;                              // channels of a group on either side
constexpr int kTaps = 27;
constexpr int kTileH = 2, kTileW = 64, kTile = kTileH * kTileW;
constexpr int kHaloT = 3, kHaloH = kTileH + 2, kHaloW = kTileW + 2;
constexpr int kHalo = kHaloT * kHaloH * kHaloW;     // 792 positions
constexpr int kPlane = 800;                         // floats between the channel planes of a channel-major halo (= 32 mod 64)
constexpr int kMaxGrid = 256;                       // one workgroup per CU: the LDS of a workgroup is 100 KB or more
static_assert(kPlane >= kHalo && kPlane % 64 == 32, "plane stride: the two halves of a wave on disjoint banks");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the tensors' extent and the tile walk over it; H0, W0, pitch0 describe the source of the upsampled channels (convup*.hip)
// and are 0 where there is none
struct Extent {
    int B, L, H, W, pitch, H0, W0, pitch0;
    int tiles_h, tiles_w;
    long long tiles;                                // B L tiles_h tiles_w
};

// float offset of plane g (16 channels) of (frame, row, column) in a C16 tensor with `planes` planes at the output resolution
__device__ __forceinline__ long long c16_at(const Extent &D, int planes, long long f, int g, int h, int w) {
    return ((((f * planes + g) * D.H + h) * D.pitch) + w) * 16;
}

__device__ __forceinline__ float4 relu_mask(float4 u, float4 yv) {
    u.x = yv.x > 0.0f ? u.x : 0.0f; u.y = yv.y > 0.0f ? u.y : 0.0f;
    u.z = yv.z > 0.0f ? u.z : 0.0f; u.w = yv.w > 0.0f ? u.w : 0.0f;
    return u;
}

struct TileAt {
    long long f;                                    // frame b L + l
    int l, h0, w0, tw;
};

__device__ __forceinline__ TileAt tile_at(const Extent &D, long long tile) {
    const int tw = (int)(tile % D.tiles_w);
    const long long r1 = tile / D.tiles_w;
    const int th = (int)(r1 % D.tiles_h);
    const long long f = r1 / D.tiles_h;
    return {f, (int)(f % D.L), th * kTileH, tw * kTileW, tw};
}

// a [128][32] tile of the planes plane0, plane0 + 1 of `src` into LDS, seen through the relu behind `y` where y is not null;
// positions outside the tensor hold zeros.  128 positions x 8 pieces of 16 bytes
__device__ __forceinline__ void stage_tile(const Extent &D, const float *__restrict__ src, const float *__restrict__ y, float *dst,
                                           int planes, int plane0, long long f, int h0, int w0, int t) {
#pragma unroll
    for (int k = 0; k < kTile * 8 / kThreads; ++k) {
        const int i = t + k * kThreads, piece = i & 3, rest = i >> 2, g = rest / kTile, p = rest % kTile;
        const int h = h0 + p / kTileW, w = w0 + p % kTileW;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (h < D.H && w < D.W) {
            const long long at = c16_at(D, planes, f, plane0 + g, h, w) + piece * 4;
            v = *reinterpret_cast<const float4 *>(src + at);
            if (y) v = relu_mask(v, *reinterpret_cast<const float4 *>(y + at));
        }
        *reinterpret_cast<float4 *>(dst + p * kC + g * 16 + piece * 4) = v;
    }
}

// thread t's share of a staged [128][32] tile's channel sums: channel t & 31 over the 16 positions (t >> 5) * 16 .. + 15
__device__ __forceinline__ void add_channel_part(const float *tile, int t, double &sum) {
    const float *row = tile + (t >> 5) * 16 * kC + (t & 31);
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += (double)row[i * kC];
}

// the eight parts of a channel meet: parts 2 wv (lanes 0 .. 31) and 2 wv + 1 (lanes 32 .. 63), summed in the order of the
// parts into dst[channel].  `red` is the workgroup's LDS, free once every thread has passed the first barrier
__device__ __forceinline__ void reduce_channel_parts(double *red, int t, double sum, double *dst) {
    __syncthreads();
    red[t] = sum;
    __syncthreads();
    if (t < kC) {
        double s = red[t];
#pragma unroll
        for (int part = 1; part < kThreads / kC; ++part) s += red[part * kC + t];
        dst[t] = s;
    }
}

// (The flush of a 32x32 accumulator into its f64 block through the C/D map stays written out in convnwgrad.hip and
// convupnwgrad.hip: as a function of one accumulator it costs nwgrad_kernel 29 registers more.)

// ---- host side ----

// B, L, H, W >= 1, pitch >= W, max_workgroups >= 0, B L H W < 2^31, B L H pitch < 2^34; with_source: pitch0 >= (W + 1) / 2
// and B L H0 pitch0 < 2^34 for the upsampled channels' source.  Fills the extent and the tile counts
inline bool make_extent(int B, int L, int H, int W, int pitch, bool with_source, int pitch0, int max_workgroups, Extent &D) {
    if (B < 1 || L < 1 || H < 1 || W < 1 || pitch < W || max_workgroups < 0) return false;
    const int H0 = with_source ? (H - 1) / 2 + 1 : 0, W0 = with_source ? (W - 1) / 2 + 1 : 0;
    if (with_source && pitch0 < W0) return false;
    const long long N = (long long)B * L * H * W;
    if ((long long)B * L >= (1ll << 31) || (long long)H * W >= (1ll << 31) || N >= (1ll << 31)) return false;
    if ((long long)B * L * H >= (1ll << 34) || (long long)B * L * H * pitch >= (1ll << 34)) return false;
    if (with_source && (long long)B * L * H0 * pitch0 >= (1ll << 34)) return false;
    D.B = B; D.L = L; D.H = H; D.W = W; D.pitch = pitch; D.H0 = H0; D.W0 = W0; D.pitch0 = with_source ? pitch0 : 0;
    D.tiles_h = (H + kTileH - 1) / kTileH;
    D.tiles_w = (W + kTileW - 1) / kTileW;
    D.tiles = (long long)B * L * D.tiles_h * D.tiles_w;
    return true;
}

// shares of the tile walk when `per` workgroups (pairs of channel groups, ...) walk every share: the grid is per x shares,
// at most kMaxGrid, and at most max_workgroups where that is not 0 -- but never less than one share
inline int plan_shares(long long tiles, int per, int max_workgroups) {
    const long long most = kMaxGrid / per;
    long long shares = tiles < most ? tiles : most;
    const long long cap = max_workgroups / per > 1 ? max_workgroups / per : 1;
    if (max_workgroups > 0 && shares > cap) shares = cap;
    return (int)shares;
}

// the channel counts of either side of a plain 3x3x3 convolution (convnwgrad.hip, convndgrad.hip): the widths of the UNet,
// up to what the entry takes (64 for v2ce_convn_* and v2ce_conv32_*, kWidest for v2ce_convc_*)
constexpr int kWidest = 512;
inline bool channels_ok(int c, int widest) {
    return (c == 32 || c == 64 || c == 128 || c == 256 || c == 512) && c <= widest;
}

inline size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// the workspace of `entry`: 8-byte aligned and at least `need` bytes -> V2CE_OK or the error, with the message set
inline int check_workspace(const char *entry, const void *workspace, size_t workspace_bytes, size_t need) {
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, V2CE_ERR_BAD_ARG, "%s: workspace must be 8-byte aligned", entry);
    V2CE_REQUIRE(workspace_bytes >= need, V2CE_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", entry, workspace_bytes, need);
    return V2CE_OK;
}

}  // namespace
}  // namespace v2ce
