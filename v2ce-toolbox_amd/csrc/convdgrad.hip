// convdgrad.hip -- the input gradient of the last decoder block's 3x3x3 Conv3d(32, 32) on gfx950, seen through the relu
// behind it (include/v2ce_hip_convdgrad.h states the formulas, the tensors and the precision contract).
//
// d_x is a GEMM with the positions as M, the input channels as N and (tap, co) as K = 864: per tap (kt, kh, kw) a block
// D[pos][ci] += sum_co m[co][pos - tap + 1] W[co][ci][tap].  v_mfma_f32_32x32x2_f32 takes two output channels per
// instruction: lane l holds A[pos = l & 31][k = l >> 5] and B[k = l >> 5][ci = l & 31].
//   B  the weights, [tap][co][ci] after the prep kernel: a wave keeps those of its taps in registers for the whole kernel
//      (wave v takes the taps 7 v .. 7 v + 6, the last wave six): 7 taps x 16 k-steps = 112 registers per lane
//   A  the halo of m in LDS, channel-major: sH[co][halo position], 3 frames x 4 rows x 66 columns = 792 positions at a
//      plane stride of kPlane = 800 floats (= 32 mod 64).  The 32 lanes of a half read 32 consecutive columns of one row of
//      one channel plane (consecutive banks); the other half reads the next plane, 32 banks further: one conflict-free
//      ds_read_b32 per MFMA
//
// A persistent workgroup of four waves walks a contiguous share of the tiles.  A tile is 2 rows x 64 columns of one frame:
// four M groups of 32 positions, one accumulator (16 registers) each per wave.  Per tile the workgroup
//   1. stages m = y > 0 ? upstream : 0 of the halo into sH (zeros outside the frame, the sequence and the row's W columns:
//      the convolution's zero padding), writes d_res from the tile's own positions on the way and zero-fills the padding
//      columns W .. pitch-1 of the tile's rows in both outputs when the tile is the last one of its rows;
//   2. runs its taps: 4 independent MFMA chains per wave, 7 x 16 steps each;
//   3. writes the four partial tiles over the halo (sP[wave][position][ci], 64 KB) and adds them in the order of the waves,
//      ((p0 + p1) + p2) + p3, one thread per four channels of a position, into d_x.
// An element's order of summation is fixed by the tap split alone: it depends neither on the grid nor on the tile walk.
#include "common.h"

#include "../../include/v2ce_hip_convdgrad.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;                       // 4 waves
constexpr int kC = 32;
constexpr int kTaps = 27;
constexpr int kTapsPerWave = 7;
constexpr int kSteps = kC / 2;                      // k-steps of a tap: two output channels per MFMA
constexpr int kTileH = 2, kTileW = 64, kTile = kTileH * kTileW;
constexpr int kGroups = kTile / 32;                 // M groups of a tile: (row, half of the columns)
constexpr int kHaloT = 3, kHaloH = kTileH + 2, kHaloW = kTileW + 2;
constexpr int kHalo = kHaloT * kHaloH * kHaloW;     // 792 positions
constexpr int kPlane = 800;                         // floats between the channel planes of sH
constexpr int kMaxGrid = 256;                       // one workgroup per CU: 100 KB of LDS each
constexpr int kWeights = kTaps * kC * kC;
constexpr size_t kLds = (size_t)kC * kPlane * sizeof(float);
static_assert(kPlane >= kHalo && kPlane % 64 == 32, "plane stride: the two halves of a wave on disjoint banks");
static_assert((size_t)4 * kTile * kC * sizeof(float) <= kLds, "the partial tiles lie over the halo");
static_assert(kLds <= 160 * 1024, "LDS of one workgroup");
static_assert(V2CE_DGRAD_TERMS == kTaps * kC, "terms of an element");
static_assert(kTapsPerWave * 4 >= kTaps && kTapsPerWave * 3 < kTaps, "every wave has a tap");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Dims {
    int B, L, H, W, pitch;
    int tiles_h, tiles_w;
    long long tiles;                                // B L tiles_h tiles_w
    int grid;
    size_t total;
};

// float offset of channel group g of (frame, row, column) in a C16 tensor
__device__ __forceinline__ long long c16_at(const Dims &D, long long f, int g, int h, int w) {
    return ((((f * 2 + g) * D.H + h) * D.pitch) + w) * 16;
}

__device__ __forceinline__ float4 relu_mask(float4 u, float4 yv) {
    u.x = yv.x > 0.0f ? u.x : 0.0f; u.y = yv.y > 0.0f ? u.y : 0.0f;
    u.z = yv.z > 0.0f ? u.z : 0.0f; u.w = yv.w > 0.0f ? u.w : 0.0f;
    return u;
}

// [co][ci][27] -> [tap][co][ci]: what a lane of the main kernel loads as consecutive floats
__global__ __launch_bounds__(kThreads) void dgrad_prep_kernel(const float *__restrict__ weight, float *__restrict__ wt) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= kWeights) return;
    const int tap = e / (kC * kC), rest = e % (kC * kC);
    wt[e] = weight[rest * kTaps + tap];
}

__global__ __launch_bounds__(kThreads) void dgrad_kernel(const float *__restrict__ wt, const float *__restrict__ y,
                                                         const float *__restrict__ up, Dims D, float *__restrict__ d_x,
                                                         float *__restrict__ d_res) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sH = smem, *sP = smem;                    // the partial tiles lie over the halo once it has been read
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(t / kWave);
    const long long t0 = (long long)blockIdx.x * D.tiles / gridDim.x, t1 = ((long long)blockIdx.x + 1) * D.tiles / gridDim.x;
    const int ntaps = kTaps - wv * kTapsPerWave < kTapsPerWave ? kTaps - wv * kTapsPerWave : kTapsPerWave;
    const bool doX = d_x != nullptr;

    // B operands of this wave's taps: step s of tap j is W[co = 2 s + (lane >> 5)][ci = lane & 31][tap]
    float wreg[kTapsPerWave][kSteps];
    int tapoff[kTapsPerWave];                       // the tap's shift inside a plane of sH: m at pos - tap + 1
#pragma unroll
    for (int j = 0; j < kTapsPerWave; ++j) {
        const int tap = wv * kTapsPerWave + j, kt = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        const bool live = doX && tap < kTaps;
        tapoff[j] = live ? ((2 - kt) * kHaloH + (2 - kh)) * kHaloW + (2 - kw) : 0;
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
            wreg[j][s] = live ? wt[(tap * kC + 2 * s + (lane >> 5)) * kC + (lane & 31)] : 0.0f;
    }

    for (long long tile = t0; tile < t1; ++tile) {
        const int tw = (int)(tile % D.tiles_w);
        const long long r1 = tile / D.tiles_w;
        const int th = (int)(r1 % D.tiles_h);
        const long long f = r1 / D.tiles_h;          // frame b L + l
        const int l = (int)(f % D.L), h0 = th * kTileH, w0 = tw * kTileW;

        __syncthreads();                             // the previous tile's partials have been read
        // the halo of m: 2 channel groups x 792 positions, 64 bytes each; consecutive lanes take consecutive positions
        for (int i = t; i < 2 * kHalo; i += kThreads) {
            const int g = i / kHalo, hp = i % kHalo;
            const int dt = hp / (kHaloH * kHaloW), rem = hp % (kHaloH * kHaloW), hh = rem / kHaloW, ww = rem % kHaloW;
            const int ll = l + dt - 1, h = h0 + hh - 1, w = w0 + ww - 1;
            const bool own = dt == 1 && hh >= 1 && hh <= kTileH && ww >= 1 && ww <= kTileW;
            if (!doX && !own) continue;
            const bool inside = ll >= 0 && ll < D.L && h >= 0 && h < D.H && w >= 0 && w < D.W;
            float4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (inside) {
                const long long at = c16_at(D, f + dt - 1, g, h, w);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const float4 *>(up + at + q * 4);
                if (y) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = relu_mask(v[q], *reinterpret_cast<const float4 *>(y + at + q * 4));
                }
                if (own && d_res) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(d_res + at + q * 4) = v[q];
                }
            }
            if (doX) {
                float *dst = sH + (g * 16) * kPlane + hp;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    dst[(q * 4 + 0) * kPlane] = v[q].x; dst[(q * 4 + 1) * kPlane] = v[q].y;
                    dst[(q * 4 + 2) * kPlane] = v[q].z; dst[(q * 4 + 3) * kPlane] = v[q].w;
                }
            }
        }
        if (tw == D.tiles_w - 1 && D.pitch > D.W) {
            // the padding columns of the tile's rows: (row, group, column, piece of 16 bytes)
            const int pad = D.pitch - D.W;
            const long long n = (long long)kTileH * 2 * pad * 4;
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (long long i = t; i < n; i += kThreads) {
                const int piece = (int)(i & 3), col = (int)((i >> 2) % pad), rg = (int)((i >> 2) / pad), g = rg & 1, h = h0 + (rg >> 1);
                if (h >= D.H) continue;
                const long long at = c16_at(D, f, g, h, D.W + col) + piece * 4;
                if (d_x) *reinterpret_cast<float4 *>(d_x + at) = zero;
                if (d_res) *reinterpret_cast<float4 *>(d_res + at) = zero;
            }
        }
        if (!doX) continue;                          // (uniform: d_res alone needs neither the LDS nor a barrier)
        __syncthreads();

        f32x16 acc[kGroups];
#pragma unroll
        for (int gq = 0; gq < kGroups; ++gq)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[gq][r] = 0.0f;
        // group gq = (row gq >> 1, columns 32 (gq & 1) ..): lane's position inside a plane before the tap's shift
        const float *a0 = sH + (lane >> 5) * kPlane + (lane & 31);
#pragma unroll
        for (int j = 0; j < kTapsPerWave; ++j) {
            if (j < ntaps) {
                const float *aj = a0 + tapoff[j];
#pragma unroll
                for (int s = 0; s < kSteps; ++s) {
#pragma unroll
                    for (int gq = 0; gq < kGroups; ++gq) {
                        const float a = aj[2 * s * kPlane + (gq >> 1) * kHaloW + (gq & 1) * 32];
                        acc[gq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wreg[j][s], acc[gq], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                             // every wave has read the halo

        // C/D map of the 32x32 MFMA: column (ci) = lane & 31, row (position) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int gq = 0; gq < kGroups; ++gq) {
            float *blk = sP + ((size_t)wv * kTile + gq * 32) * kC + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) blk[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * kC] = acc[gq][r];
        }
        __syncthreads();

        // position p = row * 64 + column of the tile; 8 pieces of four channels each
#pragma unroll
        for (int k = 0; k < kTile * 8 / kThreads; ++k) {
            const int i = t + k * kThreads, piece = i & 3, rest = i >> 2, p = rest % kTile, g = rest / kTile;
            const int h = h0 + p / kTileW, w = w0 + p % kTileW;
            if (h < D.H && w < D.W) {
                const float *src = sP + p * kC + g * 16 + piece * 4;
                float4 s = *reinterpret_cast<const float4 *>(src);
#pragma unroll
                for (int v = 1; v < 4; ++v) {
                    const float4 q = *reinterpret_cast<const float4 *>(src + v * kTile * kC);
                    s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
                }
                *reinterpret_cast<float4 *>(d_x + c16_at(D, f, g, h, w) + piece * 4) = s;
            }
        }
    }
}

bool make_dims(int B, int L, int H, int W, int pitch, int max_workgroups, Dims &D) {
    if (B < 1 || L < 1 || H < 1 || W < 1 || pitch < W || max_workgroups < 0) return false;
    const long long N = (long long)B * L * H * W;
    if ((long long)B * L >= (1ll << 31) || (long long)H * W >= (1ll << 31) || N >= (1ll << 31)) return false;
    if ((long long)B * L * H >= (1ll << 34) || (long long)B * L * H * pitch >= (1ll << 34)) return false;
    D.B = B; D.L = L; D.H = H; D.W = W; D.pitch = pitch;
    D.tiles_h = (H + kTileH - 1) / kTileH;
    D.tiles_w = (W + kTileW - 1) / kTileW;
    D.tiles = (long long)B * L * D.tiles_h * D.tiles_w;
    long long grid = D.tiles < kMaxGrid ? D.tiles : kMaxGrid;
    if (max_workgroups > 0 && grid > max_workgroups) grid = max_workgroups;
    D.grid = (int)grid;
    D.total = ((size_t)kWeights * sizeof(float) + 255) & ~(size_t)255;     // the repacked weight; the grid needs nothing
    return true;
}

const char *kNeeds = "needs B, L, H, W >= 1, pitch >= W, max_workgroups >= 0, B L H W < 2^31 and B L H pitch < 2^34";

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_conv32_dgrad_workspace_bytes(int B, int L, int H, int W, int pitch, int max_workgroups) {
    Dims D;
    return make_dims(B, L, H, W, pitch, max_workgroups, D) ? D.total : 0;
}

extern "C" int v2ce_conv32_dgrad(const float *weight, const float *y, const float *upstream, int B, int L, int H, int W, int pitch,
                                 float *d_x, float *d_res, void *workspace, size_t workspace_bytes, int max_workgroups,
                                 v2ce_stream_t stream) {
    clear_error();
    Dims D;
    V2CE_REQUIRE(make_dims(B, L, H, W, pitch, max_workgroups, D), V2CE_ERR_BAD_ARG,
                 "v2ce_conv32_dgrad: B %d L %d H %d W %d pitch %d max_workgroups %d: %s", B, L, H, W, pitch, max_workgroups, kNeeds);
    V2CE_REQUIRE(weight && upstream && workspace, V2CE_ERR_BAD_ARG, "v2ce_conv32_dgrad: null pointer");
    V2CE_REQUIRE(d_x || d_res, V2CE_ERR_BAD_ARG, "v2ce_conv32_dgrad: no output requested (d_x and d_res are both null)");
    V2CE_REQUIRE(aligned16(y, upstream, d_x, d_res), V2CE_ERR_BAD_ARG,
                 "v2ce_conv32_dgrad: y, upstream, d_x and d_res must be 16-byte aligned");
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(weight) & 3) == 0, V2CE_ERR_BAD_ARG, "v2ce_conv32_dgrad: weight must be 4-byte aligned");
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, V2CE_ERR_BAD_ARG,
                 "v2ce_conv32_dgrad: workspace must be 8-byte aligned");
    V2CE_REQUIRE(workspace_bytes >= D.total, V2CE_ERR_WORKSPACE, "v2ce_conv32_dgrad: workspace too small (%zu < %zu)",
                 workspace_bytes, D.total);
    hipStream_t st = as_stream(stream);
    float *wt = static_cast<float *>(workspace);
    if (d_x) {
        V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(dgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)kLds));
        hipLaunchKernelGGL(dgrad_prep_kernel, dim3((kWeights + kThreads - 1) / kThreads), dim3(kThreads), 0, st, weight, wt);
    }
    hipLaunchKernelGGL(dgrad_kernel, dim3((unsigned)D.grid), dim3(kThreads), d_x ? kLds : 0, st, wt, y, upstream, D, d_x, d_res);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
