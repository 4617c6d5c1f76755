// convndgrad.hip -- the input gradient of a 3x3x3 Conv3d(cin, cout) with 32, 64, 128, 256 or 512 channels on either side on
// gfx950, seen through the relu behind it (include/v2ce_hip_convcgrad.h; include/v2ce_hip_convngrad.h for the entry that
// stops at 64 channels, v2ce_convn_dgrad, and include/v2ce_hip_convdgrad.h for the 32 -> 32 entry v2ce_conv32_dgrad state
// the formulas, the tensors and the precision contract).  UNet.decoders[3].conv2 is the 32 -> 32 case, UNet.decoders[2].conv2
// the 64 -> 64 case, UNet.decoders[1].conv2 the 128 -> 128 case.
//
// d_x is a GEMM with the positions as M, the input channels as N and (co group, tap, co) as K = 27 cout: per tap (kt, kh,
// kw) a block D[pos][ci] += sum_co m[co][pos - tap + 1] W[co][ci][tap].  v_mfma_f32_32x32x2_f32 takes two output channels
// per instruction: lane l holds A[pos = l & 31][k = l >> 5] and B[k = l >> 5][ci = l & 31].  A workgroup stages 32 channels
// at a time, whatever cin and cout are, so the tile, the halo and the bank arguments do not depend on them:
//   B  the weights, [tap][co][ci] after the prep kernel.  A wave keeps those of its taps (wave v takes the taps 7 v .. 7 v
//      + 6, the last wave six) for its 32 input channels in registers: 7 taps x 16 k-steps = 112 registers per lane and co
//      group.  Up to cout = 64 those of EVERY co group stay there for the whole kernel (224 registers at cout = 64; with
//      the 64 accumulator registers that is under the 512 a wave may hold at four waves per workgroup -- one workgroup
//      per CU: the LDS decides the occupancy anyway), and nothing is fetched again inside the tile walk.  Four co groups
//      would need 448 + 64 registers, so from cout = 128 on a wave holds ONE co group at a time (the 112 registers of the
//      cout = 32 instance) and fetches each group's weights again per tile, through L2: 28 KB per wave and group, issued
//      in front of the group's halo staging and used behind its barrier, against the 448 MFMAs (28 600 cycles) the wave
//      runs on them.  (Two groups at a time, the 224 registers of the cout = 64 instance plus the chunk walk, spill)
//   A  the halo of m of ONE co group in LDS, channel-major: sH[co][halo position], 3 frames x 4 rows x 66 columns = 792
//      positions at a plane stride of kPlane = 800 floats (= 32 mod 64).  The 32 lanes of a half read 32 consecutive
//      columns of one row of one channel plane (consecutive banks); the other half reads the next plane, 32 banks further:
//      one conflict-free ds_read_b32 per MFMA
//
// The grid is (cin / 32) x shares: workgroup s * gi + cig walks share s of the tiles for the input channels 32 cig .. + 31,
// so one workgroup produces a whole d_x element.  A tile is 2 rows x 64 columns of one frame: four M groups of 32
// positions, one accumulator (16 registers) each per wave.  Per tile the workgroup
//   1. for co group 0, 1, ..., cout / 32 - 1 in that order: stages m = y > 0 ? upstream : 0 of the group's halo into sH (zeros
//      outside the frame, the sequence and the row's W columns), writes d_res from the tile's own positions on the way
//      (cig = 0 only) and runs its taps into the SAME accumulators: 4 independent MFMA chains per wave, 7 x 16 steps each
//      per group;
//   2. zero-fills the padding columns W .. pitch-1 of the tile's rows when the tile is the last one of its rows: those of
//      its 32 channels of d_x, and (cig = 0) those of d_res;
//   3. writes the four partial tiles over the halo (sP[wave][position][ci], 64 KB) and adds them in the order of the waves,
//      ((p0 + p1) + p2) + p3, one thread per four channels of a position, into d_x.
// An element's order of summation is fixed by cout and the tap split alone: it depends neither on the grid nor on the tile
// walk.  At 32 -> 32 there is one ci group and one co group: the grid is the shares, and a tile's halo is staged once.
#include "convgrad_dev.h"

#include "../../include/v2ce_hip_convdgrad.h"
#include "../../include/v2ce_hip_convcgrad.h"
#include "../../include/v2ce_hip_convngrad.h"

namespace v2ce {
namespace {

constexpr int kTapsPerWave = 7;
constexpr int kSteps = kC / 2;                      // k-steps of a tap and co group: two output channels per MFMA
constexpr int kGroups = kTile / 32;                 // M groups of a tile: (row, half of the columns)
constexpr size_t kLds = (size_t)kC * kPlane * sizeof(float);            // 100 KB
static_assert((size_t)4 * kTile * kC * sizeof(float) <= kLds, "the partial tiles lie over the halo");
static_assert(kLds <= 160 * 1024, "LDS of one workgroup");
static_assert(V2CE_DGRAD_TERMS == kTaps * kC, "terms of an element of d_x at 32 -> 32 (27 * 32)");
static_assert(kTapsPerWave * 4 >= kTaps && kTapsPerWave * 3 < kTaps, "every wave has a tap");

struct Dims : Extent {
    int cin, cout, gi;                              // gi: groups of 32 input channels
    int shares;
    size_t total;
};

// [co][ci][27] -> [tap][co][ci]: what a lane of the main kernel loads as consecutive floats
__global__ __launch_bounds__(kThreads) void ndgrad_prep_kernel(const float *__restrict__ weight, int cin, int cout,
                                                               float *__restrict__ wt) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= kTaps * cout * cin) return;
    const int tap = e / (cout * cin), rest = e % (cout * cin);
    wt[e] = weight[(size_t)rest * kTaps + tap];
}

// wave wv's B operands of the co groups cg0 .. cg0 + kCog - 1: step s of tap j and group cg is W[co = 32 (cg0 + cg) + 2 s +
// (lane >> 5)][ci = 32 cig + (lane & 31)][tap]; zeros for a tap past the last one
template <int kCog>
__device__ __forceinline__ void load_weights(const float *__restrict__ wt, const Dims &D, int wv, int lane, int cig, int cg0,
                                             bool doX, float (&wreg)[kCog][kTapsPerWave][kSteps]) {
#pragma unroll
    for (int j = 0; j < kTapsPerWave; ++j) {
        const int tap = wv * kTapsPerWave + j;
        const bool live = doX && tap < kTaps;
#pragma unroll
        for (int cg = 0; cg < kCog; ++cg)
#pragma unroll
            for (int s = 0; s < kSteps; ++s)
                wreg[cg][j][s] =
                    live ? wt[((size_t)tap * D.cout + (cg0 + cg) * kC + 2 * s + (lane >> 5)) * D.cin + cig * kC + (lane & 31)] : 0.0f;
    }
}

// kCog: co groups of 32 output channels whose weights a wave holds at a time.  !kReload: cout = 32 kCog, they are loaded
// once; kReload: cout is a multiple of 32 kCog and every chunk of kCog groups is loaded again per tile
template <int kCog, bool kReload>
__global__ __launch_bounds__(kThreads) void ndgrad_kernel(const float *__restrict__ wt, const float *__restrict__ y,
                                                          const float *__restrict__ up, Dims D, float *__restrict__ d_x,
                                                          float *__restrict__ d_res_arg) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sH = smem, *sP = smem;                    // the partial tiles lie over the halo once it has been read
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(t / kWave);
    const int cig = blockIdx.x % D.gi;
    const long long share = blockIdx.x / D.gi;
    const long long t0 = share * D.tiles / D.shares, t1 = (share + 1) * D.tiles / D.shares;
    const int ntaps = kTaps - wv * kTapsPerWave < kTapsPerWave ? kTaps - wv * kTapsPerWave : kTapsPerWave;
    const bool doX = d_x != nullptr;
    float *d_res = cig == 0 ? d_res_arg : nullptr;   // d_res is written once, by the workgroups of the first ci group
    if (!doX && !d_res) return;                      // (uniform)
    const int xplanes = D.cin / 16, mplanes = D.cout / 16;

    const int chunks = kReload ? D.cout / (kC * kCog) : 1;

    float wreg[kCog][kTapsPerWave][kSteps];         // B operands of this wave's taps
    int tapoff[kTapsPerWave];                       // the tap's shift inside a plane of sH: m at pos - tap + 1
#pragma unroll
    for (int j = 0; j < kTapsPerWave; ++j) {
        const int tap = wv * kTapsPerWave + j, kt = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
        const bool live = doX && tap < kTaps;
        tapoff[j] = live ? ((2 - kt) * kHaloH + (2 - kh)) * kHaloW + (2 - kw) : 0;
    }
    if (!kReload) load_weights<kCog>(wt, D, wv, lane, cig, 0, doX, wreg);

    for (long long tile = t0; tile < t1; ++tile) {
        const TileAt ta = tile_at(D, tile);
        const long long f = ta.f;
        const int l = ta.l, h0 = ta.h0, w0 = ta.w0, tw = ta.tw;

        f32x16 acc[kGroups];
#pragma unroll
        for (int gq = 0; gq < kGroups; ++gq)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[gq][r] = 0.0f;

        for (int chunk = 0; chunk < chunks; ++chunk) {
            if (kReload) load_weights<kCog>(wt, D, wv, lane, cig, chunk * kCog, doX, wreg);
#pragma unroll
            for (int cg = 0; cg < kCog; ++cg) {
                const int cog = chunk * kCog + cg;       // the co group on its way
                if (doX) __syncthreads();                // the previous tile's partials / group's halo have been read
                // the halo of m: 2 planes x 792 positions, 64 bytes each; consecutive lanes take consecutive positions
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
                        const long long at = c16_at(D, mplanes, f + dt - 1, cog * 2 + g, h, w);
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
                if (!doX) continue;                      // (uniform: d_res alone needs neither the LDS nor a barrier)
                __syncthreads();

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
                                acc[gq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wreg[cg][j][s], acc[gq], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            }

        if (tw == D.tiles_w - 1 && D.pitch > D.W) {
            // the padding columns of the tile's rows: (row, plane, column, piece of 16 bytes); the planes of d_x are this
            // workgroup's two, those of d_res all of them
            const int pad = D.pitch - D.W;
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (d_x) {
                const long long n = (long long)kTileH * 2 * pad * 4;
                for (long long i = t; i < n; i += kThreads) {
                    const int piece = (int)(i & 3), col = (int)((i >> 2) % pad), rg = (int)((i >> 2) / pad), g = rg & 1, h = h0 + (rg >> 1);
                    if (h >= D.H) continue;
                    *reinterpret_cast<float4 *>(d_x + c16_at(D, xplanes, f, cig * 2 + g, h, D.W + col) + piece * 4) = zero;
                }
            }
            if (d_res) {
                const long long n = (long long)kTileH * mplanes * pad * 4;
                for (long long i = t; i < n; i += kThreads) {
                    const int piece = (int)(i & 3), col = (int)((i >> 2) % pad), rg = (int)((i >> 2) / pad), g = rg % mplanes,
                              h = h0 + rg / mplanes;
                    if (h >= D.H) continue;
                    *reinterpret_cast<float4 *>(d_res + c16_at(D, mplanes, f, g, h, D.W + col) + piece * 4) = zero;
                }
            }
        }
        if (!doX) continue;                          // (uniform)
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
                *reinterpret_cast<float4 *>(d_x + c16_at(D, xplanes, f, cig * 2 + g, h, w) + piece * 4) = s;
            }
        }
    }
}

// widest: the most channels the calling entry takes on either side (64: v2ce_convn_dgrad and v2ce_conv32_dgrad)
bool make_dims(int widest, int cin, int cout, int B, int L, int H, int W, int pitch, int max_workgroups, Dims &D) {
    if (!channels_ok(cin, widest) || !channels_ok(cout, widest)) return false;
    if (!make_extent(B, L, H, W, pitch, false, 0, max_workgroups, D)) return false;
    D.cin = cin; D.cout = cout; D.gi = cin / kC;
    D.shares = plan_shares(D.tiles, D.gi, max_workgroups);
    D.total = round256((size_t)kTaps * cout * cin * sizeof(float));     // the repacked weight; the grid needs nothing
    return true;
}

const char *kNeeds = "B, L, H, W >= 1, pitch >= W, max_workgroups >= 0, B L H W < 2^31 and B L H pitch < 2^34";
const char *needs_channels(int widest) { return widest > 64 ? "{32, 64, 128, 256, 512}" : "{32, 64}"; }

// `entry`: the symbol the caller used; it leads every message
int ndgrad(const char *entry, int widest, const float *weight, const float *y, const float *upstream, int cin, int cout, int B, int L, int H,
           int W, int pitch, float *d_x, float *d_res, void *workspace, size_t workspace_bytes, int max_workgroups,
           v2ce_stream_t stream) {
    clear_error();
    Dims D;
    V2CE_REQUIRE(make_dims(widest, cin, cout, B, L, H, W, pitch, max_workgroups, D), V2CE_ERR_BAD_ARG,
                 "%s: cin %d cout %d B %d L %d H %d W %d pitch %d max_workgroups %d: needs cin, cout in %s, %s", entry, cin, cout, B,
                 L, H, W, pitch, max_workgroups, needs_channels(widest), kNeeds);
    V2CE_REQUIRE(weight && upstream && workspace, V2CE_ERR_BAD_ARG, "%s: null pointer", entry);
    V2CE_REQUIRE(d_x || d_res, V2CE_ERR_BAD_ARG, "%s: no output requested (d_x and d_res are both null)", entry);
    V2CE_REQUIRE(aligned16(y, upstream, d_x, d_res), V2CE_ERR_BAD_ARG, "%s: y, upstream, d_x and d_res must be 16-byte aligned",
                 entry);
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(weight) & 3) == 0, V2CE_ERR_BAD_ARG, "%s: weight must be 4-byte aligned", entry);
    if (const int rc = check_workspace(entry, workspace, workspace_bytes, D.total)) return rc;
    hipStream_t st = as_stream(stream);
    float *wt = static_cast<float *>(workspace);
    // up to two co groups stay in registers; from 128 output channels on they come one at a time, again per tile
    const auto kernel = cout > 64 ? ndgrad_kernel<1, true> : cout == 64 ? ndgrad_kernel<2, false> : ndgrad_kernel<1, false>;
    if (d_x) {
        const int weights = kTaps * cout * cin;
        V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)kLds));
        hipLaunchKernelGGL(ndgrad_prep_kernel, dim3((weights + kThreads - 1) / kThreads), dim3(kThreads), 0, st, weight, cin, cout,
                           wt);
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)(D.shares * D.gi)), dim3(kThreads), d_x ? kLds : 0, st, wt, y, upstream, D, d_x,
                       d_res);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_convn_dgrad_workspace_bytes(int cin, int cout, int B, int L, int H, int W, int pitch, int max_workgroups) {
    Dims D;
    return make_dims(64, cin, cout, B, L, H, W, pitch, max_workgroups, D) ? D.total : 0;
}

extern "C" int v2ce_convn_dgrad(const float *weight, const float *y, const float *upstream, int cin, int cout, int B, int L, int H,
                                int W, int pitch, float *d_x, float *d_res, void *workspace, size_t workspace_bytes,
                                int max_workgroups, v2ce_stream_t stream) {
    return ndgrad("v2ce_convn_dgrad", 64, weight, y, upstream, cin, cout, B, L, H, W, pitch, d_x, d_res, workspace, workspace_bytes,
                  max_workgroups, stream);
}

// the entries of include/v2ce_hip_convcgrad.h: every width of the UNet on either side
extern "C" size_t v2ce_convc_dgrad_workspace_bytes(int cin, int cout, int B, int L, int H, int W, int pitch, int max_workgroups) {
    Dims D;
    return make_dims(kWidest, cin, cout, B, L, H, W, pitch, max_workgroups, D) ? D.total : 0;
}

extern "C" int v2ce_convc_dgrad(const float *weight, const float *y, const float *upstream, int cin, int cout, int B, int L, int H,
                                int W, int pitch, float *d_x, float *d_res, void *workspace, size_t workspace_bytes,
                                int max_workgroups, v2ce_stream_t stream) {
    return ndgrad("v2ce_convc_dgrad", kWidest, weight, y, upstream, cin, cout, B, L, H, W, pitch, d_x, d_res, workspace,
                  workspace_bytes, max_workgroups, stream);
}

// the 32 -> 32 entries of include/v2ce_hip_convdgrad.h: ndgrad_kernel<1, false> with one ci group
extern "C" size_t v2ce_conv32_dgrad_workspace_bytes(int B, int L, int H, int W, int pitch, int max_workgroups) {
    return v2ce_convn_dgrad_workspace_bytes(32, 32, B, L, H, W, pitch, max_workgroups);
}

extern "C" int v2ce_conv32_dgrad(const float *weight, const float *y, const float *upstream, int B, int L, int H, int W, int pitch,
                                 float *d_x, float *d_res, void *workspace, size_t workspace_bytes, int max_workgroups,
                                 v2ce_stream_t stream) {
    return ndgrad("v2ce_conv32_dgrad", 64, weight, y, upstream, 32, 32, B, L, H, W, pitch, d_x, d_res, workspace, workspace_bytes,
                  max_workgroups, stream);
}
