// voxmetrics.hip -- the stage-1 score of voxel grids against a recording's voxels, on gfx950.
//
// Replaces the metric classes of train/scripts/model/metrics.py (BinaryMatch, BinaryMatchF1 / f1score, PoolMSE,
// MeanRatio, and nn.L1Loss) for inputs pred, gt of shape [B, L, 20, H, W] f32 (channels (p c): 2 polarities x 10
// bins).  One call returns per-sequence (per b) sufficient statistics that combine exactly across b:
//
//   op in {raw, sum_c, sum_cp}: int64 N, TP, FP, FN of the binarised (v > threshold) pred and gt
//   f64 sum |p - g|,  f64 sum of r = (p + 0.01f) / (g + 0.01f) with r < 1 ? 1 / r : r
//   per pool size k: f64 sum (pool_k(p) - pool_k(g))^2 and the int64 count of pooled values, where pool_k is
//   AvgPool3d(k, stride k) over ((l c), h, w) of one (b, p) -- windows of k consecutive (l c) planes cross frame
//   boundaries, and each axis is floored to a multiple of k (metrics.py:117-128).
//
// Fused pass (k = 2 and k = 4 together with the rest): one workgroup per (b, pair of frames 2m / 2m+1, band of 4
// rows); a lane owns 4 columns x 4 rows and walks the 2 x 20 planes in memory order.  The 20 planes of one polarity of
// a frame pair are five k = 4 windows, so no window leaves the workgroup; when L is odd the last frame keeps its two
// full windows and drops two planes, as torch does.  Other k run through pool_generic_kernel, one launch per size.
//
// Arithmetic (built with the EXACT flags): thresholds v > threshold in f32; sum_c adds the 10 bins of a polarity in
// order c = 0..9, sum_cp the 20 channels in order, both in f32 from zero; |p - g| and the ratio in f32 (IEEE divide);
// a pooled value is the f32 sum of its k^3 values in (d, h, w) loop order divided by (float)(k^3), its difference and
// square in f32.  Every sum is f64 per lane, then reduced in a fixed tree per workgroup, written to the workspace and
// reduced per b in a fixed order: no float atomics, so the statistics are bit-identical run to run and do not depend
// on how many sequences share the call.  A NaN is never above the threshold and propagates into the f64 sums.
#include "common.h"

#include <algorithm>

namespace v2ce {
namespace {

constexpr int kFinishThreads = 256;
constexpr int kGenThreads = 256;
constexpr int kGenBlocksMax = 1024;       // grid-stride cap per (b, k) of the generic pool kernel
constexpr int kSlots = 16;                // per-workgroup partial record: 9 int64 counts, 4 f64 sums, padding
constexpr int kChannels = 20;

struct Shape {
    int B, L, H, W;
    int bands, pairs, groups;             // ceil(H/4), ceil(L/2), ceil(W/4)
    long long plane;                      // H * W
};

__device__ __forceinline__ void wave_sum(long long &v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
}
__device__ __forceinline__ void wave_sum(double &v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
}

template <bool kVec>
__device__ __forceinline__ void load_row4(const float *__restrict__ row, int x0, int W, float *v) {
    if (kVec && x0 + 3 < W) {             // W even and 8-B aligned base: two float2 at even columns
        const float2 a = *reinterpret_cast<const float2 *>(row + x0);
        const float2 b = *reinterpret_cast<const float2 *>(row + x0 + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = x0 + j < W ? row[x0 + j] : 0.0f;
    }
}

// grid (bands, pairs, B), block = a multiple of 64 lanes, each lane one group of 4 columns at a time
template <bool kVec>
__global__ __launch_bounds__(256) void fused_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                   Shape S, float thr, double *__restrict__ part) {
    const int band = blockIdx.x, m = blockIdx.y, b = blockIdx.z;
    const int y0 = band * 4;
    const bool pool4_rows = y0 + 4 <= S.H;
    int cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};    // tp, fp, fn of raw, sum_c, sum_cp
    double l1 = 0.0, ratio = 0.0, sq2 = 0.0, sq4 = 0.0;
    bool rv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rv[r] = y0 + r < S.H;

    for (int g = threadIdx.x; g < S.groups; g += blockDim.x) {
        const int x0 = g * 4;
        bool cv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = x0 + j < S.W;
        const bool pool4_cols = x0 + 4 <= S.W;
        float s4p[2] = {0.0f, 0.0f}, s4g[2] = {0.0f, 0.0f};
        for (int fl = 0; fl < 2; ++fl) {
            const int f = 2 * m + fl;
            if (f >= S.L) break;
            float cpp[16], cpg[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) cpp[e] = cpg[e] = 0.0f;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float scp[16], scg[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) scp[e] = scg[e] = 0.0f;
                for (int cc = 0; cc < 5; ++cc) {
                    float s2p[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s2g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int c = 2 * cc + h;
                        const int d = f * 10 + c;                    // depth of this plane in (l c) of polarity p
                        const long long base = ((long long)(b * S.L + f) * kChannels + p * 10 + c) * S.plane;
                        float V[16], U[16];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const long long ro = base + (long long)(rv[r] ? y0 + r : 0) * S.W;
                            if (rv[r]) {
                                load_row4<kVec>(pred + ro, x0, S.W, V + 4 * r);
                                load_row4<kVec>(gt + ro, x0, S.W, U + 4 * r);
                            } else {
#pragma unroll
                                for (int j = 0; j < 4; ++j) V[4 * r + j] = U[4 * r + j] = 0.0f;
                            }
                        }
                        if ((d & 3) == 0) { s4p[p] = 0.0f; s4g[p] = 0.0f; }
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int e = 4 * r + j;
                                const float v = V[e], u = U[e];
                                scp[e] += v; scg[e] += u;
                                cpp[e] += v; cpg[e] += u;
                                s2p[(r >> 1) * 2 + (j >> 1)] += v;
                                s2g[(r >> 1) * 2 + (j >> 1)] += u;
                                s4p[p] += v; s4g[p] += u;
                                if (rv[r] && cv[j]) {
                                    const bool pb = v > thr, gb = u > thr;
                                    cnt[0] += pb && gb; cnt[1] += pb && !gb; cnt[2] += !pb && gb;
                                    l1 += (double)fabsf(v - u);
                                    float q = (v + 0.01f) / (u + 0.01f);
                                    q = q < 1.0f ? 1.0f / q : q;
                                    ratio += (double)q;
                                }
                            }
                        if (h == 1) {   // the four k = 2 windows of this plane pair
#pragma unroll
                            for (int w = 0; w < 4; ++w) {
                                const int a = w >> 1, bb = w & 1;
                                if (y0 + 2 * a + 2 <= S.H && x0 + 2 * bb + 2 <= S.W) {
                                    const float df = s2p[w] / 8.0f - s2g[w] / 8.0f;
                                    sq2 += (double)(df * df);
                                }
                            }
                        }
                        if ((d & 3) == 3 && pool4_rows && pool4_cols) {   // d = 4j + 3 < 10 L: the window is whole
                            const float df = s4p[p] / 64.0f - s4g[p] / 64.0f;
                            sq4 += (double)(df * df);
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (rv[e >> 2] && cv[e & 3]) {
                        const bool pb = scp[e] > thr, gb = scg[e] > thr;
                        cnt[3] += pb && gb; cnt[4] += pb && !gb; cnt[5] += !pb && gb;
                    }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (rv[e >> 2] && cv[e & 3]) {
                    const bool pb = cpp[e] > thr, gb = cpg[e] > thr;
                    cnt[6] += pb && gb; cnt[7] += pb && !gb; cnt[8] += !pb && gb;
                }
        }
    }

    // fixed-order reduction: butterfly per wave, then the waves in order
    __shared__ double red[4][kSlots];
    long long c64[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { c64[k] = cnt[k]; wave_sum(c64[k]); }
    wave_sum(l1); wave_sum(ratio); wave_sum(sq2); wave_sum(sq4);
    const int wv = threadIdx.x / kWave, nw = blockDim.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) red[wv][k] = __longlong_as_double(c64[k]);
        red[wv][9] = l1; red[wv][10] = ratio; red[wv][11] = sq2; red[wv][12] = sq4;
    }
    __syncthreads();
    if (threadIdx.x < kSlots) {
        const int k = threadIdx.x;
        double *out = part + ((size_t)b * S.pairs * S.bands + (size_t)m * S.bands + band) * kSlots;
        if (k < 9) {
            long long s = 0;
            for (int w = 0; w < nw; ++w) s += __double_as_longlong(red[w][k]);
            out[k] = __longlong_as_double(s);
        } else if (k < 13) {
            double s = 0.0;
            for (int w = 0; w < nw; ++w) s += red[w][k];
            out[k] = s;
        } else {
            out[k] = 0.0;
        }
    }
}

// one lane per pooled value of (b, p, jd, jh, jw); grid (blocks, B); one f64 partial per block
__global__ __launch_bounds__(kGenThreads) void pool_generic_kernel(const float *__restrict__ pred,
                                                                   const float *__restrict__ gt, Shape S, int k,
                                                                   double *__restrict__ part) {
    const int b = blockIdx.y;
    const int Dk = 10 * S.L / k, Hk = S.H / k, Wk = S.W / k;
    const long long nout = 2ll * Dk * Hk * Wk;
    const float div = (float)(k * k * k);
    double acc = 0.0;
    for (long long o = (long long)blockIdx.x * kGenThreads + threadIdx.x; o < nout; o += (long long)gridDim.x * kGenThreads) {
        const int jw = (int)(o % Wk);
        const int jh = (int)((o / Wk) % Hk);
        const long long t = o / ((long long)Wk * Hk);
        const int jd = (int)(t % Dk), p = (int)(t / Dk);
        float sp = 0.0f, sg = 0.0f;
        for (int dd = 0; dd < k; ++dd) {
            const int d = jd * k + dd, l = d / 10, c = d % 10;
            const float *pp = pred + ((long long)(b * S.L + l) * kChannels + p * 10 + c) * S.plane;
            const float *gg = gt + ((long long)(b * S.L + l) * kChannels + p * 10 + c) * S.plane;
            for (int hh = 0; hh < k; ++hh) {
                const long long ro = (long long)(jh * k + hh) * S.W + (long long)jw * k;
                for (int ww = 0; ww < k; ++ww) { sp += pp[ro + ww]; sg += gg[ro + ww]; }
            }
        }
        const float df = sp / div - sg / div;
        acc += (double)(df * df);
    }
    __shared__ double red[kGenThreads / kWave];
    wave_sum(acc);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kGenThreads / kWave; ++w) s += red[w];
        part[(size_t)b * gridDim.x + blockIdx.x] = s;
    }
}

struct Pools {
    int n;
    int k[V2CE_VOXMETRICS_MAX_POOLS];
    int gen_blocks[V2CE_VOXMETRICS_MAX_POOLS];     // 0: served by the fused pass (k = 2, 4)
    size_t gen_off[V2CE_VOXMETRICS_MAX_POOLS];     // byte offset of the partials in the workspace
};

// grid B: the partials of sequence b in a fixed order (strided per thread, then a fixed tree) -> stats[b]
__global__ __launch_bounds__(kFinishThreads) void finish_kernel(Shape S, Pools Q, const double *__restrict__ part,
                                                               const char *__restrict__ ws,
                                                               v2ce_voxmetrics_stats *__restrict__ stats) {
    __shared__ double red[kFinishThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nwg = S.pairs * S.bands;
    const double *pb = part + (size_t)b * nwg * kSlots;
    v2ce_voxmetrics_stats *out = stats + b;
    auto tree = [&](double v, bool as_int) -> double {
        red[t] = v;
        __syncthreads();
        for (int o = kFinishThreads / 2; o; o >>= 1) {
            if (t < o) {
                if (as_int) red[t] = __longlong_as_double(__double_as_longlong(red[t]) + __double_as_longlong(red[t + o]));
                else red[t] = red[t] + red[t + o];
            }
            __syncthreads();
        }
        const double r = red[0];
        __syncthreads();
        return r;
    };
    long long cnt[9];
    for (int k = 0; k < 9; ++k) {
        long long s = 0;
        for (int i = t; i < nwg; i += kFinishThreads) s += __double_as_longlong(pb[(size_t)i * kSlots + k]);
        cnt[k] = __double_as_longlong(tree(__longlong_as_double(s), true));
    }
    double sums[4];
    for (int k = 0; k < 4; ++k) {
        double s = 0.0;
        for (int i = t; i < nwg; i += kFinishThreads) s += pb[(size_t)i * kSlots + 9 + k];
        sums[k] = tree(s, false);
    }
    double gen[V2CE_VOXMETRICS_MAX_POOLS];
    for (int q = 0; q < Q.n; ++q) {
        gen[q] = 0.0;
        if (!Q.gen_blocks[q]) continue;
        const double *gp = reinterpret_cast<const double *>(ws + Q.gen_off[q]) + (size_t)b * Q.gen_blocks[q];
        double s = 0.0;
        for (int i = t; i < Q.gen_blocks[q]; i += kFinishThreads) s += gp[i];
        gen[q] = tree(s, false);
    }
    if (t != 0) return;
    const long long L = S.L, HW = S.plane;
    out->struct_size = (int64_t)sizeof(v2ce_voxmetrics_stats);
    const long long n[3] = {L * 20 * HW, L * 2 * HW, L * HW};
    for (int op = 0; op < 3; ++op) {
        out->n[op] = n[op];
        out->tp[op] = cnt[3 * op];
        out->fp[op] = cnt[3 * op + 1];
        out->fn[op] = cnt[3 * op + 2];
    }
    out->abs_diff_sum = sums[0];
    out->ratio_sum = sums[1];
    out->n_pools = Q.n;
    for (int q = 0; q < V2CE_VOXMETRICS_MAX_POOLS; ++q) {
        if (q >= Q.n) { out->pool_size[q] = 0; out->pool_n[q] = 0; out->pool_sq_sum[q] = 0.0; continue; }
        const int k = Q.k[q];
        out->pool_size[q] = k;
        out->pool_n[q] = 2ll * (10 * L / k) * (S.H / k) * (S.W / k);
        out->pool_sq_sum[q] = k == 2 ? sums[2] : (k == 4 ? sums[3] : gen[q]);
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

bool make_plan(int B, int L, int C, int H, int W, const int *pool_sizes, int n_pools, Shape &S, Pools &Q,
               size_t &total) {
    if (B < 1 || B > 65535 || L < 1 || L > 2 * 65535 || C != kChannels || H < 1 || W < 1) return false;
    if ((long long)H * W >= (1ll << 31) || (long long)B * L * kChannels * H * W >= (1ll << 40)) return false;
    if (n_pools < 0 || n_pools > V2CE_VOXMETRICS_MAX_POOLS || (n_pools > 0 && !pool_sizes)) return false;
    S.B = B; S.L = L; S.H = H; S.W = W;
    S.bands = (H + 3) / 4; S.pairs = (L + 1) / 2; S.groups = (W + 3) / 4; S.plane = (long long)H * W;
    if (S.bands > 65535 * 1024) return false;
    const int kmax = std::min(10 * L, std::min(H, W));
    size_t o = align256((size_t)B * S.pairs * S.bands * kSlots * sizeof(double));
    Q.n = n_pools;
    for (int q = 0; q < n_pools; ++q) {
        const int k = pool_sizes[q];
        if (k < 1 || k > kmax) return false;
        Q.k[q] = k;
        Q.gen_blocks[q] = 0;
        Q.gen_off[q] = 0;
        if (k == 2 || k == 4) continue;
        const long long nout = 2ll * (10 * L / k) * (H / k) * (W / k);
        const long long nb = (nout + kGenThreads - 1) / kGenThreads;
        Q.gen_blocks[q] = (int)(nb < 1 ? 1 : (nb > kGenBlocksMax ? kGenBlocksMax : nb));
        Q.gen_off[q] = o;
        o += align256((size_t)B * Q.gen_blocks[q] * sizeof(double));
    }
    total = o;
    return true;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_voxmetrics_workspace_bytes(int B, int L, int C, int H, int W, const int *pool_sizes, int n_pools) {
    Shape S;
    Pools Q;
    size_t total = 0;
    return make_plan(B, L, C, H, W, pool_sizes, n_pools, S, Q, total) ? total : 0;
}

extern "C" int v2ce_voxmetrics(const float *pred, const float *gt, int B, int L, int C, int H, int W, float threshold,
                               const int *pool_sizes, int n_pools, v2ce_voxmetrics_stats *stats,
                               size_t stats_struct_size, void *workspace, size_t workspace_bytes,
                               v2ce_stream_t stream) {
    clear_error();
    V2CE_REQUIRE(stats_struct_size == sizeof(v2ce_voxmetrics_stats), V2CE_ERR_BAD_ARG,
                 "v2ce_voxmetrics: stats_struct_size %zu, this library writes v2ce_voxmetrics_stats of %zu bytes",
                 stats_struct_size, sizeof(v2ce_voxmetrics_stats));
    V2CE_REQUIRE(C == kChannels, V2CE_ERR_BAD_ARG, "v2ce_voxmetrics: C = %d, only 20 channels (2 polarities x 10 bins)", C);
    Shape S;
    Pools Q;
    size_t total = 0;
    V2CE_REQUIRE(make_plan(B, L, C, H, W, pool_sizes, n_pools, S, Q, total), V2CE_ERR_BAD_ARG,
                 "v2ce_voxmetrics: needs 1 <= B <= 65535, 1 <= L <= 131070, H, W >= 1, at most %d pool sizes, each in "
                 "[1, min(10 L, H, W)]", V2CE_VOXMETRICS_MAX_POOLS);
    V2CE_REQUIRE(pred && gt && stats && workspace, V2CE_ERR_BAD_ARG, "v2ce_voxmetrics: null pointer");
    V2CE_REQUIRE(workspace_bytes >= total, V2CE_ERR_WORKSPACE, "v2ce_voxmetrics: workspace too small (%zu < %zu)",
                 workspace_bytes, total);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    double *part = reinterpret_cast<double *>(ws);
    const int threads = S.groups >= 256 ? 256 : ((S.groups + kWave - 1) / kWave) * kWave;
    const bool vec = (W % 2 == 0) && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt)) % 8 == 0);
    const dim3 grid((unsigned)S.bands, (unsigned)S.pairs, (unsigned)B);
    if (vec) hipLaunchKernelGGL(fused_kernel<true>, grid, dim3(threads), 0, st, pred, gt, S, threshold, part);
    else hipLaunchKernelGGL(fused_kernel<false>, grid, dim3(threads), 0, st, pred, gt, S, threshold, part);
    for (int q = 0; q < Q.n; ++q)
        if (Q.gen_blocks[q])
            hipLaunchKernelGGL(pool_generic_kernel, dim3((unsigned)Q.gen_blocks[q], (unsigned)B), dim3(kGenThreads), 0, st,
                               pred, gt, S, Q.k[q], reinterpret_cast<double *>(ws + Q.gen_off[q]));
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)B), dim3(kFinishThreads), 0, st, S, Q, part,
                       static_cast<const char *>(ws), stats);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
