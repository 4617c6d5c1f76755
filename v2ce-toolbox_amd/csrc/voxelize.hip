// voxelize.hip -- events -> discretised event volume on gfx950 (the inverse of LDATI).
//
// Replaces gen_discretized_event_volume of
// /root/reference/train/scripts/utils/events_utils.py:118-175 (calc_floor_ceil_delta :118-126,
// create_update :128-145): the time axis of the event set is rescaled to [0, bins-1] over its own
// [t_min, t_max], every event is split linearly between its floor and its ceil bin, positive
// polarity goes to planes [0, bins), negative (polarity 0 or -1: the reference maps 0 to -1 and
// sends p < 0 there, :153, :133-136) to [bins, 2*bins).
//
// Arithmetic follows the reference's CPU torch evaluation step by step (this file is built with
// -ffp-contract=off): scale = f32(1 / f32(t_max - t_min)) * f32(bins - 1)   (int / tensor is
// reciprocal * int), ts = clamp(f32(t - t_min) * scale, 0, bins-1), floor(ts + 1e-8f),
// ceil(ts - 1e-8f), weights (floor(ts)+1) - ts and ts - floor(ts + 1e-8f).  The only difference is
// the accumulation ORDER (float atomics instead of a sequential put_): results agree to f32
// summation error.  HBM-bound: 13 B read per event, two f32 atomics per event.
#include "common.h"

namespace v2ce {
namespace {

__global__ __launch_bounds__(256) void time_range_kernel(const int64_t *__restrict__ ts, long long n,
                                                         long long *range) {
    long long lo = 0x7fffffffffffffffll, hi = -0x7fffffffffffffffll - 1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long t = ts[i];
        lo = t < lo ? t : lo;
        hi = t > hi ? t : hi;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(range, lo);
        atomicMax(range + 1, hi);
    }
}

__global__ __launch_bounds__(256) void voxelize_kernel(const int64_t *__restrict__ ts, const int16_t *__restrict__ x,
                                                       const int16_t *__restrict__ y, const int8_t *__restrict__ p,
                                                       long long n, const long long *__restrict__ range, int bins,
                                                       int H, int W, float *__restrict__ vol) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long t_min = range[0], t_max = range[1];
    const float scale = (1.0f / (float)(t_max - t_min)) * (float)(bins - 1);       // events_utils.py:159
    float t = (float)(ts[i] - t_min) * scale;
    t = fminf(fmaxf(t, 0.0f), (float)(bins - 1));                                  // :160
    const float fl = floorf(t + 1e-8f), ce = ceilf(t - 1e-8f);                     // :119-120
    const float ce_fake = floorf(t) + 1.0f;                                        // :121
    const float d_ce = t - fl, d_fl = ce_fake - t;                                 // :123-124
    const int xi = x[i], yi = y[i];
    if (xi < 0 || xi >= W || yi < 0 || yi >= H) return;        // the host wrapper rejects these (:129-130)
    const long long plane = p[i] <= 0 ? bins : 0;                                  // :153-155, :134-136
    const long long pix = (long long)W * yi + xi;
    atomicAdd(vol + (long long)H * W * ((long long)fl + plane) + pix, d_fl);       // :164-168
    atomicAdd(vol + (long long)H * W * ((long long)ce + plane) + pix, d_ce);       // :170-173
}

size_t align_up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" int v2ce_voxelize_events(const int64_t *ts, const int16_t *x, const int16_t *y, const int8_t *p,
                                    int64_t n, int bins, int H, int W, float *volume, int64_t *t_range,
                                    v2ce_stream_t stream) {
    clear_error();
    V2CE_REQUIRE(ts && x && y && p && volume && t_range, V2CE_ERR_BAD_ARG, "v2ce_voxelize_events: null pointer");
    V2CE_REQUIRE(n > 0 && bins >= 2 && H > 0 && W > 0, V2CE_ERR_BAD_ARG,
                 "v2ce_voxelize_events: needs n > 0, bins >= 2, H, W > 0");
    hipStream_t st = as_stream(stream);
    const long long init[2] = {0x7fffffffffffffffll, -0x7fffffffffffffffll - 1};
    V2CE_HIP_CHECK(hipMemcpyAsync(t_range, init, sizeof(init), hipMemcpyHostToDevice, st));
    V2CE_HIP_CHECK(hipMemsetAsync(volume, 0, (size_t)2 * bins * H * W * sizeof(float), st));
    const long long nb = (n + 255) / 256;
    hipLaunchKernelGGL(time_range_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, st, ts, (long long)n,
                       reinterpret_cast<long long *>(t_range));
    hipLaunchKernelGGL(voxelize_kernel, dim3((unsigned)nb), dim3(256), 0, st, ts, x, y, p, (long long)n,
                       reinterpret_cast<const long long *>(t_range), bins, H, W, volume);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// v2ce_voxelize_batch: P event lists in one call, bit-identical to the reference's serial put_.
//
//   init -> range (+ coordinate check) -> status -> count -> scan -> scatter -> sort long buckets -> walk
//
// * Events are bucketed by (pair, half, pixel), half 1 for polarity <= 0, with an atomic count, a three-kernel
//   device-wide exclusive scan and an atomic scatter of the event indices (the tsdiff.hip scheme).
// * The scatter order inside a bucket is arbitrary, so each bucket's indices are put back in event order: buckets of
//   up to kSmall events by an insertion sort of the walking lane, longer ones by one workgroup each (bitonic tiles of
//   kTile in LDS, then merge passes in global memory inside that workgroup).
// * Walk: one lane per bucket visits its events twice, floor contributions then ceil contributions, into 16 register
//   accumulators (bins <= 16), and writes the bucket's `bins` cells.  This is the order put_(accumulate=True) adds in
//   on one thread, so every cell is the same f32 sum as the reference's; no float atomics.
namespace v2ce {
namespace {

constexpr int kVbThreads = 256;
constexpr int kVbSmall = 32;
constexpr int kVbTile = 4096;                 // LDS sort tile (int32): 16 KB
constexpr int kVbScanItems = 8;
constexpr int kVbScanBlock = kVbThreads * kVbScanItems;
constexpr int kVbMaxBins = 16;

struct VbParams {
    const int64_t *ts;
    const int16_t *x, *y;
    const int8_t *p;
    const int64_t *off;
    long long n;
    int P, bins, H, W;
    const int64_t *t_range;   // explicit [P][2] or null
    float *vol;
    int32_t *status;
    long long *range;         // [P][2]
    int *cnt, *start, *bsum;  // [ncells + 1], [ncells + 1], [nblocks]
    int *idx_a, *idx_b;       // event indices by bucket; idx_b: merge ping-pong
    int *longs, *nlong;       // buckets longer than kVbSmall
    int ncells;
    int halves = 2;           // 2: buckets (pair, polarity half, pixel); 1: (pair, pixel) -- the event-grid encoders below
    int skip_mask = -1;       // a pair whose status has one of these bits is not bucketed
};

__device__ __forceinline__ void pair_span(const VbParams &Q, int pair, long long &lo, long long &hi) {
    lo = Q.off[pair]; hi = Q.off[pair + 1];
    lo = lo < 0 ? 0 : (lo > Q.n ? Q.n : lo);
    hi = hi < lo ? lo : (hi > Q.n ? Q.n : hi);
}

__global__ __launch_bounds__(kVbThreads) void vb_init_kernel(VbParams Q) {
    const long long stride = (long long)gridDim.x * kVbThreads;
    for (long long i = (long long)blockIdx.x * kVbThreads + threadIdx.x; i <= Q.ncells; i += stride) {
        Q.cnt[i] = 0;
        if (i < Q.P) {
            Q.status[i] = 0;
            Q.range[2 * i] = Q.t_range ? (long long)Q.t_range[2 * i] : 0x7fffffffffffffffll;
            Q.range[2 * i + 1] = Q.t_range ? (long long)Q.t_range[2 * i + 1] : -0x7fffffffffffffffll - 1;
        }
        if (i == 0) *Q.nlong = 0;
    }
}

// grid (G, P): the time range of each pair (unless given) and its coordinate check
__global__ __launch_bounds__(kVbThreads) void vb_range_kernel(VbParams Q) {
    const int pair = blockIdx.y;
    long long lo, hi;
    pair_span(Q, pair, lo, hi);
    long long tmin = 0x7fffffffffffffffll, tmax = -0x7fffffffffffffffll - 1;
    int bad = 0;
    for (long long i = lo + (long long)blockIdx.x * kVbThreads + threadIdx.x; i < hi; i += (long long)gridDim.x * kVbThreads) {
        const long long t = Q.ts[i];
        tmin = t < tmin ? t : tmin;
        tmax = t > tmax ? t : tmax;
        const int xi = Q.x[i], yi = Q.y[i];
        if (xi < 0 || xi >= Q.W || yi < 0 || yi >= Q.H) bad = 1;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const long long a = __shfl_xor(tmin, o), b = __shfl_xor(tmax, o);
        tmin = a < tmin ? a : tmin;
        tmax = b > tmax ? b : tmax;
    }
    const bool any_bad = __any(bad);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (!Q.t_range && tmin <= tmax) {
            atomicMin(&Q.range[2 * pair], tmin);
            atomicMax(&Q.range[2 * pair + 1], tmax);
        }
        if (any_bad) atomicOr(&Q.status[pair], V2CE_VOXELIZE_BAD_XY);
    }
}

__global__ __launch_bounds__(kVbThreads) void vb_status_kernel(VbParams Q) {
    const int pair = blockIdx.x * kVbThreads + threadIdx.x;
    if (pair >= Q.P) return;
    long long lo, hi;
    pair_span(Q, pair, lo, hi);
    int s = Q.status[pair];
    const long long a = Q.range[2 * pair], b = Q.range[2 * pair + 1];
    if (hi == lo) s |= V2CE_VOXELIZE_EMPTY;
    else if (b == a) s |= V2CE_VOXELIZE_SINGLE_TIMESTAMP;
    else if (b < a) s |= V2CE_VOXELIZE_BAD_RANGE;
    Q.status[pair] = s;
}

__device__ __forceinline__ int vb_bucket(const VbParams &Q, int pair, long long i) {
    const int half = Q.halves == 2 && Q.p[i] <= 0;                                   // events_utils.py:153, :133-136
    return ((pair * Q.halves + half) * Q.H + Q.y[i]) * Q.W + Q.x[i];
}

__global__ __launch_bounds__(kVbThreads) void vb_count_kernel(VbParams Q) {
    const int pair = blockIdx.y;
    if (Q.status[pair] & Q.skip_mask) return;
    long long lo, hi;
    pair_span(Q, pair, lo, hi);
    for (long long i = lo + (long long)blockIdx.x * kVbThreads + threadIdx.x; i < hi; i += (long long)gridDim.x * kVbThreads)
        atomicAdd(&Q.cnt[vb_bucket(Q, pair, i)], 1);
}

__device__ __forceinline__ int vb_block_sum(int v, int *red) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    const int wv = threadIdx.x / kWave, nw = blockDim.x / kWave;
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) red[wv] = v;
    __syncthreads();
    int s = 0;
    for (int k = 0; k < nw; ++k) s += red[k];
    return s;
}

__device__ __forceinline__ int vb_block_exclusive(int v, int *red) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    int inc = v;
    for (int o = 1; o < kWave; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == kWave - 1) red[wv] = inc;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wv; ++k) before += red[k];
    return before + inc - v;
}

__global__ __launch_bounds__(kVbThreads) void vb_scan_reduce_kernel(VbParams Q) {
    __shared__ int red[kVbThreads / kWave];
    const long long base = (long long)blockIdx.x * kVbScanBlock + threadIdx.x * kVbScanItems;
    int s = 0;
#pragma unroll
    for (int k = 0; k < kVbScanItems; ++k)
        if (base + k <= Q.ncells) s += Q.cnt[base + k];
    s = vb_block_sum(s, red);
    if (threadIdx.x == 0) Q.bsum[blockIdx.x] = s;
}

__global__ __launch_bounds__(1024) void vb_scan_top_kernel(VbParams Q, int nb) {
    __shared__ int red[1024 / kWave];
    const int per = (nb + 1023) / 1024;
    const int lo = threadIdx.x * per, hi = min(nb, lo + per);
    int s = 0;
    for (int k = lo; k < hi; ++k) s += Q.bsum[k];
    int run = vb_block_exclusive(s, red);
    for (int k = lo; k < hi; ++k) {
        const int v = Q.bsum[k];
        Q.bsum[k] = run;
        run += v;
    }
}

__global__ __launch_bounds__(kVbThreads) void vb_scan_down_kernel(VbParams Q) {
    __shared__ int red[kVbThreads / kWave];
    const long long base = (long long)blockIdx.x * kVbScanBlock + threadIdx.x * kVbScanItems;
    int v[kVbScanItems], s = 0;
#pragma unroll
    for (int k = 0; k < kVbScanItems; ++k) {
        v[k] = base + k <= Q.ncells ? Q.cnt[base + k] : 0;
        s += v[k];
    }
    int run = Q.bsum[blockIdx.x] + vb_block_exclusive(s, red);
#pragma unroll
    for (int k = 0; k < kVbScanItems; ++k) {
        if (base + k <= Q.ncells) Q.start[base + k] = run;
        run += v[k];
    }
}

__global__ __launch_bounds__(kVbThreads) void vb_scatter_kernel(VbParams Q) {
    const int pair = blockIdx.y;
    if (Q.status[pair] & Q.skip_mask) return;
    long long lo, hi;
    pair_span(Q, pair, lo, hi);
    for (long long i = lo + (long long)blockIdx.x * kVbThreads + threadIdx.x; i < hi; i += (long long)gridDim.x * kVbThreads) {
        const int c = vb_bucket(Q, pair, i);
        Q.idx_a[Q.start[c] + atomicSub(&Q.cnt[c], 1) - 1] = (int)i;
    }
}

__global__ __launch_bounds__(kVbThreads) void vb_classify_kernel(VbParams Q) {
    for (int c = blockIdx.x * kVbThreads + threadIdx.x; c < Q.ncells; c += gridDim.x * kVbThreads)
        if (Q.start[c + 1] - Q.start[c] > kVbSmall) Q.longs[atomicAdd(Q.nlong, 1)] = c;
}

// one workgroup per long bucket: LDS bitonic tiles, then merge passes (idx_a <-> idx_b) inside the workgroup
__global__ __launch_bounds__(kVbThreads) void vb_sort_long_kernel(VbParams Q) {
    __shared__ int s[kVbTile];
    const int nl = *(volatile int *)Q.nlong;
    for (int e = blockIdx.x; e < nl; e += gridDim.x) {
        const int c = Q.longs[e];
        const int c0 = Q.start[c], n = Q.start[c + 1] - c0;
        int *a = Q.idx_a + c0, *b = Q.idx_b + c0;
        for (int t0 = 0; t0 < n; t0 += kVbTile) {
            const int m = min(kVbTile, n - t0);
            int w = 2;
            while (w < m) w <<= 1;
            for (int i = threadIdx.x; i < w; i += kVbThreads) s[i] = i < m ? a[t0 + i] : 0x7fffffff;
            __syncthreads();
            for (int k = 2; k <= w; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = threadIdx.x; i < w; i += kVbThreads) {
                        const int ixj = i ^ j;
                        if (ixj > i) {
                            const int u = s[i], v = s[ixj];
                            if ((u > v) == ((i & k) == 0)) { s[i] = v; s[ixj] = u; }
                        }
                    }
                    __syncthreads();
                }
            for (int i = threadIdx.x; i < m; i += kVbThreads) a[t0 + i] = s[i];
            __syncthreads();
        }
        // merge runs of width wd into 2 wd; indices are distinct, so ranks never tie
        int *src = a, *dst = b;
        for (long long wd = kVbTile; wd < n; wd <<= 1) {
            __threadfence();
            __syncthreads();
            for (long long j = threadIdx.x; j < n; j += kVbThreads) {
                const long long a0 = j / (2 * wd) * (2 * wd), a1 = min(a0 + wd, (long long)n), b1 = min(a0 + 2 * wd, (long long)n);
                const int v = src[j];
                long long lo, hi, r;
                if (j < a1) { lo = a1; hi = b1; } else { lo = a0; hi = a1; }
                while (lo < hi) { const long long mid = (lo + hi) >> 1; if (src[mid] < v) lo = mid + 1; else hi = mid; }
                r = j < a1 ? j - a0 + (lo - a1) : j - a1 + (lo - a0);
                dst[a0 + r] = v;
            }
            int *t = src; src = dst; dst = t;
        }
        __threadfence();
        __syncthreads();
        if (src != a)
            for (int i = threadIdx.x; i < n; i += kVbThreads) a[i] = src[i];
        __threadfence();
        __syncthreads();
    }
}

// one lane per bucket (pair, half, pixel): event order restored, floor then ceil contributions, `bins` cells written
__global__ __launch_bounds__(kVbThreads) void vb_walk_kernel(VbParams Q) {
    const long long HW = (long long)Q.H * Q.W;
    for (long long c = (long long)blockIdx.x * kVbThreads + threadIdx.x; c < Q.ncells; c += (long long)gridDim.x * kVbThreads) {
        const int pair = (int)(c / (2 * HW));
        const int half = (int)((c / HW) & 1);
        const long long pix = c % HW;
        const int c0 = Q.start[c], n = Q.start[c + 1] - c0;
        int *ix = Q.idx_a + c0;
        if (n > 1 && n <= kVbSmall)
            for (int k = 1; k < n; ++k) {
                const int v = ix[k];
                int j = k - 1;
                while (j >= 0 && ix[j] > v) { ix[j + 1] = ix[j]; --j; }
                ix[j + 1] = v;
            }
        float acc[kVbMaxBins];
#pragma unroll
        for (int q = 0; q < kVbMaxBins; ++q) acc[q] = 0.0f;
        if (n > 0) {
            const long long t_min = Q.range[2 * pair], t_max = Q.range[2 * pair + 1];
            const float scale = (1.0f / (float)(t_max - t_min)) * (float)(Q.bins - 1);   // events_utils.py:159
            const float top = (float)(Q.bins - 1);
            for (int pass = 0; pass < 2; ++pass)                                        // :164-168, then :170-173
                for (int k = 0; k < n; ++k) {
                    float t = (float)(Q.ts[ix[k]] - t_min) * scale;
                    t = fminf(fmaxf(t, 0.0f), top);                                     // :160
                    const float fl = floorf(t + 1e-8f);                                 // :119
                    float v;
                    int bin;
                    if (pass == 0) { v = (floorf(t) + 1.0f) - t; bin = (int)fl; }      // :121, :124
                    else { v = t - fl; bin = (int)ceilf(t - 1e-8f); }                   // :120, :123
#pragma unroll
                    for (int q = 0; q < kVbMaxBins; ++q) acc[q] = bin == q ? acc[q] + v : acc[q];
                }
        }
        float *out = Q.vol + ((long long)pair * 2 * Q.bins + (long long)half * Q.bins) * HW + pix;
#pragma unroll
        for (int q = 0; q < kVbMaxBins; ++q)
            if (q < Q.bins) out[(long long)q * HW] = acc[q];
    }
}

struct VbLayout {
    long long ncells, nblocks;
    size_t range, cnt, start, bsum, idx_a, idx_b, longs, nlong, total;
};

bool vb_layout(int P, int bins, int H, int W, long long n, VbLayout &L, int halves = 2, int min_bins = 2) {
    if (P < 1 || P > 65535 || bins < min_bins || bins > kVbMaxBins || H < 1 || W < 1 || H > 32767 || W > 32767) return false;
    if (n < 0 || n >= (1ll << 31)) return false;
    L.ncells = (long long)halves * P * H * W;
    if (L.ncells >= (1ll << 31) - 1) return false;
    L.nblocks = (L.ncells + 1 + kVbScanBlock - 1) / kVbScanBlock;
    const long long nlong_cap = n / (kVbSmall + 1) + 1;
    size_t o = 0;
    L.range = o; o += align_up256((size_t)P * 16);
    L.cnt = o;   o += align_up256((size_t)(L.ncells + 1) * 4);
    L.start = o; o += align_up256((size_t)(L.ncells + 1) * 4);
    L.bsum = o;  o += align_up256((size_t)L.nblocks * 4);
    L.idx_a = o; o += align_up256((size_t)n * 4 + 4);
    L.idx_b = o; o += align_up256((size_t)n * 4 + 4);
    L.longs = o; o += align_up256((size_t)nlong_cap * 4);
    L.nlong = o; o += 256;
    L.total = o;
    return true;
}

}  // namespace
}  // namespace v2ce

extern "C" size_t v2ce_voxelize_batch_workspace_bytes(int P, int bins, int H, int W, int64_t n) {
    VbLayout L;
    return vb_layout(P, bins, H, W, n, L) ? L.total : 0;
}

extern "C" int v2ce_voxelize_batch(const int64_t *ts, const int16_t *x, const int16_t *y, const int8_t *p,
                                   const int64_t *offsets, int64_t n, int P, int bins, int H, int W,
                                   const int64_t *t_range, float *volume, int32_t *status, void *workspace,
                                   size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    VbLayout L;
    V2CE_REQUIRE(vb_layout(P, bins, H, W, n, L), V2CE_ERR_BAD_ARG,
                 "v2ce_voxelize_batch: needs 1 <= P <= 65535, 2 <= bins <= %d, 1 <= H, W <= 32767, 2*P*H*W < 2^31 - 1 "
                 "and n in [0, 2^31)", kVbMaxBins);
    V2CE_REQUIRE(offsets && volume && status && workspace, V2CE_ERR_BAD_ARG, "v2ce_voxelize_batch: null pointer");
    V2CE_REQUIRE(n == 0 || (ts && x && y && p), V2CE_ERR_BAD_ARG, "v2ce_voxelize_batch: null event array");
    V2CE_REQUIRE(workspace_bytes >= L.total, V2CE_ERR_WORKSPACE, "v2ce_voxelize_batch: workspace too small (%zu < %zu)",
                 workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    VbParams Q{};
    Q.ts = ts; Q.x = x; Q.y = y; Q.p = p; Q.off = offsets; Q.n = n;
    Q.P = P; Q.bins = bins; Q.H = H; Q.W = W; Q.t_range = t_range; Q.vol = volume; Q.status = status;
    Q.range = reinterpret_cast<long long *>(ws + L.range);
    Q.cnt = reinterpret_cast<int *>(ws + L.cnt);
    Q.start = reinterpret_cast<int *>(ws + L.start);
    Q.bsum = reinterpret_cast<int *>(ws + L.bsum);
    Q.idx_a = reinterpret_cast<int *>(ws + L.idx_a);
    Q.idx_b = reinterpret_cast<int *>(ws + L.idx_b);
    Q.longs = reinterpret_cast<int *>(ws + L.longs);
    Q.nlong = reinterpret_cast<int *>(ws + L.nlong);
    Q.ncells = (int)L.ncells;
    Q.halves = 2;
    Q.skip_mask = -1;
    const long long cb = (L.ncells + kVbThreads) / kVbThreads;
    const unsigned cell_blocks = (unsigned)(cb < 8192 ? cb : 8192);
    long long per = (n / P + kVbThreads - 1) / kVbThreads;
    const unsigned ge = (unsigned)(per < 1 ? 1 : (per > 1024 ? 1024 : per));
    hipLaunchKernelGGL(vb_init_kernel, dim3(cell_blocks), dim3(kVbThreads), 0, st, Q);
    if (n > 0) hipLaunchKernelGGL(vb_range_kernel, dim3(ge, P), dim3(kVbThreads), 0, st, Q);
    hipLaunchKernelGGL(vb_status_kernel, dim3((unsigned)((P + kVbThreads - 1) / kVbThreads)), dim3(kVbThreads), 0, st, Q);
    if (n > 0) hipLaunchKernelGGL(vb_count_kernel, dim3(ge, P), dim3(kVbThreads), 0, st, Q);
    hipLaunchKernelGGL(vb_scan_reduce_kernel, dim3((unsigned)L.nblocks), dim3(kVbThreads), 0, st, Q);
    hipLaunchKernelGGL(vb_scan_top_kernel, dim3(1), dim3(1024), 0, st, Q, (int)L.nblocks);
    hipLaunchKernelGGL(vb_scan_down_kernel, dim3((unsigned)L.nblocks), dim3(kVbThreads), 0, st, Q);
    if (n > 0) {
        hipLaunchKernelGGL(vb_scatter_kernel, dim3(ge, P), dim3(kVbThreads), 0, st, Q);
        hipLaunchKernelGGL(vb_classify_kernel, dim3(cell_blocks), dim3(kVbThreads), 0, st, Q);
        if (n > kVbSmall) hipLaunchKernelGGL(vb_sort_long_kernel, dim3(512), dim3(kVbThreads), 0, st, Q);
    }
    hipLaunchKernelGGL(vb_walk_kernel, dim3(cell_blocks), dim3(kVbThreads), 0, st, Q);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// v2ce_event_grids_batch: the three other event -> grid encoders of events_utils.py on the bucket pipeline above.
//
//   init -> check (coordinates, time window, empty) -> count -> scan -> scatter -> [sort long buckets -> grid walk]
//        -> [stat walk -> zero the stat grids of flagged lists]
//
// * Both polarities of a pixel add into the SAME cells of the signed and the split grid (events_utils.py:107-112,
//   :251-256), so the buckets are (list, pixel): halves = 1.  All requested kinds read that one bucketing.
// * Grid walk: one lane per bucket, event order restored as in vb_walk_kernel, the left contributions in event order,
//   then the right ones: the order of the reference's two np.add.at calls.  Every add is
//   acc = (float)((double)acc + v) with v in f64, which is what np.add.at does to a float32 array given float64
//   values.  No float atomics.
// * Stat walk: one lane per (list, polarity plane, pixel) filters its plane out of the bucket and keeps, per bin, a
//   32-bit count and 64-bit integer sums of the residue and its square in registers.  Integer sums do not depend on
//   the order, so the stat grids need no sort; the reference's f64 sums are these integers exactly while sum(tr^2) <
//   2^53, beyond which the list is flagged instead of answered.  The f64 finalisation follows :354-356 operation by
//   operation (this file is built without FMA contraction).
namespace v2ce {
namespace {

constexpr int kEgFatal = V2CE_EVENT_GRIDS_EMPTY | V2CE_EVENT_GRIDS_BAD_XY | V2CE_EVENT_GRIDS_BAD_TIME;
constexpr int kEgStatBits = V2CE_EVENT_GRIDS_STAT_TOP_EDGE | V2CE_EVENT_GRIDS_STAT_OVERFLOW;
constexpr long long kEgTwo53 = 1ll << 53;
constexpr long long kEgMaxResidue = 94906265ll;     // floor(sqrt(2^53)): a larger residue squares to 2^53 or more

struct EgOut {
    float *signed_grid, *split_grid;
    double *count, *mean, *std;
};

__global__ __launch_bounds__(kVbThreads) void eg_init_kernel(VbParams Q) {
    const long long stride = (long long)gridDim.x * kVbThreads;
    for (long long i = (long long)blockIdx.x * kVbThreads + threadIdx.x; i <= Q.ncells; i += stride) {
        Q.cnt[i] = 0;
        if (i < Q.P) Q.status[i] = 0;
        if (i == 0) *Q.nlong = 0;
    }
}

// grid (G, P): an empty list (events[-1] raises, :87), coordinates outside H x W, a timestamp outside [first, last]
__global__ __launch_bounds__(kVbThreads) void eg_check_kernel(VbParams Q) {
    const int pair = blockIdx.y;
    long long lo, hi;
    pair_span(Q, pair, lo, hi);
    if (hi == lo) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&Q.status[pair], V2CE_EVENT_GRIDS_EMPTY);
        return;
    }
    const long long first = Q.ts[lo], last = Q.ts[hi - 1];                            // :87-88, :232-233, :334
    int bad = 0;
    for (long long i = lo + (long long)blockIdx.x * kVbThreads + threadIdx.x; i < hi; i += (long long)gridDim.x * kVbThreads) {
        const long long t = Q.ts[i];
        const int xi = Q.x[i], yi = Q.y[i];
        if (xi < 0 || xi >= Q.W || yi < 0 || yi >= Q.H) bad |= V2CE_EVENT_GRIDS_BAD_XY;
        if (t < first || t > last) bad |= V2CE_EVENT_GRIDS_BAD_TIME;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) bad |= __shfl_xor(bad, o);
    if ((threadIdx.x & (kWave - 1)) == 0 && bad) atomicOr(&Q.status[pair], bad);
}

// one lane per bucket (list, pixel): lefts in event order, then rights in event order (:107-112, :251-256)
template <bool SIGNED, bool SPLIT>
__global__ __launch_bounds__(kVbThreads) void eg_walk_grid_kernel(VbParams Q, EgOut O) {
    const long long HW = (long long)Q.H * Q.W;
    for (long long c = (long long)blockIdx.x * kVbThreads + threadIdx.x; c < Q.ncells; c += (long long)gridDim.x * kVbThreads) {
        const int pair = (int)(c / HW);
        const long long pix = c % HW;
        const int c0 = Q.start[c], n = Q.start[c + 1] - c0;
        int *ix = Q.idx_a + c0;
        if (n > 1 && n <= kVbSmall)
            for (int k = 1; k < n; ++k) {
                const int v = ix[k];
                int j = k - 1;
                while (j >= 0 && ix[j] > v) { ix[j + 1] = ix[j]; --j; }
                ix[j + 1] = v;
            }
        float acc[kVbMaxBins], accl[kVbMaxBins], accr[kVbMaxBins];      // signed | split plane 0 | split plane 1
#pragma unroll
        for (int q = 0; q < kVbMaxBins; ++q) acc[q] = accl[q] = accr[q] = 0.0f;
        if (n > 0) {
            long long lo, hi;
            pair_span(Q, pair, lo, hi);
            const long long first = Q.ts[lo], last = Q.ts[hi - 1];
            const double deltaT = last == first ? 1.0 : (double)(last - first);     // :89-92
            const double top = (double)(Q.bins - 1);
            for (int pass = 0; pass < 2; ++pass)
                for (int k = 0; k < n; ++k) {
                    const int e = ix[k];
                    const double ts = (top * (double)(Q.ts[e] - first)) / deltaT;   // :94, :239
                    const long long tis = (long long)ts;                            // :101 astype(int) truncates
                    const double dts = ts - (double)tis;                            // :102
                    const int pe = Q.p[e];
                    const double pol = pe == 0 ? -1.0 : (double)pe;                 // :99
                    const double v = pass == 0 ? pol * (1.0 - dts) : pol * dts;     // :103-104
                    const long long bin = pass == 0 ? tis : tis + 1;                // :106-112: bin >= bins is dropped
#pragma unroll
                    for (int q = 0; q < kVbMaxBins; ++q) {
                        if (SIGNED) acc[q] = bin == q ? (float)((double)acc[q] + v) : acc[q];
                        if (SPLIT && pass == 0) accl[q] = bin == q ? (float)((double)accl[q] + v) : accl[q];
                        if (SPLIT && pass == 1) accr[q] = bin == q ? (float)((double)accr[q] + v) : accr[q];
                    }
                }
        }
#pragma unroll
        for (int q = 0; q < kVbMaxBins; ++q)
            if (q < Q.bins) {
                if (SIGNED) O.signed_grid[((long long)pair * Q.bins + q) * HW + pix] = acc[q];
                if (SPLIT) {
                    O.split_grid[((long long)(pair * 2) * Q.bins + q) * HW + pix] = accl[q];
                    O.split_grid[((long long)(pair * 2 + 1) * Q.bins + q) * HW + pix] = accr[q];
                }
            }
    }
}

// sqrt(v) rounded to nearest for finite v >= 0, whatever the last bit of the device's sqrt: s is the correctly
// rounded root iff s * pred(s) < v <= s * succ(s) (the midpoints' squares lie strictly between multiples of the products'
// grid), and the sign of an fma residual is exact.  One step up or down covers a root that is off by one ulp.
__device__ __forceinline__ double eg_sqrt_rn(double v) {
    double s = sqrt(v);
    if (v > 0.0) {
        const double up = __longlong_as_double(__double_as_longlong(s) + 1);
        const double dn = __longlong_as_double(__double_as_longlong(s) - 1);
        if (fma(-s, up, v) > 0.0) s = up;
        else if (fma(-s, dn, v) <= 0.0) s = dn;
    }
    return s;
}

// one lane per (list, polarity plane, pixel): integer count, sum(tr), sum(tr^2) per bin, finalised in f64 (:334-356)
__global__ __launch_bounds__(kVbThreads) void eg_walk_stat_kernel(VbParams Q, EgOut O) {
    const long long HW = (long long)Q.H * Q.W;
    const long long total = 2ll * Q.ncells;
    for (long long g = (long long)blockIdx.x * kVbThreads + threadIdx.x; g < total; g += (long long)gridDim.x * kVbThreads) {
        const int pair = (int)(g / (2 * HW));
        const int plane = (int)((g / HW) & 1);
        const long long pix = g % HW;
        const long long c = (long long)pair * HW + pix;
        const int c0 = Q.start[c], n = Q.start[c + 1] - c0;
        const int *ix = Q.idx_a + c0;
        unsigned cnt[kVbMaxBins];
        unsigned long long sum[kVbMaxBins], sq[kVbMaxBins];
#pragma unroll
        for (int q = 0; q < kVbMaxBins; ++q) { cnt[q] = 0; sum[q] = 0; sq[q] = 0; }
        int flag = 0;
        if (n > 0) {
            long long lo, hi;
            pair_span(Q, pair, lo, hi);
            const long long first = Q.ts[lo], last = Q.ts[hi - 1];
            const long long delta_t = (long long)ceil((double)(last - first) / (double)Q.bins);      // :334
            for (int k = 0; k < n; ++k) {
                const int e = ix[k];
                if ((Q.p[e] == 1 ? 1 : 0) != plane) continue;                                       // :342
                const long long t = Q.ts[e] - first;                                                 // :336
                const long long tb = delta_t ? t / delta_t : 0, tr = delta_t ? t % delta_t : 0;      // :337-338, x // 0 = 0
                if (tb >= Q.bins) { flag |= V2CE_EVENT_GRIDS_STAT_TOP_EDGE; continue; }
                if (tr > kEgMaxResidue) { flag |= V2CE_EVENT_GRIDS_STAT_OVERFLOW; continue; }
                const unsigned long long r = (unsigned long long)tr, r2 = r * r;
#pragma unroll
                for (int q = 0; q < kVbMaxBins; ++q)
                    if (tb == q) {
                        cnt[q] += 1;
                        sum[q] += r;
                        if (sq[q] < (unsigned long long)kEgTwo53) sq[q] += r2;     // sticky at >= 2^53, never wraps
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < kVbMaxBins; ++q)
            if (q < Q.bins) {
                if (sq[q] >= (unsigned long long)kEgTwo53) flag |= V2CE_EVENT_GRIDS_STAT_OVERFLOW;
                const double N = (double)cnt[q], S = (double)sum[q], SS = (double)sq[q];
                const double d1 = N > 1.0 ? N : 1.0;                               // np.maximum(count, 1)
                const double d2 = N - 1.0 > 1.0 ? N - 1.0 : 1.0;                   // np.maximum(count - 1, 1)
                const double mean = S / d1;                                        // :354
                const double var = (SS - (S * S) / d1) / d2;                       // :355
                // :356; a negative variance is NaN there: the sign-set quiet NaN that NumPy's sqrt returns on x86-64
                const double sd = var < 0.0 ? __longlong_as_double((long long)0xfff8000000000000ull) : eg_sqrt_rn(var);
                const long long o = ((long long)(pair * 2 + plane) * Q.bins + q) * HW + pix;
                O.count[o] = N;
                O.mean[o] = mean;
                O.std[o] = sd;
            }
        if (flag) atomicOr(&Q.status[pair], flag);
    }
}

// grid (G, P): a list with a stat bit answers zero stat grids (its cells were written before the bit was known)
__global__ __launch_bounds__(kVbThreads) void eg_zero_stat_kernel(VbParams Q, EgOut O) {
    const int pair = blockIdx.y;
    if (!(Q.status[pair] & kEgStatBits)) return;
    const long long per = 2ll * Q.bins * Q.H * Q.W, base = per * pair;
    for (long long i = (long long)blockIdx.x * kVbThreads + threadIdx.x; i < per; i += (long long)gridDim.x * kVbThreads) {
        O.count[base + i] = 0.0;
        O.mean[base + i] = 0.0;
        O.std[base + i] = 0.0;
    }
}

}  // namespace
}  // namespace v2ce

extern "C" size_t v2ce_event_grids_workspace_bytes(int P, int bins, int H, int W, int64_t n, int kinds) {
    VbLayout L;
    if (kinds < 1 || kinds > 7) return 0;
    return vb_layout(P, bins, H, W, n, L, 1, 1) ? L.total : 0;
}

extern "C" int v2ce_event_grids_batch(const int64_t *ts, const int16_t *x, const int16_t *y, const int8_t *p,
                                      const int64_t *offsets, int64_t n, int P, int bins, int H, int W, int kinds,
                                      float *signed_grid, float *split_grid, double *count, double *mean, double *std,
                                      int32_t *status, void *workspace, size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    VbLayout L;
    V2CE_REQUIRE(kinds >= 1 && kinds <= 7, V2CE_ERR_BAD_ARG, "v2ce_event_grids_batch: kinds must be a non-empty mask of "
                 "V2CE_EVENT_GRIDS_SIGNED | _SPLIT | _STAT, got %d", kinds);
    V2CE_REQUIRE(vb_layout(P, bins, H, W, n, L, 1, 1), V2CE_ERR_BAD_ARG,
                 "v2ce_event_grids_batch: needs 1 <= P <= 65535, 1 <= bins <= %d, 1 <= H, W <= 32767, P*H*W < 2^31 - 1 "
                 "and n in [0, 2^31)", kVbMaxBins);
    const bool want_signed = kinds & V2CE_EVENT_GRIDS_SIGNED, want_split = kinds & V2CE_EVENT_GRIDS_SPLIT,
               want_stat = kinds & V2CE_EVENT_GRIDS_STAT;
    V2CE_REQUIRE(offsets && status && workspace, V2CE_ERR_BAD_ARG, "v2ce_event_grids_batch: null pointer");
    V2CE_REQUIRE((!want_signed || signed_grid) && (!want_split || split_grid) && (!want_stat || (count && mean && std)),
                 V2CE_ERR_BAD_ARG, "v2ce_event_grids_batch: null output of a requested kind");
    V2CE_REQUIRE(n == 0 || (ts && x && y && p), V2CE_ERR_BAD_ARG, "v2ce_event_grids_batch: null event array");
    V2CE_REQUIRE(workspace_bytes >= L.total, V2CE_ERR_WORKSPACE, "v2ce_event_grids_batch: workspace too small (%zu < %zu)",
                 workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    VbParams Q{};
    Q.ts = ts; Q.x = x; Q.y = y; Q.p = p; Q.off = offsets; Q.n = n;
    Q.P = P; Q.bins = bins; Q.H = H; Q.W = W; Q.status = status;
    Q.range = reinterpret_cast<long long *>(ws + L.range);
    Q.cnt = reinterpret_cast<int *>(ws + L.cnt);
    Q.start = reinterpret_cast<int *>(ws + L.start);
    Q.bsum = reinterpret_cast<int *>(ws + L.bsum);
    Q.idx_a = reinterpret_cast<int *>(ws + L.idx_a);
    Q.idx_b = reinterpret_cast<int *>(ws + L.idx_b);
    Q.longs = reinterpret_cast<int *>(ws + L.longs);
    Q.nlong = reinterpret_cast<int *>(ws + L.nlong);
    Q.ncells = (int)L.ncells;
    Q.halves = 1;
    Q.skip_mask = kEgFatal;
    EgOut O{signed_grid, split_grid, count, mean, std};
    const long long cb = (L.ncells + kVbThreads) / kVbThreads;
    const unsigned cell_blocks = (unsigned)(cb < 8192 ? cb : 8192);
    const unsigned stat_blocks = (unsigned)(2 * cb < 16384 ? 2 * cb : 16384);
    long long per = (n / P + kVbThreads - 1) / kVbThreads;
    const unsigned ge = (unsigned)(per < 1 ? 1 : (per > 1024 ? 1024 : per));
    hipLaunchKernelGGL(eg_init_kernel, dim3(cell_blocks), dim3(kVbThreads), 0, st, Q);
    hipLaunchKernelGGL(eg_check_kernel, dim3(ge, P), dim3(kVbThreads), 0, st, Q);
    if (n > 0) hipLaunchKernelGGL(vb_count_kernel, dim3(ge, P), dim3(kVbThreads), 0, st, Q);
    hipLaunchKernelGGL(vb_scan_reduce_kernel, dim3((unsigned)L.nblocks), dim3(kVbThreads), 0, st, Q);
    hipLaunchKernelGGL(vb_scan_top_kernel, dim3(1), dim3(1024), 0, st, Q, (int)L.nblocks);
    hipLaunchKernelGGL(vb_scan_down_kernel, dim3((unsigned)L.nblocks), dim3(kVbThreads), 0, st, Q);
    if (n > 0) hipLaunchKernelGGL(vb_scatter_kernel, dim3(ge, P), dim3(kVbThreads), 0, st, Q);
    if (want_signed || want_split) {                            // only the float grids depend on the event order
        if (n > 0) {
            hipLaunchKernelGGL(vb_classify_kernel, dim3(cell_blocks), dim3(kVbThreads), 0, st, Q);
            if (n > kVbSmall) hipLaunchKernelGGL(vb_sort_long_kernel, dim3(512), dim3(kVbThreads), 0, st, Q);
        }
        if (want_signed && want_split)
            hipLaunchKernelGGL((eg_walk_grid_kernel<true, true>), dim3(cell_blocks), dim3(kVbThreads), 0, st, Q, O);
        else if (want_signed)
            hipLaunchKernelGGL((eg_walk_grid_kernel<true, false>), dim3(cell_blocks), dim3(kVbThreads), 0, st, Q, O);
        else
            hipLaunchKernelGGL((eg_walk_grid_kernel<false, true>), dim3(cell_blocks), dim3(kVbThreads), 0, st, Q, O);
    }
    if (want_stat) {
        const long long zb = (2ll * bins * H * W + kVbThreads - 1) / kVbThreads;
        hipLaunchKernelGGL(eg_walk_stat_kernel, dim3(stat_blocks), dim3(kVbThreads), 0, st, Q, O);
        hipLaunchKernelGGL(eg_zero_stat_kernel, dim3((unsigned)(zb < 256 ? zb : 256), P), dim3(kVbThreads), 0, st, Q, O);
    }
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
