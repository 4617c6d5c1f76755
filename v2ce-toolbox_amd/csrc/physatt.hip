// physatt.hip -- physical-attention maps, ratio maps / top-K masks and log-frame residuals on gfx950.
//
// Replaces the array work of train/scripts/utils/physical_att.py for uint8 frames and the events of P frame pairs:
//
//   count_kernel     one lane per event: its pair from the offsets table (binary search), then one int32 atomic add on
//                    the pair's patch (y / pool, x / pool); a coordinate outside W x H raises the pair's flag instead.
//   delta_kernel     one lane per patch: |lut[b] - lut[a]| over the patch's pool x pool pixels, summed in the order of
//                    np.mean on skimage's block view (each block row with NumPy's pairwise inner loop, the row sums in
//                    row order), divided by pool^2.  Neighbouring lanes own neighbouring patches of one patch row, so a
//                    wave reads one contiguous 64 * pool byte span of a frame row per step; the order inside a patch is
//                    serial in NumPy as well, so a lane per patch loses nothing to it.
//   finish_kernel    one workgroup per pair, the whole [Hp, Wp] map in LDS: ratio, clip, the two passes of
//                    scipy.ndimage.gaussian_filter(sigma = 1) in f64, clip, min / max, normalisation; or the ratio map
//                    of physical_mask_generation and its K-th largest value by a four-pass radix select.
//   residual_kernel  lut[f[i + 1]] - lut[f[i]], four pixels per lane.
//
// lin_log takes 256 arguments on uint8 frames: the host passes it as a float32 table, no kernel calls log.  All counting
// is integer (global int32 atomics on the patches, LDS atomics for min / max / the select's histograms): integer adds
// commute, so the bytes do not depend on the run or on what else is in the batch.  No float atomic anywhere.
// Built with the EXACT flags (no contraction, correctly rounded division).
#include "common.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;          // grid-stride cap: eight workgroups per CU
constexpr int kMaxCells = 6144;           // finish_kernel: two f32 maps in LDS = 48 KiB (260 x 346 at pool 4: 5 655 cells)
constexpr int kMaxPool = 16;
constexpr int kBlurRadius = 4;
static_assert(kThreads == 256, "finish_kernel: one lane per bin of the select's histogram");

unsigned blocks_for(long long items) {
    const long long nb = (items + kThreads - 1) / kThreads;
    return (unsigned)(nb < 1 ? 1 : (nb > kMaxBlocks ? kMaxBlocks : nb));
}

// ---- events -> int32 counts per (pair, patch) -------------------------------------------------------------------------

// safe for ANY offsets table: the pair index always lies in [0, P), an event outside [off[0], off[P]) is skipped
__global__ __launch_bounds__(kThreads) void count_kernel(const int16_t *__restrict__ x, const int16_t *__restrict__ y,
                                                         const int64_t *__restrict__ off, long long n, int P, int H,
                                                         int W, int pool, int Wp, int cells, int *__restrict__ counts,
                                                         int *__restrict__ flags) {
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
        if (e < off[0] || e >= off[P]) continue;
        int lo = 0, hi = P;                                   // the largest i in [0, P) with off[i] <= e
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= e) lo = mid; else hi = mid;
        }
        const int ex = x[e], ey = y[e];
        if (ex < 0 || ex >= W || ey < 0 || ey >= H) {
            atomicOr(flags + lo, V2CE_PHYSATT_BAD_XY);
            continue;
        }
        atomicAdd(counts + (long long)lo * cells + (ey / pool) * Wp + ex / pool, 1);
    }
}

// ---- frames -> patch means of |lut[b] - lut[a]| (/ threshold in the RATIO mode) ---------------------------------------

template <bool kRatio>
__global__ __launch_bounds__(kThreads) void delta_kernel(const uint8_t *__restrict__ frames, long long pair_stride, int H,
                                                         int W, int pool, int Wp, int cells, long long total,
                                                         const float *__restrict__ lut_g, float threshold,
                                                         float *__restrict__ delta) {
    __shared__ float lut[256];
    for (int i = threadIdx.x; i < 256; i += kThreads) lut[i] = lut_g[i];
    __syncthreads();
    const long long HW = (long long)H * W;
    const float area = (float)(pool * pool);
    for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < total; g += (long long)gridDim.x * kThreads) {
        const long long pair = g / cells;
        const int c = (int)(g - pair * cells), py = c / Wp, px = c - py * Wp;
        const uint8_t *fa = frames + pair * pair_stride, *fb = fa + HW;
        const int x0 = px * pool, y0 = py * pool;
        float acc = 0.0f;
        for (int r = 0; r < pool; ++r) {
            float v[kMaxPool];
            const int yy = y0 + r;
            const long long row = (long long)yy * W;
#pragma unroll
            for (int j = 0; j < kMaxPool; ++j) {
                float d = 0.0f;                              // the zero padding of block_reduce
                if (j < pool && yy < H && x0 + j < W) {
                    d = fabsf(lut[fb[row + x0 + j]] - lut[fa[row + x0 + j]]);
                    if (kRatio) d = d / threshold;
                }
                v[j] = d;
            }
            float s;                                          // NumPy's pairwise inner loop for n = pool <= 16
            if (pool < 8) {
                s = 0.0f;
#pragma unroll
                for (int j = 0; j < 7; ++j)
                    if (j < pool) s = s + v[j];
            } else {
                float q[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) q[j] = v[j];
                if (pool == 16) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) q[j] = q[j] + v[8 + j];
                }
                s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
                if (pool < 16) {
#pragma unroll
                    for (int j = 8; j < 15; ++j)
                        if (j < pool) s = s + v[j];
                }
            }
            acc = acc + s;
        }
        delta[g] = acc / area;
    }
}

// ---- one workgroup per pair: the map in LDS ---------------------------------------------------------------------------

// floats as unsigned keys of the same order (-0 below +0, which the callers never mix)
__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// numpy's 'symmetric' / scipy's 'reflect': d c b a | a b c d | d c b a, repeated for a side shorter than the radius
__device__ __forceinline__ int reflect(int i, int n) {
    int m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// scipy's correlate1d, symmetric weights: the centre tap, then the tap pairs from the outermost inwards, in f64
__device__ __forceinline__ void blur_pass(const float *__restrict__ src, float *__restrict__ dst, int Hp, int Wp,
                                          bool along_y, const double *w) {
    const int cells = Hp * Wp, n = along_y ? Hp : Wp, stride = along_y ? Wp : 1;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int yy = c / Wp, xx = c - yy * Wp;
        const int i = along_y ? yy : xx, base = c - i * stride;
        double t = (double)src[c] * w[0];
#pragma unroll
        for (int j = kBlurRadius; j >= 1; --j)
            t = t + ((double)src[base + reflect(i - j, n) * stride] + (double)src[base + reflect(i + j, n) * stride]) * w[j];
        dst[c] = (float)t;
    }
}

struct GaussW { double w[kBlurRadius + 1]; };

__global__ __launch_bounds__(kThreads) void finish_kernel(const int *__restrict__ counts, const float *__restrict__ delta,
                                                          const int *__restrict__ flags, const int64_t *__restrict__ off,
                                                          long long n, int Hp, int Wp, int pool, int mode, float ceiling,
                                                          int K, GaussW gw, float *__restrict__ out_map,
                                                          uint8_t *__restrict__ out_mask, int *__restrict__ status) {
    __shared__ float A[kMaxCells], B[kMaxCells];
    __shared__ unsigned hist[256];
    __shared__ unsigned s_lo, s_hi, s_prefix;
    __shared__ int s_status, s_k;
    const int pair = blockIdx.x, cells = Hp * Wp, tid = threadIdx.x;
    const long long base = (long long)pair * cells;
    const float area = (float)(pool * pool);
    if (tid == 0) {
        const long long o0 = off[pair], o1 = off[pair + 1];
        s_status = flags[pair] | ((o0 < 0 || o1 < o0 || o1 > n) ? V2CE_PHYSATT_BAD_OFFSETS : 0);
        s_lo = 0xffffffffu;
        s_hi = 0u;
    }
    __syncthreads();
    for (int c = tid; c < cells; c += kThreads) {
        const int cnt = counts[base + c];
        if (cnt >= (1 << 24)) atomicOr(&s_status, V2CE_PHYSATT_COUNT_OVERFLOW);
        float ev = (float)cnt / area;
        float r;
        if (mode == V2CE_PHYSATT_RATIO) {
            r = ev / (delta[base + c] + 1e-6f) - 1.0f;
        } else {
            if (ev < 0.05f) ev = 0.0f;
            r = ev / (delta[base + c] + 1e-3f);
            r = fminf(fmaxf(r, 0.0f), 2.0f * ceiling);
        }
        A[c] = r;
    }
    __syncthreads();
    const int st = s_status;
    if (tid == 0) status[pair] = st;
    if (st != 0) {                                            // uniform: the pair's outputs are zeros
        for (int c = tid; c < cells; c += kThreads) {
            out_map[base + c] = 0.0f;
            if (out_mask) out_mask[base + c] = 0;
        }
        return;
    }
    if (mode == V2CE_PHYSATT_RATIO) {
        for (int c = tid; c < cells; c += kThreads) out_map[base + c] = A[c];
        if (K <= 0 || !out_mask) return;
        // the K-th largest value: four radix passes over the keys, most significant byte first
        if (tid == 0) { s_prefix = 0u; s_k = K; }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            hist[tid] = 0u;                                   // kThreads == 256 bins
            __syncthreads();
            const unsigned prefix = s_prefix;
            for (int c = tid; c < cells; c += kThreads) {
                const unsigned k = key_of(A[c] + 0.0f);
                if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int k = s_k, b = 255;
                while (b > 0 && (int)hist[b] < k) { k -= (int)hist[b]; --b; }
                s_k = k;
                s_prefix = (prefix << 8) | (unsigned)b;
            }
            __syncthreads();
        }
        const float kth = value_of(s_prefix);
        for (int c = tid; c < cells; c += kThreads) out_mask[base + c] = A[c] >= kth ? 1 : 0;
        return;
    }
    blur_pass(A, B, Hp, Wp, true, gw.w);
    __syncthreads();
    blur_pass(B, A, Hp, Wp, false, gw.w);
    __syncthreads();
    for (int c = tid; c < cells; c += kThreads) {
        const float v = fminf(fmaxf(A[c], 0.0f), ceiling);
        A[c] = v;
        const unsigned k = key_of(v + 0.0f);
        atomicMin(&s_lo, k);
        atomicMax(&s_hi, k);
    }
    __syncthreads();
    const float lo = value_of(s_lo), hi = value_of(s_hi);
    const float span = hi - lo;
    for (int c = tid; c < cells; c += kThreads) {
        float v = 0.0f;
        if (hi != lo) v = mode == V2CE_PHYSATT_ADVANCED ? (A[c] - lo) / span : A[c] / ceiling;
        out_map[base + c] = v;
    }
}

// ---- log-frame residual -----------------------------------------------------------------------------------------------

// a lane owns outputs 4k .. 4k+3 of the flat [N - 1][H * W] result; kVec: H * W % 4 == 0 and aligned bases
template <bool kVec>
__global__ __launch_bounds__(kThreads) void residual_kernel(const uint8_t *__restrict__ frames, long long HW,
                                                            long long total, const float *__restrict__ lut_g,
                                                            float *__restrict__ out) {
    __shared__ float lut[256];
    for (int i = threadIdx.x; i < 256; i += kThreads) lut[i] = lut_g[i];
    __syncthreads();
    const long long groups = (total + 3) >> 2;
    for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kThreads) {
        const long long q = g * 4;
        if (kVec) {
            const uchar4 a = *reinterpret_cast<const uchar4 *>(frames + q);
            const uchar4 b = *reinterpret_cast<const uchar4 *>(frames + q + HW);
            *reinterpret_cast<float4 *>(out + q) = make_float4(lut[b.x] - lut[a.x], lut[b.y] - lut[a.y],
                                                               lut[b.z] - lut[a.z], lut[b.w] - lut[a.w]);
        } else {
            for (int j = 0; j < 4; ++j)
                if (q + j < total) out[q + j] = lut[frames[q + j + HW]] - lut[frames[q + j]];
        }
    }
}

struct Shape { int Hp, Wp, cells; };

// false for a shape the entries refuse
bool shape_of(int P, int H, int W, int pool, int64_t n, Shape *s) {
    if (P < 1 || H < 1 || W < 1 || H > 32767 || W > 32767 || pool < 2 || pool > kMaxPool || n < 0 || n >= (1ll << 31))
        return false;
    s->Hp = (H + pool - 1) / pool;
    s->Wp = (W + pool - 1) / pool;
    const long long cells = (long long)s->Hp * s->Wp;
    if (cells > kMaxCells || (long long)P * cells >= (1ll << 31)) return false;
    s->cells = (int)cells;
    return true;
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_physatt_workspace_bytes(int P, int H, int W, int pool_size, int64_t n_events) {
    Shape s;
    if (!shape_of(P, H, W, pool_size, n_events, &s)) return 0;
    // int32 counts [P][cells] | int32 flags [P] | f32 patch means [P][cells]
    return pad16(((size_t)P * s.cells + P) * 4) + pad16((size_t)P * s.cells * 4);
}

extern "C" int v2ce_physatt_batch(const uint8_t *frames_u8, int pair_stride, int P, int H, int W, const int16_t *x,
                                  const int16_t *y, const int64_t *offsets, int64_t n, int pool_size, int mode,
                                  float ceiling, float threshold, int K, const float *lut, const double *gauss_w_host,
                                  float *out_map, uint8_t *out_mask, int32_t *status, void *workspace,
                                  size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    V2CE_REQUIRE(P >= 1 && H >= 1 && W >= 1 && n >= 0, V2CE_ERR_BAD_ARG,
                 "v2ce_physatt_batch: needs P, H, W >= 1 and n >= 0 (got %d, %d, %d, %lld)", P, H, W, (long long)n);
    V2CE_REQUIRE(mode == V2CE_PHYSATT_PLAIN || mode == V2CE_PHYSATT_ADVANCED || mode == V2CE_PHYSATT_RATIO, V2CE_ERR_BAD_ARG,
                 "v2ce_physatt_batch: mode %d is none of V2CE_PHYSATT_PLAIN, _ADVANCED, _RATIO", mode);
    V2CE_REQUIRE(pair_stride == 1 || pair_stride == 2, V2CE_ERR_BAD_ARG,
                 "v2ce_physatt_batch: pair_stride is 1 (a clip [P+1][H][W]) or 2 (pairs [P][2][H][W]) frames, got %d", pair_stride);
    Shape s;
    V2CE_REQUIRE(shape_of(P, H, W, pool_size, n, &s), V2CE_ERR_UNSUPPORTED,
                 "v2ce_physatt_batch: unsupported shape: pool_size in [2, %d], ceil(H / pool) * ceil(W / pool) <= %d, H, W <= "
                 "32767, n < 2^31 (got P = %d, H = %d, W = %d, pool_size = %d, n = %lld)", kMaxPool, kMaxCells, P, H, W,
                 pool_size, (long long)n);
    V2CE_REQUIRE(frames_u8 && offsets && lut && out_map && status && workspace && (n == 0 || (x && y)), V2CE_ERR_BAD_ARG,
                 "v2ce_physatt_batch: null pointer");
    if (mode == V2CE_PHYSATT_RATIO) {
        V2CE_REQUIRE(threshold > 0.0f && threshold <= 3.40282347e38f, V2CE_ERR_BAD_ARG,
                     "v2ce_physatt_batch: threshold must be positive and finite (got %g)", (double)threshold);
        V2CE_REQUIRE(K >= 0 && K <= s.cells && (K == 0 || out_mask), V2CE_ERR_BAD_ARG,
                     "v2ce_physatt_batch: K must lie in [0, %d] and needs out_mask when positive (got %d)", s.cells, K);
    } else {
        V2CE_REQUIRE(gauss_w_host, V2CE_ERR_BAD_ARG, "v2ce_physatt_batch: null gauss_w");
        V2CE_REQUIRE(ceiling > 0.0f && ceiling <= 1.0e38f, V2CE_ERR_BAD_ARG,
                     "v2ce_physatt_batch: ceiling must be positive and finite (got %g)", (double)ceiling);
    }
    V2CE_REQUIRE(workspace_bytes >= v2ce_physatt_workspace_bytes(P, H, W, pool_size, n), V2CE_ERR_WORKSPACE,
                 "v2ce_physatt_batch: workspace of %zu bytes, needs %zu", workspace_bytes,
                 v2ce_physatt_workspace_bytes(P, H, W, pool_size, n));
    V2CE_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, V2CE_ERR_BAD_ARG,
                 "v2ce_physatt_batch: workspace must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    const size_t int_bytes = pad16(((size_t)P * s.cells + P) * 4);
    int *counts = static_cast<int *>(workspace);
    int *flags = counts + (size_t)P * s.cells;
    float *delta = reinterpret_cast<float *>(static_cast<char *>(workspace) + int_bytes);
    V2CE_HIP_CHECK(hipMemsetAsync(counts, 0, int_bytes, st));
    if (n > 0)
        hipLaunchKernelGGL(count_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, x, y, offsets, (long long)n, P, H, W,
                           pool_size, s.Wp, s.cells, counts, flags);
    const long long total = (long long)P * s.cells, stride_px = (long long)pair_stride * H * W;
    if (mode == V2CE_PHYSATT_RATIO)
        hipLaunchKernelGGL((delta_kernel<true>), dim3(blocks_for(total)), dim3(kThreads), 0, st, frames_u8, stride_px, H, W,
                           pool_size, s.Wp, s.cells, total, lut, threshold, delta);
    else
        hipLaunchKernelGGL((delta_kernel<false>), dim3(blocks_for(total)), dim3(kThreads), 0, st, frames_u8, stride_px, H, W,
                           pool_size, s.Wp, s.cells, total, lut, threshold, delta);
    GaussW gw = {};
    if (mode != V2CE_PHYSATT_RATIO)
        for (int j = 0; j <= kBlurRadius; ++j) gw.w[j] = gauss_w_host[j];
    hipLaunchKernelGGL(finish_kernel, dim3(P), dim3(kThreads), 0, st, counts, delta, flags, offsets, (long long)n, s.Hp, s.Wp,
                       pool_size, mode, ceiling, K, gw, out_map, out_mask, status);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

extern "C" int v2ce_log_residual_batch(const uint8_t *frames_u8, int N, int H, int W, const float *lut, float *out,
                                       v2ce_stream_t stream) {
    clear_error();
    V2CE_REQUIRE(N >= 2 && H >= 1 && W >= 1, V2CE_ERR_BAD_ARG,
                 "v2ce_log_residual_batch: needs N >= 2 and H, W >= 1 (got %d, %d, %d)", N, H, W);
    V2CE_REQUIRE(frames_u8 && lut && out, V2CE_ERR_BAD_ARG, "v2ce_log_residual_batch: null pointer");
    const long long HW = (long long)H * W, total = (long long)(N - 1) * HW;
    V2CE_REQUIRE(total < (1ll << 40), V2CE_ERR_UNSUPPORTED, "v2ce_log_residual_batch: (N - 1) * H * W must stay below 2^40");
    const bool vec = HW % 4 == 0 && reinterpret_cast<uintptr_t>(frames_u8) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const dim3 grid(blocks_for((total + 3) >> 2)), block(kThreads);
    hipStream_t st = as_stream(stream);
    if (vec) hipLaunchKernelGGL((residual_kernel<true>), grid, block, 0, st, frames_u8, HW, total, lut, out);
    else hipLaunchKernelGGL((residual_kernel<false>), grid, block, 0, st, frames_u8, HW, total, lut, out);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
