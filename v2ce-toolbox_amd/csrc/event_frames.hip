// event_frames.hip -- the event-frame video's numeric stage on gfx950: sums, exact order statistics, uint8 frames.
//
// Replaces the array work of write_event_frame_video (v2ce.py:253-269,275-276) for voxels [P, 2, 10, H, W] f32:
//
//   sums_kernel    S [P, 3, H, W]: S0 / S1 = the ten bins of a polarity added in plane order, S2 = all twenty planes
//                  added in plane order, each in f32 starting from the first plane (pipeline.event_frame_sums bit for
//                  bit; S2 is not S0 + S1).  The same pass counts the positive values of the mode's channels (S0 and
//                  S1, or S2) into a clip-wide histogram keyed by bits 30..20 of the f32 pattern.
//   refine_kernel  counts, over stored sums, the next ten bits of the values whose leading bits equal one of two given
//                  prefixes: level 1 = bits 19..10 under an 11-bit prefix, level 2 = bits 9..0 under a 21-bit prefix.
//                  Two prefixes because the percentile needs two ranks, which may sit in different bins.
//   render_kernel  S + upper -> uint8 [L, H, W, 3] RGB at the pairs' places in the clip's buffer:
//                  trunc(min(max(x, 0), upper) / upper * 255), in f64 for the polarity mode (red = S0, green = S1,
//                  blue = 0) and in f32 for the grey mode (S2 three times), division and product rounded separately.
//
// Positive IEEE floats order like their bit patterns, so three histograms (11 + 10 + 10 bits) fix the value at any rank
// exactly.  All counting is integer: u32 per workgroup in LDS, then one u64 atomic per non-empty bin.  Integer adds
// commute, so a histogram does not depend on batching, batch order, launch shape or run, and two partial histograms add
// up to the histogram of the union.  A value counts when v > 0 (NaN and zeros never do).  Built with the EXACT flags.
#include "common.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;          // grid-stride cap: eight workgroups per CU
constexpr int kL1Bins = V2CE_EVENT_FRAMES_LEVEL0_BINS;
constexpr int kRefBins = V2CE_EVENT_FRAMES_REFINE_BINS;
static_assert(kL1Bins == 2048 && kRefBins == 1024, "31 bits = 11 + 10 + 10");

template <bool kVec>
__device__ __forceinline__ void load4(const float *__restrict__ p, int i0, int HW, float *v) {
    if (kVec) {
        const float4 a = *reinterpret_cast<const float4 *>(p);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < HW ? p[j] : 0.0f;
    }
}

template <bool kVec>
__device__ __forceinline__ void store4(float *__restrict__ p, int i0, int HW, const float *v) {
    if (kVec) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < HW) p[j] = v[j];
    }
}

__device__ __forceinline__ void flush_bins(const unsigned *lh, unsigned long long *__restrict__ hist, int bins) {
    for (int i = threadIdx.x; i < bins; i += kThreads) {
        const unsigned c = lh[i];
        if (c) atomicAdd(hist + i, (unsigned long long)c);
    }
}

// a lane owns four consecutive pixels of one pair; kVec: H * W % 4 == 0 and 16-B aligned bases
template <bool kVec, bool kHist>
__global__ __launch_bounds__(kThreads) void sums_kernel(const float *__restrict__ vox, float *__restrict__ sums, int HW,
                                                        int gpp, long long total_groups, int mode,
                                                        unsigned long long *__restrict__ hist) {
    __shared__ unsigned lh[kHist ? kL1Bins : 1];
    if (kHist) {
        for (int i = threadIdx.x; i < kL1Bins; i += kThreads) lh[i] = 0u;
        __syncthreads();
    }
    for (long long g = (long long)blockIdx.x * kThreads + threadIdx.x; g < total_groups;
         g += (long long)gridDim.x * kThreads) {
        const long long pair = g / gpp;
        const int i0 = (int)(g - pair * gpp) * 4;
        const float *base = vox + pair * 20 * HW + i0;
        float v[20][4];
#pragma unroll
        for (int c = 0; c < 20; ++c) load4<kVec>(base + (long long)c * HW, i0, HW, v[c]);
        float s0[4], s1[4], s2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = v[0][j];
#pragma unroll
            for (int c = 1; c < 10; ++c) a = a + v[c][j];
            float b = v[10][j];
#pragma unroll
            for (int c = 11; c < 20; ++c) b = b + v[c][j];
            float t = a;                      // the first ten steps of S2 are the steps of S0
#pragma unroll
            for (int c = 10; c < 20; ++c) t = t + v[c][j];
            s0[j] = a; s1[j] = b; s2[j] = t;
        }
        float *out = sums + pair * 3 * HW + i0;
        store4<kVec>(out, i0, HW, s0);
        store4<kVec>(out + HW, i0, HW, s1);
        store4<kVec>(out + 2ll * HW, i0, HW, s2);
        if (kHist) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!kVec && i0 + j >= HW) continue;
                if (mode == V2CE_EVENT_FRAMES_POLARITY) {
                    if (s0[j] > 0.0f) atomicAdd(&lh[__float_as_uint(s0[j]) >> 20], 1u);
                    if (s1[j] > 0.0f) atomicAdd(&lh[__float_as_uint(s1[j]) >> 20], 1u);
                } else if (s2[j] > 0.0f) {
                    atomicAdd(&lh[__float_as_uint(s2[j]) >> 20], 1u);
                }
            }
        }
    }
    if (kHist) {
        __syncthreads();
        flush_bins(lh, hist, kL1Bins);
    }
}

// one value per lane and step over the mode's channels of every pair (a contiguous span of each pair's sums)
__global__ __launch_bounds__(kThreads) void refine_kernel(const float *__restrict__ sums, int HW, int span, int first,
                                                          long long total, int key_shift, int bin_shift,
                                                          unsigned prefix_a, unsigned prefix_b,
                                                          unsigned long long *__restrict__ hist) {
    __shared__ unsigned lh[2 * kRefBins];
    for (int i = threadIdx.x; i < 2 * kRefBins; i += kThreads) lh[i] = 0u;
    __syncthreads();
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
        const long long pair = e / span;
        const float v = sums[pair * 3 * HW + first + (e - pair * span)];
        if (!(v > 0.0f)) continue;
        const unsigned bits = __float_as_uint(v);
        const unsigned key = bits >> key_shift, bin = (bits >> bin_shift) & (kRefBins - 1);
        if (key == prefix_a) atomicAdd(&lh[bin], 1u);
        if (key == prefix_b) atomicAdd(&lh[kRefBins + bin], 1u);
    }
    __syncthreads();
    flush_bins(lh, hist, 2 * kRefBins);
}

__device__ __forceinline__ unsigned to_u8(double s, double upper) {
    double x = s > 0.0 ? s : 0.0;
    x = x <= upper ? x : upper;
    const double t = x / upper;
    return (unsigned)(int)(t * 255.0);
}
__device__ __forceinline__ unsigned to_u8(float s, float upper) {
    float x = s > 0.0f ? s : 0.0f;
    x = x <= upper ? x : upper;
    const float t = x / upper;
    return (unsigned)(int)(t * 255.0f);
}

// a lane owns pixels 4k .. 4k+3 of the CLIP (twelve bytes = three whole dwords of the 4-B aligned frame buffer); only a
// group that straddles the ends of this batch's pixel range [q_lo, q_hi) falls back to byte stores
template <bool kVec, bool kPolarity>
__global__ __launch_bounds__(kThreads) void render_kernel(const float *__restrict__ sums, int HW, long long q_lo,
                                                          long long q_hi, double upper, uint8_t *__restrict__ frames) {
    const long long k_lo = q_lo >> 2, k_hi = (q_hi + 3) >> 2;
    const float upper32 = (float)upper;
    for (long long k = k_lo + (long long)blockIdx.x * kThreads + threadIdx.x; k < k_hi;
         k += (long long)gridDim.x * kThreads) {
        const long long q0 = k * 4;
        float a[4], b[4];
        if (kVec) {                            // HW % 4 == 0: the group lies in one pair at a multiple of four
            const long long local = q0 - q_lo, pair = local / HW;
            const float *p = sums + pair * 3 * HW + (local - pair * HW);
            if (kPolarity) { load4<true>(p, 0, HW, a); load4<true>(p + HW, 0, HW, b); }
            else load4<true>(p + 2ll * HW, 0, HW, a);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long q = q0 + j;
                a[j] = b[j] = 0.0f;
                if (q < q_lo || q >= q_hi) continue;
                const long long local = q - q_lo, pair = local / HW;
                const float *p = sums + pair * 3 * HW + (local - pair * HW);
                if (kPolarity) { a[j] = p[0]; b[j] = p[HW]; }
                else a[j] = p[2ll * HW];
            }
        }
        unsigned px[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (kPolarity) {
                px[3 * j] = to_u8((double)a[j], upper);
                px[3 * j + 1] = to_u8((double)b[j], upper);
                px[3 * j + 2] = 0u;
            } else {
                px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = to_u8(a[j], upper32);
            }
        }
        uint8_t *out = frames + q0 * 3;
        if (q0 >= q_lo && q0 + 4 <= q_hi) {
            unsigned *o32 = reinterpret_cast<unsigned *>(out);
#pragma unroll
            for (int d = 0; d < 3; ++d)
                o32[d] = px[4 * d] | (px[4 * d + 1] << 8) | (px[4 * d + 2] << 16) | (px[4 * d + 3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (q0 + j < q_lo || q0 + j >= q_hi) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c) out[3 * j + c] = (uint8_t)px[3 * j + c];
            }
        }
    }
}

unsigned blocks_for(long long items) {
    const long long nb = (items + kThreads - 1) / kThreads;
    return (unsigned)(nb < 1 ? 1 : (nb > kMaxBlocks ? kMaxBlocks : nb));
}

// V2CE_OK, or the error code with the message set; what: the entry's name
int check_shape(const char *what, int P, int H, int W, int mode) {
    V2CE_REQUIRE(P >= 1 && H >= 1 && W >= 1, V2CE_ERR_BAD_ARG, "%s: needs P, H, W >= 1 (got %d, %d, %d)", what, P, H, W);
    V2CE_REQUIRE(mode == V2CE_EVENT_FRAMES_POLARITY || mode == V2CE_EVENT_FRAMES_GREY, V2CE_ERR_BAD_ARG,
                 "%s: mode %d is neither V2CE_EVENT_FRAMES_POLARITY nor V2CE_EVENT_FRAMES_GREY", what, mode);
    V2CE_REQUIRE((long long)H * W < (1ll << 28) && (long long)P * 20 * H * W < (1ll << 33), V2CE_ERR_UNSUPPORTED,
                 "%s: H * W must stay below 2^28 and P * 20 * H * W below 2^33 (got P = %d, H = %d, W = %d)", what, P, H, W);
    return V2CE_OK;
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_event_frames_hist_bytes(int level) {
    if (level == 0) return (size_t)kL1Bins * sizeof(uint64_t);
    if (level == 1 || level == 2) return (size_t)2 * kRefBins * sizeof(uint64_t);
    return 0;
}

extern "C" int v2ce_event_frames_sums(const float *vox, int P, int H, int W, int mode, float *sums, uint64_t *hist,
                                      v2ce_stream_t stream) {
    clear_error();
    if (int rc = check_shape("v2ce_event_frames_sums", P, H, W, mode)) return rc;
    V2CE_REQUIRE(vox && sums, V2CE_ERR_BAD_ARG, "v2ce_event_frames_sums: null pointer");
    const int HW = H * W, gpp = (HW + 3) / 4;
    const long long groups = (long long)P * gpp;
    const bool vec = HW % 4 == 0 && aligned16(vox) && aligned16(sums);
    auto *h = reinterpret_cast<unsigned long long *>(hist);
    const dim3 grid(blocks_for(groups)), block(kThreads);
    hipStream_t st = as_stream(stream);
    if (vec && h) hipLaunchKernelGGL((sums_kernel<true, true>), grid, block, 0, st, vox, sums, HW, gpp, groups, mode, h);
    else if (vec) hipLaunchKernelGGL((sums_kernel<true, false>), grid, block, 0, st, vox, sums, HW, gpp, groups, mode, h);
    else if (h) hipLaunchKernelGGL((sums_kernel<false, true>), grid, block, 0, st, vox, sums, HW, gpp, groups, mode, h);
    else hipLaunchKernelGGL((sums_kernel<false, false>), grid, block, 0, st, vox, sums, HW, gpp, groups, mode, h);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

extern "C" int v2ce_event_frames_refine(const float *sums, int P, int H, int W, int mode, int level, uint32_t prefix_a,
                                        uint32_t prefix_b, uint64_t *hist, v2ce_stream_t stream) {
    clear_error();
    if (int rc = check_shape("v2ce_event_frames_refine", P, H, W, mode)) return rc;
    V2CE_REQUIRE(level == 1 || level == 2, V2CE_ERR_BAD_ARG, "v2ce_event_frames_refine: level %d (1: bits 19..10, 2: bits 9..0)", level);
    const uint32_t lim = level == 1 ? (uint32_t)kL1Bins : (uint32_t)kL1Bins * kRefBins;
    V2CE_REQUIRE(prefix_a < lim && prefix_b < lim, V2CE_ERR_BAD_ARG,
                 "v2ce_event_frames_refine: a level-%d prefix is below %u (got %u, %u)", level, lim, prefix_a, prefix_b);
    V2CE_REQUIRE(sums && hist, V2CE_ERR_BAD_ARG, "v2ce_event_frames_refine: null pointer");
    const int HW = H * W;
    const int span = mode == V2CE_EVENT_FRAMES_POLARITY ? 2 * HW : HW;
    const int first = mode == V2CE_EVENT_FRAMES_POLARITY ? 0 : 2 * HW;
    const long long total = (long long)P * span;
    hipLaunchKernelGGL(refine_kernel, dim3(blocks_for((total + 3) / 4)), dim3(kThreads), 0, as_stream(stream), sums, HW, span,
                       first, total, level == 1 ? 20 : 10, level == 1 ? 10 : 0, prefix_a, prefix_b,
                       reinterpret_cast<unsigned long long *>(hist));
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

extern "C" int v2ce_event_frames_render(const float *sums, int P, int H, int W, int mode, double upper, int64_t first_pair,
                                        int64_t total_pairs, uint8_t *frames, v2ce_stream_t stream) {
    clear_error();
    if (int rc = check_shape("v2ce_event_frames_render", P, H, W, mode)) return rc;
    V2CE_REQUIRE(upper > 0.0 && upper <= 1.79769313486231570815e308, V2CE_ERR_BAD_ARG,
                 "v2ce_event_frames_render: upper must be positive and finite (got %g)", upper);
    V2CE_REQUIRE(mode == V2CE_EVENT_FRAMES_POLARITY || (float)upper > 0.0f, V2CE_ERR_BAD_ARG,
                 "v2ce_event_frames_render: upper %g rounds to zero in float32 (grey mode)", upper);
    V2CE_REQUIRE(first_pair >= 0 && total_pairs >= 1 && first_pair <= total_pairs - P, V2CE_ERR_BAD_ARG,
                 "v2ce_event_frames_render: pairs [%lld, %lld) outside the clip's %lld", (long long)first_pair,
                 (long long)first_pair + P, (long long)total_pairs);
    V2CE_REQUIRE(total_pairs * (long long)H * W < (1ll << 40), V2CE_ERR_UNSUPPORTED,
                 "v2ce_event_frames_render: total_pairs * H * W must stay below 2^40");
    V2CE_REQUIRE(sums && frames, V2CE_ERR_BAD_ARG, "v2ce_event_frames_render: null pointer");
    V2CE_REQUIRE(reinterpret_cast<uintptr_t>(frames) % 4 == 0, V2CE_ERR_BAD_ARG,
                 "v2ce_event_frames_render: frames (the base of the clip's buffer) must be 4-byte aligned");
    const int HW = H * W;
    const long long q_lo = first_pair * HW, q_hi = (first_pair + P) * HW;
    const bool vec = HW % 4 == 0 && aligned16(sums);
    const dim3 grid(blocks_for(((q_hi + 3) >> 2) - (q_lo >> 2))), block(kThreads);
    hipStream_t st = as_stream(stream);
    const bool pol = mode == V2CE_EVENT_FRAMES_POLARITY;
    if (vec && pol) hipLaunchKernelGGL((render_kernel<true, true>), grid, block, 0, st, sums, HW, q_lo, q_hi, upper, frames);
    else if (vec) hipLaunchKernelGGL((render_kernel<true, false>), grid, block, 0, st, sums, HW, q_lo, q_hi, upper, frames);
    else if (pol) hipLaunchKernelGGL((render_kernel<false, true>), grid, block, 0, st, sums, HW, q_lo, q_hi, upper, frames);
    else hipLaunchKernelGGL((render_kernel<false, false>), grid, block, 0, st, sums, HW, q_lo, q_hi, upper, frames);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
