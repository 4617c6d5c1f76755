// imgrad.hip -- the image-gradient input channel and the three-channel image units on gfx950.
//
// Replaces train/scripts/utils/image_derivative.py:38-75 (get_batch_double_blurred_image_gradient) and the packet
// normalisation of train/scripts/data/event_pack_dataset.py:66-73 for uint8 frames [S][L + 1][H][W], S packets of L pairs:
//
//   grad_blur_kernel  one workgroup per (pair, 16 x 64 output tile).  The uint8 halo of both frames (tile + radius + 1 on
//                     every side) goes to LDS; the Sobel sums are INTEGERS (|Gx|, |Gy| <= 1020, Gx^2 + Gy^2 < 2^22: exact
//                     in int32 and in f32), the two frames are merged as the maximum of the integer squares, and
//                     sqrtf(max) / 255.f is taken once per halo cell.  Then the horizontal 1-D pass into LDS and the
//                     vertical pass to global f32 [S][L][H][W]; every pass is one fmaf chain from zero in tap order.
//                     The packet maximum: values are non-negative, so their bits order as unsigned; every wave reduces its
//                     own, one lane per workgroup does ONE atomicMax on the packet's uint32 word.  The maximum commutes:
//                     the bytes do not depend on the run or on what shares the call.  No float atomic.
//   units_kernel      f32 [S][L][3][H][W]: channels 0 / 1 = (u8 / 255 - mean) / std exactly as preproc.hip writes them,
//                     channel 2 = blur / max[s] (0 / 0 = NaN for a packet of black frames, as in the reference).
//
// Two borders: the Sobel sees the FRAME zero-padded (F.conv2d(padding=1)); the blur sees the GRADIENT MAP reflected without
// repeating the edge (torch 'reflect').  A gradient cell outside the frame is therefore the mirrored cell inside, which
// lies in the tile's own halo (the halo spans radius cells and H, W > radius), so only in-frame halo cells are computed
// and both passes index through reflect101.
// Built with the EXACT flags (no contraction, correctly rounded division and sqrt).
#include "common.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;
constexpr int kTH = 16, kTW = 64;                                 // output tile
constexpr int kMaxRadius = 7;                                     // kernel_size <= 15
constexpr int kGH = kTH + 2 * kMaxRadius, kGW = kTW + 2 * kMaxRadius;      // gradient halo 30 x 78
constexpr int kUH = kGH + 2, kUW = kGW + 2;                       // uint8 halo 32 x 80
// LDS: 2 * 32 * 80 B + 30 * 78 * 4 B + 30 * 64 * 4 B = 5 120 + 9 360 + 7 680 = 22 160 B

struct BlurW { float w[2 * kMaxRadius + 1]; };

// torch's 'reflect': c b | a b c d | c b; one fold suffices for -n < i < 2 n - 1
__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ __launch_bounds__(kThreads) void grad_blur_kernel(const uint8_t *__restrict__ frames, int L, int H, int W,
                                                             int R, int tiles_x, int tiles, BlurW bw,
                                                             float *__restrict__ blur, unsigned *__restrict__ gmax) {
    __shared__ uint8_t u8[2][kUH * kUW];
    __shared__ float G[kGH * kGW];
    __shared__ float Hs[kGH * kTW];
    __shared__ unsigned red[kThreads / kWave];
    const int tid = threadIdx.x;
    const long long pair = blockIdx.x / tiles;                    // s * L + l
    const int tile = (int)(blockIdx.x - pair * tiles);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const long long s = pair / L;
    const long long HW = (long long)H * W;
    const uint8_t *fa = frames + (pair + s) * HW, *fb = fa + HW;   // packet s starts at frame s * (L + 1)
    const int gh = kTH + 2 * R, gw = kTW + 2 * R, K = 2 * R + 1;

    // uint8 halo, zeros outside the frame (the Sobel's padding)
    for (int c = tid; c < (gh + 2) * (gw + 2); c += kThreads) {
        const int i = c / (gw + 2), j = c - i * (gw + 2);
        const int y = y0 - R - 1 + i, x = x0 - R - 1 + j;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const long long o = in ? (long long)y * W + x : 0;
        u8[0][i * kUW + j] = in ? fa[o] : (uint8_t)0;
        u8[1][i * kUW + j] = in ? fb[o] : (uint8_t)0;
    }
    __syncthreads();
    // gradient halo: max over the two frames of the integer Gx^2 + Gy^2, one sqrt and one division per cell
    for (int c = tid; c < gh * gw; c += kThreads) {
        const int i = c / gw, j = c - i * gw;
        const int y = y0 - R + i, x = x0 - R + j;
        float g = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            int sq[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const uint8_t *p = &u8[f][i * kUW + j];           // the cell's upper left neighbour
                const int a = p[0], b = p[1], cc = p[2], d = p[kUW], e = p[kUW + 2], ff = p[2 * kUW], gg = p[2 * kUW + 1],
                          hh = p[2 * kUW + 2];
                const int gx = (cc + 2 * e + hh) - (a + 2 * d + ff), gy = (ff + 2 * gg + hh) - (a + 2 * b + cc);
                sq[f] = gx * gx + gy * gy;
            }
            g = sqrtf((float)(sq[0] > sq[1] ? sq[0] : sq[1])) / 255.0f;
        }
        G[i * kGW + j] = g;
    }
    __syncthreads();
    // horizontal pass over the in-frame halo rows
    for (int c = tid; c < gh * kTW; c += kThreads) {
        const int i = c / kTW, j = c - i * kTW;
        const int y = y0 - R + i, x = x0 + j;
        float acc = 0.0f;
        if (y >= 0 && y < H && x < W) {
            const float *row = G + i * kGW - (x0 - R);
            for (int k = 0; k < K; ++k) acc = fmaf(bw.w[k], row[reflect101(x - R + k, W)], acc);
        }
        Hs[c] = acc;
    }
    __syncthreads();
    // vertical pass to global, the tile's maximum on the way
    unsigned m = 0u;
    float *out = blur + pair * HW;
    for (int c = tid; c < kTH * kTW; c += kThreads) {
        const int i = c / kTW, j = c - i * kTW;
        const int y = y0 + i, x = x0 + j;
        if (y < H && x < W) {
            const float *col = Hs + j - (y0 - R) * kTW;
            float acc = 0.0f;
            for (int k = 0; k < K; ++k) acc = fmaf(bw.w[k], col[reflect101(y - R + k, H) * kTW], acc);
            out[(long long)y * W + x] = acc;
            const unsigned bits = __float_as_uint(acc);           // acc >= +0: bits order as the values
            m = bits > m ? bits : m;
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)m, o);
        m = other > m ? other : m;
    }
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / kWave; ++w) m = red[w] > m ? red[w] : m;
        atomicMax(gmax + s, m);
    }
}

// one lane per output element of [S][L][3][H][W]
__global__ __launch_bounds__(kThreads) void units_kernel(const uint8_t *__restrict__ frames, const float *__restrict__ blur,
                                                         const unsigned *__restrict__ gmax, int L, long long HW,
                                                         long long total, float mean, float stdv,
                                                         float *__restrict__ units) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const long long p = e % HW, pc = e / HW;
    const long long pair = pc / 3;
    const int c = (int)(pc - pair * 3);
    const long long s = pair / L;
    if (c < 2) {
        const float x = (float)frames[(pair + s + c) * HW + p] / 255.0f;
        units[e] = (x - mean) / stdv;
    } else {
        units[e] = blur[pair * HW + p] / __uint_as_float(gmax[s]);
    }
}

struct Plan { int R, tiles_x, tiles; long long pairs, blocks; };

// false for arguments the entries refuse
bool plan_of(int S, int L, int H, int W, int kernel_size, Plan *p) {
    if (S < 1 || L < 1 || H < 1 || W < 1 || kernel_size < 3 || kernel_size > 2 * kMaxRadius + 1 || kernel_size % 2 == 0)
        return false;
    p->R = kernel_size / 2;
    if (H <= p->R || W <= p->R) return false;
    p->tiles_x = (W + kTW - 1) / kTW;
    const long long tiles = (long long)p->tiles_x * ((H + kTH - 1) / kTH);
    p->pairs = (long long)S * L;
    p->blocks = p->pairs * tiles;
    if (tiles >= (1ll << 31) || p->blocks >= (1ll << 31)) return false;
    if ((long long)S * (L + 1) * H * W >= (1ll << 40)) return false;
    if ((p->pairs * 3 * H * W + kThreads - 1) / kThreads >= (1ll << 31)) return false;
    p->tiles = (int)tiles;
    return true;
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

#define V2CE_IMGRAD_SHAPE(fn)                                                                                          \
    fn ": needs S, L >= 1, kernel_size odd in [3, %d], H and W above kernel_size / 2 and at most 2^31 - 1 workgroups " \
       "(got S = %d, L = %d, H = %d, W = %d, kernel_size = %d)"

int launch_grad(const uint8_t *frames_u8, int S, int L, int H, int W, const float *weights_host, const Plan &p, float *blur,
                uint32_t *gmax_bits, hipStream_t st) {
    BlurW bw = {};
    for (int k = 0; k < 2 * p.R + 1; ++k) bw.w[k] = weights_host[k];
    V2CE_HIP_CHECK(hipMemsetAsync(gmax_bits, 0, (size_t)S * 4, st));
    hipLaunchKernelGGL(grad_blur_kernel, dim3((unsigned)p.blocks), dim3(kThreads), 0, st, frames_u8, L, H, W, p.R, p.tiles_x,
                       p.tiles, bw, blur, gmax_bits);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_image_grad_workspace_bytes(int S, int L, int H, int W) {
    Plan p;
    if (!plan_of(S, L, H, W, 3, &p)) return 0;
    return pad16((size_t)p.pairs * H * W * 4);                     // the un-normalised blur, f32 [S][L][H][W]
}

extern "C" int v2ce_image_grad_batch(const uint8_t *frames_u8, int S, int L, int H, int W, const float *weights,
                                     int kernel_size, float *blur, uint32_t *gmax_bits, v2ce_stream_t stream) {
    clear_error();
    Plan p;
    V2CE_REQUIRE(plan_of(S, L, H, W, kernel_size, &p), V2CE_ERR_BAD_ARG, V2CE_IMGRAD_SHAPE("v2ce_image_grad_batch"), 2 * kMaxRadius + 1, S, L, H, W,
                 kernel_size);
    V2CE_REQUIRE(frames_u8 && weights && blur && gmax_bits, V2CE_ERR_BAD_ARG, "v2ce_image_grad_batch: null pointer");
    return launch_grad(frames_u8, S, L, H, W, weights, p, blur, gmax_bits, as_stream(stream));
}

extern "C" int v2ce_image_units_grad(const uint8_t *frames_u8, int S, int L, int H, int W, const float *weights,
                                     int kernel_size, float mean, float stdv, float *units, uint32_t *gmax_bits,
                                     void *workspace, size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    Plan p;
    V2CE_REQUIRE(plan_of(S, L, H, W, kernel_size, &p), V2CE_ERR_BAD_ARG, V2CE_IMGRAD_SHAPE("v2ce_image_units_grad"), 2 * kMaxRadius + 1, S, L, H, W,
                 kernel_size);
    V2CE_REQUIRE(frames_u8 && weights && units && gmax_bits && workspace, V2CE_ERR_BAD_ARG, "v2ce_image_units_grad: null pointer");
    V2CE_REQUIRE(workspace_bytes >= v2ce_image_grad_workspace_bytes(S, L, H, W), V2CE_ERR_WORKSPACE,
                 "v2ce_image_units_grad: workspace of %zu bytes, needs %zu", workspace_bytes,
                 v2ce_image_grad_workspace_bytes(S, L, H, W));
    V2CE_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, V2CE_ERR_BAD_ARG,
                 "v2ce_image_units_grad: workspace must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    float *blur = static_cast<float *>(workspace);
    const int rc = launch_grad(frames_u8, S, L, H, W, weights, p, blur, gmax_bits, st);
    if (rc != V2CE_OK) return rc;
    const long long HW = (long long)H * W, total = p.pairs * 3 * HW;
    hipLaunchKernelGGL(units_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, frames_u8, blur,
                       gmax_bits, L, HW, total, mean, stdv, units);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
