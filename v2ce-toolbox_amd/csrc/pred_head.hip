// pred_head.hip -- the prediction head UNet.pred (1x1x1 convolution 32 -> Cout with bias, relu) as a trainable layer on
// gfx950: its forward from the channels-last-16 features of the last decoder block, and its backward (d_weight, d_bias,
// d_feat).  include/v2ce_hip_train.h states the formulas and the tensors.
//
// prep: the f32 weights (and the bias) once as f64 into the workspace, so the kernels below read them with scalar loads
// and spend no conversion on them.
//
// forward: a lane owns one position: it loads the position's two 64-byte channel groups, converts them once, and walks
// the output channels; the store of channel co is a coalesced row piece of y.
//
// gradients: a workgroup owns a fixed, contiguous share of the 128-position tiles.  Per tile it stages the 32 features
// of every position (sF[p][ci]) and the masked upstream m = y > 0 ? upstream : 0 (sM[slot][p], slot = (co % 8) * 4 +
// co / 8, rows of 132 floats) in LDS as f32 -- the loads of the next tile are issued before the work on the current one
// -- and then
//   d_weight  a wave takes 32 positions of the tile; lane (cig = lane & 7, cog = lane >> 3) owns the 4 x 4 outputs
//             ci = 4 cig + i, co = cog + 8 j and reads, per 4 positions, 4 + ceil(Cout / 8) 16-byte pieces for 64 (48 at
//             Cout = 20) f64 FMAs: one piece of sF per position, one piece of sM per j (4 positions of one co)
//   d_bias    thread t sums the 16 positions (t & 7) * 16 .. + 15 of slot t >> 3
//   d_feat    thread t owns position t & 127 and channel group t >> 7: sum over co of m weight[co][ci], 16 outputs, one
//             64-byte store
// At the end the four waves' d_weight sums meet in LDS in the order ((w0 + w1) + w2) + w3, the 8 partial sums of a bias
// slot in a butterfly, and the workgroup writes its f64 partials; finish_kernel adds the partials of the workgroups
// (lane i takes workgroups i, i + 64, ... in order, then a butterfly) and rounds once.  The grid depends on the shape
// only, so the order of every sum is fixed: no atomics, the same bytes every run.
//
// Arithmetic: a product of two f32 is exact in f64, so fma(a, b, c) here equals the separate multiply and add bit for
// bit; the order of the additions is the only freedom, and it is fixed as described.
#include "common.h"

#include "../../include/v2ce_hip_train.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;             // 4 waves
constexpr int kCin = 32;
constexpr int kMaxCout = 32;
constexpr int kTile = 128;                // positions per tile
constexpr int kMPitch = 132;              // floats per row of sM: 16-byte rows, slots 4 apart land 16 banks apart
constexpr int kMaxGrid = 512;             // workgroups of the gradient kernel: two per CU
constexpr int kPartial = kMaxCout * kCin + kMaxCout;   // f64 per workgroup: d_weight [32][32], d_bias [32]
constexpr int kWantW = 1, kWantB = 2, kWantF = 4;

struct Dims {
    int B, L, Cout, H, W, pitch;
    unsigned N, HW;                       // positions B L H W, pixels H W
    int nco;                              // ceil(Cout / 8)
    long long tiles;                      // ceil(N / kTile)
    int grid;                             // min(tiles, kMaxGrid)
    size_t w_off, b_off, p_off, total;    // byte offsets into the workspace: f64 weights, f64 bias, partials
};

struct Pos {
    unsigned f, h, w, r;                  // frame b L + l, row, column, h W + w
};

__device__ __forceinline__ Pos locate(const Dims &D, unsigned n) {
    Pos P;
    P.f = n / D.HW;
    P.r = n - P.f * D.HW;
    P.h = P.r / (unsigned)D.W;
    P.w = P.r - P.h * (unsigned)D.W;
    return P;
}

// float offset of channel group g of a position in a C16 tensor
__device__ __forceinline__ long long c16_at(const Dims &D, const Pos &P, int g) {
    return ((((long long)P.f * 2 + g) * D.H + P.h) * D.pitch + P.w) * 16;
}

__device__ __forceinline__ int slot_of(int co) { return (co & 7) * 4 + (co >> 3); }

__global__ __launch_bounds__(kThreads) void prep_kernel(const float *__restrict__ weight, const float *__restrict__ bias,
                                                        int Cout, double *__restrict__ Wd, double *__restrict__ bd) {
    for (int i = threadIdx.x; i < Cout * kCin; i += kThreads) Wd[i] = (double)weight[i];
    if (bias && (int)threadIdx.x < Cout) bd[threadIdx.x] = (double)bias[threadIdx.x];
}

// grid ceil(N / 256), 256 threads: one position per lane
__global__ __launch_bounds__(kThreads) void fwd_kernel(const float *__restrict__ feat, const double *__restrict__ Wd,
                                                       const double *__restrict__ bd, Dims D, float *__restrict__ y) {
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n >= (long long)D.N) return;
    const Pos P = locate(D, (unsigned)n);
    double x[kCin];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const float4 *src = reinterpret_cast<const float4 *>(feat + c16_at(D, P, g));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = src[q];
            x[g * 16 + q * 4 + 0] = (double)v.x; x[g * 16 + q * 4 + 1] = (double)v.y;
            x[g * 16 + q * 4 + 2] = (double)v.z; x[g * 16 + q * 4 + 3] = (double)v.w;
        }
    }
    float *dst = y + (long long)P.f * D.Cout * D.HW + P.r;
    for (int co = 0; co < D.Cout; ++co) {
        const double *wr = Wd + co * kCin;
        double a = bd[co];
#pragma unroll
        for (int ci = 0; ci < kCin; ++ci) a = fma(x[ci], wr[ci], a);
        const float v = (float)a;
        dst[(long long)co * D.HW] = v > 0.0f ? v : (v == v ? 0.0f : v);
    }
}

// grid D.grid, 256 threads; workgroup g walks the tiles [g tiles / grid, (g + 1) tiles / grid).  kNco = ceil(Cout / 8), a
// template argument so that the d_weight loop is straight-line code whose LDS reads the compiler can issue ahead
template <int kNco>
__global__ __launch_bounds__(kThreads) void grads_kernel(const float *__restrict__ feat, const float *__restrict__ y,
                                                         const float *__restrict__ up, const double *__restrict__ Wd,
                                                         Dims D, int want, double *__restrict__ partial,
                                                         float *__restrict__ d_feat) {
    __shared__ __attribute__((aligned(16))) float smem[kTile * kCin + 32 * kMPitch];
    float *sF = smem, *sM = smem + kTile * kCin;
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int cig = lane & 7, cog = lane >> 3;
    const bool doW = (want & kWantW) != 0, doB = (want & kWantB) != 0, doF = (want & kWantF) != 0;
    const long long t0 = (long long)blockIdx.x * D.tiles / gridDim.x, t1 = ((long long)blockIdx.x + 1) * D.tiles / gridDim.x;

    double acc[kNco][4];
#pragma unroll
    for (int j = 0; j < kNco; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.0;
    double bsum = 0.0;

    // staging roles: features -- piece q = t & 3 of group k >> 1 of position (t >> 2) + 64 (k & 1); mask -- position
    // t & 127, channels (t >> 7) + 2 k
    float4 pf[4];
    float py[16], pu[16];                 // y and upstream as loaded: the select waits until they are stored to LDS, so the
                                          // loads of a tile are all in flight together
    const int fp = t >> 2, fq = t & 3, mp = t & (kTile - 1), mc = t >> 7;

#define V2CE_PRED_FETCH(tile)                                                                                      \
    do {                                                                                                           \
        const long long base_ = (long long)(tile) * kTile;                                                         \
        if (doW) {                                                                                                 \
            _Pragma("unroll") for (int h_ = 0; h_ < 2; ++h_) {                                                     \
                const long long n_ = base_ + fp + 64 * h_;                                                         \
                const bool ok_ = n_ < (long long)D.N;                                                              \
                const Pos P_ = locate(D, ok_ ? (unsigned)n_ : 0u);                                                 \
                _Pragma("unroll") for (int g_ = 0; g_ < 2; ++g_) {                                                 \
                    float4 v_ = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                                               \
                    if (ok_) v_ = *reinterpret_cast<const float4 *>(feat + c16_at(D, P_, g_) + fq * 4);            \
                    pf[g_ * 2 + h_] = v_;                                                                          \
                }                                                                                                  \
            }                                                                                                      \
        }                                                                                                          \
        {                                                                                                          \
            const long long n_ = base_ + mp;                                                                       \
            const bool ok_ = n_ < (long long)D.N;                                                                  \
            const Pos P_ = locate(D, ok_ ? (unsigned)n_ : 0u);                                                     \
            const long long at_ = (long long)P_.f * D.Cout * D.HW + P_.r;                                          \
            _Pragma("unroll") for (int k_ = 0; k_ < 16; ++k_) {                                                    \
                const int co_ = mc + 2 * k_;                                                                       \
                float yv_ = 0.0f, uv_ = 0.0f;                                                                      \
                if (ok_ && co_ < D.Cout) {                                                                         \
                    yv_ = y[at_ + (long long)co_ * D.HW];                                                          \
                    uv_ = up[at_ + (long long)co_ * D.HW];                                                         \
                }                                                                                                  \
                py[k_] = yv_;                                                                                      \
                pu[k_] = uv_;                                                                                      \
            }                                                                                                      \
        }                                                                                                          \
    } while (0)

    if (t0 < t1) V2CE_PRED_FETCH(t0);
    for (long long tile = t0; tile < t1; ++tile) {
        __syncthreads();                                           // the previous tile has been read
        if (doW) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                *reinterpret_cast<float4 *>(sF + (fp + 64 * (k & 1)) * kCin + (k >> 1) * 16 + fq * 4) = pf[k];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int co = mc + 2 * k;
            if (co < 8 * kNco) sM[slot_of(co) * kMPitch + mp] = py[k] > 0.0f ? pu[k] : 0.0f;   // zeros for Cout <= co < 8 kNco
        }
        __syncthreads();
        if (tile + 1 < t1) V2CE_PRED_FETCH(tile + 1);

        if (doW) {
#pragma unroll 2
            for (int it = 0; it < 8; ++it) {
                const int p0 = wv * 32 + it * 4;
                float4 f[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) f[q] = *reinterpret_cast<const float4 *>(sF + (p0 + q) * kCin + cig * 4);
                double fd[4][4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    fd[q][0] = (double)f[q].x; fd[q][1] = (double)f[q].y; fd[q][2] = (double)f[q].z; fd[q][3] = (double)f[q].w;
                }
#pragma unroll
                for (int j = 0; j < kNco; ++j) {
                    const float4 mv = *reinterpret_cast<const float4 *>(sM + (cog * 4 + j) * kMPitch + p0);
                    const double md[4] = {(double)mv.x, (double)mv.y, (double)mv.z, (double)mv.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[j][i] = fma(md[q], fd[q][i], acc[j][i]);
                }
            }
        }
        if (doB) {
            const int slot = t >> 3, co = (slot & 3) * 8 + (slot >> 2);
            if (co < D.Cout) {
                const float *row = sM + slot * kMPitch + (t & 7) * 16;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 mv = *reinterpret_cast<const float4 *>(row + i * 4);
                    bsum += (double)mv.x; bsum += (double)mv.y; bsum += (double)mv.z; bsum += (double)mv.w;
                }
            }
        }
        if (doF) {
            const int g = __builtin_amdgcn_readfirstlane(t >> 7);
            double a[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) a[i] = 0.0;
            for (int co = 0; co < D.Cout; ++co) {
                const double md = (double)sM[slot_of(co) * kMPitch + mp];
                const double *wr = Wd + co * kCin + g * 16;
#pragma unroll
                for (int i = 0; i < 16; ++i) a[i] = fma(md, wr[i], a[i]);
            }
            const long long n = tile * kTile + mp;
            if (n < (long long)D.N) {
                const Pos P = locate(D, (unsigned)n);
                float4 *dst = reinterpret_cast<float4 *>(d_feat + c16_at(D, P, g));
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    dst[q] = make_float4((float)a[q * 4], (float)a[q * 4 + 1], (float)a[q * 4 + 2], (float)a[q * 4 + 3]);
            }
        }
    }
#undef V2CE_PRED_FETCH

    double *mine = partial + (size_t)blockIdx.x * kPartial;
    if (doW) {
        double *red = reinterpret_cast<double *>(smem);            // 3 x [32][32] f64 = 24 KB of the 32.5 KB
        __syncthreads();                                           // the last tile has been read
        if (wv > 0) {
#pragma unroll
            for (int j = 0; j < kNco; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) red[(wv - 1) * 1024 + (cog + 8 * j) * kCin + cig * 4 + i] = acc[j][i];
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int j = 0; j < kNco; ++j) {
                const int co = cog + 8 * j;
                if (co < D.Cout) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = co * kCin + cig * 4 + i;
                        mine[e] = ((acc[j][i] + red[e]) + red[1024 + e]) + red[2048 + e];
                    }
                }
            }
        }
    }
    if (doB) {
        bsum += __shfl_xor(bsum, 1);
        bsum += __shfl_xor(bsum, 2);
        bsum += __shfl_xor(bsum, 4);
        const int slot = t >> 3, co = (slot & 3) * 8 + (slot >> 2);
        if ((t & 7) == 0 && co < D.Cout) mine[kMaxCout * kCin + co] = bsum;
    }
}

// grid Cout * 33, 64 threads: block e < Cout 32 is d_weight[e], the others d_bias[e - Cout 32]
__global__ __launch_bounds__(kWave) void finish_kernel(const double *__restrict__ partial, int grid, int Cout, int want,
                                                       float *__restrict__ d_weight, float *__restrict__ d_bias) {
    const int e = blockIdx.x, nw = Cout * kCin;
    const bool is_w = e < nw;
    if (is_w ? !(want & kWantW) : !(want & kWantB)) return;
    const int off = is_w ? e : kMaxCout * kCin + (e - nw);
    double s = 0.0;
    for (int g = threadIdx.x; g < grid; g += kWave) s += partial[(size_t)g * kPartial + off];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) {
        if (is_w) d_weight[e] = (float)s;
        else d_bias[e - nw] = (float)s;
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

bool make_dims(bool grads, int B, int L, int Cout, int H, int W, int pitch, Dims &D) {
    if (B < 1 || L < 1 || H < 1 || W < 1 || pitch < W || Cout < 1 || Cout > kMaxCout) return false;
    const long long N = (long long)B * L * H * W;
    if ((long long)B * L >= (1ll << 31) || (long long)H * W >= (1ll << 31) || N >= (1ll << 31)) return false;
    if ((long long)B * L * H >= (1ll << 34) || (long long)B * L * H * pitch >= (1ll << 34)) return false;
    D.B = B; D.L = L; D.Cout = Cout; D.H = H; D.W = W; D.pitch = pitch;
    D.N = (unsigned)N; D.HW = (unsigned)((long long)H * W);
    D.nco = (Cout + 7) / 8;
    D.tiles = (N + kTile - 1) / kTile;
    D.grid = (int)(D.tiles < kMaxGrid ? D.tiles : kMaxGrid);
    size_t at = 0;
    D.w_off = at; at += align256((size_t)kMaxCout * kCin * sizeof(double));
    D.b_off = at; at += align256((size_t)kMaxCout * sizeof(double));
    D.p_off = at; at += grads ? align256((size_t)D.grid * kPartial * sizeof(double)) : 0;
    D.total = at;
    return true;
}

const char *kNeeds = "needs B, L, H, W >= 1, pitch >= W, 1 <= Cout <= 32, B L H W < 2^31 and B L H pitch < 2^34";

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_pred_head_fwd_workspace_bytes(int B, int L, int Cout, int H, int W, int pitch) {
    Dims D;
    return make_dims(false, B, L, Cout, H, W, pitch, D) ? D.total : 0;
}

extern "C" int v2ce_pred_head_fwd(const float *feat, const float *weight, const float *bias, int B, int L, int Cout, int H,
                                  int W, int pitch, float *y, void *workspace, size_t workspace_bytes,
                                  v2ce_stream_t stream) {
    clear_error();
    Dims D;
    V2CE_REQUIRE(make_dims(false, B, L, Cout, H, W, pitch, D), V2CE_ERR_BAD_ARG,
                 "v2ce_pred_head_fwd: B %d L %d Cout %d H %d W %d pitch %d: %s", B, L, Cout, H, W, pitch, kNeeds);
    V2CE_REQUIRE(feat && weight && bias && y && workspace, V2CE_ERR_BAD_ARG, "v2ce_pred_head_fwd: null pointer");
    V2CE_REQUIRE(aligned16(feat), V2CE_ERR_BAD_ARG, "v2ce_pred_head_fwd: feat must be 16-byte aligned");
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, V2CE_ERR_BAD_ARG,
                 "v2ce_pred_head_fwd: workspace must be 8-byte aligned");
    V2CE_REQUIRE(workspace_bytes >= D.total, V2CE_ERR_WORKSPACE, "v2ce_pred_head_fwd: workspace too small (%zu < %zu)",
                 workspace_bytes, D.total);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    double *Wd = reinterpret_cast<double *>(ws + D.w_off), *bd = reinterpret_cast<double *>(ws + D.b_off);
    hipLaunchKernelGGL(prep_kernel, dim3(1), dim3(kThreads), 0, st, weight, bias, Cout, Wd, bd);
    const unsigned blocks = (unsigned)(((long long)D.N + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(fwd_kernel, dim3(blocks), dim3(kThreads), 0, st, feat, Wd, bd, D, y);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

extern "C" size_t v2ce_pred_head_grads_workspace_bytes(int B, int L, int Cout, int H, int W, int pitch) {
    Dims D;
    return make_dims(true, B, L, Cout, H, W, pitch, D) ? D.total : 0;
}

extern "C" int v2ce_pred_head_grads(const float *feat, const float *y, const float *upstream, const float *weight, int B,
                                    int L, int Cout, int H, int W, int pitch, float *d_weight, float *d_bias,
                                    float *d_feat, void *workspace, size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    Dims D;
    V2CE_REQUIRE(make_dims(true, B, L, Cout, H, W, pitch, D), V2CE_ERR_BAD_ARG,
                 "v2ce_pred_head_grads: B %d L %d Cout %d H %d W %d pitch %d: %s", B, L, Cout, H, W, pitch, kNeeds);
    V2CE_REQUIRE(feat && y && upstream && weight && workspace, V2CE_ERR_BAD_ARG, "v2ce_pred_head_grads: null pointer");
    V2CE_REQUIRE(d_weight || d_bias || d_feat, V2CE_ERR_BAD_ARG,
                 "v2ce_pred_head_grads: no output requested (d_weight, d_bias and d_feat are all null)");
    V2CE_REQUIRE(aligned16(feat, d_feat), V2CE_ERR_BAD_ARG, "v2ce_pred_head_grads: feat and d_feat must be 16-byte aligned");
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, V2CE_ERR_BAD_ARG,
                 "v2ce_pred_head_grads: workspace must be 8-byte aligned");
    V2CE_REQUIRE(workspace_bytes >= D.total, V2CE_ERR_WORKSPACE, "v2ce_pred_head_grads: workspace too small (%zu < %zu)",
                 workspace_bytes, D.total);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    double *Wd = reinterpret_cast<double *>(ws + D.w_off), *partial = reinterpret_cast<double *>(ws + D.p_off);
    const int want = (d_weight ? kWantW : 0) | (d_bias ? kWantB : 0) | (d_feat ? kWantF : 0);
    if (d_feat) hipLaunchKernelGGL(prep_kernel, dim3(1), dim3(kThreads), 0, st, weight, (const float *)nullptr, Cout, Wd, (double *)nullptr);
    const dim3 grid((unsigned)D.grid), block(kThreads);
    switch (D.nco) {
        case 1: hipLaunchKernelGGL(grads_kernel<1>, grid, block, 0, st, feat, y, upstream, Wd, D, want, partial, d_feat); break;
        case 2: hipLaunchKernelGGL(grads_kernel<2>, grid, block, 0, st, feat, y, upstream, Wd, D, want, partial, d_feat); break;
        case 3: hipLaunchKernelGGL(grads_kernel<3>, grid, block, 0, st, feat, y, upstream, Wd, D, want, partial, d_feat); break;
        default: hipLaunchKernelGGL(grads_kernel<4>, grid, block, 0, st, feat, y, upstream, Wd, D, want, partial, d_feat); break;
    }
    if (d_weight || d_bias)
        hipLaunchKernelGGL(finish_kernel, dim3((unsigned)(Cout * (kCin + 1))), dim3(kWave), 0, st, partial, D.grid, Cout, want,
                           d_weight, d_bias);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
