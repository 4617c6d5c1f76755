// voxlosses.hip -- the voxel-only terms of the stage-1 training loss (ModelInterface.calculate_loss and the classes
// of train/scripts/model/losses.py) as per-sequence sufficient statistics, on gfx950.
//
// Two entries share one kernel template:
//   v2ce_voxlosses      pred, gt [B][L][20][H][W]: every term below, one record per b
//   v2ce_volume_losses  pred, gt [N][D][H][W]:     the elementwise, pyramid and temporal sums, one record per n
// In the 5-D layout volume (b, p) owns the planes d = l * 10 + c at ((b L + l) 20 + p 10 + c) H W; the kernel differs
// between the two only in that address and in what two waves exchange per frame.
//
// Tile plan: a wave owns 8 rows x 8 columns of pixels (lane = row * 8 + column) of ONE volume; a lane owns one pixel
// column and walks the volume's planes in order, ten planes (one polarity of a frame) loaded at a time, so every input
// byte is read once.  For [N][D][H][W] a workgroup is four tiles side by side (8 rows x 32 columns: the four waves share
// the 128-byte lines they touch).  For sequences a workgroup is two tiles x two polarities: waves 2 j and 2 j + 1 walk
// polarity 0 and 1 of tile j and meet in LDS once per frame, where the polarity-0 wave adds its partner's event-frame
// and compensation sums to its own.  (One wave walking both polarities needed 256 VGPRs plus AGPR spills and ran at one
// wave per SIMD: 1.83 ms against 1.16 ms for this plan on [4][16][20][260][346])  Per lane and volume:
//   elementwise  f64 sums of (p - g)^2, |p - g|, |p|, p^2
//   pyramid      the lane adds its pixel over 2 planes; a butterfly over lane bits 1 and 8 makes the 2x2x2 window sum;
//                two of those and bits 2 and 16 make 4x4x4; two of those and bits 4 and 32 make 8x8x8.  Windows start
//                at d = 0, so the three sizes nest; a window counts when its rows and columns lie inside H and W
//   temporal     running sums of the windows {3j-1, 3j, 3j+1} (divisor 3, the padded ends included) and {5j .. 5j+4}
// and per lane and sequence (5-D only):
//   event frames sum over the 10 bins of |v| per polarity and frame, and over all frames
//   compensation masked sum (v * (v > 0.01f)) and count over the 10 bins, then over the tile's 8 rows with a butterfly
//                over lane bits 8, 16, 32, then polarity 0 + polarity 1; one partial per (b, l, band of 8 rows, w) in
//                the workspace
//   match        per channel over l: running maximum m, s = sum exp(v - m) rescaled when m moves (one exp per value),
//                the first maximum of gt and pred there; term = (m - pred[t]) + log(s)
//
// Arithmetic: every difference, product, pooled mean, exp and log is f64 from the f32 inputs; v > 0.01f is an f32
// compare (NaN is never above; v * mask keeps a NaN, as torch's pred * pred_mask does).  No float atomics: per-lane
// f64 partials, a butterfly per wave, one partial record per wave in the workspace, then per b a strided sum per
// thread and a fixed tree (finish kernel).  The two polarities of a sequence are reduced separately and then added, so
// the 5-D record equals the sum of the two [N][D][H][W] records of its volumes bit for bit.  Records are bit-identical
// run to run and do not depend on B.
#include "common.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;             // 4 waves: 8 rows x 32 columns
constexpr int kFinishThreads = 256;
constexpr int kChannels = 20;
constexpr int kBins = 10;
constexpr int kVolSlots = 9;              // sq, abs, pred_abs, pred_sq, pyr 2 / 4 / 8, temporal 3 / 5
constexpr int kSeqSlots = 6;              // ef c, ef cl, ef_splitp c, ef_splitp cl, match, match_low
constexpr int kAllTerms = V2CE_VOXLOSSES_PYRAMID | V2CE_VOXLOSSES_TEMPORAL | V2CE_VOXLOSSES_EF |
                          V2CE_VOXLOSSES_COMPENSATION | V2CE_VOXLOSSES_MATCH;

struct Plan {
    int N, D, L, H, W;                    // N volumes or sequences; D planes per volume (10 L for sequences)
    int bands, tiles, blocks_x;           // ceil(H / 8), ceil(W / 8), workgroups per band (2 or 4 tiles each)
    int mask, rec;                        // term mask; f64 slots of one wave's partial record (one per tile and polarity)
    long long plane;                      // H * W
    size_t comp_off, total;               // byte offset of the compensation partials; workspace bytes
};

__device__ __forceinline__ void wave_sum(double &v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
}

struct VolAcc {
    double sq, ab, pa, ps, pyr[3], t3, t5;
    double a2p, a2g, a4p, a4g, a8p, a8g;  // open pyramid windows
    double w3p, w3g, w5p, w5g;            // open temporal windows
};

__device__ __forceinline__ void vol_init(VolAcc &A) {
    A.sq = A.ab = A.pa = A.ps = A.pyr[0] = A.pyr[1] = A.pyr[2] = A.t3 = A.t5 = 0.0;
    A.a2p = A.a2g = A.a4p = A.a4g = A.a8p = A.a8g = A.w3p = A.w3g = A.w5p = A.w5g = 0.0;
}

struct LaneInfo {
    bool valid, ok2, ok4, ok8, lead2, lead4, lead8;
};

// one value of plane d of a volume; p, g are zero on a lane outside the image.  d and mask are wave-uniform.
__device__ __forceinline__ void vol_step(VolAcc &A, int d, double p, double g, const LaneInfo &I, int mask) {
    if (I.valid) {
        const double df = p - g;
        A.sq += df * df;
        A.ab += fabs(df);
        A.pa += fabs(p);
        A.ps += p * p;
    }
    if (mask & V2CE_VOXLOSSES_PYRAMID) {
        A.a2p += p; A.a2g += g;
        if (d & 1) {
            double sp = A.a2p, sg = A.a2g;
            A.a2p = A.a2g = 0.0;
            sp += __shfl_xor(sp, 1); sg += __shfl_xor(sg, 1);
            sp += __shfl_xor(sp, 8); sg += __shfl_xor(sg, 8);
            if (I.ok2 && I.lead2) { const double e = sp * 0.125 - sg * 0.125; A.pyr[0] += e * e; }
            A.a4p += sp; A.a4g += sg;
            if ((d & 3) == 3) {
                sp = A.a4p; sg = A.a4g;
                A.a4p = A.a4g = 0.0;
                sp += __shfl_xor(sp, 2); sg += __shfl_xor(sg, 2);
                sp += __shfl_xor(sp, 16); sg += __shfl_xor(sg, 16);
                if (I.ok4 && I.lead4) { const double e = sp * 0.015625 - sg * 0.015625; A.pyr[1] += e * e; }
                A.a8p += sp; A.a8g += sg;
                if ((d & 7) == 7) {
                    sp = A.a8p; sg = A.a8g;
                    A.a8p = A.a8g = 0.0;
                    sp += __shfl_xor(sp, 4); sg += __shfl_xor(sg, 4);
                    sp += __shfl_xor(sp, 32); sg += __shfl_xor(sg, 32);
                    if (I.ok8 && I.lead8) { const double e = sp * 0.001953125 - sg * 0.001953125; A.pyr[2] += e * e; }
                }
            }
        }
    }
    if (mask & V2CE_VOXLOSSES_TEMPORAL) {
        A.w3p += p; A.w3g += g;
        if (d % 3 == 1) {
            const double e = A.w3p / 3.0 - A.w3g / 3.0;
            if (I.valid) A.t3 += e * e;
            A.w3p = A.w3g = 0.0;
        }
        A.w5p += p; A.w5g += g;
        if (d % 5 == 4) {
            const double e = A.w5p / 5.0 - A.w5g / 5.0;
            if (I.valid) A.t5 += e * e;
            A.w5p = A.w5g = 0.0;
        }
    }
}

// the last temporal window of size 3 is {D-2, D-1, pad} when D = 3 m + 1; when D = 3 m plane D-1 is in no window
__device__ __forceinline__ void vol_flush(VolAcc &A, int D, const LaneInfo &I, int mask) {
    if ((mask & V2CE_VOXLOSSES_TEMPORAL) && D % 3 == 1 && I.valid) {
        const double e = A.w3p / 3.0 - A.w3g / 3.0;
        A.t3 += e * e;
    }
}

__device__ __forceinline__ void vol_store(VolAcc &A, double *out, int lane) {
    double v[kVolSlots] = {A.sq, A.ab, A.pa, A.ps, A.pyr[0], A.pyr[1], A.pyr[2], A.t3, A.t5};
#pragma unroll
    for (int k = 0; k < kVolSlots; ++k) {
        wave_sum(v[k]);
        if (lane == 0) out[k] = v[k];
    }
}

// grid (blocks_x, bands, N), 256 threads = 4 waves, each wave one 8 x 8 tile of ONE volume.  kSeq: n is a sequence b of
// [B][L][20][H][W]; waves 2 j and 2 j + 1 walk polarity 0 and 1 of tile j and meet in LDS once per frame for the terms
// that need both polarities (the 20-channel event frame, the compensation sums).  Else n is a volume of [N][D][H][W]
// and the four waves are four tiles.
template <bool kSeq>
__global__ __launch_bounds__(kThreads) void losses_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                          Plan P, double *__restrict__ part, double *__restrict__ comp) {
    __shared__ double xp[kSeq ? 3 : 1][kSeq ? kThreads : 1], xg[kSeq ? 3 : 1][kSeq ? kThreads : 1];
    __shared__ double xc[2][2][8][4];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int q = kSeq ? (wv & 1) : 0;
    const int tile = kSeq ? blockIdx.x * 2 + (wv >> 1) : blockIdx.x * 4 + wv;
    const int band = blockIdx.y, n = blockIdx.z;
    if (!kSeq && tile >= P.tiles) return;                          // the whole wave; volumes have no workgroup barrier
    const bool live = tile < P.tiles;                              // a dead wave of a sequence still meets the barriers
    const int y = band * 8 + (lane >> 3), x = tile * 8 + (lane & 7);
    LaneInfo I;
    I.valid = y < P.H && x < P.W;
    I.ok2 = (y | 1) < P.H && (x | 1) < P.W;
    I.ok4 = (y | 3) < P.H && (x | 3) < P.W;
    I.ok8 = (y | 7) < P.H && (x | 7) < P.W;
    I.lead2 = !(lane & 9); I.lead4 = !(lane & 27); I.lead8 = lane == 0;
    const long long pix = I.valid ? (long long)y * P.W + x : 0;
    const int mask = P.mask;
    const float thr = 0.01f;
    const bool meet = kSeq && (mask & (V2CE_VOXLOSSES_EF | V2CE_VOXLOSSES_COMPENSATION));

    VolAcc A;
    vol_init(A);
    // sequence terms (kSeq only), of this wave's polarity
    float mm[kBins], gm[kBins], pt[kBins];                         // match: max of pred, max of gt, pred at it
    double ms[kBins];                                              // match: sum exp(v - max)
    double clp = 0.0, clg = 0.0;                                   // event frame over all l
    double ef_c = 0.0, efs_c = 0.0;

    const int chunks = kSeq ? P.L : (P.D + kBins - 1) / kBins;
    for (int l = 0; l < chunks; ++l) {
        double efp = 0.0, efg = 0.0, csp = 0.0, csg = 0.0;
        int ccp = 0, ccg = 0;
        const long long first = kSeq ? ((long long)n * P.L + l) * kChannels + q * kBins
                                     : (long long)n * P.D + (long long)l * kBins;
        const int cnt = kSeq ? kBins : min(kBins, P.D - l * kBins);
        float V[kBins], U[kBins];
#pragma unroll
        for (int c = 0; c < kBins; ++c) {
            const bool on = I.valid && c < cnt;
            const long long o = (first + c) * P.plane + pix;
            V[c] = on ? pred[o] : 0.0f;
            U[c] = on ? gt[o] : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < kBins; ++c) {
            if (c >= cnt) continue;
            const float v = V[c], u = U[c];
            const double p = (double)v, g = (double)u;
            vol_step(A, l * kBins + c, p, g, I, mask);
            if (!kSeq) continue;
            if (mask & V2CE_VOXLOSSES_EF) { efp += fabs(p); efg += fabs(g); }
            if (mask & V2CE_VOXLOSSES_COMPENSATION) {
                const bool bp = v > thr, bg = u > thr;
                csp += p * (bp ? 1.0 : 0.0); csg += g * (bg ? 1.0 : 0.0);
                ccp += bp; ccg += bg;
            }
            if (mask & V2CE_VOXLOSSES_MATCH) {
                if (l == 0) {
                    mm[c] = v; ms[c] = 1.0; gm[c] = u; pt[c] = v;
                } else {
                    const double e = exp(-fabs(p - (double)mm[c]));
                    if (v > mm[c]) { ms[c] = ms[c] * e + 1.0; mm[c] = v; }
                    else ms[c] += e;
                    // the first maximum; a NaN counts as the maximum, as in torch.argmax
                    if (u > gm[c] || (u != u && gm[c] == gm[c])) { gm[c] = u; pt[c] = v; }
                }
            }
        }
        if (!meet) continue;
        const int buf = l & 1;                                     // a buffer is rewritten two barriers after its last read
        if (mask & V2CE_VOXLOSSES_COMPENSATION) {
#pragma unroll
            for (int o = 8; o <= 32; o <<= 1) {
                csp += __shfl_xor(csp, o); csg += __shfl_xor(csg, o);
                ccp += __shfl_xor(ccp, o); ccg += __shfl_xor(ccg, o);
            }
            if (q == 1 && lane < 8) {
                double *o = xc[buf][wv >> 1][lane];
                o[0] = csp; o[1] = csg; o[2] = (double)ccp; o[3] = (double)ccg;
            }
        }
        if (mask & V2CE_VOXLOSSES_EF) { xp[kSeq ? buf : 0][kSeq ? threadIdx.x : 0] = efp; xg[kSeq ? buf : 0][kSeq ? threadIdx.x : 0] = efg; }
        __syncthreads();
        if (mask & V2CE_VOXLOSSES_EF) {
            if (I.valid) {
                if (q == 0) {                                      // polarity 0 + polarity 1, pred and gt each
                    const double e = (efp + xp[kSeq ? buf : 0][kSeq ? threadIdx.x + kWave : 0]) -
                                     (efg + xg[kSeq ? buf : 0][kSeq ? threadIdx.x + kWave : 0]);
                    ef_c += e * e;
                }
                const double e0 = efp - efg;
                efs_c += e0 * e0;
            }
            clp += efp; clg += efg;
        }
        if ((mask & V2CE_VOXLOSSES_COMPENSATION) && q == 0 && lane < 8 && x < P.W) {
            const double *i1 = xc[buf][wv >> 1][lane];
            double *o = comp + ((((size_t)n * P.L + l) * P.bands + band) * P.W + x) * 4;
            o[0] = csp + i1[0]; o[1] = csg + i1[1]; o[2] = (double)ccp + i1[2]; o[3] = (double)ccg + i1[3];
        }
    }

    vol_flush(A, P.D, I, mask);
    double s[kSeqSlots] = {ef_c, 0.0, efs_c, 0.0, 0.0, 0.0};
    if (kSeq && (mask & V2CE_VOXLOSSES_EF)) {
        xp[kSeq ? 2 : 0][kSeq ? threadIdx.x : 0] = clp; xg[kSeq ? 2 : 0][kSeq ? threadIdx.x : 0] = clg;
        __syncthreads();
        if (I.valid) {
            if (q == 0) {
                const double e = (clp + xp[kSeq ? 2 : 0][kSeq ? threadIdx.x + kWave : 0]) -
                                 (clg + xg[kSeq ? 2 : 0][kSeq ? threadIdx.x + kWave : 0]);
                s[1] = e * e;
            }
            const double e0 = clp - clg;
            s[3] = e0 * e0;
        }
    }
    if (!live) return;
    double *out = part + ((((size_t)n * P.bands + band) * P.tiles + tile) * (kSeq ? 2 : 1) + q) * P.rec;
    vol_store(A, out, lane);
    if (!kSeq) return;
    if ((mask & V2CE_VOXLOSSES_MATCH) && I.valid) {
#pragma unroll
        for (int c = 0; c < kBins; ++c) {
            const double gap = (double)mm[c] - (double)pt[c];     // >= 0
            s[4] += gap + log(ms[c]);
            s[5] += -gap < -80.0 ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < kSeqSlots; ++k) {
        wave_sum(s[k]);
        if (lane == 0) out[kVolSlots + k] = s[k];
    }
}

// grid N: the partial records of n in a fixed order (strided per thread, then a fixed tree) -> stats[n]
template <bool kSeq>
__global__ __launch_bounds__(kFinishThreads) void finish_kernel(Plan P, const double *__restrict__ part,
                                                               const double *__restrict__ comp,
                                                               v2ce_voxlosses_stats *__restrict__ stats) {
    __shared__ double red[kFinishThreads];
    const int n = blockIdx.x, t = threadIdx.x;
    const int nrec = P.bands * P.tiles;
    const double *pn = part + (size_t)n * nrec * (kSeq ? 2 : 1) * P.rec;
    auto tree = [&](double v) -> double {
        red[t] = v;
        __syncthreads();
        for (int o = kFinishThreads / 2; o; o >>= 1) {
            if (t < o) red[t] = red[t] + red[t + o];
            __syncthreads();
        }
        const double r = red[0];
        __syncthreads();
        return r;
    };
    constexpr int NP = kSeq ? 2 : 1;
    auto slot = [&](int k, int q) -> double {
        double s = 0.0;
        for (int i = t; i < nrec; i += kFinishThreads) s += pn[((size_t)i * NP + q) * P.rec + k];
        return tree(s);
    };
    double vol[kVolSlots], seq[kSeqSlots] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, comp_sq = 0.0;
    for (int k = 0; k < kVolSlots; ++k) {
        vol[k] = slot(k, 0);
        if (kSeq) vol[k] = vol[k] + slot(k, 1);                   // polarity 0 + polarity 1
    }
    if (kSeq) {
        for (int k = 0; k < kSeqSlots; ++k) seq[k] = slot(kVolSlots + k, 0) + slot(kVolSlots + k, 1);
        if (P.mask & V2CE_VOXLOSSES_COMPENSATION) {
            double s = 0.0;
            const long long cols = (long long)P.L * P.W;
            for (long long i = t; i < cols; i += kFinishThreads) {
                const int l = (int)(i / P.W), x = (int)(i % P.W);
                double sp = 0.0, sg = 0.0, cp = 0.0, cg = 0.0;
                for (int band = 0; band < P.bands; ++band) {
                    const double *o = comp + ((((size_t)n * P.L + l) * P.bands + band) * P.W + x) * 4;
                    sp += o[0]; sg += o[1]; cp += o[2]; cg += o[3];
                }
                const double e = sp / fmax(cp, 1.0) - sg / fmax(cg, 1.0);
                s += e * e;
            }
            comp_sq = tree(s);
        }
    }
    if (t != 0) return;
    v2ce_voxlosses_stats *out = stats + n;
    const long long HW = P.plane, D = P.D;
    const bool pyr = P.mask & V2CE_VOXLOSSES_PYRAMID, tmp = P.mask & V2CE_VOXLOSSES_TEMPORAL;
    const bool ef = P.mask & V2CE_VOXLOSSES_EF, cmp = P.mask & V2CE_VOXLOSSES_COMPENSATION;
    const bool mt = P.mask & V2CE_VOXLOSSES_MATCH;
    out->struct_size = (int64_t)sizeof(v2ce_voxlosses_stats);
    out->term_mask = P.mask;
    out->n = NP * D * HW;
    out->sq_sum = vol[0]; out->abs_diff_sum = vol[1]; out->pred_abs_sum = vol[2]; out->pred_sq_sum = vol[3];
    for (int q = 0; q < 3; ++q) {
        const int k = 2 << q;
        out->pyr_n[q] = pyr ? NP * (D / k) * (P.H / k) * (P.W / k) : 0;
        out->pyr_sq_sum[q] = pyr ? vol[4 + q] : 0.0;
    }
    out->temporal_n[0] = tmp ? NP * HW * ((D - 1) / 3 + 1) : 0;
    out->temporal_n[1] = tmp ? NP * HW * (D / 5) : 0;
    out->temporal_sq_sum[0] = tmp ? vol[7] : 0.0;
    out->temporal_sq_sum[1] = tmp ? vol[8] : 0.0;
    const long long L = P.L;
    const long long ef_n[4] = {L * HW, HW, L * 2 * HW, 2 * HW};
    for (int q = 0; q < 4; ++q) {
        out->ef_n[q] = kSeq && ef ? ef_n[q] : 0;
        out->ef_sq_sum[q] = kSeq && ef ? seq[q] : 0.0;
    }
    out->comp_n = kSeq && cmp ? L * P.W : 0;
    out->comp_sq_sum = kSeq && cmp ? comp_sq : 0.0;
    out->match_n = kSeq && mt ? kChannels * HW : 0;
    out->match_sum = kSeq && mt ? seq[4] : 0.0;
    out->match_low = kSeq && mt ? (int64_t)seq[5] : 0;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// seq: N = B sequences of L frames; else N volumes of D planes
bool make_plan(bool seq, int N, int DL, int H, int W, int mask, Plan &P) {
    if (N < 1 || N > 65535 || DL < 1 || H < 1 || W < 1) return false;
    if (seq && DL > (1 << 24)) return false;
    const long long D = seq ? (long long)DL * kBins : DL;
    const long long planes = (seq ? 2 : 1) * D;
    if ((long long)H * W >= (1ll << 31) || D >= (1ll << 28) || (long long)N * planes * H * W >= (1ll << 40)) return false;
    if (mask < 0 || (mask & ~kAllTerms)) return false;
    if (!seq && (mask & ~(V2CE_VOXLOSSES_PYRAMID | V2CE_VOXLOSSES_TEMPORAL))) return false;
    if ((mask & V2CE_VOXLOSSES_PYRAMID) && (D < 8 || H < 8 || W < 8)) return false;
    if ((mask & V2CE_VOXLOSSES_TEMPORAL) && D < 5) return false;
    P.N = N; P.D = (int)D; P.L = seq ? DL : 0; P.H = H; P.W = W;
    P.bands = (H + 7) / 8; P.tiles = (W + 7) / 8; P.blocks_x = seq ? (P.tiles + 1) / 2 : (P.tiles + 3) / 4;
    if (P.bands > 65535) return false;
    P.mask = mask;
    P.rec = seq ? kVolSlots + kSeqSlots : kVolSlots;
    P.plane = (long long)H * W;
    P.comp_off = align256((size_t)N * P.bands * P.tiles * (seq ? 2 : 1) * P.rec * sizeof(double));
    P.total = P.comp_off;
    if (seq && (mask & V2CE_VOXLOSSES_COMPENSATION))
        P.total += align256((size_t)N * P.L * P.bands * W * 4 * sizeof(double));
    return true;
}

template <bool kSeq>
int run(const char *name, const float *pred, const float *gt, int N, int DL, int H, int W, int mask,
        v2ce_voxlosses_stats *stats, size_t stats_struct_size, void *workspace, size_t workspace_bytes,
        v2ce_stream_t stream) {
    V2CE_REQUIRE(stats_struct_size == sizeof(v2ce_voxlosses_stats), V2CE_ERR_BAD_ARG,
                 "%s: stats_struct_size %zu, this library writes v2ce_voxlosses_stats of %zu bytes", name,
                 stats_struct_size, sizeof(v2ce_voxlosses_stats));
    Plan P;
    V2CE_REQUIRE(make_plan(kSeq, N, DL, H, W, mask, P), V2CE_ERR_BAD_ARG,
                 "%s: needs 1 <= %s <= 65535, H, W >= 1, a term mask of known bits%s, min(D, H, W) >= 8 for the pyramid "
                 "(the 8-wide window must fit) and D >= 5 for the temporal term", name, kSeq ? "B" : "N",
                 kSeq ? "" : " (pyramid and temporal only)");
    V2CE_REQUIRE(pred && gt && stats && workspace, V2CE_ERR_BAD_ARG, "%s: null pointer", name);
    V2CE_REQUIRE(workspace_bytes >= P.total, V2CE_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", name,
                 workspace_bytes, P.total);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    double *part = reinterpret_cast<double *>(ws);
    double *comp = reinterpret_cast<double *>(ws + P.comp_off);
    const dim3 grid((unsigned)P.blocks_x, (unsigned)P.bands, (unsigned)N);
    hipLaunchKernelGGL(losses_kernel<kSeq>, grid, dim3(kThreads), 0, st, pred, gt, P, part, comp);
    hipLaunchKernelGGL(finish_kernel<kSeq>, dim3((unsigned)N), dim3(kFinishThreads), 0, st, P, part, comp, stats);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_voxlosses_workspace_bytes(int B, int L, int C, int H, int W, int term_mask) {
    Plan P;
    return C == kChannels && make_plan(true, B, L, H, W, term_mask, P) ? P.total : 0;
}

extern "C" int v2ce_voxlosses(const float *pred, const float *gt, int B, int L, int C, int H, int W, int term_mask,
                              v2ce_voxlosses_stats *stats, size_t stats_struct_size, void *workspace,
                              size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    V2CE_REQUIRE(C == kChannels, V2CE_ERR_BAD_ARG, "v2ce_voxlosses: C = %d, only 20 channels (2 polarities x 10 bins)", C);
    return run<true>("v2ce_voxlosses", pred, gt, B, L, H, W, term_mask, stats, stats_struct_size, workspace,
                     workspace_bytes, stream);
}

extern "C" size_t v2ce_volume_losses_workspace_bytes(int N, int D, int H, int W, int term_mask) {
    Plan P;
    return make_plan(false, N, D, H, W, term_mask, P) ? P.total : 0;
}

extern "C" int v2ce_volume_losses(const float *pred, const float *gt, int N, int D, int H, int W, int term_mask,
                                  v2ce_voxlosses_stats *stats, size_t stats_struct_size, void *workspace,
                                  size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    return run<false>("v2ce_volume_losses", pred, gt, N, D, H, W, term_mask, stats, stats_struct_size, workspace,
                      workspace_bytes, stream);
}
