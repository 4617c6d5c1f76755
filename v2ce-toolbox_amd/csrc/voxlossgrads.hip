// voxlossgrads.hip -- the gradient with respect to pred of the stage-1 voxel loss terms (the backward of voxlosses.hip),
// on gfx950.  include/v2ce_hip_grad.h states the formula per element; the host hands over one f64 factor per linear
// piece, so the kernels know nothing of loss lists.
//
// Two entries share the kernels:
//   v2ce_voxloss_grads      pred, gt, grad [B][L][20][H][W]: every term
//   v2ce_volume_loss_grads  pred, gt, grad [N][D][H][W]:     the elementwise, pyramid and temporal terms
// In the 5-D layout volume (b, p) owns the planes d = l * 10 + c at ((b L + l) 20 + p 10 + c) H W, as in the forward.
//
// prepare (5-D only, launched when an event-frame, compensation or match factor is non-zero): the forward's sequence
// walk -- a wave owns 8 x 8 pixels of one polarity, a lane one pixel column, waves 2 j and 2 j + 1 meet in LDS once per
// frame -- and leaves in the workspace what a pixel's gradient needs from its whole walk over l:
//   event frames  per (b, l, p, pixel)  a_ef[0] E0 + a_ef[2] E2, and per (b, p, pixel)  a_ef[1] E1 + a_ef[3] E3
//   match         per (b, channel, pixel)  logsumexp over l of pred and the first argmax over l of gt
//   compensation  the masked sums and counts per (b, l, band of 8 rows, w); a small finish turns them into
//                 e / max(cp, 1) per column (b, l, w)
//
// gradient: a wave owns 8 x 8 pixels of ONE volume, four tiles side by side per workgroup, and walks the planes in
// groups of 8, one k = 8 window.  A lane keeps 16 planes of its pixel in registers: the group, the 4 planes before it
// and the 4 after it, so every 3- and 5-window of a plane of the group is a sum of registers (planes outside [0, D) are
// zeros, which is the padding of AvgPool1d(3, padding 1)); advancing a group loads 8 new planes, so every input byte is
// loaded once.  The nested 2 / 4 / 8 window sums are the forward's butterflies over lane bits 1 / 8, 2 / 16, 4 / 32.
// Which registers form a plane's window depends on d mod 3 and d mod 5, which are wave-uniform: a scalar branch picks
// among statically indexed sums.
//
// Arithmetic: as the forward, every difference, sum, quotient, exp and log is f64 from the f32 inputs, v > 0.01f is an
// f32 compare; a term whose factor is zero is not evaluated (a NaN elsewhere does not leak through 0 * NaN).  The terms
// are added in one fixed order, multiplied by upstream, and rounded to f32 at the store.  No atomics; both entries run
// the same code on the same values, so the volume entry reproduces the 5-D entry bit for bit.
#include "common.h"

#include "../../include/v2ce_hip_grad.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;             // 4 waves
constexpr int kChannels = 20;
constexpr int kBins = 10;
constexpr int kGroup = 8;                 // planes per step of the gradient walk: one k = 8 window
constexpr int kHalo = 4;                  // planes kept before and after the group: a 5-window reaches that far

struct Coef {
    double sq, pyr[3], t3, t5, ef[4], comp, match, l1, l2;
};

struct Plan {
    int N, D, L, H, W;                    // N volumes or sequences; D planes per volume (10 L for sequences)
    int bands, tiles;                     // ceil(H / 8), ceil(W / 8)
    bool pyr, t3, t5, ef, comp, match;    // which term families are on
    long long plane;                      // H * W
    // byte offsets into the workspace (sequences only): event frames per frame and over all frames, match logsumexp and
    // argmax, compensation partials and quotients
    size_t f_off, f2_off, lse_off, t_off, cpart_off, r_off, total;
};

__device__ __forceinline__ double sign_of(double p) { return (double)(p > 0.0) - (double)(p < 0.0); }

// grid (ceil(tiles / 2), bands, B), 256 threads: waves 2 j and 2 j + 1 walk polarity 0 and 1 of tile j
__global__ __launch_bounds__(kThreads) void prepare_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                           Plan P, Coef K, double *__restrict__ F, double *__restrict__ F2,
                                                           double *__restrict__ lse, int *__restrict__ tix,
                                                           double *__restrict__ cpart) {
    __shared__ double xp[3][kThreads], xg[3][kThreads];
    __shared__ double xc[2][2][8][4];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int q = wv & 1, tile = blockIdx.x * 2 + (wv >> 1);
    const int band = blockIdx.y, b = blockIdx.z;
    const int y = band * 8 + (lane >> 3), x = tile * 8 + (lane & 7);
    const bool valid = tile < P.tiles && y < P.H && x < P.W;      // a dead wave still meets the barriers
    const long long pix = valid ? (long long)y * P.W + x : 0;
    const int partner = q ? (int)threadIdx.x - kWave : (int)threadIdx.x + kWave;
    const float thr = 0.01f;

    float mm[kBins], gm[kBins];                                    // match: max of pred, max of gt
    double ms[kBins];                                              // match: sum exp(v - max)
    int tt[kBins];                                                 // match: the first argmax of gt
    double clp = 0.0, clg = 0.0;                                   // event frame over all l

    for (int l = 0; l < P.L; ++l) {
        double efp = 0.0, efg = 0.0, csp = 0.0, csg = 0.0;
        int ccp = 0, ccg = 0;
        const long long first = ((long long)b * P.L + l) * kChannels + q * kBins;
        float V[kBins], U[kBins];
#pragma unroll
        for (int c = 0; c < kBins; ++c) {
            const long long o = (first + c) * P.plane + pix;
            V[c] = valid ? pred[o] : 0.0f;
            U[c] = valid ? gt[o] : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < kBins; ++c) {
            const float v = V[c], u = U[c];
            const double p = (double)v, g = (double)u;
            if (P.ef) { efp += fabs(p); efg += fabs(g); }
            if (P.comp) {
                const bool bp = v > thr, bg = u > thr;
                csp += p * (bp ? 1.0 : 0.0); csg += g * (bg ? 1.0 : 0.0);
                ccp += bp; ccg += bg;
            }
            if (P.match) {
                if (l == 0) {
                    mm[c] = v; ms[c] = 1.0; gm[c] = u; tt[c] = 0;
                } else {
                    const double e = exp(-fabs(p - (double)mm[c]));
                    if (v > mm[c]) { ms[c] = ms[c] * e + 1.0; mm[c] = v; }
                    else ms[c] += e;
                    // the first maximum; a NaN counts as the maximum, as in torch.argmax
                    if (u > gm[c] || (u != u && gm[c] == gm[c])) { gm[c] = u; tt[c] = l; }
                }
            }
        }
        if (!P.ef && !P.comp) continue;
        const int buf = l & 1;                                     // a buffer is rewritten two barriers after its last read
        if (P.comp) {
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
        if (P.ef) { xp[buf][threadIdx.x] = efp; xg[buf][threadIdx.x] = efg; }
        __syncthreads();
        if (P.ef) {
            if (valid) {
                const double op = xp[buf][partner], og = xg[buf][partner];
                const double e_c = (q ? op + efp : efp + op) - (q ? og + efg : efg + og);   // polarity 0 + polarity 1
                const double e_s = efp - efg;
                F[(((long long)b * P.L + l) * 2 + q) * P.plane + pix] = K.ef[0] * e_c + K.ef[2] * e_s;
            }
            clp += efp; clg += efg;
        }
        if (P.comp && q == 0 && lane < 8 && tile < P.tiles && x < P.W) {
            const double *i1 = xc[buf][wv >> 1][lane];
            double *o = cpart + ((((size_t)b * P.L + l) * P.bands + band) * P.W + x) * 4;
            o[0] = csp + i1[0]; o[1] = csg + i1[1]; o[2] = (double)ccp + i1[2]; o[3] = (double)ccg + i1[3];
        }
    }

    if (P.ef) {
        xp[2][threadIdx.x] = clp; xg[2][threadIdx.x] = clg;
        __syncthreads();
        if (valid) {
            const double op = xp[2][partner], og = xg[2][partner];
            const double e_cl = (q ? op + clp : clp + op) - (q ? og + clg : clg + og);
            const double e_scl = clp - clg;
            F2[((long long)b * 2 + q) * P.plane + pix] = K.ef[1] * e_cl + K.ef[3] * e_scl;
        }
    }
    if (P.match && valid) {
#pragma unroll
        for (int c = 0; c < kBins; ++c) {
            const long long o = (((long long)b * 2 + q) * kBins + c) * P.plane + pix;
            lse[o] = (double)mm[c] + log(ms[c]);
            tix[o] = tt[c];
        }
    }
}

// one thread per column (b, l, w): the band partials in order -> e / max(cp, 1)
__global__ __launch_bounds__(kThreads) void comp_finish_kernel(Plan P, const double *__restrict__ cpart,
                                                               double *__restrict__ R) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)P.N * P.L * P.W) return;
    const long long bl = i / P.W;
    const int x = (int)(i % P.W);
    double sp = 0.0, sg = 0.0, cp = 0.0, cg = 0.0;
    for (int band = 0; band < P.bands; ++band) {
        const double *o = cpart + (((size_t)bl * P.bands + band) * P.W + x) * 4;
        sp += o[0]; sg += o[1]; cp += o[2]; cg += o[3];
    }
    const double e = sp / fmax(cp, 1.0) - sg / fmax(cg, 1.0);
    R[i] = e / fmax(cp, 1.0);
}

// the sum of n consecutive planes from register index s (static after unrolling), in plane order
template <int n>
__device__ __forceinline__ double window(const float (&X)[kGroup + 2 * kHalo], int s) {
    double v = (double)X[s];
#pragma unroll
    for (int k = 1; k < n; ++k) v += (double)X[s + k];
    return v;
}

// grid (ceil(tiles / 4) * (kSeq ? 2 : 1), bands, B or N), 256 threads = 4 tiles of one volume.  kSeq: blockIdx.z is a
// sequence b and blockIdx.x & 1 its polarity; the volume is n = 2 b + p.
template <bool kSeq>
__global__ __launch_bounds__(kThreads) void grad_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                        Plan P, Coef K, const float *__restrict__ upstream,
                                                        const double *__restrict__ F, const double *__restrict__ F2,
                                                        const double *__restrict__ lse, const int *__restrict__ tix,
                                                        const double *__restrict__ R, float *__restrict__ grad) {
    constexpr int kRegs = kGroup + 2 * kHalo;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int q = kSeq ? (blockIdx.x & 1) : 0;
    const int tile = (kSeq ? blockIdx.x >> 1 : blockIdx.x) * 4 + wv;
    const int band = blockIdx.y;
    const long long n = kSeq ? (long long)blockIdx.z * 2 + q : blockIdx.z;
    if (tile >= P.tiles) return;                                   // the whole wave; there is no workgroup barrier
    const int y = band * 8 + (lane >> 3), x = tile * 8 + (lane & 7);
    const bool valid = y < P.H && x < P.W;
    const bool ok2 = (y | 1) < P.H && (x | 1) < P.W;
    const bool ok4 = (y | 3) < P.H && (x | 3) < P.W;
    const bool ok8 = (y | 7) < P.H && (x | 7) < P.W;
    const long long pix = valid ? (long long)y * P.W + x : 0;
    const int D = P.D;
    const double up = upstream ? (double)upstream[0] : 1.0;
    const float thr = 0.01f;
    // plane d of this volume, as a plane index of the tensor
    auto plane_of = [&](int d) -> long long {
        return kSeq ? ((long long)blockIdx.z * P.L + d / kBins) * kChannels + q * kBins + d % kBins : n * D + d;
    };

    float Xp[kRegs], Xg[kRegs];                                    // register i holds plane d0 - kHalo + i
#pragma unroll
    for (int i = 0; i < kRegs; ++i) {
        const int d = i - kHalo;
        const bool on = valid && d >= 0 && d < D;
        const long long o = on ? plane_of(d) * P.plane + pix : 0;
        Xp[i] = on ? pred[o] : 0.0f;
        Xg[i] = on ? gt[o] : 0.0f;
    }
    const double f2 = kSeq && P.ef && valid ? F2[n * P.plane + pix] : 0.0;
    const int last3 = (D - 1) / 3, count5 = D / 5;

    for (int d0 = 0; d0 < D; d0 += kGroup) {
        // the 8 planes that enter when the walk advances
        float Np[kGroup], Ng[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const int d = d0 + kGroup + kHalo + i;
            const bool on = valid && d < D;
            const long long o = on ? plane_of(d) * P.plane + pix : 0;
            Np[i] = on ? pred[o] : 0.0f;
            Ng[i] = on ? gt[o] : 0.0f;
        }
        // per-frame and per-channel state of the sequence terms: a group touches at most two frames
        const int la = d0 / kBins, lb = min(d0 + kGroup - 1, D - 1) / kBins;
        double Fa = 0.0, Fb = 0.0, Ra = 0.0, Rb = 0.0;
        double ls[kGroup] = {};
        int ti[kGroup] = {};
        if (kSeq && valid) {
            if (P.ef) {
                Fa = F[(((long long)blockIdx.z * P.L + la) * 2 + q) * P.plane + pix];
                Fb = F[(((long long)blockIdx.z * P.L + lb) * 2 + q) * P.plane + pix];
            }
            if (P.comp) {
                Ra = R[((long long)blockIdx.z * P.L + la) * P.W + x];
                Rb = R[((long long)blockIdx.z * P.L + lb) * P.W + x];
            }
            if (P.match) {
#pragma unroll
                for (int i = 0; i < kGroup; ++i) {
                    const int d = min(d0 + i, D - 1);
                    const long long o = (n * kBins + d % kBins) * P.plane + pix;
                    ls[i] = lse[o];
                    ti[i] = tix[o];
                }
            }
        }

        // pooled differences of the nested windows of this group (zero planes beyond D are never used: see below)
        double e2[4] = {0.0, 0.0, 0.0, 0.0}, e4[2] = {0.0, 0.0}, e8 = 0.0;
        if (P.pyr) {
            double a8p = 0.0, a8g = 0.0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                double a4p = 0.0, a4g = 0.0;
#pragma unroll
                for (int j = 2 * h; j < 2 * h + 2; ++j) {
                    double sp = (double)Xp[kHalo + 2 * j], sg = (double)Xg[kHalo + 2 * j];
                    sp += (double)Xp[kHalo + 2 * j + 1]; sg += (double)Xg[kHalo + 2 * j + 1];
                    sp += __shfl_xor(sp, 1); sg += __shfl_xor(sg, 1);
                    sp += __shfl_xor(sp, 8); sg += __shfl_xor(sg, 8);
                    e2[j] = sp * 0.125 - sg * 0.125;
                    a4p += sp; a4g += sg;
                }
                a4p += __shfl_xor(a4p, 2); a4g += __shfl_xor(a4g, 2);
                a4p += __shfl_xor(a4p, 16); a4g += __shfl_xor(a4g, 16);
                e4[h] = a4p * 0.015625 - a4g * 0.015625;
                a8p += a4p; a8g += a4g;
            }
            a8p += __shfl_xor(a8p, 4); a8g += __shfl_xor(a8g, 4);
            a8p += __shfl_xor(a8p, 32); a8g += __shfl_xor(a8g, 32);
            e8 = a8p * 0.001953125 - a8g * 0.001953125;
        }

#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const int d = d0 + i;                                  // wave-uniform
            if (d < D) {
                const float v = Xp[kHalo + i];
                const double p = (double)v, g = (double)Xg[kHalo + i];
                double acc = 0.0;
                if (K.sq != 0.0) acc += K.sq * (p - g);
                if (P.pyr) {                                       // windows inside the floored extents only
                    if (K.pyr[0] != 0.0 && ok2 && (d | 1) < D) acc += K.pyr[0] * e2[i >> 1];
                    if (K.pyr[1] != 0.0 && ok4 && (d | 3) < D) acc += K.pyr[1] * e4[i >> 2];
                    if (K.pyr[2] != 0.0 && ok8 && (d | 7) < D) acc += K.pyr[2] * e8;
                }
                if (P.t3 && (d + 1) / 3 <= last3) {                // window {3j-1, 3j, 3j+1}, j = (d + 1) / 3, divisor 3
                    const int r = (d + 1) % 3;
                    double sp, sg;
                    if (r == 0) { sp = window<3>(Xp, kHalo + i); sg = window<3>(Xg, kHalo + i); }
                    else if (r == 1) { sp = window<3>(Xp, kHalo + i - 1); sg = window<3>(Xg, kHalo + i - 1); }
                    else { sp = window<3>(Xp, kHalo + i - 2); sg = window<3>(Xg, kHalo + i - 2); }
                    acc += K.t3 * (sp / 3.0 - sg / 3.0);
                }
                if (P.t5 && d / 5 < count5) {                      // window {5j .. 5j+4}, j = d / 5
                    const int r = d % 5;
                    double sp, sg;
                    if (r == 0) { sp = window<5>(Xp, kHalo + i); sg = window<5>(Xg, kHalo + i); }
                    else if (r == 1) { sp = window<5>(Xp, kHalo + i - 1); sg = window<5>(Xg, kHalo + i - 1); }
                    else if (r == 2) { sp = window<5>(Xp, kHalo + i - 2); sg = window<5>(Xg, kHalo + i - 2); }
                    else if (r == 3) { sp = window<5>(Xp, kHalo + i - 3); sg = window<5>(Xg, kHalo + i - 3); }
                    else { sp = window<5>(Xp, kHalo + i - 4); sg = window<5>(Xg, kHalo + i - 4); }
                    acc += K.t5 * (sp / 5.0 - sg / 5.0);
                }
                if (kSeq) {
                    const int l = d / kBins;
                    if (P.ef) acc += sign_of(p) * ((l == la ? Fa : Fb) + f2);
                    if (P.comp && v > thr) acc += K.comp * (l == la ? Ra : Rb);
                    if (P.match) acc += K.match * (exp(p - ls[i]) - (ti[i] == l ? 1.0 : 0.0));
                    if (K.l1 != 0.0) acc += K.l1 * sign_of(p);
                    if (K.l2 != 0.0) acc += K.l2 * p;
                }
                if (valid) grad[plane_of(d) * P.plane + pix] = (float)(acc * up);
            }
        }

#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            Xp[i] = Xp[i + kGroup]; Xg[i] = Xg[i + kGroup];
            Xp[i + kGroup] = Np[i]; Xg[i + kGroup] = Ng[i];
        }
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// seq: N = B sequences of DL = L frames; else N volumes of DL = D planes
bool make_plan(bool seq, int N, int DL, int H, int W, const v2ce_voxloss_grad_coeffs *c, size_t coef_struct_size,
               Plan &P, Coef &K) {
    if (!c || coef_struct_size != sizeof(v2ce_voxloss_grad_coeffs) ||
        c->struct_size != (int64_t)sizeof(v2ce_voxloss_grad_coeffs))
        return false;
    if (N < 1 || N > 65535 || DL < 1 || H < 1 || W < 1) return false;
    if (seq && DL > (1 << 24)) return false;
    const long long D = seq ? (long long)DL * kBins : DL;
    const long long planes = (seq ? 2 : 1) * D;
    if ((long long)H * W >= (1ll << 31) || D >= (1ll << 28) || (long long)N * planes * H * W >= (1ll << 40)) return false;
    K.sq = c->a_sq; K.t3 = c->a_t3; K.t5 = c->a_t5; K.comp = c->a_comp; K.match = c->a_match; K.l1 = c->a_l1; K.l2 = c->a_l2;
    for (int q = 0; q < 3; ++q) K.pyr[q] = c->a_pyr[q];
    for (int q = 0; q < 4; ++q) K.ef[q] = c->a_ef[q];
    P.pyr = K.pyr[0] != 0.0 || K.pyr[1] != 0.0 || K.pyr[2] != 0.0;
    P.t3 = K.t3 != 0.0; P.t5 = K.t5 != 0.0;
    P.ef = K.ef[0] != 0.0 || K.ef[1] != 0.0 || K.ef[2] != 0.0 || K.ef[3] != 0.0;
    P.comp = K.comp != 0.0; P.match = K.match != 0.0;
    if (!seq && (P.ef || P.comp || P.match || K.l1 != 0.0 || K.l2 != 0.0)) return false;
    if (P.pyr && (D < 8 || H < 8 || W < 8)) return false;
    if ((P.t3 || P.t5) && D < 5) return false;
    P.N = N; P.D = (int)D; P.L = seq ? DL : 0; P.H = H; P.W = W;
    P.bands = (H + 7) / 8; P.tiles = (W + 7) / 8;
    if (P.bands > 65535) return false;
    P.plane = (long long)H * W;
    const size_t HW = (size_t)P.plane, B = (size_t)N, L = (size_t)P.L;
    size_t at = 0;
    P.f_off = at;     at += P.ef ? align256(B * L * 2 * HW * sizeof(double)) : 0;
    P.f2_off = at;    at += P.ef ? align256(B * 2 * HW * sizeof(double)) : 0;
    P.lse_off = at;   at += P.match ? align256(B * kChannels * HW * sizeof(double)) : 0;
    P.t_off = at;     at += P.match ? align256(B * kChannels * HW * sizeof(int)) : 0;
    P.cpart_off = at; at += P.comp ? align256(B * L * P.bands * W * 4 * sizeof(double)) : 0;
    P.r_off = at;     at += P.comp ? align256(B * L * W * sizeof(double)) : 0;
    P.total = at ? at : 256;                                       // never 0: that is the refusal
    return true;
}

template <bool kSeq>
int run(const char *name, const float *pred, const float *gt, int N, int DL, int H, int W,
        const v2ce_voxloss_grad_coeffs *coef, size_t coef_struct_size, const float *upstream, float *grad, void *workspace,
        size_t workspace_bytes, v2ce_stream_t stream) {
    V2CE_REQUIRE(coef, V2CE_ERR_BAD_ARG, "%s: null pointer", name);
    V2CE_REQUIRE(coef_struct_size == sizeof(v2ce_voxloss_grad_coeffs) &&
                 coef->struct_size == (int64_t)sizeof(v2ce_voxloss_grad_coeffs), V2CE_ERR_BAD_ARG,
                 "%s: coef_struct_size %zu / coef->struct_size %lld, this library reads v2ce_voxloss_grad_coeffs of %zu bytes",
                 name, coef_struct_size, (long long)coef->struct_size, sizeof(v2ce_voxloss_grad_coeffs));
    Plan P;
    Coef K;
    V2CE_REQUIRE(make_plan(kSeq, N, DL, H, W, coef, coef_struct_size, P, K), V2CE_ERR_BAD_ARG,
                 "%s: needs 1 <= %s <= 65535, H, W >= 1%s, min(D, H, W) >= 8 for a non-zero pyramid factor (the 8-wide "
                 "window must fit) and D >= 5 for a non-zero temporal factor", name, kSeq ? "B" : "N",
                 kSeq ? "" : ", only the a_sq, a_pyr, a_t3 and a_t5 factors non-zero");
    V2CE_REQUIRE(pred && gt && grad && workspace, V2CE_ERR_BAD_ARG, "%s: null pointer", name);
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, V2CE_ERR_BAD_ARG, "%s: workspace must be 8-byte aligned",
                 name);
    V2CE_REQUIRE(workspace_bytes >= P.total, V2CE_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", name,
                 workspace_bytes, P.total);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    double *F = reinterpret_cast<double *>(ws + P.f_off), *F2 = reinterpret_cast<double *>(ws + P.f2_off);
    double *lse = reinterpret_cast<double *>(ws + P.lse_off);
    int *tix = reinterpret_cast<int *>(ws + P.t_off);
    double *cpart = reinterpret_cast<double *>(ws + P.cpart_off), *R = reinterpret_cast<double *>(ws + P.r_off);
    if (kSeq && (P.ef || P.comp || P.match)) {
        const dim3 grid((unsigned)((P.tiles + 1) / 2), (unsigned)P.bands, (unsigned)N);
        hipLaunchKernelGGL(prepare_kernel, grid, dim3(kThreads), 0, st, pred, gt, P, K, F, F2, lse, tix, cpart);
        if (P.comp) {
            const long long cols = (long long)N * P.L * P.W;
            hipLaunchKernelGGL(comp_finish_kernel, dim3((unsigned)((cols + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                               P, cpart, R);
        }
    }
    const dim3 grid((unsigned)(((P.tiles + 3) / 4) * (kSeq ? 2 : 1)), (unsigned)P.bands, (unsigned)N);
    hipLaunchKernelGGL(grad_kernel<kSeq>, grid, dim3(kThreads), 0, st, pred, gt, P, K, upstream, F, F2, lse, tix, R, grad);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_voxloss_grads_workspace_bytes(int B, int L, int C, int H, int W,
                                                     const v2ce_voxloss_grad_coeffs *coef, size_t coef_struct_size) {
    Plan P;
    Coef K;
    return C == kChannels && make_plan(true, B, L, H, W, coef, coef_struct_size, P, K) ? P.total : 0;
}

extern "C" int v2ce_voxloss_grads(const float *pred, const float *gt, int B, int L, int C, int H, int W,
                                  const v2ce_voxloss_grad_coeffs *coef, size_t coef_struct_size, const float *upstream,
                                  float *grad, void *workspace, size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    V2CE_REQUIRE(C == kChannels, V2CE_ERR_BAD_ARG, "v2ce_voxloss_grads: C = %d, only 20 channels (2 polarities x 10 bins)", C);
    return run<true>("v2ce_voxloss_grads", pred, gt, B, L, H, W, coef, coef_struct_size, upstream, grad, workspace,
                     workspace_bytes, stream);
}

extern "C" size_t v2ce_volume_loss_grads_workspace_bytes(int N, int D, int H, int W, const v2ce_voxloss_grad_coeffs *coef,
                                                         size_t coef_struct_size) {
    Plan P;
    Coef K;
    return make_plan(false, N, D, H, W, coef, coef_struct_size, P, K) ? P.total : 0;
}

extern "C" int v2ce_volume_loss_grads(const float *pred, const float *gt, int N, int D, int H, int W,
                                      const v2ce_voxloss_grad_coeffs *coef, size_t coef_struct_size, const float *upstream,
                                      float *grad, void *workspace, size_t workspace_bytes, v2ce_stream_t stream) {
    clear_error();
    return run<false>("v2ce_volume_loss_grads", pred, gt, N, D, H, W, coef, coef_struct_size, upstream, grad, workspace,
                      workspace_bytes, stream);
}
