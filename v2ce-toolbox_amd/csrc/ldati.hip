// ldati.hip -- LDATI (stage 2) for gfx950: voxel grid -> stably sorted (t, x, y, p) event list.
//
// Replaces /root/reference/scripts/LDATI.py:80-106 (y_relocate), :13-51 (slope), :126-214
// (sample_voxel_statistical) and :217-310 (pick_elements / pick_and_sort).
//
// Design.  Every timestamp is a pure function of (voxel column, draw index) --
// counter-based Philox, or a replayed uniform tensor.  The reference's output order inside a
// (frame, bin) SEGMENT is the stable sort by timestamp of [neg singles, neg multis, pos singles,
// pos multis], each listed pixel-row-major; i.e. the order of the key (timestamp, category, pixel).
// Two-level counting sort with the pixel order kept BY CONSTRUCTION, so no pass ever sorts on the
// pixel bits:
//
//   count      : workgroup per (frame, polarity, 2048-pixel TILE): relocation recurrence in
//                registers -> events per (tile, bin); one tiny scan kernel -> per-tile record
//                offsets, segment offsets, statistics the host needs to allocate.
//   tile pass  : workgroup per tile, bin by bin.  Timestamps are computed ONCE: singles and
//                4-draw multi-event UNITS are compacted so that every lane of the f64 / Philox +
//                sqrt / divide code does useful work; the records land in LDS in pixel order.  A
//                stable counting sort on the COARSE key (timestamp >> shift; per-wave histograms +
//                ballot match-any ranks -- deterministic, no atomics decide an order) groups them
//                by bucket, and the tile's 4-byte records leave as ONE contiguous, coalesced run
//                per bin.
//   bucket scan: per segment, bucket totals over the tiles -> output offsets.
//   bucket sort: workgroup per (segment, bucket): gathers the tiles' runs in tile order (= pixel
//                order), one stable counting sort on (fine key, category) in LDS, and writes the
//                final 13-byte packed records (or SoA) as full coalesced lines.
//   big buckets: coarse buckets beyond the LDS capacity of a sort workgroup (degenerate ties) are ordered
//                by ldati_big_bucket_kernel inside the same call.
//   sweep      : the v1 kernel (one workgroup per segment, whole key histogram in LDS) serves
//                workspace == NULL only; both paths are bit-identical.
//
// ldati_dev.h holds LdatiParams, the device helpers and the __device__ globals; ldati_plan.h the host-side
// planning (sizes, workspace layouts, path choice); ldati_const.h the constants both read; this file the
// kernels and the entry points.  One translation unit: the globals must exist once.
//
// Arithmetic is bit-exact w.r.t. the CPU reference: every f32/f64 operation is a separate IEEE
// operation (-ffp-contract=off, correctly rounded '/' and sqrt), in the reference's order.
#include "common.h"
#include "ldati_dev.h"
#include "ldati_plan.h"

#include <atomic>
#include <mutex>
#include <type_traits>

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <cmath>
#include <cstdlib>

namespace v2ce {
namespace {

// ---------------------------------------------------------------------------------------------
// count: workgroup per (frame, tile); events per (tile, bin); max count per voxel
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCountThreads) void ldati_count_tiles_kernel(
    const float *__restrict__ vox, int HW, int tpp, int strategy, int bidir, unsigned *__restrict__ tc,
    unsigned long long *stats) {
    const int t = blockIdx.x, b = blockIdx.y, T = 2 * tpp;
    const int pidx = t < tpp ? 1 : 0;                 // negative tiles first (LDATI.py:289)
    const int x0 = (t < tpp ? t : t - tpp) * kTilePix;
    const float *plane0 = vox + (long long)(b * 2 + pidx) * 10 * HW;
    int cnt[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) cnt[i] = 0;
    int mx = 0;
    constexpr int PPT = kTilePix / kCountThreads;
    // four consecutive pixels per thread: one 16-byte load per plane, all ten in flight at once (any pixel order
    // is right: only sums are formed)
    float yq[PPT][10];
    {
        const int px = x0 + (int)threadIdx.x * PPT;
        if ((HW & 3) == 0 && px + PPT <= HW) {
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const float4 v = *reinterpret_cast<const float4 *>(plane0 + (long long)i * HW + px);
                yq[0][i] = v.x; yq[1][i] = v.y; yq[2][i] = v.z; yq[3][i] = v.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < PPT; ++q)
#pragma unroll
                for (int i = 0; i < 10; ++i) yq[q][i] = (px + q < HW) ? plane0[(long long)i * HW + px + q] : 0.0f;
        }
    }
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        int nn[9];
        float td[9];
        relocate_all(yq[q], bidir != 0, nn, td);                     // (an all-zero pixel past the image counts nothing)
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int ni = nn[i];
            cnt[i] += (strategy == V2CE_STRATEGY_NONE) ? (ni == 1) : (ni > 0 ? ni : 0);
            mx = ni > mx ? ni : mx;
        }
    }
    __shared__ int red[kCountThreads / 64][10];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const unsigned v = wave_incl_scan((unsigned)cnt[i], lane);       // (DPP: no LDS crossbar traffic)
        if (lane == 63) red[wid][i] = (int)v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int m = __shfl_xor(mx, o);
        mx = m > mx ? m : mx;
    }
    if (lane == 0) red[wid][9] = mx;
    __syncthreads();
    if (threadIdx.x < 9) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < kCountThreads / 64; ++w) s += (unsigned)red[w][threadIdx.x];
        tc[((long long)b * T + t) * 9 + threadIdx.x] = s;
    } else if (threadIdx.x == 9) {
        int m = 0;
#pragma unroll
        for (int w = 0; w < kCountThreads / 64; ++w) m = red[w][9] > m ? red[w][9] : m;
        // (a plain read first: after the first few tiles the maximum rarely grows, and 2 000 same-address atomics serialise)
        if (m > 0 && (unsigned long long)m > *reinterpret_cast<volatile unsigned long long *>(&stats[0])) atomicMax(&stats[0], (unsigned long long)m);
    }
}

// Tile counts -> exclusive tile offsets inside each segment, one wave per segment (the segment count
// lands in seg_offsets[seg]; the largest (tile, bin) and segment counts in stats[1], stats[2]).
__global__ __launch_bounds__(256) void ldati_tile_scan_kernel(const unsigned *__restrict__ tc, int B,
                                                              int T, unsigned *__restrict__ tile_off,
                                                              unsigned *__restrict__ tile_src, int Tp,
                                                              long long *seg_offsets,
                                                              unsigned long long *stats) {
    // one wave per FRAME, lane = tile, all nine bins of the tile in the lane: the nine counts of a tile are 36 contiguous bytes,
    // so the wave reads and writes whole blocks (a wave per (frame, bin) read and wrote every ninth word of the same cache
    // lines as its eight siblings: 16 us for the 576 segments of an e2e call, now 4)
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    unsigned run[9], mx = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) run[c] = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int tt = t0 + lane;
        const long long i0 = ((long long)b * T + tt) * 9;
        unsigned v[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) v[c] = tt < T ? tc[i0 + c] : 0u;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const unsigned incl = wave_incl_scan(v[c], lane);
            const unsigned ex = run[c] + incl - v[c];
            if (tt < T) {
                tile_off[i0 + c] = ex;
                tile_src[(long long)(b * 9 + c) * Tp + tt] = ex;      // the same, [segment][tile] for the bucket sort's setup
            }
            run[c] += (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
            mx = v[c] > mx ? v[c] : mx;
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned m = __shfl_xor(mx, o);
        mx = m > mx ? m : mx;
    }
    if (lane < 9) {
        unsigned r = run[0];
#pragma unroll
        for (int c = 1; c < 9; ++c) r = lane == c ? run[c] : r;
        seg_offsets[b * 9 + lane] = r;
        atomicMax(&stats[2], (unsigned long long)r);
    }
    if (lane == 0) atomicMax(&stats[1], (unsigned long long)mx);
}

// One workgroup: segment counts -> exclusive segment offsets (seg_offsets[n] = stats[3] = total).
__global__ __launch_bounds__(256) void ldati_seg_scan_kernel(int n, long long *seg_offsets, unsigned long long *stats) {
    __shared__ long long part[256];
    const int t = threadIdx.x;
    const int per = (n + 255) / 256;
    const int lo = t * per, hi = (lo + per < n) ? lo + per : n;
    long long s = 0;
    for (int i = lo; i < hi; ++i) s += seg_offsets[i];
    part[t] = s;
    __syncthreads();
    if (t < 64) {                                   // 256 partials: four per lane of one wave
        long long v[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = part[4 * t + j]; sum += v[j]; }
        long long incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long u = __shfl_up(incl, o);
            if (t >= o) incl += u;
        }
        long long run = incl - sum;
#pragma unroll
        for (int j = 0; j < 4; ++j) { part[4 * t + j] = run; run += v[j]; }
        if (t == 63) {
            seg_offsets[n] = incl;
            stats[3] = (unsigned long long)incl;
        }
    }
    __syncthreads();
    long long run = part[t];
    for (int i = lo; i < hi; ++i) {
        const long long v = seg_offsets[i];
        seg_offsets[i] = run;
        run += v;
    }
}

// ---------------------------------------------------------------------------------------------
// sweep kernel (v1): one workgroup (4 waves = the 4 tie-order categories) per (frame, bin) segment:
//   A. histogram cnt[cat][key]  B. exclusive scan in (key, category) order = stable ranks
//   C. replay the same events in pixel order; rank among the equal-key events of the wave batch
//      from a ballot match-any, running base from LDS; scatter straight to the final position.
// ---------------------------------------------------------------------------------------------
template <bool RANK>
__device__ __forceinline__ void handle_event(bool has, long long T, int px, int c, int cat,
                                             signed char pol, int lane, long long seg_lo,
                                             long long ts_add, unsigned *cnt,
                                             const LdatiParams &P) {
    const int key = key_of(T, P.kbase[c], P.NK);
    unsigned *slot = cnt + cat * P.NK + key;
    if (!RANK) {
        if (has) atomicAdd(slot, 1u);
        return;
    }
    const unsigned slot_pos = take_slots(has, (unsigned)key, P.nbits, slot);
    if (has) {
        const long long pos = seg_lo + (long long)slot_pos;
        const int yy = px / P.W;
        if (P.packed) {
            store_packed_bytes(P.packed + pos * 13, T + ts_add, (unsigned)(px - yy * P.W) & 0xFFFFu,
                               (unsigned)yy & 0xFFFFu, (unsigned)pol);
        } else {
            P.ts[pos] = T + ts_add;
            P.x[pos] = (short)(px - yy * P.W);
            P.y[pos] = (short)yy;
            P.p[pos] = pol;
        }
    }
}

template <bool RANK>
__device__ __forceinline__ void sweep_singles(int b, int c, int pidx, int cat, signed char pol,
                                              int lane, long long seg_lo, long long ts_add,
                                              unsigned *cnt, const LdatiParams &P) {
    const float *plane0 = P.vox + (long long)(b * 2 + pidx) * 10 * P.HW;
    float cur[10], nxt[10];
    load_bins(plane0, P.HW, lane, lane < P.HW, c, cur);   // singles only need bins 0..c
    for (int base = 0; base < P.HW; base += 64) {
        const int px = base + lane;
        const bool valid = px < P.HW;
        const int pxn = px + 64;
        load_bins(plane0, P.HW, pxn, pxn < P.HW, c, nxt);  // prefetch the next 64 pixels
        int n_l, n_c, n_r;
        float debt;
        relocate_bins(cur, c, c, n_l, n_c, n_r, debt);
        const bool has = valid && n_c == 1;
        const long long T = single_ts(debt, P.fps, P.offt[c]);
        handle_event<RANK>(has, T, px, c, cat, pol, lane, seg_lo, ts_add, cnt, P);
#pragma unroll
        for (int i = 0; i < 10; ++i) cur[i] = nxt[i];
    }
}

template <bool RANK>
__device__ __forceinline__ void sweep_multis(int b, int c, int pidx, int cat, signed char pol,
                                             int lane, long long seg_lo, long long ts_add,
                                             unsigned *cnt, int *s_start, float *s_k, float *s_bb,
                                             const LdatiParams &P) {
    const int last = c + 1 < 8 ? c + 1 : 8;
    const float *plane0 = P.vox + (long long)(b * 2 + pidx) * 10 * P.HW;
    const unsigned pc = (unsigned)(pidx * 9 + c);
    const unsigned frame = (unsigned)(P.frame_base + b);
    float cur[10], nxt[10];
    load_bins(plane0, P.HW, lane, lane < P.HW, last, cur);
    for (int base = 0; base < P.HW; base += 64) {
        const int px = base + lane;
        const bool valid = px < P.HW;
        const int pxn = px + 64;
        load_bins(plane0, P.HW, pxn, pxn < P.HW, last, nxt);
        int n_l, n_c, n_r;
        float debt;
        relocate_bins(cur, c, last, n_l, n_c, n_r, debt);
        const int m = (valid && n_c >= 2) ? n_c : 0;
        float k, bb;
        if (P.kbb) {
            const float2 kq = valid ? P.kbb[((long long)(b * 2 + pidx) * 9 + c) * P.HW + px] : make_float2(0.0f, 0.0f);
            k = kq.x; bb = kq.y;
        } else {
            slope_params(n_l, n_c, n_r, c, P, k, bb);
        }
        // exclusive wave scan of m -> first event index of each pixel inside this batch
        int incl = m;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        const int E = __shfl(incl, 63);
        if (E > 0) {
            s_start[lane] = incl - m;
            s_k[lane] = k;
            s_bb[lane] = bb;
            __builtin_amdgcn_wave_barrier();
            for (int e0 = 0; e0 < E; e0 += 64) {
                const int e = e0 + lane;
                const bool act = e < E;
                // last lane l with s_start[l] <= e  (pixels with m == 0 share the next start)
                int lo = 0, hi = 63;
#pragma unroll
                for (int it = 0; it < 6; ++it) {
                    const int mid = (lo + hi + 1) >> 1;
                    const bool le = s_start[mid] <= e;
                    lo = le ? mid : lo;
                    hi = le ? hi : mid - 1;
                }
                const int src = act ? lo : 0;
                const int j = e - s_start[src];
                const int spx = base + src;
                float u = 0.0f;
                if (act) {
                    if (P.rng_mode == V2CE_RNG_REPLAY) {
                        if (j < P.replay_max_n)
                            u = P.uniforms[(((long long)(b * 2 + pidx) * 9 + c) * P.HW + spx) *
                                               P.replay_max_n + j];
                    } else {
                        u = philox_uniform(P.seed, (unsigned)spx, (unsigned)j, pc, frame);
                    }
                }
                const long long T = multi_ts(s_k[src], s_bb[src], u, P.offt[c], P);
                handle_event<RANK>(act, T, spx, c, cat, pol, lane, seg_lo, ts_add, cnt, P);
            }
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int i = 0; i < 10; ++i) cur[i] = nxt[i];
    }
}

extern __shared__ __attribute__((aligned(16))) unsigned char ldati_smem[];

__global__ __launch_bounds__(256) void ldati_emit_kernel(LdatiParams P) {
    const int seg = blockIdx.x;          // b*9 + c
    const int b = seg / 9, c = seg - b * 9;
    const long long seg_lo = P.seg_offsets[seg];
    const long long seg_n = P.seg_offsets[seg + 1] - seg_lo;
    if (seg_n <= 0) return;              // uniform per workgroup
    if (P.seg_flag && !P.seg_flag[seg]) return;   // the two-level path handled this segment
    const long long ts_add = P.frame_ts_add ? P.frame_ts_add[b] : 0;

    unsigned *cnt = reinterpret_cast<unsigned *>(ldati_smem);            // [4][NK]
    unsigned *part = cnt + 4 * P.NK;                                       // [256]
    int *s_start = reinterpret_cast<int *>(part + 256);                    // [2][64]
    float *s_k = reinterpret_cast<float *>(s_start + 128);                 // [2][64]
    float *s_bb = s_k + 128;                                               // [2][64]

    const int tid = threadIdx.x, lane = tid & 63;
    const int cat = __builtin_amdgcn_readfirstlane(tid >> 6);   // 0 neg-single 1 neg-multi 2 pos-single 3 pos-multi
    const int pidx = cat < 2 ? 1 : 0;    // negative events live in P index 1 (LDATI.py:289)
    const signed char pol = cat < 2 ? 0 : 1;
    const bool multi = cat & 1;
    const bool skip = multi && P.strategy == V2CE_STRATEGY_NONE;   // wave-uniform
    int *my_start = s_start + (cat >> 1) * 64;
    float *my_k = s_k + (cat >> 1) * 64, *my_bb = s_bb + (cat >> 1) * 64;

    for (int i = tid; i < 4 * P.NK; i += 256) cnt[i] = 0;
    __syncthreads();

    // A. histogram
    if (skip) {
    } else if (multi)
        sweep_multis<false>(b, c, pidx, cat, pol, lane, seg_lo, ts_add, cnt, my_start, my_k, my_bb, P);
    else
        sweep_singles<false>(b, c, pidx, cat, pol, lane, seg_lo, ts_add, cnt, P);
    __syncthreads();

    // B. exclusive scan in (key-major, category-minor) order
    {
        const int kpt = (P.NK + 255) / 256;
        const int klo = tid * kpt, khi = (klo + kpt < P.NK) ? klo + kpt : P.NK;
        unsigned s = 0;
        for (int k = klo; k < khi; ++k)
            s += cnt[k] + cnt[P.NK + k] + cnt[2 * P.NK + k] + cnt[3 * P.NK + k];
        part[tid] = s;
        __syncthreads();
        // Hillis-Steele inclusive scan over 256 partials
        for (int o = 1; o < 256; o <<= 1) {
            const unsigned v = tid >= o ? part[tid - o] : 0u;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        unsigned run = part[tid] - s;
        for (int k = klo; k < khi; ++k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned v = cnt[q * P.NK + k];
                cnt[q * P.NK + k] = run;
                run += v;
            }
        }
    }
    __syncthreads();

    // C. rank + scatter
    if (skip) {
    } else if (multi)
        sweep_multis<true>(b, c, pidx, cat, pol, lane, seg_lo, ts_add, cnt, my_start, my_k, my_bb, P);
    else
        sweep_singles<true>(b, c, pidx, cat, pol, lane, seg_lo, ts_add, cnt, P);
}

// ---------------------------------------------------------------------------------------------
// tile pass: workgroup per (frame, tile), NT threads, PPT consecutive pixels per thread, bin by bin
// ---------------------------------------------------------------------------------------------
// LDS map (dynamic): S [capA] u32 | O [capA + 2048] u32 (aliased by the unit tables while the
// timestamps are computed) | PT [2048] {k, bb} | hist [NW/2][NB] u32 (two 16-bit chunk counters per word) | misc
extern __shared__ __attribute__((aligned(16))) unsigned char tile_smem[];

template <int NT, int PPT, bool BIDIR>
__global__ __launch_bounds__(NT) void ldati_tile_pass_kernel(LdatiParams P) {
    static_assert(NT * PPT == kTilePix, "tile geometry");
    const int t = blockIdx.x, b = blockIdx.y;
    if (P.sparse_cap) {                                 // the sparse tile kernel owns the lightly populated tiles
        const unsigned *tcr = P.tc + ((long long)b * P.T + t) * 9;
        unsigned ntot = 0;
#pragma unroll
        for (int c = 0; c < 9; ++c) ntot += tcr[c];
        if (ntot <= (unsigned)P.sparse_cap) return;
    }
    const int pidx = t < P.tpp ? 1 : 0;
    const int x0 = (t < P.tpp ? t : t - P.tpp) * kTilePix;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    constexpr int NW = NT / 64;
    const bool atomic_order = !P.ballot_ranks && __builtin_amdgcn_readfirstlane(g_lds_order_ok) != 0;
    // the checked fast form of the k == 0 time: Philox uniforms only, and only if this FPS passed the exhaustive check
    const bool slot_ok = P.fast_slot >= 0 &&
                         __builtin_amdgcn_readfirstlane((int)g_fastdiv[P.fast_slot >= 0 ? P.fast_slot : 0].fps_bits) == (int)__float_as_uint(P.FPS);
    const bool fast_k0 = slot_ok && P.rng_mode == V2CE_RNG_PHILOX && __builtin_amdgcn_readfirstlane(g_fastdiv[P.fast_slot].ok) != 0;
    const float2 *stab = (slot_ok && __builtin_amdgcn_readfirstlane(g_fastdiv[P.fast_slot].tab_ready) != 0) ? g_slope_tab[P.fast_slot] : nullptr;

    unsigned *S = reinterpret_cast<unsigned *>(tile_smem);
    unsigned *O = S + P.capA;
    float2 *PT = reinterpret_cast<float2 *>(O + P.capA + 2048);
    unsigned *hist = reinterpret_cast<unsigned *>(PT + kTilePix);
    unsigned *part = hist + (NW / 2) * P.NB;           // [NW] x 2 (hist: two 16-bit counters per word)
    // unit tables alias O: singles {debt bits, local} then multi units {info, event offset}
    uint2 *SL = reinterpret_cast<uint2 *>(O);

    const float *plane0 = P.vox + (long long)(b * 2 + pidx) * 10 * P.HW;
    const unsigned frame = (unsigned)(P.frame_base + b);
    const int lpx0 = tid * PPT;                        // first local pixel of this thread
    const float eps = 1e-6f;

    // relocation state per pixel: counts of bins c-1, c, c+1; tendency ("debt") of bin c.  Forward
    // relocation rolls along the bins (the voxels of bin c+2 are fetched while bin c is processed);
    // the bidirectional variant (LDATI.py:107-122) needs all ten voxels first and keeps all nine bins.
    int nprev[PPT], ncur[PPT], nnext[PPT];
    float dcur[PPT], dnext[PPT];
    bool valid[PPT];
    int nA[BIDIR ? PPT : 1][9];
    float tA[BIDIR ? PPT : 1][9];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int px = x0 + lpx0 + q;
        valid[q] = px < P.HW;
        if (BIDIR) {
            float yv[10];
#pragma unroll
            for (int i = 0; i < 10; ++i) yv[i] = valid[q] ? plane0[(long long)i * P.HW + px] : 0.0f;
            relocate_all(yv, true, nA[q], tA[q]);
            nprev[q] = ncur[q] = nnext[q] = 0;
            dcur[q] = dnext[q] = 0.0f;
        } else {
            const float y0 = valid[q] ? plane0[px] : 0.0f;
            const float y1 = valid[q] ? plane0[(long long)P.HW + px] : 0.0f;
            float r = y0 - 0.0f;
            float cc = ceilf(r - eps);
            dcur[q] = cc - r;
            ncur[q] = (int)cc;
            r = y1 - dcur[q];
            cc = ceilf(r - eps);
            dnext[q] = cc - r;
            nnext[q] = (int)cc;
            nprev[q] = 0;
        }
    }

    STAMP_DECL;
    for (int c = 0; c < 9; ++c) {
        STAMP(0);
        // prefetch the voxels of bin c+2 (and bin 9 with it when c+2 == 8)
        float ynn[PPT], y9[PPT];
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int px = x0 + lpx0 + q;
            ynn[q] = (!BIDIR && c + 2 <= 8 && valid[q]) ? plane0[(long long)(c + 2) * P.HW + px] : 0.0f;
            y9[q] = (!BIDIR && c + 2 == 8 && valid[q]) ? plane0[(long long)9 * P.HW + px] : 0.0f;
            if (BIDIR) {
                nprev[q] = c > 0 ? pick9(nA[q], c - 1) : 0;
                ncur[q] = pick9(nA[q], c);
                nnext[q] = c < 8 ? pick9(nA[q], c + 1) : 0;
                dcur[q] = pick9(tA[q], c);
            }
        }
        // ---- P1: classify ------------------------------------------------------------------
        // Multi-event voxels come in two classes: slope k == 0 (time = (u / fps) / 9: two constant divisions) and k != 0
        // (a square root and a division).  Their 4-draw units go to two separate regions of the unit table (k == 0
        // units first), so that a wave of the timestamp phase executes ONE of the two code paths, not both.
        unsigned a_tot = 0, e_tot = 0;                  // per thread: singles | k==0 units << 12;  multi events | k!=0 units << 14
        unsigned a_q[PPT], e_q[PPT];
        bool kz_q[PPT];
        float kk_q[PPT], bb_q[PPT];
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int n = valid[q] ? ncur[q] : 0;
            const bool single = n == 1;
            const bool multi = n >= 2 && P.strategy != V2CE_STRATEGY_NONE;
            kk_q[q] = bb_q[q] = 0.0f;
            if (multi) {
                if (P.kbb) {                         // pooled counts (LDATI.py:177-190): from the pre-pass
                    const float2 kq = P.kbb[((long long)(b * 2 + pidx) * 9 + c) * P.HW + (x0 + lpx0 + q)];
                    kk_q[q] = kq.x; bb_q[q] = kq.y;
                } else {
                    slope_params(nprev[q], n, nnext[q], c, P, kk_q[q], bb_q[q], stab);
                }
            }
            kz_q[q] = kk_q[q] == 0.0f;
            const unsigned units = multi ? (unsigned)(n + 3) >> 2 : 0u;
            a_q[q] = a_tot;
            e_q[q] = e_tot;
            a_tot += (single ? 1u : 0u) + (kz_q[q] ? units << 12 : 0u);
            e_tot += (multi ? (unsigned)n : 0u) + (kz_q[q] ? 0u : units << 14);
        }
        // ---- P2: workgroup scans in pixel order (thread-major, pixel-minor).  Their first barrier
        // also separates the previous bin's reads of O (P7) from this bin's unit tables.
        unsigned a_base, e_base, A_all, E_all;
        block_excl_scan2<NW>(a_tot, e_tot, part, a_base, e_base, A_all, E_all);
        STAMP(1);
        const unsigned Ns = A_all & 0xFFFu, U0 = A_all >> 12, Nm = E_all & 0x3FFFu, Um = U0 + (E_all >> 14);
        const unsigned N = Ns + Nm;
        uint2 *MU = SL + Ns;
        // the records are ranked in NC contiguous chunks of L records, one wave each (a sparse tile
        // needs few: the histogram work below is proportional to NC)
        const unsigned NC = N > 256u * NW ? (unsigned)NW : (N + 255u) / 256u;
        const unsigned L = NC ? ((N + 64u * NC - 1u) / (64u * NC)) * 64u : 64u;
        for (unsigned i = tid; i < ((NC + 1u) >> 1) * P.NB; i += NT) hist[i] = 0;   // (chunk pair, bucket): two 16-bit counters per word
        // ---- P3: unit tables ----------------------------------------------------------------
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int n = valid[q] ? ncur[q] : 0;
            const unsigned local = (unsigned)(lpx0 + q);
            const unsigned ab = a_base + a_q[q], eb = e_base + e_q[q];
            if (n == 1) {
                SL[ab & 0xFFFu] = make_uint2(__float_as_uint(dcur[q]), local);
            } else if (n >= 2 && P.strategy != V2CE_STRATEGY_NONE) {
                PT[local] = make_float2(kk_q[q], bb_q[q]);
                const unsigned u0 = kz_q[q] ? ab >> 12 : U0 + (eb >> 14), ev0 = eb & 0x3FFFu;
                const unsigned units = (unsigned)(n + 3) >> 2;
                for (unsigned jb = 0; jb < units; ++jb) {
                    const unsigned left = (unsigned)n - 4u * jb;
                    MU[u0 + jb] = make_uint2(local | (jb << kLocalBits) | ((left < 4u ? left : 4u) << 28),
                                             ev0 + 4u * jb);
                }
            }
        }
        __syncthreads();
        STAMP(2);
        // ---- P4: timestamps, once, every lane busy; each record also counts in the histogram of
        // the wave that will rank it (contiguous chunks of S, L records per wave) -----------------
        const float invL = 1.0f / (float)L;
        for (unsigned q = tid; q < Ns; q += NT) {
            const uint2 e = SL[q];
            const long long Tq = single_ts(__uint_as_float(e.x), P.fps, P.offt[c]);
            const unsigned key = (unsigned)(BIDIR ? key_of_reporting(true, Tq, P.kbase[c], P.NK, P.status) : key_of(Tq, P.kbase[c], P.NK));
            S[q] = (key << 12) | e.y;
            const unsigned w = (unsigned)(((float)q + 0.5f) * invL);
            if (!P.keys) atomicAdd(&hist[__umul24(w >> 1, (unsigned)P.NB) + (key >> P.shift)], 1u << ((w & 1u) * 16u));
        }
        STAMP(3);
        // The common case -- Philox draws, 32-bit timestamps, the 'slope' strategy, the bucket machinery -- has its own copy of
        // the loop without the per-event uniform tests (the pass is bound by instruction issue); COMMON 1 = with the checked
        // fast k == 0 time, 2 = with the divisions.  The slope class is tested once per unit (waves are class-homogeneous).
        auto multis = [&](auto common_c) {
            constexpr int COMMON = decltype(common_c)::value;
            const float offt_c = P.offt[c];
            const int kbase_c = (int)P.kbase[c];
            for (unsigned q = tid; q < Um; q += NT) {
                const uint2 e = MU[q];
                const unsigned local = e.x & (kTilePix - 1), jb = (e.x >> kLocalBits) & 0x1FFFFu, cnt = e.x >> 28;
                const float2 kb = PT[local];
                const unsigned px = (unsigned)x0 + local;
                float u[4];
                if (!COMMON && P.rng_mode == V2CE_RNG_REPLAY) {
                    const long long ub = (((long long)(b * 2 + pidx) * 9 + c) * P.HW + px) * P.replay_max_n;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int j = (int)(4u * jb) + s;
                        u[s] = ((unsigned)s < cnt && j < P.replay_max_n) ? P.uniforms[ub + j] : 0.0f;
                    }
                } else {
                    unsigned o[4];
                    philox4(P.seed, px, jb, (unsigned)(pidx * 9 + c), frame, o);
#pragma unroll
                    for (int s = 0; s < 4; ++s) u[s] = u24(o[s]);
                }
                unsigned key[4];
                if (COMMON) {
                    float t[4];
                    if (kb.x == 0.0f) {
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            t[s] = COMMON == 1 ? k0_time_fast(u[s], P.FPS, P.RFPS, P.R9) : (u[s] / P.FPS) / 9.0f;
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const float sq = kb.y * kb.y + (2.0f * kb.x) * u[s];
                            t[s] = (-kb.y + __builtin_sqrtf(sq)) / kb.x;
                        }
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {                   // multi_key's tail: (t + offt) * 1e6 -> key, clamped
                        float tt = t[s] + offt_c;
                        tt = tt * 1e6f;
                        int k = (int)tt - kbase_c;
                        if (BIDIR && (unsigned)s < cnt && (k < 0 || k >= P.NK)) atomicOr(reinterpret_cast<unsigned *>(P.status), kStatusKeyWindow);
                        k = k < 0 ? 0 : k;
                        key[s] = (unsigned)(k >= P.NK ? P.NK - 1 : k);
                    }
                } else if (BIDIR) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)               // (multi_ts: the 64-bit form of multi_key's time, the same value while P.ts32)
                        key[s] = (unsigned)key_of_reporting((unsigned)s < cnt, multi_ts(kb.x, kb.y, u[s], P.offt[c], P), P.kbase[c], P.NK, P.status);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        key[s] = P.ts32 ? multi_key(kb.x, kb.y, u[s], P.offt[c], (int)P.kbase[c], P, fast_k0)
                                        : (unsigned)key_of(multi_ts(kb.x, kb.y, u[s], P.offt[c], P), P.kbase[c], P.NK);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if ((unsigned)s < cnt) {
                        const unsigned pos = Ns + e.y + s;
                        S[pos] = (key[s] << 12) | (1u << kLocalBits) | local;
                        const unsigned w = (unsigned)(((float)pos + 0.5f) * invL);
                        if (COMMON || !P.keys) atomicAdd(&hist[__umul24(w >> 1, (unsigned)P.NB) + (key[s] >> P.shift)], 1u << ((w & 1u) * 16u));
                    }
                }
            }
        };
        if (P.rng_mode == V2CE_RNG_PHILOX && P.ts32 && !P.keys && P.strategy == V2CE_STRATEGY_SLOPE) {
            if (fast_k0) multis(std::integral_constant<int, 1>{});
            else multis(std::integral_constant<int, 2>{});
        } else {
            multis(std::integral_constant<int, 0>{});
        }
        STAMP(4);
        __syncthreads();
        STAMP(5);
        if (P.keys) {
            // generic path (key range beyond the bucket machinery: 'random'): one 64-bit key per event,
            // (segment | timestamp - bin start | category | pixel), sorted by a library radix sort
            unsigned long long *dst = P.keys + P.seg_offsets[b * 9 + c] + P.tile_off[((long long)b * P.T + t) * 9 + c];
            const unsigned long long seg_bits = (unsigned long long)(b * 9 + c) << 44;
            for (unsigned i = tid; i < N; i += NT) {
                const unsigned r = S[i];
                const unsigned cat = (pidx ? 0u : 2u) + ((r >> kLocalBits) & 1u);
                dst[i] = seg_bits | ((unsigned long long)(r >> 12) << 24) | ((unsigned long long)cat << 22) |
                         (unsigned long long)((unsigned)x0 + (r & (kTilePix - 1)));
            }
        } else {
        // ---- P5: bucket-major, wave-minor exclusive scan; the tile's bucket counts and run offsets
        {
            // (counts and offsets are below 2^16: a (tile, bin) holds at most kCapTile = 15360 records)
            constexpr int NWP = NW / 2;                          // chunk pairs
            const unsigned ncp = (NC + 1u) >> 1;
            unsigned v[NWP];
            unsigned run = 0;
            if (tid < P.NB) {
#pragma unroll
                for (int w = 0; w < NWP; ++w) v[w] = (unsigned)w < ncp ? hist[w * P.NB + tid] : 0u;   // independent reads
#pragma unroll
                for (int w = 0; w < NWP; ++w) {
                    const unsigned lo = v[w] & 0xFFFFu, hi = v[w] >> 16;
                    v[w] = run | ((run + lo) << 16);                // exclusive starts of the even and the odd chunk
                    run += lo + hi;
                }
            }
            unsigned tot;
            const unsigned boff = block_excl_scan<NW>(run, part, &tot);
            if (tid < P.NB) {
                const unsigned b2 = boff | (boff << 16);
#pragma unroll
                for (int w = 0; w < NWP; ++w)
                    if ((unsigned)w < ncp) hist[w * P.NB + tid] = v[w] + b2;
            }
            // the tile's row of the run table: one contiguous, coalesced store
            unsigned short *row = P.roff + ((long long)(b * 9 + c) * P.T + t) * (P.NB + 1);
            if (tid < P.NB) row[tid] = (unsigned short)boff;
            if (tid == 0) row[P.NB] = (unsigned short)N;
        }
        __syncthreads();
        STAMP(6);
        // ---- P6: stable ranks: ballot match-any inside a 64-record batch, running base in LDS ----
        const unsigned lo = wid * L, hi = (lo + L < N) ? lo + L : N;
        if (atomic_order) {                              // the rank IS what the LDS atomic returns (g_lds_order_ok)
            unsigned *myhist = hist + (wid >> 1) * P.NB;
            const unsigned sh = 12 + P.shift, hs = (wid & 1) * 16;
            for (unsigned i0 = lo; i0 < hi; i0 += 64) {
                const unsigned i = i0 + lane;
                if (i < hi) {
                    const unsigned rec = S[i];
                    O[(atomicAdd(&myhist[rec >> sh], 1u << hs) >> hs) & 0xFFFFu] = rec;
                }
            }
        } else {
            for (unsigned i0 = lo; i0 < hi; i0 += 64) {
                const unsigned i = i0 + lane;
                const bool has = i < hi;
                const unsigned rec = has ? S[i] : 0u;
                const unsigned bucket = rec >> (12 + P.shift);
                const unsigned pos = take_slots_packed(has, bucket, P.nb1, &hist[(wid >> 1) * P.NB + bucket], (wid & 1) * 16);
                if (has) O[pos] = rec;
            }
        }
        STAMP(7);
        __syncthreads();
        STAMP(8);
        // ---- P7: the tile's records of this bin leave as one contiguous run ---------------------
        {
            unsigned *dst = P.temp + P.seg_offsets[b * 9 + c] + P.tile_off[((long long)b * P.T + t) * 9 + c];
            for (unsigned i = tid; i < N; i += NT) dst[i] = O[i];
        }
        STAMP(9);
        }
        // ---- advance the relocation recurrence to bin c+2 ---------------------------------------
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            if (BIDIR) continue;
            nprev[q] = ncur[q];
            ncur[q] = nnext[q];
            dcur[q] = dnext[q];
            if (c + 2 <= 8) {
                const float r = ynn[q] - dnext[q];
                const float cc = ceilf(r - eps);
                dnext[q] = cc - r;
                int ni = (int)cc;
                if (c + 2 == 8) ni += (int)(y9[q] - dnext[q]);   // LDATI.py:106
                nnext[q] = ni;
            }
        }
        // no barrier here: the next bin touches O / hist / S only behind the barriers of its scans
    }
    STAMP(0);
    STAMP_FLUSH(0, 10);
}

// ---------------------------------------------------------------------------------------------
// dense tile pass, round 4: the common call (forward relocation, 'slope' / 'none', no pooling, 32-bit times).
//
// What the SQ counters said about ldati_tile_pass_kernel on the stress chunk (profiles/r04_a_ldati_sq_counters.txt): its
// waves are PARKED half of their cycles (six workgroup barriers and two workgroup scans per bin, one 1024-thread
// workgroup per CU with nobody to run in the gaps), 182 VALU lane-slots per event at 78 % active lanes.  This kernel
// keeps the algorithm (per bin: every timestamp once, stable counting sort by coarse bucket, one coalesced run) and
// changes what that costs:
//   * a wave OWNS 64 * PPT consecutive pixels: classification, the unit compaction (so that every lane of the
//     timestamp code is busy) and the record positions come from 64-lane DPP scans, the unit tables are private to the
//     wave, and the wave's own row of the histogram counts the records it will later rank -- no workgroup scan, no
//     chunk arithmetic per record; the waves meet at four barriers per bin (wave totals, histogram complete, bucket
//     offsets ready, run complete);
//   * the slope parameters {k, b} of a multi-event voxel travel as an 11-bit index into g_slope_tab inside the unit
//     entry (a voxel outside the table is generated by its owner lane in place), so no per-pixel table occupies LDS:
//     records in, records out, NW histogram rows -- two 512-thread workgroups fit a CU and cover each other's barriers;
//   * Philox rounds on v_bitop3_b32 (three-input xor), and for Philox draws the square root and the division of
//     LDATI.py:195 as the compiler's own correctly rounded sequences minus their range scaling, with the refined
//     reciprocal of the voxel's slope shared by its four draws (sqrt_rn_nr / div_rn_nr below: identical results inside
//     the ranges the slope table spans; tests/test_gpu_ldati.py::test_exact_math_helpers checks them exhaustively).
// Everything else (bidirectional, pooled slope, 'random', 64-bit times, a table that is not ready) stays on
// ldati_tile_pass_kernel; both produce the same bytes (test_dense_tile_kernel_equals_per_bin_kernel).
// LDS map (dynamic): S [capA] u32 | O [capA + 2] u32 (the workgroup's work lists alias it) | hist [NW][NB] | misc
// ---------------------------------------------------------------------------------------------
// correctly rounded sqrt for a == 0, a >= 2^-96, negative or NaN a: v_sqrt_f32 (1 ulp) and the two residual tests of the
// compiler's expansion (which additionally rescales a < 2^-96: never the case for b^2 + 2 k u of a table entry)
__device__ __forceinline__ float sqrt_rn_nr(float a) {
    const float r = __builtin_amdgcn_sqrtf(a);
    const float rdn = __uint_as_float(__float_as_uint(r) - 1u), rup = __uint_as_float(__float_as_uint(r) + 1u);
    const float edn = __builtin_fmaf(-rdn, r, a), eup = __builtin_fmaf(-rup, r, a);
    float o = (0.0f >= edn) ? rdn : r;
    o = (0.0f < eup) ? rup : o;
    return o;
}
// the refined reciprocal of the compiler's f32 division (v_rcp_f32 + one Newton step)
__device__ __forceinline__ float rcp_refined(float k) {
    const float r0 = __builtin_amdgcn_rcpf(k);
    const float e = __builtin_fmaf(-k, r0, 1.0f);
    return __builtin_fmaf(e, r0, r0);
}
// x / k, correctly rounded, by the compiler's sequence without v_div_scale / v_div_fixup: valid while neither rescales,
// i.e. k and 1/k normal, x zero, NaN or >= 2^-103 in magnitude, x / k normal (LDATI: |k| in [1e2, 1e8], x = sqrt(.) - b)
__device__ __forceinline__ float div_rn_nr(float x, float k, float r1) {
    float q = x * r1;
    float rem = __builtin_fmaf(-k, q, x);
    q = __builtin_fmaf(rem, r1, q);
    rem = __builtin_fmaf(-k, q, x);
    return __builtin_fmaf(rem, r1, q);
}
// Philox4x32-10 as philox4(), the two three-input xors of a round as one v_bitop3_b32 each.  `seed` must be wave-uniform (it
// is the call's seed everywhere): the key schedule lives in scalar registers
__device__ __forceinline__ void philox4_b3(unsigned long long seed, unsigned pixel, unsigned jb, unsigned pc, unsigned frame,
                                           unsigned (&out)[4]) {
    unsigned c0 = pixel, c1 = jb, c2 = pc, c3 = frame;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    // (the key schedule is recomputed here, two scalar adds per round: hoisted out of the caller's loops its twenty values
    // live in SGPRs the kernel does not have -- they were spilled to VGPR lanes and read back with v_readlane every round)
    asm volatile("" : "+s"(k0), "+s"(k1));
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = __builtin_amdgcn_bitop3_b32((unsigned)(p1 >> 32), c1, k0, 0x96);
        const unsigned n2 = __builtin_amdgcn_bitop3_b32((unsigned)(p0 >> 32), c3, k1, 0x96);
        c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// slope-table index of a multi-event voxel, or -1 when it lies outside the table (slope_params' own test)
__device__ __forceinline__ int slope_index(int n_l, int n_c, int n_r, int c) {
    const int d = (c == 0 || c == 8) ? 0 : n_r - n_l;
    if (d >= -kSlopeM && d <= kSlopeM && n_c >= 0 && n_c <= kSlopeM && n_l >= 0 && n_r >= 0 && n_l < (1 << 23) && n_r < (1 << 23))
        return (d + kSlopeM) * (kSlopeM + 1) + n_c;
    return -1;
}

// FAST: every run-time switch of the common call is known to be on (Philox draws, the checked fast divisions, the slope table,
// LDS-atomic ranks, 16-byte aligned planes, 'slope'): the switches cost SGPRs the kernel does not have (they were spilled to VGPR
// lanes and read back with v_readlane), and their untaken sides cost code
template <int NW, bool FAST>
__device__ __forceinline__ void dense_tile_body(const LdatiParams &P) {
    constexpr int NT = 64 * NW, PPT = kTilePix / NT, WPX = 64 * PPT;
    static_assert(PPT == 4 || PPT == 2, "a lane owns 2 or 4 consecutive pixels");
    const int t = blockIdx.x, b = blockIdx.y;
    if (P.sparse_cap) {                                 // the sparse tile kernel owns the lightly populated tiles
        const unsigned *tcr = P.tc + ((long long)b * P.T + t) * 9;
        unsigned ntot = 0;
#pragma unroll
        for (int c = 0; c < 9; ++c) ntot += tcr[c];
        if (ntot <= (unsigned)P.sparse_cap) return;
    }
    const int pidx = t < P.tpp ? 1 : 0;
    const int x0 = (t < P.tpp ? t : t - P.tpp) * kTilePix;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool atomic_order = FAST || (!P.ballot_ranks && __builtin_amdgcn_readfirstlane(g_lds_order_ok) != 0);
    const bool slot_ok = FAST || (P.fast_slot >= 0 &&
                         __builtin_amdgcn_readfirstlane((int)g_fastdiv[P.fast_slot >= 0 ? P.fast_slot : 0].fps_bits) == (int)__float_as_uint(P.FPS));
    const bool philox = FAST || P.rng_mode == V2CE_RNG_PHILOX;
    const bool fast_k0 = FAST || (slot_ok && philox && __builtin_amdgcn_readfirstlane(g_fastdiv[P.fast_slot].ok) != 0);
    // (a table that another stream is still filling: every multi-event voxel takes the owner-lane path once)
    const bool tab_ok = FAST || (slot_ok && __builtin_amdgcn_readfirstlane(g_fastdiv[P.fast_slot].tab_ready) != 0);
    const bool fast_s = FAST || (slot_ok && P.ts32 && __builtin_amdgcn_readfirstlane(g_fastdiv[P.fast_slot].ok64) != 0);   // single_key's fast form
    const float2 *stab = g_slope_tab[P.fast_slot >= 0 ? P.fast_slot : 0];

    unsigned *S = reinterpret_cast<unsigned *>(tile_smem);
    unsigned *O = S + P.capA;
    unsigned *hist = O + P.capA + 8;                    // [NW][NB]: row r counts the records at positions [r L, (r + 1) L)
    unsigned *part = hist + NW * P.NB;                  // [3][NW] wave totals: events | singles << 16, k == 0 units | k != 0 units << 16, slot mode: events unpacked
    unsigned *spart = part + 3 * NW;                    // [NW + 1] scan partials
    unsigned *bctr = spart + NW + 1;                    // the next batch of the timestamp phase
    unsigned *dsto = bctr + 2;                          // [9][2]: where the tile's run of bin c starts in records[] (loaded once: a
                                                        // global load per bin would stall all sixteen waves for its whole latency)
    unsigned *nbin = dsto + 18;                         // [9] slot mode: the bins' record counts
    unsigned *myhist = hist + wid * P.NB;

    const float *plane0 = P.vox + (long long)(b * 2 + pidx) * 10 * P.HW;
    const unsigned frame = (unsigned)(P.frame_base + b);
    const int lpx0 = wid * WPX + lane * PPT;           // the lane's PPT consecutive local pixels: lpx0 + q
    const int gpx0 = x0 + lpx0;
    const bool vec = FAST || (P.HW & 3) == 0;          // every plane 16-byte aligned: one load per plane and lane
    const float eps = 1e-6f;

    // one plane's voxels of the lane's pixels (zero past the image)
    auto load_plane = [&](int plane, float (&y)[PPT]) {
        const float *src = plane0 + (long long)plane * P.HW + gpx0;
        if (vec) {
            if (PPT == 4) {
                const float4 v = gpx0 < P.HW ? *reinterpret_cast<const float4 *>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
                y[0] = v.x; y[1] = v.y; y[PPT - 2] = v.z; y[PPT - 1] = v.w;
            } else {
                const float2 v = gpx0 < P.HW ? *reinterpret_cast<const float2 *>(src) : make_float2(0.f, 0.f);
                y[0] = v.x; y[1] = v.y;
            }
        } else {
#pragma unroll
            for (int q = 0; q < PPT; ++q) y[q] = gpx0 + q < P.HW ? src[q] : 0.0f;
        }
    };

    int nprev[PPT], ncur[PPT], nnext[PPT];
    float dcur[PPT], dnext[PPT];
    {
        float y0[PPT], y1[PPT];
        load_plane(0, y0);
        load_plane(1, y1);
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            float r = y0[q] - 0.0f;
            float cc = ceilf(r - eps);
            dcur[q] = cc - r;
            ncur[q] = (int)cc;
            r = y1[q] - dcur[q];
            cc = ceilf(r - eps);
            dnext[q] = cc - r;
            nnext[q] = (int)cc;
            nprev[q] = 0;
        }
    }
    for (int i = lane; i < P.NB; i += 64) myhist[i] = 0;
    if (tid == 0) *bctr = 0;
    if (tid < 9) {
        // slot mode (the kernel is the count pass too: no offsets exist yet): the (tile, bin) run goes to its own slot
        const long long d = P.slot_cap ? (((long long)b * P.T + t) * 9 + tid) * (long long)P.slot_cap
                                       : P.seg_offsets[b * 9 + tid] + (long long)P.tile_off[((long long)b * P.T + t) * 9 + tid];
        dsto[2 * tid] = (unsigned)d;
        dsto[2 * tid + 1] = (unsigned)((unsigned long long)d >> 32);
        if (P.slot_cap) P.tile_abs_w[(long long)(b * 9 + tid) * P.Tp + t] = (unsigned)d;
    }
    int vmax_l = 0;                                     // slot mode: the lane's largest voxel count (the bins' counts wait in nbin)
    __syncthreads();

    STAMP_DECL;
    for (int c = 0; c < 9; ++c) {
        STAMP(0);
        float ynn[PPT], y9[PPT];
#pragma unroll
        for (int q = 0; q < PPT; ++q) ynn[q] = y9[q] = 0.0f;
        if (c + 2 <= 8) load_plane(c + 2, ynn);
        if (c + 2 == 8) load_plane(9, y9);
        // ---- D1: classify; positions in pixel order (lane-major, slot-minor): a running sum per lane, ONE wave scan --
        // cls: 0 nothing, 1 single, 2 multi with k == 0, 3 multi with k != 0 (both from the table), 4 multi outside the table;
        // the slope-table index rides in bits 3..13
        unsigned cls[PPT], aex[PPT], uex[PPT];
        unsigned At = 0, Ut = 0;
        // slot mode: the lane's events once more, UNPACKED.  The packed totals wrap at 2^16; the two-pass path bounds a (tile, bin)
        // by capA before this kernel runs, but as the count pass it must count ANY grid right (an unphysical one behind a dense call
        // that armed the dense hint: a wrapped total would pass the `N > capA` test below and index S past the slot)
        unsigned Ae = 0;
        const bool multi_on = FAST || P.strategy != V2CE_STRATEGY_NONE, edge = c == 0 || c == 8;
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int n = ncur[q];                                          // (a pixel past the image holds zeros: no event)
            const bool multi = n >= 2 && multi_on;
            // slope-table entry (slope_index's test in three unsigned compares): |difference| <= 31, count <= 31, neighbours in [0, 2^23)
            const int dd = edge ? 0 : nnext[q] - nprev[q];
            const bool intab = tab_ok && (unsigned)(dd + kSlopeM) <= 2u * kSlopeM && (unsigned)n <= (unsigned)kSlopeM &&
                               (unsigned)(nprev[q] | nnext[q]) < (1u << 23);
            const unsigned si = (unsigned)((dd + kSlopeM) * (kSlopeM + 1) + n);
            const unsigned cl = n == 1 ? 1u : !multi ? 0u : !intab ? 4u : dd == 0 ? 2u : 3u;      // table entries: k == 0 exactly when the difference is
            cls[q] = cl | ((si & 0x7FFu) << 3);
            const unsigned units = (unsigned)(n + 3) >> 2;
            aex[q] = At;
            uex[q] = Ut;
            At += (cl ? (unsigned)n : 0u) + (cl == 1u ? 0x10000u : 0u);
            Ut += cl == 2u ? units : cl == 3u ? units << 16 : 0u;
            Ae += cl ? ((unsigned)n < (1u << 20) ? (unsigned)n : 1u << 20) : 0u;     // (saturating per voxel: the sum of a tile stays below 2^32)
        }
        const unsigned iA = wave_incl_scan(At, lane), iU = wave_incl_scan(Ut, lane);
        const unsigned baseA = iA - At, baseU = iU - Ut;
        const unsigned runA = (unsigned)__builtin_amdgcn_readlane((int)iA, 63), runU = (unsigned)__builtin_amdgcn_readlane((int)iU, 63);
        if (lane == 0) { part[wid] = runA; part[NW + wid] = runU; }      // (events | singles << 16), (k == 0 units | k != 0 units << 16)
        if (P.slot_cap) {                                                   // uniform
            const unsigned runE = (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan(Ae, lane), 63);
            if (lane == 0) part[2 * NW + wid] = runE;
        }
        __syncthreads();                                 // A: wave totals; O (the previous bin's run) is free again
        STAMP(1);
        // Work lists of the WORKGROUP in O (2 (U1 + U0) + Ns <= N words): k != 0 units | k == 0 units | singles, each in
        // pixel order; the timestamp phase below hands them out in batches of 64 to whichever wave is free, so a lane is
        // idle only in the last batch of a class (per-wave lists left 38 % of the VALU lanes idle: r04_j counters)
        unsigned sbase, N, sS, sU0, sU1, Ns, U0, U1;
        {
            // two packed scans (every total is below 2^16: a (tile, bin) holds at most kCapTile records)
            const unsigned v0 = lane < NW ? part[lane] : 0u, v1 = lane < NW ? part[NW + lane] : 0u;
            const unsigned p0 = wave_incl_scan(v0, lane), p1 = wave_incl_scan(v1, lane);
            const unsigned tA = (unsigned)__builtin_amdgcn_readlane((int)p0, NW - 1), tU = (unsigned)__builtin_amdgcn_readlane((int)p1, NW - 1);
            const unsigned bA = wid ? (unsigned)__builtin_amdgcn_readlane((int)p0, wid - 1) : 0u;
            const unsigned bU = wid ? (unsigned)__builtin_amdgcn_readlane((int)p1, wid - 1) : 0u;
            N = tA & 0xFFFFu; Ns = tA >> 16; U0 = tU & 0xFFFFu; U1 = tU >> 16;
            sbase = bA & 0xFFFFu; sS = bA >> 16; sU0 = bU & 0xFFFFu; sU1 = bU >> 16;
        }
        if (P.slot_cap) {
            // the count pass's outputs; a run beyond the slot (and the LDS) is only counted -- the host sees the largest
            // (tile, bin) count in the statistics and repeats the call on the two-pass path.  The count is the UNPACKED sum:
            // the packed N above is only meaningful once this one says the run fits (capA < 2^16)
            const unsigned N32 = (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan(lane < NW ? part[2 * NW + lane] : 0u, lane), NW - 1);
            if (tid == 0) nbin[c] = N32;                 // (written out at the end: no pointer or sum lives across the bins)
#pragma unroll
            for (int q = 0; q < PPT; ++q) vmax_l = ncur[q] > vmax_l ? ncur[q] : vmax_l;
            if (N32 > (unsigned)P.capA) {                // uniform
#pragma unroll
                for (int q = 0; q < PPT; ++q) {
                    nprev[q] = ncur[q];
                    ncur[q] = nnext[q];
                    dcur[q] = dnext[q];
                    if (c + 2 <= 8) {
                        const float r = ynn[q] - dnext[q];
                        const float cc = ceilf(r - eps);
                        dnext[q] = cc - r;
                        int ni = (int)cc;
                        if (c + 2 == 8) ni += (int)(y9[q] - dnext[q]);   // LDATI.py:106
                        nnext[q] = ni;
                    }
                }
                continue;
            }
        }
        // where the tile's run of this bin goes; its records are ranked into O at the same phase modulo four records, so that the
        // copy-out moves whole 16-byte pieces
        const unsigned dshift = dsto[2 * c] & 3u;
        uint2 *UL1 = reinterpret_cast<uint2 *>(O), *UL0 = UL1 + U1;
        unsigned *SLs = O + 2u * (U1 + U0);
        // ranks are taken in NW chunks of L = 2^lgL consecutive positions (one wave each); a record counts in its chunk's row
        int lgL = 6;
        while (((unsigned)NW << lgL) < N) ++lgL;
        const float offt_c = P.offt[c];
        const int kbase_c = (int)P.kbase[c];
        const unsigned pc = (unsigned)(pidx * 9 + c);
        // ---- D2: unit tables (and the rare voxel outside the slope table, generated in place by its owner) ---------
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const unsigned local = (unsigned)(lpx0 + q), pos = sbase + ((baseA + aex[q]) & 0xFFFFu);     // position in S
            const int n = ncur[q];
            const unsigned cl = cls[q] & 7u;
            if (cl == 1u) {
                SLs[sS + ((baseA + aex[q]) >> 16)] = pos | (local << 14);
                S[pos] = __float_as_uint(dcur[q]);               // the single's tendency waits in its record slot
            } else if (cl == 2u || cl == 3u) {
                const unsigned ue = baseU + uex[q];
                uint2 *dstu = cl == 2u ? UL0 + sU0 + (ue & 0xFFFFu) : UL1 + sU1 + (ue >> 16);
                const unsigned units = (unsigned)(n + 3) >> 2, hi = (cls[q] >> 3) << 14;
                dstu[0] = make_uint2(local | (((unsigned)n < 4u ? (unsigned)n : 4u) << 29), pos | hi);      // (most voxels: one or two units)
                if (units > 1u) {
                    const unsigned l1 = (unsigned)n - 4u;
                    dstu[1] = make_uint2(local | (1u << 11) | ((l1 < 4u ? l1 : 4u) << 29), (pos + 4u) | hi);
                    for (unsigned jb = 2; jb < units; ++jb) {
                        const unsigned left = (unsigned)n - 4u * jb;
                        dstu[jb] = make_uint2(local | (jb << 11) | ((left < 4u ? left : 4u) << 29), (pos + 4u * jb) | hi);
                    }
                }
            } else if (cl == 4u) {
                float k, bb;
                slope_params(nprev[q], n, nnext[q], c, P, k, bb);
                const unsigned px = (unsigned)x0 + local;
                for (int j = 0; j < n; ++j) {
                    float u = 0.0f;
                    if (philox) u = philox_uniform(P.seed, px, (unsigned)j, pc, frame);
                    else if (j < P.replay_max_n) u = P.uniforms[(((long long)(b * 2 + pidx) * 9 + c) * P.HW + px) * P.replay_max_n + j];
                    const unsigned key = multi_key(k, bb, u, offt_c, kbase_c, P, fast_k0);
                    const unsigned sp = pos + (unsigned)j;
                    S[sp] = (key << 12) | (1u << kLocalBits) | local;
                    atomicAdd(&hist[__umul24(sp >> lgL, (unsigned)P.NB) + (key >> P.shift)], 1u);
                }
            }
        }
        __syncthreads();                                 // A2: the work lists are complete
        STAMP(2);
        // ---- D3: timestamps, once; batches of 64 list entries, handed out through an LDS counter --------------------
        auto put = [&](unsigned sp, unsigned rec, unsigned key) {
            S[sp] = rec;
            atomicAdd(&hist[__umul24(sp >> lgL, (unsigned)P.NB) + (key >> P.shift)], 1u);
        };
        auto single_batch = [&](unsigned i) {                // (called by whole waves: single_key votes)
            const bool has = i < Ns;
            const unsigned e = has ? SLs[i] : 0u, sp = e & 0x3FFFu;
            const unsigned key = single_key(has, has ? __uint_as_float(S[sp]) : 0.0f, offt_c, P.kbase[c], fast_s, P);
            if (has) put(sp, (key << 12) | (e >> 14), key);
        };
        auto unit_batch = [&](auto mode_c, const uint2 *list, unsigned i, unsigned count) {
            // MODE 0: replayed uniforms (IEEE operations as the compiler expands them); 1 / 2: Philox, k == 0 units with /
            // without the checked fast constant divisions; 3: Philox, k != 0 units (sqrt_rn_nr / div_rn_nr)
            constexpr int MODE = decltype(mode_c)::value;
            if (i < count) {
                const uint2 e = list[i];
                const unsigned local = e.x & (kTilePix - 1), jb = (e.x >> kLocalBits) & 0x3FFFFu, cnt = e.x >> 29;
                const unsigned sp = e.y & 0x3FFFu;
                float2 kb = make_float2(0.0f, 0.0f);
                if (MODE == 0 || MODE == 3) kb = stab[e.y >> 14];
                const unsigned px = (unsigned)x0 + local;
                float u[4];
                unsigned key[4];
                if (MODE == 0 && !philox) {
                    const long long ub = (((long long)(b * 2 + pidx) * 9 + c) * P.HW + px) * P.replay_max_n;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int j = (int)(4u * jb) + s;
                        u[s] = ((unsigned)s < cnt && j < P.replay_max_n) ? P.uniforms[ub + j] : 0.0f;
                    }
                } else {
                    unsigned o[4];
                    philox4_b3(P.seed, px, jb, pc, frame, o);
#pragma unroll
                    for (int s = 0; s < 4; ++s) u[s] = u24(o[s]);
                }
                if (MODE == 0) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) key[s] = multi_key(kb.x, kb.y, u[s], offt_c, kbase_c, P, fast_k0);
                } else {
                    float tq[4];
                    if (MODE == 3) {
                        const float r1 = rcp_refined(kb.x), bb2 = kb.y * kb.y, k2 = 2.0f * kb.x;
#pragma unroll
                        for (int s = 0; s < 4; ++s) tq[s] = div_rn_nr(-kb.y + sqrt_rn_nr(bb2 + k2 * u[s]), kb.x, r1);
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) tq[s] = MODE == 1 ? k0_time_fast(u[s], P.FPS, P.RFPS, P.R9) : (u[s] / P.FPS) / 9.0f;
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float tt = tq[s] + offt_c;
                        tt = tt * 1e6f;
                        int kk = (int)tt - kbase_c;
                        kk = kk < 0 ? 0 : kk;
                        key[s] = (unsigned)(kk >= P.NK ? P.NK - 1 : kk);
                    }
                }
                const unsigned tag = (1u << kLocalBits) | local;
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if ((unsigned)s < cnt) put(sp + s, (key[s] << 12) | tag, key[s]);
            }
        };
        {
            const unsigned nK = (U1 + 63u) >> 6, nZ = (U0 + 63u) >> 6, nS = (Ns + 63u) >> 6, nb = nK + nZ + nS;
            unsigned nxt = 0;
            if (lane == 0) nxt = atomicAdd(bctr, 1u);
            for (;;) {
                const unsigned bid = (unsigned)__builtin_amdgcn_readfirstlane((int)nxt);
                if (bid >= nb) break;
                // far from the end the next batch is reserved now (its LDS round trip runs under this batch); near the end a
                // wave takes its next batch only when it is free, so that nobody sits on a batch an idle wave could run
                const bool early = bid + 2u * NW < nb;
                if (early && lane == 0) nxt = atomicAdd(bctr, 1u);
                if (bid < nK) {                          // the long batches first
                    if (philox) unit_batch(std::integral_constant<int, 3>{}, UL1, bid * 64u + lane, U1);
                    else unit_batch(std::integral_constant<int, 0>{}, UL1, bid * 64u + lane, U1);
                } else if (bid < nK + nZ) {
                    const unsigned i = (bid - nK) * 64u + lane;
                    if (!philox) unit_batch(std::integral_constant<int, 0>{}, UL0, i, U0);
                    else if (fast_k0) unit_batch(std::integral_constant<int, 1>{}, UL0, i, U0);
                    else unit_batch(std::integral_constant<int, 2>{}, UL0, i, U0);
                } else {
                    single_batch((bid - nK - nZ) * 64u + lane);
                }
                if (!early && lane == 0) nxt = atomicAdd(bctr, 1u);
            }
        }
        STAMP(4);
        __syncthreads();                                 // B: every row of the histogram is complete
        STAMP(5);
        // ---- D4: bucket-major, wave-minor exclusive scan; the tile's row of the run table ------------------------
        {
            // thread 2 b + h takes rows [h NW/2, (h + 1) NW/2) of bucket b when the workgroup has 2 NB threads (the workgroup
            // scan then runs over (bucket, half) in exactly the order the offsets need), else one thread takes the bucket
            const bool two = 2 * P.NB <= NT;                  // uniform
            constexpr int RH = NW / 2;
            const int bkt = two ? tid >> 1 : tid, r0 = two ? (tid & 1) * RH : 0, nr = two ? RH : NW;
            unsigned v[NW];
            unsigned run = 0;
            if (bkt < P.NB) {
#pragma unroll
                for (int w = 0; w < NW; ++w) v[w] = w < nr ? hist[__umul24((unsigned)(r0 + w), (unsigned)P.NB) + bkt] : 0u;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const unsigned x = v[w];
                    v[w] = run;
                    run += x;
                }
            }
            unsigned tot;
            const unsigned boff = block_excl_scan<NW>(run, spart, &tot);
            if (bkt < P.NB) {
#pragma unroll
                for (int w = 0; w < NW; ++w)
                    if (w < nr) hist[__umul24((unsigned)(r0 + w), (unsigned)P.NB) + bkt] = v[w] + boff + dshift;
            }
            unsigned short *row = P.roff + ((long long)(b * 9 + c) * P.T + t) * (P.NB + 1);
            if (bkt < P.NB && r0 == 0) row[bkt] = (unsigned short)boff;
            if (tid == 0) row[P.NB] = (unsigned short)N;
        }
        __syncthreads();                                 // C: bucket offsets per wave
        STAMP(6);
        // ---- D5: stable ranks: the wave walks its records in pixel order -------------------------------------------
        {
            const unsigned sh = 12 + P.shift;
            const unsigned lo = (unsigned)wid << lgL, hi = min(N, lo + (1u << lgL));
            if (atomic_order) {                          // the rank IS what the LDS atomic returns (g_lds_order_ok)
                // (four read -> atomic -> write chains in flight; a wave's LDS atomics execute in program order, so the ranks
                // are still taken in position order)
                unsigned i = lo + lane, i0 = lo;
                for (; i0 + 256u <= hi; i0 += 256u, i += 256u) {      // (a wave-uniform bound: every lane takes the same trips)
                    unsigned rec[4], at[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) rec[j] = S[i + 64u * j];
#pragma unroll
                    for (int j = 0; j < 4; ++j) at[j] = atomicAdd(&myhist[rec[j] >> sh], 1u);
#pragma unroll
                    for (int j = 0; j < 4; ++j) O[at[j]] = rec[j];
                }
                for (; i < hi; i += 64u) {
                    const unsigned rec = S[i];
                    O[atomicAdd(&myhist[rec >> sh], 1u)] = rec;
                }
            } else {
                for (unsigned i0 = lo; i0 < hi; i0 += 64) {
                    const unsigned i = i0 + lane;
                    const bool has = i < hi;
                    const unsigned rec = has ? S[i] : 0u;
                    const unsigned bucket = rec >> sh;
                    const unsigned pos = take_slots(has, bucket, P.nb1, &myhist[bucket]);
                    if (has) O[pos] = rec;
                }
            }
        }
        STAMP(7);
        __syncthreads();                                 // D: the run is complete in O
        STAMP(8);
        for (int i = lane; i < P.NB; i += 64) myhist[i] = 0;    // for the next bin (first touched behind its barrier A)
        if (tid == 0) *bctr = 0;
        {
            // O[dshift + i] -> dst[i]: 16-byte pieces where the piece lies inside the run, single records at its two ends
            const long long dst0 = (long long)(((unsigned long long)dsto[2 * c + 1] << 32) | dsto[2 * c]);
            unsigned *dstq = P.temp + (dst0 - (long long)dshift);             // 16-byte aligned (temp is; dst0 - dshift is a multiple of 4 records)
            const unsigned nq = (dshift + N + 3u) >> 2;
            for (unsigned q = tid; q < nq; q += NT) {
                const uint4 v = reinterpret_cast<const uint4 *>(O)[q];
                if (4u * q >= dshift && 4u * q + 4u <= dshift + N) {
                    reinterpret_cast<uint4 *>(dstq)[q] = v;
                } else {
                    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (4u * q + j >= dshift && 4u * q + j < dshift + N) dstq[4u * q + j] = w[j];
                }
            }
        }
        STAMP(9);
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            nprev[q] = ncur[q];
            ncur[q] = nnext[q];
            dcur[q] = dnext[q];
            if (c + 2 <= 8) {
                const float r = ynn[q] - dnext[q];
                const float cc = ceilf(r - eps);
                dnext[q] = cc - r;
                int ni = (int)cc;
                if (c + 2 == 8) ni += (int)(y9[q] - dnext[q]);   // LDATI.py:106
                nnext[q] = ni;
            }
        }
    }
    if (P.slot_cap) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int m = __shfl_xor(vmax_l, o);
            vmax_l = m > vmax_l ? m : vmax_l;
        }
        // (plain reads first: after the first few tiles these maxima rarely grow, and same-address atomics serialise)
        if (lane == 0 && vmax_l > 0 && (unsigned long long)vmax_l > *reinterpret_cast<volatile unsigned long long *>(&P.stats_w[0]))
            atomicMax(&P.stats_w[0], (unsigned long long)vmax_l);
        __syncthreads();
        if (tid < 9) P.tc_w[((long long)b * P.T + t) * 9 + tid] = nbin[tid];
        if (tid == 0) {
            unsigned tile_total = 0;
#pragma unroll
            for (int c = 0; c < 9; ++c) tile_total += nbin[c];
            if (tile_total > 0 && (unsigned long long)tile_total > *reinterpret_cast<volatile unsigned long long *>(&P.stats_w[4]))
                atomicMax(&P.stats_w[4], (unsigned long long)tile_total);
        }
    }
    STAMP(0);
    STAMP_FLUSH(0, 10);
}

// the common call (every run-time switch of dense_tile_body<NW, true> on) has its own copy of the body; any other call (replayed
// uniforms, 'none', ballot ranks, a device table not ready) runs the body with its run-time switches
template <int NW>
__global__ __launch_bounds__(64 * NW, 4) void ldati_tile_dense_kernel(LdatiParams P) {   // 4 waves per SIMD: two 512-thread workgroups per CU
    bool fast = P.fast_slot >= 0 && P.rng_mode == V2CE_RNG_PHILOX && !P.ballot_ranks && P.ts32 && (P.HW & 3) == 0 &&
                P.strategy != V2CE_STRATEGY_NONE;
    if (fast) {
        const FastDiv &f = g_fastdiv[P.fast_slot];
        fast = __builtin_amdgcn_readfirstlane((int)f.fps_bits) == (int)__float_as_uint(P.FPS) && __builtin_amdgcn_readfirstlane(f.ok) != 0 &&
               __builtin_amdgcn_readfirstlane(f.tab_ready) != 0 && __builtin_amdgcn_readfirstlane(f.ok64) != 0 &&
               __builtin_amdgcn_readfirstlane(g_lds_order_ok) != 0;
    }
    if (fast) dense_tile_body<NW, true>(P);
    else dense_tile_body<NW, false>(P);
}

// Exhaustive check of the dense kernel's exact-math helpers (v2ce_ldati_selfcheck; a test, never on the product path):
// for EVERY slope-table entry with k != 0 and EVERY uniform the Philox path can produce (m * 2^-24, m < 2^24) the time
// (-b + sqrt(b^2 + 2 k u)) / k by sqrt_rn_nr / div_rn_nr against the compiler's IEEE square root and division; and
// philox4_b3 against philox4 on the same counters.  bad[0] counts time mismatches, bad[1] Philox mismatches.
__global__ __launch_bounds__(256) void ldati_selfcheck_kernel(float VS, float VS2, float INV, int d0, unsigned long long *bad) {
    const unsigned m = blockIdx.x * 256u + threadIdx.x;                  // < 2^24
    const float u = (float)m * (1.0f / 16777216.0f);
    const int d = d0 + (int)blockIdx.y;
    unsigned nb = 0, np = 0;
    for (int n = 2; n <= kSlopeM; ++n) {
        const float sxy = (float)d;
        const float k0 = (3.0f * sxy) / 6.0f;
        const float k = (k0 / VS2) / ((float)n + 1e-8f);
        const float bb = INV - (VS * k) / 2.0f;
        if (k == 0.0f) continue;
        const float want = (-bb + __builtin_sqrtf(bb * bb + (2.0f * k) * u)) / k;
        const float r1 = rcp_refined(k), bb2 = bb * bb, k2 = 2.0f * k;
        const float got = div_rn_nr(-bb + sqrt_rn_nr(bb2 + k2 * u), k, r1);
        const bool same = __float_as_uint(want) == __float_as_uint(got) || (want != want && got != got);
        nb += same ? 0u : 1u;
    }
    {
        unsigned a[4], c[4];
        philox4(0x123456789ABCDEFull + (unsigned long long)d, m, m >> 7, (unsigned)(d & 15), m ^ 0x5bd1e995u, a);
        philox4_b3(0x123456789ABCDEFull + (unsigned long long)d, m, m >> 7, (unsigned)(d & 15), m ^ 0x5bd1e995u, c);
        np += (a[0] != c[0] || a[1] != c[1] || a[2] != c[2] || a[3] != c[3]) ? 1u : 0u;
    }
    if (nb) atomicAdd(&bad[0], (unsigned long long)nb);
    if (np) atomicAdd(&bad[1], (unsigned long long)np);
}

// ---------------------------------------------------------------------------------------------
// sparse tile pass: the same job as ldati_tile_pass_kernel for tiles with at most kSparseCap events
// over ALL NINE bins (real UNet output: ~2000 per 2048-pixel tile; the per-bin kernel spends its
// time in ~60 barriers and 18 workgroup scans for ~230 records per bin there).  One pass, 8 barriers:
//   1. all ten voxels of the thread's four pixels (one float4 per plane), relocation in registers
//   2. single events and multi-event (pixel, bin) pairs appended to two LDS lists (from both ends of
//      one 32 KB area), re-read densely: every lane computes a timestamp
//   3. records (bin-major combined key | multi | local pixel) appended unordered; u16 histogram
//      over the 9 * NB (bin, coarse bucket) cells by packed LDS atomics
//   4. in-place exclusive scan of the histogram; placement by a second packed atomic
//   5. inside each cell (mostly 0-2 records) the records are ordered by local pixel: the order the
//      bucket sort's stable ranks need (equal (timestamp, category) => ascending pixel)
//   6. nine coalesced runs + nine rows of the run table, exactly what the per-bin kernel writes.
// LDS: list area / records S + O (32 KB) | packed histogram (10 KB) | scalars.
// ---------------------------------------------------------------------------------------------
// FUSED (round 4, v2ce_ldati_count_fused): the kernel also IS the count pass -- it forms the tile's counts from the voxels it
// has just loaded (what ldati_count_tiles_kernel computes), so the voxel grid is read once per call instead of twice; the
// record offsets a count pass would have provided are not needed because every tile writes into its own slot of kSparseCap
// records (`temp` + slot; the (tile, bin) starts go to tile_abs for the bucket sort).  A tile beyond kSparseCap only reports
// its counts; the host then takes the two-pass path for the call (v2ce_ldati_emit_fused).
template <bool FUSED, bool BIDIR>                        // BIDIR: the instance for bidirectional calls reports keys outside the window
__global__ __launch_bounds__(kSparseThreads, V2CE_SPARSE_WAVES) void ldati_tile_sparse_kernel(LdatiParams P) {
    constexpr int NT = kSparseThreads, NW = NT / 64, PPT = kTilePix / NT;
    constexpr int HWORDS = NT * 5;                       // 10 cells per thread >= 9 * kMaxNB + 1
    const int t = blockIdx.x, b = blockIdx.y;
    unsigned ntot = 0;
    if (!FUSED) {
        const unsigned *tcr = P.tc + ((long long)b * P.T + t) * 9;
#pragma unroll
        for (int c = 0; c < 9; ++c) ntot += tcr[c];
        if (ntot > (unsigned)P.sparse_cap) return;          // dense tile: ldati_tile_pass_kernel handles it
    }
    const int pidx = t < P.tpp ? 1 : 0;
    const int x0 = (t < P.tpp ? t : t - P.tpp) * kTilePix;
    const int tid = threadIdx.x;
    const bool slot_ok = P.fast_slot >= 0 &&
                         __builtin_amdgcn_readfirstlane((int)g_fastdiv[P.fast_slot >= 0 ? P.fast_slot : 0].fps_bits) == (int)__float_as_uint(P.FPS);
    const bool fast_k0 = slot_ok && P.rng_mode == V2CE_RNG_PHILOX && __builtin_amdgcn_readfirstlane(g_fastdiv[P.fast_slot].ok) != 0;
    const float2 *stab = (slot_ok && __builtin_amdgcn_readfirstlane(g_fastdiv[P.fast_slot].tab_ready) != 0) ? g_slope_tab[P.fast_slot] : nullptr;

    unsigned *S = reinterpret_cast<unsigned *>(tile_smem);          // [kSparseCap] records (unordered, later final)
    unsigned *O = S + kSparseCap;                                   // [kSparseCap] records placed by cell
    uint2 *SL = reinterpret_cast<uint2 *>(S);                       // singles list, grows up: {debt bits, local | c << 11}
    unsigned *MPtop = S + 2 * kSparseCap;                           // multi list, grows down: {info, k, bb}
    unsigned *hist = S + 2 * kSparseCap;                            // [HWORDS] two u16 cells per word
    unsigned *misc = hist + HWORDS;                                 // cursors, scan partials, bin starts, per-bin scalars
    unsigned *cur = misc;                                           // [0] singles, [1] multi pairs, [2] records
    unsigned *part = misc + 4;                                      // [NW + 1]
    unsigned *binstart = part + 10;                                 // [10]
    float *offt_s = reinterpret_cast<float *>(binstart + 10);       // [9]
    long long *kbase_s = reinterpret_cast<long long *>(offt_s + 10);   // [9], 8-byte aligned (kSparseLds)
    unsigned *red = reinterpret_cast<unsigned *>(kbase_s + 9);         // [NW][10] the fused count's wave totals
    static_assert(NW + 1 <= 10 && ((2 * kSparseCap + HWORDS + 34) & 1) == 0, "sparse LDS map");
    long long dst_off[9];                                           // where the tile's nine runs go
#pragma unroll
    for (int c = 0; c < 9; ++c)
        dst_off[c] = FUSED ? 0ll : P.seg_offsets[b * 9 + c] + (long long)P.tile_off[((long long)b * P.T + t) * 9 + c];

    const float *plane0 = P.vox + (long long)(b * 2 + pidx) * 10 * P.HW;
    const unsigned frame = (unsigned)(P.frame_base + b);
    const int lpx0 = tid * PPT;
    const unsigned NKS = (unsigned)P.NB << P.shift;                 // key stride between bins (>= NK)

    STAMP_DECL;
    // ---- 1: loads (all in flight at once), then the LDS tables are cleared under them
    float yv[PPT][10];
    {
        const int px = x0 + lpx0;
        if ((P.HW & 3) == 0 && px + PPT <= P.HW) {
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const float4 v = *reinterpret_cast<const float4 *>(plane0 + (long long)i * P.HW + px);
                yv[0][i] = v.x; yv[1][i] = v.y; yv[2][i] = v.z; yv[3][i] = v.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < PPT; ++q)
#pragma unroll
                for (int i = 0; i < 10; ++i) yv[q][i] = (px + q < P.HW) ? plane0[(long long)i * P.HW + px + q] : 0.0f;
        }
    }
    for (int i = tid; i < HWORDS; i += NT) hist[i] = 0;
    if (tid < 4) cur[tid] = 0;
    if (tid < 9) { offt_s[tid] = P.offt[tid]; kbase_s[tid] = P.kbase[tid]; }
    __syncthreads();

    STAMP(0);
    // ---- 2a: classify; append to the lists (slots from wave_alloc: one LDS atomic per wave, pixel and list)
    const int lane_s = tid & 63;
    // FUSED: the count pass rides along (what ldati_count_tiles_kernel computes: events per bin, largest voxel count).  The
    // lists are written before the tile's total is known, so their indices are bounded: a tile whose lists would collide
    // has more than kSparseCap events and is discarded below anyway.
    int cnt9[9], vmax = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) cnt9[i] = 0;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        int nn[9];
        float td[9];
        relocate_all(yv[q], P.bidir != 0, nn, td);
        const unsigned local = (unsigned)(lpx0 + q);
        const bool valid = x0 + lpx0 + q < P.HW;
        unsigned ns = 0, nm = 0;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const int n = valid ? nn[c] : 0;
            ns += n == 1 ? 1u : 0u;
            nm += (n >= 2 && P.strategy != V2CE_STRATEGY_NONE) ? 1u : 0u;
            if (FUSED) {
                cnt9[c] += (P.strategy == V2CE_STRATEGY_NONE) ? (n == 1) : (n > 0 ? n : 0);
                vmax = n > vmax ? n : vmax;
            }
        }
        unsigned si = wave_alloc(&cur[0], ns, lane_s), mi0 = wave_alloc(&cur[1], nm, lane_s);
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const int n = valid ? nn[c] : 0;
            if (n == 1) {
                if (!FUSED || si < (unsigned)kSparseCap) SL[si] = make_uint2(__float_as_uint(td[c]), local | ((unsigned)c << kLocalBits));
                ++si;
            } else if (n >= 2 && P.strategy != V2CE_STRATEGY_NONE && (!FUSED || 3u * (mi0 + 1u) <= 2u * (unsigned)kSparseCap)) {
                float k, bb;
                if (P.kbb) {
                    const float2 kq = P.kbb[((long long)(b * 2 + pidx) * 9 + c) * P.HW + (x0 + lpx0 + q)];
                    k = kq.x; bb = kq.y;
                } else {
                    slope_params(c > 0 ? nn[c - 1] : 0, n, c < 8 ? nn[c + 1] : 0, c, P, k, bb, stab);
                }
                unsigned *e = MPtop - 3 * (mi0 + 1);
                ++mi0;
                e[0] = local | ((unsigned)c << kLocalBits) | ((unsigned)n << 15);
                e[1] = __float_as_uint(k);
                e[2] = __float_as_uint(bb);
            } else if (FUSED && n >= 2 && P.strategy != V2CE_STRATEGY_NONE) {
                ++mi0;                                       // (beyond the list: the tile is dense)
            }
        }
    }
    STAMP(1);
    if (FUSED) {
        // the tile's total and its largest voxel count: one wave scan and one wave maximum.  The per-bin counts of a tile that
        // fits come out of the cell scan for free (binstart, step 6); only a tile beyond kSparseCap -- which this kernel cannot
        // place -- reduces its nine per-bin sums here (what ldati_count_tiles_kernel reports)
        unsigned tl = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) tl += (unsigned)cnt9[i];
        const unsigned wt = wave_incl_scan(tl, lane_s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int m = __shfl_xor(vmax, o);
            vmax = m > vmax ? m : vmax;
        }
        if (lane_s == 63) red[(tid >> 6) * 10 + 8] = wt;
        if (lane_s == 0) red[(tid >> 6) * 10 + 9] = (unsigned)vmax;
    }
    __syncthreads();
    if (FUSED) {
        unsigned mx = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            ntot += red[w * 10 + 8];
            const unsigned v = red[w * 10 + 9];
            mx = v > mx ? v : mx;
        }
        // (plain reads first: after the first few tiles these maxima rarely grow, and same-address atomics serialise)
        if (tid == 9 && mx > 0 && (unsigned long long)mx > P.stats_w[0]) atomicMax(&P.stats_w[0], (unsigned long long)mx);
        if (tid == 10 && ntot > 0 && (unsigned long long)ntot > P.stats_w[4]) atomicMax(&P.stats_w[4], (unsigned long long)ntot);
        if (ntot > (unsigned)P.sparse_cap) {             // uniform: the call falls back to the two-pass path
            __syncthreads();                             // (red is rewritten)
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const unsigned tot = wave_incl_scan((unsigned)cnt9[i], lane_s);
                if (lane_s == 63) red[(tid >> 6) * 10 + i] = tot;
            }
            __syncthreads();
            if (tid < 9) {
                unsigned mine = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) mine += red[w * 10 + tid];
                P.tc_w[((long long)b * P.T + t) * 9 + tid] = mine;
            }
            return;
        }
    }
    STAMP(2);
    // ---- 2b: the lists move to registers (they share their LDS with the records)
    const unsigned Ns = cur[0], Nmp = cur[1];
    constexpr int SPT = kSparseCap / NT, MPT = kSparseCap / 2 / NT;    // most list entries per thread
    uint2 sl[SPT];
    unsigned mi[MPT];
    float mk[MPT], mb[MPT];
#pragma unroll
    for (int j = 0; j < SPT; ++j) sl[j] = (unsigned)(tid + j * NT) < Ns ? SL[tid + j * NT] : make_uint2(0u, 0u);
#pragma unroll
    for (int j = 0; j < MPT; ++j) {
        const unsigned m = (unsigned)(tid + j * NT);
        const unsigned *e = MPtop - 3 * (m + 1);
        mi[j] = m < Nmp ? e[0] : 0u;
        mk[j] = m < Nmp ? __uint_as_float(e[1]) : 0.0f;
        mb[j] = m < Nmp ? __uint_as_float(e[2]) : 0.0f;
    }
    __syncthreads();
    STAMP(3);
    // ---- 3: timestamps -> records, cell histogram
    auto put = [&](unsigned idx, unsigned c, unsigned key, unsigned multi, unsigned local) {
        const unsigned ck = __umul24(c, NKS) + key;       // (c < 9, NKS < 2^16: the 24-bit multiply issues at full rate)
        const unsigned g = ck >> P.shift;
        atomicAdd(&hist[g >> 1], 1u << ((g & 1u) * 16u));
        S[idx] = (ck << 12) | (multi << kLocalBits) | local;
    };
    const bool fast_s = slot_ok && P.ts32 && __builtin_amdgcn_readfirstlane(g_fastdiv[P.fast_slot].ok64) != 0;      // single_key's fast form
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        if ((unsigned)(j * NT) >= Ns) break;                 // uniform: no single left for anybody
        const bool has = (unsigned)(tid + j * NT) < Ns;
        const unsigned c = has ? sl[j].y >> kLocalBits : 0u;
        const unsigned key = BIDIR ? (unsigned)key_of_reporting(has, single_ts(__uint_as_float(sl[j].x), P.fps, offt_s[c]), kbase_s[c], P.NK, P.status)
                                   : single_key(has, __uint_as_float(sl[j].x), offt_s[c], kbase_s[c], fast_s, P);
        if (has) put((unsigned)(tid + j * NT), c, key, 0u, sl[j].y & (kTilePix - 1));   // a single's record index = its list index
    }
    STAMP(4);
#pragma unroll
    for (int j = 0; j < MPT; ++j) {
        if ((unsigned)(j * NT) >= Nmp) break;                // uniform: no multi-event pair left for anybody
        const bool have = (unsigned)(tid + j * NT) < Nmp;
        // the multi-event records follow the singles; cur[2] counts them (one atomic per wave)
        const unsigned i0 = Ns + wave_alloc(&cur[2], have ? mi[j] >> 15 : 0u, lane_s);
        if (have) {
            const unsigned local = mi[j] & (kTilePix - 1), c = (mi[j] >> kLocalBits) & 15u, n = mi[j] >> 15;
            const unsigned px = (unsigned)x0 + local;
            const float offt = offt_s[c];
            const long long kb64 = kbase_s[c];
            for (unsigned jb = 0; 4u * jb < n; ++jb) {
                const unsigned left = n - 4u * jb, cnt = left < 4u ? left : 4u;
                float u[4];
                if (P.rng_mode == V2CE_RNG_REPLAY) {
                    const long long ub = (((long long)(b * 2 + pidx) * 9 + c) * P.HW + px) * P.replay_max_n;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int jj = (int)(4u * jb) + s;
                        u[s] = ((unsigned)s < cnt && jj < P.replay_max_n) ? P.uniforms[ub + jj] : 0.0f;
                    }
                } else {
                    unsigned o[4];
                    philox4(P.seed, px, jb, (unsigned)pidx * 9u + c, frame, o);
#pragma unroll
                    for (int s = 0; s < 4; ++s) u[s] = u24(o[s]);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if ((unsigned)s < cnt) {
                        const unsigned key = BIDIR ? (unsigned)key_of_reporting(true, multi_ts(mk[j], mb[j], u[s], offt, P), kb64, P.NK, P.status)
                                           : P.ts32 ? multi_key(mk[j], mb[j], u[s], offt, (int)kb64, P, fast_k0)
                                                    : (unsigned)key_of(multi_ts(mk[j], mb[j], u[s], offt, P), kb64, P.NK);
                        put(i0 + 4u * jb + s, c, key, 1u, local);
                    }
            }
        }
    }
    __syncthreads();
    STAMP(5);
    const unsigned N = Ns + cur[2];
    if (N != ntot) {                                     // cannot happen: the count kernel saw the same voxels
        if (tid == 0) atomicExch(reinterpret_cast<unsigned *>(P.status), 3u);
        return;
    }
    // ---- 4: exclusive scan of the cells, in place (thread: cells 10 tid .. 10 tid + 9)
    {
        unsigned w[5], cnt[10], run = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) w[j] = hist[tid * 5 + j];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            cnt[j] = (w[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
            const unsigned v = cnt[j];
            cnt[j] = run;
            run += v;
        }
        unsigned tot;
        const unsigned ex = block_excl_scan<NW>(run, part, &tot);
#pragma unroll
        for (int j = 0; j < 5; ++j) hist[tid * 5 + j] = (cnt[2 * j] + ex) | ((cnt[2 * j + 1] + ex) << 16);
    }
    __syncthreads();
    STAMP(6);
    auto cell = [&](unsigned g) { return (hist[g >> 1] >> ((g & 1u) * 16u)) & 0xFFFFu; };
    // placement: the cell's word advances from its start to its end
    for (unsigned i = tid; i < N; i += NT) {
        const unsigned rec = S[i];
        const unsigned g = rec >> (12 + P.shift);
        const unsigned old = atomicAdd(&hist[g >> 1], 1u << ((g & 1u) * 16u));
        O[(old >> ((g & 1u) * 16u)) & 0xFFFFu] = rec;
    }
    __syncthreads();
    STAMP(7);
    if (tid < 10) binstart[tid] = tid == 9 ? N : (tid ? cell((unsigned)tid * (unsigned)P.NB - 1u) : 0u);
    // ---- 5: order inside the cells: by local pixel (ties: by arrival, any fixed order is right); four records per thread at a
    // time, so that their dependent LDS reads (record, the cell's two bounds, the cell's members) overlap
    for (unsigned i0 = tid; i0 < N; i0 += 4 * NT) {
        unsigned rec[4], lo[4], hi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rec[j] = i0 + j * NT < N ? O[i0 + j * NT] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned g = rec[j] >> (12 + P.shift);
            lo[j] = g ? cell(g - 1) : 0u;
            hi[j] = cell(g);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned i = i0 + j * NT;
            if (i < N) {
                unsigned r = lo[j];
                if (hi[j] - lo[j] > 1u) {
                    const unsigned me = rec[j] & (kTilePix - 1);
                    for (unsigned q = lo[j]; q < hi[j]; ++q) {
                        const unsigned o = O[q] & (kTilePix - 1);
                        r += (o < me || (o == me && q < i)) ? 1u : 0u;
                    }
                }
                S[r] = rec[j];
            }
        }
    }
    __syncthreads();
    STAMP(8);
    // ---- 6: nine runs of records, nine rows of the run table
    unsigned bst[10];
#pragma unroll
    for (int c = 0; c < 10; ++c) bst[c] = binstart[c];
    if (FUSED) {
        // the nine runs are contiguous in the tile's slot: one loop, the bin of a record from its position
        const long long slot = ((long long)b * P.T + t) * kSparseCap;
        if (tid < 9) {
            P.tile_abs_w[(long long)(b * 9 + tid) * P.Tp + t] = (unsigned)(slot + bst[tid]);
            P.tc_w[((long long)b * P.T + t) * 9 + tid] = bst[tid + 1] - bst[tid];       // the count pass's output
        }
        unsigned *dst = P.temp + slot;
        for (unsigned i = tid; i < N; i += NT) {
            unsigned c = 0;
#pragma unroll
            for (int j = 1; j < 9; ++j) c += i >= bst[j] ? 1u : 0u;
            dst[i] = S[i] - (__umul24(c, NKS) << 12);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const unsigned bs = bst[c], Nc = bst[c + 1] - bs;
            const unsigned strip = ((unsigned)c * NKS) << 12;
            unsigned *dst = P.temp + dst_off[c];
            for (unsigned i = tid; i < Nc; i += NT) dst[i] = S[bs + i] - strip;
        }
    }
    {
        unsigned short *row0 = P.roff + ((long long)(b * 9) * P.T + t) * (P.NB + 1);
        const long long rstep = (long long)P.T * (P.NB + 1);
        for (int k0 = 0; k0 < P.NB; k0 += NT) {          // (one trip: NB <= kSparseThreads unless the key range is huge)
            const int kk = k0 + tid;
            if (kk < P.NB) {
                unsigned cv[9];
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    const unsigned g = (unsigned)c * (unsigned)P.NB + (unsigned)kk;
                    cv[c] = g ? cell(g - 1) : 0u;
                }
#pragma unroll
                for (int c = 0; c < 9; ++c) row0[c * rstep + kk] = (unsigned short)(cv[c] - bst[c]);
            }
        }
        if (tid < 9) row0[tid * rstep + P.NB] = (unsigned short)(bst[tid + 1] - bst[tid]);
    }
    STAMP(9);
    STAMP_FLUSH(0, 10);
}

// per segment: bucket totals over the tiles, their exclusive prefix, and the SORT GROUPS: maximal
// runs of consecutive coarse buckets with at most cap2 records and at most `span` buckets (so that the
// group's (key, category) histogram fits the sort workgroup).  Timestamps crowd towards the end of a
// bin on real UNet output (small voxel values: the single event falls where the accumulated mass
// crosses 1), so equal-width buckets differ by 20x in a segment; the groups even that out.  A single
// coarse bucket beyond cap2 (degenerate ties: constant images; bidirectional relocation puts every
// single of bin 8 with y[9] = 0 at the same microsecond) goes to the big-bucket kernel's list.
__global__ __launch_bounds__(512) void ldati_bucket_scan_kernel(LdatiParams P) {
    __shared__ unsigned part[9];
    __shared__ unsigned pre[kMaxNB + 2];               // sums of the tiles' run starts, then the bucket prefix
    const int seg = blockIdx.x, t = threadIdx.x;
    const unsigned short *tab = P.roff + (long long)seg * P.T * (P.NB + 1);
    unsigned *bofs = P.bofs + (long long)seg * (P.NB + 1);
    // a bucket's total = sum over the tiles of (start of the next bucket - its start) = difference of the
    // column sums: one load per tile and thread (NB + 1 <= 513 columns, 512 threads + one straggler).
    // (Round 4 tried handing the table to the sort TRANSPOSED -- [bucket][tile], through LDS here -- so that its setup reads
    // two contiguous columns instead of one 938-byte-strided load per tile: sort 520 -> 483 us on the stress chunk, but this
    // kernel 34 -> 48 us there and 20 -> 50 us in the e2e regime (576 segments, latency-bound): removed.)
    for (int i = t; i <= P.NB; i += 512) {
        unsigned s = 0;
#pragma unroll 22                                           // (latency-bound: a quarter of the 88 tiles' loads in flight at a time)
        for (int tt = 0; tt < P.T; ++tt) s += (unsigned)tab[(long long)tt * (P.NB + 1) + i];
        pre[i] = s;
    }
    __syncthreads();
    const unsigned tot_i = t < P.NB ? pre[t + 1] - pre[t] : 0u;
    unsigned total;
    const unsigned ex = block_excl_scan<8>(tot_i, part, &total);      // barriers inside: pre[] is free afterwards
    if (t < P.NB) bofs[t] = ex;
    if (t == 0) bofs[P.NB] = total;
    __syncthreads();
    if (t < P.NB) pre[t] = ex;
    if (t == 0) pre[P.NB] = total;
    __syncthreads();
    // greedy groups: from bucket i, the farthest end with <= cap2 records and <= span buckets; a bucket beyond cap2 on its
    // own goes to the big-bucket list; runs of empty buckets are skipped.  The step from EVERY bucket is computed in
    // parallel (binary searches on the prefix: one thread per bucket), then one thread follows the chain from bucket 0
    // -- one LDS read per group instead of ~9 dependent ones (the serial version was 60 of this kernel's 75 us).
    __shared__ unsigned step_to[kMaxNB + 1];           // next bucket | kind << 16  (kind 0 skip, 1 group, 2 big, 3 stop)
    if (t < P.NB) {
        const int i = t;
        const unsigned base = pre[i];
        unsigned st;
        if (base == total) {
            st = (3u << 16);                                           // nothing but empty buckets left
        } else if (pre[i + 1] == base) {                               // a run of empty buckets: to the first non-empty one
            int lo = i + 1, hi = P.NB;                                 // first j > i with pre[j] > base
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pre[mid] > base) hi = mid; else lo = mid + 1;
            }
            st = (unsigned)(lo - 1);
        } else if (pre[i + 1] - base > (unsigned)P.cap2) {
            st = (unsigned)(i + 1) | (2u << 16);
        } else {
            int lo = i + 1, hi = i + P.span < P.NB ? i + P.span : P.NB;   // largest e in [lo, hi] with pre[e] - base <= cap2
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] - base <= (unsigned)P.cap2) lo = mid; else hi = mid - 1;
            }
            st = (unsigned)lo | (1u << 16);
        }
        step_to[i] = st;
    }
    if (t == 0) step_to[P.NB] = 3u << 16;
    __syncthreads();
    __shared__ unsigned sgrp[kMaxNB];
    __shared__ unsigned sng;
    if (t == 0) {
        unsigned *grp = P.groups + (long long)seg * P.NB;
        unsigned ng = 0;
        int i = 0;
        while (i < P.NB) {
            const unsigned st = step_to[i];
            const unsigned kind = st >> 16, nx = st & 0xFFFFu;
            if (kind == 3u) break;
            if (kind == 1u) { sgrp[ng] = (unsigned)i | (nx << 16); grp[ng++] = (unsigned)i | (nx << 16); }
            else if (kind == 2u) P.big_list[atomicAdd(P.nbig, 1u)] = ((unsigned)seg << 16) | (unsigned)i;
            i = (int)nx;
        }
        P.ngroups[seg] = ng;
        sng = ng;
        P.seg_flag[seg] = 0;
        if (seg == 0 && P.fused_status && *P.fused_status) atomicExch(reinterpret_cast<unsigned *>(P.status), (unsigned)*P.fused_status);
    }
    __syncthreads();
    // every sort group's run in every tile (the table was read a moment ago: these loads hit L2), one contiguous row per group
    {
        const unsigned ng = sng;
        unsigned *out = P.gruns + (long long)seg * P.NB * P.Tp;
        // thread = (tile, group lane): no division, the groups' loads independent of each other
        int lgT = 3;
        while ((1 << lgT) < P.T) ++lgT;
        if (lgT <= 9) {
            const unsigned tt = (unsigned)t & ((1u << lgT) - 1u), gstep = 512u >> lgT;
            if (tt < (unsigned)P.T) {
                const unsigned short *row = tab + (long long)tt * (P.NB + 1);
#pragma unroll 4
                for (unsigned g = (unsigned)t >> lgT; g < ng; g += gstep) {
                    const unsigned gr = sgrp[g];
                    const unsigned r0 = row[gr & 0xFFFFu];
                    out[(long long)g * P.Tp + tt] = r0 | (((unsigned)row[gr >> 16] - r0) << 16);
                }
            }
        } else {
            for (unsigned idx = t; idx < ng * (unsigned)P.T; idx += 512) {
                const unsigned g = idx / (unsigned)P.T, tt = idx - g * (unsigned)P.T;
                const unsigned gr = sgrp[g];
                const unsigned short *row = tab + (long long)tt * (P.NB + 1);
                const unsigned r0 = row[gr & 0xFFFFu];
                out[(long long)g * P.Tp + tt] = r0 | (((unsigned)row[gr >> 16] - r0) << 16);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// bucket sort: workgroup (256 threads) per (segment, bucket), at most K records per thread, kept in
// registers between the histogram and the rank phase.  LDS map (dynamic):
//   Out [256*K] u32 | hist [4][bins] u32 | tcnt/toff [T] | tpre [T+1] | part | stage [256*13] u32
// ---------------------------------------------------------------------------------------------
extern __shared__ __attribute__((aligned(16))) unsigned char sort_smem[];

template <bool PACKED, int K, int kSortThreads>
__global__ __launch_bounds__(kSortThreads, 4) void ldati_bucket_sort_kernel(LdatiParams P) {
    constexpr int kSortWaves = kSortThreads / 64;
    const int seg = blockIdx.y;
    // (the group word is requested together with the group count -- an entry beyond the count holds whatever the workspace held and
    // is not used --: one dependent global-load latency less in front of every working workgroup's setup)
    const unsigned ngr = P.ngroups[seg];
    const unsigned grp = P.groups[(long long)seg * P.NB + blockIdx.x];
    if (blockIdx.x >= ngr) return;                       // uniform per workgroup (flagged segments have no groups; empty
                                                         // workgroups cost nothing measurable: a compact group list changed nothing)
    const int bk0 = (int)(grp & 0xFFFFu), bk1 = (int)(grp >> 16);           // coarse buckets [bk0, bk1)
    const unsigned *bofs = P.bofs + (long long)seg * (P.NB + 1);
    const unsigned N = bofs[bk1] - bofs[bk0];
    const unsigned key0 = (unsigned)bk0 << P.shift;      // first key of the group
    const int b = seg / 9, c = seg - b * 9;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int bins = ((bk1 - bk0) << P.shift) * 4;       // (relative key, category); <= 4 * kMaxSpanKeys
    int nb2 = 2;
    while ((1 << nb2) < bins) ++nb2;
    const bool atomic_order = !P.ballot_ranks && __builtin_amdgcn_readfirstlane(g_lds_order_ok) != 0;

    unsigned *Out = reinterpret_cast<unsigned *>(sort_smem);
    unsigned *hist = Out + kSortThreads * K + 20;        // [kSortWaves][bins]  (Out: 20 more words, the slot phase of the emit loop)
    unsigned *ne_src = hist + kSortWaves * P.hist_bins;  // [T] per non-empty tile: source index - flat index
    unsigned *ne_info = ne_src + P.T;                    // [T] (polarity category << PB) | first pixel of the tile
    unsigned *bits = ne_info + P.T;                      // [K*8] bit i = a tile's run starts at flat index i
    constexpr int kWords = kSortThreads * K / 32;        // words of the run-start bit table
    unsigned *wpre = bits + kWords;                      // [kWords] run starts below each 32-index word
    unsigned *part = wpre + kWords;                      // [kSortWaves + 1]
    unsigned *stage = hist;                              // [256 * 13], 16-byte aligned; aliases the tables (dead in S5)

    STAMP_DECL;
    // S0 (wave 0; the other waves clear the histograms meanwhile): this bucket's run in every tile,
    // TPL consecutive tiles per lane; exclusive prefix of (records | non-empty << 16) over the tiles
    // by a wave scan; list of the non-empty tiles; bit table of the run starts and its word prefix.
    if (wid == 0) {
        auto setup = [&](auto tpl_c) {
        constexpr int TPL = decltype(tpl_c)::value;
        for (int i = lane; i < kWords; i += 64) bits[i] = 0;
        unsigned cv[TPL], ov[TPL];
        unsigned sum = 0;
        {
            // branch-free (tiles past the last one read the last one's entries and are masked): all 2 TPL loads are issued
            // back to back and waited for once -- behind a per-tile `if` each pair was waited for before the next was issued
            const unsigned *gr_row = P.gruns + ((long long)seg * P.NB + blockIdx.x) * P.Tp;
            const unsigned *ts_row = P.tile_src + (long long)seg * P.Tp;
            unsigned gr[TPL], ts[TPL];
#pragma unroll
            for (int q = 0; q < TPL; ++q) {
                const int tt = min(lane * TPL + q, P.T - 1);
                gr[q] = gr_row[tt];
                ts[q] = ts_row[tt];
            }
#pragma unroll
            for (int q = 0; q < TPL; ++q) {
                const bool in = lane * TPL + q < P.T;
                cv[q] = in ? gr[q] >> 16 : 0u;
                ov[q] = (gr[q] & 0xFFFFu) + ts[q];
                sum += cv[q] | (cv[q] ? 0x10000u : 0u);
            }
        }
        unsigned ex = wave_incl_scan(sum, lane) - sum;
#pragma unroll
        for (int q = 0; q < TPL; ++q) {
            if (cv[q]) {
                const unsigned tt = (unsigned)(lane * TPL + q), pre = ex & 0xFFFFu, j = ex >> 16;
                const bool neg = tt < (unsigned)P.tpp;
                ne_src[j] = ov[q] - pre;
                ne_info[j] = ((neg ? 0u : 2u) << P.PB) | ((neg ? tt : tt - (unsigned)P.tpp) * kTilePix);
                atomicOr(&bits[pre >> 5], 1u << (pre & 31u));
                ex += cv[q] | 0x10000u;
            }
        }
        // word prefix of the run starts: WPL consecutive words per lane
        constexpr int WPL = (kWords + 63) / 64;
        unsigned pc[WPL];
        unsigned ps = 0;
#pragma unroll
        for (int q = 0; q < WPL; ++q) {
            const int wd = lane * WPL + q;
            pc[q] = wd < kWords ? (unsigned)__popc(bits[wd]) : 0u;
            ps += pc[q];
        }
        unsigned pex = wave_incl_scan(ps, lane) - ps;
#pragma unroll
        for (int q = 0; q < WPL; ++q) {
            const int wd = lane * WPL + q;
            if (wd < kWords) wpre[wd] = pex;
            pex += pc[q];
        }
        };
        if (P.T <= 128) setup(std::integral_constant<int, 2>{}); else setup(std::integral_constant<int, kMaxTiles / 64>{});
    } else if (kSortWaves > 1) {
        for (int i = tid - 64; i < kSortWaves * bins; i += kSortThreads - 64) hist[i] = 0;
    }
    if (kSortWaves == 1)
        for (int i = tid; i < bins; i += 64) hist[i] = 0;
    __syncthreads();
    STAMP(0);
    // S1: gather.  The bucket's records are the tiles' runs in tile order (negative tiles first,
    // each in pixel order); wave w owns the contiguous flat range [lo, hi).  The tile of a flat
    // index = number of run starts at or below it (bit table + word prefix); every lane issues all
    // its loads before the first use.
    const unsigned L = ((N + kSortThreads - 1) / kSortThreads) * 64;
    const unsigned lo = wid * L, hi = (lo + L < N) ? lo + L : N;
    const unsigned *seg_temp = P.tile_abs ? P.temp : P.temp + P.seg_offsets[seg];
    unsigned rec[K];
    unsigned tinfo[K];
    {
        // branch-free and staged, so that every stage's LDS reads / global loads are issued back to
        // back and waited for once: indices past the wave's range are clamped (their loads are valid
        // and ignored)
        unsigned bw[K], pw[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const unsigned i = min(lo + 64u * k + lane, N - 1u);
            bw[k] = bits[i >> 5];
            pw[k] = wpre[i >> 5];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const unsigned i = min(lo + 64u * k + lane, N - 1u);
            const unsigned j = pw[k] + (unsigned)__popc(bw[k] & (0xFFFFFFFFu >> (31u - (i & 31u)))) - 1u;
            tinfo[k] = ne_info[j];
            bw[k] = ne_src[j];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const unsigned i = min(lo + 64u * k + lane, N - 1u);
            rec[k] = seg_temp[bw[k] + i];
        }
    }
    STAMP(1);
    // S2: widen to (fine | category | global pixel); per-wave histograms of (fine, category).  A wave's range is whole
    // 64-record batches plus at most one partial one: the full batches run without per-lane guards (a scalar branch per
    // batch instead of an exec-mask sequence per record; the kernel is bound by instruction issue, not by memory)
    const int nfull = __builtin_amdgcn_readfirstlane((int)((hi > lo ? hi - lo : 0u) >> 6));
    const int ntail = __builtin_amdgcn_readfirstlane((int)((hi > lo ? hi - lo : 0u) & 63u));
    unsigned *myhist = hist + wid * bins;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k < nfull || (k == nfull && lane < ntail)) {     // first test: wave-uniform
            const unsigned r = rec[k];
            rec[k] = (((r >> 12) - key0) << (2 + P.PB)) | (tinfo[k] + (((r >> kLocalBits) & 1u) << P.PB) + (r & (kTilePix - 1)));
            atomicAdd(&myhist[rec[k] >> P.PB], 1u);
        }
    }
    STAMP(2);
    __syncthreads();
    STAMP(3);
    // The packed emit loop (S5) walks SLOTS: four records per lane starting at a global record index that is a multiple of
    // 16; record i of the group is ranked into Out[i + oshift], its slot, so that a lane's four records are one aligned
    // 16-byte LDS read (they used to be four reads at a four-word lane stride: 8-way bank conflicts, and an index clamp each)
    const long long g0 = P.seg_offsets[seg] + bofs[bk0];                  // first global record
    const unsigned oshift = PACKED ? (unsigned)(g0 - (((g0 >> 2) & ~3ll) << 2)) : 0u;      // in [0, 15]
    // S3: bin-major, wave-minor exclusive scan
    {
        const int per = (bins + kSortThreads - 1) / kSortThreads;
        const int b0 = tid * per, b1 = (b0 + per < bins) ? b0 + per : bins;
        unsigned s = 0;
        for (int q = b0; q < b1; ++q)
#pragma unroll
            for (int w = 0; w < kSortWaves; ++w) s += hist[w * bins + q];
        unsigned tot;
        unsigned run = block_excl_scan<kSortWaves>(s, part, &tot) + oshift;
        for (int q = b0; q < b1; ++q) {
#pragma unroll
            for (int w = 0; w < kSortWaves; ++w) {
                const unsigned v = hist[w * bins + q];
                hist[w * bins + q] = run;
                run += v;
            }
        }
    }
    __syncthreads();
    STAMP(4);
    // S4: stable ranks
    if (atomic_order) {                                  // the rank IS the value the LDS atomic returns (g_lds_order_ok)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k < nfull) {                             // wave-uniform
                const unsigned r = rec[k];
                Out[atomicAdd(&myhist[r >> P.PB], 1u)] = r;
            } else if (k == nfull && lane < ntail) {
                const unsigned r = rec[k];
                Out[atomicAdd(&myhist[r >> P.PB], 1u)] = r;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (lo + 64u * k < hi) {                     // wave-uniform
                const unsigned i = lo + 64u * k + lane;
                const bool has = i < hi;
                const unsigned r = rec[k];
                const unsigned bin = r >> P.PB;
                const unsigned pos = take_slots(has, bin, nb2, &myhist[bin]);
                if (has) Out[pos] = r;
            }
        }
    }
    STAMP(5);
    __syncthreads();
    STAMP(6);
    // S5: decode and write the final records
    const long long tbase = P.kbase[c] + (long long)key0 +
                            (P.frame_ts_add ? P.frame_ts_add[b] : 0);
    const unsigned pmask = (1u << P.PB) - 1u;
    const unsigned W = (unsigned)P.W;
    const float rcpW = 1.0f / (float)W;
    const bool small = P.HW < (1 << 24);                 // pixel indices exact in f32
    const bool tiny = P.HW < (1 << 22) - 1;              // ... and far enough from 2^22 for div_tiny
    if (!PACKED) {
        for (unsigned i = tid; i < N; i += kSortThreads) {
            const unsigned r = Out[i];
            const unsigned px = r & pmask, cat = (r >> P.PB) & 3u, fine = r >> (P.PB + 2);
            const unsigned yy = tiny ? div_tiny(px, rcpW) : small ? div_small(px, W, rcpW) : px / W;
            P.ts[g0 + i] = tbase + fine;
            P.x[g0 + i] = (short)(px - yy * W);
            P.y[g0 + i] = (short)yy;
            P.p[g0 + i] = (signed char)(cat >> 1);
        }
        return;
    }
    // Four records starting at a global record index that is a multiple of 4 are 13 whole dwords
    // (52 bytes).  Per iteration the workgroup assembles 256 such groups (13 312 bytes, starting at a
    // 16-byte aligned global address) in LDS and copies the image out 16 bytes per lane; only the
    // two 16-byte pieces at the ends of the bucket are written byte by byte.
    const long long gN = g0 + N;
    const long long G0 = (g0 >> 2) & ~3ll, G1 = (gN + 3) >> 2;         // G0 % 4 == 0: 52*G0 % 16 == 0
    const long long B0 = 13 * g0, B1 = 13 * gN;                         // this bucket's bytes
    const int nG_all = (int)(G1 - G0);                                 // groups of four records this bucket touches
    // one copy of the loop per division form (the kernel is bound by instruction issue: a uniform three-way branch per
    // record costs more than the division it selects)
    auto emit_loop = [&](auto mode_c) {
        constexpr int MODE = decltype(mode_c)::value;                  // 0: div_tiny, 1: div_small, 2: integer division
        // Every WAVE assembles and copies out its own 64 groups (3328 bytes = 208 16-byte pieces, 16-byte aligned in global
        // memory like the workgroup's image): no workgroup barrier inside the loop (round 4; the loop used to pay two per
        // 1024 records and was 45 % of the kernel's time)
        for (int ga = 0; ga < nG_all; ga += kSortThreads) {
            const int gw0 = ga + 64 * wid;
            const int g = gw0 + lane;
            if (g < nG_all) {
                unsigned A[4], Bh[4], C[4], D[4];
                // (slots outside the bucket hold whatever the LDS held: their bytes are never copied out)
                const uint4 r4 = reinterpret_cast<const uint4 *>(Out)[g];
                const unsigned rr[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned r = rr[q];
                    const unsigned px = r & pmask, cat = (r >> P.PB) & 3u, fine = r >> (P.PB + 2);
                    const unsigned yy = MODE == 0 ? div_tiny(px, rcpW) : MODE == 1 ? div_small(px, W, rcpW) : px / W;
                    const long long tq = tbase + fine;
                    A[q] = (unsigned)tq;
                    Bh[q] = (unsigned)((unsigned long long)tq >> 32);
                    // (v_mul_lo_u32 issues at a quarter of the rate of v_mul_u32_u24; px < 2^24 in the two float-division modes)
                    // yy * W: only its low 16 bits are used, so the compiler drops __umul24's masks and falls back to the
                    // quarter-rate v_mul_lo_u32 -- hence the instruction by name (px < 2^24 in the two float-division modes)
                    unsigned yw;
                    if (MODE == 2) yw = yy * W;
                    else asm("v_mul_u32_u24 %0, %1, %2" : "=v"(yw) : "v"(yy), "v"(W));
                    C[q] = ((px - yw) & 0xFFFFu) | (yy << 16);
                    D[q] = cat >> 1;
                }
                unsigned *d = stage + tid * 13;
                d[0] = A[0]; d[1] = Bh[0]; d[2] = C[0];
                d[3] = D[0] | (A[1] << 8);
                d[4] = (A[1] >> 24) | (Bh[1] << 8);
                d[5] = (Bh[1] >> 24) | (C[1] << 8);
                d[6] = (C[1] >> 24) | (D[1] << 8) | (A[2] << 16);
                d[7] = (A[2] >> 16) | (Bh[2] << 16);
                d[8] = (Bh[2] >> 16) | (C[2] << 16);
                d[9] = (C[2] >> 16) | (D[2] << 16) | (A[3] << 24);
                d[10] = (A[3] >> 8) | (Bh[3] << 24);
                d[11] = (Bh[3] >> 8) | (C[3] << 24);
                d[12] = (C[3] >> 8) | (D[3] << 24);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                               // (one wave's LDS operations complete in order)
            const int left = nG_all - gw0;
            const int nG = left < 64 ? (left > 0 ? left : 0) : 64;
            const int nPieces = (nG * 52 + 15) >> 4;
            const long long img = 52 * (G0 + gw0);                         // global byte address of the wave's image
            // pieces [qa, qb) lie wholly inside this bucket's bytes (all but the first and the last of the bucket)
            const long long r0l = B0 - img, r1l = B1 - img;
            const int rel0 = (int)(r0l < -(1 << 20) ? -(1 << 20) : r0l), rel1 = (int)r1l;     // rel1 <= 13 * cap2 + 256
            const int qa = rel0 > 0 ? (rel0 + 15) >> 4 : 0, qb = rel1 >> 4;
            unsigned char *dst = P.packed + img;
            const unsigned *stage_w = stage + wid * (64 * 13);
            for (int q = lane; q < nPieces; q += 64) {
                if (q >= qa && q < qb) {
                    reinterpret_cast<uint4 *>(dst)[q] = reinterpret_cast<const uint4 *>(stage_w)[q];
                } else {
                    const unsigned char *sb = reinterpret_cast<const unsigned char *>(stage_w) + 16 * q;
                    for (int k = 0; k < 16; ++k)
                        if (16 * q + k >= rel0 && 16 * q + k < rel1) dst[16 * q + k] = sb[k];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    };
    if (tiny) emit_loop(std::integral_constant<int, 0>{});
    else if (small) emit_loop(std::integral_constant<int, 1>{});
    else emit_loop(std::integral_constant<int, 2>{});
    STAMP(7);
    STAMP_FLUSH(16, 8);
}

// ---------------------------------------------------------------------------------------------
// big buckets: a coarse bucket with more records than a sort workgroup holds in LDS (degenerate ties).
// One workgroup per listed bucket: histogram of (fine key, category) over all its records (any
// order), exclusive scan, then ONE wave walks the records in input order (tiles ascending, pixel order
// inside a run) and takes stable slots 64 at a time; the records go straight to their final place.
// Rare and slow on purpose; keeps the two-level path complete for any input.
// ---------------------------------------------------------------------------------------------
template <bool PACKED>
__global__ __launch_bounds__(256) void ldati_big_bucket_kernel(LdatiParams P) {
    __shared__ unsigned hist[4 << kMaxShift];
    __shared__ unsigned part[5];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool atomic_order = !P.ballot_ranks && __builtin_amdgcn_readfirstlane(g_lds_order_ok) != 0;
    const int bins = 4 << P.shift, nb2 = P.shift + 2;
    const unsigned nbig = *P.nbig;
    for (unsigned idx = blockIdx.x; idx < nbig; idx += gridDim.x) {
        const unsigned e = P.big_list[idx];
        const int seg = (int)(e >> 16), bucket = (int)(e & 0xFFFFu);
        const int b = seg / 9, c = seg - b * 9;
        const unsigned *bofs = P.bofs + (long long)seg * (P.NB + 1);
        const long long g0 = P.seg_offsets[seg] + bofs[bucket];
        const unsigned key0 = (unsigned)bucket << P.shift;
        const long long tbase = P.kbase[c] + (long long)key0 + (P.frame_ts_add ? P.frame_ts_add[b] : 0);
        const unsigned *seg_temp = P.tile_abs ? P.temp : P.temp + P.seg_offsets[seg];
        for (int i = tid; i < bins; i += 256) hist[i] = 0;
        __syncthreads();
        for (int tt = 0; tt < P.T; ++tt) {
            const unsigned short *row = P.roff + ((long long)seg * P.T + tt) * (P.NB + 1);
            const unsigned r0 = row[bucket], len = (unsigned)row[bucket + 1] - r0;
            const unsigned *src = seg_temp + P.tile_src[(long long)seg * P.Tp + tt] + r0;
            const unsigned catb = tt < P.tpp ? 0u : 2u;
            for (unsigned j = tid; j < len; j += 256) {
                const unsigned r = src[j];
                atomicAdd(&hist[(((r >> 12) - key0) << 2) | (catb + ((r >> kLocalBits) & 1u))], 1u);
            }
        }
        __syncthreads();
        {
            const int per = (bins + 255) / 256;
            const int b0 = tid * per, b1 = (b0 + per < bins) ? b0 + per : bins;
            unsigned s = 0;
            for (int q = b0; q < b1; ++q) s += hist[q];
            unsigned tot;
            unsigned run = block_excl_scan<4>(s, part, &tot);
            for (int q = b0; q < b1; ++q) {
                const unsigned v = hist[q];
                hist[q] = run;
                run += v;
            }
        }
        __syncthreads();
        if (tid < 64) {
            for (int tt = 0; tt < P.T; ++tt) {
                const unsigned short *row = P.roff + ((long long)seg * P.T + tt) * (P.NB + 1);
                const unsigned r0 = row[bucket], len = (unsigned)row[bucket + 1] - r0;
                const unsigned *src = seg_temp + P.tile_src[(long long)seg * P.Tp + tt] + r0;
                const unsigned catb = tt < P.tpp ? 0u : 2u;
                const unsigned pxb = (unsigned)(tt < P.tpp ? tt : tt - P.tpp) * kTilePix;
                for (unsigned j0 = 0; j0 < len; j0 += 64) {
                    const unsigned j = j0 + lane;
                    const bool has = j < len;
                    const unsigned r = has ? src[j] : 0u;
                    const unsigned cat = catb + ((r >> kLocalBits) & 1u);
                    const unsigned fine = has ? (r >> 12) - key0 : 0u;
                    const unsigned bin = (fine << 2) | cat;
                    const unsigned pos = take_slot(atomic_order, has, bin, nb2, &hist[bin]);
                    if (has) {
                        const unsigned px = pxb + (r & (kTilePix - 1));
                        const unsigned yy = px / (unsigned)P.W;
                        const long long g = g0 + pos;
                        if (PACKED) {
                            store_packed_bytes(P.packed + g * 13, tbase + fine, (px - yy * P.W) & 0xFFFFu, yy & 0xFFFFu, cat >> 1);
                        } else {
                            P.ts[g] = tbase + fine;
                            P.x[g] = (short)(px - yy * P.W);
                            P.y[g] = (short)yy;
                            P.p[g] = (signed char)(cat >> 1);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// pooled slope parameters (LDATI.py:177-190): thread per (frame, polarity, pixel).  The counts of the
// k x k neighbourhood are recomputed from the voxels (zero padding outside the image), pooled --
// 'weighted': [[1,2,1],[2,4,2],[1,2,1]]/16; 'avg': sum / k^2 -- and turned into {k, b} per bin.
// Counts are integers and the weights powers of two over 16: every partial sum is exact in f32.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ldati_pool_slope_kernel(LdatiParams P, int pooling, int pool_k, float2 *kbb) {
    const int px = blockIdx.x * 256 + threadIdx.x, bp = blockIdx.y;
    if (px >= P.HW) return;
    const int h = px / P.W, w = px - h * P.W;
    const int r = pooling == V2CE_POOL_WEIGHTED ? 1 : pool_k / 2;
    const float *plane0 = P.vox + (long long)bp * 10 * P.HW;
    float acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.0f;
    for (int dh = -r; dh <= r; ++dh)
        for (int dw = -r; dw <= r; ++dw) {
            const int hh = h + dh, ww = w + dw;
            if (hh < 0 || hh >= P.H || ww < 0 || ww >= P.W) continue;
            float yv[10];
#pragma unroll
            for (int i = 0; i < 10; ++i) yv[i] = plane0[(long long)i * P.HW + hh * P.W + ww];
            int nn[9];
            float td[9];
            relocate_all(yv, P.bidir != 0, nn, td);
            const float wt = pooling == V2CE_POOL_WEIGHTED ? (float)((2 - (dh < 0 ? -dh : dh)) * (2 - (dw < 0 ? -dw : dw))) / 16.0f : 1.0f;
#pragma unroll
            for (int i = 0; i < 9; ++i) acc[i] += (float)nn[i] * wt;
        }
    if (pooling == V2CE_POOL_AVG) {
        const float div = (float)(pool_k * pool_k);
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[i] = acc[i] / div;
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const float fl = c == 0 ? acc[1] : acc[c - 1], fr = c == 8 ? acc[7] : acc[c + 1];
        const float sxy = fr - fl;
        const float k0 = (3.0f * sxy) / 6.0f;
        const float k = (k0 / P.VS2) / (acc[c] + 1e-8f);
        const float bb = P.INV - (P.VS * k) / 2.0f;
        kbb[((long long)bp * 9 + c) * P.HW + px] = make_float2(k, bb);
    }
}

// generic path: sorted 64-bit keys -> SoA events
__global__ __launch_bounds__(256) void ldati_keys_decode_kernel(LdatiParams P, const unsigned long long *keys, long long n,
                                                                long long *ts, short *x, short *y, signed char *pp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const int seg = (int)(k >> 44), b = seg / 9, c = seg - b * 9;
    const unsigned rel = (unsigned)(k >> 24) & 0xFFFFFu, cat = (unsigned)(k >> 22) & 3u, px = (unsigned)k & 0x3FFFFFu;
    const unsigned yy = px / (unsigned)P.W;
    ts[i] = P.kbase[c] + (long long)rel + (P.frame_ts_add ? P.frame_ts_add[b] : 0);
    x[i] = (short)(px - yy * P.W);
    y[i] = (short)yy;
    pp[i] = (signed char)(cat >> 1);
}

// ---------------------------------------------------------------------------------------------
// pack / unpack kernels: SoA <-> 13-byte records
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void events_pack_kernel(const long long *__restrict__ ts,
                                                          const short *__restrict__ x,
                                                          const short *__restrict__ y,
                                                          const signed char *__restrict__ p,
                                                          long long n, unsigned char *packed) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[256 * 13 + 12];
    const long long first = (long long)blockIdx.x * 256;
    const long long i = first + threadIdx.x;
    if (i < n)
        store_packed_bytes(stage + threadIdx.x * 13, ts[i], (unsigned short)x[i], (unsigned short)y[i],
                           (unsigned char)p[i]);
    __syncthreads();
    const long long remain = n - first;
    const int nev = remain < 256 ? (int)remain : 256;
    const int nbytes = nev * 13;
    unsigned char *dst = packed + first * 13;   // first*13 is a multiple of 4 (256*13 = 3328)
    const int nd = nbytes >> 2;
    for (int w = threadIdx.x; w < nd; w += 256)
        reinterpret_cast<unsigned *>(dst)[w] = reinterpret_cast<const unsigned *>(stage)[w];
    for (int r = (nd << 2) + threadIdx.x; r < nbytes; r += 256) dst[r] = stage[r];
}

__global__ __launch_bounds__(256) void events_unpack_kernel(const unsigned char *__restrict__ packed,
                                                            long long n, long long *ts, short *x,
                                                            short *y, signed char *p) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[256 * 13 + 12];
    const long long first = (long long)blockIdx.x * 256;
    const long long remain = n - first;
    const int nev = remain < 256 ? (int)remain : 256;
    const int nbytes = nev * 13;
    const unsigned char *src = packed + first * 13;
    const int nd = nbytes >> 2;
    for (int w = threadIdx.x; w < nd; w += 256)
        reinterpret_cast<unsigned *>(stage)[w] = reinterpret_cast<const unsigned *>(src)[w];
    for (int r = (nd << 2) + threadIdx.x; r < nbytes; r += 256) stage[r] = src[r];
    __syncthreads();
    const long long i = first + threadIdx.x;
    if (i < n) {
        const unsigned char *s = stage + threadIdx.x * 13;
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) t |= (unsigned long long)s[k] << (8 * k);
        ts[i] = (long long)t;
        x[i] = (short)(s[8] | (s[9] << 8));
        y[i] = (short)(s[10] | (s[11] << 8));
        p[i] = (signed char)s[12];
    }
}

// the few words a call needs zeroed before its first kernel (statistics, status words): one launch instead of the two to four
// fill kernels that hipMemsetAsync makes of two small, 8-byte-aligned ranges (~5 us each plus their gaps: 4 % of an e2e call)
// (not named ldati_*: the profile summaries tell a call's steady-state kernels from first-call-only ones by their launch counts, and this
// one runs twice per call)
__global__ void zero_words_kernel(unsigned *a, int na, unsigned *b, int nb) {
    const int i = threadIdx.x;
    if (i < na) a[i] = 0u;
    if (b && i < nb) b[i] = 0u;
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

namespace {
// a failed launch would leave stale status words that the host then trusts: reported
int zero_words(hipStream_t s, void *a, int na, void *b = nullptr, int nb = 0) {
    hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(64), 0, s, static_cast<unsigned *>(a), na, static_cast<unsigned *>(b), nb);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

int probe_lds_order(hipStream_t s) {   // once per device: check that LDS atomics return ranks in lane order (see g_lds_order_ok)
    static std::atomic<unsigned long long> probed{0};
    int dev = 0;
    V2CE_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(probed.fetch_or(bit) & bit))
        hipLaunchKernelGGL(ldati_lds_order_probe_kernel, dim3(64), dim3(256), 0, s, 200);
    return V2CE_OK;
}

// NULL options = the CLI's call (v2ce.py:356): 'slope', no pooling, forward relocation
int read_options(const v2ce_ldati_options *o, Opts &out, const char *who) {
    out = Opts{V2CE_STRATEGY_SLOPE, 0, V2CE_POOL_NONE, 3};
    if (!o) return V2CE_OK;
    out = Opts{o->strategy, o->bidirectional != 0, o->pooling_type, o->pooling_kernel_size};
    V2CE_REQUIRE(out.strategy == V2CE_STRATEGY_SLOPE || out.strategy == V2CE_STRATEGY_NONE || out.strategy == V2CE_STRATEGY_RANDOM,
                 V2CE_ERR_BAD_ARG, "%s: bad strategy %d", who, out.strategy);
    V2CE_REQUIRE(out.pooling == V2CE_POOL_NONE || out.pooling == V2CE_POOL_AVG || out.pooling == V2CE_POOL_WEIGHTED,
                 V2CE_ERR_BAD_ARG, "%s: bad pooling_type %d", who, out.pooling);
    V2CE_REQUIRE(out.pooling != V2CE_POOL_AVG || (out.pool_k >= 1 && out.pool_k <= 15 && (out.pool_k & 1)), V2CE_ERR_UNSUPPORTED,
                 "%s: pooling_kernel_size %d (odd sizes 1..15: nn.AvgPool2d with padding k//2 keeps H x W only for odd k)", who, out.pool_k);
    if (out.strategy != V2CE_STRATEGY_SLOPE) out.pooling = V2CE_POOL_NONE;      // pooling only shapes the slope (LDATI.py:175)
    return V2CE_OK;
}

// what the calls that compute timestamps say about time and the random draws
struct DrawArgs { double fps; int rng_mode; const float *uniforms; int replay_max_n; uint64_t seed; int64_t frame_base; };

// The argument checks count, count_fused and emit share.  frame_grid: the call launches a grid with one row per frame;
// d: null for the count, which computes no timestamp.
int check_call(const char *who, bool pointers, int B, int H, int W, bool frame_grid, const DrawArgs *d, const v2ce_ldati_options *options, Opts &o) {
    V2CE_REQUIRE(pointers, V2CE_ERR_BAD_ARG, "%s: null pointer", who);
    V2CE_REQUIRE(B > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 30), V2CE_ERR_BAD_ARG, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    V2CE_REQUIRE(W <= 32767 && H <= 32767, V2CE_ERR_UNSUPPORTED, "%s: x/y are int16 (LDATI.py:230-231)", who);
    V2CE_REQUIRE(!frame_grid || B <= 65535, V2CE_ERR_UNSUPPORTED, "%s: B too large for one launch", who);
    if (d) {
        V2CE_REQUIRE(d->fps > 0, V2CE_ERR_BAD_ARG, "%s: fps must be positive", who);
        V2CE_REQUIRE(d->rng_mode == V2CE_RNG_REPLAY || d->rng_mode == V2CE_RNG_PHILOX, V2CE_ERR_BAD_ARG, "%s: bad rng_mode %d", who, d->rng_mode);
        V2CE_REQUIRE(d->rng_mode != V2CE_RNG_REPLAY || d->replay_max_n == 0 || d->uniforms != nullptr, V2CE_ERR_BAD_ARG, "%s: REPLAY mode needs the uniform tensor", who);
    }
    return read_options(options, o, who);
}

// the workspace of a call; the temporary size of the generic path's library radix sort is this file's to ask for
TwoLevelWs workspace_of(const Plan &pl, const Opts &o, int B, int H, int W, int64_t total, bool packed_out) {
    size_t tb = 0;
    if (o.strategy == V2CE_STRATEGY_RANDOM && total > 0)
        (void)rocprim::radix_sort_keys(nullptr, tb, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (size_t)total, 0, 60);
    return two_level_ws(pl, o, B, H, W, total, packed_out, tb);
}

template <typename T>   // base + byte offset (the offsets of TileWs, TwoLevelWs, FusedLayout)
T *at(const void *base, size_t offset) { return reinterpret_cast<T *>(static_cast<unsigned char *>(const_cast<void *>(base)) + offset); }
void set_geometry(LdatiParams &P, const Plan &pl) {
    P.shift = pl.shift; P.NB = pl.NB; P.nb1 = pl.nb1; P.T = pl.T; P.Tp = pl.Tp; P.tpp = pl.tpp; P.PB = pl.PB;
}

// once per device and FPS: the exhaustive check of k0_time_fast against the IEEE divisions (see g_fastdiv) and the table of slope parameters
// (g_slope_tab), enqueued in front of the first call that uses them.  Seven slots per device (slot 7: v2ce_ldati_selfcheck's scratch); -1 = none left
int fastdiv_slot(const HostScalars &h, const LdatiParams &P, hipStream_t st, int &slot) {
    static std::mutex mu;
    static unsigned seen[64][8];
    static int n_seen[64];
    slot = -1;
    int dev = 0;
    V2CE_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return V2CE_OK;
    unsigned bits;
    memcpy(&bits, &h.FPS, 4);
    std::lock_guard<std::mutex> g(mu);
    for (int i = 0; i < n_seen[dev]; ++i)
        if (seen[dev][i] == bits) slot = i;
    if (slot < 0 && n_seen[dev] < 7) {
        slot = n_seen[dev]++;
        seen[dev][slot] = bits;
        hipLaunchKernelGGL(ldati_fastdiv_check_kernel, dim3(65536), dim3(256), 0, st, h.FPS, P.RFPS, P.R9, slot);
        hipLaunchKernelGGL(ldati_fast64_check_kernel, dim3((0x3F800000u + kFast64Neg + 255u) / 256u), dim3(256), 0, st, P.fps, P.RFPS64, P.R9_64, slot);
        hipLaunchKernelGGL(ldati_slope_tab_kernel, dim3((kSlopeTab + 255) / 256), dim3(256), 0, st, h.VS, h.VS2, h.INV, slot);
        hipLaunchKernelGGL(ldati_fastdiv_commit_kernel, dim3(1), dim3(1), 0, st, h.FPS, slot);
    }
    return V2CE_OK;
}

int fill_params(LdatiParams &P, const HostScalars &h, const Opts &o, const Knobs &k, const float *vox, int B, int H, int W, const DrawArgs &d, hipStream_t st) {
    P.vox = vox; P.B = B; P.H = H; P.W = W; P.HW = H * W;
    P.fps = d.fps; P.VS = h.VS; P.VS2 = h.VS2; P.INV = h.INV; P.FPS = h.FPS;
    for (int c = 0; c < 9; ++c) { P.offt[c] = h.offt[c]; P.kbase[c] = h.kbase[c]; }
    P.NK = (int)h.NK; P.nbits = h.nbits;
    P.ts32 = (fabs((double)h.offt[8]) + 1.0 + 1.0 / d.fps) * 1e6 < 2.0e9 ? 1 : 0;
    P.strategy = o.strategy; P.bidir = o.bidir;
    P.rng_mode = d.rng_mode; P.uniforms = d.uniforms; P.replay_max_n = d.replay_max_n;
    P.seed = d.seed; P.frame_base = d.frame_base;
    P.sweep_ok = h.sweep_ok ? 1 : 0;
    P.RFPS = (float)(1.0 / (double)h.FPS); P.R9 = (float)(1.0 / 9.0);
    P.RFPS64 = 1.0 / d.fps; P.R9_64 = 1.0 / 9.0;
    P.fast_slot = -1;
    if (o.strategy == V2CE_STRATEGY_SLOPE && !k.no_fastdiv)
        if (int rc = fastdiv_slot(h, P, st, P.fast_slot)) return rc;
    P.ballot_ranks = k.ballot_ranks ? 1 : 0;
    return V2CE_OK;
}

CallFacts facts_of(const LdatiParams &P, const Opts &o, bool packed) { return CallFacts{o.pooling != V2CE_POOL_NONE, P.ts32 != 0, P.fast_slot >= 0, packed}; }

// the tile pass of a call: the dense kernel, or the per-bin kernel for everything the dense one does not serve (choose_path)
int launch_tile_pass(const LdatiParams &P, const Plan &pl, const PathChoice &c, hipStream_t st) {
    if (c.dense_nw) {
        auto dk = c.dense_nw == 8 ? ldati_tile_dense_kernel<8> : ldati_tile_dense_kernel<16>;
        V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(dk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.dense_lds));
        hipLaunchKernelGGL(dk, dim3(pl.T, P.B), dim3(64 * c.dense_nw), c.dense_lds, st, P);
        return V2CE_OK;
    }
    auto tile_kernel = c.bidir ? (c.tile_threads == 512 ? ldati_tile_pass_kernel<512, 4, true> : ldati_tile_pass_kernel<1024, 2, true>)
                               : (c.tile_threads == 512 ? ldati_tile_pass_kernel<512, 4, false> : ldati_tile_pass_kernel<1024, 2, false>);
    V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_tile));
    hipLaunchKernelGGL(tile_kernel, dim3(pl.T, P.B), dim3(c.tile_threads), pl.lds_tile, st, P);
    return V2CE_OK;
}

template <bool FUSED>   // FUSED: v2ce_ldati_count_fused's form (counts the tiles as well, every tile's records into its own slot)
int launch_sparse_pass(const LdatiParams &P, const Plan &pl, const PathChoice &c, hipStream_t st) {
    auto sparse_kernel = c.bidir ? ldati_tile_sparse_kernel<FUSED, true> : ldati_tile_sparse_kernel<FUSED, false>;
    V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(sparse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSparseLds));
    hipLaunchKernelGGL(sparse_kernel, dim3(pl.T, P.B), dim3(kSparseThreads), kSparseLds, st, P);
    return V2CE_OK;
}

template <bool PACKED>
auto sort_kernel_of(const PathChoice &c) -> void (*)(LdatiParams) {
    if (c.sort_k == 8) return ldati_bucket_sort_kernel<PACKED, 8, 256>;
    return c.sort_threads == 64 ? ldati_bucket_sort_kernel<PACKED, 24, 64>
                                : c.sort_threads == 128 ? ldati_bucket_sort_kernel<PACKED, 24, 128> : ldati_bucket_sort_kernel<PACKED, 24, 256>;
}

// tile counts -> per-tile offsets, segment offsets and the statistics: the tail of both count calls
int launch_count_scans(const TileWs &tw, void *tile_ws, int B, int64_t *seg_offsets, int64_t *stats, hipStream_t s) {
    hipLaunchKernelGGL(ldati_tile_scan_kernel, dim3((B + 3) / 4), dim3(256), 0, s, at<unsigned>(tile_ws, tw.tc), B, (int)tw.T, at<unsigned>(tile_ws, tw.tile_off),
                       at<unsigned>(tile_ws, tw.tile_src), (int)tw.Tp, reinterpret_cast<long long *>(seg_offsets), reinterpret_cast<unsigned long long *>(stats));
    hipLaunchKernelGGL(ldati_seg_scan_kernel, dim3(1), dim3(256), 0, s, B * 9, reinterpret_cast<long long *>(seg_offsets), reinterpret_cast<unsigned long long *>(stats));
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
}  // namespace

extern "C" size_t v2ce_ldati_tile_ws_bytes(int B, int H, int W) { return B <= 0 || H <= 0 || W <= 0 ? 0 : tile_ws(B, H, W).bytes; }
extern "C" int v2ce_ldati_count(const float *vox, int B, int H, int W, const v2ce_ldati_options *options, void *tile_ws_dev,
                                size_t tile_ws_bytes, int64_t *seg_offsets, int64_t *stats, v2ce_stream_t stream) {
    clear_error();
    Opts o;
    if (int rc = check_call("v2ce_ldati_count", vox && tile_ws_dev && seg_offsets && stats, B, H, W, true, nullptr, options, o)) return rc;
    const TileWs tw = tile_ws(B, H, W);
    V2CE_REQUIRE(tile_ws_bytes >= tw.bytes, V2CE_ERR_WORKSPACE, "v2ce_ldati_count: tile workspace %zu < %zu", tile_ws_bytes, tw.bytes);
    hipStream_t s = as_stream(stream);
    if (int rc = probe_lds_order(s)) return rc;
    if (int rc = zero_words(s, stats, 8)) return rc;
    // 'random' emits like 'slope' (every draw of a multi-event voxel); 'none' only the singles
    const int count_strategy = o.strategy == V2CE_STRATEGY_NONE ? V2CE_STRATEGY_NONE : V2CE_STRATEGY_SLOPE;
    hipLaunchKernelGGL(ldati_count_tiles_kernel, dim3((unsigned)tw.T, B), dim3(kCountThreads), 0, s, vox, H * W, (int)tw.tpp, count_strategy, o.bidir, at<unsigned>(tile_ws_dev, tw.tc),
                       reinterpret_cast<unsigned long long *>(stats));
    return launch_count_scans(tw, tile_ws_dev, B, seg_offsets, stats, s);
}

extern "C" size_t v2ce_ldati_lds_bytes(double fps, double t0) {
    if (!(fps > 0)) return 0;
    const HostScalars h = host_scalars(fps, t0);
    return h.sweep_ok ? h.lds_bytes : 0;
}

extern "C" size_t v2ce_ldati_workspace_bytes(int B, int H, int W, double fps, double t0, const v2ce_ldati_options *options,
                                             int64_t total_events, int64_t max_segment_events, int64_t max_tile_events, int packed_output) {
    if (!(fps > 0) || B <= 0 || H <= 0 || W <= 0) return 0;
    Opts o;
    if (read_options(options, o, "v2ce_ldati_workspace_bytes")) return 0;
    const HostScalars h = host_scalars(fps, t0, o.bidir, o.strategy == V2CE_STRATEGY_RANDOM);
    const Plan pl = make_plan(h, read_knobs(), B, H, W, total_events, max_segment_events, max_tile_events);
    const TwoLevelWs w = workspace_of(pl, o, B, H, W, total_events, packed_output != 0);
    return w.ok ? w.bytes : 0;
}

extern "C" size_t v2ce_ldati_fused_ws_bytes(int B, int H, int W, double fps, double t0, const v2ce_ldati_options *options,
                                            int64_t expected_max_segment_events, int64_t expected_max_tile_bin_events) {
    if (!(fps > 0) || B <= 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 30)) return 0;
    Opts o;
    if (read_options(options, o, "v2ce_ldati_fused_ws_bytes")) return 0;
    const HostScalars h = host_scalars(fps, t0, o.bidir, o.strategy == V2CE_STRATEGY_RANDOM);
    const FusedLayout F = make_fused_layout(h, o, read_knobs(), B, H, W, expected_max_segment_events, expected_max_tile_bin_events);
    return F.ok ? F.bytes : 0;
}

extern "C" int v2ce_ldati_count_fused(const float *vox, int B, int H, int W, double fps, double t0,
                                      const v2ce_ldati_options *options, int rng_mode, const float *uniforms, int replay_max_n,
                                      uint64_t seed, int64_t frame_base, int64_t expected_max_segment_events, int64_t expected_max_tile_bin_events,
                                      void *tile_ws_dev, size_t tile_ws_bytes, void *fused_ws, size_t fused_ws_bytes, int64_t *seg_offsets, int64_t *stats,
                                      v2ce_stream_t stream) {
    clear_error();
    const char *who = "v2ce_ldati_count_fused";
    const DrawArgs d{fps, rng_mode, uniforms, replay_max_n, seed, frame_base};
    Opts o;
    if (int rc = check_call(who, vox && tile_ws_dev && fused_ws && seg_offsets && stats, B, H, W, true, &d, options, o)) return rc;
    const Knobs k = read_knobs();
    const HostScalars h = host_scalars(fps, t0, o.bidir, false);
    const FusedLayout F = make_fused_layout(h, o, k, B, H, W, expected_max_segment_events, expected_max_tile_bin_events);
    const TileWs tw = tile_ws(B, H, W);
    V2CE_REQUIRE(F.ok, V2CE_ERR_UNSUPPORTED, "%s: these arguments have no fused path (v2ce_ldati_fused_ws_bytes = 0)", who);
    V2CE_REQUIRE(tile_ws_bytes >= tw.bytes, V2CE_ERR_WORKSPACE, "%s: tile workspace %zu < %zu", who, tile_ws_bytes, tw.bytes);
    V2CE_REQUIRE(fused_ws_bytes >= F.bytes, V2CE_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, fused_ws_bytes, F.bytes);
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(fused_ws) & 15) == 0, V2CE_ERR_BAD_ARG, "%s: workspace must be 16-byte aligned", who);
    hipStream_t s = as_stream(stream);
    const Plan &pl = F.p0;
    if (int rc = probe_lds_order(s)) return rc;
    if (int rc = zero_words(s, stats, 16, fused_ws, 4)) return rc;
    LdatiParams P{};
    if (int rc = fill_params(P, h, o, k, vox, B, H, W, d, s)) return rc;
    set_geometry(P, pl);
    const PathChoice c = choose_path(o, pl, k, facts_of(P, o, false));
    P.sparse_cap = kSparseCap;
    P.tc_w = at<unsigned>(tile_ws_dev, tw.tc); P.stats_w = reinterpret_cast<unsigned long long *>(stats);
    P.status = at<int>(fused_ws, 0); P.tile_abs_w = at<unsigned>(fused_ws, F.off_abs);
    P.temp = at<unsigned>(fused_ws, F.off_rec); P.roff = at<unsigned short>(fused_ws, F.off_roff);
    if (F.slot_cap && c.dense_nw) {
        // dense regime: ldati_tile_dense_kernel is the count pass and the tile pass at once (slot mode)
        P.sparse_cap = 0; P.slot_cap = F.slot_cap; P.capA = pl.capA;
        if (int rc = launch_tile_pass(P, pl, c, s)) return rc;
    } else if (F.slot_cap) {
        // (a call the dense kernel does not serve -- more than seven fps values on this device, 64-bit times: the plain count
        // pass, so that the emit phase finds valid counts and takes the two-pass path)
        hipLaunchKernelGGL(ldati_count_tiles_kernel, dim3(pl.T, B), dim3(kCountThreads), 0, s, vox, H * W, pl.tpp, o.strategy, o.bidir, P.tc_w, P.stats_w);
    } else if (int rc = launch_sparse_pass<true>(P, pl, c, s)) {
        return rc;
    }
    return launch_count_scans(tw, tile_ws_dev, B, seg_offsets, stats, s);
}

namespace {
// the arguments of v2ce_ldati_emit / v2ce_ldati_emit_fused, in the order of their parameter lists
struct EmitArgs {
    const float *vox; int B, H, W; double fps, t0; const v2ce_ldati_options *options;
    DrawArgs draw;
    const int64_t *seg_offsets, *frame_ts_add; int64_t *ts; int16_t *x, *y; int8_t *p; uint8_t *packed;
    int64_t total_events, max_segment_events, max_tile_events; const void *tile_ws; void *workspace; size_t workspace_bytes;
    const void *fused_ws; size_t fused_ws_bytes; int64_t fused_tile_max, fused_seg_hint, fused_tile_bin_hint;   // emit_fused only
    v2ce_stream_t stream;
};

// segment-sweep kernel (workspace = NULL): one workgroup per segment, every segment; what the two-level path is tested against
int emit_sweep(const EmitArgs &a, const HostScalars &h, const Opts &o, const LdatiParams &P, hipStream_t st) {
    V2CE_REQUIRE(h.sweep_ok && o.pooling == V2CE_POOL_NONE, V2CE_ERR_UNSUPPORTED, "v2ce_ldati_emit: the sweep kernel (workspace = NULL) covers forward relocation "
                 "without pooling at key ranges <= 9600 (fps=%g t0=%g needs %lld keys per bin): pass a workspace", a.fps, a.t0, h.NK);
    V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(ldati_emit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h.lds_bytes));
    hipLaunchKernelGGL(ldati_emit_kernel, dim3(a.B * 9), dim3(256), h.lds_bytes, st, P);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

// generic path ('random': timestamps spread over a second): tile pass in key mode, one library radix sort of the 60-bit keys, decode (+ pack)
int emit_generic(const EmitArgs &a, LdatiParams &P, const Plan &pl, const PathChoice &c, const TwoLevelWs &w, hipStream_t st) {
    const size_t n = (size_t)a.total_events;
    unsigned long long *kA = at<unsigned long long>(a.workspace, w.keys), *kB = at<unsigned long long>(a.workspace, w.keys_alt);
    P.keys = kA;
    if (int rc = launch_tile_pass(P, pl, c, st)) return rc;
    if (n > 0) {
        size_t tb = w.soa - w.sort_temp;
        V2CE_HIP_CHECK(rocprim::radix_sort_keys(at<unsigned char>(a.workspace, w.sort_temp), tb, kA, kB, n, 0, 60, st));
        // packed output: decode into the SoA arrays of the workspace, then pack
        long long *ts2 = a.packed ? at<long long>(a.workspace, w.soa) : P.ts;
        short *x2 = a.packed ? at<short>(a.workspace, w.soa + 8 * n) : P.x, *y2 = a.packed ? x2 + n : P.y;
        signed char *p2 = a.packed ? reinterpret_cast<signed char *>(y2 + n) : P.p;
        const unsigned blocks = (unsigned)((a.total_events + 255) / 256);
        hipLaunchKernelGGL(ldati_keys_decode_kernel, dim3(blocks), dim3(256), 0, st, P, kB, (long long)n, ts2, x2, y2, p2);
        if (a.packed) hipLaunchKernelGGL(events_pack_kernel, dim3(blocks), dim3(256), 0, st, ts2, x2, y2, p2, (long long)n, a.packed);
    }
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

// two-level path: [sparse tile kernel, tile pass -- unless the fused count left their records] -> bucket scan -> bucket sort -> big buckets
int emit_two_level(const EmitArgs &a, const HostScalars &h, const Opts &o, const Knobs &k, LdatiParams &P, const Plan &pl, const PathChoice &c, const TwoLevelWs &w, hipStream_t st) {
    P.bofs = at<unsigned>(a.workspace, w.bofs); P.groups = at<unsigned>(a.workspace, w.groups);
    P.big_list = at<unsigned>(a.workspace, w.big_list); P.ngroups = at<unsigned>(a.workspace, w.ngroups);
    P.seg_flag = at<int>(a.workspace, w.seg_flag); P.nbig = at<unsigned>(a.workspace, w.status + 4);
    P.temp = at<unsigned>(a.workspace, w.temp); P.roff = at<unsigned short>(a.workspace, w.roff);
    P.gruns = at<unsigned>(a.workspace, w.gruns);
    // the fused count already ran the tile pass: usable when the call has a fused path at all (F.ok), its assumed geometry is the plan's and every tile fitted
    bool fused = false;
    if (a.fused_ws) {
        const FusedLayout F = make_fused_layout(h, o, k, a.B, a.H, a.W, a.fused_seg_hint, a.fused_tile_bin_hint);
        // sparse form: every tile fitted its slot; dense form: the dense kernel ran (count_fused's own test) and every (tile, bin) run fitted
        fused = F.ok && a.fused_ws_bytes >= F.bytes && F.p0.shift == pl.shift && F.p0.NB == pl.NB && F.p0.T == pl.T &&
                (F.slot_cap ? choose_path(o, F.p0, k, facts_of(P, o, false)).dense_nw && a.max_tile_events <= F.slot_cap : a.fused_tile_max <= kSparseCap);
        if (k.debug) {
            fprintf(stderr, "v2ce_ldati_emit_fused: fused=%d ok=%d bytes %zu/%zu tile_max=%lld shift %d/%d NB %d/%d T %d/%d max_segment %lld sort threads %d cap2 %d\n", (int)fused,
                    (int)F.ok, a.fused_ws_bytes, F.bytes, (long long)a.fused_tile_max, F.p0.shift, pl.shift, F.p0.NB, pl.NB, F.p0.T, pl.T, (long long)a.max_segment_events, pl.sort_threads, pl.cap2);
            if (F.slot_cap) fprintf(stderr, "   dense slots of %d records, largest (tile, bin) %lld\n", F.slot_cap, (long long)a.max_tile_events);
        }
        if (fused) {
            P.fused_status = at<const int>(a.fused_ws, 0);
            P.tile_src = P.tile_abs = at<const unsigned>(a.fused_ws, F.off_abs);
            P.temp = at<unsigned>(a.fused_ws, F.off_rec); P.roff = at<unsigned short>(a.fused_ws, F.off_roff);
        }
    }
    // (Tried in round 3 and removed: walking the frames in groups so that the HBM-bound bucket sort of group g runs on a
    // low-priority side stream under the VALU-bound tile pass of group g + 1.  24 stress frame-pairs: 1 group 1.74 ms,
    // 2 groups 1.86, 4 groups 1.83, 8 groups 2.21 -- the tile pass needs whole CUs (1024 threads, ~100 KB of LDS), the sort
    // workgroups that slip in between delay its rounds, and each group adds a partial last round.)
    if (!fused) {
        if (c.sparse_cap)
            if (int rc = launch_sparse_pass<false>(P, pl, c, st)) return rc;
        if (int rc = launch_tile_pass(P, pl, c, st)) return rc;
    }
    hipLaunchKernelGGL(ldati_bucket_scan_kernel, dim3(a.B * 9), dim3(512), 0, st, P);
    auto sort_kernel = c.sort_packed ? sort_kernel_of<true>(c) : sort_kernel_of<false>(c);
    V2CE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_sort));
    hipLaunchKernelGGL(sort_kernel, dim3(pl.NB, a.B * 9), dim3(c.sort_threads), pl.lds_sort, st, P);
    hipLaunchKernelGGL(c.sort_packed ? ldati_big_bucket_kernel<true> : ldati_big_bucket_kernel<false>, dim3(256), dim3(256), 0, st, P);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

int emit(const EmitArgs &a) {
    clear_error();
    const char *who = "v2ce_ldati_emit";
    Opts o;
    if (int rc = check_call(who, a.vox && a.seg_offsets, a.B, a.H, a.W, false, &a.draw, a.options, o)) return rc;
    const bool soa = a.ts && a.x && a.y && a.p;
    V2CE_REQUIRE(soa != (a.packed != nullptr) && (soa || !(a.ts || a.x || a.y || a.p)), V2CE_ERR_BAD_ARG, "%s: give either the four SoA arrays or the packed buffer", who);
    V2CE_REQUIRE(!a.packed || (reinterpret_cast<uintptr_t>(a.packed) & 3) == 0, V2CE_ERR_BAD_ARG, "%s: packed must be 4-byte aligned", who);
    const HostScalars h = host_scalars(a.fps, a.t0, o.bidir, o.strategy == V2CE_STRATEGY_RANDOM);
    V2CE_REQUIRE(h.ok, V2CE_ERR_UNSUPPORTED, "%s: fps=%g t0=%g needs %lld keys per bin (max %d)", who, a.fps, a.t0, h.NK, kMaxNB << kMaxShift);
    const Knobs k = read_knobs();
    LdatiParams P{};
    hipStream_t st = as_stream(a.stream);
    if (int rc = fill_params(P, h, o, k, a.vox, a.B, a.H, a.W, a.draw, st)) return rc;
    P.seg_offsets = reinterpret_cast<const long long *>(a.seg_offsets); P.frame_ts_add = reinterpret_cast<const long long *>(a.frame_ts_add);
    P.ts = reinterpret_cast<long long *>(a.ts); P.x = a.x; P.y = a.y; P.p = reinterpret_cast<signed char *>(a.p);
    P.packed = a.packed;
    if (!a.workspace) return emit_sweep(a, h, o, P, st);
    V2CE_REQUIRE(a.tile_ws, V2CE_ERR_BAD_ARG, "%s: the two-level path needs v2ce_ldati_count's tile workspace", who);
    V2CE_REQUIRE(a.total_events >= 0 && a.max_segment_events >= 0 && a.max_tile_events >= 0, V2CE_ERR_BAD_ARG, "%s: bad event counts", who);
    const Plan pl = make_plan(h, k, a.B, a.H, a.W, a.total_events, a.max_segment_events, a.max_tile_events);
    const TwoLevelWs w = workspace_of(pl, o, a.B, a.H, a.W, a.total_events, a.packed != nullptr);
    V2CE_REQUIRE(w.ok, V2CE_ERR_UNSUPPORTED, "%s: shape / density outside the two-level path (tiles %d, buckets %d, largest tile-bin %lld events); pass workspace = NULL",
                 who, pl.T, pl.NB, (long long)a.max_tile_events);
    V2CE_REQUIRE(a.workspace_bytes >= w.bytes, V2CE_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, a.workspace_bytes, w.bytes);
    const TileWs tw = tile_ws(a.B, a.H, a.W);
    const PathChoice c = choose_path(o, pl, k, facts_of(P, o, a.packed != nullptr));
    set_geometry(P, pl);
    P.capA = pl.capA; P.cap2 = pl.cap2; P.tbits = pl.tbits; P.span = pl.span;
    P.tc = at<const unsigned>(a.tile_ws, tw.tc); P.tile_off = at<const unsigned>(a.tile_ws, tw.tile_off); P.tile_src = at<const unsigned>(a.tile_ws, tw.tile_src);
    P.sparse_cap = c.sparse_cap; P.hist_bins = c.hist_bins;
    if (w.bytes > w.kbb) {
        // pooled slope parameters first (LDATI.py:177-190)
        float2 *kbb = at<float2>(a.workspace, w.kbb);
        hipLaunchKernelGGL(ldati_pool_slope_kernel, dim3((P.HW + 255) / 256, 2 * a.B), dim3(256), 0, st, P, o.pooling, o.pool_k, kbb);
        P.kbb = kbb;
    }
    P.status = at<int>(a.workspace, w.status);
    if (int rc = zero_words(st, P.status, 4)) return rc;
    return c.generic ? emit_generic(a, P, pl, c, w, st) : emit_two_level(a, h, o, k, P, pl, c, w, st);
}
}  // namespace

extern "C" int v2ce_ldati_emit(const float *vox, int B, int H, int W, double fps, double t0, const v2ce_ldati_options *options, int rng_mode,
                               const float *uniforms, int replay_max_n, uint64_t seed, int64_t frame_base, const int64_t *seg_offsets,
                               const int64_t *frame_ts_add, int64_t *ts, int16_t *x, int16_t *y, int8_t *p, uint8_t *packed, int64_t total_events,
                               int64_t max_segment_events, int64_t max_tile_events, const void *tile_ws, void *workspace, size_t workspace_bytes,
                               v2ce_stream_t stream) {
    return emit(EmitArgs{vox, B, H, W, fps, t0, options, DrawArgs{fps, rng_mode, uniforms, replay_max_n, seed, frame_base}, seg_offsets, frame_ts_add, ts, x, y, p,
                         packed, total_events, max_segment_events, max_tile_events, tile_ws, workspace, workspace_bytes, nullptr, 0, 0, 0, 0, stream});
}

extern "C" int v2ce_ldati_emit_fused(const float *vox, int B, int H, int W, double fps, double t0, const v2ce_ldati_options *options, int rng_mode,
                                     const float *uniforms, int replay_max_n, uint64_t seed, int64_t frame_base, const int64_t *seg_offsets,
                                     const int64_t *frame_ts_add, int64_t *ts, int16_t *x, int16_t *y, int8_t *p, uint8_t *packed, int64_t total_events,
                                     int64_t max_segment_events, int64_t max_tile_events, const void *tile_ws, void *workspace, size_t workspace_bytes,
                                     const void *fused_ws, size_t fused_ws_bytes, int64_t largest_tile_events, int64_t expected_max_segment_events,
                                     int64_t expected_max_tile_bin_events, v2ce_stream_t stream) {
    return emit(EmitArgs{vox, B, H, W, fps, t0, options, DrawArgs{fps, rng_mode, uniforms, replay_max_n, seed, frame_base}, seg_offsets, frame_ts_add, ts, x, y, p,
                         packed, total_events, max_segment_events, max_tile_events, tile_ws, workspace, workspace_bytes, fused_ws, fused_ws_bytes,
                         largest_tile_events, expected_max_segment_events, expected_max_tile_bin_events, stream});
}

extern "C" int v2ce_ldati_plan_info(int B, int H, int W, double fps, double t0, const v2ce_ldati_options *options,
                                    int64_t total_events, int64_t max_segment_events, int64_t max_tile_events, int64_t *info) {
    clear_error();
    V2CE_REQUIRE(info && fps > 0 && B > 0 && H > 0 && W > 0, V2CE_ERR_BAD_ARG, "v2ce_ldati_plan_info: bad argument");
    Opts o;
    if (int rc = read_options(options, o, "v2ce_ldati_plan_info")) return rc;
    const HostScalars h = host_scalars(fps, t0, o.bidir, o.strategy == V2CE_STRATEGY_RANDOM);
    const Plan pl = make_plan(h, read_knobs(), B, H, W, total_events, max_segment_events, max_tile_events);
    // (workspace layout: TwoLevelWs, ldati_plan.h)
    const int64_t v[10] = {pl.ok, pl.shift, pl.NB, pl.T, pl.capA, pl.cap2, (int64_t)pl.n_tab, (int64_t)pl.n_bkt, (int64_t)pl.lds_tile, (int64_t)pl.lds_sort};
    for (int i = 0; i < 10; ++i) info[i] = v[i];
    return V2CE_OK;
}

extern "C" int v2ce_ldati_status(const void *workspace, int B, int H, int W, double fps, double t0, const v2ce_ldati_options *options,
                                 int64_t total_events, int64_t max_segment_events, int64_t max_tile_events, const int32_t **status_dev) {
    clear_error();
    V2CE_REQUIRE(workspace && status_dev, V2CE_ERR_BAD_ARG, "v2ce_ldati_status: null pointer");
    Opts o;
    if (int rc = read_options(options, o, "v2ce_ldati_status")) return rc;
    const HostScalars h = host_scalars(fps, t0, o.bidir, o.strategy == V2CE_STRATEGY_RANDOM);
    const Plan pl = make_plan(h, read_knobs(), B, H, W, total_events, max_segment_events, max_tile_events);
    const TwoLevelWs w = two_level_ws(pl, o, B, H, W, total_events, false, 0);   // (the status word sits in front of everything these two size)
    V2CE_REQUIRE(w.generic || pl.ok, V2CE_ERR_UNSUPPORTED, "v2ce_ldati_status: no two-level plan for these arguments");
    *status_dev = at<const int32_t>(workspace, w.status);
    return V2CE_OK;
}

extern "C" int v2ce_ldati_rank_mode(int32_t *mode) {
    clear_error();
    V2CE_REQUIRE(mode, V2CE_ERR_BAD_ARG, "v2ce_ldati_rank_mode: null pointer");
    int ok = 0;
    V2CE_HIP_CHECK(hipMemcpyFromSymbol(&ok, HIP_SYMBOL(g_lds_order_ok), sizeof(int)));
    *mode = (ok && !read_knobs().ballot_ranks) ? 1 : 0;
    return V2CE_OK;
}

extern "C" int v2ce_ldati_selfcheck(double fps, int64_t *mismatches) {
    clear_error();
    V2CE_REQUIRE(mismatches && fps > 0, V2CE_ERR_BAD_ARG, "v2ce_ldati_selfcheck: bad argument");
    const HostScalars h = host_scalars(fps, 0.0);
    unsigned long long *bad = nullptr;
    V2CE_HIP_CHECK(hipMalloc(&bad, 2 * sizeof(unsigned long long)));
    V2CE_HIP_CHECK(hipMemset(bad, 0, 2 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(ldati_selfcheck_kernel, dim3(65536, 2 * kSlopeM + 1), dim3(256), 0, nullptr, h.VS, h.VS2, h.INV, -kSlopeM, bad);
    unsigned long long host[2] = {0, 0};
    const hipError_t e = hipMemcpy(host, bad, sizeof(host), hipMemcpyDeviceToHost);
    (void)hipFree(bad);
    V2CE_HIP_CHECK(e);
    mismatches[0] = (int64_t)host[0];
    mismatches[1] = (int64_t)host[1];
    // the single-event time's fast form (single_time_fast): the product's own one-time check, run here in a spare slot
    const unsigned zero = 0;
    V2CE_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_fast64_bad), &zero, sizeof(unsigned), 7 * sizeof(unsigned)));
    hipLaunchKernelGGL(ldati_fast64_check_kernel, dim3((0x3F800000u + kFast64Neg + 255u) / 256u), dim3(256), 0, nullptr, fps, 1.0 / fps, 1.0 / 9.0, 7);
    unsigned bad64 = 0;
    V2CE_HIP_CHECK(hipMemcpyFromSymbol(&bad64, HIP_SYMBOL(g_fast64_bad), sizeof(unsigned), 7 * sizeof(unsigned)));
    mismatches[2] = (int64_t)bad64;
    return V2CE_OK;
}

#ifdef V2CE_STAMP
extern "C" int v2ce_debug_stamps(unsigned long long *out32_host) {
    unsigned long long zero[32] = {0};
    if (hipMemcpyFromSymbol(out32_host, HIP_SYMBOL(g_stamp), sizeof(zero)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#endif

extern "C" int v2ce_events_pack(const int64_t *ts, const int16_t *x, const int16_t *y,
                                const int8_t *p, int64_t n, uint8_t *packed, v2ce_stream_t stream) {
    clear_error();
    V2CE_REQUIRE(n >= 0, V2CE_ERR_BAD_ARG, "v2ce_events_pack: negative n");
    if (n == 0) return V2CE_OK;
    V2CE_REQUIRE(ts && x && y && p && packed, V2CE_ERR_BAD_ARG, "v2ce_events_pack: null pointer");
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 3) == 0, V2CE_ERR_BAD_ARG,
                 "v2ce_events_pack: packed must be 4-byte aligned");
    const long long blocks = (n + 255) / 256;
    V2CE_REQUIRE(blocks < (1ll << 31), V2CE_ERR_UNSUPPORTED, "v2ce_events_pack: too many events");
    hipLaunchKernelGGL(events_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const long long *>(ts), x, y,
                       reinterpret_cast<const signed char *>(p), (long long)n, packed);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}

extern "C" int v2ce_events_unpack(const uint8_t *packed, int64_t n, int64_t *ts, int16_t *x, int16_t *y,
                                  int8_t *p, v2ce_stream_t stream) {
    clear_error();
    V2CE_REQUIRE(n >= 0, V2CE_ERR_BAD_ARG, "v2ce_events_unpack: negative n");
    if (n == 0) return V2CE_OK;
    V2CE_REQUIRE(ts && x && y && p && packed, V2CE_ERR_BAD_ARG, "v2ce_events_unpack: null pointer");
    V2CE_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 3) == 0, V2CE_ERR_BAD_ARG,
                 "v2ce_events_unpack: packed must be 4-byte aligned");
    const long long blocks = (n + 255) / 256;
    V2CE_REQUIRE(blocks < (1ll << 31), V2CE_ERR_UNSUPPORTED, "v2ce_events_unpack: too many events");
    hipLaunchKernelGGL(events_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), packed,
                       (long long)n, reinterpret_cast<long long *>(ts), x, y, reinterpret_cast<signed char *>(p));
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
