// ldati_dev.h -- what LDATI's kernels (ldati.hip) share: the constants (ldati_const.h, which the host-only planning of ldati_plan.h
// reads as well), the kernel argument block LdatiParams, the device helpers and __device__ globals, and the STAMP macros of the
// -DV2CE_STAMP diagnostic build.  Included by ldati.hip only, the one LDATI translation unit: the globals must exist once.
#pragma once

#include "common.h"
#include "ldati_const.h"

namespace v2ce {
namespace {

struct LdatiParams {
    const float *vox;
    int B, H, W, HW;
    // scalars of LDATI.py:145-146 cast the way CPU torch casts python scalars
    double fps;        // python number used in the f64 single-event path
    float VS, VS2, INV, FPS;
    float RFPS, R9;    // f32(1 / FPS), f32(1 / 9): reciprocals of the two constant divisors of the k == 0 time (k0_time)
    double RFPS64, R9_64;   // RN(1 / fps), RN(1 / 9) in f64: the single-event time's two constant divisors (single_key_fast)
    int fast_slot;     // slot of g_fastdiv that holds the exhaustive check of k0_time's fast form for this FPS, or -1
    float offt[9];     // f32(arange(0,1/fps,1/fps/9)[c]) + f32(t0)
    long long kbase[9];  // key = timestamp - kbase[c], clamped to [0, NK)
    int NK, nbits;
    int ts32;          // every timestamp and key base fits int32: the f32 -> int conversions use 32 bits
    int strategy;      // V2CE_STRATEGY_*: NONE drops every multi-event voxel (LDATI.py:206-207,241)
    int bidir;         // bidirectional relocation (LDATI.py:107-122)
    const float2 *kbb; // pooled slope parameters {k, b} [B][2][9][HW] (LDATI.py:177-190), or null
    unsigned long long *keys;     // generic path ('random'): one 64-bit sort key per event, or null
    int rng_mode;
    const float *uniforms;
    int replay_max_n;
    unsigned long long seed;
    long long frame_base;
    const long long *seg_offsets;
    const long long *frame_ts_add;
    long long *ts;                // SoA outputs (all four or none)
    short *x;
    short *y;
    signed char *p;
    unsigned char *packed;        // or 13-byte packed records
    // two-level path
    int shift, NB, nb1;           // coarse bucket = key >> shift; nb1 = bits of a bucket index
    int T, tpp;                   // tiles per frame (2*tpp), tiles per polarity plane
    int PB;                       // bits of a pixel index
    int capA, cap2;               // LDS capacities (records) of the tile pass / the bucket sort
    int tbits;                    // binary-search steps over the tiles of a frame (read by no kernel any more: kept for the layout)
    const unsigned *tile_off;     // [B][T][9] exclusive prefix of the tile counts inside the segment
    const unsigned *tc;           // [B][T][9] the tile counts themselves
    int sparse_cap;               // tiles with at most this many events (all nine bins) go to the sparse tile kernel; 0 = none
    unsigned short *roff;         // [B*9][T][NB+1] per tile: exclusive prefix of its bucket counts (last = tile total <= kCapTile)
    unsigned *bofs;               // [B*9][NB+1] exclusive prefix of the bucket totals inside the segment
    unsigned *groups;             // [B*9][NB] sort groups: first bucket | (end bucket << 16)
    unsigned *ngroups;            // [B*9]
    unsigned *big_list;           // [B*9*NB] coarse buckets beyond cap2: (segment << 16) | bucket
    unsigned *nbig;               // [1] their number
    int span;                     // most coarse buckets a sort group may cover (key span <= kMaxSpanKeys)
    int hist_bins;                // bins reserved per wave in the sort's LDS histogram
    unsigned *temp;               // [total events] 4-byte records (fine | multi | local pixel)
    int *seg_flag;                // [B*9] always 0 (the bucket scan writes it; buckets beyond cap2 go to ldati_big_bucket_kernel through
                                  // big_list): read by no kernel launched after the two-level path, kept for the layout
    int *status;                  // [1] != 0: an internal limit was hit, or (bit 2) a bidirectional call met a time outside its key window
    int sweep_ok;                 // the sweep kernel could serve this key range (it runs for workspace == NULL only: see seg_flag)
    int ballot_ranks;             // 1 = ignore g_lds_order_ok and rank with the ballot match-any (V2CE_LDATI_NO_ATOMIC_ORDER=1: the
                                  // fallback a device that fails the probe would take, forced so that tests can run it)
    // fused count + sparse tile pass (v2ce_ldati_count_fused): every tile owns a slot of kSparseCap records
    unsigned *tc_w;               // [B][T][9] tile counts, written by the fused kernel
    unsigned long long *stats_w;  // [5] max voxel count | - | - | - | largest tile total (all nine bins)
    unsigned *tile_abs_w;         // [B*9][T] record index of the (tile, bin) run inside `temp`
    const unsigned *tile_abs;     // the same, read by the bucket sort (null: runs at seg_offsets + tile_off)
    const int *fused_status;      // status word of the fused kernel, folded into `status` by the bucket scan
    int slot_cap;                 // > 0: ldati_tile_dense_kernel is ALSO the count pass (v2ce_ldati_count_fused in the dense regime): every
                                  // (tile, bin) run goes to its own slot of slot_cap (= capA) records, counts to tc_w, maxima to stats_w
    int Tp;                       // T rounded up to a multiple of 8
    unsigned *gruns;              // [B*9][NB][Tp] per sort group and tile: run start inside the tile's (tile, bin) run | records << 16,
                                  // written by the bucket scan (which has the run table in L2 anyway) so that a sort workgroup's
                                  // setup is ONE contiguous row instead of two 938-byte-strided loads per tile
    const unsigned *tile_src;     // [B*9][Tp] record index of the (tile, bin) run relative to the sort's base, one contiguous row per
                                  // segment (two-pass: tile_off transposed by the tile scan; fused: the slot starts)
};

// ---- Philox4x32-10, counter (pixel, j>>2, p*9+c, frame), key = seed ---------------------------
__device__ __forceinline__ void philox4(unsigned long long seed, unsigned pixel, unsigned jb,
                                        unsigned pc, unsigned frame, unsigned (&out)[4]) {
    unsigned c0 = pixel, c1 = jb, c2 = pc, c3 = frame;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float u24(unsigned w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }

__device__ __forceinline__ float philox_uniform(unsigned long long seed, unsigned pixel, unsigned j,
                                                unsigned pc, unsigned frame) {
    unsigned o[4];
    philox4(seed, pixel, j >> 2, pc, frame, o);
    const unsigned sel = j & 3u;
    return u24(sel == 0 ? o[0] : sel == 1 ? o[1] : sel == 2 ? o[2] : o[3]);
}

// ---- relocation recurrence (LDATI.py:94-106) up to bin `last` ----------------------------------
// yv[i] holds voxel bin i of this lane's pixel (i <= last, plus yv[9] when last == 8).
// Returns the counts of bins c-1, c, c+1 and the debt of bin c.
__device__ __forceinline__ void relocate_bins(const float (&yv)[10], int c, int last, int &n_l,
                                              int &n_c, int &n_r, float &debt_c) {
    const float eps = 1e-6f;
    float d = 0.0f;
    n_l = n_c = n_r = 0;
    debt_c = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        if (i <= last) {
            const float r = yv[i] - d;
            const float cc = ceilf(r - eps);
            d = cc - r;
            int ni = (int)cc;
            if (i == 8) ni += (int)(yv[9] - d);   // LDATI.py:106
            if (i == c - 1) n_l = ni;
            if (i == c) { n_c = ni; debt_c = d; }
            if (i == c + 1) n_r = ni;
        }
    }
}

__device__ __forceinline__ void load_bins(const float *plane0, long long HW, int px, bool valid,
                                          int last, float (&yv)[10]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const bool need = (i <= last) || (i == 9 && last == 8);
        yv[i] = (need && valid) ? plane0[(long long)i * HW + px] : 0.0f;
    }
}

// all nine bins of one pixel at once: counts and tendencies (LDATI.py:94-106, or :107-122 when bidir)
__device__ __forceinline__ void relocate_all(const float (&yv)[10], bool bidir, int (&n)[9], float (&tend)[9]) {
    const float eps = 1e-6f;
    float d = 0.0f;
    if (!bidir) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const float r = yv[i] - d;
            const float cc = ceilf(r - eps);
            d = cc - r;
            n[i] = (int)cc;
            tend[i] = d;
        }
        n[8] += (int)(yv[9] - d);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float r = yv[i] - d;
        const float cc = ceilf(r - eps);
        d = cc - r;
        n[i] = (int)cc;
        tend[i] = d;
    }
    n[4] = 0;                                  // never written by the reference's bidirectional branch
    tend[4] = 0.0f;
    float bless = yv[9];
#pragma unroll
    for (int i = 8; i > 5; --i) {
        tend[i] = bless;
        float t = yv[i] + bless;
        t = floorf(t + eps);
        bless = (yv[i] - t) + bless;
        bless = bless < 0.0f ? 0.0f : bless;
        n[i] = (int)t;
    }
    tend[5] = bless - d;
    n[5] = (int)ceilf((yv[5] + bless) - d);
}

// a[c] for a wave-uniform c without dynamic register indexing
template <typename T>
__device__ __forceinline__ T pick9(const T (&a)[9], int c) {
    T v = a[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) v = c == i ? a[i] : v;
    return v;
}

// single-event timestamp, all f64 (LDATI.py:156-165)
__device__ __forceinline__ long long single_ts(float debt, double fps, float offt) {
    double t = (double)debt / fps / 9.0;
    t += (double)offt;
    t *= 1e6;
    return (long long)t;
}

// slope parameters of one multi-event voxel, f32 (LDATI.py:188-190 with :25-45 folded in)
__device__ __forceinline__ void slope_params(int n_l, int n_c, int n_r, int c, const LdatiParams &P,
                                             float &k, float &bb, const float2 *tab = nullptr) {
    if (tab) {                                                 // the tabulated results of the expressions below
        const int d = (c == 0 || c == 8) ? 0 : n_r - n_l;
        if (d >= -kSlopeM && d <= kSlopeM && n_c >= 0 && n_c <= kSlopeM && n_l >= 0 && n_r >= 0 && n_l < (1 << 23) && n_r < (1 << 23)) {
            const float2 kb = tab[(d + kSlopeM) * (kSlopeM + 1) + n_c];
            k = kb.x; bb = kb.y;
            return;
        }
    }
    // reflect padding makes the central difference vanish at the first and last bin
    const float sxy = (c == 0 || c == 8) ? 0.0f : ((float)n_r - (float)n_l);
    const float k0 = (3.0f * sxy) / 6.0f;
    k = (k0 / P.VS2) / ((float)n_c + 1e-8f);
    bb = P.INV - (P.VS * k) / 2.0f;
}

// ---- the k == 0 time (u / fps) / 9 (LDATI.py:196) without the two IEEE division sequences ------------------------
// Both divisors are constants of the call.  x / y = fma(fma(-q, y, x), r, q) with q = x * r, r = RN(1 / y), is the
// correctly rounded quotient for all but rare (x, y); instead of proving which, the composition is checked against the
// IEEE divisions for EVERY uniform the Philox path can produce (u = m * 2^-24, m < 2^24) by a 16 M-thread kernel, once
// per device and FPS, enqueued in front of the first emit that needs it; the result lands in g_fastdiv[slot] and the
// kernels take the fast form only when it says "identical for all inputs" (replayed uniforms are arbitrary floats: they
// always take the divisions).  22 -> 6 VALU operations on a path every wave with a multi-event voxel executes.
struct FastDiv { unsigned fps_bits; int ok; int tab_ready; int ok64; };
__device__ FastDiv g_fastdiv[8];
__device__ unsigned g_fastdiv_bad[8];
__device__ unsigned g_fast64_bad[8];
// The slope parameters {k, b} of a multi-event voxel (LDATI.py:188-190) depend on two small integers only -- the central
// difference of the neighbouring counts and the voxel's own count -- and cost three IEEE divisions: tabulated once per
// device and FPS by the very expressions of slope_params (so the entries ARE its results), looked up afterwards.
__device__ float2 g_slope_tab[8][kSlopeTab];

__device__ __forceinline__ float k0_time_fast(float u, float FPS, float RFPS, float R9) {
    float q = u * RFPS;
    q = __builtin_fmaf(__builtin_fmaf(-q, FPS, u), RFPS, q);
    float t = q * R9;
    t = __builtin_fmaf(__builtin_fmaf(-t, 9.0f, q), R9, t);
    return t;
}

// ---- the single-event time (LDATI.py:156-165) without its two f64 division sequences ---------------------------------
// t = (double)debt / fps / 9 with two constant divisors: q = x r, q = fma(fma(-q, y, x), r, q) with r = RN(1 / y) in f64, twice.
// As for k0_time_fast the composition is CHECKED, not proven: a kernel compares it with the IEEE divisions for every f32 the
// tendency of a forward-relocated voxel can take -- all floats in [0, 1) and all negative ones down to -2^-18 (the
// recurrence leaves debt in (-1e-6 - ulp, 1)) -- once per device and fps (~2e9 values, a few ms); the kernels use it only when
// the verdict is "identical everywhere" AND the lane's value lies inside the checked range (anything else -- the
// bidirectional branch's tendencies reach 2 -- takes the divisions).  ~70 -> ~12 f64 operations per single event, which is
// most events of real UNet output.
__device__ __forceinline__ double single_time_fast(float debt, double fps, double rfps, double r9) {
    const double x = (double)debt;
    double q = x * rfps;
    q = __builtin_fma(__builtin_fma(-q, fps, x), rfps, q);
    double t = q * r9;
    t = __builtin_fma(__builtin_fma(-t, 9.0, q), r9, t);
    return t;
}
constexpr unsigned kFast64Neg = 0x36800000u;                 // bits of 2^-18: negative tendencies checked down to -2^-18
__device__ __forceinline__ bool single_fast_range(float debt) { return debt < 1.0f && debt > -0x1p-18f; }

__global__ __launch_bounds__(256) void ldati_fast64_check_kernel(double fps, double rfps, double r9, int slot) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    const unsigned npos = 0x3F800000u;                                    // floats in [0, 1)
    if (i >= (unsigned long long)npos + kFast64Neg) return;
    const unsigned bits = i < npos ? (unsigned)i : 0x80000000u + (unsigned)(i - npos);
    const float d = __uint_as_float(bits);
    const double want = (double)d / fps / 9.0;
    const double got = single_time_fast(d, fps, rfps, r9);
    if (!(want == got)) atomicAdd(&g_fast64_bad[slot], 1u);      // (numeric: -0 against +0 for debt = -0 is the same time)
}

__global__ __launch_bounds__(256) void ldati_fastdiv_check_kernel(float FPS, float RFPS, float R9, int slot) {
    const unsigned m = blockIdx.x * 256u + threadIdx.x;                  // < 2^24
    const float u = (float)m * (1.0f / 16777216.0f);
    const float want = (u / FPS) / 9.0f;
    const float got = k0_time_fast(u, FPS, RFPS, R9);
    if (__float_as_uint(want) != __float_as_uint(got)) atomicAdd(&g_fastdiv_bad[slot], 1u);
}
__global__ __launch_bounds__(256) void ldati_slope_tab_kernel(float VS, float VS2, float INV, int slot) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kSlopeTab) return;
    const int d = i / (kSlopeM + 1) - kSlopeM, n = i % (kSlopeM + 1);
    const float sxy = (float)d;                                // = (float)n_r - (float)n_l: small integers, exact
    const float k0 = (3.0f * sxy) / 6.0f;
    const float k = (k0 / VS2) / ((float)n + 1e-8f);
    g_slope_tab[slot][i] = make_float2(k, INV - (VS * k) / 2.0f);
}
__global__ void ldati_fastdiv_commit_kernel(float FPS, int slot) {
    g_fastdiv[slot].fps_bits = __float_as_uint(FPS);
    g_fastdiv[slot].ok = g_fastdiv_bad[slot] == 0u ? 1 : 0;
    g_fastdiv[slot].ok64 = g_fast64_bad[slot] == 0u ? 1 : 0;
    g_fastdiv[slot].tab_ready = 1;
}

// multi-event timestamp, all f32 (LDATI.py:195-196,210-212)
__device__ __forceinline__ long long multi_ts(float k, float bb, float u, float offt,
                                              const LdatiParams &P) {
    float t;
    if (P.strategy == V2CE_STRATEGY_RANDOM) {
        t = u;                                    // LDATI.py:173-174: the raw uniform, in seconds
    } else if (k == 0.0f) {
        t = (u / P.FPS) / 9.0f;
    } else {
        const float s = bb * bb + (2.0f * k) * u;
        t = (-bb + __builtin_sqrtf(s)) / k;
    }
    t = t + offt;
    t = t * 1e6f;
    return (long long)t;
}

// the same, f32 -> i32 (bit-identical to the i64 conversion while |t| < 2^31: P.ts32) and the key
__device__ __forceinline__ unsigned multi_key(float k, float bb, float u, float offt, int kbase32, const LdatiParams &P,
                                              bool fast = false) {
    float t;
    if (P.strategy == V2CE_STRATEGY_RANDOM) {
        t = u;
    } else if (k == 0.0f) {
        t = fast ? k0_time_fast(u, P.FPS, P.RFPS, P.R9) : (u / P.FPS) / 9.0f;
    } else {
        const float s = bb * bb + (2.0f * k) * u;
        t = (-bb + __builtin_sqrtf(s)) / k;
    }
    t = t + offt;
    t = t * 1e6f;
    int key = (int)t - kbase32;
    key = key < 0 ? 0 : key;
    key = key >= P.NK ? P.NK - 1 : key;
    return (unsigned)key;
}

__device__ __forceinline__ int key_of(long long T, long long kbase, int NK) {
    long long k = T - kbase;
    k = k < 0 ? 0 : k;
    k = k >= NK ? NK - 1 : k;
    return (int)k;
}

// Bidirectional relocation (LDATI.py:107-122) gets a key window sized for NON-NEGATIVE voxels (host_scalars): a negative voxel can
// carry a tendency further out (bin 8's is y[9] itself).  The kernel instances that serve bidirectional calls take their keys
// from here: the same key, and kStatusKeyWindow in the call's status word when the time lies outside [kbase, kbase + NK) --
// the clamp would otherwise move the event's timestamp silently.  Forward calls never reach the clamp (the debt stays in
// (-2e-6, 1), multi-event times in their bin) and keep key_of / multi_key / single_key.
constexpr unsigned kStatusKeyWindow = 4u;
__device__ __forceinline__ int key_of_reporting(bool has, long long T, long long kbase, int NK, int *status) {
    const long long k = T - kbase;
    if (has && (k < 0 || k >= NK)) atomicOr(reinterpret_cast<unsigned *>(status), kStatusKeyWindow);
    return key_of(T, kbase, NK);
}

// the key of a single event: fast form when the wave's tendencies all lie inside the checked range (`fast`: the device
// verdict, 32-bit times), else the divisions.  Must be called by whole waves (the range test is a wave vote).
__device__ __forceinline__ unsigned single_key(bool has, float debt, float offt, long long kbase, bool fast, const LdatiParams &P) {
    const bool in = !has || single_fast_range(debt);
    if (fast && __ballot(!in) == 0ull) {
        double t = single_time_fast(debt, P.fps, P.RFPS64, P.R9_64);
        t += (double)offt;
        t *= 1e6;
        int k = (int)t - (int)kbase;                      // (int)t == (long long)t while |t| < 2^31 (P.ts32)
        k = k < 0 ? 0 : k;
        return (unsigned)(k >= P.NK ? P.NK - 1 : k);
    }
    return (unsigned)key_of(single_ts(debt, P.fps, offt), kbase, P.NK);
}


// ballot match-any: lanes of `has_mask` with equal `key` form a peer group.  Returns the rank of
// this lane inside its group (peers on lower lanes) and the group size.  ~5 VALU per key bit.
__device__ __forceinline__ unsigned match_rank(unsigned key, int nbits, unsigned long long has_mask,
                                               unsigned &npeers) {
    unsigned mlo = 0, mhi = 0;                           // lanes that differ from this lane in some bit
    for (int b = 0; b < nbits; ++b) {
        const int sel = __builtin_amdgcn_sbfe((int)key, b, 1);          // 0 or -1
        const unsigned long long m = __ballot(sel != 0);
        mlo |= (unsigned)m ^ (unsigned)sel;
        mhi |= (unsigned)(m >> 32) ^ (unsigned)sel;
    }
    const unsigned plo = (unsigned)has_mask & ~mlo, phi = (unsigned)(has_mask >> 32) & ~mhi;
    npeers = (unsigned)__popc(plo) + (unsigned)__popc(phi);
    return __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
}

// One 64-record batch of a stable counting sort: `slot` = this wave's running base of the lane's
// bin (LDS, owned by the wave).  Returns base + rank; the last peer advances the base.
__device__ __forceinline__ unsigned take_slots(bool has, unsigned key, int nbits, unsigned *slot) {
    unsigned npeers;
    const unsigned rank = match_rank(key, nbits, __ballot(has), npeers);
    unsigned pos = 0;
    if (has) {
        const unsigned base = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __builtin_amdgcn_wave_barrier();
        if (rank + 1 == npeers) __hip_atomic_store(slot, base + npeers, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        pos = base + rank;
    }
    __builtin_amdgcn_wave_barrier();
    return pos;
}

// The same on a histogram that packs the counters of TWO waves into one word (16 bits each, `sh` = 0 or 16: the tile
// pass): the word is shared with the neighbouring wave, so the group's slots are taken with one atomic add by its first
// lane and handed to the peers through the LDS crossbar.
__device__ __forceinline__ unsigned take_slots_packed(bool has, unsigned key, int nbits, unsigned *slot, unsigned sh) {
    unsigned mlo = 0, mhi = 0;
    const unsigned long long has_mask = __ballot(has);
    for (int b = 0; b < nbits; ++b) {
        const int sel = __builtin_amdgcn_sbfe((int)key, b, 1);
        const unsigned long long m = __ballot(sel != 0);
        mlo |= (unsigned)m ^ (unsigned)sel;
        mhi |= (unsigned)(m >> 32) ^ (unsigned)sel;
    }
    const unsigned plo = (unsigned)has_mask & ~mlo, phi = (unsigned)(has_mask >> 32) & ~mhi;
    const unsigned npeers = (unsigned)__popc(plo) + (unsigned)__popc(phi);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
    const int leader = plo ? __builtin_ctz(plo) : 32 + __builtin_ctz(phi | 0x80000000u);
    unsigned old = 0;
    if (has && rank == 0) old = atomicAdd(slot, npeers << sh);
    old = (unsigned)__shfl((int)old, leader);
    return ((old >> sh) & 0xFFFFu) + rank;
}

// ---- ranks straight from LDS atomics ------------------------------------------------------------
// On gfx950 one wave-instruction of ds_add_rtn_u32 serves the lanes that hit the same LDS word in
// ascending lane order (tools/micro/lds_atomic_order.hip: 0 exceptions in 5.4e9 returned values),
// so the returned value IS the stable rank and the ballot match-any (~4 VALU per key bit and batch)
// is not needed.  That order is not an architectural promise: a probe kernel checks it on every
// device the library runs on (enqueued once, in front of the first count call) and only then sets
// g_lds_order_ok; until / unless it does, the kernels use the ballot ranks (identical results).
__device__ int g_lds_order_ok = 0;
__device__ unsigned g_lds_probe_bad = 0, g_lds_probe_done = 0;

// ---- in-kernel phase stamps (diagnostic build only: make STAMP=1) ---------------------------------
#ifdef V2CE_STAMP
__device__ unsigned long long g_stamp[32];
#define STAMP_DECL unsigned long long st_last = __builtin_amdgcn_s_memtime(), st_acc[12] = {0}
#define STAMP(i) do { const unsigned long long st_now = __builtin_amdgcn_s_memtime(); st_acc[i] += st_now - st_last; st_last = st_now; } while (0)
#define STAMP_FLUSH(base, n) do { if (threadIdx.x == 0) for (int st_i = 0; st_i < (n); ++st_i) atomicAdd(&g_stamp[(base) + st_i], st_acc[st_i]); } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH(base, n)
#endif

__global__ __launch_bounds__(256) void ldati_lds_order_probe_kernel(int iters) {
    __shared__ unsigned tab[4][512];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned s = (blockIdx.x * 256 + threadIdx.x) * 2654435761u + 12345u;
    unsigned nbad = 0;
    for (int it = 0; it < iters; ++it) {
        for (int i = lane; i < 512; i += 64) tab[wid][i] = 7u * i;
        __builtin_amdgcn_wave_barrier();
        s = s * 1664525u + 1013904223u;
        const unsigned range = 1u << (it % 10);
        const unsigned key = (s >> 9) & (range - 1u);
        const bool act = ((s >> 5) & 7u) != 0u || (it & 1);
        unsigned got = 0;
        if (act) got = atomicAdd(&tab[wid][key], 1u);
        unsigned np;
        const unsigned want = 7u * key + match_rank(key, 9, __ballot(act), np);
        if (act && got != want) ++nbad;
        __builtin_amdgcn_wave_barrier();
    }
    if (nbad) atomicAdd(&g_lds_probe_bad, nbad);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned done = atomicAdd(&g_lds_probe_done, 1u);
        if (done == gridDim.x - 1) {
            __threadfence();
            g_lds_order_ok = atomicAdd(&g_lds_probe_bad, 0u) == 0u ? 1 : 0;
        }
    }
}

// slot of one record in a stable counting sort batch: LDS-atomic rank when the device passed the
// probe, ballot rank otherwise
__device__ __forceinline__ unsigned take_slot(bool atomic_order, bool has, unsigned key, int nbits, unsigned *slot) {
    if (atomic_order) return has ? atomicAdd(slot, 1u) : 0u;
    return take_slots(has, key, nbits, slot);
}

// px / W for px + 0.5 < 2^22 in three operations: (px + 0.5) / W lies at least 0.5 / W away from every integer, and the
// two roundings (1 / W, the product) move it by less than (px + 0.5) / W * 2^-23 < 0.5 / W, so the truncation is exact
__device__ __forceinline__ unsigned div_tiny(unsigned px, float rcpW) {
    return (unsigned)(((float)px + 0.5f) * rcpW);
}

// px / W for px < 2^24 (exact in f32) without an integer division
__device__ __forceinline__ unsigned div_small(unsigned px, unsigned W, float rcpW) {
    unsigned q = (unsigned)((float)px * rcpW);
    const int r = (int)(px - q * W);
    q += (r >= (int)W) ? 1u : 0u;
    q -= (r < 0) ? 1u : 0u;
    return q;
}

__device__ __forceinline__ void store_packed_bytes(unsigned char *dst, long long t, unsigned xx,
                                                   unsigned yy, unsigned pp) {
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = (unsigned char)((unsigned long long)t >> (8 * k));
    dst[8] = (unsigned char)xx; dst[9] = (unsigned char)(xx >> 8);
    dst[10] = (unsigned char)yy; dst[11] = (unsigned char)(yy >> 8);
    dst[12] = (unsigned char)pp;
}

// inclusive scan over the 64 lanes of a wave: DPP row shifts inside the rows of 16 lanes, then the two row
// broadcasts of gfx9 (lane 15 of a row into the next row; lane 31 into rows 2-3) -- six VALU operations instead
// of six dependent ds_bpermute round trips through the LDS crossbar (~100 cycles each)
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane) {
    (void)lane;
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);   // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return (unsigned)x;
}

// exclusive scan of one value per thread over a workgroup of NW <= 64 waves; `part` = NW LDS words.
// Returns the exclusive prefix; *total = sum over the workgroup.  ONE barrier: every wave scans the NW wave totals itself
// (a 64-lane DPP scan costs less than a second barrier and a serial loop on one thread).  The caller separates two scans
// that share `part` by a barrier of its own (every call site has one: the totals are read right behind the barrier here).
template <int NW>
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned *part, unsigned *total) {
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned incl = wave_incl_scan(v, lane);
    if (lane == 63) part[wid] = incl;
    __syncthreads();
    const unsigned pin = wave_incl_scan(lane < NW ? part[lane] : 0u, lane);
    *total = (unsigned)__builtin_amdgcn_readlane((int)pin, NW - 1);
    const unsigned base = wid ? (unsigned)__builtin_amdgcn_readlane((int)pin, wid - 1) : 0u;
    return base + incl - v;
}

// the same for two values per thread with one barrier; `part` = 2 * NW LDS words
template <int NW>
__device__ __forceinline__ void block_excl_scan2(unsigned a, unsigned e, unsigned *part, unsigned &a_ex,
                                                 unsigned &e_ex, unsigned &a_tot, unsigned &e_tot) {
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned ia = wave_incl_scan(a, lane), ie = wave_incl_scan(e, lane);
    if (lane == 63) { part[wid] = ia; part[NW + wid] = ie; }
    __syncthreads();
    const unsigned pa = wave_incl_scan(lane < NW ? part[lane] : 0u, lane);
    const unsigned pe = wave_incl_scan(lane < NW ? part[NW + lane] : 0u, lane);
    a_tot = (unsigned)__builtin_amdgcn_readlane((int)pa, NW - 1);
    e_tot = (unsigned)__builtin_amdgcn_readlane((int)pe, NW - 1);
    a_ex = (wid ? (unsigned)__builtin_amdgcn_readlane((int)pa, wid - 1) : 0u) + ia - a;
    e_ex = (wid ? (unsigned)__builtin_amdgcn_readlane((int)pe, wid - 1) : 0u) + ie - e;
}

// `want` consecutive slots of an LDS counter for every lane with ONE atomic per wave (all 64 lanes must be active):
// a per-lane atomicAdd on one address is served lane by lane -- up to 64 LDS cycles per wave instruction.
__device__ __forceinline__ unsigned wave_alloc(unsigned *counter, unsigned want, int lane) {
    const unsigned incl = wave_incl_scan(want, lane);
    const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
    unsigned base = 0;
    if (tot) {                                              // wave-uniform
        if (lane == 63) base = atomicAdd(counter, tot);
        base = (unsigned)__builtin_amdgcn_readlane((int)base, 63);
    }
    return base + incl - want;
}

}  // namespace
}  // namespace v2ce
