// ldati_plan.h -- the host-side planning of LDATI (ldati.hip): every size, offset and path decision of a call as a pure function
// of its arguments, each written down once.  Plain host C++ (no HIP, no rocPRIM): it compiles on its own.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/v2ce_hip.h"
#include "ldati_const.h"

namespace v2ce {
namespace {

struct Opts { int strategy, bidir, pooling, pool_k; };   // v2ce_ldati_options after validation (read_options)

// Every V2CE_LDATI_* switch of the library is read here and nowhere else.  Policy: tile_threads, nb_soft and
// dense_nw are read ONCE per process (kernel A/B runs set them before the start); every other switch is read again for each
// call, because tests flip them inside one process.
struct Knobs {
    int tile_threads;      // 512 | 1024 threads of the per-bin tile kernel; 0 = by density
    int nb_soft;           // soft limit of the coarse buckets per segment (kMaxNB = none; measured 256: tile pass -36 us, sort +31 us,
                           // bucket scan +10 us on the stress chunk)
    int dense_nw;          // 8 | 16 waves of the dense tile kernel; anything else = by LDS footprint
    int sort_threads;      // 64 | 128 | 256 threads of a sort workgroup; 0 = by density
    int span_keys;         // 128 | 256 | 512 keys a sort group spans; 0 = by regime
    bool no_sparse, no_fused, old_tile, no_fastdiv, debug;
    bool ballot_ranks;     // the fallback a device that fails the LDS-order probe would take, forced so that tests can run it
};
Knobs read_knobs() {
    const auto num = [](const char *e) { return e ? atoi(e) : 0; };
    static const int tt = num(getenv("V2CE_LDATI_TILE_THREADS")), soft = num(getenv("V2CE_LDATI_NB_SOFT")), nw = num(getenv("V2CE_LDATI_DENSE_NW"));
    const int st = num(getenv("V2CE_LDATI_SORT_THREADS")), sp = num(getenv("V2CE_LDATI_SPAN_KEYS"));
    const char *ao = getenv("V2CE_LDATI_NO_ATOMIC_ORDER");
    Knobs k{};
    k.tile_threads = tt == 512 || tt == 1024 ? tt : 0; k.nb_soft = soft >= 16 && soft <= kMaxNB ? soft : kMaxNB; k.dense_nw = nw;
    k.sort_threads = st == 64 || st == 128 || st == 256 ? st : 0;
    k.span_keys = sp == 128 || sp == 256 || sp == 512 ? sp : 0;
    k.no_sparse = getenv("V2CE_LDATI_NO_SPARSE") != nullptr; k.no_fused = getenv("V2CE_LDATI_NO_FUSED") != nullptr;
    k.old_tile = getenv("V2CE_LDATI_OLD_TILE") != nullptr; k.no_fastdiv = getenv("V2CE_LDATI_NO_FASTDIV") != nullptr;
    k.debug = getenv("V2CE_LDATI_DEBUG") != nullptr; k.ballot_ranks = ao && ao[0] == '1';
    return k;
}

// host-side scalars, computed exactly like CPU torch does
struct HostScalars {
    float VS, VS2, INV, FPS;
    float offt[9];
    long long kbase[9], NK;
    int nbits;
    size_t lds_bytes;     // of the sweep kernel
    bool sweep_ok;        // 4*NK counters fit the LDS
    bool ok;
};
HostScalars host_scalars(double fps, double t0, bool bidir = false, bool random = false) {
    HostScalars h{};
    const double vs = 1.0 / fps / 9.0;
    h.VS = (float)vs;
    h.VS2 = (float)(vs * vs);
    h.INV = (float)(1.0 / vs);
    h.FPS = (float)fps;
    for (int c = 0; c < 9; ++c) h.offt[c] = (float)(0.0 + (double)c * vs) + (float)t0;
    // f32 resolution of (t + offt)*1e6 near the last bin decides how far a multi-event timestamp
    // can round outside [offt, offt + vs]; size the slack from it.
    const double top = (double)fabsf(h.offt[8]) + vs;
    const double ulp_us = top * 1.1920929e-7 * 1e6;      // one f32 ulp of the largest time, in us
    const long long slack = 16 + (long long)(8.0 * ulp_us);
    const long long span = (long long)(vs * 1e6) + 2;
    // forward relocation: every timestamp lies in its bin, whatever the (finite) voxel values.  Bidirectional
    // (LDATI.py:107-122), NON-NEGATIVE voxels: a single event's tendency lies in (-1, 2) bin widths (bin 5: bless - debt;
    // bin 8: y[9] < 2 when n == 1) -- one bin width before and one after.  With negative voxels no margin holds (bin 8's
    // tendency is y[9] itself, and n == 1 only bounds y[8] + y[9]): the bidirectional kernel instances report a time
    // outside the window in the status word (key_of_reporting) and the call is refused (DeviceEvents.check).
    // 'random' (LDATI.py:173-174): the multi-event offsets are raw uniforms in SECONDS.
    const long long before = bidir ? span : 0;
    const long long after = (random ? 1000000 : 0) + (bidir ? span : 0);
    const long long nk = before + span + after + 2 * slack;
    for (int c = 0; c < 9; ++c) h.kbase[c] = (long long)((double)h.offt[c] * 1e6) - slack - before;
    h.NK = nk;
    // the two-level path's key range; the generic ('random') path only needs 20-bit keys
    h.ok = nk > 0 && (random ? nk < (1ll << 20) : nk <= ((long long)kMaxNB << kMaxShift));
    // sweep kernel: 4*NK*4 B must fit 160 KiB of LDS with the scratch beside it; forward relocation only
    h.sweep_ok = nk > 0 && nk <= 9600 && !bidir && !random;
    int nb = 0;
    while ((1ll << nb) < nk) ++nb;
    h.nbits = nb;
    h.lds_bytes = (size_t)(4 * nk + 256) * 4 + 3 * 128 * 4;
    return h;
}

constexpr size_t kLdsMax = 160 * 1024;   // LDS of one workgroup on gfx950
size_t round16(size_t n) { return (n + 15) / 16 * 16; }

// tile workspace (v2ce_ldati_count / _count_fused -> emit), byte offsets: tc [B][T][9] tile counts | tile_off [B][T][9] their exclusive
// prefix inside the segment | tile_src [B*9][Tp] the same offsets as one contiguous row per segment; with the tile geometry: tiles
// per polarity plane, per frame (both polarities), the latter rounded up to a multiple of 8
struct TileWs { long long tpp, T, Tp; size_t tc, tile_off, tile_src, bytes; };
TileWs tile_ws(int B, int H, int W) {
    const long long tpp = ((long long)H * W + kTilePix - 1) / kTilePix, T = 2 * tpp, Tp = (T + 7) & ~7ll;
    const size_t n = (size_t)B * (size_t)T * 9 * 4;
    return TileWs{tpp, T, Tp, 0, n, 2 * n, 2 * n + (size_t)B * 9 * (size_t)Tp * 4};
}

// dynamic LDS of ldati_tile_dense_kernel<NW>: S [capA] | O [capA + 2] | hist [NW][NB] | wave totals, scan partials, batch counter
size_t dense_tile_lds(int capA, int NB, int NW) { return ((size_t)2 * capA + 8 + (size_t)NW * NB + 3 * NW + NW + 1 + 2 + 18 + 10 + 2) * 4; }

// bins a wave reserves in the sort's LDS histogram: four per key of the widest group, <= 4 * max(kMaxSpanKeys, 2^shift)
int sort_hist_bins(int span, int shift) { return 4 * (span << shift) > 4 * kMaxSpanKeys ? 4 * (span << shift) : 4 * kMaxSpanKeys; }

// geometry and capacities of the two-level path
struct Plan {
    int tpp, T, Tp, shift, NB, nb1, PB, capA, cap2, tbits, tile_threads, span, sort_threads, sort_k;
    size_t n_tab, n_bkt;                 // entries of roff; of bofs
    size_t lds_tile, lds_sort;
    bool fields_ok;                      // every index field is wide enough; no LDS footprint counted (the per-bin kernel's is no limit of a fused layout's kernels)
    bool tile_ok;                        // the tile pass can run (all the generic path needs)
    bool ok;                             // ... and the bucket scan and sort: the two-level path
};
Plan make_plan(const HostScalars &h, const Knobs &k, int B, int H, int W, int64_t total_events, int64_t max_segment_events, int64_t max_tile_events) {
    Plan p{};
    const long long HW = (long long)H * W;
    const TileWs tw = tile_ws(B, H, W);
    p.tpp = (int)tw.tpp; p.T = (int)tw.T; p.Tp = (int)tw.Tp;
    p.PB = 1;
    while ((1ll << p.PB) < HW) ++p.PB;
    // coarse (level 1) bucket width 2^shift us: at most 16 us, finer when the densest segment would
    // put more than cap2/20 records into an AVERAGE bucket (on real UNet output the fullest bucket of a
    // segment holds ~20x the average: timestamps crowd at the end of a bin), never finer than kMaxNB
    // buckets allow.  The sort groups (bucket scan kernel) merge consecutive buckets up to cap2 records.
    // sort workgroups of 128 threads (3072 records) for segments of real UNet output, 256 (6144) for dense ones: measured on the
    // e2e step (densest segment 85 K events) 151 -> 98 us, sparse bench 93 -> 73 us, on the stress chunk 432 -> 490 us, pano sort
    // -66 us but bucket scan +80 us (V2CE_LDATI_SORT_THREADS overrides; kernel A/B runs)
    // (the densest segment spread evenly over its keys: a group of kMaxSpanKeys keys then holds at most 1.5 x 3072 records --
    // groups of such segments are closed by their key span, not by their record count)
    const bool small = max_segment_events <= 2048;     // segments of at most 2048 events: 256 threads, 8 records each
    p.sort_threads = small ? 256 : k.sort_threads ? k.sort_threads : (max_segment_events * kMaxSpanKeys > 4608 * h.NK ? 256 : 128);
    p.sort_k = small ? 8 : 24;
    p.cap2 = p.sort_threads * p.sort_k;
    const int sort_waves = p.sort_threads / 64;
    int shift = 4;
    while (shift > 0 && (double)max_segment_events * (double)(1 << shift) / (double)h.NK > p.cap2 / 20.0) --shift;
    while (shift < kMaxShift && ((h.NK + (1ll << shift) - 1) >> shift) > kMaxNB) ++shift;
    // Dense segments (the rule above asks for the finest buckets) gain nothing from more than ~256 buckets: the sort groups
    // merge consecutive buckets up to cap2 records anyway, while the tile pass pays per (wave, bucket) cell and the gather per
    // run (V2CE_LDATI_NB_SOFT overrides the soft limit; kernel A/B runs)
    while (shift < 4 && ((h.NK + (1ll << shift) - 1) >> shift) > k.nb_soft) ++shift;
    p.shift = shift;
    p.NB = (int)((h.NK + (1ll << shift) - 1) >> shift);
    while ((1 << p.nb1) < p.NB) ++p.nb1;
    // key span of a sort group: 128 keys for dense segments; for the small-group regime (128-thread workgroups) the groups are
    // closed by their span, not by their records, so a wider span means fewer, fuller groups (V2CE_LDATI_SPAN_KEYS: A/B runs;
    // measured 128 / 256 / 512: e2e sort 94 / 89 / 116 us)
    const int span_keys = k.span_keys ? k.span_keys : (p.sort_threads == 128 && !small) ? kSmallGroupSpanKeys : kMaxSpanKeys;
    p.span = (span_keys >> shift) > 0 ? (span_keys >> shift) : 1;
    while ((1 << p.tbits) < p.T) ++p.tbits;
    p.capA = max_tile_events > 256 ? (int)((max_tile_events + 255) / 256 * 256) : 256;
    p.n_bkt = (size_t)B * 9 * (size_t)(p.NB + 1);
    p.n_tab = p.n_bkt * (size_t)p.T;
    // workgroup size of the per-bin tile pass: 1024 threads (2 pixels each) for dense tiles, whose LDS footprint allows one
    // workgroup per CU anyway; 512 threads (4 pixels each, half the barrier traffic and histogram rows) for sparse ones
    p.tile_threads = k.tile_threads ? k.tile_threads : (max_tile_events > 4096 ? 1024 : 512);
    p.lds_tile = (size_t)(2 * p.capA + 2048) * 4 + (size_t)kTilePix * 8 + (size_t)(p.tile_threads / 128) * p.NB * 4 + 2 * (p.tile_threads / 64 + 1) * 4;
    const size_t tables = sort_waves * (size_t)sort_hist_bins(p.span, shift) * 4 + (size_t)(2 * p.T) * 4 + (size_t)(2 * (p.cap2 / 32)) * 4 +
                          (sort_waves + 1) * 4;
    const size_t stage = (size_t)p.sort_threads * 13 * 4;
    p.lds_sort = (size_t)(p.cap2 + 20) * 4 + (tables > stage ? tables : stage);
    const bool tile_fields_ok = h.ok && p.T <= kMaxTiles && p.capA <= kCapTile && p.PB <= 22 && B * 9 <= 65535;
    p.fields_ok = tile_fields_ok && p.NB <= kMaxNB;
    p.tile_ok = tile_fields_ok && total_events < (1ll << 32) && p.lds_tile <= kLdsMax;
    p.ok = p.tile_ok && p.fields_ok && p.lds_sort <= kLdsMax;
    return p;
}

// The workspace of one emit call, byte offsets from its start.  THE definition of the layout: v2ce_ldati_workspace_bytes
// returns `bytes`, the emit paths carve their pointers from the offsets, v2ce_ldati_status returns `status`.
//   two-level: bofs u32 [n_bkt = B*9*(NB+1)] | groups u32 [B*9*NB] | big_list u32 [B*9*NB] | ngroups u32 [B*9] | seg_flag i32 [B*9] |
//              status i32 [4] = {status, nbig = number of big buckets, -, -} | temp u32 [total] (the records) |
//              roff u16 [n_tab = B*9*T*(NB+1), rounded up to even] | gruns u32 [B*9][NB][Tp]
//   generic ('random'): status i32 [4] | keys, keys_alt u64 [total] each | sort_temp (the library radix sort's) | soa (packed output only:
//              the decoded SoA arrays, ts i64 | x i16 | y i16 | p i8, [total] each)
//   both: ... | kbb float2 [B][2][9][HW] (pooled slope only), 16-byte aligned like every generic member
struct TwoLevelWs {
    size_t bofs, groups, big_list, ngroups, seg_flag, status, temp, roff, gruns;
    size_t keys, keys_alt, sort_temp, soa, kbb, bytes;
    bool generic, ok;
};
// radix_temp_bytes: what the library radix sort asks for `total` keys (generic path only; the caller's to compute)
TwoLevelWs two_level_ws(const Plan &p, const Opts &o, int B, int H, int W, int64_t total, bool packed_out, size_t radix_temp_bytes) {
    TwoLevelWs w{};
    const size_t n = (size_t)(total > 0 ? total : 0), segs = (size_t)B * 9;
    size_t end;
    w.generic = o.strategy == V2CE_STRATEGY_RANDOM;
    if (w.generic) {   // (the tile pass still runs, in its key-writing mode)
        w.ok = p.tile_ok;
        w.keys = w.status + 16; w.keys_alt = w.keys + round16(n * 8);
        w.sort_temp = w.keys_alt + round16(n * 8); w.soa = w.sort_temp + round16(radix_temp_bytes);
        end = w.soa + (packed_out ? round16(n * 13) + 64 : 0);
    } else {
        w.ok = p.ok;
        w.groups = w.bofs + p.n_bkt * 4; w.big_list = w.groups + segs * p.NB * 4;
        w.ngroups = w.big_list + segs * p.NB * 4; w.seg_flag = w.ngroups + segs * 4;
        w.status = w.seg_flag + segs * 4; w.temp = w.status + 16;
        w.roff = w.temp + n * 4; w.gruns = w.roff + ((p.n_tab + 1) & ~(size_t)1) * 2;
        end = round16(w.gruns + segs * p.NB * p.Tp * 4);
    }
    w.kbb = end;
    w.bytes = w.kbb + (o.pooling != V2CE_POOL_NONE ? (size_t)B * 2 * 9 * (size_t)H * W * 8 : 0);
    return w;
}

// what a path choice needs to know of the call beyond its options: pooled slope parameters present (LdatiParams::kbb), every time
// fits 32 bits (ts32), the device tables of this fps are checked (fast_slot >= 0), packed output.  The size queries, which have no
// call yet, take ts32 and fast for granted.
struct CallFacts { bool pooled, ts32, fast, packed; };
// THE decision which kernels a call launches
struct PathChoice {
    bool generic;            // 'random': tile pass in key mode, library radix sort, decode
    int dense_nw;            // 8 | 16: ldati_tile_dense_kernel<dense_nw> is the tile pass; 0: ldati_tile_pass_kernel<tile_threads, ., bidir>
    size_t dense_lds;
    int tile_threads; bool bidir;   // ... and the BIDIR instance of the per-bin and the sparse tile kernel
    int sparse_cap;          // kSparseCap: tiles of at most that many events go to ldati_tile_sparse_kernel; 0: none do
    bool sort_packed;        // ldati_bucket_sort_kernel<sort_packed, sort_k, sort_threads>
    int sort_k, sort_threads;
    int hist_bins;           // bins a wave reserves in the sort's LDS histogram
};
PathChoice choose_path(const Opts &o, const Plan &p, const Knobs &k, const CallFacts &f) {
    PathChoice c{};
    c.generic = o.strategy == V2CE_STRATEGY_RANDOM;
    // the dense tile kernel serves the common call (forward relocation, 'slope' with the device tables of this fps or 'none', no
    // pooling, 32-bit times) when its 16-wave form fits the LDS; everything else stays on the per-bin kernel
    const bool dense = !o.bidir && !f.pooled && f.ts32 && !k.old_tile && dense_tile_lds(p.capA, p.NB, 16) <= kLdsMax &&
                       (o.strategy == V2CE_STRATEGY_NONE || (o.strategy == V2CE_STRATEGY_SLOPE && f.fast));
    if (dense) {
        const size_t lds8 = dense_tile_lds(p.capA, p.NB, 8);
        // eight waves when two such workgroups fit a CU (V2CE_LDATI_DENSE_NW = 8 | 16 forces one; kernel A/B runs)
        c.dense_nw = k.dense_nw == 16 ? 16 : ((k.dense_nw == 8 && lds8 <= kLdsMax) || lds8 <= kLdsMax / 2) ? 8 : 16;
        c.dense_lds = c.dense_nw == 8 ? lds8 : dense_tile_lds(p.capA, p.NB, 16);
    }
    c.tile_threads = p.tile_threads; c.bidir = o.bidir != 0;
    // lightly populated tiles (all nine bins <= kSparseCap events) take the one-pass sparse kernel; it needs the nine bins' keys
    // side by side in 20 bits
    c.sparse_cap = !c.generic && 9ll * ((long long)p.NB << p.shift) < (1ll << 20) && !k.no_sparse ? kSparseCap : 0;
    c.sort_packed = f.packed; c.sort_k = p.sort_k; c.sort_threads = p.sort_threads;
    c.hist_bins = sort_hist_bins(p.span, p.shift);
    return c;
}

// ---- fused count + tile pass: geometry the kernel assumes BEFORE the counts exist, and its workspace ----------
// The coarse-bucket geometry of a call follows from its densest segment (make_plan).  The fused kernel runs before that is
// known, with the geometry of the caller's HINT (the previous call's max_segment_events: consecutive batches of a clip
// agree); v2ce_ldati_emit_fused uses its records only if the plan made from the real counts has the same geometry and no
// tile exceeded its slot.  Layout: status i32 [4] | tile_abs u32 [B*9][Tp] | records u32 | roff u16 [n_tab].
struct FusedLayout {
    Plan p0;
    size_t off_abs, off_rec, off_roff, bytes;
    int slot_cap;                        // dense mode: records per (tile, bin) slot (= the tile pass's LDS capacity); 0 = sparse mode
    bool ok;
};
// tile_bin_hint = 0: the sparse kernel's fused form (a slot of kSparseCap records per tile);  > 0: the dense kernel's (a slot per
// (tile, bin), sized from the caller's expectation of the densest one).  Whether the dense kernel serves the CALL is for
// choose_path(o, F.p0, k, the call's facts) to say, on both sides of the count / emit pair.
FusedLayout make_fused_layout(const HostScalars &h, const Opts &o, const Knobs &k, int B, int H, int W, int64_t seg_hint, int64_t tile_bin_hint) {
    FusedLayout F{};
    F.p0 = make_plan(h, k, B, H, W, 0, seg_hint > 0 ? seg_hint : 0, tile_bin_hint > 0 ? tile_bin_hint : 0);
    const Plan &p = F.p0;
    const PathChoice c = choose_path(o, p, k, CallFacts{o.pooling != V2CE_POOL_NONE, true, true, false});
    F.slot_cap = tile_bin_hint > 0 ? p.capA : 0;
    const size_t n_abs = (size_t)B * 9 * p.Tp, n_rec = F.slot_cap ? (size_t)B * p.T * 9 * (size_t)F.slot_cap : (size_t)B * p.T * kSparseCap;
    F.ok = p.fields_ok && n_rec < (1ull << 32) &&
           (F.slot_cap ? c.dense_nw && n_rec <= (1ull << 30)   // (at most 4 GiB of slots: beyond that the count pass is the cheaper price)
                       : c.sparse_cap != 0) && !c.generic && o.pooling == V2CE_POOL_NONE && !k.no_fused;
    F.off_abs = 16; F.off_rec = round16(F.off_abs + n_abs * 4);
    F.off_roff = round16(F.off_rec + n_rec * 4); F.bytes = round16(F.off_roff + p.n_tab * 2);
    return F;
}

}  // namespace
}  // namespace v2ce
