// tsdiff.hip -- the stage-2 score of generated events against a recording, on gfx950.
//
// Replaces ts_diff_metric of train/scripts/stage2/stage2_metrics.py:22-88: for every ground-truth event
// (x, y, p, t), d = min(1e6, min |t_pred - t| over the predicted events of polarity p in the cells
// [x-r, x+r] x [y-r, y+r] clamped to the sensor), capped at cap = 1e6 / fps / 10 * 3 (a capped event is an
// "overflow").  The reference loops over events in Python; here many frame pairs go through one call:
//
//   validate -> per chunk of pairs: count -> scan -> scatter -> sort long cells -> query -> copy out
//
// * Bucketing: predicted timestamps are grouped by cell ((pair*2 + p)*H + y)*W + x with an atomic count, a
//   device-wide exclusive scan (three kernels, no library) and an atomic scatter.  The scatter order inside a
//   cell is arbitrary; the minimum does not depend on it, so results are bit-identical run to run.
// * Cells with more than kSmall events are sorted: tiles of kTile in LDS (bitonic, 16 KB), then, for cells
//   longer than one tile, ping-pong merge passes in global memory (each element finds its rank in the
//   partner run by binary search).  A cell of 2^20 events needs 9 passes.  Shorter cells are scanned
//   linearly by the query.
// * Query: one lane per ground-truth event; in each of the (2r+1)^2 clamped cells a lower_bound and its
//   left neighbour (sorted cells) or a linear scan (short cells).  S (int64 sum of the uncapped d) and K
//   (capped count) are reduced per wave and added with one int64 atomic per wave and pair: integer sums, so
//   the order of the adds does not matter.
// * Nothing is written to per_event_d / pair_stats unless the validation pass found every input in range:
//   a bad coordinate, polarity, offset or fps sets a bit of *status, and every later kernel returns at once.
//
// Built with the EXACT flags: cap is the reference's left-to-right f64 expression, and the cap test
// compares (double)d with it, as numpy does.
#include "common.h"

namespace v2ce {
namespace {

constexpr int kThreads = 256;
constexpr int kSmall = 16;          // cells up to this length are scanned linearly
constexpr int kTile = 2048;         // LDS sort tile (int64): 16 KB
constexpr int kScanItems = 8;       // per thread
constexpr int kScanBlock = kThreads * kScanItems;
constexpr long long kCellBudget = 64ll * 2 * 260 * 346;   // cells of one chunk: 64 pairs at 346x260 (46 MB)

enum : int {   // bits of *status (include/v2ce_hip.h)
    kBadOffsets = V2CE_TSDIFF_BAD_OFFSETS, kBadFps = V2CE_TSDIFF_BAD_FPS, kBadGtXY = V2CE_TSDIFF_BAD_GT_XY,
    kBadGtP = V2CE_TSDIFF_BAD_GT_POLARITY, kBadPredXY = V2CE_TSDIFF_BAD_PRED_XY, kListOverflow = 32,
};

struct Params {
    const int64_t *gt_ts;
    const int16_t *gt_x, *gt_y;
    const int8_t *gt_p;
    const int64_t *gt_off;
    long long n_gt;
    const int64_t *pr_ts;
    const int16_t *pr_x, *pr_y;
    const int8_t *pr_p;
    const int64_t *pr_off;
    long long n_pred;
    const double *fps;
    int pairs, H, W, r;
    double *d_out;
    int64_t *stats_out;
    int32_t *status;
    // workspace
    unsigned long long *acc;  // [pairs][2]: S, K
    int *meta;                // [0] tile entries, [1] long cells
    int *cnt, *start, *bsum;  // [ncells + 1], [ncells + 1], [nblocks]
    int64_t *ts_a, *ts_b;     // bucketed timestamps; ts_b: merge ping-pong (null when n_pred <= kTile)
    int2 *tiles;              // (cell, tile) of every LDS tile to sort
    int *big;                 // cells longer than one tile
    int tile_cap, big_cap;
    // chunk
    int p0, np, ncells;
};

__device__ __forceinline__ bool failed(const Params &P) { return *(volatile int32_t *)P.status != 0; }

__device__ __forceinline__ int merge_passes(int n) {   // ping-pong passes that leave a cell of n sorted
    const int nt = (int)(((long long)n + kTile - 1) / kTile);
    return nt <= 1 ? 0 : 32 - __clz(nt - 1);
}

__device__ __forceinline__ long long absdiff(long long a, long long b) {   // |a - b| in wrapping int64, as numpy
    const long long d = (long long)((unsigned long long)a - (unsigned long long)b);
    return d < 0 ? (long long)(0ull - (unsigned long long)d) : d;
}

__global__ __launch_bounds__(kThreads) void tsdiff_validate_kernel(Params P) {
    int bad = 0;
    const long long stride = (long long)gridDim.x * kThreads;
    const long long n = P.n_gt > P.n_pred ? P.n_gt : P.n_pred;
    const long long m = n > (long long)P.pairs * 2 + 1 ? n : (long long)P.pairs * 2 + 1;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < m; i += stride) {
        if (i < 2 * (long long)P.pairs) P.acc[i] = 0;
        if (i < P.pairs) {
            const double f = P.fps[i];
            if (!(f > 0.0) || !isfinite(f)) bad |= kBadFps;
            if (P.gt_off[i] > P.gt_off[i + 1] || P.pr_off[i] > P.pr_off[i + 1]) bad |= kBadOffsets;
        }
        if (i == 0 && (P.gt_off[0] < 0 || P.pr_off[0] < 0)) bad |= kBadOffsets;
        if (i == P.pairs && (P.gt_off[i] > P.n_gt || P.pr_off[i] > P.n_pred)) bad |= kBadOffsets;
        if (i < P.n_gt) {
            const int x = P.gt_x[i], y = P.gt_y[i], p = P.gt_p[i];
            if (x < 0 || x >= P.W || y < 0 || y >= P.H) bad |= kBadGtXY;
            if (p < -1 || p > 1) bad |= kBadGtP;
        }
        if (i < P.n_pred) {
            const int x = P.pr_x[i], y = P.pr_y[i];
            if (x < 0 || x >= P.W || y < 0 || y >= P.H) bad |= kBadPredXY;
        }
    }
    if (bad) atomicOr(P.status, bad);
}

__global__ __launch_bounds__(kThreads) void tsdiff_zero_kernel(Params P) {
    if (failed(P)) return;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i <= P.ncells; i += (long long)gridDim.x * kThreads)
        P.cnt[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 2) P.meta[threadIdx.x] = 0;
}

__device__ __forceinline__ int pred_cell(const Params &P, int pl, long long i) {
    const int p = P.pr_p[i] != 0;
    return ((pl * 2 + p) * P.H + P.pr_y[i]) * P.W + P.pr_x[i];
}

// grid (G, np): block row blockIdx.y walks the predicted events of pair p0 + blockIdx.y
__global__ __launch_bounds__(kThreads) void tsdiff_count_kernel(Params P) {
    if (failed(P)) return;
    const int pl = blockIdx.y;
    const long long lo = P.pr_off[P.p0 + pl], hi = P.pr_off[P.p0 + pl + 1];
    for (long long i = lo + (long long)blockIdx.x * kThreads + threadIdx.x; i < hi; i += (long long)gridDim.x * kThreads)
        atomicAdd(&P.cnt[pred_cell(P, pl, i)], 1);
}

__device__ __forceinline__ int block_sum(int v, int *red) {   // all threads get the block's sum
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    const int wv = threadIdx.x / kWave, nw = blockDim.x / kWave;
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) red[wv] = v;
    __syncthreads();
    int s = 0;
    for (int k = 0; k < nw; ++k) s += red[k];
    return s;
}

__device__ __forceinline__ int block_exclusive(int v, int *red) {   // exclusive prefix of v over the block
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

__global__ __launch_bounds__(kThreads) void tsdiff_scan_reduce_kernel(Params P) {
    __shared__ int red[kThreads / kWave];
    if (failed(P)) return;
    const long long base = (long long)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k <= P.ncells) s += P.cnt[base + k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) P.bsum[blockIdx.x] = s;
}

__global__ __launch_bounds__(1024) void tsdiff_scan_top_kernel(Params P, int nb) {
    __shared__ int red[1024 / kWave];
    if (failed(P)) return;
    const int per = (nb + 1023) / 1024;
    const int lo = threadIdx.x * per, hi = min(nb, lo + per);
    int s = 0;
    for (int k = lo; k < hi; ++k) s += P.bsum[k];
    int run = block_exclusive(s, red);
    for (int k = lo; k < hi; ++k) {
        const int v = P.bsum[k];
        P.bsum[k] = run;
        run += v;
    }
}

__global__ __launch_bounds__(kThreads) void tsdiff_scan_down_kernel(Params P) {
    __shared__ int red[kThreads / kWave];
    if (failed(P)) return;
    const long long base = (long long)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int v[kScanItems], s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = base + k <= P.ncells ? P.cnt[base + k] : 0;
        s += v[k];
    }
    int run = P.bsum[blockIdx.x] + block_exclusive(s, red);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k <= P.ncells) P.start[base + k] = run;
        run += v[k];
    }
}

__global__ __launch_bounds__(kThreads) void tsdiff_scatter_kernel(Params P) {
    if (failed(P)) return;
    const int pl = blockIdx.y;
    const long long lo = P.pr_off[P.p0 + pl], hi = P.pr_off[P.p0 + pl + 1];
    for (long long i = lo + (long long)blockIdx.x * kThreads + threadIdx.x; i < hi; i += (long long)gridDim.x * kThreads) {
        const int c = pred_cell(P, pl, i);
        const int pos = P.start[c] + atomicSub(&P.cnt[c], 1) - 1;
        P.ts_a[pos] = P.pr_ts[i];
    }
}

// lists the LDS tiles of every cell longer than kSmall, and the cells longer than one tile
__global__ __launch_bounds__(kThreads) void tsdiff_classify_kernel(Params P) {
    if (failed(P)) return;
    for (int c = blockIdx.x * kThreads + threadIdx.x; c < P.ncells; c += gridDim.x * kThreads) {
        const int n = P.start[c + 1] - P.start[c];
        if (n <= kSmall) continue;
        const int nt = (int)(((long long)n + kTile - 1) / kTile);
        const int slot = atomicAdd(&P.meta[0], nt);
        if (slot + nt > P.tile_cap) { atomicOr(P.status, kListOverflow); continue; }   // cannot happen: tile_cap >= n_pred / 17
        for (int k = 0; k < nt; ++k) P.tiles[slot + k] = make_int2(c, k);
        if (nt > 1) {
            const int b = atomicAdd(&P.meta[1], 1);
            if (b >= P.big_cap) { atomicOr(P.status, kListOverflow); continue; }
            P.big[b] = c;
        }
    }
}

__global__ __launch_bounds__(kThreads) void tsdiff_tile_sort_kernel(Params P) {
    __shared__ long long s[kTile];
    if (failed(P)) return;
    const int ntiles = min(*(volatile int *)&P.meta[0], P.tile_cap);
    for (int e = blockIdx.x; e < ntiles; e += gridDim.x) {
        const int2 ct = P.tiles[e];
        const int c0 = P.start[ct.x], n = P.start[ct.x + 1] - c0;
        const int lo = c0 + ct.y * kTile, m = min(kTile, n - ct.y * kTile);
        int w = 2;
        while (w < m) w <<= 1;
        for (int i = threadIdx.x; i < w; i += kThreads) s[i] = i < m ? (long long)P.ts_a[lo + i] : 0x7fffffffffffffffll;
        __syncthreads();
        for (int k = 2; k <= w; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < w; i += kThreads) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const long long a = s[i], b = s[ixj];
                        if ((a > b) == ((i & k) == 0)) { s[i] = b; s[ixj] = a; }
                    }
                }
                __syncthreads();
            }
        for (int i = threadIdx.x; i < m; i += kThreads) P.ts_a[lo + i] = s[i];
        __syncthreads();
    }
}

// merge pass q: sorted runs of kTile << q -> runs of twice that, ts_a -> ts_b for even q, back for odd q
__global__ __launch_bounds__(kThreads) void tsdiff_merge_kernel(Params P, int q) {
    if (failed(P)) return;
    const int nbig = min(*(volatile int *)&P.meta[1], P.big_cap);
    const int64_t *src = (q & 1) ? P.ts_b : P.ts_a;
    int64_t *dst = (q & 1) ? P.ts_a : P.ts_b;
    const long long w = (long long)kTile << q;
    for (int bi = 0; bi < nbig; ++bi) {
        const int c = P.big[bi];
        const int c0 = P.start[c], n = P.start[c + 1] - c0;
        if (q >= merge_passes(n)) continue;
        const int64_t *in = src + c0;
        int64_t *out = dst + c0;
        for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < n; j += (long long)gridDim.x * kThreads) {
            const long long a0 = j / (2 * w) * (2 * w), a1 = min(a0 + w, (long long)n), b1 = min(a0 + 2 * w, (long long)n);
            const long long v = in[j];
            long long lo, hi, rank_base;
            if (j < a1) {          // left run: elements of the right run strictly below v come first
                lo = a1; hi = b1;
                while (lo < hi) { const long long mid = (lo + hi) >> 1; if (in[mid] < v) lo = mid + 1; else hi = mid; }
                rank_base = j - a0 + (lo - a1);
            } else {               // right run: elements of the left run up to v come first
                lo = a0; hi = a1;
                while (lo < hi) { const long long mid = (lo + hi) >> 1; if (in[mid] <= v) lo = mid + 1; else hi = mid; }
                rank_base = j - a1 + (lo - a0);
            }
            out[a0 + rank_base] = v;
        }
    }
}

// grid (G, np): one lane per ground-truth event of pair p0 + blockIdx.y
__global__ __launch_bounds__(kThreads) void tsdiff_query_kernel(Params P) {
    if (failed(P)) return;
    const int pl = blockIdx.y, pair = P.p0 + pl;
    const long long lo = P.gt_off[pair], hi = P.gt_off[pair + 1];
    const double cap = 1e6 / P.fps[pair] / 10 * 3;
    long long S = 0, K = 0;
    for (long long i = lo + (long long)blockIdx.x * kThreads + threadIdx.x; i < hi; i += (long long)gridDim.x * kThreads) {
        const long long t = P.gt_ts[i];
        const int x = P.gt_x[i], y = P.gt_y[i], p = P.gt_p[i] == 1;
        const int xa = max(x - P.r, 0), xb = min(x + P.r + 1, P.W), ya = max(y - P.r, 0), yb = min(y + P.r + 1, P.H);
        long long best = 1000000;   // the reference starts from diff = 1e6
        for (int b = ya; b < yb; ++b) {
            const int row = ((pl * 2 + p) * P.H + b) * P.W;
            for (int a = xa; a < xb; ++a) {
                const int c0 = P.start[row + a], n = P.start[row + a + 1] - c0;
                if (n == 0) continue;
                if (n <= kSmall) {
                    for (int k = 0; k < n; ++k) best = min(best, absdiff(P.ts_a[c0 + k], t));
                } else {
                    const int64_t *v = (merge_passes(n) & 1) ? P.ts_b + c0 : P.ts_a + c0;
                    int l = 0, h = n;   // first element >= t
                    while (l < h) { const int mid = (l + h) >> 1; if (v[mid] < t) l = mid + 1; else h = mid; }
                    if (l < n) best = min(best, absdiff(v[l], t));
                    if (l > 0) best = min(best, absdiff(v[l - 1], t));
                }
            }
        }
        double d;
        if ((double)best > cap) { d = cap; ++K; }
        else { d = (double)best; S += best; }
        if (P.d_out) P.d_out[i] = d;
    }
    for (int o = 32; o; o >>= 1) { S += __shfl_xor(S, o); K += __shfl_xor(K, o); }
    if ((threadIdx.x & (kWave - 1)) == 0 && (S | K)) {
        atomicAdd(&P.acc[2 * pair], (unsigned long long)S);
        atomicAdd(&P.acc[2 * pair + 1], (unsigned long long)K);
    }
}

__global__ __launch_bounds__(kThreads) void tsdiff_finish_kernel(Params P) {
    if (failed(P)) return;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.pairs) return;
    P.stats_out[3 * i] = (int64_t)P.acc[2 * i];
    P.stats_out[3 * i + 1] = (int64_t)P.acc[2 * i + 1];
    P.stats_out[3 * i + 2] = P.gt_off[i + 1] - P.gt_off[i];
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    int chunk;
    long long ncells;
    long long nblocks;
    size_t acc, meta, cnt, start, bsum, ts_a, ts_b, tiles, big, total;
    int tile_cap, big_cap;
};

bool make_layout(int pairs, int H, int W, long long n_pred, Layout &L) {
    if (pairs <= 0 || H <= 0 || W <= 0 || H > 32767 || W > 32767 || n_pred < 0 || n_pred >= (1ll << 31)) return false;
    const long long cells_per_pair = 2ll * H * W;
    if (cells_per_pair >= (1ll << 30)) return false;
    long long chunk = kCellBudget / cells_per_pair;
    chunk = chunk < 1 ? 1 : (chunk > pairs ? pairs : chunk);
    chunk = chunk > 65535 ? 65535 : chunk;   // pairs of a chunk are grid rows
    L.chunk = (int)chunk;
    L.ncells = chunk * cells_per_pair;
    L.nblocks = (L.ncells + 1 + kScanBlock - 1) / kScanBlock;
    L.tile_cap = (int)(n_pred / (kSmall + 1) + 1);
    L.big_cap = (int)(n_pred / (kTile + 1) + 1);
    size_t o = 0;
    L.acc = o;   o += align256((size_t)pairs * 2 * 8);
    L.meta = o;  o += 256;
    L.cnt = o;   o += align256((size_t)(L.ncells + 1) * 4);
    L.start = o; o += align256((size_t)(L.ncells + 1) * 4);
    L.bsum = o;  o += align256((size_t)L.nblocks * 4);
    L.ts_a = o;  o += align256((size_t)n_pred * 8);
    L.ts_b = o;  o += n_pred > kTile ? align256((size_t)n_pred * 8) : 0;
    L.tiles = o; o += align256((size_t)L.tile_cap * 8);
    L.big = o;   o += align256((size_t)L.big_cap * 4);
    L.total = o;
    return true;
}

unsigned grid_for(long long events, int pairs) {   // blocks per pair row for an even spread
    const long long per = (events / pairs + kThreads - 1) / kThreads;
    return (unsigned)(per < 1 ? 1 : (per > 1024 ? 1024 : per));
}

}  // namespace
}  // namespace v2ce

using namespace v2ce;

extern "C" size_t v2ce_tsdiff_workspace_bytes(int pairs, int H, int W, int64_t n_pred) {
    Layout L;
    return make_layout(pairs, H, W, n_pred, L) ? L.total : 0;
}

extern "C" int v2ce_tsdiff(const int64_t *gt_ts, const int16_t *gt_x, const int16_t *gt_y, const int8_t *gt_p,
                           const int64_t *gt_offsets, int64_t n_gt, const int64_t *pred_ts, const int16_t *pred_x,
                           const int16_t *pred_y, const int8_t *pred_p, const int64_t *pred_offsets, int64_t n_pred,
                           const double *fps, int pairs, int H, int W, int search_range, double *per_event_d,
                           int64_t *pair_stats, int32_t *status, void *workspace, size_t workspace_bytes,
                           v2ce_stream_t stream) {
    clear_error();
    Layout L;
    V2CE_REQUIRE(search_range >= 0, V2CE_ERR_BAD_ARG, "v2ce_tsdiff: search_range < 0");
    V2CE_REQUIRE(n_gt >= 0 && n_gt < (1ll << 31), V2CE_ERR_BAD_ARG, "v2ce_tsdiff: n_gt outside [0, 2^31)");
    V2CE_REQUIRE(make_layout(pairs, H, W, n_pred, L), V2CE_ERR_BAD_ARG,
                 "v2ce_tsdiff: needs pairs > 0, 0 < H, W <= 32767, 2*H*W < 2^30 and n_pred in [0, 2^31)");
    V2CE_REQUIRE(gt_offsets && pred_offsets && fps && pair_stats && status && workspace, V2CE_ERR_BAD_ARG,
                 "v2ce_tsdiff: null pointer");
    V2CE_REQUIRE(n_gt == 0 || (gt_ts && gt_x && gt_y && gt_p), V2CE_ERR_BAD_ARG, "v2ce_tsdiff: null GT array");
    V2CE_REQUIRE(n_pred == 0 || (pred_ts && pred_x && pred_y && pred_p), V2CE_ERR_BAD_ARG,
                 "v2ce_tsdiff: null prediction array");
    V2CE_REQUIRE(workspace_bytes >= L.total, V2CE_ERR_WORKSPACE, "v2ce_tsdiff: workspace too small (%zu < %zu)",
                 workspace_bytes, L.total);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    Params P{};
    P.gt_ts = gt_ts; P.gt_x = gt_x; P.gt_y = gt_y; P.gt_p = gt_p; P.gt_off = gt_offsets; P.n_gt = n_gt;
    P.pr_ts = pred_ts; P.pr_x = pred_x; P.pr_y = pred_y; P.pr_p = pred_p; P.pr_off = pred_offsets; P.n_pred = n_pred;
    P.fps = fps; P.pairs = pairs; P.H = H; P.W = W;
    P.r = search_range > 65535 ? 65535 : search_range;   // beyond the sensor either way; keeps x + r + 1 in int
    P.d_out = per_event_d; P.stats_out = pair_stats; P.status = status;
    P.acc = reinterpret_cast<unsigned long long *>(ws + L.acc);
    P.meta = reinterpret_cast<int *>(ws + L.meta);
    P.cnt = reinterpret_cast<int *>(ws + L.cnt);
    P.start = reinterpret_cast<int *>(ws + L.start);
    P.bsum = reinterpret_cast<int *>(ws + L.bsum);
    P.ts_a = reinterpret_cast<int64_t *>(ws + L.ts_a);
    P.ts_b = n_pred > kTile ? reinterpret_cast<int64_t *>(ws + L.ts_b) : nullptr;
    P.tiles = reinterpret_cast<int2 *>(ws + L.tiles);
    P.big = reinterpret_cast<int *>(ws + L.big);
    P.tile_cap = L.tile_cap; P.big_cap = L.big_cap;

    V2CE_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    {
        long long m = n_gt > n_pred ? n_gt : n_pred;
        m = m > 2ll * pairs + 1 ? m : 2ll * pairs + 1;
        const long long g = (m + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(tsdiff_validate_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(kThreads), 0, st, P);
        V2CE_HIP_CHECK(hipGetLastError());
    }
    int passes = 0;   // enough for the longest possible cell: all of n_pred
    for (long long nt = (n_pred + kTile - 1) / kTile; (1ll << passes) < nt; ++passes) {}
    const unsigned gp = grid_for(n_pred, pairs), gg = grid_for(n_gt, pairs);
    for (int p0 = 0; p0 < pairs; p0 += L.chunk) {
        P.p0 = p0;
        P.np = pairs - p0 < L.chunk ? pairs - p0 : L.chunk;
        P.ncells = (int)((long long)P.np * 2 * H * W);
        const unsigned cell_blocks = (unsigned)((P.ncells + kThreads) / kThreads);
        const unsigned scan_blocks = (unsigned)((P.ncells + 1 + kScanBlock - 1) / kScanBlock);
        hipLaunchKernelGGL(tsdiff_zero_kernel, dim3(cell_blocks < 4096 ? cell_blocks : 4096), dim3(kThreads), 0, st, P);
        if (n_pred > 0) hipLaunchKernelGGL(tsdiff_count_kernel, dim3(gp, P.np), dim3(kThreads), 0, st, P);
        hipLaunchKernelGGL(tsdiff_scan_reduce_kernel, dim3(scan_blocks), dim3(kThreads), 0, st, P);
        hipLaunchKernelGGL(tsdiff_scan_top_kernel, dim3(1), dim3(1024), 0, st, P, (int)scan_blocks);
        hipLaunchKernelGGL(tsdiff_scan_down_kernel, dim3(scan_blocks), dim3(kThreads), 0, st, P);
        if (n_pred > 0) {
            hipLaunchKernelGGL(tsdiff_scatter_kernel, dim3(gp, P.np), dim3(kThreads), 0, st, P);
            hipLaunchKernelGGL(tsdiff_classify_kernel, dim3(cell_blocks < 4096 ? cell_blocks : 4096), dim3(kThreads), 0, st, P);
        }
        if (n_pred > kSmall) hipLaunchKernelGGL(tsdiff_tile_sort_kernel, dim3(1024), dim3(kThreads), 0, st, P);
        for (int q = 0; q < passes; ++q) hipLaunchKernelGGL(tsdiff_merge_kernel, dim3(1024), dim3(kThreads), 0, st, P, q);
        if (n_gt > 0) hipLaunchKernelGGL(tsdiff_query_kernel, dim3(gg, P.np), dim3(kThreads), 0, st, P);
        V2CE_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(tsdiff_finish_kernel, dim3((unsigned)((pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, P);
    V2CE_HIP_CHECK(hipGetLastError());
    return V2CE_OK;
}
