// ldati_const.h -- the constants of LDATI that its kernels (ldati.hip) and its host-side planning (ldati_plan.h) share.
#pragma once

#include <cstddef>

namespace v2ce {
namespace {

constexpr int kTilePix = 2048;        // pixels of one polarity plane per tile
constexpr int kLocalBits = 11;        // log2(kTilePix)
constexpr int kCountThreads = 512;
constexpr int kMaxTiles = 512;        // tiles per frame (both polarities) the bucket sort indexes
constexpr int kMaxNB = 512;           // coarse buckets per segment
constexpr int kMaxShift = 8;          // log2 of the widest coarse bucket
constexpr int kMaxSpanKeys = 128;     // timestamps a sort group spans at most (its histogram has 4x as many bins)
constexpr int kSmallGroupSpanKeys = 256;   // ... in the small-group regime (make_plan; measured 128 / 256 / 512: e2e sort 94 / 89 / 116 us)
constexpr int kCapTile = 15360;       // events of one (tile, bin) the tile pass can hold in LDS
#ifndef V2CE_SPARSE_CAP               // (diagnostic builds: tools/sparse_cap_ab.sh)
#define V2CE_SPARSE_CAP 8192
#endif
#ifndef V2CE_SPARSE_WAVES
#define V2CE_SPARSE_WAVES 1
#endif
constexpr int kSparseCap = V2CE_SPARSE_CAP;      // events of one tile over all nine bins the sparse tile kernel holds
constexpr int kSparseThreads = 512;
constexpr size_t kSparseLds = (size_t)(2 * kSparseCap + kSparseThreads * 5 + 34) * 4 + 9 * 8 + (kSparseThreads / 64) * 10 * 4;
constexpr int kSlopeM = 31;            // slope table (g_slope_tab): |count difference| <= kSlopeM, count <= kSlopeM; else computed
constexpr int kSlopeTab = (2 * kSlopeM + 1) * (kSlopeM + 1);
// sort workgroups: 256 threads (dense segments) or 128 (make_plan)

}  // namespace
}  // namespace v2ce
