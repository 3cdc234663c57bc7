// zr_order.h — the index arithmetic of the draw path that decides which block,
// wave or lane touches which tile, job or list entry: the XCD tile order and its
// inverse, the job count of a tile, the tile_order item encoding, the cost class
// of a bin entry, and the lane space of a sorted segment.  Pure functions of their
// arguments (no intrinsics, no thread indices), callable from host and device:
// the kernels call them, tests/sanitize/order_host.cpp checks them off the GPU.
#pragma once
#include <hip/hip_vector_types.h>  // (types only: DrawParams has float4 / uint2 pointers)
#include <math.h>

#include "zr_internal.h"

// Build knobs of the arithmetic below (tools/build_variant.sh).
#ifndef ZR_XCD_TILES
#define ZR_XCD_TILES 8       // tiles per XCD run (xcd_tile); 0 or 1: blockIdx order
#endif
#ifndef ZR_BIG_LANES
#define ZR_BIG_LANES 8
#endif
#ifndef ZR_MID_LANES
#define ZR_MID_LANES 4
#endif
#ifndef ZR_MID_BUCKET
#define ZR_MID_BUCKET 24
#endif

namespace zr {

constexpr uint32_t kBigLanes = ZR_BIG_LANES;    // lanes per entry at least, for the last cost bucket (127+ pair steps, ~253+ px)
constexpr uint32_t kMidLanes = ZR_MID_LANES;    // lanes per entry at least, for buckets kMidBucket..62
constexpr uint32_t kMidBucket = ZR_MID_BUCKET;  // first bucket of the middle run: 49+ pair steps (~97+ px of bbox ∩ tile)

__host__ __device__ inline uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__host__ __device__ inline uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
// floor(log2(v)) of v >= 1.
__host__ __device__ inline uint32_t log2_floor(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

// XCD-aware tile order.  Blocks are dealt round-robin over the 8 XCDs, so blocks b
// and b + 8 share an XCD and its L2 (MI355X_MICROARCH.md; affinity only, nothing
// depends on it).  Runs of ZR_XCD_TILES consecutive (row-major) tiles go to one
// XCD, the runs round-robin over the XCDs: a primitive straddling two tiles of a
// run has its record and vertices read through one L2, and a dense screen region
// still spreads over every XCD.  A bijection: blocks past the last whole round of
// runs keep their own tile.
__host__ __device__ inline uint32_t xcd_tile(uint32_t b, uint32_t n) {
    constexpr uint32_t K = ZR_XCD_TILES;
    if (K <= 1u || b >= n / (8u * K) * (8u * K)) return b;
    const uint32_t x = b & 7u, l = b >> 3;
    return ((l / K) * 8u + x) * K + l % K;
}

// The inverse of xcd_tile: the block that takes tile t in that order.
__host__ __device__ inline uint32_t xcd_block(uint32_t t, uint32_t n) {
    constexpr uint32_t K = ZR_XCD_TILES;
    if (K <= 1u || t >= n / (8u * K) * (8u * K)) return t;
    const uint32_t R = t / K, o = t - R * K;
    return ((R >> 3) * K + o) * 8u + (R & 7u);
}

// Jobs of a tile (DrawParams::job_entries, build_job_schedule): a list of `count`
// entries longer than J that takes no record scan is K = ceil(count / J) jobs,
// else one.  k_setup_bin's last workgroup and k_tile derive K from the same count
// and run word.
__host__ __device__ inline uint32_t tile_jobs(uint32_t count, uint32_t run_word, uint32_t J) {
    return (J && !(run_word & kRunDropped) && count > J) ? (count + J - 1u) / J : 1u;
}

// A tile_order item: tile | job part << kJobTileBits (tiles < kMaxTilesPerPass,
// parts < 2^18, so none equals kJobNone, the item of a job grid's spare block).
__host__ __device__ inline uint32_t job_item(uint32_t tile, uint32_t part) { return tile | (part << kJobTileBits); }
__host__ __device__ inline uint32_t item_tile(uint32_t item) { return item & kJobTileMask; }
__host__ __device__ inline uint32_t item_part(uint32_t item) { return item >> kJobTileBits; }

// Cost class of a bin entry: the lane walk's pair steps over the inclusive pixel
// rectangle bbox ∩ tile, ceil(w / 2) per row (sorting by steps instead of area: C3
// tile pass -1 %, C2 -0.8 %), as min((steps - 1) >> 1, kSortBuckets - 1).
__host__ __device__ inline uint32_t cost_bucket(int cx0, int cx1, int cy0, int cy1) {
    const uint32_t steps = (uint32_t)(((cx1 - cx0 + 2) >> 1) * (cy1 - cy0 + 1));
    return umin((steps - 1u) >> 1, kSortBuckets - 1u);
}

// Lane space of a sorted segment of n entries rasterized by NT threads (k_tile's
// chunk loop).  A sparse segment (fewer entries than lanes) gives each entry
// kl = 2^ksh_s lanes, which split its bbox rows.  Entries of the last bucket (127+
// pair steps, ~253+ pixels; sorted positions [off63, n)) get at least kBigLanes
// lanes: one lane would walk up to 1024 steps and hold its whole chunk (and the
// tile) for that long.  Likewise buckets from kMidBucket up (positions [offm,
// off63); bbox ∩ tile > 4 * kMidBucket px) get at least kMidLanes lanes.  Three
// runs of the sorted segment, each a fixed number of lanes per entry, laid end to
// end; chunks are 64 lanes of this space.
// (2 lanes from 129 px, 4 from 253: C3 tile pass 262 -> 219 us, cerberus 68
// -> 60 us, C1 / C2 within noise; 4 lanes from 97 px, 8 from 253: C1 58 ->
// 51 us, cerberus 60 -> 57, C3 219 -> 226, C2 equal -- the default.
// Gating it on the middle run's length lost the gains: a few mid-size
// entries already make the chunk that ends the tile.)
struct LaneSpace {
    uint32_t n, offm, off63;
    uint32_t ksh_s, ksh_m, ksh_b;  // log2 lanes per entry: first, middle, last run
    uint32_t lsp_s, lsp_m;         // lane-space slot where the middle / the last run starts
    uint32_t chunks;               // 64-lane chunks covering the whole space
};

__host__ __device__ inline LaneSpace lane_space(uint32_t n, uint32_t NT, uint32_t offm, uint32_t off63) {
    const uint32_t kl = umin(8u, umax(1u, NT / umax(n, 1u)));
    const uint32_t ksh_s = log2_floor(kl);  // lanes per entry: 1, 2, 4 or 8
    const uint32_t ksh_b = umax(ksh_s, log2_floor(kBigLanes));
    const uint32_t ksh_m = umax(ksh_s, log2_floor(kMidLanes));
    const uint32_t lsp_s = offm << ksh_s;                      // lane space of buckets < kMidBucket
    const uint32_t lsp_m = lsp_s + ((off63 - offm) << ksh_m);  // ... and up to the last bucket
    const uint32_t lanes_all = lsp_m + ((n - off63) << ksh_b);
    return LaneSpace{n, offm, off63, ksh_s, ksh_m, ksh_b, lsp_s, lsp_m, (lanes_all + 63u) / 64u};
}

// Lane-space slot g -> sorted entry j (>= n: none), the lane's index among the
// entry's 2^ksh lanes, and whether the entry is in the last run.
struct LaneSlot {
    uint32_t j;
    int sub;
    uint32_t ksh;
    bool last;
};

__host__ __device__ inline LaneSlot lane_slot(const LaneSpace& s, uint32_t g) {
    // (the fields as values: a choice between them is then a select, not a
    // load through a chosen address)
    const uint32_t offm = s.offm, off63 = s.off63, ksh_s = s.ksh_s, ksh_m = s.ksh_m, ksh_b = s.ksh_b;
    const uint32_t lsp_s = s.lsp_s, lsp_m = s.lsp_m;
    const bool gb = g >= lsp_m, gm = g >= lsp_s;
    const uint32_t ksh = gb ? ksh_b : gm ? ksh_m : ksh_s;
    const uint32_t g0 = gb ? g - lsp_m : gm ? g - lsp_s : g;  // slot within its run
    const uint32_t j = (gb ? off63 : gm ? offm : 0u) + (g0 >> ksh);
    const int sub = (int)(g0 & ((1u << ksh) - 1u));
    return LaneSlot{j, sub, ksh, gb};
}

}  // namespace zr
