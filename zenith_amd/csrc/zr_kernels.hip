// zr_kernels.hip — the MI355X (gfx950) draw path.
//
//   k_setup_bin  one launch, one 1024-thread workgroup per CU (fewer for small
//                draws), no grid barrier: vertex stage, clip (mesh program),
//                viewport, 8-bit sub-pixel snap, facing/cull, orientation,
//                top-left biases, clipped pixel bbox -> 32-B compact record (64-B
//                full record for large primitives); an LDS histogram of the
//                workgroup's (tile, primitive) pairs; returning atomics on the
//                per-tile counters give the workgroup's offsets in each tile's
//                fixed slab of the bin buffer; scatter of (primitive | cost
//                class) entries into the slabs.  Workgroups never wait for each
//                other, so nothing assumes co-residency.
//   k_tile       one 256- or 512-thread workgroup per 32x32 tile: LDS-resident
//                64-bit visibility keys (depth | primitive sequence) updated with
//                ds_min_u64 -- lane per primitive for small ones (cost-sorted
//                64-lane chunks), wave per primitive for large ones -- then a
//                resolve that shades each pixel's winner once, encodes to the
//                attachment format and writes colour + depth with coalesced
//                stores.  The attachment CLEAR is fused into the resolve.
//   k_route      partitioned multi-GPU setup: route primitives to the ranks
//                owning the tile rows they touch.
//   k_clear      a render pass without draws.
//
// Coverage/depth arithmetic is exact integer + explicitly ordered float math,
// bit-identical to the in-order CPU oracle (oracle/zr_oracle.c).
//
// One device translation unit in several files.  This file holds the build knobs,
// the tuning constants, the sRGB table, k_clear and the launchers; the passes are
// in the headers included below, each of which needs what precedes it:
//   zr_order.h       host + device index arithmetic (XCD tile order, tile jobs,
//                    tile_order items, cost class, lane space of a segment)
//   zr_dev_common.h  kernarg_params, index fetch, visibility keys, edge and
//                    depth-plane evaluation
//   zr_setup_geom.h  primitive assembly and setup geometry, records, owned tiles
//   zr_route.h       k_route
//   zr_schedule.h    build_tile_schedule, build_job_schedule
//   zr_setup_bin.h   pool runs, k_setup_bin and its phases
//   zr_raster.h      record decode, raster_prim (wave path), raster_lane (lane walk)
//   zr_resolve.h     store_color, shading, record table, resolve_pixels, resolve_tile
//   zr_tile_segment.h  k_tile's LDS carve-up and its per-segment phases
//   zr_tile.h        k_tile and its other phases
#include <hip/hip_runtime.h>

#include <type_traits>

#include "zr_internal.h"
#include "zr_order.h"
#include "zr_shading.h"

namespace zr {

// Diagnostic builds only (tools/build_variant.sh); production builds keep both 0.
#ifndef ZR_TILE_WORK_STATS
// Per-tile lane-walk steps and wave-path sweeps in the debug stamps (the counting
// code costs k_tile 5 VGPRs, one wave per SIMD at 512 threads).
#define ZR_TILE_WORK_STATS 0
#endif
#ifndef ZR_LANE_STEP
#define ZR_LANE_STEP 4       // pixels of a row per lane-walk step (2 or 4; 4: C3 tile pass -6.6 us, C1 -3)
#endif
#ifndef ZR_LARGE_LANES
#define ZR_LARGE_LANES 1     // 0: every large primitive takes k_tile's wave path; 2: the last cost bucket's too (A/B)
#endif
#ifndef ZR_TAB
#define ZR_TAB 1
#endif
#ifndef ZR_RESOLVE_DEDUP512
#define ZR_RESOLVE_DEDUP512 0  // 1: 512-thread tiles resolve through resolve_tile (each distinct winner fetched once per tile)
#endif
#ifndef ZR_TILE_DEBUG
#define ZR_TILE_DEBUG 0      // 1: k_tile honours the ZR_DEBUG timing switches and stamps
                             // (the checks cost the production kernel SGPRs)
#endif

// k_tile tuning constants (DESIGN.md §4 has the measurements behind each).
constexpr uint32_t kTileWgs = 8;  // 256-thread k_tile workgroups per CU the register budget is sized for
constexpr int kLaneStep = ZR_LANE_STEP;
// (8 pixels per step was measured slower and has no parity run: not a build option)
static_assert(kLaneStep == 2 || kLaneStep == 4, "lane walk: 2 or 4 pixels per step");
constexpr uint32_t kResolveBatch = 2;  // pixels per thread whose gathers are in flight together in the resolve

__constant__ float c_srgbT[255] = ZR_SRGB_THRESHOLDS_INIT;

}  // namespace zr

#include "zr_dev_common.h"
#include "zr_setup_geom.h"
#include "zr_route.h"
#include "zr_schedule.h"
#include "zr_setup_bin.h"
#include "zr_raster.h"
#include "zr_resolve.h"
#include "zr_tile_segment.h"
#include "zr_tile.h"

namespace zr {

__global__ __launch_bounds__(kTileThreads) void k_clear(DrawParams P) {
    const uint32_t t = blockIdx.x;
    uint32_t tx, ty;
    shard_tile_xy(shard_geom(P), t, tx, ty);
    const int x0 = (int)tx * kTile, y0 = (int)ty * kTile;
    const float c[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < kTilePixels; i += kTileThreads) {
        const int px = x0 + (i & (kTile - 1)), py = y0 + (i >> kTileShift);
        if (px < P.ra_x0 || px > P.ra_x1 || py < P.ra_y0 || py > P.ra_y1) continue;
        if (P.color_bpp && P.clear_color_enable) store_color(P, px, py, false, c, c_srgbT);
        if (P.depth && P.clear_depth_enable) P.depth[(size_t)py * P.fb_w + px] = P.clear_depth;
    }
}

// ---------------------------------------------------------------- launchers

static inline uint32_t blocks_for(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

const void* setup_bin_kernel(uint32_t batch, bool mesh) {
    if (mesh) return reinterpret_cast<const void*>(&k_setup_bin<1, true>);
    switch (batch) {
    case 1: return reinterpret_cast<const void*>(&k_setup_bin<1, false>);
    case 2: return reinterpret_cast<const void*>(&k_setup_bin<2, false>);
    default: return reinterpret_cast<const void*>(&k_setup_bin<4, false>);
    }
}

void launch_setup_bin(const DrawParams& p, void* stream) {
    const size_t lds = setup_bin_lds_bytes(p.ntiles, p.bbox_lds, p.bin_stage);
    const hipStream_t s = (hipStream_t)stream;
    if (p.program == kProgMesh) {  // batch 1: the clip path is heavy
        hipLaunchKernelGGL((k_setup_bin<1, true>), dim3(p.setup_wgs), dim3(kSetupThreads), lds, s, p);
        return;
    }
    switch (p.setup_batch) {
    case 1: hipLaunchKernelGGL((k_setup_bin<1, false>), dim3(p.setup_wgs), dim3(kSetupThreads), lds, s, p); break;
    case 2: hipLaunchKernelGGL((k_setup_bin<2, false>), dim3(p.setup_wgs), dim3(kSetupThreads), lds, s, p); break;
    default: hipLaunchKernelGGL((k_setup_bin<4, false>), dim3(p.setup_wgs), dim3(kSetupThreads), lds, s, p); break;
    }
}

template <int PROG, int MODE, int NT, int TS>
static void launch_tile_pmt(const DrawParams& p, hipStream_t s, bool initd) {
    const uint32_t blocks = p.ntiles + (p.job_entries ? p.job_pad : 0u);  // (tile jobs: part blocks first)
    if constexpr (MODE == kDepthLastWins) {  // (initial depths: last-wins modes only)
        if (initd) {
            hipLaunchKernelGGL((k_tile<PROG, MODE, true, NT, TS>), dim3(blocks), dim3(NT), 0, s, p);
            return;
        }
    }
    hipLaunchKernelGGL((k_tile<PROG, MODE, false, NT, TS>), dim3(blocks), dim3(NT), 0, s, p);
}

// Tile-edge instances (tile_variant_built): every program and mode at 32 px, with
// 256 or 512 threads (tile_threads_for); 16- and 64-px tiles (256 / 512 or 1024
// threads) for the flat and Blinn-Phong programs under the depth-writing modes, the draws
// tile_shift_for picks them for (dense soups, crowded scenes).
template <int PROG, int MODE>
static void launch_tile_pm(const DrawParams& p, hipStream_t s, bool initd) {
    if constexpr (tile_variant_built(PROG, MODE)) {
        if (p.tile_shift == 6u)
            return p.tile_threads == 1024u ? launch_tile_pmt<PROG, MODE, 1024, 6>(p, s, initd)
                                           : launch_tile_pmt<PROG, MODE, 512, 6>(p, s, initd);
        if (p.tile_shift == 4u) return launch_tile_pmt<PROG, MODE, kTileThreads, 4>(p, s, initd);
    }
    switch (p.tile_threads) {
    case 512: launch_tile_pmt<PROG, MODE, 512, kTileShift>(p, s, initd); break;
    default: launch_tile_pmt<PROG, MODE, kTileThreads, kTileShift>(p, s, initd); break;
    }
}

template <int PROG>
static void launch_tile_p(const DrawParams& p, hipStream_t s, bool initd) {
    switch (p.depth_mode) {
    case kDepthMinStrict: launch_tile_pm<PROG, kDepthMinStrict>(p, s, false); break;
    case kDepthMinNonStrict: launch_tile_pm<PROG, kDepthMinNonStrict>(p, s, false); break;
    case kDepthMaxStrict: launch_tile_pm<PROG, kDepthMaxStrict>(p, s, false); break;
    case kDepthMaxNonStrict: launch_tile_pm<PROG, kDepthMaxNonStrict>(p, s, false); break;
    default: launch_tile_pm<PROG, kDepthLastWins>(p, s, initd); break;
    }
}

void launch_tile(const DrawParams& p, void* stream) {
    if (p.ntiles == 0) return;
    const bool initd = p.depth_mode == kDepthLastWins && p.depth != nullptr && p.depth_op != 7;
    hipStream_t s = (hipStream_t)stream;
    switch (p.program) {
    case kProgTriangle: launch_tile_p<kProgTriangle>(p, s, initd); break;
    case kProgFlat: launch_tile_p<kProgFlat>(p, s, initd); break;
    case kProgMesh: launch_tile_p<kProgMesh>(p, s, initd); break;
    default: launch_tile_p<kProgBlinn>(p, s, initd); break;
    }
}

void launch_route(const DrawParams& p, void* stream) {
    hipLaunchKernelGGL(k_route, dim3(p.route_chunks), dim3(kRouteThreads), 0, (hipStream_t)stream, p);
}

void launch_clear(const DrawParams& p, void* stream) {
    if (p.ntiles == 0) return;
    hipLaunchKernelGGL(k_clear, dim3(p.ntiles), dim3(kTileThreads), 0, (hipStream_t)stream, p);
}

}  // namespace zr
