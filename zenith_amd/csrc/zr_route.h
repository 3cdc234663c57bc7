// zr_route.h — k_route, step 1 of the partitioned setup.
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_setup_geom.h"

namespace zr {

// ----------------------------------------------------------------- k_route
//
// Partitioned setup, step 1 (tile-row shards): one pass over this
// rank's primitive range [route_lo, route_hi).  Thread t of workgroup c sets up
// primitive route_lo + c * kRouteChunk + t (the same setup geometry k_setup_bin
// computes) and appends its RouteEntry -- compact record, bbox, draw id -- to the
// block of every rank owning a tile row the bbox touches (ty % G == rank).  A
// workgroup reserves its run in a block with one returning atomic per
// destination on the block header's `total` (zero before every route: this
// rank's previous records-mode setup on the scratch set, or the runtime, resets
// it), so runs land in any order -- the receiver keys records by the draw id,
// so block order carries no meaning.  Entries past a block's capacity are
// dropped; the receiver reads count = min(total, capacity) and sees the overflow.
__device__ __forceinline__ uint32_t dest_mask(const DrawParams& P, const PrimGeom& g) {
    const uint32_t G = P.shard_count;
    const uint32_t tsh = P.tile_shift;  // (kTileShift: shards bin 32-px tiles)
    const int ty0 = g.py0 >> tsh, ty1 = g.py1 >> tsh;
    const int tx0 = g.px0 >> tsh, tx1 = g.px1 >> tsh;
    const uint32_t all = G >= 32u ? 0xFFFFFFFFu : (1u << G) - 1u;
    const int tyf = min(ty1, (int)P.full_rows - 1);  // round-robin rows: owner ty % G
    uint32_t m = 0;
    if (tyf >= ty0) m = (uint32_t)(tyf - ty0) + 1u >= G ? all : 0u;
    if (!m)
        for (int ty = ty0; ty <= tyf; ++ty) m |= 1u << ((uint32_t)ty % G);
    if (ty1 >= (int)P.full_rows) {  // leftover rows: the owners of the bbox's columns, a contiguous rank range per row
        const uint64_t n = (uint64_t)(P.tiles_y - P.full_rows) * P.tiles_x;
        for (int ty = max(ty0, (int)P.full_rows); ty <= ty1; ++ty) {
            const uint64_t i0 = (uint64_t)(ty - (int)P.full_rows) * P.tiles_x;
            const uint32_t ra = (uint32_t)((i0 + (uint64_t)tx0) * G / n), rb = (uint32_t)((i0 + (uint64_t)tx1) * G / n);
            m |= (rb >= 31u ? 0xFFFFFFFFu : (2u << rb) - 1u) & ~((1u << ra) - 1u);
        }
    }
    return m & all;
}

__global__ __launch_bounds__(kRouteThreads) void k_route(DrawParams P) {
    constexpr uint32_t kWaves = kRouteThreads / 64;
    static_assert(kRouteChunk == kRouteThreads, "k_route: one primitive per thread");
    __shared__ uint32_t s_off[kWaves][kMaxShards];  // entries per (wave, destination) -> run offsets
    __shared__ uint32_t s_base[kMaxShards];
    const uint32_t G = P.shard_count, c = blockIdx.x, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t gid = P.route_lo + c * kRouteChunk + tid;
    PrimIn in;
    in.ok = gid < P.route_hi;
    if (in.ok) fetch_indices_gid(P, gid, in);
    fetch_positions(P, in);
    int ndropped = 0;
    PrimGeom g;
    const uint32_t m = prim_geometry(P, in, g, ndropped) ? dest_mask(P, g) : 0u;
    BBox box{kEmptyBox, 0u};
    TriCompact rec;
    if (m) rec = make_compact(g, box);
    for (uint32_t d = 0; d < G; ++d) {
        const uint32_t n = (uint32_t)__popcll(__ballot((m >> d) & 1u));
        if (lane == 0) s_off[wave][d] = n;
    }
    __syncthreads();
    const uint64_t block = route_block_bytes(P.route_cap);
    if (tid < G) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < kWaves; ++i) {
            const uint32_t n = s_off[i][tid];
            s_off[i][tid] = run;
            run += n;
        }
        uint32_t* total = &reinterpret_cast<RouteHeader*>(P.route_out + (size_t)tid * block)->total;
        s_base[tid] = run ? atomicAdd(total, run) : 0u;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t d = 0; d < G; ++d) {
        const bool on = (m >> d) & 1u;
        const unsigned long long b = __ballot(on);
        const uint32_t k = s_base[d] + s_off[wave][d] + (uint32_t)__popcll(b & below);
        if (on && k < P.route_cap) {
            int4* e = reinterpret_cast<int4*>(P.route_out + (size_t)d * block + sizeof(RouteHeader) + (size_t)k * sizeof(RouteEntry));
            const int4* q = reinterpret_cast<const int4*>(&rec);
            e[0] = q[0];
            e[1] = q[1];
            e[2] = make_int4((int)box.bb0, (int)box.bb1, (int)gid, 0);
        }
    }
}

}  // namespace zr
