// zr_setup_bin.h — k_setup_bin and its phases: the kernel at the end
// of the file reads top to bottom as the pass, each phase a function above it.
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_order.h"
#include "zr_schedule.h"
#include "zr_setup_geom.h"

namespace zr {

// ----------------------------------------------------------- k_setup_bin
//
// One launch, one 1024-thread workgroup per CU (fewer for small draws), no grid
// barrier (workgroups never wait for each other, so nothing assumes they are
// co-resident):
//   phase 1  vertex stage + setup in units of 64 * KB * rounds primitives, one
//            wave per unit (units assigned statically); records and tile bboxes
//            to HBM (bboxes also to LDS when they fit), pairs counted in an LDS
//            histogram of all tiles
//   phase 2  the histogram is added into the global per-tile counters with
//            returning atomics (a wave's adds to consecutive tiles leave L2 as
//            64-B requests); the value returned is this workgroup's offset inside
//            the tile's list
//   phase 4  scatter the workgroup's (tile, primitive) pairs straight into the
//            tile's slab: tile t's list starts at bins[t * slab], so a list
//            start needs no scan of the totals (the round-1 design's grid
//            barrier + phase 3 scan cost ~6 us of a C2 frame).  A workgroup's
//            pairs that do not fit the rest of the slab go to a pool run
//            (pool_run); a run the pool cannot hold is dropped and counted:
//            k_tile rasterizes that tile exactly by scanning every record's
//            bbox, and the runtime grows the bin buffer at the next sync point
//            (DESIGN.md §4).
// Order inside a tile's list is arbitrary (whatever order the atomics returned),
// which is free: visibility keys carry the primitive sequence (k_tile).  The
// counters return to zero in k_tile, so a draw needs no memset.
#define ZR_STAMP(i)                                                                         \
    do {                                                                                    \
        if ((P.debug & kDebugStamps) && tid == 0) P.dbg_ts[w * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)

// Phase 2's overflow run (DrawParams::runs): this workgroup's c pairs for tile t,
// reserved at offset o (ov: the count the atomic returned) of the tile's list, do not fit the rest of its slab; they
// go to the pool.  The run takes slot w (this workgroup) of t's run table and an
// offset inside the workgroup's pool allocation (an LDS counter, s_pool[0]); the
// allocation itself is one atomic per workgroup after the tile loop
// (pool_commit), which turns the returned kPoolPending | offset into the run's
// bin position.  No returning global atomic per run: one per run on the pool
// counter queued the clustered c2x scene's ~31k runs on that address (setup
// 772 us), and a slot counter per tile cost cerberus' ~100 runs ~4 us of setup.
// Returns kDropCursor for a workgroup beyond the run table (run_cap).
constexpr uint32_t kPoolPending = 0x40000000u;
__device__ __noinline__ uint32_t pool_run(const DrawParams& P, uint32_t t, uint32_t ov, uint32_t c, uint32_t* s_pool,
                                          uint32_t w) {
    if (!(ov & kCountRuns)) atomicOr(&P.tile_counts[t], kCountRuns);  // (the first run of the tile, as far as this workgroup saw)
    const uint32_t o = ov & ~kCountRuns;
    if (o < P.slab) atomicOr(&P.run_counts[t], kRunFill | (o << kRunFillShift));  // the slab holds [0, o) of the list
    if (w >= P.run_cap) {
        atomicOr(&P.run_counts[t], kRunDropped);
        return kDropCursor;
    }
    P.runs[(size_t)t * P.run_cap + w].y = c;  // (the position once the workgroup's allocation is known)
    atomicAdd(&s_pool[1], 1u);
    return kPoolPending | atomicAdd(&s_pool[0], c);
}

// After phase 2's tile loop: the workgroup's pool runs take one allocation of
// s_pool[0] entries from its sub-pool (pool_subs); each pending cursor becomes its
// run's position, or kDropCursor (and the tile's kRunDropped) when the sub-pool is
// full.
// The pool is pool_subs regions of pool_cap / subs entries (the remainder unused),
// region k the bump allocator of workgroups w % subs: one allocator for all 256
// workgroups queued their returning atomics on one word (c2x: phase 2 +8.7 us on
// average, the last workgroup's ticket 22 us late).  A workgroup's draw is a
// random sample of the primitives, so the regions fill alike; k_tile reports subs
// x the fullest region's requests as the pool the draw needs.
__device__ __noinline__ void pool_commit(const DrawParams& P, uint32_t* s_hist, uint32_t* s_pool, uint32_t rot,
                                         uint32_t w) {
    const uint32_t nt = P.ntiles, tid = threadIdx.x;
    if (tid == 0) {
        const uint32_t subs = pool_subs(P), k = w % subs, size = P.pool_cap / subs;
        const unsigned long long base = atomicAdd(
            reinterpret_cast<unsigned long long*>(&P.counters[kCtPoolSub0 + k * kCtSpread]), (unsigned long long)s_pool[0]);
        s_pool[2] = base + s_pool[0] <= size ? P.pool_off + k * size + (uint32_t)base : kDropCursor;
        atomicAdd(&P.counters[kCtPoolRuns], s_pool[1]);
    }
    __syncthreads();
    const uint32_t pb = s_pool[2];
    for (uint32_t i = tid; i < nt; i += kSetupThreads) {
        const uint32_t t = i + rot < nt ? i + rot : i + rot - nt;
        const uint32_t v = s_hist[t];
        if ((v >> 30) != 1u) continue;  // not pending
        if (pb != kDropCursor) {
            const uint32_t x = pb + (v & ~kPoolPending);
            P.runs[(size_t)t * P.run_cap + w].x = x;
            s_hist[t] = x;
        } else {
            atomicOr(&P.run_counts[t], kRunDropped);
            s_hist[t] = kDropCursor;
        }
    }
}

// i-th unit of primitives owned by workgroup w: interleaved (unit u -> workgroup
// u mod G), so every workgroup streams from the whole input at once (contiguous
// blocks per workgroup measured slower: C4 setup 286 vs 339 us).
__device__ __forceinline__ uint32_t own_unit(uint32_t w, uint32_t G, uint32_t i) { return w + i * G; }

// s_misc words.
enum SetupMisc : uint32_t {
    kSmValid = 0,     // primitives set up
    kSmDropped = 1,   // ... dropped by the clip
    kSmTop = 2,       // the largest tile count this workgroup saw
    kSmPairs = 3,     // the workgroup's (tile, primitive) pairs
    kSmRecMode = 4,   // records mode (no received block overflowed)
    kSmLast = 5,      // this is the last workgroup past phase 2
    kSmMicro = 6,     // covered micro primitives
    kSmPool = 8,      // [3] pool_run / pool_commit: entries, runs, the allocation's base
    kSmWaveSum = 16,  // [16] phase 4 staging: the waves' pair totals
};

// The workgroup's dynamic LDS: [ntiles (16-B padded) + kSetupMiscWords] + bboxes + staging.
struct SetupLds {
    uint32_t* hist;   // [ntiles] histogram -> cursors
    uint32_t* misc;   // [32] (SetupMisc)
    uint32_t* pre;    // records mode: exclusive prefix of the received blocks' counts
    uint32_t* sched;  // [8 x kSchedBuckets] the tile schedule (last workgroup)
    // this workgroup's primitives' tile bboxes, indexed like phase 4's flattened
    // (own unit, primitive in unit) space, when they fit (P.bbox_lds)
    BBox* bbox;
    // phase 4's staging (P.bin_stage): per-tile local cursors, then (bin position,
    // entry) pairs grouped by tile
    uint32_t* lcur;
    uint2* stage;
};

__device__ __forceinline__ SetupLds setup_lds(uint32_t* s_lds, uint32_t nt, uint32_t bbox_lds) {
    SetupLds L;
    L.hist = s_lds;
    L.misc = L.hist + ((nt + 3u) & ~3u);
    L.pre = L.misc + 32;
    L.sched = L.misc + 96;
    L.bbox = reinterpret_cast<BBox*>(L.misc + kSetupMiscWords);
    L.lcur = reinterpret_cast<uint32_t*>(L.bbox + bbox_lds);
    L.stage = reinterpret_cast<uint2*>(L.lcur + ((nt + 3u) & ~3u));
    return L;
}

// Partitioned draws (records mode): the received blocks' counts, and whether
// any block overflowed -- then this workgroup, like every other (they all read
// the same headers), sets up every primitive of the draw instead.  Wave 0's work.
__device__ __forceinline__ void scan_route_headers(const DrawParams& P, const SetupLds& L, uint32_t w, uint32_t tid) {
    // one lane per source block (G <= 32): the headers' loads in flight together
    const uint32_t src = tid;
    uint32_t total = 0;
    if (src < P.shard_count)
        total = reinterpret_cast<const RouteHeader*>(P.rlist + (size_t)src * route_block_bytes(P.route_cap))->total;
    const uint32_t cnt = min(total, P.route_cap);
    uint32_t inc = cnt, top = total;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if ((int)tid >= d) inc += y;
        top = max(top, (uint32_t)__shfl_xor((int)top, d, 64));
    }
    if (src <= P.shard_count) L.pre[src] = inc - cnt;  // exclusive prefix; s_pre[G] = all entries
    const bool over = __ballot(total > cnt) != 0ull;
    if (tid == 0) L.misc[kSmRecMode] = over ? 0u : 1u;
    if (tid == 0 && w == 0) {  // the draw's route statistics (one writer: workgroup 0)
        volatile uint32_t* st = P.status;
        if (over) st[kStRouteFallback] += 1u;
        if (top > st[kStRouteMax]) st[kStRouteMax] = top;
    }
}

// Phase 1, records mode: the received entries of this workgroup's units; records
// stored at their draw ids, bboxes counted.
__device__ __forceinline__ void setup_received(const SetupLds& L, uint32_t w, uint32_t G, uint32_t units, uint32_t n_pos,
                                               int& nvalid, int& ndropped) {
    const DrawParams& P = kernarg_params();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t usz = 1u << P.unit_shift;
    for (uint32_t i = 0;; ++i) {
        const uint32_t u = own_unit(w, G, wave + i * (kSetupThreads / 64u));
        if (u >= units) break;
        const uint32_t jw = wave + i * (kSetupThreads / 64u);  // own-unit ordinal
        for (uint32_t r = lane; r < usz; r += 64u) {
            const uint32_t pos = (u << P.unit_shift) + r;
            if (pos >= n_pos) break;
            uint32_t gid;
            const BBox box = receive_entry(P, L.pre, pos, L.hist, nvalid, ndropped, gid);
            P.gids[pos] = gid;
            P.bboxes[pos] = box;
            if (P.bbox_lds) L.bbox[(jw << P.unit_shift) + r] = box;
        }
    }
}

// Phase 1: vertex stage + setup of this workgroup's units, one wave per unit, KB
// primitives per lane in flight.
template <uint32_t KB, bool MESH>
__device__ __forceinline__ void setup_own_units(const SetupLds& L, uint32_t w, uint32_t G, uint32_t units, uint32_t n_pos,
                                                int& nvalid, int& ndropped, int& nmicro) {
    const DrawParams& P = kernarg_params();  // phase 1's own loads of the parameters (SGPR pressure)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t rounds = (1u << P.unit_shift) / (64u * KB);
    for (uint32_t i = 0;; ++i) {
        const uint32_t u = own_unit(w, G, wave + i * (kSetupThreads / 64u));
        if (u >= units) break;
        const uint32_t jw = wave + i * (kSetupThreads / 64u);  // own-unit ordinal
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t pb = (u << P.unit_shift) + r * 64u * KB + lane;
            const uint32_t lb = (jw << P.unit_shift) + r * 64u * KB + lane;
            PrimIn in[KB];
#pragma unroll
            for (uint32_t b = 0; b < KB; ++b) fetch_indices(P, pb + b * 64u, n_pos, in[b]);
#pragma unroll
            for (uint32_t b = 0; b < KB; ++b) fetch_positions(P, in[b]);
#pragma unroll
            for (uint32_t b = 0; b < KB; ++b) {
                const uint32_t prim = pb + b * 64u;
                if (prim >= n_pos) continue;
                BBox box;
                if constexpr (MESH)
                    box = setup_finish_mesh(P, prim, in[b], L.hist, nvalid, ndropped);
                else
                    box = setup_finish(P, prim, in[b], L.hist, nvalid, ndropped, nmicro);
                // global: the overflow scan of any tile may need it; LDS: phase 4
                P.bboxes[prim] = box;
                if (P.bbox_lds) L.bbox[lb + b * 64u] = box;
            }
        }
    }
}

// Phase 2: reserve this workgroup's slots in every tile's list; the cursor of
// tile t becomes t * slab + the offset the atomic returned.  Each workgroup
// starts at a different 64-tile block (rot) so that the workgroups' adds spread
// over the counter lines instead of all queueing on the same ones.  Then the
// workgroup's totals go to the draw's counters (one barrier inside).
__device__ __forceinline__ void reserve_slots(const DrawParams& P, const SetupLds& L, uint32_t nt, uint32_t w,
                                              uint32_t rot) {
    const uint32_t tid = threadIdx.x;
    uint32_t* const s_hist = L.hist;
    uint32_t* const s_misc = L.misc;
    uint32_t top = 0, sum = 0;  // the largest tile count this workgroup saw, its pairs
    for (uint32_t i = tid; i < nt; i += kSetupThreads) {
        const uint32_t t = i + rot < nt ? i + rot : i + rot - nt;
        const uint32_t c = s_hist[t];
        const uint32_t ov = c ? __hip_atomic_fetch_add(&P.tile_counts[t], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const uint32_t o = ov & ~kCountRuns;
        s_hist[t] = o + c <= P.slab ? t * P.slab + o : pool_run(P, t, ov, c, s_misc + kSmPool, w);
        if (P.bin_stage) L.lcur[t] = c;
        top = max(top, o + c);
        sum += c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        top = max(top, (uint32_t)__shfl_xor((int)top, o, 64));
        sum += (uint32_t)__shfl_xor((int)sum, o, 64);
    }
    if ((tid & 63u) == 0) {
        if (top) atomicMax(&s_misc[kSmTop], top);
        if (sum) atomicAdd(&s_misc[kSmPairs], sum);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_misc[kSmValid]) atomicAdd(&P.counters[kCtSetup], s_misc[kSmValid]);
        if (s_misc[kSmDropped]) atomicAdd(&P.counters[kCtDropped], s_misc[kSmDropped]);
        if (s_misc[kSmMicro]) atomicAdd(&P.counters[kCtMicro], s_misc[kSmMicro]);
        if (s_misc[kSmTop]) atomicMax(&P.counters[kCtMaxTile], s_misc[kSmTop]);
        if (s_misc[kSmPairs])
            atomicAdd(reinterpret_cast<unsigned long long*>(&P.counters[kCtPairs]), (unsigned long long)s_misc[kSmPairs]);
    }
}

// The last workgroup to take a ticket sees every tile's final count: the
// counts and the max are only ever changed by atomics, which execute at
// the memory side, and every one of this workgroup's has completed before
// its ticket (returned, or drained by the wait below); the schedule reads
// them back with atomics too, so no L2 holds a stale copy in between.
// Tickets in two levels: a workgroup takes one in its group of
// kTicketGroup (w / kTicketGroup, a word of its own), the group's last
// one a ticket of the groups; the last group's last workgroup builds.
// (One word for all 256 queued their returning atomics on it.)  The
// chain keeps the order argument: every workgroup's atomics precede its
// group ticket, which precedes its group's ticket of the groups.
// Leaves s_misc[kSmLast] set in that workgroup (two barriers inside).
__device__ __forceinline__ void take_schedule_ticket(const DrawParams& P, const SetupLds& L, uint32_t w, uint32_t G) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t g = w / kTicketGroup, gsize = min(kTicketGroup, G - g * kTicketGroup);
        const uint32_t gt = __hip_atomic_fetch_add(&P.counters[kCtTicketGroup0 + g * kCtSpread], 1u,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t last = 0u;
        if (gt == gsize - 1u)
            last = __hip_atomic_fetch_add(&P.counters[kCtSchedTicket], 1u, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT) == (G + kTicketGroup - 1u) / kTicketGroup - 1u;
        L.misc[kSmLast] = last;
    }
    __syncthreads();
}

// Staged phase 4: local offsets of the tiles' runs in the staging array from an
// exclusive scan of this workgroup's per-tile counts (s_lcur: counts -> local
// cursors; s_hist: bin cursor -> bin position - local slot).  Two barriers inside.
__device__ __forceinline__ void stage_offsets(const SetupLds& L, uint32_t nt) {
    const uint32_t tid = threadIdx.x;
    uint32_t* const s_lcur = L.lcur;
    const uint32_t per = (nt + kSetupThreads - 1u) / kSetupThreads;
    const uint32_t t0 = min(tid * per, nt), t1 = min(t0 + per, nt);
    uint32_t sum = 0;
    for (uint32_t t = t0; t < t1; ++t) sum += s_lcur[t];
    uint32_t inc = sum;  // exclusive scan of the threads' sums: waves, then the 16 wave totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if ((int)(tid & 63u) >= d) inc += y;
    }
    if ((tid & 63u) == 63u) L.misc[kSmWaveSum + (tid >> 6)] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t q = 0; q < (tid >> 6); ++q) base += L.misc[kSmWaveSum + q];
    uint32_t run = base + inc - sum;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t c = s_lcur[t];
        s_lcur[t] = run;   // the tile's local cursor
        L.hist[t] -= run;  // bin position - local slot
        run += c;
    }
    __syncthreads();
}

// Cost class of record bbox bb in tile (tx, ty) of edge tl = 1 << tsh: the lane
// walk's pair steps over bbox ∩ tile (cost_bucket).
__device__ __forceinline__ uint32_t tile_cost_bucket(const BBox bb, int tx, int ty, uint32_t tsh, int tl) {
    const int cy0 = max((int)(bb.bb0 >> 16), ty << tsh);
    const int cy1 = min((int)(bb.bb1 >> 16), (ty << tsh) + tl - 1);
    const int cx0 = max((int)(bb.bb0 & 0xFFFFu), tx << tsh);
    const int cx1 = min((int)(bb.bb1 & 0xFFFFu), (tx << tsh) + tl - 1);
    return cost_bucket(cx0, cx1, cy0, cy1);
}

// Phase 4: scatter the pairs of this workgroup's units, flattened over (own unit,
// primitive in unit) so every thread has work.
template <bool MESH>
__device__ __forceinline__ void scatter_pairs(const SetupLds& L, uint32_t nt, uint32_t w, uint32_t G, uint32_t units,
                                              uint32_t n_pos, bool rec_mode) {
    const DrawParams& P = kernarg_params();
    const uint32_t tid = threadIdx.x;
    uint32_t* const s_hist = L.hist;
    uint32_t* const s_lcur = L.lcur;
    uint2* const s_stage = L.stage;
    const uint32_t usz = 1u << P.unit_shift;
    // appends (tile, record) pairs of one setup record to its owned tiles' slabs
    // (the parameters the loops use, read once: kernarg_params() would reload them
    // per iteration)
    uint32_t* const bins = P.bins;
    const uint32_t sG = P.shard_count, srank = P.shard_rank, tiles_x = P.tiles_x;
    const uint32_t full_rows = P.full_rows, own_rows = P.own_rows, left_lo = P.left_lo, left_hi = P.left_hi;
    const uint32_t tsh = P.tile_shift;
    const int tl = 1 << tsh;
    auto scatter = [&](uint32_t rec, const BBox bb) {
        if (bb.bb0 == kEmptyBox) return;
        const int tx0 = (int)(bb.bb0 & 0xFFFFu) >> tsh, tx1 = (int)(bb.bb1 & 0xFFFFu) >> tsh;
        const int ty0 = (int)(bb.bb0 >> 16) >> tsh, ty1 = (int)(bb.bb1 >> 16) >> tsh;
        for_owned_tiles(sG, srank, tiles_x, full_rows, own_rows, left_lo, left_hi, tx0, ty0, tx1, ty1,
                        [&](uint32_t t, int tx, int ty) {
            const uint32_t bucket = tile_cost_bucket(bb, tx, ty, tsh, tl);
            const uint32_t pos = atomicAdd(&s_hist[t], 1u);
            if (pos < 0x80000000u) bins[pos] = rec | (bucket << kBinPrimBits);  // (not a dropped run)
        });
    };
    uint32_t nown = 0;
    while (own_unit(w, G, nown) < units) ++nown;
    // Staged (the workgroup's pairs fit P.bin_stage): the pairs go to LDS grouped
    // by tile -- local offsets from an exclusive scan of this workgroup's
    // per-tile counts -- with their bin positions, and are then stored in that
    // order, so the lanes of a store instruction write a tile's run side by
    // side (one request per run and line instead of one per pair).
    const uint32_t npairs = L.misc[kSmPairs];
    const bool staged = P.bin_stage && npairs <= P.bin_stage;
    if (staged) stage_offsets(L, nt);
    auto scatter_staged = [&](uint32_t rec, const BBox bb) {
        if (bb.bb0 == kEmptyBox) return;
        const int tx0 = (int)(bb.bb0 & 0xFFFFu) >> tsh, tx1 = (int)(bb.bb1 & 0xFFFFu) >> tsh;
        const int ty0 = (int)(bb.bb0 >> 16) >> tsh, ty1 = (int)(bb.bb1 >> 16) >> tsh;
        for_owned_tiles(sG, srank, tiles_x, full_rows, own_rows, left_lo, left_hi, tx0, ty0, tx1, ty1,
                        [&](uint32_t t, int tx, int ty) {
            const uint32_t bucket = tile_cost_bucket(bb, tx, ty, tsh, tl);
            const uint32_t l = atomicAdd(&s_lcur[t], 1u);
            const uint32_t pos = s_hist[t] + l;
            s_stage[l] = make_uint2(pos < 0x80000000u ? pos : 0xFFFFFFFFu, rec | (bucket << kBinPrimBits));
        });
    };
    for (uint32_t j = tid; staged && j < (nown << P.unit_shift); j += kSetupThreads) {
        const uint32_t prim = (own_unit(w, G, j >> P.unit_shift) << P.unit_shift) + (j & (usz - 1u));
        if (prim >= n_pos) continue;
        const BBox bb = P.bbox_lds ? L.bbox[j] : P.bboxes[prim];
        scatter_staged(rec_mode && bb.bb0 != kEmptyBox ? P.gids[prim] : prim, bb);
        if (MESH) {
            scatter_staged(mesh_record(P, prim, 1), P.bboxes[mesh_record(P, prim, 1)]);
            scatter_staged(mesh_record(P, prim, 2), P.bboxes[mesh_record(P, prim, 2)]);
        }
    }
    if (staged) {
        __syncthreads();
        for (uint32_t i = tid; i < npairs; i += kSetupThreads) {
            const uint2 v = s_stage[i];
            if (v.x != 0xFFFFFFFFu) bins[v.x] = v.y;
        }
    }
    for (uint32_t j = tid; !staged && j < (nown << P.unit_shift); j += kSetupThreads) {
        const uint32_t prim = (own_unit(w, G, j >> P.unit_shift) << P.unit_shift) + (j & (usz - 1u));
        if (prim >= n_pos) continue;
        const BBox bb = P.bbox_lds ? L.bbox[j] : P.bboxes[prim];
        scatter(rec_mode && bb.bb0 != kEmptyBox ? P.gids[prim] : prim, bb);
        if (MESH) {  // fans 1 and 2 (bboxes stored by this workgroup in phase 1)
            scatter(mesh_record(P, prim, 1), P.bboxes[mesh_record(P, prim, 1)]);
            scatter(mesh_record(P, prim, 2), P.bboxes[mesh_record(P, prim, 2)]);
        }
    }
}

template <uint32_t KB, bool MESH>
__global__ __launch_bounds__(kSetupThreads) void k_setup_bin(DrawParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_lds[];
    const uint32_t nt = P.ntiles, G = gridDim.x, w = blockIdx.x, tid = threadIdx.x;
    const SetupLds L = setup_lds(s_lds, nt, P.bbox_lds);
    uint32_t* const s_hist = L.hist;
    uint32_t* const s_misc = L.misc;
    ZR_STAMP(0);
    for (uint32_t t = tid; t < nt; t += kSetupThreads) s_hist[t] = 0;
    if (tid < 32) s_misc[tid] = 0;
    if (P.rlist && tid < 64) scan_route_headers(P, L, w, tid);
    __syncthreads();
    // This rank's own send headers are k_route's counters: the exchange has
    // consumed them (it precedes this kernel on the setup stream), so they are
    // zeroed here for the next route into this scratch set.
    if (P.rlist && w == 0 && tid < P.shard_count)
        reinterpret_cast<RouteHeader*>(P.route_out + (size_t)tid * route_block_bytes(P.route_cap))->total = 0u;
    const bool rec_mode = s_misc[kSmRecMode] != 0u;
    // setup records: the draw's primitives, or (records mode) the dense positions
    // of the received entries, in units of 2^unit_shift
    const uint32_t n_pos = rec_mode ? min(L.pre[P.shard_count], P.prims) : P.rlist ? P.draw_prims : P.prims;
    const uint32_t units = rec_mode || P.rlist ? (n_pos + (1u << P.unit_shift) - 1u) >> P.unit_shift : P.units;
    // records k_tile's overflow scan covers, and how their bboxes are indexed
    if (w == 0 && tid == 0) {
        P.draw_info[kInfoRecords] = MESH ? kMeshFans * n_pos : n_pos;
        P.draw_info[kInfoByPosition] = rec_mode ? 1u : 0u;
        // (kInfoJobEntries: build_job_schedule's alone.  A store of 0 here raced with
        // it -- plain stores of two workgroups, possibly in two XCDs' L2s, written
        // back at the kernel's end in either order -- and k_tile reads it only for
        // draws with tile jobs, whose schedule always writes it.)
    }

    // ---- phase 1
    int nvalid = 0, ndropped = 0, nmicro = 0;
    if (rec_mode)
        setup_received(L, w, G, units, n_pos, nvalid, ndropped);
    else
        setup_own_units<KB, MESH>(L, w, G, units, n_pos, nvalid, ndropped, nmicro);
    if (nvalid) atomicAdd(&s_misc[kSmValid], (uint32_t)nvalid);
    if (ndropped) atomicAdd(&s_misc[kSmDropped], (uint32_t)ndropped);
    if (nmicro) atomicAdd(&s_misc[kSmMicro], (uint32_t)nmicro);
    __syncthreads();
    ZR_STAMP(1);
    if (P.debug & kDebugPhase1Only) return;

    // ---- phase 2: slots in every tile's list, pool runs, and (the last
    // workgroup) the tile schedule and / or tile jobs
    {
        const DrawParams& P = kernarg_params();
        const uint32_t rot = nt ? ((w * 64u) % nt) : 0u;
        reserve_slots(P, L, nt, w, rot);
        if (s_misc[kSmPool]) {  // (the barrier in reserve_slots: every pool_run of this workgroup is done)
            pool_commit(P, s_hist, s_misc + kSmPool, rot, w);
            __syncthreads();
        }
        if (P.tile_order) {
            take_schedule_ticket(P, L, w, G);
            if (s_misc[kSmLast]) {
                if (P.job_entries) build_job_schedule(P, nt, L.sched);
                if (P.tile_sched) build_tile_schedule(P, nt, L.sched, P.tile_order + (P.job_entries ? P.job_pad : 0u));
            }
        }
    }
    ZR_STAMP(2);
    if (!P.bbox_lds || rec_mode) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // phase 4 reads global bboxes / gids
    __syncthreads();

    // ---- phase 4: scatter the pairs of this workgroup's units
    scatter_pairs<MESH>(L, nt, w, G, units, n_pos, rec_mode);
    ZR_STAMP(5);
}

}  // namespace zr
