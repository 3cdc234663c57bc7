// zr_tile.h — k_tile, the tile pass: the kernel at the end of the
// file reads top to bottom as the pass, each phase a function above it or in
// zr_tile_segment.h.
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_order.h"
#include "zr_resolve.h"
#include "zr_tile_segment.h"

namespace zr {

// ------------------------------------------------- key and table initialisation

// The tile's initial keys (the clear depth, or the attachment's), the sRGB table's
// LDS copy, an empty record table (tab) and zeroed work counters.
template <int MODE, bool INITD, int NT, int TS>
__device__ __forceinline__ void init_tile_lds(const DrawParams& P, const TileLds& L, int x0, int y0, bool tab) {
    constexpr int T = 1 << TS, TP = T * T;
    for (int i = threadIdx.x; i < TP; i += NT) {
        const int px = x0 + (i & (T - 1)), py = y0 + (i >> TS);
        float d = P.clear_depth;
        if (P.load_depth && px < (int)P.fb_w && py < (int)P.fb_h) d = P.depth[(size_t)py * P.fb_w + px];
        L.key[i] = init_key<MODE>(d);
        if (INITD) L.initd[i] = d;
    }
    if (threadIdx.x < 255) L.srgb[threadIdx.x] = c_srgbT[threadIdx.x];
    if (tab)
        for (uint32_t i = threadIdx.x; i < kRecHashSlots; i += NT) L.thash[i] = 0u;
    if (threadIdx.x < 2) L.misc[kMiDbg + threadIdx.x] = 0u;
}

// ---------------------------------------------------------- draw status report

// The first tile block dispatched reports the draw's setup and binning stats
// (k_setup_bin's counters, complete before this launch) to the runtime's status
// words: plain stores, no read of host memory unless a run was dropped
// (volatile accesses wait for each one to cross the bus).  Draws run in stream
// order; the host reads the words after a stream sync.  One thread's work.
__device__ __forceinline__ void report_draw_status(const DrawParams& P) {
    uint32_t* st = P.status;
    const unsigned long long pairs = *reinterpret_cast<const unsigned long long*>(&P.counters[kCtPairs]);
    // pool: what the runs asked for; need: subs x the fullest sub-pool's asks,
    // which passes pool_cap exactly when a sub-pool dropped a run (pool_commit)
    unsigned long long pool = 0ull, need_sub = 0ull;
    const uint32_t subs = pool_subs(P);
    for (uint32_t k = 0; k < subs; ++k) {
        const unsigned long long a = *reinterpret_cast<const unsigned long long*>(&P.counters[kCtPoolSub0 + k * kCtSpread]);
        pool += a;
        need_sub = max(need_sub, a);
    }
    const unsigned long long pool_need = need_sub * subs;
    st[kStTrianglesSetup] = P.counters[kCtSetup];
    st[kStDroppedClip] = P.counters[kCtDropped];
    st[kStMicro] = P.counters[kCtMicro];
    st[kStTotalPairs] = pairs > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pairs;
    st[kStPoolPairs] = pool > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pool;
    st[kStPoolRuns] = P.counters[kCtPoolRuns];
    st[kStJobs] = P.counters[kCtJobs];
    if (P.counters[kCtJobsDenied]) {
        const uint32_t jd = st[kStJobsDenied];
        st[kStJobsDenied] = jd + 1u;
    }
    const uint32_t target = bin_slab_target(pairs, P.ntiles);
    if (pool_need > P.pool_cap) {  // a dropped run: the buffer this draw asks for (read-modify-write only here)
        const unsigned long long need = (unsigned long long)P.ntiles * target + pool_need;
        const uint32_t need32 = need > 0x80000000ull ? 0x80000000u : (uint32_t)need;
        const uint32_t ov = st[kStOverflow], bn = st[kStBinNeed];
        st[kStOverflow] = ov + 1u;
        if (need32 > bn) st[kStBinNeed] = need32;
    }
    if (P.stat_slot < kSlabSlots) {  // (the runtime derives the buffer the draw asks for from these)
        st[kStSlabSlot0 + P.stat_slot] = target;
        st[kStPoolSlot0 + P.stat_slot] = pool_need > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pool_need;
        st[kStMaxSlot0 + P.stat_slot] = P.counters[kCtMaxTile];
        st[kStJobBufSlot0 + P.stat_slot] = P.counters[kCtJobBufs];
        st[kStJobPartSlot0 + P.stat_slot] = P.counters[kCtJobXcdMax];
    }
}

// ------------------------------------------------------------ list description

// The list: the slab's first slab_len entries, then the tile's pool runs
// (k_setup_bin pool_run), count entries in all.  A tile with a dropped run (the
// pool was full; the runtime grows the bin buffer for later draws) is
// rasterized exactly but slowly: it scans every record's bbox (k_setup_bin
// stored them all) instead.  Only a tile with kCountRuns reads its run word.
struct TileList {
    bool spill;       // a dropped run: the record scan instead of the list
    uint32_t K;       // jobs of the tile
    uint32_t seg_lo;  // this block's part of the list: [seg_lo, cnt)
    uint32_t cnt;
};

// count_v: tile_counts[t] as loaded.  Parks the slab part's length, the run slots,
// K and the key slot in s_misc.
__device__ __forceinline__ TileList describe_list(const DrawParams& P, const TileLds& L, uint32_t t, uint32_t part,
                                                  uint32_t count_v, uint32_t slab) {
    const uint32_t count = count_v & ~kCountRuns;
    const bool has_runs = (__builtin_amdgcn_readfirstlane((int)count_v) & (int)kCountRuns) != 0;
    const uint32_t rcw = has_runs ? (uint32_t)__builtin_amdgcn_readfirstlane((int)P.run_counts[t]) : 0u;
    TileList l;
    l.spill = (rcw & kRunDropped) != 0u;
    // this block's part of the list: all of it, or job `part` of K (build_job_schedule)
    const uint32_t J = P.job_entries ? (uint32_t)__builtin_amdgcn_readfirstlane((int)P.draw_info[kInfoJobEntries]) : 0u;
    l.K = tile_jobs(count, rcw, J);
    l.seg_lo = l.K > 1u ? part * J : 0u;
    l.cnt = l.spill ? 0u : l.K > 1u ? min(count, l.seg_lo + J) : count;
    // (the segment loop reads slab_len and the run count back from LDS, each wave
    // its own leader's copy: held in registers across the pass they cost the C2
    // instance VGPR spills; likewise the job count and key slot after it)
    if ((threadIdx.x & 63u) == 0) {
        L.misc[kMiSlabLen] = (rcw & kRunFill) ? (rcw & ~(kRunFill | kRunDropped)) >> kRunFillShift : min(count, slab);
        L.misc[kMiRuns] = has_runs ? P.run_cap : 0u;  // (one run slot per setup workgroup, empty ones of length 0)
        L.misc[kMiJobs] = l.K;
        L.misc[kMiJobBuf] = l.K > 1u ? P.job_slot[t] : 0u;
    }
    return l;
}

// k_setup_bin's counters back to zero for the next draw on this scratch set:
// each tile its own count (every wave has read it: the barrier before the list
// description) and, at the end of the tile, its run word (read after that barrier),
// the first tile block the draw counters
template <int NT>
__device__ __forceinline__ void reset_counters(const DrawParams& P, uint32_t t, uint32_t jp, uint32_t K) {
    if (threadIdx.x == 0 && K == 1u) P.tile_counts[t] = 0u;  // (a split tile: its resolving job)
    if (blockIdx.x == jp)
        for (uint32_t i = threadIdx.x; i < kCtWords; i += NT) P.counters[i] = 0u;
}

// -------------------------------------------------------------------- job merge

// A split tile (tile jobs): every job stores its keys to a buffer of its own
// (job_keys[job_slot[t] + part]) and takes a ticket; the last job to arrive
// folds the others' keys into its own with a min (every job started from the
// same initial keys) and resolves the tile, the others end here.  (Plain
// system-coherent stores and loads: merging with 64-bit atomic mins at device
// scope ran c2x's tile pass at 281 us with jobs of 2048 entries, 639 with 512;
// their blocks are not reliably on one XCD, so L2-local atomics lost keys.)
// Kj jobs, key buffers from buf0.  False: this job is not the tile's last.
template <int NT, int TS>
__device__ __forceinline__ bool merge_jobs(const DrawParams& P, const TileLds& L, uint32_t t, uint32_t part, uint32_t Kj,
                                           uint32_t buf0) {
    constexpr int T = 1 << TS, TP = T * T;
    unsigned long long* const s_key = L.key;
    unsigned long long* mine = P.job_keys + (size_t)(buf0 + part) * TP;
    int i0 = threadIdx.x;  // (opaque: the key addresses of the init loop, held across the pass, spilled)
    asm volatile("" : "+v"(i0));
    for (int i = i0; i < TP; i += NT)
        __hip_atomic_store(&mine[i], s_key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (each thread's stores done before the ticket)
    __syncthreads();
    if (threadIdx.x == 0)
        L.misc[kMiTicket] = __hip_atomic_fetch_add(&P.job_tickets[buf0], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)L.misc[kMiTicket]) != Kj - 1u) return false;
    // (eight buffers' loads in flight per pixel: one buffer at a time, the fold
    // of a 15-job tile was ~15 memory round trips on the pass's critical path)
    const unsigned long long* keys0 = P.job_keys + (size_t)buf0 * TP;
    for (int i = i0; i < TP; i += NT) {
        unsigned long long m = s_key[i];
        for (uint32_t j0 = 0; j0 < Kj; j0 += 8u) {
            unsigned long long v[8];
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {
                const uint32_t j = j0 + k;
                v[k] = (j < Kj && j != part)
                           ? __hip_atomic_load(&keys0[(size_t)j * TP + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                           : ~0ull;
            }
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) m = v[k] < m ? v[k] : m;
        }
        s_key[i] = m;
    }
    if (threadIdx.x == 0) {
        __hip_atomic_store(&P.job_tickets[buf0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        P.tile_counts[t] = 0u;  // (every job of the tile read it before its ticket)
    }
    __syncthreads();
    return true;
}

// ------------------------------------------------------------- resolve dispatch

// Resolve (the index width is a template parameter so a winner's record and
// index loads are issued back to back).
template <int PROG, int MODE, bool INITD, int NT, int TS>
__device__ __forceinline__ void resolve_dispatch(const DrawParams& P, const TileLds& L, int x0, int y0,
                                                 unsigned long long* ts) {
    using S = TileShape<PROG, MODE, INITD, NT, TS>;
    if constexpr (NT >= 512 && !ZR_RESOLVE_DEDUP512) {
        if (P.index_size == 4)
            resolve_pixels<PROG, MODE, true, NT, S::kTab, TS>(kernarg_params(), x0, y0, L.key, L.srgb, L.thash, L.trec, L.sorted);
        else
            resolve_pixels<PROG, MODE, false, NT, S::kTab, TS>(kernarg_params(), x0, y0, L.key, L.srgb, L.thash, L.trec, L.sorted);
    } else if (P.index_size == 4) {
        resolve_tile<PROG, MODE, true, NT, TS>(kernarg_params(), x0, y0, L.key, L.u, S::kUnionWords, L.misc + kMiNwin, L.srgb, ts);
    } else {
        resolve_tile<PROG, MODE, false, NT, TS>(kernarg_params(), x0, y0, L.key, L.u, S::kUnionWords, L.misc + kMiNwin, L.srgb, ts);
    }
}

// ------------------------------------------------- run-table reset and stamps

// A tile with pool runs clears its run table and run word for the next draw
// (every wave read them before the segment loop; a split tile: its resolving
// job, after every job's loop)
template <int NT>
__device__ __forceinline__ void reset_run_table(uint32_t t) {
    const DrawParams& Q = kernarg_params();  // (loaded here, not held across the pass)
    uint2* rt = Q.runs + (size_t)t * Q.run_cap;
    for (uint32_t i = threadIdx.x; i < Q.run_cap; i += NT) rt[i] = make_uint2(0u, 0u);
    if (threadIdx.x == 0) Q.run_counts[t] = 0u;
}

// kDebugStamps: the tile's end time, its work counters and list length (count).
template <int NT>
__device__ __forceinline__ void stamp_epilogue(const TileLds& L, unsigned long long* ts, uint32_t count) {
    ts[4] = __builtin_amdgcn_s_memrealtime();
    ts[7] = ((unsigned long long)L.misc[kMiDbg + 1] << 32) | L.misc[kMiDbg];
    if (NT >= 512) {  // (resolve_tile's own stamps use these two at 256 threads)
        if (!count) {  // no segment ran: no wave-path queue either (dbg_ts persists across draws)
            ts[5] = ts[2] = ts[1];
            ts[6] = 0ull;
        } else {
            ts[6] = (ts[6] & ~0xFFFFFFFFull) | count;  // the tile's list length (tools/tile_stamps.py)
        }
    }
}

// ----------------------------------------------------------------------- k_tile

// NT threads per tile: 256 when the pass has several tiles per CU, 512 when it
// has few (tile-row shards, small attachments), so a tile's primitives spread
// over more waves (P.tile_threads, tile_threads_for).
template <int PROG, int MODE, bool INITD, int NT, int TS>
// (launch bounds: the second argument is the minimum waves per SIMD -- 8, i.e.
// 64 VGPRs, for both sizes; 8 x 256 or 4 x 512 threads per CU)
__global__ __launch_bounds__(NT, kTileWgs * kTileThreads / 256) void k_tile(DrawParams P) {
    using S = TileShape<PROG, MODE, INITD, NT, TS>;
    constexpr int T = S::T, TP = S::TP;
    __shared__ unsigned long long s_key[TP];
    __shared__ float s_srgb[256];
    __shared__ __attribute__((aligned(16))) uint32_t s_u[S::kUnionWords];
    __shared__ uint32_t s_misc[S::kMiscWords];
    const TileLds L = tile_lds(s_key, s_srgb, s_u, s_misc);

    // ---- item decode
    // a tile_order item: tile | job part << kJobTileBits, or a job grid's spare block
    const uint32_t jp = P.job_entries ? P.job_pad : 0u;  // (tile jobs: part blocks first)
    // (reversed timing runs reverse the tile blocks only, so block jp -- the
    // reporter below -- still holds a tile, never a spare part block)
    const uint32_t b = ((tile_debug(P) & kDebugReverseTiles) && blockIdx.x >= jp) ? jp + (gridDim.x - 1u - blockIdx.x)
                                                                                   : blockIdx.x;
    const uint32_t item = (b < jp || P.tile_sched) ? P.tile_order[b] : xcd_tile(b - jp, P.ntiles);
    // (a tile past the draw's would be a schedule bug: a wrong image the parity
    // tests see, not an access outside the buffers)
    if (item == kJobNone || item_tile(item) >= P.ntiles) return;
    const uint32_t t = item_tile(item), part = item_part(item);
    uint32_t tx, ty;
    shard_tile_xy(shard_geom(P), t, tx, ty);
    const int x0 = (int)tx * T, y0 = (int)ty * T;
    const bool stamp = (tile_debug(P) & kDebugStamps) && threadIdx.x == 0 && t < kMaxTilesPerPass;
    unsigned long long* ts = P.dbg_ts + 8192 * 8 + (size_t)t * 8;
    if (stamp) ts[0] = __builtin_amdgcn_s_memrealtime();

    // The tile's first segment of bin entries is requested before anything else
    // (workgroups dispatched last would otherwise queue these loads behind the
    // record gathers of every tile that started earlier), in parallel with its
    // count: the list lives at a fixed slab, bins[t * slab, ...), so the loads need
    // not wait for it; entries past the count are never used.
    const uint32_t slab = P.slab;
    const uint32_t lbeg = t * slab;
    uint32_t ent[S::kPerThread];
    if (!(tile_debug(P) & kDebugSkipRaster) && part == 0) load_segment<NT>(P, lbeg, 0, min(kSortCap, slab), ent);
    const uint32_t count_v = P.tile_counts[t];
    const uint32_t count = count_v & ~kCountRuns;

    // ---- keys, tables, the draw's status report
    const bool tab = S::kTab && P.rec_table != 0u;  // (runtime: draws dense enough to gain from it)
    init_tile_lds<MODE, INITD, NT, TS>(P, L, x0, y0, tab);
    if (blockIdx.x == jp && threadIdx.x == 0) report_draw_status(P);  // (jp: the first tile block; part blocks before it may be spare)
    __syncthreads();

    // ---- the list, counter resets
    const TileList list = describe_list(P, L, t, part, count_v, slab);
    reset_counters<NT>(P, t, jp, list.K);

    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (stamp) ts[1] = __builtin_amdgcn_s_memrealtime();
    if (!(tile_debug(P) & kDebugSkipRaster)) {
        // The list is processed in segments of kSortCap entries.  Each segment is
        // counting-sorted in LDS by the lane walk's pair steps over bbox ∩ tile
        // so that a 64-lane chunk holds primitives of similar cost (the lane loop runs
        // as long as its largest member).  Then each wave takes every 4th chunk: one
        // lane per entry loads the 64-B record, and the wave walks the chunk.
        for (uint32_t seg = list.seg_lo; seg < list.cnt; seg += kSortCap) {
            const uint32_t n = min(kSortCap, list.cnt - seg);
            // a list with pool runs loads its segments past the slab part through
            // the run table
            const uint32_t nr = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_misc[kMiRuns]);
            const uint32_t slab_len = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_misc[kMiSlabLen]);
            if (nr && seg + n > slab_len) {
                load_segment_runs<NT>(L, t, lbeg, seg, n, slab_len, nr, ent);
            } else if (seg) {
                load_segment<NT>(P, lbeg, seg, n, ent);
            }
            const DrawParams& P = kernarg_params();  // re-loaded per segment, not held across the pass
            sort_segment<NT>(L, n, ent);
            if (stamp && seg == 0) ts[2] = __builtin_amdgcn_s_memrealtime();
            raster_chunks<PROG, MODE, INITD, NT, TS>(P, L, n, tab, x0, y0, wave, lane);
            __syncthreads();
            const uint32_t nbig = min(s_misc[kMiNbig], kBigQueue);
            if (stamp && NT >= 512 && seg == 0) {  // first segment: chunks done, wave-path queue length
                ts[5] = __builtin_amdgcn_s_memrealtime();
                ts[6] = (unsigned long long)s_misc[kMiNbig] << 32;
            }
            drain_wave_queue<PROG, MODE, INITD, TS>(P, L, nbig, x0, y0, lane);
            __syncthreads();
        }
        if (list.spill) scan_records<PROG, MODE, INITD, NT, TS>(P, L, x0, y0, wave, lane);
    }
    __syncthreads();

    // ---- job merge (a split tile: only its last job goes on)
    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)s_misc[kMiJobs]) > 1u) {
        const uint32_t Kj = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_misc[kMiJobs]);
        const uint32_t buf0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_misc[kMiJobBuf]);
        if (!merge_jobs<NT, TS>(P, L, t, part, Kj, buf0)) return;
    }
    if (stamp) ts[3] = __builtin_amdgcn_s_memrealtime();

    // ---- resolve, run-table reset, stamps
    resolve_dispatch<PROG, MODE, INITD, NT, TS>(P, L, x0, y0, stamp ? ts : nullptr);
    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)s_misc[kMiRuns])) reset_run_table<NT>(t);
    if (stamp) stamp_epilogue<NT>(L, ts, count);
}

}  // namespace zr
