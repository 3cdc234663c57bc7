// zr_tile_segment.h — k_tile's LDS by name and the phases it runs per list segment:
// load, counting sort, chunk claim and lane walk, wave-path queue; the record scan
// of a spilled tile.
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_order.h"
#include "zr_raster.h"
#include "zr_resolve.h"

namespace zr {

// ---------------------------------------------------------------- LDS carve-up

// The k_tile instances that can keep the resolve's record table (rec_table_insert):
// 512-thread tiles; last-wins modes need the records' depth terms, which it does
// not hold (64-px tiles: only 1024-thread workgroups have the LDS for it beside
// 32 KiB of keys).
constexpr bool tile_rec_table_fits(int PROG, int MODE, bool INITD, int NT, int TS) {
    return NT >= 512 && MODE != kDepthLastWins && PROG != kProgMesh && !INITD && (TS <= 5 || NT >= 1024);
}

// LDS: a workgroup's share of the CU's 160 KiB at the occupancy the launch
// bounds ask for (8 x 256 or 4 x 512 threads: 20 or 40 KiB).  The keys (8 KiB)
// become the resolve's hash table; one union holds the raster scratch (sorted
// segment, wave-path queue, bucket counts, initial depths) and then the
// resolve's per-winner array.
template <int PROG, int MODE, bool INITD, int NT, int TS>
struct TileShape {
    static constexpr int T = 1 << TS, TP = T * T;
    static constexpr uint32_t kWgsPerCu = kTileWgs * (uint32_t)kTileThreads / (uint32_t)NT;
    static constexpr uint32_t kBudget = 160u * 1024u / kWgsPerCu;
    static constexpr uint32_t kMiscWords = 16;
    static constexpr uint32_t kUnionWords = (kBudget - TP * 8u - 256u * 4u - kMiscWords * 4u) / 4u;
    static constexpr bool kTabFits = tile_rec_table_fits(PROG, MODE, INITD, NT, TS);
    static constexpr bool kTab = ZR_TAB && !ZR_RESOLVE_DEDUP512 && kTabFits;
    static constexpr uint32_t kPerThread = kSortCap / NT;  // entries of a segment per thread
    static_assert(kSortCap + kBigQueue + kSortBuckets + (INITD ? TP : 0u) + (kTabFits ? 4u * kSortCap + kRecHashSlots : 0u) <=
                      kUnionWords,
                  "k_tile raster scratch exceeds the workgroup's LDS share");
};

// s_misc words (each wave reads the list's words back through its own leader).
enum TileMisc : uint32_t {
    kMiClaim = 0,    // next 64-entry chunk of the segment to rasterize
    kMiNbig = 1,     // wave-path primitives offered to the segment's queue
    kMiBclaim = 2,   // next queued wave-path primitive
    kMiDbg = 3,      // [2] kDebugStamps: lane-walk steps of the chunks, wave-path sweeps
    kMiNwin = 5,     // resolve: distinct winners of the tile
    kMiSlabLen = 8,  // the slab part's length of the tile's list
    kMiRuns = 9,     // run slots of a tile with pool runs, else 0
    kMiJobs = 10,    // jobs of the tile (tile_jobs)
    kMiJobBuf = 11,  // first key buffer of a split tile
    kMiTicket = 12,  // a split tile's job ticket
};

// The workgroup's LDS by name.
struct TileLds {
    unsigned long long* key;  // [TP] visibility keys
    float* srgb;              // [256] the sRGB threshold table
    uint32_t* u;              // [kUnionWords] raster scratch, then the resolve's winners
    uint32_t* misc;           // [kMiscWords] (TileMisc)
    uint32_t* sorted;         // [kSortCap] the segment, sorted by cost class
    // wave-path (large) primitives of the segment, rasterized after its
    // chunks by whichever wave claims them next: the area sort groups them, so the
    // wave owning their chunk would otherwise sweep them all alone
    uint32_t* big;            // [kBigQueue]
    uint32_t* bucket;         // [kSortBuckets]
    float* initd;             // [TP] (INITD)
    int4* trec;               // [kSortCap] (kTab; over initd's place)
    uint32_t* thash;          // [kRecHashSlots]
};

__device__ __forceinline__ TileLds tile_lds(unsigned long long* s_key, float* s_srgb, uint32_t* s_u, uint32_t* s_misc) {
    TileLds L;
    L.key = s_key;
    L.srgb = s_srgb;
    L.u = s_u;
    L.misc = s_misc;
    L.sorted = s_u;
    L.big = s_u + kSortCap;
    L.bucket = L.big + kBigQueue;
    L.initd = reinterpret_cast<float*>(L.bucket + kSortBuckets);
    L.trec = reinterpret_cast<int4*>(L.bucket + kSortBuckets);
    L.thash = reinterpret_cast<uint32_t*>(L.trec + kSortCap);
    return L;
}

// ------------------------------------------------------------- segment loads

// Segment [seg, seg + n) of the list at bins[lbeg, ...) into the threads' registers.
// (lbeg, and load_segment_runs' t, are taken by reference, as the lambdas these
// functions replaced captured them: with both by value the kernel's early passes
// fold the address of tile_counts[t] into one 64-bit pointer held across the
// pass, and every instance spills 3 more SGPRs -- docs/EXPERIMENTS.md, round 8.)
template <int NT>
__device__ __forceinline__ void load_segment(const DrawParams& P, const uint32_t& lbeg, uint32_t seg, uint32_t n,
                                             uint32_t (&ent)[kSortCap / NT]) {
    // the segment's base as a uniform (scalar) pointer: lane addresses then come
    // from threadIdx alone instead of per-lane bases held (spilled) across the pass
    const uint32_t* bp = P.bins + lbeg + seg;
    asm volatile("" : "+s"(bp));
#pragma unroll
    for (uint32_t k = 0; k < kSortCap / NT; ++k) {
        const uint32_t i = threadIdx.x + k * NT;
        ent[k] = i < n ? bp[i] : 0u;  // prim | cost bucket (k_setup_bin phase 4)
    }
}

// A list with pool runs (rare: crowded tiles) is loaded through the run table,
// held in the wave-path queue's LDS (free between segments): run bases in
// s_big[0, 256), exclusive pair offsets in s_big[256, 512); a position past the
// slab part finds its run by binary search.
template <int NT>
__device__ __forceinline__ void load_segment_runs(const TileLds& L, const uint32_t& t, const uint32_t& lbeg, uint32_t seg, uint32_t n,
                                                  uint32_t slab_len, uint32_t nruns, uint32_t (&ent)[kSortCap / NT]) {
    static_assert(NT >= (int)kMaxRunsPerTile && 2u * kMaxRunsPerTile <= kBigQueue, "run table staging");
    uint32_t* const s_big = L.big;
    uint32_t* const s_sorted = L.sorted;
    const DrawParams& P = kernarg_params();  // (re-loaded here, not held across the pass)
    // one descriptor per thread (the loads in flight together), then wave 0's
    // exclusive scan of the run lengths
    if (threadIdx.x < nruns) {
        const uint2 r = P.runs[(size_t)t * P.run_cap + threadIdx.x];
        s_big[threadIdx.x] = r.x;
        s_big[kMaxRunsPerTile + threadIdx.x] = r.y;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t carry = 0;
        for (uint32_t i0 = 0; i0 < nruns; i0 += 64u) {
            const uint32_t i = i0 + threadIdx.x;
            const uint32_t len = i < nruns ? s_big[kMaxRunsPerTile + i] : 0u;
            uint32_t inc = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(inc, d, 64);
                if ((int)threadIdx.x >= d) inc += y;
            }
            if (i < nruns) s_big[kMaxRunsPerTile + i] = carry + inc - len;
            carry += (uint32_t)__shfl((int)inc, 63, 64);
        }
    }
    __syncthreads();
    // the segment's entries to s_sorted (free until the sort rewrites [0, n)),
    // then to the registers load_segment fills
    for (uint32_t i = threadIdx.x; i < n; i += NT) {
        const uint32_t p = seg + i;
        uint32_t e;
        if (p < slab_len) {
            e = P.bins[lbeg + p];
        } else {
            const uint32_t q = p - slab_len;
            uint32_t lo = 0, hi = nruns;  // the last run whose offset is <= q
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_big[kMaxRunsPerTile + mid] <= q) lo = mid; else hi = mid;
            }
            e = P.bins[s_big[lo] + (q - s_big[kMaxRunsPerTile + lo])];
        }
        s_sorted[i] = e;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kSortCap / NT; ++k) {
        const uint32_t i = threadIdx.x + k * NT;
        ent[k] = i < n ? s_sorted[i] : 0u;
    }
}

// ------------------------------------------------------------------ per segment

// Counting sort of the segment's n entries (ent: load_segment's registers) into
// s_sorted by cost class.  s_bucket[b] is left holding the sorted position where
// class b starts (the chunk loop reads kMidBucket's and the last bucket's).  Also
// resets the segment's claim counters.
template <int NT>
__device__ __forceinline__ void sort_segment(const TileLds& L, uint32_t n, const uint32_t (&ent)[kSortCap / NT]) {
    constexpr uint32_t kPerThread = kSortCap / NT;
    uint32_t* const s_bucket = L.bucket;
    if (threadIdx.x < kSortBuckets) s_bucket[threadIdx.x] = 0u;
    if (threadIdx.x < 3) L.misc[threadIdx.x] = 0u;  // kMiClaim, kMiNbig, kMiBclaim
    __syncthreads();
    uint32_t pr[kPerThread], bk[kPerThread], sl[kPerThread];
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; ++k) {
        const uint32_t i = threadIdx.x + k * NT;
        pr[k] = bk[k] = sl[k] = 0u;
        if (i < n) {
            pr[k] = ent[k] & kBinPrimMask;
            bk[k] = ent[k] >> kBinPrimBits;
            sl[k] = atomicAdd(&s_bucket[bk[k]], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {  // exclusive scan of the 64 bucket counts (one wave)
        const uint32_t c = s_bucket[threadIdx.x];
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d, 64);
            if ((int)threadIdx.x >= d) inc += y;
        }
        s_bucket[threadIdx.x] = inc - c;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPerThread; ++k) {
        const uint32_t i = threadIdx.x + k * NT;
        if (i < n) L.sorted[s_bucket[bk[k]] + sl[k]] = pr[k];
    }
    __syncthreads();
}

// Large primitives of a chunk (is_big: this lane's entry my_prim is one) are queued
// for the segment's wave pass; the whole wave sweeps them itself only when the
// queue is full.
template <int PROG, int MODE, bool INITD, int TS>
__device__ __forceinline__ void queue_wave_path(const DrawParams& P, const TileLds& L, bool is_big, uint32_t my_prim,
                                                int x0, int y0, int lane) {
    unsigned long long big = __ballot(is_big);
    if (big) {
        // The wave's batch takes the queue's free slots from `base` on; the
        // part past its end stays with this wave.  (s_nbig counts every
        // primitive offered, so the wave pass reads min(s_nbig, kBigQueue)
        // slots, and each of them must be filled: a batch straddling the end
        // fills the last slots.)
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&L.misc[kMiNbig], (uint32_t)__popcll(big));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        const uint32_t room = base < kBigQueue ? min((uint32_t)__popcll(big), kBigQueue - base) : 0u;
        const uint32_t rank = (uint32_t)__popcll(big & ((1ull << lane) - 1ull));
        if (is_big && rank < room) L.big[base + rank] = my_prim;
        for (uint32_t q = 0; q < room; ++q) big &= big - 1ull;  // the queued ones (lowest lanes)
    }
    while (big) {
        const uint32_t i = (uint32_t)__builtin_ctzll(big);
        big &= big - 1ull;
        const uint32_t prim = (uint32_t)rl((int)my_prim, i);
        const TriRecord r = load_uniform_record(P.records_big + prim);
        raster_prim<MODE, INITD, TS>(P, r, entry_seq<PROG>(P, prim), x0, y0, lane, L.key, L.initd);
        if (ZR_TILE_WORK_STATS && (tile_debug(P) & kDebugStamps) && lane == 0)
            atomicAdd(&L.misc[kMiDbg + 1], prim_sweeps<TS>(r, x0, y0));
    }
}

// One 64-lane chunk of the segment's lane space: the lane at slot g loads its
// entry's 32-B compact record, walks its share of the primitive's rows
// (raster_lane), files the record in the record table (tab) and hands a large
// primitive that cannot be walked to the wave path.
template <int PROG, int MODE, bool INITD, int TS>
__device__ __forceinline__ void raster_chunk(const DrawParams& P, const TileLds& L, const LaneSpace& ls, uint32_t g,
                                             bool tab, int x0, int y0, int lane) {
    constexpr int T = 1 << TS;
    const LaneSlot s = lane_slot(ls, g);
    const uint32_t j = s.j, ksh = s.ksh, n = ls.n;
    const int sub = s.sub;
    const bool gb = s.last;
    uint32_t my_prim = 0;
    int4 q0 = make_int4(0, 0, 0, 0), q1 = q0;
    if (j < n) {
        my_prim = L.sorted[j];
        const int4* rp = reinterpret_cast<const int4*>(P.records + my_prim);
        q0 = rp[0];
        q1 = rp[1];
    }
    const bool valid = j < n && !(tile_debug(P) & kDebugLoadOnly);
    if (tile_debug(P) & kDebugLoadOnly) asm volatile("" ::"v"(q0.x), "v"(q1.x), "v"(my_prim));
    const bool large = compact_is_large(q0);
    // A large primitive below the last cost bucket (bbox ∩ tile under ~253
    // px) takes the lane walk too when its edge values there fit int32
    // (lane_walk_fits): a wave-path sweep spends ~100 instructions of setup
    // per primitive, and sliver-heavy tiles queue hundreds of primitives with
    // a few dozen covered pixels each (cerberus: tile pass 42.6 -> 26.9 us).
    // Its other two vertices come from records_big.  The last bucket stays on
    // the wave path, which covers a large part of the tile in fewer
    // instructions (all large primitives walked: C3 tile pass +4.7 us).
    bool walk = valid && !large;
    int2 v1 = make_int2(0, 0), v2 = v1;
    if (valid && large && (!gb || compact_is_sliver(q0) || ZR_LARGE_LANES >= 2) && ZR_LARGE_LANES) {
        const int2* vp = reinterpret_cast<const int2*>(P.records_big + my_prim) + 1;
        v1 = vp[0];
        v2 = vp[1];
        walk = lane_walk_fits<TS>(decode_large(P, q0, q1, true, v1, v2), x0, y0);
    }
    if (tab && valid && sub == 0) {
        if (!large) {
            rec_table_insert(L.thash, L.trec, my_prim, j, q0, q1, x0, y0);
        } else {
            // not hashed, but position j must not keep an earlier segment's
            // small record: a hash slot that segment inserted for j would
            // pass rec_table_find's s_sorted[j] check for this primitive.
            // The large marker (dx1 == kCompactLarge in q0.z) sends such a
            // lookup to records_big.
            L.trec[j] = make_int4(0, q0.z, 0, 0);
        }
    }
    if (walk && !(tile_debug(P) & kDebugSkipLanePath))
        raster_lane<MODE, INITD, TS>(P, decode_large(P, q0, q1, large, v1, v2), entry_seq<PROG>(P, my_prim), x0, y0,
                                 L.key, L.initd, sub, (int)ksh);
    if (ZR_TILE_WORK_STATS && (tile_debug(P) & kDebugStamps)) {  // work of the chunk: its longest lane walk
        int steps = 0;
        if (valid && !large) {
            const TriRecord r = decode_compact(P, q0, q1, true);
            const int bw = min((int)(r.bb1 & 0xFFFFu), x0 + T - 1) - max((int)(r.bb0 & 0xFFFFu), x0) + 1;
            const int bh = min((int)(r.bb1 >> 16), y0 + T - 1) - max((int)(r.bb0 >> 16), y0) + 1;
            steps = (bw > 0 && bh > sub) ? bw * ((bh - sub + (1 << ksh) - 1) >> ksh) : 0;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) steps = max(steps, __shfl_xor(steps, o, 64));
        if (lane == 0) atomicAdd(&L.misc[kMiDbg], (uint32_t)steps);
    }
    queue_wave_path<PROG, MODE, INITD, TS>(P, L, valid && large && !walk && sub == 0, my_prim, x0, y0, lane);
}

// Waves claim 64-entry chunks from an LDS counter, largest bboxes first
// (the sort put them last): longest-processing-time-first balances the
// waves of a tile.  One lane per entry loads its 32-B compact record.
// A sparse segment (fewer entries than lanes) gives each entry k lanes,
// which split its bbox rows (lane_space).  With no more chunks than waves each
// wave takes one statically (measured faster there: C1 78 vs 85 us, C3 299
// vs 304 us; LPT: C2 80 vs 82 us).
template <int PROG, int MODE, bool INITD, int NT, int TS>
__device__ __forceinline__ void raster_chunks(const DrawParams& P, const TileLds& L, uint32_t n, bool tab, int x0, int y0,
                                              uint32_t wave, int lane) {
    const uint32_t off63 = L.bucket[kSortBuckets - 1];
    const uint32_t offm = L.bucket[kMidBucket];
    const LaneSpace ls = lane_space(n, (uint32_t)NT, offm, off63);
    const uint32_t nch = ls.chunks;
    const bool lpt = nch > NT / 64u;
    for (uint32_t it = 0;; ++it) {
        uint32_t claim = wave + it * (NT / 64u);  // static: wave w takes chunks w, w + waves, ...
        if (lpt) {
            if (lane == 0) claim = atomicAdd(&L.misc[kMiClaim], 1u);
            claim = (uint32_t)__builtin_amdgcn_readfirstlane((int)claim);
        }
        if (claim >= nch) break;
        const uint32_t g = (lpt ? nch - 1u - claim : claim) * 64u + (uint32_t)lane;  // lane-space slot
        raster_chunk<PROG, MODE, INITD, TS>(P, L, ls, g, tab, x0, y0, lane);
    }
}

// The segment's queued wave-path primitives (nbig of them), two per claim.
template <int PROG, int MODE, bool INITD, int TS>
__device__ __forceinline__ void drain_wave_queue(const DrawParams& P, const TileLds& L, uint32_t nbig, int x0, int y0,
                                                 int lane) {
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(&L.misc[kMiBclaim], 2u);
        i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
        if (i >= nbig || (tile_debug(P) & kDebugSkipWavePath)) break;
        const bool two = i + 1u < nbig;
        const uint32_t e0 = L.big[i], e1 = two ? L.big[i + 1u] : e0;
        // both full records' loads in flight at once (one exposed latency per
        // claim), the second held in scalar registers.  (Staging the segment's
        // queued records in LDS with one workgroup-wide load: cerberus -0.8 us,
        // C2 +0.9, C3 +2.6.)
        const int4* a = reinterpret_cast<const int4*>(P.records_big + e0);
        const int4* b = reinterpret_cast<const int4*>(P.records_big + e1);
        const int4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
        const int4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
        const TriRecord ra = uniform_record(a0, a1, a2, a3);
        const TriRecord rb = uniform_record(b0, b1, b2, b3);
        raster_prim<MODE, INITD, TS>(P, ra, entry_seq<PROG>(P, e0), x0, y0, lane, L.key, L.initd);
        if (two) raster_prim<MODE, INITD, TS>(P, rb, entry_seq<PROG>(P, e1), x0, y0, lane, L.key, L.initd);
    }
}

// ------------------------------------------------ record scan of a spilled tile

// A tile with a dropped run: every setup record whose bbox meets the tile, one
// lane per record (small) or the wave (large).
template <int PROG, int MODE, bool INITD, int NT, int TS>
__device__ __forceinline__ void scan_records(const DrawParams& P, const TileLds& L, int x0, int y0, uint32_t wave,
                                             int lane) {
    constexpr int T = 1 << TS;
    const uint32_t r0 = 0u, n_rec = P.draw_info[kInfoRecords];  // setup records of the draw
    const bool by_pos = P.draw_info[kInfoByPosition] != 0u;
    for (uint32_t cb = r0 + wave * 64u; cb < n_rec; cb += NT) {
        const uint32_t j = cb + (uint32_t)lane;
        bool hit = false;
        int4 q0 = make_int4(0, 0, 0, 0), q1 = q0;
        if (j < n_rec) {
            const BBox bb = P.bboxes[j];
            hit = bb.bb0 != kEmptyBox && (int)(bb.bb0 & 0xFFFFu) < x0 + T && (int)(bb.bb1 & 0xFFFFu) >= x0 &&
                  (int)(bb.bb0 >> 16) < y0 + T && (int)(bb.bb1 >> 16) >= y0;
        }
        uint32_t rec = j;  // bboxes by position; records by draw primitive (records mode: gids)
        if (hit) {
            if (by_pos) rec = P.gids[j];
            const int4* rp = reinterpret_cast<const int4*>(P.records + rec);
            q0 = rp[0];
            q1 = rp[1];
        }
        const bool large = compact_is_large(q0);
        if (hit && !large)
            raster_lane<MODE, INITD, TS>(P, decode_compact(P, q0, q1, true), entry_seq<PROG>(P, rec), x0, y0, L.key,
                                     L.initd, 0, 0);
        unsigned long long big = __ballot(hit && large);
        while (big) {
            const uint32_t i = (uint32_t)__builtin_ctzll(big);
            big &= big - 1ull;
            const uint32_t prim = (uint32_t)rl((int)rec, i);
            raster_prim<MODE, INITD, TS>(P, load_uniform_record(P.records_big + prim), entry_seq<PROG>(P, prim), x0, y0, lane,
                                     L.key, L.initd);
        }
    }
}

}  // namespace zr
