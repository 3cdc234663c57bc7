// zr_plan.cpp — draw planning and scratch sizing (zr_plan.h): host arithmetic only.
#include "zr_plan.h"

#include <cstdlib>

namespace zr {

Knobs read_knobs() {
    Knobs k;
    if (const char* dbg = getenv("ZR_DEBUG")) k.debug = (uint32_t)strtoul(dbg, nullptr, 0);
    if (const char* p = getenv("ZR_DEBUG_TS")) k.dbg_ts_path = p;
    // (at most 2^30 entries: k_setup_bin's cursors tag pending and dropped runs in bits 30-31)
    if (const char* cap = getenv("ZR_BIN_CAPACITY"))
        k.initial_bins = std::min<uint64_t>(std::max<uint64_t>(64, strtoull(cap, nullptr, 0)), 1ull << 30);
    if (const char* sl = getenv("ZR_BIN_SLAB")) k.forced_slab = (uint32_t)std::min<uint64_t>(strtoull(sl, nullptr, 0), kMaxSlab);
    if (const char* g = getenv("ZR_GRAPH")) k.use_graphs = strtoul(g, nullptr, 0) != 0;
    if (const char* o = getenv("ZR_SETUP_OVERLAP")) k.setup_overlap = strtoul(o, nullptr, 0) != 0 ? 1 : 0;
    if (const char* rt = getenv("ZR_REC_TABLE")) k.rec_table = strtoul(rt, nullptr, 0) != 0 ? 1 : 0;
    if (const char* ts = getenv("ZR_TILE_SCHED")) k.tile_sched = strtoul(ts, nullptr, 0) != 0 ? 1 : 0;
    if (const char* rw = getenv("ZR_REC_WGS")) k.rec_wgs = (uint32_t)strtoul(rw, nullptr, 0);
    if (const char* bs = getenv("ZR_BIN_STAGE")) k.bin_stage = atoi(bs);
    if (const char* mi = getenv("ZR_MICRO")) k.micro = atoi(mi) != 0 ? 1 : 0;
    if (const char* ss = getenv("ZR_BIN_SHRINK_SYNCS")) k.shrink_syncs = (uint32_t)strtoul(ss, nullptr, 0);
    if (const char* jb = getenv("ZR_JOBS")) k.jobs = atoi(jb) > 0 ? std::max(atoi(jb), 256) : 0;
    if (const char* sb = getenv("ZR_SETUP_BATCH")) {
        const int b = atoi(sb);
        k.setup_batch = b == 1 || b == 2 || b == 4 ? (uint32_t)b : 0u;
    }
    if (const char* tl = getenv("ZR_TILE")) {
        const unsigned long v = strtoul(tl, nullptr, 0);
        k.forced_tile_shift = v == 16 ? 4u : v == 32 ? 5u : v == 64 ? 6u : 0u;
    }
    if (const char* nt = getenv("ZR_TILE_NT")) {
        const unsigned long v = strtoul(nt, nullptr, 0);
        k.tile_threads = v >= 512 ? 512u : v ? 256u : 0u;
    }
    return k;
}

uint64_t shape_key(uint32_t ntiles, uint32_t prims) {
    const uint32_t bits = prims ? 32u - (uint32_t)__builtin_clz(prims) : 0u;
    const uint32_t drop = bits > 5u ? bits - 5u : 0u;
    return ((uint64_t)ntiles << 32) | ((prims >> drop) << drop);
}

uint64_t route_capacity_default(uint64_t span, uint64_t G) {
    if (G <= 2) return span;
    return std::min<uint64_t>(span, (2 * span + G - 1) / G + 4096);
}

int32_t choose_depth_mode(bool test, bool write, int32_t op) {
    if (!test) return kDepthLastWins;
    if (write) {
        switch (op) {
        case 1: return kDepthMinStrict;
        case 3: return kDepthMinNonStrict;
        case 4: return kDepthMaxStrict;
        case 6: return kDepthMaxNonStrict;
        default: break;
        }
    }
    return kDepthLastWins;
}

void set_tiles(DrawParams& P, uint32_t shift) {
    const uint32_t t = 1u << shift;
    P.tile_shift = shift;
    P.tiles_x = (P.fb_w + t - 1) >> shift;
    P.tiles_y = (P.fb_h + t - 1) >> shift;
    const ShardGeom sg = shard_geom(P.tiles_x, P.tiles_y, P.shard_count, P.shard_rank);
    P.full_rows = sg.full_rows;
    P.own_rows = sg.own_rows;
    P.left_lo = sg.left_lo;
    P.left_hi = sg.left_hi;
    P.ntiles = shard_tiles(sg);
}

// ------------------------------------------------------------------ plan_draw

namespace {

zr_result plan_fail(std::string& err, zr_result code, const char* msg) {
    err = msg;
    return code;
}

// Partitioned setup: this rank routes [lo, hi) of the draw's
// primitives; the setup pass then runs over the received blocks' dense
// positions (at most shard_count * span of them).
zr_result plan_route(DrawParams& P, const DrawRequest& rq, DrawPlan& plan, std::string& err) {
    const uint64_t G = P.shard_count, prims = plan.prims;
    const uint64_t per_rank = (prims + G - 1) / G;
    plan.span = std::max<uint64_t>(1, (per_rank + kRouteChunk - 1) / kRouteChunk) * kRouteChunk;
    const uint64_t cap = std::max<uint64_t>(
        1, std::min<uint64_t>(plan.span, rq.route_cap ? rq.route_cap : route_capacity_default(plan.span, G)));
    // received entries, or every draw primitive when a block overflowed
    plan.positions = std::max<uint64_t>(prims, G * cap);
    if (plan.positions > kBinPrimMask)
        return plan_fail(err, ZR_ERROR_FEATURE_NOT_PRESENT, "partitioned draw: more than 2^26-1 block positions");
    P.route_cap = (uint32_t)cap;
    P.route_chunks = (uint32_t)(plan.span / kRouteChunk);
    P.route_lo = (uint32_t)std::min<uint64_t>(prims, (uint64_t)P.shard_rank * plan.span);
    P.route_hi = (uint32_t)std::min<uint64_t>(prims, (uint64_t)P.route_lo + plan.span);
    P.prims = (uint32_t)plan.positions;
    return ZR_SUCCESS;
}

// The tile edge (tile_shift_for): 16 px for a shape whose 32-px tiles needed
// tile jobs (measured), 64 px for large dense targets, 32 px otherwise and for
// shards; ZR_TILE forces an edge (tests, A/B) where the instance exists.
void plan_tile_edge(DrawParams& P, uint64_t prims, const Knobs& k, const ShapeBook& book) {
    if (P.shard_count != 1 || !tile_variant_built(P.program, P.depth_mode)) return;
    uint32_t shift = k.forced_tile_shift;
    if (!shift) {
        // the edge by size, then 16 px if that edge's shape was measured crowded
        // (its draws keep consulting that measurement, stable once it is made)
        shift = tile_shift_for(prims, P.fb_w, P.fb_h, P.shard_count, false);
        if (shift != P.tile_shift) set_tiles(P, shift);
        const BinShape* sh = book.find(P.ntiles, P.draw_prims);
        if (sh && crowded_shape(sh->max_tile, sh->target)) shift = tile_shift_for(prims, P.fb_w, P.fb_h, P.shard_count, true);
    }
    if (shift != P.tile_shift) set_tiles(P, shift);
    if (P.ntiles > kMaxTilesPerPass) set_tiles(P, kTileShift);
}

// Binning geometry: k_setup_bin runs one kSetupThreads workgroup per CU at most
// (its LDS histogram of all tiles; workgroups never wait for each other) --
// fewer for small draws; a wave processes units of 64 * batch * 2^k primitives,
// at most ~64 units per workgroup on average (at most kMaxRunsPerTile
// workgroups: a pool run takes its workgroup's slot of the tile's run table).
void plan_setup_grid(DrawParams& P, const DrawRequest& rq, const Knobs& k, DrawPlan& plan) {
    const uint64_t positions = plan.positions;
    P.setup_batch = plan.mesh ? 1u : (k.setup_batch ? k.setup_batch : 2u);  // k_setup_bin<2> (the mesh instance: <1, true>)
    const uint64_t cus = std::min<uint64_t>((uint64_t)std::max(rq.cu_count, 1), kMaxRunsPerTile);
    const uint64_t per_wg = (uint64_t)kSetupThreads * P.setup_batch;
    P.setup_wgs = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cus, (positions + per_wg - 1) / per_wg));
    if (plan.partitioned)  // records mode: sized to the expected received entries (ZR_REC_WGS: A/B)
        P.setup_wgs = std::min<uint32_t>(
            P.setup_wgs, k.rec_wgs ? k.rec_wgs : records_setup_wgs((uint64_t)P.shard_count * P.route_cap, (uint32_t)cus));
    P.run_cap = std::min<uint32_t>(P.setup_wgs, kMaxRunsPerTile);
    uint32_t shift = 6;
    while ((1u << shift) < 64u * P.setup_batch) ++shift;
    while (((positions + (1ull << shift) - 1) >> shift) > 64ull * P.setup_wgs) ++shift;
    P.unit_shift = shift;
    P.units = (uint32_t)std::max<uint64_t>(1, (positions + (1ull << shift) - 1) >> shift);
    // a workgroup's bboxes live in LDS when they fit beside the histograms
    const uint64_t own_max = ((uint64_t)P.units + P.setup_wgs - 1) / P.setup_wgs;
    const uint64_t entries = own_max << shift;
    const uint64_t hist = setup_bin_lds_bytes(P.ntiles, 0);
    // (kSetupLdsBudget: one workgroup per CU owns the LDS; two measured slower)
    const uint64_t budget = std::min<uint64_t>(kSetupBboxLdsBytes, hist < kSetupLdsBudget ? kSetupLdsBudget - hist : 0);
    // (mesh: fans 1 and 2 keep their bboxes in global memory, so all of them do)
    P.bbox_lds = (!plan.mesh && entries * sizeof(BBox) <= budget) ? (uint32_t)entries : 0u;
    plan.stage_entries = entries;
}

}  // namespace

zr_result plan_draw(DrawParams& P, const DrawRequest& rq, const Knobs& k, const ShapeBook& book, DrawPlan& plan,
                    std::string& err) {
    plan = DrawPlan{};
    // A tile-row shard that owns no row of this target draws nothing, but a
    // partitioned one still routes its range and joins the exchange (every rank
    // calls the collective once per draw, zenith_raster.h).
    if (P.ntiles == 0 && !rq.exchange) {
        plan.nothing = true;
        return ZR_SUCCESS;
    }
    const uint64_t tpi = rq.vertex_count / 3u;
    const uint64_t prims = tpi * rq.instances;
    if (prims > kBinPrimMask) return plan_fail(err, ZR_ERROR_FEATURE_NOT_PRESENT, "more than 2^26-1 primitives in one draw");
    if (P.fb_w > 16384 || P.fb_h > 16384) return plan_fail(err, ZR_ERROR_FEATURE_NOT_PRESENT, "attachment larger than 16384");
    P.tris_per_instance = (uint32_t)tpi;
    P.prims = (uint32_t)prims;
    P.draw_prims = (uint32_t)prims;
    plan.prims = plan.positions = prims;
    plan.partitioned = rq.exchange;
    plan.mesh = P.program == kProgMesh;
    if (plan.partitioned && plan.mesh)
        return plan_fail(err, ZR_ERROR_FEATURE_NOT_PRESENT, "partitioned tile shards do not route clipped (mesh program) draws");
    if (plan.mesh && prims * kMeshFans > kBinPrimMask)
        return plan_fail(err, ZR_ERROR_FEATURE_NOT_PRESENT, "mesh program: more than (2^26-1)/3 primitives in one draw");
    if (plan.partitioned) {
        const zr_result rc = plan_route(P, rq, plan, err);
        if (rc) return rc;
    }
    plan_tile_edge(P, prims, k, book);
    if (P.ntiles > kMaxTilesPerPass)
        return plan_fail(err, ZR_ERROR_FEATURE_NOT_PRESENT,
                         "more owned tiles in one pass than the setup pass histogram holds (kMaxTilesPerPass)");
    plan_setup_grid(P, rq, k, plan);
    // k_setup_bin on the setup stream with two scratch sets (Knobs::setup_overlap);
    // not while debugging or with graph replay, whose captures bake in set 0
    plan.overlap_setup =
        (k.setup_overlap > 0 || (k.setup_overlap < 0 && use_overlap_setup(prims, P.fb_w, P.fb_h, P.shard_count))) &&
        !rq.graphs && !k.debug;
    // Overlapped and partitioned draws alternate between the scratch sets.
    // Partitioned draws always do: the route, exchange and setup of draw i+1 run
    // on their own streams while draw i's tile pass runs on the main stream
    // (DESIGN.md §7).  (ZR_SETUP_OVERLAP=0 serialises partitioned draws too: a
    // diagnostic that times each of their kernels alone)
    plan.overlap = (plan.partitioned && k.setup_overlap != 0) || plan.overlap_setup;
    // k_setup_bin phase 4 staged in LDS (pairs grouped by tile, stored run by run):
    // room for twice the workgroup's primitives, in the CU's LDS that setup owns
    // alone -- not beside a tile pass (overlapped setup), whose workgroups would
    // lose the LDS (C1 frame +1.9 us).  A workgroup whose pairs do not fit
    // scatters straight to the bins.
    {
        const uint64_t used = setup_bin_lds_bytes(P.ntiles, P.bbox_lds);
        const uint64_t cur = ((uint64_t)P.ntiles + 3u) / 4u * 4u * 4u;
        const uint64_t room = used + cur < kSetupLdsBudget ? (kSetupLdsBudget - used - cur) / 8u : 0u;
        const uint64_t cap = std::min<uint64_t>(room, 2u * std::max<uint64_t>(plan.stage_entries, 1024u));
        const bool on = k.bin_stage > 0 || (k.bin_stage < 0 && kBinStageDefault && !plan.overlap_setup);
        P.bin_stage = on && cap >= 1024u ? (uint32_t)cap : 0u;
    }
    const uint32_t cus = (uint32_t)std::max(rq.cu_count, 1);
    // (records mode never runs setup_finish: no effect there)
    P.micro = (k.micro < 0 ? use_micro_test(prims, (uint64_t)(P.ra_x1 - P.ra_x0 + 1) * (uint64_t)(P.ra_y1 - P.ra_y0 + 1))
                           : k.micro != 0) ? 1u : 0u;
    P.tile_threads = (k.tile_threads && P.tile_shift == kTileShift)
                         ? k.tile_threads
                         : tile_threads_for(P.ntiles, cus, prims, plan.partitioned, P.tile_shift);
    P.rec_table = (k.rec_table < 0 ? use_record_table(prims, P.tiles_x, P.tiles_y, P.tile_shift) : k.rec_table != 0) ? 1u : 0u;
    plan.sched = k.tile_sched < 0 ? use_tile_schedule(P.ntiles, cus, P.tile_threads, prims, P.tile_shift) : k.tile_sched != 0;
    // (a phase-1-only timing run never reaches the last workgroup's ticket, so it
    // writes no schedule: k_tile then keeps xcd_tile order instead of reading an
    // unwritten one)
    P.tile_sched = plan.sched && !(k.debug & kDebugPhase1Only) ? 1u : 0u;
    P.debug = k.debug;
    return ZR_SUCCESS;
}

// ------------------------------------------------------------------ ShapeBook

const BinShape* ShapeBook::find(uint32_t ntiles, uint32_t prims) const {
    const auto it = bin_shapes_.find(shape_key(ntiles, prims));
    return it == bin_shapes_.end() ? nullptr : &it->second;
}

uint32_t ShapeBook::take_slot(const DrawParams& P, bool capturing) {
    if (capturing || slab_keys_.size() >= kSlabSlots) return ~0u;
    slab_keys_.push_back(shape_key(P.ntiles, P.draw_prims));
    slab_tile_px_.push_back(1u << (2 * P.tile_shift));
    return (uint32_t)slab_keys_.size() - 1u;
}

ScratchSizes ShapeBook::sizes(const DrawParams& P, uint64_t bins_cap, bool sched, const Knobs& k) const {
    ScratchSizes z{};
    // the mesh program's fans 1 and 2 have records and bboxes of their own
    const bool mesh = P.program == kProgMesh;
    z.records = std::max<uint64_t>(P.prims, 1) * (mesh ? kMeshFans : 1u);
    z.mesh_edges = mesh ? std::max<uint64_t>(P.prims, 1) * 3u : 0u;
    z.tiles = (uint64_t)P.ntiles + 1;
    z.runs = (uint64_t)P.ntiles * P.run_cap;
    // (an allocation holds at least 1024 elements)
    z.bins = bins_cap ? bins_cap
                      : std::max<uint64_t>({bins_want_, k.initial_bins ? k.initial_bins : bin_default_capacity(z.records, P.ntiles),
                                            1024});
    // tile t's slab is bins[t * slab, (t + 1) * slab), the pool the rest.  Before
    // any measurement of the draw's shape: slabs of a third of the buffer.  After:
    // the buffer less the pool the shape's runs asked for (+25 %, and at least a
    // 64th of the buffer) over the tiles, but no less than the shape's target --
    // a buffer larger than the pairs need (the 2^20-entry floor; C2's 2 x prims)
    // goes to the slabs, where no run is needed (cerberus: the target slab put its
    // crowded tiles' excess in runs, setup +8 us).
    const uint64_t nt = std::max<uint32_t>(P.ntiles, 1u), cap = z.bins;
    const BinShape* shape = find(P.ntiles, P.draw_prims);
    uint64_t slab = cap / (3 * nt);
    if (k.forced_slab != ~0u) {
        slab = k.forced_slab;
    } else if (shape) {
        const uint64_t pool = std::max<uint64_t>((uint64_t)shape->pool * 5 / 4 + 4096, cap / 64);
        slab = std::max<uint64_t>({shape->target, bin_slab_whole(shape->target, shape->max_tile), cap > pool ? (cap - pool) / nt : 0});
    }
    slab = std::min<uint64_t>({slab, cap / nt, (uint64_t)kMaxSlab});
    z.slab = (uint32_t)slab;
    z.pool_off = (uint32_t)(slab * P.ntiles);
    z.pool_cap = (uint32_t)(cap - slab * P.ntiles);
    // Tile jobs (DrawParams::job_entries): for a shape whose longest list was long
    // (use_tile_jobs), or forced (ZR_JOBS).  The grid's spare blocks bound the jobs
    // beyond one per tile by the shape's pairs / J (pairs < tiles x target).
    const bool phase1 = (k.debug & kDebugPhase1Only) != 0;
    if (!phase1) {
        // (a shape not measured yet may be skewed: its first draw builds jobs for
        // whatever lists turn out long -- the clustered c2x scene's first frame
        // walked its 30-segment tile in one workgroup -- at the cost of the job
        // builder and the spare blocks once)
        if (k.jobs > 0)
            z.job_entries = (uint32_t)k.jobs;
        else if (k.jobs < 0 && (!shape || use_tile_jobs(shape->max_tile)))
            z.job_entries = kTileJobEntries;
    }
    if (z.job_entries) {
        // Key buffers (one per job of a split tile, kTilePixels x 8 B each) and the
        // grid's spare part blocks (job_pad / 8 per XCD: a tile's parts go to its
        // XCD).  A shape whose split was measured gets what it needed (+25 %): a draw
        // that did not fit is counted and rasterized unsplit, and the next draw of
        // its shape is sized from what it asked for.  A shape not measured yet gets
        // what the bin buffer's pairs can need at most -- each part past the first
        // holds job_entries pairs, each split tile more than job_entries -- within a
        // fixed memory bound (kJobKeyBytesFirst).
        uint64_t bufs, parts;
        if (shape && shape->job_bufs) {
            bufs = (uint64_t)shape->job_bufs * 5 / 4 + 16;
            parts = (uint64_t)shape->job_parts * 5 / 4 + 8;
        } else {
            const uint64_t pairs = shape ? (uint64_t)P.ntiles * shape->target + shape->pool : cap;
            bufs = std::min<uint64_t>(2 * (pairs / z.job_entries) + 64, kJobKeyBytesFirst / (8ull << (2 * P.tile_shift)));
            parts = pairs / z.job_entries / 4 + 64;  // (a few crowded tiles: parts spread over several XCDs)
        }
        z.job_pad = (uint32_t)std::min<uint64_t>(8 * parts, 1u << 20);
        z.job_slots = (uint32_t)std::min<uint64_t>(bufs, 1u << 20);
        z.job_slot = P.ntiles;
        z.job_keys = (uint64_t)z.job_slots << (2 * P.tile_shift);
        z.job_tickets = z.job_slots;
    }
    if ((sched || z.job_entries) && !phase1) z.tile_order = (uint64_t)P.ntiles + z.job_pad;
    return z;
}

// Bin buffer sizing: later draws take slabs of the target the
// draws since the last sync asked for, and the buffer grows to what they asked
// for -- slabs plus the pool their runs needed -- when it is smaller (a draw with
// a dropped run rasterized that tile by k_tile's record scan).  Every
// kBinShrinkSyncs syncs it shrinks to the most any of them asked for when it is
// more than twice that and the difference is worth it (kBinShrinkMin): not
// per sync (a device alternating between a light and a heavy scene would
// reallocate, and drop runs, every time), and not for a few MB (a shrink of
// the 8-way shard emulation's small buffers cost one rank 7 us per frame).  (Capped at 2^30
// entries, 4 GiB: a larger draw keeps using the exact spill path.)
SyncDecision ShapeBook::end_interval(volatile uint32_t* st, const uint64_t bins_cap[kScratchSets],
                                     const uint64_t job_keys_cap[kScratchSets], const Knobs& k) {
    SyncDecision dec;
    uint64_t need = st[kStBinNeed];  // (draws with a dropped run; the others from their slots)
    st[kStBinNeed] = 0;
    for (size_t i = 0; i < slab_keys_.size(); ++i) {
        const uint32_t target = st[kStSlabSlot0 + i], pool = st[kStPoolSlot0 + i], max_tile = st[kStMaxSlot0 + i];
        const uint32_t job_bufs = st[kStJobBufSlot0 + i], job_parts = st[kStJobPartSlot0 + i];
        st[kStJobBufSlot0 + i] = 0;
        st[kStJobPartSlot0 + i] = 0;
        job_want_max_ = std::max<uint64_t>(job_want_max_, (uint64_t)job_bufs * slab_tile_px_[i]);
        if (!target) continue;
        need = std::max<uint64_t>({need, (slab_keys_[i] >> 32) * target + pool,
                                   (slab_keys_[i] >> 32) * bin_slab_whole(target, max_tile) + 4096});
        st[kStSlabSlot0 + i] = 0;
        st[kStPoolSlot0 + i] = 0;
        st[kStMaxSlot0 + i] = 0;
        if (bin_shapes_.size() >= 1024) bin_shapes_.clear();  // (shapes that come and go)
        BinShape& v = bin_shapes_[slab_keys_[i]];
        if (v.target != target || v.pool != pool) dec.gen_bumps++;  // recorded graphs bake the slab in
        if (use_tile_jobs(v.max_tile) != use_tile_jobs(max_tile)) dec.gen_bumps++;
        if (v.job_bufs != job_bufs || v.job_parts != job_parts) dec.gen_bumps++;
        v = BinShape{target, pool, max_tile, job_bufs, job_parts};
    }
    slab_keys_.clear();
    slab_tile_px_.clear();
    if (!need) return dec;
    bins_want_ = std::min<uint64_t>(std::max<uint64_t>(need + need / 10 + 4096, 1ull << 20), 1ull << 30);
    bins_want_max_ = std::max(bins_want_max_, bins_want_);
    const bool check = k.shrink_syncs && ++bins_syncs_ >= k.shrink_syncs;
    for (uint32_t s = 0; s < kScratchSets; ++s) {
        const uint64_t cap = bins_cap[s];
        const bool shrink = check && cap > 2 * bins_want_max_ && cap - bins_want_max_ >= kBinShrinkMin;
        if (!cap || (cap >= need && !shrink)) continue;
        dec.bins_realloc[s] = check ? bins_want_max_ : bins_want_;
        dec.gen_bumps++;
    }
    if (check) {
        // tile-job key buffers (8 B per pixel of a tile each) follow the most
        // any draw of the interval asked for, the same way
        const uint64_t keep = job_want_max_ ? job_want_max_ * 5 / 4 + 16 * (uint64_t)kTilePixels : 0;  // (keys)
        for (uint32_t s = 0; s < kScratchSets; ++s) {
            if (!job_keys_cap[s] || job_keys_cap[s] <= 2 * keep + (1u << 16)) continue;
            dec.drop_job_keys[s] = true;
            dec.gen_bumps++;
        }
        job_want_max_ = 0;
        bins_want_max_ = 0;
        bins_syncs_ = 0;
    }
    return dec;
}

}  // namespace zr
