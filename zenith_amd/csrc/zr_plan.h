// zr_plan.h — the host-only policy of a draw: the environment overrides (Knobs),
// the per-draw plan (plan_draw: counts, route geometry, tile edge, grids) and the
// per-shape scratch sizing with its feedback from the status words (ShapeBook).
// Plain integer arithmetic: no HIP call, no device, stream or event in here; the
// runtime (zr_runtime.cpp) binds pointers, allocates and enqueues what this plans.
#pragma once
#include <hip/hip_vector_types.h>  // (types only: DrawParams has float4 / uint2 pointers)
#include <math.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "zenith_raster.h"
#include "zr_internal.h"

namespace zr {

// Every ZR_* environment override, read once per device (read_knobs).
struct Knobs {
    // ZR_SETUP_OVERLAP=0 / 1 forces k_setup_bin off / onto the setup stream, where
    // draw i+1's setup fills CUs draw i's tile pass frees; -1: use_overlap_setup
    // (round 6, us per frame: C2 107.7 -> 95.5, C3 206.8 -> 196.9, c2x 155.2 ->
    // 133.7, but C4 316.9 -> 405.8: its HBM-bound setup is the frame)
    int setup_overlap = -1;
    int rec_table = -1;        // ZR_REC_TABLE=0/1 forces k_tile's record table (A/B); -1: use_record_table
    int tile_sched = -1;       // ZR_TILE_SCHED=0/1 forces the heaviest-first tile schedule (A/B); -1: use_tile_schedule
    uint32_t rec_wgs = 0;      // ZR_REC_WGS: k_setup_bin workgroups of partitioned (records-mode) draws; 0: one per CU
    int bin_stage = -1;        // ZR_BIN_STAGE: k_setup_bin phase 4 staged through LDS (1), direct (0), default (-1)
    int micro = -1;            // ZR_MICRO=0/1: setup's micro-primitive test off / on; -1: use_micro_test
    uint32_t tile_threads = 0; // ZR_TILE_NT: k_tile workgroup size override (256, 512; 0 = by tile count)
    uint32_t debug = 0;        // ZR_DEBUG: kDebug* bits
    uint64_t initial_bins = 0; // ZR_BIN_CAPACITY; 0 = bin_default_capacity of the first draw
    uint32_t shrink_syncs = kBinShrinkSyncs;  // ZR_BIN_SHRINK_SYNCS (0: never shrink)
    int jobs = -1;             // ZR_JOBS: tile jobs of N entries (tests), 0 off; -1: use_tile_jobs
    uint32_t setup_batch = 0;  // ZR_SETUP_BATCH: primitives per lane in flight (1, 2, 4; 0: 2)
    uint32_t forced_tile_shift = 0;  // ZR_TILE: every unsharded draw with a built instance at this edge (16 / 32 / 64)
    uint32_t forced_slab = ~0u;      // ZR_BIN_SLAB: every draw's slab (tests: pool runs everywhere)
    bool use_graphs = false;   // ZR_GRAPH=1: replay resubmitted command lists as HIP graphs
    std::string dbg_ts_path;   // ZR_DEBUG_TS: where kDebugStamps runs append their phase durations
};
Knobs read_knobs();

// Measurements of one draw shape (shape_key), from the status slots of its last draw.
struct BinShape {
    uint32_t target = 0;    // bin_slab_target
    uint32_t pool = 0;      // pool entries its runs asked for (at the slab it had)
    uint32_t max_tile = 0;  // its longest tile list
    uint32_t job_bufs = 0;  // tile-job key buffers its split tiles needed (0: none built)
    uint32_t job_parts = 0; // ... and the most parts it put on one XCD
};

// A draw shape's key for the bin / job measurements: its tile count and its
// primitive count to 5 significant bits, so draws whose count varies a little
// (culling, LOD, streaming) share their measurements.
uint64_t shape_key(uint32_t ntiles, uint32_t prims);

// Entries per exchange block when the caller sets none: every primitive of the
// range for two ranks or fewer, else twice a uniform share plus a margin.  A block
// that still overflows is exact (its receiver sets up the whole draw), only slower.
uint64_t route_capacity_default(uint64_t span, uint64_t G);

int32_t choose_depth_mode(bool test, bool write, int32_t op);

// The draw's tiles at an edge of 1 << shift pixels: the grid, and the tiles this
// shard owns (ShardGeom), from P.fb_w / fb_h and P.shard_rank / shard_count.
void set_tiles(DrawParams& P, uint32_t shift);

// What a scratch set's buffers must hold for one draw, and the draw's slab / pool /
// tile-job geometry in its bin buffer (ShapeBook::sizes).
struct ScratchSizes {
    uint32_t slab, pool_off, pool_cap;
    uint32_t job_entries, job_pad, job_slots;
    // element counts (0 for mesh_edges, the job buffers and tile_order: not used by this draw)
    uint64_t records;      // records, records_big and bboxes
    uint64_t mesh_edges;
    uint64_t tiles;        // tile_counts and run_counts
    uint64_t runs;
    uint64_t bins;         // the set's bin buffer: its capacity, or what its first draw allocates
    uint64_t job_slot, job_keys, job_tickets;
    uint64_t tile_order;
};

// What the runtime does to the scratch sets at the end of a sync interval.
struct SyncDecision {
    uint32_t gen_bumps = 0;                  // times scratch_gen is bumped (recorded graphs bake the sizes in)
    uint64_t bins_realloc[kScratchSets] = {};  // != 0: free the set's bin buffer and allocate this many entries
    bool drop_job_keys[kScratchSets] = {};     // free the set's job key and ticket buffers
};

// The shape table: what each draw shape's last draw measured, the draws of the
// current sync interval in status-slot order, and the bin / job buffer wants.
class ShapeBook {
public:
    // The shape's measurements, or nullptr before its first sync point.
    const BinShape* find(uint32_t ntiles, uint32_t prims) const;
    // The status slot of the interval's next draw (DrawParams::stat_slot), or ~0u
    // when capturing or past kSlabSlots.
    uint32_t take_slot(const DrawParams& P, bool capturing);
    // `bins_cap`: the set's bin buffer (entries), 0 when it has none yet.  `sched`:
    // the draw asked for a tile schedule (DrawPlan::sched).
    ScratchSizes sizes(const DrawParams& P, uint64_t bins_cap, bool sched, const Knobs& k) const;
    // `st`: the kStWords status words (the bin / slot words are consumed and
    // cleared); per set its bin buffer and job key buffer entries, 0 for none.
    SyncDecision end_interval(volatile uint32_t* st, const uint64_t bins_cap[kScratchSets],
                              const uint64_t job_keys_cap[kScratchSets], const Knobs& k);
    uint64_t bins_want() const { return bins_want_; }
    size_t shapes() const { return bin_shapes_.size(); }

private:
    std::unordered_map<uint64_t, BinShape> bin_shapes_;
    std::vector<uint64_t> slab_keys_;      // shape of the draw in each status slot
    std::vector<uint32_t> slab_tile_px_;   // ... and its pixels per tile
    uint64_t bins_want_ = 0;      // bin buffer the last sync's draws asked for (+10 %; 0: none measured yet)
    uint64_t bins_want_max_ = 0;  // ... the most any sync asked for since the last shrink check
    uint32_t bins_syncs_ = 0;     // syncs with draws since the last shrink check
    uint64_t job_want_max_ = 0;   // the most job keys (buffers x tile pixels) a draw asked for since the last shrink check
};

// plan_draw's input besides the DrawParams fields it reads: the target
// (fb_w, fb_h, ra_*), the shard (shard_rank, shard_count), program and depth_mode.
struct DrawRequest {
    uint64_t vertex_count = 0, instances = 0;  // of the draw call (indices when indexed)
    bool exchange = false;   // a partitioned shard (zr_cmd_set_tile_shard_exchange)
    uint32_t route_cap = 0;  // zr_cmd_set_route_capacity; 0: route_capacity_default
    int cu_count = 0;
    bool graphs = false;     // command lists replay as HIP graphs
};

// The host-only decisions of a draw.
struct DrawPlan {
    bool nothing = false;      // a shard that owns no tile and joins no exchange: no work at all
    uint64_t prims = 0;        // primitives of the draw
    uint64_t positions = 0;    // setup positions: prims, or the received blocks' when partitioned
    uint64_t span = 0;         // partitioned: primitives each rank routes
    bool partitioned = false, mesh = false;
    bool overlap_setup = false;  // k_setup_bin on the setup stream beside the previous tile pass
    bool overlap = false;        // the draw alternates scratch sets (overlap_setup, or partitioned)
    bool sched = false;          // k_setup_bin builds the heaviest-first tile schedule
    uint64_t stage_entries = 0;  // primitives of the busiest setup workgroup
};

// Fills P's counts (tris_per_instance, prims, draw_prims), route geometry
// (route_cap, route_chunks, route_lo, route_hi), tile_shift and the tile grid,
// setup_batch, setup_wgs, unit_shift, units, bbox_lds, bin_stage, micro,
// tile_threads, rec_table, tile_sched, run_cap and debug.  A draw past a limit
// returns its error code and sets `err`.
zr_result plan_draw(DrawParams& P, const DrawRequest& rq, const Knobs& k, const ShapeBook& book, DrawPlan& plan,
                    std::string& err);

}  // namespace zr
