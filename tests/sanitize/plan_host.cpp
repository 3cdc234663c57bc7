// plan_host.cpp — the draw plan and the shape table (zenith_amd/csrc/zr_plan.cpp) on
// the host alone, under ASan + UBSan (tests/test_sanitize.py): no device, no kernels.
// Every expected value is worked out by hand from the planning rules as they stood
// in exec_draw / ensure_scratch / device_sync before they moved into zr_plan.cpp
// (256 CUs, default knobs unless a case sets one).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "zr_plan.h"

using namespace zr;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

struct Planned {
    DrawParams P;
    DrawPlan plan;
    zr_result rc;
    std::string err;
};

// What fill_target and bind_inputs leave in P, then plan_draw.
static Planned plan(uint64_t prims, uint32_t w, uint32_t h, int32_t program, int32_t depth_mode, const Knobs& k,
                    const ShapeBook& book, uint32_t rank = 0, uint32_t count = 1, bool exchange = false,
                    uint32_t route_cap = 0) {
    Planned r;
    memset(&r.P, 0, sizeof r.P);
    r.P.fb_w = w;
    r.P.fb_h = h;
    r.P.ra_x1 = (int32_t)w - 1;
    r.P.ra_y1 = (int32_t)h - 1;
    r.P.shard_rank = rank;
    r.P.shard_count = count;
    r.P.program = program;
    r.P.depth_mode = depth_mode;
    set_tiles(r.P, kTileShift);
    DrawRequest rq;
    rq.vertex_count = prims * 3;
    rq.instances = 1;
    rq.exchange = exchange;
    rq.route_cap = route_cap;
    rq.cu_count = 256;
    r.rc = plan_draw(r.P, rq, k, book, r.plan, r.err);
    return r;
}

static Knobs knobs_with(const char* name, const char* value) {
    setenv(name, value, 1);
    const Knobs k = read_knobs();
    unsetenv(name);
    return k;
}

static const int32_t kLess = kDepthMinStrict;  // LESS + depth write

static void test_configs() {
    const Knobs k;
    const ShapeBook book;
    {  // C2
        const Planned r = plan(1000000, 1920, 1080, kProgBlinn, kLess, k, book);
        const DrawParams& P = r.P;
        CHECK(r.rc == ZR_SUCCESS && !r.plan.nothing && !r.plan.partitioned && !r.plan.mesh);
        CHECK(P.tris_per_instance == 1000000 && P.prims == 1000000 && P.draw_prims == 1000000);
        CHECK(r.plan.prims == 1000000 && r.plan.positions == 1000000 && r.plan.span == 0);
        CHECK(P.tile_shift == 5 && P.tiles_x == 60 && P.tiles_y == 34 && P.ntiles == 2040);
        CHECK(P.setup_batch == 2 && P.setup_wgs == 256 && P.unit_shift == 7 && P.units == 7813);
        CHECK(setup_bin_lds_bytes(2040, 0) == 10592);
        CHECK(P.bbox_lds == 3968 && r.plan.stage_entries == 3968);
        CHECK(r.plan.overlap_setup && r.plan.overlap && P.bin_stage == 0);
        CHECK(P.micro == 0 && P.tile_threads == 512 && P.rec_table == 1 && P.tile_sched == 0 && !r.plan.sched);
        CHECK(P.run_cap == 256 && P.debug == 0);
    }
    {  // C1
        const Planned r = plan(100000, 1920, 1080, kProgBlinn, kLess, k, book);
        CHECK(r.rc == ZR_SUCCESS && r.P.tile_shift == 5 && r.P.ntiles == 2040 && r.P.tile_threads == 256);
        CHECK(r.plan.overlap_setup && r.plan.overlap);
    }
    {  // C3: 8160 32-px tiles of >= 64 primitives each
        const Planned r = plan(1000000, 3840, 2160, kProgBlinn, kLess, k, book);
        CHECK(r.rc == ZR_SUCCESS && r.P.tile_shift == 6 && r.P.tiles_x == 60 && r.P.tiles_y == 34 && r.P.ntiles == 2040);
        CHECK(r.P.tile_threads == 512);
    }
    {  // C4: at least one primitive per pixel
        const Planned r = plan(10000000, 1920, 1080, kProgBlinn, kLess, k, book);
        const DrawParams& P = r.P;
        CHECK(r.rc == ZR_SUCCESS && P.tile_shift == 6 && P.tiles_x == 30 && P.tiles_y == 17 && P.ntiles == 510);
        CHECK(P.tile_threads == 1024 && P.micro == 1);
        CHECK(!r.plan.overlap_setup && !r.plan.overlap);
        CHECK(P.setup_wgs == 256 && P.unit_shift == 10 && P.units == 9766 && P.bbox_lds == 0);
        CHECK(P.bin_stage > 0 && P.bin_stage == 19664);  // (160 KiB - 4480 B of histograms - 2048 B of cursors) / 8
    }
    {  // cerberus: the mesh program has no 16- or 64-px instance
        const Planned r = plan(33543, 1920, 1080, kProgMesh, kLess, k, book);
        const DrawParams& P = r.P;
        CHECK(r.rc == ZR_SUCCESS && r.plan.mesh && P.tile_shift == 5 && P.ntiles == 2040);
        CHECK(P.setup_batch == 1 && P.setup_wgs == 33 && P.bbox_lds == 0);
        CHECK(P.tile_threads == 512 && P.tile_sched == 1 && r.plan.sched);
    }
    {  // C2 partitioned, rank 3 of 8
        const Planned r = plan(1000000, 1920, 1080, kProgBlinn, kLess, k, book, 3, 8, true);
        const DrawParams& P = r.P;
        CHECK(r.rc == ZR_SUCCESS && r.plan.partitioned && r.plan.overlap && r.plan.overlap_setup);
        CHECK(r.plan.span == 125440 && P.route_chunks == 245 && P.route_cap == 35456);
        CHECK(P.route_lo == 376320 && P.route_hi == 501760);
        CHECK(P.prims == 1000000 && r.plan.positions == 1000000 && P.draw_prims == 1000000);
        CHECK(P.tile_shift == 5 && P.ntiles == 255 && P.tile_threads == 512);
        CHECK(records_setup_wgs(283648, 256) == 139 && P.setup_wgs == 139 && P.run_cap == 139);
    }
    {  // a shard that owns no tile: 2 x 1 tiles over 8 ranks, rank 7
        const Planned r = plan(1000, 64, 32, kProgFlat, kLess, k, book, 7, 8, false);
        CHECK(r.rc == ZR_SUCCESS && r.plan.nothing);
        const Planned x = plan(1000, 64, 32, kProgFlat, kLess, k, book, 7, 8, true);  // ... still joins its exchange
        CHECK(x.rc == ZR_SUCCESS && !x.plan.nothing && x.P.ntiles == 0 && x.plan.partitioned);
    }
}

static void test_limits() {
    const Knobs k;
    const ShapeBook book;
    Planned r = plan(1ull << 26, 1920, 1080, kProgBlinn, kLess, k, book);
    CHECK(r.rc == ZR_ERROR_FEATURE_NOT_PRESENT && r.err == "more than 2^26-1 primitives in one draw");
    r = plan((1ull << 26) - 1, 1920, 1080, kProgBlinn, kLess, k, book);
    CHECK(r.rc == ZR_SUCCESS);
    r = plan(1000, 16385, 64, kProgBlinn, kLess, k, book);
    CHECK(r.rc == ZR_ERROR_FEATURE_NOT_PRESENT && r.err == "attachment larger than 16384");
    r = plan(((1ull << 26) - 1) / 3 + 1, 1920, 1080, kProgMesh, kLess, k, book);
    CHECK(r.rc == ZR_ERROR_FEATURE_NOT_PRESENT && r.err == "mesh program: more than (2^26-1)/3 primitives in one draw");
    r = plan(((1ull << 26) - 1) / 3, 1920, 1080, kProgMesh, kLess, k, book);
    CHECK(r.rc == ZR_SUCCESS);
    r = plan(1000, 1920, 1080, kProgMesh, kLess, k, book, 1, 4, true);
    CHECK(r.rc == ZR_ERROR_FEATURE_NOT_PRESENT &&
          r.err == "partitioned tile shards do not route clipped (mesh program) draws");
    // 3 ranks x a whole span (22,369,792) each: 67,109,376 block positions
    r = plan((1ull << 26) - 1, 1920, 1080, kProgBlinn, kLess, k, book, 0, 3, true, 22369792);
    CHECK(r.rc == ZR_ERROR_FEATURE_NOT_PRESENT && r.err == "partitioned draw: more than 2^26-1 block positions");
    r = plan(1000, 8192, 8192, kProgFlat, kLess, k, book);  // 65,536 tiles of 32 px
    CHECK(r.rc == ZR_ERROR_FEATURE_NOT_PRESENT &&
          r.err == "more owned tiles in one pass than the setup pass histogram holds (kMaxTilesPerPass)");
}

static void test_knobs() {
    const ShapeBook book;
    Knobs k = knobs_with("ZR_TILE", "16");
    CHECK(k.forced_tile_shift == 4);
    Planned r = plan(1000000, 1920, 1080, kProgBlinn, kLess, k, book);
    CHECK(r.P.tile_shift == 4 && r.P.tiles_x == 120 && r.P.tiles_y == 68 && r.P.ntiles == 8160 && r.P.tile_threads == 256);
    r = plan(33543, 1920, 1080, kProgMesh, kLess, k, book);  // no 16-px instance of the mesh program
    CHECK(r.P.tile_shift == 5 && r.P.ntiles == 2040);
    r = plan(1000000, 1920, 1080, kProgBlinn, kDepthLastWins, k, book);  // ... nor without a depth write
    CHECK(r.P.tile_shift == 5);
    k = knobs_with("ZR_TILE_NT", "512");
    CHECK(k.tile_threads == 512);
    CHECK(plan(100000, 1920, 1080, kProgBlinn, kLess, k, book).P.tile_threads == 512);     // 32 px: forced (256 by default)
    CHECK(plan(10000000, 1920, 1080, kProgBlinn, kLess, k, book).P.tile_threads == 1024);  // 64 px: not
    CHECK(knobs_with("ZR_TILE_NT", "100").tile_threads == 256);
    CHECK(knobs_with("ZR_JOBS", "100").jobs == 256 && knobs_with("ZR_JOBS", "0").jobs == 0 && Knobs().jobs == -1);
    CHECK(knobs_with("ZR_JOBS", "4096").jobs == 4096);
    k = knobs_with("ZR_SETUP_OVERLAP", "0");
    r = plan(1000000, 1920, 1080, kProgBlinn, kLess, k, book, 3, 8, true);
    CHECK(k.setup_overlap == 0 && r.plan.partitioned && !r.plan.overlap && !r.plan.overlap_setup);
    CHECK(r.P.bin_stage > 0);  // (setup alone on its CUs: staged)
    CHECK(knobs_with("ZR_BIN_CAPACITY", "1").initial_bins == 64 && knobs_with("ZR_BIN_CAPACITY", "0x80000000").initial_bins == 1u << 30);
    CHECK(knobs_with("ZR_BIN_SLAB", "99999999").forced_slab == kMaxSlab && Knobs().forced_slab == ~0u);
    CHECK(knobs_with("ZR_SETUP_BATCH", "3").setup_batch == 0 && knobs_with("ZR_SETUP_BATCH", "4").setup_batch == 4);
    CHECK(knobs_with("ZR_GRAPH", "1").use_graphs && knobs_with("ZR_DEBUG", "0x20").debug == kDebugPhase1Only);
    CHECK(knobs_with("ZR_BIN_SHRINK_SYNCS", "0").shrink_syncs == 0 && Knobs().shrink_syncs == 16);
}

// One sync interval with one draw of `P`'s shape reporting these status words.
static SyncDecision interval(ShapeBook& book, const DrawParams& P, uint32_t target, uint32_t pool, uint32_t max_tile,
                             uint32_t job_bufs, uint32_t job_parts, const uint64_t bins_cap[kScratchSets],
                             const uint64_t job_keys_cap[kScratchSets], const Knobs& k) {
    uint32_t st[kStWords] = {};
    const uint32_t slot = book.take_slot(P, false);
    CHECK(slot == 0);
    st[kStSlabSlot0 + slot] = target;
    st[kStPoolSlot0 + slot] = pool;
    st[kStMaxSlot0 + slot] = max_tile;
    st[kStJobBufSlot0 + slot] = job_bufs;
    st[kStJobPartSlot0 + slot] = job_parts;
    const SyncDecision dec = book.end_interval(st, bins_cap, job_keys_cap, k);
    for (uint32_t w = 0; w < kStWords; ++w) CHECK(st[w] == 0);  // consumed
    return dec;
}

static const uint64_t kNone[kScratchSets] = {0, 0, 0};

static void test_sizes() {
    const Knobs k;
    ShapeBook book;
    const DrawParams P = plan(1000000, 1920, 1080, kProgBlinn, kLess, k, book).P;  // C2: 2040 tiles
    // unmeasured, the set's first draw: 2 x prims + 256 per tile = 2,522,240 entries
    ScratchSizes z = book.sizes(P, 0, false, k);
    CHECK(z.bins == 2522240 && z.slab == 2522240 / (3 * 2040) && z.slab == 412);
    CHECK(z.pool_off == 840480 && z.pool_cap == 1681760);
    CHECK(z.job_entries == kTileJobEntries && z.job_slots == 2526 && z.job_pad == 8 * 371);  // min(2 * 1231 + 64, 8192); 1231 / 4 + 64 parts
    CHECK(z.records == 1000000 && z.mesh_edges == 0 && z.tiles == 2041 && z.runs == 2040 * 256);
    CHECK(z.job_slot == 2040 && z.job_keys == 2526ull << 10 && z.job_tickets == 2526 && z.tile_order == 2040 + 2968);
    z = book.sizes(P, 1ull << 27, false, k);  // the key-buffer bound: 64 MiB / 8 KiB
    CHECK(z.bins == 1ull << 27 && z.job_slots == 8192 && z.slab == 21931);
    DrawParams P16 = P;
    set_tiles(P16, 4);
    CHECK(book.sizes(P16, 1ull << 27, false, k).job_slots == 32768);  // 64 MiB / 2 KiB
    // uniform: target 785, longest list 741, no pool
    const uint64_t caps[kScratchSets] = {2522240, 0, 0};
    SyncDecision dec = interval(book, P, 785, 0, 741, 0, 0, caps, kNone, k);
    CHECK(dec.gen_bumps == 1 && !dec.bins_realloc[0] && !dec.bins_realloc[1] && !dec.drop_job_keys[0]);
    CHECK(book.bins_want() == 1601400 + 160140 + 4096);
    z = book.sizes(P, 2522240, false, k);
    CHECK(z.job_entries == 0 && z.job_pad == 0 && z.job_slots == 0 && z.job_keys == 0 && z.tile_order == 0);
    CHECK(z.slab == 1217 && z.pool_off == 1217 * 2040 && z.pool_cap == 2522240 - 1217 * 2040);  // (cap - cap / 64) / 2040
    CHECK(book.sizes(P, 2522240, true, k).tile_order == 2040);
    dec = interval(book, P, 785, 0, 741, 0, 0, caps, kNone, k);  // the same again: nothing changes
    CHECK(dec.gen_bumps == 0);
    dec = interval(book, P, 785, 0, 29700, 0, 0, caps, kNone, k);  // now needs jobs: one bump
    CHECK(dec.gen_bumps == 1);
    // measured job split: what it needed + 25 %
    dec = interval(book, P, 785, 0, 29700, 100, 40, caps, kNone, k);
    CHECK(dec.gen_bumps == 1);
    z = book.sizes(P, 2522240, false, k);
    CHECK(z.job_entries == 2048 && z.job_slots == 141 && z.job_pad == 8 * 58 && z.tile_order == 2040 + 464);
    CHECK(z.slab == 1217);  // (29,700 is no whole-list slab: the buffer less its pool, over the tiles)
}

static void test_crowded_edges() {
    const Knobs k;
    for (int big = 0; big < 2; ++big) {
        ShapeBook book;
        const uint32_t w = big ? 3840 : 1920, h = big ? 2160 : 1080;
        Planned r = plan(1000000, w, h, kProgBlinn, kLess, k, book);
        CHECK(r.P.tile_shift == (big ? 6u : 5u) && r.P.ntiles == 2040);
        const uint64_t caps[kScratchSets] = {1ull << 24, 0, 0};
        interval(book, r.P, 785, 0, 29700, 0, 0, caps, kNone, k);
        r = plan(1000000, w, h, kProgBlinn, kLess, k, book);
        CHECK(r.P.tile_shift == (big ? 5u : 4u) && r.P.ntiles == 8160);  // (4K: 32,400 tiles of 16 px are too many)
        interval(book, r.P, 300, 0, 8000, 0, 0, caps, kNone, k);
        r = plan(1000000, w, h, kProgBlinn, kLess, k, book);
        CHECK(r.P.tile_shift == (big ? 5u : 4u) && r.P.ntiles == 8160);
    }
}

static void test_slots_and_wants() {
    const Knobs k;
    ShapeBook book;
    DrawParams P = plan(1000000, 1920, 1080, kProgBlinn, kLess, k, book).P;
    CHECK(book.take_slot(P, true) == ~0u);  // capturing
    for (uint32_t i = 0; i < kSlabSlots; ++i) CHECK(book.take_slot(P, false) == i);
    CHECK(kSlabSlots == 48 && book.take_slot(P, false) == ~0u);  // the 49th draw
    uint32_t st[kStWords] = {};
    CHECK(book.end_interval(st, kNone, kNone, k).gen_bumps == 0 && book.bins_want() == 0);
    CHECK(book.take_slot(P, false) == 0);
    book.end_interval(st, kNone, kNone, k);
    // the want: need + 10 % + 4096, within [2^20, 2^30]; a smaller buffer is reallocated
    const uint64_t caps[kScratchSets] = {1000000, 2522240, 0};
    SyncDecision dec = interval(book, P, 785, 0, 741, 0, 0, caps, kNone, k);
    CHECK(book.bins_want() == 1765636 && dec.bins_realloc[0] == 1765636 && !dec.bins_realloc[1] && !dec.bins_realloc[2]);
    CHECK(dec.gen_bumps == 2);
    DrawParams small = P;
    small.fb_w = small.fb_h = 32;
    set_tiles(small, 5);
    small.draw_prims = 10;
    interval(book, small, 70, 0, 5, 0, 0, kNone, kNone, k);
    CHECK(book.bins_want() == 1u << 20);
    st[kStBinNeed] = 0xFFFFFFFFu;
    dec = book.end_interval(st, caps, kNone, k);
    CHECK(book.bins_want() == 1u << 30 && st[kStBinNeed] == 0 && dec.bins_realloc[0] == 1u << 30 && dec.bins_realloc[1] == 1u << 30);
}

static void test_shrink() {
    DrawParams P = plan(1000000, 1920, 1080, kProgBlinn, kLess, Knobs(), ShapeBook()).P;
    // want 1,765,636: 2^26 shrinks; 18,000,000 would free < kBinShrinkMin; 3,000,000 is < 2 x the want
    const uint64_t caps[kScratchSets] = {1ull << 26, 18000000, 3000000};
    // job keys: 100 buffers x 1024 px -> keep 144,384; dropped above 2 x keep + 2^16 = 354,304
    const uint64_t keys[kScratchSets] = {354304, 354305, 0};
    for (const uint32_t syncs : {16u, 0u}) {
        Knobs k;
        k.shrink_syncs = syncs;
        ShapeBook book;
        for (int i = 1; i <= 20; ++i) {
            const SyncDecision dec = interval(book, P, 785, 0, 741, i == 3 ? 100 : 0, i == 3 ? 7 : 0, caps, keys, k);
            const bool check = syncs && i == 16;
            CHECK(dec.bins_realloc[0] == (check ? 1765636u : 0u) && !dec.bins_realloc[1] && !dec.bins_realloc[2]);
            CHECK(!dec.drop_job_keys[0] && dec.drop_job_keys[1] == check && !dec.drop_job_keys[2]);
            CHECK(dec.gen_bumps == (i == 1 || i == 3 || i == 4 ? 1u : 0u) + (check ? 2u : 0u));
        }
    }
}

static void test_shape_limit() {
    const Knobs k;
    ShapeBook book;
    DrawParams P;
    memset(&P, 0, sizeof P);
    P.tile_shift = 5;
    P.draw_prims = 100;
    for (uint32_t n = 1; n <= 1025; ++n) {
        P.ntiles = n;
        interval(book, P, 100, 0, 90, 0, 0, kNone, kNone, k);
        CHECK(book.shapes() == (n <= 1024 ? n : 1u));
    }
    CHECK(book.find(1025, 100) && !book.find(1, 100));
    // 5 significant bits of the primitive count
    CHECK(shape_key(2040, 1000000) == ((2040ull << 32) | 983040u) && shape_key(2040, 1015807) == shape_key(2040, 983040));
    CHECK(shape_key(7, 31) == ((7ull << 32) | 31u) && shape_key(0, 0) == 0);
}

int main() {
    CHECK(route_capacity_default(125440, 8) == 35456 && route_capacity_default(125440, 2) == 125440);
    CHECK(choose_depth_mode(true, true, 1) == kDepthMinStrict && choose_depth_mode(true, false, 1) == kDepthLastWins &&
          choose_depth_mode(false, true, 1) == kDepthLastWins && choose_depth_mode(true, true, 6) == kDepthMaxNonStrict);
    test_configs();
    test_limits();
    test_knobs();
    test_sizes();
    test_crowded_edges();
    test_slots_and_wants();
    test_shrink();
    test_shape_limit();
    if (g_failed) {
        fprintf(stderr, "plan_host: %d checks failed\n", g_failed);
        return 1;
    }
    printf("plan_host ok\n");
    return 0;
}
