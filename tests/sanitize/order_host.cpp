// order_host.cpp — the draw path's index arithmetic (zenith_amd/csrc/zr_order.h) on the
// host alone, under ASan + UBSan (tests/test_sanitize.py): no device, no kernels.
// Expected values are worked out by hand from the rules as they stood inside
// k_setup_bin and k_tile before they moved into zr_order.h (default build knobs).
#include <cstdio>
#include <vector>

#include "zr_order.h"  // (first: it brings the vector types zr_internal.h names)
#include "zr_internal.h"

using namespace zr;

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (g_failed < 20) fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

// ---- XCD tile order
static void check_xcd(uint32_t n) {
    const uint32_t K = ZR_XCD_TILES > 1 ? ZR_XCD_TILES : 1u;
    const uint32_t whole = ZR_XCD_TILES > 1 ? n / (8u * K) * (8u * K) : 0u;
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t b = 0; b < n; ++b) {
        const uint32_t t = xcd_tile(b, n);
        CHECK(t < n);
        if (t >= n) return;
        CHECK(!seen[t]);  // a permutation of [0, n)
        seen[t] = 1;
        CHECK(xcd_block(t, n) == b);  // ... whose inverse is xcd_block
        if (b >= whole) CHECK(t == b);  // past the last whole round: the block's own tile
        else CHECK(t < whole);
    }
    // inside the whole rounds, the tiles of one run share an XCD (block % 8)
    for (uint32_t t = 0; t + 1 < whole; ++t)
        if (t / K == (t + 1) / K) CHECK((xcd_block(t, n) & 7u) == (xcd_block(t + 1, n) & 7u));
}

static void test_xcd() {
    for (uint32_t n = 0; n <= 2100; ++n) check_xcd(n);
    for (uint32_t n : {8159u, 8160u, 16383u, 16384u}) check_xcd(n);
#if ZR_XCD_TILES == 8
    // n = 128: two rounds of 8 runs of 8.  Block b = 8 l + x is on XCD x, the l-th
    // block there; it takes tile ((l / 8) * 8 + x) * 8 + l % 8.
    CHECK(xcd_tile(0, 128) == 0);
    CHECK(xcd_tile(1, 128) == 8);     // XCD 1's first block: run 1's first tile
    CHECK(xcd_tile(8, 128) == 1);     // XCD 0's second block: run 0's second tile
    CHECK(xcd_tile(64, 128) == 64);   // l = 8: the second round's run 0
    CHECK(xcd_tile(65, 128) == 72);
    CHECK(xcd_tile(127, 128) == 127);
    // n = 100: one whole round (64), the last 36 blocks keep their tiles
    CHECK(xcd_tile(10, 100) == 17);   // x = 2, l = 1: run 2, tile 1 of it
    CHECK(xcd_block(17, 100) == 10);
    CHECK(xcd_tile(63, 100) == 63);
    CHECK(xcd_tile(64, 100) == 64);
    CHECK(xcd_tile(99, 100) == 99);
    CHECK(xcd_tile(5, 63) == 5);      // no whole round at all
#endif
}

// ---- tile jobs
static void test_tile_jobs() {
    for (uint32_t J : {1u, 7u, 512u, 2048u}) {
        for (uint32_t count : {0u, 1u, J - 1u, J, J + 1u, 2u * J - 1u, 2u * J, 2u * J + 1u, 15u * J, 15u * J + 1u, 29700u}) {
            CHECK(tile_jobs(count, 0u, 0u) == 1u);                      // jobs off
            CHECK(tile_jobs(count, kRunDropped, J) == 1u);              // a dropped run: the record scan, one job
            CHECK(tile_jobs(count, kRunDropped | kRunFill | (5u << kRunFillShift), J) == 1u);
            const uint32_t K = tile_jobs(count, kRunFill | (5u << kRunFillShift), J);
            CHECK(K == tile_jobs(count, 0u, J));                        // the fill does not matter
            if (count <= J) {
                CHECK(K == 1u);
            } else {
                CHECK((uint64_t)(K - 1u) * J < count && count <= (uint64_t)K * J);
            }
        }
        CHECK(tile_jobs(J + 1u, 0u, J) == 2u);
        CHECK(tile_jobs(15u * J, 0u, J) == 15u);
    }
    CHECK(tile_jobs(29700u, 0u, 2048u) == 15u);  // (c2x's longest list: 14 * 2048 = 28672 < 29700 <= 30720)
}

// ---- tile_order items
static void test_items() {
    for (uint32_t tile : {0u, 16383u})
        for (uint32_t part : {0u, 1u, 14u}) {
            const uint32_t item = job_item(tile, part);
            CHECK(item_tile(item) == tile);
            CHECK(item_part(item) == part);
            CHECK(item != kJobNone);
        }
    CHECK(job_item(0u, 0u) == 0u);
    CHECK(job_item(0u, 1u) == 16384u);
    CHECK(job_item(16383u, 14u) == 245759u);  // 0x3FFF | 14 << 14 = 0x3BFFF
    CHECK(item_tile(kJobNone) == 16383u);     // (why k_tile tests for kJobNone before the tile bound)
}

// ---- cost class.  w x h pixels at origin (ox, oy), as the inclusive rectangle.
static uint32_t bucket_wh(int w, int h, int ox = 0, int oy = 0) { return cost_bucket(ox, ox + w - 1, oy, oy + h - 1); }

static void test_cost_bucket() {
    CHECK(bucket_wh(1, 1) == 0u);    // 1 step
    CHECK(bucket_wh(2, 1) == 0u);    // 1 step
    CHECK(bucket_wh(3, 1) == 0u);    // 2 steps: (2 - 1) >> 1
    CHECK(bucket_wh(5, 1) == 1u);    // 3 steps
    CHECK(bucket_wh(32, 32) == 63u); // 16 * 32 = 512 steps, clamped
    CHECK(bucket_wh(64, 64) == 63u);
    // steps s land in bucket (s - 1) >> 1: bucket 24 is steps 49 and 50
    CHECK(kSortBuckets == 64u);
#if ZR_MID_BUCKET == 24
    CHECK(bucket_wh(1, 48) == 23u);  // 48 steps
    CHECK(bucket_wh(1, 49) == 24u);  // 49 steps: the first of kMidBucket
    CHECK(bucket_wh(2, 49) == 24u);
    CHECK(bucket_wh(14, 7) == 24u);  // 7 steps a row, 7 rows
    CHECK(bucket_wh(16, 6) == 23u);  // 48
    CHECK(bucket_wh(1, 51) == 25u);
#endif
    CHECK(bucket_wh(2, 127) == 63u);  // 127 steps: the last bucket's first
    CHECK(bucket_wh(2, 126) == 62u);
    for (int w = 1; w <= 64; ++w)
        for (int h = 1; h <= 64; ++h) {
            const uint32_t b = bucket_wh(w, h);
            const uint32_t steps = (uint32_t)((w + 1) / 2 * h);
            CHECK(b == ((steps - 1u) / 2u < 63u ? (steps - 1u) / 2u : 63u));
            CHECK(b <= 63u);
            CHECK(b == bucket_wh(w, h, 37, 1055));  // the origin does not matter
            if (w < 64) CHECK(bucket_wh(w + 1, h) >= b);
            if (h < 64) CHECK(bucket_wh(w, h + 1) >= b);
        }
}

// ---- lane space of a sorted segment
static uint32_t lanes_of(uint32_t j, uint32_t n, uint32_t NT, uint32_t offm, uint32_t off63) {
    uint32_t q = NT / n;  // (n >= 1)
    q = q < 1u ? 1u : q > 8u ? 8u : q;
    const uint32_t kl = q >= 8u ? 8u : q >= 4u ? 4u : q >= 2u ? 2u : 1u;
    if (j >= off63) return kl > 8u ? kl : 8u;
    if (j >= offm) return kl > 4u ? kl : 4u;
    return kl;
}

static void check_lane_space(uint32_t NT, uint32_t n, uint32_t offm, uint32_t off63) {
    const LaneSpace ls = lane_space(n, NT, offm, off63);
    uint32_t total = 0;
    for (uint32_t j = 0; j < n; ++j) total += lanes_of(j, n, NT, offm, off63);
    CHECK(ls.chunks == (total + 63u) / 64u);
    std::vector<uint8_t> seen((size_t)n * 8u, 0);
    uint32_t found = 0;
    for (uint32_t g = 0; g < 64u * ls.chunks; ++g) {
        const LaneSlot s = lane_slot(ls, g);
        if (g >= total) {
            CHECK(s.j >= n);  // every slot past the last entry's lanes is empty
            continue;
        }
        CHECK(s.j < n);
        if (s.j >= n) return;
        const uint32_t lanes = lanes_of(s.j, n, NT, offm, off63);
        CHECK((1u << s.ksh) == lanes);
        CHECK(s.sub >= 0 && (uint32_t)s.sub < lanes);
        CHECK(s.last == (s.j >= off63));
        if (s.sub < 0 || (uint32_t)s.sub >= 8u) return;
        CHECK(!seen[(size_t)s.j * 8u + (uint32_t)s.sub]);  // each (entry, sub-lane) at one slot only
        seen[(size_t)s.j * 8u + (uint32_t)s.sub] = 1;
        ++found;
    }
    CHECK(found == total);  // ... and every one of them at some slot
}

static void test_lane_space() {
    for (uint32_t NT : {256u, 512u, 1024u})
        for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 255u, 256u, 1023u, 1024u}) {
            const uint32_t cut[] = {0u, 1u, n / 3u, n / 2u, n - 1u, n};
            for (uint32_t offm : cut)
                for (uint32_t off63 : cut)
                    if (offm <= off63 && off63 <= n) check_lane_space(NT, n, offm, off63);
        }
#if ZR_BIG_LANES == 8 && ZR_MID_LANES == 4
    {   // one entry, in the last bucket: 8 lanes, one chunk
        const LaneSpace ls = lane_space(1u, 256u, 0u, 0u);
        CHECK(ls.ksh_s == 3u && ls.ksh_b == 3u && ls.chunks == 1u);
        const LaneSlot s = lane_slot(ls, 7u);
        CHECK(s.j == 0u && s.sub == 7 && s.ksh == 3u && s.last);
        CHECK(lane_slot(ls, 8u).j >= 1u);
    }
    {   // 65 cheap entries on 512 threads: 512 / 65 = 7 -> 4 lanes each, 260 lanes, 5 chunks
        const LaneSpace ls = lane_space(65u, 512u, 65u, 65u);
        CHECK(ls.ksh_s == 2u && ls.chunks == 5u);
        const LaneSlot s = lane_slot(ls, 259u);
        CHECK(s.j == 64u && s.sub == 3 && s.ksh == 2u && !s.last);
        CHECK(lane_slot(ls, 260u).j >= 65u);
    }
    {   // a full segment on 256 threads: 1000 x 1 lane, 20 x 4, 4 x 8 = 1112 lanes, 18 chunks
        const LaneSpace ls = lane_space(1024u, 256u, 1000u, 1020u);
        CHECK(ls.ksh_s == 0u && ls.ksh_m == 2u && ls.ksh_b == 3u);
        CHECK(ls.lsp_s == 1000u && ls.lsp_m == 1080u && ls.chunks == 18u);
        LaneSlot s = lane_slot(ls, 999u);
        CHECK(s.j == 999u && s.sub == 0 && s.ksh == 0u && !s.last);
        s = lane_slot(ls, 1006u);  // 6 slots into the middle run: entry 1001, lane 2 of 4
        CHECK(s.j == 1001u && s.sub == 2 && s.ksh == 2u && !s.last);
        s = lane_slot(ls, 1111u);  // the last lane of the last entry
        CHECK(s.j == 1023u && s.sub == 7 && s.ksh == 3u && s.last);
        CHECK(lane_slot(ls, 1112u).j >= 1024u);
    }
#endif
}

int main() {
    test_xcd();
    test_tile_jobs();
    test_items();
    test_cost_bucket();
    test_lane_space();
    if (g_failed) {
        fprintf(stderr, "order_host: %d checks failed\n", g_failed);
        return 1;
    }
    printf("order_host ok\n");
    return 0;
}
