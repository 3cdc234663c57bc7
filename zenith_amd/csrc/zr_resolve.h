// zr_resolve.h — k_tile's resolve: attachment stores, shading entry points, the record table, the per-pixel and the per-tile resolve.
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_dev_common.h"
#include "zr_raster.h"
#include "zr_shading.h"

namespace zr {

// ------------------------------------------------------------------- k_tile

// T: the sRGB threshold table (LDS copy in k_tile).
__device__ __forceinline__ void store_color(const DrawParams& P, int px, int py, bool have, const float c[4],
                                            const float* T) {
    const size_t idx = (size_t)py * P.fb_w + (size_t)px;
    if (P.color_bpp == 4) {
        uint32_t* cp = (uint32_t*)P.color + idx;
        const uint32_t m = rgba8_write_mask(P.write_mask, P.color_format);
        if (have) {
            const uint32_t texel = pack_rgba8_fast(c, P.color_format, T);
            if (m == 0xFFFFFFFFu) {
                *cp = texel;
            } else {
                const uint32_t base = P.clear_color_enable ? P.clear_color_packed : *cp;
                *cp = (base & ~m) | (texel & m);
            }
        } else if (P.clear_color_enable) {
            *cp = P.clear_color_packed;
        }
    } else if (P.color_bpp == 16) {
        float4* cp = (float4*)P.color + idx;
        float4 v = P.clear_color_enable ? make_float4(P.clear_color[0], P.clear_color[1], P.clear_color[2],
                                                      P.clear_color[3])
                                        : *cp;
        if (have) {
            if (P.write_mask & 1u) v.x = c[0];
            if (P.write_mask & 2u) v.y = c[1];
            if (P.write_mask & 4u) v.z = c[2];
            if (P.write_mask & 8u) v.w = c[3];
        }
        if (have || P.clear_color_enable) *cp = v;
    }
}

// Visibility sequence of setup record e (API order): e + 1, or for the mesh
// program 4p + k + 1 for fan k of primitive p (zr_internal.h kMeshFans).
template <int PROG>
__device__ __forceinline__ uint32_t entry_seq(const DrawParams& P, uint32_t e) {
    if (PROG != kProgMesh) return e + 1u;
    if (e < P.prims) return 4u * e + 1u;
    const uint32_t q = e - P.prims;
    return 4u * (q >> 1) + (q & 1u) + 2u;
}
// ... and back: the setup record and the draw primitive of sequence s + 1.
template <int PROG>
__device__ __forceinline__ uint32_t seq_record(const DrawParams& P, uint32_t s) {
    if (PROG != kProgMesh) return s;
    const uint32_t p = s >> 2, k = s & 3u;
    return k ? P.prims + 2u * p + k - 1u : p;
}
template <int PROG>
__device__ __forceinline__ uint32_t seq_prim(uint32_t s) { return PROG == kProgMesh ? s >> 2 : s; }
template <int PROG>
__device__ __forceinline__ uint32_t record_prim(const DrawParams& P, uint32_t e) {
    return (PROG == kProgMesh && e >= P.prims) ? (e - P.prims) >> 1 : e;
}

template <int PROG>
__device__ __forceinline__ void shade_winner(const DrawParams& P, const TriRecord& r, const EdgeEvalF& e, float out[4]) {
    if (PROG == kProgFlat) {
        const float* c = attr_ptr(P, r.v0, 1);  // provoking vertex = first (flat)
        out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = 1.0f;
        return;
    }
    // perspective-correct weights b_i / w_i with w_i = 1 for every built-in vertex stage
    const float pw0 = e.f0 * r.invA2, pw1 = e.f1 * r.invA2, pw2 = e.f2 * r.invA2;
    const float inv = 1.0f / ((pw0 + pw1) + pw2);
    const float* a0 = attr_ptr(P, r.v0, 1);
    const float* a1 = attr_ptr(P, r.v1, 1);
    const float* a2 = attr_ptr(P, r.v2, 1);
    float f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = ((pw0 * a0[i] + pw1 * a1[i]) + pw2 * a2[i]) * inv;
    if (PROG == kProgTriangle) {
        const float t3 = (P.time_ptr ? *P.time_ptr : 0.0f) * 3.0f;
        out[0] = shade_triangle_channel(f[0], t3);
        out[1] = shade_triangle_channel(f[1], t3);
        out[2] = shade_triangle_channel(f[2], t3);
        out[3] = 1.0f;
        return;
    }
    const float* k0 = attr_ptr(P, r.v0, 2);
    const float* k1 = attr_ptr(P, r.v1, 2);
    const float* k2 = attr_ptr(P, r.v2, 2);
    float kd[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) kd[i] = ((pw0 * k0[i] + pw1 * k1[i]) + pw2 * k2[i]) * inv;
    shade_blinn_phong(f[0], f[1], f[2], kd[0], kd[1], kd[2], out);
}

// mesh.slang psmain: perspective-correct barycentrics of the primitive (not of
// its clipped fan triangle) from its homogeneous screen vertices
// h_i = (x_i hw + w_i cx, y_i hh + w_i cy, w_i): b_i = E_i / sum E with
// E_i = p . (h_j x h_k) at the pixel centre (the planes setup stored,
// mesh_edge_planes); then normal and uv interpolated and lit like blinn_phong.slang with kd = (0.35 + 0.3 u, 0.35 + 0.3 v, 0.7)
// (zr_oracle.c shade, same operation order).
__device__ __forceinline__ void shade_mesh(const DrawParams& P, uint32_t prim, const uint32_t vid[3], int px, int py,
                                           float out[4]) {
    const float4* q = P.mesh_edges + (size_t)prim * 3u;
    const float4 qa = q[0], qb = q[1], qc = q[2];
    const float c[12] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w, qc.x, qc.y, qc.z, qc.w};
    float E[3];
    mesh_plane_eval(c, px, py, E);
    const float einv = 1.0f / ((E[0] + E[1]) + E[2]);
    const float b0 = E[0] * einv, b1 = E[1] * einv, b2 = E[2] * einv;
    const float* n0 = attr_ptr(P, vid[0], 1);
    const float* n1 = attr_ptr(P, vid[1], 1);
    const float* n2 = attr_ptr(P, vid[2], 1);
    const float* u0 = attr_ptr(P, vid[0], 2);
    const float* u1 = attr_ptr(P, vid[1], 2);
    const float* u2 = attr_ptr(P, vid[2], 2);
    float n[3], uv[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = (b0 * n0[i] + b1 * n1[i]) + b2 * n2[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) uv[i] = (b0 * u0[i] + b1 * u1[i]) + b2 * u2[i];
    shade_blinn_phong(n[0], n[1], n[2], fmaf(uv[0], 0.3f, 0.35f), fmaf(uv[1], 0.3f, 0.35f), 0.7f, out);
}

// Vertex ids of a winning primitive; IDX32: u32 index buffer (one 12-B load).
template <bool IDX32>
__device__ __forceinline__ void resolve_vids(const DrawParams& P, uint32_t prim, uint32_t v[3]) {
    if (IDX32) {
        const uint32_t tri = tri_of(P, prim);
        const uint3 ix = *reinterpret_cast<const uint3*>(P.ib + (uint64_t)(P.first + tri * 3u) * 4);
        const uint32_t off = (uint32_t)P.vertex_offset;
        v[0] = ix.x + off; v[1] = ix.y + off; v[2] = ix.z + off;
    } else {
        winner_vids(P, prim, v);
    }
}

// Record table of a 512-thread tile (LDS): the small primitives of its current
// segment, with the part of the compact record the resolve reads (vertex 0
// relative to the tile origin as int16 pairs, the deltas, +-1/A2), stored at the
// entry's sorted position j (no collisions), and a 2048-slot hash from the setup
// record to j + 1 (load factor <= 1/2: short probes).  A lookup is valid when the
// sorted array still holds that record at j (a later segment reuses positions).
// The raster inserts each entry as it loads it; the resolve looks its winners up
// and gathers the record only when that fails (a table overwritten by a later
// segment, a long probe, a large primitive).  A large primitive is not hashed, but
// its position's slot gets the large marker, so a stale hash slot an earlier
// segment left for that position decodes as large (records_big), never as the
// earlier segment's small record.  Every winner request the pass saves
// is worth ~20 ns of a C2 tile pass (docs/EXPERIMENTS.md).
constexpr uint32_t kRecHashSlots = 2048;
constexpr uint32_t kRecTabProbes = 8;
__device__ __forceinline__ uint32_t rec_hash(uint32_t rec) { return (rec * 0x9E3779B1u) >> 21; }  // 11 bits
// Vertex 0 of a small primitive (extents <= 64 px) whose bbox meets the tile lies
// within [-64 px, tile edge + 64 px) of the tile origin: stored as u16 offsets (24.8
// fixed point) from 64 px above-left of the origin.
constexpr int kRelBias = 64 * 256;
static_assert((64 + 128) * 256 <= 65536, "tile-relative vertex 0 fits u16 (tiles up to 64 px)");

__device__ __forceinline__ void rec_table_insert(uint32_t* s_thash, int4* s_trec, uint32_t rec, uint32_t j,
                                                 const int4 q0, const int4 q1, int x0, int y0) {
    const uint32_t rel = ((uint32_t)(q0.x - x0 * 256 + kRelBias) & 0xFFFFu) | ((uint32_t)(q0.y - y0 * 256 + kRelBias) << 16);
    s_trec[j] = make_int4((int)rel, q0.z, q0.w, q1.w);
    uint32_t h = rec_hash(rec);
    for (uint32_t p = 0; p < kRecTabProbes; ++p) {
        if (atomicCAS(&s_thash[h], 0u, j + 1u) == 0u) return;
        h = (h + 1u) & (kRecHashSlots - 1u);
    }
}

// The compact record words (q1: only 1/A2) of setup record `rec`.
__device__ __forceinline__ bool rec_table_find(const uint32_t* s_thash, const int4* s_trec, const uint32_t* s_sorted,
                                               uint32_t rec, int x0, int y0, int4& q0, int4& q1) {
    uint32_t h = rec_hash(rec);
    for (uint32_t p = 0; p < kRecTabProbes; ++p) {
        const uint32_t v = s_thash[h];
        if (v == 0u) return false;
        if (s_sorted[v - 1u] == rec) {
            const int4 e = s_trec[v - 1u];
            q0 = make_int4(x0 * 256 - kRelBias + (int)((uint32_t)e.x & 0xFFFFu), y0 * 256 - kRelBias + (int)((uint32_t)e.x >> 16),
                           e.y, e.z);
            q1 = make_int4(0, 0, 0, e.w);
            return true;
        }
        h = (h + 1u) & (kRecHashSlots - 1u);
    }
    return false;
}

// Per-pixel resolve (512-thread tiles: two pixels per thread, one batch): per
// pixel the winning primitive is read from its key, its compact record and vertex
// ids are gathered, its edges evaluated once and the program shaded once
// (deferred shading); colour and depth are stored.  The batch's gathers are in
// flight together, and a tile's records are still L2-resident from its raster
// phase.  Measured faster than resolve_tile at 512 threads (C2: ~78 vs 80-84 us:
// no barriers, two dependent round trips), slower at 256 threads (4 pixels per
// thread in two batches; C1 49 vs 44 us, C3 223 vs 204 us).  A wave with no
// winner skips the gathers; other pixels without a winner load the wave's first
// winner (in-bounds addresses) and discard it.
template <int PROG, int MODE, bool IDX32, int NT, bool TAB, int TS>
__device__ __forceinline__ void resolve_pixels(const DrawParams& P, int x0, int y0, const unsigned long long* s_key,
                                               const float* s_srgb, const uint32_t* s_thash, const int4* s_trec,
                                               const uint32_t* s_sorted) {
    constexpr int T = 1 << TS, TP = T * T;
    constexpr int kPer = TP / NT;
    constexpr int kB = kPer < (int)kResolveBatch ? kPer : (int)kResolveBatch;
    // recomputed here, not reused from the tile's init: a pixel coordinate kept
    // live across the raster loop spills at 64 VGPRs
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
#pragma unroll 1
    for (int k0 = 0; k0 < kPer; k0 += kB) {
        int px[kB], py[kB];
        bool have[kB], inside[kB];
        unsigned long long key[kB];
        uint32_t prim[kB], gp[kB], vid[kB][3];  // setup record, draw primitive, its vertex ids
        int4 c0[kB], c1[kB];
#pragma unroll
        for (int b = 0; b < kB; ++b) {
            const int i = tid + (k0 + b) * NT;
            px[b] = x0 + (i & (T - 1));
            py[b] = y0 + (i >> TS);
            inside[b] = !(px[b] < P.ra_x0 || px[b] > P.ra_x1 || py[b] < P.ra_y0 || py[b] > P.ra_y1);
            key[b] = s_key[i];
            const uint32_t seq = inside[b] ? winner_seq<MODE>(key[b]) : 0u;
            have[b] = seq != 0;
            prim[b] = have[b] ? seq_record<PROG>(P, seq - 1u) : 0u;
            gp[b] = have[b] ? seq_prim<PROG>(seq - 1u) : 0u;
        }
        if (P.win_bits) {  // winner census (profiling level 2 only; never in a timed pass)
#pragma unroll
            for (int b = 0; b < kB; ++b)
                if (have[b]) atomicOr(&P.win_bits[gp[b] >> 5], 1u << (gp[b] & 31u));
        }
        unsigned long long anyw = 0;
#pragma unroll
        for (int b = 0; b < kB; ++b) anyw |= __ballot(have[b]);
        if (anyw) {  // wave-uniform: some pixel of the wave has a winner, lend it to the others
            const int src = (int)__builtin_ctzll(anyw);
            uint32_t fb = 0, fg = 0;
#pragma unroll
            for (int b = 0; b < kB; ++b) {
                const unsigned long long hb = __ballot(have[b]);
                const uint32_t pb = (uint32_t)__builtin_amdgcn_readlane((int)prim[b], src);
                const uint32_t gb = (uint32_t)__builtin_amdgcn_readlane((int)gp[b], src);
                if (!fb && ((hb >> src) & 1ull)) { fb = pb + 1u; fg = gb; }
            }
#pragma unroll
            for (int b = 0; b < kB; ++b)
                if (!have[b]) { prim[b] = fb - 1u; gp[b] = fg; }
        }
        float col[kB][4];
        float zw[kB];
        if (anyw) {
#pragma unroll
            for (int b = 0; b < kB; ++b) {  // the index gathers first: the table lookups run under them
                if (tile_debug(P) & kDebugIdentityVids) {
                    const uint32_t v = P.first + tri_of(P, gp[b]) * 3u + (uint32_t)P.vertex_offset;
                    vid[b][0] = v; vid[b][1] = v + 1u; vid[b][2] = v + 2u;
                } else {
                    resolve_vids<IDX32>(P, gp[b], vid[b]);
                }
                if (tile_debug(P) & kDebugSameVids) vid[b][0] = vid[b][1] = vid[b][2] = 0u;
            }
#pragma unroll
            for (int b = 0; b < kB; ++b) {
                // the record: from the tile's record table, else gathered (mesh
                // programs read it only for a last-wins depth)
                bool tab = false;
                if (TAB && P.rec_table) tab = rec_table_find(s_thash, s_trec, s_sorted, prim[b], x0, y0, c0[b], c1[b]);
                if (!tab && (PROG != kProgMesh || MODE == kDepthLastWins)) {
                    const int4* cp = reinterpret_cast<const int4*>(P.records + ((tile_debug(P) & kDebugSameRecord) ? 0u : prim[b]));
                    c0[b] = cp[0];
                    c1[b] = cp[1];
                } else if (!tab) {
                    c0[b] = c1[b] = make_int4(0, 0, 1, 1);
                }
            }
#pragma unroll
            for (int b = 0; b < kB; ++b) {
                TriRecord r = decode_compact(P, c0[b], c1[b], false);
                if (__ballot(compact_is_large(c0[b]))) {  // rare, wave-uniform: a winner is a large primitive
                    if (compact_is_large(c0[b])) r = P.records_big[prim[b]];
                }
                const bool sw = (r.flags & kFlagSwapped) != 0u;
                r.v0 = vid[b][0];
                r.v1 = sw ? vid[b][2] : vid[b][1];
                r.v2 = sw ? vid[b][1] : vid[b][2];
                const EdgeEvalF e = eval_edges_f(r, px[b], py[b]);
                col[b][0] = col[b][1] = col[b][2] = col[b][3] = 0.0f;
                if (P.color_bpp && !(tile_debug(P) & kDebugSkipShade)) {
                    if constexpr (PROG == kProgMesh) shade_mesh(P, gp[b], vid[b], px[b], py[b], col[b]);
                    else shade_winner<PROG>(P, r, e, col[b]);
                }
                zw[b] = (MODE == kDepthLastWins) ? winner_depth(r, px[b], py[b]) : key_depth<MODE>(key[b]);
            }
        } else {
#pragma unroll
            for (int b = 0; b < kB; ++b) {
                col[b][0] = col[b][1] = col[b][2] = col[b][3] = 0.0f;
                zw[b] = 0.0f;
            }
        }
#pragma unroll
        for (int b = 0; b < kB; ++b) {
            if (!inside[b]) continue;
            if (P.color_bpp) store_color(P, px[b], py[b], have[b], col[b], s_srgb);
            if (P.depth) {
                float* dp = P.depth + (size_t)py[b] * P.fb_w + px[b];
                if (have[b] && P.depth_write_out) *dp = zw[b];
                else if (P.clear_depth_enable) *dp = P.clear_depth;
            }
        }
    }
}


// ------------------------------------------------------------ tile resolve
//
// The resolve shades each pixel's winner once, but fetches each *distinct*
// winner of the tile once (C2: ~280 winners for 1024 pixels): the pixels' winning
// records go into an LDS hash table that hands out dense winner ids, then the
// workgroup loads every winner's record, vertex ids and shading attributes with
// one cooperative pass into an LDS array (AoS, WinLayout), and each pixel shades
// from LDS.  A tile with more winners than the array holds runs it in batches.

// Per-winner words in LDS, 16-B aligned records (resolve_tile):
//   geometry  X0, Y0, (dx1 | dy1 << 16), (dx2 | dy2 << 16), |1/A2|   -- the compact
//             record (vertex 1/2 in record order); a large primitive keeps dx1 ==
//             kCompactLarge and its setup-record index in X0 (full record from HBM)
//   depth     z0, dz1, dz2                      (last-wins modes only)
//   attrs     flat: provoking colour (3); triangle: colour of v0..v2 (9); Blinn:
//             normals then colours (18); mesh: barycentric planes and their
//             reference pixel (12), normals (9), uvs (6).  Triangle/Blinn in record order, mesh/flat in API order.
template <int PROG, int MODE>
struct WinLayout {
    static constexpr bool kGeo = PROG == kProgTriangle || PROG == kProgBlinn || MODE == kDepthLastWins;
    static constexpr bool kZ = MODE == kDepthLastWins;
    static constexpr int kZOff = kGeo ? 5 : 0;
    static constexpr int kAttrOff = kZOff + (kZ ? 3 : 0);
    static constexpr int kAttrW = PROG == kProgFlat ? 3 : PROG == kProgTriangle ? 9 : PROG == kProgBlinn ? 18 : 27;
    static constexpr int kWords = (kAttrOff + kAttrW + 3) & ~3;
};

// Resolve hash table: TP setup-record ids (kWinEmpty = free), then the
// dense winner list (TP record ids); both live where the keys were.
// (TP = the tile's pixels, 1 << 2 TS)
constexpr uint32_t kWinEmpty = 0xFFFFFFFFu;
template <int TS>
__device__ __forceinline__ uint32_t win_hash(uint32_t rec) { return (rec * 0x9E3779B1u) >> (32 - 2 * TS); }  // log2(TP) bits

__device__ __forceinline__ void copy3(float* dst, const float* src) {
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
}

// Loads winner `rec` (a setup record) into w[0 .. WinLayout::kWords).
template <int PROG, int MODE, bool IDX32>
__device__ __forceinline__ void fetch_winner(const DrawParams& P, uint32_t rec, float* w) {
    using L = WinLayout<PROG, MODE>;
    uint32_t v[3];
    const uint32_t gp = record_prim<PROG>(P, rec);  // draw primitive (mesh: of the fan record)
    {
        const uint32_t tri = tri_of(P, gp);
        const uint32_t e0 = P.first + tri * 3u;
        if (IDX32) {
            const uint3 ix = *reinterpret_cast<const uint3*>(P.ib + (uint64_t)e0 * 4);
            const uint32_t off = (uint32_t)P.vertex_offset;  // two's complement: id + offset wraps to the valid id
            v[0] = ix.x + off; v[1] = ix.y + off; v[2] = ix.z + off;
        } else {
            winner_vids(P, gp, v);
        }
    }
    int4 q0 = make_int4(0, 0, 0, 0), q1 = q0;
    if (L::kGeo) {
        const int4* cp = reinterpret_cast<const int4*>(P.records + rec);
        q0 = cp[0];
        q1 = cp[1];
    }
    if (L::kGeo) {
        int* wi = reinterpret_cast<int*>(w);
        wi[0] = compact_is_large(q0) ? (int)rec : q0.x;
        wi[1] = q0.y;
        wi[2] = q0.z;
        wi[3] = q0.w;
        w[4] = fabsf(__int_as_float(q1.w));
    }
    if (L::kZ) {
        w[L::kZOff + 0] = __int_as_float(q1.x);
        w[L::kZOff + 1] = __int_as_float(q1.y);
        w[L::kZOff + 2] = __int_as_float(q1.z);
    }
    float* a = w + L::kAttrOff;
    if (PROG == kProgFlat) {
        copy3(a, attr_ptr(P, v[0], 1));  // provoking vertex = first (flat)
    } else if (PROG == kProgMesh) {
        const float4* q = P.mesh_edges + (size_t)gp * 3u;
        const float4 qa = q[0], qb = q[1], qc = q[2];
        a[0] = qa.x; a[1] = qa.y; a[2] = qa.z; a[3] = qa.w;
        a[4] = qb.x; a[5] = qb.y; a[6] = qb.z; a[7] = qb.w;
        a[8] = qc.x; a[9] = qc.y; a[10] = qc.z; a[11] = qc.w;
#pragma unroll
        for (int k = 0; k < 3; ++k) copy3(a + 12 + 3 * k, attr_ptr(P, v[k], 1));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* u = attr_ptr(P, v[k], 2);
            a[21 + 2 * k] = u[0];
            a[22 + 2 * k] = u[1];
        }
    } else {
        // record order: setup swapped v1 / v2 when it oriented the primitive (sign of 1/A2)
        const bool sw = q1.w < 0;
        const uint32_t r1 = sw ? v[2] : v[1], r2 = sw ? v[1] : v[2];
        copy3(a + 0, attr_ptr(P, v[0], 1));
        copy3(a + 3, attr_ptr(P, r1, 1));
        copy3(a + 6, attr_ptr(P, r2, 1));
        if (PROG == kProgBlinn) {
            copy3(a + 9, attr_ptr(P, v[0], 2));
            copy3(a + 12, attr_ptr(P, r1, 2));
            copy3(a + 15, attr_ptr(P, r2, 2));
        }
    }
}

// Colour (and for last-wins modes the depth) of pixel (px, py) from its winner's
// LDS words; the same operations as the oracle's per-fragment shading
// (zr_oracle.c shade), only fetched from LDS instead of the vertex buffer.
template <int PROG, int MODE>
__device__ __forceinline__ void shade_from_lds(const DrawParams& P, const float* w, int px, int py, float t3,
                                               float out[4], float& zw) {
    using L = WinLayout<PROG, MODE>;
    TriRecord r;
    EdgeEvalF e{0.0f, 0.0f, 0.0f};
    if (L::kGeo) {
        const int4 g = *reinterpret_cast<const int4*>(w);
        const bool large = compact_is_large(g);
        int4 q1 = make_int4(0, 0, 0, __float_as_int(w[4]));
        if (L::kZ) {
            q1.x = __float_as_int(w[L::kZOff + 0]);
            q1.y = __float_as_int(w[L::kZOff + 1]);
            q1.z = __float_as_int(w[L::kZOff + 2]);
        }
        r = decode_compact(P, g, q1, false);
        if (__ballot(large)) {  // rare, wave-uniform: a winner too large for the compact form
            if (large) r = P.records_big[g.x];
        }
        e = eval_edges_f(r, px, py);
        if (L::kZ) zw = winner_depth(r, px, py);
    }
    const float* a = w + L::kAttrOff;
    out[3] = 1.0f;
    if (PROG == kProgFlat) {
        out[0] = a[0]; out[1] = a[1]; out[2] = a[2];
        return;
    }
    if (PROG == kProgMesh) {
        // mesh.slang psmain: b_i = E_i / sum E with E_i = p . (h_j x h_k) at the pixel
        // centre, from the planes setup stored (mesh_edge_planes); then normal and uv
        // interpolated and lit like blinn_phong.slang, kd = (0.35 + 0.3 u, 0.35 + 0.3 v, 0.7)
        float E[3];
        mesh_plane_eval(a, px, py, E);
        const float einv = 1.0f / ((E[0] + E[1]) + E[2]);
        const float b0 = E[0] * einv, b1 = E[1] * einv, b2 = E[2] * einv;
        float n[3], uv[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) n[i] = (b0 * a[12 + i] + b1 * a[15 + i]) + b2 * a[18 + i];
#pragma unroll
        for (int i = 0; i < 2; ++i) uv[i] = (b0 * a[21 + i] + b1 * a[23 + i]) + b2 * a[25 + i];
        shade_blinn_phong(n[0], n[1], n[2], fmaf(uv[0], 0.3f, 0.35f), fmaf(uv[1], 0.3f, 0.35f), 0.7f, out);
        return;
    }
    // perspective-correct weights b_i / w_i with w_i = 1 for every built-in vertex stage
    const float pw0 = e.f0 * r.invA2, pw1 = e.f1 * r.invA2, pw2 = e.f2 * r.invA2;
    const float inv = 1.0f / ((pw0 + pw1) + pw2);
    float f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = ((pw0 * a[i] + pw1 * a[3 + i]) + pw2 * a[6 + i]) * inv;
    if (PROG == kProgTriangle) {
        out[0] = shade_triangle_channel(f[0], t3);
        out[1] = shade_triangle_channel(f[1], t3);
        out[2] = shade_triangle_channel(f[2], t3);
        return;
    }
    float kd[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) kd[i] = ((pw0 * a[9 + i] + pw1 * a[12 + i]) + pw2 * a[15 + i]) * inv;
    shade_blinn_phong(f[0], f[1], f[2], kd[0], kd[1], kd[2], out);
}

// Resolve of one tile (after the raster phase; s_key holds the final keys).
//   1  per pixel: key -> winning setup record; pixels no fragment won store the
//      clear, and the key's depth is stored now (depth-writing min/max modes).
//      The key array's upper half becomes the hash table: each thread empties the
//      slots lying over the keys it owns (so no barrier is needed before that).
//   2  winners into the hash table (LDS CAS, linear probing); the inserting lane
//      takes a dense id (one LDS add per wave) and records it beside the slot and
//      the winner in the dense list (the key array's lower half)
//   3  per batch of <= cap winners: cooperative fetch into LDS, then every pixel
//      whose winner is in the batch shades from LDS and stores its colour
// Three barriers in all.  s_u: the dense-id map (u16 per slot), then (kPer > 2)
// each pixel's dense id (u16), then the per-winner words (cap * kWords floats).
template <int PROG, int MODE, bool IDX32, int NT, int TS>
__device__ __forceinline__ void resolve_tile(const DrawParams& P, int x0, int y0, unsigned long long* s_key,
                                             uint32_t* s_u, uint32_t u_words, uint32_t* s_nwin,
                                             const float* s_srgb, unsigned long long* ts = nullptr) {
    constexpr int T = 1 << TS, TP = T * T;
    using L = WinLayout<PROG, MODE>;
    constexpr int kPer = TP / NT;
    constexpr bool kPixLds = kPer > 2;  // per-pixel ids in LDS (registers at 512 threads)
    uint32_t* s_list = reinterpret_cast<uint32_t*>(s_key);              // [TP] over keys 0..511
    uint32_t* s_tab = s_list + TP;                               // [TP] over keys 512..1023
    uint16_t* s_dmap = reinterpret_cast<uint16_t*>(s_u);                // [TP]
    uint32_t* s_pix = s_tab;  // [TP] (kPixLds): the table is free once every dense id is known
    float* s_win = reinterpret_cast<float*>(s_u + TP / 2u);
    const uint32_t cap = min((u_words - TP / 2u) / (uint32_t)L::kWords, TP);
    // recomputed here, not reused from the tile's init: a pixel coordinate kept
    // live across the raster loop spills at 64 VGPRs
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    uint32_t rec[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = tid + k * NT;
        const int px = x0 + (i & (T - 1)), py = y0 + (i >> TS);
        const bool inside = !(px < P.ra_x0 || px > P.ra_x1 || py < P.ra_y0 || py > P.ra_y1);
        const unsigned long long key = s_key[i];
        if (i >= (int)(TP / 2)) {  // this key's bytes hold hash slots 2(i - 512) and 2(i - 512) + 1
            s_tab[2 * (i - TP / 2)] = kWinEmpty;
            s_tab[2 * (i - TP / 2) + 1] = kWinEmpty;
        }
        const uint32_t seq = inside ? winner_seq<MODE>(key) : 0u;
        rec[k] = seq ? seq_record<PROG>(P, seq - 1u) : kWinEmpty;
        if (!inside) continue;
        if (!seq && P.color_bpp) {
            const float c[4] = {0.f, 0.f, 0.f, 0.f};
            store_color(P, px, py, false, c, s_srgb);
        }
        if (P.depth) {
            float* dp = P.depth + (size_t)py * P.fb_w + px;
            if (seq && P.depth_write_out) {
                if (MODE != kDepthLastWins) *dp = key_depth<MODE>(key);  // last-wins: interpolated in step 3
            } else if (P.clear_depth_enable) {
                *dp = P.clear_depth;
            }
        }
    }
    if (threadIdx.x == 0) *s_nwin = 0u;
    __syncthreads();  // every key read, every slot empty
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t hs[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        bool fresh = false;
        uint32_t h = win_hash<TS>(rec[k]);
        if (rec[k] != kWinEmpty) {
            for (;;) {  // linear probing; at most TP distinct records, so it ends
                const uint32_t old = atomicCAS(&s_tab[h], kWinEmpty, rec[k]);
                if (old == kWinEmpty) { fresh = true; break; }
                if (old == rec[k]) break;
                h = (h + 1u) & (TP - 1u);
            }
        }
        hs[k] = h;
        const unsigned long long b = __ballot(fresh);
        uint32_t base = 0;
        if (lane == 0 && b) base = atomicAdd(s_nwin, (uint32_t)__popcll(b));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (fresh) {
            const uint32_t d = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            s_list[d] = rec[k];
            s_dmap[h] = (uint16_t)d;
        }
    }
    __syncthreads();  // every winner has its dense id
    uint32_t did[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        did[k] = rec[k] != kWinEmpty ? (uint32_t)s_dmap[hs[k]] : kWinEmpty;
    }
    if (kPixLds) {
        __syncthreads();  // every lookup of the table done before it holds pixel ids
#pragma unroll
        for (int k = 0; k < kPer; ++k) s_pix[tid + k * NT] = did[k];  // read back by this thread only
    }
    const uint32_t nwin = *s_nwin;
    if (ts) ts[5] = __builtin_amdgcn_s_memrealtime();  // kDebugStamps: winners known
    const float t3 = PROG == kProgTriangle ? (P.time_ptr ? *P.time_ptr : 0.0f) * 3.0f : 0.0f;
    for (uint32_t base = 0; base < nwin; base += cap) {
        const uint32_t nb = min(cap, nwin - base);
        if (base) __syncthreads();  // the previous batch's pixels are done with s_win
        for (uint32_t j = threadIdx.x; j < nb; j += NT) {
            fetch_winner<PROG, MODE, IDX32>(P, s_list[base + j], s_win + (size_t)j * L::kWords);
            if (P.win_bits) {  // winner census (profiling level 2 only)
                const uint32_t g = record_prim<PROG>(P, s_list[base + j]);
                atomicOr(&P.win_bits[g >> 5], 1u << (g & 31u));
            }
        }
        __syncthreads();
        if (ts && !base) ts[6] = __builtin_amdgcn_s_memrealtime();  // first batch fetched
        auto shade_pixel = [&](int k, uint32_t dk) {
            const uint32_t j = dk - base;
            if (dk == kWinEmpty || j >= nb) return;
            const int i = tid + k * NT;
            const int px = x0 + (i & (T - 1)), py = y0 + (i >> TS);
            float col[4] = {0.f, 0.f, 0.f, 0.f};
            float zw = 0.0f;
            if (!(tile_debug(P) & kDebugSkipShade))
                shade_from_lds<PROG, MODE>(P, s_win + (size_t)j * L::kWords, px, py, t3, col, zw);
            if (P.color_bpp) store_color(P, px, py, true, col, s_srgb);
            if (MODE == kDepthLastWins && P.depth && P.depth_write_out) P.depth[(size_t)py * P.fb_w + px] = zw;
        };
        if (kPixLds) {
#pragma unroll 1
            for (int k = 0; k < kPer; ++k) shade_pixel(k, s_pix[tid + k * NT]);
        } else {
#pragma unroll
            for (int k = 0; k < kPer; ++k) shade_pixel(k, did[k]);
        }
    }
}

}  // namespace zr
