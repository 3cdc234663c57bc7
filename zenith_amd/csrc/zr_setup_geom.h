// zr_setup_geom.h — k_setup_bin / k_route: primitive assembly, setup geometry, records, owned-tile counting.
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_dev_common.h"

namespace zr {

// ------------------------------------------------------------------ k_setup
//
// One workgroup per chunk of 256 * tris_per_thread primitives (coalesced: step k
// of every thread covers 256 consecutive primitives).  Tile overlaps are counted
// in an LDS histogram (no global atomics); the histogram row is written to
// counts[wg][*] for the column scan.

// Primitive assembly, split in stages so that a thread's loads for several
// primitives are in flight together (index loads, then position loads, then math).
struct PrimIn {
    uint32_t vid[3];
    float3 p[3];
    bool ok;
};

__device__ __forceinline__ void fetch_indices_gid(const DrawParams& P, uint32_t gid, PrimIn& in) {
    const uint32_t tri = tri_of(P, gid);
    const uint64_t e0 = (uint64_t)P.first + (uint64_t)tri * 3u;
    bool ok = true;
    if (P.index_size == 4 && tri < P.ib_tris) {  // ib_tris: the triangles whose 3 indices are in the buffer
        const uint3 ix = *reinterpret_cast<const uint3*>(P.ib + e0 * 4);  // one 12-B load
        if (P.vertex_offset == 0) {  // wave-uniform: u32 ids need no range check
            in.vid[0] = ix.x; in.vid[1] = ix.y; in.vid[2] = ix.z;
        } else {
            const int64_t v0 = (int64_t)ix.x + P.vertex_offset, v1 = (int64_t)ix.y + P.vertex_offset,
                          v2 = (int64_t)ix.z + P.vertex_offset;
            ok = v0 >= 0 && v0 <= 0xFFFFFFFFll && v1 >= 0 && v1 <= 0xFFFFFFFFll && v2 >= 0 && v2 <= 0xFFFFFFFFll;
            in.vid[0] = (uint32_t)v0; in.vid[1] = (uint32_t)v1; in.vid[2] = (uint32_t)v2;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int64_t v = 0;
            ok = ok && fetch_index(P, e0 + (uint64_t)k, v);
            ok = ok && v >= 0 && v <= 0xFFFFFFFFll;
            in.vid[k] = (uint32_t)v;
        }
    }
    in.ok = ok;
}

// Setup record `pos` (< n_pos): the draw primitive itself.
__device__ __forceinline__ void fetch_indices(const DrawParams& P, uint32_t pos, uint32_t n_pos, PrimIn& in) {
    in.ok = pos < n_pos;
    if (in.ok) fetch_indices_gid(P, pos, in);
}

__device__ __forceinline__ void fetch_positions(const DrawParams& P, PrimIn& in) {
    if (!in.ok) return;
    // every attribute of the three vertices inside the buffer (vid_count: DrawParams)
    const bool ok = in.vid[0] < P.vid_count && in.vid[1] < P.vid_count && in.vid[2] < P.vid_count;
    in.ok = ok;
    if (!ok) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) in.p[k] = *reinterpret_cast<const float3*>(attr_ptr(P, in.vid[k], 0));  // 12-B loads
}

// Setup geometry of one primitive (vertex stage, viewport, snap, facing/cull,
// orientation, top-left biases, clipped pixel bbox): false when the primitive
// produces no sample (dropped, culled, degenerate or outside the clip rect).
// k_route and k_setup_bin both call it, so a routed primitive's bbox is the one
// its owner's setup computes.
struct PrimGeom {
    int32_t X[3], Y[3];
    float z[3];
    uint32_t rv[3];
    uint32_t flags;
    long long A2;
    int32_t px0, py0, px1, py1;
};

// Orientation to A2 > 0 (v1/v2 swapped, v0 kept: kFlagSwapped), top-left biases,
// the small flag and the clipped pixel bbox of a snapped triangle whose facing
// was already tested.  False when no pixel centre of the clip rect is inside the bbox.
__device__ __forceinline__ bool orient_and_bound(const DrawParams& P, PrimGeom& g, long long A2) {
    int32_t* X = g.X;
    int32_t* Y = g.Y;
    uint32_t flags = 0;
    if (A2 < 0) {
        int32_t t = X[1]; X[1] = X[2]; X[2] = t;
        t = Y[1]; Y[1] = Y[2]; Y[2] = t;
        const float f = g.z[1]; g.z[1] = g.z[2]; g.z[2] = f;
        const uint32_t u = g.rv[1]; g.rv[1] = g.rv[2]; g.rv[2] = u;
        A2 = -A2;
        flags |= kFlagSwapped;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // top-left rule (y-down), edge i opposite vertex i
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        const int32_t dx = X[b] - X[a], dy = Y[b] - Y[a];
        const bool tl = (dy < 0) || (dy == 0 && dx > 0);
        if (!tl) flags |= (kFlagBias0 << i);
    }
    const int32_t minX = min(X[0], min(X[1], X[2])), maxX = max(X[0], max(X[1], X[2]));
    const int32_t minY = min(Y[0], min(Y[1], Y[2])), maxY = max(Y[0], max(Y[1], Y[2]));
    if (maxX - minX <= kSmallExtent && maxY - minY <= kSmallExtent) flags |= kFlagSmall;
    g.px0 = max((minX - 128 + 255) >> 8, P.clip_x0);
    g.px1 = min((maxX - 128) >> 8, P.clip_x1);
    g.py0 = max((minY - 128 + 255) >> 8, P.clip_y0);
    g.py1 = min((maxY - 128) >> 8, P.clip_y1);
    g.flags = flags;
    g.A2 = A2;
    return g.px0 <= g.px1 && g.py0 <= g.py1;
}

__device__ __forceinline__ bool prim_geometry(const DrawParams& P, const PrimIn& in, PrimGeom& g, int& ndropped) {
    if (!in.ok) return false;
    g.rv[0] = in.vid[0]; g.rv[1] = in.vid[1]; g.rv[2] = in.vid[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = in.p[k].x, y = in.p[k].y, zc = in.p[k].z, w = 1.0f;  // vsmain (triangle.slang:22)
        if (!(w > 0.0f)) { ++ndropped; return false; }
        const float xd = x / w, yd = y / w, zd = zc / w;
        const float xf = fmaf(xd, P.hw, P.cx), yf = fmaf(yd, P.hh, P.cy);
        if (!(fabsf(xf) < 4194304.0f && fabsf(yf) < 4194304.0f)) { ++ndropped; return false; }
        g.X[k] = (int32_t)rintf(xf * 256.0f);
        g.Y[k] = (int32_t)rintf(yf * 256.0f);
        g.z[k] = fmaf(zd, P.dr, P.dmin) + 0.0f;  // -0 -> +0 (k_tile relies on it)
    }
    long long A2 = (long long)(g.X[1] - g.X[0]) * (g.Y[2] - g.Y[0]) - (long long)(g.X[2] - g.X[0]) * (g.Y[1] - g.Y[0]);
    const bool ccw = A2 < 0;  // Vulkan: a = -A2/2 > 0 is counter-clockwise
    const bool front = (P.front_face == 0) ? ccw : !ccw;
    if (A2 == 0 || ((P.cull_mode & 1u) && front) || ((P.cull_mode & 2u) && !front)) return false;
    return orient_and_bound(P, g, A2);
}

// mesh.slang vsmain: clip = view_proj * (p, 1), column-major M[c * 4 + r], per row
// t = M0r x; t = fma(M1r, y, t); t = fma(M2r, z, t); c_r = t + M3r (zr_oracle.c).
__device__ __forceinline__ void mesh_transform(const float* M, const float3 p, float c[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float t = M[r] * p.x;
        t = fmaf(M[4 + r], p.y, t);
        t = fmaf(M[8 + r], p.z, t);
        c[r] = t + M[12 + r];
    }
}

// The camera matrix of the draw: the View uniform (device memory), or for a
// pipeline whose vertex stage takes it as push constants (mesh_push.slang) the
// bytes zr_cmd_push_constants recorded, carried in this launch's kernel arguments
// (DrawParams::push; every kernel here takes the one DrawParams at offset 0).
__device__ __forceinline__ const float* view_matrix(const DrawParams& P) {
    if (P.view_push) {
        const KernargParams kp = (KernargParams)__builtin_amdgcn_kernarg_segment_ptr();
        return (const float*)kp->push;
    }
    return P.view_proj;
}

// Sutherland-Hodgman against the Vulkan depth planes z >= 0, then z <= w (x / y
// use the guard band), vertex order kept from v0: new vertex a + t (b - a),
// t = da / (da - db).  Returns the polygon size (0, 3, 4 or 5).  Only primitives
// crossing a plane get here (mesh_geometry's fast path takes the rest).
__device__ __noinline__ int clip_polygon(const float (*in)[4], float (*out)[4]) {
    float a_[5][4], b_[5][4];
    int n = 3;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 4; ++k) a_[i][k] = in[i][k];
    for (int plane = 0; plane < 2; ++plane) {
        float (*src)[4] = plane == 0 ? a_ : b_;
        float (*dst)[4] = plane == 0 ? b_ : a_;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const float* a = src[i];
            const float* b = src[(i + 1) % n];
            const float da = plane == 0 ? a[2] : a[3] - a[2];
            const float db = plane == 0 ? b[2] : b[3] - b[2];
            if (da >= 0.0f) {
                for (int k = 0; k < 4; ++k) dst[m][k] = a[k];
                ++m;
            }
            if ((da >= 0.0f) != (db >= 0.0f)) {
                const float tt = da / (da - db);
                for (int k = 0; k < 4; ++k) dst[m][k] = fmaf(tt, b[k] - a[k], a[k]);
                ++m;
            }
        }
        n = m;
        if (n == 0) return 0;
    }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 4; ++k) out[i][k] = a_[i][k];
    return n;
}

// The mesh program's setup geometry: vertex stage, clip, viewport, snap, facing
// of the clipped polygon (sum of its fan's A2), cull, then each fan triangle
// (p0, pk, pk+1) oriented and bounded on its own.  valid bit k: fan k may cover.
struct MeshFans {
    PrimGeom f[kMeshFans];
    uint32_t valid;
};

__device__ __forceinline__ bool mesh_geometry(const DrawParams& P, const PrimIn& in, MeshFans& m, int& ndropped) {
    m.valid = 0;
    if (!in.ok) return false;
    float c[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k) mesh_transform(view_matrix(P), in.p[k], c[k]);
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) inside = inside && c[k][2] >= 0.0f && c[k][3] - c[k][2] >= 0.0f;
    float poly[5][4];
    int n = 3;
    if (inside) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) poly[k][j] = c[k][j];
    } else {
        n = clip_polygon(c, poly);
        if (n == 0) {
            ++ndropped;
            return false;
        }
    }
    int32_t X[5], Y[5];
    float Z[5];
    for (int k = 0; k < n; ++k) {
        const float x = poly[k][0], y = poly[k][1], z = poly[k][2], w = poly[k][3];
        if (!(w > 0.0f)) { ++ndropped; return false; }
        const float xd = x / w, yd = y / w, zd = z / w;
        const float xf = fmaf(xd, P.hw, P.cx), yf = fmaf(yd, P.hh, P.cy);
        if (!(fabsf(xf) < 4194304.0f && fabsf(yf) < 4194304.0f)) { ++ndropped; return false; }
        X[k] = (int32_t)rintf(xf * 256.0f);
        Y[k] = (int32_t)rintf(yf * 256.0f);
        Z[k] = fmaf(zd, P.dr, P.dmin) + 0.0f;  // -0 -> +0
    }
    long long Asum = 0;
    for (int k = 1; k + 1 < n; ++k)
        Asum += (long long)(X[k] - X[0]) * (Y[k + 1] - Y[0]) - (long long)(X[k + 1] - X[0]) * (Y[k] - Y[0]);
    const bool ccw = Asum < 0;
    const bool front = (P.front_face == 0) ? ccw : !ccw;
    if (Asum == 0 || ((P.cull_mode & 1u) && front) || ((P.cull_mode & 2u) && !front)) return false;
    for (int k = 1; k + 1 < n; ++k) {
        PrimGeom& g = m.f[k - 1];
        g.X[0] = X[0]; g.X[1] = X[k]; g.X[2] = X[k + 1];
        g.Y[0] = Y[0]; g.Y[1] = Y[k]; g.Y[2] = Y[k + 1];
        g.z[0] = Z[0]; g.z[1] = Z[k]; g.z[2] = Z[k + 1];
        g.rv[0] = in.vid[0]; g.rv[1] = in.vid[1]; g.rv[2] = in.vid[2];
        const long long A2 = (long long)(g.X[1] - g.X[0]) * (g.Y[2] - g.Y[0]) -
                             (long long)(g.X[2] - g.X[0]) * (g.Y[1] - g.Y[0]);
        if (A2 != 0 && orient_and_bound(P, g, A2)) m.valid |= 1u << (k - 1);
    }
    return m.valid != 0;
}

// mesh_geometry for a primitive that needs no clipping (all vertices inside
// 0 <= z <= w): one fan, the same operations on fixed indices, so everything
// stays in registers (the general path's polygon arrays live in scratch).
__device__ __forceinline__ bool mesh_geometry_unclipped(const DrawParams& P, const PrimIn& in, const float c[3][4],
                                                        PrimGeom& g, int& ndropped) {
    int32_t X[3], Y[3];
    float Z[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = c[k][0], y = c[k][1], z = c[k][2], w = c[k][3];
        if (!(w > 0.0f)) { ++ndropped; return false; }
        const float xd = x / w, yd = y / w, zd = z / w;
        const float xf = fmaf(xd, P.hw, P.cx), yf = fmaf(yd, P.hh, P.cy);
        if (!(fabsf(xf) < 4194304.0f && fabsf(yf) < 4194304.0f)) { ++ndropped; return false; }
        X[k] = (int32_t)rintf(xf * 256.0f);
        Y[k] = (int32_t)rintf(yf * 256.0f);
        Z[k] = fmaf(zd, P.dr, P.dmin) + 0.0f;  // -0 -> +0
    }
    const long long A2 = (long long)(X[1] - X[0]) * (Y[2] - Y[0]) - (long long)(X[2] - X[0]) * (Y[1] - Y[0]);
    const bool ccw = A2 < 0;
    const bool front = (P.front_face == 0) ? ccw : !ccw;
    if (A2 == 0 || ((P.cull_mode & 1u) && front) || ((P.cull_mode & 2u) && !front)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.X[k] = X[k];
        g.Y[k] = Y[k];
        g.z[k] = Z[k];
        g.rv[k] = in.vid[k];
    }
    return orient_and_bound(P, g, A2);
}

// Counts the owned (tile, primitive) pairs of a set-up triangle in the LDS
// histogram; returns how many there are.
// The first tile row at or after ty0 that this shard owns (ty % G == rank) and its
// index among the owned rows; the next owned row is G further.  One division per
// primitive, none when the target is not sharded (G == 1, wave-uniform).
__device__ __forceinline__ int first_owned_row(uint32_t G, uint32_t rank, int ty0, uint32_t& orow) {
    if (G == 1u) {
        orow = (uint32_t)ty0;
        return ty0;
    }
    const uint32_t q = (uint32_t)ty0 / G, m = (uint32_t)ty0 - q * G;
    orow = m <= rank ? q : q + 1u;
    return (int)(orow * G + rank);
}

// Calls fn(owned tile index, tx, ty) for every tile of [tx0, tx1] x [ty0, ty1]
// this shard owns (ShardGeom): its round-robin rows, then the leftover rows'
// tiles inside its run.  G == 1: every tile, index ty * tiles_x + tx.
template <typename Fn>
__device__ __forceinline__ void for_owned_tiles(uint32_t G, uint32_t rank, uint32_t tiles_x, uint32_t full_rows,
                                                uint32_t own_rows, uint32_t left_lo, uint32_t left_hi, int tx0, int ty0,
                                                int tx1, int ty1, Fn&& fn) {
    uint32_t orow;
    const int tyf = min(ty1, (int)full_rows - 1);
    for (int ty = first_owned_row(G, rank, ty0, orow); ty <= tyf; ty += (int)G, ++orow) {
        const uint32_t row = orow * tiles_x;
        for (int tx = tx0; tx <= tx1; ++tx) fn(row + (uint32_t)tx, tx, ty);
    }
    for (int ty = max(ty0, (int)full_rows); ty <= ty1; ++ty) {  // leftover rows (G > 1 only)
        const int i0 = (ty - (int)full_rows) * (int)tiles_x;
        const int c0 = max(tx0, (int)left_lo - i0), c1 = min(tx1, (int)left_hi - 1 - i0);
        const uint32_t base = own_rows * tiles_x + (uint32_t)(i0 - (int)left_lo);
        for (int tx = c0; tx <= c1; ++tx) fn(base + (uint32_t)tx, tx, ty);
    }
}

__device__ __forceinline__ uint32_t count_owned_box(const DrawParams& P, int px0, int py0, int px1, int py1,
                                                    uint32_t* s_hist) {
    const uint32_t tsh = P.tile_shift;
    const int tx0 = px0 >> tsh, tx1 = px1 >> tsh;
    const int ty0 = py0 >> tsh, ty1 = py1 >> tsh;
    uint32_t owned = 0;
    for_owned_tiles(P.shard_count, P.shard_rank, P.tiles_x, P.full_rows, P.own_rows, P.left_lo, P.left_hi, tx0, ty0,
                    tx1, ty1, [&](uint32_t t, int, int) {
                        atomicAdd(&s_hist[t], 1u);
                        ++owned;
                    });
    return owned;
}

__device__ __forceinline__ uint32_t count_owned(const DrawParams& P, const PrimGeom& g, uint32_t* s_hist) {
    return count_owned_box(P, g.px0, g.py0, g.px1, g.py1, s_hist);
}

// A compact record (as two 16-B words) whose primitive is too large for int16 deltas.
__device__ __forceinline__ bool compact_is_large(const int4 q0) { return (int16_t)(q0.z & 0xFFFF) == kCompactLarge; }
// A large primitive covering at most a quarter of its bbox (dy1 == 1 in its
// compact record; the lane walk takes it even in the last cost bucket, k_tile).
__device__ __forceinline__ bool compact_is_sliver(const int4 q0) { return (q0.z >> 16) == 1; }

// The compact record and the clipped pixel bbox of a set-up triangle.
__device__ __forceinline__ TriCompact make_compact(const PrimGeom& g, BBox& box) {
    const int32_t* X = g.X;
    const int32_t* Y = g.Y;
    const float invA2 = 1.0f / (float)g.A2;
    const bool small = (g.flags & kFlagSmall) != 0u;
    TriCompact c;
    c.X0 = X[0]; c.Y0 = Y[0];
    c.dx1 = small ? (int16_t)(X[1] - X[0]) : kCompactLarge;
    const long long bbox = (long long)(max(X[0], max(X[1], X[2])) - min(X[0], min(X[1], X[2]))) *
                           (max(Y[0], max(Y[1], Y[2])) - min(Y[0], min(Y[1], Y[2])));
    c.dy1 = small ? (int16_t)(Y[1] - Y[0]) : (int16_t)(bbox >= 2 * g.A2 ? 1 : 0);  // large: the sliver flag
    c.dx2 = small ? (int16_t)(X[2] - X[0]) : (int16_t)0;
    c.dy2 = small ? (int16_t)(Y[2] - Y[0]) : (int16_t)0;
    c.z0 = g.z[0];
    c.dz1 = g.z[1] - g.z[0];
    c.dz2 = g.z[2] - g.z[0];
    c.invA2s = (g.flags & kFlagSwapped) ? -invA2 : invA2;
    box.bb0 = (uint32_t)g.px0 | ((uint32_t)g.py0 << 16);
    box.bb1 = (uint32_t)g.px1 | ((uint32_t)g.py1 << 16);
    return c;
}

// Stores setup record `rec` (compact, plus the full record for a large
// triangle) and returns its tile bbox.
__device__ __forceinline__ BBox write_record(const DrawParams& P, uint32_t rec, const PrimGeom& g) {
    BBox box;
    const TriCompact c = make_compact(g, box);
    P.records[rec] = c;
    if (!(g.flags & kFlagSmall)) {
        TriRecord r;
        r.X0 = g.X[0]; r.Y0 = g.Y[0]; r.X1 = g.X[1]; r.Y1 = g.Y[1]; r.X2 = g.X[2]; r.Y2 = g.Y[2];
        r.z0 = c.z0; r.dz1 = c.dz1; r.dz2 = c.dz2;
        r.invA2 = fabsf(c.invA2s);
        r.v0 = g.rv[0]; r.v1 = g.rv[1]; r.v2 = g.rv[2];
        r.bb0 = box.bb0;
        r.bb1 = box.bb1;
        r.flags = g.flags;
        P.records_big[rec] = r;
    }
    return box;
}

// The mesh program's barycentric planes: with the homogeneous
// screen vertices h_i = (x_i hw + w_i cx, y_i hh + w_i cy, w_i) of the primitive
// (not of its clipped fans), E_i(p) = p . (h_j x h_k) = c0 fx + c1 fy + c2.
// Evaluated relative to a reference pixel r near the primitive (r = floor of
// vertex 0's screen position), E_i = c0 (px - rx) + c1 (py - ry) + c2r with c2r
// = E_i at r's centre: the plane constants are formed in double and rounded once,
// so the resolve's float32 evaluation has no cancellation between large terms.
// e = {c0_0, c1_0, c2r_0, c0_1, c1_1, c2r_1, c0_2, c1_2, c2r_2, rx, ry, 0}
// (zr_oracle.c mesh_planes, same operations).
__device__ __forceinline__ void mesh_edge_planes(const DrawParams& P, const float3 p[3], float e[12]) {
    double hX[3], hY[3], hW[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float c[4];
        mesh_transform(view_matrix(P), p[k], c);
        hX[k] = (double)c[0] * (double)P.hw + (double)c[3] * (double)P.cx;
        hY[k] = (double)c[1] * (double)P.hh + (double)c[3] * (double)P.cy;
        hW[k] = (double)c[3];
    }
    // (a primitive reaching here has w > 0 at vertex 0 unless it was clipped; the
    // reference pixel only has to be finite: clamped to the guard band)
    double rx = hW[0] > 0.0 ? floor(hX[0] / hW[0]) : 0.0, ry = hW[0] > 0.0 ? floor(hY[0] / hW[0]) : 0.0;
    rx = fmin(fmax(rx, -4194304.0), 4194304.0);
    ry = fmin(fmax(ry, -4194304.0), 4194304.0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const double c0 = hY[j] * hW[k] - hW[j] * hY[k];
        const double c1 = hW[j] * hX[k] - hX[j] * hW[k];
        const double c2 = hX[j] * hY[k] - hY[j] * hX[k];
        e[3 * i + 0] = (float)c0;
        e[3 * i + 1] = (float)c1;
        e[3 * i + 2] = (float)((c0 * (rx + 0.5) + c1 * (ry + 0.5)) + c2);
    }
    e[9] = (float)rx;
    e[10] = (float)ry;
    e[11] = 0.0f;
}

// E_i of pixel (px, py) from the stored planes (float32, see mesh_edge_planes).
__device__ __forceinline__ void mesh_plane_eval(const float* e, int px, int py, float E[3]) {
    const float dx = (float)px - e[9], dy = (float)py - e[10];  // exact: integers below 2^24
#pragma unroll
    for (int i = 0; i < 3; ++i) E[i] = fmaf(e[3 * i], dx, fmaf(e[3 * i + 1], dy, e[3 * i + 2]));
}

// Setup record index of fan k of mesh primitive p (zr_internal.h kMeshFans).
__device__ __forceinline__ uint32_t mesh_record(const DrawParams& P, uint32_t p, uint32_t k) {
    return k ? P.prims + 2u * p + k - 1u : p;
}

// The mesh program's setup of primitive `prim`: returns fan 0's bbox, stores fans
// 1 and 2's in their global slots (empty when absent).
__device__ __forceinline__ BBox setup_finish_mesh(const DrawParams& P, uint32_t prim, const PrimIn& in,
                                                  uint32_t* s_hist, int& nvalid, int& ndropped) {
    BBox box[kMeshFans];
#pragma unroll
    for (uint32_t k = 0; k < kMeshFans; ++k) box[k] = BBox{kEmptyBox, 0u};
    bool fast = in.ok;
    float c[3][4];
    if (fast) {
#pragma unroll
        for (int k = 0; k < 3; ++k) mesh_transform(view_matrix(P), in.p[k], c[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) fast = fast && c[k][2] >= 0.0f && c[k][3] - c[k][2] >= 0.0f;
    }
    if (fast) {
        PrimGeom g;
        if (mesh_geometry_unclipped(P, in, c, g, ndropped)) {
            ++nvalid;
            if (count_owned(P, g, s_hist)) {
                box[0] = write_record(P, prim, g);
                float e[12];
                mesh_edge_planes(P, in.p, e);
                float4* q = P.mesh_edges + (size_t)prim * 3u;
                q[0] = make_float4(e[0], e[1], e[2], e[3]);
                q[1] = make_float4(e[4], e[5], e[6], e[7]);
                q[2] = make_float4(e[8], e[9], e[10], e[11]);
            }
        }
    } else {  // clipped (or invalid): the general path
        MeshFans m;
        if (mesh_geometry(P, in, m, ndropped)) {
            ++nvalid;
            bool owned = false;
            for (uint32_t k = 0; k < kMeshFans; ++k) {
                if (!((m.valid >> k) & 1u)) continue;
                if (count_owned(P, m.f[k], s_hist)) {
                    box[k] = write_record(P, mesh_record(P, prim, k), m.f[k]);
                    owned = true;
                }
            }
            if (owned) {  // the resolve's barycentric planes (shade_mesh)
                float e[12];
                mesh_edge_planes(P, in.p, e);
                float4* q = P.mesh_edges + (size_t)prim * 3u;
                q[0] = make_float4(e[0], e[1], e[2], e[3]);
                q[1] = make_float4(e[4], e[5], e[6], e[7]);
                q[2] = make_float4(e[8], e[9], e[10], e[11]);
            }
        }
    }
    P.bboxes[mesh_record(P, prim, 1)] = box[1];
    P.bboxes[mesh_record(P, prim, 2)] = box[2];
    return box[0];
}

// A micro primitive: its clipped bbox is one pixel, so at most that pixel's
// centre is a sample, and it is small (extents <= 64 px), so its edge values
// there fit int32 (products below 2^28, as in k_tile's lane walk).  Whether it
// covers the sample, by k_tile's biased sign test: one that does not yields no
// fragment and needs neither a record nor a bin entry (DrawParams::micro; k_tile
// tests the covered ones again, with their depth).
__device__ __forceinline__ bool micro_covers(const PrimGeom& g) {
    const int Sx = g.px0 * 256 + 128, Sy = g.py0 * 256 + 128;
    const int* X = g.X;
    const int* Y = g.Y;
    const int w0 = (X[2] - X[1]) * (Sy - Y[1]) - (Y[2] - Y[1]) * (Sx - X[1]) - (int)((g.flags >> 1) & 1u);
    const int w1 = (X[0] - X[2]) * (Sy - Y[2]) - (Y[0] - Y[2]) * (Sx - X[2]) - (int)((g.flags >> 2) & 1u);
    const int w2 = (X[1] - X[0]) * (Sy - Y[0]) - (Y[1] - Y[0]) * (Sx - X[0]) - (int)((g.flags >> 3) & 1u);
    return (w0 | w1 | w2) >= 0;
}

// Setup of draw primitive `prim`; returns its tile bbox (empty when culled,
// owning no tile, or a micro primitive that misses its sample).
__device__ __forceinline__ BBox setup_finish(const DrawParams& P, uint32_t prim, const PrimIn& in, uint32_t* s_hist,
                                             int& nvalid, int& ndropped, int& nmicro) {
    BBox box{kEmptyBox, 0u};
    PrimGeom g;
    if (prim_geometry(P, in, g, ndropped)) {
        ++nvalid;
        if (P.micro && g.px0 == g.px1 && g.py0 == g.py1 && (g.flags & kFlagSmall)) {
            if (!micro_covers(g)) return box;  // no fragment: no record, no bin entry
            ++nmicro;
        }
        if (count_owned(P, g, s_hist)) box = write_record(P, prim, g);
    }
    return box;
}

// Records mode (partitioned setup): received entry `pos` of the
// blocks (s_pre: exclusive prefix of the blocks' counts, G + 1 entries, in LDS).
// The sender set the primitive up: its compact record is stored at its draw id
// and its bbox counted; a large primitive (no compact form) is set up again here
// from the vertices every rank holds.  Returns the bbox; *gid = the draw id.
__device__ __forceinline__ BBox receive_entry(const DrawParams& P, const uint32_t* s_pre, uint32_t pos, uint32_t* s_hist,
                                              int& nvalid, int& ndropped, uint32_t& gid) {
    uint32_t src = 0;
    while (src + 1u < P.shard_count && pos >= s_pre[src + 1u]) ++src;
    const int4* e = reinterpret_cast<const int4*>(P.rlist + (size_t)src * route_block_bytes(P.route_cap) +
                                                  sizeof(RouteHeader) + (size_t)(pos - s_pre[src]) * sizeof(RouteEntry));
    const int4 q0 = e[0], q1 = e[1], q2 = e[2];
    gid = (uint32_t)q2.z;
    BBox box{(uint32_t)q2.x, (uint32_t)q2.y};
    ++nvalid;
    if (!compact_is_large(q0)) {
        int4* r = reinterpret_cast<int4*>(P.records + gid);
        r[0] = q0;
        r[1] = q1;
        count_owned_box(P, (int)(box.bb0 & 0xFFFFu), (int)(box.bb0 >> 16), (int)(box.bb1 & 0xFFFFu), (int)(box.bb1 >> 16),
                        s_hist);
        return box;
    }
    PrimIn in;
    fetch_indices_gid(P, gid, in);
    fetch_positions(P, in);
    PrimGeom g;
    if (prim_geometry(P, in, g, ndropped) && count_owned(P, g, s_hist)) return write_record(P, gid, g);
    return BBox{kEmptyBox, 0u};
}

}  // namespace zr
