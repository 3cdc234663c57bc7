// zr_raster.h — k_tile's rasterizers: record decode, the wave path (raster_prim) and the lane walk (raster_lane).
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_dev_common.h"

namespace zr {

__device__ __forceinline__ int rl(int v, uint32_t lane) { return __builtin_amdgcn_readlane(v, lane); }

// Rasterize one primitive (wave-uniform record) into the tile's LDS keys: lanes
// sweep the primitive's bbox ∩ tile, packed power-of-two rows per pass.
// Expands a compact record (two 16-B words, TriCompact) into the TriRecord fields
// the raster and resolve use: vertices, depth terms, |1/A2|, kFlagSmall/Swapped,
// and with `full` also the top-left bias flags and the clipped pixel bbox, computed
// exactly as k_setup_bin computed them.  v0..v2 are not part of the compact form.
// The top-left bias flags and the clipped pixel bbox of a record's vertices,
// computed exactly as k_setup_bin computed them.
__device__ __forceinline__ void finish_record(const DrawParams& P, TriRecord& r) {
    const int X[3] = {r.X0, r.X1, r.X2}, Y[3] = {r.Y0, r.Y1, r.Y2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // top-left rule (y-down), edge i opposite vertex i
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        const int dx = X[b] - X[a], dy = Y[b] - Y[a];
        if (!((dy < 0) || (dy == 0 && dx > 0))) r.flags |= (kFlagBias0 << i);
    }
    const int minX = min(X[0], min(X[1], X[2])), maxX = max(X[0], max(X[1], X[2]));
    const int minY = min(Y[0], min(Y[1], Y[2])), maxY = max(Y[0], max(Y[1], Y[2]));
    const int px0 = max((minX - 128 + 255) >> 8, P.clip_x0), px1 = min((maxX - 128) >> 8, P.clip_x1);
    const int py0 = max((minY - 128 + 255) >> 8, P.clip_y0), py1 = min((maxY - 128) >> 8, P.clip_y1);
    r.bb0 = (uint32_t)px0 | ((uint32_t)py0 << 16);
    r.bb1 = (uint32_t)px1 | ((uint32_t)py1 << 16);
}

__device__ __forceinline__ TriRecord decode_compact(const DrawParams& P, const int4 q0, const int4 q1, bool full) {
    TriRecord r;
    r.X0 = q0.x; r.Y0 = q0.y;
    r.X1 = q0.x + (int)(int16_t)(q0.z & 0xFFFF); r.Y1 = q0.y + (q0.z >> 16);
    r.X2 = q0.x + (int)(int16_t)(q0.w & 0xFFFF); r.Y2 = q0.y + (q0.w >> 16);
    r.z0 = __int_as_float(q1.x); r.dz1 = __int_as_float(q1.y); r.dz2 = __int_as_float(q1.z);
    r.invA2 = fabsf(__int_as_float(q1.w));
    r.flags = kFlagSmall | ((q1.w < 0) ? kFlagSwapped : 0u);
    r.v0 = r.v1 = r.v2 = 0u;
    r.bb0 = r.bb1 = 0u;
    if (full) finish_record(P, r);
    return r;
}

// A compact record for the lane walk; for a large primitive (large: its compact
// record holds vertex 0, the depth terms and |1/A2|, the same values as its full
// record) with vertices 1 and 2 from records_big (X1, Y1, X2, Y2: bytes 8-23).
// Biases and bbox as setup computed them.
__device__ __forceinline__ TriRecord decode_large(const DrawParams& P, const int4 q0, const int4 q1, bool large,
                                                  const int2 v1, const int2 v2) {
    TriRecord r;
    r.X0 = q0.x; r.Y0 = q0.y;
    r.X1 = large ? v1.x : q0.x + (int)(int16_t)(q0.z & 0xFFFF); r.Y1 = large ? v1.y : q0.y + (q0.z >> 16);
    r.X2 = large ? v2.x : q0.x + (int)(int16_t)(q0.w & 0xFFFF); r.Y2 = large ? v2.y : q0.y + (q0.w >> 16);
    r.z0 = __int_as_float(q1.x); r.dz1 = __int_as_float(q1.y); r.dz2 = __int_as_float(q1.z);
    r.invA2 = fabsf(__int_as_float(q1.w));
    r.flags = (q1.w < 0) ? kFlagSwapped : 0u;
    r.v0 = r.v1 = r.v2 = 0u;
    finish_record(P, r);
    return r;
}

// Whether the lane walk (raster_lane) is exact for a large primitive in this
// tile: every edge value it tests, over bbox ∩ tile widened by the walk's
// kLaneStep - 1 columns on either side, must fit int32.  The edge functions are linear, so
// their extremes are at the rectangle's corners: |w| <= |w(corner)| + |dy| 256 W
// + |dx| 256 H, bounded in int64 against 2^31 - 1.
template <int TS>
__device__ __forceinline__ bool lane_walk_fits(const TriRecord& r, int x0, int y0) {
    constexpr int T = 1 << TS;
    const int bx0 = max((int)(r.bb0 & 0xFFFFu), x0) - (kLaneStep - 1), by0 = max((int)(r.bb0 >> 16), y0);
    const int bx1 = min((int)(r.bb1 & 0xFFFFu), x0 + T - 1) + (kLaneStep - 1);
    const int by1 = min((int)(r.bb1 >> 16), y0 + T - 1);
    const long long Sx = (long long)bx0 * 256 + 128, Sy = (long long)by0 * 256 + 128;
    const long long Wd = (long long)(bx1 - bx0) * 256, Hd = (long long)max(by1 - by0, 0) * 256;
    auto edge = [&](int Xa, int Ya, int Xb, int Yb) {
        const long long dx = (long long)Xb - Xa, dy = (long long)Yb - Ya;
        const long long w = dx * (Sy - Ya) - dy * (Sx - Xa);
        return llabs(w) + llabs(dy) * Wd + llabs(dx) * Hd;
    };
    const long long m = max(edge(r.X1, r.Y1, r.X2, r.Y2), max(edge(r.X2, r.Y2, r.X0, r.Y0), edge(r.X0, r.Y0, r.X1, r.Y1)));
    return m < 0x7FFFFFFFll;
}

// A wave-uniform full record, moved to scalar registers right after the load so
// the wave path does not hold 16 more VGPRs.
__device__ __forceinline__ TriRecord uniform_record(const int4 a, const int4 b, const int4 c, const int4 d) {
    auto u = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    TriRecord r;
    r.X0 = u(a.x); r.Y0 = u(a.y); r.X1 = u(a.z); r.Y1 = u(a.w);
    r.X2 = u(b.x); r.Y2 = u(b.y);
    r.z0 = __int_as_float(u(b.z)); r.dz1 = __int_as_float(u(b.w));
    r.dz2 = __int_as_float(u(c.x)); r.invA2 = __int_as_float(u(c.y));
    r.v0 = (uint32_t)u(c.z); r.v1 = (uint32_t)u(c.w); r.v2 = (uint32_t)u(d.x);
    r.bb0 = (uint32_t)u(d.y); r.bb1 = (uint32_t)u(d.z); r.flags = (uint32_t)u(d.w);
    return r;
}

__device__ __forceinline__ TriRecord load_uniform_record(const TriRecord* p) {
    const int4* q = reinterpret_cast<const int4*>(p);
    return uniform_record(q[0], q[1], q[2], q[3]);
}


// Row sweeps raster_prim makes over a record's bbox ∩ tile (kDebugStamps).
template <int TS>
__device__ __forceinline__ uint32_t prim_sweeps(const TriRecord& r, int x0, int y0) {
    constexpr int T = 1 << TS;
    const int bw = min((int)(r.bb1 & 0xFFFFu), x0 + T - 1) - max((int)(r.bb0 & 0xFFFFu), x0) + 1;
    const int bh = min((int)(r.bb1 >> 16), y0 + T - 1) - max((int)(r.bb0 >> 16), y0) + 1;
    if (bw <= 0 || bh <= 0) return 0u;
    const int sh = bw <= 1 ? 0 : 32 - __clz(bw - 1);
    const int rows = 64 >> sh;
    return (uint32_t)((bh + rows - 1) / rows);
}

template <int MODE, bool INITD, int TS>
__device__ __forceinline__ void raster_prim(const DrawParams& P, const TriRecord& r, uint32_t seq, int x0, int y0,
                                            int lane, unsigned long long* s_key, const float* s_initd) {
    constexpr int T = 1 << TS;
    const int bx0 = max((int)(r.bb0 & 0xFFFFu), x0), by0 = max((int)(r.bb0 >> 16), y0);
    const int bx1 = min((int)(r.bb1 & 0xFFFFu), x0 + T - 1), by1 = min((int)(r.bb1 >> 16), y0 + T - 1);
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    if (bw <= 0 || bh <= 0) return;
    const int sh = bw <= 1 ? 0 : 32 - __clz(bw - 1);
    const int rows = 64 >> sh;
    const int lx = lane & ((1 << sh) - 1), lyo = lane >> sh;
    const long long bias0 = (r.flags >> 1) & 1, bias1 = (r.flags >> 2) & 1, bias2 = (r.flags >> 3) & 1;
    const DepthPlane dp = depth_plane(r.z0, r.dz1, r.dz2, r.invA2, (int)bias1, (int)bias2);
    const float dlo = P.dlo, dhi = P.dhi;  // (held: a per-pass kernarg reload waits on the scalar cache)
    // The lane's biased edge values at its first pixel, then stepped by `rows`
    // pixel rows per pass in int64 (exact; a pass was two int64 products per edge.
    // Stepping in double measured slower: cerberus 48.5 -> 51.3 us)
    const EdgeEval e = eval_edges(r, bx0 + lx, by0 + lyo);
    long long w0 = e.w0 - bias0, w1 = e.w1 - bias1, w2 = e.w2 - bias2;
    const long long s0 = (long long)(r.X2 - r.X1) * (256 * rows), s1 = (long long)(r.X0 - r.X2) * (256 * rows);
    const long long s2 = (long long)(r.X1 - r.X0) * (256 * rows);
    for (int ry = 0; ry < bh; ry += rows) {
        const int ly = ry + lyo;
        if (lx < bw && ly < bh && (w0 | w1 | w2) >= 0) {
            const float z = plane_z(dp, (float)w1, (float)w2);
            if (z >= dlo && z <= dhi) {
                const int li = (by0 + ly - y0) * T + (bx0 + lx - x0);
                if (!INITD || depth_pass(P.depth_op, z, s_initd[li])) atomicMin(&s_key[li], frag_key<MODE>(z, seq));
            }
        }
        w0 += s0;
        w1 += s1;
        w2 += s2;
    }
}

// Lane-parallel path for small primitives (kFlagSmall): each lane walks its own
// primitive's bbox ∩ tile in row order, stepping the three edge functions
// incrementally in int32 (exact: |w| <= 2^29 inside a small primitive's bbox).
// With k = 2^ksh lanes per primitive (sparse tiles), lane `sub` of the
// primitive's group takes the bbox rows sub, sub + k, ...
template <int MODE, bool INITD, int TS>
__device__ __forceinline__ void raster_lane(const DrawParams& P, const TriRecord& r, uint32_t seq, int x0, int y0,
                                            unsigned long long* s_key, const float* s_initd, int sub, int ksh) {
    constexpr int T = 1 << TS;
    const int k = 1 << ksh;
    const int X0 = r.X0, Y0 = r.Y0, X1 = r.X1, Y1 = r.Y1, X2 = r.X2, Y2 = r.Y2;
    const float z0 = r.z0, dz1 = r.dz1, dz2 = r.dz2, invA2 = r.invA2;
    const uint32_t bb0 = r.bb0, bb1 = r.bb1, flags = r.flags;
    int bx0 = max((int)(bb0 & 0xFFFFu), x0);
    const int by0 = max((int)(bb0 >> 16), y0);
    const int bx1 = min((int)(bb1 & 0xFFFFu), x0 + T - 1), by1 = min((int)(bb1 >> 16), y0 + T - 1);
    int bw = bx1 - bx0 + 1;
    const int bh = by1 - by0 + 1;
    if (bw <= 0 || bh <= sub) return;
    // S pixels of a row per step (kLaneStep).  A row whose width is not a multiple
    // of S leaves samples of its last step past the bbox.  When the bbox's right
    // side is the primitive's own x extent (not cut by the tile or the scissor)
    // they lie right of every vertex, so they are never covered; else, when the
    // left side is its own extent, the steps start that many columns further left
    // (left of every vertex).  Only when both sides are cut does the step test
    // for them (chk: pixels j >= rem of the row's last step).
    constexpr int S = kLaneStep;
    bool chk = false;
    int rem = S;
    if (bw & (S - 1)) {
        const int minX = min(X0, min(X1, X2)), maxX = max(X0, max(X1, X2));
        if (bx1 != (maxX - 128) >> 8) {
            if (bx0 == (minX - 128 + 255) >> 8) {
                const int e = S - (bw & (S - 1));
                bx0 -= e;
                bw += e;
            } else {
                chk = true;
                rem = bw & (S - 1);
            }
        }
    }
    // Edge values and steps in arithmetic mod 2^32 (u32 products and sums): exact
    // wherever the true value fits int32, which holds at every sample the walk
    // tests -- a small primitive's |w| <= 2^29, a large one is sent here only when
    // lane_walk_fits bounds its values over bbox ∩ tile -- whatever the steps'
    // own magnitudes (a row wrap's jump may exceed int32; the sum it lands on does not).
    auto wr = [](uint32_t a) { return (int)a; };
    const int Sx = bx0 * 256 + 128, Sy = (by0 + sub) * 256 + 128;
    const uint32_t dx0 = X2 - X1, dy0 = Y2 - Y1, dx1 = X0 - X2, dy1 = Y0 - Y2, dx2 = X1 - X0, dy2 = Y1 - Y0;
    int r0 = wr(dx0 * (uint32_t)(Sy - Y1) - dy0 * (uint32_t)(Sx - X1));
    int r1 = wr(dx1 * (uint32_t)(Sy - Y2) - dy1 * (uint32_t)(Sx - X2));
    int r2 = wr(dx2 * (uint32_t)(Sy - Y0) - dy2 * (uint32_t)(Sx - X0));
    const int sx0 = wr(0u - dy0 * 256u), sx1 = wr(0u - dy1 * 256u), sx2 = wr(0u - dy2 * 256u);  // +1 pixel in x
    const int sy0 = wr(dx0 * 256u), sy1 = wr(dx1 * 256u), sy2 = wr(dx2 * 256u);                 // +1 pixel in y
    const int b0 = (int)((flags >> 1) & 1u), b1 = (int)((flags >> 2) & 1u), b2 = (int)((flags >> 3) & 1u);
    // Sweep the bbox in row order, stepping the edge values: +sx per pixel, and at
    // the end of a row the jump back to the next row's first pixel, chosen with
    // selects (no divergent branch: a nested row / column loop, or a wrap branch,
    // idles the lanes of narrower primitives and measured slower).  The top-left
    // bias is folded into the edge values, so coverage is one sign test, and the
    // depth plane is defined on the biased values (§3.6).  Fragment depth is never
    // -0 here: setup canonicalised the vertex depths to +0 (the oracle's
    // per-fragment -0 -> +0 rule therefore gives the same bits).  The sweep ends when the key address reaches the row after the
    // last one (no separate step counter).
    const int rows = (bh - sub + k - 1) >> ksh;
    int w0 = wr((uint32_t)r0 - b0), w1 = wr((uint32_t)r1 - b1), w2 = wr((uint32_t)r2 - b2);
    int ex = 0;
    uint32_t la = (uint32_t)(((by0 + sub - y0) * T + (bx0 - x0)) * 8);  // byte offset of the key
    const uint32_t la_end = la + (uint32_t)(rows * k * T * 8);
    // The depth-range test (fragments outside [dlo, dhi] are discarded, §3) is
    // dropped from the loop when every lane's vertex depths lie inside the range
    // by a margin far above the interpolation's rounding (a few ulp of 1): then
    // no fragment can fall outside.  NaN depths fail the comparisons, so keep it.
    const float z1v = z0 + dz1, z2v = z0 + dz2, zlo = P.dlo + 1e-4f, zhi = P.dhi - 1e-4f;
    const bool zsafe = z0 >= zlo && z0 <= zhi && z1v >= zlo && z1v <= zhi && z2v >= zlo && z2v <= zhi;
    // one covered sample: depth from the (un-biased) edge values, test, key
    const DepthPlane dp = depth_plane(z0, dz1, dz2, invA2, b1, b2);
    auto frag = [&](auto ztest, int e1, int e2, uint32_t a) {
        const float z = plane_z(dp, (float)e1, (float)e2);  // e1, e2: the biased values
        if ((!decltype(ztest)::value || (z >= P.dlo && z <= P.dhi)) &&
            (!INITD || depth_pass(P.depth_op, z, s_initd[a >> 3])))
            atomicMin(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(s_key) + a), frag_key<MODE>(z, seq));
    };
    // S pixels of a row per step (VALU and loop-control SALU are what the lane
    // walk spends: one step's wrap selects and branch bookkeeping serve S
    // samples).  Pixels j >= rem of a row's last step (index lastB) lie past a
    // bbox cut on both sides and are skipped.
    const int hw = (bw + S - 1) / S, lastB = chk ? hw - 1 : hw;
    const int t0 = wr((uint32_t)S * sx0), t1 = wr((uint32_t)S * sx1), t2 = wr((uint32_t)S * sx2);
    const uint32_t kk = (uint32_t)k, hh = (uint32_t)S * (uint32_t)(hw - 1);
    const int q0 = wr(kk * sy0 - hh * sx0), q1 = wr(kk * sy1 - hh * sx1), q2 = wr(kk * sy2 - hh * sx2);
    const uint32_t lq = (uint32_t)((k * T - S * (hw - 1)) * 8);
    auto sweep = [&](auto ztest, auto wchk) {
        do {
            int a0 = w0, a1 = w1, a2 = w2;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                if (j) {
                    a0 = wr((uint32_t)a0 + sx0);
                    a1 = wr((uint32_t)a1 + sx1);
                    a2 = wr((uint32_t)a2 + sx2);
                }
                if ((j == 0 || !decltype(wchk)::value || ex != lastB || j < rem) && (a0 | a1 | a2) >= 0)
                    frag(ztest, a1, a2, la + 8u * (uint32_t)j);
            }
            const bool wrap = ++ex == hw;
            ex = wrap ? 0 : ex;
            w0 = wr((uint32_t)w0 + (wrap ? q0 : t0));
            w1 = wr((uint32_t)w1 + (wrap ? q1 : t1));
            w2 = wr((uint32_t)w2 + (wrap ? q2 : t2));
            la += wrap ? lq : 8u * (uint32_t)S;
        } while (la != la_end);
    };
    const bool wchk = __ballot(chk) != 0ull;
    const bool wz = __ballot(!zsafe) != 0ull;
    if (!wz && !wchk)
        sweep(std::false_type{}, std::false_type{});
    else if (!wz)
        sweep(std::false_type{}, std::true_type{});
    else if (!wchk)
        sweep(std::true_type{}, std::false_type{});
    else
        sweep(std::true_type{}, std::true_type{});
}

}  // namespace zr
