// zr_dev_common.h — device helpers every pass uses: the draw's parameters, index
// fetch, visibility keys, edge and depth-plane evaluation.
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_internal.h"

namespace zr {

// k_tile's view of DrawParams::debug: zero unless built with ZR_TILE_DEBUG.
__device__ __forceinline__ uint32_t tile_debug(const DrawParams& P) { return ZR_TILE_DEBUG ? P.debug : 0u; }

// The draw's parameters read through an opaque pointer to the kernel-argument
// segment (every kernel here takes one DrawParams, at offset 0).  Each call starts
// a fresh reference: fields read after it are loaded there (s_load, scalar cache)
// instead of being hoisted to the kernel entry and held in SGPRs -- or spilled --
// across the whole kernel.  Used at phase boundaries of the large kernels.
typedef const __attribute__((address_space(4))) DrawParams* KernargParams;
__device__ __forceinline__ const DrawParams& kernarg_params() {
    KernargParams kp = (KernargParams)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return *(const DrawParams*)kp;
}

// ------------------------------------------------------------------ helpers

// Regions of the draw's overflow pool (k_setup_bin pool_commit fills them, k_tile's
// status report sums them).
__device__ __forceinline__ uint32_t pool_subs(const DrawParams& P) { return min(kPoolSubs, max(P.setup_wgs, 1u)); }

__device__ __forceinline__ bool fetch_index(const DrawParams& P, uint64_t e, int64_t& v) {
    if (P.index_size == 0) {
        v = (int64_t)e;
        return true;
    }
    if ((e + 1) * P.index_size > P.ib_bytes) return false;
    const uint32_t ix = P.index_size == 2 ? (uint32_t)((const uint16_t*)P.ib)[e] : ((const uint32_t*)P.ib)[e];
    v = (int64_t)ix + (int64_t)P.vertex_offset;
    return true;
}

// Vertex ids of a primitive that k_setup_bin already validated (it won a pixel, so
// its indices were in range): no bounds checks, 32-bit arithmetic (a valid id fits).
// Triangle (within its instance) of draw primitive `gid` (instance-major order).
__device__ __forceinline__ uint32_t tri_of(const DrawParams& P, uint32_t gid) {
    return (P.tris_per_instance == P.draw_prims) ? gid : gid % P.tris_per_instance;
}

__device__ __forceinline__ void winner_vids(const DrawParams& P, uint32_t prim, uint32_t v[3]) {
    const uint32_t tri = tri_of(P, prim);
    const uint32_t e0 = P.first + tri * 3u;
    if (P.index_size == 4) {
        const uint3 ix = *reinterpret_cast<const uint3*>(P.ib + (uint64_t)e0 * 4);
        v[0] = ix.x; v[1] = ix.y; v[2] = ix.z;
    } else if (P.index_size == 2) {
        const uint16_t* ib = reinterpret_cast<const uint16_t*>(P.ib) + e0;
        v[0] = ib[0]; v[1] = ib[1]; v[2] = ib[2];
    } else {
        v[0] = e0; v[1] = e0 + 1u; v[2] = e0 + 2u;
        return;
    }
    const uint32_t off = (uint32_t)P.vertex_offset;  // two's complement: id + offset wraps to the valid id
    v[0] += off; v[1] += off; v[2] += off;
}

__device__ __forceinline__ const float* attr_ptr(const DrawParams& P, uint32_t vid, uint32_t loc) {
    return (const float*)(P.vb + (uint64_t)vid * P.stride + P.attr_offset[loc]);
}

__device__ __forceinline__ bool depth_pass(int op, float z, float d) {
    switch (op) {
    case 0: return false;
    case 1: return z < d;
    case 2: return z == d;
    case 3: return z <= d;
    case 4: return z > d;
    case 5: return z != d;
    case 6: return z >= d;
    default: return true;
    }
}

template <int MODE>
__device__ __forceinline__ unsigned long long init_key(float d) {
    const unsigned long long zb = __float_as_uint(d);
    const unsigned long long nz = (unsigned long long)(~__float_as_uint(d));
    switch (MODE) {
    case kDepthMinStrict: return zb << 32;
    case kDepthMinNonStrict: return (zb << 32) | 0xFFFFFFFFull;
    case kDepthMaxStrict: return nz << 32;
    case kDepthMaxNonStrict: return (nz << 32) | 0xFFFFFFFFull;
    default: return ~0ull;
    }
}

template <int MODE>
__device__ __forceinline__ unsigned long long frag_key(float z, uint32_t seq) {
    const unsigned long long zb = __float_as_uint(z);
    const unsigned long long nz = (unsigned long long)(~__float_as_uint(z));
    switch (MODE) {
    case kDepthMinStrict: return (zb << 32) | seq;
    case kDepthMinNonStrict: return (zb << 32) | (uint32_t)~seq;
    case kDepthMaxStrict: return (nz << 32) | seq;
    case kDepthMaxNonStrict: return (nz << 32) | (uint32_t)~seq;
    default: return (unsigned long long)(uint32_t)~seq;
    }
}

// 0 = no fragment of this draw won the pixel.
template <int MODE>
__device__ __forceinline__ uint32_t winner_seq(unsigned long long key) {
    const uint32_t lo = (uint32_t)key;
    switch (MODE) {
    case kDepthMinStrict:
    case kDepthMaxStrict: return lo;
    case kDepthMinNonStrict:
    case kDepthMaxNonStrict: return (uint32_t)~lo;
    default: return key == ~0ull ? 0u : (uint32_t)~lo;
    }
}

template <int MODE>
__device__ __forceinline__ float key_depth(unsigned long long key) {
    const uint32_t hi = (uint32_t)(key >> 32);
    return (MODE == kDepthMaxStrict || MODE == kDepthMaxNonStrict) ? __uint_as_float(~hi) : __uint_as_float(hi);
}

struct EdgeEval {
    long long w0, w1, w2;
};

__device__ __forceinline__ EdgeEval eval_edges(const TriRecord& r, int px, int py) {
    const int Sx = px * 256 + 128, Sy = py * 256 + 128;
    EdgeEval e;
    e.w0 = (long long)(r.X2 - r.X1) * (Sy - r.Y1) - (long long)(r.Y2 - r.Y1) * (Sx - r.X1);
    e.w1 = (long long)(r.X0 - r.X2) * (Sy - r.Y2) - (long long)(r.Y0 - r.Y2) * (Sx - r.X2);
    e.w2 = (long long)(r.X1 - r.X0) * (Sy - r.Y0) - (long long)(r.Y1 - r.Y0) * (Sx - r.X0);
    return e;
}

// Depth: a plane in the biased edge values w_i' = w_i - bias_i,
// z = fmaf(w2', C2, fmaf(w1', C1, Z0)) with C_i = dz_i * invA2 and Z0 = the plane
// at w' = 0, fmaf(bias2, C2, fmaf(bias1, C1, z0)).  The lane walk steps the
// biased values, so a sample costs two conversions and two FMAs.  Never -0 (z0
// is canonical +0 and a sum of nonzero terms that cancels rounds to +0).
struct DepthPlane {
    float C1, C2, Z0;
};
__device__ __forceinline__ DepthPlane depth_plane(float z0, float dz1, float dz2, float invA2, int b1, int b2) {
    DepthPlane d;
    d.C1 = dz1 * invA2;
    d.C2 = dz2 * invA2;
    d.Z0 = fmaf((float)b2, d.C2, fmaf((float)b1, d.C1, z0));
    return d;
}
__device__ __forceinline__ float plane_z(const DepthPlane& d, float w1b, float w2b) {
    return fmaf(w2b, d.C2, fmaf(w1b, d.C1, d.Z0));
}
// The top-left bias of the edge from vertex a to vertex b (y-down: an edge is
// top-left iff dy < 0 || (dy == 0 && dx > 0)); edge i is opposite vertex i.
__device__ __forceinline__ int edge_bias(int dx, int dy) { return ((dy < 0) || (dy == 0 && dx > 0)) ? 0 : 1; }

// The contract depth of record r at pixel (px, py) (last-wins resolve: no key
// carries it), from the record's vertices alone.
__device__ __forceinline__ float winner_depth(const TriRecord& r, int px, int py) {
    const EdgeEval e = eval_edges(r, px, py);
    const int b1 = edge_bias(r.X0 - r.X2, r.Y0 - r.Y2), b2 = edge_bias(r.X1 - r.X0, r.Y1 - r.Y0);
    const DepthPlane d = depth_plane(r.z0, r.dz1, r.dz2, r.invA2, b1, b2);
    return plane_z(d, (float)(e.w1 - b1), (float)(e.w2 - b2));
}

// Edge values at a pixel centre as floats (resolve: the winner's barycentrics).
// A small primitive's values fit int32 exactly (bbox <= 64 px a side),
// so (float)int32 equals (float)int64 there and the 64-bit products are skipped.
struct EdgeEvalF {
    float f0, f1, f2;
};

__device__ __forceinline__ EdgeEvalF eval_edges_f(const TriRecord& r, int px, int py) {
    const int Sx = px * 256 + 128, Sy = py * 256 + 128;
    EdgeEvalF e;
    if (r.flags & kFlagSmall) {
        // unsigned products: defined wraparound for the (discarded) fallback primitive
        // of pixels no fragment won, which may lie far outside its bbox
        auto ew = [](int ax, int ay, int bx, int by) {
            return (float)(int)((uint32_t)ax * (uint32_t)ay - (uint32_t)bx * (uint32_t)by);
        };
        e.f0 = ew(r.X2 - r.X1, Sy - r.Y1, r.Y2 - r.Y1, Sx - r.X1);
        e.f1 = ew(r.X0 - r.X2, Sy - r.Y2, r.Y0 - r.Y2, Sx - r.X2);
        e.f2 = ew(r.X1 - r.X0, Sy - r.Y0, r.Y1 - r.Y0, Sx - r.X0);
    } else {
        const EdgeEval w = eval_edges(r, px, py);
        e.f0 = (float)w.w0;
        e.f1 = (float)w.w1;
        e.f2 = (float)w.w2;
    }
    return e;
}

}  // namespace zr
