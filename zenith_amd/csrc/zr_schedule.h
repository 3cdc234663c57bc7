// zr_schedule.h — the tile schedule and the tile jobs, built by k_setup_bin's last workgroup for k_tile.
// Part of the zr_kernels.hip translation unit (included there, in order, and
// nowhere else): it relies on the build knobs and constants defined above its
// include.
#pragma once
#include "zr_dev_common.h"
#include "zr_order.h"

namespace zr {

// Tile schedule (longest-processing-time first): built by the last k_setup_bin
// workgroup past phase 2, when every tile's count is final.  Each tile keeps the
// XCD xcd_tile gives it (block % 8), but within an XCD the blocks take its tiles
// heaviest list first, so the hardware, which dispatches blocks in order as slots
// free up, starts the long tiles first and ends the pass on short ones (the
// pass has ~2 tiles per wave slot at C2; without it its last ~15 us ran at 0.77
// occupancy, docs/EXPERIMENTS.md).  Counting sort over kSchedBuckets weight
// classes per XCD (s_sched: 8 x kSchedBuckets words of LDS).
__device__ void build_tile_schedule(const DrawParams& P, uint32_t nt, uint32_t* s_sched, uint32_t* order) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 8u * kSchedBuckets; i += kSetupThreads) s_sched[i] = 0u;
    const uint32_t top = __hip_atomic_fetch_max(&P.counters[kCtMaxTile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t shift = top >= kSchedBuckets ? 32u - __clz(top / kSchedBuckets) : 0u;  // top >> shift < 64
    __syncthreads();
    auto key = [&](uint32_t t, uint32_t& x) {  // XCD and descending-weight bucket of tile t
        const uint32_t c = __hip_atomic_fetch_add(&P.tile_counts[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~kCountRuns;
        x = xcd_block(t, nt) & 7u;
        return kSchedBuckets - 1u - min(c >> shift, kSchedBuckets - 1u);
    };
    for (uint32_t t = tid; t < nt; t += kSetupThreads) {
        uint32_t x;
        const uint32_t k = key(t, x);
        atomicAdd(&s_sched[x * kSchedBuckets + k], 1u);
    }
    __syncthreads();
    if (tid < 8u * 64u) {  // one wave per XCD: exclusive scan of its 64 buckets
        static_assert(kSchedBuckets == 64, "one lane per bucket");
        const uint32_t c = s_sched[tid];
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d, 64);
            if ((int)(tid & 63u) >= d) inc += y;
        }
        s_sched[tid] = inc - c;
    }
    __syncthreads();
    for (uint32_t t = tid; t < nt; t += kSetupThreads) {
        uint32_t x;
        const uint32_t k = key(t, x);
        const uint32_t l = atomicAdd(&s_sched[x * kSchedBuckets + k], 1u);  // rank of t within its XCD
        order[l * 8u + x] = t;  // block l * 8 + x runs on XCD x (a bijection on [0, nt))
    }
}

// Tile jobs (DrawParams::job_entries), built by the same last workgroup.  A
// tile whose list is longer than J (and takes no record scan) becomes
// K = ceil(count / J) jobs, part p covering list entries [p J, (p + 1) J), with
// K key buffers from job_slot[t].  Part 0 keeps the tile's block in the usual
// order (blocks [job_pad, job_pad + nt)); parts 1.. take blocks of [0, job_pad)
// spread like their tile (block b % 8 = the tile's XCD in that order, for L2
// locality only); the blocks of [0, job_pad) left over get kJobNone.  (Every
// part among the first blocks, part 0 included, measured slower on c2x: 167.7 ->
// 172.0 us per frame, docs/EXPERIMENTS.md round 6.)  When the
// parts do not fit (an XCD's share of job_pad, or the key buffers) no tile is
// split and the draw is counted (kCtJobsDenied) for the runtime to size them up.  k_tile derives K from the
// same count and run word.

__device__ __noinline__ void build_job_schedule(const DrawParams& P, uint32_t nt, uint32_t* s_buf) {
    const uint32_t tid = threadIdx.x, J = P.job_entries, per_xcd = P.job_pad / 8u;
    uint32_t* s_cnt = s_buf;       // [8] parts per XCD, then their cursors
    uint32_t* s_tot = s_buf + 8;   // [0] key buffers (jobs of split tiles), [1] buffer cursor, [2] denied, [3] split tiles
    if (tid < 16u) s_buf[tid] = 0u;
    __syncthreads();
    // pass 1: every tile's job count, kept in this thread's registers for pass 2
    // (tiles tid + k * kSetupThreads), and the parts each XCD gets; loads in
    // batches of kB in flight together (one tile at a time, and the counts parked
    // in job_slot and read back, kept this last workgroup ~11 us at 8160 tiles;
    // all 16 at once took 120 VGPRs, which every k_setup_bin instance reserves)
    constexpr uint32_t kPer = kMaxTilesPerPass / kSetupThreads, kB = 4;
    uint32_t K[kPer];
#pragma unroll
    for (uint32_t k0 = 0; k0 < kPer; k0 += kB) {
        uint32_t c[kB], rw[kB];
        if (tid + k0 * kSetupThreads >= nt) {
#pragma unroll
            for (uint32_t k = 0; k < kB; ++k) K[k0 + k] = 1u;
            continue;
        }
#pragma unroll
        for (uint32_t k = 0; k < kB; ++k) {
            const uint32_t t = tid + (k0 + k) * kSetupThreads;
            c[k] = t < nt ? __hip_atomic_load(&P.tile_counts[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kB; ++k) {
            const uint32_t t = tid + (k0 + k) * kSetupThreads;
            rw[k] = (c[k] & kCountRuns) ? __hip_atomic_load(&P.run_counts[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kB; ++k) {
            const uint32_t t = tid + (k0 + k) * kSetupThreads;
            K[k0 + k] = t < nt ? tile_jobs(c[k] & ~kCountRuns, rw[k], J) : 1u;
            if (K[k0 + k] > 1u) {
                atomicAdd(&s_cnt[xcd_block(t, nt) & 7u], K[k0 + k] - 1u);
                atomicAdd(&s_tot[0], K[k0 + k]);
                atomicAdd(&s_tot[3], 1u);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        bool ok = s_tot[0] <= P.job_slots;
        uint32_t xmax = 0;
        for (uint32_t x = 0; x < 8u; ++x) {
            ok = ok && s_cnt[x] <= per_xcd;
            xmax = max(xmax, s_cnt[x]);
        }
        // what the split needs, fitting or not (the runtime sizes the shape's next
        // draws from it: key buffers and spare blocks per XCD)
        P.counters[kCtJobBufs] = s_tot[0];
        P.counters[kCtJobXcdMax] = xmax;
        s_tot[2] = ok ? 0u : 1u;
        P.draw_info[kInfoJobEntries] = ok ? J : 0u;
        if (!ok) atomicAdd(&P.counters[kCtJobsDenied], 1u);
    }
    __syncthreads();
    const bool ok = s_tot[2] == 0u;
    if (tid < 8u) {
        s_cnt[16 + tid] = ok ? s_cnt[tid] : 0u;  // (parts per XCD; s_cnt[0, 8) become the cursors)
        s_cnt[tid] = 0u;
    }
    if (tid == 0 && ok && s_tot[0]) atomicAdd(&P.counters[kCtJobs], s_tot[0] - s_tot[3]);  // (jobs beyond one per tile)
    __syncthreads();
    // pass 2: key slots (k_tile reads job_slot[t] of split tiles only) and part items
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t t = tid + k * kSetupThreads;
        if (!ok || K[k] <= 1u) continue;
        const uint32_t x = xcd_block(t, nt) & 7u;
        P.job_slot[t] = atomicAdd(&s_tot[1], K[k]);  // (K key buffers, one per job)
        const uint32_t l0 = atomicAdd(&s_cnt[x], K[k] - 1u);
        for (uint32_t p = 1; p < K[k]; ++p) P.tile_order[(l0 + p - 1u) * 8u + x] = job_item(t, p);
    }
    for (uint32_t i = tid; i < P.job_pad; i += kSetupThreads)  // the spare part blocks
        if ((i >> 3) >= s_cnt[16 + (i & 7u)]) P.tile_order[i] = kJobNone;
    __syncthreads();  // (s_buf is build_tile_schedule's next)
}

}  // namespace zr
