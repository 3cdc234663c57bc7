// zr_runtime.cpp — host side of libzenith_raster: the device, draw execution and
// submission of the C ABI in include/zenith_raster.h.
//
// Objects mirror zenith-rhi's (RenderDevice, Buffer, Texture, Shader, pipeline,
// CommandEncoder, Fence); command buffers record like vkCmd* (zr_cmd.cpp) and are
// executed at zr_submit by walking the recorded state machine and launching the
// HIP passes of zr_kernels.hip on the device's streams.  What a draw
// launches and how its scratch is sized is planned in zr_plan.cpp; this file binds
// pointers, allocates and enqueues.  No CPU fallback: every draw runs the HIP
// kernels or returns an error.
#include "zr_runtime.h"
#include "zr_shading.h"

using namespace zr;

namespace {
thread_local std::string g_last_error = "";
}

zr_result zr::fail(zr_result code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

zr_result zr::set_device(zr_device* d) {
    ZR_HIP(hipSetDevice(d->hip_device));
    return ZR_SUCCESS;
}

// ------------------------------------------------------------ device helpers

namespace {

hipEvent_t take_event(zr_device* d) {
    if (!d->event_pool.empty()) {
        hipEvent_t e = d->event_pool.back();
        d->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void collect_timings(zr_device* d) {
    for (auto& t : d->timed) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
            auto& slot = d->times[t.name];
            slot.first += ms;
            slot.second += 1;
        }
        d->event_pool.push_back(t.start);
        d->event_pool.push_back(t.stop);
    }
    d->timed.clear();
}

template <typename F>
void timed_launch(zr_device* d, const char* name, hipStream_t stream, F&& fn) {
    if (!d->profiling) {
        fn();
        return;
    }
    TimedLaunch t{name, take_event(d), take_event(d)};
    (void)hipEventRecord(t.start, stream);
    fn();
    (void)hipEventRecord(t.stop, stream);
    d->timed.push_back(t);
}

// Both streams idle (scratch may be freed, host-visible status is final).
zr_result sync_streams(zr_device* d) {
    ZR_HIP(hipStreamSynchronize(d->route_stream));
    ZR_HIP(hipStreamSynchronize(d->setup_stream));
    ZR_HIP(hipStreamSynchronize(d->stream));
    if (d->gather_stream) ZR_HIP(hipStreamSynchronize(d->gather_stream));
    return ZR_SUCCESS;
}

// Grows `b` to `need` elements of `elem_bytes` (never shrinks; the old contents are dropped).
zr_result grow(zr_device* d, ScratchBuf& b, uint64_t need, uint64_t elem_bytes) {
    if (need <= b.cap && b.ptr) return ZR_SUCCESS;
    if (d->capturing) return ZR_NOT_READY;  // graph capture aborted: the caller runs eagerly
    d->scratch_gen++;
    zr_result rc = sync_streams(d);
    if (rc) return rc;
    if (b.ptr) (void)hipFree(b.ptr);
    b.ptr = nullptr;
    const uint64_t n = std::max<uint64_t>(need, 1024);
    ZR_HIP(hipMalloc(&b.ptr, n * elem_bytes));
    b.cap = n;
    return ZR_SUCCESS;
}

zr_result execute(zr_device* d, zr_cmd* cmd);

// Events that only order this device's streams around data this device's own
// kernels write and read (setup_done, tile_done), never waited on by the host:
// device-scope release, no system-scope cache writeback when they are recorded.
// (Host waits go through hipStreamSynchronize or a fence's own event.)  The row
// gather's events keep the system-scope fence: RCCL moves the rows between devices.
#ifndef ZR_EVENT_SYSTEM_FENCE
constexpr unsigned kStreamEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;
#else
constexpr unsigned kStreamEventFlags = hipEventDisableTiming;
#endif

// kDebugStamps: per-phase durations of k_setup_bin across workgroups (us, 100 MHz clock).
void dump_stamps(zr_device* d) {
    std::vector<unsigned long long> ts(d->dbg_wgs * 8);
    if (hipMemcpy(ts.data(), d->dbg_ts, ts.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    FILE* f = fopen(d->knobs.dbg_ts_path.c_str(), "a");
    if (!f) return;
    unsigned long long t0 = ~0ull;
    for (uint32_t w = 0; w < d->dbg_wgs; ++w) t0 = std::min(t0, ts[w * 8]);
    fprintf(f, "wgs=%u", d->dbg_wgs);
    for (int i = 0; i <= 6; ++i) {
        double mn = 1e30, mx = 0, sum = 0;
        for (uint32_t w = 0; w < d->dbg_wgs; ++w) {
            const double v = (double)(ts[w * 8 + i] - t0) * 0.01;
            mn = std::min(mn, v); mx = std::max(mx, v); sum += v;
        }
        fprintf(f, " s%d[min %.1f avg %.1f max %.1f]", i, mn, sum / d->dbg_wgs, mx);
    }
    // phase-1 duration per workgroup, by blockIdx % 8 (a label for workgroups that share an XCD)
    double xs[8] = {0}, xn[8] = {0};
    fprintf(f, "\n  p1 by w%%8:");
    for (uint32_t w = 0; w < d->dbg_wgs; ++w) {
        xs[w % 8] += (double)(ts[w * 8 + 1] - ts[w * 8]) * 0.01;
        xn[w % 8] += 1;
    }
    for (int x = 0; x < 8; ++x) fprintf(f, " %.1f", xn[x] ? xs[x] / xn[x] : 0.0);
    {
        std::vector<unsigned long long> tt(d->dbg_tiles * 8);
        if (d->dbg_tiles && hipMemcpy(tt.data(), d->dbg_ts + 8192 * 8, tt.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            unsigned long long t1 = ~0ull;
            for (uint32_t w = 0; w < d->dbg_tiles; ++w) t1 = std::min(t1, tt[w * 8]);
            fprintf(f, "\n  tile(us from first tile start; dur = per-tile phase length):");
            // t0 start, t1 init, t2 first segment sorted, t3 raster done, t5 resolve
            // winners known, t6 first batch fetched, t4 resolve done
            for (int i : {0, 1, 2, 3, 5, 6, 4}) {
                double mn = 1e30, mx = 0, sum = 0, dsum = 0, dmx = 0;
                for (uint32_t w = 0; w < d->dbg_tiles; ++w) {
                    const double v = (double)(tt[w * 8 + i] - t1) * 0.01;
                    mn = std::min(mn, v); mx = std::max(mx, v); sum += v;
                    const int prev = i == 5 ? 3 : i == 6 ? 5 : i == 4 ? 6 : i - 1;
                    if (i) { const double dd = (double)(tt[w * 8 + i] - tt[w * 8 + prev]) * 0.01; dsum += dd; dmx = std::max(dmx, dd); }
                }
                fprintf(f, " t%d[min %.1f avg %.1f max %.1f dur avg %.1f max %.1f]", i, mn, sum / d->dbg_tiles, mx,
                        dsum / d->dbg_tiles, dmx);
            }
        }
    }
    {  // raw per-tile stamps for offline analysis: <path>.tiles.csv
        std::vector<unsigned long long> tt(d->dbg_tiles * 8);
        if (d->dbg_tiles && hipMemcpy(tt.data(), d->dbg_ts + 8192 * 8, tt.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            FILE* g = fopen((d->knobs.dbg_ts_path + ".tiles.csv").c_str(), "a");
            if (g) {
                unsigned long long t1 = ~0ull;
                for (uint32_t w = 0; w < d->dbg_tiles; ++w) t1 = std::min(t1, tt[w * 8]);
                fprintf(g, "tile,t0,t1,t2,t3,t4,t5,nbig,count,lane_steps,wave_sweeps\n");
                for (uint32_t w = 0; w < d->dbg_tiles; ++w) {
                    fprintf(g, "%u", w);
                    for (int i = 0; i <= 4; ++i) fprintf(g, ",%.2f", (double)(tt[w * 8 + i] - t1) * 0.01);
                    // 512-thread tiles: t5 = the first segment's chunks done, nbig = its
                    // wave-path queue (256: resolve_tile's own stamps, in t5 / the count word)
                    fprintf(g, ",%.2f,%llu,%llu,%llu,%llu\n", (double)(tt[w * 8 + 5] - t1) * 0.01, tt[w * 8 + 6] >> 32,
                            tt[w * 8 + 6] & 0xFFFFFFFFull, tt[w * 8 + 7] & 0xFFFFFFFFull, tt[w * 8 + 7] >> 32);
                }
                fclose(g);
            }
        }
    }
    fprintf(f, "\n  p1 first 16 wgs:");
    for (uint32_t w = 0; w < std::min(16u, d->dbg_wgs); ++w) fprintf(f, " %.1f", (double)(ts[w * 8 + 1] - ts[w * 8]) * 0.01);
    fprintf(f, "\n  p1 last 16 wgs:");
    for (uint32_t w = d->dbg_wgs > 16 ? d->dbg_wgs - 16 : 0; w < d->dbg_wgs; ++w)
        fprintf(f, " %.1f", (double)(ts[w * 8 + 1] - ts[w * 8]) * 0.01);
    fprintf(f, "\n");
    fclose(f);
}

}  // namespace

zr_result zr::device_sync(zr_device* d) {
    zr_result rc = set_device(d);
    if (rc) return rc;
    if ((rc = sync_streams(d))) return rc;
    collect_timings(d);
    volatile uint32_t* st = d->status_host;
    d->last.bin_pairs = st[kStTotalPairs];
    d->last.triangles_setup = st[kStTrianglesSetup];
    d->last.triangles_dropped_clip = st[kStDroppedClip];
    d->last.micro_fragments = st[kStMicro];
    d->last.bin_pool_pairs = st[kStPoolPairs];
    d->last.bin_pool_runs = st[kStPoolRuns];
    d->last.tile_jobs = st[kStJobs];
    st[kStJobsDenied] = 0;  // (a denied split is sized from its shape's kStJobBufSlot0: ShapeBook::end_interval)
    // partitioned draws since the previous sync point
    if (st[kStRouteMax]) {  // kept from the last interval with partitioned draws
        d->last.route_max_entries = st[kStRouteMax];
        st[kStRouteMax] = 0;
    }
    d->route_fallbacks += st[kStRouteFallback];
    d->last.route_fallback_draws = d->route_fallbacks;
    st[kStRouteFallback] = 0;
    d->pending.clear();
    if (d->dbg_ts && !d->knobs.dbg_ts_path.empty()) dump_stamps(d);
    // the shape table takes the interval's measurements and says which buffers to resize
    uint64_t bins_cap[kScratchSets], job_keys_cap[kScratchSets];
    for (uint32_t i = 0; i < kScratchSets; ++i) {
        bins_cap[i] = d->sets[i].bins.ptr ? d->sets[i].bins.cap : 0;
        job_keys_cap[i] = d->sets[i].job_keys.ptr ? d->sets[i].job_keys.cap : 0;
    }
    const SyncDecision dec = d->book.end_interval(st, bins_cap, job_keys_cap, d->knobs);
    d->scratch_gen += dec.gen_bumps;
    if (st[kStOverflow]) {
        d->overflowed_draws += st[kStOverflow];
        st[kStOverflow] = 0;
    }
    for (uint32_t i = 0; i < kScratchSets; ++i) {
        ScratchBuf& bins = d->sets[i].bins;
        if (!dec.bins_realloc[i]) continue;
        ZR_HIP(hipFree(bins.ptr));
        bins.ptr = nullptr;
        ZR_HIP(hipMalloc(&bins.ptr, dec.bins_realloc[i] * 4));
        bins.cap = dec.bins_realloc[i];
    }
    for (uint32_t i = 0; i < kScratchSets; ++i) {
        ScratchSet& S = d->sets[i];
        if (!dec.drop_job_keys[i]) continue;
        (void)hipFree(S.job_keys.ptr);
        (void)hipFree(S.job_tickets.ptr);
        S.job_keys = ScratchBuf{};
        S.job_tickets = ScratchBuf{};
    }
    d->last.tile_size = d->last_tile;
    d->last.job_key_bytes = 0;
    for (const ScratchSet& S : d->sets) d->last.job_key_bytes += S.job_keys.ptr ? S.job_keys.cap * 8 : 0;
    d->last.overflowed_draws = d->overflowed_draws;
    d->last.bin_capacity = d->sets[0].bins.cap;
    for (const ScratchSet& S : d->sets)
        if (S.bins.ptr) d->last.bin_capacity = std::min<uint64_t>(d->last.bin_capacity, S.bins.cap);
    if (d->census_words) {  // distinct primitives that won a pixel in the last census draw
        std::vector<uint32_t> bits(d->census_words);
        ZR_HIP(hipMemcpy(bits.data(), d->win_bits.ptr, bits.size() * 4, hipMemcpyDeviceToHost));
        uint64_t n = 0;
        for (uint32_t w : bits) n += (uint64_t)__builtin_popcount(w);
        d->last.winners = n;
        d->census_words = 0;
    }
    return ZR_SUCCESS;
}

// ------------------------------------------------------------ draw execution

namespace {

struct VertexBinding {
    const zr_buffer* buf = nullptr;
    uint64_t offset = 0;
};

struct ExecState {
    const zr_pipeline* pipe = nullptr;
    bool vp_set = false, sc_set = false;
    zr_viewport vp{};
    zr_rect2d sc{};
    VertexBinding vb[8];
    const zr_buffer* ib = nullptr;
    uint64_t ib_offset = 0;
    int32_t index_type = 0;
    std::map<std::pair<uint32_t, uint32_t>, std::pair<const zr_buffer*, uint64_t>> ubos;
    bool rendering = false;
    RenderingState rs;
    bool color_clear_pending = false, depth_clear_pending = false;
    uint32_t shard_rank = 0, shard_count = 1;
    zr_exchange_fn exchange = nullptr;
    void* exchange_user = nullptr;
    uint32_t route_cap = 0;  // entries per exchange block (zr_cmd_set_route_capacity; 0: route_capacity_default)
    // push-constant state (vkCmdPushConstants): bytes, which 4-byte words were
    // written, and the layout they were written with
    float push[kMaxPushWords] = {};
    uint32_t push_written = 0;
    const zr_pipeline* push_layout = nullptr;
};

zr_result fill_target(const ExecState& s, DrawParams& P) {
    const zr_texture* ct = s.rs.has_color ? s.rs.color.texture : nullptr;
    const zr_texture* dt = s.rs.has_depth ? s.rs.depth.texture : nullptr;
    if (!ct && !dt) return fail(ZR_ERROR_VALIDATION_FAILED, "render pass without attachments");
    const zr_texture* ref = ct ? ct : dt;
    if (ct && dt && (ct->width != dt->width || ct->height != dt->height))
        return fail(ZR_ERROR_VALIDATION_FAILED, "colour and depth attachment extents differ");
    if (dt && dt->format != ZR_FORMAT_D32_SFLOAT) return fail(ZR_ERROR_FORMAT_NOT_SUPPORTED, "depth format");
    if (ct && format_bpp(ct->format) == 0) return fail(ZR_ERROR_FORMAT_NOT_SUPPORTED, "colour format");
    P.fb_w = ref->width;
    P.fb_h = ref->height;
    P.color = ct ? (uint8_t*)ct->ptr : nullptr;
    P.color_format = ct ? ct->format : 0;
    P.color_bpp = ct ? ct->bpp : 0;
    P.depth = dt ? (float*)dt->ptr : nullptr;
    const int32_t ax0 = std::max(0, s.rs.area.x), ay0 = std::max(0, s.rs.area.y);
    const int64_t ax1 = std::min<int64_t>((int64_t)s.rs.area.x + s.rs.area.width, P.fb_w) - 1;
    const int64_t ay1 = std::min<int64_t>((int64_t)s.rs.area.y + s.rs.area.height, P.fb_h) - 1;
    P.ra_x0 = ax0;
    P.ra_y0 = ay0;
    P.ra_x1 = (int32_t)ax1;
    P.ra_y1 = (int32_t)ay1;
    P.shard_rank = s.shard_rank;
    P.shard_count = s.shard_count;
    set_tiles(P, kTileShift);
    // clears (fused into the first draw of the pass, else k_clear at end_rendering)
    P.clear_color_enable = (ct && s.color_clear_pending) ? 1u : 0u;
    if (ct) {
        for (int i = 0; i < 4; ++i) P.clear_color[i] = s.rs.color.clear_value[i];
        P.clear_color_packed = pack_rgba8(P.clear_color, ct->format, kSrgbThresholds);
    }
    P.clear_depth_enable = (dt && s.depth_clear_pending) ? 1u : 0u;
    P.clear_depth = dt ? s.rs.depth.clear_value[0] : 1.0f;
    P.load_depth = (dt && !s.depth_clear_pending) ? 1u : 0u;
    return ZR_SUCCESS;
}

// Allocation only: the set's buffers grown to what ShapeBook::sizes says this draw
// needs, then the draw's pointers and bin geometry into P.
zr_result ensure_scratch(zr_device* d, ScratchSet& S, DrawParams& P, const DrawPlan& plan) {
    const ScratchSizes z = d->book.sizes(P, S.bins.ptr ? S.bins.cap : 0, plan.sched, d->knobs);
    // (zeroed when grown: the kernels leave these zero after every draw)
    const struct {
        ScratchBuf& buf;
        uint64_t need, elem_bytes;
        bool zero;
    } rows[] = {
        {S.records, z.records, sizeof(TriCompact), false},
        {S.records_big, z.records, sizeof(TriRecord), false},
        {S.bboxes, z.records, sizeof(BBox), false},
        {S.mesh_edges, z.mesh_edges, sizeof(float4), false},
        {S.tile_counts, z.tiles, 4, true},
        {S.draw_info, kInfoWords, 4, false},
        {S.counters, kCtWords, 4, true},
        {S.run_counts, z.tiles, 4, true},
        {S.runs, z.runs, sizeof(uint2), true},  // (run tables start empty: length 0)
        {S.bins, z.bins, 4, false},
        {S.job_slot, z.job_slot, 4, false},
        {S.job_keys, z.job_keys, 8, false},
        {S.job_tickets, z.job_tickets, 4, true},
        {S.tile_order, z.tile_order, 4, false},
    };
    for (const auto& r : rows) {
        if (!r.need || (r.buf.ptr && r.need <= r.buf.cap)) continue;  // (0: not used by this draw)
        const zr_result rc = grow(d, r.buf, r.need, r.elem_bytes);
        if (rc) return rc;
        if (r.zero) ZR_HIP(hipMemset(r.buf.ptr, 0, r.buf.cap * r.elem_bytes));
    }
    if (!S.setup_done) {
        ZR_HIP(hipEventCreateWithFlags(&S.setup_done, kStreamEventFlags));
        ZR_HIP(hipEventCreateWithFlags(&S.tile_done, kStreamEventFlags));
        ZR_HIP(hipEventCreateWithFlags(&S.route_done, kStreamEventFlags));
    }
    P.records = (TriCompact*)S.records.ptr;
    P.records_big = (TriRecord*)S.records_big.ptr;
    P.mesh_edges = (float4*)S.mesh_edges.ptr;
    P.bboxes = (BBox*)S.bboxes.ptr;
    P.tile_counts = (uint32_t*)S.tile_counts.ptr;
    P.draw_info = (uint32_t*)S.draw_info.ptr;
    P.counters = (uint32_t*)S.counters.ptr;
    P.bins = (uint32_t*)S.bins.ptr;
    P.runs = (uint2*)S.runs.ptr;
    P.run_counts = (uint32_t*)S.run_counts.ptr;
    P.slab = z.slab;
    P.pool_off = z.pool_off;
    P.pool_cap = z.pool_cap;
    P.job_entries = z.job_entries;
    P.job_pad = z.job_pad;
    P.job_slots = z.job_slots;
    if (z.job_entries) {
        P.job_slot = (uint32_t*)S.job_slot.ptr;
        P.job_keys = (unsigned long long*)S.job_keys.ptr;
        P.job_tickets = (uint32_t*)S.job_tickets.ptr;
    }
    if (z.tile_order) P.tile_order = (uint32_t*)S.tile_order.ptr;
    P.stat_slot = d->book.take_slot(P, d->capturing);
    P.status = d->status_dev;
    return ZR_SUCCESS;
}

zr_result validate_draw_state(const zr_device* d, const ExecState& s, bool indexed) {
    if (!s.rendering) return fail(ZR_ERROR_VALIDATION_FAILED, "draw outside begin_rendering/end_rendering");
    // the runtime's own all-to-all sends one block to every communicator rank and
    // takes bit d of a route mask for comm rank d: the shard must be that communicator
    if (s.exchange == &rccl_exchange &&
        (s.exchange_user != (void*)d || !d->comm_x || d->comm_size != (int)s.shard_count ||
         d->comm_rank != (int)s.shard_rank))
        return fail(ZR_ERROR_VALIDATION_FAILED,
                    "tile shard (rank, count) differs from the device's RCCL communicator (zr_device_init_rccl)");
    const zr_pipeline* pp = s.pipe;
    if (!pp) return fail(ZR_ERROR_VALIDATION_FAILED, "draw without a bound pipeline");
    if (!s.vp_set || !s.sc_set)
        return fail(ZR_ERROR_VALIDATION_FAILED, "dynamic viewport/scissor not set (pipeline.rs:734)");
    if (pp->color_count != (s.rs.has_color ? 1u : 0u))
        return fail(ZR_ERROR_VALIDATION_FAILED, "node colour targets do not match pipeline colour attachments");
    if (!s.vb[0].buf) return fail(ZR_ERROR_VALIDATION_FAILED, "vertex buffer binding 0 not bound");
    if (indexed && !s.ib) return fail(ZR_ERROR_VALIDATION_FAILED, "draw_indexed without an index buffer");
    return ZR_SUCCESS;
}

// The draw's inputs into P: vertex and index buffers, viewport and scissor, the
// pipeline's fixed state, uniforms and push constants (with their checks).
zr_result bind_inputs(const ExecState& s, const Cmd& c, bool indexed, DrawParams& P) {
    const zr_pipeline* pp = s.pipe;
    const bool mesh = pp->program == kProgMesh;
    if (!pp->has_fs) {
        P.color = nullptr;
        P.color_bpp = 0;
    }
    const zr_buffer* vb = s.vb[0].buf;
    P.vb = (const uint8_t*)vb->ptr + s.vb[0].offset;
    P.vb_bytes = vb->size > s.vb[0].offset ? vb->size - s.vb[0].offset : 0;
    P.stride = pp->stride;
    P.nattr = pp->nattr;
    for (int i = 0; i < 4; ++i) {
        P.attr_offset[i] = pp->attr_offset[i];
        P.attr_size[i] = pp->attr_size[i];
    }
    {  // one compare per vertex in the kernels instead of one per (vertex, attribute)
        uint64_t end = 0;
        for (uint32_t a = 0; a < P.nattr; ++a) end = std::max<uint64_t>(end, (uint64_t)P.attr_offset[a] + P.attr_size[a]);
        P.vid_count = P.nattr == 0 ? (1ull << 32) : (P.vb_bytes < end ? 0ull : (P.vb_bytes - end) / P.stride + 1ull);
    }
    if (indexed) {
        P.ib = (const uint8_t*)s.ib->ptr + s.ib_offset;
        P.ib_bytes = s.ib->size > s.ib_offset ? s.ib->size - s.ib_offset : 0;
        P.index_size = s.index_type == ZR_INDEX_TYPE_UINT16 ? 2u : 4u;
        P.first = c.c;
        P.vertex_offset = c.e;
        const uint64_t nidx = P.ib_bytes / 4;  // only read for u32 indices (k_setup_bin fetch_indices_gid)
        P.ib_tris = nidx > P.first ? (uint32_t)std::min<uint64_t>((nidx - P.first) / 3, 0xFFFFFFFFull) : 0u;
    } else {
        P.ib_tris = 0;
        P.index_size = 0;
        P.first = c.c;
        P.vertex_offset = 0;
    }
    // viewport transform constants (Vulkan 1.3 §Controlling the Viewport)
    P.hw = s.vp.width * 0.5f;
    P.hh = s.vp.height * 0.5f;
    P.cx = s.vp.x + P.hw;
    P.cy = s.vp.y + P.hh;
    P.dr = s.vp.max_depth - s.vp.min_depth;
    P.dmin = s.vp.min_depth;
    P.dlo = std::min(s.vp.min_depth, s.vp.max_depth);
    P.dhi = std::max(s.vp.min_depth, s.vp.max_depth);
    P.clip_x0 = std::max<int32_t>(s.sc.x, P.ra_x0);
    P.clip_y0 = std::max<int32_t>(s.sc.y, P.ra_y0);
    P.clip_x1 = (int32_t)std::min<int64_t>((int64_t)s.sc.x + s.sc.width - 1, P.ra_x1);
    P.clip_y1 = (int32_t)std::min<int64_t>((int64_t)s.sc.y + s.sc.height - 1, P.ra_y1);
    P.cull_mode = pp->cull_mode;
    P.front_face = pp->front_face;
    P.write_mask = pp->color.write_mask;
    // depth
    const bool has_depth = P.depth != nullptr;
    const bool test = has_depth && pp->has_depth_state && pp->ds.depth_test_enable;
    const bool write = test && pp->ds.depth_write_enable;
    const int32_t op = test ? pp->ds.depth_compare_op : 7;
    if (write && op == 5) return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "NOT_EQUAL with depth writes");
    P.depth_mode = choose_depth_mode(test, write, op);
    P.depth_op = op;
    P.depth_write_out = write ? 1u : 0u;
    // shading
    P.program = pp->program;
    P.time_ptr = nullptr;
    for (const auto& b : pp->bindings) {
        auto it = s.ubos.find({b.set, b.binding});
        if (it == s.ubos.end())
            return fail(ZR_ERROR_VALIDATION_FAILED, std::string("descriptor '") + b.name + "' not bound");
        if (pp->program == kProgTriangle && !strcmp(b.name, "Time")) {
            if (it->second.second + 4 > it->second.first->size)
                return fail(ZR_ERROR_VALIDATION_FAILED, "Time uniform range out of bounds");
            P.time_ptr = (const float*)((const uint8_t*)it->second.first->ptr + it->second.second);
        }
        if (pp->program == kProgMesh && !strcmp(b.name, "View")) {
            if (it->second.second + 64 > it->second.first->size || (it->second.second & 3u))
                return fail(ZR_ERROR_VALIDATION_FAILED, "View uniform range out of bounds (float4x4 view_proj)");
            P.view_proj = (const float*)((const uint8_t*)it->second.first->ptr + it->second.second);
        }
    }
    if (pp->view_push) {
        // mesh_push.slang: View.view_proj is push-constant bytes [0, 64)
        if ((s.push_written & 0xFFFFu) != 0xFFFFu)
            return fail(ZR_ERROR_VALIDATION_FAILED, "push constants [0, 64) (View.view_proj) not pushed before the draw");
        if (s.push_layout != pp && (!s.push_layout || s.push_layout->push_ranges.size() != pp->push_ranges.size() ||
                                    !std::equal(pp->push_ranges.begin(), pp->push_ranges.end(),
                                                s.push_layout->push_ranges.begin(),
                                                [](const zr_push_constant_range& a, const zr_push_constant_range& b) {
                                                    return a.stage_flags == b.stage_flags && a.offset == b.offset &&
                                                           a.size == b.size;
                                                })))
            return fail(ZR_ERROR_VALIDATION_FAILED,
                        "push constants were pushed with a layout whose ranges differ from the bound pipeline's");
        memcpy(P.push, s.push, sizeof P.push);
        P.view_push = 1;
        P.view_proj = nullptr;
    }
    if (mesh && !P.view_proj && !P.view_push) return fail(ZR_ERROR_VALIDATION_FAILED, "descriptor 'View' not bound");
    return ZR_SUCCESS;
}

// Partitioned draws: the recorded blocks of a replay exchange are copied into this
// draw's receive buffer (G blocks), so they must have its layout.
zr_result check_replay_layout(const ExecState& s, const DrawParams& P) {
    if (s.exchange != &replay_exchange) return ZR_SUCCESS;
    const zr_replay_exchange* r = (const zr_replay_exchange*)s.exchange_user;
    if (!r || !r->src || r->bytes != (uint64_t)s.shard_count * route_block_bytes(P.route_cap))
        return fail(ZR_ERROR_VALIDATION_FAILED,
                    "zr_replay_exchange_fn: recorded bytes differ from this draw's exchange layout "
                    "(shard count x route_block_bytes(route capacity))");
    return ZR_SUCCESS;
}

// k_setup_bin must be resident with the draw's LDS histogram (asked once per tile count).
zr_result check_setup_occupancy(zr_device* d, const DrawParams& P, bool mesh) {
    if (d->occupancy_checked_tiles == P.ntiles && d->occupancy_checked_mesh == mesh) return ZR_SUCCESS;
    int nb = 0;
    ZR_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, setup_bin_kernel(P.setup_batch, mesh), kSetupThreads,
                                                        setup_bin_lds_bytes(P.ntiles, 0)));
    if (nb < 1) return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "k_setup_bin cannot be resident on a CU");
    d->occupancy_checked_tiles = P.ntiles;
    d->occupancy_checked_mesh = mesh;
    return ZR_SUCCESS;
}

// The device-wide profiling buffers a draw may write: the winner census bitmap and
// the kDebugStamps array.
zr_result bind_profiling(zr_device* d, DrawParams& P) {
    if (d->census && !d->capturing) {  // winner census: a bitmap over the draw's primitives, zeroed per draw
        const uint64_t words = ((uint64_t)P.draw_prims + 31u) / 32u + 1u;
        const zr_result rc = grow(d, d->win_bits, words, 4);
        if (rc) return rc;
        ZR_HIP(hipMemsetAsync(d->win_bits.ptr, 0, words * 4, d->stream));
        P.win_bits = (uint32_t*)d->win_bits.ptr;
        d->census_words = words;
    }
    if (P.debug & kDebugStamps) {
        if (!d->dbg_ts) ZR_HIP(hipMalloc((void**)&d->dbg_ts, (8192 + kMaxTilesPerPass) * 8 * sizeof(unsigned long long)));
        P.dbg_ts = d->dbg_ts;
        d->dbg_wgs = P.setup_wgs;
        d->dbg_tiles = P.ntiles;
    }
    return ZR_SUCCESS;
}

// The first pass into a scratch set may start on `first` once the set's previous
// reader (the k_tile kScratchSets draws back) is done.
zr_result wait_last_reader(zr_device* d, ScratchSet& S, hipStream_t first) {
    if (S.main_reader_pending) {
        // everything enqueued on the main stream so far includes that last reader
        ZR_HIP(hipEventRecord(S.tile_done, d->stream));
        S.tile_done_valid = true;
        S.main_reader_pending = false;
    }
    if (S.tile_done_valid) ZR_HIP(hipStreamWaitEvent(first, S.tile_done, 0));
    return ZR_SUCCESS;
}

// Every draw marks its set's last reader: a later draw that sets up on
// setup_stream into this set waits for it.  An overlapped draw records its own
// tile_done right here (the next setup into the other set must not wait for
// it); a draw on the main stream alone only flags the set, and the event is
// recorded when an overlapped draw next needs the set (wait_last_reader), so
// back-to-back single-stream frames carry no event at all.
// (A graph capture uses set 0 only; submit_graph_or_eager flags it after the replay.)
zr_result mark_last_reader(zr_device* d, ScratchSet& S, bool overlap) {
    if (d->capturing) return ZR_SUCCESS;
    if (overlap) {
        ZR_HIP(hipEventRecord(S.tile_done, d->stream));
        S.tile_done_valid = true;
        S.main_reader_pending = false;
    } else {
        S.main_reader_pending = true;
    }
    return ZR_SUCCESS;
}

// debug early exits skip the self-reset at the end of k_setup_bin; the memsets
// go on the stream that runs this draw's k_setup_bin, so they precede it
// (partitioned: after the route, which waited for the set's last reader)
zr_result debug_resets(const DrawParams& P, hipStream_t ss) {
    if (!P.debug) return ZR_SUCCESS;
    ZR_HIP(hipMemsetAsync(P.counters, 0, kCtWords * 4, ss));
    ZR_HIP(hipMemsetAsync(P.tile_counts, 0, (size_t)P.ntiles * 4, ss));
    ZR_HIP(hipMemsetAsync(P.run_counts, 0, (size_t)P.ntiles * 4, ss));
    return ZR_SUCCESS;
}

// A partitioned draw up to its binning: k_route and the exchange on `rs`, then the
// records-mode k_setup_bin on `ss`, joined into the device stream.  `drawn` is
// false for a rank that owns no tile of the target (it only routes and exchanges).
zr_result enqueue_partitioned_setup(zr_device* d, const ExecState& s, ScratchSet& S, DrawParams& P, const DrawPlan& plan,
                                    hipStream_t rs, hipStream_t ss, bool& drawn) {
    zr_result rc;
    drawn = false;
    const uint64_t block = route_block_bytes(P.route_cap);
    const uint64_t bytes = (uint64_t)s.shard_count * block;
    if ((rc = grow(d, S.xsend, bytes, 1))) return rc;
    if ((rc = grow(d, S.xrecv, bytes, 1))) return rc;
    if ((rc = grow(d, S.gids, plan.positions, 4))) return rc;
    // The send headers' totals are k_route's counters: zero when the block
    // layout is new; afterwards this rank's records-mode setup re-zeroes them
    // once the exchange has consumed them (a rank without rows: below).
    const uint64_t layout = ((uint64_t)s.shard_count << 32) | P.route_cap;
    auto zero_headers = [&]() -> zr_result {
        ZR_HIP(hipMemset2DAsync(S.xsend.ptr, block, 0, sizeof(RouteHeader), s.shard_count, rs));
        return ZR_SUCCESS;
    };
    if (S.xsend_layout != layout) {
        if ((rc = zero_headers())) return rc;
        S.xsend_layout = layout;
    }
    P.route_out = (uint8_t*)S.xsend.ptr;
    P.gids = (uint32_t*)S.gids.ptr;
    timed_launch(d, "route", rs, [&] { launch_route(P, rs); });
    ZR_HIP(hipGetLastError());
    zr_result xr = ZR_SUCCESS;
    timed_launch(d, "exchange", rs, [&] { xr = s.exchange(s.exchange_user, (void*)rs, S.xsend.ptr, S.xrecv.ptr, block); });
    if (xr != ZR_SUCCESS) {
        // the route's totals stay in the send headers (no records-mode setup will
        // consume and re-zero them): the next draw on this set memsets them first
        S.xsend_layout = 0;
        return fail(xr, "tile-shard exchange callback failed: " + g_last_error);
    }
    P.rlist = (const uint8_t*)S.xrecv.ptr;
    if (P.ntiles == 0) {  // routed and exchanged; nothing of this target to draw here
        if ((rc = zero_headers())) return rc;  // (no records-mode setup to reset them)
        // joined back into the device stream like every other setup-stream pass, so
        // a fence (or a caller stream waiting on the device stream) covers the
        // route's reads of the caller's vertex and index buffers
        ZR_HIP(hipEventRecord(S.route_done, rs));
        ZR_HIP(hipStreamWaitEvent(d->stream, S.route_done, 0));
        return ZR_SUCCESS;
    }
    if (rs != ss) {  // the binning stage waits for this draw's exchange
        ZR_HIP(hipEventRecord(S.route_done, rs));
        ZR_HIP(hipStreamWaitEvent(ss, S.route_done, 0));
    }
    if ((rc = debug_resets(P, ss))) return rc;
    // Records-mode setup (binning the received records) runs on the setup
    // stream behind the exchange, so draw i+1's route, exchange and binning
    // overlap draw i's tile pass (the main stream only runs tile passes;
    // DESIGN.md §7).  k_setup_bin has no grid barrier, so sharing the GPU with
    // the collectives' kernels is safe.
    timed_launch(d, "setup_bin", ss, [&] { launch_setup_bin(P, ss); });
    ZR_HIP(hipEventRecord(S.setup_done, ss));
    ZR_HIP(hipStreamWaitEvent(d->stream, S.setup_done, 0));
    drawn = true;
    return ZR_SUCCESS;
}

// The draw's passes on the device's streams: setup (behind the route and exchange
// when partitioned), then the tile pass on the main stream.
zr_result enqueue_draw(zr_device* d, const ExecState& s, ScratchSet& S, DrawParams& P, const DrawPlan& plan) {
    zr_result rc;
    const hipStream_t ss = plan.overlap ? d->setup_stream : d->stream;
    // partitioned: route + exchange on their own stream (serialised: the device stream)
    const hipStream_t rs = plan.overlap ? d->route_stream : d->stream;
    if (plan.overlap && (rc = wait_last_reader(d, S, plan.partitioned ? rs : ss))) return rc;
    if (plan.partitioned) {
        bool drawn = false;
        if ((rc = enqueue_partitioned_setup(d, s, S, P, plan, rs, ss, drawn))) return rc;
        if (!drawn) return ZR_SUCCESS;
    } else {
        if ((rc = debug_resets(P, ss))) return rc;
        timed_launch(d, "setup_bin", ss, [&] { launch_setup_bin(P, ss); });
        if (plan.overlap) {
            ZR_HIP(hipEventRecord(S.setup_done, ss));
            ZR_HIP(hipStreamWaitEvent(d->stream, S.setup_done, 0));
        }
    }
    timed_launch(d, "tile", d->stream, [&] { launch_tile(P, d->stream); });
    if ((rc = mark_last_reader(d, S, plan.overlap))) return rc;
    ZR_HIP(hipGetLastError());
    return ZR_SUCCESS;
}

zr_result exec_draw(zr_device* d, ExecState& s, const Cmd& c, bool indexed) {
    zr_result rc = validate_draw_state(d, s, indexed);
    if (rc) return rc;
    DrawParams P;
    memset(&P, 0, sizeof P);
    if ((rc = fill_target(s, P))) return rc;
    DrawRequest rq;
    rq.vertex_count = c.a;
    rq.instances = c.b;
    rq.exchange = s.exchange != nullptr;
    rq.route_cap = s.route_cap;
    rq.cu_count = d->cu_count;
    rq.graphs = d->knobs.use_graphs;
    if ((rc = bind_inputs(s, c, indexed, P))) return rc;
    DrawPlan plan;
    std::string err;
    if ((rc = plan_draw(P, rq, d->knobs, d->book, plan, err))) return fail(rc, err);
    if (plan.nothing) return ZR_SUCCESS;
    if (plan.partitioned && (rc = check_replay_layout(s, P))) return rc;
    d->last_tile = 1u << P.tile_shift;
    if ((rc = check_setup_occupancy(d, P, plan.mesh))) return rc;
    if ((rc = bind_profiling(d, P))) return rc;
    ScratchSet& S = d->sets[plan.overlap ? d->cur_set : 0];
    if (plan.overlap) d->cur_set = (d->cur_set + 1u) % kScratchSets;
    if ((rc = ensure_scratch(d, S, P, plan))) return rc;
    d->last_prims = plan.prims;
    d->last.triangles_in = plan.prims;
    if ((rc = enqueue_draw(d, s, S, P, plan))) return rc;
    s.color_clear_pending = false;
    s.depth_clear_pending = false;
    return ZR_SUCCESS;
}

zr_result exec_end_rendering(zr_device* d, ExecState& s) {
    if (s.color_clear_pending || s.depth_clear_pending) {
        DrawParams P;
        memset(&P, 0, sizeof P);
        zr_result rc = fill_target(s, P);
        if (rc) return rc;
        timed_launch(d, "clear", d->stream, [&] { launch_clear(P, d->stream); });
        ZR_HIP(hipGetLastError());
    }
    s.rendering = false;
    s.color_clear_pending = s.depth_clear_pending = false;
    return ZR_SUCCESS;
}

zr_result execute(zr_device* d, zr_cmd* cmd) {
    ExecState s;
    for (const Cmd& c : cmd->cmds) {
        zr_result rc = ZR_SUCCESS;
        switch (c.type) {
        case C_BEGIN_RENDERING:
            s.rendering = true;
            s.rs = c.rendering;
            for (const zr_texture* t : {s.rs.has_color ? s.rs.color.texture : nullptr,
                                        s.rs.has_depth ? s.rs.depth.texture : nullptr}) {
                if (!t || !t->gather_pending) continue;
                if (d->capturing) return ZR_NOT_READY;  // a gather is not part of the graph: run eagerly
                ZR_HIP(hipStreamWaitEvent(d->stream, t->gather_done, 0));
            }
            s.color_clear_pending = s.rs.has_color && s.rs.color.load_op == ZR_ATTACHMENT_LOAD_OP_CLEAR;
            s.depth_clear_pending = s.rs.has_depth && s.rs.depth.load_op == ZR_ATTACHMENT_LOAD_OP_CLEAR;
            break;
        case C_END_RENDERING: rc = exec_end_rendering(d, s); break;
        case C_CLEAR_IMAGE: {
            // the k_clear of a render pass with LOAD_OP_CLEAR and no draw, over the
            // whole image on every rank (not a tile-row shard)
            if (s.rendering) { rc = fail(ZR_ERROR_VALIDATION_FAILED, "clear_color_image inside a render pass"); break; }
            ExecState cs;
            cs.rendering = true;
            cs.rs = c.rendering;
            cs.color_clear_pending = true;
            const zr_texture* t = c.rendering.color.texture;
            if (t->gather_pending) {
                if (d->capturing) return ZR_NOT_READY;
                ZR_HIP(hipStreamWaitEvent(d->stream, t->gather_done, 0));
            }
            rc = exec_end_rendering(d, cs);
            break;
        }
        case C_BIND_PIPELINE: s.pipe = c.pipeline; break;
        case C_BIND_UNIFORM: s.ubos[{c.a, c.b}] = {c.buffer, c.offset}; break;
        case C_SET_VIEWPORT: s.vp = c.vp; s.vp_set = true; break;
        case C_SET_SCISSOR: s.sc = c.rect; s.sc_set = true; break;
        case C_BIND_VB:
            if (c.a < 8) s.vb[c.a] = {c.buffer, c.offset};
            break;
        case C_BIND_IB: s.ib = c.buffer; s.ib_offset = c.offset; s.index_type = c.e; break;
        case C_DRAW: rc = exec_draw(d, s, c, c.d != 0); break;
        case C_SET_SHARD:
            s.shard_rank = c.a;
            s.shard_count = c.b;
            s.exchange = c.exchange;
            s.exchange_user = c.exchange_user;
            break;
        case C_SET_ROUTE_CAP: s.route_cap = c.a; break;
        case C_PUSH_CONSTANTS:
            memcpy((uint8_t*)s.push + c.a, cmd->push_data.data() + c.offset, c.b);
            for (uint32_t w = c.a / 4u; w < (c.a + c.b) / 4u; ++w) s.push_written |= 1u << w;
            s.push_layout = c.pipeline;
            break;
        }
        if (rc) return rc;
    }
    if (s.rendering) return exec_end_rendering(d, s);
    return ZR_SUCCESS;
}

}  // namespace

// ======================================================================= ABI

extern "C" {

ZR_API const char* zr_last_error_message(void) { return g_last_error.c_str(); }

ZR_API const char* zr_build_info(void) {
    return "libzenith_raster (HIP, gfx950): setup/scan/bin/tile passes, tile=32x32, 64-bit LDS visibility keys";
}

ZR_API zr_result zr_device_create(int32_t hip_device, zr_device** out) {
    if (!out) return fail(ZR_ERROR_VALIDATION_FAILED, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(ZR_ERROR_INITIALIZATION_FAILED, "no HIP device available");
    if (hip_device < 0 || hip_device >= n) return fail(ZR_ERROR_INITIALIZATION_FAILED, "bad device index");
    zr_device* d = new (std::nothrow) zr_device_t();
    if (!d) return fail(ZR_ERROR_OUT_OF_HOST_MEMORY, "device alloc");
    d->hip_device = hip_device;
    d->knobs = read_knobs();
    ZR_HIP(hipSetDevice(hip_device));
    ZR_HIP(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    d->own_stream = d->stream;
    ZR_HIP(hipStreamCreateWithFlags(&d->setup_stream, hipStreamNonBlocking));
    ZR_HIP(hipStreamCreateWithFlags(&d->route_stream, hipStreamNonBlocking));
    for (uint32_t b : {1u, 2u, 4u})  // histograms + bbox array may exceed the 64 KB default
        ZR_HIP(hipFuncSetAttribute(setup_bin_kernel(b, false), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)kSetupLdsBudget));
    ZR_HIP(hipFuncSetAttribute(setup_bin_kernel(1, true), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kSetupLdsBudget));
    ZR_HIP(hipDeviceGetAttribute(&d->cu_count, hipDeviceAttributeMultiprocessorCount, hip_device));
    void* st = nullptr;
    ZR_HIP(hipHostMalloc(&st, kStWords * 4, hipHostMallocMapped));
    memset(st, 0, kStWords * 4);
    d->status_host = (uint32_t*)st;
    void* sd = nullptr;
    ZR_HIP(hipHostGetDevicePointer(&sd, st, 0));
    d->status_dev = (uint32_t*)sd;
    *out = d;
    return ZR_SUCCESS;
}

ZR_API void zr_device_destroy(zr_device* d) {
    if (!d) return;
    (void)hipSetDevice(d->hip_device);
    (void)hipStreamSynchronize(d->route_stream);
    (void)hipStreamSynchronize(d->setup_stream);
    (void)hipStreamSynchronize(d->stream);
    collect_timings(d);
    for (hipEvent_t e : d->event_pool) (void)hipEventDestroy(e);
    if (d->dbg_ts) (void)hipFree(d->dbg_ts);
    if (d->win_bits.ptr) (void)hipFree(d->win_bits.ptr);
    for (ScratchSet& S : d->sets) {
        for (const ScratchBuf* b : {&S.job_slot, &S.job_keys, &S.job_tickets, &S.runs, &S.run_counts, &S.records,
                                    &S.records_big, &S.mesh_edges, &S.bboxes, &S.tile_counts, &S.draw_info, &S.counters,
                                    &S.bins, &S.xsend, &S.xrecv, &S.gids, &S.tile_order})
            if (b->ptr) (void)hipFree(b->ptr);
        if (S.setup_done) (void)hipEventDestroy(S.setup_done);
        if (S.route_done) (void)hipEventDestroy(S.route_done);
        if (S.tile_done) (void)hipEventDestroy(S.tile_done);
    }
    (void)hipHostFree(d->status_host);
    rccl_comm_destroy(d->comm_x);
    rccl_comm_destroy(d->comm_g);
    if (d->gather_stream) (void)hipStreamDestroy(d->gather_stream);
    if (d->gather_stage) (void)hipFree(d->gather_stage);
    if (d->frame_done) (void)hipEventDestroy(d->frame_done);
    (void)hipStreamDestroy(d->setup_stream);
    (void)hipStreamDestroy(d->route_stream);
    (void)hipStreamDestroy(d->own_stream);
    delete d;
}

ZR_API zr_result zr_device_set_stream(zr_device* d, void* hip_stream) {
    if (!d) return fail(ZR_ERROR_VALIDATION_FAILED, "device is NULL");
    zr_result rc = device_sync(d);
    if (rc) return rc;
    d->stream = hip_stream ? (hipStream_t)hip_stream : d->own_stream;
    return ZR_SUCCESS;
}

ZR_API void* zr_device_stream(const zr_device* d) { return d ? (void*)d->stream : nullptr; }

ZR_API zr_result zr_device_wait_idle(zr_device* d) {
    if (!d) return fail(ZR_ERROR_VALIDATION_FAILED, "device is NULL");
    return device_sync(d);
}

ZR_API zr_result zr_device_set_profiling(zr_device* d, int32_t enable) {
    if (!d) return fail(ZR_ERROR_VALIDATION_FAILED, "device is NULL");
    d->profiling = enable != 0;
    d->census = enable >= 2 ? 1 : 0;
    return ZR_SUCCESS;
}

ZR_API int32_t zr_device_kernel_times(zr_device* d, zr_kernel_time* out, int32_t capacity, int32_t reset) {
    if (!d) return 0;
    int32_t n = 0;
    for (const auto& kv : d->times) {
        if (out && n < capacity) {
            memset(&out[n], 0, sizeof(zr_kernel_time));
            snprintf(out[n].name, sizeof(out[n].name), "%s", kv.first.c_str());
            out[n].total_ms = kv.second.first;
            out[n].launches = kv.second.second;
        }
        ++n;
    }
    if (reset) d->times.clear();
    return std::min(n, capacity);
}

ZR_API zr_result zr_device_last_draw_stats(zr_device* d, zr_draw_stats* out) {
    if (!d || !out) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    *out = d->last;
    return ZR_SUCCESS;
}

// --------------------------------------------------------------- submission

ZR_API zr_result zr_fence_create(zr_device* d, zr_fence** out) {
    if (!d || !out) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    zr_result rc = set_device(d);
    if (rc) return rc;
    zr_fence* f = new (std::nothrow) zr_fence_t();
    if (!f) return fail(ZR_ERROR_OUT_OF_HOST_MEMORY, "fence alloc");
    f->dev = d;
    if (hipEventCreateWithFlags(&f->ev, hipEventDisableTiming) != hipSuccess) {
        delete f;
        return fail(ZR_ERROR_DEVICE_LOST, "hipEventCreate failed");
    }
    *out = f;
    return ZR_SUCCESS;
}

ZR_API void zr_fence_destroy(zr_fence* f) {
    if (!f) return;
    (void)hipEventSynchronize(f->ev);
    (void)hipEventDestroy(f->ev);
    delete f;
}

// Executes a command list on the device stream.  The first submission runs eagerly
// (sizing scratch); the second captures the same launches into a HIP graph, later
// ones replay it (one launch per frame instead of one per kernel).
static zr_result submit_graph_or_eager(zr_device* d, zr_cmd* c) {
    const bool graphs = d->knobs.use_graphs && !d->profiling && !d->knobs.debug && !c->has_exchange;
    if (!graphs || c->eager_runs == 0) {
        c->eager_runs++;
        return execute(d, c);
    }
    // a replayed graph's draws read and write scratch set 0 on the main stream
    auto mark_set0 = [d]() -> zr_result {
        d->sets[0].main_reader_pending = true;
        return ZR_SUCCESS;
    };
    if (c->graph && c->graph_gen == d->scratch_gen) {
        ZR_HIP(hipGraphLaunch(c->graph, d->stream));
        return mark_set0();
    }
    c->drop_graph();
    const uint64_t gen = d->scratch_gen;
    ZR_HIP(hipStreamBeginCapture(d->stream, hipStreamCaptureModeRelaxed));
    d->capturing = true;
    zr_result rc = execute(d, c);
    d->capturing = false;
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(d->stream, &g);
    if (rc == ZR_SUCCESS && e == hipSuccess && g && d->scratch_gen == gen) {
        const hipError_t ie = hipGraphInstantiate(&c->graph, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ie == hipSuccess) {
            c->graph_gen = gen;
            ZR_HIP(hipGraphLaunch(c->graph, d->stream));
            return mark_set0();
        }
        c->graph = nullptr;
    } else if (g) {
        (void)hipGraphDestroy(g);
    }
    if (rc != ZR_SUCCESS && rc != ZR_NOT_READY) return rc;
    c->eager_runs++;
    return execute(d, c);  // scratch had to grow (or capture failed): run eagerly
}

ZR_API zr_result zr_submit(zr_device* d, zr_cmd* c, zr_fence* f) {
    if (!d || !c) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    if (c->dev != d) return fail(ZR_ERROR_VALIDATION_FAILED, "command list was created for another device (or none)");
    if (c->err) return fail(c->err, c->err_msg);
    if (c->in_rendering) return fail(ZR_ERROR_VALIDATION_FAILED, "submitted inside a render pass");
    zr_result rc = set_device(d);
    if (rc) return rc;
    rc = submit_graph_or_eager(d, c);
    if (rc) return rc;
    if (std::find(d->pending.begin(), d->pending.end(), c) == d->pending.end()) d->pending.push_back(c);
    if (f) {
        ZR_HIP(hipEventRecord(f->ev, d->stream));
        f->submitted = true;
    }
    return ZR_SUCCESS;
}

ZR_API zr_result zr_fence_wait(zr_fence* f, uint64_t timeout_ns) {
    if (!f) return fail(ZR_ERROR_VALIDATION_FAILED, "fence is NULL");
    if (!f->submitted) return ZR_SUCCESS;
    if (timeout_ns == 0) {
        hipError_t e = hipEventQuery(f->ev);
        if (e == hipErrorNotReady) return ZR_TIMEOUT;
        if (e != hipSuccess) return fail(ZR_ERROR_DEVICE_LOST, hipGetErrorString(e));
    }
    return device_sync(f->dev);
}

ZR_API zr_result zr_submit_and_wait(zr_device* d, zr_cmd* c) {
    zr_result rc = zr_submit(d, c, nullptr);
    if (rc) return rc;
    return device_sync(d);
}

}  // extern "C"
