// zr_multi.cpp — multi-GPU glue: the host-side gather and exchange plans, the RCCL
// and replay exchange callbacks of partitioned tile shards, and the tile-row gather.
#include "zr_runtime.h"

using namespace zr;

namespace zr {

// The built-in zr_exchange_fn: one grouped send + receive per rank over the
// device's exchange communicator, enqueued on the stream the runtime passes.
zr_result rccl_exchange(void* user, void* stream, const void* send, void* recv, uint64_t bytes_per_rank) {
    zr_device* d = (zr_device*)user;
    if (!d || !d->comm_x) return fail(ZR_ERROR_INITIALIZATION_FAILED, "zr_rccl_exchange_fn: device has no RCCL communicator");
    std::string err;
    const hipStream_t s = (hipStream_t)stream;
    if (rccl_has_all_to_all()) {
        if (!rccl_all_to_all(send, recv, bytes_per_rank, d->comm_x, s, err)) return fail(ZR_ERROR_DEVICE_LOST, err);
        return ZR_SUCCESS;
    }
    zr_transfer_op plan[2 * kMaxShards];
    const int32_t n = zr_exchange_plan(d->comm_size, d->comm_rank, bytes_per_rank, plan, 2 * (int32_t)kMaxShards);
    if (n < 0) return fail(ZR_ERROR_VALIDATION_FAILED, "bad exchange plan (rank / rank count)");
    P2POp ops[2 * kMaxShards];
    for (int32_t i = 0; i < n; ++i)
        ops[i] = P2POp{plan[i].send ? (void*)((const uint8_t*)send + plan[i].offset) : (void*)((uint8_t*)recv + plan[i].offset),
                       (size_t)plan[i].bytes, plan[i].peer, plan[i].send != 0};
    if (!rccl_grouped(ops, (size_t)n, d->comm_x, s, err)) return fail(ZR_ERROR_DEVICE_LOST, err);
    return ZR_SUCCESS;
}

}  // namespace zr

extern "C" {

// Host-side plans of the two collectives (no device needed; tests/test_abi.py).
// Gather (ShardGeom ownership): a round-robin tile row is a contiguous span of the
// linear image, sent from its owner straight into place on the root; a leftover
// row holds one run of tiles per owner, a rectangle (rows spans `pitch` apart)
// unless it is the whole row -- the runtime packs it into a staging buffer to send
// and unpacks it on the root.  One op per (tile row, owner), none for the root's
// own tiles.  `offset` is the byte offset in the image (the same on both sides);
// the last tile row may be partial.
ZR_API uint32_t zr_tile_size(void) { return (uint32_t)kTile; }

ZR_API int32_t zr_gather_plan(uint32_t width, uint32_t height, uint32_t bytes_per_pixel, int32_t nranks, int32_t rank,
                              int32_t root, zr_transfer_op* out, int32_t capacity) {
    if (nranks < 1 || nranks > (int32_t)kMaxShards || rank < 0 || rank >= nranks || root < 0 || root >= nranks ||
        width == 0 || height == 0 || bytes_per_pixel == 0)
        return -1;
    const uint32_t tiles_x = (width + kTile - 1) / kTile, tiles_y = (height + kTile - 1) / kTile;
    const uint64_t row_bytes = (uint64_t)width * bytes_per_pixel;
    int32_t n = 0;
    auto emit = [&](int32_t owner, uint32_t ty, uint32_t c0, uint32_t c1) {  // tiles [c0, c1] of row ty
        if (owner == root || (rank != root && rank != owner)) return;
        const uint32_t rows = std::min<uint32_t>(kTile, height - ty * kTile);
        const uint32_t x0 = c0 * kTile, x1 = std::min<uint32_t>(width, (c1 + 1) * kTile);
        if (out && n < capacity) {
            zr_transfer_op& op = out[n];
            memset(&op, 0, sizeof op);
            op.peer = rank == root ? owner : root;
            op.send = rank == root ? 0 : 1;
            op.offset = (uint64_t)ty * kTile * row_bytes + (uint64_t)x0 * bytes_per_pixel;
            if (x0 == 0 && x1 == width) {  // whole rows: one contiguous span
                op.bytes = (uint64_t)rows * row_bytes;
                op.rows = 1;
            } else {
                op.bytes = (uint64_t)(x1 - x0) * bytes_per_pixel;
                op.rows = rows;
                op.pitch = row_bytes;
            }
        }
        ++n;
    };
    for (int32_t r = 0; r < nranks; ++r) {
        const ShardGeom sg = shard_geom(tiles_x, tiles_y, (uint32_t)nranks, (uint32_t)r);
        for (uint32_t ty = (uint32_t)r; ty < sg.full_rows; ty += (uint32_t)nranks) emit(r, ty, 0, tiles_x - 1);
        for (uint32_t i = sg.left_lo; i < sg.left_hi;) {  // its leftover run, cut at row ends
            const uint32_t ty = sg.full_rows + i / tiles_x, c0 = i % tiles_x;
            const uint32_t c1 = std::min(tiles_x - 1, c0 + (sg.left_hi - i) - 1);
            emit(r, ty, c0, c1);
            i += c1 - c0 + 1;
        }
    }
    return n;
}

// Exchange (all-to-all without ncclAllToAll): to every rank p (itself included)
// send block p of the send buffer, and receive p's block for this rank at p *
// bytes_per_rank of the receive buffer, paired per peer in one group.
ZR_API int32_t zr_exchange_plan(int32_t nranks, int32_t rank, uint64_t bytes_per_rank, zr_transfer_op* out,
                                int32_t capacity) {
    if (nranks < 1 || nranks > (int32_t)kMaxShards || rank < 0 || rank >= nranks) return -1;
    int32_t n = 0;
    for (int32_t p = 0; p < nranks; ++p)
        for (int32_t send = 1; send >= 0; --send) {
            if (out && n < capacity) {
                memset(&out[n], 0, sizeof out[n]);
                out[n].peer = p;
                out[n].send = send;
                out[n].offset = (uint64_t)p * bytes_per_rank;
                out[n].bytes = bytes_per_rank;
                out[n].rows = 1;
            }
            ++n;
        }
    return n;
}

ZR_API int32_t zr_rccl_available(void) {
    std::string err;
    return rccl_load(err) ? 1 : 0;
}

ZR_API zr_result zr_rccl_get_unique_id(void* out) {
    if (!out) return fail(ZR_ERROR_VALIDATION_FAILED, "out is NULL");
    std::string err;
    if (!rccl_unique_id(out, err)) return fail(ZR_ERROR_INITIALIZATION_FAILED, err);
    return ZR_SUCCESS;
}

ZR_API zr_result zr_device_init_rccl(zr_device* d, const void* exchange_id, const void* gather_id, int32_t nranks,
                                     int32_t rank) {
    if (!d || !exchange_id || !gather_id) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    if (nranks < 1 || nranks > (int32_t)kMaxShards || rank < 0 || rank >= nranks)
        return fail(ZR_ERROR_VALIDATION_FAILED, "bad rank / rank count");
    if (d->comm_x) return fail(ZR_ERROR_VALIDATION_FAILED, "device already has RCCL communicators");
    zr_result rc = set_device(d);
    if (rc) return rc;
    std::string err;
    if (!rccl_comm_init(&d->comm_x, exchange_id, nranks, rank, err) ||
        !rccl_comm_init(&d->comm_g, gather_id, nranks, rank, err)) {
        rccl_comm_destroy(d->comm_x);
        d->comm_x = nullptr;
        return fail(ZR_ERROR_INITIALIZATION_FAILED, err);
    }
    d->comm_rank = rank;
    d->comm_size = nranks;
    ZR_HIP(hipStreamCreateWithFlags(&d->gather_stream, hipStreamNonBlocking));
    ZR_HIP(hipEventCreateWithFlags(&d->frame_done, hipEventDisableTiming));
    return ZR_SUCCESS;
}

ZR_API zr_exchange_fn zr_rccl_exchange_fn(void) { return &rccl_exchange; }

}  // extern "C"

namespace zr {

// The recorded receive blocks must be whole blocks of this draw's layout: the
// receive buffer holds shard_count x bytes_per_rank bytes (exec_draw checks the
// count against the draw before the route runs; here, without the count, a size
// that is no whole number of blocks or more than kMaxShards of them is refused --
// a buffer recorded at another route capacity or shard count would otherwise be
// copied past the end of the receive buffer).
zr_result replay_exchange(void* user, void* stream, const void* send, void* recv, uint64_t bytes_per_rank) {
    (void)send;
    const zr_replay_exchange* r = (const zr_replay_exchange*)user;
    if (!r || !r->src) return fail(ZR_ERROR_VALIDATION_FAILED, "zr_replay_exchange_fn: no recorded buffer");
    if (bytes_per_rank == 0 || r->bytes == 0 || r->bytes % bytes_per_rank != 0 || r->bytes / bytes_per_rank > kMaxShards)
        return fail(ZR_ERROR_VALIDATION_FAILED,
                    "zr_replay_exchange_fn: recorded bytes are not whole exchange blocks of this draw's layout");
    ZR_HIP(hipMemcpyAsync(recv, r->src, r->bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ZR_SUCCESS;
}

}  // namespace zr

extern "C" {

ZR_API zr_exchange_fn zr_replay_exchange_fn(void) { return &replay_exchange; }

ZR_API zr_result zr_device_gather_tile_rows(zr_device* d, zr_texture* t, int32_t root) {
    if (!d || !t) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    if (!d->comm_g) return fail(ZR_ERROR_INITIALIZATION_FAILED, "device has no RCCL communicator (zr_device_init_rccl)");
    if (root < 0 || root >= d->comm_size) return fail(ZR_ERROR_VALIDATION_FAILED, "bad root rank");
    zr_result rc = set_device(d);
    if (rc) return rc;
    if (!t->gather_done) ZR_HIP(hipEventCreateWithFlags(&t->gather_done, hipEventDisableTiming));
    // after everything enqueued so far on the device stream (the frame)
    ZR_HIP(hipEventRecord(d->frame_done, d->stream));
    ZR_HIP(hipStreamWaitEvent(d->gather_stream, d->frame_done, 0));
    const int32_t n = zr_gather_plan(t->width, t->height, t->bpp, d->comm_size, d->comm_rank, root, nullptr, 0);
    std::vector<zr_transfer_op> plan((size_t)std::max(n, 0));
    zr_gather_plan(t->width, t->height, t->bpp, d->comm_size, d->comm_rank, root, plan.data(), n);
    // rectangles (leftover rows' tile runs) travel packed through a staging buffer
    uint64_t stage_bytes = 0;
    for (const zr_transfer_op& op : plan)
        if (op.rows > 1) stage_bytes += op.bytes * op.rows;
    if (stage_bytes > d->gather_stage_cap) {
        ZR_HIP(hipStreamSynchronize(d->gather_stream));
        if (d->gather_stage) ZR_HIP(hipFree(d->gather_stage));
        d->gather_stage = nullptr;
        ZR_HIP(hipMalloc((void**)&d->gather_stage, stage_bytes));
        d->gather_stage_cap = stage_bytes;
    }
    const hipStream_t gs = d->gather_stream;
    uint64_t so = 0;
    for (const zr_transfer_op& op : plan) {  // senders pack first
        if (op.rows <= 1) continue;
        if (op.send)
            ZR_HIP(hipMemcpy2DAsync(d->gather_stage + so, op.bytes, (const uint8_t*)t->ptr + op.offset, op.pitch, op.bytes,
                                    op.rows, hipMemcpyDeviceToDevice, gs));
        so += op.bytes * op.rows;
    }
    std::string err;
    std::vector<P2POp> ops;
    ops.reserve(plan.size());
    so = 0;
    for (const zr_transfer_op& op : plan) {
        uint8_t* p = (uint8_t*)t->ptr + op.offset;
        uint64_t bytes = op.bytes;
        if (op.rows > 1) {
            p = d->gather_stage + so;
            bytes = op.bytes * op.rows;
            so += bytes;
        }
        ops.push_back(P2POp{p, (size_t)bytes, op.peer, op.send != 0});
    }
    // one balanced group (rccl_grouped: no ncclGroupEnd after a failed start)
    if (!rccl_grouped(ops.data(), ops.size(), d->comm_g, gs, err)) return fail(ZR_ERROR_DEVICE_LOST, err);
    so = 0;
    for (const zr_transfer_op& op : plan) {  // the root unpacks after the group
        if (op.rows <= 1) continue;
        if (!op.send)
            ZR_HIP(hipMemcpy2DAsync((uint8_t*)t->ptr + op.offset, op.pitch, d->gather_stage + so, op.bytes, op.bytes,
                                    op.rows, hipMemcpyDeviceToDevice, gs));
        so += op.bytes * op.rows;
    }
    ZR_HIP(hipEventRecord(t->gather_done, d->gather_stream));
    t->gather_pending = true;
    return ZR_SUCCESS;
}

}  // extern "C"
