// zr_cmd.cpp — command recording (zr_cmd_*): a list records like vkCmd* and latches
// its first error; zr_submit (zr_runtime.cpp) walks the recorded state machine.
#include "zr_runtime.h"

using namespace zr;

namespace {

void latch(zr_cmd* cmd, zr_result rc, const std::string& msg) {
    if (cmd->err == ZR_SUCCESS) {
        cmd->err = rc;
        cmd->err_msg = msg;
    }
}

}  // namespace

extern "C" {

ZR_API zr_result zr_cmd_create(zr_device* d, zr_cmd** out) {
    // d may be NULL: a list recorded without a device (host-side validation of the
    // recording calls, e.g. on a machine without a GPU); zr_submit rejects it
    if (!out) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    zr_cmd* c = new (std::nothrow) zr_cmd_t();
    if (!c) return fail(ZR_ERROR_OUT_OF_HOST_MEMORY, "cmd alloc");
    c->dev = d;
    *out = c;
    return ZR_SUCCESS;
}

ZR_API void zr_cmd_destroy(zr_cmd* c) {
    if (!c) return;
    if (c->dev) {
        auto& pend = c->dev->pending;
        if (std::find(pend.begin(), pend.end(), c) != pend.end()) device_sync(c->dev);
    }
    c->drop_graph();
    delete c;
}

ZR_API zr_result zr_cmd_begin(zr_cmd* c) {
    if (!c) return fail(ZR_ERROR_VALIDATION_FAILED, "cmd is NULL");
    if (c->dev) {
        auto& pend = c->dev->pending;
        if (std::find(pend.begin(), pend.end(), c) != pend.end()) {
            zr_result rc = device_sync(c->dev);
            if (rc) return rc;
        }
    }
    c->cmds.clear();
    c->push_data.clear();
    c->err = ZR_SUCCESS;
    c->err_msg.clear();
    c->in_rendering = false;
    c->drop_graph();
    c->eager_runs = 0;
    c->has_exchange = false;
    return ZR_SUCCESS;
}

ZR_API zr_result zr_cmd_end(zr_cmd* c) {
    if (!c) return fail(ZR_ERROR_VALIDATION_FAILED, "cmd is NULL");
    if (c->in_rendering) latch(c, ZR_ERROR_VALIDATION_FAILED, "command buffer ended inside a render pass");
    if (c->err) return fail(c->err, c->err_msg);
    return ZR_SUCCESS;
}

ZR_API void zr_cmd_begin_rendering(zr_cmd* c, const zr_rendering_info* info) {
    if (!c) return;
    if (!info) return latch(c, ZR_ERROR_VALIDATION_FAILED, "rendering info is NULL");
    if (c->in_rendering) return latch(c, ZR_ERROR_VALIDATION_FAILED, "nested begin_rendering");
    if (info->color_attachment_count > 1)
        return latch(c, ZR_ERROR_FEATURE_NOT_PRESENT, "at most one colour attachment");
    Cmd k;
    k.type = C_BEGIN_RENDERING;
    k.rendering.area = info->render_area;
    if (info->color_attachment_count == 1) {
        k.rendering.has_color = info->color_attachments[0].texture != nullptr;
        k.rendering.color = info->color_attachments[0];
    }
    if (info->depth_attachment && info->depth_attachment->texture) {
        k.rendering.has_depth = true;
        k.rendering.depth = *info->depth_attachment;
    }
    c->cmds.push_back(k);
    c->in_rendering = true;
}

ZR_API void zr_cmd_end_rendering(zr_cmd* c) {
    if (!c) return;
    if (!c->in_rendering) return latch(c, ZR_ERROR_VALIDATION_FAILED, "end_rendering without begin_rendering");
    Cmd k;
    k.type = C_END_RENDERING;
    c->cmds.push_back(k);
    c->in_rendering = false;
}

ZR_API void zr_cmd_clear_color_image(zr_cmd* c, zr_texture* t, const float clear_value[4]) {
    if (!c) return;
    if (c->in_rendering) return latch(c, ZR_ERROR_VALIDATION_FAILED, "clear_color_image inside a render pass");
    if (!t || !clear_value) return latch(c, ZR_ERROR_VALIDATION_FAILED, "clear_color_image: NULL argument");
    if (t->format == ZR_FORMAT_D32_SFLOAT) return latch(c, ZR_ERROR_VALIDATION_FAILED, "clear_color_image on a depth texture");
    Cmd k;
    k.type = C_CLEAR_IMAGE;
    k.rendering.area = zr_rect2d{0, 0, t->width, t->height};
    k.rendering.has_color = true;
    k.rendering.color.texture = t;
    k.rendering.color.load_op = ZR_ATTACHMENT_LOAD_OP_CLEAR;
    for (int i = 0; i < 4; ++i) k.rendering.color.clear_value[i] = clear_value[i];
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_bind_pipeline(zr_cmd* c, const zr_pipeline* p) {
    if (!c) return;
    if (!p) return latch(c, ZR_ERROR_VALIDATION_FAILED, "pipeline is NULL");
    Cmd k;
    k.type = C_BIND_PIPELINE;
    k.pipeline = p;
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_bind_uniform_buffer(zr_cmd* c, uint32_t set, uint32_t binding, const zr_buffer* buf,
                                       uint64_t offset, uint64_t range) {
    if (!c) return;
    if (!buf) return latch(c, ZR_ERROR_VALIDATION_FAILED, "uniform buffer is NULL");
    Cmd k;
    k.type = C_BIND_UNIFORM;
    k.a = set;
    k.b = binding;
    k.buffer = buf;
    k.offset = offset;
    k.range = range;
    c->cmds.push_back(k);
}

ZR_API zr_result zr_cmd_bind_uniform_by_name(zr_cmd* c, const zr_pipeline* p, const char* name, const zr_buffer* buf,
                                             uint64_t offset, uint64_t range) {
    if (!c || !p || !name || !buf) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    for (const auto& b : p->bindings) {
        if (!strcmp(b.name, name)) {
            if (b.descriptor_type != ZR_DESCRIPTOR_TYPE_UNIFORM_BUFFER && b.descriptor_type != ZR_DESCRIPTOR_TYPE_STORAGE_BUFFER)
                return fail(ZR_ERROR_BINDING_TYPE_MISMATCH, std::string("binding '") + name + "' is not a buffer");
            zr_cmd_bind_uniform_buffer(c, b.set, b.binding, buf, offset, range);
            return ZR_SUCCESS;
        }
    }
    return fail(ZR_ERROR_BINDING_NOT_FOUND, std::string("binding '") + name + "' not found");
}

ZR_API void zr_cmd_push_constants(zr_cmd* c, const zr_pipeline* layout, uint32_t stage_flags, uint32_t offset,
                                  uint32_t size, const void* data) {
    if (!c) return;
    if (!layout || !data) return latch(c, ZR_ERROR_VALIDATION_FAILED, "push_constants: NULL layout or data");
    if ((offset & 3u) || (size & 3u) || size == 0 || offset >= kMaxPushBytes || size > kMaxPushBytes - offset)
        return latch(c, ZR_ERROR_VALIDATION_FAILED,
                     "push_constants: offset/size not multiples of 4, empty, or past maxPushConstantsSize (128)");
    if (stage_flags == 0) return latch(c, ZR_ERROR_VALIDATION_FAILED, "push_constants: no stage flags");
    // VUID-vkCmdPushConstants-offset-01795 / -01796: every byte of the update lies in
    // a range holding every stage of stage_flags, and stage_flags holds every stage
    // of each range the update overlaps
    for (uint32_t b = offset; b < offset + size; b += 4u) {
        uint32_t stages = 0;
        for (const auto& r : layout->push_ranges) {
            if (b < r.offset || b >= r.offset + r.size) continue;
            stages |= r.stage_flags;
            if ((r.stage_flags & stage_flags) != r.stage_flags)
                return latch(c, ZR_ERROR_VALIDATION_FAILED,
                             "push_constants: stage_flags miss a stage of a push-constant range the update overlaps");
        }
        if ((stages & stage_flags) != stage_flags)
            return latch(c, ZR_ERROR_VALIDATION_FAILED,
                         "push_constants: bytes outside the layout's push-constant ranges for these stages");
    }
    Cmd k;
    k.type = C_PUSH_CONSTANTS;
    k.pipeline = layout;
    k.a = offset;
    k.b = size;
    k.offset = c->push_data.size();
    c->push_data.insert(c->push_data.end(), (const uint8_t*)data, (const uint8_t*)data + size);
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_set_viewport(zr_cmd* c, uint32_t first, uint32_t count, const zr_viewport* vps) {
    if (!c) return;
    if (!vps || count == 0) return;
    if (first != 0 || count != 1) return latch(c, ZR_ERROR_FEATURE_NOT_PRESENT, "only viewport 0");
    Cmd k;
    k.type = C_SET_VIEWPORT;
    k.vp = vps[0];
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_set_scissor(zr_cmd* c, uint32_t first, uint32_t count, const zr_rect2d* rects) {
    if (!c) return;
    if (!rects || count == 0) return;
    if (first != 0 || count != 1) return latch(c, ZR_ERROR_FEATURE_NOT_PRESENT, "only scissor 0");
    Cmd k;
    k.type = C_SET_SCISSOR;
    k.rect = rects[0];
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_bind_vertex_buffers(zr_cmd* c, uint32_t first_binding, uint32_t count, const zr_buffer* const* bufs,
                                       const uint64_t* offsets) {
    if (!c) return;
    for (uint32_t i = 0; i < count; ++i) {
        if (!bufs || !bufs[i]) return latch(c, ZR_ERROR_VALIDATION_FAILED, "vertex buffer is NULL");
        Cmd k;
        k.type = C_BIND_VB;
        k.a = first_binding + i;
        k.buffer = bufs[i];
        k.offset = offsets ? offsets[i] : 0;
        c->cmds.push_back(k);
    }
}

ZR_API void zr_cmd_bind_index_buffer(zr_cmd* c, const zr_buffer* buf, uint64_t offset, int32_t index_type) {
    if (!c) return;
    if (!buf) return latch(c, ZR_ERROR_VALIDATION_FAILED, "index buffer is NULL");
    if (index_type != ZR_INDEX_TYPE_UINT16 && index_type != ZR_INDEX_TYPE_UINT32)
        return latch(c, ZR_ERROR_FEATURE_NOT_PRESENT, "index type");
    Cmd k;
    k.type = C_BIND_IB;
    k.buffer = buf;
    k.offset = offset;
    k.e = index_type;
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_draw(zr_cmd* c, uint32_t vertex_count, uint32_t instance_count, uint32_t first_vertex,
                        uint32_t first_instance) {
    if (!c) return;
    Cmd k;
    k.type = C_DRAW;
    k.a = vertex_count;
    k.b = instance_count;
    k.c = first_vertex;
    k.d = 0;
    k.e = 0;
    (void)first_instance;
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_draw_indexed(zr_cmd* c, uint32_t index_count, uint32_t instance_count, uint32_t first_index,
                                int32_t vertex_offset, uint32_t first_instance) {
    if (!c) return;
    Cmd k;
    k.type = C_DRAW;
    k.a = index_count;
    k.b = instance_count;
    k.c = first_index;
    k.d = 1;
    k.e = vertex_offset;
    (void)first_instance;
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_set_tile_shard(zr_cmd* c, uint32_t rank, uint32_t count) {
    if (!c) return;
    if (count == 0 || rank >= count) return latch(c, ZR_ERROR_VALIDATION_FAILED, "bad tile shard");
    Cmd k;
    k.type = C_SET_SHARD;
    k.a = rank;
    k.b = count;
    c->cmds.push_back(k);
}

ZR_API void zr_cmd_set_tile_shard_exchange(zr_cmd* c, uint32_t rank, uint32_t count, zr_exchange_fn exchange,
                                           void* user) {
    if (!c) return;
    if (count == 0 || rank >= count || count > kMaxShards) return latch(c, ZR_ERROR_VALIDATION_FAILED, "bad tile shard");
    if (!exchange) return latch(c, ZR_ERROR_VALIDATION_FAILED, "tile shard exchange is NULL");
    Cmd k;
    k.type = C_SET_SHARD;
    k.a = rank;
    k.b = count;
    k.exchange = exchange;
    k.exchange_user = user;
    c->cmds.push_back(k);
    c->has_exchange = true;
}

ZR_API void zr_cmd_set_route_capacity(zr_cmd* c, uint32_t entries) {
    if (!c) return;
    Cmd k;
    k.type = C_SET_ROUTE_CAP;
    k.a = entries;
    c->cmds.push_back(k);
}

}  // extern "C"
