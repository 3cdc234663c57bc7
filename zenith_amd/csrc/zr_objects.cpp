// zr_objects.cpp — buffers, textures, the built-in shader registry and pipelines
// (with their validation) of the C ABI in include/zenith_raster.h.
#include "zr_runtime.h"
#include "zr_shading.h"

using namespace zr;

namespace {

// ------------------------------------------------------------ shader registry

struct ShaderEntry {
    const char* file;
    const char* entry;
    uint32_t stage;
    int32_t program;
    int nbind;
    zr_shader_binding bind[1];
    int ninputs;
    zr_vertex_input_attr inputs[4];
    uint32_t push_size;  // ShaderReflection::push_constant_size (shader.rs:214)
};

// Built-in stage variants.  triangle.slang is the reference's
// (content/shaders/triangle.slang:3-8 inputs, :27-32 "Time" at set 0 / binding 0);
// flat_color / blinn_phong are this repo's (content/shaders/).
const ShaderEntry kShaders[] = {
    {"triangle.slang", "vsmain", ZR_SHADER_STAGE_VERTEX, kProgTriangle, 0, {},
     2, {{0, ZR_FORMAT_R32G32B32_SFLOAT}, {1, ZR_FORMAT_R32G32B32_SFLOAT}}},
    {"triangle.slang", "psmain", ZR_SHADER_STAGE_FRAGMENT, kProgTriangle, 1,
     {{"Time", 0, 0, ZR_DESCRIPTOR_TYPE_UNIFORM_BUFFER, 1, ZR_SHADER_STAGE_FRAGMENT}}, 0, {}},
    {"flat_color.slang", "vsmain", ZR_SHADER_STAGE_VERTEX, kProgFlat, 0, {},
     2, {{0, ZR_FORMAT_R32G32B32_SFLOAT}, {1, ZR_FORMAT_R32G32B32_SFLOAT}}},
    {"flat_color.slang", "psmain", ZR_SHADER_STAGE_FRAGMENT, kProgFlat, 0, {}, 0, {}},
    {"blinn_phong.slang", "vsmain", ZR_SHADER_STAGE_VERTEX, kProgBlinn, 0, {},
     3, {{0, ZR_FORMAT_R32G32B32_SFLOAT}, {1, ZR_FORMAT_R32G32B32_SFLOAT}, {2, ZR_FORMAT_R32G32B32_SFLOAT}}},
    {"blinn_phong.slang", "psmain", ZR_SHADER_STAGE_FRAGMENT, kProgBlinn, 0, {}, 0, {}},
    // mesh.slang: camera program over zenith-asset's Vertex
    // {position, normal, uv} (zenith-asset/src/render.rs:12-16); View = view_proj
    {"mesh.slang", "vsmain", ZR_SHADER_STAGE_VERTEX, kProgMesh, 1,
     {{"View", 0, 0, ZR_DESCRIPTOR_TYPE_UNIFORM_BUFFER, 1, ZR_SHADER_STAGE_VERTEX}},
     3, {{0, ZR_FORMAT_R32G32B32_SFLOAT}, {1, ZR_FORMAT_R32G32B32_SFLOAT}, {2, ZR_FORMAT_R32G32_SFLOAT}}},
    {"mesh.slang", "psmain", ZR_SHADER_STAGE_FRAGMENT, kProgMesh, 0, {}, 0, {}},
    // mesh_push.slang: the same program with view_proj in a 64-B push-constant
    // block (CommandEncoder::push_constants, command.rs:180-185) instead of View
    {"mesh_push.slang", "vsmain", ZR_SHADER_STAGE_VERTEX, kProgMesh, 0, {},
     3, {{0, ZR_FORMAT_R32G32B32_SFLOAT}, {1, ZR_FORMAT_R32G32B32_SFLOAT}, {2, ZR_FORMAT_R32G32_SFLOAT}}, 64},
    {"mesh_push.slang", "psmain", ZR_SHADER_STAGE_FRAGMENT, kProgMesh, 0, {}, 0, {}},
};

std::string basename_of(const char* path) {
    std::string p(path ? path : "");
    const size_t s = p.find_last_of("/\\");
    return s == std::string::npos ? p : p.substr(s + 1);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ buffers

static zr_result buffer_make(zr_device* d, const zr_buffer_desc* desc, void* ext, zr_buffer** out) {
    if (!d || !desc || !out) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    *out = nullptr;
    zr_result rc = set_device(d);
    if (rc) return rc;
    zr_buffer* b = new (std::nothrow) zr_buffer_t();
    if (!b) return fail(ZR_ERROR_OUT_OF_HOST_MEMORY, "buffer alloc");
    b->dev = d;
    b->size = desc->size;
    b->name = desc->name ? desc->name : "";
    b->external = ext != nullptr;
    if (ext) {
        b->ptr = ext;
    } else {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<uint64_t>(desc->size, 16));
        if (e != hipSuccess) {
            delete b;
            return fail(ZR_ERROR_OUT_OF_DEVICE_MEMORY, "hipMalloc failed for buffer " + std::string(desc->name ? desc->name : ""));
        }
        b->ptr = p;
    }
    *out = b;
    return ZR_SUCCESS;
}

ZR_API zr_result zr_buffer_create(zr_device* d, const zr_buffer_desc* desc, zr_buffer** out) {
    return buffer_make(d, desc, nullptr, out);
}

ZR_API zr_result zr_buffer_create_external(zr_device* d, const zr_buffer_desc* desc, void* ptr, zr_buffer** out) {
    if (!ptr) return fail(ZR_ERROR_VALIDATION_FAILED, "external pointer is NULL");
    return buffer_make(d, desc, ptr, out);
}

ZR_API void zr_buffer_destroy(zr_buffer* b) {
    if (!b) return;
    device_sync(b->dev);
    if (!b->external) (void)hipFree(b->ptr);
    delete b;
}

ZR_API zr_result zr_buffer_write(zr_buffer* b, uint64_t offset, const void* src, uint64_t size) {
    if (!b) return fail(ZR_ERROR_VALIDATION_FAILED, "buffer is NULL");
    if (size == 0) return ZR_SUCCESS;  // buffer.rs:301-303
    if (offset > b->size || size > b->size - offset)
        return fail(ZR_ERROR_OUT_OF_DEVICE_MEMORY, "write past the end of buffer '" + b->name + "'");
    zr_result rc = device_sync(b->dev);
    if (rc) return rc;
    ZR_HIP(hipMemcpyAsync((uint8_t*)b->ptr + offset, src, size, hipMemcpyHostToDevice, b->dev->stream));
    ZR_HIP(hipStreamSynchronize(b->dev->stream));
    return ZR_SUCCESS;
}

ZR_API zr_result zr_buffer_read(zr_buffer* b, uint64_t offset, void* dst, uint64_t size) {
    if (!b) return fail(ZR_ERROR_VALIDATION_FAILED, "buffer is NULL");
    if (offset > b->size || size > b->size - offset) return fail(ZR_ERROR_VALIDATION_FAILED, "read out of range");
    zr_result rc = device_sync(b->dev);
    if (rc) return rc;
    ZR_HIP(hipMemcpyAsync(dst, (const uint8_t*)b->ptr + offset, size, hipMemcpyDeviceToHost, b->dev->stream));
    ZR_HIP(hipStreamSynchronize(b->dev->stream));
    return ZR_SUCCESS;
}

ZR_API uint64_t zr_buffer_size(const zr_buffer* b) { return b ? b->size : 0; }
ZR_API void* zr_buffer_device_address(const zr_buffer* b) { return b ? b->ptr : nullptr; }

// ----------------------------------------------------------------- textures

static zr_result texture_make(zr_device* d, const zr_texture_desc* desc, void* ext, zr_texture** out) {
    if (!d || !desc || !out) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    *out = nullptr;
    uint32_t bpp = desc->format == ZR_FORMAT_D32_SFLOAT ? 4u : format_bpp(desc->format);
    if (!bpp) return fail(ZR_ERROR_FORMAT_NOT_SUPPORTED, "unsupported texture format");
    if (desc->width == 0 || desc->height == 0) return fail(ZR_ERROR_VALIDATION_FAILED, "zero extent");
    zr_result rc = set_device(d);
    if (rc) return rc;
    zr_texture* t = new (std::nothrow) zr_texture_t();
    if (!t) return fail(ZR_ERROR_OUT_OF_HOST_MEMORY, "texture alloc");
    t->dev = d;
    t->width = desc->width;
    t->height = desc->height;
    t->format = desc->format;
    t->bpp = bpp;
    t->external = ext != nullptr;
    t->name = desc->name ? desc->name : "";
    if (ext) {
        t->ptr = ext;
    } else {
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)desc->width * desc->height * bpp) != hipSuccess) {
            delete t;
            return fail(ZR_ERROR_OUT_OF_DEVICE_MEMORY, "hipMalloc failed for texture");
        }
        t->ptr = p;
    }
    *out = t;
    return ZR_SUCCESS;
}

ZR_API zr_result zr_texture_create(zr_device* d, const zr_texture_desc* desc, zr_texture** out) {
    return texture_make(d, desc, nullptr, out);
}

ZR_API zr_result zr_texture_create_external(zr_device* d, const zr_texture_desc* desc, void* ptr, zr_texture** out) {
    if (!ptr) return fail(ZR_ERROR_VALIDATION_FAILED, "external pointer is NULL");
    return texture_make(d, desc, ptr, out);
}

ZR_API void zr_texture_destroy(zr_texture* t) {
    if (!t) return;
    device_sync(t->dev);
    if (!t->external) (void)hipFree(t->ptr);
    if (t->gather_done) (void)hipEventDestroy(t->gather_done);
    delete t;
}

ZR_API zr_result zr_texture_read(zr_texture* t, void* dst, uint64_t size) {
    if (!t || !dst) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    const uint64_t bytes = (uint64_t)t->width * t->height * t->bpp;
    if (size < bytes) return fail(ZR_ERROR_VALIDATION_FAILED, "destination too small");
    zr_result rc = device_sync(t->dev);
    if (rc) return rc;
    ZR_HIP(hipMemcpyAsync(dst, t->ptr, bytes, hipMemcpyDeviceToHost, t->dev->stream));
    ZR_HIP(hipStreamSynchronize(t->dev->stream));
    return ZR_SUCCESS;
}

ZR_API zr_result zr_texture_write(zr_texture* t, const void* src, uint64_t size) {
    if (!t || !src) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    const uint64_t bytes = (uint64_t)t->width * t->height * t->bpp;
    if (size < bytes) return fail(ZR_ERROR_VALIDATION_FAILED, "source too small");
    zr_result rc = device_sync(t->dev);
    if (rc) return rc;
    ZR_HIP(hipMemcpyAsync(t->ptr, src, bytes, hipMemcpyHostToDevice, t->dev->stream));
    ZR_HIP(hipStreamSynchronize(t->dev->stream));
    return ZR_SUCCESS;
}

ZR_API void* zr_texture_device_address(const zr_texture* t) { return t ? t->ptr : nullptr; }

// ------------------------------------------------------------------ shaders

ZR_API zr_result zr_shader_lookup(zr_device* d, const char* path, const char* entry, uint32_t stage, zr_shader** out) {
    (void)d;
    if (!out || !path || !entry) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    *out = nullptr;
    const std::string base = basename_of(path);
    for (const auto& s : kShaders) {
        if (base == s.file && !strcmp(entry, s.entry) && stage == s.stage) {
            zr_shader* sh = new (std::nothrow) zr_shader_t();
            if (!sh) return fail(ZR_ERROR_OUT_OF_HOST_MEMORY, "shader alloc");
            sh->program = s.program;
            sh->stage = s.stage;
            sh->file = s.file;
            sh->entry = s.entry;
            sh->bindings.assign(s.bind, s.bind + s.nbind);
            sh->inputs.assign(s.inputs, s.inputs + s.ninputs);
            sh->push_constant_size = s.push_size;
            *out = sh;
            return ZR_SUCCESS;
        }
    }
    return fail(ZR_ERROR_SHADER_NOT_FOUND, "no built-in stage for " + base + ":" + entry);
}

ZR_API void zr_shader_destroy(zr_shader* sh) { delete sh; }

ZR_API int32_t zr_shader_bindings(const zr_shader* sh, zr_shader_binding* out, int32_t capacity) {
    if (!sh) return 0;
    const int32_t n = (int32_t)sh->bindings.size();
    for (int32_t i = 0; out && i < std::min(n, capacity); ++i) out[i] = sh->bindings[i];
    return n;
}

ZR_API uint32_t zr_shader_push_constant_size(const zr_shader* sh) { return sh ? sh->push_constant_size : 0u; }

ZR_API int32_t zr_shader_vertex_inputs(const zr_shader* sh, zr_vertex_input_attr* out, int32_t capacity) {
    if (!sh) return 0;
    const int32_t n = (int32_t)sh->inputs.size();
    for (int32_t i = 0; out && i < std::min(n, capacity); ++i) out[i] = sh->inputs[i];
    return n;
}

// ---------------------------------------------------------------- pipelines

// validate_vertex_inputs, zenith-rhi/src/pipeline.rs:228-287 (strict match).
static zr_result validate_vertex_inputs(const zr_shader* vs, const zr_vertex_attribute* attrs, uint32_t n,
                                        zr_pipeline_error* err) {
    if (vs->inputs.empty()) {
        if (n == 0) return ZR_SUCCESS;
        return fail(ZR_ERROR_VERTEX_INPUT_REFLECTION_MISSING,
                    "vertex shader reflection contains no vertex_inputs, but vertex_attributes were provided");
    }
    std::map<uint32_t, int32_t> expected, provided;
    for (const auto& vi : vs->inputs) expected[vi.location] = vi.format;
    for (uint32_t i = 0; i < n; ++i) {
        auto it = provided.find(attrs[i].location);
        if (it != provided.end()) {
            if (it->second != attrs[i].format) {
                if (err) *err = {attrs[i].location, it->second, attrs[i].format};
                return fail(ZR_ERROR_DUPLICATE_VERTEX_ATTRIBUTE_LOCATION,
                            "duplicate vertex attribute location: " + std::to_string(attrs[i].location));
            }
        } else {
            provided[attrs[i].location] = attrs[i].format;
        }
    }
    for (const auto& kv : expected) {
        auto it = provided.find(kv.first);
        if (it == provided.end()) {
            if (err) *err = {kv.first, kv.second, 0};
            return fail(ZR_ERROR_MISSING_VERTEX_ATTRIBUTE,
                        "missing vertex attribute for location " + std::to_string(kv.first));
        }
        if (it->second != kv.second) {
            if (err) *err = {kv.first, kv.second, it->second};
            return fail(ZR_ERROR_VERTEX_ATTRIBUTE_FORMAT_MISMATCH,
                        "vertex attribute format mismatch at location " + std::to_string(kv.first));
        }
    }
    for (const auto& kv : provided) {
        if (!expected.count(kv.first)) {
            if (err) *err = {kv.first, 0, kv.second};
            return fail(ZR_ERROR_UNEXPECTED_VERTEX_ATTRIBUTE,
                        "unexpected vertex attribute at location " + std::to_string(kv.first));
        }
    }
    return ZR_SUCCESS;
}

// The pipeline layout's push-constant ranges.  None given: one {ALL_GRAPHICS, 0,
// merged size} range when the size is > 0 (GraphicShaderInput::create_pipeline_layout,
// pipeline.rs:112-128).  Given: the VkPushConstantRange / VkPipelineLayoutCreateInfo
// valid usage (offset and size multiples of 4, size > 0, within
// maxPushConstantsSize, no stage in two ranges), and each stage's push-constant
// block [0, size) covered by ranges holding that stage (the pipeline's layout
// must match its shaders).
static zr_result push_constant_layout(const zr_graphic_pipeline_desc* desc, const zr_shader* vs, const zr_shader* fs,
                                      uint32_t merged, std::vector<zr_push_constant_range>& out) {
    out.clear();
    if (desc->push_constant_range_count == 0) {
        if (merged > kMaxPushBytes) return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "push-constant block larger than 128 bytes");
        if (merged) out.push_back(zr_push_constant_range{ZR_SHADER_STAGE_ALL_GRAPHICS, 0u, merged});
        return ZR_SUCCESS;
    }
    if (!desc->push_constant_ranges) return fail(ZR_ERROR_VALIDATION_FAILED, "push_constant_ranges is NULL");
    uint32_t stages_seen = 0;
    for (uint32_t i = 0; i < desc->push_constant_range_count; ++i) {
        const zr_push_constant_range& r = desc->push_constant_ranges[i];
        if ((r.offset & 3u) || (r.size & 3u) || r.size == 0 || r.offset >= kMaxPushBytes || r.size > kMaxPushBytes - r.offset)
            return fail(ZR_ERROR_VALIDATION_FAILED, "push-constant range " + std::to_string(i) +
                                                        ": offset/size not multiples of 4, empty, or past 128 bytes");
        if (r.stage_flags == 0 || (r.stage_flags & ~(uint32_t)ZR_SHADER_STAGE_ALL_GRAPHICS))
            return fail(ZR_ERROR_VALIDATION_FAILED, "push-constant range " + std::to_string(i) + ": bad stage flags");
        if (stages_seen & r.stage_flags)
            return fail(ZR_ERROR_VALIDATION_FAILED, "a shader stage is in more than one push-constant range");
        stages_seen |= r.stage_flags;
        out.push_back(r);
    }
    for (const zr_shader* sh : {vs, fs}) {
        if (!sh || sh->push_constant_size == 0) continue;
        for (uint32_t w = 0; w < sh->push_constant_size / 4u; ++w) {
            bool covered = false;
            for (const auto& r : out)
                covered = covered || ((r.stage_flags & sh->stage) && w * 4u >= r.offset && w * 4u < r.offset + r.size);
            if (!covered)
                return fail(ZR_ERROR_VALIDATION_FAILED, "the layout's push-constant ranges do not cover the " +
                                                            std::string(sh->stage == ZR_SHADER_STAGE_VERTEX ? "vertex" : "fragment") +
                                                            " stage's push-constant block");
        }
    }
    return ZR_SUCCESS;
}

ZR_API zr_result zr_pipeline_create(zr_device* d, const zr_graphic_pipeline_desc* desc, zr_pipeline** out,
                                    zr_pipeline_error* err) {
    (void)d;
    if (!desc || !out) return fail(ZR_ERROR_VALIDATION_FAILED, "NULL argument");
    *out = nullptr;
    if (err) *err = {0, 0, 0};
    const zr_shader* vs = desc->vertex_shader;
    const zr_shader* fs = desc->fragment_shader;
    if (!vs) return fail(ZR_ERROR_MISSING_VERTEX_SHADER, "missing vertex shader");
    if (vs->stage != ZR_SHADER_STAGE_VERTEX || (fs && fs->stage != ZR_SHADER_STAGE_FRAGMENT))
        return fail(ZR_ERROR_VALIDATION_FAILED, "shader stage mismatch");
    zr_result rc = validate_vertex_inputs(vs, desc->vertex_attributes, desc->vertex_attribute_count, err);
    if (rc) return rc;
    if (fs && fs->program != vs->program)
        return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "vertex and fragment stages come from different programs");
    if (desc->topology != 3) return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "only TRIANGLE_LIST is supported");
    if (desc->rasterization.polygon_mode != 0) return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "only FILL polygon mode");
    if (desc->rasterization.depth_clamp || desc->rasterization.depth_bias_enable)
        return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "depth clamp / depth bias not supported");
    if (desc->samples > 1) return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "only 1x multisampling");
    if (desc->color_attachment_count > 1) return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "at most one colour attachment");
    zr_pipeline* p = new (std::nothrow) zr_pipeline_t();
    if (!p) return fail(ZR_ERROR_OUT_OF_HOST_MEMORY, "pipeline alloc");
    p->program = vs->program;
    p->has_fs = fs != nullptr;
    p->color_count = desc->color_attachment_count;
    p->color = zr_color_attachment_desc{};
    p->color.write_mask = 0xF;
    p->color_format = 0;
    if (p->color_count) {
        p->color = desc->color_attachments[0];
        p->color_format = desc->color_formats ? desc->color_formats[0] : 0;
        if (p->color.blend_enable) {
            delete p;
            return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "colour blending is not supported on this path");
        }
        if (p->color_format && format_bpp(p->color_format) == 0) {
            delete p;
            return fail(ZR_ERROR_FORMAT_NOT_SUPPORTED, "colour attachment format");
        }
    }
    p->depth_format = desc->depth_format;
    p->has_depth_state = desc->depth_stencil != nullptr;
    if (p->has_depth_state) {
        p->ds = *desc->depth_stencil;
        if (p->ds.stencil_test_enable || p->ds.depth_bounds_test_enable) {
            delete p;
            return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "stencil / depth-bounds tests are not supported");
        }
        if (p->ds.depth_write_enable && p->ds.depth_test_enable && p->ds.depth_compare_op == 5) {
            delete p;
            return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "NOT_EQUAL with depth writes is order dependent");
        }
    }
    p->cull_mode = desc->rasterization.cull_mode;
    p->front_face = desc->rasterization.front_face;
    // vertex layout: binding 0, per-vertex rate (VertexLayout derive, rhi-derive/src/lib.rs:126-131)
    p->stride = 0;
    for (uint32_t i = 0; i < desc->vertex_binding_count; ++i) {
        if (desc->vertex_bindings[i].binding == 0) {
            p->stride = desc->vertex_bindings[i].stride;
            if (desc->vertex_bindings[i].input_rate != 0) {
                delete p;
                return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "per-instance vertex input rate");
            }
        }
    }
    p->nattr = (uint32_t)vs->inputs.size();
    memset(p->attr_offset, 0, sizeof p->attr_offset);
    memset(p->attr_size, 0, sizeof p->attr_size);
    for (uint32_t i = 0; i < desc->vertex_attribute_count; ++i) {
        const auto& a = desc->vertex_attributes[i];
        if (a.binding != 0 || a.location >= 4 || (a.offset & 3u)) {
            delete p;
            return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "vertex attributes must live in binding 0, 4-byte aligned");
        }
        p->attr_offset[a.location] = a.offset;
        p->attr_size[a.location] = a.format == ZR_FORMAT_R32G32_SFLOAT ? 8u : a.format == ZR_FORMAT_R32_SFLOAT ? 4u
                                   : a.format == ZR_FORMAT_R32G32B32A32_SFLOAT ? 16u : 12u;
    }
    if (p->nattr && (p->stride == 0 || (p->stride & 3u))) {
        delete p;
        return fail(ZR_ERROR_FEATURE_NOT_PRESENT, "vertex binding 0 missing or stride not 4-byte aligned");
    }
    // ShaderReflection::merge (shader.rs:222-259): union by (set, binding), stage flags OR-ed
    std::map<std::pair<uint32_t, uint32_t>, zr_shader_binding> merged;
    for (const zr_shader* sh : {vs, fs}) {
        if (!sh) continue;
        for (const auto& b : sh->bindings) {
            auto key = std::make_pair(b.set, b.binding);
            auto it = merged.find(key);
            if (it == merged.end()) merged[key] = b;
            else it->second.stage_flags |= b.stage_flags;
        }
    }
    for (const auto& kv : merged) p->bindings.push_back(kv.second);
    // push constants: the merged size (the max over the stages, shader.rs:224-228)
    // and the layout's ranges -- derived as create_pipeline_layout does
    // (pipeline.rs:112-128), or the caller's, validated
    p->push_size = std::max(vs->push_constant_size, fs ? fs->push_constant_size : 0u);
    if ((rc = push_constant_layout(desc, vs, fs, p->push_size, p->push_ranges))) {
        delete p;
        return rc;
    }
    p->view_push = p->program == kProgMesh && vs->push_constant_size >= 64u;
    *out = p;
    return ZR_SUCCESS;
}

ZR_API void zr_pipeline_destroy(zr_pipeline* p) { delete p; }

ZR_API int32_t zr_pipeline_push_constant_ranges(const zr_pipeline* p, zr_push_constant_range* out, int32_t capacity) {
    if (!p) return 0;
    const int32_t n = (int32_t)p->push_ranges.size();
    for (int32_t i = 0; out && i < std::min(n, capacity); ++i) out[i] = p->push_ranges[i];
    return n;
}

}  // extern "C"
