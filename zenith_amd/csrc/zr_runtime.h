// zr_runtime.h — the objects behind the C ABI's handles, shared by the runtime's
// translation units: zr_runtime.cpp (device, draw execution, submission),
// zr_objects.cpp (buffers, textures, shaders, pipelines), zr_cmd.cpp (command
// recording) and zr_multi.cpp (gather / exchange plans, RCCL and replay exchange).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "zenith_raster.h"
#include "zr_internal.h"
#include "zr_plan.h"
#include "zr_rccl.h"

namespace zr {

// Records the thread's last error message (zr_last_error_message) and returns `code`.
zr_result fail(zr_result code, const std::string& msg);

#define ZR_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            return fail(_e == hipErrorOutOfMemory ? ZR_ERROR_OUT_OF_DEVICE_MEMORY : ZR_ERROR_DEVICE_LOST, \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                       \
        }                                                                                         \
    } while (0)

zr_result set_device(zr_device* d);
// A sync point: every stream idle, the status words read (stats, ShapeBook::end_interval).
zr_result device_sync(zr_device* d);
// The built-in exchange callbacks (zr_multi.cpp); exec_draw knows them by address.
zr_result rccl_exchange(void* user, void* stream, const void* send, void* recv, uint64_t bytes_per_rank);
zr_result replay_exchange(void* user, void* stream, const void* send, void* recv, uint64_t bytes_per_rank);

}  // namespace zr

struct zr_shader_t {
    int32_t program;
    uint32_t stage;
    std::string file, entry;
    std::vector<zr_shader_binding> bindings;
    std::vector<zr_vertex_input_attr> inputs;
    uint32_t push_constant_size = 0;
};

struct zr_buffer_t {
    zr_device* dev;
    void* ptr;
    uint64_t size;
    bool external;
    std::string name;
};

struct zr_texture_t {
    zr_device* dev;
    void* ptr;
    uint32_t width, height;
    int32_t format;
    uint32_t bpp;
    bool external;
    std::string name;
    // zr_device_gather_tile_rows: the gather that last read this texture (the
    // next render pass writing it waits for it on the device stream)
    hipEvent_t gather_done = nullptr;
    bool gather_pending = false;
};

struct zr_pipeline_t {
    int32_t program;
    bool has_fs;
    uint32_t stride;
    uint32_t nattr;
    uint32_t attr_offset[4];
    uint32_t attr_size[4];
    std::vector<zr_shader_binding> bindings;  // merged reflection
    uint32_t push_size = 0;                   // merged push_constant_size (shader.rs:224-228)
    std::vector<zr_push_constant_range> push_ranges;  // the layout's (pipeline.rs:112-128)
    bool view_push = false;                   // mesh program reading view_proj from push constants
    uint32_t cull_mode;
    int32_t front_face;
    bool has_depth_state;
    zr_depth_stencil_desc ds;
    uint32_t color_count;
    zr_color_attachment_desc color;
    int32_t color_format;
    int32_t depth_format;
};

enum CmdType { C_BEGIN_RENDERING, C_END_RENDERING, C_BIND_PIPELINE, C_BIND_UNIFORM, C_SET_VIEWPORT, C_SET_SCISSOR,
               C_BIND_VB, C_BIND_IB, C_DRAW, C_SET_SHARD, C_CLEAR_IMAGE, C_SET_ROUTE_CAP, C_PUSH_CONSTANTS };

struct RenderingState {
    zr_rect2d area;
    bool has_color = false, has_depth = false;
    zr_rendering_attachment color{}, depth{};
};

struct Cmd {
    CmdType type;
    RenderingState rendering;
    const zr_pipeline* pipeline = nullptr;
    const zr_buffer* buffer = nullptr;
    uint64_t offset = 0, range = 0;
    uint32_t a = 0, b = 0, c = 0, d = 0;
    int32_t e = 0;
    zr_viewport vp{};
    zr_rect2d rect{};
    zr_exchange_fn exchange = nullptr;  // C_SET_SHARD with a partitioned setup
    void* exchange_user = nullptr;
};

struct zr_cmd_t {
    zr_device* dev;
    std::vector<Cmd> cmds;
    std::vector<uint8_t> push_data;  // C_PUSH_CONSTANTS payloads (Cmd::offset indexes it)
    zr_result err = ZR_SUCCESS;
    std::string err_msg;
    bool in_rendering = false;
    bool has_exchange = false;  // a partitioned shard: its collective is called per submit, never captured
    // Replay of an unchanged command list: its launches captured once into a HIP
    // graph (valid while the device's scratch generation is unchanged).
    hipGraphExec_t graph = nullptr;
    uint64_t graph_gen = 0;
    uint32_t eager_runs = 0;
    void drop_graph() {
        if (graph) (void)hipGraphExecDestroy(graph);
        graph = nullptr;
    }
};

struct zr_fence_t {
    zr_device* dev;
    hipEvent_t ev;
    bool submitted = false;
};

// A grow-only device allocation (grow in zr_runtime.cpp); `cap` in elements.
struct ScratchBuf {
    void* ptr = nullptr;
    uint64_t cap = 0;
};

struct ScratchSet {
    ScratchBuf records, records_big;  // TriCompact / TriRecord per primitive
    ScratchBuf mesh_edges, bboxes;
    ScratchBuf tile_counts;
    ScratchBuf draw_info;   // k_setup_bin -> k_tile (kInfoWords)
    ScratchBuf counters;
    ScratchBuf bins;
    ScratchBuf runs;        // pool run table: [ntiles * run_cap] (DrawParams::runs)
    ScratchBuf run_counts;  // [ntiles] (zero between draws: k_tile resets it)
    ScratchBuf tile_order;  // k_tile's block -> tile schedule (k_setup_bin's last workgroup writes it)
    ScratchBuf job_slot;    // tile jobs (DrawParams::job_entries): key slot per split tile
    ScratchBuf job_keys;    // [slots][kTilePixels] per-job key buffers
    ScratchBuf job_tickets; // [slots], zero between draws
    ScratchBuf xsend, xrecv;  // partitioned setup: exchange blocks (bytes)
    ScratchBuf gids;        // draw primitive per received position (records mode)
    uint64_t xsend_layout = 0;  // (shard count, route capacity) the send headers were last zeroed for
    hipEvent_t setup_done = nullptr;  // k_setup_bin of the last draw that used this set
    hipEvent_t route_done = nullptr;  // partitioned draws: k_route + exchange of the last draw that used this set
    hipEvent_t tile_done = nullptr;   // k_tile of the last draw that used this set
    bool tile_done_valid = false;
    // a draw on the main stream alone used this set after tile_done was recorded:
    // the event is recorded on the main stream only when a setup-stream draw next
    // needs this set (an event record between two frames costs ~4.4 us of idle GPU)
    bool main_reader_pending = false;
};

struct TimedLaunch {
    const char* name;
    hipEvent_t start, stop;
};

struct zr_device_t {
    int hip_device = 0;
    hipStream_t stream = nullptr;
    // Scratch (grow-only) in sets: consecutive overlapped draws alternate, so the
    // setup of draw i+1 (on setup_stream) only waits for the last reader of its set
    // and runs while the tile pass of draw i finishes (DrawPlan::overlap).
    ScratchSet sets[zr::kScratchSets];
    uint32_t cur_set = 0;
    hipStream_t setup_stream = nullptr;
    // partitioned draws: k_route + the exchange on a stream of their own, so draw
    // i+2's route and exchange, draw i+1's records-mode binning (setup_stream) and
    // draw i's tile pass (main stream) run together: a three-stage pipeline over
    // three scratch sets
    hipStream_t route_stream = nullptr;
    zr::Knobs knobs;      // the ZR_* environment overrides
    zr::ShapeBook book;   // per-shape slab / job measurements and the buffer wants
    int cu_count = 0;
    uint32_t occupancy_checked_tiles = 0;
    bool occupancy_checked_mesh = false;
    uint32_t last_tile = zr::kTile;  // the tile edge of the last draw recorded
    unsigned long long* dbg_ts = nullptr;  // kDebugStamps
    uint32_t dbg_wgs = 0, dbg_tiles = 0;
    uint32_t* status_host = nullptr;
    uint32_t* status_dev = nullptr;
    // command lists submitted since the last sync point (in flight) + stats
    std::vector<zr_cmd*> pending;
    uint64_t overflowed_draws = 0;
    uint64_t route_fallbacks = 0;  // partitioned draws set up in full after a block overflow
    hipStream_t own_stream = nullptr;  // `stream` unless zr_device_set_stream installed the caller's
    // multi-GPU (zr_device_init_rccl): one communicator for the partitioned-setup
    // exchange (setup stream), one for the tile-row gather (gather stream), so an
    // exchange never queues behind the previous frame's gather
    void* comm_x = nullptr;
    void* comm_g = nullptr;
    int comm_rank = 0, comm_size = 1;
    hipStream_t gather_stream = nullptr;
    hipEvent_t frame_done = nullptr;
    uint8_t* gather_stage = nullptr;  // packed leftover-row rectangles of the row gather
    uint64_t gather_stage_cap = 0;
    zr_draw_stats last{};
    uint64_t last_prims = 0;
    // profiling (zr_device_set_profiling): 1 = per-kernel events, 2 = also the winner census
    bool profiling = false;
    int32_t census = 0;
    ScratchBuf win_bits;            // census bitmap of the last census draw (one bit per draw primitive; words)
    uint64_t census_words = 0;      // words of the last census draw, read at the next sync point
    bool capturing = false;     // inside hipStreamBeginCapture: no allocation allowed
    uint64_t scratch_gen = 0;   // bumped whenever a scratch buffer is reallocated
    std::vector<TimedLaunch> timed;
    std::vector<hipEvent_t> event_pool;
    std::map<std::string, std::pair<double, uint64_t>> times;
};
