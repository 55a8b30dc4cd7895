// rt_api.cpp — the C ABI of include/rt_hip.h: context, scene upload, frame / tile
// dispatch, read-back.  Replaces the reference's wgpu plumbing
// (src/buffers.rs:157-470 uploads, src/compute.rs:137-251 dispatch loop,
// src/renderer.rs:452-475 channel textures).  No CPU fallback: every compute entry point
// needs a HIP device and fails with RT_ERR_HIP otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt_hip.h"
#include "adaptive.h"
#include "bvh_builder.h"
#include "bvh_check.h"
#include "denoise.h"
#include "device_build.h"
#include "device_layout.h"
#include "half.h"
#include "kernels.h"
#include "ray_query.h"
#include "refit.h"
#include "shadow_grid.h"
#include "wavefront.h"

#ifndef RT_SINGLE_PASS_MAX_NODES
#define RT_SINGLE_PASS_MAX_NODES 64u /* "BVH depth <= 4" scenes of BASELINE configs[1]; larger scenes: measured in profiles/ab_r03.json */
#endif
#define RT_DEVICE_BUILD_MIN_TRIS 1024u /* below this the host build takes well under a millisecond */

namespace {

thread_local std::string g_create_error;

struct DeviceState {
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; // the second lane of the wavefront pipeline (batches alternate between the two)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_start = nullptr, ev_join = nullptr, ev_res[2] = {nullptr, nullptr};
    DevNode8* nodes = nullptr;
    DevTri* tris = nullptr;
    DevSphere* spheres = nullptr;
    DevLight* lights = nullptr;
    DevMaterial* materials = nullptr;
    float* rgba32f = nullptr;
    uint8_t* chan[3] = {nullptr, nullptr, nullptr};
    uint32_t* prim_id = nullptr;
    float* hit_t = nullptr;
    unsigned long long* counters = nullptr;
    uint32_t fb_w = 0, fb_h = 0;
    void* readback_dev = nullptr;  // epilogue output (combined rgba8 / packed rgb32f), whole-frame single-device reads
    void* readback_host = nullptr; // pinned staging for it
    size_t readback_bytes = 0;
    uint32_t tile_first = 0, tile_stride = 1, n_owned = 0; // of the last rt_render
    DevShadowGrid* grids = nullptr;                        // one per light (shadow_grid.h), null when no light has a grid
    std::vector<void*> grid_allocs;
    std::vector<rt::ShadowGridBuild> grid_info;
    bool grids_tried = false;                              // the light grids of the current scene were built (or refused) on this device
    rt::WfBuffers wf{};                                    // wavefront pipeline state (extended mode)
    rt::WfBuffers wf2{};                                   // ... of the second lane (its own path state, queues and counters; the pixel sums are shared)
    std::vector<void*> wf2_allocs;
    bool used_two_lanes = false; // the last pipeline frame ran on two lanes (its allocation is reused by a frame of the same shape)
    uint32_t wf_lights = 0;
    uint32_t wf_spp = 0; // spp the current wavefront allocation was sized for
    std::vector<hipEvent_t> stage_events; // RT_FLAG_STAGE_TIMES: event pairs around the launches of the dominant stage kernel
    uint32_t stage_events_used = 0;
    std::vector<void*> wf_allocs;
    void* rq_in = nullptr;  // ray queries: staging of host batches (rays in, hit records / bytes out), grown on demand
    void* rq_out = nullptr;
    size_t rq_in_bytes = 0, rq_out_bytes = 0;
    std::vector<hipEvent_t> rq_events; // an event pair around each launch of a query
    // rt_update_geometry (refit.h): the refit's view of the tree this device holds, made on the first update of that tree
    uint32_t* rf_vidx = nullptr;   // per triangle record: the caller's vertex indices (RT_REFIT_NO_RECORD: padding)
    uint32_t* rf_order = nullptr;  // node ids grouped by tree level (rt_ctx::rf_level_first)
    float4* rf_boxes = nullptr;    // exact box per node (min, max): scratch of the level launches
    uint32_t* rf_dropped = nullptr; // vertex indices of the triangles the tree has no record of (non-finite at upload)
    uint32_t* rf_flag = nullptr;
    float* rf_verts = nullptr;     // the positions of the last update (3 floats per vertex)
    // RT_FLAG_ACCUMULATE: the running sum of the context's accumulation over this device's pixels (DevTargets::run_sum), frame-pixel layout,
    // run_sum_w x run_sum_h x 16 bytes.  Outlives the pipeline's WfBuffers (re-sized with the batch); made by the first accumulating call, freed
    // with the scene
    float* run_sum = nullptr;
    uint32_t run_sum_w = 0, run_sum_h = 0;
    // rt_render_adaptive: the running sum over the odd-indexed samples (DevTargets::run_odd, same layout; made by the first adaptive call, freed
    // with run_sum), and the selection of a call (adaptive.h): per owned block its mask of pixels that take samples, the list of the blocks
    // with any (ad_cap entries each), the two counts k_ad_compact leaves on the device, and what the host read of them for the last call
    float* run_odd = nullptr;
    unsigned long long* ad_mask = nullptr;
    uint32_t* ad_blocks = nullptr;
    unsigned long long* ad_counts = nullptr;
    uint32_t ad_cap = 0;
    uint32_t ad_live_blocks = 0;
    uint64_t ad_pixels = 0;
    // rt_aovs / rt_denoise (denoise.h), grown on demand, kept until rt_destroy (they do not depend on the scene): the records of the
    // device's share when they cannot be written in place, the staging of host rgb, and the two colour planes of the a-trous iterations
    void* dn_aov = nullptr;
    void* dn_rgb = nullptr;
    void* dn_plane[2] = {nullptr, nullptr};
    size_t dn_aov_bytes = 0, dn_rgb_bytes = 0, dn_plane_bytes[2] = {0, 0};
};

// What an accumulating rt_render must share with the previous one to continue its running image (rt_hip.h, RT_FLAG_ACCUMULATE): the
// parameters that change the bits of a sample.  Compared bytewise (all 4-byte fields, no padding): the camera bit for bit.
struct AccumKey {
    rt_camera camera;
    uint32_t width, height, max_bounces, frame_seed, tile_size, tile_rank, tile_world, no_shadows;
    uint32_t adaptive; // the running image of rt_render_adaptive (per-pixel counts) is not continued by plain accumulating calls, nor the reverse
};

} // namespace

struct rt_ctx {
    std::vector<DeviceState> devs;
    std::string err;
    bool uploaded = false;
    bool pending_dispatch = false; // rt_dispatch_tile launches are not waited for (the reference's queue.submit is not either); see sync_pending
    DevScene scene_counts{}; // counts; pointers are per device
    rt_stats stats{};
    uint32_t frame_w = 0, frame_h = 0, frame_tile = RT_TILE_SIZE, frame_tiles_x = 0, frame_tiles_y = 0;
    bool frame_valid = false;
    unsigned long long diag[RT_CNT_N_DIAG] = {0}; // diagnostics of the counting kernel variant (rt_debug_counters)
    unsigned long long grid_diag[2] = {0}; // ... of the light grids: shadow segments they answered, list entries read
    double stage_ms[2] = {0.0, 0.0};       // RT_FLAG_STAGE_TIMES: [0] sum of the k_wf_shadow_grid launch durations of the last frame (device 0), [1] launches
    int fail_upload_at = -1;          // test hook: the next scene upload fails before its k-th device array (rt_debug_fail_upload)
    uint32_t n_input_tris = 0;        // triangles handed to the last scene upload (prim ids are < this)
    std::vector<rt::BuildTri> build_tris; // the triangles of the last upload as the builders take them (rt_prepare RT_PREPARE_QUALITY_TREE rebuilds from them)
    std::vector<DevLight> host_lights; // what the lazy light-grid build needs of the last upload: the lights, ...
    float box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0}; // ... the box of the triangles with finite vertices
    std::vector<rt_triangle> up_triangles; // the triangles of the last upload in build_tris order (rt_update_geometry gathers through them)
    std::vector<uint32_t> up_prim_ids;     // ... their prim ids when they are not the index (rt_upload_scene_packed)
    uint32_t up_vertices = 0;              // vertex count of the last upload
    bool rf_ready = false;                 // the devices hold the refit's view of the current tree (DeviceState::rf_*)
    std::vector<uint32_t> rf_level_first;  // rf_order offsets of the tree levels, root level first, plus the end
    uint32_t rf_n_dropped = 0;             // triangles without a record
    bool host_geometry_stale = false;      // build_tris / box_lo / box_hi lag behind device-resident positions in devs[0].rf_verts
    uint32_t n_textures = 0;          // bindings 6-7 as last handed over (rt_upload_textures); never sampled, like the reference
    uint64_t texture_bytes = 0;
    AccumKey acc_key{};               // RT_FLAG_ACCUMULATE: the parameters of the running image ...
    uint32_t acc_samples = 0;         // ... and its sample count (0: none; the next accumulating call starts at sample 0)

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

namespace {

#ifndef RT_WF_LANES_DEFAULT
#define RT_WF_LANES_DEFAULT 2 /* measured on the headline frame: 179.7 - 188.1 ms against 197.6 - 199.0 with one lane; 16 spp: 48.8 against 51.9 */
#endif

#define HIPCHK(ctx, call)                                                                                       \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess)                                                                                   \
            return (ctx)->fail(e_ == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, "%s failed: %s (%s:%d)", #call, \
                               hipGetErrorString(e_), __FILE__, __LINE__);                                     \
    } while (0)

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

void free_refit(DeviceState& d) { // the refit's view of a tree goes with the tree
    (void)hipSetDevice(d.device);
    for (void* p : {(void*)d.rf_vidx, (void*)d.rf_order, (void*)d.rf_boxes, (void*)d.rf_dropped, (void*)d.rf_flag}) (void)hipFree(p);
    d.rf_vidx = d.rf_order = d.rf_dropped = d.rf_flag = nullptr;
    d.rf_boxes = nullptr;
}

void free_grids(DeviceState& d) { // the light grids hold triangle records of one tree: built again when a frame or rt_prepare needs them
    (void)hipSetDevice(d.device);
    for (void* p : d.grid_allocs) (void)hipFree(p);
    d.grid_allocs.clear();
    d.grid_info.clear();
    d.grids = nullptr;
    d.grids_tried = false;
}

void free_scene(DeviceState& d) {
    (void)hipSetDevice(d.device);
    (void)hipFree(d.nodes); (void)hipFree(d.tris); (void)hipFree(d.spheres); (void)hipFree(d.lights); (void)hipFree(d.materials);
    d.nodes = nullptr; d.tris = nullptr; d.spheres = nullptr; d.lights = nullptr; d.materials = nullptr;
    free_grids(d);
    // the staging of the ray queries goes with the scene it was used for (released by the next upload and by rt_destroy)
    (void)hipFree(d.rq_in);
    (void)hipFree(d.rq_out);
    d.rq_in = d.rq_out = nullptr;
    d.rq_in_bytes = d.rq_out_bytes = 0;
    free_refit(d);
    (void)hipFree(d.rf_verts);
    d.rf_verts = nullptr;
    (void)hipFree(d.run_sum); // the running image of an accumulation ends with the scene it was rendered from
    (void)hipFree(d.run_odd);
    d.run_sum = d.run_odd = nullptr;
    d.run_sum_w = d.run_sum_h = 0;
    for (void* p : {(void*)d.ad_mask, (void*)d.ad_blocks, (void*)d.ad_counts}) (void)hipFree(p);
    d.ad_mask = nullptr;
    d.ad_blocks = nullptr;
    d.ad_counts = nullptr;
    d.ad_cap = 0;
}
void free_targets(DeviceState& d) {
    (void)hipSetDevice(d.device);
    (void)hipFree(d.rgba32f); (void)hipFree(d.chan[0]); (void)hipFree(d.chan[1]); (void)hipFree(d.chan[2]); (void)hipFree(d.prim_id); (void)hipFree(d.hit_t);
    d.rgba32f = nullptr; d.chan[0] = d.chan[1] = d.chan[2] = nullptr; d.prim_id = nullptr; d.hit_t = nullptr;
    d.fb_w = d.fb_h = 0;
    (void)hipFree(d.readback_dev);
    if (d.readback_host) (void)hipHostFree(d.readback_host);
    d.readback_dev = d.readback_host = nullptr;
    d.readback_bytes = 0;
}

void free_denoise(DeviceState& d) {
    (void)hipSetDevice(d.device);
    for (void* p : {d.dn_aov, d.dn_rgb, d.dn_plane[0], d.dn_plane[1]}) (void)hipFree(p);
    d.dn_aov = d.dn_rgb = d.dn_plane[0] = d.dn_plane[1] = nullptr;
    d.dn_aov_bytes = d.dn_rgb_bytes = d.dn_plane_bytes[0] = d.dn_plane_bytes[1] = 0;
}

void free_wavefront(DeviceState& d) {
    (void)hipSetDevice(d.device);
    for (void* p : d.wf_allocs) (void)hipFree(p);
    d.wf_allocs.clear();
    for (void* p : d.wf2_allocs) (void)hipFree(p);
    d.wf2_allocs.clear();
    d.wf2 = rt::WfBuffers{};
    d.wf = rt::WfBuffers{};
    d.wf_lights = 0;
}

template <class T>
int upload_array(rt_ctx* ctx, T** dst, const std::vector<T>& src) {
    *dst = nullptr;
    if (src.empty()) return RT_OK;
    HIPCHK(ctx, hipMalloc((void**)dst, src.size() * sizeof(T)));
    HIPCHK(ctx, hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

int ensure_targets(rt_ctx* ctx, DeviceState& d, uint32_t w, uint32_t h) {
    if (d.fb_w == w && d.fb_h == h && d.rgba32f) return RT_OK;
    if (d.stream) HIPCHK(ctx, hipStreamSynchronize(d.stream)); // dispatches in flight may still write the old targets
    free_targets(d);
    HIPCHK(ctx, hipSetDevice(d.device));
    size_t n = (size_t)w * h;
    HIPCHK(ctx, hipMalloc((void**)&d.rgba32f, n * 16));
    for (int c = 0; c < 3; c++) HIPCHK(ctx, hipMalloc((void**)&d.chan[c], n * 4));
    HIPCHK(ctx, hipMalloc((void**)&d.prim_id, n * 4));
    HIPCHK(ctx, hipMalloc((void**)&d.hit_t, n * 4));
    // fresh textures read as zero, like newly created wgpu textures.  On d.stream: it is a non-blocking stream, so a
    // memset on the null stream would not be ordered against the kernels that write these targets next
    HIPCHK(ctx, hipMemsetAsync(d.rgba32f, 0, n * 16, d.stream));
    for (int c = 0; c < 3; c++) HIPCHK(ctx, hipMemsetAsync(d.chan[c], 0, n * 4, d.stream));
    HIPCHK(ctx, hipMemsetAsync(d.prim_id, 0xFF, n * 4, d.stream));
    HIPCHK(ctx, hipMemsetAsync(d.hit_t, 0, n * 4, d.stream));
    d.fb_w = w;
    d.fb_h = h;
    return RT_OK;
}

// Per-frame camera constants in the reference's operation order (shader/src/ray.rs:33-44;
// wavefront.rs:87-98 for mode 1, which uses the f32 resolution directly).
DevCamera make_camera(const rt_camera& cam, float res_x, float res_y, bool wavefront) {
    DevCamera c;
    float wf, hf;
    if (wavefront) {
        wf = res_x;
        hf = res_y;
    } else { // `resolution[i] as u32` then `as f32` (ray.rs:23-24, 28-29, 33)
        auto as_u32 = [](float f) -> uint32_t { return !(f > 0.0f) ? 0u : (f >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)f); };
        wf = (float)as_u32(res_x);
        hf = (float)as_u32(res_y);
    }
    c.width_f = wf;
    c.height_f = hf;
    c.aspect = wf / hf;
    c.fov_scale = tanf(cam.fov * 0.5f * 3.14159265358979323846f / 180.0f);
    const float* f = cam.direction;
    const float* u = cam.up;
    // glam cross: (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y)
    float r[3] = {f[1] * u[2] - u[1] * f[2], f[2] * u[0] - u[2] * f[0], f[0] * u[1] - u[0] * f[1]};
    float t[3] = {r[1] * f[2] - f[1] * r[2], r[2] * f[0] - f[2] * r[0], r[0] * f[1] - f[0] * r[1]};
    for (int a = 0; a < 3; a++) {
        c.origin[a] = cam.position[a];
        c.forward[a] = f[a];
        c.right[a] = r[a];
        c.true_up[a] = t[a];
    }
    return c;
}

DevScene scene_for(const rt_ctx* ctx, const DeviceState& d) {
    DevScene s = ctx->scene_counts;
    s.nodes = d.nodes;
    s.tris = d.tris;
    s.spheres = d.spheres;
    s.lights = d.lights;
    s.materials = d.materials;
    return s;
}

DevTargets targets_for(const DeviceState& d, const DevFrame& f) {
    DevTargets t;
    t.rgba32f = d.rgba32f;
    for (int c = 0; c < 3; c++) t.chan[c] = d.chan[c];
    t.prim_id = d.prim_id;
    t.hit_t = d.hit_t;
    t.counters = d.counters;
    t.run_sum = (f.flags & RT_FLAG_ACCUMULATE) ? d.run_sum : nullptr;
    t.run_odd = f.adaptive ? d.run_odd : nullptr;
    return t;
}

// The context's running image ends: the next accumulating rt_render starts at sample 0 (its buffers stay for it).  Called by the scene's
// owners (drop_scene, rt_update_geometry), by every frame or dispatch that is not an accumulating one, and by an accumulating call before
// its launches, so that a call that fails part way never leaves a half-added sum counted.
void end_accumulation(rt_ctx* ctx) { ctx->acc_samples = 0; }

// The running sums of an accumulating frame of width x height, one per device (its share of the pixels is written, the rest never read);
// an adaptive one (rt_render_adaptive) also has the odd-sample sums and the selection buffers for every block of the frame's tiling.
int ensure_run_sums(rt_ctx* ctx, const DevFrame& fr) {
    const uint32_t w = fr.width, h = fr.height;
    for (auto& d : ctx->devs) {
        HIPCHK(ctx, hipSetDevice(d.device));
        if (!(d.run_sum && d.run_sum_w == w && d.run_sum_h == h)) {
            if (d.stream) HIPCHK(ctx, hipStreamSynchronize(d.stream));
            (void)hipFree(d.run_sum);
            (void)hipFree(d.run_odd);
            d.run_sum = d.run_odd = nullptr;
            d.run_sum_w = d.run_sum_h = 0;
            HIPCHK(ctx, hipMalloc((void**)&d.run_sum, (size_t)w * h * 16)); // not cleared: a first call (sample_base 0) reads none of it
            d.run_sum_w = w;
            d.run_sum_h = h;
        }
        if (!fr.adaptive) continue;
        if (!d.run_odd) HIPCHK(ctx, hipMalloc((void**)&d.run_odd, (size_t)w * h * 16)); // (as run_sum: read only once written)
        const uint64_t all_blocks = (uint64_t)fr.tiles_x * fr.tiles_y * rt::blocks_per_tile(fr.tile_size); // a device owns at most all of them
        if (all_blocks > 0xFFFFFFFFull) return ctx->fail(RT_ERR_BAD_ARG, "rt_render_adaptive: %llu pixel blocks exceed 32-bit block indices", (unsigned long long)all_blocks);
        const uint32_t blocks = (uint32_t)all_blocks;
        if (d.ad_cap < blocks || !d.ad_counts) {
            if (d.stream) HIPCHK(ctx, hipStreamSynchronize(d.stream));
            for (void* p : {(void*)d.ad_mask, (void*)d.ad_blocks, (void*)d.ad_counts}) (void)hipFree(p);
            d.ad_mask = nullptr;
            d.ad_blocks = nullptr;
            d.ad_counts = nullptr;
            d.ad_cap = 0;
            HIPCHK(ctx, hipMalloc((void**)&d.ad_mask, (size_t)std::max(1u, blocks) * 8));
            HIPCHK(ctx, hipMalloc((void**)&d.ad_blocks, (size_t)std::max(1u, blocks) * 4));
            HIPCHK(ctx, hipMalloc((void**)&d.ad_counts, 2 * 8));
            d.ad_cap = blocks;
        }
    }
    return RT_OK;
}

int sync_pending(rt_ctx* ctx);
int sync_host_geometry(rt_ctx* ctx);

// Where the tree is built.  Default (method 2): ON the device (device_build.hip: Morton sort + PLOC + collapse + emission,
// a few milliseconds), as soon as the scene is large enough for that to matter; the host builders remain for tiny scenes, as
// the fallback when a device-built tree would be deeper than the kernels' stacks allow (degenerate inputs; the host build
// bounds its depth), and on request: RT_BUILD_METHOD=0 binned SAH + insertion-based optimisation (1 % faster frames, 0.35 s
// per 262 k triangles), 1 PLOC on the host (the statement the device build is checked against).
int tree_method(size_t n_tris) {
    int method = 2;
    if (const char* e = std::getenv("RT_BUILD_METHOD")) method = std::atoi(e);
    if (method == 2 && n_tris < RT_DEVICE_BUILD_MIN_TRIS) method = 0;
    return method;
}

// The tuning knobs of the tree an upload or a rebuild makes (development).
rt::BvhBuildOptions knob_build_options() {
    rt::BvhBuildOptions opt;
    if (const char* e = std::getenv("RT_BVH_COST_TRAVERSE")) opt.cost_traverse = (float)std::atof(e);
    if (const char* e = std::getenv("RT_BVH_MAX_LEAF")) opt.max_leaf = (uint32_t)std::atoi(e);
    if (const char* e = std::getenv("RT_BVH8_COST_TRAVERSE")) opt.cost_traverse8 = (float)std::atof(e);
    if (const char* e = std::getenv("RT_BUILD_REINSERT")) opt.reinsert = std::atoi(e) != 0;
    if (const char* e = std::getenv("RT_PLOC_RADIUS")) opt.ploc_radius = (uint32_t)std::atoi(e);
    return opt;
}

// A tree built for every device of the context, not yet handed over (install_tree).  Per device, `dev` holds the arrays of the
// device build, or the host build's once install_tree has copied them there; whatever was not handed over is freed with it.
struct TreeBuild {
    int method = 0; // as built: 2 device, 0 / 1 host (the device build falls back to 0)
    std::vector<int> device_ids; // of the context, in order
    std::vector<rt::DeviceBuild> dev;
    rt::BvhBuild bvh;
    uint32_t nodes = 0, tris = 0, depth = 0;

    explicit TreeBuild(const rt_ctx* ctx) {
        for (const DeviceState& d : ctx->devs) device_ids.push_back(d.device);
    }
    TreeBuild(const TreeBuild&) = delete;
    TreeBuild& operator=(const TreeBuild&) = delete;
    ~TreeBuild() { free_dev(); }
    void free_dev() {
        for (size_t j = 0; j < dev.size(); j++) {
            (void)hipSetDevice(device_ids[j]);
            (void)hipFree(dev[j].nodes);
            (void)hipFree(dev[j].tris);
        }
        dev.clear();
    }
};

// The build part of a scene upload, of rt_update_geometry's rebuild (`method` from tree_method, `opt` from knob_build_options) and
// of rt_prepare's quality tree (method 0, default options).
int build_tree(rt_ctx* ctx, const std::vector<rt::BuildTri>& bt, int method, rt::BvhBuildOptions opt, TreeBuild& tb) {
    opt.method = method == 1 ? 1 : 0;
    std::vector<rt::DeviceBuild>& dbuilds = tb.dev;
    rt::BvhBuild& bvh = tb.bvh;
    if (method == 2) {
        dbuilds.resize(ctx->devs.size());
        bool ok = true;
        for (size_t j = 0; j < ctx->devs.size() && ok; j++) {
            DeviceState& d = ctx->devs[j];
            HIPCHK(ctx, hipSetDevice(d.device));
            const hipError_t e = rt::device_build(bt.data(), bt.size(), opt, d.stream, &dbuilds[j]);
            ok = e == hipSuccess && dbuilds[j].depth <= RT_DEV_MAX_BVH_DEPTH && dbuilds[j].n_nodes <= RT_DEV_MAX_NODES &&
                 dbuilds[j].n_nodes == dbuilds[0].n_nodes && dbuilds[j].n_tris == dbuilds[0].n_tris;
        }
        if (!ok) { // fall back to the host build (depth bound, or the device ran out of memory for the temporaries)
            tb.free_dev();
            method = 0;
        } else {
            tb.nodes = dbuilds[0].n_nodes;
            tb.tris = dbuilds[0].n_tris;
            tb.depth = dbuilds[0].depth;
        }
    }
    if (method != 2) {
        rt::build_bvh(bt.data(), bt.size(), opt, bvh);
        if (bvh.depth > RT_DEV_MAX_BVH_DEPTH) return ctx->fail(RT_ERR_INTERNAL, "BVH depth %u exceeds the bound %d", bvh.depth, RT_DEV_MAX_BVH_DEPTH);
        if (bvh.nodes.size() > RT_DEV_MAX_NODES) return ctx->fail(RT_ERR_BAD_ARG, "scene needs %zu BVH nodes > %u", bvh.nodes.size(), RT_DEV_MAX_NODES);
        tb.nodes = (uint32_t)bvh.nodes.size();
        tb.tris = (uint32_t)bvh.tris.size();
        tb.depth = bvh.depth;
    }
    tb.method = method;
    return RT_OK;
}

uint64_t scene_bytes(const DevScene& s) { // rt_stats.scene_bytes of the arrays the counts describe
    return (uint64_t)s.n_nodes * sizeof(DevNode8) + (uint64_t)s.n_tris * sizeof(DevTri) + (uint64_t)s.n_spheres * sizeof(DevSphere) +
           (uint64_t)s.n_lights * sizeof(DevLight) + (uint64_t)s.n_materials * sizeof(DevMaterial);
}

void drop_grids(rt_ctx* ctx) {
    for (auto& d : ctx->devs) free_grids(d);
    ctx->stats.grid_bytes = 0;
    ctx->stats.grid_build_ms = 0.0;
}

// The context holds no scene: what a failed upload or update leaves, and where an upload starts.  The caller decides about frame_valid.
void drop_scene(rt_ctx* ctx) {
    for (auto& d : ctx->devs) {
        (void)hipSetDevice(d.device);
        (void)hipDeviceSynchronize(); // launches in flight may still read the scene
        free_scene(d);
    }
    ctx->uploaded = false;
    ctx->scene_counts = DevScene{};
    ctx->rf_ready = false;
    ctx->host_geometry_stale = false;
    end_accumulation(ctx);
}

int injected_oom(rt_ctx* ctx) { return ctx->fail(RT_ERR_OOM, "rt_upload: allocation failure injected by rt_debug_fail_upload"); }

// The one way a tree goes onto the devices (scene uploads, rt_prepare's quality tree, rt_update_geometry's rebuild).  Every device
// gets its new arrays before any old ones are freed, so a failure leaves the old tree in place on every device.  The light grids and
// the refit's view go with the old tree.  `fail_at`: the upload's test hook (rt_debug_fail_upload), 0 before the first device's node
// array, 1 before its triangle array.
int install_tree(rt_ctx* ctx, TreeBuild& tb, int fail_at = -1) {
    const bool copy = tb.dev.empty(); // a host build: copied to every device
    if (copy) tb.dev.resize(ctx->devs.size());
    for (size_t j = 0; j < ctx->devs.size(); j++) {
        HIPCHK(ctx, hipSetDevice(ctx->devs[j].device));
        if (j == 0 && fail_at == 0) return injected_oom(ctx);
        if (copy)
            if (int rc = upload_array(ctx, &tb.dev[j].nodes, tb.bvh.nodes)) return rc;
        if (j == 0 && fail_at == 1) return injected_oom(ctx);
        if (copy)
            if (int rc = upload_array(ctx, &tb.dev[j].tris, tb.bvh.tris)) return rc;
        // the copies went through the null stream and d.stream is non-blocking; launches in flight may still read the old tree
        HIPCHK(ctx, hipDeviceSynchronize());
    }
    drop_grids(ctx);
    for (size_t j = 0; j < ctx->devs.size(); j++) {
        DeviceState& d = ctx->devs[j];
        (void)hipSetDevice(d.device);
        (void)hipFree(d.nodes);
        (void)hipFree(d.tris);
        d.nodes = std::exchange(tb.dev[j].nodes, nullptr);
        d.tris = std::exchange(tb.dev[j].tris, nullptr);
        free_refit(d);
    }
    DevScene& sc = ctx->scene_counts;
    sc.n_nodes = tb.nodes;
    sc.n_tris = tb.tris;
    sc.stack_entries = 2u * tb.depth + 2u; // a visit parks at most two groups
    ctx->stats.scene_bytes = scene_bytes(sc);
    ctx->stats.bvh_nodes = tb.nodes;
    ctx->stats.bvh_depth = tb.depth;
    ctx->stats.tree_build = (uint32_t)tb.method;
    ctx->rf_ready = false;
    return RT_OK;
}

// The box of the triangles with finite vertices (the light grids' bounds).
void finite_box(const std::vector<rt::BuildTri>& bt, float box_lo[3], float box_hi[3]) {
    for (int a = 0; a < 3; a++) box_lo[a] = INFINITY, box_hi[a] = -INFINITY;
    for (const rt::BuildTri& t : bt) {
        const float* vs[3] = {t.v0, t.v1, t.v2};
        bool finite = true;
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) finite = finite && std::isfinite(vs[k][a]);
        if (!finite) continue;
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) box_lo[a] = std::min(box_lo[a], vs[k][a]), box_hi[a] = std::max(box_hi[a], vs[k][a]);
    }
}

int upload_common(rt_ctx* ctx, const rt_sphere* spheres, uint32_t n_spheres, const rt_light* lights, uint32_t n_lights,
                  const rt_vertex* vertices, uint32_t n_vertices, const std::vector<rt_triangle>& tris,
                  const std::vector<uint32_t>& prim_ids, const rt_material* materials, uint32_t n_materials) {
    if (int rcp = sync_pending(ctx)) return rcp; // dispatches in flight still read the old scene
    if (tris.size() > RT_DEV_MAX_TRIS) return ctx->fail(RT_ERR_BAD_ARG, "too many triangles: %zu > %u", tris.size(), RT_DEV_MAX_TRIS);
    std::vector<rt::BuildTri> bt(tris.size());
    for (size_t i = 0; i < tris.size(); i++) {
        const rt_triangle& t = tris[i];
        if (t.v0_index >= n_vertices || t.v1_index >= n_vertices || t.v2_index >= n_vertices)
            return ctx->fail(RT_ERR_BAD_ARG, "triangle %zu references vertex out of range (%u,%u,%u >= %u)", i, t.v0_index,
                             t.v1_index, t.v2_index, n_vertices);
        std::memcpy(bt[i].v0, vertices[t.v0_index].position, 12);
        std::memcpy(bt[i].v1, vertices[t.v1_index].position, 12);
        std::memcpy(bt[i].v2, vertices[t.v2_index].position, 12);
        bt[i].material_id = t.material_id;
        bt[i].prim_id = prim_ids.empty() ? (uint32_t)i : prim_ids[i];
    }
    TreeBuild tb(ctx);
    if (int rc = build_tree(ctx, bt, tree_method(bt.size()), knob_build_options(), tb)) return rc;

    std::vector<DevSphere> ds(n_spheres);
    for (uint32_t i = 0; i < n_spheres; i++) {
        std::memcpy(ds[i].center, spheres[i].center, 12);
        ds[i].radius = spheres[i].radius;
        ds[i].material_id = spheres[i].material_id;
        ds[i]._pad[0] = ds[i]._pad[1] = ds[i]._pad[2] = 0;
    }
    std::vector<DevLight> dl(n_lights);
    for (uint32_t i = 0; i < n_lights; i++) {
        std::memcpy(dl[i].position, lights[i].position, 12);
        dl[i].light_type = lights[i].light_type;
        std::memcpy(dl[i].color, lights[i].color, 12);
        dl[i].intensity = lights[i].intensity;
        std::memcpy(dl[i].direction, lights[i].direction, 12);
        dl[i]._pad = 0;
        { // -normalize(direction): glam scalar-math normalize = v * (1 / sqrt(dot(v, v))), dot = (x*x + y*y) + z*z; this file is built -ffp-contract=off
            const float* v = lights[i].direction;
            const volatile float len2 = (v[0] * v[0]) + (v[1] * v[1]) + (v[2] * v[2]);
            const volatile float inv = 1.0f / std::sqrt(len2);
            for (int a = 0; a < 3; a++) dl[i].neg_ndir[a] = -(v[a] * inv);
            dl[i]._pad2 = 0;
        }
    }
    std::vector<DevMaterial> dm(n_materials);
    for (uint32_t i = 0; i < n_materials; i++) { // MaterialEvaluator accessors, shader/src/material.rs:16-63
        const rt_material& m = materials[i];
        std::memcpy(dm[i].albedo, m.albedo, 12);
        std::memcpy(dm[i].emission, m.emission, 12);
        dm[i].metallic = rt::f16_bits_to_f32((uint16_t)(m.metallic_roughness_f16 & 0xFFFF));
        dm[i].roughness = rt::f16_bits_to_f32((uint16_t)(m.metallic_roughness_f16 >> 16));
        dm[i].ior = rt::f16_bits_to_f32((uint16_t)(m.ior_transmission_f16 & 0xFFFF));
        dm[i].transmission = rt::f16_bits_to_f32((uint16_t)(m.ior_transmission_f16 >> 16));
        dm[i]._pad[0] = dm[i]._pad[1] = 0.0f;
    }

    // From here on the old scene is gone: the context counts as "nothing uploaded" until EVERY device holds the whole new
    // scene, so a failure half way (out of memory on the triangles, or on the second device) leaves no stale counts
    // pointing at freed or partly filled arrays - the next rt_render answers RT_ERR_NOT_UPLOADED.
    const rt_stats kept = ctx->stats; // what a failed upload leaves in rt_stats
    drop_scene(ctx);
    ctx->frame_valid = false;
    DevScene& sc = ctx->scene_counts;
    sc.n_spheres = n_spheres;
    sc.n_lights = n_lights;
    sc.n_materials = n_materials;
    ctx->stats = rt_stats{};
    ctx->stats.node_bytes = sizeof(DevNode8);
    ctx->stats.tri_bytes = sizeof(DevTri);
    ctx->stats.n_devices = (uint32_t)ctx->devs.size();
    ctx->stats.n_textures = ctx->n_textures;
    ctx->stats.texture_bytes = ctx->texture_bytes;
    const int fail_at = std::exchange(ctx->fail_upload_at, -1); // the test hook is one-shot
    auto upload_rest = [&](DeviceState& d) -> int {
        HIPCHK(ctx, hipSetDevice(d.device));
        if (&d == &ctx->devs[0] && fail_at == 2) return injected_oom(ctx);
        int rc;
        if ((rc = upload_array(ctx, &d.spheres, ds)) != RT_OK) return rc;
        if ((rc = upload_array(ctx, &d.lights, dl)) != RT_OK) return rc;
        if ((rc = upload_array(ctx, &d.materials, dm)) != RT_OK) return rc;
        // the copies went through the null stream and d.stream is non-blocking: make the order explicit
        HIPCHK(ctx, hipDeviceSynchronize());
        return RT_OK;
    };
    int rc = install_tree(ctx, tb, fail_at);
    for (auto& d : ctx->devs)
        if (rc == RT_OK) rc = upload_rest(d);
    if (rc != RT_OK) {
        drop_scene(ctx);
        ctx->stats = kept;
        return rc;
    }
    ctx->n_input_tris = (uint32_t)bt.size();
    ctx->build_tris.swap(bt);
    ctx->up_triangles = tris;
    ctx->up_prim_ids = prim_ids;
    ctx->up_vertices = n_vertices;
    ctx->host_lights = dl; // the light grids of the extended mode's shadow stage are built when a frame first needs them (ensure_grids)
    finite_box(ctx->build_tris, ctx->box_lo, ctx->box_hi);
    ctx->uploaded = true;
    return RT_OK;
}

// Per-light triangle lists for the shadow segments of the wavefront pipeline (shadow_grid.h), rasterised on the device from the
// triangle records of the uploaded scene.  LAZY: the reference's flow (src/scene.rs:87-119 replace_with_gltf, then
// src/compute.rs:12-50 every frame) only ever renders modes 0/1, which trace no shadow segments, so rt_upload_scene* builds
// nothing; the first extended-mode frame that traces shadow segments through the pipeline pays the build once per scene (or the
// caller asks for it ahead of time: rt_prepare).  rt_stats reports what it cost (grid_build_ms) and holds (grid_bytes).
// RT_SHADOW_GRID=0 and the RT_SHADOW_GRID_* variables are development knobs only.
int ensure_grids(rt_ctx* ctx, DeviceState& d) {
    if (d.grids_tried) return RT_OK;
    if (int rc = sync_host_geometry(ctx)) return rc; // box_lo / box_hi of positions an update left on the device
    d.grids_tried = true;
    const uint32_t n_lights = (uint32_t)ctx->host_lights.size(), tree_tris = ctx->scene_counts.n_tris;
    bool grids_on = true;
    rt::ShadowGridOptions gopt;
    if (const char* e = std::getenv("RT_SHADOW_GRID")) grids_on = std::atoi(e) != 0;
    if (const char* e = std::getenv("RT_SHADOW_GRID_RES")) gopt.res_point = (uint32_t)std::atoi(e), gopt.res_dir = 2u * (uint32_t)std::atoi(e);
    if (const char* e = std::getenv("RT_SHADOW_GRID_HEAVY")) gopt.heavy = (uint32_t)std::atoi(e);
    if (const char* e = std::getenv("RT_SHADOW_GRID_MEAN")) gopt.max_mean_list = std::atof(e), gopt.max_heavy_share = 1.0; // (forces grids onto cluttered scenes)
    if (!grids_on || n_lights == 0 || n_lights > RT_WF_MAX_LIGHTS || tree_tris == 0) return RT_OK;
    const double t0 = now_ms();
    HIPCHK(ctx, hipSetDevice(d.device));
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    std::vector<DevShadowGrid> hg(n_lights);
    bool any = false;
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    // all grids together may take a quarter of what is free now - cell blocks (128 bytes per cell: 0.8 GB per cube map at 1024 cells
    // per face side) AND list entries count against it (only the entries did); a light whose grid would not fit gets none
    rt::ShadowGridOptions lopt = gopt;
    lopt.max_bytes = free_b / 4 / n_lights;
    lopt.max_entries = std::min<uint64_t>(gopt.max_entries, lopt.max_bytes / (RT_SG_ENTRY_QUADS * sizeof(uint4)));
    // an error return below frees what was built; grids_tried stays set, so the following frames render without grids and do not try again
    struct Guard {
        DeviceState& d;
        bool ok = false;
        ~Guard() { if (!ok) { free_grids(d); d.grids_tried = true; } }
    } guard{d};
    uint64_t bytes = 0;
    bool partial = false; // a light that has triangles to cast shadows was left without a grid: then no light keeps its grid
    for (uint32_t i = 0; i < n_lights; i++) {
        rt::ShadowGridBuild gb;
        const hipError_t e = rt::shadow_grid_build(d.tris, tree_tris, ctx->host_lights[i], ctx->box_lo, ctx->box_hi, lopt, d.stream, &gb);
        if (e != hipSuccess) { // out of memory for a grid is not an error: the BVH answers for this light
            (void)hipGetLastError();
            gb = rt::ShadowGridBuild{};
        }
        hg[i] = gb.grid;
        if (gb.blocks) d.grid_allocs.push_back(gb.blocks);
        if (gb.overflow) d.grid_allocs.push_back(gb.overflow);
        if (gb.grid.kind != RT_SG_KIND_NONE) bytes += gb.bytes;
        any = any || gb.grid.kind != RT_SG_KIND_NONE;
        if (gb.grid.kind == RT_SG_KIND_NONE && gb.n_entries != 0) partial = true; // lists were counted and found too long (or too large): this light's segments walk the tree
        d.grid_info.push_back(gb);
    }
    if (any && partial) {
        // All lights or none.  The segments of a light without a grid are handed on one wave-load at a time, an atomic on the next queue's
        // counter each: a trickle when the lists leave 0.1 - 20 % to the tree, but with a whole light's segments it is millions of atomics
        // on one address per frame (bistro-like with one light of four on lists: 67 - 81 ms against 54 - 60 with no grids at all).
        HIPCHK(ctx, hipDeviceSynchronize());
        std::vector<rt::ShadowGridBuild> info = std::move(d.grid_info); // what the lists looked like stays readable (rt_debug_shadow_grid)
        free_grids(d);
        d.grids_tried = true;
        for (rt::ShadowGridBuild& g : info) g.grid = DevShadowGrid{}, g.blocks = g.overflow = nullptr, g.bytes = 0;
        d.grid_info = std::move(info);
        any = false;
        bytes = 0;
    }
    if (any) {
        const int rc = upload_array(ctx, &d.grids, hg);
        d.grid_allocs.push_back(d.grids); // (also when its copy failed)
        if (rc != RT_OK) return rc;
        HIPCHK(ctx, hipDeviceSynchronize());
    }
    if (&d == &ctx->devs[0]) { // (every device holds the same grids)
        ctx->stats.grid_bytes = bytes;
        ctx->stats.grid_build_ms = now_ms() - t0;
    }
    guard.ok = true;
    return RT_OK;
}

// Path-state arrays and queues of the wavefront pipeline, sized for `batch` samples per owned pixel block.
// `shrink`: an adaptive call (rt_render_adaptive), whose live blocks change from call to call, also runs in an allocation made for more
// blocks; it leaves the allocation's shape as it was (its lanes say how many blocks it covers, lane_of), so frames of that shape keep it.
int ensure_wavefront(rt_ctx* ctx, DeviceState& d, uint32_t n_blocks, uint32_t batch, uint32_t n_lights, bool two_lanes, bool shrink = false) {
    const uint32_t capacity = n_blocks * batch * 64u;
    // overflow entries (64-bit) per lane beyond the LDS part of the stack
    const uint32_t ovf_entries = ctx->scene_counts.stack_entries + 2u > RT_WF8_LDS_STACK ? ctx->scene_counts.stack_entries + 2u - RT_WF8_LDS_STACK : 1u;
    const bool same_shape = shrink ? d.wf.n_blocks >= n_blocks : (d.wf.n_blocks == n_blocks && d.wf.batch == batch);
    if (d.wf.capacity >= capacity && same_shape && d.wf_lights >= n_lights && d.wf.counters &&
        d.wf.ovf_entries >= ovf_entries && d.wf.stack_ovf && (!two_lanes || (d.wf2.counters && d.wf2.capacity >= capacity && d.wf2.stack_ovf)))
        return RT_OK;
    free_wavefront(d);
    HIPCHK(ctx, hipSetDevice(d.device));
    // an allocation that fails half way must not leave a lane that looks complete to the reuse test above
    struct Guard {
        DeviceState& d;
        bool ok = false;
        ~Guard() { if (!ok) free_wavefront(d); }
    } guard{d};
    for (int lane = 0; lane < (two_lanes ? 2 : 1); lane++) {
    std::vector<void*>& owned = lane ? d.wf2_allocs : d.wf_allocs;
    auto alloc = [&](void** p, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e == hipSuccess) owned.push_back(*p);
        return e;
    };
    rt::WfBuffers& w = lane ? d.wf2 : d.wf;
    const size_t P = capacity ? capacity : 64;
    // producers reserve queue space in windows (wavefront.hip): wf_queue_slots is the bound on real entries + padding
    const uint32_t lights = std::max(1u, n_lights);
    const size_t ext_slots = rt::wf_queue_slots(P, 1), shadow_slots = rt::wf_queue_slots(P * (size_t)lights, lights);
    if (ext_slots > 0xFFFFFFFFull || shadow_slots > 0xFFFFFFFFull)
        return ctx->fail(RT_ERR_INTERNAL, "wavefront queues of %zu / %zu slots exceed 32-bit positions", ext_slots, shadow_slots);
    // from depth 1 on a path's id is its extension queue position (k_wf_finish compacts): the arrays indexed by id hold S records, and
    // ids must fit the 27 bits they share with a light index in shadow queue entries (wavefront_max_paths keeps P small enough)
    const size_t S = std::min(rt::wf_state_slots(P), ext_slots);
    if (S > (size_t)RT_WF_ID_MASK + 1)
        return ctx->fail(RT_ERR_INTERNAL, "wavefront path ids of %zu slots exceed %u bits", S, 27u);
    HIPCHK(ctx, alloc((void**)&w.ray_o, S * 16));
    HIPCHK(ctx, alloc((void**)&w.ray_d, S * 16));
    HIPCHK(ctx, alloc((void**)&w.thr, S * 16));
    HIPCHK(ctx, alloc((void**)&w.rad, S * 16));
    HIPCHK(ctx, alloc((void**)&w.next_o, S * 16));
    HIPCHK(ctx, alloc((void**)&w.next_d, S * 16));
    HIPCHK(ctx, alloc((void**)&w.next_thr, S * 16));
    HIPCHK(ctx, alloc((void**)&w.next_rad, S * 16));
    HIPCHK(ctx, alloc((void**)&w.hit, S * 16));
    HIPCHK(ctx, alloc((void**)&w.vtx, S * 32));
    HIPCHK(ctx, alloc((void**)&w.sample_rad, P * 16));
    HIPCHK(ctx, alloc((void**)&w.pxy, P * 4));
    w.state_cap = (uint32_t)S;
    HIPCHK(ctx, alloc((void**)&w.q_ext[0], ext_slots * 4));
    HIPCHK(ctx, alloc((void**)&w.q_ext[1], ext_slots * 4));
    HIPCHK(ctx, alloc((void**)&w.q_shadow, shadow_slots * 4));
    HIPCHK(ctx, alloc((void**)&w.q_shadow2, (P * (size_t)lights + 64) * 4)); // written densely: one slot per entry
    w.q_ext_cap = (uint32_t)ext_slots;
    w.q_shadow_cap = (uint32_t)shadow_slots;
    HIPCHK(ctx, alloc((void**)&w.counters, rt::WF_N_COUNTERS * sizeof(uint32_t)));
    HIPCHK(ctx, alloc((void**)&w.totals, rt::WF_N_TOTALS * sizeof(unsigned long long)));
    if (lane == 0) HIPCHK(ctx, alloc((void**)&w.accum, (size_t)std::max(1u, n_blocks) * 64 * 16));
    else w.accum = d.wf.accum; // one running sum per pixel: the lanes' resolves are ordered by events
    if (lane == 0) { // the camera beams of the frame: per block a leaf list, built once per frame and read by both lanes
        HIPCHK(ctx, alloc((void**)&w.beam_count, ((size_t)std::max(1u, n_blocks) + 1) * 4));
        HIPCHK(ctx, alloc((void**)&w.beam_ref, (size_t)std::max(1u, n_blocks) * RT_BEAM_CAP * 4));
        HIPCHK(ctx, alloc((void**)&w.beam_dist, (size_t)std::max(1u, n_blocks) * RT_BEAM_CAP * 4));
    } else {
        w.beam_count = d.wf.beam_count;
        w.beam_ref = d.wf.beam_ref;
        w.beam_dist = d.wf.beam_dist;
    }
    HIPCHK(ctx, alloc((void**)&w.stack_ovf, (size_t)rt::wf_persistent_waves() * ovf_entries * 64 * 8));
    w.ovf_entries = ovf_entries;
    w.n_blocks = n_blocks;
    w.batch = batch;
    w.capacity = capacity;
    }
    d.wf_lights = n_lights;
    guard.ok = true;
    return RT_OK;
}

// Samples per pixel kept in flight by the wavefront pipeline.  Every stage of every bounce ends in a tail where
// the persistent waves drain, and late bounces carry few paths, so batches should be as large as memory allows:
// measured on the headline frame, 3 samples per batch (8 M paths) 4,640 Mrays/s, 32 per batch (71 M paths, 12 GB
// of the 288 GB while the path state was updated in place; ~21 GB per lane with compaction: two state sets over ~1.65 id slots per
// path slot) 5,840.  Target 64 M paths, bounded by half the free device memory, the 27-bit path id of a shadow
// queue entry and the 32-bit queue positions; the samples are then spread evenly over the batches.
// RT_WF_BATCH (samples per batch) / RT_WF_TARGET_PATHS override.
// Largest number of path slots the wavefront pipeline can address: 27-bit path ids in shadow queue entries - compacted ids are queue
// positions, padding included (wf_state_slots: ~88 M path slots on MI355X) - and 32-bit queue positions with up to 4 slots per
// (path, light) plus per-wave slack (wf_queue_slots).
uint64_t wavefront_max_paths(uint32_t n_lights) {
    static const uint64_t by_ids = [] { // the most path slots whose compacted ids fit 27 bits (wf_state_slots grows with P)
        uint64_t lo = 1, hi = (uint64_t)RT_WF_ID_MASK + 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) / 2;
            if (rt::wf_state_slots((size_t)mid) <= (uint64_t)RT_WF_ID_MASK + 1) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    }();
    const uint64_t lights = std::max(1u, n_lights);
    return std::min<uint64_t>(by_ids, (1ull << 29) / lights);
}

uint32_t wavefront_batch(uint32_t n_blocks, uint32_t spp, uint32_t n_lights, size_t free_bytes, bool two_lanes) {
    const uint64_t per_sample = std::max<uint64_t>(1, (uint64_t)n_blocks * 64u);
    const uint64_t hard_limit = std::max<uint64_t>(1, wavefront_max_paths(n_lights) / per_sample); // samples per batch the ids allow
    if (const char* e = std::getenv("RT_WF_BATCH")) {
        const uint32_t want = (uint32_t)std::strtoul(e, nullptr, 10);
        if (want) return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min(want, spp), hard_limit));
    }
    uint64_t target_paths = 64ull << 20;
    if (const char* e = std::getenv("RT_WF_TARGET_PATHS")) target_paths = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    const uint64_t lights = std::max(1u, n_lights);
    // path state indexed by id (two sets of ray_o / ray_d / thr / rad, hit, vtx: 176 bytes per record, wf_state_slots records = under 2 per path
    // slot for batches large enough that memory bounds them), sample_rad, pxy, two extension queues, shadow queue (4 slots per entry), the
    // handed-on shadow queue (dense)
    const uint64_t bytes_per_path = 2 * 11 * 16 + 16 + 4 + 2 * 16 + 16 * lights + 4 * lights;
    target_paths = std::min<uint64_t>(target_paths, free_bytes / 2 / bytes_per_path);
    target_paths = std::min<uint64_t>(target_paths, wavefront_max_paths(n_lights));
    uint32_t max_batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(spp, target_paths / per_sample));
    if (two_lanes && spp >= 2) max_batch = std::min(max_batch, (spp + 1) / 2); // two lanes want two batches, also of a frame that would fit one
    uint32_t n_batches = (spp + max_batch - 1) / max_batch;
    if (two_lanes && n_batches > 1 && (n_batches & 1u)) {
        // an even number of batches, so that both lanes get the same share (measured on the headline frame, round 3: 3 batches of 22/21/21
        // samples 176.8 ms, 2 of 32 170.9, 4 of 16 174.3): one batch fewer if that stays within a tenth of the target and the hard limits
        const uint32_t fewer = n_batches - 1, b = (spp + fewer - 1) / fewer;
        if ((uint64_t)b * per_sample * 10 <= target_paths * 11 && b <= hard_limit && (uint64_t)b * per_sample <= free_bytes / 2 / bytes_per_path) n_batches = fewer;
        else n_batches++;
    }
    return std::max(1u, (spp + n_batches - 1) / std::max(1u, n_batches));
}

// Largest tree (8-wide nodes) whose primary-rays-only frames take the one-pass kernel instead of the queue pipeline (run_frame).
uint32_t single_pass_max_nodes() {
    if (const char* e = std::getenv("RT_SINGLE_PASS_MAX_NODES")) return (uint32_t)std::strtoul(e, nullptr, 10); // development knob
    return RT_SINGLE_PASS_MAX_NODES;
}

// rt_dispatch_tile returns after the launch, like `queue.submit` in src/compute.rs:165.  Whatever needs the result or
// the device idle (read-back, statistics, a new scene, teardown) waits here first; the kernel time reported afterwards
// is that of the LAST dispatch.
int sync_pending(rt_ctx* ctx) {
    if (!ctx->pending_dispatch) return RT_OK;
    ctx->pending_dispatch = false;
    DeviceState& d = ctx->devs[0];
    HIPCHK(ctx, hipSetDevice(d.device));
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    float ms = 0.0f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, d.ev0, d.ev1));
    ctx->stats.kernel_ms = ms;
    return RT_OK;
}

// The tiles device j (of nd) takes of a frame: the context owns the tiles i with i % world == rank (rt_hip.h); its device j takes every
// nd-th of those.
void frame_share(DevFrame& f, uint32_t world, uint32_t rank, size_t nd, size_t j) {
    const uint32_t total_tiles = f.tiles_x * f.tiles_y, stride = world * (uint32_t)nd, first = rank + world * (uint32_t)j;
    f.tile_first = first;
    f.tile_stride = stride;
    f.n_owned_tiles = first < total_tiles ? (total_tiles - first + stride - 1) / stride : 0;
}
// ... and records it as the device's share of the last rt_render (what rt_read_* gather).
void assign_tiles(DevFrame& f, DeviceState& d, uint32_t world, uint32_t rank, size_t nd, size_t j) {
    frame_share(f, world, rank, nd, j);
    d.tile_first = f.tile_first;
    d.tile_stride = f.tile_stride;
    d.n_owned = f.n_owned_tiles;
}

struct KernelChoice {
    rt::FrameKernel kernel;
    bool fallback; // the default (the pipeline) was asked for and the frame did not fit it: RT_STAT_MEGAKERNEL_FALLBACK
};

// Which kernel renders one device's share `f` of a frame.  The flags choose first.  Primary rays only over a tiny tree (BASELINE
// configs[1]: Cornell, 12 triangles, max_bounces 0): the queue pipeline would move 132 bytes of path state per sample through six
// kernels for a closest hit that costs a few dozen instructions (measured 15.9 ms and 46.7 GB of HBM traffic per 1080p 64-spp frame);
// the nested-loop kernel loops the pixel's samples in registers, traces the closest hit and the per-light shadow segments inline and
// stores the pixel once: 2.6 ms, same bits (the per-sample order is fixed by the CPU statement).  SURVEY 7 step 6, shader/src/lib.rs:86-88
// (one write per pixel).  RT_FLAG_KERNEL_PIPELINE keeps the pipeline.  The pipeline needs one visibility bit per light and every path
// slot of ONE sample per owned pixel block addressable (wavefront_max_paths: the compacted path ids of a one-sample batch must fit
// 27 bits); anything else (more than 32 lights, a single device's share beyond ~88 M pixels, fewer with 7 or more lights) takes the
// state-machine megakernel.
KernelChoice choose_kernel(const rt_ctx* ctx, const DevFrame& f) {
    using rt::FrameKernel;
    const DevScene& sc = ctx->scene_counts;
    if (f.mode != RT_MODE_EXTENDED) return {FrameKernel::REFERENCE, false};
    if (f.flags & RT_FLAG_KERNEL_V1) return {FrameKernel::MEGAKERNEL_V1, false};
    if (f.flags & RT_FLAG_KERNEL_SM) return {FrameKernel::MEGAKERNEL_SM, false};
    if (!(f.flags & RT_FLAG_KERNEL_PIPELINE) && f.max_bounce == 0 && sc.n_nodes <= single_pass_max_nodes()) return {FrameKernel::SINGLE_PASS, false};
    const bool fits = sc.n_lights <= RT_WF_MAX_LIGHTS && (uint64_t)f.n_owned_tiles * rt::blocks_per_tile(f.tile_size) * 64u <= wavefront_max_paths(sc.n_lights);
    return fits ? KernelChoice{FrameKernel::PIPELINE, false} : KernelChoice{FrameKernel::MEGAKERNEL_SM, true};
}

// One device's walk through the batches and bounces of its share of a pipeline frame (setup_pipeline), one step at a time (run_frame).
struct WfRun {
    enum Phase { GENERATE, BOUNCE, RESOLVE, DONE };
    Phase phase = DONE;    // (from the start for a device whose share took another kernel)
    bool pipeline = false; // the device's share takes the pipeline
    size_t dev = 0;
    DevFrame f{};
    DevScene dsc{};
    uint32_t batch = 1, first = 0, j = 0, it = 0, alive = 0; // samples per batch, first sample and number of the batch, bounce, live paths
    uint32_t n_blocks = 0; // pixel blocks the walk covers (an adaptive call: the live ones, f.ad_blocks)
    bool two = false;   // batches alternate between the device's two lanes
    bool beams = false; // camera segments test their block's beam list (else they walk the tree)
    hipStream_t poll_stream = nullptr;
};

// Pipeline setup of one device's share `f` of a frame: light grids, lanes, batch, path-state allocation, the camera beams and the start of
// the second lane.  The launches of the batches follow in run_frame: a device's every-8-bounces read-back of its live paths must not hold
// back the launches of the next device.
int setup_pipeline(rt_ctx* ctx, size_t j, const DevFrame& f, WfRun& r) {
    DeviceState& d = ctx->devs[j];
    const uint32_t n_lights = ctx->scene_counts.n_lights;
    if (!(f.flags & (RT_FLAG_NO_SHADOW_GRID | RT_FLAG_NO_SHADOWS))) // the first frame that traces shadow segments through the pipeline builds the light grids
        if (int rc = ensure_grids(ctx, d)) return rc;
    // an adaptive call's pipeline covers the blocks k_ad_select listed (f.ad_blocks): path slots, queues and launches scale with the live pixels
    const uint32_t n_blocks = f.adaptive ? d.ad_live_blocks : f.n_owned_tiles * rt::blocks_per_tile(f.tile_size);
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    const char* lanes_env = std::getenv("RT_WF_LANES"); // (read per frame: tests and A/B runs switch it)
    // by default only for frames whose shadow stage runs on light grids: with the BVH walk both big stages are VALU-bound and sharing
    // the chip gains nothing (bistro-like 4K share: 136.7 ms on two lanes against 127.3 on one)
    bool two_lanes_on = lanes_env ? std::atoi(lanes_env) >= 2 : (RT_WF_LANES_DEFAULT >= 2 && d.grids != nullptr && !(f.flags & RT_FLAG_NO_SHADOW_GRID));
    // ... and not for a frame of long paths that fits ONE batch: two lanes would cut it in two, every launch would come twice, and
    // beyond four bounces most launches serve few paths and cost their latency whatever they serve (bistro-like 4K share, 64 spp,
    // 8 bounces, 66 M paths: one batch on one lane 105.3 ms, two of 32 samples on two lanes 116.7; 4 bounces: the two lanes win)
    if (!lanes_env && two_lanes_on && f.max_bounce > 4 && wavefront_batch(n_blocks, f.spp, n_lights, free_b, false) >= f.spp) two_lanes_on = false;
    const uint32_t batch = d.wf.n_blocks == n_blocks && d.wf_spp == f.spp && d.wf.batch && d.wf_lights >= n_lights && d.used_two_lanes == (two_lanes_on && f.spp >= 2) ? d.wf.batch // same frame shape as last time: keep the allocation
                                                                                               : wavefront_batch(n_blocks, f.spp, n_lights, two_lanes_on ? free_b / 2 : free_b, two_lanes_on);
    d.wf_spp = f.spp;
    // Two lanes (RT_WF_LANES=2, the default when a frame has two or more batches): batches alternate between two streams with their own
    // path state, so that one batch's shadow stage (bound by HBM bandwidth since the light grids) runs beside the other's closest-hit
    // traversal (bound by VALU issue).  The pixel sums are added in batch order: a resolve waits for the previous batch's.
    const uint32_t n_batches = (f.spp + batch - 1) / batch;
    const bool two = two_lanes_on && n_batches >= 2 && d.stream2;
    if (int rc = ensure_wavefront(ctx, d, n_blocks, batch, n_lights, two, f.adaptive != 0)) return rc;
    HIPCHK(ctx, hipMemsetAsync(d.wf.totals, 0, rt::WF_N_TOTALS * sizeof(unsigned long long), d.stream));
    if (!f.adaptive) HIPCHK(ctx, hipEventRecord(d.ev0, d.stream)); // re-record: allocation above is not part of the kernel time (an adaptive call's selection is)
    // camera beams: on by default, RT_WF_BEAMS=0 (development knob) or RT_FLAG_NO_BEAMS walks the tree for every camera segment
    const char* be = std::getenv("RT_WF_BEAMS");
    const bool beams = !(f.flags & RT_FLAG_NO_BEAMS) && (be ? std::atoi(be) != 0 : true);
    if (beams) {
        rt::WfBuffers wb = d.wf;
        wb.n_blocks = n_blocks; // (an adaptive call may run in an allocation made for more blocks)
        wb.batch = batch;
        HIPCHK(ctx, rt::wf_beams(scene_for(ctx, d), f, wb, d.stream));
    }
    if (two) {
        HIPCHK(ctx, hipEventRecord(d.ev_start, d.stream));
        HIPCHK(ctx, hipStreamWaitEvent(d.stream2, d.ev_start, 0));
        HIPCHK(ctx, hipMemsetAsync(d.wf2.totals, 0, rt::WF_N_TOTALS * sizeof(unsigned long long), d.stream2));
    }
    d.wf.grids = d.wf2.grids = (f.flags & RT_FLAG_NO_SHADOW_GRID) ? nullptr : d.grids;
    const char* pe = std::getenv("RT_WF_PROBE");
    d.wf.probe = d.wf2.probe = pe ? (uint32_t)std::atoi(pe) : 0u;
    d.used_two_lanes = two;
    r = WfRun{};
    r.phase = WfRun::GENERATE;
    r.pipeline = true;
    r.dev = j;
    r.f = f;
    r.dsc = scene_for(ctx, d);
    r.batch = batch;
    r.n_blocks = n_blocks;
    r.two = two;
    r.beams = beams;
    return RT_OK;
}

// The lane of r's current batch: its buffers (a copy: the kernels take them by value) and its stream.
struct WfLane { rt::WfBuffers w; hipStream_t st; };
WfLane lane_of(const DeviceState& d, const WfRun& r) {
    const bool second = r.two && (r.j & 1u);
    WfLane l{second ? d.wf2 : d.wf, second ? d.stream2 : d.stream};
    if (!r.beams) l.w.beam_count = nullptr;
    l.w.n_blocks = r.n_blocks; // (the allocation's own unless the walk is an adaptive call's)
    l.w.batch = r.batch;
    return l;
}
uint32_t batch_samples(const WfRun& r) { return std::min(r.batch, r.f.spp - r.first); }

// One step per phase of a pipeline walk, on the lane `l` of its current batch (the caller has made r's device current).
// GENERATE: the paths of the current batch.
int wf_step_generate(rt_ctx* ctx, DeviceState& d, WfRun& r, const WfLane& l) {
    HIPCHK(ctx, rt::wf_generate(r.dsc, r.f, l.w, targets_for(d, r.f), r.first, batch_samples(r), l.st));
    r.it = 0;
    r.phase = WfRun::BOUNCE;
    return RT_OK;
}

// BOUNCE: one bounce of the current batch.  After every 8th the live paths are read back and the device goes on `polls`: run_frame waits
// for them when every device has its next launches queued, and a batch of long paths stops as soon as every path has ended.
int wf_step_bounce(rt_ctx* ctx, DeviceState& d, WfRun& r, const WfLane& l, bool counters, std::vector<WfRun*>& polls) {
    hipEvent_t* gev = nullptr;
    if ((r.f.flags & RT_FLAG_STAGE_TIMES) && r.dev == 0 && rt::wf_runs_shadow_grid(r.f, l.w)) { // (bench.py: the dominant kernel's launch durations, measured live)
        if (d.stage_events.size() < (size_t)d.stage_events_used + 2) {
            hipEvent_t a = nullptr, b = nullptr;
            HIPCHK(ctx, hipEventCreate(&a));
            HIPCHK(ctx, hipEventCreate(&b));
            d.stage_events.push_back(a);
            d.stage_events.push_back(b);
        }
        gev = d.stage_events.data() + d.stage_events_used;
        d.stage_events_used += 2;
    }
    HIPCHK(ctx, rt::wf_bounce(r.dsc, r.f, l.w, r.it, batch_samples(r), counters, l.st, gev));
    if (r.it >= r.f.max_bounce) r.phase = WfRun::RESOLVE;
    else if ((r.it & 7u) == 7u) {
        HIPCHK(ctx, hipMemcpyAsync(&r.alive, l.w.counters + rt::WF_EXT_COUNT, 4, hipMemcpyDeviceToHost, l.st));
        r.poll_stream = l.st;
        polls.push_back(&r);
    } else r.it++;
    return RT_OK;
}

// RESOLVE: the batch's samples into the pixel sums, in batch order; after the last batch the frame ends when both lanes have.
int wf_step_resolve(rt_ctx* ctx, DeviceState& d, WfRun& r, const WfLane& l) {
    const uint32_t n = batch_samples(r);
    if (r.two && r.j > 0) HIPCHK(ctx, hipStreamWaitEvent(l.st, d.ev_res[(r.j - 1u) & 1u], 0));
    HIPCHK(ctx, rt::wf_resolve(r.f, l.w, targets_for(d, r.f), n, r.first, r.first == 0, r.first + n >= r.f.spp, l.st));
    if (r.two) HIPCHK(ctx, hipEventRecord(d.ev_res[r.j & 1u], l.st));
    r.first += r.batch;
    r.j++;
    if (r.first < r.f.spp) {
        r.phase = WfRun::GENERATE;
        return RT_OK;
    }
    if (r.two) {
        HIPCHK(ctx, hipEventRecord(d.ev_join, d.stream2));
        HIPCHK(ctx, hipStreamWaitEvent(d.stream, d.ev_join, 0));
    }
    if (r.f.adaptive) HIPCHK(ctx, rt::launch_ad_image(r.f, targets_for(d, r.f), d.stream));
    HIPCHK(ctx, hipEventRecord(d.ev1, d.stream));
    r.phase = WfRun::DONE;
    return RT_OK;
}

// What a frame took and counted, over the devices that rendered it.
struct FrameTotals {
    double kernel_ms = 0.0;
    uint64_t pixels = 0;
    unsigned long long segments = 0, camera = 0, continuation = 0, shadow = 0, node_visits = 0, tri_tests = 0;
    unsigned long long diag[RT_CNT_N_DIAG] = {0};          // rt_debug_counters
    unsigned long long grid_answered = 0, grid_entries = 0; // rt_debug_shadow_grid
};

// DevTargets::counters of one device (reference-mode kernels, megakernels).
void add_counters(FrameTotals& t, const unsigned long long (&c)[RT_CNT_SLOTS]) {
    t.segments += c[RT_CNT_SEGMENTS], t.camera += c[RT_CNT_CAMERA], t.continuation += c[RT_CNT_CONTINUATION], t.shadow += c[RT_CNT_SHADOW];
    t.node_visits += c[RT_CNT_NODE_VISITS], t.tri_tests += c[RT_CNT_TRI_TESTS];
    for (int k = 0; k < RT_CNT_N_DIAG; k++) t.diag[k] += c[RT_CNT_DIAG + k];
}

// WfBuffers::totals of a device's second lane into those of its first.
void merge_lanes(unsigned long long (&t)[rt::WF_N_TOTALS], const unsigned long long (&t2)[rt::WF_N_TOTALS]) {
    for (int k = 0; k < rt::WF_N_TOTALS; k++) t[k] = k == rt::WF_TOTAL_STACK_MAX ? std::max(t[k], t2[k]) : t[k] + t2[k];
}

// WfBuffers::totals of one device (the pipeline).  Its diagnostics go to rt_debug_counters in slot order, the high-water mark first.
int add_totals(rt_ctx* ctx, FrameTotals& t, const unsigned long long (&w)[rt::WF_N_TOTALS]) {
    t.segments += w[rt::WF_TOTAL_CAMERA] + w[rt::WF_TOTAL_CONTINUATION] + w[rt::WF_TOTAL_SHADOW];
    t.camera += w[rt::WF_TOTAL_CAMERA], t.continuation += w[rt::WF_TOTAL_CONTINUATION], t.shadow += w[rt::WF_TOTAL_SHADOW];
    t.node_visits += w[rt::WF_TOTAL_NODE_VISITS], t.tri_tests += w[rt::WF_TOTAL_TRI_TESTS];
    if (w[rt::WF_TOTAL_ERROR] != 0)
        return ctx->fail(RT_ERR_INTERNAL, "wavefront pipeline: %s (frame discarded)",
                         (w[rt::WF_TOTAL_ERROR] & 2ull) ? "a traversal stack grew beyond the depth the tree reports" : "a queue reservation exceeded its allocation");
    t.diag[0] = std::max(t.diag[0], w[rt::WF_TOTAL_STACK_MAX]);
    for (int k = 1; k < RT_CNT_N_DIAG; k++) t.diag[k] += w[rt::WF_TOTAL_STACK_MAX + k];
    t.grid_answered += w[rt::WF_TOTAL_GRID_ANSWERED], t.grid_entries += w[rt::WF_TOTAL_GRID_ENTRIES];
    return RT_OK;
}

// Pixels of device d's share of frame fr: the explicit tile of a dispatch, or the tiles the device owns.
uint64_t owned_pixels(const DevFrame& fr, uint32_t first, uint32_t stride, uint32_t n_owned) {
    uint64_t pixels = 0;
    for (uint32_t k = 0; k < n_owned; k++) {
        const uint32_t tile = first + k * stride, ty = tile / fr.tiles_x, tx = tile % fr.tiles_x;
        pixels += (uint64_t)std::min(fr.tile_size, fr.width - tx * fr.tile_size) * std::min(fr.tile_size, fr.height - ty * fr.tile_size);
    }
    return pixels;
}
uint64_t share_pixels(const DevFrame& fr, const DeviceState& d) {
    if (fr.single_tile)
        return (uint64_t)std::min(fr.tile_w, fr.width - std::min(fr.width, fr.tile_off_x)) * std::min(fr.tile_h, fr.height - std::min(fr.height, fr.tile_off_y));
    return owned_pixels(fr, d.tile_first, d.tile_stride, d.n_owned);
}

// Waits for device j's share of a frame and adds its kernel time, stage times, counters and pixels to `t`.
int collect_device(rt_ctx* ctx, size_t j, const DevFrame& fr, bool counters, const WfRun& r, FrameTotals& t) {
    DeviceState& d = ctx->devs[j];
    HIPCHK(ctx, hipSetDevice(d.device));
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    float ms = 0.0f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, d.ev0, d.ev1));
    t.kernel_ms = std::max(t.kernel_ms, (double)ms);
    if (j == 0 && d.stage_events_used) {
        if (d.stream2) HIPCHK(ctx, hipStreamSynchronize(d.stream2));
        for (uint32_t k = 0; k + 1 < d.stage_events_used; k += 2) {
            float sm = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&sm, d.stage_events[k], d.stage_events[k + 1]));
            ctx->stage_ms[0] += sm;
            ctx->stage_ms[1] += 1.0;
        }
    }
    if (r.pipeline) {
        unsigned long long w[rt::WF_N_TOTALS];
        HIPCHK(ctx, hipMemcpy(w, d.wf.totals, sizeof w, hipMemcpyDeviceToHost));
        if (r.two) {
            unsigned long long w2[rt::WF_N_TOTALS];
            HIPCHK(ctx, hipMemcpy(w2, d.wf2.totals, sizeof w2, hipMemcpyDeviceToHost));
            merge_lanes(w, w2);
        }
        if (int rc = add_totals(ctx, t, w)) return rc;
    } else if (counters || fr.mode == RT_MODE_EXTENDED) {
        unsigned long long c[RT_CNT_SLOTS];
        HIPCHK(ctx, hipMemcpy(c, d.counters, sizeof c, hipMemcpyDeviceToHost));
        add_counters(t, c);
    }
    t.pixels += fr.adaptive ? d.ad_pixels : share_pixels(fr, d); // (an adaptive call: the pixels that received samples)
    return RT_OK;
}

// rt_stats (and what rt_debug_counters / rt_debug_shadow_grid report) of a frame from its totals.
void finish_frame(rt_ctx* ctx, const DevFrame& fr, bool counters, const FrameTotals& t, uint32_t stat_flags, double w0) {
    rt_stats& st = ctx->stats;
    st.pixels = t.pixels;
    if (fr.mode == RT_MODE_EXTENDED) { // segments counted on the device
        st.rays = t.segments, st.primary_rays = t.camera, st.continuation_rays = t.continuation, st.shadow_rays = t.shadow;
    } else {
        const bool traced = fr.mode == RT_MODE_LEGACY || fr.cur_bounce <= fr.max_bounce;
        st.rays = traced ? t.pixels : 0; // modes 0/1: one segment per pixel
        st.primary_rays = st.rays;
        st.continuation_rays = st.shadow_rays = 0;
    }
    st.node_visits = counters ? t.node_visits : 0;
    st.tri_tests = counters ? t.tri_tests : 0;
    for (int k = 0; k < RT_CNT_N_DIAG; k++) ctx->diag[k] = counters ? t.diag[k] : 0;
    ctx->grid_diag[0] = counters ? t.grid_answered : 0, ctx->grid_diag[1] = counters ? t.grid_entries : 0;
    st.kernel_ms = t.kernel_ms, st.wall_ms = now_ms() - w0, st.flags = stat_flags;
}

// Launch one frame (or one explicit tile) on every device and wait.
int run_frame(rt_ctx* ctx, DevFrame fr, bool counters, uint32_t world, uint32_t rank, bool single_tile) {
    const double w0 = now_ms();
    if (!single_tile || counters)
        if (int rc = sync_pending(ctx)) return rc;
    const size_t nd = single_tile ? 1 : ctx->devs.size();
    std::vector<WfRun> runs(nd); // one per device (polls hold pointers into it)
    uint32_t stat_flags = 0;
    for (size_t j = 0; j < nd; j++) ctx->devs[j].stage_events_used = 0;
    ctx->stage_ms[0] = ctx->stage_ms[1] = 0.0;
    for (size_t j = 0; j < nd; j++) {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        if (int rc = ensure_targets(ctx, d, fr.width, fr.height)) return rc;
        DevFrame f = fr;
        if (!single_tile) assign_tiles(f, d, world, rank, nd, j);
        HIPCHK(ctx, hipMemsetAsync(d.counters, 0, RT_CNT_SLOTS * sizeof(unsigned long long), d.stream));
        HIPCHK(ctx, hipEventRecord(d.ev0, d.stream));
        if (f.adaptive) { // rt_render_adaptive: which pixels take samples, read back once per call and device to size what follows
            f.ad_mask = d.ad_mask;
            f.ad_blocks = d.ad_blocks;
            unsigned long long counts[2] = {0, 0};
            HIPCHK(ctx, rt::launch_ad_select(f, targets_for(d, f), d.ad_mask, d.ad_blocks, d.ad_counts, d.stream));
            HIPCHK(ctx, hipMemcpyAsync(counts, d.ad_counts, sizeof counts, hipMemcpyDeviceToHost, d.stream));
            HIPCHK(ctx, hipStreamSynchronize(d.stream));
            d.ad_live_blocks = (uint32_t)counts[0];
            d.ad_pixels = counts[1];
            if (d.ad_live_blocks == 0) { // every pixel of the share has stopped: nothing to trace
                HIPCHK(ctx, rt::launch_ad_image(f, targets_for(d, f), d.stream));
                HIPCHK(ctx, hipEventRecord(d.ev1, d.stream));
                continue;
            }
        }
        const KernelChoice k = choose_kernel(ctx, f);
        stat_flags |= (k.fallback ? RT_STAT_MEGAKERNEL_FALLBACK : 0u) | (k.kernel == rt::FrameKernel::SINGLE_PASS ? RT_STAT_SINGLE_PASS : 0u);
        if (k.kernel == rt::FrameKernel::PIPELINE) {
            if (int rc = setup_pipeline(ctx, j, f, runs[j])) return rc;
            continue;
        }
        if (k.kernel == rt::FrameKernel::REFERENCE) HIPCHK(ctx, rt::launch_render_reference(scene_for(ctx, d), f, targets_for(d, f), counters, d.stream));
        else HIPCHK(ctx, rt::launch_render_extended(scene_for(ctx, d), f, targets_for(d, f), k.kernel, counters, d.stream));
        if (f.adaptive) HIPCHK(ctx, rt::launch_ad_image(f, targets_for(d, f), d.stream));
        HIPCHK(ctx, hipEventRecord(d.ev1, d.stream));
    }
    // The pipeline's launches: every device advances by one step (a batch's generation, one bounce, a batch's resolve) in turn, so that
    // several devices of one context fill up side by side; the devices that have just passed a multiple of 8 bounces are then polled
    // together, after every device has its next launches queued.
    for (bool busy = true; busy;) {
        busy = false;
        std::vector<WfRun*> polls;
        for (WfRun& r : runs) {
            if (r.phase == WfRun::DONE) continue;
            busy = true;
            DeviceState& d = ctx->devs[r.dev];
            HIPCHK(ctx, hipSetDevice(d.device));
            const WfLane l = lane_of(d, r);
            const int rc = r.phase == WfRun::GENERATE ? wf_step_generate(ctx, d, r, l) : r.phase == WfRun::BOUNCE ? wf_step_bounce(ctx, d, r, l, counters, polls) : wf_step_resolve(ctx, d, r, l);
            if (rc != RT_OK) return rc;
        }
        for (WfRun* r : polls) {
            HIPCHK(ctx, hipSetDevice(ctx->devs[r->dev].device));
            HIPCHK(ctx, hipStreamSynchronize(r->poll_stream));
            if (r->alive == 0) r->phase = WfRun::RESOLVE;
            else r->it++;
        }
    }
    if (single_tile && !counters && fr.mode != RT_MODE_EXTENDED) { // one explicit tile of the reference's dispatch sequence: do not wait
        rt_stats& st = ctx->stats;
        st.pixels = share_pixels(fr, ctx->devs[0]);
        st.rays = st.primary_rays = (fr.mode == RT_MODE_LEGACY || fr.cur_bounce <= fr.max_bounce) ? st.pixels : 0;
        st.continuation_rays = st.shadow_rays = st.node_visits = st.tri_tests = 0;
        st.kernel_ms = 0.0; // filled in by sync_pending
        st.wall_ms = now_ms() - w0;
        ctx->pending_dispatch = true;
        return RT_OK;
    }
    FrameTotals t;
    for (size_t j = 0; j < nd; j++)
        if (int rc = collect_device(ctx, j, fr, counters, runs[j], t)) return rc;
    finish_frame(ctx, fr, counters, t, stat_flags, w0);
    return RT_OK;
}

int gather(rt_ctx* ctx, uint8_t* out, size_t elem, int which, void* const* per_device = nullptr);

// A dispatch sequence runs on the context's first device and starts from the textures as they are (tiles that are
// not dispatched keep their texels, like the reference's storage textures).  After an rt_render that was split over
// several devices those texels are spread over the devices: bring them together on the first one (a slow path through
// host memory, taken once at the transition).
int consolidate_on_first_device(rt_ctx* ctx, uint32_t w, uint32_t h) {
    if (ctx->devs.size() < 2 || ctx->frame_w != w || ctx->frame_h != h) return RT_OK;
    DeviceState& d0 = ctx->devs[0];
    if (d0.fb_w != w || d0.fb_h != h) return RT_OK;
    bool spread = false;
    for (size_t j = 1; j < ctx->devs.size(); j++) spread = spread || (ctx->devs[j].n_owned > 0 && ctx->devs[j].fb_w == w && ctx->devs[j].fb_h == h);
    if (!spread) return RT_OK;
    for (auto& d : ctx->devs) {
        HIPCHK(ctx, hipSetDevice(d.device));
        HIPCHK(ctx, hipStreamSynchronize(d.stream));
    }
    const size_t n = (size_t)w * h;
    std::vector<uint8_t> buf;
    HIPCHK(ctx, hipSetDevice(d0.device));
    for (int which = 0; which < 6; which++) {
        const size_t elem = which == 0 ? 16 : 4;
        void* dst = which == 0 ? (void*)d0.rgba32f : which <= 3 ? (void*)d0.chan[which - 1] : which == 4 ? (void*)d0.prim_id : (void*)d0.hit_t;
        buf.resize(n * elem);
        HIPCHK(ctx, hipSetDevice(d0.device));
        HIPCHK(ctx, hipMemcpy(buf.data(), dst, n * elem, hipMemcpyDeviceToHost)); // what the first device holds outside everyone's tiles
        int rc = gather(ctx, buf.data(), elem, which);
        if (rc != RT_OK) return rc;
        HIPCHK(ctx, hipSetDevice(d0.device));
        HIPCHK(ctx, hipMemcpy(dst, buf.data(), n * elem, hipMemcpyHostToDevice));
    }
    HIPCHK(ctx, hipDeviceSynchronize());
    d0.tile_first = 0;
    d0.tile_stride = 1;
    d0.n_owned = ctx->frame_tiles_x * ctx->frame_tiles_y;
    for (size_t j = 1; j < ctx->devs.size(); j++) ctx->devs[j].n_owned = 0;
    return RT_OK;
}

// The argument rules of rt_render (rt_hip.h), shared by rt_aovs and rt_sample_rays (`fn` names the call in the error text): the frame p
// describes, as a closed frame (without its tile share), and the tile_world / tile_rank share.
int frame_of_params(rt_ctx* ctx, const char* fn, const rt_render_params* p, DevFrame& fr, uint32_t& world, uint32_t& rank) {
    if (p->width == 0 || p->height == 0 || p->width > 65535u * 8u || p->height > 65535u * 8u)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: bad resolution %ux%u", fn, p->width, p->height);
    if (p->mode > RT_MODE_EXTENDED) return ctx->fail(RT_ERR_BAD_ARG, "%s: mode %u not supported", fn, p->mode);
    const bool accumulate = (p->flags & RT_FLAG_ACCUMULATE) != 0;
    if ((p->flags & RT_FLAG_ACCUMULATE_RESTART) && !accumulate)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: RT_FLAG_ACCUMULATE_RESTART without RT_FLAG_ACCUMULATE", fn);
    if (accumulate && p->mode != RT_MODE_EXTENDED)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: RT_FLAG_ACCUMULATE needs the extended mode (mode %u has no samples)", fn, p->mode);
    if (p->mode == RT_MODE_EXTENDED && (p->spp == 0 || p->spp > 65536u))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: spp %u out of range", fn, p->spp);
    // bounce depths travel in 8 bits in the reference (pack_flags, shared/src/lib.rs:1154-1179); modes 0/1 mask as the
    // reference does, the extended mode refuses what it cannot represent rather than looping 2^32 times
    if (p->mode == RT_MODE_EXTENDED && p->max_bounces > RT_MAX_BOUNCES)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: max_bounces %u > %u", fn, p->max_bounces, RT_MAX_BOUNCES);
    world = p->tile_world ? p->tile_world : 1, rank = p->tile_rank;
    if (rank >= world) return ctx->fail(RT_ERR_BAD_ARG, "%s: tile_rank %u >= tile_world %u", fn, rank, world);
    fr = DevFrame{};
    fr.width = p->width;
    fr.height = p->height;
    fr.tile_size = p->tile_size ? p->tile_size : RT_TILE_SIZE;
    if (fr.tile_size > 4096) return ctx->fail(RT_ERR_BAD_ARG, "%s: tile_size %u too large", fn, fr.tile_size);
    fr.tiles_x = (fr.width + fr.tile_size - 1) / fr.tile_size; // TileHelper::calculate_tile_count, shared/src/lib.rs:1187-1191
    fr.tiles_y = (fr.height + fr.tile_size - 1) / fr.tile_size;
    fr.mode = p->mode;
    fr.channel_mask = 7u;
    fr.cur_bounce = 0; // the bounce-0 pass of src/compute.rs:413-479 (later passes redraw the same pixels)
    fr.max_bounce = p->mode == RT_MODE_EXTENDED ? p->max_bounces : (p->max_bounces & 0xFF);
    fr.spp = p->mode == RT_MODE_EXTENDED ? p->spp : 1;
    fr.flags = p->flags;
    fr.frame_seed = p->frame_seed;
    fr.cam = make_camera(p->camera, (float)p->width, (float)p->height, p->mode != RT_MODE_LEGACY);
    fr.n_total = fr.spp; // a closed frame: samples 0 .. spp-1, jittered when there are several
    fr.jitter = fr.spp > 1 ? 1u : 0u;
    return RT_OK;
}

} // namespace

extern "C" {

const char* rt_version(void) { return "librt_hip 0.1 gfx950 (fp-contract=off, IEEE div/sqrt)"; }

const char* rt_last_error(rt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int rt_create(rt_ctx** out, const int* device_ids, int n_devices) {
    if (!out || n_devices < 1) {
        g_create_error = "rt_create: bad arguments";
        return RT_ERR_BAD_ARG;
    }
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count < 1) {
        g_create_error = std::string("rt_create: no HIP device (") + hipGetErrorString(e) + "); this library has no CPU fallback";
        return RT_ERR_HIP;
    }
    rt_ctx* ctx = new rt_ctx();
    for (int i = 0; i < n_devices; i++) {
        DeviceState d;
        d.device = device_ids ? device_ids[i] : i;
        if (d.device < 0 || d.device >= count) {
            g_create_error = "rt_create: device id out of range";
            rt_destroy(ctx);
            return RT_ERR_BAD_ARG;
        }
        if ((e = hipSetDevice(d.device)) != hipSuccess || (e = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking)) != hipSuccess || (e = hipStreamCreateWithFlags(&d.stream2, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&d.ev_start, hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&d.ev_join, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&d.ev_res[0], hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&d.ev_res[1], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreate(&d.ev0)) != hipSuccess || (e = hipEventCreate(&d.ev1)) != hipSuccess ||
            (e = hipMalloc((void**)&d.counters, RT_CNT_SLOTS * sizeof(unsigned long long))) != hipSuccess) {
            g_create_error = std::string("rt_create: ") + hipGetErrorString(e);
            ctx->devs.push_back(d);
            rt_destroy(ctx);
            return RT_ERR_HIP;
        }
        ctx->devs.push_back(d);
    }
    *out = ctx;
    return RT_OK;
}

void rt_destroy(rt_ctx* ctx) {
    if (!ctx) return;
    for (auto& d : ctx->devs) {
        if (d.device < 0) continue;
        (void)hipSetDevice(d.device);
        if (d.stream) (void)hipStreamSynchronize(d.stream);
        free_scene(d);
        free_targets(d);
        free_wavefront(d);
        free_denoise(d);
        (void)hipFree(d.counters);
        if (d.ev0) (void)hipEventDestroy(d.ev0);
        if (d.ev1) (void)hipEventDestroy(d.ev1);
        for (hipEvent_t e : {d.ev_start, d.ev_join, d.ev_res[0], d.ev_res[1]})
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : d.stage_events) (void)hipEventDestroy(e);
        for (hipEvent_t e : d.rq_events) (void)hipEventDestroy(e);
        if (d.stream2) (void)hipStreamDestroy(d.stream2);
        if (d.stream) (void)hipStreamDestroy(d.stream);
    }
    delete ctx;
}

int rt_upload_scene(rt_ctx* ctx, const rt_sphere* spheres, uint32_t n_spheres, const rt_light* lights, uint32_t n_lights,
                    const rt_vertex* vertices, uint32_t n_vertices, const rt_triangle* triangles, uint32_t n_triangles,
                    const rt_material* materials, uint32_t n_materials, const rt_bvh_node* ref_nodes, uint32_t n_ref_nodes,
                    const uint32_t* ref_tri_indices, uint32_t n_ref_tri_indices) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if ((n_spheres && !spheres) || (n_lights && !lights) || (n_vertices && !vertices) || (n_triangles && !triangles) ||
        (n_materials && !materials))
        return ctx->fail(RT_ERR_BAD_ARG, "rt_upload_scene: null array with non-zero count");
    // The reference BVH is accepted for interface compatibility and sanity-checked only.
    if (ref_nodes) {
        for (uint32_t i = 0; i < n_ref_nodes; i++) {
            const rt_bvh_node& n = ref_nodes[i];
            bool leaf = n.left_child == RT_INVALID_INDEX;
            if (!leaf && (n.left_child >= n_ref_nodes || (n.right_child != RT_INVALID_INDEX && n.right_child >= n_ref_nodes)))
                return ctx->fail(RT_ERR_BAD_ARG, "reference BVH node %u has a child out of range", i);
            if (leaf && ref_tri_indices && (uint64_t)n.triangle_start + n.triangle_count > n_ref_tri_indices)
                return ctx->fail(RT_ERR_BAD_ARG, "reference BVH leaf %u exceeds triangle_indices", i);
        }
    }
    std::vector<rt_triangle> tris(triangles, triangles + n_triangles);
    return upload_common(ctx, spheres, n_spheres, lights, n_lights, vertices, n_vertices, tris, {}, materials, n_materials);
}

int rt_upload_scene_packed(rt_ctx* ctx, const uint32_t* md, size_t n_u32, const rt_scene_metadata_offsets* off,
                           const rt_triangle* const tri_buffers[3], const uint32_t tri_counts[3], uint32_t triangles_per_buffer,
                           const rt_material* materials, uint32_t n_materials) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!off || (n_u32 && !md) || !tri_buffers || !tri_counts || (n_materials && !materials))
        return ctx->fail(RT_ERR_BAD_ARG, "rt_upload_scene_packed: null argument");
    auto section_ok = [&](uint32_t o, uint32_t count, uint32_t words) { return (uint64_t)o + (uint64_t)count * words <= n_u32; };
    if (!section_ok(off->spheres_offset, off->spheres_count, RT_SPHERE_WORDS) ||
        !section_ok(off->lights_offset, off->lights_count, RT_LIGHT_WORDS) ||
        !section_ok(off->bvh_nodes_offset, off->bvh_nodes_count, RT_BVH_NODE_WORDS) ||
        !section_ok(off->triangle_indices_offset, off->triangle_indices_count, 1) ||
        !section_ok(off->vertices_offset, off->vertices_count, RT_VERTEX_WORDS))
        return ctx->fail(RT_ERR_BAD_ARG, "rt_upload_scene_packed: a metadata section exceeds the buffer (%zu words)", n_u32);
    // Sections are plain reinterpretations of the host Vec<T> bytes (src/buffers.rs:213-234).
    const rt_sphere* spheres = reinterpret_cast<const rt_sphere*>(md + off->spheres_offset);
    const rt_light* lights = reinterpret_cast<const rt_light*>(md + off->lights_offset);
    const rt_vertex* vertices = reinterpret_cast<const rt_vertex*>(md + off->vertices_offset);
    std::vector<rt_triangle> tris;
    std::vector<uint32_t> prim_ids;
    for (int b = 0; b < 3; b++) {
        if (tri_counts[b] == 0) continue;
        if (!tri_buffers[b]) return ctx->fail(RT_ERR_BAD_ARG, "rt_upload_scene_packed: triangle buffer %d is null", b);
        if (triangles_per_buffer == 0 || tri_counts[b] > triangles_per_buffer)
            return ctx->fail(RT_ERR_BAD_ARG, "rt_upload_scene_packed: buffer %d holds %u > triangles_per_buffer %u", b, tri_counts[b],
                             triangles_per_buffer);
        for (uint32_t i = 0; i < tri_counts[b]; i++) {
            tris.push_back(tri_buffers[b][i]);
            prim_ids.push_back((uint32_t)b * triangles_per_buffer + i); // logical index, shader/src/triangle_access.rs:26-27
        }
    }
    return upload_common(ctx, spheres, off->spheres_count, lights, off->lights_count, vertices, off->vertices_count, tris, prim_ids,
                         materials, n_materials);
}

int rt_upload_textures(rt_ctx* ctx, const rt_texture_info* textures, uint32_t n_textures, const uint8_t* texture_data, size_t n_bytes) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if ((n_textures && !textures) || (n_bytes && !texture_data)) return ctx->fail(RT_ERR_BAD_ARG, "rt_upload_textures: null array with non-zero count");
    for (uint32_t i = 0; i < n_textures; i++)
        if ((uint64_t)textures[i].offset + textures[i].size > n_bytes)
            return ctx->fail(RT_ERR_BAD_ARG, "rt_upload_textures: texture %u (offset %u, %u bytes) exceeds the %zu bytes of texture data", i,
                             textures[i].offset, textures[i].size, n_bytes);
    // main_cs binds both buffers and reads neither (`_textures`, `_texture_data`, shader/src/lib.rs:34-35): nothing goes to the device
    ctx->n_textures = n_textures;
    ctx->texture_bytes = n_bytes;
    ctx->stats.n_textures = n_textures;
    ctx->stats.texture_bytes = n_bytes;
    return RT_OK;
}

// Development aid (not part of rt_hip.h): make the next scene upload fail before its k-th device array, as an allocation failure would.
int rt_debug_fail_upload(rt_ctx* ctx, int k) {
    if (!ctx) return RT_ERR_BAD_ARG;
    ctx->fail_upload_at = k;
    return RT_OK;
}

// Development aid (not part of rt_hip.h): download the tree the context holds on its first device and validate it the way the
// kernels decode it (bvh_check.h: slots and masks, every finite triangle in exactly one leaf, conservative boxes, depth).
// out[0] nodes, [1] leaves, [2] reported depth, [3] real depth, [4] triangles placed exactly once, [5] build method, [6] / [7] FNV-1a
// hashes of the node and triangle arrays (the device build lays its tree out exactly as its host statement does); returns the number of failures.
int rt_debug_check_bvh(rt_ctx* ctx, uint32_t out[8]) {
    if (!ctx || !ctx->uploaded) return -1;
    DeviceState& d = ctx->devs[0];
    if (hipSetDevice(d.device) != hipSuccess) return -1;
    (void)hipStreamSynchronize(d.stream);
    rt::BvhBuild b;
    b.nodes.resize(ctx->scene_counts.n_nodes);
    b.tris.resize(ctx->scene_counts.n_tris);
    if (!b.nodes.empty() && hipMemcpy(b.nodes.data(), d.nodes, b.nodes.size() * sizeof(DevNode8), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (!b.tris.empty() && hipMemcpy(b.tris.data(), d.tris, b.tris.size() * sizeof(DevTri), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    b.depth = ctx->stats.bvh_depth;
    b.n_leaves = (uint32_t)(b.tris.size() / RT_DEV_LEAF_STRIDE);
    std::vector<uint32_t> seen(ctx->n_input_tris, 0);
    uint32_t real_depth = 0;
    size_t leaves = 0;
    rtcheck::g_print = true;
    int fails = rtcheck::check_tree(b, seen, &real_depth, &leaves);
    uint32_t once = 0;
    for (uint32_t v : seen) {
        once += v == 1 ? 1u : 0u;
        if (v > 1) fails++;
    }
    if (out) {
        out[0] = (uint32_t)b.nodes.size();
        out[1] = (uint32_t)leaves;
        out[2] = b.depth;
        out[3] = real_depth;
        out[4] = once;
        out[5] = ctx->stats.tree_build;
        auto fnv = [](const void* p, size_t n) {
            uint32_t h = 2166136261u;
            const unsigned char* c = static_cast<const unsigned char*>(p);
            for (size_t i = 0; i < n; i++) h = (h ^ c[i]) * 16777619u;
            return h;
        };
        out[6] = fnv(b.nodes.data(), b.nodes.size() * sizeof(DevNode8));
        out[7] = fnv(b.tris.data(), b.tris.size() * sizeof(DevTri));
    }
    return fails;
}

// Development aids (not part of rt_hip.h): the queue allocation bound and the window rule, host-only arithmetic (tests/test_queue_bound.py).
unsigned long long rt_debug_queue_slots(unsigned long long max_entries, uint32_t per_lane, unsigned long long waves) {
    return rt::wf_queue_slots_for((size_t)max_entries, per_lane, (size_t)waves);
}
uint32_t rt_debug_pick_window(uint32_t iterations, uint32_t per_lane) { return rt::wf_pick_window(iterations, per_lane); }
unsigned long long rt_debug_state_slots(unsigned long long paths, unsigned long long waves) { return rt::wf_state_slots_for((size_t)paths, (size_t)waves); }

// RT_PREPARE_QUALITY_TREE: the tree of the uploaded scene rebuilt by the host builder (bvh_builder.cpp method 0: multithreaded binned SAH +
// insertion-based optimisation + the same 8-slot collapse) in place of the one rt_upload_scene* built on the device in milliseconds.  For
// scenes that stay: 0.35 s per 262 k triangles, 4.8 s for 3.8 M; frames 2 % (sponza-like) to 9 % (bistro-like) faster, same images (closest
// hits do not depend on the tree).  The light grids hold triangle records in leaf order: they go with the old tree and are built again on demand.
static int prepare_quality_tree(rt_ctx* ctx) {
    if (ctx->stats.tree_build == 0 || ctx->build_tris.empty()) return RT_OK; // already the host builder's (tiny scenes, a fallback, an earlier call)
    if (int rc = sync_host_geometry(ctx)) return rc; // positions an update left on the device
    TreeBuild tb(ctx);
    if (build_tree(ctx, ctx->build_tris, 0, rt::BvhBuildOptions{}, tb) != RT_OK || tb.bvh.nodes.empty())
        return ctx->fail(RT_ERR_INTERNAL, "rt_prepare: the host build gave %zu nodes at depth %u (the device-built tree stays)", tb.bvh.nodes.size(), tb.bvh.depth);
    if (int rc = install_tree(ctx, tb)) return rc;
    ctx->frame_valid = false;
    return RT_OK;
}

int rt_prepare(rt_ctx* ctx, uint32_t what) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_prepare: no scene uploaded");
    const uint32_t known = RT_PREPARE_SHADOW_GRIDS | RT_PREPARE_QUALITY_TREE;
    if (what & ~known) return ctx->fail(RT_ERR_BAD_ARG, "rt_prepare: unknown bits 0x%x", what & ~known);
    if (int rcp = sync_pending(ctx)) return rcp;
    if (what & RT_PREPARE_QUALITY_TREE)
        if (int rc = prepare_quality_tree(ctx)) return rc;
    if (what & RT_PREPARE_SHADOW_GRIDS)
        for (auto& d : ctx->devs)
            if (int rc = ensure_grids(ctx, d)) return rc;
    return RT_OK;
}

} // extern "C"

namespace {

// The running image an accumulating call (rt_render with RT_FLAG_ACCUMULATE, rt_render_adaptive) continues or starts: its key, and fr's
// sample base and count.  Fails, changing nothing, when the call would pass RT_ACCUMULATE_MAX_SAMPLES.
int accumulation_of(rt_ctx* ctx, const char* fn, const rt_render_params* p, uint32_t world, uint32_t rank, bool adaptive, DevFrame& fr, AccumKey& key) {
    key = AccumKey{};
    key.camera = p->camera;
    key.width = p->width, key.height = p->height, key.max_bounces = p->max_bounces, key.frame_seed = p->frame_seed;
    key.tile_size = fr.tile_size, key.tile_rank = rank, key.tile_world = world, key.no_shadows = p->flags & RT_FLAG_NO_SHADOWS;
    key.adaptive = adaptive ? 1u : 0u;
    const bool cont = ctx->acc_samples && !(p->flags & RT_FLAG_ACCUMULATE_RESTART) && std::memcmp(&key, &ctx->acc_key, sizeof key) == 0;
    const uint32_t base = cont ? ctx->acc_samples : 0u;
    if ((uint64_t)base + fr.spp > RT_ACCUMULATE_MAX_SAMPLES)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: %u + %u samples would pass the accumulation limit of %u", fn, base, fr.spp, RT_ACCUMULATE_MAX_SAMPLES);
    fr.sample_base = base; // this call traces samples base .. base + spp - 1 and divides by all of them; every sample is jittered
    fr.n_total = base + fr.spp; // (adaptive: the count of a pixel that never stopped; each pixel has its own)
    fr.jitter = 1u;
    return RT_OK;
}

// An rt_render or rt_render_adaptive call whose arguments have been checked: the frame fr, and with `accumulate` the running image `key`.
int render_call(rt_ctx* ctx, const DevFrame& fr, bool counters, uint32_t world, uint32_t rank, bool accumulate, const AccumKey& key) {
    end_accumulation(ctx); // counted again below once the frame has completed
    if (accumulate)
        if (int rc = ensure_run_sums(ctx, fr)) return rc;
    int rc = run_frame(ctx, fr, counters, world, rank, false);
    if (rc != RT_OK) return rc;
    if (accumulate) {
        ctx->acc_key = key;
        ctx->acc_samples = fr.n_total;
    }
    ctx->frame_w = fr.width;
    ctx->frame_h = fr.height;
    ctx->frame_tile = fr.tile_size;
    ctx->frame_tiles_x = fr.tiles_x;
    ctx->frame_tiles_y = fr.tiles_y;
    ctx->frame_valid = true;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_render(rt_ctx* ctx, const rt_render_params* p) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!p) return ctx->fail(RT_ERR_BAD_ARG, "rt_render: null params");
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_render: no scene uploaded");
    uint32_t world = 1, rank = 0;
    DevFrame fr{};
    if (int rc = frame_of_params(ctx, "rt_render", p, fr, world, rank)) return rc;
    const bool accumulate = (p->flags & RT_FLAG_ACCUMULATE) != 0;
    AccumKey key{};
    if (accumulate)
        if (int rc = accumulation_of(ctx, "rt_render", p, world, rank, false, fr, key)) return rc;
    return render_call(ctx, fr, (p->flags & RT_FLAG_COUNTERS) != 0, world, rank, accumulate, key);
}

int rt_render_adaptive(rt_ctx* ctx, const rt_render_params* p, const rt_adaptive_params* ap) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!p || !ap) return ctx->fail(RT_ERR_BAD_ARG, "rt_render_adaptive: null params");
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_render_adaptive: no scene uploaded");
    uint32_t world = 1, rank = 0;
    DevFrame fr{};
    if (int rc = frame_of_params(ctx, "rt_render_adaptive", p, fr, world, rank)) return rc;
    if (p->mode != RT_MODE_EXTENDED || !(p->flags & RT_FLAG_ACCUMULATE))
        return ctx->fail(RT_ERR_BAD_ARG, "rt_render_adaptive: needs the extended mode with RT_FLAG_ACCUMULATE (mode %u, flags 0x%x)", p->mode, p->flags);
    if (!std::isfinite(ap->threshold) || !(ap->threshold >= 0.0f))
        return ctx->fail(RT_ERR_BAD_ARG, "rt_render_adaptive: threshold %g is not finite and >= 0", (double)ap->threshold);
    if (ap->min_samples < 2u || ap->min_samples > RT_ACCUMULATE_MAX_SAMPLES)
        return ctx->fail(RT_ERR_BAD_ARG, "rt_render_adaptive: min_samples %u outside [2, %u]", ap->min_samples, RT_ACCUMULATE_MAX_SAMPLES);
    if (ap->flags != 0u) return ctx->fail(RT_ERR_BAD_ARG, "rt_render_adaptive: flags 0x%x reserved", ap->flags);
    AccumKey key{};
    if (int rc = accumulation_of(ctx, "rt_render_adaptive", p, world, rank, true, fr, key)) return rc;
    fr.adaptive = 1u;
    fr.ad_threshold = ap->threshold;
    fr.ad_min_samples = ap->min_samples;
    return render_call(ctx, fr, (p->flags & RT_FLAG_COUNTERS) != 0, world, rank, true, key);
}

int rt_dispatch_tile(rt_ctx* ctx, const rt_push_constants* pc) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!pc) return ctx->fail(RT_ERR_BAD_ARG, "rt_dispatch_tile: null push constants");
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_dispatch_tile: no scene uploaded");
    uint32_t channel = pc->packed_flags & 0xFF;
    if (channel > 2) return ctx->fail(RT_ERR_BAD_ARG, "rt_dispatch_tile: invalid color channel %u", channel); // src/renderer.rs:769-776
    auto as_u32 = [](float f) -> uint32_t { return !(f > 0.0f) ? 0u : (f >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)f); };
    uint32_t w = as_u32(pc->resolution[0]), h = as_u32(pc->resolution[1]);
    if (w == 0 || h == 0 || w > 65535u * 8u || h > 65535u * 8u)
        return ctx->fail(RT_ERR_BAD_ARG, "rt_dispatch_tile: bad resolution %gx%g", pc->resolution[0], pc->resolution[1]);
    uint32_t mode = (pc->packed_flags >> 24) & 0xFF;
    DevFrame fr{};
    fr.width = w;
    fr.height = h;
    fr.single_tile = 1;
    fr.tile_off_x = pc->tile_offset[0];
    fr.tile_off_y = pc->tile_offset[1];
    fr.tile_w = pc->tile_size_packed & 0xFFFF; // unpack_tile_size, shared/src/lib.rs:1146-1150
    fr.tile_h = (pc->tile_size_packed >> 16) & 0xFFFF;
    fr.tile_size = std::max(1u, std::max(fr.tile_w, fr.tile_h));
    fr.tiles_x = fr.tiles_y = 1;
    fr.mode = mode ? RT_MODE_WAVEFRONT : RT_MODE_LEGACY;
    fr.channel_mask = 1u << channel;
    fr.cur_bounce = (pc->packed_flags >> 8) & 0xFF;
    fr.max_bounce = (pc->packed_flags >> 16) & 0xFF;
    fr.spp = 1;
    fr.frame_seed = pc->frame_seed;
    fr.cam = make_camera(pc->camera, pc->resolution[0], pc->resolution[1], mode != 0);
    // Only texture `channel` receives texels (the other two keep theirs, as separate bind groups do);
    // the float and hit targets of the tile are refreshed as a by-product.
    DeviceState& d = ctx->devs[0];
    end_accumulation(ctx);
    int rc = consolidate_on_first_device(ctx, w, h);
    if (rc != RT_OK) return rc;
    rc = run_frame(ctx, fr, false, 1, 0, true);
    if (rc != RT_OK) return rc;
    ctx->frame_w = w;
    ctx->frame_h = h;
    ctx->frame_tile = RT_TILE_SIZE;
    ctx->frame_tiles_x = (w + RT_TILE_SIZE - 1) / RT_TILE_SIZE;
    ctx->frame_tiles_y = (h + RT_TILE_SIZE - 1) / RT_TILE_SIZE;
    ctx->frame_valid = true;
    // a dispatch sequence is owned entirely by device 0
    d.tile_first = 0;
    d.tile_stride = 1;
    d.n_owned = ctx->frame_tiles_x * ctx->frame_tiles_y;
    for (size_t j = 1; j < ctx->devs.size(); j++) ctx->devs[j].n_owned = 0; // whatever they own dates from an earlier rt_render
    return RT_OK;
}

// Copy `elem` bytes per pixel of the tiles first, first + stride, ... (n_owned of them) of a w x h frame of tile_size tiles, tiles_x
// per row, from `src` to `dst` (both full frames, row-major).
namespace {
void copy_share(uint8_t* dst, const uint8_t* src, size_t elem, uint32_t w, uint32_t h, uint32_t ts, uint32_t tiles_x, uint32_t first, uint32_t stride,
                uint32_t n_owned) {
    for (uint32_t k = 0; k < n_owned; k++) {
        uint32_t tile = first + k * stride;
        uint32_t ty = tile / tiles_x, tx = tile % tiles_x;
        uint32_t x0 = tx * ts, y0 = ty * ts, tw = std::min(ts, w - x0), th = std::min(ts, h - y0);
        for (uint32_t y = y0; y < y0 + th; y++)
            std::memcpy(dst + ((size_t)y * w + x0) * elem, src + ((size_t)y * w + x0) * elem, (size_t)tw * elem);
    }
}

// Copy `elem` bytes per pixel of every device's owned tiles into `out` (full frame, row-major), from the target `which` or, with
// `per_device`, from a full-frame buffer per device.
int gather(rt_ctx* ctx, uint8_t* out, size_t elem, int which /*0 rgba32f, 1..3 chan, 4 prim, 5 t*/, void* const* per_device) {
    uint32_t w = ctx->frame_w, h = ctx->frame_h;
    size_t n = (size_t)w * h;
    std::vector<uint8_t> tmp;
    for (size_t j = 0; j < ctx->devs.size(); j++) {
        DeviceState& d = ctx->devs[j];
        if (d.fb_w != w || d.fb_h != h || d.n_owned == 0) continue;
        const void* src = which == 0 ? (const void*)d.rgba32f : which <= 3 ? (const void*)d.chan[which - 1] : which == 4 ? (const void*)d.prim_id : (const void*)d.hit_t;
        if (per_device && !per_device[j]) continue;
        if (per_device) src = per_device[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        bool all = d.tile_stride == 1 && d.tile_first == 0;
        if (all) {
            HIPCHK(ctx, hipMemcpy(out, src, n * elem, hipMemcpyDeviceToHost));
            continue;
        }
        tmp.resize(n * elem);
        HIPCHK(ctx, hipMemcpy(tmp.data(), src, n * elem, hipMemcpyDeviceToHost));
        copy_share(out, tmp.data(), elem, w, h, ctx->frame_tile, ctx->frame_tiles_x, d.tile_first, d.tile_stride, d.n_owned);
    }
    return RT_OK;
}
} // namespace

// The read-back staging of device d (current): at least `bytes` on the device and pinned on the host.
static int ensure_readback(rt_ctx* ctx, DeviceState& d, size_t bytes) {
    if (d.readback_bytes < bytes) {
        (void)hipFree(d.readback_dev);
        if (d.readback_host) (void)hipHostFree(d.readback_host);
        d.readback_dev = d.readback_host = nullptr;
        d.readback_bytes = 0;
        HIPCHK(ctx, hipMalloc(&d.readback_dev, bytes));
        HIPCHK(ctx, hipHostMalloc(&d.readback_host, bytes, hipHostMallocDefault));
        d.readback_bytes = bytes;
    }
    return RT_OK;
}

// Whole frame on one device: run the epilogue there and bring the result back through pinned staging
// (`which` 0: packed rgb32f, 1: combined rgba8).  Returns RT_OK, an error, or 1 when the caller must use the gather path.
static int read_epilogue(rt_ctx* ctx, int which, void* out, size_t bytes) {
    if (ctx->devs.size() != 1) return 1;
    DeviceState& d = ctx->devs[0];
    if (d.fb_w != ctx->frame_w || d.fb_h != ctx->frame_h || !(d.tile_stride == 1 && d.tile_first == 0)) return 1;
    HIPCHK(ctx, hipSetDevice(d.device));
    if (int rc = ensure_readback(ctx, d, bytes)) return rc;
    const size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    if (which == 0) HIPCHK(ctx, rt::launch_pack_rgb32f(d.rgba32f, (float*)d.readback_dev, n, d.stream));
    else HIPCHK(ctx, rt::launch_combine_rgba8(d.chan[0], d.chan[1], d.chan[2], (uint8_t*)d.readback_dev, n, d.stream));
    HIPCHK(ctx, hipMemcpyAsync(d.readback_host, d.readback_dev, bytes, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    std::memcpy(out, d.readback_host, bytes);
    return RT_OK;
}

int rt_read_rgb32f(rt_ctx* ctx, float* out, size_t n_floats) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->frame_valid) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_read_rgb32f: nothing rendered yet");
    size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    if (!out || n_floats != n * 3) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_rgb32f: expected %zu floats, got %zu", n * 3, n_floats);
    int rc = read_epilogue(ctx, 0, out, n * 12);
    if (rc <= 0) return rc;
    std::vector<float> tmp(n * 4, 0.0f);
    rc = gather(ctx, reinterpret_cast<uint8_t*>(tmp.data()), 16, 0);
    if (rc != RT_OK) return rc;
    for (size_t i = 0; i < n; i++) {
        out[3 * i + 0] = tmp[4 * i + 0];
        out[3 * i + 1] = tmp[4 * i + 1];
        out[3 * i + 2] = tmp[4 * i + 2];
    }
    return RT_OK;
}

int rt_read_rgba8_channels(rt_ctx* ctx, uint8_t* red, uint8_t* green, uint8_t* blue, size_t n_bytes_each) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->frame_valid) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_read_rgba8_channels: nothing rendered yet");
    size_t n = (size_t)ctx->frame_w * ctx->frame_h * 4;
    if (n_bytes_each != n) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_rgba8_channels: expected %zu bytes each, got %zu", n, n_bytes_each);
    uint8_t* outs[3] = {red, green, blue};
    for (int c = 0; c < 3; c++) {
        if (!outs[c]) continue;
        std::memset(outs[c], 0, n);
        int rc = gather(ctx, outs[c], 4, 1 + c);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

int rt_read_rgba8_combined(rt_ctx* ctx, uint8_t* out, size_t n_bytes) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->frame_valid) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_read_rgba8_combined: nothing rendered yet");
    size_t n = (size_t)ctx->frame_w * ctx->frame_h * 4;
    if (!out || n_bytes != n) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_rgba8_combined: expected %zu bytes, got %zu", n, n_bytes);
    int rc = read_epilogue(ctx, 1, out, n);
    if (rc <= 0) return rc;
    std::vector<uint8_t> r(n), g(n), b(n);
    rc = rt_read_rgba8_channels(ctx, r.data(), g.data(), b.data(), n);
    if (rc != RT_OK) return rc;
    for (size_t i = 0; i < n; i += 4) { // main_fs, shader/src/lib.rs:383-388
        out[i + 0] = r[i + 0];
        out[i + 1] = g[i + 1];
        out[i + 2] = b[i + 2];
        out[i + 3] = 255;
    }
    return RT_OK;
}

int rt_read_hits(rt_ctx* ctx, uint32_t* prim_ids, float* t, size_t n_pixels) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->frame_valid) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_read_hits: nothing rendered yet");
    size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    if (n_pixels != n) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_hits: expected %zu pixels, got %zu", n, n_pixels);
    int rc;
    if (prim_ids) {
        std::memset(prim_ids, 0xFF, n * 4);
        if ((rc = gather(ctx, reinterpret_cast<uint8_t*>(prim_ids), 4, 4)) != RT_OK) return rc;
    }
    if (t) {
        std::memset(t, 0, n * 4);
        if ((rc = gather(ctx, reinterpret_cast<uint8_t*>(t), 4, 5)) != RT_OK) return rc;
    }
    return RT_OK;
}

// Development aid: the camera beams of the last extended-mode frame on the first device: per owned 8x8 pixel block the length of its
// triangle list (0xFFFFFFFF: no list).  Returns the number of blocks (<= n), negative on error.
int rt_debug_beams(rt_ctx* ctx, uint32_t* counts, uint32_t n) {
    if (!ctx || ctx->devs.empty()) return RT_ERR_BAD_ARG;
    DeviceState& d = ctx->devs[0];
    if (!d.wf.beam_count) return 0;
    if (hipSetDevice(d.device) != hipSuccess) return RT_ERR_HIP;
    (void)hipStreamSynchronize(d.stream);
    const uint32_t m = std::min(n, d.wf.n_blocks);
    if (m && hipMemcpy(counts, d.wf.beam_count, (size_t)m * 4, hipMemcpyDeviceToHost) != hipSuccess) return RT_ERR_HIP;
    for (uint32_t i = 0; i < m; i++)
        if (counts[i] & RT_BEAM_OVERFLOW) counts[i] = 0xFFFFFFFFu;
    return (int)m;
}

// Development aid / bench.py: with RT_FLAG_STAGE_TIMES, the launches of the frame's dominant stage kernel (k_wf_shadow_grid) on the first
// device, timed with HIP events on the stream they were launched on: out[0] sum of their durations in ms, out[1] their number.
int rt_debug_stage_times(rt_ctx* ctx, double out[2]) {
    if (!ctx || !out) return RT_ERR_BAD_ARG;
    out[0] = ctx->stage_ms[0];
    out[1] = ctx->stage_ms[1];
    return RT_OK;
}

// Development aid (not part of rt_hip.h): the diagnostics of the last render, zero unless it ran with RT_FLAG_COUNTERS.  Their meaning
// depends on the kernel that rendered it.  State-machine megakernel (DevCounterSlot RT_CNT_SM_*, summed over waves and devices):
// transition passes, lanes served in them, node iterations, lanes active in them, leaf iterations, lanes active in them, cycles in
// transition phases, cycles in traversal phases.  Pipeline (WfTotal 5-12, wavefront.h, over both lanes and the devices): traversal stack
// high-water mark (a maximum), node visits that enter no child, children entered, node steps, leaf steps, lanes in leaf steps, leaf
// trips, refills.  Other kernels: zeros.
int rt_debug_counters(rt_ctx* ctx, unsigned long long out[8]) {
    if (!ctx || !out) return RT_ERR_BAD_ARG;
    for (int k = 0; k < 8; k++) out[k] = ctx->diag[k];
    return RT_OK;
}

// Development aid: what the light grids (shadow_grid.h) of the first device look like.  light < n_lights: out = {kind (0: refused), cells per
// side, entries, near-list length, longest list, cells left to the BVH, cells with a list, 0}; light == 0xFFFFFFFF: out = {lights with a grid, all
// entries, bytes, shadow segments the grids answered in the last frame rendered with RT_FLAG_COUNTERS, list entries read, 0, 0, 0}.
int rt_debug_shadow_grid(rt_ctx* ctx, uint32_t light, unsigned long long out[8]) {
    if (!ctx || !out) return RT_ERR_BAD_ARG;
    for (int k = 0; k < 8; k++) out[k] = 0;
    if (ctx->devs.empty()) return RT_OK;
    const DeviceState& d = ctx->devs[0];
    if (light == 0xFFFFFFFFu) {
        for (const rt::ShadowGridBuild& g : d.grid_info) {
            if (g.grid.kind == RT_SG_KIND_NONE) continue;
            out[0]++;
            out[1] += g.n_entries;
            out[2] += g.bytes;
        }
        out[3] = ctx->grid_diag[0];
        out[4] = ctx->grid_diag[1];
        return RT_OK;
    }
    if (light >= d.grid_info.size()) return RT_OK;
    const rt::ShadowGridBuild& g = d.grid_info[light];
    out[0] = g.grid.kind;
    out[1] = g.grid.res;
    out[2] = g.n_entries;
    out[3] = g.near_count;
    out[4] = g.longest;
    out[5] = g.heavy_cells;
    out[6] = g.filled_cells;
    return RT_OK;
}

int rt_read_adaptive(rt_ctx* ctx, rt_adaptive_pixel* out, size_t n_pixels) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->acc_samples || !ctx->acc_key.adaptive) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_adaptive: the context has no adaptive running image");
    const size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    if (!out || n_pixels != n) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_adaptive: expected %zu records, got %zu", n, n_pixels);
    static_assert(sizeof(rt_adaptive_pixel) == 32, "two float4 per record (k_ad_records)");
    // every device's records of the whole frame (those outside its share are never copied), then its share of them into `out`
    std::vector<void*> src(ctx->devs.size(), nullptr);
    for (size_t j = 0; j < ctx->devs.size(); j++) {
        DeviceState& d = ctx->devs[j];
        if (d.fb_w != ctx->frame_w || d.fb_h != ctx->frame_h || d.n_owned == 0 || !d.run_sum || !d.run_odd) continue;
        HIPCHK(ctx, hipSetDevice(d.device));
        if (int rc = ensure_readback(ctx, d, n * sizeof(rt_adaptive_pixel))) return rc;
        HIPCHK(ctx, rt::launch_ad_records(d.run_sum, d.run_odd, d.readback_dev, n, d.stream));
        HIPCHK(ctx, hipStreamSynchronize(d.stream));
        src[j] = d.readback_dev;
    }
    std::memset(out, 0, n * sizeof(rt_adaptive_pixel));
    return gather(ctx, reinterpret_cast<uint8_t*>(out), sizeof(rt_adaptive_pixel), 0, src.data());
}

int rt_accumulated_samples(rt_ctx* ctx, uint32_t* samples) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!samples) return ctx->fail(RT_ERR_BAD_ARG, "rt_accumulated_samples: null output");
    *samples = ctx->acc_samples;
    return RT_OK;
}

int rt_get_stats(rt_ctx* ctx, rt_stats* out) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!out) return ctx->fail(RT_ERR_BAD_ARG, "rt_get_stats: null out");
    if (int rcp = sync_pending(ctx)) return rcp;
    *out = ctx->stats;
    return RT_OK;
}

// ------------------------------------------------------------------------------------
// Ray queries (rt_hip.h "Ray queries"): rt_intersect, rt_occluded, rt_camera_rays.
// ------------------------------------------------------------------------------------
} // extern "C"

namespace {

struct QueryPtr {
    bool device = false; // device memory of one of the context's devices (else host memory of any kind: staged)
    size_t dev = 0;      // ... its index in ctx->devs
};

// Where `p` lives.  Pageable memory the runtime has never seen may come back as an error or as unregistered: both are host memory.
int classify_ptr(rt_ctx* ctx, const char* fn, const char* what, const void* p, QueryPtr& q, uintptr_t align = 16) {
    q = QueryPtr{};
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return RT_OK;
    }
    if (a.type != hipMemoryTypeDevice || a.isManaged) return RT_OK; // pinned, managed, unregistered
    for (size_t j = 0; j < ctx->devs.size(); j++)
        if (ctx->devs[j].device == a.device) {
            if (reinterpret_cast<uintptr_t>(p) & (align - 1))
                return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is device memory that is not %u-byte aligned (%p)", fn, what, (unsigned)align, p);
            q.device = true;
            q.dev = j;
            return RT_OK;
        }
    return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is device memory of HIP device %d, which is not a device of this context", fn, what, a.device);
}

int ensure_buffer(rt_ctx* ctx, void** buf, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return RT_OK;
    (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    HIPCHK(ctx, hipMalloc(buf, bytes));
    *cap = bytes;
    return RT_OK;
}

int ensure_query_events(rt_ctx* ctx, DeviceState& d, size_t n) {
    while (d.rq_events.size() < n) {
        hipEvent_t e = nullptr;
        HIPCHK(ctx, hipEventCreate(&e));
        d.rq_events.push_back(e);
    }
    return RT_OK;
}

// Both query kinds: out_elem = 16 (rt_hit) or 1 (occluded byte).
int run_query(rt_ctx* ctx, const char* fn, const rt_ray* rays, size_t n, void* out, size_t out_elem, uint32_t flags) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    const char* out_name = out_elem == 1 ? "occluded" : "hits";
    if (!rays || !out) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !rays ? "rays" : out_name, n);
    if (flags & ~RT_QUERY_COUNTERS) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~RT_QUERY_COUNTERS);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pin, pout;
    if (int rc = classify_ptr(ctx, fn, "rays", rays, pin)) return rc;
    if (int rc = classify_ptr(ctx, fn, out_name, out, pout)) return rc;
    if (pin.device != pout.device || pin.dev != pout.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: rays (%s %zu) and %s (%s %zu) must both be host memory or both device memory of the same device", fn,
                         pin.device ? "device memory of context device" : "host memory", pin.device ? pin.dev : (size_t)0, out_name,
                         pout.device ? "device memory of context device" : "host memory", pout.device ? pout.dev : (size_t)0);
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0;
    const size_t nd = ctx->devs.size();
    std::vector<size_t> first(nd, 0), count(nd, 0);
    if (pin.device) count[pin.dev] = n; // a device batch runs where it lives
    else
        for (size_t j = 0; j < nd; j++) first[j] = n * j / nd, count[j] = n * (j + 1) / nd - first[j]; // contiguous ranges, one per device
    const uint8_t* src = reinterpret_cast<const uint8_t*>(rays);
    uint8_t* dst = reinterpret_cast<uint8_t*>(out);
    // every device's range is enqueued before any is waited for
    auto enqueue = [&](size_t j) -> int {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        const DevScene sc = scene_for(ctx, d);
        const size_t chunks = (count[j] + RT_QUERY_CHUNK - 1) / RT_QUERY_CHUNK;
        if (int rc = ensure_query_events(ctx, d, 2 * chunks)) return rc;
        if (!pin.device) {
            const size_t m = std::min<size_t>(count[j], RT_QUERY_CHUNK);
            if (int rc = ensure_buffer(ctx, &d.rq_in, &d.rq_in_bytes, m * sizeof(rt_ray))) return rc;
            if (int rc = ensure_buffer(ctx, &d.rq_out, &d.rq_out_bytes, m * out_elem)) return rc;
        }
        if (counters) HIPCHK(ctx, hipMemsetAsync(d.counters, 0, (RT_CNT_TRI_TESTS + 1) * sizeof(unsigned long long), d.stream));
        for (size_t c = 0; c < chunks; c++) {
            const size_t off = first[j] + c * RT_QUERY_CHUNK, m = std::min<size_t>(RT_QUERY_CHUNK, first[j] + count[j] - off);
            const void* in = src + off * sizeof(rt_ray);
            void* res = dst + off * out_elem;
            if (!pin.device) {
                HIPCHK(ctx, hipMemcpyAsync(d.rq_in, in, m * sizeof(rt_ray), hipMemcpyHostToDevice, d.stream));
                in = d.rq_in;
                res = d.rq_out;
            }
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c], d.stream));
            HIPCHK(ctx, rt::launch_ray_query(sc, in, res, (uint32_t)m, out_elem == 1, counters ? d.counters : nullptr, d.stream));
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c + 1], d.stream));
            if (!pin.device) HIPCHK(ctx, hipMemcpyAsync(dst + off * out_elem, d.rq_out, m * out_elem, hipMemcpyDeviceToHost, d.stream));
        }
        return RT_OK;
    };
    auto drain = [&]() { // after a failure: nothing of this call is left writing into the caller's memory
        for (auto& d : ctx->devs) {
            (void)hipSetDevice(d.device);
            (void)hipStreamSynchronize(d.stream);
        }
    };
    for (size_t j = 0; j < nd; j++)
        if (count[j] > 0)
            if (int rc = enqueue(j)) {
                drain();
                return rc;
            }
    double kernel_ms = 0.0;
    unsigned long long nodes = 0, tris = 0;
    for (size_t j = 0; j < nd; j++) {
        if (count[j] == 0) continue;
        DeviceState& d = ctx->devs[j];
        hipError_t e = hipSetDevice(d.device);
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        if (e != hipSuccess) {
            drain();
            return ctx->fail(RT_ERR_HIP, "%s: device %d: %s", fn, d.device, hipGetErrorString(e));
        }
        double ms = 0.0;
        for (size_t c = 0; 2 * c + 1 < d.rq_events.size() && c * RT_QUERY_CHUNK < count[j]; c++) {
            float cm = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&cm, d.rq_events[2 * c], d.rq_events[2 * c + 1]));
            ms += cm;
        }
        kernel_ms = std::max(kernel_ms, ms);
        if (counters) {
            unsigned long long cn[RT_CNT_TRI_TESTS + 1];
            HIPCHK(ctx, hipMemcpy(cn, d.counters, sizeof cn, hipMemcpyDeviceToHost));
            nodes += cn[RT_CNT_NODE_VISITS];
            tris += cn[RT_CNT_TRI_TESTS];
        }
    }
    rt_stats& st = ctx->stats;
    st.rays = n;
    st.primary_rays = st.continuation_rays = st.shadow_rays = st.pixels = 0;
    st.node_visits = counters ? nodes : 0;
    st.tri_tests = counters ? tris : 0;
    st.kernel_ms = kernel_ms;
    st.wall_ms = now_ms() - w0;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_intersect(rt_ctx* ctx, const rt_ray* rays, size_t n, rt_hit* hits, uint32_t flags) {
    return run_query(ctx, "rt_intersect", rays, n, hits, sizeof(rt_hit), flags);
}

int rt_occluded(rt_ctx* ctx, const rt_ray* rays, size_t n, uint8_t* occluded, uint32_t flags) {
    return run_query(ctx, "rt_occluded", rays, n, occluded, 1, flags);
}

int rt_camera_rays(rt_ctx* ctx, const rt_camera* camera, uint32_t width, uint32_t height, uint32_t mode, rt_ray* out) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (mode != RT_MODE_LEGACY && mode != RT_MODE_WAVEFRONT) return ctx->fail(RT_ERR_BAD_ARG, "rt_camera_rays: mode %u (0 or 1)", mode);
    const size_t n = (size_t)width * height;
    if (n == 0) return RT_OK;
    if (!camera || !out) return ctx->fail(RT_ERR_BAD_ARG, "rt_camera_rays: %s is NULL", !camera ? "camera" : "out");
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr po;
    if (int rc = classify_ptr(ctx, "rt_camera_rays", "out", out, po)) return rc;
    DeviceState& d = ctx->devs[po.dev];
    HIPCHK(ctx, hipSetDevice(d.device));
    if (!po.device)
        if (int rc = ensure_buffer(ctx, &d.rq_in, &d.rq_in_bytes, std::min<size_t>(n, RT_QUERY_CHUNK) * sizeof(rt_ray))) return rc;
    // the frames' camera constants (make_camera) and ray generation (camera_ray): the rays are those rt_render traces
    const DevCamera cam = make_camera(*camera, (float)width, (float)height, mode != RT_MODE_LEGACY);
    uint8_t* dst = reinterpret_cast<uint8_t*>(out);
    for (size_t off = 0; off < n; off += RT_QUERY_CHUNK) {
        const size_t m = std::min<size_t>(RT_QUERY_CHUNK, n - off);
        void* res = po.device ? (void*)(dst + off * sizeof(rt_ray)) : d.rq_in;
        hipError_t e = rt::launch_camera_rays(cam, width, mode != RT_MODE_LEGACY, res, off, (uint32_t)m, d.stream);
        if (e == hipSuccess && !po.device) e = hipMemcpyAsync(dst + off * sizeof(rt_ray), d.rq_in, m * sizeof(rt_ray), hipMemcpyDeviceToHost, d.stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(d.stream);
            return ctx->fail(RT_ERR_HIP, "rt_camera_rays: %s", hipGetErrorString(e));
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// rt_update_geometry: new positions for the uploaded scene's vertices and spheres.  The tree in use is refitted (refit.hip: the
// triangle records and the node boxes follow the positions, the topology stays) or, on request or when a triangle the tree has no
// record of became finite, rebuilt through the upload's own build and hand-over (build_tree / install_tree).
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

// build_tris and the finite box from positions in host memory (3 floats per vertex), through the upload's triangles.
void gather_positions(rt_ctx* ctx, const float* verts) {
    for (size_t i = 0; i < ctx->up_triangles.size(); i++) {
        const rt_triangle& t = ctx->up_triangles[i];
        rt::BuildTri& b = ctx->build_tris[i];
        std::memcpy(b.v0, verts + 3 * (size_t)t.v0_index, 12);
        std::memcpy(b.v1, verts + 3 * (size_t)t.v1_index, 12);
        std::memcpy(b.v2, verts + 3 * (size_t)t.v2_index, 12);
    }
    finite_box(ctx->build_tris, ctx->box_lo, ctx->box_hi);
}

int read_positions(rt_ctx* ctx, std::vector<float>& out) { // the positions of the last update, as the first device holds them
    DeviceState& d = ctx->devs[0];
    out.resize(3 * (size_t)ctx->up_vertices);
    HIPCHK(ctx, hipSetDevice(d.device));
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    if (!out.empty()) HIPCHK(ctx, hipMemcpy(out.data(), d.rf_verts, out.size() * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

// What the host side keeps of the scene (build_tris, box_lo / box_hi: rt_prepare RT_PREPARE_QUALITY_TREE and the light grids read
// them) after an update from device memory: read back once, when one of them needs it.
int sync_host_geometry(rt_ctx* ctx) {
    if (!ctx->host_geometry_stale) return RT_OK;
    std::vector<float> v;
    if (int rc = read_positions(ctx, v)) return rc;
    gather_positions(ctx, v.data());
    ctx->host_geometry_stale = false;
    return RT_OK;
}

// The refit's view of the current tree (made once per tree, from the first device's arrays; every device holds the same tree): the
// tree levels, the vertex indices of every triangle record, and the triangles that have no record.
int ensure_refit_view(rt_ctx* ctx) {
    if (ctx->rf_ready) return RT_OK;
    const uint32_t n_nodes = ctx->scene_counts.n_nodes, n_rec = ctx->scene_counts.n_tris;
    std::vector<DevNode8> nodes(n_nodes);
    std::vector<DevTri> recs(n_rec);
    {
        DeviceState& d = ctx->devs[0];
        HIPCHK(ctx, hipSetDevice(d.device));
        HIPCHK(ctx, hipStreamSynchronize(d.stream));
        if (n_nodes) HIPCHK(ctx, hipMemcpy(nodes.data(), d.nodes, nodes.size() * sizeof(DevNode8), hipMemcpyDeviceToHost));
        if (n_rec) HIPCHK(ctx, hipMemcpy(recs.data(), d.tris, recs.size() * sizeof(DevTri), hipMemcpyDeviceToHost));
    }
    const size_t n_in = ctx->up_triangles.size();
    std::vector<uint32_t> index_of; // prim id -> upload index (identity unless the upload was packed)
    if (!ctx->up_prim_ids.empty()) {
        index_of.assign((size_t)*std::max_element(ctx->up_prim_ids.begin(), ctx->up_prim_ids.end()) + 1, 0xFFFFFFFFu);
        for (size_t i = 0; i < n_in; i++) index_of[ctx->up_prim_ids[i]] = (uint32_t)i;
    }
    std::vector<uint32_t> vidx(3 * (size_t)n_rec, RT_REFIT_NO_RECORD), order, level_first;
    std::vector<uint8_t> has_record(n_in, 0), visited(n_nodes, 0);
    auto bad = [&](const char* what, uint32_t node) { return ctx->fail(RT_ERR_INTERNAL, "rt_update_geometry: node %u: %s", node, what); };
    if (n_nodes) {
        order.push_back(0);
        visited[0] = 1;
    }
    for (size_t begin = 0; begin < order.size();) { // breadth first: one level per pass
        const size_t end = order.size();
        level_first.push_back((uint32_t)begin);
        if (level_first.size() > RT_DEV_MAX_BVH_DEPTH) return bad("the tree is deeper than the depth bound", order[begin]);
        for (size_t k = begin; k < end; k++) {
            const uint32_t node = order[k];
            const DevNode8& n = nodes[node];
            const uint32_t imask = n.ex_imask >> 24, lmask = n.lmask & 0xFFu;
            for (uint32_t sl = 0; sl < 8; sl++) {
                const uint32_t bit = 1u << sl, below = bit - 1u;
                if (imask & bit) {
                    const uint64_t c = (uint64_t)n.child_base + (uint32_t)__builtin_popcount(imask & below);
                    if (c >= n_nodes || visited[c]) return bad("inner child out of range or reached twice", node);
                    visited[c] = 1;
                    order.push_back((uint32_t)c);
                } else if (lmask & bit) {
                    const uint64_t first = (uint64_t)n.tri_base + RT_DEV_LEAF_STRIDE * (uint32_t)__builtin_popcount(lmask & below);
                    if (first + RT_DEV_LEAF_STRIDE > n_rec || recs[first].leaf_count > RT_DEV_LEAF_STRIDE) return bad("leaf out of range", node);
                    for (uint32_t r = 0; r < recs[first].leaf_count; r++) {
                        const uint32_t prim = recs[first + r].prim_id;
                        const uint32_t i = index_of.empty() ? prim : (prim < index_of.size() ? index_of[prim] : 0xFFFFFFFFu);
                        if (i >= n_in) return bad("record with an unknown prim id", node);
                        const rt_triangle& t = ctx->up_triangles[i];
                        vidx[3 * (first + r)] = t.v0_index;
                        vidx[3 * (first + r) + 1] = t.v1_index;
                        vidx[3 * (first + r) + 2] = t.v2_index;
                        has_record[i] = 1;
                    }
                }
            }
        }
        begin = end;
    }
    level_first.push_back((uint32_t)order.size());
    std::vector<uint32_t> dropped;
    for (size_t i = 0; i < n_in; i++)
        if (!has_record[i]) {
            const rt_triangle& t = ctx->up_triangles[i];
            dropped.insert(dropped.end(), {t.v0_index, t.v1_index, t.v2_index});
        }
    for (auto& d : ctx->devs) {
        free_refit(d);
        HIPCHK(ctx, hipSetDevice(d.device));
        int rc;
        if ((rc = upload_array(ctx, &d.rf_vidx, vidx)) != RT_OK || (rc = upload_array(ctx, &d.rf_order, order)) != RT_OK ||
            (rc = upload_array(ctx, &d.rf_dropped, dropped)) != RT_OK)
            return rc;
        HIPCHK(ctx, hipMalloc((void**)&d.rf_boxes, std::max<size_t>(1, 2 * (size_t)n_nodes) * sizeof(float4)));
        HIPCHK(ctx, hipMalloc((void**)&d.rf_flag, sizeof(uint32_t)));
    }
    ctx->rf_level_first = level_first;
    ctx->rf_n_dropped = (uint32_t)(dropped.size() / 3);
    ctx->rf_ready = true;
    return RT_OK;
}

// Everything after the argument checks; a failure here leaves the context "not uploaded" (rt_update_geometry).
int update_geometry(rt_ctx* ctx, const rt_vertex* vertices, const QueryPtr& pv, const rt_sphere* spheres, uint32_t n_spheres, const QueryPtr& ps,
                    bool rebuild, uint32_t* stat_flags, double* kernel_ms) {
    const size_t nd = ctx->devs.size();
    // spheres: rt_sphere (20 B) -> the first 20 B of each DevSphere (32 B, padding stays zero): one strided copy, no kernel
    if (spheres && n_spheres) {
        std::vector<rt_sphere> staged;
        const void* src = spheres;
        if (ps.device && nd > 1) { // device input for several devices: through the host
            staged.resize(n_spheres);
            HIPCHK(ctx, hipSetDevice(ctx->devs[ps.dev].device));
            HIPCHK(ctx, hipMemcpy(staged.data(), spheres, n_spheres * sizeof(rt_sphere), hipMemcpyDeviceToHost));
            src = staged.data();
        }
        for (auto& d : ctx->devs) {
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, hipMemcpy2DAsync(d.spheres, sizeof(DevSphere), src, sizeof(rt_sphere), sizeof(rt_sphere), n_spheres, hipMemcpyDefault, d.stream));
            HIPCHK(ctx, hipStreamSynchronize(d.stream));
        }
    }
    if (!vertices || ctx->up_vertices == 0) return RT_OK;
    // vertices: a copy on every device (the refit reads it; after device input it is also what a later readback reads)
    const size_t vbytes = (size_t)ctx->up_vertices * sizeof(rt_vertex);
    for (auto& d : ctx->devs)
        if (!d.rf_verts) {
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, hipMalloc((void**)&d.rf_verts, vbytes));
        }
    if (!pv.device) {
        for (auto& d : ctx->devs) {
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, hipMemcpyAsync(d.rf_verts, vertices, vbytes, hipMemcpyHostToDevice, d.stream));
        }
    } else {
        DeviceState& s = ctx->devs[pv.dev];
        HIPCHK(ctx, hipSetDevice(s.device));
        HIPCHK(ctx, hipMemcpyAsync(s.rf_verts, vertices, vbytes, hipMemcpyDeviceToDevice, s.stream));
        HIPCHK(ctx, hipStreamSynchronize(s.stream));
        std::vector<float> staged;
        for (size_t j = 0; j < nd; j++) {
            if (j == pv.dev) continue;
            DeviceState& d = ctx->devs[j];
            HIPCHK(ctx, hipSetDevice(d.device));
            if (staged.empty() && hipMemcpyPeer(d.rf_verts, d.device, s.rf_verts, s.device, vbytes) == hipSuccess) continue;
            (void)hipGetLastError(); // no peer copy between these two: through the host
            if (staged.empty()) {
                staged.resize(3 * (size_t)ctx->up_vertices);
                HIPCHK(ctx, hipSetDevice(s.device));
                HIPCHK(ctx, hipMemcpy(staged.data(), s.rf_verts, vbytes, hipMemcpyDeviceToHost));
                HIPCHK(ctx, hipSetDevice(d.device));
            }
            HIPCHK(ctx, hipMemcpy(d.rf_verts, staged.data(), vbytes, hipMemcpyHostToDevice));
        }
    }
    drop_grids(ctx);
    if (!rebuild) {
        if (int rc = ensure_refit_view(ctx)) return rc;
        if (ctx->rf_n_dropped) { // a triangle the tree has no record of may have become finite: then only a new tree places it
            DeviceState& d = ctx->devs[0];
            uint32_t flag = 0;
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, hipMemsetAsync(d.rf_flag, 0, sizeof(uint32_t), d.stream));
            HIPCHK(ctx, rt::launch_refit_any_finite(d.rf_dropped, ctx->rf_n_dropped, d.rf_verts, d.rf_flag, d.stream));
            HIPCHK(ctx, hipMemcpyAsync(&flag, d.rf_flag, sizeof flag, hipMemcpyDeviceToHost, d.stream));
            HIPCHK(ctx, hipStreamSynchronize(d.stream));
            rebuild = flag != 0;
        }
    }
    if (rebuild) {
        std::vector<float> staged;
        const float* hv = reinterpret_cast<const float*>(vertices);
        if (pv.device) {
            if (int rc = read_positions(ctx, staged)) return rc;
            hv = staged.data();
        }
        gather_positions(ctx, hv);
        ctx->host_geometry_stale = false;
        TreeBuild tb(ctx);
        if (int rc = build_tree(ctx, ctx->build_tris, tree_method(ctx->build_tris.size()), knob_build_options(), tb)) return rc;
        if (int rc = install_tree(ctx, tb)) return rc;
        *stat_flags = RT_STAT_REBUILT;
        return RT_OK;
    }
    // the refit: every device's launches are queued before any is waited for
    const std::vector<uint32_t>& lv = ctx->rf_level_first;
    for (auto& d : ctx->devs) {
        HIPCHK(ctx, hipSetDevice(d.device));
        HIPCHK(ctx, hipEventRecord(d.ev0, d.stream));
        HIPCHK(ctx, rt::launch_refit_tris(d.tris, d.rf_vidx, d.rf_verts, ctx->scene_counts.n_tris, d.stream));
        for (size_t l = lv.size() - 1; l-- > 0;) // deepest level first
            HIPCHK(ctx, rt::launch_refit_nodes(d.nodes, d.rf_boxes, d.tris, d.rf_vidx, d.rf_verts, d.rf_order + lv[l], lv[l + 1] - lv[l], d.stream));
        HIPCHK(ctx, hipEventRecord(d.ev1, d.stream));
    }
    for (auto& d : ctx->devs) {
        HIPCHK(ctx, hipSetDevice(d.device));
        HIPCHK(ctx, hipStreamSynchronize(d.stream));
        float ms = 0.0f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, d.ev0, d.ev1));
        *kernel_ms = std::max(*kernel_ms, (double)ms);
    }
    if (pv.device) ctx->host_geometry_stale = true; // read back when rt_prepare or the light grids need it
    else {
        gather_positions(ctx, reinterpret_cast<const float*>(vertices));
        ctx->host_geometry_stale = false;
    }
    *stat_flags = RT_STAT_REFIT;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_update_geometry(rt_ctx* ctx, const rt_vertex* vertices, uint32_t n_vertices, const rt_sphere* spheres, uint32_t n_spheres, uint32_t flags) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (flags & ~RT_UPDATE_REBUILD) return ctx->fail(RT_ERR_BAD_ARG, "rt_update_geometry: unknown flag bits 0x%x", flags & ~RT_UPDATE_REBUILD);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_update_geometry: no scene uploaded");
    if (!vertices && n_vertices) return ctx->fail(RT_ERR_BAD_ARG, "rt_update_geometry: vertices is NULL with n_vertices = %u", n_vertices);
    if (!spheres && n_spheres) return ctx->fail(RT_ERR_BAD_ARG, "rt_update_geometry: spheres is NULL with n_spheres = %u", n_spheres);
    if (vertices && n_vertices != ctx->up_vertices)
        return ctx->fail(RT_ERR_BAD_ARG, "rt_update_geometry: %u vertices, the scene was uploaded with %u", n_vertices, ctx->up_vertices);
    if (spheres && n_spheres != ctx->scene_counts.n_spheres)
        return ctx->fail(RT_ERR_BAD_ARG, "rt_update_geometry: %u spheres, the scene was uploaded with %u", n_spheres, ctx->scene_counts.n_spheres);
    if (int rcp = sync_pending(ctx)) return rcp; // a dispatch in flight still reads the old positions
    QueryPtr pv, ps;
    if (vertices && n_vertices)
        if (int rc = classify_ptr(ctx, "rt_update_geometry", "vertices", vertices, pv, 4)) return rc;
    if (spheres && n_spheres)
        if (int rc = classify_ptr(ctx, "rt_update_geometry", "spheres", spheres, ps, 4)) return rc;
    uint32_t stat_flags = 0;
    double kernel_ms = 0.0;
    end_accumulation(ctx); // moved geometry: the samples so far are of another scene
    const int rc = update_geometry(ctx, n_vertices ? vertices : nullptr, pv, spheres, n_spheres, ps, (flags & RT_UPDATE_REBUILD) != 0, &stat_flags, &kernel_ms);
    if (rc != RT_OK) { // as a failed upload: nothing is left pointing at half-written arrays (the last frame stays readable)
        drop_scene(ctx);
        return rc;
    }
    rt_stats& st = ctx->stats;
    st.rays = st.primary_rays = st.continuation_rays = st.shadow_rays = st.pixels = 0;
    st.node_visits = st.tri_tests = 0;
    st.flags = stat_flags;
    st.kernel_ms = kernel_ms;
    st.wall_ms = now_ms() - w0;
    return RT_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// Feature buffers and denoising (rt_hip.h "Feature buffers (AOVs) and denoising"): rt_aovs, rt_sample_rays, rt_denoise.  Kernels in
// denoise.hip.  None of them touches the frame targets, the tile shares rt_read_* gather, or the running image of an accumulation.
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

// The jitter rule of the frames: a closed frame jitters when it has several samples (frame_of_params), an accumulation always.
void sample_jitter(DevFrame& fr, uint32_t flags) {
    if (flags & RT_FLAG_ACCUMULATE) fr.jitter = 1u;
}

void drain_streams(rt_ctx* ctx) { // after a failure: nothing of the call is left writing into the caller's memory
    for (auto& d : ctx->devs) {
        (void)hipSetDevice(d.device);
        (void)hipStreamSynchronize(d.stream);
    }
}

// One device's share of rt_aovs, enqueued: zero the frame's records (the pixels outside the share stay zero), then the samples in runs of
// at most RT_AOV_SAMPLES_PER_LAUNCH, between the device's query event pair.
int enqueue_aovs(rt_ctx* ctx, DeviceState& d, const DevFrame& f, void* acc, size_t bytes) {
    HIPCHK(ctx, hipSetDevice(d.device));
    if (int rc = ensure_query_events(ctx, d, 2)) return rc;
    HIPCHK(ctx, hipMemsetAsync(acc, 0, bytes, d.stream));
    HIPCHK(ctx, hipEventRecord(d.rq_events[0], d.stream));
    const DevScene sc = scene_for(ctx, d);
    for (uint32_t s0 = 0; s0 < f.n_total; s0 += RT_AOV_SAMPLES_PER_LAUNCH)
        HIPCHK(ctx, rt::launch_aov_samples(sc, f, s0, std::min(RT_AOV_SAMPLES_PER_LAUNCH, f.n_total - s0), acc, d.stream));
    HIPCHK(ctx, hipEventRecord(d.rq_events[1], d.stream));
    return RT_OK;
}

int aovs(rt_ctx* ctx, const rt_render_params* p, rt_aov* out) {
    const double w0 = now_ms();
    uint32_t world = 1, rank = 0;
    DevFrame fr{};
    if (int rc = frame_of_params(ctx, "rt_aovs", p, fr, world, rank)) return rc;
    if (!out) return ctx->fail(RT_ERR_BAD_ARG, "rt_aovs: out is NULL");
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr po;
    if (int rc = classify_ptr(ctx, "rt_aovs", "out", out, po)) return rc;
    sample_jitter(fr, p->flags);
    const size_t n = (size_t)fr.width * fr.height, bytes = n * sizeof(rt_aov);
    const size_t nd = ctx->devs.size();
    const bool in_place = po.device && nd == 1; // else every device works on its own records and the shares are put together here
    std::vector<DevFrame> share(nd, fr);
    for (size_t j = 0; j < nd; j++) {
        DeviceState& d = ctx->devs[j];
        frame_share(share[j], world, rank, nd, j);
        HIPCHK(ctx, hipSetDevice(d.device));
        if (!in_place)
            if (int rc = ensure_buffer(ctx, &d.dn_aov, &d.dn_aov_bytes, bytes)) return rc;
        if (int rc = enqueue_aovs(ctx, d, share[j], in_place ? (void*)out : d.dn_aov, bytes)) {
            drain_streams(ctx);
            return rc;
        }
    }
    double kernel_ms = 0.0;
    uint64_t pixels = 0;
    for (size_t j = 0; j < nd; j++) {
        DeviceState& d = ctx->devs[j];
        hipError_t e = hipSetDevice(d.device);
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        if (e != hipSuccess) {
            drain_streams(ctx);
            return ctx->fail(RT_ERR_HIP, "rt_aovs: device %d: %s", d.device, hipGetErrorString(e));
        }
        float ms = 0.0f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, d.rq_events[0], d.rq_events[1]));
        kernel_ms = std::max(kernel_ms, (double)ms);
        pixels += owned_pixels(share[j], share[j].tile_first, share[j].tile_stride, share[j].n_owned_tiles);
    }
    if (!in_place && nd == 1) {
        HIPCHK(ctx, hipSetDevice(ctx->devs[0].device));
        HIPCHK(ctx, hipMemcpy(out, ctx->devs[0].dn_aov, bytes, hipMemcpyDeviceToHost));
    } else if (!in_place) { // several devices: each holds its own tiles; zeros elsewhere, as rt_read_rgb32f gives them
        std::vector<uint8_t> whole(bytes, 0), tmp(bytes);
        for (size_t j = 0; j < nd; j++) {
            const DeviceState& d = ctx->devs[j];
            const DevFrame& f = share[j];
            if (f.n_owned_tiles == 0) continue;
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, hipMemcpy(tmp.data(), d.dn_aov, bytes, hipMemcpyDeviceToHost));
            copy_share(whole.data(), tmp.data(), sizeof(rt_aov), f.width, f.height, f.tile_size, f.tiles_x, f.tile_first, f.tile_stride, f.n_owned_tiles);
        }
        if (po.device) {
            HIPCHK(ctx, hipSetDevice(ctx->devs[po.dev].device));
            HIPCHK(ctx, hipMemcpy(out, whole.data(), bytes, hipMemcpyHostToDevice));
        } else {
            std::memcpy(out, whole.data(), bytes);
        }
    }
    rt_stats& st = ctx->stats;
    st.pixels = pixels;
    st.rays = st.primary_rays = pixels * fr.n_total;
    st.continuation_rays = st.shadow_rays = st.node_visits = st.tri_tests = 0;
    st.kernel_ms = kernel_ms;
    st.wall_ms = now_ms() - w0;
    return RT_OK;
}

int check_sigma(rt_ctx* ctx, const char* name, float s) {
    if (!(s > 0.0f) || !std::isfinite(s)) return ctx->fail(RT_ERR_BAD_ARG, "rt_denoise: %s %g (finite and > 0)", name, (double)s);
    return RT_OK;
}

int denoise(rt_ctx* ctx, const rt_denoise_params* dp, const float* rgb, const rt_aov* aov, float* out) {
    const double w0 = now_ms();
    if (!dp || !rgb || !aov || !out)
        return ctx->fail(RT_ERR_BAD_ARG, "rt_denoise: %s is NULL", !dp ? "params" : !rgb ? "rgb" : !aov ? "aov" : "out");
    if (dp->width == 0 || dp->height == 0 || dp->width > 65535u * 8u || dp->height > 65535u * 8u)
        return ctx->fail(RT_ERR_BAD_ARG, "rt_denoise: bad resolution %ux%u", dp->width, dp->height);
    if (dp->iterations < 1 || dp->iterations > RT_DENOISE_MAX_ITERATIONS)
        return ctx->fail(RT_ERR_BAD_ARG, "rt_denoise: iterations %u (1 .. %u)", dp->iterations, RT_DENOISE_MAX_ITERATIONS);
    if (dp->flags & ~RT_DENOISE_DEMODULATE) return ctx->fail(RT_ERR_BAD_ARG, "rt_denoise: unknown flag bits 0x%x", dp->flags & ~RT_DENOISE_DEMODULATE);
    if (int rc = check_sigma(ctx, "sigma_color", dp->sigma_color)) return rc;
    if (int rc = check_sigma(ctx, "sigma_normal", dp->sigma_normal)) return rc;
    if (int rc = check_sigma(ctx, "sigma_depth", dp->sigma_depth)) return rc;
    if (int rc = check_sigma(ctx, "sigma_albedo", dp->sigma_albedo)) return rc;
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pr, pa, po;
    if (int rc = classify_ptr(ctx, "rt_denoise", "rgb", rgb, pr, 4)) return rc;
    if (int rc = classify_ptr(ctx, "rt_denoise", "aov", aov, pa, 16)) return rc;
    if (int rc = classify_ptr(ctx, "rt_denoise", "out", out, po, 4)) return rc;
    if (pr.device != pa.device || pr.device != po.device || pr.dev != pa.dev || pr.dev != po.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "rt_denoise: rgb, aov and out must all be host memory or all device memory of the same device");
    const bool device = pr.device;
    DeviceState& d = ctx->devs[pr.dev]; // host buffers: the first device
    const uint32_t n = dp->width * dp->height;
    if ((size_t)dp->width * dp->height > 0xFFFFFFFFull) return ctx->fail(RT_ERR_BAD_ARG, "rt_denoise: %ux%u pixels", dp->width, dp->height);
    HIPCHK(ctx, hipSetDevice(d.device));
    for (int k = 0; k < 2; k++)
        if (int rc = ensure_buffer(ctx, &d.dn_plane[k], &d.dn_plane_bytes[k], (size_t)n * 16)) return rc;
    if (!device) {
        if (int rc = ensure_buffer(ctx, &d.dn_rgb, &d.dn_rgb_bytes, (size_t)n * 12)) return rc;
        if (int rc = ensure_buffer(ctx, &d.dn_aov, &d.dn_aov_bytes, (size_t)n * sizeof(rt_aov))) return rc;
    }
    if (int rc = ensure_query_events(ctx, d, 2)) return rc;
    const float* c_rgb = device ? rgb : (const float*)d.dn_rgb;
    const void* c_aov = device ? (const void*)aov : d.dn_aov;
    float* c_out = device ? out : (float*)d.dn_rgb; // the pack has read the staged rgb before the last iteration writes over it
    float4* plane[2] = {(float4*)d.dn_plane[0], (float4*)d.dn_plane[1]};
    const bool demod = (dp->flags & RT_DENOISE_DEMODULATE) != 0;
    auto enqueue = [&]() -> hipError_t {
        hipError_t e = hipSuccess;
        if (!device) {
            if ((e = hipMemcpyAsync(d.dn_rgb, rgb, (size_t)n * 12, hipMemcpyHostToDevice, d.stream)) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(d.dn_aov, aov, (size_t)n * sizeof(rt_aov), hipMemcpyHostToDevice, d.stream)) != hipSuccess) return e;
        }
        if ((e = hipEventRecord(d.rq_events[0], d.stream)) != hipSuccess) return e;
        if ((e = rt::launch_denoise_pack(c_rgb, c_aov, plane[0], n, demod, d.stream)) != hipSuccess) return e;
        for (uint32_t i = 0; i < dp->iterations; i++) {
            rt::AtrousParams ap;
            ap.width = dp->width, ap.height = dp->height, ap.iter = i;
            const float sc = dp->sigma_color * std::ldexp(1.0f, -(int)i); // sigma_color * 2^-i
            ap.inv_sc2 = 1.0f / (sc * sc);
            ap.inv_sn2 = 1.0f / (dp->sigma_normal * dp->sigma_normal);
            ap.sigma_depth = dp->sigma_depth;
            ap.inv_sa2 = 1.0f / (dp->sigma_albedo * dp->sigma_albedo);
            ap.demodulate = demod;
            const bool last = i + 1 == dp->iterations;
            if ((e = rt::launch_denoise_atrous(ap, plane[i & 1], c_aov, plane[(i + 1) & 1], c_out, last, d.stream)) != hipSuccess) return e;
        }
        if ((e = hipEventRecord(d.rq_events[1], d.stream)) != hipSuccess) return e;
        if (!device) e = hipMemcpyAsync(out, d.dn_rgb, (size_t)n * 12, hipMemcpyDeviceToHost, d.stream);
        return e;
    };
    hipError_t e = enqueue();
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    if (e != hipSuccess) {
        drain_streams(ctx);
        return ctx->fail(e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, "rt_denoise: %s", hipGetErrorString(e));
    }
    float ms = 0.0f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, d.rq_events[0], d.rq_events[1]));
    rt_stats& st = ctx->stats;
    st.rays = st.primary_rays = st.continuation_rays = st.shadow_rays = st.node_visits = st.tri_tests = 0;
    st.pixels = n;
    st.kernel_ms = ms;
    st.wall_ms = now_ms() - w0;
    return RT_OK;
}

} // namespace

extern "C" {

int rt_aovs(rt_ctx* ctx, const rt_render_params* p, rt_aov* out) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!p) return ctx->fail(RT_ERR_BAD_ARG, "rt_aovs: null params");
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_aovs: no scene uploaded");
    return aovs(ctx, p, out);
}

int rt_sample_rays(rt_ctx* ctx, const rt_render_params* p, uint32_t sample, rt_ray* out) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!p) return ctx->fail(RT_ERR_BAD_ARG, "rt_sample_rays: null params");
    if (p->mode != RT_MODE_EXTENDED) return ctx->fail(RT_ERR_BAD_ARG, "rt_sample_rays: mode %u (the extended mode's samples only)", p->mode);
    rt_render_params q = *p;
    q.tile_size = q.tile_rank = q.tile_world = 0; // ignored
    uint32_t world = 1, rank = 0;
    DevFrame fr{};
    if (int rc = frame_of_params(ctx, "rt_sample_rays", &q, fr, world, rank)) return rc;
    if (!out) return ctx->fail(RT_ERR_BAD_ARG, "rt_sample_rays: out is NULL");
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr po;
    if (int rc = classify_ptr(ctx, "rt_sample_rays", "out", out, po)) return rc;
    sample_jitter(fr, p->flags);
    const size_t n = (size_t)fr.width * fr.height;
    DeviceState& d = ctx->devs[po.dev];
    HIPCHK(ctx, hipSetDevice(d.device));
    if (!po.device)
        if (int rc = ensure_buffer(ctx, &d.rq_in, &d.rq_in_bytes, std::min<size_t>(n, RT_QUERY_CHUNK) * sizeof(rt_ray))) return rc;
    uint8_t* dst = reinterpret_cast<uint8_t*>(out);
    for (size_t off = 0; off < n; off += RT_QUERY_CHUNK) { // as rt_camera_rays
        const size_t m = std::min<size_t>(RT_QUERY_CHUNK, n - off);
        void* res = po.device ? (void*)(dst + off * sizeof(rt_ray)) : d.rq_in;
        hipError_t e = rt::launch_sample_rays(fr, sample, res, off, (uint32_t)m, d.stream);
        if (e == hipSuccess && !po.device) e = hipMemcpyAsync(dst + off * sizeof(rt_ray), d.rq_in, m * sizeof(rt_ray), hipMemcpyDeviceToHost, d.stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(d.stream);
            return ctx->fail(RT_ERR_HIP, "rt_sample_rays: %s", hipGetErrorString(e));
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

int rt_denoise(rt_ctx* ctx, const rt_denoise_params* dp, const float* rgb, const rt_aov* aov, float* out) {
    if (!ctx) return RT_ERR_BAD_ARG;
    return denoise(ctx, dp, rgb, aov, out);
}

} // extern "C"
