// rt_internal.h — what the host units of the C ABI (rt_context / rt_scene / rt_frame / rt_readback / rt_query / rt_mesh_query / rt_posed_query .cpp) share: the owner of
// device memory, the per-device state grouped by lifetime, the context, and the helpers more than one unit calls.  Nothing here is
// exported from the library.
#ifndef RT_INTERNAL_H
#define RT_INTERNAL_H

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
#include "closest_point.h"
#include "closest_point_all.h"
#include "contact_capsule.h"
#include "contact_triangle.h"
#include "denoise.h"
#include "device_build.h"
#include "device_layout.h"
#include "direct_light.h"
#include "half.h"
#include "inside.h"
#include "irradiance_query.h"
#include "kernels.h"
#include "overlap.h"
#include "overlap_obb.h"
#include "overlap_triangle.h"
#include "path_query.h"
#include "posed_mesh.h"
#include "probe_query.h"
#include "ray_query.h"
#include "refit.h"
#include "shadow_grid.h"
#include "surface_query.h"
#include "sweep.h"
#include "sweep_box.h"
#include "sweep_capsule.h"
#include "sweep_obb.h"
#include "sweep_triangle.h"
#include "wavefront.h"

#define HIPCHK(ctx, call)                                                                                       \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess)                                                                                   \
            return (ctx)->fail(e_ == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, "%s failed: %s (%s:%d)", #call, \
                               hipGetErrorString(e_), __FILE__, __LINE__);                                     \
    } while (0)

namespace rti __attribute__((visibility("hidden"))) {

// The one owner of a device allocation: a pointer and its size in bytes, freed by the destructor and by reset().  Move-only.
// Pinned = true: page-locked host memory instead (the read-back staging).
template <bool Pinned>
class Mem {
    void* p_ = nullptr;
    size_t bytes_ = 0;
public:
    Mem() = default;
    Mem(void* adopted, size_t bytes) : p_(adopted), bytes_(adopted ? bytes : 0) {} // takes over an allocation made elsewhere
    Mem(Mem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Mem& operator=(Mem&& o) noexcept {
        if (this != &o) reset(), p_ = std::exchange(o.p_, nullptr), bytes_ = std::exchange(o.bytes_, 0);
        return *this;
    }
    ~Mem() { reset(); }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr, bytes_ = 0;
    }
    // Grow on demand, on the current device: an allocation of at least `bytes` stays, a smaller one is freed before the new one is
    // made (contents are not kept).  Empty after a failure.
    hipError_t reserve(size_t bytes) {
        if (bytes_ >= bytes) return hipSuccess;
        reset();
        const hipError_t e = Pinned ? hipHostMalloc(&p_, bytes, hipHostMallocDefault) : hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        else bytes_ = bytes;
        return e;
    }
    void* get() const { return p_; }
};
using DevMem = Mem<false>;
using PinnedMem = Mem<true>;
template <class T>
struct DevBuf : DevMem { // a DevMem whose get() has the element type the kernels take
    using DevMem::DevMem;
    T* get() const { return static_cast<T*>(DevMem::get()); }
};

// One device of a context.  Streams and events are created by rt_create and destroyed by rt_destroy, nowhere else.  Device memory
// sits in groups by what ends its life: releasing a group is `group = {}` (the device current), which also returns the shapes and
// flags kept beside the pointers to their defaults.
struct DeviceState {
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; // the second lane of the wavefront pipeline (batches alternate between the two)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_start = nullptr, ev_join = nullptr, ev_res[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> stage_events; // RT_FLAG_STAGE_TIMES: event pairs around the launches of the dominant stage kernel
    uint32_t stage_events_used = 0;
    std::vector<hipEvent_t> rq_events; // an event pair around each launch of a query
    DevBuf<unsigned long long> counters; // DevTargets::counters, from rt_create to rt_destroy
    uint32_t tile_first = 0, tile_stride = 1, n_owned = 0; // of the last rt_render

    struct Scene { // the tree and the scene arrays: install_tree replaces the first two, free_scene ends all
        DevBuf<DevNode8> nodes;
        DevBuf<DevTri> tris;
        DevBuf<DevSphere> spheres;
        DevBuf<DevLight> lights;
        DevBuf<DevMaterial> materials;
        DevBuf<float> verts; // rt_update_geometry: the positions of the last update (3 floats per vertex)
    } scene;
    struct Grids { // the light grids (shadow_grid.h) hold triangle records of one tree: built again when a frame or rt_prepare needs them
        DevBuf<DevShadowGrid> table; // one per light, empty when no light has a grid
        std::vector<DevMem> allocs;  // the cell blocks and overflow lists behind them (sizes are not reported: adopted with 0)
        std::vector<rt::ShadowGridBuild> info;
        bool tried = false;          // the light grids of the current scene were built (or refused) on this device
    } grids;
    // rt_update_geometry (refit.h): the refit's view of the tree this device holds, made on the first update of that tree, gone with it
    struct Refit {
        DevBuf<uint32_t> vidx;    // per triangle record: the caller's vertex indices (RT_REFIT_NO_RECORD: padding)
        DevBuf<uint32_t> order;   // node ids grouped by tree level (rt_ctx::rf_level_first)
        DevBuf<float4> boxes;     // exact box per node (min, max): scratch of the level launches
        DevBuf<uint32_t> dropped; // vertex indices of the triangles the tree has no record of (non-finite at upload)
        DevBuf<uint32_t> flag;
    } refit;
    struct Targets { // the frame targets of one resolution (ensure_targets) and the read-back staging
        DevBuf<float> rgba32f;
        DevBuf<uint8_t> chan[3];
        DevBuf<uint32_t> prim_id;
        DevBuf<float> hit_t;
        uint32_t w = 0, h = 0;
        DevMem readback_dev;     // epilogue output (combined rgba8 / packed rgb32f), whole-frame single-device reads
        PinnedMem readback_host; // pinned staging for it
    } fb;
    struct Lanes { // the wavefront pipeline's state (extended mode), one allocation shape at a time (ensure_wavefront)
        rt::WfBuffers wf{};  // views into allocs, as the kernels take them
        rt::WfBuffers wf2{}; // ... of the second lane (its own path state, queues and counters in allocs2; the pixel sums and beams are wf's)
        std::vector<DevMem> allocs, allocs2;
        uint32_t lights = 0;
    } pipe;
    bool used_two_lanes = false; // the last pipeline frame ran on two lanes (its allocation is reused by a frame of the same shape)
    uint32_t wf_spp = 0;         // spp the current wavefront allocation was sized for
    struct Query { // ray, surface, direct-light and path queries: staging of host batches (rays or points in, records / bytes out, rt_intersect_all's and rt_closest_point_all's counts, rt_inside's and rt_signed_distance's votes), grown on demand
        DevMem in, out, counts;
        DevBuf<uint32_t> ao; // rt_ambient_occlusion: the per-point counts its kernel adds to, for host and device batches alike
        DevMem mesh;         // rt_overlap_mesh, rt_sweep_mesh: a host mesh's copy on this device, for the duration of the call
        DevBuf<uint4> paths; // rt_radiance with several samples, rt_radiance_sh, rt_irradiance: one record per path of a chunk (at most RT_QUERY_CHUNK), which its reduction / projection adds up
    } rq;
    // RT_FLAG_ACCUMULATE: the running sum of the context's accumulation over this device's pixels (DevTargets::run_sum), frame-pixel
    // layout, w x h x 16 bytes.  Outlives the pipeline's WfBuffers (re-sized with the batch); made by the first accumulating call.
    // rt_render_adaptive: the running sum over the odd-indexed samples (DevTargets::run_odd, same layout, made by the first adaptive call)
    struct Accum {
        DevBuf<float> run_sum, run_odd;
        uint32_t w = 0, h = 0;
    } acc;
    // ... and the selection of a call (adaptive.h): per owned block its mask of pixels that take samples, the list of the blocks with
    // any (cap entries each), the two counts k_ad_compact leaves on the device, and what the host read of them for the last call
    struct Adaptive {
        DevBuf<unsigned long long> mask;
        DevBuf<uint32_t> blocks;
        DevBuf<unsigned long long> counts;
        uint32_t cap = 0, live_blocks = 0;
        uint64_t pixels = 0;
    } ad;
    // rt_aovs / rt_denoise (denoise.h), grown on demand, kept until rt_destroy (they do not depend on the scene): the records of the
    // device's share when they cannot be written in place, the staging of host rgb, and the two colour planes of the a-trous iterations
    struct Denoise {
        DevMem aov, rgb;
        DevBuf<float4> plane[2];
    } dn;
};

// What an accumulating rt_render must share with the previous one to continue its running image (rt_hip.h, RT_FLAG_ACCUMULATE): the
// parameters that change the bits of a sample.  Compared bytewise (all 4-byte fields, no padding): the camera bit for bit.
struct AccumKey {
    rt_camera camera;
    uint32_t width, height, max_bounces, frame_seed, tile_size, tile_rank, tile_world, no_shadows;
    uint32_t adaptive; // the running image of rt_render_adaptive (per-pixel counts) is not continued by plain accumulating calls, nor the reverse
};

} // namespace rti

struct rt_ctx {
    std::vector<rti::DeviceState> devs;
    std::string err;
    bool uploaded = false;
    bool pending_dispatch = false; // rt_dispatch_tile launches are not waited for (the reference's queue.submit is not either); see sync_pending
    DevScene scene_counts{}; // counts; pointers are per device
    rt_stats stats{};
    uint32_t frame_w = 0, frame_h = 0, frame_tile = RT_TILE_SIZE, frame_tiles_x = 0, frame_tiles_y = 0;
    bool frame_valid = false;
    unsigned long long diag[RT_CNT_N_DIAG] = {0}; // diagnostics of the counting kernel variant (rt_debug_counters)
    unsigned long long grid_diag[2] = {0}; // ... of the light grids: shadow segments they answered, list entries read (the last counting frame or rt_direct_light)
    double stage_ms[2] = {0.0, 0.0};       // RT_FLAG_STAGE_TIMES: [0] sum of the k_wf_shadow_grid launch durations of the last frame (device 0), [1] launches
    int fail_upload_at = -1;          // test hook: the next scene upload fails before its k-th device array (rt_debug_fail_upload)
    uint32_t n_input_tris = 0;        // triangles handed to the last scene upload (prim ids are < this)
    std::vector<rt::BuildTri> build_tris; // the triangles of the last upload as the builders take them (rt_prepare RT_PREPARE_QUALITY_TREE rebuilds from them)
    std::vector<DevLight> host_lights; // what the lazy light-grid build needs of the last upload: the lights, ...
    float box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0}; // ... the box of the triangles with finite vertices
    std::vector<rt_triangle> up_triangles; // the triangles of the last upload in build_tris order (rt_update_geometry gathers through them)
    std::vector<uint32_t> up_prim_ids;     // ... their prim ids when they are not the index (rt_upload_scene_packed)
    uint32_t up_vertices = 0;              // vertex count of the last upload
    bool rf_ready = false;                 // the devices hold the refit's view of the current tree (DeviceState::refit)
    std::vector<uint32_t> rf_level_first;  // refit.order offsets of the tree levels, root level first, plus the end
    uint32_t rf_n_dropped = 0;             // triangles without a record
    bool host_geometry_stale = false;      // build_tris / box_lo / box_hi lag behind device-resident positions in devs[0].scene.verts
    uint32_t n_textures = 0;          // bindings 6-7 as last handed over (rt_upload_textures); never sampled, like the reference
    uint64_t texture_bytes = 0;
    rti::AccumKey acc_key{};               // RT_FLAG_ACCUMULATE: the parameters of the running image ...
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

namespace rti __attribute__((visibility("hidden"))) {

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The context's running image ends: the next accumulating rt_render starts at sample 0 (its buffers stay for it).  Called by the scene's
// owners (drop_scene, rt_update_geometry), by every frame or dispatch that is not an accumulating one, and by an accumulating call before
// its launches, so that a call that fails part way never leaves a half-added sum counted.
inline void end_accumulation(rt_ctx* ctx) { ctx->acc_samples = 0; }

struct QueryPtr {
    bool device = false; // device memory of one of the context's devices (else host memory of any kind: staged)
    size_t dev = 0;      // ... its index in ctx->devs
};

int sync_pending(rt_ctx* ctx); // rt_context.cpp
void free_scene(DeviceState& d); // rt_scene.cpp, with the next
int ensure_grids(rt_ctx* ctx, DeviceState& d);
DevCamera make_camera(const rt_camera& cam, float res_x, float res_y, bool wavefront); // rt_frame.cpp, with the next four
DevScene scene_for(const rt_ctx* ctx, const DeviceState& d);
void frame_share(DevFrame& f, uint32_t world, uint32_t rank, size_t nd, size_t j);
uint64_t owned_pixels(const DevFrame& fr, uint32_t first, uint32_t stride, uint32_t n_owned);
int frame_of_params(rt_ctx* ctx, const char* fn, const rt_render_params* p, DevFrame& fr, uint32_t& world, uint32_t& rank);
void copy_share(uint8_t* dst, const uint8_t* src, size_t elem, uint32_t w, uint32_t h, uint32_t ts, uint32_t tiles_x, uint32_t first, uint32_t stride,
                uint32_t n_owned); // rt_readback.cpp, with the next
int consolidate_on_first_device(rt_ctx* ctx, uint32_t w, uint32_t h);
int classify_ptr(rt_ctx* ctx, const char* fn, const char* what, const void* p, QueryPtr& q, uintptr_t align = 16); // rt_query.cpp
// rt_query.cpp: the one-record-in, one-record-out batch with its argument types, for every call of that shape (rt_intersect ..
// rt_sweep_capsule there; rt_sweep_triangle in rt_mesh_query.cpp).  launch: the call's kernel launcher.
enum Stage { ST_OUT, ST_COUNTS, ST_AO, ST_PATHS }; // a buffer of DeviceState::rq
struct BatchIn {
    const char* name; // in messages
    const void* p;
    size_t size;      // bytes per record
};
struct BatchOut {
    const char* name = nullptr;
    void* p = nullptr;    // null: an output the call does not have, or the caller did not ask for
    size_t size = 0;
    uintptr_t align = 16; // asked of device memory
    Stage stage = ST_OUT; // where a host batch's chunk of it is written before it is copied back
};
using RecordLaunch = hipError_t (*)(const DevScene&, const void*, void*, uint32_t, unsigned long long*, hipStream_t);
int record_query(rt_ctx* ctx, const char* fn, BatchIn in, size_t n, BatchOut out, uint32_t flags, RecordLaunch launch);
// rt_query.cpp: the argument checks and the batch of rt_overlap_box, for every call of its shape (rt_overlap_obb; rt_overlap_triangle
// in rt_mesh_query.cpp).  in_name: the input array in messages; in_size: bytes per input record; launch: the call's kernel launcher.
using OverlapLaunch = hipError_t (*)(const DevScene&, const void*, uint32_t*, uint32_t*, uint32_t, uint32_t, int, unsigned long long*, hipStream_t);
int overlap_query(rt_ctx* ctx, const char* fn, const char* in_name, const void* in, size_t in_size, size_t n, uint32_t max_prims, uint32_t* prims,
                  uint32_t* counts, uint32_t flags, OverlapLaunch launch);
// rt_query.cpp: the argument checks and the batch of rt_contact_capsule, for every call of its shape (rt_contact_triangle in
// rt_mesh_query.cpp).  out: max_contacts 32-byte records per query.  in_name, in_size, launch: as for overlap_query.
using ContactLaunch = hipError_t (*)(const DevScene&, const void*, void*, uint32_t*, uint32_t, uint32_t, int, unsigned long long*, hipStream_t);
int contact_query(rt_ctx* ctx, const char* fn, const char* in_name, const void* in, size_t in_size, size_t n, uint32_t max_contacts, void* out,
                  uint32_t* counts, uint32_t flags, ContactLaunch launch);
// rt_query.cpp: the argument checks and the batch of the posed-mesh calls (rt_overlap_mesh, rt_sweep_mesh in rt_posed_query.cpp): a mesh
// of m rt_query_triangle given once, one record per pose in, one or two per pose out (out1.p null: none).  launch gets the mesh as
// the device holds it; mode is handed through to it.
using PoseLaunch = hipError_t (*)(const DevScene&, const void* mesh, uint32_t m, const void* poses, void* out0, void* out1, uint32_t n, uint32_t mode,
                                  unsigned long long*, hipStream_t);
int pose_query(rt_ctx* ctx, const char* fn, const void* mesh, size_t m, BatchIn in, size_t n, BatchOut out0, BatchOut out1, uint32_t flags, uint32_t mode,
               PoseLaunch launch);

} // namespace rti
#endif
