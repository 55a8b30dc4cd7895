// rt_context.cpp — the context of the C ABI (include/rt_hip.h): creation and teardown, the wait for an rt_dispatch_tile in flight,
// statistics and the development read-outs.  No CPU fallback: every compute entry point needs a HIP device and fails with RT_ERR_HIP
// otherwise.
#include "rt_internal.h"

#include "bvh_check.h"

namespace rti {
namespace { thread_local std::string g_create_error; }

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

} // namespace rti

using namespace rti;

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
        const int id = device_ids ? device_ids[i] : i;
        if (id < 0 || id >= count) {
            g_create_error = "rt_create: device id out of range";
            rt_destroy(ctx);
            return RT_ERR_BAD_ARG;
        }
        ctx->devs.emplace_back(); // made in place: rt_destroy releases whatever the steps below got as far as creating
        DeviceState& d = ctx->devs.back();
        d.device = id;
        if ((e = hipSetDevice(d.device)) != hipSuccess || (e = hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking)) != hipSuccess || (e = hipStreamCreateWithFlags(&d.stream2, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&d.ev_start, hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&d.ev_join, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&d.ev_res[0], hipEventDisableTiming)) != hipSuccess || (e = hipEventCreateWithFlags(&d.ev_res[1], hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreate(&d.ev0)) != hipSuccess || (e = hipEventCreate(&d.ev1)) != hipSuccess ||
            (e = d.counters.reserve(RT_CNT_SLOTS * sizeof(unsigned long long))) != hipSuccess) {
            g_create_error = std::string("rt_create: ") + hipGetErrorString(e);
            rt_destroy(ctx);
            return RT_ERR_HIP;
        }
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
        free_scene(d); // device memory first (nothing is left for ~rt_ctx to free), then the events, then the streams
        d.fb = {};
        d.pipe = {};
        d.dn = {};
        d.counters.reset();
        for (hipEvent_t e : {d.ev0, d.ev1, d.ev_start, d.ev_join, d.ev_res[0], d.ev_res[1]})
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : d.stage_events) (void)hipEventDestroy(e);
        for (hipEvent_t e : d.rq_events) (void)hipEventDestroy(e);
        if (d.stream2) (void)hipStreamDestroy(d.stream2);
        if (d.stream) (void)hipStreamDestroy(d.stream);
    }
    delete ctx;
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
// hashes of the node and triangle arrays (the device build lays its tree out exactly as the host's PLOC build does; rtcheck::hash_nodes / hash_tris); returns the number of failures.
int rt_debug_check_bvh(rt_ctx* ctx, uint32_t out[8]) {
    if (!ctx || !ctx->uploaded) return -1;
    DeviceState& d = ctx->devs[0];
    if (hipSetDevice(d.device) != hipSuccess) return -1;
    (void)hipStreamSynchronize(d.stream);
    rt::BvhBuild b;
    b.nodes.resize(ctx->scene_counts.n_nodes);
    b.tris.resize(ctx->scene_counts.n_tris);
    if (!b.nodes.empty() && hipMemcpy(b.nodes.data(), d.scene.nodes.get(), b.nodes.size() * sizeof(DevNode8), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (!b.tris.empty() && hipMemcpy(b.tris.data(), d.scene.tris.get(), b.tris.size() * sizeof(DevTri), hipMemcpyDeviceToHost) != hipSuccess) return -1;
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
        out[6] = rtcheck::hash_nodes(b);
        out[7] = rtcheck::hash_tris(b);
    }
    return fails;
}

// Development aids (not part of rt_hip.h): the queue allocation bound and the window rule, host-only arithmetic (tests/test_queue_bound.py).
unsigned long long rt_debug_queue_slots(unsigned long long max_entries, uint32_t per_lane, unsigned long long waves) {
    return rt::wf_queue_slots_for((size_t)max_entries, per_lane, (size_t)waves);
}
uint32_t rt_debug_pick_window(uint32_t iterations, uint32_t per_lane) { return rt::wf_pick_window(iterations, per_lane); }
unsigned long long rt_debug_state_slots(unsigned long long paths, unsigned long long waves) { return rt::wf_state_slots_for((size_t)paths, (size_t)waves); }

// Development aid: the camera beams of the last extended-mode frame on the first device: per owned 8x8 pixel block the length of its
// triangle list (0xFFFFFFFF: no list).  Returns the number of blocks (<= n), negative on error.
int rt_debug_beams(rt_ctx* ctx, uint32_t* counts, uint32_t n) {
    if (!ctx || ctx->devs.empty()) return RT_ERR_BAD_ARG;
    DeviceState& d = ctx->devs[0];
    if (!d.pipe.wf.beam_count) return 0;
    if (hipSetDevice(d.device) != hipSuccess) return RT_ERR_HIP;
    (void)hipStreamSynchronize(d.stream);
    const uint32_t m = std::min(n, d.pipe.wf.n_blocks);
    if (m && hipMemcpy(counts, d.pipe.wf.beam_count, (size_t)m * 4, hipMemcpyDeviceToHost) != hipSuccess) return RT_ERR_HIP;
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
// entries, bytes, shadow segments the grids answered in the last frame rendered with RT_FLAG_COUNTERS or the last rt_direct_light with
// RT_QUERY_COUNTERS, list entries read, 0, 0, 0}.
int rt_debug_shadow_grid(rt_ctx* ctx, uint32_t light, unsigned long long out[8]) {
    if (!ctx || !out) return RT_ERR_BAD_ARG;
    for (int k = 0; k < 8; k++) out[k] = 0;
    if (ctx->devs.empty()) return RT_OK;
    const DeviceState& d = ctx->devs[0];
    if (light == 0xFFFFFFFFu) {
        for (const rt::ShadowGridBuild& g : d.grids.info) {
            if (g.grid.kind == RT_SG_KIND_NONE) continue;
            out[0]++;
            out[1] += g.n_entries;
            out[2] += g.bytes;
        }
        out[3] = ctx->grid_diag[0];
        out[4] = ctx->grid_diag[1];
        return RT_OK;
    }
    if (light >= d.grids.info.size()) return RT_OK;
    const rt::ShadowGridBuild& g = d.grids.info[light];
    out[0] = g.grid.kind;
    out[1] = g.grid.res;
    out[2] = g.n_entries;
    out[3] = g.near_count;
    out[4] = g.longest;
    out[5] = g.heavy_cells;
    out[6] = g.filled_cells;
    return RT_OK;
}

int rt_get_stats(rt_ctx* ctx, rt_stats* out) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!out) return ctx->fail(RT_ERR_BAD_ARG, "rt_get_stats: null out");
    if (int rcp = sync_pending(ctx)) return rcp;
    *out = ctx->stats;
    return RT_OK;
}

} // extern "C"
