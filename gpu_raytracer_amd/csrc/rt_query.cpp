// rt_query.cpp — calls that trace or filter outside a frame: ray queries (rt_hip.h "Ray queries": rt_intersect, rt_occluded,
// rt_intersect_all, rt_camera_rays), surface queries ("Surface queries": rt_surface, rt_ambient_occlusion; kernels in
// surface_query.hip), the direct-light query ("Direct-light queries": rt_direct_light; kernel in direct_light.hip), the path query ("Path queries":
// rt_radiance; kernels in path_query.hip), the probe query ("Probe queries": rt_radiance_sh; kernels in probe_query.hip), the irradiance query ("Irradiance queries": rt_irradiance; kernels in irradiance_query.hip), the closest-point queries ("Closest-point queries": rt_closest_point, rt_closest_point_all; kernels in closest_point.hip, closest_point_all.hip), the inside test and the signed distance ("Inside tests and signed distance": rt_inside, rt_signed_distance; kernel in inside.hip), the sphere sweep ("Sphere sweeps": rt_sweep_sphere; kernel in sweep.hip), the box sweep ("Box sweeps": rt_sweep_box; kernel in sweep_box.hip), the capsule sweep ("Capsule sweeps": rt_sweep_capsule; kernel in sweep_capsule.hip), the overlap query ("Overlap queries": rt_overlap_box; kernel in overlap.hip; its checks and batch, overlap_query, also serve rt_overlap_obb and rt_mesh_query.cpp), the contact query ("Contact queries": rt_contact_capsule; kernel in contact_capsule.hip; its checks and batch, contact_query, also serve rt_mesh_query.cpp), the checks, the mesh placement and the batch of the posed-mesh queries ("Posed meshes": pose_query, which serves rt_posed_query.cpp; kernels in posed_mesh.hip) and the image passes ("Feature buffers (AOVs) and denoising": rt_aovs, rt_sample_rays, rt_denoise; kernels in
// denoise.hip).  None of them touches the frame targets, the tile shares rt_read_* gather, or the running image of an accumulation.
#include "rt_internal.h"
#include "contact_capsule_rules.h"
#include "inside_rules.h"
#include "overlap_rules.h"
#include "query_plan.h"

namespace rti {
// Where `p` lives.  Pageable memory the runtime has never seen may come back as an error or as unregistered: both are host memory.
int classify_ptr(rt_ctx* ctx, const char* fn, const char* what, const void* p, QueryPtr& q, uintptr_t align) {
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

namespace {

int ensure_query_events(rt_ctx* ctx, DeviceState& d, size_t n) {
    while (d.rq_events.size() < n) {
        hipEvent_t e = nullptr;
        HIPCHK(ctx, hipEventCreate(&e));
        d.rq_events.push_back(e);
    }
    return RT_OK;
}

void drain_streams(rt_ctx* ctx) { // after a failure: nothing of the call is left writing into the caller's memory
    for (auto& d : ctx->devs) {
        (void)hipSetDevice(d.device);
        (void)hipStreamSynchronize(d.stream);
    }
}

// ---- batch calls: an array of records in, one or two arrays of records out ------------------------------------------------------
// run_batch is the procedure all of them share; an entry function states its own checks, describes its arrays in a Batch, supplies the
// launches of one chunk and turns the Totals into rt_stats.

DevMem& stage_of(DeviceState& d, Stage s) {
    switch (s) {
    case ST_COUNTS: return d.rq.counts;
    case ST_AO: return d.rq.ao;
    case ST_PATHS: return d.rq.paths;
    default: return d.rq.out;
    }
}

// BatchIn, BatchOut and Stage: rt_internal.h
struct Batch {
    const char* fn;
    size_t n;
    BatchIn in; // a host batch's chunk of it is staged in rq.in
    BatchOut out[2];
    size_t host_chunk, device_chunk; // records per chunk
    uint32_t counter_slots;          // the first slots of the device's counters are zeroed before the launches and added up after them (0: none)
    bool device_one_pair = false;    // a device batch has no copies between its launches: one event pair around all its chunks
    Stage scratch = ST_PATHS;        // scratch_size bytes per record of a chunk, reserved for host and device batches alike
    size_t scratch_size = 0;
};
struct Chunk { // what a launch works on: device pointers, the chunk's first index in the caller's arrays and its records
    const void* in;
    void* out[2]; // null where Batch::out[k].p is
    size_t off;
    uint32_t m;
    bool staged; // a host batch: in and out are the staging buffers
};
struct Totals {
    double kernel_ms = 0.0; // the maximum over the devices of each device's summed event pairs
    unsigned long long cn[RT_CNT_DIAG] = {0}; // the counter slots summed over the devices
};
static_assert(RT_CNT_TRI_TESTS + 1 <= RT_CNT_DIAG, "Totals::cn holds either set of slots");

std::string array_names(const Batch& b) { // "rays, hits and counts"
    std::string s = b.in.name;
    const bool two = b.out[0].p && b.out[1].p;
    for (int k = 0; k < 2; k++)
        if (b.out[k].p) s += std::string(two && k == 0 ? ", " : " and ") + b.out[k].name;
    return s;
}

// After the caller's own checks: sync_pending, where the arrays live, then per device a contiguous range (query_plan.h; a device batch
// runs where it lives) in chunks - H2D, event, launch(d, scene, chunk), event, D2H - with every device enqueued before any is waited
// for.  Nothing on a device is touched before the checks pass; after the first enqueue every failure drains all streams before it
// returns.
template <class Launch>
int run_batch(rt_ctx* ctx, const Batch& b, Totals& tot, Launch&& launch) {
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pin, pout[2];
    if (int rc = classify_ptr(ctx, b.fn, b.in.name, b.in.p, pin)) return rc;
    for (int k = 0; k < 2; k++)
        if (b.out[k].p)
            if (int rc = classify_ptr(ctx, b.fn, b.out[k].name, b.out[k].p, pout[k], b.out[k].align)) return rc;
    for (int k = 0; k < 2; k++)
        if (b.out[k].p && (pout[k].device != pin.device || pout[k].dev != pin.dev))
            return ctx->fail(RT_ERR_BAD_ARG, "%s: %s must all be host memory or all device memory of the same device", b.fn, array_names(b).c_str());
    const bool device = pin.device, one_pair = device && b.device_one_pair;
    const size_t chunk = device ? b.device_chunk : b.host_chunk;
    const size_t nd = ctx->devs.size();
    std::vector<PlanRange> range(nd, PlanRange{0, 0});
    if (device) range[pin.dev] = {0, b.n};
    else
        for (size_t j = 0; j < nd; j++) range[j] = device_range(b.n, nd, j);
    auto enqueue = [&](size_t j) -> int {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        const DevScene sc = scene_for(ctx, d);
        const size_t chunks = chunk_count(range[j].count, chunk), most = std::min(range[j].count, chunk);
        if (int rc = ensure_query_events(ctx, d, 2 * event_pairs(range[j].count, chunk, one_pair))) return rc;
        if (b.scratch_size) HIPCHK(ctx, stage_of(d, b.scratch).reserve(most * b.scratch_size));
        if (!device) {
            HIPCHK(ctx, d.rq.in.reserve(most * b.in.size));
            for (const BatchOut& o : b.out)
                if (o.p) HIPCHK(ctx, stage_of(d, o.stage).reserve(most * o.size));
        }
        if (b.counter_slots) HIPCHK(ctx, hipMemsetAsync(d.counters.get(), 0, b.counter_slots * sizeof(unsigned long long), d.stream));
        for (size_t c = 0; c < chunks; c++) {
            const PlanChunk pc = chunk_of(range[j], chunk, c);
            Chunk ck{static_cast<const char*>(b.in.p) + pc.off * b.in.size, {nullptr, nullptr}, pc.off, (uint32_t)pc.m, !device};
            void* host[2] = {nullptr, nullptr};
            for (int k = 0; k < 2; k++)
                if (b.out[k].p) ck.out[k] = host[k] = static_cast<char*>(b.out[k].p) + pc.off * b.out[k].size;
            if (!device) {
                HIPCHK(ctx, hipMemcpyAsync(d.rq.in.get(), ck.in, pc.m * b.in.size, hipMemcpyHostToDevice, d.stream));
                ck.in = d.rq.in.get();
                for (int k = 0; k < 2; k++)
                    if (b.out[k].p) ck.out[k] = stage_of(d, b.out[k].stage).get();
            }
            const size_t pair = one_pair ? 0 : c; // the copies stay outside the pair
            if (!one_pair || c == 0) HIPCHK(ctx, hipEventRecord(d.rq_events[2 * pair], d.stream));
            HIPCHK(ctx, launch(d, sc, ck));
            if (!one_pair || c + 1 == chunks) HIPCHK(ctx, hipEventRecord(d.rq_events[2 * pair + 1], d.stream));
            for (int k = 0; k < 2; k++)
                if (!device && b.out[k].p) HIPCHK(ctx, hipMemcpyAsync(host[k], ck.out[k], pc.m * b.out[k].size, hipMemcpyDeviceToHost, d.stream));
        }
        return RT_OK;
    };
    auto collect = [&]() -> int {
        for (size_t j = 0; j < nd; j++) {
            if (range[j].count == 0) continue;
            DeviceState& d = ctx->devs[j];
            hipError_t e = hipSetDevice(d.device);
            if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
            if (e != hipSuccess) return ctx->fail(RT_ERR_HIP, "%s: device %d: %s", b.fn, d.device, hipGetErrorString(e));
            double ms = 0.0;
            for (size_t c = 0; c < event_pairs(range[j].count, chunk, one_pair); c++) {
                float cm = 0.0f;
                HIPCHK(ctx, hipEventElapsedTime(&cm, d.rq_events[2 * c], d.rq_events[2 * c + 1]));
                ms += cm;
            }
            tot.kernel_ms = std::max(tot.kernel_ms, ms);
            if (b.counter_slots) {
                unsigned long long cn[RT_CNT_DIAG];
                HIPCHK(ctx, hipMemcpy(cn, d.counters.get(), b.counter_slots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
                for (uint32_t s = 0; s < b.counter_slots; s++) tot.cn[s] += cn[s];
            }
        }
        return RT_OK;
    };
    int rc = RT_OK;
    for (size_t j = 0; j < nd && rc == RT_OK; j++)
        if (range[j].count > 0) rc = enqueue(j);
    if (rc == RT_OK) rc = collect();
    if (rc != RT_OK) drain_streams(ctx);
    return rc;
}

// A successful batch call's rt_stats, wall_ms from the call's entry at w0.  node_visits and tri_tests are counted only with RT_QUERY_COUNTERS.
void batch_stats(rt_ctx* ctx, double w0, const Totals& t, bool counters, uint64_t rays, uint64_t primary = 0, uint64_t continuation = 0, uint64_t shadow = 0) {
    rt_stats& st = ctx->stats;
    st.rays = rays;
    st.primary_rays = primary;
    st.continuation_rays = continuation;
    st.shadow_rays = shadow;
    st.pixels = 0;
    st.node_visits = counters ? t.cn[RT_CNT_NODE_VISITS] : 0;
    st.tri_tests = counters ? t.cn[RT_CNT_TRI_TESTS] : 0;
    st.kernel_ms = t.kernel_ms;
    st.wall_ms = now_ms() - w0;
}

hipError_t launch_closest_hit(const DevScene& sc, const void* rays, void* out, uint32_t n, unsigned long long* cnt, hipStream_t s) {
    return rt::launch_ray_query(sc, rays, out, n, false, cnt, s);
}
hipError_t launch_any_hit(const DevScene& sc, const void* rays, void* out, uint32_t n, unsigned long long* cnt, hipStream_t s) {
    return rt::launch_ray_query(sc, rays, out, n, true, cnt, s);
}

// rt_radiance (rays), rt_radiance_sh (probes) and rt_irradiance (surface points): samples paths per record and a scratch of one record
// per path.  `own_directions`: the call draws a direction per path itself - the two draws RT_PATH_CAMERA_DRAWS names, so the flag is
// refused - and its reduction always runs, so the scratch is there with one sample too (rt_radiance_sh, rt_irradiance).  Host and
// device batches alike go in chunks of max(1, RT_QUERY_CHUNK / samples) records, so a launch covers at most RT_QUERY_CHUNK paths and
// the scratch never grows past that; the chunk's first index goes to the kernel, so a record's seed is that of its place in the
// caller's array.  The segments are counted on the device (rt_stats.rays), so every call zeroes and reads the device's counters.
using PathLaunch = hipError_t (*)(const DevScene&, const rt::PathArgs&, const void*, uint64_t, uint32_t, void*, void*, bool, unsigned long long*, hipStream_t);
int path_query(rt_ctx* ctx, const char* fn, BatchIn in, size_t n, const rt_path_params* p, void* out, size_t out_size, bool own_directions, PathLaunch launch) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!in.p || !p || !out) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !in.p ? in.name : !p ? "params" : "out", n);
    if (p->samples < 1 || p->samples > RT_PATH_MAX_SAMPLES) return ctx->fail(RT_ERR_BAD_ARG, "%s: samples %u (1 .. %u)", fn, p->samples, RT_PATH_MAX_SAMPLES);
    if (p->max_bounces > RT_MAX_BOUNCES) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_bounces %u (0 .. %u)", fn, p->max_bounces, RT_MAX_BOUNCES);
    if ((uint64_t)p->first_sample + p->samples > (1ull << 32))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: first_sample %u + samples %u passes 2^32", fn, p->first_sample, p->samples);
    if (own_directions && (p->flags & RT_PATH_CAMERA_DRAWS))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: flags: RT_PATH_CAMERA_DRAWS (the call spends those two draws itself)", fn);
    const uint32_t known = RT_QUERY_COUNTERS | RT_PATH_NO_SHADOWS | RT_PATH_CAMERA_DRAWS;
    if (p->flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, p->flags & ~known);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    const rt::PathArgs args{p->samples, p->max_bounces, p->seed, p->first_sample, (p->flags & RT_PATH_NO_SHADOWS) ? 0u : 1u,
                            (own_directions || (p->flags & RT_PATH_CAMERA_DRAWS)) ? 1u : 0u};
    const bool counters = (p->flags & RT_QUERY_COUNTERS) != 0;
    const size_t chunk = std::max<size_t>(1, RT_QUERY_CHUNK / p->samples);
    Batch b{fn, n, in, {{"out", out, out_size}, {}}, chunk, chunk, RT_CNT_DIAG};
    b.device_one_pair = true;
    if (own_directions || args.samples > 1) b.scratch_size = args.samples * sizeof(uint4); // with one sample the record is the ray's result
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            return launch(sc, args, ck.in, ck.off, ck.m, d.rq.paths.get(), ck.out[0], counters, d.counters.get(), d.stream);
        }))
        return rc;
    const uint64_t camera = t.cn[RT_CNT_CAMERA], continuation = t.cn[RT_CNT_CONTINUATION], shadow = t.cn[RT_CNT_SHADOW];
    batch_stats(ctx, w0, t, counters, camera + continuation + shadow, camera, continuation, shadow);
    return RT_OK;
}

// rt_camera_rays and rt_sample_rays: n rays that launch(where, first index, rays, stream) writes, in chunks of RT_QUERY_CHUNK: into
// `out` on the device it lives on, or through the first device's rq.in to the host.
template <class Launch>
int generate_rays(rt_ctx* ctx, const char* fn, rt_ray* out, size_t n, Launch&& launch) {
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr po;
    if (int rc = classify_ptr(ctx, fn, "out", out, po)) return rc;
    DeviceState& d = ctx->devs[po.dev];
    HIPCHK(ctx, hipSetDevice(d.device));
    if (!po.device)
        HIPCHK(ctx, d.rq.in.reserve(std::min<size_t>(n, RT_QUERY_CHUNK) * sizeof(rt_ray)));
    for (size_t off = 0; off < n; off += RT_QUERY_CHUNK) {
        const size_t m = std::min<size_t>(RT_QUERY_CHUNK, n - off);
        hipError_t e = launch(po.device ? (void*)(out + off) : d.rq.in.get(), off, (uint32_t)m, d.stream);
        if (e == hipSuccess && !po.device) e = hipMemcpyAsync(out + off, d.rq.in.get(), m * sizeof(rt_ray), hipMemcpyDeviceToHost, d.stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(d.stream);
            return ctx->fail(RT_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
}

constexpr size_t RT_AO_DEVICE_CHUNK = (size_t)1 << 24; // points of a device batch per chunk: bounds the counts beside them (64 MiB)
static_assert(RT_DIRECT_MAX_LIGHTS == RT_WF_MAX_LIGHTS, "the grid table and lit_mask hold one entry / bit per light, as the pipeline's visibility word");

// The jitter rule of the frames: a closed frame jitters when it has several samples (frame_of_params), an accumulation always.
void sample_jitter(DevFrame& fr, uint32_t flags) {
    if (flags & RT_FLAG_ACCUMULATE) fr.jitter = 1u;
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
            HIPCHK(ctx, d.dn.aov.reserve(bytes));
        if (int rc = enqueue_aovs(ctx, d, share[j], in_place ? (void*)out : d.dn.aov.get(), bytes)) {
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
        HIPCHK(ctx, hipMemcpy(out, ctx->devs[0].dn.aov.get(), bytes, hipMemcpyDeviceToHost));
    } else if (!in_place) { // several devices: each holds its own tiles; zeros elsewhere, as rt_read_rgb32f gives them
        std::vector<uint8_t> whole(bytes, 0), tmp(bytes);
        for (size_t j = 0; j < nd; j++) {
            const DeviceState& d = ctx->devs[j];
            const DevFrame& f = share[j];
            if (f.n_owned_tiles == 0) continue;
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, hipMemcpy(tmp.data(), d.dn.aov.get(), bytes, hipMemcpyDeviceToHost));
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
        HIPCHK(ctx, d.dn.plane[k].reserve((size_t)n * 16));
    if (!device) {
        HIPCHK(ctx, d.dn.rgb.reserve((size_t)n * 12));
        HIPCHK(ctx, d.dn.aov.reserve((size_t)n * sizeof(rt_aov)));
    }
    if (int rc = ensure_query_events(ctx, d, 2)) return rc;
    const float* c_rgb = device ? rgb : (const float*)d.dn.rgb.get();
    const void* c_aov = device ? (const void*)aov : d.dn.aov.get();
    float* c_out = device ? out : (float*)d.dn.rgb.get(); // the pack has read the staged rgb before the last iteration writes over it
    float4* plane[2] = {d.dn.plane[0].get(), d.dn.plane[1].get()};
    const bool demod = (dp->flags & RT_DENOISE_DEMODULATE) != 0;
    auto enqueue = [&]() -> hipError_t {
        hipError_t e = hipSuccess;
        if (!device) {
            if ((e = hipMemcpyAsync(d.dn.rgb.get(), rgb, (size_t)n * 12, hipMemcpyHostToDevice, d.stream)) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(d.dn.aov.get(), aov, (size_t)n * sizeof(rt_aov), hipMemcpyHostToDevice, d.stream)) != hipSuccess) return e;
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
        if (!device) e = hipMemcpyAsync(out, d.dn.rgb.get(), (size_t)n * 12, hipMemcpyDeviceToHost, d.stream);
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

// rt_inside and rt_signed_distance: one answer per point (a byte, or an rt_nearest) and a second output, the votes.  A chunk is
// RT_QUERY_CHUNK / rays points, so a launch traces at most RT_QUERY_CHUNK parity rays.  The rays traced are counted on the device
// (rt_stats.rays), so every call zeroes and reads the device's counters.
int inside_query(rt_ctx* ctx, const char* fn, const rt_point_query* points, size_t n, const rt_inside_params* p, BatchOut out, uint8_t* votes, bool distance) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!points || !p || !out.p) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !points ? "points" : !p ? "params" : out.name, n);
    if (!rt::inside_rays_valid(p->rays)) return ctx->fail(RT_ERR_BAD_ARG, "%s: rays %u (1, 3, 5 or %u)", fn, p->rays, RT_INSIDE_MAX_RAYS);
    if (p->flags & ~RT_QUERY_COUNTERS) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, p->flags & ~RT_QUERY_COUNTERS);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    const bool counters = (p->flags & RT_QUERY_COUNTERS) != 0;
    const uint32_t rays = p->rays;
    const size_t chunk = RT_QUERY_CHUNK / rays;
    const Batch b{fn, n, {"points", points, sizeof(rt_point_query)}, {out, {"votes", votes, 1, 1, ST_COUNTS}}, chunk, chunk, RT_CNT_TRI_TESTS + 1u};
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            return rt::launch_inside(sc, ck.in, ck.out[0], static_cast<uint8_t*>(ck.out[1]), ck.m, rays, distance, counters, d.counters.get(), d.stream);
        }))
        return rc;
    batch_stats(ctx, w0, t, counters, t.cn[RT_CNT_SEGMENTS]);
    return RT_OK;
}

static_assert(RT_OVERLAP_MAX == rt::OV_PRIMS_MAX, "the kernel's list holds RT_OVERLAP_MAX entries");

} // namespace

// rt_intersect, rt_occluded, rt_surface, rt_closest_point, rt_sweep_sphere, rt_sweep_box, rt_sweep_obb, rt_sweep_capsule, and
// rt_sweep_triangle (rt_mesh_query.cpp): one record in, one record out, one lane of `launch` per record.
int record_query(rt_ctx* ctx, const char* fn, BatchIn in, size_t n, BatchOut out, uint32_t flags, RecordLaunch launch) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!in.p || !out.p) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !in.p ? in.name : out.name, n);
    if (flags & ~RT_QUERY_COUNTERS) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~RT_QUERY_COUNTERS);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0;
    const Batch b{fn, n, in, {out, {}}, RT_QUERY_CHUNK, RT_QUERY_CHUNK, counters ? RT_CNT_TRI_TESTS + 1u : 0u};
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            return launch(sc, ck.in, ck.out[0], ck.m, counters ? d.counters.get() : nullptr, d.stream);
        }))
        return rc;
    batch_stats(ctx, w0, t, counters, n);
    return RT_OK;
}

// max_prims ids per record and a second output, the counts: rt_closest_point_all's shape with 4-byte records.  A chunk is RT_QUERY_CHUNK /
// max(max_prims, 1) records.  rt_overlap_box, rt_overlap_obb and rt_overlap_triangle (rt_mesh_query.cpp): the same argument checks and batch, with the input's name,
// the record's size and the launcher of each.
int overlap_query(rt_ctx* ctx, const char* fn, const char* in_name, const void* in, size_t in_size, size_t n, uint32_t max_prims, uint32_t* prims,
                  uint32_t* counts, uint32_t flags, OverlapLaunch launch) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!in || (!prims && max_prims > 0)) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !in ? in_name : "prims", n);
    if (max_prims > RT_OVERLAP_MAX) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_prims %u (0 .. %u)", fn, max_prims, RT_OVERLAP_MAX);
    const uint32_t known = RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL | RT_OVERLAP_ANY;
    if (flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~known);
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0, all = (flags & RT_QUERY_COUNT_ALL) != 0, any = (flags & RT_OVERLAP_ANY) != 0;
    if (any && (all || max_prims > 0)) return ctx->fail(RT_ERR_BAD_ARG, "%s: RT_OVERLAP_ANY needs max_prims 0 and excludes RT_QUERY_COUNT_ALL", fn);
    if (max_prims == 0 && ((!all && !any) || !counts))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: max_prims 0 needs RT_QUERY_COUNT_ALL or RT_OVERLAP_ANY, and counts", fn);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (max_prims == 0) prims = nullptr; // ignored: a pure count
    const int mode = any ? rt::OV_ANY : all ? rt::OV_COUNT_ALL : rt::OV_LIST;
    const size_t chunk = RT_QUERY_CHUNK / std::max(max_prims, 1u);
    const Batch b{fn, n, {in_name, in, in_size},
                  {{"prims", prims, max_prims * sizeof(uint32_t), 4}, {"counts", counts, sizeof(uint32_t), 4, ST_COUNTS}},
                  chunk, chunk, counters ? RT_CNT_TRI_TESTS + 1u : 0u};
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            return launch(sc, ck.in, static_cast<uint32_t*>(ck.out[0]), static_cast<uint32_t*>(ck.out[1]), ck.m, max_prims, mode,
                          counters ? d.counters.get() : nullptr, d.stream);
        }))
        return rc;
    batch_stats(ctx, w0, t, counters, n);
    return RT_OK;
}

// max_contacts 32-byte records per query and a second output, the counts: rt_closest_point_all's shape with rt_overlap_box's modes.  A
// chunk is RT_QUERY_CHUNK / max(max_contacts, 1) queries.  rt_contact_capsule and rt_contact_triangle (rt_mesh_query.cpp): the same
// argument checks and batch, with the input's name, the record's size and the launcher of each.
static_assert(RT_CONTACT_MAX == rt::CC_CONTACT_MAX && RT_CONTACT_MAX == rt::CT_CONTACT_MAX, "the kernels' lists hold RT_CONTACT_MAX entries");
static_assert(sizeof(rt_contact) == 32 && sizeof(rt_triangle_contact) == 32, "contact_query writes 32-byte records");
int contact_query(rt_ctx* ctx, const char* fn, const char* in_name, const void* in, size_t in_size, size_t n, uint32_t max_contacts, void* out,
                  uint32_t* counts, uint32_t flags, ContactLaunch launch) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!in || (!out && max_contacts > 0)) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !in ? in_name : "out", n);
    if (max_contacts > RT_CONTACT_MAX) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_contacts %u (0 .. %u)", fn, max_contacts, RT_CONTACT_MAX);
    const uint32_t known = RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL | RT_CONTACT_ANY;
    if (flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~known);
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0, all = (flags & RT_QUERY_COUNT_ALL) != 0, any = (flags & RT_CONTACT_ANY) != 0;
    if (any && (all || max_contacts > 0)) return ctx->fail(RT_ERR_BAD_ARG, "%s: RT_CONTACT_ANY needs max_contacts 0 and excludes RT_QUERY_COUNT_ALL", fn);
    if (max_contacts == 0 && ((!all && !any) || !counts))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: max_contacts 0 needs RT_QUERY_COUNT_ALL or RT_CONTACT_ANY, and counts", fn);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (max_contacts == 0) out = nullptr; // ignored: a pure count
    const int mode = any ? rt::CC_ANY : all ? rt::CC_COUNT_ALL : rt::CC_LIST;
    const size_t chunk = RT_QUERY_CHUNK / std::max(max_contacts, 1u);
    const Batch b{fn, n, {in_name, in, in_size},
                  {{"out", out, max_contacts * sizeof(rt_contact)}, {"counts", counts, sizeof(uint32_t), 4, ST_COUNTS}},
                  chunk, chunk, counters ? RT_CNT_TRI_TESTS + 1u : 0u};
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            return launch(sc, ck.in, ck.out[0], static_cast<uint32_t*>(ck.out[1]), ck.m, max_contacts, mode, counters ? d.counters.get() : nullptr, d.stream);
        }))
        return rc;
    batch_stats(ctx, w0, t, counters, n);
    return RT_OK;
}

// rt_overlap_mesh and rt_sweep_mesh (rt_posed_query.cpp): a mesh of m triangles given once and one record per pose in, one or two
// records per pose out.  The mesh lives where the poses and the outputs live: device memory of the poses' device is handed to the
// launcher as it is; a host mesh is copied into rq.mesh of every device that takes a share of the poses, once per call and ahead of
// the launches on that device's stream.  A chunk is max(1, RT_QUERY_CHUNK / m) poses, so a launch poses at most RT_QUERY_CHUNK
// triangles (or one pose's).  The entry states the checks that are its own (flags, `first` with RT_OVERLAP_ANY) before it calls.
static_assert(sizeof(rt_query_triangle) == 48 && sizeof(rt_pose) == 32 && sizeof(rt_pose_sweep) == 48 && sizeof(rt_mesh_sweep_hit) == 32,
              "the records posed_mesh.hip reads and writes");
int pose_query(rt_ctx* ctx, const char* fn, const void* mesh, size_t m, BatchIn in, size_t n, BatchOut out0, BatchOut out1, uint32_t flags, uint32_t mode,
               PoseLaunch launch) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!mesh || !in.p || !out0.p) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !mesh ? "mesh" : !in.p ? in.name : out0.name, n);
    if (m < 1 || m > RT_POSED_MESH_MAX) return ctx->fail(RT_ERR_BAD_ARG, "%s: m %zu (1 .. %u)", fn, m, RT_POSED_MESH_MAX);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0;
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pm, pin;
    if (int rc = classify_ptr(ctx, fn, "mesh", mesh, pm)) return rc;
    if (int rc = classify_ptr(ctx, fn, in.name, in.p, pin)) return rc;
    if (pm.device != pin.device || pm.dev != pin.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: mesh and %s must both be host memory or both device memory of the same device", fn, in.name);
    for (const BatchOut* o : {&out0, &out1}) { // run_batch asks again; asked here so that nothing is copied for a call it refuses
        QueryPtr po;
        if (!o->p) continue;
        if (int rc = classify_ptr(ctx, fn, o->name, o->p, po, o->align)) return rc;
        if (po.device != pin.device || po.dev != pin.dev)
            return ctx->fail(RT_ERR_BAD_ARG, "%s: mesh, %s and the outputs must all be host memory or all device memory of the same device", fn, in.name);
    }
    const size_t nd = ctx->devs.size(), mesh_bytes = m * sizeof(rt_query_triangle);
    if (!pm.device)
        for (size_t j = 0; j < nd; j++) {
            if (device_range(n, nd, j).count == 0) continue;
            DeviceState& d = ctx->devs[j];
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, d.rq.mesh.reserve(mesh_bytes));
            HIPCHK(ctx, hipMemcpyAsync(d.rq.mesh.get(), mesh, mesh_bytes, hipMemcpyHostToDevice, d.stream));
        }
    const size_t chunk = std::max<size_t>(1, RT_QUERY_CHUNK / m);
    const Batch b{fn, n, in, {out0, out1}, chunk, chunk, counters ? RT_CNT_TRI_TESTS + 1u : 0u};
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            return launch(sc, pm.device ? mesh : d.rq.mesh.get(), (uint32_t)m, ck.in, ck.out[0], ck.out[1], ck.m, mode, counters ? d.counters.get() : nullptr, d.stream);
        }))
        return rc;
    batch_stats(ctx, w0, t, counters, n);
    return RT_OK;
}

} // namespace rti

using namespace rti;

extern "C" {

int rt_intersect(rt_ctx* ctx, const rt_ray* rays, size_t n, rt_hit* hits, uint32_t flags) {
    return record_query(ctx, "rt_intersect", {"rays", rays, sizeof(rt_ray)}, n, {"hits", hits, sizeof(rt_hit)}, flags, launch_closest_hit);
}

int rt_occluded(rt_ctx* ctx, const rt_ray* rays, size_t n, uint8_t* occluded, uint32_t flags) {
    return record_query(ctx, "rt_occluded", {"rays", rays, sizeof(rt_ray)}, n, {"occluded", occluded, 1}, flags, launch_any_hit);
}

int rt_surface(rt_ctx* ctx, const rt_ray* rays, size_t n, rt_surface_point* out, uint32_t flags) {
    return record_query(ctx, "rt_surface", {"rays", rays, sizeof(rt_ray)}, n, {"out", out, sizeof(rt_surface_point)}, flags, rt::launch_surface_query);
}

int rt_closest_point(rt_ctx* ctx, const rt_point_query* points, size_t n, rt_nearest* out, uint32_t flags) {
    return record_query(ctx, "rt_closest_point", {"points", points, sizeof(rt_point_query)}, n, {"out", out, sizeof(rt_nearest)}, flags, rt::launch_closest_point);
}

int rt_sweep_sphere(rt_ctx* ctx, const rt_sweep* sweeps, size_t n, rt_sweep_hit* out, uint32_t flags) {
    return record_query(ctx, "rt_sweep_sphere", {"sweeps", sweeps, sizeof(rt_sweep)}, n, {"out", out, sizeof(rt_sweep_hit)}, flags, rt::launch_sweep_sphere);
}

int rt_sweep_box(rt_ctx* ctx, const rt_box_sweep* sweeps, size_t n, rt_box_sweep_hit* out, uint32_t flags) {
    return record_query(ctx, "rt_sweep_box", {"sweeps", sweeps, sizeof(rt_box_sweep)}, n, {"out", out, sizeof(rt_box_sweep_hit)}, flags, rt::launch_sweep_box);
}

int rt_sweep_obb(rt_ctx* ctx, const rt_obb_sweep* sweeps, size_t n, rt_box_sweep_hit* out, uint32_t flags) {
    return record_query(ctx, "rt_sweep_obb", {"sweeps", sweeps, sizeof(rt_obb_sweep)}, n, {"out", out, sizeof(rt_box_sweep_hit)}, flags, rt::launch_sweep_obb);
}

int rt_sweep_capsule(rt_ctx* ctx, const rt_capsule_sweep* sweeps, size_t n, rt_capsule_sweep_hit* out, uint32_t flags) {
    return record_query(ctx, "rt_sweep_capsule", {"sweeps", sweeps, sizeof(rt_capsule_sweep)}, n, {"out", out, sizeof(rt_capsule_sweep_hit)}, flags, rt::launch_sweep_capsule);
}

// max_hits records per ray and a second output, the counts.  A chunk is RT_QUERY_CHUNK / max(max_hits, 1) rays: its hit records never
// need more staging than an rt_intersect chunk's.
int rt_intersect_all(rt_ctx* ctx, const rt_ray* rays, size_t n, uint32_t max_hits, rt_hit* hits, uint32_t* counts, uint32_t flags) {
    const char* fn = "rt_intersect_all";
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!rays || (!hits && max_hits > 0)) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !rays ? "rays" : "hits", n);
    if (max_hits > RT_MULTI_HIT_MAX) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_hits %u (0 .. %u)", fn, max_hits, RT_MULTI_HIT_MAX);
    if (max_hits == 0 && (!(flags & RT_QUERY_COUNT_ALL) || !counts))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: max_hits 0 needs RT_QUERY_COUNT_ALL and counts", fn);
    const uint32_t known = RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL;
    if (flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~known);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (max_hits == 0) hits = nullptr; // ignored: a pure count
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0, all = (flags & RT_QUERY_COUNT_ALL) != 0;
    const size_t chunk = RT_QUERY_CHUNK / std::max(max_hits, 1u);
    const Batch b{fn, n, {"rays", rays, sizeof(rt_ray)}, {{"hits", hits, max_hits * sizeof(rt_hit)}, {"counts", counts, sizeof(uint32_t), 4, ST_COUNTS}},
                  chunk, chunk, counters ? RT_CNT_TRI_TESTS + 1u : 0u};
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            return rt::launch_ray_query_all(sc, ck.in, ck.out[0], static_cast<uint32_t*>(ck.out[1]), ck.m, max_hits, all, counters ? d.counters.get() : nullptr, d.stream);
        }))
        return rc;
    batch_stats(ctx, w0, t, counters, n);
    return RT_OK;
}

// max_nearest records per point and a second output, the counts: rt_intersect_all's shape.  A chunk is RT_QUERY_CHUNK /
// max(max_nearest, 1) points: its records never need more staging than an rt_closest_point chunk's.
static_assert(RT_NEAREST_MAX == rt::CP_NEAREST_MAX, "the kernel's list holds RT_NEAREST_MAX entries");
int rt_closest_point_all(rt_ctx* ctx, const rt_point_query* points, size_t n, uint32_t max_nearest, rt_nearest* out, uint32_t* counts, uint32_t flags) {
    const char* fn = "rt_closest_point_all";
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!points || (!out && max_nearest > 0)) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !points ? "points" : "out", n);
    if (max_nearest > RT_NEAREST_MAX) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_nearest %u (0 .. %u)", fn, max_nearest, RT_NEAREST_MAX);
    if (max_nearest == 0 && (!(flags & RT_QUERY_COUNT_ALL) || !counts))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: max_nearest 0 needs RT_QUERY_COUNT_ALL and counts", fn);
    const uint32_t known = RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL;
    if (flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~known);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (max_nearest == 0) out = nullptr; // ignored: a pure count
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0, all = (flags & RT_QUERY_COUNT_ALL) != 0;
    const size_t chunk = RT_QUERY_CHUNK / std::max(max_nearest, 1u);
    const Batch b{fn, n, {"points", points, sizeof(rt_point_query)},
                  {{"out", out, max_nearest * sizeof(rt_nearest)}, {"counts", counts, sizeof(uint32_t), 4, ST_COUNTS}},
                  chunk, chunk, counters ? RT_CNT_TRI_TESTS + 1u : 0u};
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            return rt::launch_closest_point_all(sc, ck.in, ck.out[0], static_cast<uint32_t*>(ck.out[1]), ck.m, max_nearest, all, counters ? d.counters.get() : nullptr, d.stream);
        }))
        return rc;
    batch_stats(ctx, w0, t, counters, n);
    return RT_OK;
}

int rt_overlap_box(rt_ctx* ctx, const rt_box* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts, uint32_t flags) {
    return overlap_query(ctx, "rt_overlap_box", "boxes", boxes, sizeof(rt_box), n, max_prims, prims, counts, flags, rt::launch_overlap_box);
}
int rt_overlap_obb(rt_ctx* ctx, const rt_obb* boxes, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts, uint32_t flags) {
    return overlap_query(ctx, "rt_overlap_obb", "boxes", boxes, sizeof(rt_obb), n, max_prims, prims, counts, flags, rt::launch_overlap_obb);
}

int rt_contact_capsule(rt_ctx* ctx, const rt_capsule* capsules, size_t n, uint32_t max_contacts, rt_contact* out, uint32_t* counts, uint32_t flags) {
    return contact_query(ctx, "rt_contact_capsule", "capsules", capsules, sizeof(rt_capsule), n, max_contacts, out, counts, flags, rt::launch_contact_capsule);
}

int rt_inside(rt_ctx* ctx, const rt_point_query* points, size_t n, const rt_inside_params* params, uint8_t* inside, uint8_t* votes) {
    return inside_query(ctx, "rt_inside", points, n, params, {"inside", inside, 1, 1}, votes, false);
}

int rt_signed_distance(rt_ctx* ctx, const rt_point_query* points, size_t n, const rt_inside_params* params, rt_nearest* out, uint8_t* votes) {
    return inside_query(ctx, "rt_signed_distance", points, n, params, {"out", out, sizeof(rt_nearest)}, votes, true);
}

// samples lanes per point and two optional outputs.  Every chunk (a host batch: max(1, RT_QUERY_CHUNK / samples) points; a device
// batch: RT_AO_DEVICE_CHUNK) zeroes the device's per-point counts in rq.ao, lets the kernel add to them and finishes them into
// visibility and counts; the chunk's first index goes to the kernel, so a point's seed is that of its place in the caller's array.
int rt_ambient_occlusion(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_ao_params* p, float* visibility, uint32_t* unoccluded) {
    const char* fn = "rt_ambient_occlusion";
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!points || !p) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !points ? "points" : "params", n);
    if (!visibility && !unoccluded) return ctx->fail(RT_ERR_BAD_ARG, "%s: visibility and unoccluded are both NULL with n = %zu", fn, n);
    if (p->samples < 1 || p->samples > RT_AO_MAX_SAMPLES) return ctx->fail(RT_ERR_BAD_ARG, "%s: samples %u (1 .. %u)", fn, p->samples, RT_AO_MAX_SAMPLES);
    if (!(p->max_distance > 0.0f)) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_distance %g (> 0, +inf allowed)", fn, (double)p->max_distance);
    if (!std::isfinite(p->bias) || p->bias < 0.0f) return ctx->fail(RT_ERR_BAD_ARG, "%s: bias %g (finite and >= 0)", fn, (double)p->bias);
    if (p->flags & ~RT_QUERY_COUNTERS) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, p->flags & ~RT_QUERY_COUNTERS);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    const rt::AoParams ap{p->samples, p->seed, p->max_distance, p->bias};
    const bool counters = (p->flags & RT_QUERY_COUNTERS) != 0;
    // a host batch's counts go to the host from rq.ao, where the kernel left them
    Batch b{fn, n, {"points", points, sizeof(rt_surface_point)},
            {{"visibility", visibility, sizeof(float), 4}, {"unoccluded", unoccluded, sizeof(uint32_t), 4, ST_AO}},
            std::max<size_t>(1, RT_QUERY_CHUNK / p->samples), RT_AO_DEVICE_CHUNK, counters ? RT_CNT_TRI_TESTS + 1u : 0u};
    b.scratch = ST_AO, b.scratch_size = sizeof(uint32_t);
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            float* vis = static_cast<float*>(ck.out[0]);
            uint32_t* cnt_out = ck.staged ? nullptr : static_cast<uint32_t*>(ck.out[1]);
            hipError_t e = hipMemsetAsync(d.rq.ao.get(), 0, ck.m * sizeof(uint32_t), d.stream);
            if (e == hipSuccess) e = rt::launch_ao(sc, ck.in, ck.off, ck.m, ap, d.rq.ao.get(), counters ? d.counters.get() : nullptr, d.stream);
            if (e == hipSuccess && (vis || cnt_out)) e = rt::launch_ao_finish(d.rq.ao.get(), ck.m, ap.samples, vis, cnt_out, d.stream);
            return e;
        }))
        return rc;
    batch_stats(ctx, w0, t, counters, (uint64_t)n * p->samples);
    return RT_OK;
}

// One 16-byte record out per point.  The segments are counted on the device (rt_stats.rays), so every call zeroes and reads the
// device's counters.  A device hands over the light grids it already holds - from rt_prepare or an extended-mode frame - when the
// call's bias is the one they were derived for; this call never builds any (ensure_grids).
int rt_direct_light(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_direct_light_params* p, rt_lighting* out) {
    const char* fn = "rt_direct_light";
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!points || !p || !out) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !points ? "points" : !p ? "params" : "out", n);
    const uint32_t known = RT_QUERY_COUNTERS | RT_DIRECT_AMBIENT | RT_DIRECT_NO_SHADOWS | RT_DIRECT_NO_SHADOW_GRID;
    if (p->flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, p->flags & ~known);
    if (!std::isfinite(p->bias) || p->bias < 0.0f) return ctx->fail(RT_ERR_BAD_ARG, "%s: bias %g (finite and >= 0)", fn, (double)p->bias);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (ctx->scene_counts.n_lights > RT_DIRECT_MAX_LIGHTS)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: the scene has %u lights (at most %u: one bit of lit_mask each)", fn, ctx->scene_counts.n_lights, RT_DIRECT_MAX_LIGHTS);
    rt::DirectLightArgs args{};
    args.bias = p->bias;
    args.ambient = (p->flags & RT_DIRECT_AMBIENT) ? 1u : 0u;
    args.shadows = (p->flags & RT_DIRECT_NO_SHADOWS) ? 0u : 1u;
    // the lists are supersets of what the triangle test accepts for segments that start EXT_EPS off their point: any other bias walks the tree
    const float grid_bias = RT_SG_EXT_EPS;
    const bool grids_allowed = args.shadows && !(p->flags & RT_DIRECT_NO_SHADOW_GRID) && std::memcmp(&p->bias, &grid_bias, sizeof(float)) == 0;
    rt::direct_light_box(ctx->box_lo, ctx->box_hi, args.lo, args.hi); // (current whenever a device holds grids: ensure_grids)
    const bool counters = (p->flags & RT_QUERY_COUNTERS) != 0;
    const Batch b{fn, n, {"points", points, sizeof(rt_surface_point)}, {{"out", out, sizeof(rt_lighting)}, {}}, RT_QUERY_CHUNK, RT_QUERY_CHUNK, RT_CNT_DIAG};
    Totals t;
    if (int rc = run_batch(ctx, b, t, [&](DeviceState& d, const DevScene& sc, const Chunk& ck) {
            rt::DirectLightArgs a = args;
            a.grids = grids_allowed ? d.grids.table.get() : nullptr; // each device's own
            return rt::launch_direct_light(sc, a, ck.in, ck.out[0], ck.m, counters, d.counters.get(), d.stream);
        }))
        return rc;
    if (counters) ctx->grid_diag[0] = t.cn[RT_CNT_DL_GRID_ANSWERED], ctx->grid_diag[1] = t.cn[RT_CNT_DL_GRID_ENTRIES]; // (rt_debug_shadow_grid: the lists' share of the segments)
    batch_stats(ctx, w0, t, counters, t.cn[RT_CNT_SHADOW], 0, 0, t.cn[RT_CNT_SHADOW]);
    return RT_OK;
}

int rt_radiance(rt_ctx* ctx, const rt_ray* rays, size_t n, const rt_path_params* params, rt_path_result* out) {
    return path_query(ctx, "rt_radiance", {"rays", rays, sizeof(rt_ray)}, n, params, out, sizeof(rt_path_result), false, rt::launch_path_query);
}

int rt_radiance_sh(rt_ctx* ctx, const rt_probe* probes, size_t n, const rt_path_params* params, rt_sh9* out) {
    return path_query(ctx, "rt_radiance_sh", {"probes", probes, sizeof(rt_probe)}, n, params, out, sizeof(rt_sh9), true, rt::launch_probe_query);
}

int rt_irradiance(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_path_params* params, rt_irradiance_result* out) {
    return path_query(ctx, "rt_irradiance", {"points", points, sizeof(rt_surface_point)}, n, params, out, sizeof(rt_irradiance_result), true,
                      rt::launch_irradiance_query);
}

int rt_camera_rays(rt_ctx* ctx, const rt_camera* camera, uint32_t width, uint32_t height, uint32_t mode, rt_ray* out) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (mode != RT_MODE_LEGACY && mode != RT_MODE_WAVEFRONT) return ctx->fail(RT_ERR_BAD_ARG, "rt_camera_rays: mode %u (0 or 1)", mode);
    const size_t n = (size_t)width * height;
    if (n == 0) return RT_OK;
    if (!camera || !out) return ctx->fail(RT_ERR_BAD_ARG, "rt_camera_rays: %s is NULL", !camera ? "camera" : "out");
    // the frames' camera constants (make_camera) and ray generation (camera_ray): the rays are those rt_render traces
    const DevCamera cam = make_camera(*camera, (float)width, (float)height, mode != RT_MODE_LEGACY);
    return generate_rays(ctx, "rt_camera_rays", out, n, [&](void* res, size_t off, uint32_t m, hipStream_t s) {
        return rt::launch_camera_rays(cam, width, mode != RT_MODE_LEGACY, res, off, m, s);
    });
}

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
    sample_jitter(fr, p->flags);
    return generate_rays(ctx, "rt_sample_rays", out, (size_t)fr.width * fr.height, [&](void* res, size_t off, uint32_t m, hipStream_t s) {
        return rt::launch_sample_rays(fr, sample, res, off, m, s);
    });
}

int rt_denoise(rt_ctx* ctx, const rt_denoise_params* dp, const float* rgb, const rt_aov* aov, float* out) {
    if (!ctx) return RT_ERR_BAD_ARG;
    return denoise(ctx, dp, rgb, aov, out);
}

} // extern "C"
