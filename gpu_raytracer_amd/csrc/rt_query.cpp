// rt_query.cpp — calls that trace or filter outside a frame: ray queries (rt_hip.h "Ray queries": rt_intersect, rt_occluded,
// rt_intersect_all, rt_camera_rays), surface queries ("Surface queries": rt_surface, rt_ambient_occlusion; kernels in
// surface_query.hip), the direct-light query ("Direct-light queries": rt_direct_light; kernel in direct_light.hip), the path query ("Path queries":
// rt_radiance; kernels in path_query.hip), the probe query ("Probe queries": rt_radiance_sh; kernels in probe_query.hip), the closest-point query ("Closest-point queries": rt_closest_point; kernel in closest_point.hip), the sphere sweep ("Sphere sweeps": rt_sweep_sphere; kernel in sweep.hip) and the image passes ("Feature buffers (AOVs) and denoising": rt_aovs, rt_sample_rays, rt_denoise; kernels in
// denoise.hip).  None of them touches the frame targets, the tile shares rt_read_* gather, or the running image of an accumulation.
#include "rt_internal.h"

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

// rt_intersect_all's part of a query: max_hits records per ray, and a second output array.
struct MultiHit {
    uint32_t max_hits;
    uint32_t* counts; // may be null
};

// Every query kind: out_elem = the bytes per ray at `out`: 16 (rt_hit), 1 (occluded byte), with `surface` 32 (rt_surface_point), or
// with `mh` max_hits * 16 (`out` is then ignored when that is 0).  Host batches go in chunks of RT_QUERY_CHUNK rays, with `mh` RT_QUERY_CHUNK / max(max_hits, 1): the hit
// records of a chunk never need more staging than an rt_intersect chunk's.
int run_query(rt_ctx* ctx, const char* fn, const rt_ray* rays, size_t n, void* out, size_t out_elem, uint32_t flags, const MultiHit* mh = nullptr,
              bool surface = false) {
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    const char* out_name = out_elem == 1 ? "occluded" : surface ? "out" : "hits";
    uint32_t known = RT_QUERY_COUNTERS;
    if (mh) {
        known |= RT_QUERY_COUNT_ALL;
        if (!rays || (!out && mh->max_hits > 0)) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !rays ? "rays" : out_name, n);
        if (mh->max_hits > RT_MULTI_HIT_MAX) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_hits %u (0 .. %u)", fn, mh->max_hits, RT_MULTI_HIT_MAX);
        if (mh->max_hits == 0 && (!(flags & RT_QUERY_COUNT_ALL) || !mh->counts))
            return ctx->fail(RT_ERR_BAD_ARG, "%s: max_hits 0 needs RT_QUERY_COUNT_ALL and counts", fn);
        if (mh->max_hits == 0) out = nullptr; // ignored
    } else if (!rays || !out) {
        return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !rays ? "rays" : out_name, n);
    }
    if (flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~known);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (int rcp = sync_pending(ctx)) return rcp;
    uint32_t* counts = mh ? mh->counts : nullptr;
    QueryPtr pin, pout, pcnt;
    if (int rc = classify_ptr(ctx, fn, "rays", rays, pin)) return rc;
    if (out) {
        if (int rc = classify_ptr(ctx, fn, out_name, out, pout)) return rc;
    }
    if (counts) {
        if (int rc = classify_ptr(ctx, fn, "counts", counts, pcnt, 4)) return rc;
    }
    if (!out) pout = pcnt, out_name = "counts"; // a pure count: max_hits == 0
    if (!counts) pcnt = pout;
    if (pin.device != pout.device || pin.dev != pout.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: rays (%s %zu) and %s (%s %zu) must both be host memory or both device memory of the same device", fn,
                         pin.device ? "device memory of context device" : "host memory", pin.device ? pin.dev : (size_t)0, out_name,
                         pout.device ? "device memory of context device" : "host memory", pout.device ? pout.dev : (size_t)0);
    if (pcnt.device != pout.device || pcnt.dev != pout.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: rays, hits and counts must all be host memory or all device memory of the same device", fn);
    const size_t chunk = mh ? RT_QUERY_CHUNK / std::max(mh->max_hits, 1u) : RT_QUERY_CHUNK;
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0;
    const size_t nd = ctx->devs.size();
    std::vector<size_t> first(nd, 0), count(nd, 0);
    if (pin.device) count[pin.dev] = n; // a device batch runs where it lives
    else
        for (size_t j = 0; j < nd; j++) first[j] = n * j / nd, count[j] = n * (j + 1) / nd - first[j]; // contiguous ranges, one per device
    const uint8_t* src = reinterpret_cast<const uint8_t*>(rays);
    uint8_t* dst = reinterpret_cast<uint8_t*>(out);
    const bool all = (flags & RT_QUERY_COUNT_ALL) != 0;
    // every device's range is enqueued before any is waited for
    auto enqueue = [&](size_t j) -> int {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        const DevScene sc = scene_for(ctx, d);
        const size_t chunks = (count[j] + chunk - 1) / chunk;
        if (int rc = ensure_query_events(ctx, d, 2 * chunks)) return rc;
        if (!pin.device) {
            const size_t m = std::min<size_t>(count[j], chunk);
            HIPCHK(ctx, d.rq.in.reserve(m * sizeof(rt_ray)));
            HIPCHK(ctx, d.rq.out.reserve(m * out_elem));
            if (counts) HIPCHK(ctx, d.rq.counts.reserve(m * sizeof(uint32_t)));
        }
        if (counters) HIPCHK(ctx, hipMemsetAsync(d.counters.get(), 0, (RT_CNT_TRI_TESTS + 1) * sizeof(unsigned long long), d.stream));
        for (size_t c = 0; c < chunks; c++) {
            const size_t off = first[j] + c * chunk, m = std::min<size_t>(chunk, first[j] + count[j] - off);
            const void* in = src + off * sizeof(rt_ray);
            void* res = out ? dst + off * out_elem : nullptr;
            uint32_t* res_counts = counts ? counts + off : nullptr;
            if (!pin.device) {
                HIPCHK(ctx, hipMemcpyAsync(d.rq.in.get(), in, m * sizeof(rt_ray), hipMemcpyHostToDevice, d.stream));
                in = d.rq.in.get();
                res = d.rq.out.get();
                if (counts) res_counts = static_cast<uint32_t*>(d.rq.counts.get());
            }
            unsigned long long* cnt = counters ? d.counters.get() : nullptr;
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c], d.stream));
            if (mh) HIPCHK(ctx, rt::launch_ray_query_all(sc, in, res, res_counts, (uint32_t)m, mh->max_hits, all, cnt, d.stream));
            else if (surface) HIPCHK(ctx, rt::launch_surface_query(sc, in, res, (uint32_t)m, cnt, d.stream));
            else HIPCHK(ctx, rt::launch_ray_query(sc, in, res, (uint32_t)m, out_elem == 1, cnt, d.stream));
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c + 1], d.stream));
            if (!pin.device && out) HIPCHK(ctx, hipMemcpyAsync(dst + off * out_elem, res, m * out_elem, hipMemcpyDeviceToHost, d.stream));
            if (!pin.device && counts) HIPCHK(ctx, hipMemcpyAsync(counts + off, res_counts, m * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
        }
        return RT_OK;
    };
    for (size_t j = 0; j < nd; j++)
        if (count[j] > 0)
            if (int rc = enqueue(j)) {
                drain_streams(ctx);
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
            drain_streams(ctx);
            return ctx->fail(RT_ERR_HIP, "%s: device %d: %s", fn, d.device, hipGetErrorString(e));
        }
        double ms = 0.0;
        for (size_t c = 0; 2 * c + 1 < d.rq_events.size() && c * chunk < count[j]; c++) {
            float cm = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&cm, d.rq_events[2 * c], d.rq_events[2 * c + 1]));
            ms += cm;
        }
        kernel_ms = std::max(kernel_ms, ms);
        if (counters) {
            unsigned long long cn[RT_CNT_TRI_TESTS + 1];
            HIPCHK(ctx, hipMemcpy(cn, d.counters.get(), sizeof cn, hipMemcpyDeviceToHost));
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

// rt_ambient_occlusion: run_query's shape with points for rays, samples lanes per point and two optional outputs.  Every chunk (host
// batches: max(1, RT_QUERY_CHUNK / samples) points; a device batch: RT_AO_DEVICE_CHUNK) zeroes the device's per-point counts, lets the
// kernel add to them and finishes them into visibility and counts; the chunk's first index goes to the kernel, so a point's seed is
// that of its place in the caller's array.
constexpr size_t RT_AO_DEVICE_CHUNK = (size_t)1 << 24; // points of a device batch per chunk: bounds the counts beside them (64 MiB)

int run_ao(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_ao_params* p, float* visibility, uint32_t* unoccluded) {
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
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pin, pvis, pcnt;
    if (int rc = classify_ptr(ctx, fn, "points", points, pin)) return rc;
    if (visibility) {
        if (int rc = classify_ptr(ctx, fn, "visibility", visibility, pvis, 4)) return rc;
    }
    if (unoccluded) {
        if (int rc = classify_ptr(ctx, fn, "unoccluded", unoccluded, pcnt, 4)) return rc;
    }
    if (!visibility) pvis = pcnt;
    if (!unoccluded) pcnt = pvis;
    if (pin.device != pvis.device || pin.dev != pvis.dev || pin.device != pcnt.device || pin.dev != pcnt.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: points, visibility and unoccluded must all be host memory or all device memory of the same device", fn);
    const rt::AoParams ap{p->samples, p->seed, p->max_distance, p->bias};
    const size_t chunk = pin.device ? RT_AO_DEVICE_CHUNK : std::max<size_t>(1, RT_QUERY_CHUNK / p->samples);
    const bool counters = (p->flags & RT_QUERY_COUNTERS) != 0;
    const size_t nd = ctx->devs.size();
    std::vector<size_t> first(nd, 0), count(nd, 0);
    if (pin.device) count[pin.dev] = n; // a device batch runs where it lives
    else
        for (size_t j = 0; j < nd; j++) first[j] = n * j / nd, count[j] = n * (j + 1) / nd - first[j]; // contiguous ranges, one per device
    // every device's range is enqueued before any is waited for
    auto enqueue = [&](size_t j) -> int {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        const DevScene sc = scene_for(ctx, d);
        const size_t chunks = (count[j] + chunk - 1) / chunk;
        if (int rc = ensure_query_events(ctx, d, 2 * chunks)) return rc;
        const size_t most = std::min<size_t>(count[j], chunk);
        HIPCHK(ctx, d.rq.ao.reserve(most * sizeof(uint32_t)));
        if (!pin.device) {
            HIPCHK(ctx, d.rq.in.reserve(most * sizeof(rt_surface_point)));
            if (visibility) HIPCHK(ctx, d.rq.out.reserve(most * sizeof(float)));
        }
        if (counters) HIPCHK(ctx, hipMemsetAsync(d.counters.get(), 0, (RT_CNT_TRI_TESTS + 1) * sizeof(unsigned long long), d.stream));
        for (size_t c = 0; c < chunks; c++) {
            const size_t off = first[j] + c * chunk, m = std::min<size_t>(chunk, first[j] + count[j] - off);
            const void* in = points + off;
            float* vis = visibility ? visibility + off : nullptr;
            uint32_t* cnt_out = unoccluded ? unoccluded + off : nullptr;
            if (!pin.device) {
                HIPCHK(ctx, hipMemcpyAsync(d.rq.in.get(), in, m * sizeof(rt_surface_point), hipMemcpyHostToDevice, d.stream));
                in = d.rq.in.get();
                vis = visibility ? static_cast<float*>(d.rq.out.get()) : nullptr;
                cnt_out = nullptr; // the counts go to the host from where the kernel left them
            }
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c], d.stream));
            HIPCHK(ctx, hipMemsetAsync(d.rq.ao.get(), 0, m * sizeof(uint32_t), d.stream));
            HIPCHK(ctx, rt::launch_ao(sc, in, off, (uint32_t)m, ap, d.rq.ao.get(), counters ? d.counters.get() : nullptr, d.stream));
            if (vis || cnt_out) HIPCHK(ctx, rt::launch_ao_finish(d.rq.ao.get(), (uint32_t)m, ap.samples, vis, cnt_out, d.stream));
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c + 1], d.stream));
            if (!pin.device && visibility) HIPCHK(ctx, hipMemcpyAsync(visibility + off, vis, m * sizeof(float), hipMemcpyDeviceToHost, d.stream));
            if (!pin.device && unoccluded) HIPCHK(ctx, hipMemcpyAsync(unoccluded + off, d.rq.ao.get(), m * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
        }
        return RT_OK;
    };
    for (size_t j = 0; j < nd; j++)
        if (count[j] > 0)
            if (int rc = enqueue(j)) {
                drain_streams(ctx);
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
            drain_streams(ctx);
            return ctx->fail(RT_ERR_HIP, "%s: device %d: %s", fn, d.device, hipGetErrorString(e));
        }
        double ms = 0.0;
        for (size_t c = 0; c * chunk < count[j]; c++) {
            float cm = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&cm, d.rq_events[2 * c], d.rq_events[2 * c + 1]));
            ms += cm;
        }
        kernel_ms = std::max(kernel_ms, ms);
        if (counters) {
            unsigned long long cn[RT_CNT_TRI_TESTS + 1];
            HIPCHK(ctx, hipMemcpy(cn, d.counters.get(), sizeof cn, hipMemcpyDeviceToHost));
            nodes += cn[RT_CNT_NODE_VISITS];
            tris += cn[RT_CNT_TRI_TESTS];
        }
    }
    rt_stats& st = ctx->stats;
    st.rays = (uint64_t)n * p->samples;
    st.primary_rays = st.continuation_rays = st.shadow_rays = st.pixels = 0;
    st.node_visits = counters ? nodes : 0;
    st.tri_tests = counters ? tris : 0;
    st.kernel_ms = kernel_ms;
    st.wall_ms = now_ms() - w0;
    return RT_OK;
}

// rt_direct_light: run_ao's shape with one 16-byte record out per point.  The segments are counted on the device (rt_stats.rays), so
// every call zeroes and reads the device's counters.  A device hands over the light grids it already holds - from rt_prepare or an
// extended-mode frame - when the call's bias is the one they were derived for; this call never builds any (ensure_grids).
static_assert(RT_DIRECT_MAX_LIGHTS == RT_WF_MAX_LIGHTS, "the grid table and lit_mask hold one entry / bit per light, as the pipeline's visibility word");
int run_direct_light(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_direct_light_params* p, rt_lighting* out) {
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
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pin, pout;
    if (int rc = classify_ptr(ctx, fn, "points", points, pin)) return rc;
    if (int rc = classify_ptr(ctx, fn, "out", out, pout)) return rc;
    if (pin.device != pout.device || pin.dev != pout.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: points and out must both be host memory or both device memory of the same device", fn);
    rt::DirectLightArgs args{};
    args.bias = p->bias;
    args.ambient = (p->flags & RT_DIRECT_AMBIENT) ? 1u : 0u;
    args.shadows = (p->flags & RT_DIRECT_NO_SHADOWS) ? 0u : 1u;
    // the lists are supersets of what the triangle test accepts for segments that start EXT_EPS off their point: any other bias walks the tree
    const float grid_bias = RT_SG_EXT_EPS;
    const bool grids_allowed = args.shadows && !(p->flags & RT_DIRECT_NO_SHADOW_GRID) && std::memcmp(&p->bias, &grid_bias, sizeof(float)) == 0;
    rt::direct_light_box(ctx->box_lo, ctx->box_hi, args.lo, args.hi); // (current whenever a device holds grids: ensure_grids)
    const size_t chunk = RT_QUERY_CHUNK;
    const bool counters = (p->flags & RT_QUERY_COUNTERS) != 0;
    const size_t nd = ctx->devs.size();
    std::vector<size_t> first(nd, 0), count(nd, 0);
    if (pin.device) count[pin.dev] = n; // a device batch runs where it lives
    else
        for (size_t j = 0; j < nd; j++) first[j] = n * j / nd, count[j] = n * (j + 1) / nd - first[j]; // contiguous ranges, one per device
    // every device's range is enqueued before any is waited for
    auto enqueue = [&](size_t j) -> int {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        const DevScene sc = scene_for(ctx, d);
        rt::DirectLightArgs a = args;
        a.grids = grids_allowed ? d.grids.table.get() : nullptr;
        const size_t chunks = (count[j] + chunk - 1) / chunk;
        if (int rc = ensure_query_events(ctx, d, 2 * chunks)) return rc;
        if (!pin.device) {
            const size_t most = std::min<size_t>(count[j], chunk);
            HIPCHK(ctx, d.rq.in.reserve(most * sizeof(rt_surface_point)));
            HIPCHK(ctx, d.rq.out.reserve(most * sizeof(rt_lighting)));
        }
        HIPCHK(ctx, hipMemsetAsync(d.counters.get(), 0, RT_CNT_DIAG * sizeof(unsigned long long), d.stream));
        for (size_t c = 0; c < chunks; c++) {
            const size_t off = first[j] + c * chunk, m = std::min<size_t>(chunk, first[j] + count[j] - off);
            const void* in = points + off;
            void* res = out + off;
            if (!pin.device) {
                HIPCHK(ctx, hipMemcpyAsync(d.rq.in.get(), in, m * sizeof(rt_surface_point), hipMemcpyHostToDevice, d.stream));
                in = d.rq.in.get();
                res = d.rq.out.get();
            }
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c], d.stream));
            HIPCHK(ctx, rt::launch_direct_light(sc, a, in, res, (uint32_t)m, counters, d.counters.get(), d.stream));
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c + 1], d.stream));
            if (!pin.device) HIPCHK(ctx, hipMemcpyAsync(out + off, res, m * sizeof(rt_lighting), hipMemcpyDeviceToHost, d.stream));
        }
        return RT_OK;
    };
    for (size_t j = 0; j < nd; j++)
        if (count[j] > 0)
            if (int rc = enqueue(j)) {
                drain_streams(ctx);
                return rc;
            }
    double kernel_ms = 0.0;
    unsigned long long segments = 0, nodes = 0, tris = 0, answered = 0, entries = 0;
    for (size_t j = 0; j < nd; j++) {
        if (count[j] == 0) continue;
        DeviceState& d = ctx->devs[j];
        hipError_t e = hipSetDevice(d.device);
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        if (e != hipSuccess) {
            drain_streams(ctx);
            return ctx->fail(RT_ERR_HIP, "%s: device %d: %s", fn, d.device, hipGetErrorString(e));
        }
        double ms = 0.0;
        for (size_t c = 0; c * chunk < count[j]; c++) {
            float cm = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&cm, d.rq_events[2 * c], d.rq_events[2 * c + 1]));
            ms += cm;
        }
        kernel_ms = std::max(kernel_ms, ms);
        unsigned long long cn[RT_CNT_DIAG];
        HIPCHK(ctx, hipMemcpy(cn, d.counters.get(), sizeof cn, hipMemcpyDeviceToHost));
        segments += cn[RT_CNT_SHADOW];
        nodes += cn[RT_CNT_NODE_VISITS];
        tris += cn[RT_CNT_TRI_TESTS];
        answered += cn[RT_CNT_DL_GRID_ANSWERED];
        entries += cn[RT_CNT_DL_GRID_ENTRIES];
    }
    if (counters) ctx->grid_diag[0] = answered, ctx->grid_diag[1] = entries; // (rt_debug_shadow_grid: the lists' share of the segments)
    rt_stats& st = ctx->stats;
    st.rays = st.shadow_rays = segments;
    st.primary_rays = st.continuation_rays = st.pixels = 0;
    st.node_visits = counters ? nodes : 0;
    st.tri_tests = counters ? tris : 0;
    st.kernel_ms = kernel_ms;
    st.wall_ms = now_ms() - w0;
    return RT_OK;
}

// rt_radiance: run_direct_light's shape with rays in, samples paths per ray and a per-device scratch of one record per path.  Host and
// device batches alike go in chunks of max(1, RT_QUERY_CHUNK / samples) rays, so a launch covers at most RT_QUERY_CHUNK paths and the
// scratch never grows past that; the chunk's first index goes to the kernel, so a ray's seed is that of its place in the caller's array.
// The segments are counted on the device (rt_stats.rays), so every call zeroes and reads the device's counters.
int run_radiance(rt_ctx* ctx, const rt_ray* rays, size_t n, const rt_path_params* p, rt_path_result* out) {
    const char* fn = "rt_radiance";
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!rays || !p || !out) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !rays ? "rays" : !p ? "params" : "out", n);
    if (p->samples < 1 || p->samples > RT_PATH_MAX_SAMPLES) return ctx->fail(RT_ERR_BAD_ARG, "%s: samples %u (1 .. %u)", fn, p->samples, RT_PATH_MAX_SAMPLES);
    if (p->max_bounces > RT_MAX_BOUNCES) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_bounces %u (0 .. %u)", fn, p->max_bounces, RT_MAX_BOUNCES);
    if ((uint64_t)p->first_sample + p->samples > (1ull << 32))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: first_sample %u + samples %u passes 2^32", fn, p->first_sample, p->samples);
    const uint32_t known = RT_QUERY_COUNTERS | RT_PATH_NO_SHADOWS | RT_PATH_CAMERA_DRAWS;
    if (p->flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, p->flags & ~known);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pin, pout;
    if (int rc = classify_ptr(ctx, fn, "rays", rays, pin)) return rc;
    if (int rc = classify_ptr(ctx, fn, "out", out, pout)) return rc;
    if (pin.device != pout.device || pin.dev != pout.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: rays and out must both be host memory or both device memory of the same device", fn);
    const rt::PathArgs args{p->samples, p->max_bounces, p->seed, p->first_sample, (p->flags & RT_PATH_NO_SHADOWS) ? 0u : 1u,
                            (p->flags & RT_PATH_CAMERA_DRAWS) ? 1u : 0u};
    const size_t chunk = std::max<size_t>(1, RT_QUERY_CHUNK / p->samples);
    const bool counters = (p->flags & RT_QUERY_COUNTERS) != 0;
    const size_t nd = ctx->devs.size();
    std::vector<size_t> first(nd, 0), count(nd, 0);
    if (pin.device) count[pin.dev] = n; // a device batch runs where it lives
    else
        for (size_t j = 0; j < nd; j++) first[j] = n * j / nd, count[j] = n * (j + 1) / nd - first[j]; // contiguous ranges, one per device
    // every device's range is enqueued before any is waited for
    auto enqueue = [&](size_t j) -> int {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        const DevScene sc = scene_for(ctx, d);
        const size_t chunks = (count[j] + chunk - 1) / chunk;
        // a host batch times each chunk's launches apart from its copies; a device batch has no copies between its launches: one pair
        if (int rc = ensure_query_events(ctx, d, pin.device ? 2 : 2 * chunks)) return rc;
        const size_t most = std::min<size_t>(count[j], chunk);
        if (args.samples > 1) HIPCHK(ctx, d.rq.paths.reserve(most * args.samples * sizeof(uint4)));
        if (!pin.device) {
            HIPCHK(ctx, d.rq.in.reserve(most * sizeof(rt_ray)));
            HIPCHK(ctx, d.rq.out.reserve(most * sizeof(rt_path_result)));
        }
        HIPCHK(ctx, hipMemsetAsync(d.counters.get(), 0, RT_CNT_DIAG * sizeof(unsigned long long), d.stream));
        for (size_t c = 0; c < chunks; c++) {
            const size_t off = first[j] + c * chunk, m = std::min<size_t>(chunk, first[j] + count[j] - off);
            const void* in = rays + off;
            void* res = out + off;
            if (!pin.device) {
                HIPCHK(ctx, hipMemcpyAsync(d.rq.in.get(), in, m * sizeof(rt_ray), hipMemcpyHostToDevice, d.stream));
                in = d.rq.in.get();
                res = d.rq.out.get();
            }
            if (!pin.device || c == 0) HIPCHK(ctx, hipEventRecord(d.rq_events[pin.device ? 0 : 2 * c], d.stream));
            HIPCHK(ctx, rt::launch_path_query(sc, args, in, off, (uint32_t)m, d.rq.paths.get(), res, counters, d.counters.get(), d.stream));
            if (!pin.device || c + 1 == chunks) HIPCHK(ctx, hipEventRecord(d.rq_events[pin.device ? 1 : 2 * c + 1], d.stream));
            if (!pin.device) HIPCHK(ctx, hipMemcpyAsync(out + off, res, m * sizeof(rt_path_result), hipMemcpyDeviceToHost, d.stream));
        }
        return RT_OK;
    };
    for (size_t j = 0; j < nd; j++)
        if (count[j] > 0)
            if (int rc = enqueue(j)) {
                drain_streams(ctx);
                return rc;
            }
    double kernel_ms = 0.0;
    unsigned long long camera = 0, continuation = 0, shadow = 0, nodes = 0, tris = 0;
    for (size_t j = 0; j < nd; j++) {
        if (count[j] == 0) continue;
        DeviceState& d = ctx->devs[j];
        hipError_t e = hipSetDevice(d.device);
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        if (e != hipSuccess) {
            drain_streams(ctx);
            return ctx->fail(RT_ERR_HIP, "%s: device %d: %s", fn, d.device, hipGetErrorString(e));
        }
        double ms = 0.0;
        for (size_t c = 0; c * chunk < count[j] && (c == 0 || !pin.device); c++) {
            float cm = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&cm, d.rq_events[2 * c], d.rq_events[2 * c + 1]));
            ms += cm;
        }
        kernel_ms = std::max(kernel_ms, ms);
        unsigned long long cn[RT_CNT_DIAG];
        HIPCHK(ctx, hipMemcpy(cn, d.counters.get(), sizeof cn, hipMemcpyDeviceToHost));
        camera += cn[RT_CNT_CAMERA];
        continuation += cn[RT_CNT_CONTINUATION];
        shadow += cn[RT_CNT_SHADOW];
        nodes += cn[RT_CNT_NODE_VISITS];
        tris += cn[RT_CNT_TRI_TESTS];
    }
    rt_stats& st = ctx->stats;
    st.rays = camera + continuation + shadow;
    st.primary_rays = camera;
    st.continuation_rays = continuation;
    st.shadow_rays = shadow;
    st.pixels = 0;
    st.node_visits = counters ? nodes : 0;
    st.tri_tests = counters ? tris : 0;
    st.kernel_ms = kernel_ms;
    st.wall_ms = now_ms() - w0;
    return RT_OK;
}

// rt_radiance_sh: run_radiance's shape with probes for rays (16 bytes in, 112 bytes out per probe).  The scratch of one record per path
// is used with any number of samples: the record is not the result, a projection always runs.
int run_radiance_sh(rt_ctx* ctx, const rt_probe* probes, size_t n, const rt_path_params* p, rt_sh9* out) {
    const char* fn = "rt_radiance_sh";
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!probes || !p || !out) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !probes ? "probes" : !p ? "params" : "out", n);
    if (p->samples < 1 || p->samples > RT_PATH_MAX_SAMPLES) return ctx->fail(RT_ERR_BAD_ARG, "%s: samples %u (1 .. %u)", fn, p->samples, RT_PATH_MAX_SAMPLES);
    if (p->max_bounces > RT_MAX_BOUNCES) return ctx->fail(RT_ERR_BAD_ARG, "%s: max_bounces %u (0 .. %u)", fn, p->max_bounces, RT_MAX_BOUNCES);
    if ((uint64_t)p->first_sample + p->samples > (1ull << 32))
        return ctx->fail(RT_ERR_BAD_ARG, "%s: first_sample %u + samples %u passes 2^32", fn, p->first_sample, p->samples);
    if (p->flags & RT_PATH_CAMERA_DRAWS) return ctx->fail(RT_ERR_BAD_ARG, "%s: flags: RT_PATH_CAMERA_DRAWS (the call spends those two draws itself)", fn);
    const uint32_t known = RT_QUERY_COUNTERS | RT_PATH_NO_SHADOWS;
    if (p->flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, p->flags & ~known);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pin, pout;
    if (int rc = classify_ptr(ctx, fn, "probes", probes, pin)) return rc;
    if (int rc = classify_ptr(ctx, fn, "out", out, pout)) return rc;
    if (pin.device != pout.device || pin.dev != pout.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: probes and out must both be host memory or both device memory of the same device", fn);
    const rt::PathArgs args{p->samples, p->max_bounces, p->seed, p->first_sample, (p->flags & RT_PATH_NO_SHADOWS) ? 0u : 1u, 1u};
    const size_t chunk = std::max<size_t>(1, RT_QUERY_CHUNK / p->samples);
    const bool counters = (p->flags & RT_QUERY_COUNTERS) != 0;
    const size_t nd = ctx->devs.size();
    std::vector<size_t> first(nd, 0), count(nd, 0);
    if (pin.device) count[pin.dev] = n; // a device batch runs where it lives
    else
        for (size_t j = 0; j < nd; j++) first[j] = n * j / nd, count[j] = n * (j + 1) / nd - first[j]; // contiguous ranges, one per device
    // every device's range is enqueued before any is waited for
    auto enqueue = [&](size_t j) -> int {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        const DevScene sc = scene_for(ctx, d);
        const size_t chunks = (count[j] + chunk - 1) / chunk;
        // a host batch times each chunk's launches apart from its copies; a device batch has no copies between its launches: one pair
        if (int rc = ensure_query_events(ctx, d, pin.device ? 2 : 2 * chunks)) return rc;
        const size_t most = std::min<size_t>(count[j], chunk);
        HIPCHK(ctx, d.rq.paths.reserve(most * args.samples * sizeof(uint4)));
        if (!pin.device) {
            HIPCHK(ctx, d.rq.in.reserve(most * sizeof(rt_probe)));
            HIPCHK(ctx, d.rq.out.reserve(most * sizeof(rt_sh9)));
        }
        HIPCHK(ctx, hipMemsetAsync(d.counters.get(), 0, RT_CNT_DIAG * sizeof(unsigned long long), d.stream));
        for (size_t c = 0; c < chunks; c++) {
            const size_t off = first[j] + c * chunk, m = std::min<size_t>(chunk, first[j] + count[j] - off);
            const void* in = probes + off;
            void* res = out + off;
            if (!pin.device) {
                HIPCHK(ctx, hipMemcpyAsync(d.rq.in.get(), in, m * sizeof(rt_probe), hipMemcpyHostToDevice, d.stream));
                in = d.rq.in.get();
                res = d.rq.out.get();
            }
            if (!pin.device || c == 0) HIPCHK(ctx, hipEventRecord(d.rq_events[pin.device ? 0 : 2 * c], d.stream));
            HIPCHK(ctx, rt::launch_probe_query(sc, args, in, off, (uint32_t)m, d.rq.paths.get(), res, counters, d.counters.get(), d.stream));
            if (!pin.device || c + 1 == chunks) HIPCHK(ctx, hipEventRecord(d.rq_events[pin.device ? 1 : 2 * c + 1], d.stream));
            if (!pin.device) HIPCHK(ctx, hipMemcpyAsync(out + off, res, m * sizeof(rt_sh9), hipMemcpyDeviceToHost, d.stream));
        }
        return RT_OK;
    };
    for (size_t j = 0; j < nd; j++)
        if (count[j] > 0)
            if (int rc = enqueue(j)) {
                drain_streams(ctx);
                return rc;
            }
    double kernel_ms = 0.0;
    unsigned long long camera = 0, continuation = 0, shadow = 0, nodes = 0, tris = 0;
    for (size_t j = 0; j < nd; j++) {
        if (count[j] == 0) continue;
        DeviceState& d = ctx->devs[j];
        hipError_t e = hipSetDevice(d.device);
        if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
        if (e != hipSuccess) {
            drain_streams(ctx);
            return ctx->fail(RT_ERR_HIP, "%s: device %d: %s", fn, d.device, hipGetErrorString(e));
        }
        double ms = 0.0;
        for (size_t c = 0; c * chunk < count[j] && (c == 0 || !pin.device); c++) {
            float cm = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&cm, d.rq_events[2 * c], d.rq_events[2 * c + 1]));
            ms += cm;
        }
        kernel_ms = std::max(kernel_ms, ms);
        unsigned long long cn[RT_CNT_DIAG];
        HIPCHK(ctx, hipMemcpy(cn, d.counters.get(), sizeof cn, hipMemcpyDeviceToHost));
        camera += cn[RT_CNT_CAMERA];
        continuation += cn[RT_CNT_CONTINUATION];
        shadow += cn[RT_CNT_SHADOW];
        nodes += cn[RT_CNT_NODE_VISITS];
        tris += cn[RT_CNT_TRI_TESTS];
    }
    rt_stats& st = ctx->stats;
    st.rays = camera + continuation + shadow;
    st.primary_rays = camera;
    st.continuation_rays = continuation;
    st.shadow_rays = shadow;
    st.pixels = 0;
    st.node_visits = counters ? nodes : 0;
    st.tri_tests = counters ? tris : 0;
    st.kernel_ms = kernel_ms;
    st.wall_ms = now_ms() - w0;
    return RT_OK;
}

// rt_closest_point and rt_sweep_sphere: run_query's shape with records of in_size bytes for rays and records of out_size bytes out,
// one lane of `launch` per record.  in_name: what the records are called in messages.
using RecordLaunch = hipError_t (*)(const DevScene&, const void*, void*, uint32_t, unsigned long long*, hipStream_t);
int run_record_query(rt_ctx* ctx, const char* fn, const char* in_name, const void* records, size_t in_size, size_t n, void* results, size_t out_size,
                     uint32_t flags, RecordLaunch launch) {
    const char* points = static_cast<const char*>(records);
    char* out = static_cast<char*>(results);
    const double w0 = now_ms();
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (!points || !out) return ctx->fail(RT_ERR_BAD_ARG, "%s: %s is NULL with n = %zu", fn, !points ? in_name : "out", n);
    if (flags & ~RT_QUERY_COUNTERS) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~RT_QUERY_COUNTERS);
    if (!ctx->uploaded) return ctx->fail(RT_ERR_NOT_UPLOADED, "%s: no scene uploaded", fn);
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr pin, pout;
    if (int rc = classify_ptr(ctx, fn, in_name, points, pin)) return rc;
    if (int rc = classify_ptr(ctx, fn, "out", out, pout)) return rc;
    if (pin.device != pout.device || pin.dev != pout.dev)
        return ctx->fail(RT_ERR_BAD_ARG, "%s: %s and out must both be host memory or both device memory of the same device", fn, in_name);
    const size_t chunk = RT_QUERY_CHUNK;
    const bool counters = (flags & RT_QUERY_COUNTERS) != 0;
    const size_t nd = ctx->devs.size();
    std::vector<size_t> first(nd, 0), count(nd, 0);
    if (pin.device) count[pin.dev] = n; // a device batch runs where it lives
    else
        for (size_t j = 0; j < nd; j++) first[j] = n * j / nd, count[j] = n * (j + 1) / nd - first[j]; // contiguous ranges, one per device
    // every device's range is enqueued before any is waited for
    auto enqueue = [&](size_t j) -> int {
        DeviceState& d = ctx->devs[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        const DevScene sc = scene_for(ctx, d);
        const size_t chunks = (count[j] + chunk - 1) / chunk;
        if (int rc = ensure_query_events(ctx, d, 2 * chunks)) return rc;
        if (!pin.device) {
            const size_t most = std::min<size_t>(count[j], chunk);
            HIPCHK(ctx, d.rq.in.reserve(most * in_size));
            HIPCHK(ctx, d.rq.out.reserve(most * out_size));
        }
        if (counters) HIPCHK(ctx, hipMemsetAsync(d.counters.get(), 0, (RT_CNT_TRI_TESTS + 1) * sizeof(unsigned long long), d.stream));
        for (size_t c = 0; c < chunks; c++) {
            const size_t off = first[j] + c * chunk, m = std::min<size_t>(chunk, first[j] + count[j] - off);
            const void* in = points + off * in_size;
            void* res = out + off * out_size;
            if (!pin.device) {
                HIPCHK(ctx, hipMemcpyAsync(d.rq.in.get(), in, m * in_size, hipMemcpyHostToDevice, d.stream));
                in = d.rq.in.get();
                res = d.rq.out.get();
            }
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c], d.stream));
            HIPCHK(ctx, launch(sc, in, res, (uint32_t)m, counters ? d.counters.get() : nullptr, d.stream));
            HIPCHK(ctx, hipEventRecord(d.rq_events[2 * c + 1], d.stream));
            if (!pin.device) HIPCHK(ctx, hipMemcpyAsync(out + off * out_size, res, m * out_size, hipMemcpyDeviceToHost, d.stream));
        }
        return RT_OK;
    };
    for (size_t j = 0; j < nd; j++)
        if (count[j] > 0)
            if (int rc = enqueue(j)) {
                drain_streams(ctx);
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
            drain_streams(ctx);
            return ctx->fail(RT_ERR_HIP, "%s: device %d: %s", fn, d.device, hipGetErrorString(e));
        }
        double ms = 0.0;
        for (size_t c = 0; c * chunk < count[j]; c++) {
            float cm = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&cm, d.rq_events[2 * c], d.rq_events[2 * c + 1]));
            ms += cm;
        }
        kernel_ms = std::max(kernel_ms, ms);
        if (counters) {
            unsigned long long cn[RT_CNT_TRI_TESTS + 1];
            HIPCHK(ctx, hipMemcpy(cn, d.counters.get(), sizeof cn, hipMemcpyDeviceToHost));
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

} // namespace

} // namespace rti

using namespace rti;

extern "C" {

int rt_intersect(rt_ctx* ctx, const rt_ray* rays, size_t n, rt_hit* hits, uint32_t flags) {
    return run_query(ctx, "rt_intersect", rays, n, hits, sizeof(rt_hit), flags);
}

int rt_occluded(rt_ctx* ctx, const rt_ray* rays, size_t n, uint8_t* occluded, uint32_t flags) {
    return run_query(ctx, "rt_occluded", rays, n, occluded, 1, flags);
}

int rt_intersect_all(rt_ctx* ctx, const rt_ray* rays, size_t n, uint32_t max_hits, rt_hit* hits, uint32_t* counts, uint32_t flags) {
    const MultiHit mh{max_hits, counts};
    return run_query(ctx, "rt_intersect_all", rays, n, hits, (size_t)max_hits * sizeof(rt_hit), flags, &mh);
}

int rt_surface(rt_ctx* ctx, const rt_ray* rays, size_t n, rt_surface_point* out, uint32_t flags) {
    return run_query(ctx, "rt_surface", rays, n, out, sizeof(rt_surface_point), flags, nullptr, true);
}

int rt_ambient_occlusion(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_ao_params* params, float* visibility, uint32_t* unoccluded) {
    return run_ao(ctx, points, n, params, visibility, unoccluded);
}

int rt_direct_light(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_direct_light_params* params, rt_lighting* out) {
    return run_direct_light(ctx, points, n, params, out);
}

int rt_radiance(rt_ctx* ctx, const rt_ray* rays, size_t n, const rt_path_params* params, rt_path_result* out) {
    return run_radiance(ctx, rays, n, params, out);
}

int rt_radiance_sh(rt_ctx* ctx, const rt_probe* probes, size_t n, const rt_path_params* params, rt_sh9* out) {
    return run_radiance_sh(ctx, probes, n, params, out);
}

int rt_closest_point(rt_ctx* ctx, const rt_point_query* points, size_t n, rt_nearest* out, uint32_t flags) {
    return run_record_query(ctx, "rt_closest_point", "points", points, sizeof(rt_point_query), n, out, sizeof(rt_nearest), flags, rt::launch_closest_point);
}
int rt_sweep_sphere(rt_ctx* ctx, const rt_sweep* sweeps, size_t n, rt_sweep_hit* out, uint32_t flags) {
    return run_record_query(ctx, "rt_sweep_sphere", "sweeps", sweeps, sizeof(rt_sweep), n, out, sizeof(rt_sweep_hit), flags, rt::launch_sweep_sphere);
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
        HIPCHK(ctx, d.rq.in.reserve(std::min<size_t>(n, RT_QUERY_CHUNK) * sizeof(rt_ray)));
    // the frames' camera constants (make_camera) and ray generation (camera_ray): the rays are those rt_render traces
    const DevCamera cam = make_camera(*camera, (float)width, (float)height, mode != RT_MODE_LEGACY);
    uint8_t* dst = reinterpret_cast<uint8_t*>(out);
    for (size_t off = 0; off < n; off += RT_QUERY_CHUNK) {
        const size_t m = std::min<size_t>(RT_QUERY_CHUNK, n - off);
        void* res = po.device ? (void*)(dst + off * sizeof(rt_ray)) : d.rq.in.get();
        hipError_t e = rt::launch_camera_rays(cam, width, mode != RT_MODE_LEGACY, res, off, (uint32_t)m, d.stream);
        if (e == hipSuccess && !po.device) e = hipMemcpyAsync(dst + off * sizeof(rt_ray), d.rq.in.get(), m * sizeof(rt_ray), hipMemcpyDeviceToHost, d.stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(d.stream);
            return ctx->fail(RT_ERR_HIP, "rt_camera_rays: %s", hipGetErrorString(e));
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    return RT_OK;
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
    if (int rcp = sync_pending(ctx)) return rcp;
    QueryPtr po;
    if (int rc = classify_ptr(ctx, "rt_sample_rays", "out", out, po)) return rc;
    sample_jitter(fr, p->flags);
    const size_t n = (size_t)fr.width * fr.height;
    DeviceState& d = ctx->devs[po.dev];
    HIPCHK(ctx, hipSetDevice(d.device));
    if (!po.device)
        HIPCHK(ctx, d.rq.in.reserve(std::min<size_t>(n, RT_QUERY_CHUNK) * sizeof(rt_ray)));
    uint8_t* dst = reinterpret_cast<uint8_t*>(out);
    for (size_t off = 0; off < n; off += RT_QUERY_CHUNK) { // as rt_camera_rays
        const size_t m = std::min<size_t>(RT_QUERY_CHUNK, n - off);
        void* res = po.device ? (void*)(dst + off * sizeof(rt_ray)) : d.rq.in.get();
        hipError_t e = rt::launch_sample_rays(fr, sample, res, off, (uint32_t)m, d.stream);
        if (e == hipSuccess && !po.device) e = hipMemcpyAsync(dst + off * sizeof(rt_ray), d.rq.in.get(), m * sizeof(rt_ray), hipMemcpyDeviceToHost, d.stream);
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
