// rt_frame.cpp — frames: targets, pipeline sizing and allocation, kernel choice, the round-robin launch loop, totals, accumulation,
// rt_render / rt_render_adaptive / rt_dispatch_tile.  Replaces the reference's dispatch loop (src/compute.rs:137-251).
#include "rt_internal.h"

#ifndef RT_SINGLE_PASS_MAX_NODES
#define RT_SINGLE_PASS_MAX_NODES 64u /* "BVH depth <= 4" scenes of BASELINE configs[1]; larger scenes: measured in profiles/ab_r03.json */
#endif
#ifndef RT_WF_LANES_DEFAULT
#define RT_WF_LANES_DEFAULT 2 /* measured on the headline frame: 179.7 - 188.1 ms against 197.6 - 199.0 with one lane; 16 spp: 48.8 against 51.9 */
#endif

namespace rti {
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
    s.nodes = d.scene.nodes.get();
    s.tris = d.scene.tris.get();
    s.spheres = d.scene.spheres.get();
    s.lights = d.scene.lights.get();
    s.materials = d.scene.materials.get();
    return s;
}

// The tiles device j (of nd) takes of a frame: the context owns the tiles i with i % world == rank (rt_hip.h); its device j takes every
// nd-th of those.
void frame_share(DevFrame& f, uint32_t world, uint32_t rank, size_t nd, size_t j) {
    const uint32_t total_tiles = f.tiles_x * f.tiles_y, stride = world * (uint32_t)nd, first = rank + world * (uint32_t)j;
    f.tile_first = first;
    f.tile_stride = stride;
    f.n_owned_tiles = first < total_tiles ? (total_tiles - first + stride - 1) / stride : 0;
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

namespace {

int ensure_targets(rt_ctx* ctx, DeviceState& d, uint32_t w, uint32_t h) {
    if (d.fb.w == w && d.fb.h == h && d.fb.rgba32f.get()) return RT_OK;
    if (d.stream) HIPCHK(ctx, hipStreamSynchronize(d.stream)); // dispatches in flight may still write the old targets
    HIPCHK(ctx, hipSetDevice(d.device));
    d.fb = {}; // (the read-back staging goes with the targets it was sized for)
    size_t n = (size_t)w * h;
    HIPCHK(ctx, d.fb.rgba32f.reserve(n * 16));
    for (int c = 0; c < 3; c++) HIPCHK(ctx, d.fb.chan[c].reserve(n * 4));
    HIPCHK(ctx, d.fb.prim_id.reserve(n * 4));
    HIPCHK(ctx, d.fb.hit_t.reserve(n * 4));
    // fresh textures read as zero, like newly created wgpu textures.  On d.stream: it is a non-blocking stream, so a
    // memset on the null stream would not be ordered against the kernels that write these targets next
    HIPCHK(ctx, hipMemsetAsync(d.fb.rgba32f.get(), 0, n * 16, d.stream));
    for (int c = 0; c < 3; c++) HIPCHK(ctx, hipMemsetAsync(d.fb.chan[c].get(), 0, n * 4, d.stream));
    HIPCHK(ctx, hipMemsetAsync(d.fb.prim_id.get(), 0xFF, n * 4, d.stream));
    HIPCHK(ctx, hipMemsetAsync(d.fb.hit_t.get(), 0, n * 4, d.stream));
    d.fb.w = w;
    d.fb.h = h;
    return RT_OK;
}

DevTargets targets_for(const DeviceState& d, const DevFrame& f) {
    DevTargets t;
    t.rgba32f = d.fb.rgba32f.get();
    for (int c = 0; c < 3; c++) t.chan[c] = d.fb.chan[c].get();
    t.prim_id = d.fb.prim_id.get();
    t.hit_t = d.fb.hit_t.get();
    t.counters = d.counters.get();
    t.run_sum = (f.flags & RT_FLAG_ACCUMULATE) ? d.acc.run_sum.get() : nullptr;
    t.run_odd = f.adaptive ? d.acc.run_odd.get() : nullptr;
    return t;
}

// The running sums of an accumulating frame of width x height, one per device (its share of the pixels is written, the rest never read);
// an adaptive one (rt_render_adaptive) also has the odd-sample sums and the selection buffers for every block of the frame's tiling.
int ensure_run_sums(rt_ctx* ctx, const DevFrame& fr) {
    const uint32_t w = fr.width, h = fr.height;
    for (auto& d : ctx->devs) {
        HIPCHK(ctx, hipSetDevice(d.device));
        if (!(d.acc.run_sum.get() && d.acc.w == w && d.acc.h == h)) {
            if (d.stream) HIPCHK(ctx, hipStreamSynchronize(d.stream));
            d.acc = {};
            HIPCHK(ctx, d.acc.run_sum.reserve((size_t)w * h * 16)); // not cleared: a first call (sample_base 0) reads none of it
            d.acc.w = w;
            d.acc.h = h;
        }
        if (!fr.adaptive) continue;
        HIPCHK(ctx, d.acc.run_odd.reserve((size_t)w * h * 16)); // (as run_sum: read only once written)
        const uint64_t all_blocks = (uint64_t)fr.tiles_x * fr.tiles_y * rt::blocks_per_tile(fr.tile_size); // a device owns at most all of them
        if (all_blocks > 0xFFFFFFFFull) return ctx->fail(RT_ERR_BAD_ARG, "rt_render_adaptive: %llu pixel blocks exceed 32-bit block indices", (unsigned long long)all_blocks);
        const uint32_t blocks = (uint32_t)all_blocks;
        if (d.ad.cap < blocks || !d.ad.counts.get()) {
            if (d.stream) HIPCHK(ctx, hipStreamSynchronize(d.stream));
            d.ad = {};
            HIPCHK(ctx, d.ad.mask.reserve((size_t)std::max(1u, blocks) * 8));
            HIPCHK(ctx, d.ad.blocks.reserve((size_t)std::max(1u, blocks) * 4));
            HIPCHK(ctx, d.ad.counts.reserve(2 * 8));
            d.ad.cap = blocks;
        }
    }
    return RT_OK;
}

// Path-state arrays and queues of the wavefront pipeline, sized for `batch` samples per owned pixel block.
// `shrink`: an adaptive call (rt_render_adaptive), whose live blocks change from call to call, also runs in an allocation made for more
// blocks; it leaves the allocation's shape as it was (its lanes say how many blocks it covers, lane_of), so frames of that shape keep it.
int ensure_wavefront(rt_ctx* ctx, DeviceState& d, uint32_t n_blocks, uint32_t batch, uint32_t n_lights, bool two_lanes, bool shrink = false) {
    const uint32_t capacity = n_blocks * batch * 64u;
    // overflow entries (64-bit) per lane beyond the LDS part of the stack
    const uint32_t ovf_entries = ctx->scene_counts.stack_entries + 2u > RT_WF8_LDS_STACK ? ctx->scene_counts.stack_entries + 2u - RT_WF8_LDS_STACK : 1u;
    const bool same_shape = shrink ? d.pipe.wf.n_blocks >= n_blocks : (d.pipe.wf.n_blocks == n_blocks && d.pipe.wf.batch == batch);
    if (d.pipe.wf.capacity >= capacity && same_shape && d.pipe.lights >= n_lights && d.pipe.wf.counters &&
        d.pipe.wf.ovf_entries >= ovf_entries && d.pipe.wf.stack_ovf && (!two_lanes || (d.pipe.wf2.counters && d.pipe.wf2.capacity >= capacity && d.pipe.wf2.stack_ovf)))
        return RT_OK;
    HIPCHK(ctx, hipSetDevice(d.device));
    d.pipe = {}; // the old lanes go before the new ones are made
    // the lanes are built here and handed to the device when complete: an allocation that fails half way must not leave a lane that
    // looks complete to the reuse test above
    DeviceState::Lanes fresh;
    for (int lane = 0; lane < (two_lanes ? 2 : 1); lane++) {
    std::vector<DevMem>& owned = lane ? fresh.allocs2 : fresh.allocs;
    auto alloc = [&](void** p, size_t bytes) -> hipError_t {
        owned.emplace_back();
        const hipError_t e = owned.back().reserve(bytes ? bytes : 16);
        *p = owned.back().get();
        return e;
    };
    rt::WfBuffers& w = lane ? fresh.wf2 : fresh.wf;
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
    else w.accum = fresh.wf.accum; // one running sum per pixel: the lanes' resolves are ordered by events
    if (lane == 0) { // the camera beams of the frame: per block a leaf list, built once per frame and read by both lanes
        HIPCHK(ctx, alloc((void**)&w.beam_count, ((size_t)std::max(1u, n_blocks) + 1) * 4));
        HIPCHK(ctx, alloc((void**)&w.beam_ref, (size_t)std::max(1u, n_blocks) * RT_BEAM_CAP * 4));
        HIPCHK(ctx, alloc((void**)&w.beam_dist, (size_t)std::max(1u, n_blocks) * RT_BEAM_CAP * 4));
    } else {
        w.beam_count = fresh.wf.beam_count;
        w.beam_ref = fresh.wf.beam_ref;
        w.beam_dist = fresh.wf.beam_dist;
    }
    HIPCHK(ctx, alloc((void**)&w.stack_ovf, (size_t)rt::wf_persistent_waves() * ovf_entries * 64 * 8));
    w.ovf_entries = ovf_entries;
    w.n_blocks = n_blocks;
    w.batch = batch;
    w.capacity = capacity;
    }
    fresh.lights = n_lights;
    d.pipe = std::move(fresh);
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
    // path state indexed by id (two sets of ray_o / ray_d / thr / rad, vtx: 160 bytes per record, wf_state_slots records = under 2 per path
    // slot for batches large enough that memory bounds them), sample_rad, pxy, two extension queues, shadow queue (4 slots per entry), the
    // handed-on shadow queue (dense)
    const uint64_t bytes_per_path = 2 * 10 * 16 + 16 + 4 + 2 * 16 + 16 * lights + 4 * lights;
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
    const uint32_t n_blocks = f.adaptive ? d.ad.live_blocks : f.n_owned_tiles * rt::blocks_per_tile(f.tile_size);
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    const char* lanes_env = std::getenv("RT_WF_LANES"); // (read per frame: tests and A/B runs switch it)
    // by default only for frames whose shadow stage runs on light grids: with the BVH walk both big stages are VALU-bound and sharing
    // the chip gains nothing (bistro-like 4K share: 136.7 ms on two lanes against 127.3 on one)
    bool two_lanes_on = lanes_env ? std::atoi(lanes_env) >= 2 : (RT_WF_LANES_DEFAULT >= 2 && d.grids.table.get() != nullptr && !(f.flags & RT_FLAG_NO_SHADOW_GRID));
    // ... and not for a frame of long paths that fits ONE batch: two lanes would cut it in two, every launch would come twice, and
    // beyond four bounces most launches serve few paths and cost their latency whatever they serve (bistro-like 4K share, 64 spp,
    // 8 bounces, 66 M paths: one batch on one lane 105.3 ms, two of 32 samples on two lanes 116.7; 4 bounces: the two lanes win)
    if (!lanes_env && two_lanes_on && f.max_bounce > 4 && wavefront_batch(n_blocks, f.spp, n_lights, free_b, false) >= f.spp) two_lanes_on = false;
    const uint32_t batch = d.pipe.wf.n_blocks == n_blocks && d.wf_spp == f.spp && d.pipe.wf.batch && d.pipe.lights >= n_lights && d.used_two_lanes == (two_lanes_on && f.spp >= 2) ? d.pipe.wf.batch // same frame shape as last time: keep the allocation
                                                                                               : wavefront_batch(n_blocks, f.spp, n_lights, two_lanes_on ? free_b / 2 : free_b, two_lanes_on);
    d.wf_spp = f.spp;
    // Two lanes (RT_WF_LANES=2, the default when a frame has two or more batches): batches alternate between two streams with their own
    // path state, so that one batch's shadow stage (bound by HBM bandwidth since the light grids) runs beside the other's closest-hit
    // traversal (bound by VALU issue).  The pixel sums are added in batch order: a resolve waits for the previous batch's.
    const uint32_t n_batches = (f.spp + batch - 1) / batch;
    const bool two = two_lanes_on && n_batches >= 2 && d.stream2;
    if (int rc = ensure_wavefront(ctx, d, n_blocks, batch, n_lights, two, f.adaptive != 0)) return rc;
    HIPCHK(ctx, hipMemsetAsync(d.pipe.wf.totals, 0, rt::WF_N_TOTALS * sizeof(unsigned long long), d.stream));
    if (!f.adaptive) HIPCHK(ctx, hipEventRecord(d.ev0, d.stream)); // re-record: allocation above is not part of the kernel time (an adaptive call's selection is)
    // camera beams: on by default, RT_WF_BEAMS=0 (development knob) or RT_FLAG_NO_BEAMS walks the tree for every camera segment
    const char* be = std::getenv("RT_WF_BEAMS");
    const bool beams = !(f.flags & RT_FLAG_NO_BEAMS) && (be ? std::atoi(be) != 0 : true);
    if (beams) {
        rt::WfBuffers wb = d.pipe.wf;
        wb.n_blocks = n_blocks; // (an adaptive call may run in an allocation made for more blocks)
        wb.batch = batch;
        HIPCHK(ctx, rt::wf_beams(scene_for(ctx, d), f, wb, d.stream));
    }
    if (two) {
        HIPCHK(ctx, hipEventRecord(d.ev_start, d.stream));
        HIPCHK(ctx, hipStreamWaitEvent(d.stream2, d.ev_start, 0));
        HIPCHK(ctx, hipMemsetAsync(d.pipe.wf2.totals, 0, rt::WF_N_TOTALS * sizeof(unsigned long long), d.stream2));
    }
    d.pipe.wf.grids = d.pipe.wf2.grids = (f.flags & RT_FLAG_NO_SHADOW_GRID) ? nullptr : d.grids.table.get();
    const char* pe = std::getenv("RT_WF_PROBE");
    d.pipe.wf.probe = d.pipe.wf2.probe = pe ? (uint32_t)std::atoi(pe) : 0u;
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
    WfLane l{second ? d.pipe.wf2 : d.pipe.wf, second ? d.stream2 : d.stream};
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
    HIPCHK(ctx, rt::wf_bounce(r.dsc, r.f, l.w, r.it, batch_samples(r), r.first, counters, l.st, gev));
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
        HIPCHK(ctx, hipMemcpy(w, d.pipe.wf.totals, sizeof w, hipMemcpyDeviceToHost));
        if (r.two) {
            unsigned long long w2[rt::WF_N_TOTALS];
            HIPCHK(ctx, hipMemcpy(w2, d.pipe.wf2.totals, sizeof w2, hipMemcpyDeviceToHost));
            merge_lanes(w, w2);
        }
        if (int rc = add_totals(ctx, t, w)) return rc;
    } else if (counters || fr.mode == RT_MODE_EXTENDED) {
        unsigned long long c[RT_CNT_SLOTS];
        HIPCHK(ctx, hipMemcpy(c, d.counters.get(), sizeof c, hipMemcpyDeviceToHost));
        add_counters(t, c);
    }
    t.pixels += fr.adaptive ? d.ad.pixels : share_pixels(fr, d); // (an adaptive call: the pixels that received samples)
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
        HIPCHK(ctx, hipMemsetAsync(d.counters.get(), 0, RT_CNT_SLOTS * sizeof(unsigned long long), d.stream));
        HIPCHK(ctx, hipEventRecord(d.ev0, d.stream));
        if (f.adaptive) { // rt_render_adaptive: which pixels take samples, read back once per call and device to size what follows
            f.ad_mask = d.ad.mask.get();
            f.ad_blocks = d.ad.blocks.get();
            unsigned long long counts[2] = {0, 0};
            HIPCHK(ctx, rt::launch_ad_select(f, targets_for(d, f), d.ad.mask.get(), d.ad.blocks.get(), d.ad.counts.get(), d.stream));
            HIPCHK(ctx, hipMemcpyAsync(counts, d.ad.counts.get(), sizeof counts, hipMemcpyDeviceToHost, d.stream));
            HIPCHK(ctx, hipStreamSynchronize(d.stream));
            d.ad.live_blocks = (uint32_t)counts[0];
            d.ad.pixels = counts[1];
            if (d.ad.live_blocks == 0) { // every pixel of the share has stopped: nothing to trace
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

} // namespace rti

using namespace rti;

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

} // extern "C"
