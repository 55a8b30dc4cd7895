// kernels.hip — gfx950 kernels of the ray-casting hot path.
//
// Replaces the reference's rust-gpu kernel `main_cs` (shader/src/lib.rs:25-89) and
// everything it calls (ray.rs, bvh.rs, intersection.rs, lighting.rs, material.rs,
// wavefront.rs).  One wavefront (64 lanes) = one 8x8 pixel block; each lane owns a
// pixel.  All three colour channels are produced in ONE pass: the trace and the
// lighting are channel independent, only the transmission term of
// shader/src/lib.rs:323-337 depends on the channel, so the reference's three
// dispatches per tile (src/compute.rs:184-190) collapse into one.
//
// Arithmetic that decides WHICH primitive is hit (ray generation, Möller–Trumbore,
// sphere quadratic) and the shading keep the reference's f32 operation order; the file
// is compiled with -ffp-contract=off so nothing is fused implicitly.  The boxes of the
// 8-wide tree are a conservative filter (device_common.h); culling by the closest hit.
//
// The two extended-mode megakernels here own their control flow only (nested loops; a per-lane
// state machine).  What a path vertex does - sample ray, light sum, leaving the vertex, scatter,
// roulette - is stated once in device_common.h (ext_*), which the queue pipeline calls too.
#include "kernels.h"

#include <algorithm>

#include "../../include/rt_hip.h"
#include "device_common.h"

using namespace rtdev;

namespace {

// ------------------------------------------------------------------------------------
// k_render_reference: modes 0 and 1 (reference semantics): one pixel-centre ray per pixel,
// closest hit, direct lighting; miss = black (mode 0, lib.rs:77) or sky (mode 1,
// wavefront.rs:146-151).  Mode 1 only produces colour when current_bounce <= max_bounce
// (lib.rs:117-121), otherwise (0,0,0).
// ------------------------------------------------------------------------------------
template <bool COUNT>
__global__ __launch_bounds__(WAVE) void k_render_reference(DevScene sc, DevFrame fr, DevTargets tg) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries: one entry per visit
    PixelCoord px = block_pixel(fr);
    if (!px.valid) return;
    uint2* stack = s_stack + threadIdx.x;
    Counts cnt = {0u, 0u};
    const bool wavefront = fr.mode != 0;
    V3 color = v3(0.0f, 0.0f, 0.0f);
    Hit hit;
    hit.t = RT_F32_MAX;
    hit.prim = RT_PRIM_MISS;
    hit.slot = 0;
    const bool traced = !wavefront || fr.cur_bounce <= fr.max_bounce;
    if (traced) {
        V3 o, d;
        camera_ray(fr.cam, (float)px.x + 0.5f, (float)px.y + 0.5f, wavefront, o, d);
        hit = find_closest<COUNT>(sc, o, d, stack, cnt);
        if (hit.prim != RT_PRIM_MISS) color = shade_hit(sc, hit, o, d);
        else if (wavefront) color = RT_SKY();
    }
    const size_t pix = (size_t)px.y * fr.width + px.x;
    if (tg.rgba32f) reinterpret_cast<float4*>(tg.rgba32f)[pix] = make_float4(color.x, color.y, color.z, 1.0f);
    if (tg.prim_id) tg.prim_id[pix] = hit.prim;
    if (tg.hit_t) tg.hit_t[pix] = hit.t;
    // channel texture c keeps only component c (filter_color_by_channel) and alpha 1
    if ((fr.channel_mask & 1u) && tg.chan[0]) reinterpret_cast<uint32_t*>(tg.chan[0])[pix] = unorm8(color.x) | 0xFF000000u;
    if ((fr.channel_mask & 2u) && tg.chan[1]) reinterpret_cast<uint32_t*>(tg.chan[1])[pix] = (unorm8(color.y) << 8) | 0xFF000000u;
    if ((fr.channel_mask & 4u) && tg.chan[2]) reinterpret_cast<uint32_t*>(tg.chan[2])[pix] = (unorm8(color.z) << 16) | 0xFF000000u;
    if (COUNT && tg.counters) {
        atomicAdd(&tg.counters[RT_CNT_SEGMENTS], traced ? 1ull : 0ull);
        atomicAdd(&tg.counters[RT_CNT_NODE_VISITS], (unsigned long long)cnt.nodes);
        atomicAdd(&tg.counters[RT_CNT_TRI_TESTS], (unsigned long long)cnt.tris);
        atomicAdd(&tg.counters[RT_CNT_CAMERA], traced ? 1ull : 0ull);
    }
}


// The nested loops' light sum: a light that needs a shadow segment gets it traced on the spot.
template <bool COUNT>
__device__ __forceinline__ V3 ext_direct(const DevScene& sc, const DevMaterial& m, V3 point, V3 normal, bool terminal, bool shadows,
                                         uint2* stack, Counts& cnt, SegCounts& seg) {
    return ext_light_sum(sc.lights, sc.n_lights, m, point, normal, terminal, shadows, [&](uint32_t, V3 sdir, float sdist) {
        seg.shadow++;
        return !occluded<COUNT>(sc, point + normal * EXT_EPS, sdir, RT_MIN_RAY_DISTANCE, sdist, stack, cnt);
    });
}

template <bool COUNT>
__device__ __forceinline__ V3 ext_trace_path(const DevScene& sc, const DevFrame& fr, uint32_t px, uint32_t py, uint32_t sample,
                                             uint2* stack, Counts& cnt, SegCounts& seg) {
    V3 o, d;
    SimpleRng rng = ext_sample_ray(fr.cam, fr.width, fr.frame_seed, fr.jitter, px, py, sample, true, o, d);
    V3 radiance = v3(0.0f, 0.0f, 0.0f);
    V3 throughput = v3(1.0f, 1.0f, 1.0f);
    uint32_t channel = 3;
    const bool shadows = (fr.flags & RT_FLAG_NO_SHADOWS) == 0;
    for (uint32_t depth = 0;; depth++) {
        if (depth == 0) seg.camera++; else seg.continuation++;
        Hit hit = find_closest<COUNT>(sc, o, d, stack, cnt);
        if (hit.prim == RT_PRIM_MISS) {
            radiance = radiance + RT_SKY() * throughput;
            break;
        }
        V3 point, normal;
        uint32_t material_id;
        hit_geometry(sc, hit, o, d, point, normal, material_id);
        if (material_id >= sc.n_materials) {
            radiance = radiance + RT_MAGENTA() * throughput;
            break;
        }
        const DevMaterial m = sc.materials[material_id];
        const bool terminal = depth >= fr.max_bounce;
        const V3 lighting = ext_direct<COUNT>(sc, m, point, normal, terminal, shadows, stack, cnt, seg);
        const float tf = ext_leave_vertex(m, lighting, terminal, throughput, radiance);
        if (terminal) break;
        V3 norigin, ndir;
        if (!ext_scatter(m, point, normal, d, tf, depth, rng, channel, throughput, norigin, ndir)) break;
        o = norigin;
        d = ndir;
    }
    return radiance;
}

// AD: the adaptive variant (rt_render_adaptive): a lane whose pixel k_ad_select left out behaves like a pixel outside the image; the
// others trace their own samples n .. n+spp-1 and add them to S (and the odd-indexed ones to H); k_ad_image writes the targets.
template <bool COUNT, bool AD>
__global__ __launch_bounds__(WAVE) void k_render_extended(DevScene sc, DevFrame fr, DevTargets tg) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries: one entry per visit
    PixelCoord px = block_pixel(fr);
    if (AD) px.valid = px.valid && ad_lane_active(fr, blockIdx.x, threadIdx.x);
    uint2* stack = s_stack + threadIdx.x;
    Counts cnt = {0u, 0u};
    SegCounts seg = {0u, 0u, 0u};
    if (px.valid && AD) {
        const size_t pix = (size_t)px.y * fr.width + px.x;
        AdPixel a = ad_load(fr, tg, pix);
        for (uint32_t s = 0; s < fr.spp; s++) {
            const uint32_t g = a.n + s;
            const V3 x = ext_trace_path<COUNT>(sc, fr, px.x, px.y, g, stack, cnt, seg);
            a.s = a.s + x;
            if (g & 1u) a.h = a.h + x;
        }
        ad_keep(tg, pix, a.s, a.h, a.n + fr.spp);
    } else if (px.valid) {
        const size_t pix = (size_t)px.y * fr.width + px.x;
        V3 sum = run_sum_start(fr, tg, pix);
        for (uint32_t s = 0; s < fr.spp; s++) sum = sum + ext_trace_path<COUNT>(sc, fr, px.x, px.y, fr.sample_base + s, stack, cnt, seg);
        run_sum_keep(tg, pix, sum);
        store_image(tg, pix, sum, (float)fr.n_total);
    }
    flush_segment_counts<COUNT>(tg, seg, cnt);
}


// ====================================================================================
// k_render_extended_sm — extended mode as a per-lane STATE MACHINE (v2).
//
// v1 (k_render_extended) nests the loops samples -> path vertices -> lights -> traversal, so a
// wave runs every traversal in lockstep and lanes whose segment ends early idle until the
// slowest lane is done (measured: ~17 % lane utilisation, profiles/r01_extended_*_v1).  Here
// every lane carries its own path state and the wave alternates between two phases:
//   traversal phase  - one BVH step at a time for every lane that has a segment in flight
//                      (closest-hit and any-hit shadow segments mixed); a lane whose segment
//                      finishes parks;
//   transition phase - entered when no lane is traversing or RT_SM_PARK_THRESHOLD lanes are
//                      parked (__ballot + popcount): parked lanes consume their result (shade,
//                      next light, next bounce, next sample) and set up their next segment.
// Per-lane arithmetic and its order are exactly those of v1 / the CPU statement; only the
// interleaving across lanes changes, so results stay bit-identical.
// ====================================================================================
#ifndef RT_SM_MIN_WAVES
#define RT_SM_MIN_WAVES 4
#endif
#ifndef RT_SM_PARK_THRESHOLD
#define RT_SM_PARK_THRESHOLD 8
#endif

enum : uint32_t { ST_NEW_SAMPLE = 0, ST_CLOSEST_DONE = 1, ST_SHADOW_DONE = 2, ST_LIGHTS = 3, ST_TRAVERSING = 4, ST_DONE = 5 };

template <bool COUNT, bool AD> // AD: the adaptive variant, as k_render_extended's
__global__ __launch_bounds__(WAVE, RT_SM_MIN_WAVES) void k_render_extended_sm(DevScene sc, DevFrame fr, DevTargets tg) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries: one entry per visit
    PixelCoord px = block_pixel(fr);
    if (AD) px.valid = px.valid && ad_lane_active(fr, blockIdx.x, threadIdx.x);
    uint2* __restrict__ stack = s_stack + threadIdx.x;
    const uint4* __restrict__ nodes = reinterpret_cast<const uint4*>(sc.nodes);
    Counts cnt = {0u, 0u};
    SegCounts seg = {0u, 0u, 0u};
    const bool shadows = (fr.flags & RT_FLAG_NO_SHADOWS) == 0;

    // ---- per-lane path state ----
    uint32_t state = px.valid ? ST_NEW_SAMPLE : ST_DONE;
    uint32_t sample = 0, depth = 0, channel = 3, li = 0, material_id = 0;
    SimpleRng rng = {0u};
    V3 sum = v3(0.0f, 0.0f, 0.0f), radiance = sum, throughput = sum, lighting = sum, pending = sum;
    V3 point = sum, normal = sum, din = sum; // vertex position, geometric normal, incoming direction
    bool terminal = false;
    // ---- per-lane segment (traversal) state ----
    V3 o = sum, d = sum;
    FilterRay fray;
    fray.o = sum;
    fray.inv = sum;
    Hit hit;
    hit.t = RT_F32_MAX;
    hit.prim = RT_PRIM_MISS;
    hit.slot = 0;
    uint32_t g_base = 0, g_bits = 0; // inner children still to visit: (child_base, hits | imask << 8)
    uint32_t t_base = 0, t_bits = 0; // leaves of the last visited node still to test: (tri_base, hits | lmask << 8)
    uint32_t oct = 0;
    int sp = 0;
    bool anyhit = false;
    if (px.valid) sum = run_sum_start(fr, tg, (size_t)px.y * fr.width + px.x); // the samples earlier calls of an accumulation left
    V3 odd = v3(0.0f, 0.0f, 0.0f);
    uint32_t base = fr.sample_base; // the pixel's first global sample of this launch
    if (AD && px.valid) {
        const AdPixel a = ad_load(fr, tg, (size_t)px.y * fr.width + px.x);
        sum = a.s;
        odd = a.h;
        base = a.n;
    }

    // start a segment: spheres are tested right away (wave-uniform loop), the BVH walk is deferred to the traversal phase
    auto begin_segment = [&](V3 so, V3 sd, float tmax, bool any) {
        o = so;
        d = sd;
        fray = make_filter_ray(so, sd);
        hit.t = tmax;
        hit.prim = RT_PRIM_MISS;
        hit.slot = 0;
        anyhit = any;
        oct = ray_octant(fray);
        test_spheres(sc, so, sd, hit, RT_MIN_RAY_DISTANCE);
        sp = 0;
        g_base = 0;
        g_bits = 1u | (1u << 8); // the root as the only child of a group
        t_bits = 0;
        const bool finished = sc.n_nodes == 0 || (any && hit.prim != RT_PRIM_MISS);
        state = finished ? (any ? ST_SHADOW_DONE : ST_CLOSEST_DONE) : ST_TRAVERSING;
    };

    // diagnostics of the counting variant (wave-level, lane 0 accumulates): counters[RT_CNT_SM_*] (device_layout.h)
    unsigned long long dg_tp = 0, dg_tl = 0, dg_ni = 0, dg_nl = 0, dg_li = 0, dg_ll = 0, dg_ct = 0, dg_cv = 0;
    for (;;) {
        // =========================== transition phase ===========================
        unsigned long long t_begin = 0;
        if (COUNT) {
            unsigned long long need = __ballot(state != ST_TRAVERSING && state != ST_DONE);
            if (need) {
                dg_tp++;
                dg_tl += __popcll(need);
            }
            t_begin = __builtin_readcyclecounter();
        }
        while (state != ST_TRAVERSING && state != ST_DONE) {
            if (state == ST_NEW_SAMPLE) {
                if (sample >= fr.spp) {
                    const size_t pix = (size_t)px.y * fr.width + px.x;
                    if (AD) {
                        ad_keep(tg, pix, sum, odd, base + fr.spp);
                    } else {
                        run_sum_keep(tg, pix, sum);
                        store_image(tg, pix, sum, (float)fr.n_total);
                    }
                    state = ST_DONE;
                    break;
                }
                V3 co, cd;
                rng = ext_sample_ray(fr.cam, fr.width, fr.frame_seed, fr.jitter, px.x, px.y, (AD ? base : fr.sample_base) + sample, true, co, cd);
                radiance = v3(0.0f, 0.0f, 0.0f);
                throughput = v3(1.0f, 1.0f, 1.0f);
                channel = 3;
                depth = 0;
                seg.camera++;
                begin_segment(co, cd, RT_F32_MAX, false);
                continue;
            }
            bool end_sample = false;
            if (state == ST_CLOSEST_DONE) {
                if (hit.prim == RT_PRIM_MISS) {
                    radiance = radiance + RT_SKY() * throughput;
                    end_sample = true;
                } else {
                    hit_geometry(sc, hit, o, d, point, normal, material_id);
                    din = d;
                    if (material_id >= sc.n_materials) {
                        radiance = radiance + RT_MAGENTA() * throughput;
                        end_sample = true;
                    } else {
                        terminal = depth >= fr.max_bounce;
                        lighting = light_sum_begin(sc.materials[material_id], terminal);
                        li = 0;
                        state = ST_LIGHTS;
                    }
                }
            } else if (state == ST_SHADOW_DONE) {
                if (hit.prim == RT_PRIM_MISS) lighting = lighting + pending;
                li++;
                state = ST_LIGHTS;
            }
            if (!end_sample && state == ST_LIGHTS) {
                const DevMaterial m = sc.materials[material_id];
                bool launched = false;
                while (li < sc.n_lights) {
                    V3 sdir;
                    float sdist;
                    V3 contrib = light_contribution(sc.lights[li], m, point, normal, sdir, sdist);
                    if (needs_shadow_segment(contrib) && shadows) {
                        pending = contrib;
                        seg.shadow++;
                        launched = true;
                        begin_segment(point + normal * EXT_EPS, sdir, sdist, true); // overwrites o/d: the incoming direction lives in `din`
                        break;
                    }
                    lighting = lighting + contrib;
                    li++;
                }
                if (launched) continue;
                // ---- all lights done: finish the vertex ----
                lighting = light_sum_end(lighting, m);
                const float tf = ext_leave_vertex(m, lighting, terminal, throughput, radiance);
                V3 norigin, ndir;
                if (terminal || !ext_scatter(m, point, normal, din, tf, depth, rng, channel, throughput, norigin, ndir)) {
                    end_sample = true;
                } else {
                    depth++;
                    seg.continuation++;
                    begin_segment(norigin, ndir, RT_F32_MAX, false);
                }
            }
            if (end_sample) {
                sum = sum + radiance;
                if (AD && ((base + sample) & 1u)) odd = odd + radiance;
                sample++;
                state = ST_NEW_SAMPLE;
            }
        }
        if (COUNT) {
            unsigned long long t_mid = __builtin_readcyclecounter();
            dg_ct += t_mid - t_begin;
            t_begin = t_mid;
        }
        // =========================== anything left? ===========================
        if (__ballot(state == ST_TRAVERSING) == 0ull) {
            if (__ballot(state != ST_DONE) == 0ull) break;
            continue;
        }
        // =========================== traversal phase ===========================
        // while-while on groups: every lane that has an inner child to visit (and no leaves waiting) steps until none has,
        // then the lanes whose last visit entered leaves test them.  (A speculative variant that postponed one leaf per lane
        // and kept descending raised lane utilisation of the node steps from 26 % to 48 % in round 1 but was not faster here;
        // the queue pipeline's persistent kernels do postpone, wavefront.hip.)
        for (;;) {
            for (;;) {
                const bool trav = state == ST_TRAVERSING;
                if (trav && (t_bits & 0xFFu) == 0u && (g_bits & 0xFFu) == 0u && sp > 0) {
                    sp--;
                    const uint2 e = stack[sp * WAVE];
                    g_base = e.x;
                    g_bits = e.y;
                }
                const bool want = trav && (t_bits & 0xFFu) == 0u && (g_bits & 0xFFu) != 0u;
                const unsigned long long wmask = __ballot(want);
                if (wmask == 0ull) break;
                if (COUNT) {
                    dg_ni++;
                    dg_nl += __popcll(wmask);
                }
                if (want) {
                    const uint32_t i = first_slot(g_bits, oct);
                    g_bits ^= 1u << i;
                    const uint32_t node = g_base + (uint32_t)__popc(__builtin_amdgcn_ubfe(g_bits, 8u, i));
                    if (g_bits & 0xFFu) {
                        stack[sp * WAVE] = make_uint2(g_base, g_bits);
                        sp++;
                    }
                    uint32_t cb, tb, im, lm;
                    const uint32_t hm = visit_node8<COUNT>(nodes, node, fray, hit.t, cnt, cb, tb, im, lm);
                    g_base = cb;
                    g_bits = (hm & im) | (im << 8);
                    t_base = tb;
                    t_bits = (hm & lm) | (lm << 8);
                }
            }
            if (COUNT) {
                unsigned long long lm_ = __ballot(state == ST_TRAVERSING && (t_bits & 0xFFu) != 0u);
                if (lm_) {
                    dg_li++;
                    dg_ll += __popcll(lm_);
                }
            }
            if (state == ST_TRAVERSING) {
                // `anyhit` differs between lanes, so one loop serves both kinds (any-hit lanes leave it at their first hit)
                bool stop = false;
                while ((t_bits & 0xFFu) != 0u && !stop) {
                    const uint32_t sl = first_slot(t_bits, oct);
                    t_bits ^= 1u << sl;
                    const uint32_t start = t_base + RT_DEV_LEAF_STRIDE * (uint32_t)__popc(__builtin_amdgcn_ubfe(t_bits, 8u, sl));
                    uint32_t n_tri = 1;
                    for (uint32_t i = 0; i < n_tri; i++) {
                        if (COUNT) cnt.tris++;
                        const uint32_t lc = test_triangle(sc.tris, start + i, o, d, hit, RT_MIN_RAY_DISTANCE);
                        if (i == 0) n_tri = lc;
                        if (anyhit && hit.prim != RT_PRIM_MISS) {
                            stop = true;
                            break;
                        }
                    }
                }
                if (stop) state = ST_SHADOW_DONE;
                else if ((g_bits & 0xFFu) == 0u && sp == 0) state = anyhit ? ST_SHADOW_DONE : ST_CLOSEST_DONE;
            }
            const unsigned long long still = __ballot(state == ST_TRAVERSING);
            const unsigned long long parked = __ballot(state != ST_TRAVERSING && state != ST_DONE);
            if (still == 0ull || __popcll(parked) >= RT_SM_PARK_THRESHOLD) break;
        }
        if (COUNT) dg_cv += __builtin_readcyclecounter() - t_begin;
    }
    flush_segment_counts<COUNT>(tg, seg, cnt);
    if (COUNT && threadIdx.x == 0 && tg.counters) {
        atomicAdd(&tg.counters[RT_CNT_SM_TRANSITION_PASSES], dg_tp);
        atomicAdd(&tg.counters[RT_CNT_SM_TRANSITION_LANES], dg_tl);
        atomicAdd(&tg.counters[RT_CNT_SM_NODE_ITERS], dg_ni);
        atomicAdd(&tg.counters[RT_CNT_SM_NODE_LANES], dg_nl);
        atomicAdd(&tg.counters[RT_CNT_SM_LEAF_ITERS], dg_li);
        atomicAdd(&tg.counters[RT_CNT_SM_LEAF_LANES], dg_ll);
        atomicAdd(&tg.counters[RT_CNT_SM_CYCLES_TRANSITION], dg_ct);
        atomicAdd(&tg.counters[RT_CNT_SM_CYCLES_TRAVERSAL], dg_cv);
    }
}

} // namespace

namespace rt {

__global__ __launch_bounds__(256) void k_combine_rgba8(const uint32_t* __restrict__ red, const uint32_t* __restrict__ green, const uint32_t* __restrict__ blue,
                                                        uint32_t* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = (red[i] & 0x000000FFu) | (green[i] & 0x0000FF00u) | (blue[i] & 0x00FF0000u) | 0xFF000000u;
}
__global__ __launch_bounds__(256) void k_pack_rgb32f(const float4* __restrict__ rgba, float* __restrict__ rgb, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = rgba[i];
        rgb[3 * i + 0] = v.x;
        rgb[3 * i + 1] = v.y;
        rgb[3 * i + 2] = v.z;
    }
}

uint32_t blocks_per_tile(uint32_t tile_size) {
    uint32_t b = (tile_size + 7u) >> 3;
    return b * b;
}

hipError_t launch_combine_rgba8(const uint8_t* red, const uint8_t* green, const uint8_t* blue, uint8_t* out, size_t n_pixels, hipStream_t stream) {
    if (n_pixels == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n_pixels + 255) / 256, 4096);
    hipLaunchKernelGGL(k_combine_rgba8, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const uint32_t*>(red), reinterpret_cast<const uint32_t*>(green),
                       reinterpret_cast<const uint32_t*>(blue), reinterpret_cast<uint32_t*>(out), n_pixels);
    return hipGetLastError();
}
hipError_t launch_pack_rgb32f(const float* rgba, float* rgb, size_t n_pixels, hipStream_t stream) {
    if (n_pixels == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n_pixels + 255) / 256, 4096);
    hipLaunchKernelGGL(k_pack_rgb32f, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float4*>(rgba), rgb, n_pixels);
    return hipGetLastError();
}

hipError_t launch_render_reference(const DevScene& sc, const DevFrame& fr, const DevTargets& tg, bool counters, hipStream_t stream) {
    uint32_t n_tiles = fr.single_tile ? 1u : fr.n_owned_tiles;
    if (n_tiles == 0) return hipSuccess;
    dim3 grid(n_tiles * blocks_per_tile(fr.tile_size)), block(WAVE);
    if (counters)
        hipLaunchKernelGGL(k_render_reference<true>, grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
    else
        hipLaunchKernelGGL(k_render_reference<false>, grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
    return hipGetLastError();
}

hipError_t launch_render_extended(const DevScene& sc, const DevFrame& fr, const DevTargets& tg, FrameKernel kernel, bool counters, hipStream_t stream) {
    uint32_t n_tiles = fr.n_owned_tiles;
    if (n_tiles == 0) return hipSuccess;
    dim3 grid(n_tiles * blocks_per_tile(fr.tile_size)), block(WAVE);
    if (kernel != FrameKernel::MEGAKERNEL_SM) { // the nested loops (also the one-pass kernel)
        if (fr.adaptive && counters)
            hipLaunchKernelGGL((k_render_extended<true, true>), grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
        else if (fr.adaptive)
            hipLaunchKernelGGL((k_render_extended<false, true>), grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
        else if (counters)
            hipLaunchKernelGGL((k_render_extended<true, false>), grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
        else
            hipLaunchKernelGGL((k_render_extended<false, false>), grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
    } else {
        if (fr.adaptive && counters)
            hipLaunchKernelGGL((k_render_extended_sm<true, true>), grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
        else if (fr.adaptive)
            hipLaunchKernelGGL((k_render_extended_sm<false, true>), grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
        else if (counters)
            hipLaunchKernelGGL((k_render_extended_sm<true, false>), grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
        else
            hipLaunchKernelGGL((k_render_extended_sm<false, false>), grid, block, lane_stack_bytes(sc), stream, sc, fr, tg);
    }
    return hipGetLastError();
}

} // namespace rt
