/*
 * rt_hip.h — C ABI of librt_hip.so, the MI355X (gfx950) replacement for the
 * reference's device kernel `main_cs` and the wgpu plumbing around it.
 *
 * The reference has no FFI layer; the seam this ABI replaces is
 *   - src/buffers.rs:157-470  (BufferManager::update_*: host Vec<T> -> GPU buffers,
 *                              bindings 1-5 of src/renderer.rs:250-341),
 *   - src/compute.rs:137-251  (execute_compute_pass / process_tile /
 *                              process_color_channel: push constants + dispatch),
 *   - shader/src/lib.rs:25-89 (main_cs, what each dispatch computes),
 *   - shader/src/lib.rs:367-391 (main_fs, the 3-texture combine).
 * Each entry point below names the reference interface it stands in for.
 *
 * Conventions
 *   - Plain C: pointers + sizes, the Pod structs of rt_shared.h by pointer.
 *   - Every input pointer is borrowed for the duration of the call and copied
 *     (as queue.write_buffer does, src/buffers.rs:236-240); outputs go to
 *     caller-allocated memory; the context owns all device memory.
 *   - Return value: 0 = RT_OK, negative = error class; text via rt_last_error.
 *     Nothing throws or unwinds across this boundary.
 *   - A context is single-caller (not re-entrant), as the reference's
 *     RenderState is only touched from the winit thread (src/main.rs:239-292).
 *   - rt_render is synchronous: it returns after the device finished, so timing
 *     is well defined.  rt_dispatch_tile returns after the launch, as
 *     queue.submit does (src/compute.rs:165: the reference never waits); the
 *     next call that needs the result or an idle device (rt_read_*, rt_get_stats,
 *     rt_upload_*, rt_render, rt_destroy) waits for it, and rt_get_stats then
 *     reports the kernel time of the last dispatch.
 *   - There is no CPU fallback: without a HIP device every compute entry
 *     point fails with RT_ERR_HIP.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include "rt_shared.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERR_BAD_ARG (-1)
#define RT_ERR_OOM (-2)
#define RT_ERR_HIP (-3)
#define RT_ERR_NOT_UPLOADED (-4)
#define RT_ERR_INTERNAL (-5)

/* Render modes of rt_render. */
#define RT_MODE_LEGACY 0u    /* shader/src/lib.rs:58-79: one pixel-centre ray, miss = black           */
#define RT_MODE_WAVEFRONT 1u /* shader/src/lib.rs:92-149 + wavefront.rs:116-165: same, miss = sky      */
#define RT_MODE_EXTENDED 2u  /* jittered spp + real bounces built on the reference's declared-but-stub
                                wavefront API (SimpleRng, WavefrontRay types, russian roulette);
                                no reference implementation exists: see DESIGN.md "extended mode"      */

/* rt_render_params.flags */
#define RT_FLAG_COUNTERS 1u   /* run the counting variant of the kernel: fills node_visits / tri_tests  */
#define RT_FLAG_NO_SHADOWS 2u /* extended mode only: lights are not gated by shadow rays (as in the     */
                              /* reference, which never traces them)                                    */
#define RT_FLAG_KERNEL_V1 4u  /* extended mode only: run the nested-loop megakernel (v1) instead of the   */
                              /* wavefront pipeline (A/B measurements; same results)                    */
#define RT_FLAG_KERNEL_SM 8u  /* extended mode only: run the state-machine megakernel (v2) instead      */
#define RT_FLAG_NO_SHADOW_GRID 16u /* extended mode only: every shadow segment walks the BVH instead of its  */
                              /* light's triangle lists (A/B measurements and tests; same results)      */

#define RT_FLAG_KERNEL_PIPELINE 32u /* extended mode only: always the queue pipeline, also for the frames that take the one-pass kernel */
                              /* by rule (max_bounces 0 over a tiny tree; tests and A/B measurements; same results)        */

#define RT_FLAG_NO_BEAMS 64u  /* extended mode only: camera segments walk the tree like every other segment instead of testing their   */
                              /* pixel block's leaf list (A/B measurements and tests; same results)                                 */

#define RT_FLAG_STAGE_TIMES 128u /* extended mode only: time every launch of the frame's dominant stage kernel with HIP events on its stream  */
                              /* (bench.py's roofline of that kernel; read with rt_debug_stage_times)                                   */

#define RT_FLAG_ACCUMULATE 256u /* extended mode only (RT_ERR_BAD_ARG with modes 0/1): progressive rendering - this call adds its spp samples to */
                              /* the context's running image; rt_read_* then return the mean over all its samples.  See "Progressive       */
                              /* accumulation" below                                                                                       */
#define RT_FLAG_ACCUMULATE_RESTART 512u /* with RT_FLAG_ACCUMULATE only (RT_ERR_BAD_ARG otherwise): start a new running image at sample 0 */

typedef struct rt_ctx rt_ctx;

typedef struct rt_render_params {
    rt_camera camera;
    uint32_t width, height;
    uint32_t spp;         /* samples per pixel; modes 0/1 have no spp in the reference: they trace   */
                          /* the single pixel-centre ray and ignore this field                       */
    uint32_t max_bounces; /* mode 1: max_bounce_depth of pack_flags; mode 2: continuation segments,  */
                          /* at most RT_MAX_BOUNCES (RT_ERR_BAD_ARG beyond)                          */
    uint32_t mode;        /* RT_MODE_*                                                               */
    uint32_t frame_seed;  /* PushConstants::frame_seed (shared/src/lib.rs:226)                       */
    uint32_t tile_size;   /* 0 = RT_TILE_SIZE (128). Tile grid = TileHelper::calculate_tile_count    */
    uint32_t tile_rank;   /* this context renders tiles with (row-major index % tile_world) ==       */
    uint32_t tile_world;  /* tile_rank; 0/1 = all tiles. Used by one-process-per-GPU launches.       */
                          /* A context over several devices splits those tiles among its devices.   */
    uint32_t flags;       /* RT_FLAG_*                                                               */
} rt_render_params;

typedef struct rt_stats {
    uint64_t rays;         /* ray segments traced by the last render/dispatch (primary + continuation + shadow) */
    uint64_t primary_rays; /* camera segments among them                                             */
    uint64_t continuation_rays; /* bounce segments (extended mode)                                   */
    uint64_t shadow_rays;  /* shadow segments (extended mode)                                        */
    uint64_t pixels;       /* pixels written                                                          */
    uint64_t node_visits;  /* BVH nodes fetched   (only with RT_FLAG_COUNTERS, else 0)                */
    uint64_t tri_tests;    /* triangle records fetched and tested (only with RT_FLAG_COUNTERS)        */
    double kernel_ms;      /* HIP-event time of the trace kernel(s) on the launch stream              */
    double wall_ms;        /* host wall time of the call                                              */
    uint64_t node_bytes;   /* bytes of one BVH node record in the device layout                       */
    uint64_t tri_bytes;    /* bytes of one triangle record in the device layout                       */
    uint64_t scene_bytes;  /* device bytes held by the scene (nodes + triangles + materials + lights) */
    uint32_t bvh_nodes;    /* nodes in the device BVH                                                 */
    uint32_t bvh_depth;    /* its depth                                                               */
    uint32_t n_devices;
    uint32_t flags;        /* RT_STAT_* of the last render                                            */
    uint64_t texture_bytes; /* bytes of texture data last handed to rt_upload_textures (never sampled) */
    uint32_t n_textures;   /* TextureInfo records last handed to rt_upload_textures                   */
    uint32_t tree_build;   /* how the tree in use was built: 2 on the device (rt_upload_scene*, milliseconds), 0 by the host builder  */
                           /* (tiny scenes, the fallback for degenerate input, rt_prepare RT_PREPARE_QUALITY_TREE), 1 host PLOC (development) */
    uint64_t grid_bytes;   /* device bytes of the per-light triangle lists ("light grids") of the extended mode's shadow stage;   */
                           /* 0 until an extended-mode frame (or rt_prepare) has built them: rt_upload_scene* builds none          */
    double grid_build_ms;  /* host wall time that build took (once per uploaded scene)                                            */
} rt_stats;

/* rt_stats.flags */
#define RT_STAT_MEGAKERNEL_FALLBACK 1u /* extended mode: the frame did not fit the queue pipeline (more than 32 lights: one
                                          visibility bit per light; or a device share beyond the addressable path slots) and
                                          was rendered by the state-machine megakernel: same image, about 3x slower */

#define RT_STAT_SINGLE_PASS 2u /* extended mode: primary rays only (max_bounces 0) over a tiny tree: rendered by the one-pass kernel that
                                  keeps a pixel's samples in registers and stores it once (same image as the pipeline, several times faster) */

#define RT_STAT_REFIT 4u   /* rt_update_geometry: the tree in use was refitted to the new positions (topology kept)                     */
#define RT_STAT_REBUILT 8u /* rt_update_geometry: a new tree was built from the new positions (RT_UPDATE_REBUILD, or the fallback below) */

#define RT_MAX_BOUNCES 255u /* extended mode: bounce depths travel in 8 bits, as in pack_flags (shared/src/lib.rs:1154-1179) */

/* Create a context on `n_devices` HIP devices (ids in device_ids; NULL = device 0..n-1).
 * Replaces RenderState::new's adapter/device acquisition (src/renderer.rs:93-125).
 * With n_devices > 1 the scene is replicated and tiles are interleaved over the devices. */
int rt_create(rt_ctx** out, const int* device_ids, int n_devices);

/* Upload a scene from the host Vecs of SceneState (src/scene.rs:8-18).
 * Replaces BufferManager::update_scene_metadata / update_triangles / update_materials
 * (src/buffers.rs:157-377).  ref_nodes / ref_tri_indices (the output of
 * BvhBuilder::build, src/bvh.rs:104-122) are optional and only validated: the
 * library always builds its own acceleration structure, closest-hit results do
 * not depend on BVH topology. */
int rt_upload_scene(rt_ctx* ctx,
                    const rt_sphere* spheres, uint32_t n_spheres,
                    const rt_light* lights, uint32_t n_lights,
                    const rt_vertex* vertices, uint32_t n_vertices,
                    const rt_triangle* triangles, uint32_t n_triangles,
                    const rt_material* materials, uint32_t n_materials,
                    const rt_bvh_node* ref_nodes, uint32_t n_ref_nodes,
                    const uint32_t* ref_tri_indices, uint32_t n_ref_tri_indices);

/* Upload byte-for-byte what bindings 1-5 carry (src/renderer.rs:250-341):
 * binding 1 = scene_metadata [spheres|lights|bvh_nodes|triangle_indices|vertices] with
 * offsets in u32 words (src/buffers.rs:213-268), bindings 2-4 = Triangle buffers split
 * every triangles_per_buffer (src/buffers.rs:274-336), binding 5 = materials. */
int rt_upload_scene_packed(rt_ctx* ctx,
                           const uint32_t* scene_metadata, size_t n_u32,
                           const rt_scene_metadata_offsets* offsets,
                           const rt_triangle* const tri_buffers[3], const uint32_t tri_counts[3],
                           uint32_t triangles_per_buffer,
                           const rt_material* materials, uint32_t n_materials);

/* Hand over what bindings 6-7 carry (src/renderer.rs:250-341): the TextureInfo array of
 * BufferManager::update_textures (src/buffers.rs:381-419) and the texture bytes of update_texture_data
 * (src/buffers.rs:422-470, which packs them four to a u32).  main_cs binds both and reads neither
 * (shader/src/lib.rs:34-35), so they are validated (every texture inside the data) and recorded in rt_stats, nothing
 * else: a host that keeps its update_* call sequence maps one to one.  Independent of rt_upload_scene*. */
int rt_upload_textures(rt_ctx* ctx, const rt_texture_info* textures, uint32_t n_textures,
                       const uint8_t* texture_data, size_t n_bytes);

/* Optional: pay now what rt_render would otherwise pay on the first frame that needs it.  RT_PREPARE_SHADOW_GRIDS: the per-light
 * triangle lists of the extended mode's shadow stage (rt_stats.grid_bytes / grid_build_ms; 45-50 ms and 7.5 GB for a 262k-triangle
 * scene with five lights).  A host that only renders the reference's modes 0/1 (src/compute.rs:12-50) never calls this and never
 * pays: rt_upload_scene* builds only the tree.  No reference counterpart (the reference traces no shadow segments). */
#define RT_PREPARE_SHADOW_GRIDS 1u
/* RT_PREPARE_QUALITY_TREE: for scenes that stay - rebuild the acceleration structure with the host builder (binned SAH + insertion-based
 * optimisation, 0.35 s per 262 k triangles, 4.8 s for 3.8 M) in place of the tree rt_upload_scene* built on the device in milliseconds:
 * frames 2 % (sponza-like) to 9 % (bistro-like) faster, same images.  rt_stats.tree_build tells which tree is in use. */
#define RT_PREPARE_QUALITY_TREE 2u
int rt_prepare(rt_ctx* ctx, uint32_t what);

/* Render a whole frame (all tiles of this context's share, all three colour channels in
 * one pass).  Replaces ComputeRenderer::run_compute's tile x channel loop
 * (src/compute.rs:12-50, 137-251). */
int rt_render(rt_ctx* ctx, const rt_render_params* params);

/* Exact analogue of ONE process_color_channel dispatch (src/compute.rs:212-251): renders
 * the tile named by the push constants into the rgba8 texture of channel
 * pc->packed_flags & 0xFF (0..2; anything else is RT_ERR_BAD_ARG, as
 * get_compute_bind_group fails, src/renderer.rs:769-776).  Scene counts inside
 * pc->metadata_offsets are ignored in favour of the uploaded scene.  Asynchronous (see above). */
int rt_dispatch_tile(rt_ctx* ctx, const rt_push_constants* pc);

/* Read back the float RGB framebuffer of the last rt_render: width*height*3 floats, row-major, y down. */
int rt_read_rgb32f(rt_ctx* ctx, float* out, size_t n_floats);

/* Read back the three Rgba8Unorm channel textures (src/renderer.rs:452-475): width*height*4 bytes each. */
int rt_read_rgba8_channels(rt_ctx* ctx, uint8_t* red, uint8_t* green, uint8_t* blue, size_t n_bytes_each);

/* main_fs combine (shader/src/lib.rs:383-388): (red.x, green.y, blue.z, 255); width*height*4 bytes. */
int rt_read_rgba8_combined(rt_ctx* ctx, uint8_t* out, size_t n_bytes);

/* Per-pixel closest-hit record of the last mode-0/1 rt_render: original triangle index
 * (0xFFFFFFFF = miss, 0x80000000|i = sphere i) and hit distance t.  Index parity hook. */
int rt_read_hits(rt_ctx* ctx, uint32_t* prim_ids, float* t, size_t n_pixels);

int rt_get_stats(rt_ctx* ctx, rt_stats* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Progressive accumulation (RT_FLAG_ACCUMULATE; Cycles' viewport and the reference's ProgressiveState, src/renderer.rs:821-855,
 * are the model): many short rt_render calls refine one image.
 *
 * An accumulating call traces the samples n .. n+spp-1 of every pixel of its share, n being the samples already accumulated, adds them
 * to the running sums in sample order and writes the mean over all n+spp samples to the targets rt_read_rgb32f / rt_read_rgba8_* read.
 * Every sample of an accumulation is jittered (a closed frame jitters only when spp > 1), so an accumulation of N >= 2 samples gives
 * exactly the bits of ONE closed frame of N spp with the same parameters, however the N samples were split over calls and whichever
 * kernel (RT_FLAG_KERNEL_*) rendered each call.  An accumulation of exactly 1 sample is a jittered 1-spp image, which no closed frame gives.
 * The running image continues only while camera (bitwise), width, height, max_bounces, frame_seed, tile_size, tile_rank, tile_world
 * (0 read as 1, tile_size 0 as RT_TILE_SIZE) and RT_FLAG_NO_SHADOWS equal those of the previous accumulating call; otherwise the call starts
 * a new one at sample 0 by itself, as RT_FLAG_ACCUMULATE_RESTART does.  The other RT_FLAG_* bits change no bits and may differ.
 * The running image ends (the next accumulating call starts at 0) with rt_upload_scene*, rt_update_geometry, rt_dispatch_tile, any
 * rt_render without RT_FLAG_ACCUMULATE and an accumulating call that fails once it has passed its argument checks.  It survives rt_prepare,
 * rt_upload_textures, the ray queries, the surface queries, rt_direct_light, rt_radiance, rt_radiance_sh, rt_irradiance, rt_closest_point, rt_closest_point_all, rt_inside, rt_signed_distance, rt_overlap_box, rt_sweep_sphere, rt_sweep_box, rt_sweep_capsule, rt_contact_capsule, rt_overlap_obb, rt_sweep_obb, rt_overlap_triangle, rt_sweep_triangle, rt_contact_triangle, rt_overlap_mesh, rt_sweep_mesh, rt_camera_rays, rt_aovs, rt_sample_rays, rt_denoise, rt_get_stats and rt_read_*.  A call rejected for its arguments changes nothing.
 * Limit: RT_ACCUMULATE_MAX_SAMPLES samples (where the float sample count stops being exact); a call that would pass it is RT_ERR_BAD_ARG
 * and leaves the running image as it was.  rt_stats describes the call alone (its segments, pixels, kernel_ms).
 * A context over several devices, and a tile_rank / tile_world share, accumulates its own share of the pixels.
 * --------------------------------------------------------------------------------------------------------------- */
#define RT_ACCUMULATE_MAX_SAMPLES 16777216u /* 2^24 */

/* Samples in the context's running image (0 when there is none).  After an accumulating call, a count equal to that call's spp means
 * it started a new running image. */
int rt_accumulated_samples(rt_ctx* ctx, uint32_t* samples);

/* ---------------------------------------------------------------------------------------------------------------
 * Adaptive sampling (Cycles' adaptive sampling and Dammertz et al. 2010, "A hierarchical automatic stopping condition for Monte
 * Carlo global illumination", are the model): progressive accumulation that stops spending samples on pixels that have converged.
 *
 * Every owned pixel of an adaptive running image keeps n (its samples so far), S (the sum of its samples x_0 .. x_{n-1} in sample
 * order) and H (the sum of its odd-indexed samples x_1, x_3, ... in sample order).  At the start of every call each pixel's error is
 * evaluated from them in f32, in exactly this order:
 *     I = S / n,  A = (H + H) / n                      (per channel)
 *     d = |I.r - A.r| + |I.g - A.g| + |I.b - A.b|      (left to right)
 *     e = d / (1e-4f + sqrtf(I.r + I.g + I.b))
 * and the pixel is active when n < min_samples or e >= threshold (a NaN error counts as converged; n == 0 is always active).  An
 * active pixel traces its global samples n .. n+spp-1 (all jittered), adds them to S, the odd-indexed ones to H, and n += spp; an
 * inactive one traces nothing.  Every owned pixel's targets then hold S / (float)n: a pixel that stopped at n samples holds exactly
 * the bits of the closed n-spp frame (n >= 2) at that pixel, whichever kernel rendered each call.  There is no exchange between
 * neighbours: a pixel's fate depends on its own samples only, so tile shares and devices stay independent.
 *
 * p follows rt_render's rules and must be mode 2 with RT_FLAG_ACCUMULATE (RT_FLAG_ACCUMULATE_RESTART allowed); ap needs a finite
 * threshold >= 0 (0: no pixel with a finite error stops, i.e. plain accumulation), 2 <= min_samples <= RT_ACCUMULATE_MAX_SAMPLES and
 * flags == 0.  Anything else is RT_ERR_BAD_ARG and changes nothing.
 * The running image continues under the key of RT_FLAG_ACCUMULATE and is marked adaptive: a plain accumulating rt_render after
 * adaptive calls starts a new running image, and so does the reverse.  threshold and min_samples are not part of the key: a tighter
 * threshold on a later call wakes stopped pixels up.  Everything else that ends an accumulation ends this one.
 * rt_accumulated_samples returns the count of a pixel that never stopped (the sum of the spp of the image's calls); a call that could
 * take a pixel past RT_ACCUMULATE_MAX_SAMPLES is RT_ERR_BAD_ARG.  rt_stats of the call: rays / primary_rays / continuation_rays /
 * shadow_rays count what was traced, pixels the pixels that received samples, kernel_ms includes the selection and image passes.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_adaptive_params {
    float threshold;       /* e at or above which a pixel keeps sampling; 0 = never stop (plain accumulation) */
    uint32_t min_samples;  /* samples every pixel gets before it may stop; >= 2 */
    uint32_t flags;        /* reserved, 0 */
    uint32_t _pad;
} rt_adaptive_params;      /* 16 B */

typedef struct rt_adaptive_pixel {
    float sum[3];  float samples;   /* S, n (as float: exact below RT_ACCUMULATE_MAX_SAMPLES) */
    float odd[3];  float error;     /* H, e by the rule above (0 when n == 0) */
} rt_adaptive_pixel;       /* 32 B */

RT_STATIC_ASSERT(sizeof(rt_adaptive_params) == 16, "rt_adaptive_params is 16 B");
RT_STATIC_ASSERT(offsetof(rt_adaptive_params, min_samples) == 4 && offsetof(rt_adaptive_params, flags) == 8, "rt_adaptive_params offsets");
RT_STATIC_ASSERT(sizeof(rt_adaptive_pixel) == 32, "rt_adaptive_pixel is 32 B");
RT_STATIC_ASSERT(offsetof(rt_adaptive_pixel, samples) == 12 && offsetof(rt_adaptive_pixel, odd) == 16 && offsetof(rt_adaptive_pixel, error) == 28,
                 "rt_adaptive_pixel offsets");

int rt_render_adaptive(rt_ctx* ctx, const rt_render_params* p, const rt_adaptive_params* ap);

/* One record per pixel (n_pixels == width*height of the running image), gathered over devices and tile shares as rt_read_rgb32f
 * does; pixels outside the share read as zeros.  RT_ERR_BAD_ARG when the context has no adaptive running image. */
int rt_read_adaptive(rt_ctx* ctx, rt_adaptive_pixel* out, size_t n_pixels);

/* ---------------------------------------------------------------------------------------------------------------
 * Ray queries: closest hit, occlusion and the first K hits for caller-supplied rays (no reference counterpart; Embree's rtcIntersect /
 * rtcOccluded are the model).  They trace the uploaded scene with the frames' rules and leave the last frame alone.
 *
 * Range: a triangle or sphere is accepted at tmin < t < tmax, both strict; t is parametric along `direction`, which
 * need not be normalised.  A tmin below RT_MIN_RAY_DISTANCE (1e-5, negative values included) is raised to it: the
 * floor the tree's box filter is conservative for, and the render path's own.  tmax = +inf is allowed.
 * Rules: the Moller-Trumbore arithmetic, the tie rule (equal t: the lower original triangle index wins among
 * triangles, strict against spheres) and "spheres first" of the frames.  A camera ray (rt_camera_rays) therefore gives
 * exactly the prim_id and t bits rt_read_hits gives for its pixel, and the answer does not depend on the tree
 * (RT_PREPARE_QUALITY_TREE or not).
 * Hit record: prim_id = original triangle index, 0x80000000 | i for sphere i, 0xFFFFFFFF for a miss (as rt_read_hits).
 * Triangle: u, v = the Moller-Trumbore barycentrics (weights of v1 and v2) of the arithmetic that accepted the hit.
 * Sphere: u = v = 0.  Miss: t = the ray's tmax as given, u = v = 0.
 * Occlusion: occluded[i] = 1 if any primitive is accepted in the range, else 0 (any-hit walk, early exit); always equal
 * to rt_intersect's prim_id != 0xFFFFFFFF.
 * Degenerate rays (a non-finite origin or direction component, a zero direction, a NaN bound, or !(tmin < tmax) after
 * the floor) are misses / not occluded, without a walk.  The kernel checks this itself.
 * Buffers: each pointer is classified by the library.  Device memory of one of the context's devices is read and
 * written in place on that device (input and output on the same device, 16-byte aligned: RT_ERR_BAD_ARG otherwise);
 * host memory of any kind (pageable, pinned, managed) is staged through per-device buffers in chunks of at most
 * RT_QUERY_CHUNK rays, and on a context with several devices split into one contiguous range per device.
 * Synchronous: the results are in place when the call returns.  Device-resident input must be complete before the call:
 * the library reads it on its own stream.  A query first waits for an rt_dispatch_tile still in flight.
 * Statistics: rays = n; primary_rays, continuation_rays, shadow_rays, pixels = 0; kernel_ms (max over devices) and
 * wall_ms; node_visits / tri_tests with RT_QUERY_COUNTERS (else 0).  rt_read_* still return the last frame.
 * Errors: n == 0 is RT_OK and does nothing; a NULL pointer with n > 0 or unknown flag bits are RT_ERR_BAD_ARG; a query
 * before any upload is RT_ERR_NOT_UPLOADED.  An empty scene gives all misses.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_ray {
    float origin[3];
    float tmin;
    float direction[3];
    float tmax;
} rt_ray; /* 32 bytes */

typedef struct rt_hit {
    float t;
    float u, v;
    uint32_t prim_id;
} rt_hit; /* 16 bytes */

RT_STATIC_ASSERT(sizeof(rt_ray) == 32, "rt_ray is 32 B");
RT_STATIC_ASSERT(offsetof(rt_ray, tmin) == 12 && offsetof(rt_ray, direction) == 16 && offsetof(rt_ray, tmax) == 28, "rt_ray offsets");
RT_STATIC_ASSERT(sizeof(rt_hit) == 16, "rt_hit is 16 B");
RT_STATIC_ASSERT(offsetof(rt_hit, u) == 4 && offsetof(rt_hit, v) == 8 && offsetof(rt_hit, prim_id) == 12, "rt_hit offsets");

/* flags of rt_intersect / rt_occluded (a set of their own, not RT_FLAG_*) */
#define RT_QUERY_COUNTERS 1u /* run the counting variant of the query kernel: fills rt_stats.node_visits / tri_tests */

#define RT_QUERY_CHUNK 4194304u /* host batches are staged in chunks of at most this many rays */

/* Closest hit of each of the n rays. */
int rt_intersect(rt_ctx* ctx, const rt_ray* rays, size_t n, rt_hit* hits, uint32_t flags);

/* Any hit of each of the n rays: occluded[i] = 0 or 1. */
int rt_occluded(rt_ctx* ctx, const rt_ray* rays, size_t n, uint8_t* occluded, uint32_t flags);

/* Multi-hit: the first max_hits hits along each of the n rays, in order (Embree's / OptiX's "all hits" idiom: transparency done by
 * the caller, depth peeling, thickness, crossing parity), in one walk per ray.
 * Candidates: a triangle is a candidate when the frames' Moller-Trumbore arithmetic accepts it at tmin < t < tmax, both strict,
 * tmin raised to RT_MIN_RAY_DISTANCE as for rt_intersect.  A sphere is a candidate at the single t the frames' sphere test gives
 * for the ray's own tmin (t1 if t1 > tmin, else t2), if that lies in the range: a sphere appears at most once per ray.  Every
 * triangle has exactly one record in the tree (the builders never split a triangle), so a triangle appears at most once per ray.
 * Order: ascending t; at equal t bits spheres before triangles, spheres by ascending sphere index, triangles by ascending
 * original triangle index.  That is the order in which rt_intersect's rules would pick a winner: for max_hits >= 1 ray i's first
 * record hits[i * max_hits] is bit for bit the rt_intersect record of ray i.
 * Output: ray i's first min(total, max_hits) candidates in that order as rt_hit records at hits[i * max_hits ..] (ray-major),
 * t, u, v and prim_id exactly as rt_intersect defines them (u, v from the arithmetic that accepted the triangle, 0 for spheres).
 * Unused slots are miss records: t = the ray's tmax as given, u = v = 0, prim_id = 0xFFFFFFFF.  max_hits == 1 gives exactly
 * rt_intersect's bytes, degenerate rays (all misses without a walk, the same degeneracy rules) and an empty scene included.
 * counts[i] = the number of hit records written for ray i; with RT_QUERY_COUNT_ALL instead the total number of candidates in the
 * range, which can exceed max_hits (the records written are the same; the walk can then not shrink its range, so it costs more).
 * `counts` may be NULL unless max_hits == 0.  max_hits == 0 is allowed only with RT_QUERY_COUNT_ALL and a non-NULL counts; `hits`
 * is then ignored: a pure crossing count.
 * The result does not depend on the tree in use (device build, host build, RT_PREPARE_QUALITY_TREE, refitted).
 * Buffers: each pointer is classified as for the other queries; all are host memory, or all device memory of one context device
 * (rays and hits 16-byte aligned, counts 4-byte aligned), anything else is RT_ERR_BAD_ARG.  Host batches are staged in chunks of
 * at most RT_QUERY_CHUNK / max(max_hits, 1) rays, so the staged hit records never exceed those of an rt_intersect chunk; a context
 * over several devices splits the batch into one contiguous range per device.
 * Errors: n == 0 is RT_OK; a NULL rays, or a NULL hits with max_hits > 0, max_hits > RT_MULTI_HIT_MAX, max_hits == 0 without
 * RT_QUERY_COUNT_ALL and counts, and unknown flag bits are RT_ERR_BAD_ARG; a call before any upload is RT_ERR_NOT_UPLOADED.
 * Statistics, synchronisation and side effects as for rt_intersect: synchronous, first waits for an rt_dispatch_tile in flight;
 * rays = n, the other counts 0, kernel_ms the maximum over devices, node_visits / tri_tests only with RT_QUERY_COUNTERS; the last
 * frame, the rt_read_* results and a running accumulation are left alone. */
#define RT_QUERY_COUNT_ALL 2u   /* rt_intersect_all, rt_closest_point_all, rt_overlap_box, rt_overlap_obb, rt_overlap_triangle and rt_contact_capsule only; also rt_contact_triangle */
#define RT_MULTI_HIT_MAX 16u

int rt_intersect_all(rt_ctx* ctx, const rt_ray* rays, size_t n, uint32_t max_hits,
                     rt_hit* hits,      /* n * max_hits records, ray-major: ray i's hits at hits[i*max_hits ..] */
                     uint32_t* counts,  /* n entries; may be NULL unless max_hits == 0 */
                     uint32_t flags);   /* RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL */

/* The width x height pixel-centre camera rays of mode 0 (RT_MODE_LEGACY: direction normalised twice, as Ray::new) or
 * mode 1 (RT_MODE_WAVEFRONT: once), computed by the frames' own ray generation; any other mode is RT_ERR_BAD_ARG.
 * Row-major, y down, tmin = RT_MIN_RAY_DISTANCE, tmax = FLT_MAX.  `out` (width * height records) may be host or
 * device memory, classified as for the queries.  Needs no scene.  Synchronous. */
int rt_camera_rays(rt_ctx* ctx, const rt_camera* camera, uint32_t width, uint32_t height, uint32_t mode, rt_ray* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Surface queries: what a caller needs AT the hit - the point, the geometric normal and the material - and the ambient occlusion
 * of such points (no reference counterpart; Embree's rtcInterpolate after rtcIntersect and the ambient-occlusion pass of every
 * baker are the model).  Both are defined by composing calls above, so their results follow the device's records (after
 * rt_update_geometry too) and the device's arithmetic.
 *
 * rt_surface: ray i's closest hit is exactly rt_intersect's (range, tmin floor, degenerate rays, tie rule, spheres first).  On a hit:
 *   position = origin + direction * t (one multiply, one add per component, as Ray::at); normal = the geometric normal of the
 *   primitive (triangle: normalize(cross(e1, e2)); sphere: normalize(position - centre)) face-forwarded against the ray:
 *   dot(normal, direction) < 0 ? normal : -normal, the normal rt_aovs reports; prim_id as rt_hit.prim_id; material_id = the
 *   record's material id, not checked against the material table.  On a miss, a degenerate ray included: position = normal = 0,
 *   prim_id = 0xFFFFFFFF, material_id = 0.
 * rt_ambient_occlusion: for point i (its index in the caller's array) with position P and normal N, and sample s < samples:
 *   rng = rng_for(seed + i (mod 2^32), s) (the frames' generator), u1 = next_f32(), u2 = next_f32(),
 *   direction = normalize(N + unit_vector(u1, u2)) (the cosine lobe of the extended mode's diffuse bounce), origin = P + N * bias,
 *   tmin = RT_MIN_RAY_DISTANCE, tmax = max_distance, and this ray is traced by rt_occluded's rules, its degenerate-ray rule
 *   included (a zero-length N + unit_vector is not occluded).  unoccluded[i] = the samples that were not occluded,
 *   visibility[i] = (float)unoccluded[i] / (float)samples.  So unoccluded[i] = samples - the sum of rt_occluded over those rays,
 *   whatever the tree, the device count, the kind of memory and the chunking.  A point with a non-finite position or normal
 *   component or a zero normal traces nothing: unoccluded = samples, visibility = 1.  N is used as given (rt_surface gives unit
 *   normals); prim_id and material_id are ignored.
 *   params: samples 1 .. RT_AO_MAX_SAMPLES; max_distance > 0, +inf allowed (NaN or <= 0: RT_ERR_BAD_ARG); bias finite and >= 0
 *   (the frames offset their secondary segments by 1e-3); flags RT_QUERY_COUNTERS; _pad ignored.
 * Buffers: each pointer is classified as for the ray queries; all are host memory, or all device memory of one context device
 * (records 16-byte aligned, visibility and unoccluded 4-byte aligned), anything else is RT_ERR_BAD_ARG.  Host batches are staged in
 * chunks of at most RT_QUERY_CHUNK rays (rt_surface) or max(1, RT_QUERY_CHUNK / samples) points (rt_ambient_occlusion); a context
 * over several devices splits the batch into one contiguous range per device.  Either of visibility and unoccluded may be NULL.
 * Errors: n == 0 is RT_OK; a NULL rays / out / points / params, visibility and unoccluded both NULL, bad parameters and unknown flag
 * bits are RT_ERR_BAD_ARG and change nothing; a call before any upload is RT_ERR_NOT_UPLOADED.
 * Statistics, synchronisation and side effects as for rt_intersect: synchronous, first waits for an rt_dispatch_tile in flight;
 * rays = n (rt_surface) or n * samples (rt_ambient_occlusion), the other counts 0, kernel_ms the maximum over devices,
 * node_visits / tri_tests only with RT_QUERY_COUNTERS; the last frame, the rt_read_* results and a running accumulation are left alone.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_surface_point {
    float position[3];
    uint32_t prim_id;     /* as rt_hit.prim_id; 0xFFFFFFFF = miss */
    float normal[3];
    uint32_t material_id; /* the record's material id, unchecked; 0 on a miss */
} rt_surface_point; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_surface_point) == 32, "rt_surface_point is 32 B");
RT_STATIC_ASSERT(offsetof(rt_surface_point, prim_id) == 12 && offsetof(rt_surface_point, normal) == 16 && offsetof(rt_surface_point, material_id) == 28,
                 "rt_surface_point offsets");

#define RT_AO_MAX_SAMPLES 4096u

typedef struct rt_ao_params {
    uint32_t samples;   /* 1 .. RT_AO_MAX_SAMPLES */
    uint32_t seed;
    float max_distance; /* > 0, +inf allowed */
    float bias;         /* finite, >= 0: the origin's offset along the normal */
    uint32_t flags;     /* RT_QUERY_COUNTERS */
    uint32_t _pad[3];
} rt_ao_params; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_ao_params) == 32, "rt_ao_params is 32 B");
RT_STATIC_ASSERT(offsetof(rt_ao_params, seed) == 4 && offsetof(rt_ao_params, max_distance) == 8 && offsetof(rt_ao_params, bias) == 12 &&
                     offsetof(rt_ao_params, flags) == 16,
                 "rt_ao_params offsets");

/* Point, face-forwarded geometric normal and material of the closest hit of each of the n rays. */
int rt_surface(rt_ctx* ctx, const rt_ray* rays, size_t n, rt_surface_point* out, uint32_t flags);

/* Ambient occlusion of the n points: params->samples cosine-distributed occlusion rays each. */
int rt_ambient_occlusion(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_ao_params* params,
                         float* visibility,     /* n entries; may be NULL */
                         uint32_t* unoccluded); /* n entries; may be NULL, not both */

/* ---------------------------------------------------------------------------------------------------------------
 * Direct-light queries: the light that the scene's own lights deliver to points the caller supplies, with shadows (no reference
 * counterpart; the direct-lighting pass of a baker or a probe is the model).  It is the first vertex of the extended mode's path and
 * nothing more: one light sum per point, no bounces, no random numbers.  Every bit is fixed by calls above and by the frames.
 *
 * rt_direct_light: for point i with position P, normal N and material_id as given (prim_id is ignored):
 *   - a record with a non-finite P or N component or with N == 0 (what rt_surface writes for a miss) is no point: nothing is
 *     traced, radiance = 0, lit_mask = 0;
 *   - material_id >= the uploaded material count: radiance = (1, 0, 1), the frames' magenta, lit_mask = 0, nothing is traced;
 *   - otherwise radiance is the extended mode's ordered light sum at a vertex with materials[material_id]:
 *     0.1 * albedo first when RT_DIRECT_AMBIENT is set (as the frames' terminal vertex adds it), then the contribution of every light
 *     in index order (the reference's calculate_light_contribution: f16-rounded attenuation, 0/1 type masks, spot factor), a light
 *     whose shadow segment is occluded skipped, then the emission.  The transmission mix the frames apply when they leave a terminal
 *     vertex of a transmissive material is NOT applied: radiance equals a closed frame's pixel (mode 2, max_bounces 0, 1 spp) only
 *     for materials with transmission <= 0.
 *   A light has a shadow segment when its contribution is non-zero and RT_DIRECT_NO_SHADOWS is clear: origin = P + N * bias (one
 *   multiply, one add per component), direction and tmax = the direction toward the light and its distance as the contribution
 *   computes them (normalize(L - P) and |L - P|; a directional light: -normalize(direction) and FLT_MAX), tmin =
 *   RT_MIN_RAY_DISTANCE, traced by rt_occluded's rules, its degenerate-ray rule included.  So "occluded" is exactly rt_occluded of
 *   that ray, whatever the tree, the device count, the kind of memory, the chunking, and whether light grids exist.
 *   lit_mask: bit li is set when light li's contribution is non-zero and (unless RT_DIRECT_NO_SHADOWS) its segment is not occluded:
 *   the lights that entered the sum.
 *   N is used as given, neither flipped nor normalised.  The frames shade with the UNFLIPPED geometric normal of the primitive;
 *   rt_surface reports the normal face-forwarded against its ray.  Pass rt_surface's normal to light the side the ray arrived on
 *   (bakers, probes); negate it on back faces (dot(geometric normal, ray direction) > 0) to reproduce a frame's pixel.
 *   params: bias finite and >= 0 (the frames use 1e-3); flags RT_DIRECT_AMBIENT, RT_DIRECT_NO_SHADOWS, RT_DIRECT_NO_SHADOW_GRID,
 *   RT_QUERY_COUNTERS; _pad ignored.
 * Light grids: the call never builds them.  A device that holds them (rt_prepare(RT_PREPARE_SHADOW_GRIDS), or an extended-mode frame
 *   before) answers segments from the per-light triangle lists where that is proven to give rt_occluded's answer: bias bit-equal to
 *   1e-3f, |N.N - 1| <= 1e-5 and P within one largest extent of the triangles' bounding box; every other segment, and every
 *   segment with RT_DIRECT_NO_SHADOW_GRID, walks the tree.  The results are the same bits either way.
 * Buffers, synchronisation and side effects as for rt_surface: both pointers host memory, or both device memory of one context
 * device (16-byte aligned), anything else is RT_ERR_BAD_ARG; host batches are staged in chunks of at most RT_QUERY_CHUNK points; a
 * context over several devices splits the batch into one contiguous range per device; synchronous, first waits for an
 * rt_dispatch_tile in flight; the last frame, the rt_read_* results and a running accumulation are left alone.
 * Errors: n == 0 is RT_OK; NULL points / params / out, unknown flag bits, a bad bias and a scene with more than
 * RT_DIRECT_MAX_LIGHTS lights are RT_ERR_BAD_ARG and change nothing; a call before any upload is RT_ERR_NOT_UPLOADED.  A scene
 * without lights gives radiance = emission (+ the ambient term with RT_DIRECT_AMBIENT) and lit_mask = 0.
 * Statistics: rays = shadow_rays = the shadow segments of the call (counted on the device), the other counts 0, kernel_ms the
 * maximum over devices, node_visits / tri_tests only with RT_QUERY_COUNTERS (list entries tested count as triangle tests).
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_lighting {
    float radiance[3];
    uint32_t lit_mask; /* bit li: light li entered the sum */
} rt_lighting; /* 16 bytes */

typedef struct rt_direct_light_params {
    float bias;     /* finite, >= 0: the segments' origin offset along the normal */
    uint32_t flags; /* RT_DIRECT_* | RT_QUERY_COUNTERS */
    uint32_t _pad[2];
} rt_direct_light_params; /* 16 bytes */

RT_STATIC_ASSERT(sizeof(rt_lighting) == 16 && offsetof(rt_lighting, lit_mask) == 12, "rt_lighting is 16 B, lit_mask at 12");
RT_STATIC_ASSERT(sizeof(rt_direct_light_params) == 16 && offsetof(rt_direct_light_params, flags) == 4 && offsetof(rt_direct_light_params, _pad) == 8,
                 "rt_direct_light_params is 16 B, flags at 4");

#define RT_DIRECT_AMBIENT 4u         /* add the 0.1 * albedo ambient term first, as the frames' terminal vertex does */
#define RT_DIRECT_NO_SHADOWS 8u      /* no shadow segments: every non-zero contribution counts (RT_FLAG_NO_SHADOWS) */
#define RT_DIRECT_NO_SHADOW_GRID 16u /* every segment walks the tree (A/B and tests; same results) */
#define RT_DIRECT_MAX_LIGHTS 32u     /* one bit per light; the light count the extended mode's pipeline takes */

/* Shadowed direct lighting of the n points. */
int rt_direct_light(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_direct_light_params* params, rt_lighting* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Path queries: the radiance the extended mode carries back along rays the caller supplies (no reference counterpart; the probe,
 * lightmap-texel and irradiance-cache passes of a baker are the model).  It is the extended mode's whole path - the nested-loop
 * statement of DESIGN.md section 5 - started from a ray that need not be a camera ray.  Every bit is fixed by calls above and by the
 * frames.
 *
 * rt_radiance: for ray i (its index in the caller's array):
 *   - a degenerate ray (rt_intersect's rules: a non-finite origin or direction component, a zero direction, a NaN bound, or
 *     !(tmin < tmax) after tmin is raised to RT_MIN_RAY_DISTANCE) is no path: nothing is traced, radiance = 0, segments = 0;
 *   - otherwise sample k < samples draws from rng = rng_for(seed + i (mod 2^32), first_sample + k), the frames' generator; with
 *     RT_PATH_CAMERA_DRAWS two next_f32() are drawn and dropped first.  Then radiance = 0, throughput = 1, no hero channel, and for
 *     depth = 0, 1, ..: the closest hit of the segment - the first segment in the ray's own (tmin, tmax) exactly as rt_intersect, every
 *     later one as the frames trace a continuation; a miss adds sky * throughput and ends the path; a material id past the table adds
 *     (1, 0, 1) * throughput and ends it; else the vertex is terminal when depth >= max_bounces, its light sum is rt_direct_light's
 *     (the scene's lights in index order, the ambient term at the terminal vertex only, each shadow segment from point + normal * 1e-3
 *     by rt_occluded's rules, none with RT_PATH_NO_SHADOWS) with the UNFLIPPED geometric normal, as in the frames; the path leaves the
 *     vertex as the frames do (the transmission mix at the terminal vertex) and scatters as they do (transmission with the hero
 *     channel and Snell's refraction, the metallic lobe, the cosine lobe, the roulette from the third vertex on, the same draws in the
 *     same order).  x_k is the path's radiance.
 *   out[i].radiance = (0 + x_0 + x_1 + ...) / (float)samples: an f32 sum from zero in sample order and one division, the frames'
 *   pixel reduction.  out[i].segments = the segments traced for ray i over all its samples (first + continuation + shadow), mod 2^32.
 *   Any number of lights: the 32-light limit of the extended mode's pipeline and of rt_direct_light does not apply.
 * What follows:
 *   - rays = rt_camera_rays(mode 1) of a W x H frame, seed = frame_seed, first_sample = 0, samples = 1, no RT_PATH_CAMERA_DRAWS:
 *     out[x + y * W].radiance is bit for bit that pixel of the closed mode-2 frame with 1 spp, for any max_bounces, with or without
 *     shadows, and the sum of the segments is that frame's rt_stats.rays;
 *   - rays = rt_sample_rays(p, s), first_sample = s, samples = 1, RT_PATH_CAMERA_DRAWS: the result is sample x_s of that pixel of a
 *     frame of S >= 2 spp; summing s = 0 .. S-1 from zero in f32 and dividing by (float)S gives that frame's pixel bit for bit;
 *   - the result does not depend on the tree in use (device build, host build, RT_PREPARE_QUALITY_TREE, refitted), the device count,
 *     the kind of memory or the chunking.  Light grids are never looked at: every shadow segment walks the tree.
 * params: samples 1 .. RT_PATH_MAX_SAMPLES; max_bounces 0 .. RT_MAX_BOUNCES; first_sample + samples <= 2^32; flags RT_PATH_NO_SHADOWS,
 *   RT_PATH_CAMERA_DRAWS, RT_QUERY_COUNTERS; _pad ignored.
 * Buffers, synchronisation and side effects as for rt_direct_light: both pointers host memory, or both device memory of one context
 * device (16-byte aligned), anything else is RT_ERR_BAD_ARG; batches are traced in chunks of at most max(1, RT_QUERY_CHUNK / samples)
 * rays, host batches staged chunk by chunk; a context over several devices splits a host batch into one contiguous range per device
 * (the seed's i stays the index in the caller's array); synchronous, first waits for an rt_dispatch_tile in flight; the last frame,
 * the rt_read_* results and a running accumulation are left alone.
 * Errors: n == 0 is RT_OK; NULL rays / params / out, samples out of range, max_bounces > RT_MAX_BOUNCES, first_sample + samples > 2^32
 * and unknown flag bits are RT_ERR_BAD_ARG and change nothing; a call before any upload is RT_ERR_NOT_UPLOADED.  An empty scene gives
 * the sky and segments = samples.
 * Statistics: rays = all segments, primary_rays = first segments (valid rays x samples), continuation_rays and shadow_rays as the
 * frames count them (on the device), pixels = 0, kernel_ms the maximum over devices, node_visits / tri_tests only with
 * RT_QUERY_COUNTERS.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_path_params {
    uint32_t samples;      /* paths per ray, 1 .. RT_PATH_MAX_SAMPLES */
    uint32_t max_bounces;  /* as rt_render_params.max_bounces in mode 2: 0 .. RT_MAX_BOUNCES */
    uint32_t seed;         /* the frames' frame_seed */
    uint32_t first_sample; /* global index of the ray's first sample; first_sample + samples must not pass 2^32 */
    uint32_t flags;        /* RT_PATH_* | RT_QUERY_COUNTERS */
    uint32_t _pad[3];
} rt_path_params; /* 32 bytes */

typedef struct rt_path_result {
    float radiance[3];
    uint32_t segments; /* segments traced for this ray over all its samples (first + continuation + shadow), mod 2^32 */
} rt_path_result; /* 16 bytes */

RT_STATIC_ASSERT(sizeof(rt_path_params) == 32, "rt_path_params is 32 B");
RT_STATIC_ASSERT(offsetof(rt_path_params, max_bounces) == 4 && offsetof(rt_path_params, seed) == 8 && offsetof(rt_path_params, first_sample) == 12 &&
                     offsetof(rt_path_params, flags) == 16 && offsetof(rt_path_params, _pad) == 20,
                 "rt_path_params offsets");
RT_STATIC_ASSERT(sizeof(rt_path_result) == 16 && offsetof(rt_path_result, segments) == 12, "rt_path_result is 16 B, segments at 12");

#define RT_PATH_NO_SHADOWS 32u   /* lights are not gated by shadow segments (RT_FLAG_NO_SHADOWS) */
#define RT_PATH_CAMERA_DRAWS 64u /* two next_f32 are drawn and dropped before the path: the draws a jittered camera sample spent on its jitter */
#define RT_PATH_MAX_SAMPLES 4096u

/* Extended-mode path radiance along each of the n rays: params->samples paths each. */
int rt_radiance(rt_ctx* ctx, const rt_ray* rays, size_t n, const rt_path_params* params, rt_path_result* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Probe queries: the radiance field at points the caller supplies, as 9 real spherical-harmonic coefficients per colour channel (L2;
 * Ramamoorthi and Hanrahan 2001) - the form DDGI-style probe grids and lightmap bakers store (no reference counterpart).  It is
 * rt_radiance over directions the device draws itself, projected in sample order.  Every bit is fixed by rt_radiance and one f32
 * statement.
 *
 * rt_radiance_sh: for probe i (its index in the caller's array) and sample k < samples:
 *   1. rng = rng_for(seed + i (mod 2^32), first_sample + k), the frames' generator; u1 = next_f32(), u2 = next_f32();
 *      d_k = unit_vector(u1, u2), the frames' uniformly distributed unit direction, used as it comes: not renormalised.
 *   2. x_k = the radiance rt_radiance gives for the ray {origin = position, tmin = RT_MIN_RAY_DISTANCE, direction = d_k, tmax = FLT_MAX}
 *      with samples = 1, first_sample = first_sample + k, the same seed and ray index i, the same max_bounces and RT_PATH_NO_SHADOWS,
 *      and RT_PATH_CAMERA_DRAWS: the path goes on from the generator's third draw.  g_k = that ray's segments.
 *   3. the basis at d = (x, y, z), every operation one f32 rounding, as written, nothing fused:
 *        Y0 = 0.2820948f                   Y1 = 0.4886025f*y                        Y2 = 0.4886025f*z
 *        Y3 = 0.4886025f*x                 Y4 = 1.0925484f*(x*y)                    Y5 = 1.0925484f*(y*z)
 *        Y6 = 0.31539157f*(3.0f*(z*z) - 1.0f)   Y7 = 1.0925484f*(x*z)               Y8 = 0.5462742f*(x*x - y*y)
 *   4. out[i].sh[j][c] = (0 + x_0[c]*Y_j(d_0) + x_1[c]*Y_j(d_1) + ...) * (12.566371f / (float)samples): an f32 sum from zero in
 *      sample order, each term one product, then one division and one multiply in that grouping (the Monte-Carlo estimate of the
 *      projection integral over the sphere, 4 pi / samples per sample).  out[i].segments = g_0 + g_1 + ... mod 2^32.
 *   5. a probe with a non-finite position component is no probe: nothing is traced, all 27 coefficients are 0 and segments = 0.  A
 *      sample whose d_k is zero contributes x_k = 0, g_k = 0 by rt_radiance's own degeneracy rule.
 * What follows:
 *   - the result does not depend on the tree in use (device build, host build, RT_PREPARE_QUALITY_TREE, refitted), the device count,
 *     the kind of memory or the chunking.  Light grids are never looked at.  Any number of lights, as rt_radiance.
 *   - an empty scene gives the sky's projection: sh[0][c] = sky[c] * 4 pi * 0.2820948 within (samples + 4) * 2^-24 of it, the other
 *     coefficients the Monte-Carlo noise around 0 (standard deviation sky[c] * sqrt(4 pi / samples)), segments = samples.
 * params: rt_path_params as rt_radiance reads it - samples (directions per probe) 1 .. RT_PATH_MAX_SAMPLES; max_bounces 0 ..
 *   RT_MAX_BOUNCES; first_sample + samples <= 2^32; flags RT_PATH_NO_SHADOWS, RT_QUERY_COUNTERS - except RT_PATH_CAMERA_DRAWS, which
 *   is RT_ERR_BAD_ARG: the call spends those two draws itself.  _pad ignored; rt_probe._pad ignored.
 * Buffers, synchronisation and side effects as for rt_radiance: both pointers host memory, or both device memory of one context
 * device (16-byte aligned), anything else is RT_ERR_BAD_ARG; batches are traced in chunks of at most max(1, RT_QUERY_CHUNK / samples)
 * probes, host batches staged chunk by chunk; a context over several devices splits a host batch into one contiguous range per device
 * (the seed's i stays the index in the caller's array); synchronous, first waits for an rt_dispatch_tile in flight; the last frame,
 * the rt_read_* results and a running accumulation are left alone.
 * Errors: n == 0 is RT_OK; NULL probes / params / out, samples out of range, max_bounces > RT_MAX_BOUNCES, first_sample + samples > 2^32,
 * RT_PATH_CAMERA_DRAWS and unknown flag bits are RT_ERR_BAD_ARG and change nothing; a call before any upload is RT_ERR_NOT_UPLOADED.
 * Statistics: as rt_radiance - rays = all segments, primary_rays = first segments (valid probes x samples), continuation_rays and
 * shadow_rays as the frames count them, pixels = 0, kernel_ms the maximum over devices, node_visits / tri_tests only with
 * RT_QUERY_COUNTERS.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_probe {
    float position[3];
    uint32_t _pad; /* ignored */
} rt_probe; /* 16 bytes */

typedef struct rt_sh9 {
    float sh[9][3];    /* coefficient j, channel c at sh[j][c] */
    uint32_t segments; /* segments traced for this probe over all its samples (first + continuation + shadow), mod 2^32 */
} rt_sh9; /* 112 bytes */

RT_STATIC_ASSERT(sizeof(rt_probe) == 16 && offsetof(rt_probe, _pad) == 12, "rt_probe is 16 B, _pad at 12");
RT_STATIC_ASSERT(sizeof(rt_sh9) == 112 && offsetof(rt_sh9, sh) == 0 && offsetof(rt_sh9, segments) == 108, "rt_sh9 is 112 B, segments at 108");

/* L2 spherical-harmonic radiance probes at each of the n points: params->samples paths each. */
int rt_radiance_sh(rt_ctx* ctx, const rt_probe* probes, size_t n, const rt_path_params* params, rt_sh9* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Irradiance queries: the cosine-weighted hemispherical gather at surface points the caller supplies, E = integral of L(w) cos(theta)
 * over the hemisphere of the point's normal - what a lightmap texel's or an irradiance-cache record's diffuse response multiplies (no
 * reference counterpart).  It is rt_radiance over directions the device draws itself from the frames' cosine lobe, summed in sample
 * order: the frames' diffuse continuation from that point.  Every bit is fixed by rt_radiance and one f32 statement.
 *
 * rt_irradiance: for point i (its index in the caller's array), position P and normal N as given - N is not renormalised and not
 * flipped; prim_id and material_id are ignored - and sample k < samples:
 *   1. rng = rng_for(seed + i (mod 2^32), first_sample + k), the frames' generator; u1 = next_f32(), u2 = next_f32().
 *   2. the frames' cosine lobe as their diffuse continuation writes it, with dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z and every
 *      operation one f32 rounding, nothing fused:
 *        w = N + unit_vector(u1, u2);  if (dot(w, w) < 1e-12f) w = N;  d_k = w * (1.0f / sqrtf(dot(w, w)));
 *        o = P + N * 0.001f  (per component: the continuation's origin offset).
 *   3. x_k = the radiance rt_radiance gives for the ray {origin = o, tmin = RT_MIN_RAY_DISTANCE, direction = d_k, tmax = FLT_MAX}
 *      with samples = 1, first_sample = first_sample + k, the same seed and ray index i, the same max_bounces and RT_PATH_NO_SHADOWS,
 *      and RT_PATH_CAMERA_DRAWS: the path goes on from the generator's third draw.  g_k = that ray's segments.  A ray that is
 *      degenerate by rt_radiance's own rule (a non-finite component of o or d_k, d_k = 0: only a very large N gives one) contributes
 *      x_k = 0, g_k = 0.
 *   4. out[i].irradiance[c] = (0 + x_0[c] + x_1[c] + ...) * (3.1415927f / (float)samples): an f32 sum from zero in sample order, then
 *      one division and one multiply in that grouping, nothing fused (the estimator pi / samples * sum of L for directions of density
 *      cos(theta) / pi).  out[i].segments = g_0 + g_1 + ... mod 2^32.
 *   5. a point with a non-finite component of P or N, or with N = (0, 0, 0), is no point (rt_ambient_occlusion's rule): nothing is
 *      traced, the irradiance is 0 and segments = 0.  A miss record of rt_surface has a zero normal, so it is no point.
 * What follows:
 *   - the result does not depend on the tree in use (device build, host build, RT_PREPARE_QUALITY_TREE, refitted), the device count,
 *     the kind of memory or the chunking.  Light grids are never looked at.  Any number of lights, as rt_radiance.
 *   - an empty scene gives pi * sky[c] within a relative (samples + 4) * 2^-24, and segments = samples.
 *   - unlike rt_radiance_sh followed by a cosine convolution it is not band-limited, and no light from behind the surface enters it.
 * params: rt_path_params as rt_radiance_sh reads it - samples (directions per point) 1 .. RT_PATH_MAX_SAMPLES; max_bounces 0 ..
 *   RT_MAX_BOUNCES; first_sample + samples <= 2^32; flags RT_PATH_NO_SHADOWS, RT_QUERY_COUNTERS - except RT_PATH_CAMERA_DRAWS, which
 *   is RT_ERR_BAD_ARG: the call spends those two draws itself.  _pad ignored.
 * Buffers, synchronisation and side effects as for rt_radiance_sh: both pointers host memory, or both device memory of one context
 * device (16-byte aligned), anything else is RT_ERR_BAD_ARG; batches are traced in chunks of at most max(1, RT_QUERY_CHUNK / samples)
 * points, host batches staged chunk by chunk; a context over several devices splits a host batch into one contiguous range per device
 * (the seed's i stays the index in the caller's array); synchronous, first waits for an rt_dispatch_tile in flight; the last frame,
 * the rt_read_* results and a running accumulation are left alone.
 * Errors: n == 0 is RT_OK; NULL points / params / out, samples out of range, max_bounces > RT_MAX_BOUNCES, first_sample + samples > 2^32,
 * RT_PATH_CAMERA_DRAWS and unknown flag bits are RT_ERR_BAD_ARG and change nothing; a call before any upload is RT_ERR_NOT_UPLOADED.
 * Statistics: as rt_radiance_sh - rays = all segments, primary_rays = first segments (valid first segments: valid points x samples
 * but for degenerate rays), continuation_rays and shadow_rays as the frames count them, pixels = 0, kernel_ms the maximum over
 * devices, node_visits / tri_tests only with RT_QUERY_COUNTERS.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_irradiance_result {
    float irradiance[3];
    uint32_t segments; /* segments traced for this point over all its samples (first + continuation + shadow), mod 2^32 */
} rt_irradiance_result; /* 16 bytes */

RT_STATIC_ASSERT(sizeof(rt_irradiance_result) == 16 && offsetof(rt_irradiance_result, segments) == 12, "rt_irradiance_result is 16 B, segments at 12");

/* Cosine-weighted path irradiance at each of the n surface points: params->samples paths each. */
int rt_irradiance(rt_ctx* ctx, const rt_surface_point* points, size_t n, const rt_path_params* params, rt_irradiance_result* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Closest-point queries: the nearest point of the scene's surface to points the caller supplies (no reference counterpart; Embree's
 * rtcPointQuery is the model): snapping probes and lightmap texels onto geometry, clearance tests, distance fields.  No ray call can
 * answer it.  The answer is one f32 statement (csrc/closest_point_rules.h; every operation one f32 rounding, nothing fused):
 *
 * Triangle, from its record's v0, e1 = v1 - v0, e2 = v2 - v0 (the f32 differences the ray queries use) and the point p, with
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z:
 *     ap = p - v0;        d1 = dot(e1, ap); d2 = dot(e2, ap)
 *     bp = ap - e1;       d3 = dot(e1, bp); d4 = dot(e2, bp)
 *     cp = ap - e2;       d5 = dot(e1, cp); d6 = dot(e2, cp)
 *     vc = d1*d4 - d3*d2; vb = d5*d2 - d1*d6; va = d3*d6 - d5*d4
 *     the first rule that holds, in this order:
 *       d1 <= 0 && d2 <= 0                         -> (v, w) = (0, 0)
 *       d3 >= 0 && d4 <= d3                        -> (1, 0)
 *       vc <= 0 && d1 >= 0 && d3 <= 0              -> (d1 / (d1 - d3), 0)
 *       d6 >= 0 && d5 <= d6                        -> (0, 1)
 *       vb <= 0 && d2 >= 0 && d6 <= 0              -> (0, d2 / (d2 - d6))
 *       va <= 0 && d4-d3 >= 0 && d5-d6 >= 0        -> w = (d4-d3) / ((d4-d3) + (d5-d6)), v = 1 - w
 *       otherwise                                  -> den = 1 / ((va + vb) + vc), v = vb*den, w = vc*den
 *     r = (e1*v + e2*w) - ap;  dist2 = dot(r, r);  position = v0 + (e1*v + e2*w);  u = v, v = w (the weights of v1 and v2, as rt_hit)
 *   (Ericson, Real-Time Collision Detection 5.1.5.)
 * Sphere i: oc = p - centre; len = sqrtf(dot(oc, oc)); d = fabsf(len - radius); dist2 = d*d;
 *     position = len > 0 ? centre + oc * (radius / len) : centre + (radius, 0, 0); u = v = 0.  The surface, from inside or outside.
 * Order: a candidate is (the bits of dist2, key) as one 64-bit unsigned number, key = prim_id ^ 0x80000000 (rt_intersect_all's key: at
 *   equal dist2 spheres before triangles, each kind by ascending index).  The best starts at (the bits of radius * radius, 0) and a
 *   candidate replaces it iff it is below it.  So only dist2 < radius * radius is ever accepted, strictly; a NaN or infinite dist2
 *   never is (degenerate triangles, triangles with a non-finite vertex, bad spheres).  radius = +inf is allowed.
 * Result: position, distance = sqrtf(dist2), u, v of the winner; prim_id as rt_hit.prim_id; material_id = the record's, not checked
 *   against the material table.  Nothing accepted: position = 0, distance = the radius as given, u = v = 0, prim_id = 0xFFFFFFFF,
 *   material_id = 0.  A query with a non-finite position component, a NaN radius or radius <= 0 is such a miss without a walk.  The
 *   kernel checks this itself.
 * The result follows from these rules alone: it does not depend on the tree in use (device build, host build,
 *   RT_PREPARE_QUALITY_TREE, refitted), the device count, the kind of memory or the chunking, and after rt_update_geometry it is
 *   that of a fresh upload of the moved scene.  The tree only culls, by a lower bound of each box widened past the statement's own
 *   rounding.
 * Buffers, synchronisation and side effects as for rt_intersect: both pointers host memory, or both device memory of one context
 * device (16-byte aligned), anything else is RT_ERR_BAD_ARG; host batches are staged in chunks of at most RT_QUERY_CHUNK points; a
 * context over several devices splits a host batch into one contiguous range per device; synchronous, first waits for an
 * rt_dispatch_tile in flight; the last frame, the rt_read_* results and a running accumulation are left alone.
 * flags: RT_QUERY_COUNTERS.  Statistics: rays = n, the other counts 0, kernel_ms the maximum over devices, node_visits / tri_tests
 * only with RT_QUERY_COUNTERS.
 * Errors: n == 0 is RT_OK; a NULL pointer with n > 0 or unknown flag bits are RT_ERR_BAD_ARG; a call before any upload is
 * RT_ERR_NOT_UPLOADED.  An empty scene gives all misses.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_point_query {
    float position[3];
    float radius; /* only surface strictly nearer than this is reported; > 0, +inf allowed */
} rt_point_query; /* 16 bytes */

typedef struct rt_nearest {
    float position[3];    /* the nearest point of the surface */
    float distance;       /* from the query's position; the radius as given on a miss */
    float u, v;           /* triangle: the weights of v1 and v2 at the point; sphere: 0 */
    uint32_t prim_id;     /* as rt_hit.prim_id; 0xFFFFFFFF = miss */
    uint32_t material_id; /* the record's material id, unchecked; 0 on a miss */
} rt_nearest; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_point_query) == 16 && offsetof(rt_point_query, radius) == 12, "rt_point_query is 16 B, radius at 12");
RT_STATIC_ASSERT(sizeof(rt_nearest) == 32, "rt_nearest is 32 B");
RT_STATIC_ASSERT(offsetof(rt_nearest, distance) == 12 && offsetof(rt_nearest, u) == 16 && offsetof(rt_nearest, v) == 20 &&
                     offsetof(rt_nearest, prim_id) == 24 && offsetof(rt_nearest, material_id) == 28,
                 "rt_nearest offsets");

/* Nearest surface point to each of the n points. */
int rt_closest_point(rt_ctx* ctx, const rt_point_query* points, size_t n, rt_nearest* out, uint32_t flags);

/* Nearest-K: the max_nearest nearest primitives of each of the n points within the query's radius, nearest first, in one walk per
 * point (rtcPointQuery as the collecting query it is: contact manifolds, de-penetration, brushes and selection, cache lookups).
 * rt_closest_point cannot be told to skip the primitive it returned, so no sequence of its calls gives this.
 * Candidates: every sphere s, as (its dist2 above, key s), and every triangle record, as (its dist2 above on the record's v0, e1, e2,
 * key 0x80000000 | prim_id).  A candidate is in range iff (the bits of dist2, key) is below (the bits of radius * radius, 0):
 * dist2 < radius * radius, strictly; a NaN or infinite dist2 never is.  That is rt_closest_point's acceptance.  Every triangle has
 * exactly one record in the tree (the builders never split a triangle), so no primitive is listed twice.
 * Order: ascending (the bits of dist2, key) as one 64-bit unsigned number; at equal dist2 spheres before triangles, spheres by
 * ascending sphere index, triangles by ascending original triangle index.  That is the order in which rt_closest_point's rules
 * would pick a winner: for max_nearest >= 1 point i's first record out[i * max_nearest] is bit for bit the rt_closest_point record
 * of point i.
 * Output: point i's first min(total, max_nearest) candidates in that order as rt_nearest records at out[i * max_nearest ..]
 * (query-major), each the record rt_closest_point would give were that primitive alone in the scene: position, distance =
 * sqrtf(dist2), u, v, prim_id, the record's material_id.  Unused slots are miss records: position = 0, distance = the radius as
 * given, u = v = 0, prim_id = 0xFFFFFFFF, material_id = 0.  max_nearest == 1 gives exactly rt_closest_point's bytes, misses,
 * degenerate queries (all misses and a count of 0 without a walk, the same rules; the kernel checks this itself) and an empty scene
 * included, and with RT_QUERY_COUNTERS its node visits and triangle tests: the walk is culled by the same values at every step.
 * counts[i] = the number of records written for point i; with RT_QUERY_COUNT_ALL instead the number of candidates in range, which
 * can exceed max_nearest (the records written are the same).  The walk can then not shrink its range: it is culled by
 * radius * radius throughout, and RT_QUERY_COUNT_ALL with radius = +inf tests every primitive of the scene for every point.
 * `counts` may be NULL unless max_nearest == 0.  max_nearest == 0 is allowed only with RT_QUERY_COUNT_ALL and a non-NULL counts;
 * `out` is then ignored: a pure count of what lies within the radius.
 * The result follows from these rules alone - it is the max_nearest smallest elements of a totally ordered set - so it does not
 * depend on the tree in use (device build, host build, RT_PREPARE_QUALITY_TREE, refitted), the device count, the kind of memory or
 * the chunking, and after rt_update_geometry it is that of a fresh upload of the moved scene.  The tree only culls, by the bound of
 * rt_closest_point held against the list's last entry once the list is full (csrc/closest_point_all_rules.h).
 * Buffers: each pointer is classified as for the other queries; all are host memory, or all device memory of one context device
 * (points and out 16-byte aligned, counts 4-byte aligned), anything else is RT_ERR_BAD_ARG.  Batches go in chunks of at most
 * RT_QUERY_CHUNK / max(max_nearest, 1) points, so the staged records never exceed those of an rt_closest_point chunk; a context
 * over several devices splits a host batch into one contiguous range per device.
 * Errors: n == 0 is RT_OK; a NULL points, or a NULL out with max_nearest > 0, max_nearest > RT_NEAREST_MAX, max_nearest == 0 without
 * RT_QUERY_COUNT_ALL and counts, and unknown flag bits are RT_ERR_BAD_ARG and change nothing; a call before any upload is
 * RT_ERR_NOT_UPLOADED.  An empty scene gives all misses and counts of 0.
 * Statistics, synchronisation and side effects as for rt_intersect_all: synchronous, first waits for an rt_dispatch_tile in flight;
 * rays = n, the other counts 0, kernel_ms the maximum over devices, node_visits / tri_tests only with RT_QUERY_COUNTERS; the last
 * frame, the rt_read_* results and a running accumulation are left alone. */
#define RT_NEAREST_MAX 16u

int rt_closest_point_all(rt_ctx* ctx, const rt_point_query* points, size_t n, uint32_t max_nearest,
                         rt_nearest* out,   /* n * max_nearest records, query-major: point i's at out[i*max_nearest ..] */
                         uint32_t* counts,  /* n entries; may be NULL unless max_nearest == 0 */
                         uint32_t flags);   /* RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL */

/* ---------------------------------------------------------------------------------------------------------------
 * Inside tests and signed distance: on which side of the surface a point lies, and rt_closest_point's distance with that sign (no
 * reference counterpart; Open3D's RaycastingScene::compute_occupancy / compute_signed_distance is the model): voxelisation, SDF and
 * TSDF baking, seeding particles inside a solid, dropping light probes that landed inside walls, the sign of a de-penetration.  The
 * sign is a majority vote of crossing parities along R fixed directions; the magnitude is rt_closest_point's.  Every bit is fixed by
 * the calls above (csrc/inside_rules.h):
 *
 * Directions: D_0 .. D_6 = RT_INSIDE_DIRECTIONS below, used as given, not normalised: seven roughly unit-length vectors with no zero
 *   component, the same for every point and every call, so that neighbouring points walk the tree coherently, and skewed so that
 *   lattice points send no ray along the edges of axis-aligned or 45-degree tessellations.
 * Vote k of point P: on the ray {origin = P, tmin = RT_MIN_RAY_DISTANCE, direction = D_k, tmax = +inf}, c_k = the number of
 *   TRIANGLE candidates of rt_intersect_all's rule in that range: the frames' Moller-Trumbore on the record's v0, e1, e2 with
 *   tmin < t < tmax, strictly, one record per triangle.  Spheres are not counted.  The vote is c_k & 1.  c_k is a count over all
 *   triangles of the scene and does not depend on the tree: it is counts[] of rt_intersect_all(max_hits = 0, RT_QUERY_COUNT_ALL) for
 *   that ray on the scene without its spheres.
 * Tracing order: k = 0, 1, .., R - 1, R = params->rays, one of 1, 3, 5, 7.  odd = the odd votes so far, even = the even ones.
 *   Without a `votes` array a point stops as soon as its majority is decided: odd * 2 > R or even * 2 > R; the votes not taken
 *   cannot change it.  With a `votes` array all R rays are traced and votes[i] = odd.  tri_inside = odd * 2 > R.
 * Spheres: sphere_inside = some sphere s has dot(oc, oc) < radius * radius, oc = P - centre, dot as in "Closest-point queries", in
 *   f32; tested in index order, before any ray.  Without a `votes` array a point inside a sphere traces no ray.
 * Result: inside = sphere_inside || tri_inside: the union of the solids.
 * rt_inside reads the position only; the record's radius is ignored, NaN included.  A non-finite position component gives
 *   inside = 0 and votes = 0 with nothing traced.
 * rt_signed_distance: out[i] is rt_closest_point's record of point i bit for bit, and when the point is inside the sign bit of
 *   `distance` is set.  That holds on a miss within a finite radius too: distance = -radius, the truncated field, so that a TSDF bake
 *   keeps its cheap bounded walk.  A degenerate query by rt_closest_point's rules (a non-finite position component, a NaN radius,
 *   radius <= 0) gives its unsigned miss record and votes = 0 without any walk.
 * Limits: the answer means something only where the triangles form a watertight surface; neither orientation nor shared indices are
 *   needed.  votes strictly between 0 and R is how a caller sees that the surface is not watertight around a point, or that a ray
 *   grazed an edge.  Moller-Trumbore rejects |det| < 1e-5, so a triangle whose doubled area projected along D_k is below that is
 *   transparent to vote k, as it is to the frames; and a point within 1e-5 of the surface along a ray can miss that crossing.
 * The result follows from these rules alone: it does not depend on the tree in use (device build, host build,
 *   RT_PREPARE_QUALITY_TREE, refitted), the device count, the kind of memory or the chunking.
 * Buffers, chunking, the split over devices, synchronisation, errors and side effects as for rt_closest_point_all: each pointer is
 * classified as for the other queries; all are host memory, or all device memory of one context device (points and the rt_nearest
 * records 16-byte aligned; the byte arrays `inside` and `votes` 1-byte aligned), anything else is RT_ERR_BAD_ARG.  Batches go in
 * chunks of at most RT_QUERY_CHUNK / rays points; a context over several devices splits a host batch into one contiguous range per
 * device; synchronous, first waits for an rt_dispatch_tile in flight; the last frame, the rt_read_* results and a running
 * accumulation are left alone.
 * Errors: n == 0 is RT_OK; a NULL points, params or inside / out with n > 0, rays not in {1, 3, 5, 7} and flag bits other than
 * RT_QUERY_COUNTERS are RT_ERR_BAD_ARG and change nothing; a call before any upload is RT_ERR_NOT_UPLOADED.  An empty scene gives
 * inside = 0, votes = 0 and miss records; a scene of spheres alone works.
 * Statistics: rays = the parity rays actually traced, counted on the device: n_valid * R with `votes`, fewer without; the other
 * counts 0; kernel_ms the maximum over devices; node_visits / tri_tests only with RT_QUERY_COUNTERS, summed over the closest-point
 * walk and the ray walks.
 * --------------------------------------------------------------------------------------------------------------- */
#define RT_INSIDE_MAX_RAYS 7u
#define RT_INSIDE_DIRECTIONS \
    { 0.5377f,  0.7431f,  0.3982f}, {-0.6241f,  0.3517f,  0.6977f}, { 0.2893f, -0.4719f,  0.8328f}, \
    {-0.3361f, -0.8154f, -0.4703f}, { 0.8467f, -0.2249f, -0.4821f}, {-0.1873f,  0.5566f, -0.8094f}, \
    { 0.4129f,  0.1683f, -0.8951f}

typedef struct rt_inside_params {
    uint32_t rays;  /* R: 1, 3, 5 or 7 */
    uint32_t flags; /* RT_QUERY_COUNTERS */
    uint32_t _pad[2];
} rt_inside_params; /* 16 bytes */

RT_STATIC_ASSERT(sizeof(rt_inside_params) == 16 && offsetof(rt_inside_params, flags) == 4, "rt_inside_params is 16 B, flags at 4");

int rt_inside(rt_ctx* ctx, const rt_point_query* points, size_t n, const rt_inside_params* params,
              uint8_t* inside, /* n entries: 1 inside, 0 outside */
              uint8_t* votes); /* n entries: the odd votes of all R rays; may be NULL */

int rt_signed_distance(rt_ctx* ctx, const rt_point_query* points, size_t n, const rt_inside_params* params,
                       rt_nearest* out, /* n records: rt_closest_point's, the sign bit of distance set when inside */
                       uint8_t* votes); /* n entries: the odd votes of all R rays; may be NULL */

/* ---------------------------------------------------------------------------------------------------------------
 * Sphere sweeps: the first contact of a moving sphere with the scene's surface (no reference counterpart; the "sphere cast" of the
 * collision libraries is the model): camera and character collision, pushing a probe along a direction until it has clearance,
 * clearance along a path, thick-ray visibility.  A ray is not conservative for a body with extent, and stepping rt_closest_point
 * along the segment misses thin contacts between steps.  The sphere's centre moves as centre(t) = origin + direction * t; the answer
 * is the smallest t in [0, tmax) at which it lies within `radius` of the surface, and the point of the surface it touches there.
 * The surface is two-sided and a sphere primitive is its surface, as for rt_closest_point.  The answer is one f32 statement
 * (csrc/sweep_rules.h; every operation one f32 rounding, nothing fused), with dot as in "Closest-point queries",
 * cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), c = origin, d = direction, r = radius, rr = r*r,
 * dd = dot(d, d).  The candidate time of a primitive is the minimum, by value, of the pieces below that accept (a -0 counts as +0);
 * a NaN never accepts.  The pieces are the first entry into the primitive's Minkowski sum with the ball.
 *
 * Triangle, from its record's v0, e1, e2; ap = c - v0:
 *   Overlap at the start: the closest-point statement's dist2 of the triangle from c is <= rr               -> t = 0
 *   Face: n = cross(e1, e2); nn = dot(n, n); ln = sqrtf(nn); h = dot(n, ap); nd = dot(n, d); s = h < 0 ? -1 : 1
 *       num = fabsf(h) - r*ln; den = -(s*nd); t = num / den; k = s*r / ln; q = (ap + d*t) - n*k  (per component)
 *       fv = dot(cross(q, e2), n) / nn; fw = dot(cross(e1, q), n) / nn
 *       accepts iff num >= 0 && den > 0 && fv >= 0 && fw >= 0 && fv + fw <= 1
 *   Vertices a in (0, e1, e2): m = ap - a; b = dot(m, d); x = cross(m, d); disc = dd*rr - dot(x, x); t = (-b - sqrtf(disc)) / dd
 *       accepts iff disc >= 0 && t >= 0
 *   Edges (a, e) in ((0, e1), (0, e2), (e1, e2 - e1)): m = ap - a; g = cross(e, d); p = cross(g, e)
 *       A = dot(g, g); B = dot(m, p); h = dot(m, g); ee = dot(e, e); disc = rr*A - h*h; t = (-B - sqrtf(ee*disc)) / A
 *       sp = (dot(m, e) + t*dot(d, e)) / ee
 *       accepts iff A > 0 && disc >= 0 && t >= 0 && 0 <= sp && sp <= 1
 *     The cylinder's caps and the prism's sides lie inside the vertex balls and the cylinders, so these pieces give the exact first
 *     contact.  disc is b*b - dd*(dot(m, m) - rr) and (B*B - A*C) / ee of the usual quadratics, in the form that does not cancel two
 *     terms of the size |m|^2 to get at r^2.
 * Sphere i (centre o, radius R): m = c - o; len = sqrtf(dot(m, m)); b = dot(m, d); x = cross(m, d); xx = dot(x, x)
 *   fabsf(len - R) <= r                                                                                        -> t = 0
 *   otherwise len > R (from outside):  rs = R + r; disc = dd*(rs*rs) - xx; t = (-b - sqrtf(disc)) / dd  (the entering root)
 *   otherwise (from inside):           rs = R - r; disc = dd*(rs*rs) - xx; t = (-b + sqrtf(disc)) / dd  (the leaving root)
 *   both accept iff disc >= 0 && t >= 0
 * Order: a candidate is (the bits of t, key) as one 64-bit unsigned number, key = prim_id ^ 0x80000000 as for rt_closest_point.  The
 *   best starts at (the bits of tmax, 0) and a candidate replaces it iff it is below it.  So only t < tmax is ever accepted,
 *   strictly; at equal t spheres come before triangles, each kind by ascending index.  Among several primitives in contact at the
 *   start (all of them t = 0) the LOWEST KEY wins, not the nearest.
 * Result: t of the winner; position, u, v are the closest-point statement of the winner alone, evaluated at
 *   centre = c + d*t (per component c_a + d_a*t).  So a contact at t = 0 carries exactly the point rt_closest_point computes for
 *   that primitive from `origin`.  The contact normal is centre - position; the caller computes it.  prim_id as rt_hit.prim_id;
 *   material_id = the record's, unchecked.  A miss: position = 0, t = tmax as given, u = v = 0, prim_id = 0xFFFFFFFF, material_id = 0.
 *   A query with a non-finite origin or direction component, a zero direction, a radius that is NaN, <= 0 or infinite, or a tmax that
 *   is NaN or <= 0 is such a miss without a walk.  The kernel checks this itself.
 * The result follows from these rules alone: it does not depend on the tree in use, the device count, the kind of memory or the
 *   chunking, and after rt_update_geometry it is that of a fresh upload of the moved scene.  The tree only culls, by the ray's entry
 *   time into each box widened by the radius and a margin past the statement's own rounding.
 * Buffers, synchronisation and side effects as for rt_closest_point: both pointers host memory, or both device memory of one context
 * device (16-byte aligned), anything else is RT_ERR_BAD_ARG; host batches are staged in chunks of at most RT_QUERY_CHUNK sweeps; a
 * context over several devices splits a host batch into one contiguous range per device; synchronous, first waits for an
 * rt_dispatch_tile in flight; the last frame, the rt_read_* results and a running accumulation are left alone.
 * flags: RT_QUERY_COUNTERS.  Statistics: rays = n, the other counts 0, kernel_ms the maximum over devices, node_visits / tri_tests
 * only with RT_QUERY_COUNTERS.
 * Errors: n == 0 is RT_OK; a NULL pointer with n > 0 or unknown flag bits are RT_ERR_BAD_ARG; a call before any upload is
 * RT_ERR_NOT_UPLOADED.  An empty scene gives all misses.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_sweep {  /* rt_ray's layout with the radius where tmin is */
    float origin[3];       /* the sphere's centre at t = 0 */
    float radius;          /* > 0, finite */
    float direction[3];    /* need not be normalised; centre(t) = origin + direction * t */
    float tmax;            /* contacts at 0 <= t < tmax are reported; > 0, +inf allowed */
} rt_sweep; /* 32 bytes */

typedef struct rt_sweep_hit { /* rt_nearest's layout with t where distance is */
    float position[3];    /* the point of the surface the sphere touches */
    float t;              /* time of first contact; tmax as given on a miss */
    float u, v;           /* triangle: the weights of v1 and v2 at `position`; sphere: 0 */
    uint32_t prim_id;     /* as rt_hit.prim_id; 0xFFFFFFFF = miss */
    uint32_t material_id; /* the record's material id, unchecked; 0 on a miss */
} rt_sweep_hit; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_sweep) == 32 && offsetof(rt_sweep, origin) == 0 && offsetof(rt_sweep, radius) == 12 &&
                     offsetof(rt_sweep, direction) == 16 && offsetof(rt_sweep, tmax) == 28,
                 "rt_sweep is 32 B: origin, radius at 12, direction at 16, tmax at 28");
RT_STATIC_ASSERT(sizeof(rt_sweep_hit) == 32 && offsetof(rt_sweep_hit, position) == 0 && offsetof(rt_sweep_hit, t) == 12 &&
                     offsetof(rt_sweep_hit, u) == 16 && offsetof(rt_sweep_hit, v) == 20 && offsetof(rt_sweep_hit, prim_id) == 24 &&
                     offsetof(rt_sweep_hit, material_id) == 28,
                 "rt_sweep_hit is 32 B: position, t at 12, u, v, prim_id at 24, material_id at 28");

/* First contact of each of the n moving spheres. */
int rt_sweep_sphere(rt_ctx* ctx, const rt_sweep* sweeps, size_t n, rt_sweep_hit* out, uint32_t flags);

/* ---------------------------------------------------------------------------------------------------------------
 * Box sweeps: the first contact of a moving axis-aligned box with the scene's surface (no reference counterpart; the "box cast" of
 * the collision libraries is the model): character and camera controllers with box or voxel hulls, continuous collision of a fast
 * body, clearance of a crate-shaped probe along a path, conservative advancement of a trigger volume.  rt_sweep_sphere with the
 * circumscribed sphere reports contacts the box never makes and with the inscribed one misses contacts; stepping rt_overlap_box along
 * the path tunnels through thin geometry and gives no time.  The box keeps its orientation and its centre moves as
 * centre(t) = center + direction * t; the answer is the smallest t in [0, tmax) at which the closed box touches the surface, with the
 * contact's normal and the separating axis that closed last.  The surface is two-sided and a sphere primitive is its surface, as for
 * rt_overlap_box.  The answer is one f32 statement (csrc/sweep_box_rules.h, whose header comment is the specification; every
 * operation one f32 rounding, nothing fused), with dot, cross, min and max as in "Overlap queries", c = center, h = half_extent,
 * d = direction, and every test in its positive form, so that a NaN makes it false.
 * Triangle, from its record's v0, e1, e2; a0 = v0 - c, a1 = (v0 + e1) - c, a2 = (v0 + e2) - c: the thirteen axes of "Overlap queries",
 *   numbered 0, 1, 2 the box axes x, y, z; 3 the normal n = cross(e1, e2); 4 + 3j + i cross(unit_i, f_j), f = (e1, e2 - e1, e2).  Per
 *   axis p_k and r are the overlap statement's (for the normal p_0 = p_1 = p_2 = dot(n, a0)) and w is the projection of d in the form
 *   of p_k (d[a]; dot(n, d); f.y*d.z - f.z*d.y, f.z*d.x - f.x*d.z, f.x*d.y - f.y*d.x).  lo = min_k p_k - r, hi = max_k p_k + r;
 *     w > 0: enter = lo / w, exit = hi / w;   w < 0: enter = hi / w, exit = lo / w;   the axis holds iff enter <= exit
 *     w == 0: the axis holds iff min_k p_k <= r && max_k p_k >= -r and constrains nothing;   w a NaN: it does not hold
 *     an axis 4..12 holds only if (p_0 + p_1) + p_2 is no NaN
 *   The running entry starts at (t_in = 0, RT_SWEEP_AXIS_NONE); an axis replaces it iff its enter is strictly larger; t_out is the
 *   minimum of the exits, from +inf.  Contact iff all nine components of the a_k are finite, every axis holds and t_in <= t_out; then
 *   t = t_in + 0.0f and axis is the one that set t_in.  t = 0 with RT_SWEEP_AXIS_NONE results exactly when the triangle touches the
 *   box at the start by the statement of rt_overlap_box.
 *   normal_a = (w > 0 ? -L_a : L_a) / sqrtf(dot(L, L)) + 0.0f for that axis' vector L (unit_a; n; (0, -f.z, f.y), (f.z, 0, -f.x),
 *   (-f.y, f.x, 0)) and its w; 0 for RT_SWEEP_AXIS_NONE.
 * Sphere i (centre o, radius R, rr = R*R): g = o - c; seen from the box its centre is P(t), P_a(t) = g_a - d_a*t; near and far as in
 *   "Overlap queries".
 *   touching at the start by the statement of rt_overlap_box                                            -> t = 0
 *   otherwise dot(near, near) > rr (from outside), the minimum over the accepting pieces of the box widened by the ball:
 *     faces, per axis a with d_a != 0: plane = h_a + R; t = (g_a - (d_a > 0 ? plane : -plane)) / d_a
 *       accepts iff t >= 0 && |P_b(t)| <= h_b && |P_c(t)| <= h_c on the other two axes
 *     edges along a, (b, c) = (a + 1, a + 2) mod 3, four signs: m_b = g_b -+ h_b, m_c = g_c -+ h_c; dd2 = d_b*d_b + d_c*d_c
 *       bq = m_b*d_b + m_c*d_c; x = m_b*d_c - m_c*d_b; disc = dd2*rr - x*x; t = (bq - sqrtf(disc)) / dd2
 *       accepts iff disc >= 0 && t >= 0 && |P_a(t)| <= h_a
 *     corners, eight signs: m = g -+ h; b = dot(m, d); x = cross(m, d); disc = dot(d, d)*rr - dot(x, x)
 *       t = (b - sqrtf(disc)) / dot(d, d);  accepts iff disc >= 0 && t >= 0
 *   otherwise dot(far, far) < rr (from inside): the minimum over the eight corners of t = (b + sqrtf(disc)) / dot(d, d), accepted
 *     iff disc >= 0 && t >= 0
 *   t is that minimum + 0.0f.  A contact at t > 0 has axis RT_SWEEP_AXIS_SPHERE and, with P = P(t), the normal v / sqrtf(dot(v, v))
 *   for v = clamp(P, -h, h) - P from outside and v = P - corner, corner_a = (P_a >= 0 ? -h_a : h_a), from inside; 0 where that length
 *   is not > 0.  A contact at t = 0 has RT_SWEEP_AXIS_NONE and normal 0.
 * Order: as for rt_sweep_sphere: (the bits of t, key) as one 64-bit unsigned number from (the bits of tmax, 0).  Only t < tmax is ever
 *   accepted, strictly; at equal t spheres come before triangles, each kind by ascending index; among several primitives in contact
 *   at the start the lowest key wins.
 * A miss: normal 0, t = tmax as given, axis RT_SWEEP_AXIS_NONE, prim_id 0xFFFFFFFF, material_id 0.  A query with a non-finite
 *   component of center, half_extent or direction, a negative half extent, a zero direction, or a tmax that is NaN or <= 0 is such a
 *   miss without a walk.  The kernel checks this itself.
 * The result follows from these rules alone: it does not depend on the tree in use, the device count, the kind of memory or the
 *   chunking, and after rt_update_geometry it is that of a fresh upload of the moved scene.  The tree only culls, by the centre's
 *   entry time into each box widened by the half extents and a margin past the statement's own rounding.
 * Buffers, chunking, the split over devices, synchronisation, side effects, flags, statistics and errors as for rt_sweep_sphere; the
 * records are 48 bytes in and 32 bytes out, device memory 16-byte aligned.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_box_sweep {  /* its first 32 bytes are an rt_box, its last 16 the second half of an rt_sweep */
    float center[3];       /* the box's centre at t = 0 */
    uint32_t _pad0;        /* pads are ignored */
    float half_extent[3];  /* >= 0 per axis, finite; 0 allowed (a moving slab, segment, point) */
    uint32_t _pad1;
    float direction[3];    /* need not be normalised; centre(t) = center + direction * t */
    float tmax;            /* contacts at 0 <= t < tmax are reported; > 0, +inf allowed */
} rt_box_sweep; /* 48 bytes */

typedef struct rt_box_sweep_hit {
    float normal[3];       /* unit, against the motion; 0 on a miss and for a start in contact */
    float t;               /* time of first contact; tmax as given on a miss */
    uint32_t axis;         /* which separating axis closed last: 0 .. 12, RT_SWEEP_AXIS_SPHERE or RT_SWEEP_AXIS_NONE */
    uint32_t _reserved;    /* written as 0 */
    uint32_t prim_id;      /* as rt_hit.prim_id; 0xFFFFFFFF = miss */
    uint32_t material_id;  /* the record's material id, unchecked; 0 on a miss */
} rt_box_sweep_hit; /* 32 bytes */

#define RT_SWEEP_AXIS_SPHERE 13u
#define RT_SWEEP_AXIS_NONE 0xFFFFFFFFu

RT_STATIC_ASSERT(sizeof(rt_box_sweep) == 48 && offsetof(rt_box_sweep, center) == 0 && offsetof(rt_box_sweep, half_extent) == 16 &&
                     offsetof(rt_box_sweep, direction) == 32 && offsetof(rt_box_sweep, tmax) == 44,
                 "rt_box_sweep is 48 B: center, half_extent at 16, direction at 32, tmax at 44");
RT_STATIC_ASSERT(sizeof(rt_box_sweep_hit) == 32 && offsetof(rt_box_sweep_hit, normal) == 0 && offsetof(rt_box_sweep_hit, t) == 12 &&
                     offsetof(rt_box_sweep_hit, axis) == 16 && offsetof(rt_box_sweep_hit, prim_id) == 24 &&
                     offsetof(rt_box_sweep_hit, material_id) == 28,
                 "rt_box_sweep_hit is 32 B: normal, t at 12, axis at 16, prim_id at 24, material_id at 28");

/* First contact of each of the n moving boxes. */
int rt_sweep_box(rt_ctx* ctx, const rt_box_sweep* sweeps, size_t n, rt_box_sweep_hit* out, uint32_t flags); /* RT_QUERY_COUNTERS */

/* ---------------------------------------------------------------------------------------------------------------
 * Capsule sweeps: the first contact of a moving capsule with the scene's surface (no reference counterpart; the "capsule cast" of
 * the collision libraries is the model): the body that character and camera controllers move.  A chain of rt_sweep_sphere calls
 * along the axis misses what passes between the spheres, rt_sweep_box with the capsule's bounding box reports contacts at corners
 * the rounded body never makes, and one fat sphere is wrong by the length of the body.  The capsule is every point within radius of
 * the segment A(t) .. B(t), A(t) = origin + direction * t, B(t) = A(t) + axis; it keeps its orientation.  The answer is the smallest
 * t in [0, tmax) at which it touches the surface, the point of the primitive in contact and the place s on the axis (0 at A, 1 at
 * B) nearest to it.  The surface is two-sided and a sphere primitive is its surface, as for rt_sweep_sphere.  The answer is one f32
 * statement (csrc/sweep_capsule_rules.h, whose header comment is the specification; every operation one f32 rounding, nothing
 * fused), built from the pieces of "Sphere sweeps" (the pushed-out face, sw_vertex, sw_edge) with r = radius, d = direction:
 * Closest pair cap_triangle(v0, e1, e2, P, axis) -> dist2, s, v, w of the axis segment from P and a triangle: the first candidate
 *   with the strictly smallest dist2 of: end P by the closest-point statement (s = 0); end P + axis (s = 1); the axis against the
 *   edges (v0, e1), (v0, e2), (v0 + e1, e2 - e1) as two clamped segments, each only if dot(axis, axis) > 0 and dot(e, e) > 0; the
 *   axis piercing the triangle (dist2 = 0), only if dot(axis, axis) > 0, the ends' heights over the plane have strictly opposite
 *   signs and the crossing point's weights satisfy v >= 0, w >= 0, v + w <= 1.
 * Triangle: cap_triangle at the start <= r * r -> t = 0.  Otherwise, with ap_k = A - v_k and mB_k = ap_k + axis, the minimum over the
 *   accepting pieces of: the seven pieces of "Sphere sweeps" from ap_k (end A); the same seven from mB_k (end B); the cylinder wall
 *   against the vertices, sw_edge(mB_k, axis), k = 0, 1, 2; the cylinder wall against the edges, the face piece on (mB_0, e1, axis),
 *   (mB_0, e2, axis), (mB_1, e2 - e1, axis) accepted as a parallelogram (both weights in [0, 1]); t is that minimum + 0.0f.
 * Sphere i (centre C, radius R): dmin the distance of C from the axis segment, dmax the larger of the ends' distances.
 *   dmin - R <= r && R - dmax <= r -> t = 0.  From outside (dmin > R): the minimum of the two ends' entering roots and the cylinder's
 *   (sw_edge's form) against R + r.  Otherwise: the smaller of the two ends' leaving roots against R - r.
 * The hit: for a triangle s, v, w = cap_triangle at P = origin + direction * t (per component) and position = v0 + (e1 v + e2 w); for
 *   a sphere s is the clamped foot of C on the axis at that pose from outside, the end farther from C (A on a tie) from inside, and
 *   position the nearest point of the sphere to that axis point.  A contact at t = 0 carries the closest pair of the start pose.
 * With axis == 0 exactly the call returns rt_sweep_sphere's t, position, prim_id and material_id bit for bit, with s = 0.
 * Order: as for rt_sweep_sphere: (the bits of t, key) as one 64-bit unsigned number from (the bits of tmax, 0).  Only t < tmax is ever
 *   accepted, strictly; at equal t spheres come before triangles, each kind by ascending index.
 * A miss: position 0, t = tmax as given, s = 0, prim_id 0xFFFFFFFF, material_id 0.  A query with a non-finite component of origin,
 *   axis or direction, a zero direction, a radius that is NaN, <= 0 or infinite, or a tmax that is NaN or <= 0 is such a miss
 *   without a walk.  The kernel checks this itself.
 * The result follows from these rules alone: it does not depend on the tree in use, the device count, the kind of memory or the
 *   chunking, and after rt_update_geometry it is that of a fresh upload of the moved scene.  The tree only culls, by the entry time
 *   of the centre of the capsule's bounding box into each child box widened by that box's half extents and a margin past the
 *   statement's own rounding; the bound is loose for a long diagonal capsule.
 * Buffers, chunking, the split over devices, synchronisation, side effects, flags, statistics and errors as for rt_sweep_sphere; the
 * records are 48 bytes in and 32 bytes out, device memory 16-byte aligned.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_capsule_sweep {  /* an rt_sweep with 16 bytes inserted at offset 16 */
    float origin[3];       /* end A of the axis at t = 0 */
    float radius;          /* > 0, finite */
    float axis[3];         /* B - A; zero allowed (a moving sphere) */
    uint32_t _pad;         /* ignored */
    float direction[3];    /* need not be normalised; A(t) = origin + direction * t */
    float tmax;            /* contacts at 0 <= t < tmax are reported; > 0, +inf allowed */
} rt_capsule_sweep; /* 48 bytes */

typedef struct rt_capsule_sweep_hit {
    float position[3];     /* the point of the primitive in contact; 0 on a miss */
    float t;               /* time of first contact; tmax as given on a miss */
    float s;               /* where on the axis the contact is nearest: 0 at A .. 1 at B; 0 on a miss */
    uint32_t _reserved;    /* written as 0 */
    uint32_t prim_id;      /* as rt_hit.prim_id; 0xFFFFFFFF = miss */
    uint32_t material_id;  /* the record's material id, unchecked; 0 on a miss */
} rt_capsule_sweep_hit; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_capsule_sweep) == 48 && offsetof(rt_capsule_sweep, origin) == 0 && offsetof(rt_capsule_sweep, radius) == 12 &&
                     offsetof(rt_capsule_sweep, axis) == 16 && offsetof(rt_capsule_sweep, direction) == 32 && offsetof(rt_capsule_sweep, tmax) == 44,
                 "rt_capsule_sweep is 48 B: origin, radius at 12, axis at 16, direction at 32, tmax at 44");
RT_STATIC_ASSERT(sizeof(rt_capsule_sweep_hit) == 32 && offsetof(rt_capsule_sweep_hit, position) == 0 && offsetof(rt_capsule_sweep_hit, t) == 12 &&
                     offsetof(rt_capsule_sweep_hit, s) == 16 && offsetof(rt_capsule_sweep_hit, prim_id) == 24 &&
                     offsetof(rt_capsule_sweep_hit, material_id) == 28,
                 "rt_capsule_sweep_hit is 32 B: position, t at 12, s at 16, prim_id at 24, material_id at 28");

/* First contact of each of the n moving capsules. */
int rt_sweep_capsule(rt_ctx* ctx, const rt_capsule_sweep* sweeps, size_t n, rt_capsule_sweep_hit* out, uint32_t flags); /* RT_QUERY_COUNTERS */

/* ---------------------------------------------------------------------------------------------------------------
 * Overlap queries: the primitives that touch caller-supplied axis-aligned boxes (no reference counterpart; the OverlapBox /
 * contactTest of the collision libraries and the triangle-box test behind surface voxelisers are the model): the shell of a
 * voxelisation (rt_inside gives the solid), marquee and brush selection, trigger volumes and broad phase, "is this probe cell
 * empty".  rt_closest_point_all with the box's circumscribed sphere lists at most RT_NEAREST_MAX ids, pays a closest-point
 * evaluation per candidate and over-reports by the volume ratio of sphere to box, without bound for a slab.
 * The answer is one f32 statement (csrc/overlap_rules.h; every operation one f32 rounding, nothing fused), with dot and cross as
 * in "Sphere sweeps", c = center, h = half_extent, and every test in its positive form, so that a NaN makes it false.  A primitive
 * TOUCHES the box iff all its tests hold.
 * Triangle, from its record's v0, e1, e2; a0 = v0 - c, a1 = (v0 + e1) - c, a2 = (v0 + e2) - c (Akenine-Moeller 2001, thirteen axes):
 *   0. all nine components of a0, a1, a2 are finite: a triangle with a non-finite vertex is never listed
 *   1. per axis x, y, z:  min_k a_k[x] <= h[x] && max_k a_k[x] >= -h[x]
 *   2. n = cross(e1, e2); d = dot(n, a0); r = dot(|n|, h):  d <= r && d >= -r
 *   3. for f in (e1, e2 - e1, e2) and each unit axis, cross(unit, f) without its multiplications by 0 and 1:
 *        x:  p_k = f.y * a_k.z - f.z * a_k.y;  r = |f.z| * h.y + |f.y| * h.z
 *        y:  p_k = f.z * a_k.x - f.x * a_k.z;  r = |f.z| * h.x + |f.x| * h.z
 *        z:  p_k = f.x * a_k.y - f.y * a_k.x;  r = |f.y| * h.x + |f.x| * h.y
 *      min_k p_k <= r && max_k p_k >= -r, and (p_0 + p_1) + p_2 is not a NaN (min and max themselves ignore a NaN operand)
 *   The box is closed: a triangle that only touches a face, an edge or a corner is listed, one that lies an ulp outside is not.  A
 *   degenerate triangle comes out as the segment or point test.
 * Sphere i (centre o, radius R), a surface as for rt_closest_point: g = |o - c| per axis; near = max(g - h, 0); far = g + h;
 *   rr = R * R; touches iff dot(near, near) <= rr && dot(far, far) >= rr.  A box wholly inside the ball is not touched.
 * A degenerate query - a non-finite component of center or half_extent, or a negative half extent - touches nothing, without a
 *   walk.  The kernel checks this itself.  half_extent = 0 on an axis is allowed: a slab, a segment, a point.
 * Order: key = prim_id ^ 0x80000000 as for rt_closest_point: spheres first by sphere index, then triangles by original triangle
 *   index.
 * List mode (flags without RT_QUERY_COUNT_ALL and RT_OVERLAP_ANY): box i's min(total, max_prims) touching primitives of lowest key,
 *   ascending in key, as ids in rt_hit.prim_id's encoding at prims[i * max_prims ..] (query-major); unused slots are 0xFFFFFFFF.
 *   counts[i] = the number written; `counts` may be NULL.  1 <= max_prims <= RT_OVERLAP_MAX.
 * RT_QUERY_COUNT_ALL: the same ids; counts[i] = the number of all touching primitives, which can exceed max_prims.  max_prims == 0
 *   is allowed with it, needs a non-NULL counts and ignores `prims`: a pure count.
 * RT_OVERLAP_ANY: requires max_prims == 0 and a non-NULL counts, and excludes RT_QUERY_COUNT_ALL; counts[i] = 1 if anything touches
 *   box i, else 0.  The walk stops at the first touching primitive; which one that is depends on the tree, so it is not reported.
 *   This is the fast occupancy path.
 * The result follows from these rules alone, so it does not depend on the tree in use (device build, host build,
 *   RT_PREPARE_QUALITY_TREE, refitted), the device count, the kind of memory or the chunking, and after rt_update_geometry it is that
 *   of a fresh upload of the moved scene.  The tree only culls: a child box is skipped when it lies further from the query box on
 *   some axis than a margin past the statement's own rounding.  The list gives no spatial bound - a key says
 *   nothing about where its primitive lies - so list mode and RT_QUERY_COUNT_ALL both visit every node the box reaches, and a box
 *   that spans the scene tests every primitive of it, as RT_QUERY_COUNT_ALL with radius = +inf does for rt_closest_point_all; a full
 *   list only spares the test of a record whose key is above its last entry's.
 * Buffers, chunking, the split over devices, synchronisation, side effects and statistics as for rt_closest_point_all: the three
 *   pointers are all host memory or all device memory of one context device (boxes 16-byte aligned, prims and counts 4-byte
 *   aligned), anything else is RT_ERR_BAD_ARG; batches go in chunks of at most RT_QUERY_CHUNK / max(max_prims, 1) boxes; a context
 *   over several devices splits a host batch into one contiguous range per device; synchronous, first waits for an rt_dispatch_tile
 *   in flight; rays = n, the other counts 0, kernel_ms the maximum over devices, node_visits / tri_tests (the records read) only
 *   with RT_QUERY_COUNTERS; the last frame, the rt_read_* results and a running accumulation are left alone.
 * Errors: n == 0 is RT_OK; a NULL boxes, or a NULL prims with max_prims > 0, max_prims > RT_OVERLAP_MAX, max_prims == 0 without
 *   RT_QUERY_COUNT_ALL or RT_OVERLAP_ANY and counts, RT_OVERLAP_ANY with max_prims > 0 or with RT_QUERY_COUNT_ALL, and unknown flag
 *   bits are RT_ERR_BAD_ARG and change nothing; a call before any upload is RT_ERR_NOT_UPLOADED.  An empty scene gives counts of 0
 *   and ids of 0xFFFFFFFF.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_box {      /* an axis-aligned box, closed */
    float center[3];
    uint32_t _pad0;          /* pads are ignored */
    float half_extent[3];    /* >= 0 per axis; 0 is allowed (a slab, a segment, a point) */
    uint32_t _pad1;
} rt_box; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_box) == 32 && offsetof(rt_box, center) == 0 && offsetof(rt_box, _pad0) == 12 && offsetof(rt_box, half_extent) == 16 &&
                     offsetof(rt_box, _pad1) == 28,
                 "rt_box is 32 B: center, _pad0 at 12, half_extent at 16, _pad1 at 28");

#define RT_OVERLAP_MAX 32u
#define RT_OVERLAP_ANY 4u   /* rt_overlap_box, rt_overlap_obb and rt_overlap_triangle only: counts[i] = 1 if anything touches box i, else 0; stops at the first */

int rt_overlap_box(rt_ctx* ctx, const rt_box* boxes, size_t n, uint32_t max_prims,
                   uint32_t* prims,   /* n * max_prims ids, query-major, rt_hit.prim_id's encoding; unused slots 0xFFFFFFFF */
                   uint32_t* counts,  /* n entries; may be NULL unless max_prims == 0 */
                   uint32_t flags);   /* RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL | RT_OVERLAP_ANY */

/* ---------------------------------------------------------------------------------------------------------------
 * Contact queries: the primitives a RESTING capsule touches (no reference counterpart; computePenetration / the contact manifold
 * and CheckCapsule / CheckSphere of the collision libraries are the model): what a character or camera controller pushes out of on
 * every step, and "is this pose free".  rt_sweep_capsule answers t = 0 for a capsule that starts in contact and names one primitive,
 * the lowest key and not the deepest; rt_overlap_box with the bounding box over-reports at the corners; a chain of
 * rt_closest_point_all calls along the axis misses what lies between the points and lists a primitive once per point.
 * The capsule is every point within radius of the segment A .. B, A = origin, B = origin + axis.  For each capsule the call lists
 * the max_contacts nearest primitives whose distance from the axis segment is below the radius, nearest first, each with the point
 * of the primitive, the distance and the place s on the axis (0 at A, 1 at B), so that
 *   normal = ((origin + axis * s) - position) / distance,   depth = radius - distance
 * give the push-out.  The surface is two-sided and a sphere primitive is its surface.  The answer is one f32 statement
 * (csrc/contact_capsule_rules.h, whose header comment is the specification; every operation one f32 rounding, nothing fused):
 * Triangle, from its record's v0, e1, e2: dist2, s, v, w = cap_triangle(v0, e1, e2, origin, axis) of "Capsule sweeps";
 *   position = v0 + (e1 v + e2 w).  An axis that pierces the triangle has dist2 = 0.
 * Sphere i (centre C, radius R): dmin the distance of C from the axis segment with its clamped foot f, lenA and lenB the ends'
 *   distances and dmax the larger, as in "Capsule sweeps".  The first that holds:
 *     outside,        dmin > R:                d = dmin - R, s = f
 *     wholly inside,  dmax < R:                d = R - dmax, s = the end farther from C, A on a tie
 *     crossing,       dmin <= R && R <= dmax:  d = 0, s = the smallest root in [0, 1] of |A - C + axis s| = R: with mA = A - C,
 *                     b = dot(mA, axis), c = dot(mA, mA) - R * R, disc = b * b - aa * c, q = disc > 0 ? sqrtf(disc) : 0,
 *                     s = aa > 0 ? clamp((lenA > R ? -b - q : q - b) / aa) : 0
 *   and dist2 = d * d; none holds for a NaN centre or radius, and dist2 is a NaN.  position is the nearest point of the sphere to
 *   origin + axis * s by the closest-point statement.
 * Order and range: rt_closest_point_all's: (the bits of dist2, key) as one 64-bit unsigned number, in range iff below (the bits of
 *   radius * radius, 0).  Only dist2 < radius * radius is accepted, strictly; a NaN or infinite dist2 never; at equal dist2 spheres
 *   come before triangles, each kind by ascending index.  rt_sweep_capsule's start-in-contact test is <=: a listed contact implies
 *   t = 0 there for the same pose, and the converse fails only at dist2 == radius * radius.
 * A degenerate query - a non-finite component of origin or axis, or a radius that is NaN or <= 0 - lists nothing, without a walk.
 *   The kernel checks this itself.  radius = +inf is allowed, as for rt_closest_point; axis = 0 is allowed: with it the call returns
 *   rt_closest_point_all's records (position, distance, prim_id, material_id) and counts bit for bit, with s = 0.
 * List mode (flags without RT_QUERY_COUNT_ALL and RT_CONTACT_ANY): capsule i's min(total, max_contacts) nearest contacts at
 *   out[i * max_contacts ..] (query-major), nearest first; unused slots are misses: position 0, distance = radius as given, s = 0,
 *   prim_id 0xFFFFFFFF, material_id 0.  counts[i] = the number written; `counts` may be NULL.  1 <= max_contacts <= RT_CONTACT_MAX.
 * RT_QUERY_COUNT_ALL: the same records; counts[i] = the number of all primitives in range, which can exceed max_contacts.
 *   max_contacts == 0 is allowed with it, needs a non-NULL counts and ignores `out`: a pure count.
 * RT_CONTACT_ANY: requires max_contacts == 0 and a non-NULL counts, and excludes RT_QUERY_COUNT_ALL; counts[i] = 1 if anything is in
 *   range of capsule i, else 0.  The walk stops at the first primitive in range; which one that is depends on the tree, so it is not
 *   reported.  This is the occupancy test.
 * The result follows from these rules alone: it does not depend on the tree in use, the device count, the kind of memory or the
 *   chunking, and after rt_update_geometry it is that of a fresh upload of the moved scene.  The tree only culls, by the distance
 *   between each child box and the axis segment's bounding box less a margin past the statement's own rounding (DESIGN.md section
 *   4); the bound is loose for a long diagonal capsule.
 * Buffers, chunking (RT_QUERY_CHUNK / max(max_contacts, 1) capsules), the split over devices, synchronisation, side effects and
 *   statistics as for rt_closest_point_all; the records are 32 bytes in and 32 bytes out, device memory 16-byte aligned (counts
 *   4-byte).
 * Errors: n == 0 is RT_OK; a NULL capsules, or a NULL out with max_contacts > 0, max_contacts > RT_CONTACT_MAX, max_contacts == 0
 *   without RT_QUERY_COUNT_ALL or RT_CONTACT_ANY and counts, RT_CONTACT_ANY with max_contacts > 0 or with RT_QUERY_COUNT_ALL, and
 *   unknown flag bits are RT_ERR_BAD_ARG and change nothing; a call before any upload is RT_ERR_NOT_UPLOADED.  An empty scene gives
 *   counts of 0 and misses.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_capsule {  /* the first 32 bytes of an rt_capsule_sweep */
    float origin[3];       /* end A of the axis */
    float radius;          /* > 0; +inf allowed */
    float axis[3];         /* B - A; zero allowed (a resting sphere: rt_closest_point_all) */
    uint32_t _pad;         /* ignored */
} rt_capsule; /* 32 bytes */

typedef struct rt_contact {  /* rt_capsule_sweep_hit's layout with the distance where t is */
    float position[3];     /* the point of the primitive nearest the axis; 0 in an unused slot */
    float distance;        /* its distance from the axis segment, < radius; the radius as given in an unused slot */
    float s;               /* where on the axis: 0 at A .. 1 at B; 0 in an unused slot */
    uint32_t _reserved;    /* written as 0 */
    uint32_t prim_id;      /* as rt_hit.prim_id; 0xFFFFFFFF = unused slot */
    uint32_t material_id;  /* the record's material id, unchecked; 0 in an unused slot */
} rt_contact; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_capsule) == 32 && offsetof(rt_capsule, origin) == 0 && offsetof(rt_capsule, radius) == 12 &&
                     offsetof(rt_capsule, axis) == 16 && offsetof(rt_capsule, _pad) == 28,
                 "rt_capsule is 32 B: origin, radius at 12, axis at 16, _pad at 28");
RT_STATIC_ASSERT(sizeof(rt_contact) == 32 && offsetof(rt_contact, position) == 0 && offsetof(rt_contact, distance) == 12 &&
                     offsetof(rt_contact, s) == 16 && offsetof(rt_contact, _reserved) == 20 && offsetof(rt_contact, prim_id) == 24 &&
                     offsetof(rt_contact, material_id) == 28,
                 "rt_contact is 32 B: position, distance at 12, s at 16, _reserved at 20, prim_id at 24, material_id at 28");

#define RT_CONTACT_MAX 16u
#define RT_CONTACT_ANY 4u   /* rt_contact_capsule only: counts[i] = 1 if anything is in range of capsule i, else 0; stops at the first; also rt_contact_triangle */

int rt_contact_capsule(rt_ctx* ctx, const rt_capsule* capsules, size_t n, uint32_t max_contacts,
                       rt_contact* out,   /* n * max_contacts records, query-major; unused slots are misses */
                       uint32_t* counts,  /* n entries; may be NULL unless max_contacts == 0 */
                       uint32_t flags);   /* RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL | RT_CONTACT_ANY */

/* ---------------------------------------------------------------------------------------------------------------
 * Oriented boxes: rt_overlap_box and rt_sweep_box for a box with an orientation (no reference counterpart; OverlapBox, BoxCast,
 * contactTest and the box sweep of the collision libraries, which all take an orientation, are the model): a crate on a slope, a
 * vehicle hull, a door leaf, a turned trigger volume.  The world-aligned bounding box of a turned box has up to 3 sqrt 3 times its
 * volume and reports contacts the body never makes, the inscribed box tunnels, and turning the scene instead costs an
 * rt_update_geometry per orientation.  The answer is one f32 statement (csrc/obb_rules.h, whose header comment is the specification;
 * every operation one f32 rounding, nothing fused):
 * Frame: rotation = (x, y, z, w) is the quaternion that turns the box's own axes into world axes; it need not be normalised.
 *   n = ((x*x + y*y) + z*z) + w*w, s = 2.0f / n, xs = x*s, ys = y*s, zs = z*s, wx = w*xs, wy = w*ys, wz = w*zs, xx = x*xs, xy = x*ys,
 *   xz = x*zs, yy = y*ys, yz = y*zs, zz = z*zs, R = [[1-(yy+zz), xy-wz, xz+wy], [xy+wz, 1-(xx+zz), yz-wx], [xz-wy, yz+wx, 1-(xx+yy)]],
 *   whose columns are the box's axes in the world.  Into the frame: u'_j = (R_0j*u_0 + R_1j*u_1) + R_2j*u_2; back to the world:
 *   u_a = (R_a0*u'_0 + R_a1*u'_1) + R_a2*u'_2.
 * Triangle, from its record's v0, e1, e2: a_k as in "Overlap queries" (v0 - c, (v0 + e1) - c, (v0 + e2) - c), each taken into the
 *   frame, with e1' = frame(e1), e2' = frame(e2) and, for the sweep, d' = frame(direction); then the thirteen axes of "Overlap
 *   queries" / "Box sweeps" on (a'_0, a'_1, a'_2, e1', e2', h[, d']), f1 = e2' - e1', dd = dot(d', d'); "all nine components finite"
 *   is asked of the a'_k.
 * Sphere (centre o): o' = frame(o - c) per component, then the sphere rules of "Overlap queries" / "Box sweeps" with the sphere's
 *   centre o', the box's centre 0, h and d'.
 * rt_sweep_obb's record: t, axis, prim_id and material_id as in "Box sweeps", with `axis` read in the box's frame (0 - 2 the box's
 *   own axes, 3 the triangle's normal, 4 - 12 the cross axes, RT_SWEEP_AXIS_SPHERE, RT_SWEEP_AXIS_NONE); normal = world(normal') +
 *   0.0f per component, in world space.  Order and acceptance as there: (the bits of t, key) from (the bits of tmax, 0), strictly.
 * A degenerate query - one that is degenerate by the rules of rt_overlap_box / rt_sweep_box on center, half_extent (direction, tmax),
 *   a non-finite component of rotation, or an n that is not finite and > 0 (the zero quaternion; one whose n overflows or underflows
 *   to 0) - touches nothing, or is the miss record carrying tmax as given, without a walk.  The kernel checks this itself.
 * With rotation = (0, 0, 0, w), w finite and not 0 (a -0 among x, y, z included), R is the identity and both calls return
 *   rt_overlap_box's and rt_sweep_box's bytes; the one exception is the sign of a zero component of a sphere contact's normal, which is always + here
 *   (csrc/obb_rules.h, consequence (a)).  rt_sweep_obb answers t = 0 with RT_SWEEP_AXIS_NONE for a triangle exactly when
 *   rt_overlap_obb lists that triangle for the start pose.
 * The result follows from these rules alone: it does not depend on the tree in use, the device count, the kind of memory or the
 *   chunking, and after rt_update_geometry it is that of a fresh upload of the moved scene.  The tree only culls, in world space, by
 *   the bounding box of the turned box, H_a = (|R_a0|*h_0 + |R_a1|*h_1) + |R_a2|*h_2 and a margin; the bound
 *   is loose for a long box turned 45 degrees.
 * rt_overlap_obb: modes, list order and unused slots, counts, chunking (RT_QUERY_CHUNK / max(max_prims, 1) boxes), the split over
 *   devices, buffer classification, synchronisation, side effects, statistics and error codes as for rt_overlap_box; the records
 *   are 48 bytes in, device memory 16-byte aligned (prims and counts 4-byte).
 * rt_sweep_obb: buffers, chunking, the split over devices, synchronisation, side effects, statistics and error codes as for
 *   rt_sweep_box; the records are 64 bytes in and 32 bytes out, device memory 16-byte aligned.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_obb {  /* its first 32 bytes are an rt_box */
    float center[3];
    uint32_t _pad0;          /* pads are ignored */
    float half_extent[3];    /* >= 0 per axis, along the box's own axes; 0 is allowed */
    uint32_t _pad1;
    float rotation[4];       /* quaternion x, y, z, w: the box's axes -> world axes; any length that is finite and not 0 */
} rt_obb; /* 48 bytes */

typedef struct rt_obb_sweep {  /* its first 48 bytes are an rt_obb, its last 16 the second half of an rt_sweep */
    float center[3];         /* of the box at t = 0 */
    uint32_t _pad0;
    float half_extent[3];
    uint32_t _pad1;
    float rotation[4];
    float direction[3];      /* world space; not zero; need not be normalised: t is in units of it.  The box does not turn on the way */
    float tmax;              /* > 0; +inf allowed */
} rt_obb_sweep; /* 64 bytes */

RT_STATIC_ASSERT(sizeof(rt_obb) == 48 && offsetof(rt_obb, center) == 0 && offsetof(rt_obb, _pad0) == 12 && offsetof(rt_obb, half_extent) == 16 &&
                     offsetof(rt_obb, _pad1) == 28 && offsetof(rt_obb, rotation) == 32,
                 "rt_obb is 48 B: center, _pad0 at 12, half_extent at 16, _pad1 at 28, rotation at 32");
RT_STATIC_ASSERT(sizeof(rt_obb_sweep) == 64 && offsetof(rt_obb_sweep, center) == 0 && offsetof(rt_obb_sweep, half_extent) == 16 &&
                     offsetof(rt_obb_sweep, rotation) == 32 && offsetof(rt_obb_sweep, direction) == 48 && offsetof(rt_obb_sweep, tmax) == 60,
                 "rt_obb_sweep is 64 B: center, half_extent at 16, rotation at 32, direction at 48, tmax at 60");

int rt_overlap_obb(rt_ctx* ctx, const rt_obb* boxes, size_t n, uint32_t max_prims,
                   uint32_t* prims,   /* n * max_prims ids, query-major, rt_hit.prim_id's encoding; unused slots 0xFFFFFFFF */
                   uint32_t* counts,  /* n entries; may be NULL unless max_prims == 0 */
                   uint32_t flags);   /* RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL | RT_OVERLAP_ANY; max_prims <= RT_OVERLAP_MAX */
int rt_sweep_obb(rt_ctx* ctx, const rt_obb_sweep* sweeps, size_t n, rt_box_sweep_hit* out, uint32_t flags); /* RT_QUERY_COUNTERS */

/* ---------------------------------------------------------------------------------------------------------------
 * Triangle queries: the primitives of the scene that the caller's own triangles touch (no reference counterpart; Embree's
 * rtcCollide and the collision managers of FCL / trimesh are the model): a moving mesh against the static scene, clash detection
 * between an inserted part and a building, the seed of a cut or a CSG, self-intersection checks with the scene's own triangles as
 * queries.  rt_overlap_box over each triangle's bounding box is a different and much looser query: a thin diagonal triangle's box
 * is almost all empty space.  The answer is one f32 statement (csrc/overlap_triangle_rules.h, whose header comment is the
 * specification; every operation one f32 rounding, nothing fused, every test in its positive form so that a NaN makes it false).
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).
 * Query: q0, q1, q2 = v0, v1, v2 of the record; u1 = q1 - q0, u2 = q2 - q0, u3 = u2 - u1; qlo, qhi the per-axis min and max of the
 *   three vertices (exact).  A query with a non-finite component touches nothing and is not walked; the kernel checks this itself.
 *   A finite degenerate query (a segment, a point) is allowed.
 * Triangle of the scene, from its record's v0, e1, e2: s0 = v0, s1 = v0 + e1, s2 = v0 + e2; f1 = e1, f2 = e2, f3 = e2 - e1.  It
 *   touches iff all of these hold:
 *   0. all nine components of the s_k are finite;
 *   1. per coordinate axis a: min_k s_k[a] <= qhi[a] && max_k s_k[a] >= qlo[a];
 *   2. with a_k = s_k - q0, for each of the 23 axes L below: pS_k = dot(L, a_k), pQ = (0, dot(L, u1), dot(L, u2));
 *      min_k pS_k <= max pQ && max_k pS_k >= min pQ, and ((pS_0 + pS_1) + pS_2) + (pQ_1 + pQ_2) is not a NaN (the min and max are
 *      fminf / fmaxf, which ignore a NaN operand).
 *   The axes: nS = cross(f1, f2) and nQ = cross(u1, u2); the nine cross(u_i, f_j); cross(nQ, u_i) and cross(nS, f_j), which decide
 *   coplanar pairs; cross(nS, u_i) and cross(nQ, f_j), which decide a pair in which one triangle is a segment.  Any vector is a
 *   legitimate candidate for a separating axis, so a noisy axis from nearly parallel edges never wrongly separates in exact
 *   arithmetic; only the rounding of the projections matters.
 *   Two limits.  Two degenerate triangles (segments, points) can be listed although they are disjoint: for two parallel segments or
 *   two points every axis is the zero vector and test 1 alone decides; this errs on the side of listing.  And "closed" means closed
 *   on the record: the scene's vertices are the s_k above, and a vertex the caller shares with the scene is bit-equal only where
 *   v0 + e reproduces it.
 * Sphere (o, R), a surface as everywhere: near2 = the squared distance of "Closest-point queries" from o to the triangle (q0, u1,
 *   u2), far2 = max_k dot(q_k - o, q_k - o), rr = R * R.  It touches iff near2 <= rr && far2 >= rr: a triangle wholly inside the
 *   ball is not touched.
 * The closed test lists, for a query that is one of the scene's own triangles, that triangle and its neighbours.
 * The result follows from these rules alone: it does not depend on the tree in use, the device count, the kind of memory or the
 *   chunking, and after rt_update_geometry it is that of a fresh upload of the moved scene.  The tree only culls, by the query's
 *   bounds qlo, qhi and the margin of "Overlap queries" (DESIGN.md section 4).
 * rt_overlap_triangle: key order (prim_id ^ 0x80000000: spheres by index, then triangles by original index), the modes (the list,
 *   RT_QUERY_COUNT_ALL - with it max_prims 0 is allowed - and RT_OVERLAP_ANY), 1 <= max_prims <= RT_OVERLAP_MAX, unused slots
 *   0xFFFFFFFF, counts (may be NULL unless max_prims == 0), chunking (RT_QUERY_CHUNK / max(max_prims, 1) triangles), the split over
 *   devices, buffer classification (host or device memory, all of one kind), synchronisation, side effects (the last frame and a
 *   running accumulation are left alone), statistics (rays = n; visits and records only with RT_QUERY_COUNTERS) and error codes as
 *   for rt_overlap_box; the records are 48 bytes in, device memory 16-byte aligned (prims and counts 4-byte).
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_query_triangle {
    float v0[3];
    uint32_t _pad0;          /* pads are ignored */
    float v1[3];
    uint32_t _pad1;
    float v2[3];
    uint32_t _pad2;
} rt_query_triangle; /* 48 bytes */

RT_STATIC_ASSERT(sizeof(rt_query_triangle) == 48 && offsetof(rt_query_triangle, v0) == 0 && offsetof(rt_query_triangle, _pad0) == 12 &&
                     offsetof(rt_query_triangle, v1) == 16 && offsetof(rt_query_triangle, _pad1) == 28 && offsetof(rt_query_triangle, v2) == 32 &&
                     offsetof(rt_query_triangle, _pad2) == 44,
                 "rt_query_triangle is 48 B: v0, _pad0 at 12, v1 at 16, _pad1 at 28, v2 at 32, _pad2 at 44");

int rt_overlap_triangle(rt_ctx* ctx, const rt_query_triangle* triangles, size_t n, uint32_t max_prims,
                        uint32_t* prims,   /* n * max_prims ids, query-major, rt_hit.prim_id's encoding; unused slots 0xFFFFFFFF */
                        uint32_t* counts,  /* n entries; may be NULL unless max_prims == 0 */
                        uint32_t flags);   /* RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL | RT_OVERLAP_ANY; max_prims <= RT_OVERLAP_MAX */

/* ---------------------------------------------------------------------------------------------------------------
 * Triangle sweeps: the first contact of the caller's own triangles, each in translation, with the scene's surface (no reference
 * counterpart; the translational triangle cast of mesh collision libraries is the model): continuous collision for a moving mesh,
 * which "Triangle queries" can only test where it stands.  Stepping rt_overlap_triangle along the path tunnels through thin
 * geometry and gives no contact time; rt_sweep_box over the triangle's bounds reports contacts of empty space; chained sphere
 * sweeps miss what lies between the spheres.  The answer is one f32 statement (csrc/sweep_triangle_rules.h, whose header comment is
 * the specification; every operation one f32 rounding, nothing fused, every test in its positive form so that a NaN makes it
 * false); dot and cross as in "Triangle queries".
 * Query: q0, q1, q2, u1, u2, u3, qlo, qhi as in "Triangle queries", d = direction and tmax.  The triangle at time t is q_k + d t; a
 *   finite segment or point is allowed.  A miss without a walk, which the kernel checks itself: a non-finite component of a vertex
 *   or of d, a zero d, a tmax that is NaN or <= 0.
 * Triangle of the scene, from its record's v0, e1, e2: s_k, f_j and a_k = s_k - q0 as in "Triangle queries".  Two convex bodies in
 *   translation touch at t iff no axis of a complete static axis set separates them at t, and the axes of rt_overlap_triangle do
 *   not depend on position: each gives an interval of t and the contact is the intersection of the intervals.  The 26 axes, whose
 *   numbers are rt_triangle_sweep_hit.axis:
 *     0, 1, 2  the coordinate axes;  3  nS = cross(f1, f2);  4  nQ = cross(u1, u2);  5 + 3(i-1) + (j-1)  cross(u_i, f_j);
 *     14 - 16  cross(nQ, u_i);  17 - 19  cross(nS, f_j);  20 - 22  cross(nS, u_i);  23 - 25  cross(nQ, f_j).
 *   Coordinate axis a: lo = min_k s_k[a] - qhi[a], hi = max_k s_k[a] - qlo[a], w = d[a].  Axis L of the other 23: pS_k = dot(L, a_k),
 *   pQ = (0, dot(L, u1), dot(L, u2)), lo = min pS - max pQ, hi = max pS - min pQ, w = dot(L, d); it holds only if
 *   ((pS_0 + pS_1) + pS_2) + (pQ_1 + pQ_2) is not a NaN.  Then, as in "Box sweeps": w > 0: enter = lo / w, exit = hi / w; w < 0:
 *   the two swapped; in both cases the axis holds iff enter <= exit, it replaces the running entry (0, RT_SWEEP_AXIS_NONE) iff its
 *   enter is strictly larger, and t_out is the minimum of the exits.  w == 0: the axis holds iff lo <= 0 && hi >= 0 and constrains
 *   nothing.  w a NaN: the axis does not hold.
 *   Contact iff all nine components of the s_k are finite, every axis holds and t_in <= t_out; then t = t_in + 0.0f and axis is
 *   the one that set t_in (at equal enter the lowest number).  t = 0 with RT_SWEEP_AXIS_NONE results exactly when
 *   rt_overlap_triangle lists the triangle for q0, q1, q2: the sign of a rounded difference is exact (csrc/sweep_triangle_rules.h
 *   has the argument and its two remarks on overflow).
 *   normal = (w_in > 0 ? -L : L) / sqrtf(dot(L, L)) + 0.0f for the closing axis' vector L, against the motion; 0 for
 *   RT_SWEEP_AXIS_NONE, and 0 where that length is not finite or not > 0.
 *   Three limits.  Two degenerate triangles (segments, points) may be reported although they never meet; "closed" means closed on
 *   the record (both as in "Triangle queries"); and two coplanar triangles moving inside their common plane are decided exactly
 *   only where the plane's coordinates are exact (a coordinate plane): elsewhere the answer is that of a pair tilted by rounding.
 *   A fourth concerns spheres alone, below: a segment given as v1 == v0.
 * Sphere (o, R), a surface as everywhere; near2, far2, rr as in "Triangle queries", dd = dot(d, d).  Touching at the start (near2
 *   <= rr && far2 >= rr): t = 0, RT_SWEEP_AXIS_NONE.  Otherwise from outside (near2 > rr): the time of "Sphere sweeps" for a ball
 *   of radius R that starts at o and moves by -d against the triangle (q0, u1, u2).  Otherwise from inside (far2 < rr): the minimum
 *   over the three vertices, with m = o - q_k, of t = (dot(m, d) + sqrtf(disc)) / dd, disc = dd * rr - dot(cross(m, d), cross(m,
 *   d)), accepted iff disc >= 0 && t >= 0.  A contact at t > 0 has axis RT_SWEEP_TRIANGLE_AXIS_SPHERE and as normal the unit
 *   vector, with P = o - d t: from outside, from P to the closest point of the triangle (q0, u1, u2) to P; from inside, from the
 *   vertex farthest from P to P; 0 if its length is not > 0.  A contact at t = 0 has RT_SWEEP_AXIS_NONE and normal 0.
 *   The fourth limit: near2 is the closest-point statement's for a degenerate query too, and for a segment given as v1 == v0 its
 *   edge rule divides 0 by 0 wherever the closest point is not v0 itself: near2 is a NaN, every test on it fails, and that segment
 *   meets no sphere, at the start or later (rt_overlap_triangle's behaviour, carried over).  A segment given as v2 == v1 or as
 *   v2 == v0, and a point, have no such case and meet spheres as stated; give a moving segment in one of these forms.  The
 *   scene's triangles are not affected.
 * Order and acceptance as for rt_sweep_box: only t < tmax is accepted, strictly; at equal t spheres come before triangles, and
 *   within each kind the lowest index wins.  A miss: normal 0, t = tmax as given, axis RT_SWEEP_AXIS_NONE, prim_id 0xFFFFFFFF,
 *   material_id 0.
 * The result follows from these rules alone: it does not depend on the tree in use, the device count, the kind of memory or the
 *   chunking, and after rt_update_geometry it is that of a fresh upload of the moved scene.  The tree only culls, by the box of
 *   the query's bounds swept along d with the margin of "Box sweeps" (DESIGN.md section 4).
 * rt_sweep_triangle: buffers (host or device memory, both of one kind, device memory 16-byte aligned), chunking (RT_QUERY_CHUNK
 *   records), the split over devices, synchronisation, side effects (the last frame and a running accumulation are left alone),
 *   statistics (rays = n; visits and records only with RT_QUERY_COUNTERS) and error codes as for rt_sweep_box.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_triangle_sweep {
    float v0[3];           /* the first 48 bytes are an rt_query_triangle: the triangle at t = 0 */
    uint32_t _pad0;        /* pads are ignored */
    float v1[3];
    uint32_t _pad1;
    float v2[3];
    uint32_t _pad2;
    float direction[3];    /* the last 16 bytes are the second half of an rt_sweep; not normalised: t is in units of |direction| */
    float tmax;            /* only contacts with t < tmax are reported */
} rt_triangle_sweep; /* 64 bytes */

typedef struct rt_triangle_sweep_hit {
    float normal[3];       /* unit, against the motion; 0 for a miss and for a start in contact */
    float t;               /* time of first contact; tmax as given for a miss */
    uint32_t axis;         /* which separating axis closed last: 0 .. 25, RT_SWEEP_TRIANGLE_AXIS_SPHERE or RT_SWEEP_AXIS_NONE */
    uint32_t _reserved;    /* 0 */
    uint32_t prim_id;      /* rt_hit.prim_id's encoding; 0xFFFFFFFF for a miss */
    uint32_t material_id;
} rt_triangle_sweep_hit; /* 32 bytes: rt_box_sweep_hit's layout */

#define RT_SWEEP_TRIANGLE_AXIS_SPHERE 26u

RT_STATIC_ASSERT(sizeof(rt_triangle_sweep) == 64 && offsetof(rt_triangle_sweep, v0) == 0 && offsetof(rt_triangle_sweep, _pad0) == 12 &&
                     offsetof(rt_triangle_sweep, v1) == 16 && offsetof(rt_triangle_sweep, _pad1) == 28 && offsetof(rt_triangle_sweep, v2) == 32 &&
                     offsetof(rt_triangle_sweep, _pad2) == 44 && offsetof(rt_triangle_sweep, direction) == 48 && offsetof(rt_triangle_sweep, tmax) == 60,
                 "rt_triangle_sweep is 64 B: an rt_query_triangle, direction at 48, tmax at 60");
RT_STATIC_ASSERT(sizeof(rt_triangle_sweep_hit) == 32 && offsetof(rt_triangle_sweep_hit, normal) == 0 && offsetof(rt_triangle_sweep_hit, t) == 12 &&
                     offsetof(rt_triangle_sweep_hit, axis) == 16 && offsetof(rt_triangle_sweep_hit, _reserved) == 20 &&
                     offsetof(rt_triangle_sweep_hit, prim_id) == 24 && offsetof(rt_triangle_sweep_hit, material_id) == 28,
                 "rt_triangle_sweep_hit is 32 B: normal, t at 12, axis at 16, _reserved at 20, prim_id at 24, material_id at 28");

int rt_sweep_triangle(rt_ctx* ctx, const rt_triangle_sweep* sweeps, size_t n, rt_triangle_sweep_hit* out, uint32_t flags); /* RT_QUERY_COUNTERS */

/* ---------------------------------------------------------------------------------------------------------------
 * Triangle contacts: the primitives near the caller's own RESTING triangles, with the closest pair of points (no reference
 * counterpart; FCL's distance, the contact manifold with a collision margin of Bullet and PhysX for mesh shapes and the clearance
 * query of robot and tool-path planners are the model).  rt_overlap_triangle says "touches", rt_sweep_triangle says when; this says
 * how far, from which primitive and at which pair of points: what de-penetration, resting contact and the step of conservative
 * advancement need.
 *
 * For each query triangle v0, v1, v2 - equal vertices are allowed: a segment, a point - the max_contacts nearest primitives of the
 * scene whose distance from the triangle is STRICTLY below `margin`, nearest first.  The distance of the query from a triangle of
 * the scene is the distance of the two triangles as closed sets, 0 when they intersect; a sphere is its surface, as everywhere: the
 * distance is that of the triangle from the surface, from outside, from inside, or 0 when the triangle crosses it.  One f32
 * statement (csrc/contact_triangle_rules.h), independent of the tree:
 *   a triangle of the scene: the least of the three query vertices against it, its three vertices against the query (a query
 *   with an area only), the nine edge pairs as clamped segments, and 0 where an edge of one passes through the other; the first
 *   of these in that order with the strictly smallest squared distance gives the pair of points;
 *   a sphere: the query's point nearest the centre when that lies outside, its farthest vertex when the whole triangle lies
 *   inside, else the point between the two that lies on the surface.
 * A record gives the point of the PRIMITIVE, the distance and the weights of the QUERY's own point, so that
 *   normal = ((v0 + (v1 - v0) qu + (v2 - v0) qv) - position) / distance     and     depth = margin - distance
 * are the push-out.  Two triangles that intersect have distance 0 and no normal: the penetration depth of an intersecting pair is
 * out of scope here.  A degenerate query - a non-finite vertex component, or a margin that is NaN or <= 0 - lists nothing; a margin
 * of +inf is allowed.  With v0 == v1 == v2 the records are rt_closest_point_all's at that point with the margin as the radius, bit
 * for bit (position, distance, prim_id, material_id; qu = qv = 0).  A segment is answered the same whichever two of its
 * vertices coincide (rt_sweep_triangle's fourth limit does not apply here).
 *
 * rt_contact_triangle: everything that is not the statement above is rt_contact_capsule's, with `margin` where `radius` is: the
 *   modes (the list; RT_QUERY_COUNT_ALL, with which max_contacts == 0 is allowed; RT_CONTACT_ANY), the order (bits of dist2, key),
 *   the strict range dist2 < margin * margin, unused slots and counts, 1 <= max_contacts <= RT_CONTACT_MAX, chunking at
 *   RT_QUERY_CHUNK / max(max_contacts, 1) triangles, the split over devices, buffers (host or device memory, all of one kind, device
 *   memory 16-byte aligned, counts 4-byte), synchronisation, side effects (the last frame and a running accumulation are left alone),
 *   statistics (rays = n; visits and records only with RT_QUERY_COUNTERS) and the error codes, one for one.  The tree only culls, by
 *   the distance between the box of the query's vertices and each child box: loose for a large triangle askew to the axes.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_triangle_contact_query {   /* rt_query_triangle's layout with the margin where _pad0 is (offset 12, where rt_point_query and rt_capsule keep the radius) */
    float v0[3];
    float margin;          /* only surface strictly nearer than this is listed; > 0, +inf allowed */
    float v1[3];
    uint32_t _pad1;        /* pads are ignored */
    float v2[3];
    uint32_t _pad2;
} rt_triangle_contact_query; /* 48 bytes */

typedef struct rt_triangle_contact {         /* rt_nearest's layout; qu, qv are the QUERY's weights */
    float position[3];     /* the point of the scene's primitive nearest the query triangle; 0 in an unused slot */
    float distance;        /* between the two; < margin; the margin as given in an unused slot */
    float qu, qv;          /* the weights of the query's v1 and v2 at its own point of the closest pair; 0 in an unused slot */
    uint32_t prim_id;      /* as rt_hit.prim_id; 0xFFFFFFFF = unused slot */
    uint32_t material_id;  /* the record's material id, unchecked; 0 in an unused slot */
} rt_triangle_contact; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_triangle_contact_query) == 48 && offsetof(rt_triangle_contact_query, v0) == 0 && offsetof(rt_triangle_contact_query, margin) == 12 &&
                     offsetof(rt_triangle_contact_query, v1) == 16 && offsetof(rt_triangle_contact_query, _pad1) == 28 &&
                     offsetof(rt_triangle_contact_query, v2) == 32 && offsetof(rt_triangle_contact_query, _pad2) == 44,
                 "rt_triangle_contact_query is 48 B: v0, margin at 12, v1 at 16, _pad1 at 28, v2 at 32, _pad2 at 44");
RT_STATIC_ASSERT(sizeof(rt_triangle_contact) == 32 && offsetof(rt_triangle_contact, position) == 0 && offsetof(rt_triangle_contact, distance) == 12 &&
                     offsetof(rt_triangle_contact, qu) == 16 && offsetof(rt_triangle_contact, qv) == 20 && offsetof(rt_triangle_contact, prim_id) == 24 &&
                     offsetof(rt_triangle_contact, material_id) == 28,
                 "rt_triangle_contact is 32 B: position, distance at 12, qu at 16, qv at 20, prim_id at 24, material_id at 28");

int rt_contact_triangle(rt_ctx* ctx, const rt_triangle_contact_query* triangles, size_t n, uint32_t max_contacts,
                        rt_triangle_contact* out,   /* n * max_contacts records, query-major; unused slots are misses */
                        uint32_t* counts,           /* n entries; may be NULL unless max_contacts == 0 */
                        uint32_t flags);            /* RT_QUERY_COUNTERS | RT_QUERY_COUNT_ALL | RT_CONTACT_ANY; max_contacts <= RT_CONTACT_MAX */

/* ---------------------------------------------------------------------------------------------------------------
 * Posed meshes: the caller's own mesh of m triangles, given ONCE, at n candidate poses (no reference counterpart; the call of
 * FCL, Bullet, PhysX and Embree's rtcCollide that takes a shape once and a transform per query is the model): a planner's robot link
 * at many configurations, a hull dropped at many spots.  "Triangle queries" and "Triangle sweeps" answer per triangle: their caller
 * transforms n * m triangles, ships 64 bytes for each, gets n * m records back and reduces them per pose.  Here the device poses the
 * triangles, one lane runs per posed triangle with the statements of those two sections, and the reduction per pose happens on the
 * device; in a sweep the lanes of a pose share the body's best time so far, so that each culls by the body's first contact.
 *
 * The answer for a pose is BY DEFINITION the reduction of rt_overlap_triangle / rt_sweep_triangle over the posed triangles, bit for
 * bit, and the posing is one f32 statement (csrc/mesh_pose_rules.h, whose header comment is the specification; every operation
 * one f32 rounding, nothing fused):
 *   R = the frame of `rotation` as in "Oriented boxes" (the quaternion x, y, z, w need not be normalised);
 *   vertex v of the mesh becomes  w_a = ((R_a0 * v_0 + R_a1 * v_1) + R_a2 * v_2) + position_a.
 * A pose is valid iff its three position components are finite and the rotation is valid as in "Oriented boxes" (all four
 * components finite, the squared norm finite and > 0).  An invalid pose is answered without a walk: rt_overlap_mesh gives pairs = 0
 * and first = 0xFFFFFFFF, rt_sweep_mesh the miss record below.  A posed triangle is then judged by the triangle call's own rule:
 * a non-finite mesh vertex makes that triangle touch nothing, a zero direction or a tmax that is NaN or <= 0 a miss.  With rotation
 * (0, 0, 0, w), w != 0, and position 0 the posed vertices are the mesh's, up to the sign of a zero.
 *
 * With T_ij = mesh triangle j posed by pose i:
 * rt_overlap_mesh: c_j = the count rt_overlap_triangle gives T_ij with RT_QUERY_COUNT_ALL and max_prims = 0.
 *   pairs[i] = min(sum_j c_j, 0xFFFFFFFF), the sum taken in 64 bits; first[i] = the lowest j with c_j > 0, else 0xFFFFFFFF.
 *   RT_OVERLAP_ANY: pairs[i] = 1 if some c_j > 0, else 0, and the pose may stop at the first touch; `first` must then be NULL
 *   (RT_ERR_BAD_ARG otherwise).
 * rt_sweep_mesh: h_j = rt_sweep_triangle's record for (T_ij, direction, tmax); the direction is in world space and is NOT turned by
 *   the pose.  The answer is h_j of the hit with the least (bits of t, prim_id ^ 0x80000000, j), its _reserved word replaced by j:
 *   at equal time spheres come before triangles, a lower scene index before a higher, a lower mesh triangle before a higher.  If
 *   every h_j is a miss: normal 0, t = tmax as given, axis RT_SWEEP_AXIS_NONE, triangle = prim_id = 0xFFFFFFFF, material_id 0.
 * Arguments: 1 <= m <= RT_POSED_MESH_MAX, else RT_ERR_BAD_ARG; n = 0 is RT_OK and touches nothing, as for rt_sweep_triangle.
 * Buffers: mesh, the poses and the outputs are all host memory or all device memory of one device; device memory 16-byte aligned,
 *   pairs and first 4-byte.  A host mesh is copied to every device that takes part, once per call.  Chunks are
 *   max(1, RT_QUERY_CHUNK / m) poses; the split over devices is by poses.
 * Statistics: rays = n; visits and records only with RT_QUERY_COUNTERS.  The bytes of the answer are deterministic; with the
 *   shared bound the counters of rt_sweep_mesh are not (they depend on which lane found the body's contact first).
 * Everything else - synchronisation, side effects (the last frame and a running accumulation are left alone), error codes - as for
 *   rt_sweep_triangle.  The result does not depend on the tree in use, the device count, the kind of memory or the chunking.
 * Limit: a pose never spans more than one wave of the device, so a call with few poses and a very large mesh occupies few waves;
 *   such a caller is better off with rt_sweep_triangle over its own posed triangles and its own reduction.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_pose {
    float position[3];     /* added after the rotation */
    uint32_t _pad0;        /* ignored */
    float rotation[4];     /* x, y, z, w: rt_obb's quaternion, mesh axes -> world axes; need not be normalised */
} rt_pose; /* 32 bytes */

typedef struct rt_pose_sweep {
    float position[3];     /* the first 32 bytes are an rt_pose */
    uint32_t _pad0;
    float rotation[4];
    float direction[3];    /* the last 16 bytes are the second half of an rt_sweep; world space, NOT turned by the pose; not normalised */
    float tmax;            /* only contacts with t < tmax are reported */
} rt_pose_sweep; /* 48 bytes */

typedef struct rt_mesh_sweep_hit {
    float normal[3];       /* rt_triangle_sweep_hit's fields, of the posed triangle that touches first */
    float t;
    uint32_t axis;
    uint32_t triangle;     /* its index in the mesh; 0xFFFFFFFF for a miss */
    uint32_t prim_id;
    uint32_t material_id;
} rt_mesh_sweep_hit; /* 32 bytes: rt_triangle_sweep_hit with `triangle` where _reserved is */

#define RT_POSED_MESH_MAX 65536u  /* triangles in a query mesh */

RT_STATIC_ASSERT(sizeof(rt_pose) == 32 && offsetof(rt_pose, position) == 0 && offsetof(rt_pose, _pad0) == 12 && offsetof(rt_pose, rotation) == 16,
                 "rt_pose is 32 B: position, _pad0 at 12, rotation at 16");
RT_STATIC_ASSERT(sizeof(rt_pose_sweep) == 48 && offsetof(rt_pose_sweep, position) == 0 && offsetof(rt_pose_sweep, _pad0) == 12 &&
                     offsetof(rt_pose_sweep, rotation) == 16 && offsetof(rt_pose_sweep, direction) == 32 && offsetof(rt_pose_sweep, tmax) == 44,
                 "rt_pose_sweep is 48 B: an rt_pose, direction at 32, tmax at 44");
RT_STATIC_ASSERT(sizeof(rt_mesh_sweep_hit) == 32 && offsetof(rt_mesh_sweep_hit, normal) == 0 && offsetof(rt_mesh_sweep_hit, t) == 12 &&
                     offsetof(rt_mesh_sweep_hit, axis) == 16 && offsetof(rt_mesh_sweep_hit, triangle) == 20 &&
                     offsetof(rt_mesh_sweep_hit, prim_id) == 24 && offsetof(rt_mesh_sweep_hit, material_id) == 28,
                 "rt_mesh_sweep_hit is 32 B: normal, t at 12, axis at 16, triangle at 20, prim_id at 24, material_id at 28");

int rt_overlap_mesh(rt_ctx* ctx, const rt_query_triangle* mesh, size_t m, const rt_pose* poses, size_t n,
                    uint32_t* pairs,   /* n entries */
                    uint32_t* first,   /* n entries or NULL */
                    uint32_t flags);   /* RT_QUERY_COUNTERS | RT_OVERLAP_ANY */
int rt_sweep_mesh(rt_ctx* ctx, const rt_query_triangle* mesh, size_t m, const rt_pose_sweep* sweeps, size_t n, rt_mesh_sweep_hit* out,
                  uint32_t flags);     /* RT_QUERY_COUNTERS */

/* ---------------------------------------------------------------------------------------------------------------
 * Geometry updates: new positions for the uploaded scene, in place (no reference counterpart; Embree's refit build,
 * RTC_BUILD_QUALITY_REFIT, is the model).
 *
 * What changes: positions only - the vertex positions, and each sphere's centre, radius and material.  Triangles (their
 * vertex indices and material ids), materials, lights and textures stay as uploaded; moving lights or changing the
 * topology needs rt_upload_scene*.  A non-NULL array must hold exactly the count of the last upload (for
 * rt_upload_scene_packed: offsets->vertices_count / spheres_count), else RT_ERR_BAD_ARG.  NULL with count 0: unchanged.
 * Where the input may live: each pointer is classified as for the ray queries.  Host memory of any kind is accepted, and
 * device memory of one of the context's devices (4-byte alignment is enough); on a context with several devices, device
 * input is copied to the others (peer copy, or through the host).  Device-resident input must be complete before the call.
 * Result: afterwards every frame mode, rt_dispatch_tile, rt_intersect, rt_occluded and rt_read_hits give exactly the bits a
 * fresh rt_upload_scene of the moved scene gives, refitted or rebuilt, whichever tree was in use (device build, host build,
 * RT_PREPARE_QUALITY_TREE).  By default the tree in use is REFITTED: its triangle records and node boxes follow the new
 * positions, its topology stays, so a tree refitted across large motions gets slower to trace (not less exact);
 * RT_UPDATE_REBUILD builds a new one instead, as rt_upload_scene* would.  A triangle with a non-finite vertex is never hit
 * (the builders leave it out; a refit keeps its record, which no ray accepts).  A triangle that had a non-finite vertex at
 * upload and is finite now has no record to refit: the call then rebuilds by itself.
 * Derived state: a vertex update drops the light grids of the extended mode (rebuilt by the next frame that needs them, or
 * rt_prepare); a sphere-only update keeps them.  rt_prepare(RT_PREPARE_QUALITY_TREE) afterwards builds from the new positions.
 * Synchronous; first waits for an rt_dispatch_tile still in flight.  rt_read_* still return the last frame.
 * Statistics: kernel_ms (HIP events around the refit kernels, max over devices; 0 for a rebuild), wall_ms, flags =
 * RT_STAT_REFIT or RT_STAT_REBUILT (0 for a sphere-only update); bvh_nodes, bvh_depth, tree_build and scene_bytes describe
 * the tree in use afterwards; rays and the other counts are 0.
 * Errors: unknown flag bits and wrong counts are RT_ERR_BAD_ARG, a call before any upload RT_ERR_NOT_UPLOADED; these leave the
 * scene untouched.  A HIP or allocation failure part way leaves the context "not uploaded", as a failed upload does.
 * --------------------------------------------------------------------------------------------------------------- */
#define RT_UPDATE_REBUILD 1u /* build a new tree from the new positions instead of refitting the current one */

int rt_update_geometry(rt_ctx* ctx,
                       const rt_vertex* vertices, uint32_t n_vertices, /* NULL: vertices unchanged */
                       const rt_sphere* spheres, uint32_t n_spheres,   /* NULL: spheres unchanged  */
                       uint32_t flags);

/* ---------------------------------------------------------------------------------------------------------------
 * Feature buffers (AOVs) and denoising (no reference counterpart; Cycles' viewport denoising and the edge-avoiding a-trous
 * wavelet filter of Dammertz, Sewtz, Hanika and Lensch, HPG 2010, are the model).  The statement is DESIGN.md section 4,
 * "Feature buffers and the a-trous denoiser".
 *
 * rt_aovs: per pixel, what the first vertex of the frame `p` describes traces: albedo, geometric normal and depth of the first hit.
 *   p is the struct rt_render takes, validated by the same rules (same errors).  The samples are those of a frame with p: mode 2
 *   traces samples 0 .. spp-1 (rng_for(frame_seed + x + y * width, s), then the camera ray), jittered when spp > 1 or when
 *   RT_FLAG_ACCUMULATE is set; so for a running image of N samples (rt_accumulated_samples) pass spp = N with RT_FLAG_ACCUMULATE.
 *   Modes 0/1: the single pixel-centre ray of that mode; spp is ignored.  No other field or flag changes the result.
 *   Per sample, the closest hit is the frames' (spheres first, the tie rule).  On a hit: albedo = the material's albedo (magenta
 *   for an invalid material id), normal = the geometric normal face-forwarded against the ray, depth = t.  On a miss: albedo = the
 *   colour the mode gives a miss (sky (0.1, 0.2, 0.3) in modes 1/2, black in mode 0), normal = 0.
 *   Per pixel, f32 sums in sample order: albedo = sum albedo_s / spp; normal = sum over hits of normal_s / spp (not renormalised:
 *   a silhouette pixel has a shorter normal); depth = sum over hits of t_s / hits, 0 without a hit; coverage = hits / spp.
 *   The pixel set is the frame's: pixels outside the context's tile_rank / tile_world share are written as zero, a context over
 *   several devices splits the tiles as rt_render does; the result does not depend on the device count, tile_size or the tree.
 *   A launch traces at most RT_AOV_SAMPLES_PER_LAUNCH samples; the partial sums stay on the device in sample order.
 *   Statistics: rays = primary_rays = camera segments traced, pixels, kernel_ms (max over devices), wall_ms; the rest 0.
 * rt_sample_rays: the width * height mode-2 camera rays of global sample `sample` of the frame p (jitter rule as above), row-major,
 *   tmin = RT_MIN_RAY_DISTANCE, tmax = FLT_MAX.  Other modes are RT_ERR_BAD_ARG; the tile fields are ignored; needs no scene.  For a
 *   closed 1-spp p these are the bits of rt_camera_rays(mode 1).  Statistics as rt_camera_rays (unchanged).
 * rt_denoise: C = rgb (rt_read_rgb32f layout), A, N, Z = albedo, normal, depth of `aov`.
 *   1. D = max(A, 1e-3) per channel with RT_DENOISE_DEMODULATE, else 1; c_0 = C / D.
 *   2. For i = 0 .. iterations-1, h = 2^i, every pixel p: taps q = p + h * (dx, dy), dy outer, dx inner, each -2..2, kernel
 *      k = {1/16, 1/4, 3/8, 1/4, 1/16}.  A tap outside the image or whose colour is not finite is skipped.
 *      e = |c_i(p) - c_i(q)|^2 / (sigma_color * 2^-i)^2 + |N(p) - N(q)|^2 / sigma_normal^2 + e_z + |A(p) - A(q)|^2 / sigma_albedo^2,
 *      e_z = ((Z(p) - Z(q)) / (sigma_depth * max(Z(p), Z(q))))^2, 0 when both depths are 0; w = k[dx] * k[dy] * expf(-e);
 *      c_{i+1}(p) = sum w * c_i(q) / sum w.  A pixel whose own colour is not finite is passed through unchanged.
 *   3. out = c_K * D.
 *   Buffers are classified as for the ray queries: all three host memory (staged through the context's first device), or all
 *   device memory of one of the context's devices (aov 16-byte aligned, rgb / out 4-byte aligned).  out may equal rgb.
 *   Statistics: pixels, kernel_ms, wall_ms; the rest 0.  Needs no scene.
 * Shared: all three are synchronous, first wait for an rt_dispatch_tile still in flight, and leave the last frame, rt_read_* and
 * the running image of an accumulation alone.  rt_aovs before an upload is RT_ERR_NOT_UPLOADED; NULL pointers, bad sizes and bad
 * parameters are RT_ERR_BAD_ARG and change nothing.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct rt_aov {
    float albedo[3];
    float depth;
    float normal[3];
    float coverage;
} rt_aov; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_aov) == 32, "rt_aov is 32 B");
RT_STATIC_ASSERT(offsetof(rt_aov, depth) == 12 && offsetof(rt_aov, normal) == 16 && offsetof(rt_aov, coverage) == 28, "rt_aov offsets");

#define RT_AOV_SAMPLES_PER_LAUNCH 64u /* rt_aovs: samples one kernel launch traces at most */

#define RT_DENOISE_DEMODULATE 1u       /* rt_denoise_params.flags: filter C / max(albedo, 1e-3), multiply back afterwards */
#define RT_DENOISE_MAX_ITERATIONS 10u

/* Defaults (the sweep they were chosen by). */
#define RT_DENOISE_DEFAULT_ITERATIONS 2u
#define RT_DENOISE_DEFAULT_SIGMA_COLOR 4.0f
#define RT_DENOISE_DEFAULT_SIGMA_NORMAL 1.0f
#define RT_DENOISE_DEFAULT_SIGMA_DEPTH 0.1f
#define RT_DENOISE_DEFAULT_SIGMA_ALBEDO 0.3f

typedef struct rt_denoise_params {
    uint32_t width, height;
    uint32_t iterations; /* 1 .. RT_DENOISE_MAX_ITERATIONS */
    uint32_t flags;      /* RT_DENOISE_DEMODULATE */
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo; /* > 0, finite */
} rt_denoise_params; /* 32 bytes */

RT_STATIC_ASSERT(sizeof(rt_denoise_params) == 32, "rt_denoise_params is 32 B");
RT_STATIC_ASSERT(offsetof(rt_denoise_params, flags) == 12 && offsetof(rt_denoise_params, sigma_color) == 16 &&
                     offsetof(rt_denoise_params, sigma_albedo) == 28,
                 "rt_denoise_params offsets");

/* First-hit feature buffers of the frame p: width * height records, row-major, y down. */
int rt_aovs(rt_ctx* ctx, const rt_render_params* p, rt_aov* out);

/* The frame p's mode-2 camera rays of global sample `sample`: width * height records. */
int rt_sample_rays(rt_ctx* ctx, const rt_render_params* p, uint32_t sample, rt_ray* out);

/* Edge-avoiding a-trous filter of rgb (width * height * 3 floats) guided by aov (width * height records) -> out (may equal rgb). */
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* dp, const float* rgb, const rt_aov* aov, float* out);

/* Last error text of this context (or of the failed rt_create when ctx is NULL). */
const char* rt_last_error(rt_ctx* ctx);

void rt_destroy(rt_ctx* ctx);

/* Library build info: "gfx950 strict|fast ..." */
const char* rt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
