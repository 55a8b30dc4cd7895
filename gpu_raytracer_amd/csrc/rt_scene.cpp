// rt_scene.cpp — what the devices hold of a scene and every step that changes it: tree build and hand-over, uploads, the lazy light
// grids, rt_prepare, rt_update_geometry and the refit's view.  Replaces the reference's wgpu uploads (src/buffers.rs:157-470).
#include "rt_internal.h"

#define RT_DEVICE_BUILD_MIN_TRIS 1024u /* below this the host build takes well under a millisecond */

namespace rti {
namespace {

template <class T>
int upload_array(rt_ctx* ctx, DevBuf<T>& dst, const std::vector<T>& src) {
    dst.reset();
    if (src.empty()) return RT_OK;
    HIPCHK(ctx, dst.reserve(src.size() * sizeof(T)));
    HIPCHK(ctx, hipMemcpy(dst.get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

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

// A tree built for every device of the context, not yet handed over (install_tree).  Per device, `dev` owns the arrays of the
// device build, or the host build's once install_tree has copied them there; whatever was not handed over is freed with it.
struct TreeBuild {
    int method = 0; // as built: 2 device, 0 / 1 host (the device build falls back to 0)
    struct Arrays { int device = -1; DevBuf<DevNode8> nodes; DevBuf<DevTri> tris; };
    std::vector<Arrays> dev; // one per device of the context, in order
    rt::BvhBuild bvh;
    uint32_t nodes = 0, tris = 0, depth = 0;
    void reset_dev(size_t n = 0) { // releases every device's arrays with that device current, and leaves n empty entries
        for (Arrays& a : dev)
            if (a.nodes.get() || a.tris.get()) (void)hipSetDevice(a.device), a = Arrays{};
        dev = std::vector<Arrays>(n);
    }
    ~TreeBuild() { reset_dev(); }
};

// The build part of a scene upload, of rt_update_geometry's rebuild (`method` from tree_method, `opt` from knob_build_options) and
// of rt_prepare's quality tree (method 0, default options).
int build_tree(rt_ctx* ctx, const std::vector<rt::BuildTri>& bt, int method, rt::BvhBuildOptions opt, TreeBuild& tb) {
    opt.method = method == 1 ? 1 : 0;
    rt::BvhBuild& bvh = tb.bvh;
    if (method == 2) {
        tb.reset_dev(ctx->devs.size());
        rt::DeviceBuild b0; // the first device's: every device must build the same tree
        bool ok = true;
        for (size_t j = 0; j < ctx->devs.size() && ok; j++) {
            DeviceState& d = ctx->devs[j];
            HIPCHK(ctx, hipSetDevice(d.device));
            rt::DeviceBuild b;
            tb.dev[j].device = d.device;
            const hipError_t e = rt::device_build(bt.data(), bt.size(), opt, d.stream, &b);
            tb.dev[j].nodes = DevBuf<DevNode8>(b.nodes, b.n_nodes * sizeof(DevNode8)); // the arrays it returns are the caller's
            tb.dev[j].tris = DevBuf<DevTri>(b.tris, b.n_tris * sizeof(DevTri));
            if (j == 0) b0 = b;
            ok = e == hipSuccess && b.depth <= RT_DEV_MAX_BVH_DEPTH && b.n_nodes <= RT_DEV_MAX_NODES && b.n_nodes == b0.n_nodes && b.n_tris == b0.n_tris;
        }
        if (!ok) { // fall back to the host build (depth bound, or the device ran out of memory for the temporaries)
            tb.reset_dev();
            method = 0;
        } else {
            tb.nodes = b0.n_nodes;
            tb.tris = b0.n_tris;
            tb.depth = b0.depth;
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
    for (auto& d : ctx->devs) {
        (void)hipSetDevice(d.device);
        d.grids = {};
    }
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
    if (copy) tb.reset_dev(ctx->devs.size());
    for (size_t j = 0; j < ctx->devs.size(); j++) {
        tb.dev[j].device = ctx->devs[j].device;
        HIPCHK(ctx, hipSetDevice(ctx->devs[j].device));
        if (j == 0 && fail_at == 0) return injected_oom(ctx);
        if (copy)
            if (int rc = upload_array(ctx, tb.dev[j].nodes, tb.bvh.nodes)) return rc;
        if (j == 0 && fail_at == 1) return injected_oom(ctx);
        if (copy)
            if (int rc = upload_array(ctx, tb.dev[j].tris, tb.bvh.tris)) return rc;
        // the copies went through the null stream and d.stream is non-blocking; launches in flight may still read the old tree
        HIPCHK(ctx, hipDeviceSynchronize());
    }
    drop_grids(ctx);
    for (size_t j = 0; j < ctx->devs.size(); j++) {
        DeviceState& d = ctx->devs[j];
        (void)hipSetDevice(d.device);
        d.scene.nodes = std::move(tb.dev[j].nodes); // (the old array is freed here)
        d.scene.tris = std::move(tb.dev[j].tris);
        d.refit = {};
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
    if (!out.empty()) HIPCHK(ctx, hipMemcpy(out.data(), d.scene.verts.get(), out.size() * sizeof(float), hipMemcpyDeviceToHost));
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
    TreeBuild tb;
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
        if ((rc = upload_array(ctx, d.scene.spheres, ds)) != RT_OK) return rc;
        if ((rc = upload_array(ctx, d.scene.lights, dl)) != RT_OK) return rc;
        if ((rc = upload_array(ctx, d.scene.materials, dm)) != RT_OK) return rc;
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

// RT_PREPARE_QUALITY_TREE: the tree of the uploaded scene rebuilt by the host builder (bvh_builder.cpp method 0: multithreaded binned SAH +
// insertion-based optimisation + the same 8-slot collapse) in place of the one rt_upload_scene* built on the device in milliseconds.  For
// scenes that stay: 0.35 s per 262 k triangles, 4.8 s for 3.8 M; frames 2 % (sponza-like) to 9 % (bistro-like) faster, same images (closest
// hits do not depend on the tree).  The light grids hold triangle records in leaf order: they go with the old tree and are built again on demand.
int prepare_quality_tree(rt_ctx* ctx) {
    if (ctx->stats.tree_build == 0 || ctx->build_tris.empty()) return RT_OK; // already the host builder's (tiny scenes, a fallback, an earlier call)
    if (int rc = sync_host_geometry(ctx)) return rc; // positions an update left on the device
    TreeBuild tb;
    if (build_tree(ctx, ctx->build_tris, 0, rt::BvhBuildOptions{}, tb) != RT_OK || tb.bvh.nodes.empty())
        return ctx->fail(RT_ERR_INTERNAL, "rt_prepare: the host build gave %zu nodes at depth %u (the device-built tree stays)", tb.bvh.nodes.size(), tb.bvh.depth);
    return install_tree(ctx, tb); // the last frame stays readable, as after RT_UPDATE_REBUILD: the targets do not depend on the tree
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
        if (n_nodes) HIPCHK(ctx, hipMemcpy(nodes.data(), d.scene.nodes.get(), nodes.size() * sizeof(DevNode8), hipMemcpyDeviceToHost));
        if (n_rec) HIPCHK(ctx, hipMemcpy(recs.data(), d.scene.tris.get(), recs.size() * sizeof(DevTri), hipMemcpyDeviceToHost));
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
        HIPCHK(ctx, hipSetDevice(d.device));
        d.refit = {};
        int rc;
        if ((rc = upload_array(ctx, d.refit.vidx, vidx)) != RT_OK || (rc = upload_array(ctx, d.refit.order, order)) != RT_OK ||
            (rc = upload_array(ctx, d.refit.dropped, dropped)) != RT_OK)
            return rc;
        HIPCHK(ctx, d.refit.boxes.reserve(std::max<size_t>(1, 2 * (size_t)n_nodes) * sizeof(float4)));
        HIPCHK(ctx, d.refit.flag.reserve(sizeof(uint32_t)));
    }
    ctx->rf_level_first = level_first;
    ctx->rf_n_dropped = (uint32_t)(dropped.size() / 3);
    ctx->rf_ready = true;
    return RT_OK;
}

// rt_update_geometry: new positions for the uploaded scene's vertices and spheres.  The tree in use is refitted (refit.hip: the
// triangle records and the node boxes follow the positions, the topology stays) or, on request or when a triangle the tree has no
// record of became finite, rebuilt through the upload's own build and hand-over (build_tree / install_tree).
// This is everything after the argument checks; a failure here leaves the context "not uploaded" (rt_update_geometry).
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
            HIPCHK(ctx, hipMemcpy2DAsync(d.scene.spheres.get(), sizeof(DevSphere), src, sizeof(rt_sphere), sizeof(rt_sphere), n_spheres, hipMemcpyDefault, d.stream));
            HIPCHK(ctx, hipStreamSynchronize(d.stream));
        }
    }
    if (!vertices || ctx->up_vertices == 0) return RT_OK;
    // vertices: a copy on every device (the refit reads it; after device input it is also what a later readback reads)
    const size_t vbytes = (size_t)ctx->up_vertices * sizeof(rt_vertex);
    for (auto& d : ctx->devs)
        if (!d.scene.verts.get()) {
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, d.scene.verts.reserve(vbytes));
        }
    if (!pv.device) {
        for (auto& d : ctx->devs) {
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, hipMemcpyAsync(d.scene.verts.get(), vertices, vbytes, hipMemcpyHostToDevice, d.stream));
        }
    } else {
        DeviceState& s = ctx->devs[pv.dev];
        HIPCHK(ctx, hipSetDevice(s.device));
        HIPCHK(ctx, hipMemcpyAsync(s.scene.verts.get(), vertices, vbytes, hipMemcpyDeviceToDevice, s.stream));
        HIPCHK(ctx, hipStreamSynchronize(s.stream));
        std::vector<float> staged;
        for (size_t j = 0; j < nd; j++) {
            if (j == pv.dev) continue;
            DeviceState& d = ctx->devs[j];
            HIPCHK(ctx, hipSetDevice(d.device));
            if (staged.empty() && hipMemcpyPeer(d.scene.verts.get(), d.device, s.scene.verts.get(), s.device, vbytes) == hipSuccess) continue;
            (void)hipGetLastError(); // no peer copy between these two: through the host
            if (staged.empty()) {
                staged.resize(3 * (size_t)ctx->up_vertices);
                HIPCHK(ctx, hipSetDevice(s.device));
                HIPCHK(ctx, hipMemcpy(staged.data(), s.scene.verts.get(), vbytes, hipMemcpyDeviceToHost));
                HIPCHK(ctx, hipSetDevice(d.device));
            }
            HIPCHK(ctx, hipMemcpy(d.scene.verts.get(), staged.data(), vbytes, hipMemcpyHostToDevice));
        }
    }
    drop_grids(ctx);
    if (!rebuild) {
        if (int rc = ensure_refit_view(ctx)) return rc;
        if (ctx->rf_n_dropped) { // a triangle the tree has no record of may have become finite: then only a new tree places it
            DeviceState& d = ctx->devs[0];
            uint32_t flag = 0;
            HIPCHK(ctx, hipSetDevice(d.device));
            HIPCHK(ctx, hipMemsetAsync(d.refit.flag.get(), 0, sizeof(uint32_t), d.stream));
            HIPCHK(ctx, rt::launch_refit_any_finite(d.refit.dropped.get(), ctx->rf_n_dropped, d.scene.verts.get(), d.refit.flag.get(), d.stream));
            HIPCHK(ctx, hipMemcpyAsync(&flag, d.refit.flag.get(), sizeof flag, hipMemcpyDeviceToHost, d.stream));
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
        TreeBuild tb;
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
        HIPCHK(ctx, rt::launch_refit_tris(d.scene.tris.get(), d.refit.vidx.get(), d.scene.verts.get(), ctx->scene_counts.n_tris, d.stream));
        for (size_t l = lv.size() - 1; l-- > 0;) // deepest level first
            HIPCHK(ctx, rt::launch_refit_nodes(d.scene.nodes.get(), d.refit.boxes.get(), d.scene.tris.get(), d.refit.vidx.get(), d.scene.verts.get(), d.refit.order.get() + lv[l], lv[l + 1] - lv[l], d.stream));
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

// Everything a device holds of the uploaded scene (the next upload and rt_destroy come through here).  The staging of the ray queries
// was sized for batches against this scene and the running sums are an image of it, so both end with it, like the refit's view and
// the light grids; the frame targets, the pipeline's lanes and the denoiser's buffers do not depend on a scene and stay.
void free_scene(DeviceState& d) {
    (void)hipSetDevice(d.device);
    d.scene = {};
    d.grids = {};
    d.rq = {};
    d.refit = {};
    d.acc = {};
    d.ad = {};
}

// Per-light triangle lists for the shadow segments of the wavefront pipeline (shadow_grid.h), rasterised on the device from the
// triangle records of the uploaded scene.  LAZY: the reference's flow (src/scene.rs:87-119 replace_with_gltf, then
// src/compute.rs:12-50 every frame) only ever renders modes 0/1, which trace no shadow segments, so rt_upload_scene* builds
// nothing; the first extended-mode frame that traces shadow segments through the pipeline pays the build once per scene (or the
// caller asks for it ahead of time: rt_prepare).  rt_stats reports what it cost (grid_build_ms) and holds (grid_bytes).
// RT_SHADOW_GRID=0 and the RT_SHADOW_GRID_* variables are development knobs only.
int ensure_grids(rt_ctx* ctx, DeviceState& d) {
    if (d.grids.tried) return RT_OK;
    if (int rc = sync_host_geometry(ctx)) return rc; // box_lo / box_hi of positions an update left on the device
    d.grids.tried = true;
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
    // an error return below frees what was built; grids.tried stays set, so the following frames render without grids and do not try again
    struct Guard {
        DeviceState& d;
        bool ok = false;
        ~Guard() { if (!ok) { d.grids = {}; d.grids.tried = true; } }
    } guard{d};
    uint64_t bytes = 0;
    bool partial = false; // a light that has triangles to cast shadows was left without a grid: then no light keeps its grid
    for (uint32_t i = 0; i < n_lights; i++) {
        rt::ShadowGridBuild gb;
        const hipError_t e = rt::shadow_grid_build(d.scene.tris.get(), tree_tris, ctx->host_lights[i], ctx->box_lo, ctx->box_hi, lopt, d.stream, &gb);
        if (e != hipSuccess) { // out of memory for a grid is not an error: the BVH answers for this light
            (void)hipGetLastError();
            gb = rt::ShadowGridBuild{};
        }
        hg[i] = gb.grid;
        if (gb.blocks) d.grids.allocs.emplace_back(gb.blocks, 0);
        if (gb.overflow) d.grids.allocs.emplace_back(gb.overflow, 0);
        if (gb.grid.kind != RT_SG_KIND_NONE) bytes += gb.bytes;
        any = any || gb.grid.kind != RT_SG_KIND_NONE;
        if (gb.grid.kind == RT_SG_KIND_NONE && gb.n_entries != 0) partial = true; // lists were counted and found too long (or too large): this light's segments walk the tree
        d.grids.info.push_back(gb);
    }
    if (any && partial) {
        // All lights or none.  The segments of a light without a grid are handed on one wave-load at a time, an atomic on the next queue's
        // counter each: a trickle when the lists leave 0.1 - 20 % to the tree, but with a whole light's segments it is millions of atomics
        // on one address per frame (bistro-like with one light of four on lists: 67 - 81 ms against 54 - 60 with no grids at all).
        HIPCHK(ctx, hipDeviceSynchronize());
        std::vector<rt::ShadowGridBuild> info = std::move(d.grids.info); // what the lists looked like stays readable (rt_debug_shadow_grid)
        d.grids = {};
        d.grids.tried = true;
        for (rt::ShadowGridBuild& g : info) g.grid = DevShadowGrid{}, g.blocks = g.overflow = nullptr, g.bytes = 0;
        d.grids.info = std::move(info);
        any = false;
        bytes = 0;
    }
    if (any) {
        if (int rc = upload_array(ctx, d.grids.table, hg)) return rc;
        HIPCHK(ctx, hipDeviceSynchronize());
    }
    if (&d == &ctx->devs[0]) { // (every device holds the same grids)
        ctx->stats.grid_bytes = bytes;
        ctx->stats.grid_build_ms = now_ms() - t0;
    }
    guard.ok = true;
    return RT_OK;
}

} // namespace rti

using namespace rti;

extern "C" {

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
