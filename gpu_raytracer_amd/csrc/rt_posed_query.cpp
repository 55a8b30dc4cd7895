// rt_posed_query.cpp — queries whose input is the caller's own mesh, given once, and a pose per query (rt_hip.h "Posed meshes":
// rt_overlap_mesh, rt_sweep_mesh; kernels in posed_mesh.hip).  The argument checks they share, where the mesh is placed and the batch
// are written once in rt_query.cpp (rti::pose_query); this unit supplies the records, the flags of each call and the launchers.
#include "rt_internal.h"
#include "overlap_rules.h"

using namespace rti;

namespace {

hipError_t launch_overlap(const DevScene& sc, const void* mesh, uint32_t m, const void* poses, void* pairs, void* first, uint32_t n, uint32_t mode,
                          unsigned long long* counters, hipStream_t stream) {
    return rt::launch_overlap_mesh(sc, mesh, m, poses, static_cast<uint32_t*>(pairs), static_cast<uint32_t*>(first), n, (int)mode, counters, stream);
}
hipError_t launch_sweep(const DevScene& sc, const void* mesh, uint32_t m, const void* sweeps, void* out, void*, uint32_t n, uint32_t share,
                        unsigned long long* counters, hipStream_t stream) {
    return rt::launch_sweep_mesh(sc, mesh, m, sweeps, out, n, share != 0u, counters, stream);
}

// development knob, read per call (the probe switches it): RT_POSED_MESH_SHARE=0 runs rt_sweep_mesh without the shared bound
bool share_bound() {
    const char* e = std::getenv("RT_POSED_MESH_SHARE");
    return !e || std::atoi(e) != 0;
}

} // namespace

extern "C" {

int rt_overlap_mesh(rt_ctx* ctx, const rt_query_triangle* mesh, size_t m, const rt_pose* poses, size_t n, uint32_t* pairs, uint32_t* first, uint32_t flags) {
    const char* fn = "rt_overlap_mesh";
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    const uint32_t known = RT_QUERY_COUNTERS | RT_OVERLAP_ANY;
    if (flags & ~known) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~known);
    const bool any = (flags & RT_OVERLAP_ANY) != 0;
    if (any && first) return ctx->fail(RT_ERR_BAD_ARG, "%s: RT_OVERLAP_ANY may stop at any touching triangle and needs first = NULL", fn);
    return pose_query(ctx, fn, mesh, m, {"poses", poses, sizeof(rt_pose)}, n, {"pairs", pairs, sizeof(uint32_t), 4},
                      {"first", first, sizeof(uint32_t), 4, ST_COUNTS}, flags, any ? rt::OV_ANY : rt::OV_COUNT_ALL, launch_overlap);
}

int rt_sweep_mesh(rt_ctx* ctx, const rt_query_triangle* mesh, size_t m, const rt_pose_sweep* sweeps, size_t n, rt_mesh_sweep_hit* out, uint32_t flags) {
    const char* fn = "rt_sweep_mesh";
    if (!ctx) return RT_ERR_BAD_ARG;
    if (n == 0) return RT_OK;
    if (flags & ~RT_QUERY_COUNTERS) return ctx->fail(RT_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", fn, flags & ~RT_QUERY_COUNTERS);
    return pose_query(ctx, fn, mesh, m, {"sweeps", sweeps, sizeof(rt_pose_sweep)}, n, {"out", out, sizeof(rt_mesh_sweep_hit)}, {}, flags,
                      share_bound() ? 1u : 0u, launch_sweep);
}

} // extern "C"
