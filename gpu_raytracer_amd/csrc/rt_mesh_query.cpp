// rt_mesh_query.cpp — queries whose input is the caller's own geometry: the triangle query (rt_hip.h "Triangle queries":
// rt_overlap_triangle; kernel in overlap_triangle.hip), the triangle sweep (rt_hip.h "Triangle sweeps": rt_sweep_triangle; kernel
// in sweep_triangle.hip) and the triangle contacts (rt_hip.h "Triangle contacts": rt_contact_triangle; kernel in
// contact_triangle.hip).  The argument checks and the batches are rt_overlap_box's, rt_sweep_box's and rt_contact_capsule's, written
// once in rt_query.cpp (rti::overlap_query, rti::record_query, rti::contact_query); this unit supplies the records and the launchers.
#include "rt_internal.h"

using namespace rti;

extern "C" {

int rt_overlap_triangle(rt_ctx* ctx, const rt_query_triangle* triangles, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts, uint32_t flags) {
    return overlap_query(ctx, "rt_overlap_triangle", "triangles", triangles, sizeof(rt_query_triangle), n, max_prims, prims, counts, flags,
                         rt::launch_overlap_triangle);
}

int rt_sweep_triangle(rt_ctx* ctx, const rt_triangle_sweep* sweeps, size_t n, rt_triangle_sweep_hit* out, uint32_t flags) {
    return record_query(ctx, "rt_sweep_triangle", {"sweeps", sweeps, sizeof(rt_triangle_sweep)}, n, {"out", out, sizeof(rt_triangle_sweep_hit)}, flags,
                        rt::launch_sweep_triangle);
}

int rt_contact_triangle(rt_ctx* ctx, const rt_triangle_contact_query* triangles, size_t n, uint32_t max_contacts, rt_triangle_contact* out,
                        uint32_t* counts, uint32_t flags) {
    return contact_query(ctx, "rt_contact_triangle", "triangles", triangles, sizeof(rt_triangle_contact_query), n, max_contacts, out, counts, flags,
                         rt::launch_contact_triangle);
}

} // extern "C"
