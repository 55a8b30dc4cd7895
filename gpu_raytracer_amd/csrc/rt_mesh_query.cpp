// rt_mesh_query.cpp — queries whose input is the caller's own geometry: the triangle query (rt_hip.h "Triangle queries":
// rt_overlap_triangle; kernel in overlap_triangle.hip).  The argument checks and the batch are rt_overlap_box's, written once in
// rt_query.cpp (rti::overlap_query); this unit supplies the record and the launcher.
#include "rt_internal.h"

using namespace rti;

extern "C" {

int rt_overlap_triangle(rt_ctx* ctx, const rt_query_triangle* triangles, size_t n, uint32_t max_prims, uint32_t* prims, uint32_t* counts, uint32_t flags) {
    return overlap_query(ctx, "rt_overlap_triangle", "triangles", triangles, sizeof(rt_query_triangle), n, max_prims, prims, counts, flags,
                         rt::launch_overlap_triangle);
}

} // extern "C"
