// refit.h — host-callable launchers of refit.hip (rt_update_geometry): new vertex positions written into the triangle records and the
// node boxes of the tree a context holds, its topology kept.
#ifndef RT_REFIT_H
#define RT_REFIT_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

#define RT_REFIT_NO_RECORD 0xFFFFFFFFu // vertex-index triple of a padding record (first word)

namespace rt {

// Records with a vertex-index triple (3 words per record at vidx; RT_REFIT_NO_RECORD: padding, skipped) and finite new positions get
// v0 = p0, e1 = p1 - p0, e2 = p2 - p0 from `verts` (3 floats per vertex, 4-byte aligned).  Records with a non-finite position are left
// to launch_refit_nodes.  Asynchronous on `stream`.
hipError_t launch_refit_tris(DevTri* tris, const uint32_t* vidx, const float* verts, uint32_t n_records, hipStream_t stream);

// One level of the tree: the n nodes order[0..n-1], whose inner children were refitted by an earlier launch.  Each node's exact box (of
// the finite triangles below it) goes to boxes[2 * node] (min) / [2 * node + 1] (max); the node is re-quantised with k_db_emit's rule,
// child_base, tri_base, masks and slot order kept.  A leaf without finite triangles counts as the point (0, 0, 0); the records of
// non-finite triangles become v0 = the leaf box minimum, e1 = e2 = 0, which no ray accepts.  Asynchronous on `stream`.
hipError_t launch_refit_nodes(DevNode8* nodes, float4* boxes, DevTri* tris, const uint32_t* vidx, const float* verts, const uint32_t* order,
                              uint32_t n, hipStream_t stream);

// flag[0] |= 1 if any of the n vertex-index triples (3 words each) has only finite positions in `verts`.  Asynchronous on `stream`.
hipError_t launch_refit_any_finite(const uint32_t* vidx, uint32_t n, const float* verts, uint32_t* flag, hipStream_t stream);

} // namespace rt
#endif
