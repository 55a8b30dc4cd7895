// posed_mesh.h — host-callable launchers of posed_mesh.hip (rt_overlap_mesh, rt_sweep_mesh).
#ifndef RT_POSED_MESH_H
#define RT_POSED_MESH_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// The lanes that serve one pose of a mesh of m triangles: 1 for m = 1, else the smallest power of two >= m, at most 64.
inline uint32_t posed_mesh_group(uint32_t m) {
    uint32_t g = 1u;
    while (g < m && g < 64u) g <<= 1;
    return g;
}

// m rt_query_triangle records (48 bytes, 16-byte aligned) at `mesh`, on the device; n rt_pose records (32 bytes) at `poses` -> n
// words at `pairs` and, unless null, n words at `first`.  mode: OV_COUNT_ALL or OV_ANY (overlap_rules.h).  `counters` as
// launch_sweep_box.  Asynchronous on `stream`.
hipError_t launch_overlap_mesh(const DevScene& sc, const void* mesh, uint32_t m, const void* poses, uint32_t* pairs, uint32_t* first, uint32_t n, int mode,
                               unsigned long long* counters, hipStream_t stream);
// ... n rt_pose_sweep records (48 bytes) at `sweeps` -> n rt_mesh_sweep_hit records (32 bytes, 16-byte aligned) at `out`.  share: the
// lanes of a pose cull by the body's best time so far (mesh_pose_rules.h, rule 4); the bytes of the answer are the same without.
hipError_t launch_sweep_mesh(const DevScene& sc, const void* mesh, uint32_t m, const void* sweeps, void* out, uint32_t n, bool share,
                             unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
