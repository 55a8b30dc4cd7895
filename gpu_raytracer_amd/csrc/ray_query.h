// ray_query.h — host-callable launchers of ray_query.hip (rt_intersect / rt_occluded / rt_intersect_all / rt_camera_rays).
#ifndef RT_RAY_QUERY_H
#define RT_RAY_QUERY_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// n rt_ray records (32 bytes, 16-byte aligned) at `rays` -> n rt_hit records (16 bytes) at `out`, or n bytes (0/1) when any_hit.
// counters != null (the counting variant): counters[RT_CNT_NODE_VISITS] += node visits, counters[RT_CNT_TRI_TESTS] += triangle tests.  Asynchronous on `stream`.
hipError_t launch_ray_query(const DevScene& sc, const void* rays, void* out, uint32_t n, bool any_hit, unsigned long long* counters,
                            hipStream_t stream);

// rt_intersect_all: n rt_ray records at `rays` -> n * max_hits rt_hit records at `hits`, ray-major (not touched when max_hits == 0), and,
// counts != null, n counts: the records listed per ray, or with count_all every candidate in the ray's range.  max_hits <=
// RT_MULTI_HIT_MAX: the launch sizes the dynamic LDS as stack + list.  `counters` as above.  Asynchronous on `stream`.
hipError_t launch_ray_query_all(const DevScene& sc, const void* rays, void* hits, uint32_t* counts, uint32_t n, uint32_t max_hits, bool count_all,
                                unsigned long long* counters, hipStream_t stream);

// The pixel-centre camera rays of pixels first .. first + n - 1 of a frame `width` pixels wide (row-major) -> n rt_ray records at `out`.
hipError_t launch_camera_rays(const DevCamera& cam, uint32_t width, bool wavefront, void* out, uint64_t first, uint32_t n, hipStream_t stream);

} // namespace rt
#endif
