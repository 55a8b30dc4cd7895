// closest_point_all.h — host-callable launcher of closest_point_all.hip (rt_closest_point_all).
#ifndef RT_CLOSEST_POINT_ALL_H
#define RT_CLOSEST_POINT_ALL_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

constexpr uint32_t CP_NEAREST_MAX = 16u; // RT_NEAREST_MAX of rt_hip.h: the most entries a lane's list holds

// n rt_point_query records (16 bytes, 16-byte aligned) at `points` -> n * max_nearest rt_nearest records (32 bytes, 16-byte aligned) at
// `out`, query-major, and (counts != null) n counts: the records listed, or with count_all every candidate in range.  max_nearest <=
// CP_NEAREST_MAX (more is hipErrorInvalidValue); max_nearest == 0: `out` is not touched.  The launch sizes the dynamic LDS as stack +
// list.  `counters` as launch_closest_point.  Asynchronous on `stream`.
hipError_t launch_closest_point_all(const DevScene& sc, const void* points, void* out, uint32_t* counts, uint32_t n, uint32_t max_nearest, bool count_all,
                                    unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
