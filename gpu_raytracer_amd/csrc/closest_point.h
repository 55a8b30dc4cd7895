// closest_point.h — host-callable launcher of closest_point.hip (rt_closest_point).
#ifndef RT_CLOSEST_POINT_H
#define RT_CLOSEST_POINT_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// n rt_point_query records (16 bytes, 16-byte aligned) at `points` -> n rt_nearest records (32 bytes, 16-byte aligned) at `out`.
// counters != null (the counting variant): counters[RT_CNT_NODE_VISITS] += node visits, counters[RT_CNT_TRI_TESTS] += triangle tests.
// Asynchronous on `stream`.
hipError_t launch_closest_point(const DevScene& sc, const void* points, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
