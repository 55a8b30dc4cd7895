// inside.h — host-callable launcher of inside.hip (rt_inside, rt_signed_distance).
#ifndef RT_INSIDE_H
#define RT_INSIDE_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// n rt_point_query records (16 bytes, 16-byte aligned) at `points` -> distance: n rt_nearest records (32 bytes, 16-byte aligned) at
// `out`, the sign bit of the distance set for points inside; else n bytes at `out`, 1 inside.  votes != null: n bytes, the odd votes
// of all `rays` rays of each point; null: a point stops at its majority.  rays: 1, 3, 5 or 7 (anything else is
// hipErrorInvalidValue).  counters (never null): counters[RT_CNT_SEGMENTS] += the rays traced and, `count`,
// counters[RT_CNT_NODE_VISITS] += node visits, counters[RT_CNT_TRI_TESTS] += triangle tests, of both walks.  Asynchronous on `stream`.
hipError_t launch_inside(const DevScene& sc, const void* points, void* out, uint8_t* votes, uint32_t n, uint32_t rays, bool distance, bool count,
                         unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
