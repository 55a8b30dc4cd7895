// contact_triangle.h — host-callable launcher of contact_triangle.hip (rt_contact_triangle).
#ifndef RT_CONTACT_TRIANGLE_H
#define RT_CONTACT_TRIANGLE_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

constexpr uint32_t CT_CONTACT_MAX = 16u; // RT_CONTACT_MAX of rt_hip.h: the most entries a lane's list holds

// n rt_triangle_contact_query records (48 bytes, 16-byte aligned) at `triangles` -> n * max_contacts rt_triangle_contact records (32
// bytes, 16-byte aligned) at `out`, query-major, and (counts != null) n counts, as launch_contact_capsule: the records listed (mode
// CC_LIST), every candidate in range (CC_COUNT_ALL) or 1 where there is one (CC_ANY, which needs max_contacts == 0); the modes are
// CcMode of contact_capsule_rules.h.  max_contacts <= CT_CONTACT_MAX (more is hipErrorInvalidValue); max_contacts == 0: `out` is not
// touched.  The launch sizes the dynamic LDS as stack + list.  `counters` as launch_closest_point.  Asynchronous on `stream`.
hipError_t launch_contact_triangle(const DevScene& sc, const void* triangles, void* out, uint32_t* counts, uint32_t n, uint32_t max_contacts, int mode,
                                   unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
