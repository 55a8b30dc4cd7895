// overlap.h — host-callable launcher of overlap.hip (rt_overlap_box).
#ifndef RT_OVERLAP_H
#define RT_OVERLAP_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

constexpr uint32_t OV_PRIMS_MAX = 32u; // RT_OVERLAP_MAX of rt_hip.h: the most entries a lane's list holds

// n rt_box records (32 bytes, 16-byte aligned) at `boxes` -> n * max_prims primitive ids (4-byte aligned) at `prims`, query-major,
// unused slots 0xFFFFFFFF, and (counts != null) n counts.  mode (overlap_rules.h OvMode): OV_LIST counts the ids listed, OV_COUNT_ALL
// every touching primitive, OV_ANY writes 0 or 1 and stops at the first (max_prims must be 0).  max_prims <= OV_PRIMS_MAX (more, or an
// unknown mode, is hipErrorInvalidValue); max_prims == 0: `prims` is not touched.  The launch sizes the dynamic LDS as stack + list.
// `counters` as launch_closest_point.  Asynchronous on `stream`.
hipError_t launch_overlap_box(const DevScene& sc, const void* boxes, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims, int mode,
                              unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
