// overlap_obb.h — host-callable launcher of overlap_obb.hip (rt_overlap_obb).
#ifndef RT_OVERLAP_OBB_H
#define RT_OVERLAP_OBB_H

#include "overlap.h"

namespace rt {

// n rt_obb records (48 bytes, 16-byte aligned) at `boxes`; everything else as launch_overlap_box (overlap.h).
hipError_t launch_overlap_obb(const DevScene& sc, const void* boxes, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims, int mode,
                              unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
