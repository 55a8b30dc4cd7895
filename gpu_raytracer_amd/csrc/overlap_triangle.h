// overlap_triangle.h — host-callable launcher of overlap_triangle.hip (rt_overlap_triangle).
#ifndef RT_OVERLAP_TRIANGLE_H
#define RT_OVERLAP_TRIANGLE_H

#include "overlap.h"

namespace rt {

// n rt_query_triangle records (48 bytes, 16-byte aligned) at `triangles`; everything else as launch_overlap_box (overlap.h).
hipError_t launch_overlap_triangle(const DevScene& sc, const void* triangles, uint32_t* prims, uint32_t* counts, uint32_t n, uint32_t max_prims,
                                   int mode, unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
