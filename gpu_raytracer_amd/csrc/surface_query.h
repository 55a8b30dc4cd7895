// surface_query.h — host-callable launchers of surface_query.hip (rt_surface / rt_ambient_occlusion).
#ifndef RT_SURFACE_QUERY_H
#define RT_SURFACE_QUERY_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// n rt_ray records (32 bytes, 16-byte aligned) at `rays` -> n rt_surface_point records (32 bytes, 16-byte aligned) at `out`.
// counters != null (the counting variant): counters[RT_CNT_NODE_VISITS] += node visits, counters[RT_CNT_TRI_TESTS] += triangle tests.
// Asynchronous on `stream`.
hipError_t launch_surface_query(const DevScene& sc, const void* rays, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream);

// The parameters of rt_ambient_occlusion a launch needs (validated by the caller).
struct AoParams {
    uint32_t samples, seed;
    float max_distance, bias;
};

// rt_ambient_occlusion: n rt_surface_point records at `points`, the points first .. first + n - 1 of the caller's array (`first` enters
// each point's seed, so the result does not depend on where a batch is cut) -> unoccluded[k] += the samples of point k that are not
// occluded.  `unoccluded` (n entries) must be zero before the first launch.  n * samples lanes, at most RT_AO_LAUNCH_LANES of them per
// kernel launch; a point's samples may straddle waves and launches.  `counters` as above.  Asynchronous on `stream`.
#define RT_AO_LAUNCH_LANES 0x4000000ull /* 2^26: a launch's grid stays far below 2^32 threads, and a test can afford to cross it */
hipError_t launch_ao(const DevScene& sc, const void* points, uint64_t first, uint32_t n, const AoParams& ap, uint32_t* unoccluded,
                     unsigned long long* counters, hipStream_t stream);

// The counts of launch_ao -> visibility[k] = (float)unoccluded[k] / (float)samples (visibility != null) and counts_out[k] = unoccluded[k]
// (counts_out != null).
hipError_t launch_ao_finish(const uint32_t* unoccluded, uint32_t n, uint32_t samples, float* visibility, uint32_t* counts_out, hipStream_t stream);

} // namespace rt
#endif
