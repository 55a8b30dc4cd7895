// irradiance_query.h — host-callable launcher of irradiance_query.hip (rt_irradiance).
#ifndef RT_IRRADIANCE_QUERY_H
#define RT_IRRADIANCE_QUERY_H

#include <hip/hip_runtime.h>

#include "device_layout.h"
#include "path_query.h"

namespace rt {

// The irradiance at n rt_surface_point records (32 bytes, 16-byte aligned) at `points`, a.samples directions of the cosine lobe around
// each record's normal, n * a.samples <= RT_QUERY_CHUNK: path g of the launch is sample g % samples of point g / samples; point r draws
// its direction and its path from rng_for(a.seed + first + r, a.first_sample + sample) (`first`: the index of points[0] in the caller's
// array; a.camera_draws is not looked at: the direction's two draws are the ones it names) and starts at position + normal * EXT_EPS.
// Every path leaves one (radiance, segments) record in `scratch` (n * a.samples records of 16 bytes, 16-byte aligned, also with one
// sample), and a second kernel adds each point's records in sample order from zero, scales once by 3.1415927f / (float)samples and
// writes the point's rt_irradiance_result (16 bytes, 16-byte aligned) at `out`.
// counters as launch_path_query.  Asynchronous on `stream`.
hipError_t launch_irradiance_query(const DevScene& sc, const PathArgs& a, const void* points, uint64_t first, uint32_t n, void* scratch, void* out, bool count,
                                   unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
