// path_query.h — host-callable launchers of path_query.hip (rt_radiance).
#ifndef RT_PATH_QUERY_H
#define RT_PATH_QUERY_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// What a launch needs of rt_path_params (validated by the caller).
struct PathArgs {
    uint32_t samples, max_bounces, seed, first_sample;
    uint32_t shadows, camera_draws; // RT_PATH_NO_SHADOWS clear / RT_PATH_CAMERA_DRAWS set
};

// The paths of n rt_ray records (32 bytes, 16-byte aligned) at `rays`, a.samples each, n * a.samples <= RT_QUERY_CHUNK: path g of the
// launch is sample g % samples of ray g / samples, and ray r draws from rng_for(a.seed + first + r, a.first_sample + sample) (`first`:
// the index of rays[0] in the caller's array).  Every path leaves one (radiance, segments) record in `scratch` (n * a.samples records
// of 16 bytes, 16-byte aligned), and a second kernel adds each ray's records in sample order from zero, divides by (float)samples and
// writes the ray's rt_path_result (16 bytes, 16-byte aligned) at `out`.  With a.samples == 1 the trace kernel writes `out` itself and
// `scratch` is not touched.
// counters (never null): counters[RT_CNT_CAMERA] += first segments, counters[RT_CNT_CONTINUATION] += continuation segments,
// counters[RT_CNT_SHADOW] += shadow segments, one atomic per wave and counter; with `count` (the counting variant) also
// counters[RT_CNT_NODE_VISITS] and counters[RT_CNT_TRI_TESTS].  Asynchronous on `stream`.
hipError_t launch_path_query(const DevScene& sc, const PathArgs& a, const void* rays, uint64_t first, uint32_t n, void* scratch, void* out, bool count,
                             unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
