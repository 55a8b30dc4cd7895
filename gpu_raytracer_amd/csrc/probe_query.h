// probe_query.h — host-callable launcher of probe_query.hip (rt_radiance_sh).
#ifndef RT_PROBE_QUERY_H
#define RT_PROBE_QUERY_H

#include <hip/hip_runtime.h>

#include "device_layout.h"
#include "path_query.h"

namespace rt {

// The radiance fields of n rt_probe records (16 bytes, 16-byte aligned) at `probes`, a.samples directions each, n * a.samples <=
// RT_QUERY_CHUNK: path g of the launch is sample g % samples of probe g / samples; probe r draws its direction and its path from
// rng_for(a.seed + first + r, a.first_sample + sample) (`first`: the index of probes[0] in the caller's array; a.camera_draws is not
// looked at: the direction's two draws are the ones it names).  Every path leaves one (radiance, segments) record in `scratch`
// (n * a.samples records of 16 bytes, 16-byte aligned), and a second kernel regenerates each direction, adds radiance * basis in sample
// order from zero, scales once and writes the probe's rt_sh9 (112 bytes, 16-byte aligned) at `out`.
// counters as launch_path_query.  Asynchronous on `stream`.
hipError_t launch_probe_query(const DevScene& sc, const PathArgs& a, const void* probes, uint64_t first, uint32_t n, void* scratch, void* out, bool count,
                              unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
