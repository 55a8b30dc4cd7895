// sweep_triangle.h — host-callable launcher of sweep_triangle.hip (rt_sweep_triangle).
#ifndef RT_SWEEP_TRIANGLE_H
#define RT_SWEEP_TRIANGLE_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// n rt_triangle_sweep records (64 bytes, 16-byte aligned) at `sweeps` -> n rt_triangle_sweep_hit records (32 bytes, 16-byte aligned)
// at `out`.  `counters` as launch_sweep_box.  Asynchronous on `stream`.
hipError_t launch_sweep_triangle(const DevScene& sc, const void* sweeps, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
