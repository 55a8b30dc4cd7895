// sweep_capsule.h — host-callable launcher of sweep_capsule.hip (rt_sweep_capsule).
#ifndef RT_SWEEP_CAPSULE_H
#define RT_SWEEP_CAPSULE_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// n rt_capsule_sweep records (48 bytes, 16-byte aligned) at `sweeps` -> n rt_capsule_sweep_hit records (32 bytes, 16-byte aligned) at `out`.
// counters != null (the counting variant): counters[RT_CNT_NODE_VISITS] += node visits, counters[RT_CNT_TRI_TESTS] += triangle tests.
// Asynchronous on `stream`.
hipError_t launch_sweep_capsule(const DevScene& sc, const void* sweeps, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
