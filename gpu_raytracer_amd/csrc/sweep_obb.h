// sweep_obb.h — host-callable launcher of sweep_obb.hip (rt_sweep_obb).
#ifndef RT_SWEEP_OBB_H
#define RT_SWEEP_OBB_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// n rt_obb_sweep records (64 bytes, 16-byte aligned) at `sweeps` -> n rt_box_sweep_hit records (32 bytes, 16-byte aligned) at `out`.
// `counters` as launch_sweep_box.  Asynchronous on `stream`.
hipError_t launch_sweep_obb(const DevScene& sc, const void* sweeps, void* out, uint32_t n, unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
