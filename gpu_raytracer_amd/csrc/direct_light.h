// direct_light.h — host-callable launcher of direct_light.hip (rt_direct_light).
#ifndef RT_DIRECT_LIGHT_H
#define RT_DIRECT_LIGHT_H

#include <hip/hip_runtime.h>

#include "device_layout.h"
#include "shadow_grid.h"

namespace rt {

// What a launch needs of rt_direct_light_params and of the context (validated by the caller).
struct DirectLightArgs {
    float bias;
    uint32_t ambient, shadows;  // RT_DIRECT_AMBIENT set / RT_DIRECT_NO_SHADOWS clear
    const DevShadowGrid* grids; // the device's light grids, one per light (null: every segment walks the tree)
    // grids != null: a point whose position lies outside [lo, hi] walks the tree (the grids' box widened: direct_light_box)
    float lo[3], hi[3];
};

// The box a point must lie in for its segments to look at the light grids built from the triangle box [box_lo, box_hi]: that box
// widened on every side by its largest extent ("Direct-light queries": the lists are supersets for segments
// whose rounding the grids' eps_eff, margins and limit_margin cover; they budget 2e-6 of the box's distances and coordinates where a
// segment inside it needs 3e-7, and within one extent of the box the need stays below two thirds of that budget).
inline void direct_light_box(const float box_lo[3], const float box_hi[3], float lo[3], float hi[3]) {
    float m = 0.0f;
    for (int a = 0; a < 3; a++) m = box_hi[a] - box_lo[a] > m ? box_hi[a] - box_lo[a] : m;
    for (int a = 0; a < 3; a++) lo[a] = box_lo[a] - m, hi[a] = box_hi[a] + m;
}

// n rt_surface_point records (32 bytes, 16-byte aligned) at `points` -> n rt_lighting records (16 bytes, 16-byte aligned) at `out`.
// counters (never null): counters[RT_CNT_SHADOW] += the shadow segments traced; with `count` (the counting variant) also
// counters[RT_CNT_NODE_VISITS] += node visits, counters[RT_CNT_TRI_TESTS] += triangle tests of the tree and of the lists,
// counters[RT_CNT_DL_GRID_ANSWERED] += segments the lists answered, counters[RT_CNT_DL_GRID_ENTRIES] += list entries they read.
// sc.n_lights <= RT_DIRECT_MAX_LIGHTS.  Asynchronous on `stream`.
#define RT_CNT_DL_GRID_ANSWERED 6u /* (slots 6 and 7 of DevCounterSlot, unused by the frames) */
#define RT_CNT_DL_GRID_ENTRIES 7u
hipError_t launch_direct_light(const DevScene& sc, const DirectLightArgs& a, const void* points, void* out, uint32_t n, bool count,
                               unsigned long long* counters, hipStream_t stream);

} // namespace rt
#endif
