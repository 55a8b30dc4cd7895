// adaptive.h — host-callable launchers of adaptive.hip: the passes of rt_render_adaptive around the frame kernels (DESIGN.md sections 4, 5).
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// Selection of device share fr (fr.n_owned_tiles tiles): every owned 8x8 block gets the mask of its pixels that take samples this call
// (the rule of rt_hip.h with fr.ad_threshold / fr.ad_min_samples, from tg.run_sum / tg.run_odd) in mask[owned block]; the blocks with any
// are listed in block order in blocks[0 .. counts[0]), and counts[1] is the number of pixels that take samples.  mask and blocks hold one
// entry per owned block.  Asynchronous on `stream`.
hipError_t launch_ad_select(const DevFrame& fr, const DevTargets& tg, unsigned long long* mask, uint32_t* blocks, unsigned long long* counts,
                            hipStream_t stream);

// The image of share fr from the running sums: every owned pixel's targets get S / n (store_image, as the frame kernels write them).
hipError_t launch_ad_image(const DevFrame& fr, const DevTargets& tg, hipStream_t stream);

// rt_read_adaptive: n_pixels rt_adaptive_pixel records (S, n, H, error) at `out` from the running sums run_sum / run_odd (float4 each).
hipError_t launch_ad_records(const float* run_sum, const float* run_odd, void* out, size_t n_pixels, hipStream_t stream);

} // namespace rt
#endif
