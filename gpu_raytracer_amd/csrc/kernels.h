// kernels.h — host-callable launchers of kernels.hip.
#ifndef RT_KERNELS_H
#define RT_KERNELS_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

uint32_t blocks_per_tile(uint32_t tile_size);

// Modes 0/1 (reference semantics).  Asynchronous on `stream`.
hipError_t launch_render_reference(const DevScene& sc, const DevFrame& fr, const DevTargets& tg, bool counters, hipStream_t stream);

// What renders one device's share of a frame (run_frame's choice): the reference-mode kernel (modes 0/1); in the extended mode the
// one-pass kernel (primary rays over a tiny tree: the nested-loop kernel by rule), the queue pipeline (wavefront.h), or one of the
// megakernels: the state machine (RT_FLAG_KERNEL_SM, and the fallback for frames the pipeline cannot address) or the nested loops (RT_FLAG_KERNEL_V1).
enum class FrameKernel { REFERENCE, SINGLE_PASS, PIPELINE, MEGAKERNEL_SM, MEGAKERNEL_V1 };

// Mode 2 (extended: jittered spp, shadow rays, bounces) by `kernel`: SINGLE_PASS, MEGAKERNEL_SM or MEGAKERNEL_V1.  Segment counts in
// tg.counters (DevCounterSlot).  Asynchronous on `stream`.
hipError_t launch_render_extended(const DevScene& sc, const DevFrame& fr, const DevTargets& tg, FrameKernel kernel, bool counters, hipStream_t stream);

// Read-back epilogues (single device owning the whole frame).  combine: main_fs of the reference (shader/src/lib.rs:383-388),
// out = (red_tex.x, green_tex.y, blue_tex.z, 255).  pack: rgba32f -> tightly packed rgb32f.
hipError_t launch_combine_rgba8(const uint8_t* red, const uint8_t* green, const uint8_t* blue, uint8_t* out, size_t n_pixels, hipStream_t stream);
hipError_t launch_pack_rgb32f(const float* rgba, float* rgb, size_t n_pixels, hipStream_t stream);

} // namespace rt
#endif
