// denoise.h — host-callable launchers of denoise.hip: the first-hit feature buffers (rt_aovs), the frames' per-sample camera rays
// (rt_sample_rays) and the edge-avoiding a-trous filter (rt_denoise).
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include <hip/hip_runtime.h>

#include "device_layout.h"

namespace rt {

// rt_aovs: samples s0 .. s0 + ns - 1 of every pixel of fr's tile share (fr.mode, fr.jitter, fr.frame_seed and fr.cam as a frame of these
// parameters has them; fr.n_total = the samples of the whole call).  `acc` holds two float4 per frame pixel (row-major): the running sums
// (albedo.xyz, depth | normal.xyz, hits) while s0 + ns < fr.n_total, the finished rt_aov record after the launch that ends the call.  s0 == 0
// starts the sums, later launches read them.  Pixels outside the share are not touched.  Asynchronous on `stream`.
hipError_t launch_aov_samples(const DevScene& sc, const DevFrame& fr, uint32_t s0, uint32_t ns, void* acc, hipStream_t stream);

// rt_sample_rays: the mode-2 camera rays of global sample `sample` of pixels first .. first + n - 1 of a frame fr.width pixels wide
// -> n rt_ray records at `out`.  Jittered when fr.jitter != 0.
hipError_t launch_sample_rays(const DevFrame& fr, uint32_t sample, void* out, uint64_t first, uint32_t n, hipStream_t stream);

// rt_denoise.  pack: rgb (3 floats per pixel, any 4-byte alignment) -> c_0 = C / D as float4 per pixel.  D = max(albedo, 1e-3) per
// channel when `demodulate`, else 1; albedo is read from the rt_aov records at `aov` (16-byte aligned).
hipError_t launch_denoise_pack(const float* rgb, const void* aov, float4* c0, uint32_t n_pixels, bool demodulate, hipStream_t stream);

// One a-trous iteration `iter` (tap spacing 2^iter) from c_in.  Not `last`: writes c_out (float4 per pixel).  `last`: writes the
// remodulated result c * D to rgb_out (3 floats per pixel).  inv_* are 1 / sigma^2 of rt_denoise_params.
struct AtrousParams {
    uint32_t width, height, iter;
    float inv_sc2; // 1 / (sigma_color * 2^-iter)^2
    float inv_sn2, sigma_depth, inv_sa2;
    bool demodulate;
};
hipError_t launch_denoise_atrous(const AtrousParams& ap, const float4* c_in, const void* aov, float4* c_out, float* rgb_out, bool last,
                                 hipStream_t stream);

} // namespace rt
#endif
