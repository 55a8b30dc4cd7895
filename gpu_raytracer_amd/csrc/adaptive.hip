// adaptive.hip — the passes of rt_render_adaptive around the frame kernels (adaptive.h; the rule is stated in rt_hip.h and DESIGN.md
// section 5, its code is device_common.h ad_error / ad_active):
//   k_ad_select   one wave per owned 8x8 block: the rule for its 64 pixels, __ballot -> the block's mask of pixels that take samples
//   k_ad_compact  one workgroup: the blocks with a non-empty mask, listed in block order (a scan over per-wave ballots), and the counts
//                 the host reads to size the call (the pipeline's batch, path slots and queues scale with the live blocks)
//   k_ad_image    one wave per owned block: S / n into the targets, through the frame kernels' own store (store_image)
//   k_ad_records  one thread per pixel: rt_read_adaptive's records
#include "adaptive.h"

#include <algorithm>

#include "../../include/rt_hip.h"
#include "device_common.h"
#include "kernels.h"

using namespace rtdev;

namespace {

__global__ __launch_bounds__(WAVE) void k_ad_select(DevFrame fr, DevTargets tg, unsigned long long* __restrict__ mask) {
    const PixelCoord px = block_pixel(fr);
    bool active = false;
    if (px.valid) active = ad_active(ad_load(fr, tg, (size_t)px.y * fr.width + px.x), fr.ad_threshold, fr.ad_min_samples);
    const unsigned long long m = __ballot(active);
    if (threadIdx.x == 0) mask[blockIdx.x] = m;
}

#define AD_COMPACT_THREADS 1024u
__global__ __launch_bounds__(AD_COMPACT_THREADS) void k_ad_compact(const unsigned long long* __restrict__ mask, uint32_t n_blocks, uint32_t* __restrict__ blocks,
                                                                    unsigned long long* __restrict__ counts) {
    constexpr uint32_t N_WAVES = AD_COMPACT_THREADS / WAVE;
    __shared__ uint32_t s_wave[N_WAVES];
    __shared__ unsigned long long s_pixels[N_WAVES];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint32_t listed = 0;
    uint32_t pixels = 0; // (at most 64 per chunk and thread)
    unsigned long long pixels_all = 0;
    for (uint32_t c = 0; c < n_blocks; c += AD_COMPACT_THREADS) {
        const uint32_t i = c + t;
        const unsigned long long m = i < n_blocks ? mask[i] : 0ull;
        pixels = (uint32_t)__popcll(m);
        pixels_all += wave_sum(pixels); // (lane 0's is the wave's)
        const bool live = m != 0ull;
        const unsigned long long bal = __ballot(live);
        if (lane == 0) s_wave[w] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t k = 0; k < N_WAVES; k++) {
            const uint32_t v = s_wave[k];
            before += k < w ? v : 0u;
            total += v;
        }
        if (live) blocks[listed + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = i;
        listed += total;
        __syncthreads(); // (s_wave is written again)
    }
    if (lane == 0) s_pixels[w] = pixels_all;
    __syncthreads();
    if (t == 0) {
        unsigned long long p = 0;
        for (uint32_t k = 0; k < N_WAVES; k++) p += s_pixels[k];
        counts[0] = listed;
        counts[1] = p;
    }
}

__global__ __launch_bounds__(WAVE) void k_ad_image(DevFrame fr, DevTargets tg) {
    const PixelCoord px = block_pixel(fr);
    if (!px.valid) return;
    const size_t pix = (size_t)px.y * fr.width + px.x;
    const float4 s = reinterpret_cast<const float4*>(tg.run_sum)[pix];
    store_image(tg, pix, v3(s.x, s.y, s.z), s.w);
}

__global__ __launch_bounds__(256) void k_ad_records(const float4* __restrict__ run_sum, const float4* __restrict__ run_odd, float4* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float4 s = run_sum[i], h = run_odd[i];
        const uint32_t n_samples = (uint32_t)s.w;
        const float e = n_samples ? ad_error(v3(s.x, s.y, s.z), v3(h.x, h.y, h.z), n_samples) : 0.0f;
        out[2 * i] = s;
        out[2 * i + 1] = make_float4(h.x, h.y, h.z, e);
    }
}

} // namespace

namespace rt {

hipError_t launch_ad_select(const DevFrame& fr, const DevTargets& tg, unsigned long long* mask, uint32_t* blocks, unsigned long long* counts,
                            hipStream_t stream) {
    const uint32_t n_blocks = fr.n_owned_tiles * blocks_per_tile(fr.tile_size);
    if (n_blocks) hipLaunchKernelGGL(k_ad_select, dim3(n_blocks), dim3(WAVE), 0, stream, fr, tg, mask);
    hipLaunchKernelGGL(k_ad_compact, dim3(1), dim3(AD_COMPACT_THREADS), 0, stream, mask, n_blocks, blocks, counts);
    return hipGetLastError();
}

hipError_t launch_ad_image(const DevFrame& fr, const DevTargets& tg, hipStream_t stream) {
    const uint32_t n_blocks = fr.n_owned_tiles * blocks_per_tile(fr.tile_size);
    if (n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ad_image, dim3(n_blocks), dim3(WAVE), 0, stream, fr, tg);
    return hipGetLastError();
}

hipError_t launch_ad_records(const float* run_sum, const float* run_odd, void* out, size_t n_pixels, hipStream_t stream) {
    if (n_pixels == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n_pixels + 255) / 256, 4096);
    hipLaunchKernelGGL(k_ad_records, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float4*>(run_sum), reinterpret_cast<const float4*>(run_odd),
                       reinterpret_cast<float4*>(out), n_pixels);
    return hipGetLastError();
}

} // namespace rt
