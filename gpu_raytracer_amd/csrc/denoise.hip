// denoise.hip — the kernels of rt_aovs, rt_sample_rays and rt_denoise (include/rt_hip.h, DESIGN.md "Feature buffers and the a-trous
// denoiser").
//
// rt_aovs traces the camera samples of a frame with the frames' own first-vertex rules (device_common.h: ext_sample_ray,
// find_closest, hit_geometry) and reduces them per pixel in sample order.  One wave per 8x8 pixel block of an owned tile (block_pixel, as
// the frames), the per-lane stack in LDS as in k_render_reference.  A launch takes a bounded run of samples and keeps the partial sums in
// the output records, so that a large frame at many samples is many short kernels.
//
// rt_denoise is the edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) with albedo demodulation: one pack
// launch (rgb -> demodulated float4 colour), then one launch per iteration that ping-pongs float4 colour planes; the guides are read from
// the rt_aov records (two float4: albedo + depth, normal + coverage), and the last iteration remodulates into the rgb layout.
#include "denoise.h"

#include "device_common.h"
#include "kernels.h"

using namespace rtdev;

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// rt_aovs
// ---------------------------------------------------------------------------------------------------------------------------------
// acc per pixel: [albedo sum xyz, depth sum] [normal sum xyz, hits] while the call runs; the rt_aov record once it has ended.
__global__ __launch_bounds__(WAVE) void k_aov_samples(DevScene sc, DevFrame fr, uint32_t s0, uint32_t ns, float4* __restrict__ acc) {
    extern __shared__ uint2 s_stack[]; // lane_stack_entries * 64 64-bit entries
    const PixelCoord px = block_pixel(fr);
    if (!px.valid) return;
    uint2* stack = s_stack + threadIdx.x;
    const size_t pix = (size_t)px.y * fr.width + px.x;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (s0 > 0) {
        a = acc[2 * pix];
        b = acc[2 * pix + 1];
    }
    const bool wavefront = fr.mode != 0; // RT_MODE_LEGACY: the pixel-centre ray normalised twice
    const V3 miss = wavefront ? RT_SKY() : v3(0.0f, 0.0f, 0.0f); // the colour the mode gives a miss
    Counts cnt = {0u, 0u};
    for (uint32_t k = 0; k < ns; k++) {
        V3 o, d; // the frames' rule: the pixel's seed and the global sample index
        ext_sample_ray(fr.cam, fr.width, fr.frame_seed, fr.jitter, px.x, px.y, s0 + k, wavefront, o, d);
        const Hit hit = find_closest<false>(sc, o, d, stack, cnt);
        V3 albedo = miss;
        if (hit.prim != RT_PRIM_MISS) {
            V3 point, normal;
            uint32_t material_id;
            hit_geometry(sc, hit, o, d, point, normal, material_id);
            albedo = material_id < sc.n_materials ? ld3(sc.materials[material_id].albedo) : RT_MAGENTA(); // as shade_hit
            const V3 nf = dot(normal, d) < 0.0f ? normal : -normal; // face-forwarded, the continuation's nf
            b.x = b.x + nf.x;
            b.y = b.y + nf.y;
            b.z = b.z + nf.z;
            b.w = b.w + 1.0f;
            a.w = a.w + hit.t;
        }
        a.x = a.x + albedo.x;
        a.y = a.y + albedo.y;
        a.z = a.z + albedo.z;
    }
    if (s0 + ns == fr.n_total) { // the call's last launch: the record
        const float n = (float)fr.n_total;
        a = make_float4(a.x / n, a.y / n, a.z / n, b.w > 0.0f ? a.w / b.w : 0.0f);
        b = make_float4(b.x / n, b.y / n, b.z / n, b.w / n);
    }
    acc[2 * pix] = a;
    acc[2 * pix + 1] = b;
}

// rt_sample_rays: camera_ray of the frames at the sample's jittered position, one lane per pixel.
__global__ __launch_bounds__(256) void k_aov_sample_rays(DevCamera cam, uint32_t width, uint32_t frame_seed, uint32_t jitter, uint32_t sample,
                                                          float4* __restrict__ out, uint64_t first, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t pix = first + i;
    const uint32_t px = (uint32_t)(pix % width), py = (uint32_t)(pix / width);
    V3 o, d;
    ext_sample_ray(cam, width, frame_seed, jitter, px, py, sample, true, o, d);
    out[2 * (size_t)i] = make_float4(o.x, o.y, o.z, RT_MIN_RAY_DISTANCE);
    out[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, RT_F32_MAX);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rt_denoise
// ---------------------------------------------------------------------------------------------------------------------------------
#define DN_ALBEDO_FLOOR 1e-3f
#define DN_TILE 16 // 16 x 16 pixels per block: four waves of 4 rows x 16 columns

__device__ __forceinline__ bool finite3(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }

__global__ __launch_bounds__(256) void k_dn_pack(const float* __restrict__ rgb, const float4* __restrict__ aov, float4* __restrict__ c0, uint32_t n,
                                                 bool demodulate) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 c = make_float4(rgb[3 * (size_t)i], rgb[3 * (size_t)i + 1], rgb[3 * (size_t)i + 2], 0.0f);
    if (demodulate) {
        const float4 al = aov[2 * (size_t)i];
        c.x = c.x / fmaxf(al.x, DN_ALBEDO_FLOOR);
        c.y = c.y / fmaxf(al.y, DN_ALBEDO_FLOOR);
        c.z = c.z / fmaxf(al.z, DN_ALBEDO_FLOOR);
    }
    c0[i] = c;
}

template <bool LAST>
__global__ __launch_bounds__(256) void k_dn_atrous(rt::AtrousParams ap, const float4* __restrict__ c_in, const float4* __restrict__ aov,
                                                   float4* __restrict__ c_out, float* __restrict__ rgb_out) {
    const int x = (int)(blockIdx.x * DN_TILE + threadIdx.x), y = (int)(blockIdx.y * DN_TILE + threadIdx.y);
    const int w = (int)ap.width, h = (int)ap.height;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * ap.width + x;
    const float4 cp = c_in[p];
    const float4 ap0 = aov[2 * p], ap1 = aov[2 * p + 1]; // albedo + depth, normal + coverage
    float4 res = cp;
    if (finite3(cp)) { // a non-finite pixel is passed through and never spreads (its taps are skipped below)
        const float kern[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        const int step = 1 << ap.iter;
        float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + step * dy;
            if (qy < 0 || qy >= h) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + step * dx;
                if (qx < 0 || qx >= w) continue;
                const size_t q = (size_t)qy * ap.width + qx;
                const float4 cq = c_in[q];
                if (!finite3(cq)) continue;
                const float4 aq0 = aov[2 * q], aq1 = aov[2 * q + 1];
                const float cx = cp.x - cq.x, cy = cp.y - cq.y, cz = cp.z - cq.z;
                const float nx = ap1.x - aq1.x, ny = ap1.y - aq1.y, nz = ap1.z - aq1.z;
                const float ax = ap0.x - aq0.x, ay = ap0.y - aq0.y, az = ap0.z - aq0.z;
                float ez = 0.0f;
                if (!(ap0.w == 0.0f && aq0.w == 0.0f)) {
                    const float r = (ap0.w - aq0.w) / (ap.sigma_depth * fmaxf(ap0.w, aq0.w));
                    ez = r * r;
                }
                const float e = (cx * cx + cy * cy + cz * cz) * ap.inv_sc2 + (nx * nx + ny * ny + nz * nz) * ap.inv_sn2 + ez +
                                (ax * ax + ay * ay + az * az) * ap.inv_sa2;
                const float wq = kern[dx + 2] * kern[dy + 2] * expf(-e);
                sw = sw + wq;
                sx = sx + wq * cq.x;
                sy = sy + wq * cq.y;
                sz = sz + wq * cq.z;
            }
        }
        res = make_float4(sx / sw, sy / sw, sz / sw, 0.0f); // sw > 0: the centre tap has weight (3/8)^2
    }
    if (LAST) {
        if (ap.demodulate) {
            res.x = res.x * fmaxf(ap0.x, DN_ALBEDO_FLOOR);
            res.y = res.y * fmaxf(ap0.y, DN_ALBEDO_FLOOR);
            res.z = res.z * fmaxf(ap0.z, DN_ALBEDO_FLOOR);
        }
        rgb_out[3 * p] = res.x;
        rgb_out[3 * p + 1] = res.y;
        rgb_out[3 * p + 2] = res.z;
    } else {
        c_out[p] = res;
    }
}

} // namespace

namespace rt {

hipError_t launch_aov_samples(const DevScene& sc, const DevFrame& fr, uint32_t s0, uint32_t ns, void* acc, hipStream_t stream) {
    if (fr.n_owned_tiles == 0 || ns == 0) return hipSuccess;
    const dim3 grid(fr.n_owned_tiles * blocks_per_tile(fr.tile_size)), block(WAVE);
    const size_t lds = lane_stack_bytes(sc);
    hipLaunchKernelGGL(k_aov_samples, grid, block, lds, stream, sc, fr, s0, ns, reinterpret_cast<float4*>(acc));
    return hipGetLastError();
}

hipError_t launch_sample_rays(const DevFrame& fr, uint32_t sample, void* out, uint64_t first, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_aov_sample_rays, dim3((n + 255u) / 256u), dim3(256), 0, stream, fr.cam, fr.width, fr.frame_seed, fr.jitter, sample,
                       reinterpret_cast<float4*>(out), first, n);
    return hipGetLastError();
}

hipError_t launch_denoise_pack(const float* rgb, const void* aov, float4* c0, uint32_t n_pixels, bool demodulate, hipStream_t stream) {
    if (n_pixels == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dn_pack, dim3((n_pixels + 255u) / 256u), dim3(256), 0, stream, rgb, reinterpret_cast<const float4*>(aov), c0, n_pixels,
                       demodulate);
    return hipGetLastError();
}

hipError_t launch_denoise_atrous(const AtrousParams& ap, const float4* c_in, const void* aov, float4* c_out, float* rgb_out, bool last,
                                 hipStream_t stream) {
    const dim3 grid((ap.width + DN_TILE - 1) / DN_TILE, (ap.height + DN_TILE - 1) / DN_TILE), block(DN_TILE, DN_TILE);
    const float4* g = reinterpret_cast<const float4*>(aov);
    if (last) hipLaunchKernelGGL(k_dn_atrous<true>, grid, block, 0, stream, ap, c_in, g, c_out, rgb_out);
    else hipLaunchKernelGGL(k_dn_atrous<false>, grid, block, 0, stream, ap, c_in, g, c_out, rgb_out);
    return hipGetLastError();
}

} // namespace rt
