// rt_readback.cpp — bringing a frame back: the shares of the devices put together, the epilogue through pinned staging, rt_read_*.
// Replaces the reference's channel textures (src/renderer.rs:452-475).
#include "rt_internal.h"

namespace rti {
// Copy `elem` bytes per pixel of the tiles first, first + stride, ... (n_owned of them) of a w x h frame of tile_size tiles, tiles_x
// per row, from `src` to `dst` (both full frames, row-major).
void copy_share(uint8_t* dst, const uint8_t* src, size_t elem, uint32_t w, uint32_t h, uint32_t ts, uint32_t tiles_x, uint32_t first, uint32_t stride,
                uint32_t n_owned) {
    for (uint32_t k = 0; k < n_owned; k++) {
        uint32_t tile = first + k * stride;
        uint32_t ty = tile / tiles_x, tx = tile % tiles_x;
        uint32_t x0 = tx * ts, y0 = ty * ts, tw = std::min(ts, w - x0), th = std::min(ts, h - y0);
        for (uint32_t y = y0; y < y0 + th; y++)
            std::memcpy(dst + ((size_t)y * w + x0) * elem, src + ((size_t)y * w + x0) * elem, (size_t)tw * elem);
    }
}

namespace {

// Copy `elem` bytes per pixel of every device's owned tiles into `out` (full frame, row-major), from the target `which` or, with
// `per_device`, from a full-frame buffer per device.
int gather(rt_ctx* ctx, uint8_t* out, size_t elem, int which /*0 rgba32f, 1..3 chan, 4 prim, 5 t*/, void* const* per_device = nullptr) {
    uint32_t w = ctx->frame_w, h = ctx->frame_h;
    size_t n = (size_t)w * h;
    std::vector<uint8_t> tmp;
    for (size_t j = 0; j < ctx->devs.size(); j++) {
        DeviceState& d = ctx->devs[j];
        if (d.fb.w != w || d.fb.h != h || d.n_owned == 0) continue;
        const void* src = which == 0 ? (const void*)d.fb.rgba32f.get() : which <= 3 ? (const void*)d.fb.chan[which - 1].get() : which == 4 ? (const void*)d.fb.prim_id.get() : (const void*)d.fb.hit_t.get();
        if (per_device && !per_device[j]) continue;
        if (per_device) src = per_device[j];
        HIPCHK(ctx, hipSetDevice(d.device));
        bool all = d.tile_stride == 1 && d.tile_first == 0;
        if (all) {
            HIPCHK(ctx, hipMemcpy(out, src, n * elem, hipMemcpyDeviceToHost));
            continue;
        }
        tmp.resize(n * elem);
        HIPCHK(ctx, hipMemcpy(tmp.data(), src, n * elem, hipMemcpyDeviceToHost));
        copy_share(out, tmp.data(), elem, w, h, ctx->frame_tile, ctx->frame_tiles_x, d.tile_first, d.tile_stride, d.n_owned);
    }
    return RT_OK;
}

// The read-back staging of device d (current): at least `bytes` on the device and pinned on the host.
int ensure_readback(rt_ctx* ctx, DeviceState& d, size_t bytes) {
    HIPCHK(ctx, d.fb.readback_dev.reserve(bytes));
    HIPCHK(ctx, d.fb.readback_host.reserve(bytes));
    return RT_OK;
}

// Whole frame on one device: run the epilogue there and bring the result back through pinned staging
// (`which` 0: packed rgb32f, 1: combined rgba8).  Returns RT_OK, an error, or 1 when the caller must use the gather path.
int read_epilogue(rt_ctx* ctx, int which, void* out, size_t bytes) {
    if (ctx->devs.size() != 1) return 1;
    DeviceState& d = ctx->devs[0];
    if (d.fb.w != ctx->frame_w || d.fb.h != ctx->frame_h || !(d.tile_stride == 1 && d.tile_first == 0)) return 1;
    HIPCHK(ctx, hipSetDevice(d.device));
    if (int rc = ensure_readback(ctx, d, bytes)) return rc;
    const size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    if (which == 0) HIPCHK(ctx, rt::launch_pack_rgb32f(d.fb.rgba32f.get(), (float*)d.fb.readback_dev.get(), n, d.stream));
    else HIPCHK(ctx, rt::launch_combine_rgba8(d.fb.chan[0].get(), d.fb.chan[1].get(), d.fb.chan[2].get(), (uint8_t*)d.fb.readback_dev.get(), n, d.stream));
    HIPCHK(ctx, hipMemcpyAsync(d.fb.readback_host.get(), d.fb.readback_dev.get(), bytes, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(ctx, hipStreamSynchronize(d.stream));
    std::memcpy(out, d.fb.readback_host.get(), bytes);
    return RT_OK;
}

} // namespace

// A dispatch sequence runs on the context's first device and starts from the textures as they are (tiles that are
// not dispatched keep their texels, like the reference's storage textures).  After an rt_render that was split over
// several devices those texels are spread over the devices: bring them together on the first one (a slow path through
// host memory, taken once at the transition).
int consolidate_on_first_device(rt_ctx* ctx, uint32_t w, uint32_t h) {
    if (ctx->devs.size() < 2 || ctx->frame_w != w || ctx->frame_h != h) return RT_OK;
    DeviceState& d0 = ctx->devs[0];
    if (d0.fb.w != w || d0.fb.h != h) return RT_OK;
    bool spread = false;
    for (size_t j = 1; j < ctx->devs.size(); j++) spread = spread || (ctx->devs[j].n_owned > 0 && ctx->devs[j].fb.w == w && ctx->devs[j].fb.h == h);
    if (!spread) return RT_OK;
    for (auto& d : ctx->devs) {
        HIPCHK(ctx, hipSetDevice(d.device));
        HIPCHK(ctx, hipStreamSynchronize(d.stream));
    }
    const size_t n = (size_t)w * h;
    std::vector<uint8_t> buf;
    HIPCHK(ctx, hipSetDevice(d0.device));
    for (int which = 0; which < 6; which++) {
        const size_t elem = which == 0 ? 16 : 4;
        void* dst = which == 0 ? (void*)d0.fb.rgba32f.get() : which <= 3 ? (void*)d0.fb.chan[which - 1].get() : which == 4 ? (void*)d0.fb.prim_id.get() : (void*)d0.fb.hit_t.get();
        buf.resize(n * elem);
        HIPCHK(ctx, hipSetDevice(d0.device));
        HIPCHK(ctx, hipMemcpy(buf.data(), dst, n * elem, hipMemcpyDeviceToHost)); // what the first device holds outside everyone's tiles
        int rc = gather(ctx, buf.data(), elem, which);
        if (rc != RT_OK) return rc;
        HIPCHK(ctx, hipSetDevice(d0.device));
        HIPCHK(ctx, hipMemcpy(dst, buf.data(), n * elem, hipMemcpyHostToDevice));
    }
    HIPCHK(ctx, hipDeviceSynchronize());
    d0.tile_first = 0;
    d0.tile_stride = 1;
    d0.n_owned = ctx->frame_tiles_x * ctx->frame_tiles_y;
    for (size_t j = 1; j < ctx->devs.size(); j++) ctx->devs[j].n_owned = 0;
    return RT_OK;
}

} // namespace rti

using namespace rti;

extern "C" {

int rt_read_rgb32f(rt_ctx* ctx, float* out, size_t n_floats) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->frame_valid) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_read_rgb32f: nothing rendered yet");
    size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    if (!out || n_floats != n * 3) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_rgb32f: expected %zu floats, got %zu", n * 3, n_floats);
    int rc = read_epilogue(ctx, 0, out, n * 12);
    if (rc <= 0) return rc;
    std::vector<float> tmp(n * 4, 0.0f);
    rc = gather(ctx, reinterpret_cast<uint8_t*>(tmp.data()), 16, 0);
    if (rc != RT_OK) return rc;
    for (size_t i = 0; i < n; i++) {
        out[3 * i + 0] = tmp[4 * i + 0];
        out[3 * i + 1] = tmp[4 * i + 1];
        out[3 * i + 2] = tmp[4 * i + 2];
    }
    return RT_OK;
}

int rt_read_rgba8_channels(rt_ctx* ctx, uint8_t* red, uint8_t* green, uint8_t* blue, size_t n_bytes_each) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->frame_valid) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_read_rgba8_channels: nothing rendered yet");
    size_t n = (size_t)ctx->frame_w * ctx->frame_h * 4;
    if (n_bytes_each != n) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_rgba8_channels: expected %zu bytes each, got %zu", n, n_bytes_each);
    uint8_t* outs[3] = {red, green, blue};
    for (int c = 0; c < 3; c++) {
        if (!outs[c]) continue;
        std::memset(outs[c], 0, n);
        int rc = gather(ctx, outs[c], 4, 1 + c);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

int rt_read_rgba8_combined(rt_ctx* ctx, uint8_t* out, size_t n_bytes) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->frame_valid) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_read_rgba8_combined: nothing rendered yet");
    size_t n = (size_t)ctx->frame_w * ctx->frame_h * 4;
    if (!out || n_bytes != n) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_rgba8_combined: expected %zu bytes, got %zu", n, n_bytes);
    int rc = read_epilogue(ctx, 1, out, n);
    if (rc <= 0) return rc;
    std::vector<uint8_t> r(n), g(n), b(n);
    rc = rt_read_rgba8_channels(ctx, r.data(), g.data(), b.data(), n);
    if (rc != RT_OK) return rc;
    for (size_t i = 0; i < n; i += 4) { // main_fs, shader/src/lib.rs:383-388
        out[i + 0] = r[i + 0];
        out[i + 1] = g[i + 1];
        out[i + 2] = b[i + 2];
        out[i + 3] = 255;
    }
    return RT_OK;
}

int rt_read_hits(rt_ctx* ctx, uint32_t* prim_ids, float* t, size_t n_pixels) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->frame_valid) return ctx->fail(RT_ERR_NOT_UPLOADED, "rt_read_hits: nothing rendered yet");
    size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    if (n_pixels != n) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_hits: expected %zu pixels, got %zu", n, n_pixels);
    int rc;
    if (prim_ids) {
        std::memset(prim_ids, 0xFF, n * 4);
        if ((rc = gather(ctx, reinterpret_cast<uint8_t*>(prim_ids), 4, 4)) != RT_OK) return rc;
    }
    if (t) {
        std::memset(t, 0, n * 4);
        if ((rc = gather(ctx, reinterpret_cast<uint8_t*>(t), 4, 5)) != RT_OK) return rc;
    }
    return RT_OK;
}

int rt_read_adaptive(rt_ctx* ctx, rt_adaptive_pixel* out, size_t n_pixels) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (int rcp = sync_pending(ctx)) return rcp;
    if (!ctx->acc_samples || !ctx->acc_key.adaptive) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_adaptive: the context has no adaptive running image");
    const size_t n = (size_t)ctx->frame_w * ctx->frame_h;
    if (!out || n_pixels != n) return ctx->fail(RT_ERR_BAD_ARG, "rt_read_adaptive: expected %zu records, got %zu", n, n_pixels);
    static_assert(sizeof(rt_adaptive_pixel) == 32, "two float4 per record (k_ad_records)");
    // every device's records of the whole frame (those outside its share are never copied), then its share of them into `out`
    std::vector<void*> src(ctx->devs.size(), nullptr);
    for (size_t j = 0; j < ctx->devs.size(); j++) {
        DeviceState& d = ctx->devs[j];
        if (d.fb.w != ctx->frame_w || d.fb.h != ctx->frame_h || d.n_owned == 0 || !d.acc.run_sum.get() || !d.acc.run_odd.get()) continue;
        HIPCHK(ctx, hipSetDevice(d.device));
        if (int rc = ensure_readback(ctx, d, n * sizeof(rt_adaptive_pixel))) return rc;
        HIPCHK(ctx, rt::launch_ad_records(d.acc.run_sum.get(), d.acc.run_odd.get(), d.fb.readback_dev.get(), n, d.stream));
        HIPCHK(ctx, hipStreamSynchronize(d.stream));
        src[j] = d.fb.readback_dev.get();
    }
    std::memset(out, 0, n * sizeof(rt_adaptive_pixel));
    return gather(ctx, reinterpret_cast<uint8_t*>(out), sizeof(rt_adaptive_pixel), 0, src.data());
}

int rt_accumulated_samples(rt_ctx* ctx, uint32_t* samples) {
    if (!ctx) return RT_ERR_BAD_ARG;
    if (!samples) return ctx->fail(RT_ERR_BAD_ARG, "rt_accumulated_samples: null output");
    *samples = ctx->acc_samples;
    return RT_OK;
}

} // extern "C"
