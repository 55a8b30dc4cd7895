// refit.hip — rt_update_geometry's refit: the tree a context holds follows new vertex positions with its topology unchanged.
//
// Closest hits do not depend on the tree (ties resolve by triangle index, any-hit is a boolean), only on the triangle records, and a
// node's boxes only filter.  So a refit rewrites exactly the fields that depend on positions and keeps everything else:
//   1. k_rf_tris, one thread per DevTri record: v0, e1 = v1 - v0, e2 = v2 - v0 from the new positions, gathered through a per-record
//      vertex-index triple (the same f32 subtractions as db_put_tri / put_tri; the library is built with -ffp-contract=off, so the
//      record is bit-identical to a fresh upload's);
//   2. k_rf_nodes, one launch per tree level, deepest first, one thread per node: the exact box of every child (leaves: from the new
//      positions of their finite triangles; inner children: the scratch box the previous launch wrote), the node's box as their
//      union, and the node re-quantised on that box with k_db_emit's rule.  Levels are ordered by the stream: no synchronisation
//      between workgroups, and the result does not depend on scheduling.
// The quantisation below is a restatement of k_db_emit's (device_build.hip), kept apart so that k_db_emit's code stays as it was;
// tests/test_gpu_geometry_update.py pins the two to each other (a refit with unchanged positions reproduces the device-built nodes
// byte for byte).
#include "refit.h"

#include <hip/hip_runtime.h>

#include <cmath>

namespace rt {
namespace {

__device__ __forceinline__ bool rf_gather(const uint32_t* __restrict__ vidx, const float* __restrict__ verts, uint32_t rec, float p[3][3]) {
    bool finite = true;
    for (int k = 0; k < 3; k++) {
        const uint32_t v = vidx[3 * (size_t)rec + k];
        for (int a = 0; a < 3; a++) {
            p[k][a] = verts[3 * (size_t)v + a];
            finite = finite && isfinite(p[k][a]);
        }
    }
    return finite;
}

__global__ __launch_bounds__(256) void k_rf_tris(DevTri* __restrict__ tris, const uint32_t* __restrict__ vidx, const float* __restrict__ verts, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || vidx[3 * (size_t)i] == RT_REFIT_NO_RECORD) return;
    float p[3][3];
    if (!rf_gather(vidx, verts, i, p)) return; // k_rf_nodes writes it, once the leaf's box is known
    DevTri& t = tris[i];
    for (int a = 0; a < 3; a++) {
        t.v0[a] = p[0][a];
        t.e1[a] = p[1][a] - p[0][a];
        t.e2[a] = p[2][a] - p[0][a];
    }
}

__global__ __launch_bounds__(64) void k_rf_nodes(DevNode8* __restrict__ nodes, float4* __restrict__ boxes, DevTri* __restrict__ tris, const uint32_t* __restrict__ vidx,
                                                  const float* __restrict__ verts, const uint32_t* __restrict__ order, uint32_t n) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t node = order[i];
    DevNode8 d = nodes[node];
    const uint32_t imask = d.ex_imask >> 24, lmask = d.lmask & 0xFFu;
    float cmn[8][3], cmx[8][3];
    float pmn[3] = {INFINITY, INFINITY, INFINITY}, pmx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int sl = 0; sl < 8; sl++) {
        const uint32_t bit = 1u << sl, below = bit - 1u;
        if (lmask & bit) {
            const uint32_t first = d.tri_base + RT_DEV_LEAF_STRIDE * (uint32_t)__popc(lmask & below);
            const uint32_t count = min(tris[first].leaf_count, RT_DEV_LEAF_STRIDE);
            float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            bool any = false, dropped = false;
            for (uint32_t r = 0; r < count; r++) {
                float p[3][3];
                if (!rf_gather(vidx, verts, first + r, p)) {
                    dropped = true;
                    continue;
                }
                any = true;
                for (int a = 0; a < 3; a++) { // the triangle's box as k_db_bounds takes it, then the union
                    mn[a] = fminf(mn[a], fminf(fminf(p[0][a], p[1][a]), p[2][a]));
                    mx[a] = fmaxf(mx[a], fmaxf(fmaxf(p[0][a], p[1][a]), p[2][a]));
                }
            }
            if (!any)
                for (int a = 0; a < 3; a++) mn[a] = mx[a] = 0.0f;
            if (dropped)
                for (uint32_t r = 0; r < count; r++) {
                    float p[3][3];
                    if (rf_gather(vidx, verts, first + r, p)) continue;
                    DevTri& t = tris[first + r];
                    for (int a = 0; a < 3; a++) t.v0[a] = mn[a], t.e1[a] = 0.0f, t.e2[a] = 0.0f;
                }
            for (int a = 0; a < 3; a++) cmn[sl][a] = mn[a], cmx[sl][a] = mx[a];
        } else if (imask & bit) {
            const uint32_t c = d.child_base + (uint32_t)__popc(imask & below);
            const float4 mn = boxes[2 * (size_t)c], mx = boxes[2 * (size_t)c + 1];
            cmn[sl][0] = mn.x, cmn[sl][1] = mn.y, cmn[sl][2] = mn.z;
            cmx[sl][0] = mx.x, cmx[sl][1] = mx.y, cmx[sl][2] = mx.z;
        } else {
            continue;
        }
        for (int a = 0; a < 3; a++) pmn[a] = fminf(pmn[a], cmn[sl][a]), pmx[a] = fmaxf(pmx[a], cmx[sl][a]);
    }
    if (!(pmn[0] <= pmx[0])) // a node without children (cannot happen in a tree the builders made): a point, like an empty leaf
        for (int a = 0; a < 3; a++) pmn[a] = pmx[a] = 0.0f;
    boxes[2 * (size_t)node] = make_float4(pmn[0], pmn[1], pmn[2], 0.0f);
    boxes[2 * (size_t)node + 1] = make_float4(pmx[0], pmx[1], pmx[2], 0.0f);
    // k_db_emit's rule: per-axis power-of-two grid on the node's box, planes rounded outward, exponent clamped to [-126, 127]
    uint32_t ex[3];
    for (int a = 0; a < 3; a++) {
        d.org[a] = pmn[a];
        const double extent = (double)pmx[a] - (double)pmn[a];
        int e = 1;
        if (extent > 0.0) {
            int fe;
            (void)frexp(extent / 255.0, &fe);
            e = fe + 127;
            if (e < 1) e = 1;
            if (e > 254) e = 254;
        }
        ex[a] = (uint32_t)(e - 127) & 0xFFu;
        const double scale = ldexp(1.0, e - 127);
        for (int h = 0; h < 2; h++) {
            uint32_t lo_word = 0, hi_word = 0;
            for (int k = 0; k < 4; k++) {
                const int sl = 4 * h + k;
                uint32_t qlo = 255, qhi = 0; // empty slots stay inverted
                if ((imask | lmask) & (1u << sl)) {
                    double lo = floor(((double)cmn[sl][a] - (double)d.org[a]) / scale);
                    double hi = ceil(((double)cmx[sl][a] - (double)d.org[a]) / scale);
                    lo = fmin(fmax(lo, 0.0), 255.0);
                    hi = fmin(fmax(hi, 0.0), 255.0);
                    while (lo > 0.0 && (double)d.org[a] + lo * scale > (double)cmn[sl][a]) lo -= 1.0;
                    while (hi < 255.0 && (double)d.org[a] + hi * scale < (double)cmx[sl][a]) hi += 1.0;
                    qlo = (uint32_t)lo;
                    qhi = (uint32_t)hi;
                }
                lo_word |= qlo << (8 * k);
                hi_word |= qhi << (8 * k);
            }
            d.qlo[a][h] = lo_word;
            d.qhi[a][h] = hi_word;
        }
    }
    d.ex_imask = ex[0] | (ex[1] << 8) | (ex[2] << 16) | (imask << 24);
    nodes[node] = d;
}

__global__ __launch_bounds__(256) void k_rf_any_finite(const uint32_t* __restrict__ vidx, uint32_t n, const float* __restrict__ verts, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float p[3][3];
    if (rf_gather(vidx, verts, i, p)) atomicOr(flag, 1u);
}

} // namespace

hipError_t launch_refit_tris(DevTri* tris, const uint32_t* vidx, const float* verts, uint32_t n_records, hipStream_t stream) {
    if (n_records == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rf_tris, dim3((n_records + 255u) / 256u), dim3(256), 0, stream, tris, vidx, verts, n_records);
    return hipGetLastError();
}

hipError_t launch_refit_nodes(DevNode8* nodes, float4* boxes, DevTri* tris, const uint32_t* vidx, const float* verts, const uint32_t* order,
                              uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rf_nodes, dim3((n + 63u) / 64u), dim3(64), 0, stream, nodes, boxes, tris, vidx, verts, order, n);
    return hipGetLastError();
}

hipError_t launch_refit_any_finite(const uint32_t* vidx, uint32_t n, const float* verts, uint32_t* flag, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rf_any_finite, dim3((n + 255u) / 256u), dim3(256), 0, stream, vidx, n, verts, flag);
    return hipGetLastError();
}

} // namespace rt
