// refit.hip — rt_update_geometry's refit: the tree a context holds follows new vertex positions with its topology unchanged.
//
// Closest hits do not depend on the tree (ties resolve by triangle index, any-hit is a boolean), only on the triangle records, and a
// node's boxes only filter.  So a refit rewrites exactly the fields that depend on positions and keeps everything else:
//   1. k_rf_tris, one thread per DevTri record: the position part of the record (put_positions) from the new positions, gathered
//      through a per-record vertex-index triple (the library is built with -ffp-contract=off, so the record is bit-identical to a
//      fresh upload's);
//   2. k_rf_nodes, one launch per tree level, deepest first, one thread per node: the exact box of every child (leaves: from the new
//      positions of their finite triangles; inner children: the scratch box the previous launch wrote), the node's box as their
//      union, and the node re-quantised on that box (quantise_node).  Levels are ordered by the stream: no synchronisation
//      between workgroups, and the result does not depend on scheduling.
// The triangle's box, the record and the quantisation are the builders' own functions (bvh_rules.h): a refit with unchanged positions
// reproduces the built nodes byte for byte (tests/test_gpu_geometry_update.py).
#include "refit.h"

#include <hip/hip_runtime.h>

#include <cmath>

#include "bvh_rules.h"

namespace rt {
namespace {

__device__ __forceinline__ bool rf_gather(const uint32_t* __restrict__ vidx, const float* __restrict__ verts, uint32_t rec, float p[3][3]) {
    for (int k = 0; k < 3; k++) {
        const uint32_t v = vidx[3 * (size_t)rec + k];
        for (int a = 0; a < 3; a++) p[k][a] = verts[3 * (size_t)v + a];
    }
    return tri_finite(p[0], p[1], p[2]);
}

__global__ __launch_bounds__(256) void k_rf_tris(DevTri* __restrict__ tris, const uint32_t* __restrict__ vidx, const float* __restrict__ verts, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || vidx[3 * (size_t)i] == RT_REFIT_NO_RECORD) return;
    float p[3][3];
    if (!rf_gather(vidx, verts, i, p)) return; // k_rf_nodes writes it, once the leaf's box is known
    put_positions(p[0], p[1], p[2], &tris[i]);
}

__global__ __launch_bounds__(64) void k_rf_nodes(DevNode8* __restrict__ nodes, float4* __restrict__ boxes, DevTri* __restrict__ tris, const uint32_t* __restrict__ vidx,
                                                  const float* __restrict__ verts, const uint32_t* __restrict__ order, uint32_t n) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t node = order[i];
    DevNode8 d = nodes[node];
    const uint32_t imask = d.ex_imask >> 24, lmask = d.lmask & 0xFFu;
    Box cb[W8], pb;
    pb.reset();
    for (int sl = 0; sl < W8; sl++) {
        const uint32_t bit = 1u << sl, below = bit - 1u;
        if (lmask & bit) {
            const uint32_t first = d.tri_base + RT_DEV_LEAF_STRIDE * (uint32_t)__popc(lmask & below);
            const uint32_t count = min(tris[first].leaf_count, RT_DEV_LEAF_STRIDE);
            Box lb;
            lb.reset();
            bool any = false, dropped = false;
            for (uint32_t r = 0; r < count; r++) {
                float p[3][3];
                if (!rf_gather(vidx, verts, first + r, p)) {
                    dropped = true;
                    continue;
                }
                any = true;
                lb.grow(tri_box(p[0], p[1], p[2]));
            }
            if (!any)
                for (int a = 0; a < 3; a++) lb.mn[a] = lb.mx[a] = 0.0f;
            if (dropped)
                for (uint32_t r = 0; r < count; r++) {
                    float p[3][3];
                    if (rf_gather(vidx, verts, first + r, p)) continue;
                    DevTri& t = tris[first + r];
                    for (int a = 0; a < 3; a++) t.v0[a] = lb.mn[a], t.e1[a] = 0.0f, t.e2[a] = 0.0f;
                }
            cb[sl] = lb;
        } else if (imask & bit) {
            const uint32_t c = d.child_base + (uint32_t)__popc(imask & below);
            const float4 mn = boxes[2 * (size_t)c], mx = boxes[2 * (size_t)c + 1];
            cb[sl] = Box{{mn.x, mn.y, mn.z}, {mx.x, mx.y, mx.z}};
        } else {
            continue;
        }
        pb.grow(cb[sl]);
    }
    if (!(pb.mn[0] <= pb.mx[0])) // a node without children (cannot happen in a tree the builders made): a point, like an empty leaf
        for (int a = 0; a < 3; a++) pb.mn[a] = pb.mx[a] = 0.0f;
    boxes[2 * (size_t)node] = make_float4(pb.mn[0], pb.mn[1], pb.mn[2], 0.0f);
    boxes[2 * (size_t)node + 1] = make_float4(pb.mx[0], pb.mx[1], pb.mx[2], 0.0f);
    quantise_node(d, imask, pb, [&](int sl) { return (imask | lmask) & (1u << sl) ? &cb[sl] : (const Box*)nullptr; }); // the children keep their slots
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
