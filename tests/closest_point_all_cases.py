"""The nearest-K query's statement (include/rt_hip.h "Closest-point queries", rt_closest_point_all) in numpy.

nearest_all() evaluates closest_point_cases.py's float32 candidates of every point against every triangle and sphere of a scene,
keeps those below cp_start(radius), sorts them by (dist2 bits, key) and writes the first K as rt_nearest records with miss padding:
the bytes rt_closest_point_all must return.  The first k < K records of a point are the statement's at max_nearest = k (first_k).
Helpers, no tests."""
import dataclasses

import numpy as np

import closest_point_cases as cc
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

F32 = np.float32
NEAREST_MAX = 16
OUT_OF_RANGE = np.uint64(0xFFFFFFFFFFFFFFFF)


def nearest_all(scene, points, k=NEAREST_MAX):
    """(N, 4) float32 points (position, radius) -> records (N, k, 8) float32, listed counts (N,) uint32 = min(total, k), total counts
    (N,) uint32 = the candidates in range (what RT_QUERY_COUNT_ALL reports)."""
    points = np.ascontiguousarray(points, F32)
    n = len(points)
    out = np.zeros((n, k), T.NEAREST)
    out["distance"] = points[:, 3, None]
    out["prim_id"] = cc.PRIM_MISS
    total = np.zeros(n, np.uint32)
    p, radius = points[:, 0:3], points[:, 3]
    with np.errstate(all="ignore"):
        start = cc._order(radius * radius, np.zeros(n, np.uint32))
    valid = np.isfinite(p).all(1) & (radius > 0)
    v0, e1, e2, mat = cc.records(scene)
    n_tri = len(v0)
    sph = scene.spheres
    n_sph = len(sph)
    centre, sph_radius = np.ascontiguousarray(sph["center"], F32).reshape(-1, 3), sph["radius"].astype(F32)
    # the candidates' columns: spheres first, then triangles; the order decides, not the column
    key = np.concatenate([np.arange(n_sph, dtype=np.uint64), np.arange(n_tri, dtype=np.uint64) | np.uint64(cc.SPHERE_FLAG)])
    material = np.concatenate([sph["material_id"].astype(np.uint32), mat])
    step = max(1, cc.PAIRS_PER_CHUNK // max(n_tri + n_sph, 1))
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        q, m = p[lo:hi], hi - lo
        sd2, spos = cc.sphere_candidates(centre, sph_radius, q) if n_sph else (np.zeros((m, 0), F32), np.zeros((m, 0, 3), F32))
        td2, tv, tw = cc.triangle_candidates(v0, e1, e2, q) if n_tri else (np.zeros((m, 0), F32),) * 3
        d2 = np.concatenate([sd2, td2], 1)
        order = cc._order(d2, np.broadcast_to(key, d2.shape))
        in_range = (order < start[lo:hi, None]) & valid[lo:hi, None]
        total[lo:hi] = in_range.sum(1)
        order = np.where(in_range, order, OUT_OF_RANGE)
        first = np.argsort(order, 1, kind="stable")[:, :k]  # (m, <= k) columns, ascending order
        rows = np.arange(m)[:, None]
        listed = np.take_along_axis(in_range, first, 1)
        rec = np.zeros(first.shape, T.NEAREST)
        is_tri = first >= n_sph
        t = np.where(is_tri, first - n_sph, 0)
        s = np.where(is_tri, 0, first)
        if n_tri:
            vk, wk = tv[rows, t], tw[rows, t]
            tpos = v0[t] + (e1[t] * vk[..., None] + e2[t] * wk[..., None])
            rec["u"], rec["v"] = np.where(is_tri, vk, 0), np.where(is_tri, wk, 0)
        else:
            tpos = np.zeros(first.shape + (3,), F32)
        pos = np.where(is_tri[..., None], tpos, spos[rows, s]) if n_sph else tpos
        rec["position"] = pos
        with np.errstate(all="ignore"):
            rec["distance"] = np.sqrt(d2[rows, first])
        rec["prim_id"] = (key[first] ^ np.uint64(cc.SPHERE_FLAG)).astype(np.uint32)
        rec["material_id"] = material[first]
        blank = out[lo:hi, :first.shape[1]]
        out[lo:hi, :first.shape[1]] = np.where(listed, rec, blank)
    listed_counts = np.minimum(total, k).astype(np.uint32)
    return out.view(F32).reshape(n, k, 8), listed_counts, total


def first_k(records, total, k):
    """The statement at max_nearest = k from nearest_all's at a larger one: (records (N, k, 8), listed counts)."""
    return np.ascontiguousarray(records[:, :k]), np.minimum(total, k).astype(np.uint32)


# -- scenes with exact ties ----------------------------------------------------------------------------------------------------
def triangles_scene(corners, spheres=()):
    """A scene of the triangles given by their three corners each, and spheres (centre, radius, material)."""
    base = scenes.single_triangle()
    corners = np.asarray(corners, F32).reshape(-1, 3, 3)
    v = np.zeros(3 * len(corners), base.vertices.dtype)
    v["position"] = corners.reshape(-1, 3)
    t = np.zeros(len(corners), base.triangles.dtype)
    idx = np.arange(3 * len(corners)).reshape(-1, 3)
    t["v0_index"], t["v1_index"], t["v2_index"] = idx[:, 0], idx[:, 1], idx[:, 2]
    t["material_id"] = np.arange(len(corners)) % max(1, len(base.materials))
    return dataclasses.replace(base, vertices=v, triangles=t, spheres=np.array(list(spheres), T.SPHERE))


UNIT = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]


def tripled_triangle():
    return triangles_scene([UNIT, UNIT, UNIT])


def sphere_and_triangle_tie():
    """From the origin the sphere (centre (0, 0, 2), radius 1) and the triangle in z = -1 under it are both at dist2 = 1."""
    return triangles_scene([[[-1, -1, -1], [3, -1, -1], [-1, 3, -1]]], spheres=[((0, 0, 2), 1.0, 0)])


def coplanar_walls():
    """Two unit squares in z = 0 sharing the edge x = 1 (triangles 0, 1 | 2, 3), a third in x = 2 standing on the second's far edge
    (4, 5) and the first square once more (6, 7): a point above a shared edge, corner or diagonal is equally far, bit for bit, from
    every triangle that holds it - up to five above the corner (1, 1, 0)."""
    def quad(a, b, c, d):
        return [[a, b, c], [a, c, d]]
    return triangles_scene(quad([0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]) + quad([1, 0, 0], [2, 0, 0], [2, 1, 0], [1, 1, 0]) +
                           quad([2, 0, 0], [2, 0, 1], [2, 1, 1], [2, 1, 0]) + quad([0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]))
