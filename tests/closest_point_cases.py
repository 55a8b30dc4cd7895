"""The closest-point query's statement (include/rt_hip.h "Closest-point queries", csrc/closest_point_rules.h) in numpy, and the
points the tests ask about.

brute_force() evaluates the statement for every point against every triangle and sphere of a scene, in float32 - every numpy
operation is one f32 rounding, in the header's order, so its records are the bytes rt_closest_point must return - or in float64
(the same statement on the exact edges), which gives the distances the float32 statement is held to.  Helpers, no tests."""
import numpy as np

from gpu_raytracer_amd import types as T

F32 = np.float32
PRIM_MISS = 0xFFFFFFFF
SPHERE_FLAG = 0x80000000
PAIRS_PER_CHUNK = 1 << 20  # point x triangle pairs evaluated at a time


def records(scene, dtype=F32):
    """The scene's triangles as the device's records: v0, e1 = v1 - v0, e2 = v2 - v0 (differences in `dtype`), material ids."""
    pos = np.ascontiguousarray(scene.vertices["position"], F32).astype(dtype)
    t = scene.triangles
    v0 = pos[t["v0_index"]]
    return v0, pos[t["v1_index"]] - v0, pos[t["v2_index"]] - v0, t["material_id"].astype(np.uint32)


def diagonal(scene):
    pos = scene.vertices["position"].astype(np.float64)
    return float(np.linalg.norm(pos.max(0) - pos.min(0)))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def triangle_candidates(v0, e1, e2, p):
    """p (m, 3) against n records -> dist2, v, w, each (m, n), in the arrays' dtype: the header's statement, all quantities up front
    and the first rule that holds applied last."""
    one = p.dtype.type(1)
    with np.errstate(all="ignore"):
        ap = p[:, None, :] - v0[None]
        d1, d2 = _dot(e1, ap), _dot(e2, ap)
        bp = ap - e1
        d3, d4 = _dot(e1, bp), _dot(e2, bp)
        cp = ap - e2
        d5, d6 = _dot(e1, cp), _dot(e2, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den = one / ((va + vb) + vc)
        v, w = vb * den, vc * den
        d43, d56 = d4 - d3, d5 - d6
        w6 = d43 / (d43 + d56)
        c = (va <= 0) & (d43 >= 0) & (d56 >= 0)
        v, w = np.where(c, one - w6, v), np.where(c, w6, w)
        c = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = np.where(c, 0, v), np.where(c, d2 / (d2 - d6), w)
        c = (d6 >= 0) & (d5 <= d6)
        v, w = np.where(c, 0, v), np.where(c, one, w)
        c = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = np.where(c, d1 / (d1 - d3), v), np.where(c, 0, w)
        c = (d3 >= 0) & (d4 <= d3)
        v, w = np.where(c, one, v), np.where(c, 0, w)
        c = (d1 <= 0) & (d2 <= 0)
        v, w = np.where(c, 0, v).astype(p.dtype), np.where(c, 0, w).astype(p.dtype)
        r = (e1 * v[..., None] + e2 * w[..., None]) - ap
        return _dot(r, r), v, w


def sphere_candidates(centre, radius, p):
    """p (m, 3) against s spheres -> dist2 (m, s), position (m, s, 3)."""
    with np.errstate(all="ignore"):
        oc = p[:, None, :] - centre[None]
        length = np.sqrt(_dot(oc, oc))
        d = np.abs(length - radius)
        at_centre = np.zeros_like(oc)
        at_centre[..., 0] = radius
        pos = np.where((length > 0)[..., None], centre + oc * (radius / length)[..., None], centre + at_centre)
        return d * d, pos


def _order(dist2, key):
    return (np.ascontiguousarray(dist2, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | key.astype(np.uint64)


def brute_force(scene, points, prefilter=False, return_dist2=False):
    """(N, 4) float32 points (position, radius) -> (N, 8) float32 rt_nearest records: the bytes rt_closest_point returns.
    prefilter (for scenes of 10^5 triangles, where the statement on every pair takes tens of seconds): a triangle's distance from p lies
    in [dc - R, dc], dc the distance of its centroid and R the centroid's distance to its farthest vertex, so U = the smallest dc bounds
    the answer from above and a triangle with dc - R > U + 1e-3 x the scene's diagonal (ten thousand times the f32 statement's error)
    can neither win nor tie; the statement is then evaluated on the others only.  test_closest_point_abi.py holds the filtered result to
    the unfiltered one.  return_dist2: also the winners' dist2 (N,), whose root the records carry; inf for a miss."""
    points = np.ascontiguousarray(points, F32)
    n = len(points)
    dist2 = np.full(n, np.inf, F32)
    out = np.zeros(n, T.NEAREST)
    out["distance"] = points[:, 3]
    out["prim_id"] = PRIM_MISS
    p, radius = points[:, 0:3], points[:, 3]
    with np.errstate(all="ignore"):
        start = _order(radius * radius, np.zeros(n, np.uint32))
    valid = np.isfinite(p).all(1) & (radius > 0)
    v0, e1, e2, mat = records(scene)
    all_v0, all_e1, all_e2, all_mat = v0, e1, e2, mat
    all_prim = np.arange(len(v0), dtype=np.uint32)
    prim = all_prim
    if prefilter and len(v0):
        centroid = v0 + (e1 + e2) / F32(3)
        reach = np.sqrt(np.maximum(np.maximum(_dot(v0 - centroid, v0 - centroid), _dot(v0 + e1 - centroid, v0 + e1 - centroid)),
                                   _dot(v0 + e2 - centroid, v0 + e2 - centroid)))
        margin = F32(1e-3 * diagonal(scene))
    sph = scene.spheres
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        q = p[lo:hi]
        rows = np.arange(hi - lo)
        best = start[lo:hi].copy()
        rec = out[lo:hi]
        found = np.zeros(hi - lo, bool)
        if len(sph):
            d2, pos = sphere_candidates(np.ascontiguousarray(sph["center"], F32), sph["radius"].astype(F32), q)
            order = _order(d2, np.broadcast_to(np.arange(len(sph), dtype=np.uint32), d2.shape))
            k = order.argmin(1)
            win = order[rows, k] < best
            best = np.where(win, order[rows, k], best)
            found |= win
            rec["position"][win] = pos[rows, k][win]
            rec["distance"][win] = np.sqrt(d2[rows, k][win])
            dist2[lo:hi][win] = d2[rows, k][win]
            rec["prim_id"][win] = (k[win] | SPHERE_FLAG).astype(np.uint32)
            rec["material_id"][win] = sph["material_id"][k][win]
        if prefilter and len(all_v0):
            with np.errstate(all="ignore"):
                dc = np.sqrt(_dot(q[:, None, :] - centroid[None], q[:, None, :] - centroid[None]))
                upper = np.where(np.isfinite(dc), dc, np.inf).min(1)
                prim = np.flatnonzero((dc - reach[None] <= (upper + margin)[:, None]).any(0)).astype(np.uint32)
            v0, e1, e2, mat = all_v0[prim], all_e1[prim], all_e2[prim], all_mat[prim]
        if len(v0):
            d2, v, w = triangle_candidates(v0, e1, e2, q)
            order = _order(d2, np.broadcast_to(prim.astype(np.uint64) | np.uint64(SPHERE_FLAG), d2.shape))
            k = order.argmin(1)  # the lowest (dist2 bits, key): at equal dist2 the lower index
            win = order[rows, k] < best
            found |= win
            vk, wk = v[rows, k], w[rows, k]
            pos = v0[k] + (e1[k] * vk[:, None] + e2[k] * wk[:, None])
            rec["position"][win] = pos[win]
            rec["distance"][win] = np.sqrt(d2[rows, k][win])
            dist2[lo:hi][win] = d2[rows, k][win]
            rec["u"][win], rec["v"][win] = vk[win], wk[win]
            rec["prim_id"][win] = prim[k][win]
            rec["material_id"][win] = mat[k][win]
        miss = ~(found & valid[lo:hi])
        blank = np.zeros(int(miss.sum()), T.NEAREST)
        blank["distance"] = radius[lo:hi][miss]
        blank["prim_id"] = PRIM_MISS
        rec[miss] = blank
        dist2[lo:hi][miss] = np.inf
    return (out.view(F32).reshape(n, 8), dist2) if return_dist2 else out.view(F32).reshape(n, 8)


def distances(scene, positions, dtype):
    """The distance of the statement in `dtype` (float32: on the stored f32 edges; float64: on the exact ones) from each of the (N, 3)
    positions to the scene's triangles and spheres, radius = inf."""
    v0, e1, e2, _ = records(scene, dtype)
    p = np.ascontiguousarray(positions, F32).astype(dtype)
    out = np.full(len(p), np.inf, dtype)
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    for lo in range(0, len(p), step):
        q = p[lo:lo + step]
        d2 = triangle_candidates(v0, e1, e2, q)[0]
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        if len(scene.spheres):
            s2 = sphere_candidates(scene.spheres["center"].astype(dtype), scene.spheres["radius"].astype(dtype), q)[0]
            d2 = np.concatenate([d2, np.where(np.isfinite(s2), s2, np.inf)], 1)
        out[lo:lo + step] = np.sqrt(d2.min(1))
    return out


def _on_surface(scene, rng, n):
    v0, e1, e2, _ = records(scene, np.float64)
    k = rng.integers(0, len(v0), n)
    a, b = rng.random(n), rng.random(n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    return v0[k] + e1[k] * a[:, None] + e2[k] * b[:, None]


def near_surface(scene, n, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    return (_on_surface(scene, rng, n) + rng.normal(0.0, sigma, (n, 3))).astype(F32)


def scattered(scene, n, seed):
    """Uniform over three times the scene's bounding box, about its centre."""
    rng = np.random.default_rng(seed)
    pos = scene.vertices["position"].astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    return ((lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * 3 * (hi - lo)).astype(F32)


def on_vertices(scene, n, seed):
    rng = np.random.default_rng(seed)
    pos = np.ascontiguousarray(scene.vertices["position"], F32)
    return pos[rng.integers(0, len(pos), n)].copy()


def on_surface(scene, n, seed):
    return _on_surface(scene, np.random.default_rng(seed), n).astype(F32)


def four_kinds(scene, n, seed):
    """n positions, a quarter each: near surfaces (sigma 0.05), scattered over three times the box, on vertices, on surfaces."""
    q = n // 4
    return np.concatenate([near_surface(scene, q, seed), scattered(scene, q, seed + 1), on_vertices(scene, q, seed + 2),
                           on_surface(scene, n - 3 * q, seed + 3)])
