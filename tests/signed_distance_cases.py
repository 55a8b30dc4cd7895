"""The inside test's and the signed distance's statement (include/rt_hip.h "Inside tests and signed distance", csrc/inside_rules.h)
in numpy, closed shapes with an analytic truth, and the points the tests ask about.

Every numpy operation below is one f32 rounding in the header's order, so crossings() gives the counts the kernel's parity rays give,
and statement() / signed_records() the bytes rt_inside and rt_signed_distance return.  Helpers, no tests."""
import dataclasses

import numpy as np

import closest_point_cases as cc
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

F32 = np.float32
MIN_T = F32(1e-5)  # RT_MIN_RAY_DISTANCE
MAX_RAYS = 7
RAYS = (1, 3, 5, 7)
DIRECTIONS = np.array([  # RT_INSIDE_DIRECTIONS, restated: test_signed_distance_abi.py holds it to the header and to api.INSIDE_DIRECTIONS
    [0.5377, 0.7431, 0.3982], [-0.6241, 0.3517, 0.6977], [0.2893, -0.4719, 0.8328],
    [-0.3361, -0.8154, -0.4703], [0.8467, -0.2249, -0.4821], [-0.1873, 0.5566, -0.8094],
    [0.4129, 0.1683, -0.8951]], F32)
PAIRS_PER_CHUNK = 1 << 19  # point x triangle pairs evaluated at a time


# ---- the statement ---------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2],
                     a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def moller_trumbore(v0, e1, e2, o, d):
    """device_common.h's moller_trumbore on broadcastable (..., 3) arrays -> (ok, t, u, v): test_gpu_ray_queries._moller_trumbore's
    operations in its order."""
    with np.errstate(all="ignore"):
        h = _cross(d, e2)
        a = _dot(e1, h)
        ok = ~(np.abs(a) < MIN_T)
        f = F32(1.0) / a
        s = o - v0
        u = f * _dot(s, h)
        ok = ok & ~((u < 0) | (u > 1))
        q = _cross(s, e1)
        v = f * _dot(d, q)
        ok = ok & ~((v < 0) | (u + v > 1))
        t = f * _dot(e2, q)
    return ok, t, u, v


def crossings(scene, positions):
    """(N, 3) float32 positions -> (N, 7) counts c_k: the triangles of the scene whose test accepts the ray (P, D_k) with
    RT_MIN_RAY_DISTANCE < t < inf.  A row with a non-finite component is 0: nothing is traced for it."""
    p = np.ascontiguousarray(positions, F32)
    v0, e1, e2, _ = cc.records(scene)
    out = np.zeros((len(p), MAX_RAYS), np.uint32)
    if not len(v0):
        return out
    finite = np.isfinite(p).all(1)
    step = max(1, PAIRS_PER_CHUNK // len(v0))
    for lo in range(0, len(p), step):
        o = p[lo:lo + step, None, :]
        for k in range(MAX_RAYS):
            ok, t, _, _ = moller_trumbore(v0[None], e1[None], e2[None], o, DIRECTIONS[k][None, None, :])
            with np.errstate(all="ignore"):
                out[lo:lo + step, k] = (ok & (t > MIN_T) & (t < F32(np.inf))).sum(1)
    out[~finite] = 0
    return out


def sphere_inside(scene, positions):
    """(N,) bool: some sphere has dot(oc, oc) < radius * radius, oc = P - centre."""
    p = np.ascontiguousarray(positions, F32)
    sph = scene.spheres
    if not len(sph):
        return np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        oc = p[:, None, :] - np.ascontiguousarray(sph["center"], F32)[None]
        r = sph["radius"].astype(F32)
        return (_dot(oc, oc) < (r * r)[None]).any(1)


def vote(parity, rays, valid, in_sphere, with_votes):
    """parity (N, 7) of 0 / 1, valid and in_sphere (N,) bool -> (inside (N,) bool, votes (N,) uint8 - the odd votes of all `rays`
    rays, as the call reports them when asked - and traced (N,), the rays the call traces for each point: all of them for a valid
    point with a votes array; without one, none inside a sphere, and otherwise up to the first k at which odd * 2 > rays or
    even * 2 > rays)."""
    assert rays in RAYS
    n = len(parity)
    odd, traced = np.zeros(n, np.int64), np.zeros(n, np.int64)
    go = valid & (with_votes | ~in_sphere)
    for k in range(rays):
        traced += go
        odd += go & (parity[:, k] != 0)
        if not with_votes:
            go = go & ~((odd * 2 > rays) | ((traced - odd) * 2 > rays))
    inside = valid & (in_sphere | (odd * 2 > rays))
    votes = np.where(valid, (parity[:, :rays] != 0).sum(1), 0).astype(np.uint8)
    return inside, votes, traced


def statement(scene, points, rays, with_votes, distance=False, counts=None):
    """(N, 4) float32 points -> (inside, votes, traced) of rt_inside, or with `distance` of rt_signed_distance, whose degenerate
    queries are rt_closest_point's.  counts: crossings(scene, points[:, :3]) when the caller already has them."""
    points = np.ascontiguousarray(points, F32)
    pos = points[:, :3]
    valid = np.isfinite(pos).all(1)
    if distance:
        with np.errstate(all="ignore"):
            valid = valid & (points[:, 3] > 0)
    if counts is None:
        counts = crossings(scene, pos)
    return vote(counts & 1, rays, valid, sphere_inside(scene, pos), with_votes)


def sign(records, inside):
    """(N, 8) float32 rt_nearest records -> a copy, the sign bit of the distance set where `inside`."""
    out = np.array(records, F32).reshape(-1, 8)
    w = out.view(np.uint32)
    w[:, 3] |= np.where(inside, np.uint32(0x80000000), np.uint32(0))
    return out


def signed_records(scene, points, rays, with_votes, counts=None):
    """The bytes of rt_signed_distance: closest_point_cases.brute_force's records signed by the statement -> (records, votes, traced)."""
    inside, votes, traced = statement(scene, points, rays, with_votes, distance=True, counts=counts)
    return sign(cc.brute_force(scene, points), inside), votes, traced


def inside_rays(positions):
    """The 7 parity rays of each of the (N, 3) positions as rt_ray records, direction-major: ray k of point i at [k, i] of (7, N, 8)."""
    p = np.ascontiguousarray(positions, F32)
    out = np.empty((MAX_RAYS, len(p), 8), F32)
    out[:, :, 0:3] = p[None]
    out[:, :, 3] = MIN_T
    out[:, :, 4:7] = DIRECTIONS[:, None, :]
    out[:, :, 7] = np.inf
    return out


# ---- closed shapes and their analytic truth --------------------------------------------------------------------------------
BOX_LO, BOX_HI, BOX_N = np.array([-1.0, -0.5, -0.75]), np.array([1.25, 0.5, 0.5]), (4, 3, 5)
TORUS_R, TORUS_r, TORUS_SEGMENTS = 1.0, 0.4, (48, 24)


def box_mesh(open_top=False):
    """scenes._box on BOX_LO, BOX_HI, tessellated BOX_N with per-face vertices: 188 triangles; open_top: without the face y = hi."""
    v, t = scenes._box(BOX_LO, BOX_HI, BOX_N)
    if open_top:
        n_face = 2 * BOX_N[0] * BOX_N[2]
        t = np.concatenate([t[:n_face], t[2 * n_face:]])  # _box's second face is the top
    return v, t


def torus_mesh(centre=(0.0, 0.0, 0.0)):
    """An index-shared torus about the y axis through `centre`: 48 segments around, 24 around the tube, 2304 triangles."""
    nu, nv = TORUS_SEGMENTS
    u = np.arange(nu) * (2 * np.pi / nu)
    v = np.arange(nv) * (2 * np.pi / nv)
    U, V = np.meshgrid(u, v, indexing="ij")
    ring = TORUS_R + TORUS_r * np.cos(V)
    verts = np.stack([ring * np.cos(U), TORUS_r * np.sin(V), ring * np.sin(U)], -1).reshape(-1, 3) + np.asarray(centre, np.float64)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a = (i * nv + j).ravel()
    b = (((i + 1) % nu) * nv + j).ravel()
    c = (i * nv + (j + 1) % nv).ravel()
    d = (((i + 1) % nu) * nv + (j + 1) % nv).ravel()
    return verts, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])


def tetrahedron_mesh():
    """(0,0,0), (1,0,0), (0,1,0), (0,0,1): inside iff x, y, z > 0 and x + y + z < 1."""
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def make_scene(name, meshes, spheres=()):
    """A scene of the (verts, tris) meshes and (centre, radius) spheres, one material."""
    mesh = scenes._Mesh()
    for v, t in meshes:
        mesh.add(v, t, 0)
    vertices, triangles = mesh.finish()
    sph = np.zeros(len(spheres), T.SPHERE)
    for k, (c, r) in enumerate(spheres):
        sph[k] = (tuple(c), r, 0)
    return dataclasses.replace(scenes.empty_scene(), name=name, vertices=vertices, triangles=triangles, spheres=sph)


def box_inside(p):
    p = np.asarray(p, np.float64)
    return ((p > BOX_LO) & (p < BOX_HI)).all(1)


def box_distance(p):
    """float64 distance to the box's surface."""
    p = np.asarray(p, np.float64)
    q = np.maximum(BOX_LO - p, p - BOX_HI)  # per axis: > 0 outside the slab
    outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(1))
    return np.where((q < 0).all(1), -q.max(1), outside)


def torus_inside(p, centre=(0.0, 0.0, 0.0)):
    p = np.asarray(p, np.float64) - np.asarray(centre, np.float64)
    return (np.hypot(p[:, 0], p[:, 2]) - TORUS_R) ** 2 + p[:, 1] ** 2 < TORUS_r ** 2


def torus_distance(p, centre=(0.0, 0.0, 0.0)):
    """float64 distance to the smooth torus; the mesh is inscribed in it and departs from it by less than 0.007 (the two sagittas:
    1.4 (1 - cos(pi / 48)) + 0.4 (1 - cos(pi / 24)))."""
    p = np.asarray(p, np.float64) - np.asarray(centre, np.float64)
    return np.abs(np.hypot(np.hypot(p[:, 0], p[:, 2]) - TORUS_R, p[:, 1]) - TORUS_r)


def box_exit_face(p, d):
    """For positions strictly inside the box and one direction: the (axis, side) of the face the ray leaves through, float64."""
    p, d = np.asarray(p, np.float64), np.asarray(d, np.float64)
    t = np.where(d > 0, (BOX_HI - p) / d, (BOX_LO - p) / d)
    axis = t.argmin(1)
    return axis, (d[axis] > 0).astype(np.int64)


BOX_KEEP, TORUS_KEEP = 1e-3, 0.02  # conditions on the inputs: points nearer the surface than this are not asked about


def closed_shape_points(seed=5):
    """The two point sets of the tests, float32, generated in this order from one generator: 4096 uniform points in the box grown by
    0.5, the 13^3 lattice over the box grown by 0.25, 4096 uniform points in +-(1.6, 0.6, 1.6) about the torus; of each, the points
    farther than BOX_KEEP / TORUS_KEEP from the surface -> (box points, torus points)."""
    rng = np.random.default_rng(seed)
    uniform = (BOX_LO - 0.5) + rng.random((4096, 3)) * (BOX_HI - BOX_LO + 1.0)
    axes = [np.linspace(BOX_LO[a] - 0.25, BOX_HI[a] + 0.25, 13) for a in range(3)]
    lattice = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    box = np.concatenate([uniform, lattice]).astype(F32)
    torus = ((rng.random((4096, 3)) * 2.0 - 1.0) * np.array([1.6, 0.6, 1.6])).astype(F32)
    return box[box_distance(box) > BOX_KEEP], torus[torus_distance(torus) > TORUS_KEEP]


# ---- the scene of the GPU tests: the box, the torus beside it and two spheres, one of which overlaps the box ----------------------
UNION_TORUS_CENTRE = (0.0, 1.5, 0.0)
UNION_SPHERES = (((1.25, 0.0, 0.0), 0.4), ((-2.2, 0.0, 0.0), 0.5))
SPHERE_KEEP = 1e-3


def union_scene():
    return make_scene("box, torus and spheres", [box_mesh(), torus_mesh(UNION_TORUS_CENTRE)], UNION_SPHERES)


def union_points(n_each=768, seed=5):
    """Points of closed_shape_points (n_each of each set, the torus set moved with the torus) and 256 uniform points about the spheres,
    of which those stay that are farther than BOX_KEEP, TORUS_KEEP and SPHERE_KEEP from the three kinds of surface -> (positions (N, 3)
    float32, the analytic truth (N,) bool: inside the box, the torus or a sphere)."""
    box, torus = closed_shape_points(seed)
    rng = np.random.default_rng(seed + 1)
    box = box[rng.permutation(len(box))[:n_each]]
    torus = (torus[rng.permutation(len(torus))[:n_each]].astype(np.float64) + np.asarray(UNION_TORUS_CENTRE)).astype(F32)
    about = np.concatenate([np.asarray(c) + (rng.random((128, 3)) * 2.0 - 1.0) * 1.5 * r for c, r in UNION_SPHERES]).astype(F32)
    p = np.concatenate([box, torus, about])
    to_sphere = np.stack([np.linalg.norm(p.astype(np.float64) - np.asarray(c), axis=1) - r for c, r in UNION_SPHERES], 1)
    keep = (box_distance(p) > BOX_KEEP) & (torus_distance(p, UNION_TORUS_CENTRE) > TORUS_KEEP) & (np.abs(to_sphere) > SPHERE_KEEP).all(1)
    p, to_sphere = p[keep], to_sphere[keep]
    return p, box_inside(p) | torus_inside(p, UNION_TORUS_CENTRE) | (to_sphere < 0).any(1)
