"""Posed meshes (rt_overlap_mesh, rt_sweep_mesh) in numpy: the answers as the reduction, per pose, of the triangle statements over
api.pose_triangles(mesh, poses).  Nothing here is new geometry: overlap_want and sweep_want are built only from pose_triangles,
overlap_triangle_cases' brute force (touching) and sweep_triangle_cases.brute_force, and the two reducers also serve the GPU tests,
which hand them the records of the existing triangle calls.  Plus the meshes, poses and sweeps the tests use."""
import numpy as np

import overlap_triangle_cases as tc
import sweep_triangle_cases as st
from gpu_raytracer_amd import api

F32 = np.float32
PRIM_MISS = 0xFFFFFFFF
SPHERE_FLAG = 0x80000000
AXIS_NONE = 0xFFFFFFFF
INF = np.inf


# -- the reducers -----------------------------------------------------------------------------------------------------------------
def reduce_overlap(counts, valid):
    """counts (N, M): what overlap_triangle gives each posed triangle with count_all; valid (N,) -> pairs (N,) uint32, first (N,)
    uint32: the sum in 64 bits capped at 0xFFFFFFFF, the lowest j with a count, PRIM_MISS if none; an invalid pose gives 0 and
    PRIM_MISS."""
    c = np.where(np.asarray(valid, bool)[:, None], np.asarray(counts).astype(np.uint64), np.uint64(0))
    pairs = np.minimum(c.sum(axis=1, dtype=np.uint64), np.uint64(0xFFFFFFFF)).astype(np.uint32)
    first = np.where((c > 0).any(axis=1), (c > 0).argmax(axis=1), PRIM_MISS).astype(np.uint32)
    return pairs, first


def reduce_sweep(records, tmax, valid):
    """records (N, M, 8) float32: sweep_triangle's record of each posed triangle; tmax (N,) as given; valid (N,) -> (N, 8) float32
    rt_mesh_sweep_hit records: the hit with the least (bits of t, prim_id ^ 0x80000000, j), its word 5 replaced by j; no hit, or an
    invalid pose: normal 0, tmax as given, AXIS_NONE, triangle = prim_id = PRIM_MISS, material 0."""
    words = np.ascontiguousarray(records, F32).view(np.uint32)
    n, m = words.shape[:2]
    hit = (words[:, :, 6] != PRIM_MISS) & np.asarray(valid, bool)[:, None]
    key = (words[:, :, 3].astype(np.uint64) << np.uint64(32)) | (words[:, :, 6] ^ np.uint32(SPHERE_FLAG)).astype(np.uint64)
    key = np.where(hit, key, np.uint64(0xFFFFFFFFFFFFFFFF))
    j = key.argmin(axis=1)  # the first of equal keys: the lowest j
    out = np.zeros((n, 8), np.uint32)
    out[:, 3] = np.ascontiguousarray(tmax, F32).view(np.uint32)
    out[:, 4], out[:, 5], out[:, 6] = AXIS_NONE, PRIM_MISS, PRIM_MISS
    any_hit = hit.any(axis=1)
    out[any_hit] = words[any_hit, j[any_hit]]
    out[any_hit, 5] = j[any_hit].astype(np.uint32)
    return out.view(F32)


# -- the expectations by the numpy statements ---------------------------------------------------------------------------------------
def posed_sweeps(mesh, sweeps):
    """(M, 12) mesh and (N, 12) pose sweeps -> (N * M, 16) triangle sweeps, pose-major: the posed triangles with the pose's direction
    and tmax."""
    tris = api.pose_triangles(mesh, sweeps)
    n, m = tris.shape[:2]
    out = np.zeros((n, m, 16), F32)
    out[:, :, 0:12] = tris
    out[:, :, 12:16] = np.asarray(sweeps, F32)[:, None, 8:12]
    return out.reshape(n * m, 16)


def overlap_counts(scene, mesh, poses):
    """-> (N, M) counts of touching primitives per posed triangle, by overlap_triangle_cases' brute force."""
    tris = api.pose_triangles(mesh, poses)
    n, m = tris.shape[:2]
    return tc.touching(scene, tris.reshape(n * m, 12)).sum(axis=1).reshape(n, m)


def overlap_want(scene, mesh, poses):
    return reduce_overlap(overlap_counts(scene, mesh, poses), api.pose_frames(poses)[1])


def sweep_want(scene, mesh, sweeps):
    sweeps = np.asarray(sweeps, F32)
    rec = st.brute_force(scene, posed_sweeps(mesh, sweeps)).reshape(len(sweeps), len(mesh), 8)
    return reduce_sweep(rec, sweeps[:, 11], api.pose_frames(sweeps)[1])


# -- meshes -----------------------------------------------------------------------------------------------------------------------
def box_hull(half=0.05, centre=(0.0, 0.0, 0.0)):
    """The 12 triangles of an axis-aligned box around `centre` -> (12, 12) float32.  Triangles 0 and 1 are the bottom (y = -half),
    2 and 3 the top, then the z and the x faces."""
    h = np.broadcast_to(np.asarray(half, np.float64), (3,))
    c = np.asarray(centre, np.float64)
    corner = lambda sx, sy, sz: c + h * (sx, sy, sz)
    quads = [((-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1)), ((-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)),
             ((-1, -1, -1), (-1, 1, -1), (1, 1, -1), (1, -1, -1)), ((-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)),
             ((-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (-1, 1, -1)), ((1, -1, -1), (1, 1, -1), (1, 1, 1), (1, -1, 1))]
    v = []
    for a, b, cc, d in quads:
        v += [(corner(*a), corner(*b), corner(*cc)), (corner(*a), corner(*cc), corner(*d))]
    v = np.asarray(v, F32)
    return api.make_triangles(v[:, 0], v[:, 1], v[:, 2])


def random_mesh(m, seed, edge=0.1, spread=0.1):
    """m seeded triangles of mean edge about `edge` whose centres lie within `spread` of the origin -> (m, 12) float32."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (m, 1, 3))
    v = (c + rng.uniform(-0.6 * edge, 0.6 * edge, (m, 3, 3))).astype(F32)
    return api.make_triangles(v[:, 0], v[:, 1], v[:, 2])


# -- poses ------------------------------------------------------------------------------------------------------------------------
def surface_points(scene, n, rng):
    """n seeded points on the scene's triangles and their (unnormalised) face normals."""
    v = np.asarray(scene.vertices["position"], np.float64)
    t = scene.triangles
    k = rng.integers(0, len(t), n)
    a, b, c = v[t["v0_index"][k]], v[t["v1_index"][k]], v[t["v2_index"][k]]
    u = rng.uniform(0.05, 0.45, (n, 2))
    return a + (b - a) * u[:, :1] + (c - a) * u[:, 1:], np.cross(b - a, c - a)


def soup_pose_sweeps(scene, n, seed):
    """n seeded pose sweeps for the soup, random unnormalised quaternions, tmax = inf, in a cycle of eight kinds: four stand off
    the soup's surfaces by 0 (in contact at the start), 0.02, 0.05 and 0.6 and move back toward their surface point; three stand
    outside the soup's cube and move toward its middle (a first contact at t > 0); one stands outside and moves away (a miss that
    touches nothing)."""
    rng = np.random.default_rng(seed)
    p, normal = surface_points(scene, n, rng)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    off = normal * rng.choice([-1.0, 1.0], (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3))
    kind = np.arange(n) % 8
    dist = np.array([0.0, 0.0, 0.02, 0.0, 0.05, 0.0, 0.6, 0.0])[kind][:, None]
    position = p + off * dist
    direction = -off * rng.uniform(0.5, 2.0, (n, 1))
    outside = kind % 2 == 1
    out_dir = rng.normal(size=(n, 3))
    out_dir /= np.linalg.norm(out_dir, axis=1, keepdims=True)
    position[outside] = (np.array([0.0, 0.0, -3.0]) + out_dir * 6.0)[outside]
    direction[outside] = ((p - position) * rng.uniform(0.1, 0.4, (n, 1)))[outside]  # toward a point of the surface
    direction[kind == 3] = out_dir[kind == 3]
    rotation = rng.normal(size=(n, 4)) * rng.uniform(0.2, 3.0, (n, 1))
    return api.make_pose_sweeps(position.astype(F32), rotation.astype(F32), direction.astype(F32), INF)


# every way a pose can be invalid (mesh_pose_rules.h, rule 1)
NAN = np.nan
INVALID_POSES = {  # position, rotation
    "zero_quaternion": ((0, 0, 0), (0, 0, 0, 0)),
    "norm_overflows": ((0, 0, 0), (3e19, 3e19, 0, 1)),
    "norm_underflows": ((0, 0, 0), (1e-30, 0, 0, 1e-30)),
    "nan_position": ((NAN, 0, 0), (0, 0, 0, 1)),
    "inf_position": ((0, -INF, 0), (0, 0, 0, 1)),
    "nan_rotation": ((1, 2, 3), (0, NAN, 0, 1)),
    "inf_rotation": ((1, 2, 3), (0, 0, INF, 1)),
}


# -- the hand-worked cases ----------------------------------------------------------------------------------------------------------
def cornell_drop():
    """The box hull of half extent 0.25 centred at (0, 0, 0) of cornell12, identity rotation, swept straight down at unit speed: its
    bottom (triangles 0 and 1, at y = -0.25) reaches the floor y = -1 (scene triangles 0 and 1) at t = 0.75 exactly, and so do the
    bottom edges of the eight side triangles.  Every one of them touches at the same t: the record must carry scene triangle 0 and
    mesh triangle 0, whose diagonal crosses the floor's.  -> (mesh, sweeps, t, prim_id, triangle)"""
    mesh = box_hull(0.25)
    sweeps = api.make_pose_sweeps(np.zeros((1, 3), F32), np.array([[0, 0, 0, 1]], F32), np.array([[0, -1, 0]], F32), INF)
    return mesh, sweeps, F32(0.75), 0, 0


def duplicated_triangle(scene):
    """A mesh that holds the same triangle twice (and a third, far smaller one first that touches later), dropped on cornell12's
    floor: the two copies tie in everything and the lower index wins.  -> (mesh, sweeps, triangle)"""
    tri = np.array([[-0.5, 0.0, -0.25], [0.5, 0.0, -0.25], [0.0, 0.0, 0.5]], F32)
    small = tri * F32(0.125) + np.array([0.0, 0.5, 0.0], F32)
    v = np.stack([small, tri, tri])
    mesh = api.make_triangles(v[:, 0], v[:, 1], v[:, 2])
    sweeps = api.make_pose_sweeps(np.zeros((1, 3), F32), np.array([[0, 0, 0, 2]], F32), np.array([[0, -2, 0]], F32), INF)
    return mesh, sweeps, 1
