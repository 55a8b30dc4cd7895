"""Shadow segments aimed at the places where the light grids (csrc/shadow_grid.hip, csrc/shadow_grid_walk.h) can go wrong: an
occluder's silhouette as the light sees it, cube-face seams and corners, cell borders, the grid's last cell and outer edge, the
near-list threshold, a key next to its own limit, and every boundary of the list bookkeeping (the block's two entries, the header's
third key, the walk's give-up at entry 31, the ordered prefix of 32, `heavy`).

numpy only: nothing here imports the library or the oracle.  test_shadow_grid_edge_cases.py checks, from the float64 reference below
alone, the conditions under which test_gpu_shadow_grid_edges.py means something.

A case is plain data (Case): occluder triangles, lights, rt_direct_light points with their tags, a ground to tessellate (the filler
that sets the grids' resolution: coarse or production) and a camera for the frames.  Every case shares one triangle box: the ground
square and four small pin triangles at the box's other extremes, so that eps_eff and the orthographic grid's frame do not depend on
the occluders.

Rungs.  Every targeted feature gets the ladder DELTAS of signed offsets across it, in the feature's own units (a triangle's
barycentric coordinates across an edge, units of u = x / z across a seam or a cube cell's border, cells across an orthographic
border, the segment's length along it).  delta > 0 is the side on which the occluder is missed.  The segment's ORIGIN o = P + N * 1e-3
is what is aimed: P is chosen so that the line from o along L - P passes through the target, whatever the normal.

Normals.  Every position gets eight unit normals: one toward the light, seven with N.l = 0.05 in seven directions around the
segment, which makes the origin offset sideways - what the lists' cone dilation exists for."""
import dataclasses

import numpy as np

F32 = np.float32
EXT_EPS = 1e-3        # shadow_grid_walk.h:55 (EXT_EPS, device_common.h:624)
MIN_T = 1e-5          # device_common.h:17, the range shadow_grid_walk.h:107 applies
MIN_A = 1e-5          # device_common.h:121
CLEAR = 1e-4
F32_MAX = float(np.finfo(np.float32).max)
DELTAS = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 3e-4, -3e-4, 1e-3, -1e-3, 1e-2, -1e-2)
N_NORMALS = 8
TILT = 0.05
WALK = 31             # RT_WF_GRID_WALK, shadow_grid_walk.h:26
SORTED_PREFIX = 32    # RT_SG_SORTED_PREFIX, shadow_grid.h:66
HEAVY = 128           # ShadowGridOptions::heavy, shadow_grid.h:74
STACK_KS = (1, 2, 3, 4, 31, 32, 33, 128, 129)

GROUND = dict(z=-20.0, size=60.0)              # the filler: a square in the plane z = -20, centred on the origin
GROUND_N = {"coarse": 8, "production": 390}    # quads per side: 128 / 304 200 triangles
PINS = np.array([[(49.0, 0.0, 0.0), (50.0, 0.0, 0.0), (49.0, 1.0, 0.0)],
                 [(20.0, 20.0, 19.0), (21.0, 20.0, 20.0), (20.0, 21.0, 19.0)],
                 [(-30.0, -30.0, -19.0), (-29.0, -30.0, -19.0), (-30.0, -29.0, -19.0)],
                 [(29.0, 30.0, -19.0), (30.0, 30.0, -19.0), (30.0, 29.0, -19.0)]], F32)
BOX_LO, BOX_HI = np.array([-30.0, -30.0, -20.0]), np.array([50.0, 30.0, 20.0])
POINT_L = np.array([0.0, 0.0, 6.0])            # exact in f32
SPOT_DIR = np.array([0.0, 0.0, 1.0])           # stacks / depth: the spot light looks up, at its points
DIR_TOWARD = np.array([0.1, 0.2, 0.97])        # directional lights: the direction TOWARD the light, before normalisation
ORTHO_UNIT = 16.0                              # the ladder's unit across an orthographic border: the coordinates' size (1e-7: an ulp)


@dataclasses.dataclass
class Case:
    name: str
    occluders: np.ndarray      # (n, 3, 3) f32, the pins included
    lights: list               # dicts: kind ("point" | "spot" | "directional"), position, direction (the light's own, away from it)
    points: np.ndarray         # (n, 8) f32 rt_surface_point records, material 0
    tags: dict                 # per point: light, feature, delta (nan: not a rung), role; per case: whatever the builder adds
    camera: tuple              # (position, direction)


# ---------------------------------------------------------------------------------------------------------------------------------
# restated rules (float64 unless a line says f32)
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def neg_ndir32(light):
    """DevLight::neg_ndir: -normalize(direction) in f32."""
    d = np.asarray(light["direction"], F32)
    with np.errstate(all="ignore"):
        return -(d * (F32(1.0) / np.sqrt(_dot32(d, d))))


def segment32(light, points):
    """shadow_grid_walk.h:52-55 / device_common.h:764-772 in f32: o = P + N * 1e-3, d = normalize(L - P), dist."""
    P, N = points[:, 0:3], points[:, 4:7]
    o = P + N * F32(EXT_EPS)
    if light["kind"] == "directional":
        return o, np.broadcast_to(neg_ndir32(light), P.shape).astype(F32), np.full(len(P), F32_MAX, F32)
    to_light = np.asarray(light["position"], F32)[None, :] - P
    dist = np.sqrt(_dot32(to_light, to_light)).astype(F32)
    with np.errstate(all="ignore"):
        d = to_light * (F32(1.0) / dist)[:, None]
    return o, d, dist


def pow2_at_least(v):
    r = 1
    while r < v and r < (1 << 30):
        r <<= 1
    return r


def resolution(kind, leaves):
    """shadow_grid.hip:408 / :434 with ShadowGridOptions' 2048 / 1024 (n_real: the leaves of the tree, four records each)."""
    if kind == "directional":
        return min(max(pow2_at_least(4.0 * np.sqrt(leaves)), 32), 2048)
    return min(max(pow2_at_least(2.0 * np.sqrt(leaves)), 16), 1024)


def eps_eff(L, lo=BOX_LO, hi=BOX_HI):
    """shadow_grid.hip:424-432."""
    L = np.asarray(L, np.float64)
    c_max = max(np.abs(lo).max(), np.abs(hi).max(), np.abs(L).max())
    d_max = np.sqrt((np.maximum(np.abs(L - lo), np.abs(L - hi)) ** 2).sum())
    return EXT_EPS * 1.01 + 2.0e-6 * (d_max + c_max), d_max, c_max


def r_near(L, res):
    """shadow_grid.hip:232-233: cone_cells = 3.5 * eps_eff / r_min * scale > 8 sends a triangle to the near list."""
    return 3.5 * eps_eff(L)[0] * (0.5 * res) / 8.0


def cube_limit_margin(L):
    """shadow_grid.hip:442."""
    e, d_max, _ = eps_eff(L)
    return float(F32(2.0 * e + 1.0e-5 * d_max))


def cube_cell(w, res):
    """shadow_grid_walk.h:67-75 for w = -d, the direction from the light toward the vertex -> face, ix, iy, fu, fv."""
    w = np.asarray(w, np.float64).reshape(-1, 3)
    ax = np.abs(w)
    a = np.where((ax[:, 0] >= ax[:, 1]) & (ax[:, 0] >= ax[:, 2]), 0, np.where(ax[:, 1] >= ax[:, 2], 1, 2))
    r = np.arange(len(w))
    wa, wb, wc = w[r, a], w[r, (a + 1) % 3], w[r, (a + 2) % 3]
    scale = 0.5 * res
    fu, fv = (wb / np.abs(wa) + 1.0) * scale, (wc / np.abs(wa) + 1.0) * scale
    ix = np.clip(np.floor(fu), 0, res - 1).astype(np.int64)
    iy = np.clip(np.floor(fv), 0, res - 1).astype(np.int64)
    return 2 * a + (wa < 0), ix, iy, fu, fv


def ortho_frame(light, res, lo=BOX_LO, hi=BOX_HI):
    """shadow_grid.hip:389-422: the grid's axes, corner, scale, key_top, margins - the f32 values the device holds, as float64."""
    w = neg_ndir32(light).astype(np.float64)
    least = 0
    for a in (1, 2):
        if abs(w[a]) < abs(w[least]):
            least = a
    axis = np.zeros(3)
    axis[least] = 1.0
    u = np.cross(w, axis)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    corners = np.array([[(hi if k & 1 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 4 else lo)[2]] for k in range(8)])
    pu, pv, ps = corners @ u, corners @ v, corners @ w
    c_max = max(np.abs(lo).max(), np.abs(hi).max())
    extent = max(pu.max() - pu.min(), pv.max() - pv.min(), 1e-6) * (1.0 + 4.0 / res) + 1e-5 * c_max + 1e-30
    scale = res / extent
    f = lambda x: float(F32(x))
    return dict(au=u.astype(F32).astype(np.float64), av=v.astype(F32).astype(np.float64), aw=w, res=res, scale=f(scale),
                u0=f(0.5 * (pu.min() + pu.max()) - 0.5 * extent), v0=f(0.5 * (pv.min() + pv.max()) - 0.5 * extent),
                key_top=f(ps.max() + 1.0 + 1e-3 * c_max), limit_margin=f(1.0e-4 + 4.0e-6 * c_max),
                margin_cells=f(0.5 + 1.6e-6 * c_max * scale * 4.0))


def ortho_cell(fr, o):
    """shadow_grid_walk.h:78-80 for the segment's origin o -> fu, fv, inside."""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    fu, fv = (o @ fr["au"] - fr["u0"]) * fr["scale"], (o @ fr["av"] - fr["v0"]) * fr["scale"]
    return fu, fv, (fu >= 0) & (fu < fr["res"]) & (fv >= 0) & (fv < fr["res"])


def tri_dist(L, tris):
    """Distance from L to each triangle (what shadow_grid.hip:66-99 computes in f32)."""
    out = []
    for v0, v1, v2 in np.asarray(tris, np.float64):
        n = np.cross(v1 - v0, v2 - v0)
        best = np.inf
        if np.linalg.norm(n) > 0:
            n = n / np.linalg.norm(n)
            q = L - n * ((L - v0) @ n)
            m = np.array([v1 - v0, v2 - v0]).T
            uv = np.linalg.lstsq(m, q - v0, rcond=None)[0]
            if uv[0] >= 0 and uv[1] >= 0 and uv.sum() <= 1:
                best = abs((L - v0) @ n)
        for a, b in ((v0, v1), (v1, v2), (v2, v0)):
            t = np.clip(((L - a) @ (b - a)) / max((b - a) @ (b - a), 1e-300), 0, 1)
            best = min(best, np.linalg.norm(L - (a + t * (b - a))))
        out.append(best)
    return np.array(out)


def cube_key(L, tris):
    """shadow_grid.hip:229-231: the nearest point's distance shrunk by 1e-4 of itself and 1e-5 of the triangle's extent."""
    t = np.asarray(tris, np.float64)
    extent = np.linalg.norm(t[:, 1] - t[:, 0], axis=1) + np.linalg.norm(t[:, 2] - t[:, 0], axis=1)
    return np.maximum(tri_dist(np.asarray(L, np.float64), t) * (1.0 - 1.0e-4) - 1.0e-5 * extent, 0.0)


def in_near_list(L, tris, res):
    """shadow_grid.hip:232-233."""
    return cube_key(L, tris) < r_near(L, res)


def widened_box(lo=BOX_LO, hi=BOX_HI):
    """direct_light.h:25-29."""
    m = (hi - lo).max()
    return lo - m, hi + m


def walk(keys, limit, hits):
    """shadow_grid_walk.h:97-153 for one segment over its cell's list in key order (hits[i]: entry i is accepted) ->
    (answered, entries read).  No near list."""
    count = len(keys)
    if count > HEAVY:
        return False, 0
    reads = 0
    for i in range(count):
        if i >= WALK:
            return False, reads
        if not keys[i] < limit:
            return True, reads
        reads += 1
        if hits[i]:
            return True, reads
    return True, reads


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 reference
def device_triangles(tris):
    """(v0, e1, e2) as the records hold them: f32 differences (bvh_rules.h:311)."""
    t = np.asarray(tris, F32)
    return t[:, 0].astype(np.float64), (t[:, 1] - t[:, 0]).astype(np.float64), (t[:, 2] - t[:, 0]).astype(np.float64)


EPS32 = 2.0 ** -24
ROUNDINGS = 8.0


def f32_slack(reach, e1n, e2n, a, s_len, t_scale):
    """How far the f32 triangle test (device_common.h:118-135) may be from the float64 one, per term (u, v, 1 - u - v, t / scale).
    u = f * dot(s, cross(d, e2)), v = f * dot(d, cross(s, e1)), t = f * dot(e2, cross(s, e1)) with f = 1 / a: a cross product and a
    dot product are three products and two sums each, nested: about eight roundings of terms as large as the factors' magnitudes,
    |s| |e2|, |s| |e1| and |s| |e1| |e2|; s = o - v0 itself carries the rounding of o.  With reach = |s| + |o| that is
    8 * 2^-24 * reach * (|e2|, |e1|, |e1| |e2| |s| / scale) / |a|: the test places a ray within 5e-7 of its reach, which is 1e-4 of a
    triangle's side only while the side is 1 / 200 of the reach or more."""
    k = ROUNDINGS * EPS32 * reach / np.abs(a)
    du, dv = k * e2n, k * e1n
    return du, dv, du + dv, k * e1n * e2n * s_len / t_scale


def reference(case):
    """Brute force in float64 over the f32 segments the device composes -> dict(
    margin (n, L, T): the smallest of u, v, 1 - u - v, (t - 1e-5) / dist, (dist - t) / dist, (|a| - 1e-5) / (|e1| |e2|) - the
        triangle is accepted iff it is >= 0 (a directional light's segment has no end: its t is taken relative to the box's diagonal),
    segment (n, L): the facing (and spot) terms are positive, lit (n, L), clear (n, L)).
    A pair is clear when the facing terms are 1e-4 from zero and, for every occluder, either |a| is 1e-4 under its threshold (relative
    to |e1| |e2|), or some other term is negative by 1e-4 - and by f32_slack() of that term, which is more than 1e-4 only for triangles
    under 1 / 200 of their distance from the origin - or |a| is 1e-4 over its threshold and every term is positive by that much."""
    pts = case.points
    n, n_l = len(pts), len(case.lights)
    v0, e1, e2 = device_triangles(case.occluders)
    n_t = len(v0)
    margin = np.zeros((n, n_l, n_t))
    segment, clear = np.zeros((n, n_l), bool), np.zeros((n, n_l), bool)
    N = pts[:, 4:7].astype(np.float64)
    diag = np.linalg.norm(BOX_HI - BOX_LO)
    for li, light in enumerate(case.lights):
        o32, d32, dist32 = segment32(light, pts)
        o, d, dist = o32.astype(np.float64), d32.astype(np.float64), dist32.astype(np.float64)
        terms = [(N * d).sum(1)]
        if light["kind"] == "spot":
            terms.append(d @ neg_ndir32(light).astype(np.float64))
        if light["kind"] != "directional":
            terms.append(1.0 / (1.0 + dist ** 2 * 0.01))
        terms = np.stack(terms, 1)
        segment[:, li] = (terms > 0).all(1)
        ok = (np.abs(terms) >= CLEAR).all(1)
        t_scale = np.full(n, diag) if light["kind"] == "directional" else dist
        o_len = np.linalg.norm(o, axis=1)
        for k in range(n_t):
            e1n, e2n = np.linalg.norm(e1[k]), np.linalg.norm(e2[k])
            with np.errstate(all="ignore"):
                h = np.cross(d, e2[k])
                a = h @ e1[k]
                a = np.where(np.abs(a) < 1e-30, 1e-30, a)  # (a ray parallel to the plane: the terms and their slack grow alike)
                f = 1.0 / a
                s = o - v0[k]
                u = f * (s * h).sum(1)
                q = np.cross(s, e1[k])
                v = f * (d * q).sum(1)
                t = f * (q @ e2[k])
                s_len = np.linalg.norm(s, axis=1)
                m = np.stack([u, v, 1.0 - u - v, (t - MIN_T) / t_scale, (dist - t) / t_scale], 1)
                du, dv, dw, dt = f32_slack(s_len + o_len, e1n, e2n, a, s_len, t_scale)
                slack = np.maximum(np.stack([du, dv, dw, dt, dt], 1), CLEAR)
                a_term = (np.abs(a) - MIN_A) / (e1n * e2n)
                # rejected for |a|, or by the term that is most negative relative to its slack (term and slack both grow as 1 / |a|, so
                # this holds for a ray in the triangle's plane too), or accepted with |a| and every term over its slack
                rel = (m / slack).min(1)
                ok &= (a_term <= -CLEAR) | (rel <= -1.0) | ((a_term >= CLEAR) & (rel >= 1.0))
            margin[:, li, k] = np.minimum(m.min(1), a_term)
        clear[:, li] = ok | ~segment[:, li] & (np.abs(terms) >= CLEAR).all(1)
    hit = (margin >= 0).any(2) if n_t else np.zeros((n, n_l), bool)
    return dict(margin=margin, segment=segment, lit=segment & ~hit, clear=clear)


def ground_clearance(case):
    """The smallest distance, along z, between any segment and the ground's plane (the ground lies under everything)."""
    worst = np.inf
    for light in case.lights:
        o, d, _ = segment32(light, case.points)
        worst = min(worst, float(o[:, 2].min()) - GROUND["z"])
        if light["kind"] == "directional":
            assert d[0, 2] > 0  # the segments rise
        else:
            worst = min(worst, float(light["position"][2]) - GROUND["z"])
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# points
def normals8(l):
    """(m, 3) unit directions toward the light -> (m, 8, 3) unit normals: l itself, and seven with N.l = TILT around it."""
    l = _unit(l)
    least = np.argmin(np.abs(l), axis=1)
    a = _unit(np.cross(l, np.eye(3)[least]))
    b = np.cross(l, a)
    out = [l]
    for k in range(N_NORMALS - 1):
        phi = 0.3 + 2.0 * np.pi * k / (N_NORMALS - 1)
        out.append(TILT * l + np.sqrt(1.0 - TILT * TILT) * (np.cos(phi) * a + np.sin(phi) * b))
    return np.stack(out, 1)


def aim(light, X, s):
    """rt_surface_point records (m * 8, 8) f32 whose segments' lines pass through the targets X (m, 3): for a point or spot light
    P = L + s * (X - N * 1e-3 - L) (s > 1: the target lies between P and the light; s = 1: the origin IS the target), for a
    directional one P = X - N * 1e-3 - s * toward (s in world units)."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    s = np.broadcast_to(np.asarray(s, np.float64), (len(X),))[:, None, None]
    if light["kind"] == "directional":
        toward = neg_ndir32(light).astype(np.float64)
        N = normals8(np.broadcast_to(toward, X.shape))
        P = X[:, None, :] - N * EXT_EPS - s * toward
    else:
        L = np.asarray(light["position"], np.float64)
        N = normals8(L - X)
        P = L + s * (X[:, None, :] - N * EXT_EPS - L)
    rec = np.zeros((len(X) * N_NORMALS, 8), F32)
    rec[:, 0:3], rec[:, 4:7] = P.reshape(-1, 3), N.reshape(-1, 3)
    return rec


class _Points:
    def __init__(self):
        self.rec, self.light, self.feature, self.delta, self.role = [], [], [], [], []
        self.features = []  # names, index = feature id

    def feature_id(self, name):
        self.features.append(name)
        return len(self.features) - 1

    def add(self, light_index, light, X, s, feature, delta=np.nan, role=0):
        X = np.asarray(X, np.float64).reshape(-1, 3)
        m = len(X) * N_NORMALS
        self.rec.append(aim(light, X, s))
        for lst, v in ((self.light, light_index), (self.feature, feature), (self.delta, delta), (self.role, role)):
            lst.append(np.repeat(np.broadcast_to(np.asarray(v), (len(X),)), N_NORMALS))
        return m

    def done(self):
        tags = dict(light=np.concatenate(self.light).astype(np.int64), feature=np.concatenate(self.feature).astype(np.int64),
                    delta=np.concatenate(self.delta).astype(np.float64), role=np.concatenate(self.role).astype(np.int64), features=list(self.features))
        return np.ascontiguousarray(np.concatenate(self.rec)), tags


def _light(kind, position=POINT_L, direction=None):
    if kind == "point":
        return dict(kind="point", position=np.asarray(position, np.float64), direction=np.zeros(3))
    if kind == "spot":
        return dict(kind="spot", position=np.asarray(position, np.float64), direction=np.asarray(SPOT_DIR if direction is None else direction, np.float64))
    return dict(kind="directional", position=np.zeros(3), direction=-np.asarray(DIR_TOWARD if direction is None else direction, np.float64))


def _camera(points, occluders):
    pos = points[:, 0:3].astype(np.float64).mean(0)
    at = np.asarray(occluders, np.float64).reshape(-1, 3).mean(0)
    return tuple(pos), tuple(_unit(at - pos))


def _case(name, occluders, lights, pts):
    occ = np.concatenate([np.asarray(occluders, F32).reshape(-1, 3, 3), PINS])
    points, tags = pts.done()
    return Case(name, occ, lights, points, tags, _camera(points, occ[:-len(PINS)]))


def _bary(tri, u, v):
    """v0 + u e1 + v e2 of the device's triangle, float64."""
    v0, e1, e2 = device_triangles(np.asarray(tri, F32)[None])
    return v0[0] + np.asarray(u)[..., None] * e1[0] + np.asarray(v)[..., None] * e2[0]


EDGE_PLACES = (0.1, 0.3, 0.5, 0.7, 0.9)


def silhouette_targets(tri, toward, reach):
    """The ladder across each edge of `tri` at five places and across each vertex -> list of (feature name, delta, X): delta > 0
    outside.  The unit is the barycentric coordinate that decides across the feature - or, on a needle or a triangle that is small for
    its distance, as much more of it (k) as keeps the rung of 3e-4 at twice what the f32 test can place (f32_slack; `toward`: the
    unit direction to the light, `reach`: the largest |s| + |o| of the points to come)."""
    v0, e1, e2 = (x[0] for x in device_triangles(np.asarray(tri, F32)[None]))
    corners = [v0, v0 + e1, v0 + e2, v0 + (e1 + e2) / 3.0]  # (a triangle next to a point light is seen at another angle from every corner)
    a = min(abs(e1 @ np.cross(toward(x) if callable(toward) else toward, e2)) for x in corners)
    du, dv, _, _ = f32_slack(reach, np.linalg.norm(e1), np.linalg.norm(e2), a, 1.0, 1.0)
    k = max(1.0, 2.0 * (du + dv) / 3e-4)  # (du + dv: the slack of 1 - u - v)
    centre = np.array([1.0 / 3.0, 1.0 / 3.0])
    out = []

    def rung(name, d, at):
        # from the feature's point `at` (barycentric u, v) toward the centroid (d < 0: inside) or away from it, by 3 |d| k of the way and
        # no farther than the centroid's own distance: across an edge the coordinate that decides moves by |d| k
        lam = min(1.0, 3.0 * abs(d) * k)
        uv = np.asarray(at) - np.sign(d) * lam * (centre - np.asarray(at))
        out.append((name, d, _bary(tri, uv[0], uv[1])))
    for d in DELTAS:
        for f in EDGE_PLACES:
            rung("edge01", d, (f, 0.0))
            rung("edge02", d, (0.0, f))
            rung("edge12", d, (f, 1.0 - f))
        rung("vertex0", d, (0.0, 0.0))
        rung("vertex1", d, (1.0, 0.0))
        rung("vertex2", d, (0.0, 1.0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# builders
def _tangent_triangle(L, direction, r, size, rng, right_angle=False):
    """A triangle of about `size` around L + r * direction, facing the light roughly (tilted by up to ~35 degrees)."""
    c = L + r * _unit(direction)
    n = _unit(_unit(direction) + 0.6 * rng.uniform(-1, 1, 3))
    a = _unit(np.cross(n, np.eye(3)[np.argmin(np.abs(n))]))
    b = np.cross(n, a)
    if right_angle:
        return np.array([c, c + size * a, c + size * b])
    ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.3, 0.3, 3)
    return np.array([c + 0.6 * size * (np.cos(t) * a + np.sin(t) * b) for t in ang])


def _needle(L, direction, r, cells_long, factor, res):
    """A right-angled needle lying diagonally in its cube face's cells, cells_long cells long, whose doubled area in cell units is
    `factor` times the sliver rule's threshold 1e-3 * box + 1e-3 (shadow_grid.hip:143)."""
    direction = _unit(direction)
    c = L + r * direction
    a = _unit(np.cross(direction, (0.0, 0.0, 1.0)))
    b = np.cross(direction, a)
    cell = 2.0 / res * r  # a cell's width at this distance, near the face's middle
    diag = _unit(a + b)
    across = np.cross(direction, diag)
    length = min(cells_long, 3.0 / cell)  # (at most three units long: a coarse grid's cells are wide)
    width = factor * (1e-3 * (length * length / 2.0) + 1e-3) / length
    return np.array([c, c + length * cell * diag, c + width * cell * across])


def silhouettes(kind, res):
    """About 35 occluders between one light and free-space points, the ladder across every edge (five places) and vertex of each, at
    s = 1.5 and 4 (world units for the directional light)."""
    rng = np.random.default_rng(7)
    light = _light(kind, direction=(-0.15, 0.0, -1.0) if kind == "spot" else None)
    occ, names = [], []
    if kind == "directional":
        toward = _unit(DIR_TOWARD)
        fr = ortho_frame(light, res)
        cell = 1.0 / fr["scale"]
        for j in range(5):
            for i in range(5):
                c = np.array([-8.0 + 4.0 * i, -8.0 + 4.0 * j, 1.0 + 0.5 * ((i * 3 + j) % 5)])
                occ.append(_tangent_triangle(c, toward, 0.0, 1.2, rng)), names.append("ordinary")
        for i in range(4):  # smaller than a production cell (0.04), and still accepted by the test (|a| > 1e-5)
            occ.append(_tangent_triangle(np.array([-12.0 + 8.0 * i, 13.0, 2.0]), toward, 0.0, 0.02, rng, right_angle=True)), names.append("tiny")
        occ.append(np.array([(14.0, -25.0, 3.0), (44.0, -20.0, 5.0), (20.0, 22.0, 2.0)])), names.append("large")
        for i, factor in enumerate((0.5, 2.0, 0.5, 2.0)):  # needles on both sides of the sliver rule, diagonal in the grid's cells
            c = np.array([-14.0 + 9.0 * i, -14.0, 2.0])
            diag = _unit(fr["au"] + fr["av"]) if i < 2 else _unit(fr["au"] - fr["av"])
            across = np.cross(toward, diag)
            length = min(40.0, 3.0 / cell)  # (long: the rule's threshold grows with the box, and a needle 40 cells long is wide enough for f32)
            width = factor * (1e-3 * (length * length / 2.0) + 1e-3) / length
            occ.append(np.array([c, c + length * cell * diag, c + width * cell * across])), names.append(f"needle x{factor}")
    else:
        L = POINT_L
        rn = r_near(L, res)
        for j, y in enumerate((-1.5, -0.9, -0.3, 0.3, 0.9, 1.5)):  # under the light: the -z face and over its seams into the side faces
            for i, x in enumerate((-0.3, 0.3, 0.9, 1.5)):
                occ.append(_tangent_triangle(L, (x, y, -1.0), 3.2 * np.sqrt(1 + x * x + y * y), 0.5, rng)), names.append("ordinary")
        for i, az in enumerate((60, 80, 100, 130)):   # smaller than a production cell (0.002 of the distance), |a| > 1e-5 still
            d = (np.cos(np.radians(az)), np.sin(np.radians(az)), -0.1)
            occ.append(_tangent_triangle(L, d, 12.0, 0.012, rng, right_angle=True)), names.append("tiny")
        for i, (az, factor) in enumerate(((215, 0.5), (240, 2.0), (265, 0.5), (290, 2.0))):
            d = (np.cos(np.radians(az)), np.sin(np.radians(az)), -0.1)
            occ.append(_needle(L, d, 20.0, 40.0, factor, res)), names.append(f"needle x{factor}")
        occ.append(np.array([(-9.0, -7.0, 8.0), (9.0, -7.0, 8.0), (0.0, 10.0, 8.0)])), names.append("larger than a face")
        # its plane passes 1.5 r_near over the light (0.15 at least: seen at less than a degree f32 places no ray on it); it lies across
        # +x and reaches into +y and -y
        h = max(1.5 * rn, 0.15)
        occ.append(np.array([(3.0, -9.0, 6.0 + h), (3.0, 9.0, 6.0 + h), (12.0, 0.0, 6.0 + h)])), names.append("plane next to the light")
        occ.append(np.array([(-3.2, -1.0, 3.0), (-3.2, 1.0, 3.0), (-9.0, 0.0, 8.0)])), names.append("vertex behind the -z face")
    occ = np.asarray(np.asarray(occ), F32)
    pts = _Points()
    for k, tri in enumerate(occ):
        mid = tri.astype(np.float64).mean(0)
        if kind == "directional":  # (the points lie up to 4 under the target, at coordinates up to the box's)
            targets = silhouette_targets(tri, _unit(DIR_TOWARD), 5.0 + np.linalg.norm(mid) + 5.0)
        else:                      # (s = 4: the origin lies 3 r behind the target, 4 r from the light)
            r = np.linalg.norm(mid - POINT_L)
            targets = silhouette_targets(tri, lambda x: _unit(POINT_L - x), 3.0 * r + 4.0 * r + np.linalg.norm(POINT_L))
        ids = {}
        for name, d, X in targets:
            if name not in ids:
                ids[name] = pts.feature_id(f"{names[k]} {k} {name}")
        for s in (1.5, 4.0):
            for name in ids:
                sel = [(d, X) for nm, d, X in targets if nm == name]
                pts.add(0, light, np.array([X for _, X in sel]), s, ids[name], delta=np.array([d for d, _ in sel]), role=k)
    case = _case(f"silhouettes {kind} res {res}", occ, [light], pts)
    case.tags["occluder_names"] = names
    return case


def depth_ladder(kind):
    """P on the ladder ALONG the segment across an occluder's plane, in units of the target's distance from the light (of the box's diagonal
    for the directional light, whose segments have no length): at the triangle's point nearest to the light, where key and limit are closest, and far from it on a large one."""
    light = _light(kind)
    if kind == "directional":
        toward = neg_ndir32(light).astype(np.float64)
        a = _unit(np.cross(toward, (1.0, 0.0, 0.0)))
        b = np.cross(toward, a)
        c0, c1 = np.array([2.0, 3.0, 4.0]), np.array([-6.0, -4.0, 3.0])
        small = np.array([c0 - 0.5 * a - 0.4 * b, c0 + 0.7 * a - 0.3 * b, c0 + 0.1 * a + 0.8 * b])                # across the light's direction
        large = np.array([c1 - 9.0 * a - 7.0 * b - 2.0 * toward, c1 + 11.0 * a - 6.0 * b + 1.0 * toward, c1 + 1.0 * a + 12.0 * b + 3.0 * toward])
        targets = [("small, its middle", small, (0.3, 0.3)), ("large, its highest corner", large, (0.02, 0.96)), ("large, far from it", large, (0.45, 0.05))]
        unit, away = float(np.linalg.norm(BOX_HI - BOX_LO)), -toward
    else:
        L = POINT_L
        small = np.array([(-0.6, -0.5, 10.0), (0.8, -0.4, 10.0), (0.1, 0.9, 10.0)])     # L's foot (0, 0, 10) lies inside: r_min = 4
        large = np.array([(-11.0, -8.0, 12.0), (12.0, -7.0, 11.0), (1.0, 13.0, 13.0)])  # behind it, its foot inside too
        n = _unit(np.cross(large[1] - large[0], large[2] - large[0]))
        foot = L + n * ((large[0] - L) @ n)
        uv = np.linalg.lstsq(np.array([large[1] - large[0], large[2] - large[0]]).T, foot - large[0], rcond=None)[0]
        assert uv.min() > 0.1 and uv.sum() < 0.9
        targets = [("small, its nearest point", small, (float(np.linalg.lstsq(np.array([small[1] - small[0], small[2] - small[0]]).T, np.array([0.0, 0.0, 10.0]) - small[0], rcond=None)[0][0]),
                                                        float(np.linalg.lstsq(np.array([small[1] - small[0], small[2] - small[0]]).T, np.array([0.0, 0.0, 10.0]) - small[0], rcond=None)[0][1]))),
                   ("large, far from its nearest point", large, (0.05, 0.9)), ("large, far from it, the other way", large, (0.85, 0.08))]
        unit, away = None, None
    occ = np.asarray(np.array([small, large]), F32)
    pts = _Points()
    for name, tri, (u, v) in targets:
        X = _bary(tri, u, v)
        if kind == "directional":
            step, back = unit, away
        else:
            step, back = np.linalg.norm(X - POINT_L), _unit(X - POINT_L)
        if name.startswith("large") and kind != "directional":
            # the small triangle must not shade the large one's targets
            assert abs(_unit(X - POINT_L)[2]) < 0.95
        fid = pts.feature_id(name)
        # delta > 0: the origin lies in FRONT of the plane (toward the light): the occluder is missed
        Xs = np.array([X - d * step * back for d in DELTAS])
        pts.add(0, light, Xs, 1.0 if kind != "directional" else 0.0, fid, delta=np.array(DELTAS))
    return _case(f"depth ladder {kind}", occ, [light], pts)


def _stack_layout(res):
    """The cube cells of the nine stacks (face, ix, iy): next to the middles of the faces +z, -x, +y and -y, where u and v are small -
    a strip's distance from the light is z * sqrt(1 + u^2 + v^2), and only there does it follow the depth z alone - and at or above
    the light's height, where nothing of the ground or the pins projects.  The strips run along +v and are dilated by up to a cell:
    two stacks of one face lie three columns apart."""
    h = res // 2
    return [(4, h - 2, h), (4, h + 1, h), (1, h - 2, h), (1, h + 1, h), (0, h - 2, h), (0, h + 1, h), (2, h, h), (2, h + 3, h), (3, h, h)]


def stacks(kind, res):
    """Per K in STACK_KS: K disjoint narrow right-angled strips side by side in the middle 60 % of ONE cell's directions, at strictly
    increasing distance from the light (their key order is their index); nothing else projects into that cell.  Points (roles):
      0  behind all strips, aimed at strip j's middle: occluded by strip j - and by no other when the normal points at the light; a
         sideways origin offset leaves the line 1e-3 beside the light, so that away from the target it may cross a neighbour too
      1  behind all strips, aimed at the gap after strip j: lit (with the same reservation)
      2  between the depths of strips m - 1 and m, on strip m's middle: lit (strip m is behind the point)
      3  between those depths on strip m - 1's middle: occluded by strip m - 1
    tags: stack (index into STACK_KS), strip (j or m), cell (the cell all of a stack's points must look up)."""
    light = _light(kind)
    occ, pts = [], _Points()
    stack_tag, strip_tag, cells, tri_stack = [], [], [], []
    if kind == "directional":
        fr = ortho_frame(light, res)
        au, av, aw, cell = fr["au"], fr["av"], fr["aw"], 1.0 / fr["scale"]
        fu0, fv0, _ = ortho_cell(fr, np.array([[40.0, -22.0, 4.0]]))
    for si, K in enumerate(STACK_KS):
        fid = pts.feature_id(f"stack K={K}")
        pitch = 0.6 / K
        if kind == "directional":
            cu, cv = int(np.floor(fu0[0])) + 3 * si, int(np.floor(fv0[0]))
            cells.append((0, cu, cv))
            length = max(2.0, 4.0 * cell)
            depth = lambda m: 4.0 - 0.04 * m  # coordinate along aw: the light is up there, strip 0 is the nearest to it
            # (au, av, aw are orthonormal up to the f32 rounding of the axes: a position is given by its three coordinates)
            basis = np.linalg.inv(np.array([au, av, aw]))
            at = lambda fu, fv, s: basis @ np.array([fr["u0"] + fu * cell, fr["v0"] + fv * cell, s])
            for i in range(K):
                u_i = cu + 0.2 + pitch * i
                v0 = at(u_i, cv + 0.75, depth(i))
                occ.append(np.array([v0, at(u_i, cv + 0.75 - length / cell, depth(i)), at(u_i + pitch / 2, cv + 0.75, depth(i))]))
                tri_stack.append(si)
            f_c = 0.25 * cell / length  # the points' place along the strips: the cell's middle row
            mid = lambda j: at(cu + 0.2 + pitch * j + 0.45 * (pitch / 2) * (1 - f_c), cv + 0.5, depth(j))
            gap = lambda j: at(cu + 0.2 + pitch * j + 0.75 * pitch, cv + 0.5, depth(j))
            back = lambda j, m: depth(j) - depth(m - 0.5)  # how far under the target (strip j's plane) the origin lies
        else:
            L = POINT_L
            face, ix, iy = _stack_layout(res)[si]
            cells.append((face, ix, iy))
            scale = 0.5 * res
            pitch = min(pitch, 2.0e-3 * scale / K)  # (all strips within 0.002 of u: a coarse grid's cells are wide)
            lv = 0.25
            depth = lambda m: 8.0 * (1.0 + 0.004 * m)

            def at(fu, fv, z, face=face):  # shadow_grid_walk.h:69-72 the other way round
                w = np.zeros(3)
                a = face // 2
                w[a], w[(a + 1) % 3], w[(a + 2) % 3] = (-1.0 if face & 1 else 1.0), fu / scale - 1.0, fv / scale - 1.0
                return L + z * w
            lo = lambda i: ix + 0.2 + pitch * i  # strip i starts there
            for i in range(K):
                occ.append(np.array([at(lo(i), iy + 0.25, depth(i)), at(lo(i), iy + 0.25 + lv * scale, depth(i)), at(lo(i) + pitch / 2, iy + 0.25, depth(i))]))
                tri_stack.append(si)
            f_c = 0.25 / (lv * scale)
            mid = lambda j: at(lo(j) + 0.45 * (pitch / 2) * (1 - f_c), iy + 0.5, depth(j))
            gap = lambda j: at(lo(j) + 0.75 * pitch, iy + 0.5, depth(j))
            back = lambda j, m: depth(m - 0.5) / depth(j)          # aim()'s s: the origin's depth over the target's
        # (tag, target on strip j's plane, the origin's depth): the line from the origin along L - P passes through the target
        groups = [(0, [(j, mid(j), back(j, K)) for j in range(K)]), (1, [(j, gap(j), back(j, K)) for j in range(K)]),
                  (2, [(m, mid(m), back(m, m)) for m in range(K)]), (3, [(m, mid(m - 1), back(m - 1, m)) for m in range(1, K)])]
        for role, items in groups:
            if not items:
                continue
            n = pts.add(0, light, np.array([x for _, x, _ in items]), np.array([b for _, _, b in items]), fid, role=role)
            stack_tag.append(np.full(n, si))
            strip_tag.append(np.repeat(np.array([j for j, _, _ in items]), N_NORMALS))
    case = _case(f"stacks {kind} res {res}", np.asarray(np.array(occ), F32), [light], pts)
    case.tags.update(stack=np.concatenate(stack_tag), strip=np.concatenate(strip_tag), cells=cells, tri_stack=np.array(tri_stack))
    return case


def stack_expectation(case, ref, si):
    """From the restatement: for the points of stack si -> (segments, answered by the lists, entries read, tight).  The cell's list is the
    stack's K strips in index order (nothing else projects there; the CPU test checks what can be checked of that), a segment walks it
    as walk() says, with the keys and limits of shadow_grid.hip:231 / :442 (cube) and :221 / :422 (orthographic)."""
    light = case.lights[0]
    rows = np.flatnonzero(case.tags["stack"] == si)
    tri = np.flatnonzero(case.tags["tri_stack"] == si)
    tris = case.occluders[tri]
    o, d, dist = segment32(light, case.points[rows])
    if light["kind"] == "directional":
        fr = ortho_frame(light, int(case.name.split()[-1]))
        keys = fr["key_top"] - (tris.astype(np.float64) @ fr["aw"]).max(1)
        limits = fr["key_top"] - o.astype(np.float64) @ fr["aw"] + fr["limit_margin"]
    else:
        keys = cube_key(light["position"], tris)
        limits = dist.astype(np.float64) + cube_limit_margin(light["position"])
    assert np.all(np.diff(keys) > 0)
    hits = ref["margin"][rows][:, 0, :][:, tri] >= 0
    answered = reads = 0
    for r in range(len(rows)):
        a, n = walk(keys, limits[r], hits[r])
        answered += a
        reads += n
    tight = float(min(np.abs(keys[None, :] - limits[:, None]).min(), np.diff(keys).min() if len(keys) > 1 else np.inf))  # how close a key comes to a limit or to the next key
    return int(ref["segment"][rows, 0].sum()), answered, reads, tight


def near_threshold(res):
    """Around the point light: right-angled triangles whose nearest point lies at 0.8 and at 1.25 r_near from it, in six directions
    each (the key's 1e-4 shrink leaves both clear of the threshold); the ladder runs across every edge of them with the sideways
    normals, so that the origin's line passes through the occluder while P's own direction looks up another cell.  Their legs are
    0.4 r_near, and 0.006 at least: anything smaller has |a| < 1e-5 and is accepted by no ray, so at a coarse resolution (r_near =
    0.008) they are wide as the light sees them.  The far set is turned by half a turn and lies beside the near set.
    Light 1, a spot light that looks away from all of that, sits exactly on a vertex of a triangle of its own (r_min = 0: its near
    list); a segment toward it ends ON that triangle, so none of its pairs is clear - they are held to the tree only."""
    L = POINT_L
    rn = r_near(L, res)
    occ, expect_near = [], []
    dirs = [(1.0, 0.15, 0.1), (-1.0, 0.1, -0.15), (0.12, 1.0, 0.2), (-0.1, -1.0, 0.15), (0.2, -0.1, 1.0), (0.15, 0.2, -1.0)]
    size = max(0.006, 0.4 * rn)
    for factor in (0.8, 1.25):
        for dr in dirs:
            n = _unit(dr)
            a = _unit(np.cross(n, np.eye(3)[np.argmin(np.abs(n))]))
            b = np.cross(n, a)
            sgn = 1.0 if factor < 1 else -1.0
            if factor < 1:  # the light's foot lies inside, a tenth of a leg from the corner
                v0 = L + factor * rn * n - size * 0.1 * (a + b)
            else:           # the far set lies beside the foot, in the opposite quadrant: as the light sees them the two sets do not overlap
                g = 0.27 * size * np.sqrt(2.0)  # from the foot to the corner, which is the nearest point
                v0 = L + np.sqrt((factor * rn) ** 2 - g * g) * n - size * 0.27 * (a + b)
            occ.append(np.array([v0, v0 + sgn * size * a, v0 + sgn * size * b]))
            expect_near.append(factor < 1)
    occ = np.asarray(np.array(occ), F32)
    L1 = np.array([9.0, 4.0, 7.0])
    on_vertex = np.asarray(np.array([[L1, L1 + (0.5, 0.0, -0.5), L1 + (0.0, 0.5, -0.5)]]), F32)
    lights = [_light("point"), _light("spot", position=L1, direction=(-1.0, 0.0, 0.0))]  # (lights what lies at larger x only)
    pts = _Points()
    for k, tri in enumerate(occ):
        mid = tri.astype(np.float64).mean(0)
        targets = silhouette_targets(tri, lambda x: _unit(L - x), 7.0 * np.linalg.norm(mid - L) + np.linalg.norm(L))
        for name in ("edge01", "edge02", "edge12"):
            fid = pts.feature_id(f"{'near' if expect_near[k] else 'far'} {k} {name}")
            sel = [(d, X) for nm, d, X in targets if nm == name]
            for s in (1.5, 4.0):
                pts.add(0, lights[0], np.array([X for _, X in sel]), s, fid, delta=np.array([d for d, _ in sel]), role=k)
    fid = pts.feature_id("on the light")
    around = np.array([L1 + (2.0, y, z) for y in (-0.6, 0.1, 0.7) for z in (-0.9, -0.2, 0.5)])
    pts.add(1, lights[1], around, 1.0, fid, role=len(occ))
    case = _case(f"near threshold res {res}", np.concatenate([occ, on_vertex]), lights, pts)
    case.tags["expect_near"] = [int(np.sum(expect_near)), 1]
    case.tags["never_clear"] = ["on the light"]
    return case


def displaced_cells(case, res):
    """For the points aimed at light 0 with a sideways normal: how many cells lie between the cell P's direction looks up and the cell
    of the direction through the target (the origin's line)."""
    light = case.lights[0]
    rows = np.flatnonzero(case.tags["light"] == 0)
    o, d, dist = segment32(light, case.points[rows])
    L = np.asarray(light["position"], np.float64)
    face, ix, iy, _, _ = cube_cell(-d.astype(np.float64), res)
    # where the origin's line passes the occluder: its point nearest to the occluder's middle, and the direction from L through it
    tri_of = case.tags["role"][rows]
    c = np.asarray(case.occluders, np.float64)[tri_of].mean(1)
    t = ((c - o.astype(np.float64)) * d.astype(np.float64)).sum(1)
    X = o.astype(np.float64) + d.astype(np.float64) * t[:, None]
    face2, ix2, iy2, _, _ = cube_cell(X - L, res)
    tilted = np.arange(len(rows)) % N_NORMALS != 0
    apart = np.where(face == face2, np.maximum(np.abs(ix - ix2), np.abs(iy - iy2)), 99)
    return apart[tilted]


def seams_and_borders(res_cube, res_ortho):
    """Directions that fall EXACTLY (in float64, from coordinates that are exact in f32) on a cube-face seam, a cube corner, a cell
    border and the face's last cell, and origins on an orthographic cell border, the orthographic grid's last cell and outside its
    outer edges; the ladder runs across each, in units of u = x / z (cube) or cells (orthographic), behind a triangle that ENDS on the
    feature's plane (both outcomes), behind one that straddles it (occluded throughout) and in the open (lit throughout).
    Light 0: the point light (0, 0, 6); light 1: a directional light straight down (its grid's axes are +y and -x)."""
    L = POINT_L
    point, sun = _light("point"), _light("directional", direction=(0.0, 0.0, 1.0))
    lights = [point, sun]
    pts = _Points()
    occ = []
    exact = []  # (feature id, direction (3,) exact in f64, what) for the builder's own assertion
    scale = 0.5 * res_cube
    k_border = res_cube // 2 + res_cube // 8 + 1          # a cell border right of the face's middle
    g = k_border / scale - 1.0                             # u of that border: a dyadic number
    # planes through L, each given by (name, in-plane directions p and q, across direction c): a target direction is p + f q + delta c
    planes = [("seam +x/+y", np.array([1.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([0.0, -1.0, 0.0]), (-0.5, -0.25, 0.25, 0.5)),
              ("seam +x/-z", np.array([1.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), (-0.5, -0.25, 0.25, 0.5)),
              ("cell border, face -y", np.array([g, -1.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([-1.0, 0.0, 0.0]), (-0.5, -0.25, 0.25, 0.5)),
              ("corner +x+y+z", np.array([1.0, 1.0, 1.0]), np.array([0.0, 0.0, 0.0]), np.array([0.0, -1.0, -0.5]), (0.0,)),
              ("corner -x-y-z", np.array([-1.0, -1.0, -1.0]), np.array([0.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.5]), (0.0,))]
    for name, p, q, c, places in planes:
        # a triangle that ends on the plane (its edge 0-1 lies in it, the rest on the side of -c), one that straddles it, at r ~ 4 and 5
        far = 4.0
        if name.startswith("corner"):
            ends = np.array([L + far * (p + 0.25 * np.cross(p, c)), L + far * (p - 0.25 * np.cross(p, c)), L + far * (p - 0.5 * c)])
            occ.append(ends)
            fid = pts.feature_id(name)
            for s in (1.5, 4.0):
                dirs = np.array([p + d * c for d in DELTAS])
                pts.add(0, point, L + far * dirs, s, fid, delta=np.array(DELTAS), role=len(occ) - 1)
            exact.append((name, p))
            continue
        ends = np.array([L + far * (p - 0.75 * q), L + far * (p + 0.125 * q), L + far * (p - 0.25 * q - 0.5 * c)])
        straddles = np.array([L + 5.0 * (p + 0.1875 * q - 0.25 * c), L + 5.0 * (p + 0.1875 * q + 0.25 * c), L + 5.0 * (p + 0.625 * q)])
        occ.append(ends), occ.append(straddles)
        for f in places:
            fid = pts.feature_id(f"{name} at {f}")
            dirs = np.array([p + f * q + d * c for d in DELTAS])
            for s in (1.5, 4.0):
                pts.add(0, point, L + far * dirs, s, fid, delta=np.array(DELTAS), role=len(occ) - 2)
            exact.append((name, p + f * q))
    n_cube_occ = len(occ)
    # the orthographic grid: a border between two cells, in u (world y) and in v (world -x), under a triangle that ends on it
    fr = ortho_frame(sun, res_ortho)
    cell = 1.0 / fr["scale"]
    ku, kv = res_ortho // 2 + 3, res_ortho // 2 - 5
    yb, xb = fr["u0"] + ku * cell, -(fr["v0"] + kv * cell)  # au = +y, av = -x
    assert abs(fr["au"][1] - 1.0) < 1e-12 and abs(fr["av"][0] + 1.0) < 1e-12
    yb, xb = float(F32(yb)), float(F32(xb))
    ends_u = np.array([(12.0, yb, -3.0), (16.0, yb, -2.0), (14.0, yb - 3.0, -2.5)])   # ends on the plane y = yb, lies on its low side
    ends_v = np.array([(xb, -14.0, -3.0), (xb, -10.0, -2.0), (xb + 3.0, -12.0, -2.5)])
    occ.append(ends_u), occ.append(ends_v)
    ortho_exact = []
    for name, tri, axis, b in (("ortho border in u", ends_u, 1, yb), ("ortho border in v", ends_v, 0, xb)):
        for f in (0.25, 0.5, 0.75):
            fid = pts.feature_id(f"{name} at {f}")
            base = tri[0] + f * (tri[1] - tri[0])
            Xs = []
            for d in DELTAS:
                x = base.copy()
                x[axis] = b + (d if tri[2][axis] < b else -d) * ORTHO_UNIT
                Xs.append(x)
            pts.add(1, sun, np.array(Xs), 2.0, fid, delta=np.array(DELTAS), role=len(occ) - (2 if axis == 1 else 1))
            ortho_exact.append((name, axis, b))
    # the grid's last cell and its outer edges: nothing projects there (the box ends two cells further in): lit throughout
    for name, axis, edge in (("ortho outer edge u = res", 1, fr["u0"] + res_ortho * cell), ("ortho outer edge u = 0", 1, fr["u0"]),
                             ("ortho outer edge v = res", 0, -(fr["v0"] + res_ortho * cell)), ("ortho outer edge v = 0", 0, -fr["v0"])):
        fid = pts.feature_id(name)
        Xs = []
        for d in DELTAS:
            x = np.array([6.3, 2.9, 2.0])
            x[axis] = edge + d * ORTHO_UNIT
            Xs.append(x)
        pts.add(1, sun, np.array(Xs), 0.0, fid, delta=np.array(DELTAS), role=-1)
    case = _case(f"seams and borders res {res_cube} {res_ortho}", np.asarray(np.array(occ), F32), lights, pts)
    case.tags.update(exact=exact, k_border=k_border, n_cube_occ=n_cube_occ, ortho_borders=dict(ku=ku, kv=kv, yb=yb, xb=xb), all_lit=[n for n in case.tags["features"] if "outer edge" in n],
                     all_occluded=[n for n in case.tags["features"] if n.endswith(" at 0.25") and not n.startswith("ortho") or n.endswith(" at 0.5") and not n.startswith("ortho")])
    # the builder's own assertion: in float64 the target directions fall exactly on their features
    for name, w in exact:
        face, ix, iy, fu, fv = cube_cell(w, res_cube)
        aw = np.sort(np.abs(w))
        if name.startswith("seam"):
            assert aw[2] == aw[1] and (fu[0] == res_cube or fv[0] == res_cube or fu[0] == 0 or fv[0] == 0), (name, w)
        elif name.startswith("corner"):
            assert aw[0] == aw[1] == aw[2]
        else:
            assert fu[0] == k_border or fv[0] == k_border, (name, w, fu, fv)
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases by name; a builder takes the resolutions of the cube maps and of the orthographic grids
ASSUMED_RES = {"coarse": (32, 64), "production": (1024, 2048)}
BUILDERS = {
    "silhouettes point": lambda rc, ro: silhouettes("point", rc),
    "silhouettes spot": lambda rc, ro: silhouettes("spot", rc),
    "silhouettes directional": lambda rc, ro: silhouettes("directional", ro),
    "seams and borders": lambda rc, ro: seams_and_borders(rc, ro),
    "near threshold": lambda rc, ro: near_threshold(rc),
    "depth ladder point": lambda rc, ro: depth_ladder("point"),
    "depth ladder spot": lambda rc, ro: depth_ladder("spot"),
    "depth ladder directional": lambda rc, ro: depth_ladder("directional"),
    "stacks point": lambda rc, ro: stacks("point", rc),
    "stacks spot": lambda rc, ro: stacks("spot", rc),
    "stacks directional": lambda rc, ro: stacks("directional", ro),
}
MAX_NOT_CLEAR = 0.5  # a condition on the cases, not a measurement: the ladder alone gives 5 rungs of 11


def aimed(case, ref, what):
    """ref[what] (n, L) at each point's own light -> (n,)."""
    return ref[what][np.arange(len(case.points)), case.tags["light"]]


def one_sided_features(case, ref):
    """Features that have one outcome by construction: ladders that cross a grid feature behind a straddling triangle or in the open
    (tags all_lit / all_occluded), and - under the spot light - features all of whose points the light's own cosine term leaves dark."""
    seg = aimed(case, ref, "segment")
    dark = {name for f, name in enumerate(case.tags["features"]) if not seg[case.tags["feature"] == f].any()}
    return set(case.tags.get("all_lit", [])) | set(case.tags.get("all_occluded", [])) | set(case.tags.get("never_clear", [])) | dark, dark
