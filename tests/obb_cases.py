"""The oriented-box statements (include/rt_hip.h "Oriented boxes", csrc/obb_rules.h) in numpy, and the queries the tests ask about.

What is new is the frame: frame() is the header's R from the quaternion, into() / back() its two products, each numpy operation one
f32 rounding in the header's order.  What happens IN the frame is overlap_cases.py and sweep_box_cases.py: the spheres go through
their sphere_touches / sphere_times / sphere_normals unchanged (centre o', box centre 0), the triangles through their span tests
(overlap_cases._span, sweep_box_cases._Span) and axis_normals.  The one thing written here a second time is the list of the thirteen
axes over RELATIVE vertices (the entry ov_triangle_rel / sb_triangle_rel of the rules headers: those modules subtract the centre
themselves and take one edge per record, where a turned box has one per pair); test_obb_abi.py holds it to theirs byte for byte at the
identity.  overlap_all() and brute_force() are the bytes rt_overlap_obb and rt_sweep_obb must return; times() is the sweep's time
alone in float32 or float64 (from the same f32 quaternion, with an offset on the half extents).  Helpers, no tests."""
import numpy as np

import closest_point_cases as cc
import overlap_cases as oc
import sweep_box_cases as sb
import sweep_cases as sc
from gpu_raytracer_amd import types as T

F32 = np.float32
F64 = np.float64
PRIM_MISS = cc.PRIM_MISS
SPHERE_FLAG = cc.SPHERE_FLAG
AXIS_NONE = sb.AXIS_NONE
AXIS_SPHERE = sb.AXIS_SPHERE
PAIRS_PER_CHUNK = 1 << 17

# The smallest k of sweep_box_cases' grid (1, 1.5, 2, 3, 5, 7 x 10^n) at which t64(h + k diag) <= t32 <= t64(h - k diag) holds, with
# its relative 1e-6 on finite t, for every one of five_kinds(scene, 4096, 11) whose extents are all >= 1e-3 x the diagonal (3586),
# measured on the CPU against the float64 statement, never against the kernel (test_obb_abi.py asserts the sandwich at twice this;
# DESIGN.md section 4 "Oriented boxes").  Soup: 22 outside at 1e-10, 4 at 2e-9, one from 1e-8 to 3e-7, none from 5e-7 - the
# axis-aligned statement's own figure.  cornell12: 49 outside at 1e-10, 13 at 1e-8, one from 5e-8 to 2e-6, none from 3e-6, where the
# axis-aligned statement is unviolated down to 0: its boxes meet the walls on box axes in two roundings, a turned box meets them
# through R, which is itself rounded.
K_MEASURED = {"soup": 5e-7, "cornell12": 3e-6}

_dot = cc._dot
_cross = sc._cross
_order = cc._order
records = cc.records
diagonal = cc.diagonal


# -- the frame ----------------------------------------------------------------------------------------------------------------------
def frame(q, dtype=F32):
    """q (m, 4) float32 quaternions x y z w -> R (m, 3, 3) in `dtype` (the f32 values, then every operation in dtype), valid (m,)."""
    q32 = np.ascontiguousarray(q, F32)
    q = q32.astype(dtype)
    ty = q.dtype.type
    with np.errstate(all="ignore"):
        x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        n = ((x * x + y * y) + z * z) + w * w
        s = ty(2) / n
        xs, ys, zs = x * s, y * s, z * s
        wx, wy, wz = w * xs, w * ys, w * zs
        xx, xy, xz, yy, yz, zz = x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
        one = ty(1)
        R = np.stack([np.stack([one - (yy + zz), xy - wz, xz + wy], -1), np.stack([xy + wz, one - (xx + zz), yz - wx], -1),
                      np.stack([xz - wy, yz + wx, one - (xx + yy)], -1)], 1)
        x32, y32, z32, w32 = (q32[:, k] for k in range(4))
        n32 = ((x32 * x32 + y32 * y32) + z32 * z32) + w32 * w32  # validity is the f32 statement's, whatever dtype R is in
        return R, np.isfinite(q32).all(1) & np.isfinite(n32) & (n32 > 0)


def _rows(R, u):
    return R.reshape((R.shape[0],) + (1,) * (u.ndim - 2) + (3, 3))


def into(R, u):
    """R (m, 3, 3), u (m or 1, ..., 3) -> u' (m, ..., 3): u'_j = (R_0j u_0 + R_1j u_1) + R_2j u_2."""
    Rb = _rows(R, u)
    with np.errstate(all="ignore"):
        return np.stack([(Rb[..., 0, j] * u[..., 0] + Rb[..., 1, j] * u[..., 1]) + Rb[..., 2, j] * u[..., 2] for j in range(3)], -1)


def back(R, u):
    """u_a = (R_a0 u'_0 + R_a1 u'_1) + R_a2 u'_2."""
    Rb = _rows(R, u)
    with np.errstate(all="ignore"):
        return np.stack([(Rb[..., a, 0] * u[..., 0] + Rb[..., a, 1] * u[..., 1]) + Rb[..., a, 2] * u[..., 2] for a in range(3)], -1)


def world_half(R, h):
    """The half extents of the turned box's world bounding box, without the walk's margin: (|R_a0| h_0 + |R_a1| h_1) + |R_a2| h_2."""
    A = np.abs(R)
    return np.stack([(A[:, a, 0] * h[:, 0] + A[:, a, 1] * h[:, 1]) + A[:, a, 2] * h[:, 2] for a in range(3)], -1)


def _in_frame(v0, e1, e2, c, R):
    """n records against m boxes -> a' (m, n, vertex, axis), e1', e2' (m, n, 3): rule 3 of the header."""
    with np.errstate(all="ignore"):
        cc_ = c[:, None, :]
        a = np.stack([v0[None] - cc_, (v0 + e1)[None] - cc_, (v0 + e2)[None] - cc_], 2)
        return into(R, a), into(R, np.broadcast_to(e1[None], a.shape[:2] + (3,))), into(R, np.broadcast_to(e2[None], a.shape[:2] + (3,)))


# -- the thirteen axes over relative vertices -----------------------------------------------------------------------------------------
def _cross_forms(f, a, h, d=None):
    """For an edge f (m, n, 3): the three axes cross(unit_i, f) as (p (m, n, 3 vertices), r (m, n), w (m, n) or None)."""
    g = np.abs(f)
    fx, fy, fz = f[..., None, 0], f[..., None, 1], f[..., None, 2]
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    hx, hy, hz = h[..., 0], h[..., 1], h[..., 2]
    w = [None] * 3
    if d is not None:
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        w = [f[..., 1] * dz - f[..., 2] * dy, f[..., 2] * dx - f[..., 0] * dz, f[..., 0] * dy - f[..., 1] * dx]
    return [(fy * az - fz * ay, g[..., 2] * hy + g[..., 1] * hz, w[0]), (fz * ax - fx * az, g[..., 2] * hx + g[..., 0] * hz, w[1]),
            (fx * ay - fy * ax, g[..., 1] * hx + g[..., 0] * hy, w[2])]


def rel_touches(a, e1, e2, h):
    """a (m, n, vertex, axis), e1, e2 (m, n, 3), h (m, 1, 3) -> (m, n) bool: ov_triangle_rel."""
    with np.errstate(all="ignore"):
        ok = (np.abs(a) <= np.finfo(a.dtype).max).all((2, 3))
        ok &= ((np.fmin(np.fmin(a[:, :, 0], a[:, :, 1]), a[:, :, 2]) <= h) & (np.fmax(np.fmax(a[:, :, 0], a[:, :, 1]), a[:, :, 2]) >= -h)).all(2)
        n = _cross(e1, e2)
        p, r = _dot(n, a[:, :, 0]), _dot(np.abs(n), h)
        ok &= (p <= r) & (p >= -r)
        for f in (e1, e2 - e1, e2):
            for p, r, _ in _cross_forms(f, a, h):
                ok &= oc._span(p, r)
        return ok


def rel_contacts(a, e1, e2, h, d):
    """As rel_touches, with d (m, 1, 3) -> t (m, n) (inf: no contact), axis (m, n) uint32, w_in (m, n): sb_triangle_rel, every axis
    evaluated."""
    ty = a.dtype.type
    with np.errstate(all="ignore"):
        s = sb._Span(a.shape[:2], a.dtype)
        s.ok &= (np.abs(a) <= np.finfo(a.dtype).max).all((2, 3))
        for ax in range(3):
            s.add3(ax, a[..., ax], h[..., ax], d[..., ax])
        n = _cross(e1, e2)
        p = _dot(n, a[:, :, 0])
        s.add(3, p, p, _dot(np.abs(n), h), _dot(n, d))
        for j, f in enumerate((e1, e2 - e1, e2)):
            for i, (p, r, w) in enumerate(_cross_forms(f, a, h, d)):
                s.add3(4 + 3 * j + i, p, r, w)
        contact = s.ok & (s.t_in <= s.t_out)
        return np.where(contact, s.t_in + ty(0), ty(np.inf)).astype(a.dtype), s.axis, s.w_in


# -- the overlap ----------------------------------------------------------------------------------------------------------------------
def make_obbs(center, half_extent, rotation):
    """(N, 12) float32 rt_obb records: cx cy cz 0 hx hy hz 0 qx qy qz qw."""
    out = np.zeros((len(np.asarray(center).reshape(-1, 3)), 12), F32)
    out[:, 0:8] = oc.make_boxes(center, half_extent)
    out[:, 8:12] = np.asarray(rotation, F32)
    return out


def valid_boxes(boxes):
    return oc.valid(boxes) & frame(boxes[:, 8:12])[1]


def _spheres(scene, dtype=F32):
    sph = scene.spheres
    return np.ascontiguousarray(sph["center"], F32).reshape(-1, 3).astype(dtype), sph["radius"].astype(F32).astype(dtype)


def touching(scene, boxes, prefilter=False):
    """(N, 12) float32 boxes -> (N, n_spheres + n_triangles) bool in key order, as overlap_cases.touching.  prefilter (for scenes of
    10^5 triangles): a triangle whose centroid is farther from the box's centre than the centroid's reach + the box's half diagonal +
    1e-3 x the scene's diagonal cannot touch, so the statement is evaluated on the others only (test_obb_abi.py holds the filtered
    result to the unfiltered one)."""
    boxes = np.ascontiguousarray(boxes, F32)
    all_v0, all_e1, all_e2, _ = records(scene)
    centre, radius = _spheres(scene)
    n, cols = len(boxes), len(centre) + len(all_v0)
    out = np.zeros((n, cols), bool)
    ok = valid_boxes(boxes)
    zero = np.zeros((1, 3), F32)
    step = max(1, PAIRS_PER_CHUNK // max(len(all_v0), 1))
    if prefilter and len(all_v0):
        centroid, reach = sc._reach(all_v0, all_e1, all_e2)
        margin, step = 1e-3 * diagonal(scene), 4
    with np.errstate(all="ignore"):
        for lo in range(0, n, step):
            c, h = boxes[lo:lo + step, 0:3], boxes[lo:lo + step, 4:7]
            R = frame(boxes[lo:lo + step, 8:12])[0]
            for k in range(len(centre)):  # a sphere at a time: its centre in the frame is one per box
                o = into(R, centre[k][None] - c)
                out[lo:lo + step, k] = oc.sphere_touches(zero, radius[k:k + 1], -o, h)[:, 0]
            prim = np.arange(len(all_v0))
            if prefilter and len(all_v0):
                live = ok[lo:lo + step]
                far = np.sqrt(((centroid[None] - c[live][:, None, :]).astype(F64) ** 2).sum(-1))
                prim = np.flatnonzero((far <= reach[None] + np.sqrt((h[live].astype(F64) ** 2).sum(1))[:, None] + margin).any(0))
            if len(prim):
                a, f1, f2 = _in_frame(all_v0[prim], all_e1[prim], all_e2[prim], c, R)
                out[lo:lo + step, len(centre) + prim] = rel_touches(a, f1, f2, h[:, None, :])
    return out & ok[:, None]


def overlap_all(scene, boxes, k=oc.OVERLAP_MAX, touch=None):
    """-> ids (N, k), listed counts (N,), total counts (N,), as overlap_cases.overlap_all."""
    return oc.overlap_all(scene, boxes, k, touching(scene, boxes) if touch is None else touch)


# -- the sweep ------------------------------------------------------------------------------------------------------------------------
def make_obb_sweeps(center, half_extent, rotation, direction, tmax=np.inf):
    """(N, 16) float32 rt_obb_sweep records: cx cy cz 0 hx hy hz 0 qx qy qz qw dx dy dz tmax."""
    out = np.zeros((len(np.asarray(center).reshape(-1, 3)), 16), F32)
    out[:, 0:12] = make_obbs(center, half_extent, rotation)
    out[:, 12:15], out[:, 15] = np.asarray(direction, F32), tmax
    return out


def as_box_sweeps(sweeps):
    """The (N, 12) rt_box_sweep records of (N, 16) rt_obb_sweep records: the rotation left out."""
    return np.ascontiguousarray(np.concatenate([sweeps[:, 0:8], sweeps[:, 12:16]], 1), F32)


def with_rotation(box_sweeps, rotation):
    """(N, 12) rt_box_sweep records -> (N, 16) rt_obb_sweep records."""
    out = np.zeros((len(box_sweeps), 16), F32)
    out[:, 0:8], out[:, 8:12], out[:, 12:16] = box_sweeps[:, 0:8], np.asarray(rotation, F32), box_sweeps[:, 8:12]
    return out


def valid(sweeps):
    return sb.valid(as_box_sweeps(sweeps)) & frame(sweeps[:, 8:12])[1]


def _sphere_times(centre, radius, c, h, dl, R):
    """-> t (m, s), o' (m, s, 3)."""
    zero = np.zeros((1, 3), c.dtype)
    o = np.stack([into(R, centre[k][None] - c) for k in range(len(centre))], 1)
    t = np.stack([sb.sphere_times(zero, radius[k:k + 1], -o[:, k], h, dl)[:, 0] for k in range(len(centre))], 1)
    return t, o


def brute_force(scene, sweeps, prefilter=False):
    """(N, 16) float32 sweeps -> (N, 8) float32 rt_box_sweep_hit records: the bytes rt_sweep_obb returns.  prefilter: as
    sweep_box_cases.brute_force, with the box's half diagonal, which no rotation changes."""
    sweeps = np.ascontiguousarray(sweeps, F32)
    n = len(sweeps)
    out = np.zeros(n, T.BOX_SWEEP_HIT)
    c, h, q, d, tmax = sweeps[:, 0:3], sweeps[:, 4:7], sweeps[:, 8:12], sweeps[:, 12:15], sweeps[:, 15]
    start = _order(tmax, np.zeros(n, np.uint32))
    ok = valid(sweeps)
    all_v0, all_e1, all_e2, all_mat = records(scene)
    all_prim = np.arange(len(all_v0), dtype=np.uint32)
    if prefilter and len(all_v0):
        centroid, reach = sc._reach(all_v0, all_e1, all_e2)
        margin = 1e-3 * diagonal(scene)
    s_c, s_r = _spheres(scene)
    s_mat = scene.spheres["material_id"]
    step = max(1, PAIRS_PER_CHUNK // max(len(all_v0), 1))
    if prefilter:
        step = min(step, 4)
    zero3 = np.zeros((1, 3), F32)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        rows = np.arange(hi - lo)
        qc, qh, qd = c[lo:hi], h[lo:hi], d[lo:hi]
        R = frame(q[lo:hi])[0]
        best = start[lo:hi].copy()
        rec = out[lo:hi]
        found = np.zeros(hi - lo, bool)
        normal = np.zeros((hi - lo, 3), F32)
        with np.errstate(all="ignore"):
            dl = into(R, qd)
            if len(s_c):
                t, o = _sphere_times(s_c, s_r, qc, qh, dl, R)
                order = _order(t, np.broadcast_to(np.arange(len(s_c), dtype=np.uint32), t.shape))
                k = order.argmin(1)
                win = order[rows, k] < best
                best = np.where(win, order[rows, k], best)
                found |= win
                tk = t[rows, k]
                moving = win & (tk > 0)
                normal[win] = 0
                normal[moving] = sb.sphere_normals(o[rows, k], s_r[k], np.broadcast_to(zero3, qc.shape), qh, dl, tk)[moving]
                rec["t"][win] = tk[win]
                rec["axis"][win] = np.where(tk > 0, AXIS_SPHERE, AXIS_NONE).astype(np.uint32)[win]
                rec["prim_id"][win] = (k[win] | SPHERE_FLAG).astype(np.uint32)
                rec["material_id"][win] = s_mat[k][win]
            prim = all_prim
            if prefilter and len(all_v0):
                live = ok[lo:hi]
                half_diagonal = np.sqrt((qh[live].astype(F64) ** 2).sum(1)).astype(F32)
                prim = sc._near_the_path(centroid, reach, qc[live], qd[live], half_diagonal, margin) if live.any() else all_prim[:0]
            if len(prim):
                v0, e1, e2, mat = all_v0[prim], all_e1[prim], all_e2[prim], all_mat[prim]
                a, f1, f2 = _in_frame(v0, e1, e2, qc, R)
                t, axis, w_in = rel_contacts(a, f1, f2, qh[:, None, :], dl[:, None, :])
                order = _order(t, np.broadcast_to(prim.astype(np.uint64) | np.uint64(SPHERE_FLAG), t.shape))
                k = order.argmin(1)
                win = order[rows, k] < best
                found |= win
                normal[win] = sb.axis_normals(f1[rows, k], f2[rows, k], axis[rows, k], w_in[rows, k])[win]
                rec["t"][win] = t[rows, k][win]
                rec["axis"][win] = axis[rows, k][win]
                rec["prim_id"][win] = prim[k][win]
                rec["material_id"][win] = mat[k][win]
            rec["normal"] = back(R, normal) + F32(0)
        miss = ~(found & ok[lo:hi])
        blank = np.zeros(int(miss.sum()), T.BOX_SWEEP_HIT)
        blank["t"] = tmax[lo:hi][miss]
        blank["axis"] = AXIS_NONE
        blank["prim_id"] = PRIM_MISS
        rec[miss] = blank
    return out.view(F32).reshape(n, 8)


def triangle_times_all(scene, sweeps, dtype=F32):
    """(N, n_triangles): the statement's time of every sweep with every triangle, inf where they do not touch (small scenes)."""
    v0, e1, e2, _ = records(scene, dtype)
    s = np.ascontiguousarray(sweeps, F32)
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    parts = []
    for lo in range(0, len(s), step):
        p = s[lo:lo + step].astype(dtype)
        R = frame(s[lo:lo + step, 8:12], dtype)[0]
        a, f1, f2 = _in_frame(v0, e1, e2, np.ascontiguousarray(p[:, 0:3]), R)
        parts.append(rel_contacts(a, f1, f2, p[:, None, 4:7], into(R, np.ascontiguousarray(p[:, 12:15]))[:, None, :])[0])
    return np.concatenate(parts)


def times(scene, sweeps, dtype, eps=0.0):
    """The time of first contact of each sweep by the statement in `dtype` (float32: on the stored f32 edges; float64: on the exact
    ones, R in float64 from the f32 quaternion), with half extents + eps on every axis and tmax = inf; inf for a miss."""
    v0, e1, e2, _ = records(scene, dtype)
    s32 = np.ascontiguousarray(sweeps, F32)
    s = s32.astype(dtype)
    s_c, s_r = _spheres(scene, dtype)
    out = np.full(len(s), np.inf, dtype)
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    with np.errstate(all="ignore"):
        for lo in range(0, len(s), step):
            sl = slice(lo, lo + step)
            c, h, d = np.ascontiguousarray(s[sl, 0:3]), s[sl, 4:7] + dtype(eps), np.ascontiguousarray(s[sl, 12:15])
            R = frame(s32[sl, 8:12], dtype)[0]
            dl = into(R, d)
            t = np.full((len(c), 1), np.inf, dtype)
            if len(v0):
                a, f1, f2 = _in_frame(v0, e1, e2, c, R)
                t = rel_contacts(a, f1, f2, h[:, None, :], dl[:, None, :])[0]
            if len(s_c):
                t = np.concatenate([t, _sphere_times(s_c, s_r, c, h, dl, R)[0]], 1)
            out[sl] = np.where(np.isnan(t), np.inf, t).min(1)
    return out


# -- the queries ----------------------------------------------------------------------------------------------------------------------
IDENTITY = (0.0, 0.0, 0.0, 1.0)
QUARTER_Z = (0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5))


def rotations(n, seed, identity_share=0.125, near_share=0.125):
    """(n, 4) float32 quaternions: uniform over the rotations (a normalised 4-d normal vector) times a length in 0.5 .. 2 (they need
    not be normalised); the first `identity_share` of every run of 16 exactly (0, 0, 0, 1), the next `near_share` within 1e-3 rad
    of it."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= rng.uniform(0.5, 2.0, (n, 1))
    k = np.arange(n) % 16
    near = (k >= 16 * identity_share) & (k < 16 * (identity_share + near_share))
    half_angle = rng.uniform(0.0, 0.5e-3, n)
    axis = sc._unit(rng, n)
    q[near] = np.concatenate([axis * np.sin(half_angle)[:, None], np.cos(half_angle)[:, None]], 1)[near]
    q[k < 16 * identity_share] = IDENTITY
    return q.astype(F32)


def five_kinds(scene, n, seed):
    """sweep_box_cases.five_kinds with rotations(): (n, 16) rt_obb_sweep records."""
    return with_rotation(sb.five_kinds(scene, n, seed), rotations(n, seed + 100))


def sphere_directed(scene, n, seed):
    """At the scene's sphere primitives, with boxes small against the sphere: a third from 1.3 to 2 radii off the centre aimed at
    points within 0.8 radii of it, a third from within 0.4 radii of the centre outward, a third starting at 0.9 to 1.1 radii, across
    the surface or a little off it."""
    rng = np.random.default_rng(seed)
    s_c, s_r = _spheres(scene, F64)
    k = (np.arange(n) // 3) % len(s_c)
    kind = np.arange(n) % 3
    inside = kind != 0
    off = np.where(kind == 0, rng.uniform(1.3, 2.0, n), np.where(kind == 1, rng.uniform(0.0, 0.4, n), rng.uniform(0.9, 1.1, n)))
    origin = s_c[k] + sc._unit(rng, n) * (s_r[k] * off)[:, None]
    target = np.where(inside[:, None], origin + sc._unit(rng, n), s_c[k] + sc._unit(rng, n) * (s_r[k] * rng.uniform(0.0, 0.8, n))[:, None])
    to = target - origin
    d = to / np.linalg.norm(to, axis=1, keepdims=True) * rng.uniform(0.2, 5.0, (n, 1))
    h = s_r[k][:, None] * rng.uniform(0.02, 0.2, (n, 3))
    return with_rotation(sb._pack(origin, h, d), rotations(n, seed + 100))


def full_extents(scene, sweeps):
    return sb.full_extents(scene, sweeps)
