"""The triangle sweep's statement (include/rt_hip.h "Triangle sweeps", csrc/sweep_triangle_rules.h) in numpy, and the sweeps the tests
ask about.

brute_force() evaluates the statement for every sweep against every triangle and sphere of a scene, in float32 - every numpy
operation is one f32 rounding, in the header's order, so its records are the bytes rt_sweep_triangle must return.  The coordinate axes
are evaluated on all pairs and the 23 others on the pairs they leave only: the statement's first early return, which changes no
answer.  times() gives the time of first contact alone, in float32 or in float64 (the same statement on the exact edges, every span
widened by eps), which the float32 statement is held to; clearance() is the static 26-axis test in float64 as a signed gap, which the
float64 statement is held to along the path; feature_times() is an independent float64 computation from vertex rays and edge pairs.
Helpers, no tests."""
import numpy as np

import closest_point_all_cases as ca
import closest_point_cases as cc
import overlap_triangle_cases as tc
import sweep_box_cases as bc
import sweep_cases as sc
from gpu_raytracer_amd import types as T

F32 = np.float32
F64 = np.float64
PRIM_MISS = cc.PRIM_MISS
SPHERE_FLAG = cc.SPHERE_FLAG
AXIS_NONE = 0xFFFFFFFF
AXIS_SPHERE = 26
PAIRS_PER_CHUNK = 1 << 19  # sweep x triangle pairs whose coordinate axes are evaluated at a time

# The smallest k of the grid 1, 1.5, 2, 3, 5, 7 x 10^n at which t64(+k diag) <= t32 <= t64(-k diag), with a relative 1e-6 on finite
# times, holds for every sweep of fixtures(scene) (test_sweep_triangle_abi.py asserts the sandwich at twice this and prints the
# violations on either side; DESIGN.md section 4 "Triangle sweeps").  measure_k() below is the bisection over the grid that found
# them: soup 5e-8 (38 of 3840 sweeps violate eps = 0, 1 still 3e-8), cornell12 3e-9 (20 of 1630 at 0, 1 at 2e-9); on the plane scene, whose coordinates are exact, no
# value of the grid is violated down to eps = 0, and 1e-12 is the smallest value tried.
K_MEASURED = {"soup": 5e-8, "cornell12": 3e-9, "plane": 1e-12}

_dot = cc._dot
_cross = tc._cross
_order = cc._order
records = cc.records
diagonal = cc.diagonal


def make_sweeps(v0, v1, v2, direction, tmax=np.inf):
    """(N, 16) float32 rt_triangle_sweep records: v0 0 v1 0 v2 0 direction tmax."""
    t = tc.make_triangles(v0, v1, v2)
    out = np.zeros((len(t), 16), F32)
    out[:, 0:12], out[:, 12:15], out[:, 15] = t, np.asarray(direction, F32).reshape(-1, 3), tmax
    return out


def vertices(sweeps):
    return sweeps[:, 0:3], sweeps[:, 4:7], sweeps[:, 8:11]


def valid(sweeps):
    """The sweeps that walk: finite vertices and direction, a direction that is not zero, tmax > 0."""
    s = np.asarray(sweeps)
    with np.errstate(all="ignore"):
        return (np.isfinite(s[:, 0:3]).all(1) & np.isfinite(s[:, 4:7]).all(1) & np.isfinite(s[:, 8:11]).all(1) & np.isfinite(s[:, 12:15]).all(1)
                & (s[:, 12:15] != 0).any(1) & (s[:, 15] > 0))


# -- the statement ------------------------------------------------------------------------------------------------------------------
class _Span:
    """The running entry and exit of sweep x record pairs over the axes: st_axis."""

    def __init__(self, shape, dtype):
        self.t_in = np.zeros(shape, dtype)
        self.t_out = np.full(shape, np.inf, dtype)
        self.w_in = np.zeros(shape, dtype)
        self.axis = np.full(shape, AXIS_NONE, np.uint32)
        self.ok = np.ones(shape, bool)

    def add(self, axis, lo, hi, w):
        pos, neg = w > 0, w < 0
        moving = pos | neg
        enter, leave = np.where(pos, lo, hi) / w, np.where(pos, hi, lo) / w
        self.ok &= np.where(moving, enter <= leave, (w == 0) & (lo <= 0) & (hi >= 0))
        replace = np.broadcast_to(moving & (enter > self.t_in), self.t_in.shape)
        self.t_in = np.where(replace, enter, self.t_in)
        self.w_in = np.where(replace, w, self.w_in)
        self.axis = np.where(replace, np.uint32(axis), self.axis)
        self.t_out = np.where(moving, np.fmin(self.t_out, leave), self.t_out)

    def take(self, rows, cols):
        sub = _Span(len(rows), self.t_in.dtype)
        sub.t_in, sub.t_out, sub.w_in, sub.axis, sub.ok = (x[rows, cols] for x in (self.t_in, self.t_out, self.w_in, self.axis, self.ok))
        return sub

    def time(self):
        ty = self.t_in.dtype.type
        return np.where(self.ok & (self.t_in <= self.t_out), self.t_in + ty(0), ty(np.inf)).astype(self.t_in.dtype)


def triangle_contacts(v0, e1, e2, q0, q1, q2, d, eps=0.0):
    """Sweeps q0, q1, q2, d (m, 3) against n records -> t (m, n) in the arrays' dtype (inf: no contact), axis (m, n) uint32, w_in
    (m, n): the header's statement.  eps widens every span: by eps on a coordinate axis, by eps |L| on the others."""
    ty = q0.dtype.type
    with np.errstate(all="ignore"):
        s = (v0, v0 + e1, v0 + e2)
        smin, smax = np.fmin(np.fmin(s[0], s[1]), s[2]), np.fmax(np.fmax(s[0], s[1]), s[2])
        qlo, qhi = np.fmin(np.fmin(q0, q1), q2), np.fmax(np.fmax(q0, q1), q2)
        span = _Span((len(q0), len(v0)), q0.dtype)
        span.ok &= (np.abs(np.stack(s)) <= np.finfo(q0.dtype).max).all((0, 2))[None]
        for a in range(3):
            lo, hi = smin[None, :, a] - qhi[:, None, a], smax[None, :, a] - qlo[:, None, a]
            if eps:
                lo, hi = lo - ty(eps), hi + ty(eps)
            span.add(a, lo, hi, np.broadcast_to(d[:, None, a], lo.shape))
        t = np.full(span.ok.shape, np.inf, q0.dtype)
        rows, cols = np.nonzero(span.ok & (span.t_in <= span.t_out))  # the first early return
        sub = span.take(rows, cols)
        p0, dd = q0[rows], d[rows]
        u1, u2 = q1[rows] - p0, q2[rows] - p0
        a_k = [sk[cols] - p0 for sk in s]
        for k, L in enumerate(tc.axes(u1, u2, e1[cols], e2[cols])):
            smin_, smax_, qmin, qmax, total = tc._project(L, a_k, u1, u2)
            sub.ok &= total == total
            lo, hi = smin_ - qmax, smax_ - qmin
            if eps:
                length = np.sqrt(_dot(L, L))
                lo, hi = lo - ty(eps) * length, hi + ty(eps) * length
            sub.add(3 + k, lo, hi, _dot(L, dd))
        t[rows, cols] = sub.time()
        span.axis[rows, cols], span.w_in[rows, cols] = sub.axis, sub.w_in
        return t, span.axis, span.w_in


def axis_normals(e1, e2, q0, q1, q2, axis, w_in):
    """Elementwise: records (k, 3), queries (k, 3), axis (k,), w_in (k,) -> normal (k, 3): st_axis_normal."""
    ty = e1.dtype.type
    with np.errstate(all="ignore"):
        unit = np.eye(3, dtype=e1.dtype)
        every = np.stack([np.broadcast_to(unit[a], e1.shape) for a in range(3)] + tc.axes(q1 - q0, q2 - q0, e1, e2))  # (26, k, 3)
        L = every[np.minimum(axis, 25).astype(np.int64), np.arange(len(axis))]
        length = np.sqrt(_dot(L, L))
        normal = np.where((w_in > 0)[:, None], -L, L) / length[:, None] + ty(0)
        ok = (axis < 26) & (length > 0) & (length < np.inf)
        return np.where(ok[:, None], normal, ty(0)).astype(e1.dtype)


def _closest_elementwise(q0, u1, u2, p):
    """cp_triangle of triangle i at point i -> dist2, v, w, each (k,)."""
    d2, v, w = (np.zeros(len(p), p.dtype) for _ in range(3))
    for lo in range(0, len(p), 64):
        sl = slice(lo, lo + 64)
        dd, vv, ww = cc.triangle_candidates(q0[sl], u1[sl], u2[sl], p[sl])
        d2[sl], v[sl], w[sl] = np.diagonal(dd), np.diagonal(vv), np.diagonal(ww)
    return d2, v, w


def _ball_on_triangles(q0, u1, u2, centre, radius, back):
    """sw_triangle of the ball (centre, radius), one per row, moving by back[i] against triangle i -> t (k,)."""
    t = np.zeros(len(q0), q0.dtype)
    for lo in range(0, len(q0), 64):
        sl = slice(lo, lo + 64)
        t[sl] = np.diagonal(sc.triangle_times(q0[sl], u1[sl], u2[sl], centre[sl], back[sl], radius[sl]))
    return t


def sphere_times(centre, radius, q0, q1, q2, d, eps=0.0):
    """Sweeps (m, 3) against s spheres -> t (m, s).  eps (float64 only): met from outside the ball has radius R + eps, from inside
    R - eps, and the start is in contact where near <= R + eps and far >= R - eps."""
    ty = q0.dtype.type
    m, out = len(q0), []
    with np.errstate(all="ignore"):
        u1, u2 = q1 - q0, q2 - q0
        ddq = _dot(d, d)
        for k in range(len(centre)):
            o = np.broadcast_to(centre[k], q0.shape)
            r_out, r_in = np.full(m, radius[k] + ty(eps), q0.dtype), np.full(m, radius[k] - ty(eps), q0.dtype)
            near2 = _closest_elementwise(q0, u1, u2, np.ascontiguousarray(o))[0]
            ms = [o - q for q in (q0, q1, q2)]
            far2 = np.fmax(np.fmax(_dot(ms[0], ms[0]), _dot(ms[1], ms[1])), _dot(ms[2], ms[2]))
            rr_out, rr_in = r_out * r_out, r_in * r_in
            start = (near2 <= rr_out) & (far2 >= rr_in)
            outside = near2 > rr_out
            inside = ~outside & (far2 < rr_in)
            t_outside = _ball_on_triangles(q0, u1, u2, np.ascontiguousarray(o), r_out, -d)
            best = np.full(m, np.inf, q0.dtype)
            for mk in ms:
                x = _cross(mk, d)
                disc = ddq * rr_in - _dot(x, x)
                t = (_dot(mk, d) + np.sqrt(disc)) / ddq
                best = np.where((disc >= 0) & (t >= 0) & (t < best), t, best)
            t = np.where(outside, t_outside, np.where(inside, best + ty(0), ty(np.inf)))
            out.append(np.where(start, ty(0), t).astype(q0.dtype))
    return np.stack(out, 1) if out else np.zeros((m, 0), q0.dtype)


def sphere_normals(centre, radius, q0, q1, q2, d, t):
    """Elementwise, all (k, ...): st_sphere_normal."""
    ty = q0.dtype.type
    with np.errstate(all="ignore"):
        u1, u2 = q1 - q0, q2 - q0
        P = centre - d * t[:, None]
        outside = _closest_elementwise(q0, u1, u2, np.ascontiguousarray(centre))[0] > radius * radius
        _, v, w = _closest_elementwise(q0, u1, u2, np.ascontiguousarray(P))
        out_v = (u1 * v[:, None] + u2 * w[:, None]) - (P - q0)
        g = np.stack([q - P for q in (q0, q1, q2)])  # (3, k, 3)
        far = np.argmax(_dot(g, g), 0)                # the first of equal maxima: the lowest k
        qs = np.stack([q0, q1, q2])
        in_v = P - qs[far, np.arange(len(far))]
        n = np.where(outside[:, None], out_v, in_v)
        length = np.sqrt(_dot(n, n))
        return np.where((length > 0)[:, None], n / length[:, None], ty(0)).astype(q0.dtype)


def _bound_box(q0, q1, q2):
    """The box the walk culls by -> centre, half diagonal (float32)."""
    lo, hi = np.fmin(np.fmin(q0, q1), q2), np.fmax(np.fmax(q0, q1), q2)
    c = lo * F32(0.5) + hi * F32(0.5)
    h = np.fmax(hi - c, c - lo)
    return c, np.sqrt((h.astype(F64) ** 2).sum(1)).astype(F32)


def brute_force(scene, sweeps, prefilter=False):
    """(N, 16) float32 sweeps -> (N, 8) float32 rt_triangle_sweep_hit records: the bytes rt_sweep_triangle returns.  prefilter (for
    scenes of 10^5 triangles): a triangle whose centroid is farther from the half-line of the bound's centre than the centroid's
    reach + the bound's half diagonal + 1e-3 x the scene's diagonal cannot be touched, so the statement is evaluated on the others
    only.  test_sweep_triangle_abi.py holds the filtered result to the unfiltered one."""
    sweeps = np.ascontiguousarray(sweeps, F32)
    n = len(sweeps)
    out = np.zeros(n, T.TRIANGLE_SWEEP_HIT)
    (q0, q1, q2), d, tmax = vertices(sweeps), sweeps[:, 12:15], sweeps[:, 15]
    start = _order(tmax, np.zeros(n, np.uint32))
    ok = valid(sweeps)
    all_v0, all_e1, all_e2, all_mat = records(scene)
    all_prim = np.arange(len(all_v0), dtype=np.uint32)
    if prefilter and len(all_v0):
        centroid, reach = sc._reach(all_v0, all_e1, all_e2)
        margin = 1e-3 * diagonal(scene)
    sph = scene.spheres
    step = max(1, PAIRS_PER_CHUNK // max(len(all_v0), 1))
    if prefilter:
        step = min(step, 4)  # few sweeps at a time, so that the union of what they can touch stays small
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        rows = np.arange(hi - lo)
        p0, p1, p2, qd = q0[lo:hi], q1[lo:hi], q2[lo:hi], d[lo:hi]
        best = start[lo:hi].copy()
        rec = out[lo:hi]
        found = np.zeros(hi - lo, bool)
        with np.errstate(all="ignore"):
            if len(sph):
                s_c, s_r = np.ascontiguousarray(sph["center"], F32).reshape(-1, 3), sph["radius"].astype(F32)
                t = sphere_times(s_c, s_r, p0, p1, p2, qd)
                order = _order(t, np.broadcast_to(np.arange(len(sph), dtype=np.uint32), t.shape))
                k = order.argmin(1)
                win = order[rows, k] < best
                best = np.where(win, order[rows, k], best)
                found |= win
                tk = t[rows, k]
                moving = win & (tk > 0)
                rec["normal"][win] = 0
                if moving.any():
                    rec["normal"][moving] = sphere_normals(s_c[k], s_r[k], p0, p1, p2, qd, tk)[moving]
                rec["t"][win] = tk[win]
                rec["axis"][win] = np.where(tk > 0, AXIS_SPHERE, AXIS_NONE).astype(np.uint32)[win]
                rec["prim_id"][win] = (k[win] | SPHERE_FLAG).astype(np.uint32)
                rec["material_id"][win] = sph["material_id"][k][win]
            prim = all_prim
            if prefilter and len(all_v0):
                live = ok[lo:hi]
                c, half_diagonal = _bound_box(p0[live], p1[live], p2[live])
                prim = sc._near_the_path(centroid, reach, c, qd[live], half_diagonal, margin) if live.any() else all_prim[:0]
            if len(prim):
                v0, e1, e2, mat = all_v0[prim], all_e1[prim], all_e2[prim], all_mat[prim]
                t, axis, w_in = triangle_contacts(v0, e1, e2, p0, p1, p2, qd)
                order = _order(t, np.broadcast_to(prim.astype(np.uint64) | np.uint64(SPHERE_FLAG), t.shape))
                k = order.argmin(1)  # the lowest (t bits, key): at equal t the lower index
                win = order[rows, k] < best
                found |= win
                rec["normal"][win] = axis_normals(e1[k], e2[k], p0, p1, p2, axis[rows, k], w_in[rows, k])[win]
                rec["t"][win] = t[rows, k][win]
                rec["axis"][win] = axis[rows, k][win]
                rec["prim_id"][win] = prim[k][win]
                rec["material_id"][win] = mat[k][win]
        miss = ~(found & ok[lo:hi])
        blank = np.zeros(int(miss.sum()), T.TRIANGLE_SWEEP_HIT)
        blank["t"] = tmax[lo:hi][miss]
        blank["axis"] = AXIS_NONE
        blank["prim_id"] = PRIM_MISS
        rec[miss] = blank
    return out.view(F32).reshape(n, 8)


def _scene_spheres(scene, dtype):
    sph = scene.spheres
    return np.ascontiguousarray(sph["center"], F32).reshape(-1, 3).astype(dtype), sph["radius"].astype(F32).astype(dtype)


def _parts(sweeps, dtype):
    s = np.ascontiguousarray(sweeps, F32).astype(dtype)
    return [np.ascontiguousarray(s[:, k:k + 3]) for k in (0, 4, 8, 12)]


def triangle_times_all(scene, sweeps, dtype=F32, eps=0.0):
    """(N, n_triangles): the statement's time of every sweep with every triangle, inf where they do not touch."""
    v0, e1, e2, _ = records(scene, dtype)
    q0, q1, q2, d = _parts(sweeps, dtype)
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    return np.concatenate([triangle_contacts(v0, e1, e2, q0[lo:lo + step], q1[lo:lo + step], q2[lo:lo + step], d[lo:lo + step], eps)[0]
                           for lo in range(0, len(q0), step)])


def times(scene, sweeps, dtype, eps=0.0):
    """The time of first contact of each sweep by the statement in `dtype` (float32: on the stored f32 edges; float64: on the exact
    ones), every span widened by eps and tmax = inf; inf for a miss."""
    q0, q1, q2, d = _parts(sweeps, dtype)
    out = np.full(len(q0), np.inf, dtype)
    if len(scene.triangles):
        t = triangle_times_all(scene, sweeps, dtype, eps)
        out = np.where(np.isnan(t), np.inf, t).min(1)
    s_c, s_r = _scene_spheres(scene, dtype)
    if len(s_c):
        t = sphere_times(s_c, s_r, q0, q1, q2, d, eps)
        out = np.minimum(out, np.where(np.isnan(t), np.inf, t).min(1))
    return out


def clearance(scene, q0, q1, q2, near=None):
    """The static test in float64 as a distance, for float64 query vertices (N, 3) each: the smallest over the scene's primitives of
    overlap_triangle_cases' gap - the largest over the 26 axes with |L| > 0 of the separation on that axis over |L|; a sphere:
    max(|near| - R, R - |far|).  > 0: the triangle is clear of everything by at least that on some axis; <= 0: it touches something.
    The 23 axes are evaluated where the coordinate axes' gap is <= near (default a thousandth of the diagonal); elsewhere that gap,
    a lower bound, stands."""
    q0, q1, q2 = (np.asarray(q, F64) for q in (q0, q1, q2))
    near = 1e-3 * diagonal(scene) if near is None else near
    out = np.full(len(q0), np.inf)
    centre, radius = _scene_spheres(scene, F64)
    _, _, _, s = tc._records(scene, F64)
    with np.errstate(all="ignore"):
        if len(centre):
            near2, far2, _ = tc._sphere_terms(centre, radius, q0, q1, q2)
            gap = np.maximum(np.sqrt(near2) - radius[None], radius[None] - np.sqrt(far2))
            out = np.minimum(out, np.where(np.isnan(gap), np.inf, gap).min(1))  # a NaN near2 (a segment's 0 / 0) touches nothing, as in the statement
        if len(s[0]):
            qlo, qhi = np.minimum(np.minimum(q0, q1), q2), np.maximum(np.maximum(q0, q1), q2)
            smin, smax = np.minimum(np.minimum(s[0], s[1]), s[2]), np.maximum(np.maximum(s[0], s[1]), s[2])
            step = max(1, PAIRS_PER_CHUNK // len(smin))
            for lo in range(0, len(q0), step):
                sl = slice(lo, lo + step)
                cg = np.full((len(q0[sl]), len(smin)), -np.inf)
                for ax in range(3):
                    cg = np.maximum(cg, np.maximum(smin[None, :, ax] - qhi[sl, None, ax], qlo[sl, None, ax] - smax[None, :, ax]))
                rows, cols = np.nonzero(cg <= near)
                _, gap = tc._pairs(s, q0[sl], q1[sl], q2[sl], rows, cols, True)
                cg[rows, cols] = np.maximum(cg[rows, cols], gap)
                out[sl] = np.minimum(out[sl], cg.min(1))
    return out


def feature_times(v0, e1, e2, q0, q1, q2, d):
    """The independent computation, elementwise in float64 on pair i: the earliest t >= 0 of three query-vertex rays (along d)
    against the scene's triangle, three scene-vertex rays (along -d) against the query's, and nine moving-edge-against-edge solves.
    -> t (k,) (inf: none) and singular (k,): some 3 x 3 system of the pair has |det| <= 1e-12 x the product of its columns' lengths."""
    s = [v0, v0 + e1, v0 + e2]
    q = [q0, q1, q2]
    best = np.full(len(v0), np.inf)
    singular = np.zeros(len(v0), bool)

    def solve(c0, c1, c2, rhs):
        """x with c0 x0 + c1 x1 + c2 x2 = rhs, by Cramer's rule."""
        det = (c0 * np.cross(c1, c2)).sum(-1)
        scale = np.linalg.norm(c0, axis=-1) * np.linalg.norm(c1, axis=-1) * np.linalg.norm(c2, axis=-1)
        bad = ~(np.abs(det) > 1e-12 * scale)
        with np.errstate(all="ignore"):
            x0 = (rhs * np.cross(c1, c2)).sum(-1) / det
            x1 = (c0 * np.cross(rhs, c2)).sum(-1) / det
            x2 = (c0 * np.cross(c1, rhs)).sum(-1) / det
        return x0, x1, x2, bad

    def offer(t, accept, bad):
        nonlocal best, singular
        singular |= bad
        best = np.where(accept & ~bad & (t >= 0) & (t < best), t, best)

    for k in range(3):  # p + dir t = a + g1 b1 + g2 b2
        t, b1, b2, bad = solve(d, -(s[1] - s[0]), -(s[2] - s[0]), s[0] - q[k])
        offer(t, (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1), bad)
        t, b1, b2, bad = solve(-d, -(q[1] - q[0]), -(q[2] - q[0]), q[0] - s[k])
        offer(t, (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1), bad)
    for i, j in ((0, 1), (1, 2), (2, 0)):  # q_i + u a + d t = s_k + f b
        for k, l in ((0, 1), (1, 2), (2, 0)):
            t, a, b, bad = solve(d, q[j] - q[i], -(s[l] - s[k]), s[k] - q[i])
            offer(t, (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1), bad)
    return best, singular


def point_ray_times(v0, e1, e2, p, d):
    """Moeller-Trumbore in float64, elementwise: the point p moving along d against the closed triangle -> t (inf: none)."""
    with np.errstate(all="ignore"):
        h = np.cross(d, e2)
        det = (e1 * h).sum(-1)
        sv = p - v0
        u = (sv * h).sum(-1) / det
        qv = np.cross(sv, e1)
        v, t = (d * qv).sum(-1) / det, (e2 * qv).sum(-1) / det
        return np.where((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0), t, np.inf)


def contact_kinds(records_):
    """Of (N, 8) records: masks (coordinate, normals, edge_pairs, coplanar, segment, sphere, at_start, miss), from `axis`: 0-2, 3-4,
    5-13, 14-19, 20-25, 26, NONE on a hit, and the misses."""
    rec = np.ascontiguousarray(records_, F32).view(T.TRIANGLE_SWEEP_HIT).reshape(-1)
    miss = rec["prim_id"] == PRIM_MISS
    axis = rec["axis"]
    between = lambda lo, hi: ~miss & (axis >= lo) & (axis <= hi)
    return (between(0, 2), between(3, 4), between(5, 13), between(14, 19), between(20, 25), ~miss & (axis == AXIS_SPHERE),
            ~miss & (axis == AXIS_NONE), miss)


# -- the sweeps ---------------------------------------------------------------------------------------------------------------------
def _from_boxes(box_sweeps, seed, inscribed):
    """Box sweeps (sweep_box_cases) -> triangle sweeps with the same start and direction: a triangle of soup_triangles' four sizes
    around the centre (vertex k = centre + (uniform[0, 1)^3 - 0.5) x size, size cycling by index), or where `inscribed` the sliver
    (lo, lo, lo), (hi, hi, lo), (lo, hi, hi) of the box, whose bounds are the box's."""
    b = np.asarray(box_sweeps, F32)
    n = len(b)
    c, h = b[:, 0:3].astype(F64), b[:, 4:7].astype(F64)
    offset = (np.random.default_rng(seed).random((n, 3, 3)) - 0.5) * tc.SOUP_SIZES[np.arange(n) % 4][:, None, None]
    v = c[:, None, :] + offset
    lo, hi = c - h, c + h
    sliver = np.stack([lo, np.stack([hi[:, 0], hi[:, 1], lo[:, 2]], 1), np.stack([lo[:, 0], hi[:, 1], hi[:, 2]], 1)], 1)
    v = np.where(np.asarray(inscribed, bool)[:, None, None], sliver, v)
    return make_sweeps(v[:, 0], v[:, 1], v[:, 2], b[:, 8:11], b[:, 11])


def toward_surfaces(scene, n, seed):
    """sweep_box_cases.toward_surfaces with triangles of the four sizes around the centres."""
    return _from_boxes(bc.toward_surfaces(scene, n, seed), seed, np.zeros(n, bool))


def five_kinds(scene, n, seed):
    """n sweeps: toward surfaces, scattered, grazing, starting in contact, from far outside, a fifth each - sweep_box_cases' with a
    triangle in place of each box: the grazing and the in-contact ones the inscribed sliver, the others of the four sizes."""
    q = n // 5
    kind = np.repeat(np.arange(5), [q, q, q, q, n - 4 * q])
    return _from_boxes(bc.five_kinds(scene, n, seed), seed, (kind == 2) | (kind == 3))


def segments_and_points(scene, n, seed):
    """toward_surfaces and scattered with degenerate queries: q1 == q0 (a segment q0 q2), q2 on q0 q1 (halfway, or beyond q1), and a
    point (all three equal), by index mod 3."""
    s = _from_boxes(np.concatenate([bc.toward_surfaces(scene, n - n // 2, seed), bc.scattered(scene, n // 2, seed + 1)]), seed, np.zeros(n, bool))
    k = np.arange(n) % 3
    s[k == 0, 4:7] = s[k == 0, 0:3]
    on = (s[:, 0:3].astype(F64) + (s[:, 4:7].astype(F64) - s[:, 0:3]) * np.where(np.arange(n) % 2 == 0, 0.5, 2.0)[:, None]).astype(F32)
    s[k == 1, 8:11] = on[k == 1]
    s[k == 2, 4:7] = s[k == 2, 8:11] = s[k == 2, 0:3]
    return s


def plane_scene():
    """Three triangles in the plane z = 0 with no edge along a coordinate axis, two of them sharing an edge."""
    return ca.triangles_scene([[[0, 0, 0], [2, 0.5, 0], [0.5, 2, 0]], [[2, 0.5, 0], [2.75, 2.5, 0], [0.5, 2, 0]], [[-3, -1, 0], [-1.5, -2.5, 0], [-1.25, -0.5, 0]]])


def coplanar_sweeps(n, seed, plane=2, level=0.0, extent=3.0):
    """Sweeps inside the coordinate plane x_plane = level: every vertex has exactly that coordinate and d an exact 0 there.  Triangles,
    segments (q1 == q0) and points by index mod 4 (two of four are triangles), from a ring around the origin toward points within
    `extent` of it."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n)
    centre = np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(1.5, 3.0, (n, 1)) * extent
    v = centre[:, None, :] + (rng.random((n, 3, 2)) - 0.5) * rng.choice([0.3, 1.0, 2.5], (n, 1, 1))
    to = rng.uniform(-extent, extent, (n, 2)) - centre
    d2 = to / np.linalg.norm(to, axis=1, keepdims=True) * rng.uniform(0.2, 5.0, (n, 1))
    k = np.arange(n) % 4
    v[k == 2, 1] = v[k == 2, 0]
    v[k == 3, 1] = v[k == 3, 2] = v[k == 3, 0]
    inplane = [a for a in range(3) if a != plane]
    full = np.full((n, 3, 3), level)
    full[:, :, inplane] = v
    d = np.zeros((n, 3))
    d[:, inplane] = d2
    return make_sweeps(full[:, 0], full[:, 1], full[:, 2], d)


def wall_sweeps(n, seed):
    """For cornell12, the cube [-1, 1]^3: triangles in planes parallel to a wall, from inside the cube, moving along that wall's axis
    (two exact zero direction components) - the wall's coordinate axis, nS and nQ close together and the lowest number wins - and
    triangles in a wall's own plane from outside the cube sliding in (coplanar_sweeps on the wall's level)."""
    rng = np.random.default_rng(seed)
    m = n // 2
    axis, sign = np.arange(m) % 3, np.where(np.arange(m) % 6 < 3, -1.0, 1.0)
    v = rng.integers(-10, 11, (m, 3, 3)) / 16.0
    rows = np.arange(m)
    v[rows, :, axis] = (rng.integers(-8, 9, m) / 16.0)[:, None]
    d = np.zeros((m, 3))
    d[rows, axis] = sign * rng.choice([0.5, 1.0, 3.0], m)
    facing = make_sweeps(v[:, 0], v[:, 1], v[:, 2], d)
    q = (n - m) // 3
    sliding = [coplanar_sweeps(q, seed + 1, 2, -1.0, 1.0), coplanar_sweeps(q, seed + 2, 0, -1.0, 1.0), coplanar_sweeps(n - m - 2 * q, seed + 3, 1, 1.0, 1.0)]
    return np.concatenate([facing] + sliding)


def sphere_sweeps(scene, n, seed):
    """Toward, from inside and across the scene's spheres: triangles from around each sphere aimed at its centre, small triangles
    from inside it moving outward, and triangles that start across its surface."""
    rng = np.random.default_rng(seed)
    centre, radius = _scene_spheres(scene, F64)
    k = np.arange(n) % len(centre)
    kind = (np.arange(n) // len(centre)) % 3
    c, r = centre[k], radius[k][:, None]
    u = sc._unit(rng, n)
    start = c + u * r * np.where(kind == 0, rng.uniform(1.5, 4.0, n), np.where(kind == 1, rng.uniform(0.0, 0.4, n), rng.uniform(0.9, 1.1, n)))[:, None]
    v = start[:, None, :] + (rng.random((n, 3, 3)) - 0.5) * r[:, None, :] * np.where(kind == 1, 0.3, 0.8)[:, None, None]
    aim = np.where((kind == 0)[:, None], c - start + sc._unit(rng, n) * r * 0.5, sc._unit(rng, n))
    d = aim / np.linalg.norm(aim, axis=1, keepdims=True) * rng.uniform(0.2, 5.0, (n, 1))
    return make_sweeps(v[:, 0], v[:, 1], v[:, 2], d)


def fixtures(name, scene):
    """The sweeps the GPU tests ask of scene `name` ("soup": random_soup(3000, n_spheres=3); "cornell12"; "plane": plane_scene()),
    as a dict of named sets."""
    if name == "soup":
        return {"five_kinds": five_kinds(scene, 3000, 11), "segments": segments_and_points(scene, 600, 21), "spheres": sphere_sweeps(scene, 240, 31)}
    if name == "cornell12":
        return {"five_kinds": five_kinds(scene, 1000, 12), "walls": wall_sweeps(480, 22), "segments": segments_and_points(scene, 150, 23)}
    return {"coplanar": coplanar_sweeps(600, 41)}


K_GRID = sorted(m * 10.0 ** e for e in range(-12, 1) for m in (1, 1.5, 2, 3, 5, 7))


def sandwich_violations(scene, sweeps, k, t32=None):
    """The sweeps for which t64(+k diag) <= t32 <= t64(-k diag), with a relative 1e-6 on finite times, does not hold -> (before, after)."""
    eps = k * diagonal(scene)
    t32 = times(scene, sweeps, F32).astype(F64) if t32 is None else t32
    early, late = times(scene, sweeps, F64, eps), times(scene, sweeps, F64, -eps)
    return ~(early * (1 - 1e-6) <= t32), ~(t32 <= np.where(np.isfinite(late), late * (1 + 1e-6), late))


def measure_k(name, scene):
    """K_MEASURED[name] again: the smallest k of K_GRID without a violation over fixtures(name, scene), by bisection (a minute on the
    soup); 0.0 where eps = 0 has none.  `PYTHONPATH=. python tests/sweep_triangle_cases.py` prints all three."""
    sweeps = np.concatenate(list(fixtures(name, scene).values()))
    t32 = times(scene, sweeps, F32).astype(F64)
    bad = lambda k: int(sum(v.sum() for v in sandwich_violations(scene, sweeps, k, t32)))
    at_zero = bad(0.0)
    lo, hi = 0, len(K_GRID) - 1
    while at_zero and lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if bad(K_GRID[mid]) == 0 else (mid + 1, hi)
    return (K_GRID[lo] if at_zero else 0.0), at_zero, len(sweeps)


if __name__ == "__main__":
    from gpu_raytracer_amd import scenes
    for name_, scene_ in (("soup", scenes.random_soup(3000, n_spheres=3)), ("cornell12", scenes.cornell12()), ("plane", plane_scene())):
        k_, at_zero_, n_ = measure_k(name_, scene_)
        print(f"{name_}: K = {k_:g} ({at_zero_} of {n_} sweeps violate eps = 0; recorded {K_MEASURED[name_]:g})")
