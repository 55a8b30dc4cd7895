"""The box sweep's statement (include/rt_hip.h "Box sweeps", csrc/sweep_box_rules.h) in numpy, and the sweeps the tests ask about.

brute_force() evaluates the statement for every sweep against every triangle and sphere of a scene, in float32 - every numpy
operation is one f32 rounding, in the header's order, so its records are the bytes rt_sweep_box must return.  times() gives the time
of first contact alone, in float32 or in float64 (the same statement on the exact edges, with an offset on the half extents), which
is what the float32 statement is held to; clearance() is the static thirteen-axis test in float64 as a signed gap, which the float64
statement is held to along the path.  Helpers, no tests."""
import numpy as np

import closest_point_cases as cc
import sweep_cases as sc
from gpu_raytracer_amd import types as T

F32 = np.float32
F64 = np.float64
PRIM_MISS = cc.PRIM_MISS
SPHERE_FLAG = cc.SPHERE_FLAG
AXIS_NONE = 0xFFFFFFFF
AXIS_SPHERE = 13
PAIRS_PER_CHUNK = 1 << 17  # sweep x triangle pairs evaluated at a time (the statement holds some sixty arrays of that size)

# The smallest k of the grid 1, 1.5, 2, 3, 5, 7 x 10^n at which t64(h + k diag) <= t32 <= t64(h - k diag) holds for every one of
# five_kinds(scene, 4096, 11) whose extents are all >= 1e-3 x the diagonal (test_sweep_box_abi.py asserts the sandwich at twice this;
# DESIGN.md section 4 "Box sweeps").  On cornell12 no value of the grid is violated, down to eps = 0: every contact there closes on a
# box axis, t = (plane - h - c) / d in two roundings, which the relative 1e-6 on t covers; 1e-10 is the smallest value tried.
K_MEASURED = {"soup": 5e-7, "cornell12": 1e-10}

_dot = cc._dot
_cross = sc._cross
_order = cc._order
records = cc.records
diagonal = cc.diagonal


# -- the statement ------------------------------------------------------------------------------------------------------------------
class _Span:
    """The running entry and exit of one sweep x record pair over the axes: sb_axis."""

    def __init__(self, shape, dtype):
        self.t_in = np.zeros(shape, dtype)
        self.t_out = np.full(shape, np.inf, dtype)
        self.w_in = np.zeros(shape, dtype)
        self.axis = np.full(shape, AXIS_NONE, np.uint32)
        self.ok = np.ones(shape, bool)

    def add(self, axis, pmin, pmax, r, w):
        lo, hi = pmin - r, pmax + r
        pos, neg = w > 0, w < 0
        moving = pos | neg
        enter, leave = np.where(pos, lo, hi) / w, np.where(pos, hi, lo) / w
        self.ok &= np.where(moving, enter <= leave, (w == 0) & (pmin <= r) & (pmax >= -r))
        replace = np.broadcast_to(moving & (enter > self.t_in), self.t_in.shape)
        self.t_in = np.where(replace, enter, self.t_in)
        self.w_in = np.where(replace, w, self.w_in)
        self.axis = np.where(replace, np.uint32(axis), self.axis)
        self.t_out = np.where(moving, np.fmin(self.t_out, leave), self.t_out)

    def add3(self, axis, p, r, w):
        """p (..., 3) over the vertices: sb_span."""
        s = (p[..., 0] + p[..., 1]) + p[..., 2]
        self.ok &= s == s
        self.add(axis, np.fmin(np.fmin(p[..., 0], p[..., 1]), p[..., 2]), np.fmax(np.fmax(p[..., 0], p[..., 1]), p[..., 2]), r, w)


def triangle_contacts(v0, e1, e2, c, h, d):
    """c, h, d (m, 3) against n records -> t (m, n) in the arrays' dtype (inf: no contact), axis (m, n) uint32, w_in (m, n): the
    header's statement, every axis evaluated (the early returns change no answer)."""
    ty = c.dtype.type
    with np.errstate(all="ignore"):
        cc_, hh, dd = c[:, None, :], h[:, None, :], d[:, None, :]
        a = np.stack([v0[None] - cc_, (v0 + e1)[None] - cc_, (v0 + e2)[None] - cc_], 2)  # (m, n, vertex, axis)
        s = _Span(a.shape[:2], c.dtype)
        s.ok &= (np.abs(a) <= np.finfo(a.dtype).max).all((2, 3))
        for ax in range(3):
            s.add3(ax, a[..., ax], hh[..., ax], dd[..., ax])
        n = _cross(e1, e2)
        p = _dot(n[None], a[:, :, 0])
        s.add(3, p, p, _dot(np.abs(n)[None], hh), _dot(n[None], dd))
        ax_, ay, az = a[..., 0], a[..., 1], a[..., 2]
        hx, hy, hz = hh[..., 0], hh[..., 1], hh[..., 2]
        dx, dy, dz = dd[..., 0], dd[..., 1], dd[..., 2]
        for j, f in enumerate((e1, e2 - e1, e2)):
            g = np.abs(f)
            fx, fy, fz = f[None, :, None, 0], f[None, :, None, 1], f[None, :, None, 2]
            s.add3(4 + 3 * j, fy * az - fz * ay, g[None, :, 2] * hy + g[None, :, 1] * hz, f[None, :, 1] * dz - f[None, :, 2] * dy)
            s.add3(5 + 3 * j, fz * ax_ - fx * az, g[None, :, 2] * hx + g[None, :, 0] * hz, f[None, :, 2] * dx - f[None, :, 0] * dz)
            s.add3(6 + 3 * j, fx * ay - fy * ax_, g[None, :, 1] * hx + g[None, :, 0] * hy, f[None, :, 0] * dy - f[None, :, 1] * dx)
        contact = s.ok & (s.t_in <= s.t_out)
        return np.where(contact, s.t_in + ty(0), ty(np.inf)).astype(c.dtype), s.axis, s.w_in


def axis_normals(e1, e2, axis, w_in):
    """Elementwise: records (k, 3), axis (k,), w_in (k,) -> normal (k, 3): sb_axis_normal."""
    ty = e1.dtype.type
    with np.errstate(all="ignore"):
        L = np.zeros_like(e1)
        for a in range(3):
            L[axis == a, a] = 1
        L[axis == 3] = _cross(e1, e2)[axis == 3]
        fs = (e1, e2 - e1, e2)
        for j in range(3):
            f = fs[j]
            zero = np.zeros(len(f), f.dtype)
            forms = (np.stack([zero, -f[:, 2], f[:, 1]], 1), np.stack([f[:, 2], zero, -f[:, 0]], 1), np.stack([-f[:, 1], f[:, 0], zero], 1))
            for i in range(3):
                sel = axis == 4 + 3 * j + i
                L[sel] = forms[i][sel]
        length = np.sqrt(_dot(L, L))
        normal = np.where((w_in > 0)[:, None], -L, L) / length[:, None] + ty(0)
        return np.where((axis < 13)[:, None], normal, ty(0)).astype(e1.dtype)


def _take(best, accepts, t):
    return np.where(accepts & (t < best), t, best)


def sphere_times(centre, radius, c, h, d):
    """c, h, d (m, 3) against s spheres -> t (m, s)."""
    ty = c.dtype.type
    with np.errstate(all="ignore"):
        c, h, d = c[:, None, :], h[:, None, :], d[:, None, :]
        g = centre[None] - c
        gabs = np.abs(g)
        near, far = np.fmax(gabs - h, ty(0)), gabs + h
        radius = radius[None]
        rr = radius * radius
        dn, df = _dot(near, near), _dot(far, far)
        start = (dn <= rr) & (df >= rr)
        outside, inside = dn > rr, df < rr
        ddq = _dot(d, d)
        best = np.full(g.shape[:2], np.inf, c.dtype)
        h = np.broadcast_to(h, g.shape)
        d = np.broadcast_to(d, g.shape)
        for a in range(3):
            b, c_ = (a + 1) % 3, (a + 2) % 3
            plane = h[..., a] + radius
            t = (g[..., a] - np.where(d[..., a] > 0, plane, -plane)) / d[..., a]
            acc = ((d[..., a] > 0) | (d[..., a] < 0)) & (t >= 0) & (np.abs(g[..., b] - d[..., b] * t) <= h[..., b]) & (np.abs(g[..., c_] - d[..., c_] * t) <= h[..., c_])
            best = _take(best, outside & acc, t)
            for k in range(4):
                mb = g[..., b] + h[..., b] if k & 1 else g[..., b] - h[..., b]
                mc = g[..., c_] + h[..., c_] if k & 2 else g[..., c_] - h[..., c_]
                dd2 = d[..., b] * d[..., b] + d[..., c_] * d[..., c_]
                bq = mb * d[..., b] + mc * d[..., c_]
                x = mb * d[..., c_] - mc * d[..., b]
                disc = dd2 * rr - x * x
                t = (bq - np.sqrt(disc)) / dd2
                best = _take(best, outside & (disc >= 0) & (t >= 0) & (np.abs(g[..., a] - d[..., a] * t) <= h[..., a]), t)
        for k in range(8):
            m = np.stack([g[..., a] + h[..., a] if (k >> a) & 1 else g[..., a] - h[..., a] for a in range(3)], -1)
            b = _dot(m, d)
            x = _cross(m, d)
            disc = ddq * rr - _dot(x, x)
            root = np.sqrt(disc)
            t = np.where(outside, b - root, b + root) / ddq
            best = _take(best, (outside | inside) & (disc >= 0) & (t >= 0), t)
        return np.where(start, ty(0), best + ty(0)).astype(g.dtype)


def sphere_normals(centre, radius, c, h, d, t):
    """Elementwise, all (k, ...): sb_sphere_normal."""
    ty = c.dtype.type
    with np.errstate(all="ignore"):
        g = centre - c
        near = np.fmax(np.abs(g) - h, ty(0))
        P = g - d * t[:, None]
        out_v = np.fmin(np.fmax(P, -h), h) - P
        in_v = P - np.where(P >= 0, -h, h)
        v = np.where((_dot(near, near) > radius * radius)[:, None], out_v, in_v)
        length = np.sqrt(_dot(v, v))
        return np.where((length > 0)[:, None], v / length[:, None], ty(0)).astype(c.dtype)


def valid(sweeps):
    """The sweeps that walk: finite centre, half extent and direction, half extents >= 0, a direction that is not zero, tmax > 0."""
    s = np.asarray(sweeps)
    with np.errstate(all="ignore"):
        return (np.isfinite(s[:, 0:3]).all(1) & np.isfinite(s[:, 4:7]).all(1) & np.isfinite(s[:, 8:11]).all(1) & (s[:, 4:7] >= 0).all(1)
                & (s[:, 8:11] != 0).any(1) & (s[:, 11] > 0))


def _near_the_path(centroid, reach, c, d, r, margin):
    return sc._near_the_path(centroid, reach, c, d, r, margin)


def brute_force(scene, sweeps, prefilter=False):
    """(N, 12) float32 sweeps (centre, 0, half extent, 0, direction, tmax) -> (N, 8) float32 rt_box_sweep_hit records: the bytes
    rt_sweep_box returns.  prefilter (for scenes of 10^5 triangles): a triangle whose centroid is farther from the sweep's half-line
    than the centroid's reach + the box's half diagonal + 1e-3 x the scene's diagonal (far above the f32 statement's error) cannot be
    touched, so the statement is evaluated on the others only.  test_sweep_box_abi.py holds the filtered result to the unfiltered one."""
    sweeps = np.ascontiguousarray(sweeps, F32)
    n = len(sweeps)
    out = np.zeros(n, T.BOX_SWEEP_HIT)
    c, h, d, tmax = sweeps[:, 0:3], sweeps[:, 4:7], sweeps[:, 8:11], sweeps[:, 11]
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
        qc, qh, qd = c[lo:hi], h[lo:hi], d[lo:hi]
        best = start[lo:hi].copy()
        rec = out[lo:hi]
        found = np.zeros(hi - lo, bool)
        with np.errstate(all="ignore"):
            if len(sph):
                s_c, s_r = np.ascontiguousarray(sph["center"], F32).reshape(-1, 3), sph["radius"].astype(F32)
                t = sphere_times(s_c, s_r, qc, qh, qd)
                order = _order(t, np.broadcast_to(np.arange(len(sph), dtype=np.uint32), t.shape))
                k = order.argmin(1)
                win = order[rows, k] < best
                best = np.where(win, order[rows, k], best)
                found |= win
                tk = t[rows, k]
                moving = win & (tk > 0)
                rec["normal"][win] = 0
                rec["normal"][moving] = sphere_normals(s_c[k], s_r[k], qc, qh, qd, tk)[moving]
                rec["t"][win] = tk[win]
                rec["axis"][win] = np.where(tk > 0, AXIS_SPHERE, AXIS_NONE).astype(np.uint32)[win]
                rec["prim_id"][win] = (k[win] | SPHERE_FLAG).astype(np.uint32)
                rec["material_id"][win] = sph["material_id"][k][win]
            prim = all_prim
            if prefilter and len(all_v0):
                live = ok[lo:hi]
                half_diagonal = np.sqrt((qh[live].astype(F64) ** 2).sum(1)).astype(F32)
                prim = _near_the_path(centroid, reach, qc[live], qd[live], half_diagonal, margin) if live.any() else all_prim[:0]
            if len(prim):
                v0, e1, e2, mat = all_v0[prim], all_e1[prim], all_e2[prim], all_mat[prim]
                t, axis, w_in = triangle_contacts(v0, e1, e2, qc, qh, qd)
                order = _order(t, np.broadcast_to(prim.astype(np.uint64) | np.uint64(SPHERE_FLAG), t.shape))
                k = order.argmin(1)  # the lowest (t bits, key): at equal t the lower index
                win = order[rows, k] < best
                found |= win
                rec["normal"][win] = axis_normals(e1[k], e2[k], axis[rows, k], w_in[rows, k])[win]
                rec["t"][win] = t[rows, k][win]
                rec["axis"][win] = axis[rows, k][win]
                rec["prim_id"][win] = prim[k][win]
                rec["material_id"][win] = mat[k][win]
        miss = ~(found & ok[lo:hi])
        blank = np.zeros(int(miss.sum()), T.BOX_SWEEP_HIT)
        blank["t"] = tmax[lo:hi][miss]
        blank["axis"] = AXIS_NONE
        blank["prim_id"] = PRIM_MISS
        rec[miss] = blank
    return out.view(F32).reshape(n, 8)


def _scene_spheres(scene, dtype):
    sph = scene.spheres
    return np.ascontiguousarray(sph["center"], F32).reshape(-1, 3).astype(dtype), sph["radius"].astype(F32).astype(dtype)


def triangle_times_all(scene, sweeps, dtype=F32):
    """(N, n_triangles): the statement's time of every sweep with every triangle, inf where they do not touch (small scenes)."""
    v0, e1, e2, _ = records(scene, dtype)
    s = np.ascontiguousarray(sweeps, F32).astype(dtype)
    c, h, d = (np.ascontiguousarray(s[:, k:k + 3]) for k in (0, 4, 8))
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    return np.concatenate([triangle_contacts(v0, e1, e2, c[lo:lo + step], h[lo:lo + step], d[lo:lo + step])[0] for lo in range(0, len(s), step)])


def times(scene, sweeps, dtype, eps=0.0):
    """The time of first contact of each sweep by the statement in `dtype` (float32: on the stored f32 edges; float64: on the exact
    ones), with half extents + eps on every axis and tmax = inf; inf for a miss."""
    v0, e1, e2, _ = records(scene, dtype)
    s = np.ascontiguousarray(sweeps, F32).astype(dtype)
    c, h, d = np.ascontiguousarray(s[:, 0:3]), s[:, 4:7] + dtype(eps), np.ascontiguousarray(s[:, 8:11])
    s_c, s_r = _scene_spheres(scene, dtype)
    out = np.full(len(s), np.inf, dtype)
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    for lo in range(0, len(s), step):
        sl = slice(lo, lo + step)
        t = triangle_contacts(v0, e1, e2, c[sl], h[sl], d[sl])[0] if len(v0) else np.full((len(c[sl]), 1), np.inf, dtype)
        if len(s_c):
            t = np.concatenate([t, sphere_times(s_c, s_r, c[sl], h[sl], d[sl])], 1)
        out[sl] = np.where(np.isnan(t), np.inf, t).min(1)
    return out


def clearance(scene, centre, half_extent):
    """The static test in float64 as a distance: for boxes (N, 3), (N, 3) the smallest over the scene's primitives of the largest gap
    over the thirteen axes, each gap max(pmin - r, -(pmax + r)) over the length of its axis (zero axes left out).  > 0: the box is
    clear of everything by at least that on some axis; <= 0: it touches something.  A sphere: max(|near| - R, R - |far|)."""
    v0, e1, e2, _ = records(scene, F64)
    s_c, s_r = _scene_spheres(scene, F64)
    c, h = np.asarray(centre, F64), np.asarray(half_extent, F64)
    out = np.full(len(c), np.inf)
    unit = np.eye(3)
    axes = [np.broadcast_to(unit[i], v0.shape) for i in range(3)] + [np.cross(e1, e2)] + [np.cross(unit[i][None], f) for f in (e1, e2 - e1, e2) for i in range(3)]
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    with np.errstate(all="ignore"):
        for lo in range(0, len(c), step):
            cc_, hh = c[lo:lo + step, None, :], h[lo:lo + step, None, :]
            if len(v0):
                a = np.stack([v0[None] - cc_, (v0 + e1)[None] - cc_, (v0 + e2)[None] - cc_], 2)
                gap = np.full(a.shape[:2], -np.inf)
                for x in axes:
                    p = (a * x[None, :, None, :]).sum(-1)
                    r = (np.abs(x)[None] * hh).sum(-1)
                    length = np.linalg.norm(x, axis=1)[None]
                    g = np.maximum(p.min(-1) - r, -(p.max(-1) + r)) / length
                    gap = np.where(length > 0, np.maximum(gap, g), gap)
                out[lo:lo + step] = gap.min(1)
            if len(s_c):
                g = np.abs(s_c[None] - cc_)
                near, far = np.maximum(g - hh, 0.0), g + hh
                gap = np.maximum(np.linalg.norm(near, axis=-1) - s_r[None], s_r[None] - np.linalg.norm(far, axis=-1))
                out[lo:lo + step] = np.minimum(out[lo:lo + step], gap.min(1))
    return out


def contact_kinds(records_):
    """Of (N, 8) records: masks (box_face, triangle_face, edge_edge, sphere, at_start, miss), from `axis`: 0-2 a face of the box, 3
    the triangle's face, 4-12 an edge of each."""
    rec = np.ascontiguousarray(records_, F32).view(T.BOX_SWEEP_HIT).reshape(-1)
    miss = rec["prim_id"] == PRIM_MISS
    axis = rec["axis"]
    return (~miss & (axis < 3), ~miss & (axis == 3), ~miss & (axis >= 4) & (axis <= 12), ~miss & (axis == AXIS_SPHERE),
            ~miss & (axis == AXIS_NONE), miss)


# -- the sweeps ---------------------------------------------------------------------------------------------------------------------
H_RANGE = (1e-3, 0.05)  # half extents per axis, in diagonals


def _pack(centre, half_extent, direction, tmax=np.inf):
    out = np.zeros((len(centre), 12), F32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11], out[:, 11] = centre, half_extent, direction, tmax
    return out


def _extents(scene, rng, n):
    """Per axis log-uniform in H_RANGE x the scene's diagonal; every eighth sweep has one zero extent."""
    h = np.exp(rng.uniform(np.log(H_RANGE[0]), np.log(H_RANGE[1]), (n, 3))) * diagonal(scene)
    k = np.arange(7, n, 8)
    h[k, k % 3] = 0.0
    return h


def toward_surfaces(scene, n, seed, half_extent=None):
    """Centres over 1.5 times the box, aimed at points of the surface, |d| in 0.2 .. 5; half_extent: one value for every axis and sweep
    in place of the drawn ones."""
    rng = np.random.default_rng(seed)
    lo, hi = sc._box(scene)
    origin = (lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * 1.5 * (hi - lo)
    to = sc._targets(scene, rng, n) - origin
    d = to / np.linalg.norm(to, axis=1, keepdims=True) * rng.uniform(0.2, 5.0, (n, 1))
    h = _extents(scene, rng, n)
    return _pack(origin, h if half_extent is None else half_extent, d)


def scattered(scene, n, seed):
    """Centres over 1.5 times the box, directions uniform on the sphere, |d| in 0.2 .. 5."""
    rng = np.random.default_rng(seed)
    lo, hi = sc._box(scene)
    origin = (lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * 1.5 * (hi - lo)
    return _pack(origin, _extents(scene, rng, n), sc._unit(rng, n) * rng.uniform(0.2, 5.0, (n, 1)))


def grazing(scene, n, seed):
    """Past a point of the surface with a face of the box at h (1 -+ 1e-3) from it on one axis, moving across that axis (a zero
    direction component): a hair inside and a hair outside of touching it."""
    rng = np.random.default_rng(seed)
    p, h = sc._targets(scene, rng, n), _extents(scene, rng, n)
    across = np.arange(n) % 3
    rows = np.arange(n)
    side = sc._unit(rng, n)
    side[rows, across] = 0.0
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    passing = p.copy()
    passing[rows, across] += rng.choice([-1.0, 1.0], n) * h[rows, across] * np.where(rows % 2 == 0, 1 - 1e-3, 1 + 1e-3)
    return _pack(passing - side * rng.uniform(0.5, 3.0, (n, 1)), h, side * rng.uniform(0.2, 5.0, (n, 1)))


def in_contact(scene, n, seed):
    """Starting with a point of the surface inside the box."""
    rng = np.random.default_rng(seed)
    h = _extents(scene, rng, n)
    origin = sc._targets(scene, rng, n) + h * rng.uniform(-0.95, 0.95, (n, 3))
    return _pack(origin, h, sc._unit(rng, n) * rng.uniform(0.2, 5.0, (n, 1)))


def far_outside(scene, n, seed):
    """From 20 to 100 diagonals away, aimed at points of the surface."""
    rng = np.random.default_rng(seed)
    p = sc._targets(scene, rng, n)
    origin = p + sc._unit(rng, n) * (diagonal(scene) * rng.uniform(20.0, 100.0, (n, 1)))
    to = p - origin
    return _pack(origin, _extents(scene, rng, n), to / np.linalg.norm(to, axis=1, keepdims=True) * rng.uniform(0.2, 5.0, (n, 1)))


def five_kinds(scene, n, seed):
    """n sweeps: toward surfaces, scattered, grazing, starting in contact, from far outside, a fifth each."""
    q = n // 5
    return np.concatenate([toward_surfaces(scene, q, seed), scattered(scene, q, seed + 1), grazing(scene, q, seed + 2),
                           in_contact(scene, q, seed + 3), far_outside(scene, n - 4 * q, seed + 4)])


def full_extents(scene, sweeps):
    """The sweeps whose half extents are all >= 1e-3 x the scene's diagonal (as f32 stores them)."""
    return (np.asarray(sweeps)[:, 4:7] >= F32(H_RANGE[0] * diagonal(scene))).all(1)


def cube_sweeps(seed):
    """1024 sweeps for cornell12, the cube [-1, 1]^3 whose walls share edges and corners, with boxes whose faces are parallel to the
    walls: along an axis (two zero direction components, some of them -0) from a grid of interior points, toward points of the walls
    from in and around the cube, toward points of the cube's edges and its corners, cubes along the cube's diagonals (by symmetry
    equally early on two or three walls, bit for bit), and starting with faces in or across two or three walls.  Coordinates and
    extents are multiples of 1/16 where the ties are meant to be exact."""
    rng = np.random.default_rng(seed)
    n = 256
    grid = rng.integers(-7, 8, (n, 3)) / 16.0
    axis, sign = np.arange(n) % 3, np.where(np.arange(n) % 6 < 3, 1.0, -1.0)
    along = np.where(np.arange(n) % 4 < 2, 0.0, -0.0)[:, None] * np.ones((n, 3))
    along[np.arange(n), axis] = sign * rng.choice([0.5, 1.0, 3.0], n)
    axial = _pack(grid, rng.choice([0.0625, 0.125, 0.25], (n, 3)), along)
    target = np.where(rng.random((n, 3)) < 0.7, rng.choice([-1.0, 1.0], (n, 3)), rng.uniform(-1.0, 1.0, (n, 3)))  # mostly edges and corners
    target[:, 0] = np.where(np.abs(target[:, 1:]).max(1) < 1, np.sign(target[:, 0] + 1e-9), target[:, 0])     # on the cube's surface at least
    origin = np.where((np.arange(n) % 2 == 0)[:, None], rng.uniform(-0.7, 0.7, (n, 3)),                         # from inside, where seams are concave,
                      target * rng.uniform(1.3, 2.5, (n, 1)) + rng.uniform(-0.1, 0.1, (n, 3)))                  # and from outside, where they stick out
    seams = _pack(origin, rng.uniform(0.02, 0.25, (n, 3)), (target - origin) * rng.uniform(0.3, 2.0, (n, 1)))
    a = rng.integers(-8, 9, n) / 16.0
    signs = rng.choice([-1.0, 1.0], (n, 3))
    diagonal_ = _pack(a[:, None] * signs * rng.choice([1.0, -1.0], (n, 1)), rng.choice([0.0625, 0.125, 0.25], (n, 1)) * np.ones((1, 3)),
                      signs * rng.choice([0.5, 1.0, 2.0], (n, 1)))
    corner = rng.choice([-1.0, 1.0], (n // 2, 3))
    free = rng.random((n // 2, 3)) < 0.3  # a free coordinate: near an edge rather than a corner
    free[:, 0] &= ~free[:, 1:].all(1)
    inset = np.where(free, rng.integers(-8, 9, (n // 2, 3)) / 16.0, corner * (1 - rng.choice([0.0625, 0.125, 0.25], (n // 2, 1))))
    touching = _pack(inset, rng.choice([0.125, 0.25], (n // 2, 1)) * np.ones((1, 3)), sc._unit(rng, n // 2))
    return np.concatenate([axial, _toward_surfaces_cube(rng, n // 2), seams, diagonal_, touching])


def _toward_surfaces_cube(rng, n):
    origin = rng.uniform(-1.5, 1.5, (n, 3))
    target = rng.uniform(-1.0, 1.0, (n, 3))
    target[np.arange(n), np.arange(n) % 3] = np.where(np.arange(n) % 6 < 3, -1.0, 1.0)  # on a wall's plane (z = +1 is open)
    to = target - origin
    return _pack(origin, rng.uniform(0.01, 0.3, (n, 3)), to / np.linalg.norm(to, axis=1, keepdims=True) * rng.uniform(0.2, 5.0, (n, 1)))
