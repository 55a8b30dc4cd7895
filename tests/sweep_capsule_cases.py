"""The capsule sweep's statement (include/rt_hip.h "Capsule sweeps", csrc/sweep_capsule_rules.h) in numpy, and the sweeps the tests
ask about.

brute_force() evaluates the statement for every sweep against every triangle and sphere of a scene, in float32 - every numpy
operation is one f32 rounding, in the header's order, so its records are the bytes rt_sweep_capsule must return.  times() gives the
time of first contact alone, in float32 or in float64 (the same statement on the exact edges, with an offset on the radius), which
is what the float32 statement is held to; cap_triangle() is the closest pair of the axis and a triangle, which the float64 statement
is held to along the path.  Helpers, no tests."""
import numpy as np

import closest_point_cases as cc
import sweep_cases as sc
from gpu_raytracer_amd import types as T

F32 = np.float32
F64 = np.float64
PRIM_MISS = cc.PRIM_MISS
SPHERE_FLAG = cc.SPHERE_FLAG
PAIRS_PER_CHUNK = 1 << 16  # sweep x triangle pairs evaluated at a time (the statement holds some hundred arrays of that size)

# The smallest k of the grid 1, 1.5, 2, 3, 5, 7 x 10^n at which t64(r + k diag) <= t32 <= t64(r - k diag) holds for every one of
# five_kinds(scene, 4096, 11), none left out (test_sweep_capsule_abi.py asserts the sandwich at twice this; DESIGN.md section 4
# "Capsule sweeps").  Violations below it: soup 2 of 4096 at 2e-9, 17 at 1e-11; cornell12 2 at 2e-8, 11 at 1e-11.
K_MEASURED = {"soup": 3e-9, "cornell12": 3e-8}

_dot = cc._dot
_cross = sc._cross
_order = cc._order
_take = sc._take
records = cc.records
diagonal = cc.diagonal


# -- the statement ------------------------------------------------------------------------------------------------------------------
def _cp_tri(e1, e2, ap):
    """cp_triangle on ap = p - v0, all operands broadcast against each other -> dist2, v, w (closest_point_cases.triangle_candidates
    with the point already relative to v0)."""
    ty = ap.dtype.type
    one = ty(1)
    with np.errstate(all="ignore"):
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
        v, w = np.where(c, ty(0), v), np.where(c, d2 / (d2 - d6), w)
        c = (d6 >= 0) & (d5 <= d6)
        v, w = np.where(c, ty(0), v), np.where(c, one, w)
        c = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = np.where(c, d1 / (d1 - d3), v), np.where(c, ty(0), w)
        c = (d3 >= 0) & (d4 <= d3)
        v, w = np.where(c, one, v), np.where(c, ty(0), w)
        c = (d1 <= 0) & (d2 <= 0)
        v, w = np.where(c, ty(0), v), np.where(c, ty(0), w)
        r = (e1 * v[..., None] + e2 * w[..., None]) - ap
        return _dot(r, r), v, w


def _clamp01(x):
    ty = x.dtype.type
    return np.where(x < 0, ty(0), np.where(x > 1, ty(1), x))


def _pair_edge(m, e, ax, aa):
    """sc_pair_edge: the axis from m (relative to the edge's origin) against the edge e -> dist2 (inf where absent), s, u."""
    ty = m.dtype.type
    ee, f, c, b = _dot(e, e), _dot(e, m), _dot(ax, m), _dot(ax, e)
    den = aa * ee - b * b
    s = np.where(den > 0, _clamp01((b * f - c * ee) / den), ty(0))
    u = (b * s + f) / ee
    lo, hi = u < 0, u > 1
    s = np.where(lo, _clamp01(-c / aa), np.where(hi, _clamp01((b - c) / aa), s))
    u = np.where(lo, ty(0), np.where(hi, ty(1), u))
    g = (m + ax * s[..., None]) - e * u[..., None]
    return np.where((aa > 0) & (ee > 0), _dot(g, g), ty(np.inf)), s, u


def cap_triangle(v0, e1, e2, P, ax):
    """The closest pair of the axis segment P .. P + ax and a triangle, operands broadcast against each other (..., 3) -> dist2, s, v,
    w: the header's rule 1."""
    ty = P.dtype.type
    zero, one = ty(0), ty(1)
    with np.errstate(all="ignore"):
        ap = P - v0
        best, v, w = _cp_tri(e1, e2, ap)
        s = np.zeros_like(best)
        d2, bv, bw = _cp_tri(e1, e2, (P + ax) - v0)
        r = d2 < best
        best, s, v, w = np.where(r, d2, best), np.where(r, one, s), np.where(r, bv, v), np.where(r, bw, w)
        aa = _dot(ax, ax)
        m1, e3 = ap - e1, e2 - e1
        for kind, (m, e) in enumerate(((ap, e1), (ap, e2), (m1, e3))):
            d2, cs, cu = _pair_edge(m, e, ax, aa)
            r = d2 < best
            best, s = np.where(r, d2, best), np.where(r, cs, s)
            v = np.where(r, (cu, zero, one - cu)[kind], v)
            w = np.where(r, (zero, cu, cu)[kind], w)
        n = _cross(e1, e2)
        nn, hA, hB = _dot(n, n), _dot(n, ap), _dot(n, ap + ax)
        ps = hA / (hA - hB)
        p = ap + ax * ps[..., None]
        fv, fw = _dot(_cross(p, e2), n) / nn, _dot(_cross(e1, p), n) / nn
        r = (aa > 0) & (((hA < 0) & (hB > 0)) | ((hA > 0) & (hB < 0))) & (fv >= 0) & (fw >= 0) & (fv + fw <= 1) & (0 < best)
        best, s, v, w = np.where(r, zero, best), np.where(r, ps, s), np.where(r, fv, v), np.where(r, fw, w)
        return best.astype(P.dtype), s.astype(P.dtype), v.astype(P.dtype), w.astype(P.dtype)


def _face(best, m, a, b, d, r, parallelogram):
    ty = m.dtype.type
    n = _cross(a, b)
    nn = _dot(n, n)
    ln = np.sqrt(nn)
    h, nd = _dot(n, m), _dot(n, d)
    sg = np.where(h < 0, ty(-1), ty(1))
    num, den = np.abs(h) - r * ln, -(sg * nd)
    t = num / den
    k = sg * r / ln
    p = (m + d * t[..., None]) - n * k[..., None]
    fv, fw = _dot(_cross(p, b), n) / nn, _dot(_cross(a, p), n) / nn
    inside = ((fv <= 1) & (fw <= 1)) if parallelogram else (fv + fw <= 1)
    return _take(best, (num >= 0) & (den > 0) & (fv >= 0) & (fw >= 0) & inside, t)


def _vertex(best, m, d, dd, rr):
    b = _dot(m, d)
    x = _cross(m, d)
    disc = dd * rr - _dot(x, x)
    t = (-b - np.sqrt(disc)) / dd
    return _take(best, (disc >= 0) & (t >= 0), t)


def _edge(best, m, e, d, rr):
    g = _cross(e, d)
    p = _cross(g, e)
    A, B, hh, ee = _dot(g, g), _dot(m, p), _dot(m, g), _dot(e, e)
    disc = rr * A - hh * hh
    t = (-B - np.sqrt(ee * disc)) / A
    sp = (_dot(m, e) + t * _dot(d, e)) / ee
    return _take(best, (A > 0) & (disc >= 0) & (t >= 0) & (0 <= sp) & (sp <= 1), t)


def _groups(v0, e1, e2, c, ax, d, r):
    """sc_pieces and the start rule on operands that broadcast against each other ((..., 3), r (...)) -> (start (...) bool, g (4, ...))."""
    with np.errstate(all="ignore"):
        rr, dd = r * r, _dot(d, d)
        ap = c - v0
        m1, m2, e3 = ap - e1, ap - e2, e2 - e1
        b0, b1, b2 = ap + ax, m1 + ax, m2 + ax
        fresh = lambda: np.full(ap.shape[:-1], np.inf, c.dtype)
        g = []
        for n0, n1, n2 in ((ap, m1, m2), (b0, b1, b2)):
            best = _face(fresh(), n0, e1, e2, d, r, False)
            for m in (n0, n1, n2):
                best = _vertex(best, m, d, dd, rr)
            for m, e in ((n0, e1), (n0, e2), (n1, e3)):
                best = _edge(best, m, e, d, rr)
            g.append(best)
        best = fresh()
        for m in (b0, b1, b2):
            best = _edge(best, m, ax, d, rr)
        g.append(best)
        best = fresh()
        for m, e in ((b0, e1), (b0, e2), (b1, e3)):
            best = _face(best, m, e, ax, d, r, True)
        g.append(best)
        start = cap_triangle(v0, e1, e2, c, ax)[0] <= rr
        return start, np.stack(g).astype(c.dtype)


def _times(v0, e1, e2, c, ax, d, r):
    """sc_triangle on operands that broadcast against each other."""
    ty = c.dtype.type
    start, g = _groups(v0, e1, e2, c, ax, d, r)
    best = g[0]
    for k in (1, 2, 3):
        best = np.where(g[k] < best, g[k], best)
    return np.where(start, ty(0), best + ty(0)).astype(c.dtype)


def triangle_groups(v0, e1, e2, A, ax, d, r):
    """A, ax, d (m, 3), r (m,) against n records -> (start (m, n) bool: cap_triangle at the start <= rr; g (4, m, n): the best time
    of each of the four piece groups, inf where none accepts)."""
    return _groups(v0[None], e1[None], e2[None], A[:, None, :], ax[:, None, :], d[:, None, :], r[:, None])


def triangle_times(v0, e1, e2, A, ax, d, r):
    """A, ax, d (m, 3), r (m,) against n records -> t (m, n) in the arrays' dtype, inf where no piece accepts: sc_triangle."""
    return _times(v0[None], e1[None], e2[None], A[:, None, :], ax[:, None, :], d[:, None, :], r[:, None])


def _sphere_pose(centre, A, ax):
    """mA, mB, lenA, lenB, f, dmin of sc_sphere_pose; operands broadcast."""
    ty = A.dtype.type
    mA = A - centre
    mB = mA + ax
    lenA, lenB = np.sqrt(_dot(mA, mA)), np.sqrt(_dot(mB, mB))
    aa = _dot(ax, ax)
    f = np.where(aa > 0, _clamp01(-_dot(mA, ax) / aa), ty(0))
    pm = mA + ax * f[..., None]
    return mA, mB, lenA, lenB, f, np.sqrt(_dot(pm, pm))


def sphere_times(centre, radius, A, ax, d, r):
    """A, ax, d (m, 3), r (m,) against s spheres -> t (m, s): sc_sphere."""
    ty = A.dtype.type
    with np.errstate(all="ignore"):
        c, d, r, ax = A[:, None, :], d[:, None, :], r[:, None], ax[:, None, :]
        dd = _dot(d, d)
        mA, mB, lenA, lenB, f, dmin = _sphere_pose(centre[None], c, ax)
        R = radius[None]
        dmax = np.where(lenB > lenA, lenB, lenA)
        start = (dmin - R <= r) & (R - dmax <= r)
        rs = R + r
        rr = rs * rs
        out = np.full(lenA.shape, np.inf, A.dtype)
        out = _vertex(out, mA, d, dd, rr)
        out = _vertex(out, mB, d, dd, rr)
        out = _edge(out, mB, np.broadcast_to(ax, mB.shape), d, rr)
        rs = R - r
        rr = rs * rs
        ins = np.full(lenA.shape, np.inf, A.dtype)
        for m in (mA, mB):
            b = _dot(m, d)
            x = _cross(m, d)
            disc = dd * rr - _dot(x, x)
            t = (-b + np.sqrt(disc)) / dd
            ins = _take(ins, (disc >= 0) & (t >= 0), t)
        t = np.where(dmin > R, out, ins) + ty(0)
        return np.where(start, ty(0), t).astype(A.dtype)


def sphere_points(centre, radius, Ap, ax):
    """Elementwise (k, ...): s = sc_sphere_s at the pose Ap and cp_sphere's point from Ap + ax * s."""
    ty = Ap.dtype.type
    with np.errstate(all="ignore"):
        _, _, lenA, lenB, f, dmin = _sphere_pose(centre, Ap, ax)
        s = np.where(dmin > radius, f, np.where(lenB > lenA, ty(1), ty(0))).astype(Ap.dtype)
        p = Ap + ax * s[:, None]
        oc = p - centre
        length = np.sqrt(_dot(oc, oc))
        at_centre = np.zeros_like(oc)
        at_centre[:, 0] = radius
        pos = np.where((length > 0)[:, None], centre + oc * (radius / length)[:, None], centre + at_centre)
        return s, pos.astype(Ap.dtype)


def valid(sweeps):
    """The sweeps that walk: finite origin, axis and direction, a direction that is not zero, 0 < radius < inf, tmax > 0."""
    s = np.asarray(sweeps)
    with np.errstate(all="ignore"):
        return (np.isfinite(s[:, 0:3]).all(1) & np.isfinite(s[:, 4:7]).all(1) & np.isfinite(s[:, 8:11]).all(1) & (s[:, 8:11] != 0).any(1)
                & (s[:, 3] > 0) & np.isfinite(s[:, 3]) & (s[:, 11] > 0))


def brute_force(scene, sweeps, prefilter=False, return_groups=False):
    """(N, 12) float32 sweeps (origin, radius, axis, 0, direction, tmax) -> (N, 8) float32 rt_capsule_sweep_hit records: the bytes
    rt_sweep_capsule returns.  prefilter (for scenes of 10^5 triangles): a triangle whose centroid is farther from the half-line of
    end A than the centroid's reach + the radius + the axis' length + 1e-3 x the scene's diagonal (far above the f32 statement's
    error) cannot be touched, so the statement is evaluated on the others only."""
    sweeps = np.ascontiguousarray(sweeps, F32)
    n = len(sweeps)
    out = np.zeros(n, T.CAPSULE_SWEEP_HIT)
    A, r, ax, d, tmax = sweeps[:, 0:3], sweeps[:, 3], sweeps[:, 4:7], sweeps[:, 8:11], sweeps[:, 11]
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
        qA, qx, qd, qr = A[lo:hi], ax[lo:hi], d[lo:hi], r[lo:hi]
        best = start[lo:hi].copy()
        rec = out[lo:hi]
        found = np.zeros(hi - lo, bool)
        with np.errstate(all="ignore"):
            if len(sph):
                s_c, s_r = np.ascontiguousarray(sph["center"], F32).reshape(-1, 3), sph["radius"].astype(F32)
                t = sphere_times(s_c, s_r, qA, qx, qd, qr)
                order = _order(t, np.broadcast_to(np.arange(len(sph), dtype=np.uint32), t.shape))
                k = order.argmin(1)
                win = order[rows, k] < best
                best = np.where(win, order[rows, k], best)
                found |= win
                tk = t[rows, k]
                s, pos = sphere_points(s_c[k], s_r[k], qA + qd * tk[:, None], qx)
                rec["position"][win] = pos[win]
                rec["t"][win] = tk[win]
                rec["s"][win] = s[win]
                rec["prim_id"][win] = (k[win] | SPHERE_FLAG).astype(np.uint32)
                rec["material_id"][win] = sph["material_id"][k][win]
            prim = all_prim
            if prefilter and len(all_v0):
                live = ok[lo:hi]
                length = np.sqrt((qx[live].astype(F64) ** 2).sum(1)).astype(F32)
                prim = sc._near_the_path(centroid, reach, qA[live], qd[live], qr[live] + length, margin) if live.any() else all_prim[:0]
            if len(prim):
                v0, e1, e2, mat = all_v0[prim], all_e1[prim], all_e2[prim], all_mat[prim]
                t = triangle_times(v0, e1, e2, qA, qx, qd, qr)
                order = _order(t, np.broadcast_to(prim.astype(np.uint64) | np.uint64(SPHERE_FLAG), t.shape))
                k = order.argmin(1)  # the lowest (t bits, key): at equal t the lower index
                win = order[rows, k] < best
                found |= win
                tk = t[rows, k]
                _, s, v, w = cap_triangle(v0[k], e1[k], e2[k], qA + qd * tk[:, None], qx)
                pos = v0[k] + (e1[k] * v[:, None] + e2[k] * w[:, None])
                rec["position"][win] = pos[win]
                rec["t"][win] = tk[win]
                rec["s"][win] = s[win]
                rec["prim_id"][win] = prim[k][win]
                rec["material_id"][win] = mat[k][win]
        miss = ~(found & ok[lo:hi])
        blank = np.zeros(int(miss.sum()), T.CAPSULE_SWEEP_HIT)
        blank["t"] = tmax[lo:hi][miss]
        blank["prim_id"] = PRIM_MISS
        rec[miss] = blank
    return out.view(F32).reshape(n, 8)


def _scene_spheres(scene, dtype):
    sph = scene.spheres
    return np.ascontiguousarray(sph["center"], F32).reshape(-1, 3).astype(dtype), sph["radius"].astype(F32).astype(dtype)


def _pairs(centroid, reach, A, ax, d, r, margin):
    """(i, j): the sweep x record pairs that can touch: the centroid's distance from the half-line of end A is at most the
    centroid's reach + r + the axis' length + margin.  In float64."""
    m = centroid[None] - A[:, None, :]
    dn = (d / np.linalg.norm(d, axis=1, keepdims=True))[:, None, :]
    along = np.maximum((m * dn).sum(-1), 0.0)
    m = m - along[..., None] * dn
    limit = reach[None] + (r + np.linalg.norm(ax, axis=1) + margin)[:, None]
    return np.nonzero((m * m).sum(-1) <= limit * limit)


def times(scene, sweeps, dtype, radius_offset=0.0, prefilter=True):
    """The time of first contact of each sweep by the statement in `dtype` (float32: on the stored f32 edges; float64: on the exact
    ones), with radius + radius_offset for the radius and tmax = inf; inf for a miss.  prefilter: the statement is evaluated only on
    the pairs that can touch (_pairs, with a margin of 1e-3 x the diagonal + |radius_offset|, far above either statement's error);
    test_sweep_capsule_abi.py holds the filtered times to the unfiltered ones."""
    v0, e1, e2, _ = records(scene, dtype)
    s = np.ascontiguousarray(sweeps, F32).astype(dtype)
    A, ax, d = (np.ascontiguousarray(s[:, k:k + 3]) for k in (0, 4, 8))
    r = s[:, 3] + dtype(radius_offset)
    s_c, s_r = _scene_spheres(scene, dtype)
    out = np.full(len(s), np.inf, dtype)
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    if prefilter and len(v0):
        centroid, reach = sc._reach(*records(scene, F64)[:3])
        margin = 1e-3 * diagonal(scene) + abs(radius_offset)
        live = valid(sweeps)
        step *= 4
    for lo in range(0, len(s), step):
        sl = slice(lo, lo + step)
        if prefilter and len(v0):
            s64 = np.ascontiguousarray(sweeps, F32)[sl].astype(F64)[live[sl]]
            i, j = _pairs(centroid, reach, s64[:, 0:3], s64[:, 4:7], s64[:, 8:11], s64[:, 3], margin)
            i = np.flatnonzero(live[sl])[i] + lo
            t = _times(v0[j], e1[j], e2[j], A[i], ax[i], d[i], r[i])
            np.minimum.at(out, i, np.where(np.isnan(t), np.inf, t))
        elif len(v0):
            t = triangle_times(v0, e1, e2, A[sl], ax[sl], d[sl], r[sl])
            out[sl] = np.where(np.isnan(t), np.inf, t).min(1)
        if len(s_c):
            t = sphere_times(s_c, s_r, A[sl], ax[sl], d[sl], r[sl])
            out[sl] = np.minimum(out[sl], np.where(np.isnan(t), np.inf, t).min(1))
    return out


def clearance(scene, sweeps, t, dtype=F64):
    """The distance of the axis segment of each sweep's pose at time t (N,) from the scene's surface, in `dtype`: the smallest
    sqrt(cap_triangle) over the triangles, and for a sphere the nearer of dmin - R and R - dmax where positive, else 0."""
    v0, e1, e2, _ = records(scene, dtype)
    s = np.ascontiguousarray(sweeps, F32).astype(dtype)
    P = s[:, 0:3] + s[:, 8:11] * np.asarray(t, dtype)[:, None]
    ax = np.ascontiguousarray(s[:, 4:7])
    s_c, s_r = _scene_spheres(scene, dtype)
    out = np.full(len(s), np.inf, dtype)
    step = max(1, PAIRS_PER_CHUNK // max(len(v0), 1))
    with np.errstate(all="ignore"):
        for lo in range(0, len(s), step):
            sl = slice(lo, lo + step)
            if len(v0):
                d2 = cap_triangle(v0[None], e1[None], e2[None], P[sl, None, :], ax[sl, None, :])[0]
                out[sl] = np.sqrt(np.where(np.isnan(d2), np.inf, d2).min(1))
            if len(s_c):
                _, _, lenA, lenB, _, dmin = _sphere_pose(s_c[None], P[sl, None, :], ax[sl, None, :])
                gap = np.maximum(np.maximum(dmin - s_r[None], s_r[None] - np.maximum(lenA, lenB)), 0)
                out[sl] = np.minimum(out[sl], gap.min(1))
    return out


# -- the sweeps ---------------------------------------------------------------------------------------------------------------------
def _pack(origin, axis, direction, radius, tmax=np.inf):
    out = np.zeros((len(origin), 12), F32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 8:11], out[:, 11] = origin, radius, axis, direction, tmax
    return out


def _axes(scene, rng, n):
    """By index mod 5: zero; parallel to an edge of some triangle; in some triangle's plane; upright (+-y); diagonal.  Lengths
    log-uniform in 0.02 .. 0.6."""
    v0, e1, e2, _ = records(scene, F64)
    k = rng.integers(0, len(v0), n)
    length = np.exp(rng.uniform(np.log(0.02), np.log(0.6), (n, 1)))
    unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    kind = np.arange(n) % 5
    a, b = rng.uniform(-1, 1, (n, 1)), rng.uniform(-1, 1, (n, 1))
    upright = np.zeros((n, 3))
    upright[:, 1] = rng.choice([-1.0, 1.0], n)
    axis = np.where((kind == 1)[:, None], unit(e1[k]), np.where((kind == 2)[:, None], unit(e1[k] * a + e2[k] * b),
                    np.where((kind == 3)[:, None], upright, sc._unit(rng, n)))) * length
    axis[kind == 0] = 0.0
    return axis


def _origin_for(point, axis, rng):
    """End A such that `point` is a random point of the axis: the body as a whole, not its end, is what is aimed."""
    return point - axis * rng.random((len(point), 1))


def toward_surfaces(scene, n, seed, radius=(0.01, 0.3), axes=None):
    """Bodies over 1.5 times the box, aimed at points of the surface (inside triangles, on edges, on vertices), |d| in 0.2 .. 5,
    radius log-uniform in `radius`; axes: (n, 3) or one triple in place of the drawn ones."""
    rng = np.random.default_rng(seed)
    lo, hi = sc._box(scene)
    mid = (lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * 1.5 * (hi - lo)
    to = sc._targets(scene, rng, n) - mid
    d = to / np.linalg.norm(to, axis=1, keepdims=True) * rng.uniform(0.2, 5.0, (n, 1))
    r = np.exp(rng.uniform(np.log(radius[0]), np.log(radius[1]), n))
    axis = _axes(scene, rng, n) if axes is None else np.broadcast_to(np.asarray(axes, F64), (n, 3))
    return _pack(mid - axis / 2, axis, d, r)


def scattered(scene, n, seed):
    """Origins over 1.5 times the box, directions uniform on the sphere, |d| in 0.2 .. 5, r in 0.01 .. 0.3."""
    rng = np.random.default_rng(seed)
    lo, hi = sc._box(scene)
    origin = (lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * 1.5 * (hi - lo)
    return _pack(origin, _axes(scene, rng, n), sc._unit(rng, n) * rng.uniform(0.2, 5.0, (n, 1)), rng.uniform(0.01, 0.3, n))


def grazing(scene, n, seed):
    """Some point of the axis passes a point of the surface at a distance of radius * (1 -+ 1e-3), moving across the offset and the
    axis: a hair inside and a hair outside of touching it."""
    rng = np.random.default_rng(seed)
    p, axis = sc._targets(scene, rng, n), _axes(scene, rng, n)
    r = rng.uniform(0.02, 0.2, n)
    other = sc._unit(rng, n)
    off = np.cross(np.where((np.linalg.norm(axis, axis=1) > 0)[:, None], axis, other), sc._unit(rng, n))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    side = np.cross(off, np.where((np.linalg.norm(axis, axis=1) > 0)[:, None], axis, other))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    passing = p + off * (r * np.where(np.arange(n) % 2 == 0, 1 - 1e-3, 1 + 1e-3))[:, None]
    return _pack(_origin_for(passing, axis, rng) - side * rng.uniform(0.5, 3.0, (n, 1)), axis, side * rng.uniform(0.2, 5.0, (n, 1)), r)


def in_contact(scene, n, seed):
    """Starting with some point of the axis within the radius of a point of the surface; every fourth with an axis that pierces a
    triangle's interior with both ends farther than the radius from it."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.05, 0.3, n)
    axis = _axes(scene, rng, n)
    near = sc._targets(scene, rng, n) + sc._unit(rng, n) * (r * rng.uniform(0.0, 0.95, n))[:, None]
    origin = _origin_for(near, axis, rng)
    v0, e1, e2, _ = records(scene, F64)
    k = rng.integers(0, len(v0), n)
    nrm = np.cross(e1[k], e2[k])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    through = v0[k] + e1[k] * 0.3 + e2[k] * 0.3
    lean = nrm + 0.3 * sc._unit(rng, n)
    lean /= np.linalg.norm(lean, axis=1, keepdims=True)
    small = rng.uniform(0.01, 0.03, n)
    reach = small * rng.uniform(3.0, 6.0, n)  # each end this far along the lean: beyond the radius from the plane
    pierce = np.arange(n) % 4 == 3
    origin = np.where(pierce[:, None], through - lean * reach[:, None], origin)
    axis = np.where(pierce[:, None], lean * (2 * reach)[:, None], axis)
    r = np.where(pierce, small, r)
    return _pack(origin, axis, sc._unit(rng, n) * rng.uniform(0.2, 5.0, (n, 1)), r)


def far_outside(scene, n, seed):
    """From 20 to 100 diagonals away, aimed at points of the surface."""
    rng = np.random.default_rng(seed)
    p = sc._targets(scene, rng, n)
    mid = p + sc._unit(rng, n) * (diagonal(scene) * rng.uniform(20.0, 100.0, (n, 1)))
    to = p - mid
    axis = _axes(scene, rng, n)
    return _pack(mid - axis / 2, axis, to / np.linalg.norm(to, axis=1, keepdims=True) * rng.uniform(0.2, 5.0, (n, 1)), rng.uniform(0.01, 0.3, n))


def five_kinds(scene, n, seed):
    """n sweeps: toward surfaces, scattered, grazing, starting in contact, from far outside, a fifth each; within each the axes are
    zero, parallel to an edge, in a triangle's plane, upright and diagonal, a fifth each."""
    q = n // 5
    return np.concatenate([toward_surfaces(scene, q, seed), scattered(scene, q, seed + 1), grazing(scene, q, seed + 2),
                           in_contact(scene, q, seed + 3), far_outside(scene, n - 4 * q, seed + 4)])


def zero_axis(sphere_sweeps):
    """(N, 8) rt_sweep records -> the (N, 12) capsule sweeps with the same origin, radius, direction and tmax and a zero axis."""
    s = np.asarray(sphere_sweeps, F32)
    return _pack(s[:, 0:3], 0.0, s[:, 4:7], s[:, 3], s[:, 7])


def cube_sweeps(seed):
    """1024 sweeps for cornell12, the cube [-1, 1]^3 whose walls share edges and corners: sweep_cases.cube_sweeps' origins, radii
    and directions with axes along a coordinate axis (multiples of 1/8, so that a capsule lying parallel to a wall lands flat on both
    of its triangles and on their shared diagonal), zero, and diagonal.  Ties between neighbouring triangles and starts in contact
    with several walls are what they are for."""
    s = sc.cube_sweeps(seed)
    n = len(s)
    rng = np.random.default_rng(seed + 1000)
    axis = np.zeros((n, 3))
    kind = np.arange(n) % 4
    along = rng.integers(0, 3, n)
    axis[np.arange(n), along] = rng.choice([-0.5, -0.25, -0.125, 0.125, 0.25, 0.5], n)
    axis[kind == 2] = 0.0
    diag = sc._unit(rng, n) * rng.uniform(0.05, 0.5, (n, 1))
    axis = np.where((kind == 3)[:, None], diag, axis)
    return _pack(s[:, 0:3], axis, s[:, 4:7], s[:, 3], s[:, 7])
