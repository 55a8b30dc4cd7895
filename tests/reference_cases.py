"""The reference's legacy (mode 0) and first-hit wavefront (mode 1) pixel, stated independently in float64 numpy, and the cases.

Every other test of the reference-semantics path compares the HIP kernels with oracle/ bit for bit, and both were written by one
reading of the reference's source.  This module is a second reading: each function cites the file:line of the reference's shader
crate (shader/src/...) it restates, and nothing here imports `oracle`, reads its sources or calls the library.  The packed f16
fields are decoded here from their bits.  test_reference_oracle.py runs the cases on the CPU oracle, test_gpu_reference.py on
the HIP kernels; the assertions (`check_frame`, `check_alternatives`, ...) are shared and live at the end of this file.

Rules the statement found worth stating (DESIGN.md section 2 lists them too):
  * ray-gen uses camera.direction as given: right = direction x up, true_up = right x direction, D = direction + right cx +
    true_up cy, then normalised (ray.rs:41-48, wavefront.rs:95-102).  A direction of length k scales `right` by k and `true_up`
    by k^2, so the field of view changes with it;
  * the sphere takes t1 if t1 > 1e-5, else t2, and the normal is (P - C) / |P - C|, outward also from inside (intersection.rs:62-87);
  * a triangle's normal is normalize(e1 x e2) and is never turned toward the ray (intersection.rs:132);
  * a light's range_packed and cone_angles_packed are never read; the spot factor is max(dot(-normalize(direction), l), 0)
    (lighting.rs:132); light types above 2 contribute nothing (lighting.rs:80-86);
  * `.max(0.0)` is Rust's f32::max, which returns the other operand when one is NaN: a zero-length light direction or a point
    light exactly at the hit point (normalize -> NaN) gives that factor 0, not NaN (lighting.rs:104, 129, 132);
  * roughness is decoded nowhere on this path (material.rs:31-33 has no caller in modes 0 / 1);
  * metallic is `f16 > 0.5`, strictly (material.rs:66-68);
  * the transmission is clamped to [0, 1] BEFORE the mix, and the mix divides by (ior - 1): ior = 1 gives -inf / NaN / +inf
    for red / green / blue (lib.rs:323-334, wavefront.rs:197-207);
  * a NaN is stored as byte 0, values outside [0, 1] saturate (Rgba8Unorm store, lib.rs:85-88).
"""
import math
from dataclasses import dataclass, field

import numpy as np

from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import types as T
from gpu_raytracer_amd.scenes import Scene, _Mesh, random_soup

MIN_RAY_DISTANCE = 1e-5                   # RaytracerConfig::MIN_RAY_DISTANCE (intersection.rs:76, 109)
SKY = np.array([0.1, 0.2, 0.3])           # wavefront.rs:148
TRANSMITTED = np.array([0.2, 0.2, 0.3])   # lib.rs:332, wavefront.rs:204
DISPERSION = np.array([-0.018, 0.0, 0.035])   # material.rs:48-53
PRIM_MISS = 0xFFFFFFFF
PRIM_SPHERE = 0x80000000
U32 = 2.0 ** -24                          # unit roundoff of f32

# What leaves a pixel (or a ray) out of the comparison: f32 and float64 may legitimately classify it differently there.
BARY_MARGIN = 1e-5        # a barycentric within this of 0
DISC_MARGIN = 1e-5        # sphere discriminant within this, relative to b^2, of 0
THRESHOLD_MARGIN = 0.01   # |a| or t within 1 % of the 1e-5 thresholds
TIE_MARGIN = 1e-5         # the two nearest candidates' t within this, relative
EDGE_SHARE_CAP = 0.02     # at most this share of a case may be left out (a condition on the case, checked on the CPU)
CLASS_SHARE_MIN = 0.10    # every primitive class a case is about covers at least this share of the frame

F16_REL_TOL = 2.0 ** -10  # point- and spot-lit pixels: one f16 ulp of the attenuation is 2^-11 (as estimator_cases.check_direct_light)

# Largest error of the CPU ORACLE (oracle/rt_oracle.cpp, brute force and BVH, modes 0 and 1) against this statement, measured with
# test_reference_oracle.py (test_measured_constants_are_what_the_oracle_measures prints them) over all cases of each group, on the
# classified pixels, separately for the pixels whose primitive is a sphere ("sphere") and all others ("flat": triangles, misses):
#   rgb: |oracle - statement| / scale over the pixels no point or spot light reaches; `scale` is the sum of the absolute values of
#        the terms the pixel is made of (ambient, each light's contribution, emission, the transmitted colour), which is the pixel
#        itself wherever all terms are positive;
#   t:   |oracle - statement| / statement over the hits.
# The f32 chain is the reference's own operation order, so this is the f32 error of the reference's arithmetic at these scenes.
# On a sphere it is largest near the silhouette, where sqrt(discriminant) cancels; a flat pixel of the same frame is held to the
# flat figure.  The figures are recorded as measured and the bounds are exactly 4 x them, the margin for cases not yet written.
# Neither is ever taken from a HIP result.
MEASURED_RGB_REL = {"raygen": {"flat": 9.069e-08, "sphere": 5.588e-08}, "spheres": {"flat": 9.413e-08, "sphere": 2.593e-05},
                    "triangles": {"flat": 8.011e-08, "sphere": 0.0}, "lights": {"flat": 1.158e-07, "sphere": 3.187e-05},
                    "materials": {"flat": 1.158e-07, "sphere": 3.187e-05}, "store": {"flat": 0.0, "sphere": 2.344e-05}}
# (0.0: the class has no such pixel - no sphere in the triangles group, no flat pixel in the store group that is finite and free of
# f16 light - so that bound is never applied)
MEASURED_T_REL = {"raygen": {"flat": 8.641e-07, "sphere": 5.948e-06}, "spheres": {"flat": 3.357e-07, "sphere": 8.782e-06},
                  "triangles": {"flat": 2.707e-07, "sphere": 0.0}, "lights": {"flat": 2.439e-07, "sphere": 8.782e-06},
                  "materials": {"flat": 2.439e-07, "sphere": 8.782e-06}, "store": {"flat": 2.572e-07, "sphere": 7.232e-06}}
# The ray-query batch below.  The oracle has no entry point for caller-supplied rays and exports no barycentrics, so this
# measurement is the statement's own closest_hit evaluated in float32 (numpy: one IEEE rounding per operation, the reference's
# operation order) against float64, in units of each ray's own conditioning (closest_hit's cond_t / cond_uv: the first-order
# amplification of one rounding, large only for a ray that grazes its triangle or the sphere): |dt| / (t cond_t) and
# |du|, |dv| / cond_uv.  A well-conditioned ray (cond about 2 to 10) is thereby held to about 1e-6, a grazing one to
# proportionally more.  test_ray_query_batch_conditions_and_f32_measurement repeats the measurement.
MEASURED_QUERY_T = 1.207e-07       # largest |dt| / (t * cond_t)
MEASURED_QUERY_UV = 7.594e-08      # largest |du|, |dv| / cond_uv
RGB_REL_BOUND = {g: {k: 4.0 * v for k, v in d.items()} for g, d in MEASURED_RGB_REL.items()}
T_REL_BOUND = {g: {k: 4.0 * v for k, v in d.items()} for g, d in MEASURED_T_REL.items()}
QUERY_T_BOUND = 4.0 * MEASURED_QUERY_T
QUERY_UV_BOUND = 4.0 * MEASURED_QUERY_UV


def f16_decode(bits):
    """The f16 whose bit pattern is the low 16 bits of `bits`, as float64 (spirv_std f16_to_f32; material.rs:27, 37, 62)."""
    return (np.asarray(bits, np.uint32) & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16).astype(np.float64)


def _normalize(v):
    """glam Vec3::normalize: v * (1 / |v|); a zero vector becomes NaN."""
    with np.errstate(all="ignore"):
        return v * (1.0 / np.sqrt((v * v).sum(-1, keepdims=True)))


def _rust_max0(x):
    """f32::max(x, 0.0): NaN gives 0.0."""
    return np.fmax(x, 0.0)


# ------------------------------------------------------------------------------------------------------------------------
# Ray generation: ray.rs:22-53 (mode 0, Ray::new normalises once more, ray.rs:14-19) and wavefront.rs:75-112 (mode 1).
# Both are the same real-number function.
# ------------------------------------------------------------------------------------------------------------------------
def camera_rays(cam, w, h, variant="right"):
    """-> origin (3,), unit directions (h, w, 3).  variant "normalised_forward": the wrong alternative that normalises
    camera.direction before right / true_up / the offsets are formed."""
    px = (np.arange(w, dtype=np.float64) + 0.5) / w                      # ray.rs:27-30
    py = (np.arange(h, dtype=np.float64) + 0.5) / h
    fov_scale = math.tan(float(cam["fov"]) * 0.5 * math.pi / 180.0)      # ray.rs:34
    cx = ((px * 2.0 - 1.0) * (w / h) * fov_scale).reshape(1, w, 1)       # ray.rs:37
    cy = ((1.0 - py * 2.0) * fov_scale).reshape(h, 1, 1)                 # ray.rs:38
    fwd = np.asarray(cam["direction"], np.float64)
    if variant == "normalised_forward":
        fwd = fwd / np.linalg.norm(fwd)
    up = np.asarray(cam["up"], np.float64)
    right = np.cross(fwd, up)                                            # ray.rs:43
    true_up = np.cross(right, fwd)                                       # ray.rs:44
    d = fwd + right * cx + true_up * cy                                  # ray.rs:47
    return np.asarray(cam["position"], np.float64), _normalize(d)        # ray.rs:48


def camera_dir_bound(cam, w, h):
    """Largest absolute f32 error of a component of a camera direction against camera_rays, from the operation count.

    u = 2^-24.  theta = fov / 2 in radians is (fov * 0.5 * PI) / 180: the constant PI and two roundings (0.5 is exact), 3u relative,
    which tan amplifies by kappa = theta (1 + tan^2) / tan = 2 theta / sin(2 theta); tanf itself is within 2 ulp = 4u: fov_scale
    carries (3 kappa + 4) u.  cx: (x + 0.5) / w is two roundings, * 2 - 1 one more (absolute, at magnitude <= 1), * aspect (itself
    one rounding) and * fov_scale two: 6u + fov_scale's.  right = direction x up: three roundings per component; true_up = right x
    direction: three more on top of right's.  right * cx and true_up * cy: one rounding each, the two additions one each.  So every
    component of D is within (6 + 6 + 1 + 2 + 3 kappa + 4) u = (19 + 3 kappa) u of S = |direction| + |right| aspect fov_scale +
    |true_up| fov_scale, the largest magnitude in the chain.  Normalising: the dot is five roundings (2.5u after the square
    root), sqrt, reciprocal and the product three: 6u, twice in mode 0 (Ray::new normalises again, ray.rs:17).  |D| >= |direction|
    because right and true_up are orthogonal to it.  Bound: ((19 + 3 kappa) S / |direction| + 12) u."""
    theta = float(cam["fov"]) * 0.5 * math.pi / 180.0
    kappa = 2.0 * theta / abs(math.sin(2.0 * theta))
    f = abs(math.tan(theta))
    fwd, up = np.asarray(cam["direction"], np.float64), np.asarray(cam["up"], np.float64)
    right = np.cross(fwd, up)
    true_up = np.cross(right, fwd)
    s = np.linalg.norm(fwd) + np.linalg.norm(right) * (w / h) * f + np.linalg.norm(true_up) * f
    return ((19.0 + 3.0 * kappa) * s / np.linalg.norm(fwd) + 12.0) * U32


# ------------------------------------------------------------------------------------------------------------------------
# Closest hit: intersection.rs:52-87 (sphere), :91-138 (Moeller-Trumbore), lib.rs:174-296 (spheres first, each list in index
# order with a strict `t < closest`, the triangle list starting from the sphere's t).
# ------------------------------------------------------------------------------------------------------------------------
def _scene_arrays(scene):
    p = scene.vertices["position"].astype(np.float64)
    tr = scene.triangles
    v0, v1, v2 = p[tr["v0_index"]], p[tr["v1_index"]], p[tr["v2_index"]]
    return v0, v1, v2, tr["material_id"].astype(np.int64)


def closest_hit(scene, o, d, tmin=MIN_RAY_DISTANCE, tmax=np.inf, variant="right", chunk=1024, dtype=np.float64):
    """Rays o, d (N, 3) (d as the caller gives it: not normalised here) -> dict of (N,) arrays: prim (project encoding), t, u, v,
    point (N, 3), normal (N, 3), mat, unsure.  tmin / tmax: scalars or (N,); the acceptance is tmin < t < tmax, strictly
    (intersection.rs:78, 130 with tmin = 1e-5).  variant "t1_always": the wrong alternative that never falls back to t2.
    dtype=np.float32 evaluates the same formulas with one f32 rounding per operation: used only to MEASURE what f32 costs where
    the oracle exports nothing to compare with (the barycentrics of the ray queries)."""
    o, d = np.asarray(o, dtype).reshape(-1, 3), np.asarray(d, dtype).reshape(-1, 3)
    n = len(d)
    o = np.broadcast_to(o, (n, 3))
    tmin, tmax = np.broadcast_to(np.asarray(tmin, dtype), (n,)), np.broadcast_to(np.asarray(tmax, dtype), (n,))
    out = {k: [] for k in ("prim", "t", "u", "v", "normal", "mat", "unsure", "cond_t", "cond_uv")}
    for s0 in range(0, n, chunk):
        r = _closest_hit_chunk(scene, o[s0:s0 + chunk], d[s0:s0 + chunk], tmin[s0:s0 + chunk], tmax[s0:s0 + chunk], variant, dtype)
        for k in out:
            out[k].append(r[k])
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["point"] = o + d * np.where(np.isfinite(out["t"]), out["t"], 0.0)[:, None]     # ray.rs:56-58
    return out


def _closest_hit_chunk(scene, o, d, tmin, tmax, variant, dtype):
    n = len(d)
    v0, v1, v2, tri_mat = _scene_arrays(scene)
    v0, v1, v2 = v0.astype(dtype), v1.astype(dtype), v2.astype(dtype)
    nt, ns = len(v0), len(scene.spheres)
    # candidates: spheres first, then triangles; t = inf where the primitive is not hit
    cand_t = np.full((n, ns + nt), np.inf, dtype)
    unsure = np.zeros(n, bool)
    sph_cond = np.ones((n, max(ns, 1)))
    with np.errstate(all="ignore"):
        for i, sp in enumerate(scene.spheres):
            c, r = sp["center"].astype(dtype), dtype(sp["radius"])
            oc = o - c                                                    # intersection.rs:62
            a = (d * d).sum(-1)                                           # :63
            b = 2.0 * (oc * d).sum(-1)                                    # :64
            cc = (oc * oc).sum(-1) - r * r                                # :65
            disc = b * b - 4.0 * a * cc                                   # :66
            sq = np.sqrt(np.maximum(disc, 0.0))                           # :72
            t1 = (-b - sq) / (2.0 * a)                                    # :73
            t2 = (-b + sq) / (2.0 * a)                                    # :74
            t = t1 if variant == "t1_always" else np.where(t1 > tmin, t1, t2)   # :76
            ok = (disc >= 0.0) & (t > tmin)                               # :68, :78
            cand_t[:, i] = np.where(ok, t, np.inf)
            # first-order f32 error of t in units of eps * t: b carries eps |oc| |d|, the discriminant eps (b^2 + 4 a (|oc|^2 + r^2)),
            # which the square root divides by 2 sqrt(disc)
            oc_n, d_n = np.sqrt((oc * oc).sum(-1)), np.sqrt(a)
            sph_cond[:, i] = (2.0 * oc_n * d_n + (b * b + 4.0 * a * (oc_n * oc_n + r * r)) / (2.0 * sq)) / (2.0 * a * np.abs(t))
            near_disc = np.abs(disc) < DISC_MARGIN * b * b
            near_min = (disc >= 0.0) & ((np.abs(t1 - tmin) < THRESHOLD_MARGIN * tmin) | (np.abs(t2 - tmin) < THRESHOLD_MARGIN * tmin))
            unsure |= near_disc | near_min
        if nt:
            e1, e2 = (v1 - v0)[None], (v2 - v0)[None]                     # :104-105
            dd, oo = d[:, None, :], o[:, None, :]
            hh = np.cross(dd, e2)                                         # :106
            a = (e1 * hh).sum(-1)                                         # :107
            ok = ~(np.abs(a) < MIN_RAY_DISTANCE)                          # :109
            f = 1.0 / a                                                   # :113
            s = oo - v0[None]                                             # :114
            u = f * (s * hh).sum(-1)                                      # :115
            q = np.cross(s, e1)                                           # :121
            v = f * (dd * q).sum(-1)                                      # :122
            t = f * (e2 * q).sum(-1)                                      # :128
            inside = ~((u < 0.0) | (u > 1.0)) & ~((v < 0.0) | (u + v > 1.0))    # :117, :124
            tm = tmin[:, None]
            hit = ok & inside & (t > tm)                                  # :130
            cand_t[:, ns:] = np.where(hit, t, np.inf)
            tri_u, tri_v, tri_a = u, v, a
            edge = np.abs(np.minimum(np.minimum(u, v), 1.0 - u - v)) < BARY_MARGIN      # the barycentric that decides in / out
            relevant = np.isfinite(t) & (t > 0.0) & (np.abs(a) > 0.5 * MIN_RAY_DISTANCE)
            near_a = np.abs(np.abs(a) - MIN_RAY_DISTANCE) < THRESHOLD_MARGIN * MIN_RAY_DISTANCE
            near_min = ok & inside & (np.abs(t - tm) < THRESHOLD_MARGIN * tm)
            unsure |= (edge & relevant).any(1) | (near_a & np.isfinite(t)).any(1) | near_min.any(1)
    with np.errstate(all="ignore"):   # a range that ends within TIE_MARGIN of a candidate (ray queries): `t < tmax` may go either way
        unsure |= (np.isfinite(cand_t) & np.isfinite(tmax[:, None]) & (np.abs(cand_t - tmax[:, None]) <= TIE_MARGIN * tmax[:, None])).any(1)
    in_range = cand_t < tmax[:, None]
    cand_t = np.where(in_range, cand_t, np.inf)
    rows = np.arange(n)
    # lowest index among equal t: lib.rs:262, 288 replace the closest only on a strict `t < closest`
    if ns:
        js = np.argmin(cand_t[:, :ns], 1)
        ts = cand_t[rows, js]
    else:
        js, ts = np.zeros(n, np.int64), np.full(n, np.inf)
    if nt:
        jt = np.argmin(cand_t[:, ns:], 1)
        tt = cand_t[rows, ns + jt]
    else:
        jt, tt = np.zeros(n, np.int64), np.full(n, np.inf)
    use_tri = tt < ts                                                     # lib.rs:186-189: triangles start from the sphere's t
    t = np.where(use_tri, tt, ts)
    hit = np.isfinite(t)
    prim = np.where(hit, np.where(use_tri, jt, PRIM_SPHERE | js), PRIM_MISS).astype(np.uint32)
    # the two nearest candidates, unless the runner-up is the very same triangle stored again (its f32 t is then bit-equal)
    if ns + nt > 1:
        part = np.partition(cand_t, 1, axis=1)
        with np.errstate(all="ignore"):
            tied = np.abs(cand_t - t[:, None]) <= TIE_MARGIN * np.abs(t[:, None])
            close = np.isfinite(part[:, 1]) & (np.abs(part[:, 1] - part[:, 0]) <= TIE_MARGIN * np.abs(part[:, 0]))
        if close.any() and nt:
            key = np.concatenate([v0, v1, v2], 1).astype(np.float32)
            _, canon = np.unique(key, axis=0, return_inverse=True)
            canon = canon.reshape(-1)
            tied_tri = tied[:, ns:]
            all_same = np.where(tied_tri, canon[None, :], -1).max(1) == np.where(tied_tri, canon[None, :], len(canon)).min(1)
            close &= ~(all_same & ~tied[:, :ns].any(1))
        unsure |= close
    normal = np.zeros((n, 3))
    mat = np.zeros(n, np.int64)
    uu, vv = np.zeros(n), np.zeros(n)
    cond_t, cond_uv = np.ones(n), np.ones(n)
    with np.errstate(all="ignore"):
        if ns:
            sc = scene.spheres["center"].astype(dtype)[js]
            pt = o + d * np.where(hit, t, 0.0)[:, None]
            n_s = _normalize(pt - sc)                                     # intersection.rs:80
            sel = hit & ~use_tri
            normal[sel] = n_s[sel]
            mat[sel] = scene.spheres["material_id"].astype(np.int64)[js][sel]
            cond_t[sel] = sph_cond[rows, js][sel]
        if nt:
            n_t = _normalize(np.cross(v1 - v0, v2 - v0))[jt]              # :132
            sel = hit & use_tri
            normal[sel] = n_t[sel]
            mat[sel] = tri_mat[jt][sel]
            uu[sel], vv[sel] = tri_u[rows, jt][sel], tri_v[rows, jt][sel]
            # first-order f32 error of Moeller-Trumbore in units of eps: every numerator is a triple product of s (or e1), d and
            # an edge, divided by a; g = |d| |e1| |e2| / |a| is 1 / (sine of the grazing angle x sine of the edges' angle)
            e1_n, e2_n = (np.linalg.norm(x, axis=-1)[jt] for x in (v1 - v0, v2 - v0))
            s_n, d_n = np.linalg.norm(o - v0[jt], axis=-1), np.linalg.norm(d, axis=-1)
            g = d_n * e1_n * e2_n / np.abs(tri_a[rows, jt])
            cond_uv[sel] = (g * (1.0 + s_n / np.minimum(e1_n, e2_n)))[sel]          # absolute error of u, v
            cond_t[sel] = (g * (1.0 + s_n / (np.abs(t) * d_n)))[sel]                # relative error of t
    return {"prim": prim, "t": t, "u": uu, "v": vv, "normal": normal, "mat": mat, "unsure": unsure, "cond_t": cond_t, "cond_uv": cond_uv}


# ------------------------------------------------------------------------------------------------------------------------
# Shading: lighting.rs:20-139, material.rs:16-83, lib.rs:300-338 (mode 0) and wavefront.rs:168-211 (mode 1, throughput 1).
# ------------------------------------------------------------------------------------------------------------------------
def _material_fields(scene, variant):
    m = scene.materials
    mr, it = m["metallic_roughness_f16"].astype(np.uint32), m["ior_transmission_f16"].astype(np.uint32)
    metallic = f16_decode(mr >> np.uint32(16) if variant == "metallic_roughness_swapped" else mr)          # material.rs:27
    if variant == "ior_transmission_swapped":
        ior, trans = f16_decode(it >> np.uint32(16)), f16_decode(it)
    else:
        ior, trans = f16_decode(it), f16_decode(it >> np.uint32(16))                                         # material.rs:37, 62
    return m["albedo"].astype(np.float64), m["emission"].astype(np.float64), metallic, ior, trans


def shade(scene, hit, variant="right"):
    """The colour of every hit in all three channels -> dict: rgb (N, 3) (component c from the channel-c pass), scale (N, 3) (sum
    of the absolute terms, see MEASURED_RGB_REL), f16 (N,) bool: a point or spot light of positive intensity faces the hit (its f16 attenuation may enter)."""
    n = len(hit["t"])
    albedo_m, emission_m, metallic_m, ior_m, trans_m = _material_fields(scene, variant)
    n_mat = len(scene.materials)
    valid = hit["mat"] < n_mat                                            # lib.rs:307
    mid = np.where(valid, hit["mat"], 0)
    albedo, emission = albedo_m[mid], emission_m[mid]
    is_metal = (metallic_m[mid] > 0.5)[:, None]                           # material.rs:66-68
    nrm, pt = hit["normal"], hit["point"]
    total = albedo * 0.1                                                  # lighting.rs:30
    scale = np.abs(total)
    f16_lit = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for li in scene.lights:                                           # lighting.rs:34, index order
            lpos, ldir = li["position"].astype(np.float64), li["direction"].astype(np.float64)
            lint, lcol, ltype = float(li["intensity"]), li["color"].astype(np.float64), int(li["light_type"])
            ndir = _normalize(ldir)
            directional = _rust_max0((nrm * -ndir).sum(-1)) * lint        # lighting.rs:103-104
            to_light = lpos - pt                                          # :120
            dist = np.sqrt((to_light * to_light).sum(-1))                 # :121
            l = _normalize(to_light)                                      # :122
            att = 1.0 / (1.0 + dist * dist * 0.01)                        # :125
            if variant != "attenuation_not_f16":
                att = att.astype(np.float32).astype(np.float16).astype(np.float64)   # :126-127
            point = _rust_max0((nrm * l).sum(-1)) * lint * att            # :129
            spot_dir = ndir if variant == "spot_plus_direction" else -ndir
            spot = point * _rust_max0((l * spot_dir).sum(-1))             # :132-133
            is_dir, is_point, is_spot = ltype == 0, ltype == 1, ltype == 2
            if variant.startswith("type_3_as_") and ltype > 2:           # the wrong alternatives: a select that falls through
                is_dir, is_point, is_spot = (variant == "type_3_as_" + k for k in ("directional", "point", "spot"))
            final = directional * float(is_dir) + point * float(is_point) + spot * float(is_spot)   # :80-86
            brdf = np.where(is_metal, albedo * final[:, None] * 0.5, albedo / math.pi * final[:, None])     # material.rs:76-83
            ok = (final > 0.0).astype(np.float64)[:, None]                # lighting.rs:92
            contrib = brdf * lcol * ok                                    # :93
            total = total + contrib                                       # :42
            scale = scale + np.abs(np.nan_to_num(contrib, nan=0.0, posinf=0.0, neginf=0.0))
            if ltype in (1, 2) and lint > 0.0:   # where f32 may see the light although float64 has it at exactly 0 (a grazing N . l)
                facing = np.nan_to_num((nrm * l).sum(-1), nan=-1.0) > -1e-4
                if ltype == 2:
                    facing &= np.nan_to_num((l * spot_dir).sum(-1), nan=-1.0) > -1e-4
                f16_lit |= facing
        total = total + emission                                          # :46
        scale = scale + np.abs(emission)
        trans = trans_m[mid]
        tf = np.fmin(np.fmax(trans, 0.0), 1.0)                            # lib.rs:323
        ior = ior_m[mid]
        disp = (ior[:, None] + DISPERSION[None, :] - 1.0) / (ior[:, None] - 1.0)     # material.rs:57, lib.rs:331; channel c in column c
        if variant == "dispersion_red_blue_swapped":
            disp = disp[:, ::-1]
        transmitted = TRANSMITTED[None, :] * disp                         # lib.rs:332: component c of the channel-c pass
        if variant == "clamp_after_mix":
            raw = trans[:, None]
            mixed = np.clip(total * (1.0 - raw) + transmitted * raw, 0.0, 1.0)
            mix_on = (trans > 0.0)[:, None]
        else:
            mixed = total * (1.0 - tf[:, None]) + transmitted * tf[:, None]          # lib.rs:334
            mix_on = (tf > 0.0)[:, None]                                  # lib.rs:326
        rgb = np.where(mix_on, mixed, total)
        scale = np.where(mix_on, scale * np.abs(1.0 - tf[:, None]) + np.abs(np.nan_to_num(transmitted, nan=0.0, posinf=0.0, neginf=0.0)) * tf[:, None], scale)
    magenta = np.array([1.0, 0.0, 1.0])                                   # lib.rs:308
    rgb = np.where(valid[:, None], rgb, magenta)
    scale = np.where(valid[:, None], scale, magenta)
    f16_lit &= valid
    return {"rgb": rgb, "scale": scale, "f16": f16_lit}


def to_unorm8(x):
    """Rgba8Unorm store of a float: NaN -> 0, clamp to [0, 1], scale by 255, round to nearest."""
    x = np.where(np.isnan(x), 0.0, x)
    return np.floor(np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def pixel_statement(scene, cam, w, h, mode, variant="right"):
    """The frame: dict prim (h, w) uint32, t (h, w) (inf on a miss), rgb (h, w, 3), scale (h, w, 3), f16 (h, w), bytes (h, w, 3),
    channels (3 x (h, w, 4)), combined (h, w, 4), unsure (h, w), rays (origin, directions)."""
    o, d = camera_rays(cam, w, h, variant)
    hit = closest_hit(scene, o, d.reshape(-1, 3), variant=variant)
    sh = shade(scene, hit, variant)
    is_hit = hit["prim"] != PRIM_MISS
    miss = SKY if mode == 1 else np.zeros(3)                              # wavefront.rs:146-151 / lib.rs:77
    rgb = np.where(is_hit[:, None], sh["rgb"], miss)
    scale = np.where(is_hit[:, None], sh["scale"], miss)
    by = to_unorm8(rgb).reshape(h, w, 3)
    chans = []
    for c in range(3):                                                    # lib.rs:342-349 and the alpha of :85
        img = np.zeros((h, w, 4), np.uint8)
        img[..., c], img[..., 3] = by[..., c], 255
        chans.append(img)
    comb = np.zeros((h, w, 4), np.uint8)                                  # main_fs, lib.rs:383-388
    comb[..., :3], comb[..., 3] = by, 255
    return {"prim": hit["prim"].reshape(h, w), "t": hit["t"].reshape(h, w), "rgb": rgb.reshape(h, w, 3),
            "scale": scale.reshape(h, w, 3), "f16": (sh["f16"] & is_hit).reshape(h, w), "bytes": by, "channels": chans,
            "combined": comb, "unsure": hit["unsure"].reshape(h, w), "rays": (o, d)}


# ------------------------------------------------------------------------------------------------------------------------
# Cases
# ------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    group: str
    scene: Scene
    w: int
    h: int
    classes: tuple                      # primitive classes the case is about: "sphere", "triangle", "miss", or a prim id
    asserted: tuple = ()                # wrong alternatives that must differ on more than half of the classified pixels
    printed: tuple = ()                 # wrong alternatives that are only printed (inside the tolerance)
    twin: Scene = None                  # a second upload whose frames must carry the same bits
    duplicates: tuple = ()              # triangle ids that are one triangle stored several times (lowest index wins)
    info: dict = field(default_factory=dict)

    @property
    def camera(self):
        return self.scene.camera


def _mat(albedo, metallic=0.0, roughness=1.0, emission=(0, 0, 0), ior=1.5, transmission=0.0, metallic_bits=None):
    m = H.material_new(albedo, metallic, roughness, emission, ior, transmission)
    if metallic_bits is not None:
        m["metallic_roughness_f16"] = (int(m["metallic_roughness_f16"]) & 0xFFFF0000) | metallic_bits
    return m


def _scene(name, tris, spheres, materials, lights, cam):
    """tris: [(v0, v1, v2, material)], spheres: [(center, radius, material)]."""
    mesh = _Mesh()
    for v0, v1, v2, m in tris:
        mesh.add([v0, v1, v2], [(0, 1, 2)], m)
    vertices, triangles = mesh.finish()
    sp = np.array(list(spheres), dtype=T.SPHERE) if len(spheres) else np.zeros(0, T.SPHERE)
    li = np.array(list(lights), dtype=T.LIGHT) if len(lights) else np.zeros(0, T.LIGHT)
    return Scene(name, sp, li, vertices, triangles, np.array(list(materials), dtype=T.MATERIAL), cam)


def _quad_tris(a, b, c, d, m):
    return [(a, b, c, m), (a, c, d, m)]


STAGE_CAM = dict(position=(0.13, 0.21, 2.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=60.0)
PLANE_Z = -3.0
# the wall z = -3 facing the camera (normal +z); its diagonal runs from (-9, -7) to (9, 8), off the frame's centre
PLANE = _quad_tris((-9.0, -7.0, PLANE_Z), (9.0, -7.0, PLANE_Z), (9.0, 8.0, PLANE_Z), (-9.0, 8.0, PLANE_Z), 0)
BALL = ((0.0, 0.0, -1.5), 1.0, 1)
PLANE_RHO, BALL_RHO = (0.7, 0.5, 0.3), (0.3, 0.6, 0.8)


def stage(name, group, lights, plane_mat=None, ball_mat=None, w=64, h=48, cam=None, twin_lights=None, twin_mats=None, ball=BALL,
          n_materials=None, **kw):
    """A wall of material 0 behind a ball of material 1, seen from in front: the ball covers about 14 % of the frame."""
    mats = [plane_mat if plane_mat is not None else _mat(PLANE_RHO), ball_mat if ball_mat is not None else _mat(BALL_RHO)]
    mats = mats[:n_materials] if n_materials else mats
    cam = H.camera(**(cam or STAGE_CAM))
    scene = _scene(name, PLANE, [ball], mats, lights, cam)
    twin = None
    if twin_lights is not None or twin_mats is not None:
        twin = _scene(name + "_twin", PLANE, [ball], twin_mats if twin_mats is not None else mats,
                      twin_lights if twin_lights is not None else lights, cam)
    return Case(name, group, scene, w, h, ("sphere", "triangle"), twin=twin, **kw)


SUN = H.light_directional((0.3, -0.5, -1.0), (1.0, 0.9, 0.8), 1.5)
LAMP_POS = (1.5, 2.0, 1.0)
LAMP = H.light_point(LAMP_POS, (0.9, 1.0, 0.8), 3.0)


def _spot(rng, inner, outer, direction=(-0.3, -0.4, -1.0), intensity=4.0):
    return H.light_spot(LAMP_POS, direction, (1.0, 0.8, 0.9), intensity, rng, inner, outer)


def _half_plane_scene(name, fov, w, h):
    """A wall z = -3 that ends at a slanted edge through the view's middle, sized to the field of view so that the margin of
    1e-5 in its barycentrics stays far below a pixel: half of the frame hits, half misses, at every fov."""
    half = 5.0 * math.tan(math.radians(fov / 2)) * max(w / h, 1.0)
    s = 4.0 * half
    e = 0.07 * half
    tris = [((-s, -s, PLANE_Z), (e - 0.1 * s, -s, PLANE_Z), (e + 0.1 * s, s, PLANE_Z), 0), ((-s, -s, PLANE_Z), (e + 0.1 * s, s, PLANE_Z), (-s, s, PLANE_Z), 0)]
    cam = H.camera((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), fov)
    return _scene(name, tris, [], [_mat(PLANE_RHO, emission=(0.1, 0.0, 0.2))], [SUN], cam)


def _cases():
    c = []
    # ---- ray generation ------------------------------------------------------------------------------------------------
    for fov, (w, h) in ((1.0, (64, 48)), (45.0, (50, 38)), (120.0, (40, 24)), (170.0, (64, 48))):
        c.append(Case(f"raygen_fov{int(fov)}", "raygen", _half_plane_scene(f"half_plane_fov{int(fov)}", fov, w, h), w, h, ("triangle", "miss")))
    long_cam = dict(position=(0.13, 0.21, 2.0), direction=(0.1 * 2.5 / math.sqrt(1.01), 0.0, -2.5 / math.sqrt(1.01)), up=(0.3, 1.7, -0.4), fov=25.0)
    c.append(stage("raygen_long_direction", "raygen", [LAMP], cam=long_cam, w=50, h=38, asserted=("normalised_forward",),
                   ball=((0.3, 0.0, -1.5), 1.0, 1)))
    # ---- spheres ---------------------------------------------------------------------------------------------------------
    two = _scene("two_spheres", [], [((0.5, 0.1, -3.0), 1.4, 0), ((-0.5, -0.2, -1.0), 0.8, 1)], [_mat(PLANE_RHO), _mat(BALL_RHO)], [SUN], H.camera(**STAGE_CAM))
    c.append(Case("spheres_reverse_depth_order", "spheres", two, 50, 38, (PRIM_SPHERE | 0, PRIM_SPHERE | 1, "miss")))
    inside = _scene("inside_sphere", [], [((0.0, 0.0, 0.0), 3.0, 0)], [_mat(PLANE_RHO)], [H.light_directional((0.2, 0.3, 1.0), (1.0, 1.0, 0.9), 1.2)],
                    H.camera((0.4, -0.3, 0.5), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 70.0))
    c.append(Case("sphere_from_inside", "spheres", inside, 64, 48, ("sphere",), asserted=("t1_always",)))
    front_back = _scene("triangle_front_and_behind", [((-2.5, -1.8, -0.2), (0.4, -1.5, -0.2), (-1.0, 1.9, -0.4), 0),
                                                      ((-0.5, -3.0, -4.0), (6.0, -2.5, -4.0), (2.5, 4.0, -3.5), 2)], [BALL],
                        [_mat(PLANE_RHO), _mat(BALL_RHO), _mat((0.5, 0.8, 0.2))], [SUN], H.camera(**STAGE_CAM))
    c.append(Case("sphere_between_two_triangles", "spheres", front_back, 64, 48, (0, 1, "sphere", "miss")))
    # ---- triangles -------------------------------------------------------------------------------------------------------
    left = ((-3.0, -2.0, -2.0), (-0.1, -2.0, -2.0), (-1.5, 2.2, -2.0), 0)          # e1 x e2 faces +z: toward the camera
    right = ((0.1, -2.0, -2.0), (1.6, 2.2, -2.0), (3.1, -2.0, -2.0), 1)            # wound the other way: faces -z
    for where, direction in (("front", (0.2, -0.3, -1.0)), ("behind", (0.2, -0.3, 1.0))):
        s = _scene(f"windings_light_{where}", [left, right], [], [_mat(PLANE_RHO), _mat(BALL_RHO)],
                   [H.light_directional(direction, (1.0, 0.9, 0.8), 1.5)], H.camera(**STAGE_CAM))
        c.append(Case(f"triangle_windings_light_{where}", "triangles", s, 50 if where == "front" else 64, 38 if where == "front" else 48, (0, 1, "miss")))
    dup = ((-2.6, -2.0, -2.0), (2.9, -1.9, -2.0), (0.2, 2.3, -2.5))
    s = _scene("coplanar_duplicates", [(*dup, 1), (*dup, 0), (*dup, 2), ((-8.0, -6.0, -5.0), (8.0, -6.0, -5.0), (0.0, 9.0, -5.0), 2)], [],
               [_mat(PLANE_RHO), _mat(BALL_RHO), _mat((0.5, 0.8, 0.2))], [SUN], H.camera(**STAGE_CAM))
    c.append(Case("triangle_coplanar_duplicates", "triangles", s, 64, 48, (0, 3), duplicates=(0, 1, 2)))
    # ---- lights ----------------------------------------------------------------------------------------------------------
    c.append(stage("light_directional", "lights", [SUN], w=50, h=38))
    c.append(stage("light_point", "lights", [LAMP], printed=("attenuation_not_f16",)))
    c.append(stage("light_spot", "lights", [_spot(20.0, 0.3, 0.5)], twin_lights=[_spot(0.5, 1.2, 0.1)], asserted=("spot_plus_direction",)))
    # types 3 and 0xFFFFFFFF, each with a position AND a direction that would light the wall and the ball as a directional, a point
    # and a spot light alike: a select that falls through to any of the three (`>= 2`, `== 0 || == 3`, an else branch) shows
    other, last = _spot(20.0, 0.3, 0.5), _spot(20.0, 0.3, 0.5, direction=(0.3, -0.5, -1.0))
    other["light_type"], last["light_type"] = 3, 0xFFFFFFFF
    c.append(stage("light_type_3", "lights", [other, last], w=50, h=38,
                   asserted=("type_3_as_directional", "type_3_as_point", "type_3_as_spot")))
    c.append(stage("light_negative_intensity", "lights", [H.light_directional((0.3, -0.5, -1.0), (1.0, 0.9, 0.8), -1.5), H.light_point(LAMP_POS, (1, 1, 1), -2.0)]))
    c.append(stage("light_negative_colour", "lights", [H.light_directional((0.3, -0.5, -1.0), (-0.2, 0.4, -0.1), 1.5)]))
    zero = (0.0, 0.0, 0.0)
    zd = H.light_directional(zero, (1.0, 0.9, 0.8), 1.5)
    zp = H.light_point(LAMP_POS, (0.9, 1.0, 0.8), 3.0)     # hostpack gives a point light the direction (0, 0, 0) anyway
    zs = _spot(20.0, 0.3, 0.5, direction=zero)
    c.append(stage("light_zero_direction_directional", "lights", [zd], w=50, h=38))
    c.append(stage("light_zero_direction_point", "lights", [zp], w=50, h=38))
    c.append(stage("light_zero_direction_spot", "lights", [zs], w=50, h=38))
    # a point light ON the wall, exactly at the hit point of a pixel centre's ray where f32 allows it: the wall sees it at a right
    # angle (N . l = 0), the hit point itself normalises a zero vector
    c.append(stage("light_at_a_hit_point", "lights", [H.light_point((0.13, 0.21, PLANE_Z), (0.9, 1.0, 0.8), 3.0)], cam=dict(STAGE_CAM, position=(0.13, 0.21, 2.0)),
                   w=49, h=37, ball=((1.2, 0.9, -1.5), 1.0, 1)))
    c.append(stage("lights_two", "lights", [SUN, LAMP]))
    c.append(stage("lights_three", "lights", [_spot(20.0, 0.3, 0.5), SUN, LAMP], w=50, h=38))
    # ---- materials -------------------------------------------------------------------------------------------------------
    c.append(stage("metallic_exactly_half", "materials", [SUN], _mat(PLANE_RHO, roughness=1.0, metallic_bits=0x3800), _mat(BALL_RHO, roughness=1.0, metallic_bits=0x3800),
                   asserted=("metallic_roughness_swapped",)))
    c.append(stage("metallic_next_above_half", "materials", [SUN], _mat(PLANE_RHO, roughness=0.0, metallic_bits=0x3801), _mat(BALL_RHO, roughness=0.0, metallic_bits=0x3801),
                   twin_mats=[_mat(PLANE_RHO, roughness=1.0, metallic_bits=0x3801), _mat(BALL_RHO, roughness=0.7, metallic_bits=0x3801)],
                   asserted=("metallic_roughness_swapped",), w=50, h=38))
    c.append(stage("roughness_unused_dielectric", "materials", [SUN, LAMP], _mat(PLANE_RHO, roughness=0.1), _mat(BALL_RHO, roughness=0.2),
                   twin_mats=[_mat(PLANE_RHO, roughness=0.9), _mat(BALL_RHO, roughness=0.4)]))
    c.append(stage("emission_after_lights", "materials", [SUN], _mat(PLANE_RHO, emission=(0.05, 0.2, 0.1)), _mat(BALL_RHO, emission=(0.3, 0.1, 0.2)), w=50, h=38))
    for label, tr in (("negative", -0.5), ("quarter", 0.25), ("one", 1.0), ("two", 2.0)):
        kw = {"quarter": dict(asserted=("dispersion_red_blue_swapped", "ior_transmission_swapped")), "two": dict(asserted=("clamp_after_mix",))}.get(label, {})
        c.append(stage(f"transmission_{label}", "materials", [SUN], _mat(PLANE_RHO, ior=1.33, transmission=tr), _mat(BALL_RHO, ior=1.5, transmission=tr),
                       w=50 if label in ("negative", "one") else 64, h=38 if label in ("negative", "one") else 48, **kw))
    c.append(stage("material_id_equal_to_count", "materials", [SUN], n_materials=1))
    # ---- store and combine -----------------------------------------------------------------------------------------------
    c.append(stage("store_saturation_and_nan", "store", [SUN], _mat(PLANE_RHO, ior=1.0, transmission=0.25), _mat(BALL_RHO, emission=(3.0, 3.0, 3.0)), w=50, h=38))
    c.append(stage("tile_edge_130x70", "store", [SUN, LAMP], _mat(PLANE_RHO, emission=(0.05, 0.2, 0.1)), w=130, h=70, cam=dict(STAGE_CAM, fov=40.0)))
    return c


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
GROUPS = ("raygen", "spheres", "triangles", "lights", "materials", "store")

_STATEMENTS = {}


def statement(case, mode, variant="right"):
    """pixel_statement of a case, computed once per (case, mode, variant) and never modified."""
    key = (case.name, mode, variant)
    if key not in _STATEMENTS:
        _STATEMENTS[key] = pixel_statement(case.scene, case.camera, case.w, case.h, mode, variant)
    return _STATEMENTS[key]


def padded(case, n_triangles=1024):
    """The case's scene with far-away small triangles appended (behind the camera, 500 units off) up to n_triangles: the
    frame is the same, the tree builders get a scene large enough for the device build."""
    s = case.scene
    extra = n_triangles - len(s.triangles)
    k = np.arange(extra, dtype=np.float64)
    base = np.stack([500.0 + (k % 32) * 1.5, -20.0 + (k // 32) * 1.5, 400.0 + (k % 7)], 1)
    verts = np.stack([base, base + [1.0, 0.0, 0.0], base + [0.0, 1.0, 0.2]], 1).reshape(-1, 3)
    va = np.zeros(len(s.vertices) + len(verts), T.VERTEX)
    va["position"][:len(s.vertices)] = s.vertices["position"]
    va["position"][len(s.vertices):] = verts
    ta = np.zeros(len(s.triangles) + extra, T.TRIANGLE)
    ta[:len(s.triangles)] = s.triangles
    idx = len(s.vertices) + np.arange(extra * 3).reshape(-1, 3)
    ta["v0_index"][len(s.triangles):], ta["v1_index"][len(s.triangles):], ta["v2_index"][len(s.triangles):] = idx[:, 0], idx[:, 1], idx[:, 2]
    return Scene(s.name + "_padded", s.spheres, s.lights, va, ta, s.materials, s.camera)


# ------------------------------------------------------------------------------------------------------------------------
# Ray-query batch: 4,096 rays around a 300-triangle soup with three spheres, plus the camera rays of one case (light_directional:
# its 50 x 38 pixel-centre rays look into the soup from (0.13, 0.21, 2)).
# ------------------------------------------------------------------------------------------------------------------------
QUERY_RAYS = 4096


def query_scene():
    return random_soup(300, seed=3, size=0.5, n_spheres=3, n_lights=1)


def query_rays(scene, n=QUERY_RAYS, seed=20):
    """-> (N, 8) float32 batch (ox oy oz tmin dx dy dz tmax): n rays, a quarter aimed at triangle interiors, a quarter toward the
    spheres from nearby (some from inside), a quarter random with directions that are not unit, a quarter random unit; then the
    camera rays of the case light_directional."""
    rng = np.random.default_rng(seed)
    v0, v1, v2, _ = _scene_arrays(scene)
    k = n // 4
    o = rng.uniform(-4, 4, (n, 3)) + [0, 0, -2]
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ti = rng.integers(0, len(v0), k)
    wts = rng.dirichlet([2, 2, 2], k)
    d[:k] = _normalize((v0[ti] * wts[:, :1] + v1[ti] * wts[:, 1:2] + v2[ti] * wts[:, 2:3]) - o[:k])
    sp = scene.spheres[rng.integers(0, len(scene.spheres), k)]            # the second quarter: toward the spheres, some past them
    aim = sp["center"].astype(np.float64) + rng.uniform(-1, 1, (k, 3)) * 0.8 * sp["radius"].astype(np.float64)[:, None]
    o[k:2 * k] = aim + _normalize(rng.standard_normal((k, 3))) * rng.uniform(0.1, 2.5, (k, 1))
    d[k:2 * k] = _normalize(aim - o[k:2 * k])
    d[2 * k:3 * k] *= rng.uniform(0.05, 20, (k, 1))
    case = CASE_BY_NAME["light_directional"]
    co, cd = camera_rays(case.camera, case.w, case.h)
    cd = cd.reshape(-1, 3)
    o, d = np.concatenate([o, np.broadcast_to(co, cd.shape)]), np.concatenate([d, cd])
    rays = np.empty((len(o), 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, MIN_RAY_DISTANCE, d, np.finfo(np.float32).max
    return rays


_QUERY = {}


def query_statement():
    """(scene, rays, closest hits of the rays as the f32 batch holds them), computed once."""
    if not _QUERY:
        scene = query_scene()
        rays = query_rays(scene)
        r64 = rays.astype(np.float64)
        hit = closest_hit(scene, r64[:, 0:3], r64[:, 4:7], r64[:, 3], np.inf)
        _QUERY.update(scene=scene, rays=rays, hit=hit)
    return _QUERY["scene"], _QUERY["rays"], _QUERY["hit"]


def query_errors(hit, t, u, v):
    """A renderer's t, u, v for the query batch against the statement's, in units of each ray's conditioning:
    -> (|dt| / (t cond_t), max(|du|, |dv|) / cond_uv), (N,) each; compare with QUERY_T_BOUND / QUERY_UV_BOUND."""
    with np.errstate(all="ignore"):
        t_err = np.abs(np.asarray(t, np.float64) - hit["t"]) / (hit["t"] * hit["cond_t"])
        uv_err = np.maximum(np.abs(np.asarray(u, np.float64) - hit["u"]), np.abs(np.asarray(v, np.float64) - hit["v"])) / hit["cond_uv"]
    return t_err, uv_err


def occlusion_batch():
    """Rays of the query batch with a finite range: for the rays that hit, tmax just before (t (1 - 1e-3)) and just beyond
    (t (1 + 1e-3)) the closest hit, and tmin beyond it (t * 1.05: the nearest surface is skipped); for the others a range of 5.
    -> (rays (M, 8) float32, expected (M,) bool, unsure (M,) bool)."""
    scene, rays, hit = query_statement()
    is_hit = hit["prim"] != PRIM_MISS
    t = np.where(is_hit, hit["t"], 5.0)
    batches = []
    for lo, hi in ((None, 1.0 - 1e-3), (None, 1.0 + 1e-3), (1.05, None)):
        r = rays.copy()
        if lo is not None:
            r[:, 3] = np.where(is_hit, t * lo, r[:, 3])
        r[:, 7] = np.where(is_hit, t * hi, 5.0) if hi is not None else 50.0
        batches.append(r)
    r = np.concatenate(batches)
    r64 = r.astype(np.float64)
    tmin = np.maximum(r64[:, 3], MIN_RAY_DISTANCE)
    got = closest_hit(scene, r64[:, 0:3], r64[:, 4:7], tmin, r64[:, 7])
    return r, got["prim"] != PRIM_MISS, got["unsure"]


# ------------------------------------------------------------------------------------------------------------------------
# The assertions, shared by the CPU and the GPU file.  `frame` is whatever rendered the case: dict prim, t, rgb (float32), and
# optionally red / green / blue / combined (uint8).  Each prints its figures, then asserts; no bound comes from the frame.
# ------------------------------------------------------------------------------------------------------------------------
def class_mask(ex, cls):
    if cls == "sphere":
        return (ex["prim"] != PRIM_MISS) & ((ex["prim"] & PRIM_SPHERE) != 0)
    if cls == "triangle":
        return (ex["prim"] & PRIM_SPHERE) == 0
    if cls == "miss":
        return ex["prim"] == PRIM_MISS
    return ex["prim"] == np.uint32(cls)


def check_case_conditions(case, mode=0):
    """The conditions on a case itself: at most EDGE_SHARE_CAP left out, every class at least CLASS_SHARE_MIN of the frame."""
    ex = statement(case, mode)
    share = ex["unsure"].mean()
    cover = {str(c): float((class_mask(ex, c) & ~ex["unsure"]).mean()) for c in case.classes}
    print(f"{case.name}: unsure share {share:.4f} (cap {EDGE_SHARE_CAP}), classes {cover}")
    assert share <= EDGE_SHARE_CAP
    assert min(cover.values()) >= CLASS_SHARE_MIN, cover


def _per_class(ex, bounds):
    """(h, w): bounds["sphere"] where the statement's primitive is a sphere, bounds["flat"] elsewhere."""
    return np.where(class_mask(ex, "sphere"), bounds["sphere"], bounds["flat"])


def _tolerances(case, ex):
    """Per pixel and channel: the absolute float tolerance."""
    rel = np.where(ex["f16"], F16_REL_TOL, _per_class(ex, RGB_REL_BOUND[case.group]))
    return rel[..., None] * ex["scale"]


def measure_frame(case, mode, frame):
    """-> dict: "rgb" / "t": {"flat": .., "sphere": ..} largest rgb error / scale on the classified pixels without f16 light and largest
    relative t error, per class; "f16": largest rgb error / scale on the pixels with f16 light."""
    ex = statement(case, mode)
    ok = ~ex["unsure"] & (frame["prim"] == ex["prim"])
    with np.errstate(all="ignore"):
        rel = np.abs(frame["rgb"].astype(np.float64) - ex["rgb"]) / ex["scale"]
    rel = np.where(np.isfinite(ex["rgb"]) & (ex["scale"] > 0), rel, 0.0).max(-1)
    hit = ok & (ex["prim"] != PRIM_MISS)
    with np.errstate(all="ignore"):
        t_rel = np.abs(frame["t"].astype(np.float64) - ex["t"]) / ex["t"]
    sphere = class_mask(ex, "sphere")

    def top(values, mask):
        return float(values[mask].max()) if mask.any() else 0.0
    plain, f16 = ok & ~ex["f16"], ok & ex["f16"]
    return {"rgb": {"flat": top(rel, plain & ~sphere), "sphere": top(rel, plain & sphere)},
            "t": {"flat": top(t_rel, hit & ~sphere), "sphere": top(t_rel, hit & sphere)}, "f16": top(rel, f16)}


def check_frame(case, mode, frame, label="", canonical_duplicates=False):
    """Primitive ids equal on the classified pixels; t within T_REL_BOUND (per class: sphere pixels, flat pixels); rgb within the pixel's tolerance, NaN and inf where the
    statement has them; bytes equal wherever the statement's value x 255 is further from a rounding boundary than 255 x the
    tolerance, within 1 elsewhere; channel textures and the combined image laid out as lib.rs:342-349, 383-388.
    canonical_duplicates: a walk of the reference-format BVH meets stored-twice triangles in tree order, which the reference's
    absent BVH crate decides: such ids are compared as their lowest."""
    ex = statement(case, mode)
    ok = ~ex["unsure"]
    prim = frame["prim"].copy()
    if canonical_duplicates and case.duplicates:
        prim[np.isin(prim, case.duplicates)] = min(case.duplicates)
    m = measure_frame(case, mode, dict(frame, prim=prim))
    rb, tb = RGB_REL_BOUND[case.group], T_REL_BOUND[case.group]
    print(f"{case.name} mode {mode} {label}: unsure {ex['unsure'].mean():.4f}, rgb error / scale flat {m['rgb']['flat']:.3e} (bound {rb['flat']:.3e}), "
          f"sphere {m['rgb']['sphere']:.3e} (bound {rb['sphere']:.3e}), with f16 attenuation {m['f16']:.3e} (bound {F16_REL_TOL:.3e}), "
          f"t flat {m['t']['flat']:.3e} (bound {tb['flat']:.3e}), sphere {m['t']['sphere']:.3e} (bound {tb['sphere']:.3e})")
    wrong = (prim != ex["prim"]) & ok
    assert not wrong.any(), f"{case.name}: {wrong.sum()} classified pixels with another primitive, first at {np.argwhere(wrong)[0]}"
    hit = ok & (ex["prim"] != PRIM_MISS)
    assert (np.abs(frame["t"].astype(np.float64)[hit] - ex["t"][hit]) <= _per_class(ex, T_REL_BOUND[case.group])[hit] * ex["t"][hit]).all()
    got = frame["rgb"].astype(np.float64)
    tol = _tolerances(case, ex)
    okc = np.broadcast_to(ok[..., None], got.shape)
    finite = np.isfinite(ex["rgb"])
    np.testing.assert_array_equal(np.isnan(got)[okc], np.isnan(ex["rgb"])[okc], err_msg=f"{case.name}: NaN pattern")
    inf = okc & np.isinf(ex["rgb"])
    np.testing.assert_array_equal(got[inf], ex["rgb"][inf], err_msg=f"{case.name}: infinities")
    sel = okc & finite
    with np.errstate(invalid="ignore"):
        bad = sel & ~(np.abs(got - np.where(finite, ex["rgb"], 0.0)) <= tol)
    assert not bad.any(), f"{case.name}: {bad.sum()} values off, first at {np.argwhere(bad)[0]}"
    if "combined" in frame:
        check_bytes(case, mode, frame)


def check_bytes(case, mode, frame):
    """The three channel textures and the combined image alone (what rt_dispatch_tile writes): bytes exact away from the rounding
    boundaries, within 1 at them; each texture keeps its own component with alpha 255; the combine takes R, G, B from them."""
    ex = statement(case, mode)
    tol = _tolerances(case, ex)
    finite = np.isfinite(ex["rgb"])
    okc = np.broadcast_to(~ex["unsure"][..., None], ex["rgb"].shape)
    x = np.where(finite, np.clip(np.where(finite, ex["rgb"], 0.0), 0.0, 1.0) * 255.0, 0.0)
    safe = (np.abs(x - np.floor(x) - 0.5) > 255.0 * tol) | ~finite
    by = np.stack([frame["red"][..., 0], frame["green"][..., 1], frame["blue"][..., 2]], -1).astype(np.int64)
    diff = np.abs(by - ex["bytes"].astype(np.int64))
    print(f"  bytes: {(diff[okc] != 0).sum()} differ, {(~safe & okc).sum()} at a rounding boundary")
    assert (diff[okc & safe] == 0).all() and (diff[okc] <= 1).all()
    for c, k in enumerate(("red", "green", "blue")):
        img = frame[k]
        others = [j for j in range(3) if j != c]
        assert (img[..., others] == 0).all() and (img[..., 3] == 255).all(), f"{case.name}: {k} texture keeps another component"
    np.testing.assert_array_equal(frame["combined"][..., :3], by.astype(np.uint8))
    assert (frame["combined"][..., 3] == 255).all()


def check_alternatives(case, mode=0):
    """Each named wrong alternative differs from the statement by more than twice the tolerance (in some channel, or in the
    primitive) on more than half of the classified pixels; the printed-only ones are reported."""
    ex = statement(case, mode)
    ok = ~ex["unsure"]
    tol = _tolerances(case, ex)
    for variant in case.asserted + case.printed:
        alt = statement(case, mode, variant)
        with np.errstate(all="ignore"):
            differs = (np.abs(alt["rgb"] - ex["rgb"]) > 2.0 * tol) | (np.isnan(alt["rgb"]) != np.isnan(ex["rgb"]))
        differs = differs.any(-1) | (alt["prim"] != ex["prim"])
        share = differs[ok].mean()
        print(f"{case.name} mode {mode}: alternative {variant} differs by more than twice the tolerance on {share:.3f} of the classified pixels"
              + ("" if variant in case.asserted else " (printed only)"))
        if variant in case.asserted:
            assert share > 0.5, (case.name, variant, share)
