"""Rates of the surface queries beside the calls they compose, on sponza-like (262 k triangles, device-built tree).

    python scripts/ao_rate.py [--out FILE.json] [--commit HASH] [--rays N] [--reps R] [--distance D]

rt_surface beside rt_intersect on 1 Mi device-resident incoherent rays (surface points, random directions, tmax = the distance to a
light: the batch of scripts/multi_hit_rate.py).  rt_ambient_occlusion over the hit points among rt_surface's records, S = 16 and 64,
max_distance = inf and D, beside rt_occluded on the same n * S rays, composed here on the device and resident there: the call a
caller had before, without the staging that would dominate it.  (The rays are composed with torch's sin / cos instead of the
library's polynomial, so a few samples in a million fall on the other side of an edge; `count_mismatch` tells how many points differ.)

Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11), so that drift of the machine falls on all of them alike; reported are the median of each
variant's R times, their spread (min, max), the rate in rays/s and the ratio of the time to its yardstick's.  One more run of each
S = 64 variant with RT_QUERY_COUNTERS gives the node visits and triangle tests per ray."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
from gpu_raytracer_amd import api, scenes  # noqa: E402
from multi_hit_rate import sponza_rays  # noqa: E402

DEV = "cuda:0"
M32 = 0xFFFFFFFF
BIAS = 1e-3


def compose(points, samples, seed, max_distance):
    """The n * samples rays of rt_ambient_occlusion's definition for device-resident points, point-major (int64 arithmetic masked to
    32 bits for the generator; torch's sin / cos for unit_vector)."""
    n = points.shape[0]
    i = torch.arange(n, device=DEV, dtype=torch.int64)
    s = torch.arange(samples, device=DEV, dtype=torch.int64)
    h = (((seed + i) & M32)[:, None] + s[None, :] * 0x9E3779B9) & M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    x1 = (h * 1664525 + 1013904223) & M32
    x2 = (x1 * 1664525 + 1013904223) & M32
    u1 = (x1 >> 8).float() / 16777216.0
    u2 = (x2 >> 8).float() / 16777216.0
    del h, x1, x2
    z = 1.0 - 2.0 * u1
    r = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
    ang = u2 * (2.0 * math.pi)
    unit = torch.stack([r * torch.cos(ang), r * torch.sin(ang), z], -1)
    del u1, u2, r, ang, z
    normal = points[:, None, 4:7]
    d = normal + unit
    d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    rays = torch.empty((n, samples, 8), device=DEV)
    rays[..., 0:3] = points[:, None, 0:3] + normal * BIAS
    rays[..., 3] = 1e-5
    rays[..., 4:7] = d
    rays[..., 7] = max_distance
    return rays.reshape(-1, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--distance", type=float, default=3.0)
    args = ap.parse_args()
    reps = max(args.reps, 11)
    scene = scenes.sponza_like()
    n_rays = args.rays
    rays = torch.from_numpy(sponza_rays(scene, n_rays, seed=5)).to(DEV)
    seed = 5
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        hits, surf = torch.empty((n_rays, 4), device=DEV), torch.empty((n_rays, 8), device=DEV)
        ctx.surface(rays, out=surf)
        prim = api.split_surface(surf)[1]
        points = surf[prim != api.PRIM_MISS].contiguous()
        n = points.shape[0]
        variants = {"rt_intersect": (lambda: ctx.intersect(rays, out=hits), n_rays, None),
                    "rt_surface": (lambda: ctx.surface(rays, out=surf), n_rays, "rt_intersect")}
        vis, cnt = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
        composed, occluded_fraction, mismatch = {}, {}, {}
        for samples in (16, 64):
            occ = torch.empty(n * samples, dtype=torch.bool, device=DEV)
            for dist in (float("inf"), args.distance):
                tag = f"S{samples}_{'inf' if math.isinf(dist) else 'd%g' % dist}"
                composed[tag] = compose(points, samples, seed, dist)
                ctx.occluded(composed[tag], out=occ)
                ctx.ambient_occlusion(points, samples, seed=seed, max_distance=dist, bias=BIAS, out=vis, counts=cnt)
                open_composed = samples - occ.view(n, samples).sum(1)
                occluded_fraction[tag] = float(occ.float().mean().item())
                mismatch[tag] = int((open_composed != cnt).sum().item())
                variants["rt_occluded_" + tag] = (lambda t=tag, o=occ: ctx.occluded(composed[t], out=o), n * samples, None)
                variants["rt_ambient_occlusion_" + tag] = (lambda s=samples, d=dist: ctx.ambient_occlusion(points, s, seed=seed, max_distance=d, bias=BIAS,
                                                                                                             out=vis, counts=cnt), n * samples, "rt_occluded_" + tag)
        times = {name: [] for name in variants}
        for fn, _, _ in variants.values():
            for _ in range(2):
                fn()
        for _ in range(reps):
            for name, (fn, _, _) in variants.items():
                fn()
                times[name].append(ctx.stats()["kernel_ms"])
        counters = {}
        for tag in ("S64_inf", "S64_d%g" % args.distance):
            dist = float("inf") if tag.endswith("inf") else args.distance
            ctx.occluded(composed[tag], counters=True)
            a = ctx.stats()
            ctx.ambient_occlusion(points, 64, seed=seed, max_distance=dist, bias=BIAS, out=vis, counts=cnt, counters=True)
            b = ctx.stats()
            counters[tag] = {"rt_occluded": {k: round(a[k] / a["rays"], 3) for k in ("node_visits", "tri_tests")},
                             "rt_ambient_occlusion": {k: round(b[k] / b["rays"], 3) for k in ("node_visits", "tri_tests")}}
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "rays": n_rays, "points": n, "reps": reps, "bias": BIAS,
           "distance": args.distance, "occluded_fraction": occluded_fraction, "count_mismatch_points": mismatch, "per_ray_counters": counters, "variants": {}}
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    for name, ts in times.items():
        _, n_traced, yardstick = variants[name]
        res["variants"][name] = {"kernel_ms_median": round(med[name], 4), "kernel_ms_min": round(min(ts), 4), "kernel_ms_max": round(max(ts), 4),
                                 "rays_per_s": round(n_traced / (med[name] * 1e-3))}
        if yardstick:
            res["variants"][name]["time_over_" + yardstick.split("_S")[0]] = round(med[name] / med[yardstick], 3)
        print(name, res["variants"][name], flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
