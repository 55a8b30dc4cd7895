"""Rate of rt_direct_light beside the call it composes, on sponza-like (262 k triangles, device-built tree, five lights).

    python scripts/direct_light_rate.py [--out FILE.json] [--commit HASH] [--rays N] [--reps R]

Points: the hits of rt_surface over 1 Mi device-resident incoherent rays (the batch of scripts/multi_hit_rate.py), with rt_surface's
face-forwarded normals.  Yardstick: rt_occluded on exactly the shadow segments the definition traces - the (point, light) pairs
rt_direct_light itself reports as contributing (lit_mask with RT_DIRECT_NO_SHADOWS) - composed here on the device and resident
there, without the staging a caller would pay.  (The segments are composed with torch's arithmetic, so a few in a million may round
to the other side of an edge; `mask_mismatch_points` tells how many points differ from lit_mask.)  Variants: rt_direct_light with the
light grids rt_prepare built, and with RT_DIRECT_NO_SHADOW_GRID.

Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11); reported are the median of each variant's R times, their spread (min, max), the rate in
segments/s and the ratio of the time to the yardstick's.  One more run of each with RT_QUERY_COUNTERS gives node visits and triangle
tests per segment and the share of the segments the lists answered."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
from gpu_raytracer_amd import api, scenes  # noqa: E402
from multi_hit_rate import sponza_rays  # noqa: E402

DEV = "cuda:0"
BIAS = 1e-3
F32_MAX = float(np.finfo(np.float32).max)


def compose(points, contributing, lights):
    """The segments of rt_direct_light's definition, point-major: one per set bit of `contributing` -> ((m, 8) rays, (m,) point, (m,) light)."""
    rays, rows, which = [], [], []
    origin = points[:, 0:3] + points[:, 4:7] * BIAS
    for li, L in enumerate(lights):
        at = torch.nonzero((contributing >> li) & 1).flatten()
        r = torch.empty((at.shape[0], 8), device=DEV)
        r[:, 0:3] = origin[at]
        r[:, 3] = 1e-5
        if int(L["light_type"]) == 0:
            d = torch.tensor(L["direction"].astype(np.float32), device=DEV)
            r[:, 4:7] = -(d * (1.0 / torch.sqrt((d * d).sum())))
            r[:, 7] = F32_MAX
        else:
            to_light = torch.tensor(L["position"].astype(np.float32), device=DEV)[None, :] - points[at, 0:3]
            dist = torch.sqrt((to_light[:, 0] * to_light[:, 0] + to_light[:, 1] * to_light[:, 1]) + to_light[:, 2] * to_light[:, 2])
            r[:, 4:7] = to_light * (1.0 / dist)[:, None]
            r[:, 7] = dist
        rays.append(r)
        rows.append(at)
        which.append(torch.full_like(at, li))
    rays, rows, which = torch.cat(rays), torch.cat(rows), torch.cat(which)
    order = torch.argsort(rows * len(lights) + which)  # point-major, as the query goes through them
    return rays[order].contiguous(), rows[order], which[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps = max(args.reps, 11)
    scene = scenes.sponza_like()
    rays = torch.from_numpy(sponza_rays(scene, args.rays, seed=5)).to(DEV)
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        surf = ctx.surface(rays)
        points = surf[api.split_surface(surf)[1] != api.PRIM_MISS].contiguous()
        n = points.shape[0]
        out = torch.empty((n, 4), device=DEV)
        contributing = api.split_lighting(ctx.direct_light(points, shadows=False))[1]
        segs, seg_point, seg_light = compose(points, contributing, scene.lights)
        m = segs.shape[0]
        occ = torch.empty(m, dtype=torch.bool, device=DEV)
        ctx.prepare()
        grid_bytes = ctx.stats()["grid_bytes"]
        assert grid_bytes > 0
        # the composed segments give the query's mask (but for torch's rounding)
        ctx.occluded(segs, out=occ)
        lit = torch.zeros(n, dtype=torch.int64, device=DEV)
        lit.index_add_(0, seg_point, (~occ).to(torch.int64) << seg_light)
        mask = api.split_lighting(ctx.direct_light(points, out=out))[1]
        assert ctx.stats()["rays"] == m
        mismatch = int((lit != mask).sum().item())
        tree = ctx.direct_light(points, use_grids=False).clone()
        assert torch.equal(tree.view(torch.int32), out.view(torch.int32)), "grids and tree differ"
        variants = {"rt_occluded": lambda: ctx.occluded(segs, out=occ),
                    "rt_direct_light_grids": lambda: ctx.direct_light(points, out=out),
                    "rt_direct_light_tree": lambda: ctx.direct_light(points, use_grids=False, out=out)}
        times = {name: [] for name in variants}
        for fn in variants.values():
            for _ in range(2):
                fn()
        for _ in range(reps):
            for name, fn in variants.items():
                fn()
                times[name].append(ctx.stats()["kernel_ms"])
        counters = {}
        ctx.occluded(segs, out=occ, counters=True)
        a = ctx.stats()
        counters["rt_occluded"] = {k: round(a[k] / m, 4) for k in ("node_visits", "tri_tests")}
        for name, use in (("rt_direct_light_grids", True), ("rt_direct_light_tree", False)):
            ctx.direct_light(points, use_grids=use, out=out, counters=True)
            b, g = ctx.stats(), ctx.debug_shadow_grid()
            counters[name] = {k: round(b[k] / m, 4) for k in ("node_visits", "tri_tests")}
            counters[name]["answered_by_lists"] = round(g["segments_answered"] / m, 4)
            counters[name]["list_entries_per_segment"] = round(g["entries_read"] / m, 4)
        assert a["node_visits"] == b["node_visits"], "RT_DIRECT_NO_SHADOW_GRID does the yardstick's walks"
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "lights": len(scene.lights), "rays": args.rays, "points": n,
           "segments": m, "reps": reps, "bias": BIAS, "grid_bytes": grid_bytes, "occluded_fraction": round(float(occ.float().mean().item()), 4),
           "mask_mismatch_points": mismatch, "per_segment_counters": counters, "variants": {}}
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    for name, ts in times.items():
        res["variants"][name] = {"kernel_ms_median": round(med[name], 4), "kernel_ms_min": round(min(ts), 4), "kernel_ms_max": round(max(ts), 4),
                                 "segments_per_s": round(m / (med[name] * 1e-3)), "time_over_rt_occluded": round(med[name] / med["rt_occluded"], 3)}
        print(name, res["variants"][name], flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
