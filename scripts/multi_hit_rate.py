"""Rates of the multi-hit query (rt_intersect_all) beside rt_intersect, on sponza-like (262 k triangles) with 1 M device-resident
incoherent rays (surface points, random directions, tmax = the distance to a light: the batch of tests/test_gpu_ray_queries.py).

    python scripts/multi_hit_rate.py [--out FILE.json] [--commit HASH] [--rays N] [--reps R] [--only-intersect]

Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds, so that drift of the machine falls on all of them alike; reported are the median of each variant's R times,
their spread (min, max), the rate in rays/s and the ratio of the time to rt_intersect's.  Device tensors in and out: no copies are timed.
--only-intersect: rt_intersect alone (with RT_HIP_LIB pointing at an older build: the yardstick the new kernels must not move)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
from gpu_raytracer_amd import api, scenes  # noqa: E402

F32 = np.float32


def sponza_rays(scene, n, seed):
    """Incoherent rays from seeded surface points, random directions, tmax = distance to a light."""
    rng = np.random.default_rng(seed)
    p = scene.vertices["position"].astype(F32)
    tr = scene.triangles
    v0 = p[tr["v0_index"]]
    e1, e2 = p[tr["v1_index"]] - v0, p[tr["v2_index"]] - v0
    ti = rng.integers(0, len(v0), n)
    w = rng.dirichlet([1, 1, 1], n).astype(F32)
    o = v0[ti] + e1[ti] * w[:, 1:2] + e2[ti] * w[:, 2:3]
    d = rng.standard_normal((n, 3)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lp = scene.lights["position"][1:].astype(F32)  # the point lights
    tmax = np.linalg.norm(lp[rng.integers(0, len(lp), n)] - o, axis=1).astype(F32)
    return api.make_rays(o, d, F32(1e-5), tmax)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--only-intersect", action="store_true")
    args = ap.parse_args()
    scene = scenes.sponza_like()
    n = args.rays
    rays = torch.from_numpy(sponza_rays(scene, n, seed=5)).to("cuda:0")
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        hit1 = torch.empty((n, 4), device="cuda:0")
        variants = {"rt_intersect": lambda: ctx.intersect(rays, out=hit1)}
        if not args.only_intersect:
            counts = torch.empty(n, dtype=torch.int32, device="cuda:0")
            for k in (1, 4, 16):
                out = torch.empty((n, k, 4), device="cuda:0")
                variants[f"intersect_all_k{k}"] = lambda k=k, out=out: ctx.intersect_all(rays, k, out=out, counts=counts)
            variants["count_all_k0"] = lambda: ctx.intersect_all(rays, 0, counts=counts, count_all=True)
        times = {name: [] for name in variants}
        for name, fn in variants.items():
            for _ in range(2):
                fn()
        for _ in range(args.reps):
            for name, fn in variants.items():
                fn()
                times[name].append(ctx.stats()["kernel_ms"])
        hits_per_ray = None
        if not args.only_intersect:
            hits_per_ray = float(counts.double().mean().item())  # of the count_all call: candidates in range per ray
    res = {"commit": args.commit, "library": os.environ.get("RT_HIP_LIB", "in-tree"), "scene": scene.name, "triangles": scene.n_triangles, "rays": n,
           "reps": args.reps, "candidates_per_ray": hits_per_ray, "variants": {}}
    base = float(np.median(times["rt_intersect"]))
    for name, ts in times.items():
        med = float(np.median(ts))
        res["variants"][name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ts), 4), "kernel_ms_max": round(max(ts), 4),
                                 "rays_per_s": round(n / (med * 1e-3)), "time_over_rt_intersect": round(med / base, 3)}
        print(name, res["variants"][name], flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
