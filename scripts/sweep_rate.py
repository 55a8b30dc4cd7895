"""Rate and walk of rt_sweep_sphere on sponza-like (262 k triangles, device-built tree), beside rt_intersect on the same rays.

    python scripts/sweep_rate.py [--out FILE.json] [--commit HASH] [--sweeps N] [--reps R]

Three batches of N (default 1 M) records, device-resident, the results staying on the device too, tmax = +inf:
  sweep_r0.05    origins over 1.5 times the bounding box, aimed at points of the surface, |d| in 0.2 .. 5, radius 0.05
  sweep_r0.001   the same origins and directions, radius 1e-3
  intersect      rt_intersect on the same origins and directions (tmin = 0): what the widened boxes and the dearer primitive test cost
Times: kernel_ms = the HIP events of the library around its launch (rt_stats).  Each batch is warmed up twice, then the three take
turns for R rounds (at least 11); reported are the median of each batch's R times and their spread (min, max).  One more run of each
with RT_QUERY_COUNTERS gives node visits and triangle tests per query.  The first 64 answers of each sweep batch are held to the numpy
brute force of tests/sweep_cases.py before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import sweep_cases as sc  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--sweeps", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.sweeps
    scene = scenes.sponza_like()
    wide = sc.toward_surfaces(scene, n, 3, radius=(0.05, 0.05))
    thin = wide.copy()
    thin[:, 3] = 1e-3
    host = {"sweep_r0.05": wide, "sweep_r0.001": thin, "intersect": api.make_rays(wide[:, 0:3], wide[:, 4:7], tmin=0.0)}
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "sweeps": n, "reps": reps, "batches": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
        outs = {k: torch.empty((n, 4 if k == "intersect" else 8), device=DEV) for k in host}
        calls = {k: ctx.intersect if k == "intersect" else ctx.sweep_sphere for k in host}
        for name in ("sweep_r0.05", "sweep_r0.001"):  # the statement's bytes
            ctx.sweep_sphere(dev[name], out=outs[name])
            want = sc.brute_force(scene, host[name][:64], prefilter=True)
            assert np.array_equal(outs[name][:64].cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{name}: not the brute force's answers"
        times = {name: [] for name in dev}
        for name in dev:
            for _ in range(2):
                calls[name](dev[name], out=outs[name])
        for _ in range(reps):
            for name in dev:
                calls[name](dev[name], out=outs[name])
                times[name].append(ctx.stats()["kernel_ms"])
        for name in dev:
            calls[name](dev[name], out=outs[name], counters=True)
            st = ctx.stats()
            med = float(np.median(times[name]))
            hit = outs[name][:, 3 if name == "intersect" else 6].contiguous().view(torch.int32) != -1
            res["batches"][name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[name]), 4), "kernel_ms_max": round(max(times[name]), 4),
                                    "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_query": round(st["node_visits"] / n, 3),
                                    "tri_tests_per_query": round(st["tri_tests"] / n, 3), "hit_fraction": round(float(hit.float().mean()), 4)}
            print(name, res["batches"][name], flush=True)
        for name in ("sweep_r0.05", "sweep_r0.001"):
            res["batches"][name]["ratio_to_intersect"] = round(res["batches"][name]["kernel_ms_median"] / res["batches"]["intersect"]["kernel_ms_median"], 3)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
