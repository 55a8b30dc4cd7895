"""Rate and walk of rt_closest_point on sponza-like (262 k triangles, device-built tree).

    python scripts/closest_point_rate.py [--out FILE.json] [--commit HASH] [--points N] [--reps R]

Two batches of N (default 1 M) points, device-resident, the results staying on the device too, radius = +inf:
  near_surface   points on random triangles, displaced by a normal deviate of sigma 0.05 per axis (probes to snap)
  scattered      uniform over three times the scene's bounding box (a distance field's samples; most lie outside the atrium)
Times: kernel_ms = the HIP events of the library around its launch (rt_stats).  Each batch is warmed up twice, then the two take turns
for R rounds (at least 11); reported are the median of each batch's R times and their spread (min, max).  One more run of each with
RT_QUERY_COUNTERS gives node visits and triangle tests per query.  The first 64 answers of each batch are held to the numpy brute
force of tests/closest_point_cases.py before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import closest_point_cases as cc  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.points
    scene = scenes.sponza_like()
    host = {"near_surface": api.make_points(cc.near_surface(scene, n, 3)), "scattered": api.make_points(cc.scattered(scene, n, 4))}
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "points": n, "reps": reps, "batches": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
        out = torch.empty((n, 8), device=DEV)
        for name, pts in dev.items():  # the statement's bytes
            ctx.closest_point(pts, out=out)
            want = cc.brute_force(scene, host[name][:64], prefilter=True)
            assert np.array_equal(out[:64].cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{name}: not the brute force's answers"
        times = {name: [] for name in dev}
        for pts in dev.values():
            for _ in range(2):
                ctx.closest_point(pts, out=out)
        for _ in range(reps):
            for name, pts in dev.items():
                ctx.closest_point(pts, out=out)
                times[name].append(ctx.stats()["kernel_ms"])
        for name, pts in dev.items():
            ctx.closest_point(pts, out=out, counters=True)
            st = ctx.stats()
            med = float(np.median(times[name]))
            res["batches"][name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[name]), 4), "kernel_ms_max": round(max(times[name]), 4),
                                    "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_query": round(st["node_visits"] / n, 3),
                                    "tri_tests_per_query": round(st["tri_tests"] / n, 3)}
            print(name, res["batches"][name], flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
