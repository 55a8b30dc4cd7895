"""Rate and walk of rt_sweep_box on sponza-like (262 k triangles, device-built tree), beside rt_sweep_sphere with the circumscribed and
the inscribed sphere and rt_intersect on the same centres and directions, all in one run.

    python scripts/sweep_box_rate.py [--out FILE.json] [--commit HASH] [--sweeps N] [--reps R]

Batches of N (default 1 M) records, device-resident, the results staying on the device too, tmax = +inf; centres over 1.5 times the
bounding box, aimed at points of the surface, |d| in 0.2 .. 5; per half extent h in (0.05, 1e-3), a cube:
  box_h           rt_sweep_box, half extents (h, h, h)
  sphere_out_h    rt_sweep_sphere, the circumscribed radius h sqrt 3: reports contacts the box never makes
  sphere_in_h     rt_sweep_sphere, the inscribed radius h: misses contacts the box makes
  intersect       rt_intersect on the same origins and directions (tmin = 0)
Times: kernel_ms = the HIP events of the library around its launch (rt_stats).  Each batch is warmed up twice, then all take turns for
R rounds (at least 11); reported are the median of each batch's R times and their spread (min, max).  One more run of each with
RT_QUERY_COUNTERS gives node visits and triangle tests per query.  The first 64 answers of each box batch are held to the numpy brute
force of tests/sweep_box_cases.py before anything is timed; how many box contacts do not lie between the two spheres' in time (to 1e-5
of t and 1e-6) is reported and expected to be 0."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import sweep_box_cases as sb  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
EXTENTS = (0.05, 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--sweeps", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.sweeps
    scene = scenes.sponza_like()
    host, calls = {}, {}
    base = sb.toward_surfaces(scene, n, 3, half_extent=EXTENTS[0])
    centre, direction = np.ascontiguousarray(base[:, 0:3]), np.ascontiguousarray(base[:, 8:11])
    with api.Context() as ctx:
        for h in EXTENTS:
            host[f"box_{h:g}"] = api.make_box_sweeps(centre, h, direction)
            host[f"sphere_out_{h:g}"] = api.make_sweeps(centre, direction, np.float32(h * np.sqrt(3.0)))
            host[f"sphere_in_{h:g}"] = api.make_sweeps(centre, direction, h)
        host["intersect"] = api.make_rays(centre, direction, tmin=0.0)
        for k in host:
            calls[k] = ctx.sweep_box if k.startswith("box") else ctx.sweep_sphere if k.startswith("sphere") else ctx.intersect
        res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "sweeps": n, "reps": reps, "batches": {}}
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
        outs = {k: torch.empty((n, 4 if k == "intersect" else 8), device=DEV) for k in host}
        for name in host:
            calls[name](dev[name], out=outs[name])
        for h in EXTENTS:  # the statement's bytes, and the box between its two spheres
            name = f"box_{h:g}"
            want = sb.brute_force(scene, host[name][:64], prefilter=True)
            assert np.array_equal(outs[name][:64].cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{name}: not the brute force's answers"
            t_box, t_out, t_in = (outs[k.format(h)][:, 3].cpu().numpy().astype(np.float64) for k in ("box_{:g}", "sphere_out_{:g}", "sphere_in_{:g}"))
            res["batches"][name] = {"outside_the_spheres": int(((t_out * (1 - 1e-5) > t_box + 1e-6) | (t_box > t_in * (1 + 1e-5) + 1e-6)).sum()),
                                    "earlier_than_inscribed": round(float((t_box < t_in * (1 - 1e-5)).mean()), 4),
                                    "later_than_circumscribed": round(float((t_box > t_out * (1 + 1e-5)).mean()), 4)}
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
            res["batches"].setdefault(name, {}).update(
                {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[name]), 4), "kernel_ms_max": round(max(times[name]), 4),
                 "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_query": round(st["node_visits"] / n, 3),
                 "tri_tests_per_query": round(st["tri_tests"] / n, 3), "hit_fraction": round(float(hit.float().mean()), 4)})
            print(name, res["batches"][name], flush=True)
        for name in res["batches"]:
            res["batches"][name]["ratio_to_intersect"] = round(res["batches"][name]["kernel_ms_median"] / res["batches"]["intersect"]["kernel_ms_median"], 3)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
