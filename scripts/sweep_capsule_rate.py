"""Rate and walk of rt_sweep_capsule on sponza-like (262 k triangles, device-built tree), beside what a caller had before - a chain of
three rt_sweep_sphere along the axis, rt_sweep_box with the capsule's bounding box - and beside rt_sweep_sphere and rt_intersect on
the same origins and directions, all in one run.

    python scripts/sweep_capsule_rate.py [--out FILE.json] [--commit HASH] [--sweeps N] [--reps R]

Batches of N (default 1 M) records, device-resident, the results staying on the device too, tmax = +inf; the bodies' middles over 1.5
times the bounding box, aimed at points of the surface, |d| in 0.2 .. 5:
  capsule_upright     rt_sweep_capsule, r = 0.05, axis (0, 0.2, 0)
  capsule_diagonal    rt_sweep_capsule, r = 0.05, axis 0.2 (1, 1, 1) / sqrt 3: the same body, whose bounding box is the loosest
  capsule_zero        rt_sweep_capsule, r = 1e-3, axis 0: the statement's price at equal work, beside
  sphere_1e-3         rt_sweep_sphere, r = 1e-3, from the same origins
  chain_upright       rt_sweep_sphere x 3 at the axis' ends and middle of capsule_upright, one batch of 3 N: misses what passes between
  box_upright         rt_sweep_box with capsule_upright's bounding box: reports contacts at corners the rounded body never makes
  intersect           rt_intersect on capsule_zero's origins and directions (tmin = 0)
Times: kernel_ms = the HIP events of the library around its launch (rt_stats).  Each batch is warmed up twice, then all take turns for
R rounds (at least 11); reported are the median of each batch's R times and their spread (min, max).  One more run of each with
RT_QUERY_COUNTERS gives node visits and triangle tests per query.  The first 64 answers of each capsule batch are held to the numpy
brute force of tests/sweep_capsule_cases.py before anything is timed.  Reported too: the share of upright capsule contacts that are
earlier than the chain's minimum (by more than 1e-5 of t and 1e-6), and the share of the box's contacts that are earlier than the
capsule's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import sweep_capsule_cases as cap  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
R, LENGTH, R_THIN = 0.05, 0.2, 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--sweeps", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.sweeps
    scene = scenes.sponza_like()
    upright, diagonal = np.array([0.0, LENGTH, 0.0]), np.full(3, LENGTH / np.sqrt(3.0))
    host = {"capsule_upright": cap.toward_surfaces(scene, n, 3, radius=(R, R), axes=upright),
            "capsule_diagonal": cap.toward_surfaces(scene, n, 3, radius=(R, R), axes=diagonal),
            "capsule_zero": cap.toward_surfaces(scene, n, 3, radius=(R_THIN, R_THIN), axes=np.zeros(3))}
    up = host["capsule_upright"]
    origin, direction = np.ascontiguousarray(up[:, 0:3]), np.ascontiguousarray(up[:, 8:11])
    zero = host["capsule_zero"]
    host["sphere_1e-3"] = api.make_sweeps(np.ascontiguousarray(zero[:, 0:3]), np.ascontiguousarray(zero[:, 8:11]), R_THIN)
    host["chain_upright"] = np.concatenate([api.make_sweeps(origin + np.float32(f) * upright.astype(np.float32), direction, R) for f in (0.0, 0.5, 1.0)])
    host["box_upright"] = api.make_box_sweeps(origin + np.float32(0.5) * upright.astype(np.float32), np.abs(upright) / 2 + R, direction)
    host["intersect"] = api.make_rays(np.ascontiguousarray(zero[:, 0:3]), np.ascontiguousarray(zero[:, 8:11]), tmin=0.0)
    with api.Context() as ctx:
        calls = {k: ctx.sweep_capsule if k.startswith("capsule") else ctx.sweep_box if k.startswith("box") else ctx.intersect if k == "intersect"
                 else ctx.sweep_sphere for k in host}
        res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "sweeps": n, "reps": reps, "batches": {}}
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
        outs = {k: torch.empty((len(v), 4 if k == "intersect" else 8), device=DEV) for k, v in host.items()}
        for name in host:
            calls[name](dev[name], out=outs[name])
        for name in ("capsule_upright", "capsule_diagonal", "capsule_zero"):  # the statement's bytes
            want = cap.brute_force(scene, host[name][:64], prefilter=True)
            assert np.array_equal(outs[name][:64].cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{name}: not the brute force's answers"
        t_cap = outs["capsule_upright"][:, 3].cpu().numpy().astype(np.float64)
        t_chain = outs["chain_upright"][:, 3].cpu().numpy().astype(np.float64).reshape(3, n).min(0)
        t_box = outs["box_upright"][:, 3].cpu().numpy().astype(np.float64)
        res["batches"]["capsule_upright"] = {"earlier_than_the_chain": round(float((t_cap < t_chain * (1 - 1e-5) - 1e-6).mean()), 4),
                                             "later_than_the_chain": int((t_cap > t_chain * (1 + 1e-5) + 1e-6).sum())}
        res["batches"]["box_upright"] = {"earlier_than_the_capsule": round(float((t_box < t_cap * (1 - 1e-5) - 1e-6).mean()), 4),
                                         "later_than_the_capsule": int((t_box > t_cap * (1 + 1e-5) + 1e-6).sum())}
        t_zero, t_sph = outs["capsule_zero"][:, 3].cpu().numpy(), outs["sphere_1e-3"][:, 3].cpu().numpy()
        res["batches"]["capsule_zero"] = {"times_that_differ_from_the_sphere_sweep": int((t_zero.view(np.uint32) != t_sph.view(np.uint32)).sum())}
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
            med, m = float(np.median(times[name])), len(host[name])
            hit = outs[name][:, 3 if name == "intersect" else 6].contiguous().view(torch.int32) != -1
            res["batches"].setdefault(name, {}).update(
                {"records": m, "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[name]), 4), "kernel_ms_max": round(max(times[name]), 4),
                 "queries_per_s": round(m / (med * 1e-3)), "node_visits_per_query": round(st["node_visits"] / m, 3),
                 "tri_tests_per_query": round(st["tri_tests"] / m, 3), "hit_fraction": round(float(hit.float().mean()), 4)})
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
