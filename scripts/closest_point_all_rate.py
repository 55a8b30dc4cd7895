"""Rate and walk of rt_closest_point_all on sponza-like (262 k triangles, device-built tree), beside rt_closest_point on the same points.

    python scripts/closest_point_all_rate.py [--out FILE.json] [--commit HASH] [--points N] [--reps R]

One batch of N (default 1 M) near-surface points (points on random triangles, displaced by a normal deviate of sigma 0.05 per axis),
device-resident, the results staying on the device too.  Variants:
  closest_point      rt_closest_point, radius = +inf: the yardstick of k1 - the same walk, so the difference is the list and the stores
  k1, k4, k16        rt_closest_point_all, max_nearest = 1, 4, 16, radius = +inf
  k16_r025           max_nearest = 16, radius = 0.25
  count_all_r025     max_nearest = 0 with RT_QUERY_COUNT_ALL, radius = 0.25: the count alone
Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11); reported are the median of each variant's R times and their spread (min, max), and k1's median
over closest_point's.  One more run of each with RT_QUERY_COUNTERS gives node visits and triangle tests per query.  The first 64
answers of each variant are held to the numpy statement of tests/closest_point_all_cases.py before anything is timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import closest_point_all_cases as ca  # noqa: E402
import closest_point_cases as cc  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
CHECKED = 64
# name: (max_nearest or None for rt_closest_point, radius, count_all)
VARIANTS = {"closest_point": (None, np.inf, False), "k1": (1, np.inf, False), "k4": (4, np.inf, False), "k16": (16, np.inf, False),
            "k16_r025": (16, 0.25, False), "count_all_r025": (0, 0.25, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.points
    scene = scenes.sponza_like()
    positions = cc.near_surface(scene, n, 3)
    host = {r: api.make_points(positions, radius=r) for r in sorted({v[1] for v in VARIANTS.values()})}
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "points": n, "reps": reps, "variants": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        dev = {r: torch.from_numpy(p).to(DEV) for r, p in host.items()}
        single = torch.empty((n, 8), device=DEV)
        lists = {k: torch.empty((n, k, 8), device=DEV) for k in sorted({v[0] for v in VARIANTS.values() if v[0]})}
        counts = torch.empty((n,), dtype=torch.int32, device=DEV)

        def run(name, counters=False):
            k, radius, count_all = VARIANTS[name]
            if k is None:
                ctx.closest_point(dev[radius], out=single, counters=counters)
            else:
                ctx.closest_point_all(dev[radius], k, out=lists.get(k), counts=counts, count_all=count_all, counters=counters)
            return ctx.stats()

        want = {r: ca.nearest_all(scene, p[:CHECKED]) for r, p in host.items()}  # the statement's bytes: (records, listed, total) at K = 16
        for name, (k, radius, count_all) in VARIANTS.items():
            run(name)
            rec, _, total = want[radius]
            if k is None:
                assert np.array_equal(single[:CHECKED].cpu().numpy().view(np.uint32), rec[:, 0].view(np.uint32)), f"{name}: not the statement's answers"
                continue
            if k:
                assert np.array_equal(lists[k][:CHECKED].cpu().numpy().view(np.uint32), rec[:, :k].view(np.uint32)), f"{name}: not the statement's answers"
            assert np.array_equal(counts[:CHECKED].cpu().numpy(), total if count_all else np.minimum(total, k)), f"{name}: not the statement's counts"
        times = {name: [] for name in VARIANTS}
        for name in VARIANTS:
            for _ in range(2):
                run(name)
        for _ in range(reps):
            for name in VARIANTS:
                times[name].append(run(name)["kernel_ms"])
        for name in VARIANTS:
            st = run(name, counters=True)
            med = float(np.median(times[name]))
            res["variants"][name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[name]), 4), "kernel_ms_max": round(max(times[name]), 4),
                                     "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_query": round(st["node_visits"] / n, 3),
                                     "tri_tests_per_query": round(st["tri_tests"] / n, 3)}
            print(name, res["variants"][name], flush=True)
        res["k1_over_closest_point"] = round(res["variants"]["k1"]["kernel_ms_median"] / res["variants"]["closest_point"]["kernel_ms_median"], 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
