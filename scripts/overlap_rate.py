"""Rate and walk of rt_overlap_box on sponza-like (262 k triangles, device-built tree), beside what a caller had to use before it:
rt_closest_point_all(max_nearest = 0, RT_QUERY_COUNT_ALL) with the box's circumscribed sphere.

    python scripts/overlap_rate.py [--out FILE.json] [--commit HASH] [--boxes N] [--reps R]

One batch of N (default 1 M) cubes centred near surfaces (points on random triangles, displaced by a normal deviate of sigma 0.05 per
axis), device-resident, the results staying on the device too, at half extents 0.05 and 0.25.  Variants per half extent h:
  any       RT_OVERLAP_ANY: is the box occupied
  count     max_prims = 0 with RT_QUERY_COUNT_ALL: the count alone
  k4, k32   max_prims = 4, 32: the lists
  sphere    rt_closest_point_all(0, RT_QUERY_COUNT_ALL) at radius = |half_extent| = h * sqrt(3): a different query, the yardstick only
            in the sense that it is what was there
Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11); reported are the median of each variant's R times and their spread (min, max).  One more run of
each with RT_QUERY_COUNTERS gives node visits and triangle tests per box.  sphere_over_box_count is the sum of the sphere's counts
over the sum of the box's: by how much the circumscribed sphere over-reports.  The first 64 answers of each overlap variant are held to
the numpy statement of tests/overlap_cases.py before anything is timed.  A record, not a gate: no threshold is set on these numbers."""
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
import overlap_cases as oc  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
CHECKED = 64
HALF_EXTENTS = (0.05, 0.25)
# name: (max_prims, count_all, any_hit); "sphere" is rt_closest_point_all
MODES = {"any": (0, False, True), "count": (0, True, False), "k4": (4, False, False), "k32": (32, False, False), "sphere": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--boxes", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.boxes
    scene = scenes.sponza_like()
    centres = cc.near_surface(scene, n, 3)
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "boxes": n, "reps": reps, "variants": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        host = {h: oc.make_boxes(centres, (h, h, h)) for h in HALF_EXTENTS}
        boxes = {h: torch.from_numpy(b).to(DEV) for h, b in host.items()}
        points = {h: torch.from_numpy(api.make_points(centres, radius=float(np.sqrt(np.float32(3)) * np.float32(h)))).to(DEV) for h in HALF_EXTENTS}
        lists = {k: torch.empty((n, k), dtype=torch.int32, device=DEV) for k in (4, 32)}
        counts = torch.empty((n,), dtype=torch.int32, device=DEV)
        variants = [(h, m) for h in HALF_EXTENTS for m in MODES]

        def run(variant, counters=False):
            h, mode = variant
            if MODES[mode] is None:
                ctx.closest_point_all(points[h], 0, counts=counts, count_all=True, counters=counters)
            else:
                k, count_all, any_hit = MODES[mode]
                ctx.overlap_box(boxes[h], k, out=lists.get(k), counts=counts, count_all=count_all, any_hit=any_hit, counters=counters)
            return ctx.stats()

        totals = {}
        for h in HALF_EXTENTS:
            ids, _, total = oc.overlap_all(scene, host[h][:CHECKED])
            for mode, spec in MODES.items():
                run((h, mode))
                got = counts.cpu().numpy().astype(np.int64)
                totals[(h, mode)] = int(got.sum())
                if spec is None:
                    continue
                k, count_all, any_hit = spec
                want = (total > 0) if any_hit else total if count_all else np.minimum(total, k)
                assert np.array_equal(got[:CHECKED], want.astype(np.int64)), f"h {h} {mode}: not the statement's counts"
                if k:
                    assert np.array_equal(lists[k][:CHECKED].cpu().numpy().view(np.uint32), ids[:, :k]), f"h {h} {mode}: not the statement's ids"
        times = {v: [] for v in variants}
        for v in variants:
            for _ in range(2):
                run(v)
        for _ in range(reps):
            for v in variants:
                times[v].append(run(v)["kernel_ms"])
        for v in variants:
            st = run(v, counters=True)
            med = float(np.median(times[v]))
            name = f"h{v[0]}_{v[1]}"
            res["variants"][name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[v]), 4), "kernel_ms_max": round(max(times[v]), 4),
                                     "boxes_per_s": round(n / (med * 1e-3)), "node_visits_per_box": round(st["node_visits"] / n, 3),
                                     "tri_tests_per_box": round(st["tri_tests"] / n, 3), "count_sum": totals[v]}
            print(name, res["variants"][name], flush=True)
        for h in HALF_EXTENTS:
            res[f"h{h}_sphere_over_box_count"] = round(totals[(h, "sphere")] / max(totals[(h, "count")], 1), 3)
            res[f"h{h}_occupied"] = round(totals[(h, "any")] / n, 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
