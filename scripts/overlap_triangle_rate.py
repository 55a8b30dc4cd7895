"""Rate and walk of rt_overlap_triangle on sponza-like (262 k triangles, device-built tree), beside what a caller had to use before it:
rt_overlap_box over each triangle's bounding box.

    python scripts/overlap_triangle_rate.py [--out FILE.json] [--commit HASH] [--triangles N] [--reps R]

One batch of N (default 1 M) query triangles centred near surfaces (points on random triangles, displaced by a normal deviate of sigma
0.05 per axis), device-resident, the results staying on the device too, at two sizes: the vertices uniform in a cube of side 0.15 and
of side 0.75 about the centre, which makes the mean edge about 0.1 and about 0.5.  Variants per size, for the triangles (tri_*) and for
their bounding boxes (box_*: centre and half extent of the bounds, rounded to f32 - a different and looser query, the yardstick only
in the sense that it is what was there):
  any       RT_OVERLAP_ANY: is anything touched
  count     max_prims = 0 with RT_QUERY_COUNT_ALL: the count alone
  k4, k32   max_prims = 4, 32: the lists
Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11); reported are the median of each variant's R times and their spread (min, max).  One more run of
each with RT_QUERY_COUNTERS gives node visits and records read per query.  box_over_triangle_count is the sum of the boxes' counts over
the sum of the triangles': how many times as many primitives the bounding box reports.  The first 64 answers of every variant are held
to the numpy statements of tests/overlap_triangle_cases.py and tests/overlap_cases.py before anything is timed.  A record, not a gate:
no threshold is set on these numbers."""
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
import overlap_triangle_cases as tc  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
CHECKED = 64
SIDES = (0.15, 0.75)
# name: (max_prims, count_all, any_hit)
MODES = {"any": (0, False, True), "count": (0, True, False), "k4": (4, False, False), "k32": (32, False, False)}
SHAPES = ("tri", "box")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--triangles", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.triangles
    scene = scenes.sponza_like()
    centres = cc.near_surface(scene, n, 3).astype(np.float64)
    offsets = np.random.default_rng(3).random((n, 3, 3)) - 0.5
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "queries": n, "reps": reps, "variants": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        host = {}
        for side in SIDES:
            v = (centres[:, None, :] + offsets * side).astype(np.float32)
            tris = tc.make_triangles(v[:, 0], v[:, 1], v[:, 2])
            lo, hi = (b.astype(np.float64) for b in tc.bounds(tris))
            host[(side, "tri")], host[(side, "box")] = tris, oc.make_boxes((lo + hi) / 2, (hi - lo) / 2)
            edge = np.concatenate([np.linalg.norm(v[:, i].astype(np.float64) - v[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))])
            res[f"side{side}_mean_edge"] = round(float(edge.mean()), 4)
        dev = {key: torch.from_numpy(b).to(DEV) for key, b in host.items()}
        lists = {k: torch.empty((n, k), dtype=torch.int32, device=DEV) for k in (4, 32)}
        counts = torch.empty((n,), dtype=torch.int32, device=DEV)
        variants = [(side, shape, m) for side in SIDES for shape in SHAPES for m in MODES]

        def run(variant, counters=False):
            side, shape, mode = variant
            k, count_all, any_hit = MODES[mode]
            call = ctx.overlap_triangle if shape == "tri" else ctx.overlap_box
            call(dev[(side, shape)], k, out=lists.get(k), counts=counts, count_all=count_all, any_hit=any_hit, counters=counters)
            return ctx.stats()

        totals = {}
        for side in SIDES:
            for shape in SHAPES:
                statement = tc.overlap_all if shape == "tri" else oc.overlap_all
                ids, _, total = statement(scene, host[(side, shape)][:CHECKED])
                for mode, (k, count_all, any_hit) in MODES.items():
                    run((side, shape, mode))
                    got = counts.cpu().numpy().astype(np.int64)
                    totals[(side, shape, mode)] = int(got.sum())
                    want = (total > 0) if any_hit else total if count_all else np.minimum(total, k)
                    assert np.array_equal(got[:CHECKED], want.astype(np.int64)), f"side {side} {shape} {mode}: not the statement's counts"
                    if k:
                        assert np.array_equal(lists[k][:CHECKED].cpu().numpy().view(np.uint32), ids[:, :k]), f"side {side} {shape} {mode}: not the statement's ids"
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
            name = f"side{v[0]}_{v[1]}_{v[2]}"
            res["variants"][name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[v]), 4), "kernel_ms_max": round(max(times[v]), 4),
                                     "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_query": round(st["node_visits"] / n, 3),
                                     "records_per_query": round(st["tri_tests"] / n, 3), "count_sum": totals[v]}
            print(name, res["variants"][name], flush=True)
        for side in SIDES:
            res[f"side{side}_box_over_triangle_count"] = round(totals[(side, "box", "count")] / max(totals[(side, "tri", "count")], 1), 3)
            res[f"side{side}_touching"] = round(totals[(side, "tri", "any")] / n, 4)
            res[f"side{side}_box_occupied"] = round(totals[(side, "box", "any")] / n, 4)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
