"""Rate and walk of rt_contact_triangle on sponza-like (262 k triangles, device-built tree), beside what a caller had to use before it.

    python scripts/contact_triangle_rate.py [--out FILE.json] [--commit HASH] [--queries N] [--reps R]

One batch of N (default 1 M) triangles near surfaces (closest_point_cases.near_surface, sigma 0.02; the vertices uniform in a cube
of side 0.15 about the point, mean edge about 0.1), margin 0.03, device-resident, the results staying on the device too.  Variants:
  k4, k16, count, any   rt_contact_triangle at max_contacts 4 and 16, RT_QUERY_COUNT_ALL alone, RT_CONTACT_ANY
  capsules              three rt_contact_capsule calls, count only, one per edge with the margin as the radius: misses every contact
                        in which a vertex of the scene faces the interior of the triangle.  missed_by_capsules is the share of
                        queries with a contact whose three counts are all 0, fewer_by_capsules the share whose largest edge count is
                        below the triangle's count
  sphere                rt_closest_point_all, count only, at the centroid with the circumscribed radius + margin: lists primitives
                        the triangle is nowhere near.  sphere_ratio = its mean count / the triangle's
  box                   rt_overlap_box, count only, over the bounds grown by the margin.  box_ratio likewise
Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11); reported are the median of each variant's R times and their spread (min, max).  One more run of
each with RT_QUERY_COUNTERS gives node visits and triangle tests per query.  The first 64 answers at K = 4 are held to the numpy
statement of tests/contact_triangle_cases.py before anything is timed.  A record, not a gate: no threshold is set on these numbers."""
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
import contact_triangle_cases as kt  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
CHECKED = 64
SIDE, MARGIN = 0.15, 0.03
CALLS = ("k4", "k16", "count", "any", "capsules", "sphere", "box")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.queries
    scene = scenes.sponza_like()
    at = cc.near_surface(scene, n, 3, sigma=0.02).astype(np.float64)
    v = (at[:, None, :] + (np.random.default_rng(3).random((n, 3, 3)) - 0.5) * SIDE).astype(np.float32)
    tris = kt.make_contact_triangles(v[:, 0], v[:, 1], v[:, 2], MARGIN)
    v64 = v.astype(np.float64)
    centroid = v64.mean(1)
    reach = np.linalg.norm(v64 - centroid[:, None], axis=2).max(1) + MARGIN
    lo, hi = v64.min(1) - MARGIN, v64.max(1) + MARGIN
    host = {"tris": tris, "sphere": np.concatenate([centroid, reach[:, None]], 1).astype(np.float32),
            "box": api.make_boxes(((lo + hi) / 2).astype(np.float32), ((hi - lo) / 2).astype(np.float32))}
    for e, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        host[f"cap{e}"] = api.make_capsules(v[:, i], MARGIN, v[:, j] - v[:, i])
    edge = np.concatenate([np.linalg.norm(v64[:, i] - v64[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))])
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "queries": n, "reps": reps, "margin": MARGIN,
           "mean_edge": round(float(edge.mean()), 4), "variants": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        dev = {key: torch.from_numpy(b).to(DEV) for key, b in host.items()}
        out = {k: torch.empty((n, k, 8), dtype=torch.float32, device=DEV) for k in (4, 16)}
        counts = {c: torch.empty((n,), dtype=torch.int32, device=DEV) for c in ("tri", "cap0", "cap1", "cap2", "sphere", "box", "any")}

        def run(call, counters=False):
            """-> (kernel_ms, node visits, triangle tests) of the call's launches"""
            stats = []
            if call in ("k4", "k16"):
                k = int(call[1:])
                ctx.contact_triangle(dev["tris"], k, out=out[k], counts=counts["any"], counters=counters)
                stats.append(ctx.stats())
            elif call == "count":
                ctx.contact_triangle(dev["tris"], 0, counts=counts["tri"], count_all=True, counters=counters)
                stats.append(ctx.stats())
            elif call == "any":
                ctx.contact_triangle(dev["tris"], 0, counts=counts["any"], any_hit=True, counters=counters)
                stats.append(ctx.stats())
            elif call == "capsules":
                for e in range(3):
                    ctx.contact_capsule(dev[f"cap{e}"], 0, counts=counts[f"cap{e}"], count_all=True, counters=counters)
                    stats.append(ctx.stats())
            elif call == "sphere":
                ctx.closest_point_all(dev["sphere"], 0, counts=counts["sphere"], count_all=True, counters=counters)
                stats.append(ctx.stats())
            else:
                ctx.overlap_box(dev["box"], 0, counts=counts["box"], count_all=True, counters=counters)
                stats.append(ctx.stats())
            return tuple(sum(s[key] for s in stats) for key in ("kernel_ms", "node_visits", "tri_tests"))

        run("k4")
        want = kt.contacts_all(scene, tris[:CHECKED], 4)[0]
        assert np.array_equal(out[4][:CHECKED].cpu().numpy().view(np.uint32), want.view(np.uint32)), "not the statement's records"
        for call in ("count", "capsules", "sphere", "box"):
            run(call)
        c = {key: t.cpu().numpy().astype(np.int64) for key, t in counts.items()}
        caps = np.maximum(np.maximum(c["cap0"], c["cap1"]), c["cap2"])
        res["with_contact"] = round(float((c["tri"] > 0).mean()), 4)
        res["contacts_per_query"] = round(float(c["tri"].mean()), 3)
        res["missed_by_capsules"] = round(float(((c["tri"] > 0) & (caps == 0)).mean()), 5)
        res["fewer_by_capsules"] = round(float((caps < c["tri"]).mean()), 4)
        res["sphere_ratio"] = round(float(c["sphere"].mean() / max(c["tri"].mean(), 1e-300)), 2)
        res["box_ratio"] = round(float(c["box"].mean() / max(c["tri"].mean(), 1e-300)), 2)
        print({k: v for k, v in res.items() if k != "variants"}, flush=True)
        times = {call: [] for call in CALLS}
        for call in CALLS:
            for _ in range(2):
                run(call)
        for _ in range(reps):
            for call in CALLS:
                times[call].append(run(call)[0])
        for call in CALLS:
            _, visits, tests = run(call, counters=True)
            med = float(np.median(times[call]))
            res["variants"][call] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[call]), 4), "kernel_ms_max": round(max(times[call]), 4),
                                     "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_query": round(visits / n, 3),
                                     "tri_tests_per_query": round(tests / n, 3)}
            print(call, res["variants"][call], flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
