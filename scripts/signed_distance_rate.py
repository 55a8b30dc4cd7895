"""Rate and walk of rt_inside / rt_signed_distance on sponza-like (262 k triangles, device-built tree), beside rt_closest_point on the
same points and beside the composition of existing calls that they replace.

    python scripts/signed_distance_rate.py [--out FILE.json] [--commit HASH] [--points N] [--reps R]

One batch of N (default 1 M) near-surface points (points on random triangles, displaced by a normal deviate of sigma 0.05 per axis),
device-resident, radius = +inf, the results staying on the device too.  Variants:
  closest_point          rt_closest_point: the yardstick of the magnitude
  inside_r1, inside_r3   rt_inside with 1 and 3 rays, no votes array: a point stops at its majority
  inside_r1_votes, inside_r3_votes    ... with a votes array: every ray traced
  sd_r3, sd_r3_votes     rt_signed_distance with 3 rays, without and with a votes array
  composition            what sd_r3_votes replaces: rt_closest_point plus rt_intersect_all(max_hits = 0, RT_QUERY_COUNT_ALL) over the
                         3 N pre-generated rays (direction-major), kernel times summed; the host-side vote is not timed
Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11); reported are the median of each variant's R times and their spread (min, max).  The yardstick
of sd_r3_votes - equal work - is the composition in the same run, and the margin is the composition's own min - max range.  One more
run of each with RT_QUERY_COUNTERS gives node visits and triangle tests per point, and rays traced per point.  Also reported: the share
of the points whose three votes disagree.  The first 64 answers of each variant are held to the numpy statement of
tests/signed_distance_cases.py before anything is timed."""
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
import signed_distance_cases as sd  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
CHECKED = 64
# name: (call, rays, votes)
VARIANTS = {"closest_point": ("closest_point", 0, False),
            "inside_r1": ("inside", 1, False), "inside_r1_votes": ("inside", 1, True),
            "inside_r3": ("inside", 3, False), "inside_r3_votes": ("inside", 3, True),
            "sd_r3": ("signed_distance", 3, False), "sd_r3_votes": ("signed_distance", 3, True),
            "composition": ("composition", 3, True)}


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
    host = api.make_points(positions)
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "points": n, "reps": reps, "variants": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        dev = torch.from_numpy(host).to(DEV)
        rays = torch.from_numpy(np.ascontiguousarray(sd.inside_rays(positions)[:3]).reshape(-1, 8)).to(DEV)  # 3 N rays, direction-major
        records = torch.empty((n, 8), device=DEV)
        inside = torch.empty((n,), dtype=torch.bool, device=DEV)
        votes = torch.empty((n,), dtype=torch.uint8, device=DEV)
        counts = torch.empty((3 * n,), dtype=torch.int32, device=DEV)

        def run(name, counters=False):
            """-> (kernel_ms, node visits, triangle tests, rays traced)"""
            call, r, with_votes = VARIANTS[name]
            if call == "closest_point":
                ctx.closest_point(dev, out=records, counters=counters)
            elif call == "inside":
                ctx.inside(dev, rays=r, out=inside, votes=votes if with_votes else False, counters=counters)
            elif call == "signed_distance":
                ctx.signed_distance(dev, rays=r, out=records, votes=votes if with_votes else False, counters=counters)
            else:
                ctx.closest_point(dev, out=records, counters=counters)
                a = ctx.stats()
                ctx.intersect_all(rays, 0, counts=counts, count_all=True, counters=counters)
                b = ctx.stats()
                return a["kernel_ms"] + b["kernel_ms"], a["node_visits"] + b["node_visits"], a["tri_tests"] + b["tri_tests"], b["rays"]
            st = ctx.stats()
            return st["kernel_ms"], st["node_visits"], st["tri_tests"], 0 if call == "closest_point" else st["rays"]

        # the statement's bytes for the first points
        head = host[:CHECKED]
        head_counts = sd.crossings(scene, head[:, :3])
        unsigned = cc.brute_force(scene, head, prefilter=True)
        for name, (call, r, with_votes) in VARIANTS.items():
            run(name)
            want_inside, want_votes, _ = sd.statement(scene, head, max(r, 1), with_votes, counts=head_counts)
            if call == "closest_point":
                assert np.array_equal(records[:CHECKED].cpu().numpy().view(np.uint32), unsigned.view(np.uint32)), f"{name}: not the statement's answers"
                continue
            if call == "inside":
                assert np.array_equal(inside[:CHECKED].cpu().numpy(), want_inside), f"{name}: not the statement's answers"
            elif call == "signed_distance":
                assert np.array_equal(records[:CHECKED].cpu().numpy().view(np.uint32), sd.sign(unsigned, want_inside).view(np.uint32)), f"{name}: not the statement's records"
            else:
                got = counts.view(3, n)[:, :CHECKED].cpu().numpy().T
                assert np.array_equal(got, head_counts[:, :3]), f"{name}: not the statement's crossing counts"
            if with_votes and call != "composition":
                assert np.array_equal(votes[:CHECKED].cpu().numpy(), want_votes), f"{name}: not the statement's votes"
        times = {name: [] for name in VARIANTS}
        for name in VARIANTS:
            for _ in range(2):
                run(name)
        for _ in range(reps):
            for name in VARIANTS:
                times[name].append(run(name)[0])
        for name in VARIANTS:
            _, nodes, tris, traced = run(name, counters=True)
            med = float(np.median(times[name]))
            res["variants"][name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[name]), 4), "kernel_ms_max": round(max(times[name]), 4),
                                     "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_point": round(nodes / n, 3),
                                     "tri_tests_per_point": round(tris / n, 3), "rays_per_point": round(traced / n, 4)}
            print(name, res["variants"][name], flush=True)
        ctx.inside(dev, rays=3, out=inside, votes=votes)
        v = votes.cpu().numpy()
        res["split_votes_share_r3"] = round(float(((v > 0) & (v < 3)).mean()), 5)
        res["inside_share_r3"] = round(float(inside.cpu().numpy().mean()), 5)
        var = res["variants"]
        res["sd_r3_votes_over_composition"] = round(var["sd_r3_votes"]["kernel_ms_median"] / var["composition"]["kernel_ms_median"], 4)
        res["sd_r3_over_sd_r3_votes"] = round(var["sd_r3"]["kernel_ms_median"] / var["sd_r3_votes"]["kernel_ms_median"], 4)
        res["sd_r3_votes_inside_compositions_range"] = bool(var["composition"]["kernel_ms_min"] <= var["sd_r3_votes"]["kernel_ms_median"] <= var["composition"]["kernel_ms_max"])
        res["sd_r3_votes_above_compositions_max"] = bool(var["sd_r3_votes"]["kernel_ms_median"] > var["composition"]["kernel_ms_max"])
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
