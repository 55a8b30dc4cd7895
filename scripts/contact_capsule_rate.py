"""Rate and walk of rt_contact_capsule on sponza-like (262 k triangles, device-built tree), beside what a caller had before - a chain
of three rt_closest_point_all along the axis, rt_overlap_box with the capsule's bounding box - all in one run.

    python scripts/contact_capsule_rate.py [--out FILE.json] [--commit HASH] [--capsules N] [--reps R]

Batches of N (default 1 M) records, device-resident, the results staying on the device too; some point of each axis within 0.05 of a
point of the surface (closest_point_cases.near_surface), radius 0.1:
  contact_upright_k4   rt_contact_capsule, axis (0, 0.2, 0), max_contacts 4
  contact_diagonal_k4  rt_contact_capsule, axis 0.2 (1, 1, 1) / sqrt 3, max_contacts 4: the same body, whose bound is the loosest
  contact_upright_k16  rt_contact_capsule, the upright capsules, max_contacts 16
  contact_count_all    rt_contact_capsule, the upright capsules, max_contacts 0 with count_all
  contact_any          rt_contact_capsule, the upright capsules, any_hit: the occupancy test
  contact_zero_k4      rt_contact_capsule, axis 0, max_contacts 4: the statement's price at equal work, beside
  points_k4            rt_closest_point_all at the same points, max_nearest 4
  chain_upright_k4     rt_closest_point_all x 3 at the ends and the middle of the upright axes, one batch of 3 N, max_nearest 4: misses what
                       lies between the points and lists a primitive once per point
  box_upright_any      rt_overlap_box with the upright capsules' bounding boxes, any_hit: over-reports at the corners
Times: kernel_ms = the HIP events of the library around its launch (rt_stats).  Each batch is warmed up twice, then all take turns for
R rounds (at least 11); reported are the median of each batch's R times and their spread (min, max).  One more run of each with
RT_QUERY_COUNTERS gives node visits and triangle tests per query.  The first 32 answers of each contact batch are held to the numpy
statement of tests/contact_capsule_cases.py before anything is timed.  Reported too: the share of capsules in contact that the chain's
three points all miss, and the share of occupied bounding boxes whose capsule is free."""
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
import contact_capsule_cases as kc  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
R, LENGTH = 0.1, 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--capsules", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.capsules
    scene = scenes.sponza_like()
    at = cc.near_surface(scene, n, 3, sigma=0.05)
    where = np.random.default_rng(4).random((n, 1)).astype(np.float32)
    upright, diagonal = np.array([0.0, LENGTH, 0.0], np.float32), np.full(3, LENGTH / np.sqrt(3.0), np.float32)
    up = kc.make_capsules(at - upright * where, R, upright)
    origin = np.ascontiguousarray(up[:, 0:3])
    host = {"contact_upright_k4": up, "contact_diagonal_k4": kc.make_capsules(at - diagonal * where, R, diagonal), "contact_upright_k16": up,
            "contact_count_all": up, "contact_any": up, "contact_zero_k4": kc.make_capsules(at, R, (0, 0, 0)),
            "points_k4": api.make_points(at, R),
            "chain_upright_k4": np.concatenate([api.make_points(origin + np.float32(f) * upright, R) for f in (0.0, 0.5, 1.0)]),
            "box_upright_any": api.make_boxes(origin + np.float32(0.5) * upright, np.abs(upright) / 2 + R)}
    with api.Context() as ctx:
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
        outs, counts = {}, {k: torch.empty(len(v), dtype=torch.int32, device=DEV) for k, v in host.items()}
        calls = {}
        for name, k in (("contact_upright_k4", 4), ("contact_diagonal_k4", 4), ("contact_upright_k16", 16), ("contact_zero_k4", 4)):
            outs[name] = torch.empty((n, k, 8), device=DEV)
            calls[name] = lambda name=name, k=k, **kw: ctx.contact_capsule(dev[name], k, out=outs[name], counts=counts[name], **kw)
        calls["contact_count_all"] = lambda **kw: ctx.contact_capsule(dev["contact_count_all"], 0, counts=counts["contact_count_all"], count_all=True, **kw)
        calls["contact_any"] = lambda **kw: ctx.contact_capsule(dev["contact_any"], 0, counts=counts["contact_any"], any_hit=True, **kw)
        for name in ("points_k4", "chain_upright_k4"):
            outs[name] = torch.empty((len(host[name]), 4, 8), device=DEV)
            calls[name] = lambda name=name, **kw: ctx.closest_point_all(dev[name], 4, out=outs[name], counts=counts[name], **kw)
        calls["box_upright_any"] = lambda **kw: ctx.overlap_box(dev["box_upright_any"], 0, counts=counts["box_upright_any"], any_hit=True, **kw)
        res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "capsules": n, "reps": reps, "batches": {}}
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        for name in host:
            calls[name]()
        for name, k in (("contact_upright_k4", 4), ("contact_diagonal_k4", 4), ("contact_upright_k16", 16), ("contact_zero_k4", 4)):  # the statement's bytes
            want, want_counts, _ = kc.contacts_all(scene, host[name][:32], k)
            assert np.array_equal(outs[name][:32].cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{name}: not the statement's records"
            assert np.array_equal(counts[name][:32].cpu().numpy().astype(np.int64), want_counts.astype(np.int64)), f"{name}: not the statement's counts"
        same = outs["contact_zero_k4"][..., [0, 1, 2, 3, 6, 7]].contiguous().view(torch.int32) == outs["points_k4"][..., [0, 1, 2, 3, 6, 7]].contiguous().view(torch.int32)
        res["batches"]["contact_zero_k4"] = {"words_that_differ_from_closest_point_all": int((~same).sum())}
        touching = counts["contact_any"].cpu().numpy() > 0
        chain = counts["chain_upright_k4"].cpu().numpy().reshape(3, n).sum(0) > 0
        box = counts["box_upright_any"].cpu().numpy() > 0
        res["batches"]["chain_upright_k4"] = {"capsules_in_contact_that_the_chain_misses": round(float((touching & ~chain).sum() / max(touching.sum(), 1)), 4),
                                              "chain_contacts_the_capsule_does_not_have": int((chain & ~touching).sum())}
        res["batches"]["box_upright_any"] = {"occupied_boxes_whose_capsule_is_free": round(float((box & ~touching).sum() / max(box.sum(), 1)), 4),
                                             "capsules_in_contact_whose_box_is_free": int((touching & ~box).sum())}
        times = {name: [] for name in dev}
        for name in dev:
            for _ in range(2):
                calls[name]()
        for _ in range(reps):
            for name in dev:
                calls[name]()
                times[name].append(ctx.stats()["kernel_ms"])
        for name in dev:
            calls[name](counters=True)
            st = ctx.stats()
            med, m = float(np.median(times[name])), len(host[name])
            res["batches"].setdefault(name, {}).update(
                {"records": m, "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[name]), 4), "kernel_ms_max": round(max(times[name]), 4),
                 "queries_per_s": round(m / (med * 1e-3)), "node_visits_per_query": round(st["node_visits"] / m, 3),
                 "tri_tests_per_query": round(st["tri_tests"] / m, 3), "mean_count": round(float(counts[name].float().mean()), 4)})
            print(name, res["batches"][name], flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
