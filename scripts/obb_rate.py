"""Rate and walk of rt_sweep_obb and rt_overlap_obb on sponza-like (262 k triangles, device-built tree), beside rt_sweep_box and
rt_overlap_box on the same centres - the axis-aligned kernels are the yardstick - all in one run.

    python scripts/obb_rate.py [--out FILE.json] [--commit HASH] [--queries N] [--reps R]

Batches of N (default 1 M) records, device-resident, the results staying on the device too, tmax = +inf; centres over 1.5 times the
bounding box, aimed at points of the surface, |d| in 0.2 .. 5; per half extent h in (0.05, 1e-3), a cube:
  sweep_obb_identity_h   rt_sweep_obb, rotation (0, 0, 0, 1): the cost of the frame products alone
  sweep_obb_random_h     rt_sweep_obb, rotations uniform over SO(3)
  sweep_box_h            rt_sweep_box on the same centres
  sweep_box_bound_h      rt_sweep_box with the world bounding box of the randomly turned box: what a caller had before
and at half extent 0.05, with the random rotations, the identity and the axis-aligned call, each as occupancy (RT_OVERLAP_ANY), count
(RT_QUERY_COUNT_ALL, K = 0) and list (K = 4):
  overlap_obb_random_*   overlap_obb_identity_*   overlap_box_*
Times: kernel_ms = the HIP events of the library around its launch (rt_stats).  Each batch is warmed up twice, then all take turns for
R rounds (at least 11); reported are the median of each batch's R times and their spread (min, max).  One more run of each with
RT_QUERY_COUNTERS gives node visits and triangle tests per query.  Before anything is timed the first 64 answers of the random sweeps
and counts are held to the numpy brute force of tests/obb_cases.py, and the identity batches to the axis-aligned calls' bytes.  Also
reported: the share of the bounding box's contacts that are earlier than the oriented box's (to 1e-5 of t), the error a caller made
before."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import obb_cases as ob  # noqa: E402
import sweep_box_cases as sb  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
EXTENTS = (0.05, 1e-3)
OVERLAP_MODES = {"any": dict(max_prims=0, any_hit=True), "count": dict(max_prims=0, count_all=True), "k4": dict(max_prims=4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.queries
    scene = scenes.sponza_like()
    base = sb.toward_surfaces(scene, n, 3, half_extent=EXTENTS[0])
    centre, direction = np.ascontiguousarray(base[:, 0:3]), np.ascontiguousarray(base[:, 8:11])
    rot = ob.rotations(n, 7, identity_share=0.0, near_share=0.0)
    identity = np.broadcast_to(np.float32(ob.IDENTITY), (n, 4))
    R = ob.frame(rot)[0]
    host, calls = {}, {}
    with api.Context() as ctx:
        for h in EXTENTS:
            hh = np.full((n, 3), h, np.float32)
            host[f"sweep_obb_identity_{h:g}"] = (ctx.sweep_obb, api.make_obb_sweeps(centre, h, identity, direction), {})
            host[f"sweep_obb_random_{h:g}"] = (ctx.sweep_obb, api.make_obb_sweeps(centre, h, rot, direction), {})
            host[f"sweep_box_{h:g}"] = (ctx.sweep_box, api.make_box_sweeps(centre, h, direction), {})
            host[f"sweep_box_bound_{h:g}"] = (ctx.sweep_box, api.make_box_sweeps(centre, ob.world_half(R, hh), direction), {})
        for mode, kw in OVERLAP_MODES.items():
            host[f"overlap_obb_random_{mode}"] = (ctx.overlap_obb, api.make_obbs(centre, EXTENTS[0], rot), kw)
            host[f"overlap_obb_identity_{mode}"] = (ctx.overlap_obb, api.make_obbs(centre, EXTENTS[0], identity), kw)
            host[f"overlap_box_{mode}"] = (ctx.overlap_box, api.make_boxes(centre, EXTENTS[0]), kw)
        res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "queries": n, "reps": reps, "batches": {}}
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        dev = {k: torch.from_numpy(v[1]).to(DEV) for k, v in host.items()}
        outs = {}
        for name, (call, _, kw) in host.items():
            if name.startswith("sweep"):
                outs[name] = dict(out=torch.empty((n, 8), device=DEV))
            else:
                outs[name] = dict(counts=torch.empty(n, dtype=torch.int32, device=DEV))
                if kw["max_prims"]:
                    outs[name]["out"] = torch.empty((n, kw["max_prims"]), dtype=torch.int32, device=DEV)

        def run(name, **more):
            call, _, kw = host[name]
            if name.startswith("sweep"):
                call(dev[name], **outs[name], **more)
            else:
                call(dev[name], kw["max_prims"], **{k: v for k, v in kw.items() if k != "max_prims"}, **outs[name], **more)

        for name in host:
            run(name)
        words = lambda t: t.cpu().numpy().view(np.uint32)
        for h in EXTENTS:  # the statement's bytes; the identity is the axis-aligned kernel's answer; the bound against the turned box
            name = f"sweep_obb_random_{h:g}"
            want = ob.brute_force(scene, host[name][1][:64], prefilter=True)
            assert np.array_equal(words(outs[name]["out"][:64]), want.view(np.uint32)), f"{name}: not the brute force's answers"
            assert torch.equal(outs[f"sweep_obb_identity_{h:g}"]["out"].view(torch.int32), outs[f"sweep_box_{h:g}"]["out"].view(torch.int32)), "identity"
            t_obb, t_bound = (outs[k.format(h)]["out"][:, 3].cpu().numpy().astype(np.float64) for k in ("sweep_obb_random_{:g}", "sweep_box_bound_{:g}"))
            res["batches"][f"sweep_box_bound_{h:g}"] = {"earlier_than_oriented": round(float((t_bound < t_obb * (1 - 1e-5)).mean()), 4),
                                                        "later_than_oriented": int((t_bound > t_obb * (1 + 1e-5) + 1e-6).sum())}
        boxes = host["overlap_obb_random_count"][1]
        want_total = ob.overlap_all(scene, boxes[:64], 4, touch=ob.touching(scene, boxes[:64], prefilter=True))
        assert np.array_equal(words(outs["overlap_obb_random_count"]["counts"][:64]), want_total[2]), "counts: not the brute force's"
        assert np.array_equal(words(outs["overlap_obb_random_k4"]["out"][:64]), want_total[0]), "ids: not the brute force's"
        for mode in OVERLAP_MODES:
            assert torch.equal(outs[f"overlap_obb_identity_{mode}"]["counts"], outs[f"overlap_box_{mode}"]["counts"]), "identity"
        times = {name: [] for name in host}
        for name in host:
            for _ in range(2):
                run(name)
        for _ in range(reps):
            for name in host:
                run(name)
                times[name].append(ctx.stats()["kernel_ms"])
        for name in host:
            run(name, counters=True)
            st = ctx.stats()
            med = float(np.median(times[name]))
            if name.startswith("sweep"):
                hit = outs[name]["out"][:, 6].contiguous().view(torch.int32) != -1
            else:
                hit = outs[name]["counts"] > 0
            res["batches"].setdefault(name, {}).update(
                {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[name]), 4), "kernel_ms_max": round(max(times[name]), 4),
                 "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_query": round(st["node_visits"] / n, 3),
                 "tri_tests_per_query": round(st["tri_tests"] / n, 3), "hit_fraction": round(float(hit.float().mean()), 4)})
            print(name, res["batches"][name], flush=True)
        for h in EXTENTS:
            for kind in ("identity", "random"):
                b = res["batches"][f"sweep_obb_{kind}_{h:g}"]
                b["ratio_to_sweep_box"] = round(b["kernel_ms_median"] / res["batches"][f"sweep_box_{h:g}"]["kernel_ms_median"], 3)
        for mode in OVERLAP_MODES:
            for kind in ("identity", "random"):
                b = res["batches"][f"overlap_obb_{kind}_{mode}"]
                b["ratio_to_overlap_box"] = round(b["kernel_ms_median"] / res["batches"][f"overlap_box_{mode}"]["kernel_ms_median"], 3)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
