"""Rate and walk of rt_sweep_triangle on sponza-like (262 k triangles, device-built tree), beside what a caller had to use before it.

    python scripts/sweep_triangle_rate.py [--out FILE.json] [--commit HASH] [--sweeps N] [--reps R]

One batch of N (default 1 M) sweeps toward surfaces (sweep_box_cases.toward_surfaces: starts over 1.5 times the scene's box, aimed at
points of the surface, |d| in 0.2 .. 5), device-resident, the results staying on the device too, at two sizes: the vertices uniform in
a cube of side 0.15 and of side 0.75 about the start, which makes the mean edge about 0.1 and about 0.5.  Variants per size:
  sweep_triangle   rt_sweep_triangle
  sweep_box        rt_sweep_box over each triangle's bounding box with the same direction - a different and looser query, the
                   yardstick only in the sense that it is what was there.  The box is the bounds' centre and half extent rounded
                   to f32, and where the triangle meets the scene with a vertex that is a corner of its bounds, or face on with an
                   axis-aligned wall, the two times are equal in exact arithmetic and rounding decides.  So the times are compared
                   with a relative tolerance TIE = 1e-5: box_tie is the share of sweeps whose times differ by at most TIE x the
                   larger (two misses tie), box_earlier the share for which the box's contact is before the triangle's by more
                   than that (or the triangle has none), box_later the reverse, which a box that holds the triangle cannot be but
                   by rounding; box_later_max_rel is the largest relative difference among ALL sweeps whose box time is the
                   larger one and box_later_max_abs the largest absolute one (where both hit), box_later_triangle_at_start the share
                   of sweeps beyond the tolerance whose triangle starts in contact (t = 0, so any later box time is relative 1), and
                   box_earlier_strict / box_later_strict are the shares by the raw f32 comparison
  overlap_count    rt_overlap_triangle, count only, at the start pose: the static half of the pair
  intersect        rt_intersect on the ray of q0 along d
Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11); reported are the median of each variant's R times and their spread (min, max).  One more run of
each with RT_QUERY_COUNTERS gives node visits and triangle tests per sweep.  The first 64 answers of rt_sweep_triangle are held to the
numpy statement of tests/sweep_triangle_cases.py before anything is timed.  A record, not a gate: no threshold is set on these
numbers."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import overlap_triangle_cases as tc  # noqa: E402
import sweep_box_cases as bc  # noqa: E402
import sweep_triangle_cases as st  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
CHECKED = 64
SIDES = (0.15, 0.75)
TIE = 1e-5  # relative: far above the f32 statements' error, far below a contact of empty space
CALLS = ("sweep_triangle", "sweep_box", "overlap_count", "intersect")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--sweeps", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.sweeps
    scene = scenes.sponza_like()
    boxes = bc.toward_surfaces(scene, n, 3)
    start, d = boxes[:, 0:3].astype(np.float64), boxes[:, 8:11]
    offsets = np.random.default_rng(3).random((n, 3, 3)) - 0.5
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "sweeps": n, "reps": reps, "variants": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        host = {}
        for side in SIDES:
            v = (start[:, None, :] + offsets * side).astype(np.float32)
            sweeps = st.make_sweeps(v[:, 0], v[:, 1], v[:, 2], d)
            lo, hi = (b.astype(np.float64) for b in tc.bounds(sweeps[:, 0:12]))
            host[(side, "sweep_triangle")] = sweeps
            host[(side, "sweep_box")] = bc._pack((lo + hi) / 2, (hi - lo) / 2, d)
            host[(side, "overlap_count")] = np.ascontiguousarray(sweeps[:, 0:12])
            host[(side, "intersect")] = api.make_rays(v[:, 0], d, tmin=0.0)
            edge = np.concatenate([np.linalg.norm(v[:, i].astype(np.float64) - v[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))])
            res[f"side{side}_mean_edge"] = round(float(edge.mean()), 4)
        dev = {key: torch.from_numpy(b).to(DEV) for key, b in host.items()}
        out8 = torch.empty((n, 8), dtype=torch.float32, device=DEV)
        out4 = torch.empty((n, 4), dtype=torch.float32, device=DEV)
        counts = torch.empty((n,), dtype=torch.int32, device=DEV)
        variants = [(side, call) for side in SIDES for call in CALLS]

        def run(variant, counters=False):
            side, call = variant
            if call == "sweep_triangle":
                ctx.sweep_triangle(dev[variant], out=out8, counters=counters)
            elif call == "sweep_box":
                ctx.sweep_box(dev[variant], out=out8, counters=counters)
            elif call == "overlap_count":
                ctx.overlap_triangle(dev[variant], 0, counts=counts, count_all=True, counters=counters)
            else:
                ctx.intersect(dev[variant], out=out4, counters=counters)
            return ctx.stats()

        for side in SIDES:
            run((side, "sweep_triangle"))
            tri = out8.cpu().numpy()
            want = st.brute_force(scene, host[(side, "sweep_triangle")][:CHECKED], prefilter=True)
            assert np.array_equal(tri[:CHECKED].view(np.uint32), want.view(np.uint32)), f"side {side}: not the statement's records"
            run((side, "sweep_box"))
            box = out8.cpu().numpy()
            t_tri = np.where(tri[:, 6].view(np.uint32) != st.PRIM_MISS, tri[:, 3], np.inf)
            t_box = np.where(box[:, 6].view(np.uint32) != st.PRIM_MISS, box[:, 3], np.inf)
            t_tri, t_box = t_tri.astype(np.float64), t_box.astype(np.float64)
            with np.errstate(invalid="ignore"):
                both = np.isfinite(t_tri) & np.isfinite(t_box)
                rel = np.where(both, np.abs(t_box - t_tri) / np.maximum(np.maximum(t_box, t_tri), 1e-300), np.where(t_box == t_tri, 0.0, np.inf))
            tie = rel <= TIE
            res[f"side{side}_box_tie"] = round(float(tie.mean()), 4)
            res[f"side{side}_box_earlier"] = round(float((~tie & (t_box < t_tri)).mean()), 4)
            res[f"side{side}_box_later"] = round(float((~tie & (t_box > t_tri)).mean()), 6)
            worst = float(rel[t_box > t_tri].max()) if (t_box > t_tri).any() else 0.0
            res[f"side{side}_box_later_max_rel"] = worst if np.isfinite(worst) else None  # None: the box misses where the triangle hits
            later = both & (t_box > t_tri)
            res[f"side{side}_box_later_max_abs"] = float((t_box - t_tri)[later].max()) if later.any() else 0.0  # in units of t
            res[f"side{side}_box_later_triangle_at_start"] = round(float((~tie & later & (t_tri == 0)).mean()), 6)
            res[f"side{side}_box_earlier_strict"] = round(float((t_box < t_tri).mean()), 4)
            res[f"side{side}_box_later_strict"] = round(float((t_box > t_tri).mean()), 4)
            res[f"side{side}_hit"] = round(float(np.isfinite(t_tri).mean()), 4)
            res[f"side{side}_at_start"] = round(float((t_tri == 0).mean()), 4)
            res[f"side{side}_box_at_start"] = round(float((t_box == 0).mean()), 4)
            print({k: v for k, v in res.items() if k.startswith(f"side{side}")}, flush=True)
        times = {v: [] for v in variants}
        for v in variants:
            for _ in range(2):
                run(v)
        for _ in range(reps):
            for v in variants:
                times[v].append(run(v)["kernel_ms"])
        for v in variants:
            s = run(v, counters=True)
            med = float(np.median(times[v]))
            name = f"side{v[0]}_{v[1]}"
            res["variants"][name] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[v]), 4), "kernel_ms_max": round(max(times[v]), 4),
                                     "queries_per_s": round(n / (med * 1e-3)), "node_visits_per_query": round(s["node_visits"] / n, 3),
                                     "tri_tests_per_query": round(s["tri_tests"] / n, 3)}
            print(name, res["variants"][name], flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
