"""Rate of rt_irradiance beside the composition it replaces, on sponza-like (262 k triangles, device-built tree, five lights).

    python scripts/irradiance_rate.py [--out FILE.json] [--commit HASH] [--points N --samples S] [--reps R]

4,096 surface points x 256 samples, max_bounces 4, points and results device-resident.  The points are a baker's: rt_surface over the
camera rays of a frame seen from the scene's own camera, the hits among them thinned evenly to N.
Yardstick: what a caller did before - ONE rt_radiance call with samples = 1 and RT_PATH_CAMERA_DRAWS over the same N x S rays
pre-generated on the device, ray i * S + k = (P_i + N_i * 0.001, d_{i,k}) with the directions of the statement.  That call's per-ray
seeds are the rays' indices, not the points', so its paths are not the points' paths past the first segment: the same kind of work,
not the same bits (the tests hold the bits).  Its reduction, which the caller also had to run, is not in its time.

Times: kernel_ms = the HIP events of the library around its launches (rt_stats), the reduction kernel included for rt_irradiance.
Both are warmed up twice, then take turns for R rounds (at least 11); reported are the medians, the spread (min, max) and the ratio."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import oracle  # noqa: E402  unit_vector on the host, for the yardstick's rays
import irradiance_cases as ic  # noqa: E402  the statement's directions (tests/)
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
BOUNCES, SEED = 4, 0
FRAME = (160, 120)  # the frame whose camera rays find the points: more hits than any N asked for here
U32, F32 = np.uint32, np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps = max(args.reps, 11)
    n, samples = args.points, args.samples
    scene = scenes.sponza_like()
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        found = ctx.surface(ctx.camera_rays(FRAME[0], FRAME[1], scene.camera, mode=1))
        found = found[ic.is_point(found)]
        assert len(found) >= n, (len(found), n)
        host_points = np.ascontiguousarray(found[np.linspace(0, len(found) - 1, n).astype(np.int64)])
        d = ic.directions(oracle, host_points, np.arange(n), samples, SEED, 0)
        host_rays = api.make_rays(np.repeat(ic.origins(host_points), samples, 0), d.reshape(-1, 3), 1e-5, np.finfo(F32).max)
        points = torch.from_numpy(host_points).to(DEV)
        rays = torch.from_numpy(host_rays).to(DEV)
        out_e = torch.empty((n, 4), device=DEV)
        out_rays = torch.empty((n * samples, 4), device=DEV)
        variants = {"rt_radiance_composition": lambda: ctx.radiance(rays, samples=1, max_bounces=BOUNCES, seed=SEED, camera_draws=True, out=out_rays),
                    "rt_irradiance": lambda: ctx.irradiance(points, samples, max_bounces=BOUNCES, seed=SEED, out=out_e)}
        stats = {}
        for name, fn in variants.items():
            for _ in range(2):
                fn()
            stats[name] = ctx.stats()
        # the same first segments (the same origins and directions), so the same number of paths and of first hits
        assert stats["rt_irradiance"]["primary_rays"] == stats["rt_radiance_composition"]["primary_rays"] == n * samples
        e = out_e.cpu().numpy()
        assert np.isfinite(e[:, :3]).all() and int(np.ascontiguousarray(e[:, 3]).view(U32).astype(np.uint64).sum()) == stats["rt_irradiance"]["rays"]
        times = {name: [] for name in variants}
        for _ in range(reps):
            for name, fn in variants.items():
                fn()
                times[name].append(ctx.stats()["kernel_ms"])
    seg_keys = ("rays", "primary_rays", "continuation_rays", "shadow_rays")
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    res = {"scene": scene.name, "triangles": scene.n_triangles, "lights": len(scene.lights), "points": n, "samples": samples,
           "max_bounces": BOUNCES, "reps": reps, **({"commit": args.commit} if args.commit else {}),
           "input_bytes": {"rt_irradiance": n * 32, "rt_radiance_composition": n * samples * 32},
           "output_bytes": {"rt_irradiance": n * 16, "rt_radiance_composition": n * samples * 16}, "variants": {}}
    for name, ts in times.items():
        res["variants"][name] = {"kernel_ms_median": round(med[name], 4), "kernel_ms_min": round(min(ts), 4), "kernel_ms_max": round(max(ts), 4),
                                 "segments": {k: stats[name][k] for k in seg_keys},
                                 "segments_per_s": round(stats[name]["rays"] / (med[name] * 1e-3)),
                                 "time_over_composition": round(med[name] / med["rt_radiance_composition"], 4)}
        print(name, res["variants"][name], flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
