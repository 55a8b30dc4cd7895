"""Rate of rt_radiance_sh beside the composition it replaces, on sponza-like (262 k triangles, device-built tree, five lights).

    python scripts/radiance_sh_rate.py [--out FILE.json] [--commit HASH] [--probes N --samples S] [--reps R]

4,096 probes (seeded, uniform in the scene's bounding box) x 256 samples, max_bounces 4, probes and results device-resident.
Yardstick: what a caller did before - ONE rt_radiance call with samples = 1 and RT_PATH_CAMERA_DRAWS over the same N x S rays
pre-generated on the device, ray i * S + k = (P_i, d_{i,k}) with the directions of the statement.  That call's per-ray seeds are the
rays' indices, not the probes', so its paths are not the probes' paths past the first segment: the same kind of work, not the same
bits (the tests hold the bits).  Its projection, which the caller also had to run, is not in its time.

Times: kernel_ms = the HIP events of the library around its launches (rt_stats), the projection kernel included for rt_radiance_sh.
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
import radiance_sh_cases as rc  # noqa: E402  the statement's directions (tests/)
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
BOUNCES, SEED = 4, 0
U32, F32 = np.uint32, np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps = max(args.reps, 11)
    n, samples = args.probes, args.samples
    scene = scenes.sponza_like()
    pos = scene.vertices["position"].astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    points = np.random.default_rng(1).uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), (n, 3)).astype(F32)
    d = rc.directions(oracle, np.arange(n), samples, SEED, 0)
    host_rays = api.make_rays(np.repeat(points, samples, 0), d.reshape(-1, 3), 1e-5, np.finfo(F32).max)
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        probes = torch.from_numpy(api.make_probes(points)).to(DEV)
        rays = torch.from_numpy(host_rays).to(DEV)
        out_sh = torch.empty((n, 28), device=DEV)
        out_rays = torch.empty((n * samples, 4), device=DEV)
        variants = {"rt_radiance_composition": lambda: ctx.radiance(rays, samples=1, max_bounces=BOUNCES, seed=SEED, camera_draws=True, out=out_rays),
                    "rt_radiance_sh": lambda: ctx.radiance_sh(probes, samples, max_bounces=BOUNCES, seed=SEED, out=out_sh)}
        stats = {}
        for name, fn in variants.items():
            for _ in range(2):
                fn()
            stats[name] = ctx.stats()
        # the same first segments (the same origins and directions), so the same number of paths and of first hits
        assert stats["rt_radiance_sh"]["primary_rays"] == stats["rt_radiance_composition"]["primary_rays"] == n * samples
        sh = out_sh.cpu().numpy()
        assert np.isfinite(sh[:, :27]).all() and int(np.ascontiguousarray(sh[:, 27]).view(U32).astype(np.uint64).sum()) == stats["rt_radiance_sh"]["rays"]
        times = {name: [] for name in variants}
        for _ in range(reps):
            for name, fn in variants.items():
                fn()
                times[name].append(ctx.stats()["kernel_ms"])
    seg_keys = ("rays", "primary_rays", "continuation_rays", "shadow_rays")
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    res = {"scene": scene.name, "triangles": scene.n_triangles, "lights": len(scene.lights), "probes": n, "samples": samples,
           "max_bounces": BOUNCES, "reps": reps, **({"commit": args.commit} if args.commit else {}), "input_bytes": {"rt_radiance_sh": n * 16, "rt_radiance_composition": n * samples * 32}, "variants": {}}
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
