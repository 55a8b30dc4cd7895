"""Rate of rt_radiance beside the frame it re-states, on sponza-like (262 k triangles, device-built tree, five lights).

    python scripts/path_query_rate.py [--out FILE.json] [--commit HASH] [--width W --height H] [--reps R]

Rays: rt_camera_rays(mode 1) of a 1920 x 1080 frame, device-resident; the results stay on the device too.  1 spp, max_bounces 4,
seed = the frame's.  Yardstick: the closed extended-mode frame of the same parameters with RT_FLAG_KERNEL_V1 |
RT_FLAG_NO_SHADOW_GRID - the nested loops, the same paths and the same walks (the script asserts the same bits and the same segment
counts).  For orientation only: the default frame (the queue pipeline with light grids), and the loop a caller had to run before,
at ONE bounce with numpy on the host: rt_surface -> rt_direct_light -> a cosine-lobe scatter -> rt_surface -> rt_direct_light,
wall time, staging included (it treats every material as diffuse and opaque: it is there for its cost, not for its image).

Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every variant is warmed up twice, then the variants
take turns for R rounds (at least 11); reported are the median of each variant's R times, their spread (min, max) and the ratio of
the time to the yardstick's.  One more run of the query and of the yardstick with counters gives node visits and triangle tests per
segment."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
BOUNCES, SEED = 4, 0


def host_loop_one_bounce(ctx, rays, rng):
    """What a caller did before at one bounce, on the host: wall ms."""
    t0 = time.perf_counter()
    pts = ctx.surface(rays)
    hit = api.split_surface(pts)[1] != api.PRIM_MISS
    pts = np.ascontiguousarray(pts[hit])
    ctx.direct_light(pts)
    n = pts[:, 4:7]
    u = rng.random((len(pts), 2), dtype=np.float32)
    z = 1.0 - 2.0 * u[:, 0]
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    d = n + np.stack([r * np.cos(2 * np.pi * u[:, 1]), r * np.sin(2 * np.pi * u[:, 1]), z], 1)
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-20)
    nxt = api.make_rays(pts[:, 0:3] + n * np.float32(1e-3), d.astype(np.float32))
    pts2 = ctx.surface(nxt)
    ctx.direct_light(np.ascontiguousarray(pts2[api.split_surface(pts2)[1] != api.PRIM_MISS]), ambient=True)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps = max(args.reps, 11)
    w, h = args.width, args.height
    scene = scenes.sponza_like()
    frame_kw = dict(mode=api.MODE_EXTENDED, spp=1, max_bounces=BOUNCES, frame_seed=SEED)
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        rays = torch.empty((w * h, 8), device=DEV)
        ctx.camera_rays(w, h, scene.camera, mode=1, out=rays)
        out = torch.empty((w * h, 4), device=DEV)
        variants = {"frame_nested_loops_tree": lambda: ctx.render(w, h, scene.camera, kernel_v1=True, no_shadow_grid=True, **frame_kw),
                    "rt_radiance": lambda: ctx.radiance(rays, max_bounces=BOUNCES, seed=SEED, out=out),
                    "frame_default": lambda: ctx.render(w, h, scene.camera, **frame_kw)}
        # the same paths: the same bits and the same segments
        st_f = variants["frame_nested_loops_tree"]()
        frame = ctx.read_rgb32f().reshape(-1, 3)
        variants["rt_radiance"]()
        st_q = ctx.stats()
        assert np.array_equal(out[:, 0:3].cpu().numpy().view(np.uint32), frame.view(np.uint32)), "the query and the frame differ"
        seg_keys = ("rays", "primary_rays", "continuation_rays", "shadow_rays")
        assert all(st_f[k] == st_q[k] for k in seg_keys)
        times = {name: [] for name in variants}
        for fn in variants.values():
            for _ in range(2):
                fn()
        for _ in range(reps):
            for name, fn in variants.items():
                fn()
                times[name].append(ctx.stats()["kernel_ms"])
        counters = {}
        a = ctx.render(w, h, scene.camera, kernel_v1=True, no_shadow_grid=True, counters=True, **frame_kw)
        ctx.radiance(rays, max_bounces=BOUNCES, seed=SEED, out=out, counters=True)
        b = ctx.stats()
        for name, st in (("frame_nested_loops_tree", a), ("rt_radiance", b)):
            counters[name] = {k: round(st[k] / st["rays"], 4) for k in ("node_visits", "tri_tests")}
        host_rays = rays.cpu().numpy()
        rng = np.random.default_rng(1)
        host_loop_one_bounce(ctx, host_rays, rng)
        host_ms = sorted(host_loop_one_bounce(ctx, host_rays, rng) for _ in range(3))
        ctx.radiance(rays, max_bounces=1, seed=SEED, out=out)
        one_bounce_ms = ctx.stats()["kernel_ms"]
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "lights": len(scene.lights), "width": w, "height": h,
           "rays": w * h, "max_bounces": BOUNCES, "reps": reps, "segments": {k: st_q[k] for k in seg_keys}, "per_segment_counters": counters,
           "host_loop_one_bounce_wall_ms_median": round(host_ms[1], 2), "rt_radiance_one_bounce_kernel_ms": round(one_bounce_ms, 4), "variants": {}}
    med = {name: float(np.median(ts)) for name, ts in times.items()}
    for name, ts in times.items():
        res["variants"][name] = {"kernel_ms_median": round(med[name], 4), "kernel_ms_min": round(min(ts), 4), "kernel_ms_max": round(max(ts), 4),
                                 "segments_per_s": round(st_q["rays"] / (med[name] * 1e-3)),
                                 "time_over_frame_nested_loops_tree": round(med[name] / med["frame_nested_loops_tree"], 3)}
        print(name, res["variants"][name], flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
