"""rt_update_geometry on sponza-like (262 k triangles): what a refit costs against an upload and a rebuild, and how much slower the
refitted tree traces than a freshly built one after small and large motions (DESIGN.md "Geometry updates").

    python scripts/update_perf.py [--out FILE.json] [--once]

--once: one upload and one refit only (for `rocprofv3 --kernel-trace --stats`, to list the launches an update makes).
Times: kernel_ms = HIP events of the library, wall_ms = host time of the call; medians over repetitions after a warm-up."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # before any context: torch's device runtime comes up first
except ImportError:
    torch = None
from gpu_raytracer_amd import api, scenes  # noqa: E402

F32 = np.float32


def moved(scene, kind, seed=0):
    p = np.ascontiguousarray(scene.vertices["position"], dtype=np.float64)
    rng = np.random.default_rng(seed)
    lo, hi = p.min(0), p.max(0)
    if kind == "jitter":  # 0.1 % of the box per vertex
        p = p + rng.normal(0.0, 0.001 * float((hi - lo).max()), p.shape)
    elif kind == "large":  # half the vertices carried 60 % across the box
        sub = np.arange(len(p)) % 2 == 0
        p[sub] = p[sub] + np.array([0.6, 0.0, 0.3]) * (hi - lo)
    return np.ascontiguousarray(p.astype(F32))


def with_positions(scene, pos):
    v = scene.vertices.copy()
    v["position"] = pos
    return dataclasses.replace(scene, vertices=v)


def med(xs):
    return float(np.median(xs))


def incoherent_rays(scene, n, seed=1):
    p = np.ascontiguousarray(scene.vertices["position"], dtype=F32)
    tr = scene.triangles
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(tr), n)
    o = (p[tr["v0_index"][k]] + p[tr["v1_index"][k]] + p[tr["v2_index"][k]]) / F32(3)
    d = rng.normal(0, 1, (n, 3)).astype(F32)
    return api.make_rays(o, d, tmin=1e-3, tmax=np.float32(3.0e38))


def trace_times(ctxs, scene, cam_rays, inc_rays, reps=5):
    """Kernel times of the same work on each context, the contexts' repetitions interleaved (order alternating) so that clock
    drift falls on both alike."""
    out = [{} for _ in ctxs]

    def each(rep, fn):
        order = list(range(len(ctxs)))[:: 1 if rep % 2 == 0 else -1]
        for i in order:
            yield i, fn(ctxs[i], rep)

    for name, rays in (("camera_closest_hit", cam_rays), ("incoherent_closest_hit", inc_rays)):
        ks = [[] for _ in ctxs]
        for r in range(reps + 1):
            for i, ms in each(r, lambda c, rep: (c.intersect(rays), c.stats()["kernel_ms"])[1]):
                if r:
                    ks[i].append(ms)
        for i in range(len(ctxs)):
            out[i][name + "_kernel_ms"] = med(ks[i])
    ks = [[] for _ in ctxs]
    for r in range(reps + 1):
        for i, ms in each(r, lambda c, rep: c.render(1920, 1080, scene.camera, mode=2, spp=4, max_bounces=2, frame_seed=rep)["kernel_ms"]):
            if r:
                ks[i].append(ms)
    for i in range(len(ctxs)):
        out[i]["extended_1080p_4spp_2b_kernel_ms"] = med(ks[i])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    scene = scenes.sponza_like()
    jit = moved(scene, "jitter")
    if args.once:
        with api.Context() as ctx:
            ctx.upload_scene(scene)
            st = ctx.update_geometry(jit)
            print(json.dumps({"flags": st["flags"], "kernel_ms": st["kernel_ms"], "wall_ms": st["wall_ms"]}))
        return
    res = {"scene": "sponza_like", "triangles": int(len(scene.triangles)), "vertices": int(len(scene.vertices))}
    with api.Context() as ctx:
        ups = []
        for r in range(4):
            t0 = time.perf_counter()
            ctx.upload_scene(scene)
            ups.append((time.perf_counter() - t0) * 1e3)
        res["upload_wall_ms"] = med(ups[1:])
        res["bvh_nodes"] = ctx.stats()["bvh_nodes"]
        pos = [jit, np.ascontiguousarray(scene.vertices["position"], dtype=F32)]
        rk, rw, rcall = [], [], []
        for r in range(11):
            t0 = time.perf_counter()
            st = ctx.update_geometry(pos[r % 2])
            t1 = (time.perf_counter() - t0) * 1e3
            if r:
                rk.append(st["kernel_ms"]); rw.append(st["wall_ms"]); rcall.append(t1)
        res["refit_host_input"] = {"kernel_ms": med(rk), "wall_ms": med(rw), "python_call_ms": med(rcall), "first_call_wall_ms": None}
        if torch is not None:
            dev = [torch.from_numpy(p).to("cuda:0") for p in pos]
            dk, dw = [], []
            for r in range(11):
                st = ctx.update_geometry(dev[r % 2])
                if r:
                    dk.append(st["kernel_ms"]); dw.append(st["wall_ms"])
            res["refit_device_input"] = {"kernel_ms": med(dk), "wall_ms": med(dw)}
        bw = []
        for r in range(4):
            st = ctx.update_geometry(pos[r % 2], rebuild=True)
            assert st["flags"] == api.STAT_REBUILT
            if r:
                bw.append(st["wall_ms"])
        res["rebuild_wall_ms"] = med(bw)
    with api.Context() as ctx:  # the first update of a tree also makes the refit's view of it
        ctx.upload_scene(scene)
        st = ctx.update_geometry(jit)
        res["refit_host_input"]["first_call_wall_ms"] = st["wall_ms"]
    cam = None
    degr = {}
    for kind in ("jitter", "large"):
        p = moved(scene, kind)
        ms = with_positions(scene, p)
        inc = incoherent_rays(ms, 1 << 21)
        with api.Context() as refit, api.Context() as fresh:
            refit.upload_scene(scene)
            refit.update_geometry(p)
            fresh.upload_scene(ms)
            if cam is None:
                cam = fresh.camera_rays(1920, 1080, scene.camera)
            a, b = trace_times([refit, fresh], ms, cam, inc)
            degr[kind] = {"refit": a, "rebuilt": b, "ratio": {k: a[k] / b[k] for k in a}}
    res["degradation"] = degr
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(s)


if __name__ == "__main__":
    main()
