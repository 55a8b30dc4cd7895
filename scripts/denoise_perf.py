"""rt_aovs and rt_denoise on sponza-like (262 k triangles): the AOV pass at 1, 16 and 64 spp and the denoiser at the default parameters,
at 1080p and 4K; then the sweep the defaults were chosen by (DESIGN.md "Feature buffers and the a-trous denoiser").

    python scripts/denoise_perf.py [--out FILE.json] [--no-sweep]

Times: kernel_ms = HIP events of the library (rt_stats), wall_ms = host time of the call; medians of 5 calls after a warm-up, with
device buffers (torch) so that the denoiser's times hold no copies.  Sweep: cornell12 and sponza-like at 256 x 256, 4 spp, 4 bounces;
MSE of the raw and of the denoised image against a 1024-spp frame of the same view (another seed); the ratio denoised / raw per setting."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch  # before any context: torch's device runtime comes up first
except ImportError:
    torch = None
from gpu_raytracer_amd import api, scenes  # noqa: E402

SIZES = {"1080p": (1920, 1080), "4K": (3840, 2160)}


def median_stats(fn, reps=5):
    fn()
    runs = []
    for _ in range(reps):
        st = fn()
        runs.append((st["kernel_ms"], st["wall_ms"]))
    k, w = np.median(np.array(runs), axis=0)
    return {"kernel_ms": round(float(k), 3), "wall_ms": round(float(w), 3)}


def perf(ctx, scene):
    out = {}
    for size, (w, h) in SIZES.items():
        dev = "cuda:0" if torch is not None else None
        aov = torch.empty((h, w, 8), device=dev) if dev else None
        for spp in (1, 16, 64):
            if size == "4K" and spp == 64:
                continue
            def run_aovs(spp=spp):
                ctx.aovs(w, h, scene.camera, mode=2, spp=spp, out=aov)
                return ctx.stats()
            out[f"aovs_{size}_{spp}spp"] = median_stats(run_aovs)
            print(f"aovs {size} {spp} spp: {out[f'aovs_{size}_{spp}spp']}", flush=True)
        ctx.render(w, h, scene.camera, mode=2, spp=1, max_bounces=4)
        rgb = ctx.read_rgb32f()
        rgb_d = torch.from_numpy(rgb).to(dev) if dev else rgb
        aov_d = aov if dev else ctx.aovs(w, h, scene.camera, mode=2, spp=1)
        den = torch.empty_like(rgb_d) if dev else np.empty_like(rgb)

        def run_denoise():
            ctx.denoise(rgb_d, aov_d, out=den)
            return ctx.stats()
        out[f"denoise_{size}"] = median_stats(run_denoise)
        print(f"denoise {size} ({api.DENOISE_DEFAULTS['iterations']} iterations): {out[f'denoise_{size}']}", flush=True)
    return out


def sweep_case(ctx, scene, w=256, h=256, spp=4, bounces=4):
    ctx.upload_scene(scene)
    kw = dict(mode=2, max_bounces=bounces, frame_seed=1)
    ctx.render(w, h, scene.camera, spp=1024, **dict(kw, frame_seed=99))
    ref = ctx.read_rgb32f().astype(np.float64)
    ctx.render(w, h, scene.camera, spp=spp, **kw)
    raw = ctx.read_rgb32f()
    return raw, ctx.aovs(w, h, scene.camera, spp=spp, **kw), ref


GRID = dict(iterations=(2, 3, 4, 5), sigma_color=(0.5, 1.0, 2.0, 4.0, 8.0, 16.0), sigma_normal=(0.3, 1.0, 2.0), sigma_depth=(0.02, 0.05, 0.1),
            sigma_albedo=(0.1, 0.3, 1.0))


def sweep(ctx):
    cases = {name: sweep_case(ctx, fn()) for name, fn in (("cornell12", scenes.cornell12), ("sponza_like", scenes.sponza_like))}
    raw_mse = {name: float(np.mean((raw - ref) ** 2)) for name, (raw, _, ref) in cases.items()}
    rows = []
    for values in itertools.product(*GRID.values()):
        prm = dict(zip(GRID.keys(), values))
        ratios = {}
        for name, (raw, aov, ref) in cases.items():
            den = ctx.denoise(raw, aov, **prm)
            ratios[name] = float(np.mean((den - ref) ** 2)) / raw_mse[name]
        rows.append(dict(prm, **{f"ratio_{k}": round(v, 4) for k, v in ratios.items()}))
    # the defaults: the setting whose worse ratio (of the two scenes) is the lowest
    rows.sort(key=lambda r: max(r["ratio_cornell12"], r["ratio_sponza_like"]))
    defaults = {k: v for k, v in rows[0].items()}
    at_defaults = [r for r in rows if all(r[k] == api.DENOISE_DEFAULTS[k] for k in GRID)]
    print("raw MSE:", raw_mse)
    print("best 10:")
    for r in rows[:10]:
        print(" ", r)
    print("committed defaults:", at_defaults[0] if at_defaults else "not on the grid")
    return {"raw_mse": raw_mse, "best": rows[:20], "chosen": defaults, "at_committed_defaults": at_defaults[0] if at_defaults else None,
            "n_settings": len(rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    res = {}
    with api.Context() as ctx:
        scene = scenes.sponza_like()
        ctx.upload_scene(scene)
        res["perf_sponza_like"] = perf(ctx, scene)
        if not args.no_sweep:
            res["sweep"] = sweep(ctx)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
