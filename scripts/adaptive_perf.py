"""Adaptive sampling (rt_render_adaptive) on sponza-like (262 k triangles), 1080p, 4 bounces, 8 spp per call: its overhead at threshold 0
against plain accumulation, the call time against the fraction of live pixels (and the fixed floor of a call whose pixels have all
stopped), and the MSE it buys at equal device time ("Adaptive sampling").

    python scripts/adaptive_perf.py [--out FILE.json] [--no-mse]

Times: kernel_ms = HIP events of the library (rt_stats), wall_ms = host time of the call; medians after a warm-up.  Overhead: calls that
each start a new image (restart), so that every call traces 8 spp for every pixel; plain and adaptive alternate.  Scaling: each measured
call follows two threshold-0 calls of a new image (16 samples per pixel), its threshold a quantile of the errors they leave.  MSE: 960 x
540, uniform and adaptive accumulation in calls of 8 spp against a 1024-spp frame of another seed, compared at equal device time."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_raytracer_amd import api, scenes  # noqa: E402

W, H, BOUNCES, SPP = 1920, 1080, 4, 8


def np_error(rec):
    """The rule's error (rt_hip.h) from rt_read_adaptive's records, in float32."""
    s, n, hh = rec[..., 0:3], rec[..., 3], rec[..., 4:7]
    with np.errstate(all="ignore"):
        i = s / n[..., None]
        a = (hh + hh) / n[..., None]
        d = np.abs(i[..., 0] - a[..., 0]) + np.abs(i[..., 1] - a[..., 1]) + np.abs(i[..., 2] - a[..., 2])
        return d / (np.float32(1e-4) + np.sqrt(i[..., 0] + i[..., 1] + i[..., 2]))


def med(runs):
    k, w = np.median(np.array([(s["kernel_ms"], s["wall_ms"]) for s in runs]), axis=0)
    return {"kernel_ms": round(float(k), 3), "wall_ms": round(float(w), 3)}


def overhead(ctx, scene, reps):
    plain = lambda: ctx.render(W, H, scene.camera, mode=2, spp=SPP, max_bounces=BOUNCES, accumulate=True, restart=True)
    adaptive = lambda: ctx.render_adaptive(W, H, scene.camera, SPP, 0.0, max_bounces=BOUNCES, restart=True)
    for _ in range(2):
        plain(), adaptive()
    a, b = [], []
    for _ in range(reps):
        a.append(plain())
        b.append(adaptive())
    out = {"plain_accumulating": med(a), "adaptive_threshold0": med(b)}
    out["overhead_kernel_pct"] = round(100.0 * (out["adaptive_threshold0"]["kernel_ms"] / out["plain_accumulating"]["kernel_ms"] - 1.0), 2)
    out["overhead_wall_pct"] = round(100.0 * (out["adaptive_threshold0"]["wall_ms"] / out["plain_accumulating"]["wall_ms"] - 1.0), 2)
    return out


def scaling(ctx, scene, reps):
    warm = lambda: [ctx.render_adaptive(W, H, scene.camera, SPP, 0.0, max_bounces=BOUNCES, restart=i == 0) for i in range(2)]
    warm()
    e = np_error(ctx.read_adaptive())
    e = e[np.isfinite(e)]
    levels = {"100%": 0.0, "50%": float(np.quantile(e, 0.5)), "10%": float(np.quantile(e, 0.9)), "1%": float(np.quantile(e, 0.99)),
              "0% (floor)": float(np.inf)}
    out = {}
    for name, t in levels.items():
        runs = []
        for _ in range(reps + 1):
            warm()
            st = ctx.render_adaptive(W, H, scene.camera, SPP, min(t, 3.0e38), max_bounces=BOUNCES)
            runs.append(st)
        runs = runs[1:]
        out[name] = dict(med(runs), threshold=t if np.isfinite(t) else "max", live_fraction=round(runs[-1]["pixels"] / (W * H), 4))
        print(f"live {name}: {out[name]}", flush=True)
    return out


def mse_at_equal_time(ctx, scene):
    w, h = 960, 540
    ctx.render(w, h, scene.camera, mode=2, spp=1024, max_bounces=BOUNCES, frame_seed=12345)
    ref = ctx.read_rgb32f().astype(np.float64)
    mse = lambda: float(np.mean((ctx.read_rgb32f().astype(np.float64) - ref) ** 2))
    uniform, t_uniform = [], 0.0
    for i in range(8):
        t_uniform += ctx.render(w, h, scene.camera, mode=2, spp=SPP, max_bounces=BOUNCES, accumulate=True, restart=i == 0)["kernel_ms"]
        uniform.append({"samples": SPP * (i + 1), "device_ms": round(t_uniform, 3), "mse": mse()})
    out = {"uniform": uniform}
    for q in (0.1, 0.25, 0.5):
        curve, t_ad = [], 0.0
        for i in range(2):
            t_ad += ctx.render_adaptive(w, h, scene.camera, SPP, 0.0, min_samples=16, max_bounces=BOUNCES, restart=i == 0)["kernel_ms"]
        e = np_error(ctx.read_adaptive())
        thr = float(np.quantile(e[np.isfinite(e)], q))
        curve.append({"samples_max": 16, "device_ms": round(t_ad, 3), "mse": mse()})
        while t_ad < t_uniform and len(curve) < 64:
            st = ctx.render_adaptive(w, h, scene.camera, SPP, thr, min_samples=16, max_bounces=BOUNCES)
            t_ad += st["kernel_ms"]
            curve.append({"samples_max": ctx.accumulated_samples(), "device_ms": round(t_ad, 3), "live_fraction": round(st["pixels"] / (w * h), 4),
                          "mse": mse()})
            if st["pixels"] == 0:
                break
        out[f"adaptive_q{q}"] = {"threshold": thr, "curve": curve}
    print(json.dumps({k: (v[-1] if k == "uniform" else v["curve"][-1]) for k, v in out.items()}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-mse", action="store_true")
    args = ap.parse_args()
    scene = scenes.sponza_like()
    res = {"scene": "sponza_like", "size": [W, H], "bounces": BOUNCES, "spp_per_call": SPP, "version": api.version()}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        ctx.prepare(api.PREPARE_SHADOW_GRIDS)
        res["overhead"] = overhead(ctx, scene, args.reps)
        print("overhead:", res["overhead"], flush=True)
        res["scaling"] = scaling(ctx, scene, args.reps)
        if not args.no_mse:
            res["mse"] = mse_at_equal_time(ctx, scene)
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
