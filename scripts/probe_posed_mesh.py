"""rt_sweep_mesh and rt_overlap_mesh on sponza-like (262 k triangles, device-built tree), beside the composition they replace.

    python scripts/probe_posed_mesh.py [--out FILE.json] [--commit HASH] [--poses N] [--reps R]

N (default 2^16) poses near surfaces with random rotations, swept toward the surface with tmax = inf; two meshes: the 12-triangle box
hull of half extent 0.05 and a 256-triangle sphere-like hull (16 segments x 8 rings) of radius 0.05.  Everything is device-resident, the
results too.  Variants, per mesh:
  sweep_shared, sweep_plain     rt_sweep_mesh with the lanes of a pose sharing their best time, and without (RT_POSED_MESH_SHARE=0)
  sweep_triangles               rt_sweep_triangle over the same N * m triangles, posed beforehand: the composition it replaces
  overlap_count, overlap_any    rt_overlap_mesh, counting and with RT_OVERLAP_ANY
  triangles_count, triangles_any   rt_overlap_triangle over the posed triangles with RT_QUERY_COUNT_ALL and with RT_OVERLAP_ANY
The comparison EXCLUDES what the composition's caller also pays: transforming N * m triangles, shipping 64 bytes for each, and the
segmented reduction of N * m records per pose.  Times: kernel_ms = the HIP events of the library around its launches (rt_stats).  Every
variant is warmed up twice, then the variants take turns for R rounds (at least 11); reported are the median of each variant's R times
and their spread (min, max).  One more run of each with RT_QUERY_COUNTERS gives node visits and triangle tests per pose.  Before
anything is timed the answers of the first 256 poses are held to the numpy reduction of the triangle calls' records.  A record, not a
gate: no threshold is set on these numbers."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  before any context: torch's device runtime comes up first
import posed_mesh_cases as pm  # noqa: E402
from gpu_raytracer_amd import api, scenes  # noqa: E402

DEV = "cuda:0"
CHECKED = 256
CALLS = ("sweep_shared", "sweep_plain", "sweep_triangles", "overlap_count", "overlap_any", "triangles_count", "triangles_any")


def sphere_hull(radius=0.05, segments=16, rings=8):
    """2 * segments * rings triangles on a sphere; the ones at the poles are segments, which the calls allow."""
    th = np.linspace(0.0, np.pi, rings + 1)
    ph = np.linspace(0.0, 2.0 * np.pi, segments + 1)
    p = radius * np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None]], -1)
    a, b, c, d = p[:-1, :-1], p[1:, :-1], p[1:, 1:], p[:-1, 1:]
    v = np.concatenate([np.stack([a, b, c], -2).reshape(-1, 3, 3), np.stack([a, c, d], -2).reshape(-1, 3, 3)]).astype(np.float32)
    return api.make_triangles(v[:, 0], v[:, 1], v[:, 2])


def pose_on_device(mesh, sweeps, R):
    """api.pose_triangles in torch, operation for operation (every elementwise op rounds once) -> (N * M, 16) triangle sweeps."""
    n, m = sweeps.shape[0], mesh.shape[0]
    out = torch.zeros((n, m, 16), dtype=torch.float32, device=DEV)
    for k in range(3):
        v = mesh[None, :, 4 * k:4 * k + 3]
        for a in range(3):
            r = (R[:, a, 0, None] * v[:, :, 0] + R[:, a, 1, None] * v[:, :, 1]) + R[:, a, 2, None] * v[:, :, 2]
            out[:, :, 4 * k + a] = r + sweeps[:, a, None]
    out[:, :, 12:16] = sweeps[:, None, 8:12]
    return out.reshape(n * m, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--poses", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    reps, n = max(args.reps, 11), args.poses
    scene = scenes.sponza_like()
    rng = np.random.default_rng(5)
    p, normal = pm.surface_points(scene, n, rng)
    normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-30)
    off = normal * rng.choice([-1.0, 1.0], (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3))
    sweeps = api.make_pose_sweeps((p + off * rng.uniform(0.05, 0.5, (n, 1))).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32),
                                  (-off).astype(np.float32), np.inf)
    R = torch.from_numpy(api.pose_frames(sweeps)[0]).to(DEV)
    res = {"commit": args.commit, "scene": scene.name, "triangles": scene.n_triangles, "poses": n, "reps": reps, "meshes": {}}
    with api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        d_sweeps = torch.from_numpy(sweeps).to(DEV)
        d_poses = d_sweeps[:, :8].contiguous()
        for name, mesh in (("box12", pm.box_hull(0.05)), ("sphere256", sphere_hull())):
            m = len(mesh)
            d_mesh = torch.from_numpy(mesh).to(DEV)
            d_tris = pose_on_device(d_mesh, d_sweeps, R)
            d_static = d_tris[:, :12].contiguous()
            assert np.array_equal(d_tris[:CHECKED * m].cpu().numpy().view(np.uint32), pm.posed_sweeps(mesh, sweeps[:CHECKED]).view(np.uint32)), "not the posing statement"
            out = torch.empty((n, 8), dtype=torch.float32, device=DEV)
            tri_out = torch.empty((n * m, 8), dtype=torch.float32, device=DEV)
            tri_counts = torch.empty((n * m,), dtype=torch.int32, device=DEV)

            def run(call, counters=False):
                """-> (kernel_ms, node visits, triangle tests, the result)"""
                os.environ["RT_POSED_MESH_SHARE"] = "0" if call == "sweep_plain" else "1"
                if call in ("sweep_shared", "sweep_plain"):
                    got = ctx.sweep_mesh(d_mesh, d_sweeps, out=out, counters=counters)
                elif call == "sweep_triangles":
                    got = ctx.sweep_triangle(d_tris, out=tri_out, counters=counters)
                elif call in ("overlap_count", "overlap_any"):
                    got = ctx.overlap_mesh(d_mesh, d_poses, any_hit=call == "overlap_any", counters=counters)
                else:
                    got = ctx.overlap_triangle(d_static, 0, counts=tri_counts, count_all=call == "triangles_count", any_hit=call == "triangles_any",
                                               counters=counters)[1]
                s = ctx.stats()
                return s["kernel_ms"], s["node_visits"], s["tri_tests"], got

            # the answers, before anything is timed
            valid = np.ones(CHECKED, bool)
            rec = run("sweep_triangles")[3][:CHECKED * m].cpu().numpy().reshape(CHECKED, m, 8)
            want = pm.reduce_sweep(rec, sweeps[:CHECKED, 11], valid).view(np.uint32)
            for call in ("sweep_shared", "sweep_plain"):
                assert np.array_equal(run(call)[3][:CHECKED].cpu().numpy().view(np.uint32), want), call
            counts = run("triangles_count")[3][:CHECKED * m].cpu().numpy().view(np.uint32).reshape(CHECKED, m)
            pairs = pm.reduce_overlap(counts, valid)[0]
            assert np.array_equal(run("overlap_count")[3][:CHECKED].cpu().numpy().view(np.uint32), pairs)
            assert np.array_equal(run("overlap_any")[3][:CHECKED].cpu().numpy().view(np.uint32), (pairs > 0).astype(np.uint32))
            hits = run("sweep_shared")[3].cpu().numpy().view(np.uint32)
            entry = {"m": m, "group": min(64, 1 << (m - 1).bit_length()),
                     "hit": round(float((hits[:, 6] != 0xFFFFFFFF).mean()), 4), "at_start": round(float(((hits[:, 6] != 0xFFFFFFFF) & (hits[:, 3] == 0)).mean()), 4),
                     "variants": {}}
            times = {call: [] for call in CALLS}
            for call in CALLS:
                for _ in range(2):
                    run(call)
            for _ in range(reps):
                for call in CALLS:
                    times[call].append(run(call)[0])
            for call in CALLS:
                _, visits, tests, _ = run(call, counters=True)
                med = float(np.median(times[call]))
                entry["variants"][call] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(times[call]), 4), "kernel_ms_max": round(max(times[call]), 4),
                                           "poses_per_s": round(n / (med * 1e-3)), "node_visits_per_pose": round(visits / n, 2),
                                           "tri_tests_per_pose": round(tests / n, 2)}
                print(name, call, entry["variants"][call], flush=True)
            res["meshes"][name] = entry
            del d_tris, d_static, tri_out, tri_counts
        os.environ.pop("RT_POSED_MESH_SHARE", None)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
