"""Modes 0 and 1 and the ray queries of the HIP path against the independent float64 statement of reference_cases.py.

The same assertions test_reference_oracle.py makes of the CPU oracle, on what librt_hip.so renders on the MI355X: Context.render
in both modes read back through read_hits / read_rgb32f / read_rgba8_channels / read_rgba8_combined, the 130 x 70 case again as
rt_dispatch_tile calls, the three tree builders, and rt_intersect / rt_occluded / rt_camera_rays.  Every frame is also asserted
equal to the oracle's bits: that assertion exists elsewhere, but here it tells a reader which side moved should the statement
ever disagree.  No bound in this file or in reference_cases.py was taken from a HIP result.
"""
import numpy as np
import pytest

import reference_cases as rc
from gpu_raytracer_amd import hostpack as H

pytestmark = pytest.mark.gpu

CASE_IDS = [c.name for c in rc.CASES]


def _read(ctx):
    prim, t = ctx.read_hits()
    red, green, blue = ctx.read_rgba8_channels()
    return {"prim": prim, "t": t, "rgb": ctx.read_rgb32f(), "red": red, "green": green, "blue": blue, "combined": ctx.read_rgba8_combined()}


def _render(ctx, case, mode):
    st = ctx.render(case.w, case.h, case.camera, mode=mode)
    assert st["rays"] == case.w * case.h
    return _read(ctx)


def _assert_same_bits(a, b, what):
    for k in ("prim", "red", "green", "blue", "combined"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(a["rgb"].view(np.uint32), b["rgb"].view(np.uint32), err_msg=f"{what}: rgb")
    hit = a["prim"] != rc.PRIM_MISS
    np.testing.assert_array_equal(a["t"][hit].view(np.uint32), b["t"][hit].view(np.uint32), err_msg=f"{what}: t")


@pytest.mark.parametrize("case", rc.CASES, ids=CASE_IDS)
def test_frame_matches_the_statement(rt_api, oracle_mod, case):
    """Context.render in modes 0 and 1 against the float64 statement (reference_cases.check_frame), against the oracle's bits, and
    a twin upload (other range / cone angles / roughness) against the first one's bits."""
    with rt_api.Context() as ctx, rt_api.Context() as twin_ctx:
        ctx.upload_scene(case.scene)
        if case.twin is not None:
            twin_ctx.upload_scene(case.twin)
        for mode in (0, 1):
            frame = _render(ctx, case, mode)
            rc.check_frame(case, mode, frame, "HIP")
            ref = oracle_mod.render_frame(oracle_mod.PackedScene(case.scene, use_bvh=False), case.w, case.h, camera=case.camera, mode=mode, threads=4)
            _assert_same_bits(frame, ref, f"{case.name} mode {mode} against the oracle")
            if case.twin is not None:
                _assert_same_bits(frame, _render(twin_ctx, case, mode), f"{case.name} mode {mode} against its twin upload")


def test_tile_edge_case_as_dispatch_tile_sequence(gpu_ctx, oracle_mod):
    """130 x 70 through rt_dispatch_tile, one call per tile and channel, on the reference's own packed buffers: the channel
    textures and the combined image against the statement's bytes."""
    case = rc.CASE_BY_NAME["tile_edge_130x70"]
    packed = oracle_mod.PackedScene(case.scene)
    gpu_ctx.upload_scene_packed(packed.metadata, packed.offsets, packed.tri_bufs, packed.triangles_per_buffer, case.scene.materials)
    tx, ty = H.tile_count(case.w, case.h)
    assert tx == 2 and ty == 1
    for mode in (0, 1):
        for tile in range(tx * ty):
            ox, oy = (tile % tx) * 128, (tile // tx) * 128
            for ch in range(3):
                gpu_ctx.dispatch_tile(packed.push_constants(case.w, case.h, channel=ch, mode=mode, tile_offset=(ox, oy)))
        red, green, blue = gpu_ctx.read_rgba8_channels()   # rt_dispatch_tile writes the textures only: no float image, no hit records
        comb = gpu_ctx.read_rgba8_combined()
        rc.check_bytes(case, mode, {"red": red, "green": green, "blue": blue, "combined": comb})
        ref = oracle_mod.render_frame(packed, case.w, case.h, camera=case.camera, mode=mode, threads=4)
        for k, img in (("red", red), ("green", green), ("blue", blue), ("combined", comb)):
            np.testing.assert_array_equal(img, ref[k], err_msg=f"dispatch_tile sequence mode {mode} against the oracle: {k}")


@pytest.mark.parametrize("method", ["0", "1", None], ids=["host_sah", "host_ploc", "device"])
def test_tree_builders(rt_api, oracle_mod, monkeypatch, method):
    """A case padded to 1,024 triangles with far-away geometry behind the camera, through each builder (RT_BUILD_METHOD 0 and 1: the host's
    binned SAH and PLOC; unset: the device build, which starts at 1,024 triangles): the frame is the unpadded case's, and carries
    the bits of the oracle's brute-force frame of the padded scene."""
    case = rc.CASE_BY_NAME["sphere_between_two_triangles"]
    scene = rc.padded(case, 1024)
    assert len(scene.triangles) >= 1024
    if method is None:
        monkeypatch.delenv("RT_BUILD_METHOD", raising=False)
    else:
        monkeypatch.setenv("RT_BUILD_METHOD", method)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.debug_check_bvh()["method"] == (2 if method is None else int(method))
        for mode in (0, 1):
            frame = _render(ctx, case, mode)
            rc.check_frame(case, mode, frame, f"HIP, builder {method or 'device'}")
            ref = oracle_mod.render_frame(oracle_mod.PackedScene(scene, use_bvh=False), case.w, case.h, camera=case.camera, mode=mode, threads=4)
            _assert_same_bits(frame, ref, f"builder {method or 'device'} mode {mode} against the oracle")


# ---- ray queries ---------------------------------------------------------------------------------------------------------
def test_intersect_against_the_float64_closest_hit(gpu_ctx, rt_api):
    """4,096 rays around a 300-triangle soup with three spheres (aimed at triangles, at the spheres, random with unit and non-unit
    directions) plus the camera rays of the case light_directional: primitive equal on the classified rays; t and the barycentrics
    within 4 x what f32 costs, measured on the CPU in units of each ray's conditioning (reference_cases.MEASURED_QUERY_*): about
    1e-5 for the bulk of the rays, more only for a ray that grazes what it hits."""
    scene, rays, hit = rc.query_statement()
    assert hit["unsure"].mean() <= rc.EDGE_SHARE_CAP
    gpu_ctx.upload_scene(scene)
    t, u, v, prim = rt_api.split_hits(gpu_ctx.intersect(rays))
    ok = ~hit["unsure"]
    wrong = ok & (prim != hit["prim"])
    h = ok & (hit["prim"] != rc.PRIM_MISS)
    tri = h & ((hit["prim"] & rc.PRIM_SPHERE) == 0)
    t_err, uv_err = rc.query_errors(hit, t, u, v)
    print(f"intersect: {len(rays)} rays, unsure {hit['unsure'].mean():.4f}, wrong primitive on {wrong.sum()} classified rays, "
          f"|dt| / (t cond) {t_err[h].max():.3e} (bound {rc.QUERY_T_BOUND:.3e}), |du|, |dv| / cond {uv_err[tri].max():.3e} (bound {rc.QUERY_UV_BOUND:.3e})")
    assert not wrong.any()
    assert (t_err[h] <= rc.QUERY_T_BOUND).all() and (uv_err[tri] <= rc.QUERY_UV_BOUND).all()
    # the alternatives this rejects on most triangle hits (test_reference_oracle.py asserts the shares from the statement alone)
    tol_uv = rc.QUERY_UV_BOUND * hit["cond_uv"][tri]
    for name, alt_u in (("u and v swapped", hit["v"]), ("u off by 1e-3", hit["u"] + 1e-3)):
        share = (np.abs(alt_u - hit["u"])[tri] > 2.0 * tol_uv).mean()
        print(f"  alternative {name}: differs by more than twice the tolerance on {share:.3f} of the triangle hits")
        assert share > 0.5


def test_occluded_against_a_hit_exists_in_the_range(gpu_ctx):
    """Rays that end just before and just beyond their closest hit, and that start beyond it: occluded == the float64 statement has
    a hit in (tmin, tmax) on the classified rays."""
    scene, _, _ = rc.query_statement()
    rays, expected, unsure = rc.occlusion_batch()
    assert unsure.mean() <= rc.EDGE_SHARE_CAP
    gpu_ctx.upload_scene(scene)
    got = gpu_ctx.occluded(rays)
    wrong = (got != expected) & ~unsure
    print(f"occluded: {len(rays)} rays, occluded {expected.mean():.3f}, unsure {unsure.mean():.4f}, wrong {wrong.sum()}")
    assert not wrong.any()


@pytest.mark.parametrize("case", [c for c in rc.CASES if c.group == "raygen"], ids=lambda c: c.name)
def test_camera_rays_against_the_float64_ray_generation(gpu_ctx, case):
    """rt_camera_rays in both modes: the origin is the camera's, every direction component within camera_dir_bound (derived from
    the operation count, reference_cases.camera_dir_bound) of the float64 ray-gen; a forward normalised first is rejected."""
    o, d = rc.camera_rays(case.camera, case.w, case.h)
    bound = rc.camera_dir_bound(case.camera, case.w, case.h)
    for mode in (0, 1):
        rays = gpu_ctx.camera_rays(case.w, case.h, case.camera, mode=mode)
        np.testing.assert_array_equal(rays[:, 0:3], np.broadcast_to(o.astype(np.float32), (len(rays), 3)))
        err = np.abs(rays[:, 4:7].astype(np.float64) - d.reshape(-1, 3)).max()
        print(f"{case.name} mode {mode}: largest direction error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    if "normalised_forward" in case.asserted:
        alt = rc.camera_rays(case.camera, case.w, case.h, "normalised_forward")[1]
        share = (np.abs(alt - d).max(-1) > 2 * bound).mean()
        print(f"  alternative normalised_forward: differs by more than twice the bound on {share:.3f} of the frame")
        assert share > 0.5
