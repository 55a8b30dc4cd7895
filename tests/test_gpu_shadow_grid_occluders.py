"""The light grids' lists (csrc/shadow_grid.h, read through csrc/shadow_grid_walk.h) on the scenes that were made for the resident
occluder map - one candidate triangle per light and coarse cell, tested before the cell's block; it answered 46 % of the headline
frame's shadow segments, made the frame slower and was removed again - and that exercise the walk where occluders sit well
before a segment's end: a frame rendered with the grids and one rendered with RT_FLAG_NO_SHADOW_GRID must carry the same bits over plain
occluders under every kind of light, with lit geometry in front of an occluder and on it, with triangles that are degenerate for the
test (edge-on, in the light's plane, slivers), with cells over `heavy`, without grids, after geometry updates that move the occluder or
remove records, on small soups, and for rt_direct_light.  The geometry is checked on the CPU to put vertices behind the occluder, and
the counters say that the lists answered."""
import os

import numpy as np
import pytest

from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T
from test_gpu_adversarial import _grid, _scene

pytestmark = pytest.mark.gpu

W = HGT = 64
SPP, BOUNCES = 4, 2
MISS = 0xFFFFFFFF


class _env:
    """Development knobs of the grids' build (read when the grids are built: rt_prepare / the first frame after an upload or update)."""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _quad(z, half, cx=0.0, cy=0.0):
    a, b, c, d = (cx - half, cy - half, z), (cx + half, cy - half, z), (cx + half, cy + half, z), (cx - half, cy + half, z)
    return np.array([(a, b, c), (a, c, d)], np.float32)


def _frames(ctx, scene, camera=None):
    """The frame with the grids, the frame without, and the counted frame's use of the lists."""
    cam = scene.camera if camera is None else camera
    st_ref = ctx.render(W, HGT, cam, mode=2, spp=SPP, max_bounces=BOUNCES, frame_seed=9, no_shadow_grid=True)
    ref = ctx.read_rgb32f().copy()
    st = ctx.render(W, HGT, cam, mode=2, spp=SPP, max_bounces=BOUNCES, frame_seed=9)
    got = ctx.read_rgb32f().copy()
    assert (st_ref["primary_rays"], st_ref["continuation_rays"], st_ref["shadow_rays"]) == (st["primary_rays"], st["continuation_rays"], st["shadow_rays"])
    ctx.render(W, HGT, cam, mode=2, spp=SPP, max_bounces=BOUNCES, frame_seed=9, counters=True)
    counted = ctx.read_rgb32f()
    return ref, got, counted, st, ctx.debug_shadow_grid()


def _assert_same_bits(scene, ref, got, counted):
    for name, img in (("grids", got), ("grids, counting kernels", counted)):
        diff = np.flatnonzero((ref.view(np.uint32) != img.view(np.uint32)).reshape(HGT * W, -1).any(axis=1))
        assert diff.size == 0, f"{scene.name} ({name}): {diff.size} pixels differ from the BVH's frame, first at {divmod(int(diff[0]), W)[::-1]}"


def _same_frame(ctx, scene, camera=None, upload=True):
    if upload:
        ctx.upload_scene(scene)
        ctx.prepare()
    ref, got, counted, st, use = _frames(ctx, scene, camera)
    _assert_same_bits(scene, ref, got, counted)
    assert use["segments_answered"] <= st["shadow_rays"]
    print(scene.name, "segments", st["shadow_rays"], "lists", use)
    return st, use


def _hit_points(ctx, scene, camera=None):
    """The first vertices of the frame's paths: the camera rays' hits -> (points (n, 3) float64, prim ids)."""
    pts = ctx.surface(ctx.camera_rays(W, HGT, scene.camera if camera is None else camera, mode=1))
    prim = np.ascontiguousarray(pts[:, 3]).view(np.uint32)
    keep = prim != MISS
    return pts[keep, 0:3].astype(np.float64), prim[keep]


def _segments_hit(points, toward, tris):
    """CPU, float64: for each point, whether the segment from it toward the light (`toward`: (n, 3) end points) crosses one of `tris`."""
    o, d = points, toward - points
    hit = np.zeros(len(points), bool)
    for v0, v1, v2 in np.asarray(tris, np.float64):
        e1, e2 = v1 - v0, v2 - v0
        h = np.cross(d, e2)
        a = h @ e1
        with np.errstate(all="ignore"):
            f = 1.0 / a
            s = o - v0
            u = f * np.einsum("ij,ij->i", s, h)
            q = np.cross(s, e1)
            v = f * np.einsum("ij,ij->i", d, q)
            t = f * (q @ e2)
        hit |= (np.abs(a) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-3) & (t < 1 - 1e-3)
    return hit


def _toward(light_kind, points, position, direction):
    return points - 100.0 * np.asarray(direction, np.float64) if light_kind == "directional" else np.broadcast_to(np.asarray(position, np.float64), points.shape)


# 1. an occluder over a floor ------------------------------------------------------------------------------------------------------
LIGHT_POS, LIGHT_DIR = (0.3, 0.2, 1.0), (-0.5, -0.3, -1.0)  # (slanted: the quad's shadow must not hide behind the quad itself)


def _occluder_scene(kind):
    floor, ids = _grid(24, 24, z=-4.0, size=6.0)
    quad = _quad(-2.0, 0.9)
    light = {"point": H.light_point(LIGHT_POS, (1, 1, 1), 30.0), "spot": H.light_spot(LIGHT_POS, (-0.05, -0.03, -1.0), (1, 1, 1), 40.0, 30.0, 0.5, 0.9),
             "directional": H.light_directional(LIGHT_DIR, (1, 1, 1), 0.9)}[kind]
    return _scene(f"occluder over a floor, {kind} light", np.concatenate([floor, quad]), list(ids) + [2, 2], lights=np.array([light], dtype=T.LIGHT)), quad


@pytest.mark.parametrize("kind", ["point", "spot", "directional"])
def test_occluder_over_a_floor(gpu_ctx, kind):
    scene, quad = _occluder_scene(kind)
    gpu_ctx.upload_scene(scene)
    gpu_ctx.prepare()
    assert gpu_ctx.debug_shadow_grid()["lights_with_grid"] == 1
    points, prim = _hit_points(gpu_ctx, scene)
    behind = _segments_hit(points, _toward(kind, points, LIGHT_POS, LIGHT_DIR), quad)
    assert behind.sum() > 50, "the geometry must put camera-visible floor points behind the quad"
    st, use = _same_frame(gpu_ctx, scene, upload=False)
    assert use["segments_answered"] > 0


# 2. lit geometry in front of the occluder, and on it ----------------------------------------------------------------------------------
def test_object_in_front_of_the_occluder_stays_lit(gpu_ctx):
    floor, ids = _grid(24, 24, z=-4.0, size=6.0)
    quad = _quad(-2.0, 1.2)
    small = _quad(-0.5, 0.25, cx=0.1, cy=0.05)  # between the light and the quad: lit
    tris = np.concatenate([floor, quad, small])
    scene = _scene("object in front of the occluder", tris, list(ids) + [2, 2, 0, 0], lights=np.array([H.light_point(LIGHT_POS, (1, 1, 1), 30.0)], dtype=T.LIGHT))
    gpu_ctx.upload_scene(scene)
    gpu_ctx.prepare()
    points, prim = _hit_points(gpu_ctx, scene)
    n_floor = len(floor)
    on_quad, on_small = (prim == n_floor) | (prim == n_floor + 1), prim >= n_floor + 2
    toward = _toward("point", points, LIGHT_POS, None)
    assert on_small.sum() > 20 and not _segments_hit(points[on_small], toward[on_small], np.concatenate([quad, floor])).any(), "the small object is lit"
    quad_behind_small = _segments_hit(points[on_quad], toward[on_quad], small)
    assert quad_behind_small.any() and (~quad_behind_small).sum() > 50, "vertices ON the quad: some lit, some behind the small object"
    st, use = _same_frame(gpu_ctx, scene, upload=False)
    assert use["segments_answered"] > 0


# 3. triangles the test has special cases for, cells over heavy, no grids ----------------------------------------------------
def _edge_case_scene():
    floor, ids = _grid(20, 20, z=-4.0, size=6.0)
    blade = np.array([[(-1.0, 0.5, -3.0), (1.0, 0.5, -3.0), (0.0, 0.5, -1.0)]], np.float32)           # in the plane y = 0.5
    slivers = np.array([[(-2.0, y, -2.5), (2.0, y + 1.0e-4, -2.5), (2.0, y, -2.5)] for y in np.linspace(-1.5, 1.5, 13)] +
                       [[(x, -2.0, -3.2), (x + 3.0e-5, 2.0, -3.2), (x, 2.0, -3.2)] for x in np.linspace(-1.0, 1.0, 9)], np.float32)
    quad = _quad(-2.0, 0.6, cx=-0.8, cy=-0.7)
    lights = np.array([
        H.light_point((0.0, 0.5, 2.0), (1, 1, 1), 30.0),                    # IN the blade's plane: every ray of it sees the blade edge-on (a = 0)
        H.light_point((0.2, 0.5 + 2.0e-5, 1.5), (1, 0.9, 0.8), 20.0),       # a hair off that plane: |a| around the test's 1e-5
        H.light_directional((0.0, 0.0, -1.0), (1, 1, 1), 0.4),              # along the blade's plane and the slivers' normals
        H.light_spot((0.5, -0.5, 1.0), (-0.1, 0.1, -1.0), (1, 1, 1), 30.0, 30.0, 0.5, 0.9),
    ], dtype=T.LIGHT)
    tris = np.concatenate([floor, blade, slivers, quad])
    return _scene("edge cases", tris, list(ids) + [1] + [3] * len(slivers) + [2, 2], lights=lights)


@pytest.mark.parametrize("knobs", [{}, {"RT_SHADOW_GRID_HEAVY": 1, "RT_SHADOW_GRID_MEAN": "1e9"}], ids=["default", "cells over heavy"])
def test_edge_cases(gpu_ctx, knobs):
    """Edge-on triangles, a light in a triangle's plane, slivers; heavy = 1: every cell with two triangles, the floor's among them, is
    left to the BVH."""
    scene = _edge_case_scene()
    with _env(**knobs):
        gpu_ctx.upload_scene(scene)
        gpu_ctx.prepare()
    assert gpu_ctx.debug_shadow_grid()["lights_with_grid"] == len(scene.lights)
    st, use = _same_frame(gpu_ctx, scene, upload=False)
    assert use["segments_answered"] > 0
    if knobs:
        assert max(gpu_ctx.debug_shadow_grid(i)["heavy_cells"] for i in range(len(scene.lights))) > 0


def test_a_scene_without_grids(gpu_ctx):
    """Coordinates too large for a grid: no light gets one and nothing else differs."""
    floor, ids = _grid(8, 8, z=-4.0, size=4.0)
    far = np.concatenate([floor, _quad(-3.2, 0.6)]) + np.float32(2.0e7)
    cam = H.camera(position=(2.0e7, 2.0e7, 2.0e7))
    scene = _scene("far away", far, list(ids) + [1, 1], camera=cam)
    st, use = _same_frame(gpu_ctx, scene, camera=cam)
    assert use["lights_with_grid"] == 0 and use["segments_answered"] == 0 and gpu_ctx.stats()["grid_bytes"] == 0


# 4. geometry updates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rebuild", [False, True], ids=["refit", "rebuild with fewer records"])
def test_nothing_stale_after_a_geometry_update(gpu_ctx, rebuild):
    """The occluder moves out of the way (and, with a rebuild, half of the floor's triangles become non-finite and lose their records):
    the grids are built again from the new records, and the frame is the one a fresh upload of the moved scene gives."""
    scene, quad = _occluder_scene("point")
    gpu_ctx.upload_scene(scene)
    gpu_ctx.prepare()
    _same_frame(gpu_ctx, scene, upload=False)
    pos = np.ascontiguousarray(scene.vertices["position"], np.float32).copy()
    pos[-6:] += np.float32((40.0, 0.0, 0.0))  # the quad's two triangles (no vertex sharing): far to the side
    if rebuild:
        pos[: 3 * (len(scene.triangles) // 2)] = np.nan
    gpu_ctx.update_geometry(pos, rebuild=rebuild)
    moved = scenes.Scene(scene.name + ", moved", scene.spheres, scene.lights, scene.vertices.copy(), scene.triangles, scene.materials, scene.camera)
    moved.vertices["position"] = pos
    points, _ = _hit_points(gpu_ctx, moved)
    assert not _segments_hit(points, _toward("point", points, LIGHT_POS, None), pos[-6:].reshape(2, 3, 3)).any()
    ref, got, counted, st, use = _frames(gpu_ctx, moved)  # (the first frame builds the grids again)
    _assert_same_bits(moved, ref, got, counted)
    assert use["lights_with_grid"] == 1 and use["segments_answered"] > 0
    # the same frame from a fresh upload of the moved scene
    gpu_ctx.upload_scene(moved)
    gpu_ctx.render(W, HGT, moved.camera, mode=2, spp=SPP, max_bounces=BOUNCES, frame_seed=9)
    np.testing.assert_array_equal(gpu_ctx.read_rgb32f().view(np.uint32), got.view(np.uint32))


# 5. random soups -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(24))
def test_random_soups(gpu_ctx, case):
    n_tris = 300 + (case * 1700) // 23  # 300 .. 2000
    scene = scenes.random_soup(n_tris, seed=100 + case, n_spheres=case % 3, n_lights=2 + case % 2)  # point, directional (and spot) lights
    with _env(RT_SHADOW_GRID_MEAN="1e9"):  # (a small soup's lists are long for its few cells: keep the grids)
        gpu_ctx.upload_scene(scene)
        gpu_ctx.prepare()
    assert gpu_ctx.debug_shadow_grid()["lights_with_grid"] > 0
    _same_frame(gpu_ctx, scene, upload=False)


# 6. rt_direct_light ----------------------------------------------------------------------------------------------------------------
def test_direct_light_matches_the_tree(gpu_ctx):
    scene, quad = _occluder_scene("point")
    gpu_ctx.upload_scene(scene)
    rays = gpu_ctx.camera_rays(W, HGT, scene.camera, mode=1)
    pts = gpu_ctx.surface(rays)
    pts = np.ascontiguousarray(pts[np.ascontiguousarray(pts[:, 3]).view(np.uint32) != MISS])
    tree = gpu_ctx.direct_light(pts, counters=True)
    assert gpu_ctx.debug_shadow_grid()["segments_answered"] == 0
    gpu_ctx.prepare()
    with_lists = gpu_ctx.direct_light(pts, counters=True)
    st, use = gpu_ctx.stats(), gpu_ctx.debug_shadow_grid()
    assert with_lists.tobytes() == tree.tobytes()
    behind = _segments_hit(pts[:, 0:3].astype(np.float64), _toward("point", pts[:, 0:3].astype(np.float64), LIGHT_POS, None), quad)
    assert behind.sum() > 50 and 0 < use["segments_answered"] <= st["rays"]
    assert gpu_ctx.direct_light(pts, use_grids=False).tobytes() == tree.tobytes()
