"""Direct-light queries on the MI355X (rt_direct_light), held to calls that already exist.

Against the frames: with the ambient term and bias 1e-3, the radiance at rt_surface's hit of a pixel's camera ray - the normal turned
back into the unflipped geometric one - is that pixel of a closed extended-mode frame with one sample and no bounce, bit for bit.
Against its definition: every shadow segment is built here in numpy float32 (the library is built with -ffp-contract=off, so numpy
reproduces every rounding) and traced by rt_occluded; lit_mask must be "faces the light and is not occluded" wherever float64 says
the facing terms are clear of zero.  Against itself: the light grids change no byte, and the counters say that the lists ran."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import hostpack as HP
from gpu_raytracer_amd import types as T

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
MISS = 0xFFFFFFFF
MIN_T = F32(1e-5)
F32_MAX = np.finfo(np.float32).max
EPS = F32(1e-3)
W, H = 64, 48
CLEAR = 1e-4  # a facing or spot term closer to zero than this may round either way: the pair is left out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _length(a):
    with np.errstate(all="ignore"):
        return np.sqrt(_dot32(a, a)).astype(F32)


def _normalize(a):
    with np.errstate(all="ignore"):
        return a * (F32(1.0) / _length(a))[..., None]


def _f16(m, shift):
    return ((np.asarray(m) >> U32(shift)) & U32(0xFFFF)).astype(np.uint16).view(np.float16).astype(np.float64)


# scenes ------------------------------------------------------------------------------------------------------------------------
def _opaque(scene):
    """The scene with every material's transmission set to 0 (the query does not apply the frames' transmission mix)."""
    m = scene.materials.copy()
    ior = m["ior_transmission_f16"] & U32(0xFFFF)
    m["ior_transmission_f16"] = ior | (U32(HP.f16_bits(0.0)) << U32(16))
    return dataclasses.replace(scene, materials=m)


def _scene(name, tris_xyz, mat_ids, lights, camera=None):
    """tris_xyz: (n, 3, 3) triangle corners, no vertex sharing (the construction of test_gpu_adversarial._scene, opaque materials)."""
    tris_xyz = np.asarray(tris_xyz, np.float32).reshape(-1, 3, 3)
    n = len(tris_xyz)
    vertices = np.zeros(n * 3, dtype=T.VERTEX)
    vertices["position"] = tris_xyz.reshape(-1, 3)
    triangles = np.zeros(n, dtype=T.TRIANGLE)
    idx = np.arange(n * 3, dtype=np.uint32).reshape(-1, 3)
    triangles["v0_index"], triangles["v1_index"], triangles["v2_index"] = idx[:, 0], idx[:, 1], idx[:, 2]
    triangles["material_id"] = np.asarray(mat_ids, np.uint32)
    materials = np.array([HP.material_new((0.8, 0.3, 0.3), 0.0, 0.5, (0, 0, 0), 1.5, 0.0), HP.material_new((0.3, 0.8, 0.3), 1.0, 0.2, (0, 0, 0), 1.5, 0.0),
                          HP.material_new((0.9, 0.9, 0.9), 0.0, 0.0, (0, 0, 0), 1.5, 0.0), HP.material_new((0.2, 0.2, 0.9), 0.0, 0.9, (0.4, 0.3, 0.2), 1.5, 0.0)],
                         dtype=T.MATERIAL)
    return scenes.Scene(name, np.zeros(0, dtype=T.SPHERE), lights, vertices, triangles, materials, camera if camera is not None else HP.camera())


def _grid(nx, ny, z, size, mats=4):
    xs, ys = np.linspace(-size / 2, size / 2, nx + 1), np.linspace(-size / 2, size / 2, ny + 1)
    tris, ids = [], []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = (xs[i], ys[j], z), (xs[i + 1], ys[j], z), (xs[i + 1], ys[j + 1], z), (xs[i], ys[j + 1], z)
            tris += [(a, b, c), (a, c, d)]
            ids += [(i + j) % mats, (i * 3 + j) % mats]
    return np.array(tris, np.float32), ids


def _room_scene():
    """test_gpu_shadow_grid.test_lights_in_awkward_places: lights on geometry (the near list), on a triangle's plane, at a corner of
    the room (cube-face seams), far outside, axis-aligned directional lights, a spot light."""
    x0, y0, z0, x1, y1, z1 = -2, -2, -6, 2, 2, -1
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    room = []
    for a, b, cc, d in [(0, 1, 2, 3), (5, 4, 7, 6), (4, 0, 3, 7), (1, 5, 6, 2), (4, 5, 1, 0), (3, 2, 6, 7)]:
        room += [(c[a], c[b], c[cc]), (c[a], c[cc], c[d])]
    room = np.array(room, np.float32)
    floor, ids = _grid(12, 12, z=-5.5, size=3.0)
    blockers = np.array([[(-0.5, -0.5, -3.0), (0.5, -0.5, -3.0), (0.0, 0.5, -3.0)], [(-1.0, 0.2, -4.0), (0.3, 0.1, -4.0), (-0.4, 1.0, -4.2)]], np.float32)
    cam = HP.camera(position=(0.0, 0.0, -1.2), direction=(0.0, -0.1, -1.0))
    lights = np.array([
        HP.light_point((0.0, 0.0, -3.5), (1, 1, 1), 2.0), HP.light_point((0.0, 0.0, -3.0), (1, 0.8, 0.6), 1.0),
        HP.light_point((2.0, 2.0, -1.0), (0.5, 0.7, 1.0), 3.0), HP.light_point((40.0, 55.0, 30.0), (1, 1, 1), 900.0),
        HP.light_directional((0.0, -1.0, 0.0), (1, 1, 1), 0.5), HP.light_directional((0.0, 0.0, -1.0), (1, 1, 1), 0.5),
        HP.light_spot((0.0, 1.9, -3.0), (0.0, -1.0, 0.0), (1, 1, 1), 3.0, 20.0, 0.3, 0.6)], dtype=T.LIGHT)
    return _scene("awkward lights", np.concatenate([room, floor, blockers]), [0] * len(room) + list(ids) + [1, 3], lights, cam)


def _fan_scene():
    """test_gpu_shadow_grid's fan of 300 needles under a point light: lists decided in the cell's block, lists walked on
    (GRID_PENDING), walks that reach their limit and cells over `heavy` (GRID_FORWARD)."""
    n = 300
    ang = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    z = -1.0 + 2.5 * (np.arange(n) * 37 % n) / n
    r1, half = 3.5, 0.004
    c, s = np.cos(ang), np.sin(ang)
    a = np.stack([0 * c, 0 * s, z], 1)
    b = np.stack([r1 * c - half * s, r1 * s + half * c, z], 1)
    d = np.stack([r1 * c + half * s, r1 * s - half * c, z], 1)
    blades = np.stack([a, b, d], 1).astype(np.float32)
    floor, ids = _grid(12, 12, z=-3.0, size=9.0)
    lights = np.array([HP.light_point((0.0, 0.0, 4.0), (1, 1, 1), 30.0), HP.light_directional((0.0, 0.0, -1.0), (1, 1, 1), 0.6)], dtype=T.LIGHT)
    cam = HP.camera(position=(0.0, -6.5, 3.0), direction=(0.0, 6.5, -6.0), up=(0.0, 0.0, 1.0), fov=55.0)
    return _scene("fan", np.concatenate([floor, blades]), list(ids) + [int(i) % 4 for i in range(n)], lights, cam)


@pytest.fixture(scope="module")
def scene_of():
    made = {}
    makers = {"cornell12": scenes.cornell12, "soup": lambda: _opaque(scenes.random_soup(2000, n_spheres=3, n_lights=6)), "room": _room_scene,
              "fan": _fan_scene}
    for seed in (1, 2, 3):
        makers[f"soup{seed}"] = lambda seed=seed: _opaque(scenes.random_soup(30000, seed=seed, n_spheres=3, n_lights=6))

    def get(name):
        if name not in made:
            made[name] = makers[name]()
        return made[name]
    return get


def _incoherent_rays(scene, n, seed):
    rng = np.random.default_rng(seed)
    p = scene.vertices["position"].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    o = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (n, 3)).astype(F32)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return api.make_rays(o, d.astype(F32), MIN_T, np.inf)


def _points(ctx, scene, n_incoherent=2048):
    """The hits of rt_surface over the camera rays of a 64 x 48 frame and over incoherent rays."""
    rays = np.concatenate([ctx.camera_rays(W, H, scene.camera, mode=1), _incoherent_rays(scene, n_incoherent, seed=21)])
    pts = ctx.surface(rays)
    return np.ascontiguousarray(pts[_bits(pts[:, 3]) != MISS])


# the definition ----------------------------------------------------------------------------------------------------------------
def _is_point(points):
    with np.errstate(all="ignore"):
        return np.isfinite(points[:, 0:3]).all(1) & np.isfinite(points[:, 4:7]).all(1) & (points[:, 4:7] != 0).any(1)


def definition(ctx, scene, points, bias=EPS, shadows=True):
    """-> (lit (n, L) bool, clear (n, L) bool, segments): lit[i, li] = light li enters point i's sum, decided where `clear` by float64
    facing / spot terms of the float32 directions the device uses, and by rt_occluded over the float32 segments composed here."""
    n, n_l = len(points), len(scene.lights)
    P, N = points[:, 0:3], points[:, 4:7]
    mid = _bits(points[:, 7]).astype(np.int64)
    real = _is_point(points) & (mid < len(scene.materials))
    albedo = scene.materials["albedo"][np.minimum(mid, len(scene.materials) - 1)]
    lit, clear = np.zeros((n, n_l), bool), np.zeros((n, n_l), bool)
    rays, where = [], []
    with np.errstate(all="ignore"):
        o = P + N * F32(bias)
        for li, L in enumerate(scene.lights):
            neg_ndir = -_normalize(L["direction"].astype(F32)[None, :])[0]
            to_light = L["position"].astype(F32)[None, :] - P
            dist = _length(to_light)
            pld = to_light * (F32(1.0) / dist)[:, None]
            n64, p64, d64 = N.astype(np.float64), pld.astype(np.float64), neg_ndir.astype(np.float64)
            att = 1.0 / (1.0 + dist.astype(np.float64) ** 2 * 0.01)
            kind = int(L["light_type"])
            if kind == 0:
                terms, sdir, sdist = [n64 @ d64], np.broadcast_to(neg_ndir, P.shape), np.full(n, F32_MAX, F32)
            elif kind == 1:
                terms, sdir, sdist = [(n64 * p64).sum(1), att], pld, dist
            else:
                terms, sdir, sdist = [(n64 * p64).sum(1), p64 @ d64, att], pld, dist
            terms = np.stack(terms, 1)
            ok = real & np.isfinite(terms).all(1) & (np.abs(terms) > CLEAR).all(1)
            facing = ok & (terms > 0).all(1) & (albedo != 0).any(1) & bool((L["color"] != 0).any()) & bool(L["intensity"] > 0)
            clear[:, li] = ok
            lit[:, li] = facing
            rows = np.flatnonzero(facing)
            rays.append(api.make_rays(o[rows], sdir[rows], MIN_T, sdist[rows]))
            where.append((rows, li))
    segments = int(lit.sum()) if shadows else 0
    if shadows and segments:
        occ = ctx.occluded(np.ascontiguousarray(np.concatenate(rays))).astype(bool)
        at = 0
        for rows, li in where:
            lit[rows, li] &= ~occ[at:at + len(rows)]
            at += len(rows)
    return lit, clear, segments


def _check_definition(ctx, scene, points, got, bias=EPS, shadows=True, max_excluded=None):
    lit, clear, segments = definition(ctx, scene, points, bias, shadows)
    _, mask = api.split_lighting(got)
    got_bits = ((mask[:, None] >> np.arange(lit.shape[1], dtype=U32)[None, :]) & U32(1)).astype(bool)
    np.testing.assert_array_equal(got_bits[clear], lit[clear])
    real = _is_point(points) & (_bits(points[:, 7]) < len(scene.materials))
    excluded = (~clear[real]).mean() if real.any() and lit.shape[1] else 0.0
    print(f"{scene.name}: {len(points)} points x {lit.shape[1]} lights, {segments} segments, {lit.sum()} lit, excluded pairs {excluded:.4f}")
    if max_excluded is not None:
        assert excluded <= max_excluded
    return lit, clear, segments


# 1. the frames ------------------------------------------------------------------------------------------------------------------
def _geometric_facing(scene, rays, prim, position):
    """cos of the angle between the primitive's unflipped geometric normal and the ray, in float64 from the scene's own arrays."""
    pos = scene.vertices["position"].astype(np.float64)
    cosang = np.zeros(len(rays))
    sphere = prim >= 0x80000000
    tri = ~sphere
    d = rays[:, 4:7].astype(np.float64)
    trs = scene.triangles[prim[tri].astype(np.int64)]
    v0 = pos[trs["v0_index"]]
    ng = np.zeros((len(rays), 3))
    ng[tri] = np.cross(pos[trs["v1_index"]] - v0, pos[trs["v2_index"]] - v0)
    if sphere.any():
        sp = scene.spheres[(prim[sphere] & 0x7FFFFFFF).astype(np.int64)]
        ng[sphere] = position[sphere].astype(np.float64) - sp["center"].astype(np.float64)
    cosang = (ng * d).sum(1) / (np.linalg.norm(ng, axis=1) * np.linalg.norm(d, axis=1))
    return cosang


@pytest.mark.parametrize("name", ["cornell12", "soup"])
def test_equals_the_frames_bit_for_bit(gpu_ctx, scene_of, name):
    scene = scene_of(name)
    assert np.all(_f16(scene.materials["ior_transmission_f16"], 16) <= 0)
    kinds = set(int(k) for k in scene.lights["light_type"])
    assert name != "soup" or (kinds == {0, 1, 2} and len(scene.spheres) > 0)
    gpu_ctx.upload_scene(scene)
    rays = gpu_ctx.camera_rays(W, H, scene.camera, mode=1)
    pts = gpu_ctx.surface(rays)
    position, prim, normal, _ = api.split_surface(pts)
    hit = prim != MISS
    cosang = np.zeros(len(rays))
    cosang[hit] = _geometric_facing(scene, rays[hit], prim[hit], position[hit])
    use = hit & (np.abs(cosang) >= 1e-4)
    left_out = 1.0 - use.sum() / hit.sum()
    print(f"{name}: {hit.sum()} hit pixels, {left_out:.4f} left out, {(cosang[use] > 0).sum()} back faces")
    assert hit.sum() > 0.3 * W * H and left_out <= 0.02
    if name == "soup":
        assert (cosang[use] > 0).any() and (prim[use] >= 0x80000000).any(), "back faces and spheres among the pixels"
    geo = pts.copy()
    geo[cosang > 0, 4:7] = -geo[cosang > 0, 4:7]  # rt_surface's face-forwarded normal turned back into the geometric one
    for shadows in (True, False):
        gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=1, max_bounces=0, no_shadows=not shadows)
        frame = gpu_ctx.read_rgb32f().reshape(-1, 3)
        got = gpu_ctx.direct_light(geo, bias=1e-3, ambient=True, shadows=shadows)
        radiance, mask = api.split_lighting(got)
        # (0 + x) * 1 / 1 of the frame's reduction: the bits of x, but for a zero's sign
        np.testing.assert_array_equal(_bits((F32(0) + radiance[use]) / F32(1)), _bits(frame[use]), err_msg=f"{name} shadows={shadows}")
        assert len(np.unique(mask[use])) > 1 or len(scene.lights) == 1
        if shadows:
            lit_all = api.split_lighting(gpu_ctx.direct_light(geo, ambient=True, shadows=False))[1]
            assert np.all(mask & ~lit_all == 0), "shadows only remove lights"
            assert name != "soup" or (mask[use] != lit_all[use]).any(), "... and some are removed"


# 2. the definition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell12", "soup"])
def test_equals_its_definition(gpu_ctx, scene_of, name):
    scene = scene_of(name)
    gpu_ctx.upload_scene(scene)
    pts = _points(gpu_ctx, scene)
    for bias, ambient in ((1e-3, False), (0.0, True), (1e-2, False)):
        got = gpu_ctx.direct_light(pts, bias=bias, ambient=ambient)
        st = gpu_ctx.stats()
        lit, clear, segments = _check_definition(gpu_ctx, scene, pts, got, bias=bias, max_excluded=0.02)
        assert st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["tri_tests"] == 0 and st["kernel_ms"] > 0
        assert st["rays"] == st["shadow_rays"]
        if clear.all():
            assert st["rays"] == segments
        else:  # every excluded pair may or may not have a segment
            assert segments <= st["rays"] <= segments + int((~clear).sum())
        assert 0 < lit.sum() <= segments
        assert name != "soup" or lit.sum() < segments, "some segments are occluded and some are not"
    none = gpu_ctx.direct_light(pts, shadows=False)
    assert gpu_ctx.stats()["rays"] == 0 and gpu_ctx.stats()["shadow_rays"] == 0
    _check_definition(gpu_ctx, scene, pts, none, shadows=False)


def test_segment_count_on_a_case_with_no_excluded_pair(gpu_ctx, scene_of):
    scene = scene_of("cornell12")
    gpu_ctx.upload_scene(scene)
    pts = _points(gpu_ctx, scene)
    lit, clear, segments = definition(gpu_ctx, scene, pts)
    pts = np.ascontiguousarray(pts[clear.all(1)])
    assert len(pts) > 1000
    got = gpu_ctx.direct_light(pts, counters=True)
    st = gpu_ctx.stats()
    lit, clear, segments = _check_definition(gpu_ctx, scene, pts, got, max_excluded=0.0)
    assert clear.all() and st["rays"] == st["shadow_rays"] == segments > 0 and st["node_visits"] > 0 and st["tri_tests"] > 0


# 3. the light grids -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell12", "soup1", "soup2", "soup3", "room", "fan"])
def test_grids_change_nothing_and_the_grid_path_runs(gpu_ctx, scene_of, name):
    scene = scene_of(name)
    if name != "cornell12":
        os.environ["RT_SHADOW_GRID_MEAN"] = "1e9"  # (long lists - clutter seen end-on, the fan's axis - must not make the build refuse the grids)
    try:
        gpu_ctx.upload_scene(scene)
        pts = _points(gpu_ctx, scene)
        before = gpu_ctx.direct_light(pts, counters=True)
        tree = gpu_ctx.stats()
        assert tree["grid_bytes"] == 0 and gpu_ctx.debug_shadow_grid()["lights_with_grid"] == 0, "the call builds no grids"
        gpu_ctx.prepare()
        print(name, [gpu_ctx.debug_shadow_grid(i) for i in range(len(scene.lights))])
        assert gpu_ctx.stats()["grid_bytes"] > 0
        with_grids = gpu_ctx.direct_light(pts, counters=True)
        st = gpu_ctx.stats()
        use = gpu_ctx.debug_shadow_grid()
        without = gpu_ctx.direct_light(pts, use_grids=False, counters=True)
        st_off = gpu_ctx.stats()
    finally:
        os.environ.pop("RT_SHADOW_GRID_MEAN", None)
    print(f"{name}: {len(pts)} points, {st['rays']} segments, answered by the lists {use['segments_answered']}, entries {use['entries_read']}, "
          f"node visits {st['node_visits']} with / {st_off['node_visits']} without")
    assert with_grids.tobytes() == before.tobytes() and without.tobytes() == before.tobytes()
    assert st["rays"] == st_off["rays"] == tree["rays"] > 0
    assert st_off["node_visits"] == tree["node_visits"] and st_off["tri_tests"] == tree["tri_tests"]
    assert st["node_visits"] < st_off["node_visits"] and 0 < use["segments_answered"] <= st["rays"]
    if name == "fan":
        assert use["segments_answered"] < st["rays"] and use["entries_read"] > 3.0 * use["segments_answered"]  # handed on, and walked on
    if name == "room":
        assert gpu_ctx.debug_shadow_grid(1)["near"] >= 1
    _check_definition(gpu_ctx, scene, pts, with_grids)


# 4. ineligible input ------------------------------------------------------------------------------------------------------------
def test_ineligible_input_falls_back_silently_and_equally(gpu_ctx, scene_of, monkeypatch):
    scene = scene_of("soup1")
    gpu_ctx.upload_scene(scene)
    monkeypatch.setenv("RT_SHADOW_GRID_MEAN", "1e9")  # (as above)
    gpu_ctx.prepare()
    assert gpu_ctx.stats()["grid_bytes"] > 0
    base = np.ascontiguousarray(_points(gpu_ctx, scene, 512)[::3])
    p = scene.vertices["position"].astype(np.float64)
    centre, extent = (p.min(0) + p.max(0)) / 2, float((p.max(0) - p.min(0)).max())
    outward = _normalize((base[:, 0:3] - centre.astype(F32)))

    def moved(dist):
        q = base.copy()
        q[:, 0:3] = centre.astype(F32) + outward * F32(dist)
        q[:, 4:7] = outward  # facing away from the scene: the directional lights behind it still reach it
        return q

    def scaled(s):
        q = base.copy()
        q[:, 4:7] *= F32(s)
        return q
    cases = [("normals x 2", scaled(2.0), 1e-3), ("normals x 0.5", scaled(0.5), 1e-3), ("10 x extent outside", moved(10 * extent), 1e-3),
             ("1e4 x extent outside", moved(1e4 * extent), 1e-3), ("at 1e30", moved(1e30), 1e-3), ("bias 0", base, 0.0), ("bias 1e-2", base, 1e-2),
             ("bias nextafter(1e-3)", base, float(np.nextafter(EPS, F32(1))))]
    for what, pts, bias in cases:
        pts = np.ascontiguousarray(pts)
        got = gpu_ctx.direct_light(pts, bias=bias, counters=True)
        st = gpu_ctx.stats()
        assert gpu_ctx.debug_shadow_grid()["segments_answered"] == 0, f"{what}: no segment may look at a list"
        off = gpu_ctx.direct_light(pts, bias=bias, use_grids=False, counters=True)
        st_off = gpu_ctx.stats()
        assert got.tobytes() == off.tobytes(), what
        assert (st["rays"], st["node_visits"], st["tri_tests"]) == (st_off["rays"], st_off["node_visits"], st_off["tri_tests"]), what
        _check_definition(gpu_ctx, scene, pts, got, bias=bias)
    got = gpu_ctx.direct_light(base, counters=True)  # the same points as they are: eligible
    assert gpu_ctx.debug_shadow_grid()["segments_answered"] > 0


# 5. edges -----------------------------------------------------------------------------------------------------------------------
def _expected_unlit(scene, mid, ambient):
    m = scene.materials[mid]
    total = np.zeros(3, F32)
    if ambient:
        total = total + m["albedo"].astype(F32) * F32(0.1)
    return total + m["emission"].astype(F32)


def test_edges(gpu_ctx, scene_of):
    scene = scene_of("cornell12")
    gpu_ctx.upload_scene(scene)
    pts = _points(gpu_ctx, scene)
    whole = gpu_ctx.direct_light(pts[:65])
    for n in (0, 1, 63, 64, 65):
        got = gpu_ctx.direct_light(np.ascontiguousarray(pts[:n]))
        assert got.shape == (n, 4) and got.tobytes() == whole[:n].tobytes()
    odd = np.tile(pts[:1], (6, 1))
    odd[0, 1] = np.nan                                    # a NaN position
    odd[1, 4:7] = 0                                       # a zero normal
    odd[2, 5] = np.inf                                    # an inf normal
    odd[3] = gpu_ctx.surface(api.make_rays(np.array([[0, 0, 50]], F32), np.array([[0, 0, 1]], F32)))[0]  # a miss record of rt_surface
    odd[4, 7] = np.array([len(scene.materials)], U32).view(F32)[0]  # an invalid material id
    odd[5, 0:3] = scene.lights["position"][0]             # exactly at the point light
    odd[5, 4:7], odd[5, 7] = (0, 1, 0), np.array([1], U32).view(F32)[0]
    assert _bits(odd[3, 3]) == MISS
    for ambient in (False, True):
        got = gpu_ctx.direct_light(np.ascontiguousarray(np.concatenate([odd, pts[:70]])), ambient=ambient)
        assert gpu_ctx.direct_light(np.ascontiguousarray(pts[:70]), ambient=ambient).tobytes() == got[6:].tobytes()
        assert not got[:4].view(U32).any(), "records that are no points: zero radiance, zero mask"
        assert got[4].tobytes() == np.array([1, 0, 1, 0], F32).tobytes(), "the frames' magenta, mask 0"
        np.testing.assert_array_equal(got[5, 0:3], _expected_unlit(scene, 1, ambient))
        assert _bits(got[5, 3]) == 0
    # no lights: emission (+ ambient), mask 0, nothing traced
    dark = dataclasses.replace(scene, lights=np.zeros(0, T.LIGHT))
    gpu_ctx.upload_scene(dark)
    for ambient in (False, True):
        got = gpu_ctx.direct_light(pts, ambient=ambient)
        assert gpu_ctx.stats()["rays"] == 0
        radiance, mask = api.split_lighting(got)
        mid = _bits(pts[:, 7])
        for k in np.unique(mid):
            np.testing.assert_array_equal(radiance[mid == k], np.broadcast_to(_expected_unlit(scene, int(k), ambient), (int((mid == k).sum()), 3)))
        assert not mask.any()
    # an empty scene: one material, no lights, no triangles
    gpu_ctx.upload_scene(scenes.empty_scene())
    got = gpu_ctx.direct_light(pts, ambient=True)
    radiance, mask = api.split_lighting(got)
    mid = _bits(pts[:, 7])
    np.testing.assert_array_equal(radiance[mid == 0], np.broadcast_to(_expected_unlit(scenes.empty_scene(), 0, True), (int((mid == 0).sum()), 3)))
    assert np.all(radiance[mid != 0] == np.array([1, 0, 1], F32)) and not mask.any()


# 6. plumbing --------------------------------------------------------------------------------------------------------------------
def test_memory_kinds_devices_tree_and_updates(gpu_ctx, scene_of, monkeypatch):
    monkeypatch.setenv("RT_SHADOW_GRID_MEAN", "1e9")  # (as above; only rt_prepare reads it)
    scene = scene_of("soup")
    gpu_ctx.upload_scene(scene)
    pts = _points(gpu_ctx, scene)
    want = gpu_ctx.direct_light(pts, ambient=True)
    rays_one = gpu_ctx.stats()["rays"]
    own = np.full((len(pts), 4), 7, F32)
    assert gpu_ctx.direct_light(pts, ambient=True, out=own) is own and own.tobytes() == want.tobytes()
    if torch is not None:
        dev = torch.from_numpy(pts).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
        got = gpu_ctx.direct_light(dev, ambient=True)
        assert got.device == dev.device and got.dtype == torch.float32 and tuple(got.shape) == (len(pts), 4)
        assert got.cpu().numpy().tobytes() == want.tobytes()
        assert gpu_ctx.direct_light(torch.from_numpy(pts.copy()), ambient=True).numpy().tobytes() == want.tobytes()
        np.testing.assert_array_equal(api.split_lighting(got)[1].cpu().numpy(), api.split_lighting(want)[1].astype(np.int64))
    with api.Context((0, 0)) as two:  # each device gets a contiguous range of the points
        two.upload_scene(scene)
        assert two.direct_light(pts, ambient=True).tobytes() == want.tobytes() and two.stats()["rays"] == rays_one
        two.prepare()  # ... and walks its own grids
        assert two.direct_light(pts, ambient=True, counters=True).tobytes() == want.tobytes() and two.stats()["rays"] == rays_one
        assert two.debug_shadow_grid()["segments_answered"] > 0
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.stats()["tree_build"] == 0
    assert gpu_ctx.direct_light(pts, ambient=True).tobytes() == want.tobytes()
    # after a vertex update the grids are gone and the call walks the refitted tree: the result of a fresh upload
    gpu_ctx.prepare()
    assert gpu_ctx.stats()["grid_bytes"] > 0
    pos = scene.vertices["position"].astype(F32)
    moved_pos = np.ascontiguousarray(pos + F32(0.2) * np.sin(pos[:, ::-1] * F32(3.0)), dtype=F32)
    v = scene.vertices.copy()
    v["position"] = moved_pos
    assert gpu_ctx.update_geometry(vertices=moved_pos)["flags"] & (api.STAT_REFIT | api.STAT_REBUILT)
    after = gpu_ctx.direct_light(pts, ambient=True, counters=True)
    assert gpu_ctx.stats()["grid_bytes"] == 0 and gpu_ctx.debug_shadow_grid()["segments_answered"] == 0
    with api.Context() as fresh:
        fresh.upload_scene(dataclasses.replace(scene, vertices=v))
        assert fresh.direct_light(pts, ambient=True).tobytes() == after.tobytes()
    assert after.tobytes() != want.tobytes()


def test_host_batch_across_a_chunk_boundary(gpu_ctx, scene_of):
    scene = scene_of("cornell12")
    gpu_ctx.upload_scene(scene)
    some = _points(gpu_ctx, scene, 0)
    rows, n = len(some), api.QUERY_CHUNK + 5
    once = gpu_ctx.direct_light(some)
    per_point = np.array([bin(int(m)).count("1") for m in api.split_lighting(gpu_ctx.direct_light(some, shadows=False))[1]])  # its segments
    pts = np.ascontiguousarray(np.resize(some, (n, 8)))
    got = gpu_ctx.direct_light(pts)  # two chunks: 4 Mi points and 5
    assert gpu_ctx.stats()["rays"] == int(np.resize(per_point, n).sum()) > 0
    full = rows * (n // rows)
    assert got[:full].reshape(n // rows, rows, 4).tobytes() == np.broadcast_to(once, (n // rows, rows, 4)).tobytes()
    assert got[full:].tobytes() == once[: n - full].tobytes()
    if torch is not None:
        dev = gpu_ctx.direct_light(torch.from_numpy(pts).to("cuda:0"))  # one device-resident call
        assert dev.cpu().numpy().tobytes() == got.tobytes()


def test_the_frame_and_a_running_accumulation_are_left_alone(gpu_ctx, scene_of):
    scene = scene_of("soup")
    gpu_ctx.upload_scene(scene)
    pts = _points(gpu_ctx, scene)
    gpu_ctx.render(W, H, scene.camera, mode=1)
    rgb, comb, hits = gpu_ctx.read_rgb32f(), gpu_ctx.read_rgba8_combined(), gpu_ctx.read_hits()
    gpu_ctx.direct_light(pts)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.read_rgba8_combined().tobytes() == comb.tobytes()
    again = gpu_ctx.read_hits()
    assert again[0].tobytes() == hits[0].tobytes() and again[1].tobytes() == hits[1].tobytes()
    gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    gpu_ctx.direct_light(pts, ambient=True, counters=True)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4


# 7. the library's own checks ------------------------------------------------------------------------------------------------------
def test_the_librarys_own_checks(gpu_ctx, scene_of):
    scene = scene_of("cornell12")
    pts, out = np.zeros((64, 8), F32), np.full((64, 4), 7, F32)
    pts[:, 5], pts[:, 1] = 1.0, -0.5
    dp = np.zeros((), T.DIRECT_LIGHT_PARAMS)
    dp["bias"] = 1e-3
    lib, h = gpu_ctx.lib, gpu_ctx._h
    call = lambda p, n, a, o: lib.rt_direct_light(h, C.c_void_p(p), C.c_size_t(n), C.c_void_p(a), C.c_void_p(o))
    assert call(pts.ctypes.data, 64, dp.ctypes.data, out.ctypes.data) == -4  # before any upload
    assert call(0, 0, 0, 0) == 0  # n == 0 (even then)
    gpu_ctx.upload_scene(scene)
    assert call(0, 0, 0, 0) == 0
    assert call(0, 64, dp.ctypes.data, out.ctypes.data) == -1 and "points" in lib.rt_last_error(h).decode()
    assert call(pts.ctypes.data, 64, 0, out.ctypes.data) == -1 and "params" in lib.rt_last_error(h).decode()
    assert call(pts.ctypes.data, 64, dp.ctypes.data, 0) == -1 and "out" in lib.rt_last_error(h).decode()
    for field, bad in (("bias", -1e-3), ("bias", np.inf), ("bias", np.nan), ("flags", 2), ("flags", 32), ("flags", 1 << 31)):
        p = dp.copy()
        p[field] = bad
        assert call(pts.ctypes.data, 64, p.ctypes.data, out.ctypes.data) == -1, (field, bad)
        assert field in lib.rt_last_error(h).decode() or field == "flags"
    assert np.all(out == 7), "a rejected call changes nothing"
    many = dataclasses.replace(scene, lights=np.repeat(scene.lights, 33))
    gpu_ctx.upload_scene(many)
    assert call(pts.ctypes.data, 64, dp.ctypes.data, out.ctypes.data) == -1 and "33 lights" in lib.rt_last_error(h).decode()
    assert np.all(out == 7)
    gpu_ctx.upload_scene(dataclasses.replace(scene, lights=np.repeat(scene.lights, 32)))
    assert call(pts.ctypes.data, 64, dp.ctypes.data, out.ctypes.data) == 0  # 32 lights are fine, and the context is usable
    assert np.all(_bits(out[:, 3]) == 0xFFFFFFFF), "a point under the light, facing it, in the open: all 32 copies of the light reach it"
    if torch is not None:
        dev = torch.from_numpy(pts).to("cuda:0")
        skew = torch.zeros(64 * 8 + 4, device="cuda:0")[1:1 + 64 * 8].view(-1, 8)
        with pytest.raises(api.RtError) as e:
            gpu_ctx.direct_light(skew)
        assert e.value.code == -1 and "aligned" in str(e.value)
        assert call(dev.data_ptr(), 64, dp.ctypes.data, out.ctypes.data) == -1  # device points, host out
        assert gpu_ctx.direct_light(dev).cpu().numpy().tobytes() == out.tobytes()
