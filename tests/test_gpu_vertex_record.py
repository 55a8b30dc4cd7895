"""The path vertex written by the kernels that find the closest hit (k_wf_trace<closest>, k_wf_trace_camera), the path ends that
k_wf_finish takes over, and the shadow stage that works out by itself which lights need a segment (k_wf_shadow_grid).

Nothing here is a new statement of the estimator: every frame is compared, bit for bit and with its segment counts, against the CPU
statement (oracle.render_extended without a tree), against the state-machine megakernel, or against the same frame rendered another
way (no light grids, no beams, one lane, batches of one sample, two ranks, accumulating and adaptive calls).  The shapes are the
smallest at which each piece can go wrong: extension queues of 1, 63, 64, 65, 255, 256 and 257 paths (a wave that never refills, one
that refills exactly once, the flush at the kernel's exit), scenes whose paths all end on the sky or on an invalid material, sphere
normals, and materials and lights for which `needs_shadow_segment` is decided by a zero, an underflow or the metallic branch.

257 is prime, so that queue comes from a 257 x 1 frame: wider than the other frames here, still 257 pixels on one device."""
import dataclasses

import numpy as np
import pytest

from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

pytestmark = pytest.mark.gpu

SM = {"kernel_sm": True}
# first extension queue of w * h * spp paths (every pixel of these frames has a path)
QUEUES = {1: (1, 1, 1), 63: (9, 7, 1), 64: (4, 4, 4), 65: (13, 5, 1), 255: (17, 5, 3), 256: (8, 8, 4), 257: (257, 1, 1)}
_refs = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _frame(ctx, scene, w, h, spp, bounces, **kw):
    st = ctx.render(w, h, scene.camera, mode=2, spp=spp, max_bounces=bounces, **kw)
    return ctx.read_rgb32f().copy(), (st["primary_rays"], st["continuation_rays"], st["shadow_rays"])


def _cpu(oracle_mod, key, scene, w, h, spp, bounces, frame_seed=0, flags=0):
    """The CPU statement of a frame, computed once per (scene key, shape)."""
    k = (key, w, h, spp, bounces, frame_seed, flags)
    if k not in _refs:
        r = oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), w, h, spp, bounces, frame_seed=frame_seed, flags=flags)
        s = r["segments"]
        _refs[k] = (r["rgb"], (s["camera"], s["continuation"], s["shadow"]))
    return _refs[k]


def _equal(got, want, what):
    assert got[1] == want[1], f"{what}: segments {got[1]} != {want[1]}"
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=what)


def _on_grids(ctx, scene, w, h, spp, bounces, **kw):
    """The frame took the grid path: every light has a grid and the lists answered segments."""
    assert ctx.debug_shadow_grid()["lights_with_grid"] == len(scene.lights), ctx.debug_shadow_grid()
    ctx.render(w, h, scene.camera, mode=2, spp=spp, max_bounces=bounces, counters=True, **kw)
    assert ctx.debug_shadow_grid()["segments_answered"] > 0


# 1 + 6 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", list(QUEUES))
def test_queue_lengths_around_a_wave(gpu_ctx, oracle_mod, paths):
    """The deferred epilogue and the flush at exit: depth 0 through the tree walk (no_beams) and through the camera kernel."""
    scene = scenes.cornell12()
    w, h, spp = QUEUES[paths]
    gpu_ctx.upload_scene(scene)
    for bounces in (1, 3):
        want = _cpu(oracle_mod, "cornell12", scene, w, h, spp, bounces)
        for beams in ({"no_beams": True}, {}):
            _equal(_frame(gpu_ctx, scene, w, h, spp, bounces, **beams), want, f"{paths} paths, {bounces} bounces, {beams}: pipeline against the CPU statement")
            _equal(_frame(gpu_ctx, scene, w, h, spp, bounces, **beams, **SM), want, f"{paths} paths, {bounces} bounces, {beams}: megakernel against the CPU statement")
    _on_grids(gpu_ctx, scene, w, h, spp, 3)


def test_nine_bounces(gpu_ctx, oracle_mod):
    scene = scenes.cornell12()
    w, h, spp = QUEUES[255]
    gpu_ctx.upload_scene(scene)
    want = _cpu(oracle_mod, "cornell12", scene, w, h, spp, 9)
    _equal(_frame(gpu_ctx, scene, w, h, spp, 9), want, "pipeline")
    _equal(_frame(gpu_ctx, scene, w, h, spp, 9, **SM), want, "megakernel")
    _on_grids(gpu_ctx, scene, w, h, spp, 9)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def _bad_material_soup():
    s = scenes.random_soup(200, seed=4, size=0.9, n_spheres=2, n_lights=2)
    tris, spheres = s.triangles.copy(), s.spheres.copy()
    tris["material_id"][::3] = 77  # past the five materials: magenta, the path ends
    spheres["material_id"][0] = 99
    return dataclasses.replace(s, triangles=tris, spheres=spheres, name="bad_material_soup")


ENDS = {"empty": scenes.empty_scene, "single_triangle": scenes.single_triangle, "bad_material_soup": _bad_material_soup}


@pytest.mark.parametrize("bounces", [0, 1, 4])
@pytest.mark.parametrize("name", list(ENDS))
def test_paths_that_end_at_the_hit(gpu_ctx, oracle_mod, name, bounces):
    """Sky misses and invalid materials: k_wf_finish ends the path from the marker the closest-hit kernel left."""
    scene = ENDS[name]()
    w, h, spp = 40, 24, 3
    want = _cpu(oracle_mod, name, scene, w, h, spp, bounces, frame_seed=9)
    gpu_ctx.upload_scene(scene)
    pipeline = {"kernel_pipeline": True} if bounces == 0 else {}  # (a frame without bounces would take the one-pass kernel)
    for beams in ({"no_beams": True}, {}):
        _equal(_frame(gpu_ctx, scene, w, h, spp, bounces, frame_seed=9, **beams, **pipeline), want, f"{name}, {beams}")
    _equal(_frame(gpu_ctx, scene, w, h, spp, bounces, frame_seed=9, **SM), want, f"{name}, megakernel")
    if name == "bad_material_soup":
        assert (want[0] == np.array([1.0, 0.0, 1.0], np.float32)).all(-1).any()  # pixels whose every sample ends on an invalid material


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_sphere_normals(gpu_ctx, oracle_mod):
    scene = scenes.random_soup(400, seed=21, size=0.7, n_spheres=3, n_lights=3)  # glass, metal, emissive and diffuse; spheres in view
    want = _cpu(oracle_mod, "soup400", scene, 72, 48, 6, 5, frame_seed=77)
    gpu_ctx.upload_scene(scene)
    for beams in ({"no_beams": True}, {}):
        _equal(_frame(gpu_ctx, scene, 72, 48, 6, 5, frame_seed=77, **beams), want, f"{beams}")


# 4 ------------------------------------------------------------------------------------------------------------------------------
def _mask_scene(n_lights):
    """The twelve triangles of cornell12 with materials and lights that decide `needs_shadow_segment` every way it can be decided."""
    s = scenes.cornell12()
    materials = np.array([
        H.material_diffuse((0.73, 0.73, 0.73)),
        H.material_diffuse((0.0, 0.0, 0.0)),                                   # black: no light contributes, no segment
        H.material_diffuse((1e-38, 0.7, 0.7)),                                 # brdf x colour underflows in one channel
        H.material_emissive((1.0, 1.0, 1.0), (1.0, 1.0, 1.0)),
        H.material_metallic((0.9, 0.6, 0.3), 0.3),                             # the other branch of evaluate_brdf
        H.material_diffuse((1e-38, 1e-38, 1e-38)),                             # ... in all of them, for the weaker lights
    ], dtype=T.MATERIAL)
    tris = s.triangles.copy()
    tris["material_id"] = [0, 0, 4, 4, 2, 2, 1, 1, 5, 5, 3, 3]  # floor, ceiling, back, left, right, the emissive quad
    lights = [H.light_point((0.0, 0.9, 0.0), (1.0, 1.0, 1.0), 1.0)]
    if n_lights > 1:
        lights += [
            H.light_directional((0.0, 0.0, 1.0), (1.0, 1.0, 1.0), 0.8),       # shines out of the box: behind or edge-on to every surface
            H.light_point((0.0, 0.0, -3.0), (1.0, 0.9, 0.8), 4.0),             # behind the back wall, which hides it from the others
            H.light_spot((0.3, 0.9, 0.2), (0.0, -1.0, -0.2), (1.0, 1.0, 1.0), 2.0, 20.0, 0.3, 0.6),
            H.light_directional((0.3, -1.0, -0.2), (0.6, 0.7, 1.0), 0.8),
        ]
    rng = np.random.default_rng(7)
    while len(lights) < n_lights:
        u, kind = rng.random(6), len(lights) % 3
        if kind == 0:
            lights.append(H.light_point(tuple(u[:3] * 1.6 - 0.8), (1.0, 0.9, 0.8), 0.05 + 0.5 * u[3]))
        elif kind == 1:
            lights.append(H.light_directional((u[0] - 0.5, -1.0, u[2] - 0.5), (0.6, 0.7, 1.0), 0.01 + 0.3 * u[3]))
        else:
            lights.append(H.light_spot((u[0] * 1.2 - 0.6, 0.9, u[2] * 1.2 - 0.6), (u[3] - 0.5, -1.0, u[4] - 0.5), (1.0, 1.0, 1.0), 0.5 + u[5], 20.0, 0.3, 0.6))
    return dataclasses.replace(s, materials=materials, triangles=tris, lights=np.array(lights[:n_lights], dtype=T.LIGHT), name=f"mask{n_lights}")


MASK_FRAME = (48, 32, 4, 3)


@pytest.mark.parametrize("n_lights", [1, 5, 32])
def test_lights_that_need_a_segment(gpu_ctx, oracle_mod, n_lights):
    """The grid kernel's own mask: same bits and the same number of shadow segments as the shadow queue of a frame without grids, and
    as the CPU statement - with lights that contribute nothing, a black albedo, albedos that underflow, and a metallic material."""
    scene = _mask_scene(n_lights)
    want = _cpu(oracle_mod, scene.name, scene, *MASK_FRAME, frame_seed=3)
    gpu_ctx.upload_scene(scene)
    grids = _frame(gpu_ctx, scene, *MASK_FRAME, frame_seed=3)
    _equal(grids, want, "light grids against the CPU statement")
    _equal(_frame(gpu_ctx, scene, *MASK_FRAME, frame_seed=3, no_shadow_grid=True), grids, "no light grids")
    _on_grids(gpu_ctx, scene, *MASK_FRAME, frame_seed=3)
    assert want[1][2] < n_lights * (want[1][0] + want[1][1])  # some vertices need no segment to some light


def test_no_shadows(gpu_ctx, oracle_mod):
    scene = _mask_scene(5)
    want = _cpu(oracle_mod, scene.name, scene, *MASK_FRAME, frame_seed=3, flags=oracle_mod.EXT_NO_SHADOWS)
    assert want[1][2] == 0
    gpu_ctx.upload_scene(scene)
    _equal(_frame(gpu_ctx, scene, *MASK_FRAME, frame_seed=3, no_shadows=True), want, "no shadows")
    _equal(_frame(gpu_ctx, scene, *MASK_FRAME, frame_seed=3, no_shadows=True, no_shadow_grid=True), want, "no shadows, no light grids")


# 5 ------------------------------------------------------------------------------------------------------------------------------
INVARIANT = {"queue255": (scenes.cornell12, QUEUES[255] + (3,), 0, 8), "mask5": (lambda: _mask_scene(5), MASK_FRAME, 3, 16)}


@pytest.mark.parametrize("case", list(INVARIANT))
def test_scheduling_does_not_change_the_frame(rt_api, monkeypatch, case):
    make, (w, h, spp, bounces), seed, tile = INVARIANT[case]
    scene = make()
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        plain = _frame(ctx, scene, w, h, spp, bounces, frame_seed=seed)
        # two ranks, assembled: tile t belongs to rank t % 2
        tx, ty = (w + tile - 1) // tile, (h + tile - 1) // tile
        assert tx * ty >= 2
        acc, seg = np.zeros_like(plain[0]), np.zeros(3, np.int64)
        for rank in range(2):
            part, s = _frame(ctx, scene, w, h, spp, bounces, frame_seed=seed, tile_size=tile, tile_rank=rank, tile_world=2)
            seg += s
            for t in range(rank, tx * ty, 2):
                ox, oy = (t % tx) * tile, (t // tx) * tile
                acc[oy:oy + tile, ox:ox + tile] = part[oy:oy + tile, ox:ox + tile]
        _equal((acc, tuple(int(v) for v in seg)), plain, "two ranks")
        # an accumulating second call, and the adaptive calls with a threshold nothing meets
        first = spp // 2
        ctx.render(w, h, scene.camera, mode=2, spp=first, max_bounces=bounces, frame_seed=seed, accumulate=True, restart=True)
        ctx.render(w, h, scene.camera, mode=2, spp=spp - first, max_bounces=bounces, frame_seed=seed, accumulate=True)
        np.testing.assert_array_equal(_bits(ctx.read_rgb32f()), _bits(plain[0]), err_msg="accumulating calls")
        ctx.render_adaptive(w, h, scene.camera, first, 0.0, min_samples=spp, max_bounces=bounces, frame_seed=seed, restart=True)
        ctx.render_adaptive(w, h, scene.camera, spp - first, 0.0, min_samples=spp, max_bounces=bounces, frame_seed=seed)
        np.testing.assert_array_equal(_bits(ctx.read_rgb32f()), _bits(plain[0]), err_msg="adaptive calls")
    for var in ("RT_WF_LANES", "RT_WF_BATCH"):
        with monkeypatch.context() as m:
            m.setenv(var, "1")
            with rt_api.Context() as ctx:
                ctx.upload_scene(scene)
                _equal(_frame(ctx, scene, w, h, spp, bounces, frame_seed=seed), plain, f"{var}=1")
