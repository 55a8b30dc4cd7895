"""Progressive accumulation (RT_FLAG_ACCUMULATE) on the GPU: an accumulation of N >= 2 samples is bit for bit one closed frame of N spp
(and the CPU statement's), however the samples were split over calls, whichever kernel rendered each call, across batches, lanes,
light grids, tile shares and devices; the running image restarts exactly when rt_hip.h says it does, and errors leave it alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = [[1, 2, 5], [3, 3, 2], [1] * 8, [8]]


def _assert_equal(a, b, msg=""):
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=msg)


def _images(ctx):
    return ctx.read_rgb32f(), ctx.read_rgba8_combined()


def _assert_same_images(got, want, msg=""):
    _assert_equal(got[0], want[0], msg + " (rgb32f)")
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg + " (rgba8 combined)")


def _frame(rt_api, scene, w, h, spp, bounces, **kw):
    """One closed frame in a fresh context: its images and stats."""
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        st = ctx.render(w, h, kw.pop("camera", scene.camera), mode=2, spp=spp, max_bounces=bounces, **kw)
        return _images(ctx), st


def _accumulate(ctx, scene, w, h, split, bounces, kws=None, **kw):
    """Accumulating calls of split[i] spp (call i with kws[i] on top of kw); returns the per-call stats."""
    stats, total = [], 0
    for i, n in enumerate(split):
        extra = dict(kw, **(kws[i] if kws else {}))
        stats.append(ctx.render(w, h, extra.pop("camera", scene.camera), mode=2, spp=n, max_bounces=bounces, accumulate=True, **extra))
        total += n
        assert ctx.accumulated_samples() == total
    return stats


def _owned(w, h, tile, world, rank):
    """Pixels of the tiles i with i % world == rank (rt_render_params.tile_rank / tile_world)."""
    tx = (w + tile - 1) // tile
    ys, xs = np.mgrid[0:h, 0:w]
    return ((ys // tile) * tx + xs // tile) % world == rank


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,name,bounces,kw", [
    ("pipeline", "cornell12", 3, {}), ("state_machine", "cornell12", 3, {"kernel_sm": True}), ("nested", "cornell12", 3, {"kernel_v1": True}),
    ("one_pass", "cornell12", 0, {}), ("pipeline_default_scene", "default", 4, {})])
def test_splits_equal_one_frame_and_the_oracle(rt_api, oracle_mod, path, name, bounces, kw):
    scene = scenes.SCENES[name]()
    w, h = 64, 48
    want, st8 = _frame(rt_api, scene, w, h, 8, bounces, **kw)
    ref = oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), w, h, 8, bounces)
    _assert_equal(want[0], ref["rgb"], "closed frame against the oracle")
    seg = ref["segments"]
    if path == "one_pass":
        assert st8["flags"] & rt_api.STAT_SINGLE_PASS
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        for split in SPLITS:
            first = ctx.render(w, h, scene.camera, mode=2, spp=split[0], max_bounces=bounces, accumulate=True, restart=True, **kw)
            stats = [first] + _accumulate_rest(ctx, scene, w, h, split, bounces, **kw)
            assert ctx.accumulated_samples() == 8
            _assert_same_images(_images(ctx), want, f"{path} {split}")
            for key, field in (("camera", "primary_rays"), ("continuation", "continuation_rays"), ("shadow", "shadow_rays")):
                assert sum(s[field] for s in stats) == seg[key], (split, key)
            assert sum(s["pixels"] for s in stats) == w * h * len(split)
            if path == "one_pass":
                assert all(s["flags"] & rt_api.STAT_SINGLE_PASS for s in stats)


def _accumulate_rest(ctx, scene, w, h, split, bounces, **kw):
    """The calls after the first of `split` (the first was made with restart=True)."""
    stats, total = [], split[0]
    for n in split[1:]:
        stats.append(ctx.render(w, h, scene.camera, mode=2, spp=n, max_bounces=bounces, accumulate=True, **kw))
        total += n
        assert ctx.accumulated_samples() == total
    return stats


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_mixed_kernel_paths_in_one_accumulation(rt_api):
    scene = scenes.random_soup(400, seed=21, size=0.7, n_spheres=3, n_lights=3)  # metal, glass, emissive, diffuse
    w, h, bounces = 72, 48, 5
    want, _ = _frame(rt_api, scene, w, h, 8, bounces, frame_seed=77)
    kws = [{}, {"kernel_sm": True}, {"kernel_v1": True}, {"no_beams": True}, {"no_shadow_grid": True}, {"kernel_pipeline": True, "counters": True}]
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        _accumulate(ctx, scene, w, h, [1, 2, 1, 2, 1, 1], bounces, kws, frame_seed=77)
        _assert_same_images(_images(ctx), want)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["1", None])  # None: the library's own batch
def test_accumulation_across_batches_lanes_and_grids(rt_api, monkeypatch, batch):
    """The second call's spp re-sizes the pipeline's batch (its WfBuffers may be reallocated); the running sum lives outside them."""
    scene = scenes.sponza_like()
    w, h, bounces = 480, 270, 3
    if batch:
        monkeypatch.setenv("RT_WF_BATCH", batch)
    else:
        monkeypatch.delenv("RT_WF_BATCH", raising=False)
    want, _ = _frame(rt_api, scene, w, h, 7, bounces)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        ctx.prepare(rt_api.PREPARE_SHADOW_GRIDS)
        assert ctx.stats()["grid_bytes"] > 0
        _accumulate(ctx, scene, w, h, [3, 4], bounces)
        got = _images(ctx)
    assert np.isfinite(got[0]).all()
    _assert_same_images(got, want)


# 4 ------------------------------------------------------------------------------------------------------------------------------
W, H, B = 64, 48, 3


def _check_restarted(rt_api, ctx, scene, spp=3, **kw):
    """An accumulating call of `spp` after an event that ends the running image: the count is spp and the image is a fresh accumulation."""
    cam = kw.pop("camera", scene.camera)
    w, h = kw.pop("w", W), kw.pop("h", H)
    ctx.render(w, h, cam, mode=2, spp=spp, max_bounces=kw.pop("bounces", B), accumulate=True, **kw)
    assert ctx.accumulated_samples() == spp
    return _images(ctx)


@pytest.mark.parametrize("change", ["camera", "size", "max_bounces", "frame_seed", "tile_size", "tile_share", "no_shadows", "restart"])
def test_key_change_restarts(rt_api, change):
    scene = scenes.default_scene()
    cam = scene.camera.copy()
    cam["fov"] = cam["fov"] * np.float32(1.0001)
    kw = {"camera": {"camera": cam}, "size": {"w": 48, "h": 40}, "max_bounces": {"bounces": 2}, "frame_seed": {"frame_seed": 5},
          "tile_size": {"tile_size": 32}, "tile_share": {"tile_world": 2, "tile_rank": 1, "tile_size": 16}, "no_shadows": {"no_shadows": True},
          "restart": {"restart": True}}[change]
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        ctx.render(W, H, scene.camera, mode=2, spp=2, max_bounces=B, accumulate=True)
        assert ctx.accumulated_samples() == 2
        got = _check_restarted(rt_api, ctx, scene, **dict(kw))
    fk = {k: v for k, v in kw.items() if k not in ("w", "h", "bounces", "restart")}
    want, _ = _frame(rt_api, scene, kw.get("w", W), kw.get("h", H), 3, kw.get("bounces", B), **fk)
    if change == "tile_share":
        m = _owned(W, H, 16, 2, 1)
        _assert_equal(got[0][m], want[0][m])
        np.testing.assert_array_equal(got[1][m], want[1][m])
    else:
        _assert_same_images(got, want, change)


@pytest.mark.parametrize("event", ["upload_scene", "update_vertices", "update_spheres", "closed_render", "dispatch_tile"])
def test_scene_and_frame_events_restart(rt_api, oracle_mod, event):
    scene = scenes.default_scene()
    want, _ = _frame(rt_api, scene, W, H, 3, B)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        ctx.render(W, H, scene.camera, mode=2, spp=2, max_bounces=B, accumulate=True)
        if event == "upload_scene":
            ctx.upload_scene(scene)
        elif event == "update_vertices":
            ctx.update_geometry(np.ascontiguousarray(scene.vertices["position"], dtype=np.float32))
        elif event == "update_spheres":
            ctx.update_geometry(spheres=scene.spheres.copy())
        elif event == "closed_render":
            ctx.render(W, H, scene.camera, mode=2, spp=2, max_bounces=B)
        else:
            ctx.dispatch_tile(oracle_mod.PackedScene(scene, use_bvh=False).push_constants(W, H, channel=0, tile_offset=(0, 0)))
        assert ctx.accumulated_samples() == 0
        got = _check_restarted(rt_api, ctx, scene)
    _assert_same_images(got, want, event)


def test_what_does_not_restart(rt_api):
    """A/B flags, rt_prepare (both kinds: the quality tree replaces the device-built one), textures, ray queries, camera rays, statistics
    and reads between the calls: the bits continue."""
    scene = scenes.random_soup(2000, seed=5, size=0.5, n_spheres=2, n_lights=2)
    w, h, bounces = 64, 48, 3
    want, _ = _frame(rt_api, scene, w, h, 8, bounces)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        assert ctx.stats()["tree_build"] == 2
        go = lambda n, **kw: ctx.render(w, h, scene.camera, mode=2, spp=n, max_bounces=bounces, accumulate=True, **kw)
        go(1)
        ctx.prepare(rt_api.PREPARE_SHADOW_GRIDS | rt_api.PREPARE_QUALITY_TREE)
        assert ctx.stats()["tree_build"] == 0
        go(2, stage_times=True)
        rays = ctx.camera_rays(w, h, scene.camera, mode=1)
        ctx.intersect(rays)
        ctx.occluded(rays)
        ctx.upload_textures(np.zeros(0, T.TEXTURE_INFO), np.zeros(0, np.uint8))
        _images(ctx)
        ctx.read_rgba8_channels()
        ctx.stats()
        assert ctx.accumulated_samples() == 3
        go(1, counters=True, no_beams=True)
        go(2, kernel_sm=True, no_shadow_grid=True)
        go(2, kernel_v1=True)
        assert ctx.accumulated_samples() == 8
        _assert_same_images(_images(ctx), want)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_running_image(rt_api):
    scene = scenes.default_scene()
    want, _ = _frame(rt_api, scene, W, H, 5, B)
    lib = rt_api.load()
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        ctx.render(W, H, scene.camera, mode=2, spp=2, max_bounces=B, accumulate=True)
        for mode in (0, 1):
            with pytest.raises(rt_api.RtError, match="BAD_ARG"):
                ctx.render(W, H, scene.camera, mode=mode, accumulate=True)
            assert ctx.accumulated_samples() == 2
        for bad in ({"spp": 0}, {"spp": 65537}, {"max_bounces": 256}, {"tile_size": 5000}):
            args = {"spp": 1, "max_bounces": B}
            args.update(bad)
            with pytest.raises(rt_api.RtError, match="BAD_ARG"):
                ctx.render(W, H, scene.camera, mode=2, accumulate=True, **args)
            assert ctx.accumulated_samples() == 2, bad
        p = np.zeros((), T.RENDER_PARAMS)  # the restart bit alone
        p["camera"], p["width"], p["height"], p["spp"], p["max_bounces"], p["mode"] = scene.camera, W, H, 1, B, 2
        p["tile_world"], p["flags"] = 1, rt_api.FLAG_ACCUMULATE_RESTART
        assert lib.rt_render(ctx._h, C.c_void_p(p.ctypes.data)) == -1
        assert ctx.accumulated_samples() == 2
        ctx.render(W, H, scene.camera, mode=2, spp=3, max_bounces=B, accumulate=True)
        assert ctx.accumulated_samples() == 5
        _assert_same_images(_images(ctx), want)


def test_sample_limit(rt_api):
    """2^24 samples, where the float count stops being exact: 256 calls of 65536 reach it, the next one is refused."""
    scene = scenes.empty_scene()
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        for i in range(256):
            ctx.render(8, 8, scene.camera, mode=2, spp=65536, max_bounces=0, accumulate=True)
        assert ctx.accumulated_samples() == rt_api.ACCUMULATE_MAX_SAMPLES
        with pytest.raises(rt_api.RtError, match="BAD_ARG"):
            ctx.render(8, 8, scene.camera, mode=2, spp=1, max_bounces=0, accumulate=True)
        assert ctx.accumulated_samples() == rt_api.ACCUMULATE_MAX_SAMPLES
        assert np.isfinite(ctx.read_rgb32f()).all()
        ctx.render(8, 8, scene.camera, mode=2, spp=1, max_bounces=0, accumulate=True, restart=True)
        assert ctx.accumulated_samples() == 1


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_tile_shares_assemble_the_frame(rt_api):
    scene = scenes.cornell12()
    w, h, tile, bounces = 96, 80, 32, 3
    want, _ = _frame(rt_api, scene, w, h, 5, bounces, tile_size=tile)
    rgb, comb = np.zeros_like(want[0]), np.zeros_like(want[1])
    for rank in (0, 1):
        with rt_api.Context() as ctx:
            ctx.upload_scene(scene)
            _accumulate(ctx, scene, w, h, [2, 3], bounces, tile_size=tile, tile_world=2, tile_rank=rank)
            got = _images(ctx)
        m = _owned(w, h, tile, 2, rank)
        rgb[m], comb[m] = got[0][m], got[1][m]
    _assert_same_images((rgb, comb), want)


def test_two_device_context(rt_api):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    scene = scenes.cornell12()
    w, h, tile, bounces = 96, 80, 32, 3
    want, _ = _frame(rt_api, scene, w, h, 5, bounces, tile_size=tile)
    with rt_api.Context((0, 1)) as ctx:
        ctx.upload_scene(scene)
        _accumulate(ctx, scene, w, h, [2, 3], bounces, tile_size=tile)
        _assert_same_images(_images(ctx), want)


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_front_end_progressive(tmp_path):
    exe = os.path.join(ROOT, "build", "rt_render")
    a, b = str(tmp_path / "a.exr"), str(tmp_path / "b.exr")
    out = subprocess.run([exe, "--size", "160x96", "--spp", "2", "--progressive", "3", "--out", a], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "6 samples accumulated" in out.stdout and out.stdout.count("progressive call") == 3
    out = subprocess.run([exe, "--size", "160x96", "--spp", "6", "--out", b], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert open(a, "rb").read() == open(b, "rb").read()  # the same writer: the same float pixels give the same file
