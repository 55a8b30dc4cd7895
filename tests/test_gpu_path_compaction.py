"""The wavefront pipeline with compacted path state (k_wf_finish writes a continuing path's record at the slot it reserves in the next
extension queue, so from depth 1 on a path's id is its queue position and its sample goes back to its origin slot).

Bit-for-bit against the CPU statement and the two megakernels (which keep a path in registers) on workloads that end paths at every
depth: misses into the sky, glass (transmission with the channel split), metal (absorption below the surface), Russian roulette from
depth 2, invalid hits.  Frames here are small, so the producing waves' reservation windows make the queue positions - the compacted
ids - run far beyond the batch's path slots: the arrays indexed by id are read and written in their padding range."""
import numpy as np
import pytest

from gpu_raytracer_amd import scenes

pytestmark = pytest.mark.gpu

MEGAKERNELS = {"state_machine": {"kernel_sm": True}, "nested": {"kernel_v1": True}}


def _u32(a):
    return a.view(np.uint32)


def _render(rt_api, scene, w, h, spp, bounces, **kw):
    """One closed frame in a fresh context (the batch size and lanes are chosen per allocation): image and stats."""
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        st = ctx.render(w, h, scene.camera, mode=2, spp=spp, max_bounces=bounces, **kw)
        return ctx.read_rgb32f(), st


def _soup():
    return scenes.random_soup(300, seed=5, size=0.6, n_spheres=3, n_lights=3)  # metal, glass, emissive, diffuse; open sky around it


CASES = [("soup", _soup, 37, 23, 5, 1), ("soup", _soup, 37, 23, 5, 4), ("soup", _soup, 29, 17, 3, 8),
         ("cornell12", scenes.cornell12, 40, 33, 4, 8), ("default", scenes.default_scene, 45, 27, 4, 4)]


@pytest.mark.parametrize("name,make,w,h,spp,bounces", CASES, ids=[f"{c[0]}-{c[2]}x{c[3]}-{c[4]}spp-{c[5]}b" for c in CASES])
def test_pipeline_bit_exact_vs_statement_and_megakernels(rt_api, oracle_mod, name, make, w, h, spp, bounces):
    scene = make()
    ref = oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), w, h, spp, bounces, frame_seed=11)
    rgb, st = _render(rt_api, scene, w, h, spp, bounces, frame_seed=11)
    seg = ref["segments"]
    assert (st["primary_rays"], st["continuation_rays"], st["shadow_rays"]) == (seg["camera"], seg["continuation"], seg["shadow"])
    if bounces >= 2:
        assert seg["continuation"] < seg["camera"] * bounces  # paths do end before the last bounce: the queues thin out
    np.testing.assert_array_equal(_u32(rgb), _u32(ref["rgb"]))
    for kernel, kw in MEGAKERNELS.items():
        mk, _ = _render(rt_api, scene, w, h, spp, bounces, frame_seed=11, **kw)
        np.testing.assert_array_equal(_u32(rgb), _u32(mk), err_msg=kernel)


@pytest.mark.parametrize("lanes", ["1", "2"])
@pytest.mark.parametrize("batch", ["1", "3"])
def test_batches_and_lanes(rt_api, oracle_mod, monkeypatch, lanes, batch):
    """Several batches (RT_WF_BATCH) on one lane or alternating between two (RT_WF_LANES): every batch starts on the first state set
    again, whatever parity the previous one ended on."""
    scene = _soup()
    w, h, spp, bounces = 35, 21, 7, 5
    ref = oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), w, h, spp, bounces, frame_seed=3)
    monkeypatch.setenv("RT_WF_LANES", lanes)
    monkeypatch.setenv("RT_WF_BATCH", batch)
    rgb, _ = _render(rt_api, scene, w, h, spp, bounces, frame_seed=3)
    np.testing.assert_array_equal(_u32(rgb), _u32(ref["rgb"]))


@pytest.mark.parametrize("tile", [8, 16])
def test_small_tiles_many_blocks(rt_api, oracle_mod, tile):
    """Small tiles over a ragged frame: many pixel blocks without a full set of pixels, queue positions far beyond the path slots."""
    scene = _soup()
    w, h, spp, bounces = 61, 45, 3, 4
    ref = oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), w, h, spp, bounces, frame_seed=9)
    rgb, _ = _render(rt_api, scene, w, h, spp, bounces, frame_seed=9, tile_size=tile)
    np.testing.assert_array_equal(_u32(rgb), _u32(ref["rgb"]))


def test_accumulating_calls_equal_one_frame(rt_api):
    scene = _soup()
    w, h, bounces = 33, 19, 6
    want, _ = _render(rt_api, scene, w, h, 6, bounces)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        for n in (2, 4):
            ctx.render(w, h, scene.camera, mode=2, spp=n, max_bounces=bounces, accumulate=True)
        assert ctx.accumulated_samples() == 6
        got = ctx.read_rgb32f()
    np.testing.assert_array_equal(_u32(got), _u32(want))
