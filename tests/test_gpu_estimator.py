"""The extended mode's estimator against closed-form expectations, on the HIP kernels.

test_estimator_oracle.py pins the CPU statement to the closed forms of estimator_cases.py; here every device implementation is
(a) bit-identical to that statement on the same frames and (b) held to the same closed-form assertions on its own output, and
the queue pipeline is taken to 4096 samples per pixel - more than the CPU can afford - under the correspondingly tighter bands,
with the light grids and camera beams on and off.
"""
import numpy as np
import pytest

import estimator_cases as ec
from test_estimator_oracle import (DIRECT_KINDS, DIRECT_SPP, FURNACE_SPP, GLASS_SPP, HERO_FRAMES, MIRROR_SPP, ROUGH_CASES, ROUGH_SPP,
                                   SKY_WALL_SPP)
from test_gpu_extended import KERNELS

pytestmark = pytest.mark.gpu


def _furnace(b):
    w, h, spp = FURNACE_SPP[b]
    return (lambda: ec.furnace(b, w, h)), spp, ec.check_furnace


CASES = {f"furnace_b{b}": _furnace(b) for b in FURNACE_SPP}
CASES.update({f"sky_{k}": ((lambda k=k: ec.sky_wall(k)), SKY_WALL_SPP, ec.check_sky_wall) for k in ec.WALL_LAYOUTS})
CASES.update({f"glass_T{t}": ((lambda t=t: ec.glass_over_black_floor(t)), GLASS_SPP, ec.check_glass_black) for t in (0.25, 1.0)})
CASES.update({"glass_hero": (ec.glass_over_emissive_floor, GLASS_SPP, ec.check_hero), "glass_slab": (ec.glass_slab, GLASS_SPP, ec.check_hero),
              "mirror": (ec.mirror, MIRROR_SPP, ec.check_mirror)})
CASES.update({f"direct_{k}": ((lambda k=k: ec.direct_light(k)), DIRECT_SPP, ec.check_direct_light) for k in DIRECT_KINDS})
CASES.update({"refract_front": (ec.refract_front, 1, ec.check_refract_front), "tir_back": (ec.tir_back, 1, ec.check_tir_back)})
CASES.update({f"rough_metal_{r}_{l}": ((lambda r=r, l=l: ec.rough_metal(r, l)), ROUGH_SPP, ec.check_rough_metal) for r, l in ROUGH_CASES})
# checks that also take the frame's segment counts
WITH_SEGMENTS = (ec.check_direct_light, ec.check_refract_front, ec.check_tir_back, ec.check_rough_metal)

PRIMARY_ONLY = [name for name, (make, _, _) in CASES.items() if make().bounces == 0]
PATHS = [(name, kernel) for name in CASES for kernel in KERNELS] + [(name, "one_pass") for name in PRIMARY_ONLY]

_STATEMENT = {}


def _statement(oracle_mod, name, case, spp):
    if name not in _STATEMENT:
        _STATEMENT[name] = oracle_mod.render_extended(oracle_mod.PackedScene(case.scene, use_bvh=False), case.w, case.h, spp,
                                                      case.bounces, frame_seed=case.frame_seed)
    return _STATEMENT[name]


@pytest.mark.parametrize("name,kernel", PATHS, ids=[f"{n}-{k}" for n, k in PATHS])
def test_every_kernel_path_meets_the_closed_forms(gpu_ctx, oracle_mod, rt_api, name, kernel):
    """wavefront pipeline, state-machine megakernel, nested-loop megakernel, and the one-pass kernel where B = 0: the statement's
    bits and segment counts, and the closed form on the device's own image."""
    make, spp, check = CASES[name]
    case = make()
    ref = _statement(oracle_mod, name, case, spp)
    kw = dict(KERNELS.get(kernel, {}))
    if kernel == "wavefront" and case.bounces == 0:
        kw["kernel_pipeline"] = True   # a B = 0 frame over a tiny tree takes the one-pass kernel unless told otherwise
    gpu_ctx.upload_scene(case.scene)
    st = gpu_ctx.render(case.w, case.h, case.scene.camera, mode=2, spp=spp, max_bounces=case.bounces, frame_seed=case.frame_seed, **kw)
    assert bool(st["flags"] & rt_api.STAT_SINGLE_PASS) == (kernel == "one_pass")
    rgb = gpu_ctx.read_rgb32f()
    seg = ref["segments"]
    assert (st["primary_rays"], st["continuation_rays"], st["shadow_rays"]) == (seg["camera"], seg["continuation"], seg["shadow"])
    np.testing.assert_array_equal(rgb.view(np.uint32), ref["rgb"].view(np.uint32))
    if check is ec.check_furnace:
        check(rgb, case, spp, st["continuation_rays"])
    elif check in WITH_SEGMENTS:
        check(rgb, case, spp, {"camera": st["primary_rays"], "continuation": st["continuation_rays"], "shadow": st["shadow_rays"]})
    else:
        check(rgb, case, spp)


DEEP_SPP, DEEP_CALLS = 4096, 8
DEEP = {"furnace_b6": (lambda: ec.furnace(6, 128, 128), ec.check_furnace)}
DEEP.update({f"sky_{k}": ((lambda k=k: ec.sky_wall(k)), ec.check_sky_wall) for k in ec.WALL_LAYOUTS})
DEEP.update({"glass_T0.25": (lambda: ec.glass_over_black_floor(0.25), ec.check_glass_black),
             "glass_hero": (ec.glass_over_emissive_floor, ec.check_hero), "glass_slab": (ec.glass_slab, ec.check_hero)})
# the absorbed cap at 64 x 64: Hoeffding's band of 1.7e7 samples is 7.2e-5 in red (64 spp: 5.8e-4)
DEEP["rough_metal_1.0_front"] = (lambda: ec.rough_metal(1.0, "front"), ec.check_rough_metal)
DEEP_SIZE = {"rough_metal_1.0_front": (64, 64)}


@pytest.mark.parametrize("name", list(DEEP))
def test_pipeline_at_4096_spp_with_and_without_grids_and_beams(gpu_ctx, name):
    """128 x 128 (the rough metal: 64 x 64) accumulated to 4096 samples per pixel in 8 calls on the queue pipeline, once as the
    library would run it and once with RT_FLAG_NO_SHADOW_GRID | RT_FLAG_NO_BEAMS: the same bits, and the closed form within the band
    of 6.7e7 (1.7e7) samples."""
    make, check = DEEP[name]
    case = make()
    assert (case.w, case.h) == DEEP_SIZE.get(name, (128, 128))
    gpu_ctx.upload_scene(case.scene)
    images = []
    for flags in ({}, {"no_shadow_grid": True, "no_beams": True}):
        for call in range(DEEP_CALLS):
            gpu_ctx.render(case.w, case.h, case.scene.camera, mode=2, spp=DEEP_SPP // DEEP_CALLS, max_bounces=case.bounces,
                           frame_seed=case.frame_seed, accumulate=True, restart=(call == 0), **flags)
        assert gpu_ctx.accumulated_samples() == DEEP_SPP
        images.append(gpu_ctx.read_rgb32f())
    np.testing.assert_array_equal(images[0].view(np.uint32), images[1].view(np.uint32))
    check(images[0], case, DEEP_SPP)


def test_hero_pick_is_uniform_over_disjoint_streams(gpu_ctx):
    """refract_front on the queue pipeline with frame seeds w * h apart: each frame meets the closed form, and over the pixels whose
    three channels all land on the emitter the hero counts pass chi-square (estimator_cases.check_hero_uniform)."""
    case = ec.refract_front()
    gpu_ctx.upload_scene(case.scene)
    images = []
    for k in range(HERO_FRAMES):
        case.frame_seed = k * case.w * case.h
        gpu_ctx.render(case.w, case.h, case.scene.camera, mode=2, spp=1, max_bounces=case.bounces, frame_seed=case.frame_seed)
        images.append(gpu_ctx.read_rgb32f())
        ec.check_refract_front(images[-1], case, 1)
    ec.check_hero_uniform(images, case)


def test_sample_rays_follow_the_restated_sampler(gpu_ctx):
    """rt_sample_rays of a 64 x 64, 8-spp frame: each direction is the float64 camera ray through the restated jitter within
    CAMERA_DIR_F32_BOUND (32 * 2^-24, derived in estimator_cases.py), each origin the camera position."""
    case = ec.mirror(w=64, h=64)
    case.frame_seed = 12345
    gpu_ctx.upload_scene(case.scene)
    o, d = case.rays(np.arange(8))
    worst = 0.0
    for s in range(8):
        rays = gpu_ctx.sample_rays(case.w, case.h, case.scene.camera, s, spp=8, frame_seed=case.frame_seed).reshape(case.h, case.w, 8)
        np.testing.assert_array_equal(rays[..., 0:3], np.broadcast_to(o.astype(np.float32), rays[..., 0:3].shape))
        worst = max(worst, float(np.abs(rays[..., 4:7].astype(np.float64) - d[s]).max()))
    print(f"largest direction error {worst:.3e}, bound {ec.CAMERA_DIR_F32_BOUND:.3e}")
    assert worst <= ec.CAMERA_DIR_F32_BOUND
    # a jitter of half a pixel is 0.5 / 64 * 2 tan(20 deg) = 5.7e-3 in direction: the bound tells the streams apart
    centre = ec.camera_rays(case.scene.camera, case.w, case.h, 0.5, 0.5)[1]
    assert np.abs(centre - d[0]).max() > 100 * ec.CAMERA_DIR_F32_BOUND
