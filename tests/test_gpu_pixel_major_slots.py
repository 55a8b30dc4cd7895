"""The path slots of a wavefront batch are pixel-major (csrc/wf_slots.h): slot p = (b * 64 + j) * n_samples + k, so a wave of every depth-0
stage holds all samples of a few neighbouring pixels and a lane's pixel AND sample both follow from a division by the batch's own sample
count.  A slip there gives a path another pixel's or another sample's ray, or adds a pixel's samples out of order, so whole frames are
compared bit for bit with yardsticks the layout cannot touch:

  kernel_sm=True   the state-machine megakernel (no slots, no queues);
  the CPU oracle   oracle.render_extended, brute force (on the frames small enough for it).

The cases sit where the arithmetic can go wrong: samples per batch (RT_WF_BATCH) below, at and above the 64 lanes of a wave, dividing 64
or not (a pixel's samples end inside a wave, fill one exactly, span several), a shorter last batch, one lane and two, images whose blocks
miss pixels or have none, the two ways k_wf_resolve reads a block's samples, tile partitions, blocks whose camera segments walk the tree
(the dense second queue), accumulating and adaptive calls, and a frame of sky.  The mapping itself is held to its statement on the host
by tests/check_wf_slots.cpp, in all three orders."""
import os
import re
import subprocess

import numpy as np
import pytest

import beam_edge_cases as ec
from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import scenes
from test_gpu_adaptive import np_error

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
KEYS = ("primary_rays", "continuation_rays", "shadow_rays")
NONE = 0xFFFFFFFF
SEED = 0x9E3779B9
BOUNCES = 3
BATCHES = (1, 2, 3, 5, 21, 32, 33, 64, 65, 85, 86, 100)  # 85 / 86: the last batch k_wf_resolve stages through LDS, the first it reads by lane
ORACLE_UP_TO_SPP = 13  # brute force over every triangle per segment: the frames of the four smallest batches


def _spp_for(batch):
    """Two whole batches and a shorter last one (a batch of one sample cannot be cut short: three of them)."""
    return 3 if batch == 1 else 2 * batch + (batch + 1) // 2


def _scene():
    """240 triangles and two spheres in front of the default camera; of the six materials two are metallic, one transmits, one emits and
    the rest are diffuse (all three branches of ext_scatter); a point, a directional, a spot and another point light."""
    return scenes.random_soup(240, seed=5, n_materials=6, n_spheres=2, n_lights=4)


def _frame(ctx, w, h, cam, **kw):
    """-> (float image bytes, rgba8 bytes, segment counts)"""
    st = ctx.render(w, h, cam, mode=2, **kw)
    return ctx.read_rgb32f().tobytes(), ctx.read_rgba8_combined().tobytes(), tuple(st[k] for k in KEYS)


def _assert_equal(got, want, w, h, what):
    if got[0] != want[0]:
        a, b = (np.frombuffer(x[0], np.uint32).reshape(h, w, 3) for x in (got, want))
        diff = np.argwhere((a != b).any(-1))
        y, x = (int(v) for v in diff[0])
        raise AssertionError(f"{what}: {len(diff)} of {w * h} pixels differ, first at (x, y) = ({x}, {y}): {a[y, x].view(np.float32)} != {b[y, x].view(np.float32)}")
    assert got[1] == want[1], f"{what}: rgba8 targets differ"
    assert got[2] == want[2], f"{what}: segment counts {got[2]} != {want[2]}"


def _oracle(oracle_mod, scene, w, h, spp, bounces, cam, seed):
    return oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), w, h, spp, bounces, camera=cam, frame_seed=seed)["rgb"].tobytes()


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    monkeypatch.delenv("RT_WF_BATCH", raising=False)
    monkeypatch.delenv("RT_WF_LANES", raising=False)


# samples per batch ---------------------------------------------------------------------------------------------------------------
BW, BH = 44, 28  # 6 x 4 blocks, the last column and the last row with pixels missing


@pytest.fixture(scope="module")
def batch_yardsticks(rt_api):
    """The state machine's frame for every sample count of the batch cases, rendered once."""
    scene = _scene()
    want = {}
    with rt_api.Context() as ref:
        ref.upload_scene(scene)
        for spp in sorted({_spp_for(b) for b in BATCHES}):
            want[spp] = _frame(ref, BW, BH, scene.camera, spp=spp, max_bounces=BOUNCES, frame_seed=SEED, kernel_sm=True)
    return want


@gpu
@pytest.mark.parametrize("lanes", ["1", "2"])
@pytest.mark.parametrize("batch", BATCHES)
def test_samples_per_batch(rt_api, oracle_mod, batch_yardsticks, monkeypatch, batch, lanes):
    scene = _scene()
    spp = _spp_for(batch)
    monkeypatch.setenv("RT_WF_BATCH", str(batch))
    monkeypatch.setenv("RT_WF_LANES", lanes)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        got = _frame(ctx, BW, BH, scene.camera, spp=spp, max_bounces=BOUNCES, frame_seed=SEED, kernel_pipeline=True)
    assert got[2][0] == BW * BH * spp
    _assert_equal(got, batch_yardsticks[spp], BW, BH, f"batch {batch} spp {spp} lanes {lanes}: state machine")
    if spp <= ORACLE_UP_TO_SPP and lanes == "1":
        assert got[0] == _oracle(oracle_mod, scene, BW, BH, spp, BOUNCES, scene.camera, SEED), f"batch {batch} spp {spp}: the oracle"


# ragged images and small tiles ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batch,spp", [(5, 13), (33, 40)])
def test_ragged_image_in_small_tiles(rt_api, oracle_mod, monkeypatch, batch, spp):
    """37 x 29 in tiles of 16: 3 x 2 tiles of 2 x 2 blocks; the tiles of the last column are 5 pixels wide and those of the last row 13
    high, so some blocks have lanes without a pixel and some have none at all (wave-groups without a pixel).  Then the same frame as
    three shares of a tile partition."""
    scene = _scene()
    w, h, tile, world = 37, 29, 16, 3
    monkeypatch.setenv("RT_WF_BATCH", str(batch))
    kw = dict(spp=spp, max_bounces=BOUNCES, frame_seed=SEED, tile_size=tile)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        whole = _frame(ctx, w, h, scene.camera, kernel_pipeline=True, **kw)
        assert whole[2][0] == w * h * spp
        _assert_equal(whole, _frame(ctx, w, h, scene.camera, kernel_sm=True, **kw), w, h, f"37x29 tile 16 batch {batch}: state machine")
        if spp <= ORACLE_UP_TO_SPP:
            assert whole[0] == _oracle(oracle_mod, scene, w, h, spp, BOUNCES, scene.camera, SEED), "37x29 tile 16: the oracle"
        acc, segs = np.zeros((h, w, 3), np.float32), np.zeros(3, np.int64)
        for rank in range(world):
            st = ctx.render(w, h, scene.camera, mode=2, tile_rank=rank, tile_world=world, kernel_pipeline=True, **kw)
            own = ec.owned_mask(w, h, tile, rank, world)
            assert st["primary_rays"] == int(own.sum()) * spp
            acc[own] = ctx.read_rgb32f()[own]
            segs += [st[k] for k in KEYS]
        assert acc.tobytes() == whole[0] and tuple(int(v) for v in segs) == whole[2]


# blocks without a beam list ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batch,spp", [(3, 8), (5, 13), (65, 70)])
@pytest.mark.parametrize("frame", ["20x12 tile 12", "32x16 rank 1 of 3"])
def test_listed_and_tree_walk_blocks(rt_api, oracle_mod, monkeypatch, frame, batch, spp):
    """Every other block's list is past the cap: its segments reach the tree walk through the dense second queue, wave-group by wave-group;
    with no_beams=True every block's do, through the first queue."""
    case = ec.fallback(frame, "alternate", spp=spp)
    scene = case.scene()
    monkeypatch.setenv("RT_WF_BATCH", str(batch))
    kw = dict(case.render_kw(spp), max_bounces=BOUNCES)
    del kw["mode"], kw["kernel_pipeline"]
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        got = _frame(ctx, case.w, case.h, case.camera, kernel_pipeline=True, **kw)
        lists = ctx.debug_beams(1 << 20)
        assert (lists == NONE).any() and (lists != NONE).any(), lists.tolist()
        own = ec.owned_mask(case.w, case.h, case.tile, case.rank, case.world)
        assert got[2][0] == int(own.sum()) * spp
        want = _frame(ctx, case.w, case.h, case.camera, kernel_sm=True, **kw)
        _assert_equal(got, want, case.w, case.h, f"{case.name} batch {batch}: state machine")
        _assert_equal(_frame(ctx, case.w, case.h, case.camera, kernel_pipeline=True, no_beams=True, **kw), want, case.w, case.h, f"{case.name} batch {batch}, no beams: state machine")
    if spp <= ORACLE_UP_TO_SPP:
        ref = np.frombuffer(_oracle(oracle_mod, scene, case.w, case.h, spp, BOUNCES, case.camera, case.frame_seed), np.uint32).reshape(case.h, case.w, 3)
        img = np.frombuffer(got[0], np.uint32).reshape(case.h, case.w, 3)
        assert (img[own] == ref[own]).all(), f"{case.name} batch {batch}: the oracle"


# accumulation --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batch", [3, 21])
def test_accumulating_calls(rt_api, monkeypatch, batch):
    """The second call has sample_base = 23 and runs its own batches from there."""
    scene = _scene()
    w, h, first, second = 64, 48, 23, 25
    monkeypatch.setenv("RT_WF_BATCH", str(batch))
    with rt_api.Context() as ctx, rt_api.Context() as ref:
        ctx.upload_scene(scene)
        ref.upload_scene(scene)
        for i, spp in enumerate((first, second)):
            kw = dict(spp=spp, max_bounces=BOUNCES, frame_seed=SEED, accumulate=True, restart=i == 0)
            got = _frame(ctx, w, h, scene.camera, kernel_pipeline=True, **kw)
            _assert_equal(got, _frame(ref, w, h, scene.camera, kernel_sm=True, **kw), w, h, f"accumulating call {i}, batch {batch}: state machine")
        assert ctx.accumulated_samples() == first + second
        closed = _frame(ref, w, h, scene.camera, spp=first + second, max_bounces=BOUNCES, frame_seed=SEED, kernel_sm=True)
        assert got[0] == closed[0], "two accumulating calls against one frame of all the samples"


# adaptive calls ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batch", [None, 3])
def test_adaptive_calls(rt_api, monkeypatch, batch):
    """rt_render_adaptive (the AD variants of generate and resolve): spp samples per selected pixel, each pixel from its own count, lanes
    that stopped left out of their wave-groups; against the state machine's adaptive calls."""
    scene = _scene()
    w, h = 61, 45
    if batch:
        monkeypatch.setenv("RT_WF_BATCH", str(batch))
    with rt_api.Context() as ctx, rt_api.Context() as ref:
        ctx.upload_scene(scene)
        ref.upload_scene(scene)
        pixels, t = [], 0.0
        for i, spp in enumerate((2, 2, 5, 9)):
            kw = dict(min_samples=4, max_bounces=BOUNCES, frame_seed=SEED, restart=i == 0)
            a = ctx.render_adaptive(w, h, scene.camera, spp, t, **kw)
            b = ref.render_adaptive(w, h, scene.camera, spp, t, kernel_sm=True, **kw)
            assert tuple(a[k] for k in KEYS) == tuple(b[k] for k in KEYS) and a["pixels"] == b["pixels"]
            assert ctx.read_rgb32f().tobytes() == ref.read_rgb32f().tobytes(), f"adaptive call {i}"
            assert ctx.read_adaptive().tobytes() == ref.read_adaptive().tobytes(), f"adaptive call {i}"
            pixels.append(a["pixels"])
            if i == 1:  # every pixel has its four samples: from here on a threshold that stops the quieter 60 % of those with any error
                e = np_error(ctx.read_adaptive())
                t = float(np.quantile(e[np.isfinite(e) & (e > 0)], 0.6))
        assert pixels[0] == pixels[1] == w * h and 0 < pixels[3] <= pixels[2] < w * h, pixels


# a frame of sky ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("batch,spp", [(5, 13), (33, 70)])
def test_a_frame_of_sky(rt_api, oracle_mod, monkeypatch, batch, spp):
    """The camera looks away from the scene: every path ends at depth 0 through the "no vertex" branch."""
    scene = _scene()
    cam = H.camera(position=(0.0, 0.0, 3.4), direction=(0.0, 0.3, 1.0))
    w, h = 61, 45
    monkeypatch.setenv("RT_WF_BATCH", str(batch))
    kw = dict(spp=spp, max_bounces=BOUNCES, frame_seed=SEED)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        got = _frame(ctx, w, h, cam, kernel_pipeline=True, **kw)
        assert got[2] == (w * h * spp, 0, 0)
        _assert_equal(got, _frame(ctx, w, h, cam, kernel_sm=True, **kw), w, h, f"sky batch {batch}: state machine")
    if spp <= ORACLE_UP_TO_SPP:
        assert got[0] == _oracle(oracle_mod, scene, w, h, spp, BOUNCES, cam, SEED)


# the mapping itself, on the host -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 1, 0])
def test_slot_mapping_on_the_host(tmp_path, order):
    """tests/check_wf_slots.cpp under AddressSanitizer + UBSan: n_samples 1 .. 130 x block counts {1, 2, 3, 7, 24, 61} = 780 cases; slot ->
    (b, j, k) -> slot is the identity and every slot is hit exactly once.  Order 2 (pixel-major) is the default; 1 and 0 stay buildable."""
    exe = str(tmp_path / f"check_wf_slots_{order}")
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-fno-sanitize-recover=undefined", f"-DRT_WF_BLOCK_MAJOR={order}", "-I" + CSRC, os.path.join(HERE, "check_wf_slots.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert re.search(r"^780 cases, 0 failures$", run.stdout.strip()), run.stdout[-500:]

