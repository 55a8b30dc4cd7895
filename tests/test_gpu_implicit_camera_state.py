"""The depth-0 path state of the wavefront pipeline is derived, not stored (csrc/wavefront.hip, wf_camera_state): k_wf_generate writes
only the rays the tree walk reads, k_wf_trace_camera and the depth-0 k_wf_finish work origin, direction, rng state, throughput, radiance,
channel, depth and origin slot out from the frame and the slot number.  A slip in that arithmetic gives a path another pixel's or another
sample's ray, so every comparison here is on whole byte strings, against yardsticks that never had a stored camera state or keep it:

  kernel_sm=True   the state-machine megakernel;
  no_beams=True    every slot keeps its stored ray, only throughput, radiance and the finish side are derived;
  the CPU oracle   oracle.render_extended, brute force.

The cases sit where slot arithmetic can go wrong: images whose blocks have lanes outside the image, sample counts one below, at and one
above the 8-sample chunk of k_wf_trace_camera (chunks start at k = 0, 8, 16), paths that end at depth 0, continue once or several times,
jitter on and off, tile partitions, sample_base != 0 (accumulation), first_sample != 0 (batches, on one lane and two), blocks with a
list beside blocks whose segments walk the tree, spheres, and a frame of sky.  rt_render_adaptive keeps the stored state and must still
give its own bits."""
import numpy as np
import pytest

import beam_edge_cases as ec
from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import scenes
from test_gpu_adaptive import np_error

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
KEYS = ("primary_rays", "continuation_rays", "shadow_rays")
PIPELINE = dict(kernel_pipeline=True)                 # (max_bounces 0 over a small tree would take the one-pass kernel otherwise)
YARDSTICKS = {"state machine": dict(kernel_sm=True), "stored rays": dict(kernel_pipeline=True, no_beams=True)}
SPPS = (1, 8, 9, 17)                                  # RT_BEAM_SAMPLES_PER_WAVE = 8
SEEDS = (3, 0x9E3779B9)


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


# ragged images -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [0, 1, 3])
@pytest.mark.parametrize("w,h", [(70, 45), (9, 7)])
@pytest.mark.parametrize("name", ["cornell12", "default"])  # default: six spheres over two triangles
def test_ragged_images(gpu_ctx, oracle_mod, name, w, h, bounces):
    scene = scenes.SCENES[name]()
    gpu_ctx.upload_scene(scene)
    for spp in SPPS:  # spp 1: pixel centres, no jitter; above: jitter
        for seed in SEEDS:
            kw = dict(spp=spp, max_bounces=bounces, frame_seed=seed)
            got = _frame(gpu_ctx, w, h, scene.camera, **kw, **PIPELINE)
            assert got[2][0] == w * h * spp
            for what, flags in YARDSTICKS.items():
                _assert_equal(got, _frame(gpu_ctx, w, h, scene.camera, **kw, **flags), w, h, f"{name} {w}x{h} spp {spp} bounces {bounces} seed {seed}: {what}")
        assert got[0] == _oracle(oracle_mod, scene, w, h, spp, bounces, scene.camera, SEEDS[-1]), f"{name} {w}x{h} spp {spp} bounces {bounces}: the oracle"


# tile partitions -----------------------------------------------------------------------------------------------------------------
def test_tile_partitions(gpu_ctx):
    scene = scenes.cornell12()
    gpu_ctx.upload_scene(scene)
    w, h, tile, world = 70, 45, 12, 3
    kw = dict(spp=9, max_bounces=3, frame_seed=SEEDS[0])
    whole = _frame(gpu_ctx, w, h, scene.camera, tile_size=tile, **kw)
    _assert_equal(whole, _frame(gpu_ctx, w, h, scene.camera, **kw, **YARDSTICKS["state machine"]), w, h, "tile 12, one rank: state machine")
    acc, segs = np.zeros((h, w, 3), np.float32), np.zeros(3, np.int64)
    for rank in range(world):
        st = gpu_ctx.render(w, h, scene.camera, mode=2, tile_size=tile, tile_rank=rank, tile_world=world, **kw)
        own = ec.owned_mask(w, h, tile, rank, world)
        assert st["primary_rays"] == int(own.sum()) * kw["spp"]
        acc[own] = gpu_ctx.read_rgb32f()[own]
        segs += [st[k] for k in KEYS]
    assert acc.tobytes() == whole[0] and tuple(int(v) for v in segs) == whole[2]


# accumulation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,second", [(8, 9), (1, 1)])
def test_accumulating_calls(rt_api, first, second):
    """The second call has sample_base = first; an accumulating call jitters at spp 1 too."""
    scene = scenes.cornell12()
    w, h, bounces = 70, 45, 3
    with rt_api.Context() as ctx, rt_api.Context() as ref:
        ctx.upload_scene(scene)
        ref.upload_scene(scene)
        for i, spp in enumerate((first, second)):
            kw = dict(spp=spp, max_bounces=bounces, frame_seed=SEEDS[0], accumulate=True, restart=i == 0)
            got = _frame(ctx, w, h, scene.camera, **kw)
            _assert_equal(got, _frame(ref, w, h, scene.camera, **kw, **YARDSTICKS["state machine"]), w, h, f"accumulating call {i}: state machine")
        assert ctx.accumulated_samples() == first + second
        closed = _frame(ref, w, h, scene.camera, spp=first + second, max_bounces=bounces, frame_seed=SEEDS[0])
        assert got[0] == closed[0], "two accumulating calls against one frame of all the samples"


# batches and lanes ---------------------------------------------------------------------------------------------------------------
def test_batches_on_one_lane_and_two(rt_api, monkeypatch):
    """Two lanes cut a frame of two or more samples into two batches (first_sample != 0 in the second, on the second lane's buffers);
    RT_WF_LANES=1 with RT_WF_BATCH=2 runs three batches of a 5-sample frame on one lane."""
    scene = scenes.sponza_like()
    w, h, bounces = 480, 270, 4
    want = {}
    with rt_api.Context() as ref:
        ref.upload_scene(scene)
        for spp in (2, 5):
            want[spp] = _frame(ref, w, h, scene.camera, spp=spp, max_bounces=bounces, frame_seed=SEEDS[0], kernel_sm=True)
    for lanes, batch in (("2", None), ("1", None), ("1", "2")):
        monkeypatch.setenv("RT_WF_LANES", lanes)
        if batch:
            monkeypatch.setenv("RT_WF_BATCH", batch)
        with rt_api.Context() as ctx:
            ctx.upload_scene(scene)
            for spp in (2, 5):
                got = _frame(ctx, w, h, scene.camera, spp=spp, max_bounces=bounces, frame_seed=SEEDS[0])
                _assert_equal(got, want[spp], w, h, f"lanes {lanes} batch {batch} spp {spp}: state machine")


# listed blocks and tree-walk blocks in one frame ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [0, 3])
@pytest.mark.parametrize("frame", ["20x12 tile 12", "32x16 rank 1 of 3"])
def test_listed_and_tree_walk_blocks(gpu_ctx, oracle_mod, frame, bounces):
    """Every other block's list is past the cap of 128: its segments walk the tree from stored rays, its neighbours' come from the slot."""
    case = ec.fallback(frame, "alternate", spp=9)
    scene = case.scene()
    gpu_ctx.upload_scene(scene)
    for spp in (9, 1):
        kw = dict(case.render_kw(spp), max_bounces=bounces)
        del kw["mode"], kw["kernel_pipeline"]
        got = _frame(gpu_ctx, case.w, case.h, case.camera, **kw, **PIPELINE)
        lists = gpu_ctx.debug_beams(1 << 20)
        assert (lists == NONE).any() and (lists != NONE).any(), lists.tolist()
        assert got[2][0] == int(ec.owned_mask(case.w, case.h, case.tile, case.rank, case.world).sum()) * spp
        for what, flags in YARDSTICKS.items():
            _assert_equal(got, _frame(gpu_ctx, case.w, case.h, case.camera, **kw, **flags), case.w, case.h, f"{case.name} spp {spp} bounces {bounces}: {what}")
        own = ec.owned_mask(case.w, case.h, case.tile, case.rank, case.world)
        ref = np.frombuffer(_oracle(oracle_mod, scene, case.w, case.h, spp, bounces, case.camera, case.frame_seed), np.uint32).reshape(case.h, case.w, 3)
        img = np.frombuffer(got[0], np.uint32).reshape(case.h, case.w, 3)
        assert (img[own] == ref[own]).all(), f"{case.name} spp {spp} bounces {bounces}: the oracle"


# rt_render_adaptive keeps the stored state ---------------------------------------------------------------------------------------
def test_adaptive_calls_still_run_on_stored_state(rt_api):
    """spp samples per selected pixel, each pixel from its own count n: the pipeline's adaptive variants against the state machine's."""
    scene = scenes.cornell12()
    w, h = 70, 45
    with rt_api.Context() as ctx, rt_api.Context() as ref:
        ctx.upload_scene(scene)
        ref.upload_scene(scene)
        pixels, t = [], 0.0
        for i, spp in enumerate((2, 2, 4, 9)):
            kw = dict(min_samples=4, max_bounces=3, frame_seed=SEEDS[0], restart=i == 0)
            a = ctx.render_adaptive(w, h, scene.camera, spp, t, **kw)
            b = ref.render_adaptive(w, h, scene.camera, spp, t, kernel_sm=True, **kw)
            assert tuple(a[k] for k in KEYS) == tuple(b[k] for k in KEYS) and a["pixels"] == b["pixels"]
            assert ctx.read_rgb32f().tobytes() == ref.read_rgb32f().tobytes(), f"adaptive call {i}"
            assert ctx.read_adaptive().tobytes() == ref.read_adaptive().tobytes(), f"adaptive call {i}"
            pixels.append(a["pixels"])
            if i == 1:  # every pixel has its four samples: from here on a threshold that stops the quieter 60 % of those with any error
                e = np_error(ctx.read_adaptive())
                t = float(np.quantile(e[np.isfinite(e) & (e > 0)], 0.6))
        assert pixels[0] == pixels[1] == w * h and 0 < pixels[3] <= pixels[2] < w * h, pixels  # pixels stopped, pixels went on: their sample bases differ


# a frame of sky ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 9])
def test_a_frame_of_sky(gpu_ctx, oracle_mod, spp):
    """The camera looks away from the box: every path ends at depth 0 through the "no vertex" branch (0 + sky x 1)."""
    scene = scenes.cornell12()
    cam = H.camera(position=(0.0, 0.0, 3.4), direction=(0.0, 0.3, 1.0))
    gpu_ctx.upload_scene(scene)
    w, h = 70, 45
    kw = dict(spp=spp, max_bounces=3, frame_seed=SEEDS[1])
    got = _frame(gpu_ctx, w, h, cam, **kw)
    assert got[2] == (w * h * spp, 0, 0)
    for what, flags in YARDSTICKS.items():
        _assert_equal(got, _frame(gpu_ctx, w, h, cam, **kw, **flags), w, h, f"sky spp {spp}: {what}")
    assert got[0] == _oracle(oracle_mod, scene, w, h, spp, 3, cam, SEEDS[1])
