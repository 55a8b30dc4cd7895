"""Irradiance queries on the MI355X (rt_irradiance), held to the calls below it.

Composition: every channel is, bit for bit, the ordered f32 sum times pi / S (irradiance_cases.py) of what rt_radiance gives along the
directions the statement draws from each point's normal, with RT_PATH_CAMERA_DRAWS, sample by sample; the segments and the statistics
are the sums.  Against itself: the kind of memory, the chunking, the device count and the tree change no byte.  Against closed forms:
the sky of an empty scene is pi * sky, and a black sphere over the point takes the cosine-weighted share of its cap away."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import irradiance_cases as ic
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import hostpack as HP
from gpu_raytracer_amd import types as T

import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first; the device-memory cases need it

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
SEED = 0xFFFFFFF0  # the per-point seed wraps at point 16
SKY = np.array([0.1, 0.2, 0.3], F32)
W, H = 10, 7
STAT_KEYS = ("rays", "primary_rays", "continuation_rays", "shadow_rays")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _box_scene():
    """cornell12 with a half-transmissive sphere standing in it."""
    base = scenes.cornell12()
    glass = HP.material_new((0.9, 0.85, 0.95), 0.0, 0.1, (0, 0, 0), 1.5, 0.5)
    materials = np.concatenate([base.materials, np.array([glass], dtype=T.MATERIAL)])
    spheres = np.array([((0.3, -0.55, 0.1), 0.45, len(base.materials))], dtype=T.SPHERE)
    return dataclasses.replace(base, name="probe box", spheres=spheres, materials=materials)


def _make_points(positions, normals):
    p = np.zeros((len(positions), 8), F32)
    p[:, 0:3], p[:, 4:7] = positions, normals
    return p


def _texels(ctx, box):
    """What a baker has after its first pass: rt_surface over the camera rays of a 10 x 7 frame - walls, the sphere, and the misses
    beside the box, whose records have a zero normal - and two hand-made records that are no points either."""
    points = ctx.surface(ctx.camera_rays(W, H, box.camera, mode=1))
    odd = _make_points([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3]], [[0, np.nan, 1], [0, 0, 0]])
    points = np.ascontiguousarray(np.concatenate([points, odd]))
    ok = ic.is_point(points)
    prim = api.split_surface(points)[1]
    assert np.array_equal(ok[:W * H], prim[:W * H] != api.PRIM_MISS), "a miss record of rt_surface is no point, a hit is one"
    assert 10 < ok.sum() < W * H and (~ok).sum() >= 4, "hits and no-points"
    return points, ok


@pytest.fixture(scope="module")
def box():
    return _box_scene()


def compose(ctx, oracle_mod, points, samples, seed, first_sample, max_bounces, shadows):
    """The statement through Context.radiance: one call per sample over the rays (P_i + N_i * 0.001, d_{i,k}) -> (E, segments, summed
    statistics).  The rays' own indices are the points', so the whole array goes in; rule 5 - nothing is traced for a no-point,
    whatever its ray would give - is stated by a zero direction, for which rt_radiance traces nothing either, so the statistics are
    plain sums."""
    n = len(points)
    ok = ic.is_point(points)
    d = ic.directions(oracle_mod, points, np.arange(n), samples, seed, first_sample)
    o = ic.origins(points)
    d[~ok] = 0
    x = np.zeros((n, samples, 3), F32)
    segments = np.zeros(n, U32)
    totals = dict.fromkeys(STAT_KEYS, 0)
    for k in range(samples):
        rays = api.make_rays(o, d[:, k], ic.MIN_T, ic.F32_MAX)
        radiance, g = api.split_radiance(ctx.radiance(rays, samples=1, max_bounces=max_bounces, seed=seed, first_sample=first_sample + k,
                                                      shadows=shadows, camera_draws=True))
        st = ctx.stats()
        for key in STAT_KEYS:
            totals[key] += st[key]
        x[:, k] = radiance
        segments = segments + g
    assert not x[~ok].any() and not segments[~ok].any()
    return ic.reduce(x), segments, totals


# 1. composition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 3, 64, 65])  # a wave holds 64, 21 1/3, 1 and less than one point
def test_is_the_ordered_sum_of_rt_radiance_bit_for_bit(gpu_ctx, oracle_mod, box, samples):
    gpu_ctx.upload_scene(box)
    points, ok = _texels(gpu_ctx, box)
    for bounces in (0, 3):
        for shadows in (True, False):
            for first in (0, 5):
                want, want_segments, totals = compose(gpu_ctx, oracle_mod, points, samples, SEED, first, bounces, shadows)
                got = gpu_ctx.irradiance(points, samples, max_bounces=bounces, seed=SEED, first_sample=first, shadows=shadows)
                st = gpu_ctx.stats()
                e, segments = api.split_irradiance(got)
                label = f"S={samples} max_bounces={bounces} shadows={shadows} first_sample={first}"
                print(label, {k: st[k] for k in STAT_KEYS})
                np.testing.assert_array_equal(_bits(e), _bits(want), err_msg=label)
                np.testing.assert_array_equal(segments, want_segments, err_msg=label)
                assert all(st[k] == totals[k] for k in STAT_KEYS), (label, st, totals)
                assert st["primary_rays"] == int(ok.sum()) * samples and st["pixels"] == 0 and st["kernel_ms"] > 0
                assert st["rays"] == int(segments.astype(np.uint64).sum()) and st["node_visits"] == 0 and st["tri_tests"] == 0
                assert (st["shadow_rays"] > 0) == shadows and (st["continuation_rays"] > 0) == (bounces > 0)
                assert not _bits(got[~ok]).any(), "a no-point is 16 zero bytes"
                assert np.isfinite(e).all() and (e >= 0).all() and (segments[ok] >= samples).all()
                assert len(np.unique(_bits(e[ok, 0]))) > 10, "the points see different things"


# 2. memory, chunks, devices -----------------------------------------------------------------------------------------------------
def test_memory_kinds_and_devices(gpu_ctx, box):
    gpu_ctx.upload_scene(box)
    points, _ = _texels(gpu_ctx, box)
    n = len(points)
    kw = dict(max_bounces=3, seed=SEED, first_sample=3)
    want = gpu_ctx.irradiance(points, 65, **kw)
    st_one = gpu_ctx.stats()
    own = np.full((n, 4), 7, F32)
    assert gpu_ctx.irradiance(points, 65, out=own, **kw) is own and own.tobytes() == want.tobytes()
    assert all(gpu_ctx.stats()[k] == st_one[k] for k in STAT_KEYS)
    dev = torch.from_numpy(points).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    got = gpu_ctx.irradiance(dev, 65, **kw)
    assert got.device == dev.device and got.dtype == torch.float32 and tuple(got.shape) == (n, 4)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert all(gpu_ctx.stats()[k] == st_one[k] for k in STAT_KEYS)
    host = gpu_ctx.irradiance(torch.from_numpy(points.copy()), 65, **kw)
    assert host.device.type == "cpu" and host.numpy().tobytes() == want.tobytes()
    assert all(gpu_ctx.stats()[k] == st_one[k] for k in STAT_KEYS)
    np.testing.assert_array_equal(api.split_irradiance(got)[1].cpu().numpy(), api.split_irradiance(want)[1].astype(np.int64))
    with api.Context((0, 0)) as two:  # each device gets a contiguous range of the points; the seed's index stays the caller's
        two.upload_scene(box)
        assert two.irradiance(points, 65, **kw).tobytes() == want.tobytes()
        st_two = two.stats()
        assert all(st_two[k] == st_one[k] for k in STAT_KEYS)


def test_batch_across_a_chunk_boundary(gpu_ctx):
    """With 4096 samples a chunk is RT_QUERY_CHUNK / 4096 = 1024 points: 1026 points are two chunks, and the second one's points keep
    the seeds of their places in the caller's array."""
    scene = scenes.single_triangle()
    gpu_ctx.upload_scene(scene)
    samples = api.PATH_MAX_SAMPLES
    chunk = api.QUERY_CHUNK // samples
    assert chunk == 1024
    rng = np.random.default_rng(8)
    normals = rng.standard_normal((chunk + 2, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    points = _make_points(rng.uniform(-1.5, 1.5, (chunk + 2, 3)).astype(F32) + np.array([0, 0, -0.5], F32), normals)
    # the points around the boundary look at the triangle from half a unit away: which of their directions meet it is the seed's doing
    points[1020:, 0:3] = rng.uniform(-0.3, 0.3, (6, 3)).astype(F32) + np.array([0, -0.3, -1.5], F32)
    points[1020:, 4:7] = (0, 0, -1)
    kw = dict(max_bounces=0)
    whole = gpu_ctx.irradiance(points, samples, seed=7, **kw)
    st = gpu_ctx.stats()
    assert st["primary_rays"] == len(points) * samples and st["rays"] == int(api.split_irradiance(whole)[1].astype(np.uint64).sum())
    tail = gpu_ctx.irradiance(np.ascontiguousarray(points[1023:]), samples, seed=7 + 1023, **kw)
    assert len(tail) == 3 and whole[1023:].tobytes() == tail.tobytes()
    other = gpu_ctx.irradiance(np.ascontiguousarray(points[1023:]), samples, seed=7, **kw)
    assert all(other[i].tobytes() != tail[i].tobytes() for i in range(3)), "each of the three has the seed of its own place"
    e = api.split_irradiance(whole)[0]
    assert len(np.unique(_bits(e[:, 1]))) > 256, "the points that face the triangle see it from different places"
    dev = gpu_ctx.irradiance(torch.from_numpy(points).to("cuda:0"), samples, seed=7, **kw)
    assert dev.cpu().numpy().tobytes() == whole.tobytes()


# 3. the tree --------------------------------------------------------------------------------------------------------------------
def test_tree_and_updates(gpu_ctx, box):
    gpu_ctx.upload_scene(box)
    points, _ = _texels(gpu_ctx, box)
    kw = dict(max_bounces=3, seed=SEED, first_sample=1)
    want = gpu_ctx.irradiance(points, 65, **kw)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.stats()["tree_build"] == 0
    assert gpu_ctx.irradiance(points, 65, **kw).tobytes() == want.tobytes()
    gpu_ctx.prepare()  # light grids on the device: never looked at
    assert gpu_ctx.irradiance(points, 65, **kw).tobytes() == want.tobytes()
    # after a vertex update the call walks the refitted tree: the result of a fresh upload of the moved scene
    pos = box.vertices["position"].astype(F32)
    moved_pos = np.ascontiguousarray(pos + F32(0.2) * np.sin(pos[:, ::-1] * F32(3.0)), dtype=F32)
    v = box.vertices.copy()
    v["position"] = moved_pos
    assert gpu_ctx.update_geometry(vertices=moved_pos)["flags"] & (api.STAT_REFIT | api.STAT_REBUILT)
    after = gpu_ctx.irradiance(points, 65, **kw)
    with api.Context() as fresh:
        fresh.upload_scene(dataclasses.replace(box, vertices=v))
        assert fresh.irradiance(points, 65, **kw).tobytes() == after.tobytes()
    assert after.tobytes() != want.tobytes()


# 4. closed forms ----------------------------------------------------------------------------------------------------------------
def _sky_points(n):
    rng = np.random.default_rng(5)
    normals = rng.standard_normal((n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    return _make_points(rng.uniform(-2, 2, (n, 3)).astype(F32), normals)


@pytest.mark.parametrize("samples", [64, 4096])
def test_an_empty_scene_gives_pi_times_the_sky(gpu_ctx, samples):
    gpu_ctx.upload_scene(scenes.empty_scene())
    points = _sky_points(67)
    for seed in (0, 7, 12345, SEED):
        e, segments = api.split_irradiance(gpu_ctx.irradiance(points, samples, seed=seed))
        rel = np.abs(e.astype(np.float64) / (np.pi * SKY.astype(np.float64)) - 1.0).max()
        print(f"sky, seed {seed:#x}, S={samples}: pi sky off by {rel:.3e} (bound {(samples + 4) * 2.0 ** -24:.3e})")
        assert rel <= (samples + 4) * 2.0 ** -24
        assert np.all(segments == samples) and gpu_ctx.stats()["rays"] == len(points) * samples
        # every path is the sky: the statement's reduction of a constant field, whatever the directions
        np.testing.assert_array_equal(_bits(e), _bits(ic.reduce(np.broadcast_to(SKY, (len(points), samples, 3)).copy())))


def test_the_blocked_cap(gpu_ctx):
    """A black sphere of radius 0.6 whose centre stands 1 above the point on its normal, no light, no bounce: a path is the sky or
    nothing, and the cosine-weighted share of the cap is 0.36 (a uniform hemisphere or an unweighted sum gives 0.2, more than 20 sigma
    away).  sigma is that of the fraction of 4096 independent directions, as test_irradiance_cases.py has it for the statement."""
    samples = 4096
    fraction, sigma = ic.blocked_cap_sigma(samples)
    assert fraction == pytest.approx(0.36) and (fraction - 0.2) / sigma > 20.0
    base = scenes.empty_scene()
    black = HP.material_new((0, 0, 0), 0.0, 0.5, (0, 0, 0), 1.5, 0.0)
    scene = dataclasses.replace(base, name="blocked cap", spheres=np.array([((0.0, 0.0, 1.0), 0.6, 0)], dtype=T.SPHERE),
                                materials=np.array([black], dtype=T.MATERIAL))
    assert len(scene.lights) == 0
    gpu_ctx.upload_scene(scene)
    points = _make_points(np.zeros((16, 3)), np.tile(np.array([0, 0, 1], F32), (16, 1)))  # 16 seeds
    e, segments = api.split_irradiance(gpu_ctx.irradiance(points, samples, max_bounces=0, seed=3))
    assert np.all(segments == samples), "one segment per path: no light, no bounce"
    want = np.pi * SKY.astype(np.float64) * (1.0 - fraction)
    off = np.abs(e.astype(np.float64) - want) / (np.pi * SKY.astype(np.float64) * sigma)
    print(f"blocked cap: E / (pi sky) = {(e[0].astype(np.float64) / (np.pi * SKY)).round(4)} at point 0 (0.64 expected, 0.8 unweighted), worst {off.max():.2f} sigma (bound 6)")
    assert off.max() <= 6.0


# 5. edges -----------------------------------------------------------------------------------------------------------------------
def test_the_frame_and_a_running_accumulation_are_left_alone(gpu_ctx, box):
    gpu_ctx.upload_scene(box)
    points, _ = _texels(gpu_ctx, box)
    gpu_ctx.render(64, 48, box.camera, mode=1)
    rgb, comb, hits = gpu_ctx.read_rgb32f(), gpu_ctx.read_rgba8_combined(), gpu_ctx.read_hits()
    gpu_ctx.irradiance(points, 8)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.read_rgba8_combined().tobytes() == comb.tobytes()
    again = gpu_ctx.read_hits()
    assert again[0].tobytes() == hits[0].tobytes() and again[1].tobytes() == hits[1].tobytes()
    gpu_ctx.render(64, 48, box.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    gpu_ctx.irradiance(points, 8, counters=True)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(64, 48, box.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4


def test_the_librarys_own_checks(gpu_ctx, box):
    points = _make_points(np.random.default_rng(4).uniform(-0.9, 0.9, (64, 3)), np.tile(np.array([0, 1, 0], F32), (64, 1)))
    out = np.full((64, 4), 7, F32)
    pp = np.zeros((), T.PATH_PARAMS)
    pp["samples"], pp["max_bounces"] = 4, 2
    lib, h = gpu_ctx.lib, gpu_ctx._h
    call = lambda r, n, a, o: lib.rt_irradiance(h, C.c_void_p(r), C.c_size_t(n), C.c_void_p(a), C.c_void_p(o))
    assert call(points.ctypes.data, 64, pp.ctypes.data, out.ctypes.data) == -4  # before any upload
    assert call(0, 0, 0, 0) == 0  # n == 0 (even then)
    gpu_ctx.upload_scene(box)
    gpu_ctx.render(64, 48, box.camera, mode=1)
    before = gpu_ctx.stats()
    assert call(0, 0, 0, 0) == 0
    assert call(0, 64, pp.ctypes.data, out.ctypes.data) == -1 and "points" in lib.rt_last_error(h).decode()
    assert call(points.ctypes.data, 64, 0, out.ctypes.data) == -1 and "params" in lib.rt_last_error(h).decode()
    assert call(points.ctypes.data, 64, pp.ctypes.data, 0) == -1 and "out" in lib.rt_last_error(h).decode()
    bad = [("samples", 0), ("samples", api.PATH_MAX_SAMPLES + 1), ("max_bounces", api.MAX_BOUNCES + 1), ("first_sample", 0xFFFFFFFF),
           ("flags", api.PATH_CAMERA_DRAWS), ("flags", api.PATH_CAMERA_DRAWS | api.PATH_NO_SHADOWS), ("flags", 2), ("flags", 4), ("flags", 16), ("flags", 128),
           ("flags", 1 << 31)]
    assert api.MAX_BOUNCES + 1 == 256 and api.PATH_MAX_SAMPLES + 1 == 4097
    for field, value in bad:
        p = pp.copy()
        p[field] = value
        if field == "first_sample":
            p["samples"] = 2  # 2^32 - 1 + 2
        assert call(points.ctypes.data, 64, p.ctypes.data, out.ctypes.data) == -1, (field, value)
        assert field in lib.rt_last_error(h).decode() or field == "flags"
        if value == api.PATH_CAMERA_DRAWS:
            assert "RT_PATH_CAMERA_DRAWS" in lib.rt_last_error(h).decode()
    assert np.all(out == 7) and gpu_ctx.stats() == before, "a rejected call changes nothing"
    p = pp.copy()
    p["first_sample"], p["samples"] = (1 << 32) - 2, 2  # the last two samples there are
    assert call(points.ctypes.data, 64, p.ctypes.data, out.ctypes.data) == 0
    assert gpu_ctx.stats()["primary_rays"] == 128 and np.all(_bits(out[:, 3]) >= 2)
    p = pp.copy()
    p["_pad"] = 0xDEADBEEF  # ignored
    padded = np.full((64, 4), 7, F32)
    assert call(points.ctypes.data, 64, p.ctypes.data, padded.ctypes.data) == 0
    assert call(points.ctypes.data, 64, pp.ctypes.data, out.ctypes.data) == 0 and out.tobytes() == padded.tobytes()
    # prim_id and material_id are ignored
    tagged = points.copy()
    tagged.view(U32)[:, 3], tagged.view(U32)[:, 7] = 0xDEADBEEF, api.PRIM_MISS
    assert gpu_ctx.irradiance(tagged, 4, max_bounces=2).tobytes() == out.tobytes()
    # counters change no byte
    st = gpu_ctx.stats()
    assert st["node_visits"] == 0 and st["tri_tests"] == 0
    counted = gpu_ctx.irradiance(points, 4, max_bounces=2, counters=True)
    st = gpu_ctx.stats()
    assert st["node_visits"] > 0 and st["tri_tests"] > 0 and counted.tobytes() == out.tobytes()
    # a misaligned device pointer and mixed kinds are rejected, device memory gives the host's bytes
    dev = torch.from_numpy(points).to("cuda:0")
    skew = torch.zeros(64 * 8 + 4, device="cuda:0")[1:1 + 64 * 8].view(-1, 8)
    with pytest.raises(api.RtError) as e:
        gpu_ctx.irradiance(skew, 4)
    assert e.value.code == -1 and "aligned" in str(e.value)
    host = np.full((64, 4), 7, F32)
    assert call(dev.data_ptr(), 64, pp.ctypes.data, host.ctypes.data) == -1 and np.all(host == 7)  # device points, host out
    dev_out = torch.full((64, 4), 7.0, device="cuda:0")
    assert call(points.ctypes.data, 64, pp.ctypes.data, dev_out.data_ptr()) == -1 and bool((dev_out == 7).all())  # host points, device out
    assert gpu_ctx.irradiance(dev, 4, max_bounces=2).cpu().numpy().tobytes() == out.tobytes()
    # 33 lights: more than the extended mode's pipeline takes, and no limit here
    gpu_ctx.upload_scene(dataclasses.replace(box, lights=np.repeat(box.lights, 33)))
    e33, _ = api.split_irradiance(gpu_ctx.irradiance(points, 4, max_bounces=0, seed=SEED))
    assert gpu_ctx.stats()["shadow_rays"] > 33 and np.isfinite(e33).all()
