"""Probe queries on the MI355X (rt_radiance_sh), held to the calls below it.

Composition: every coefficient is, bit for bit, the ordered f32 projection (radiance_sh_cases.py) of what rt_radiance gives along
the directions the statement draws, with RT_PATH_CAMERA_DRAWS, sample by sample; the segments and the statistics are the sums.
Against itself: the kind of memory, the chunking, the device count and the tree change no byte.  Against closed forms: a constant
field (the sky of an empty scene, the inside of an emissive sphere) lands on sh[0] within the bounds of the CPU test."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import radiance_sh_cases as rc
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import hostpack as HP
from gpu_raytracer_amd import types as T

import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first; the device-memory cases need it

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
SEED = 0xFFFFFFF0  # the per-probe seed wraps at probe 16
SKY = np.array([0.1, 0.2, 0.3], F32)
N_PROBES = 67
W, H = 64, 48
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


def _lattice():
    """67 probes on a lattice through and around the box: the outer planes lie outside the walls and in front of the open side, and
    probe 10 sits at the centre of the sphere."""
    x, y, z = np.meshgrid(np.linspace(-1.15, 1.15, 5), np.linspace(-0.9, 0.9, 4), np.linspace(-0.8, 1.6, 4), indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)[np.linspace(0, 79, N_PROBES).astype(np.int64)].astype(F32)
    p[10] = (0.3, -0.55, 0.1)
    return api.make_probes(p)


@pytest.fixture(scope="module")
def box():
    return _box_scene()


def compose(ctx, oracle_mod, probes, index, samples, seed, first_sample, max_bounces, shadows):
    """The statement through Context.radiance: one call per sample over the rays (P_i, d_{i,k}) -> (sh, segments, summed statistics).
    `index`: the probes' indices in the caller's array; the rays' own indices must be those, so it has to be 0 .. n-1."""
    assert np.array_equal(index, np.arange(len(probes)))
    d = rc.directions(oracle_mod, index, samples, seed, first_sample)
    x = np.zeros((len(probes), samples, 3), F32)
    segments = np.zeros(len(probes), U32)
    totals = dict.fromkeys(STAT_KEYS, 0)
    for k in range(samples):
        rays = api.make_rays(probes[:, 0:3], d[:, k], rc.MIN_T, rc.F32_MAX)
        radiance, g = api.split_radiance(ctx.radiance(rays, samples=1, max_bounces=max_bounces, seed=seed, first_sample=first_sample + k,
                                                      shadows=shadows, camera_draws=True))
        st = ctx.stats()
        for key in STAT_KEYS:
            totals[key] += st[key]
        x[:, k] = radiance
        segments = segments + g
    return rc.project(x, d), segments, totals


# 1. composition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 3, 64, 65])  # a wave holds 64, 21 1/3, 1 and less than one probe
def test_is_the_ordered_projection_of_rt_radiance_bit_for_bit(gpu_ctx, oracle_mod, box, samples):
    gpu_ctx.upload_scene(box)
    probes = _lattice()
    inside = np.abs(probes[:, 0:3]).max(1) < 1.0
    assert 10 < inside.sum() < N_PROBES - 10, "probes inside and outside the room"
    index = np.arange(N_PROBES)
    for bounces in (0, 3):
        for shadows in (True, False):
            for first in (0, 5):
                want, want_segments, totals = compose(gpu_ctx, oracle_mod, probes, index, samples, SEED, first, bounces, shadows)
                got = gpu_ctx.radiance_sh(probes, samples, max_bounces=bounces, seed=SEED, first_sample=first, shadows=shadows)
                st = gpu_ctx.stats()
                sh, segments = api.split_sh(got)
                label = f"S={samples} max_bounces={bounces} shadows={shadows} first_sample={first}"
                print(label, {k: st[k] for k in STAT_KEYS})
                np.testing.assert_array_equal(_bits(sh), _bits(want), err_msg=label)
                np.testing.assert_array_equal(segments, want_segments, err_msg=label)
                assert all(st[k] == totals[k] for k in STAT_KEYS), (label, st, totals)
                assert st["primary_rays"] == N_PROBES * samples and st["pixels"] == 0 and st["kernel_ms"] > 0
                assert st["rays"] == int(segments.astype(np.uint64).sum()) and st["node_visits"] == 0 and st["tri_tests"] == 0
                assert (st["shadow_rays"] > 0) == shadows and (st["continuation_rays"] > 0) == (bounces > 0)
                # (radiance is a sum of non-negative terms, and Y0 is positive; the probes see different things)
                assert np.isfinite(sh).all() and (sh[:, 0, :] >= 0).all() and len(np.unique(_bits(sh[:, 0, 0]))) > 1


# 2. memory, chunks, devices -----------------------------------------------------------------------------------------------------
def test_memory_kinds_and_devices(gpu_ctx, box):
    gpu_ctx.upload_scene(box)
    probes = _lattice()
    kw = dict(max_bounces=3, seed=SEED, first_sample=3)
    want = gpu_ctx.radiance_sh(probes, 65, **kw)
    st_one = gpu_ctx.stats()
    own = np.full((N_PROBES, 28), 7, F32)
    assert gpu_ctx.radiance_sh(probes, 65, out=own, **kw) is own and own.tobytes() == want.tobytes()
    dev = torch.from_numpy(probes).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    got = gpu_ctx.radiance_sh(dev, 65, **kw)
    assert got.device == dev.device and got.dtype == torch.float32 and tuple(got.shape) == (N_PROBES, 28)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert gpu_ctx.radiance_sh(torch.from_numpy(probes.copy()), 65, **kw).numpy().tobytes() == want.tobytes()
    np.testing.assert_array_equal(api.split_sh(got)[1].cpu().numpy(), api.split_sh(want)[1].astype(np.int64))
    with api.Context((0, 0)) as two:  # each device gets a contiguous range of the probes; the seed's index stays the caller's
        two.upload_scene(box)
        assert two.radiance_sh(probes, 65, **kw).tobytes() == want.tobytes()
        st_two = two.stats()
        assert all(st_two[k] == st_one[k] for k in STAT_KEYS)


def test_batch_across_a_chunk_boundary(gpu_ctx):
    """With 4096 samples a chunk is RT_QUERY_CHUNK / 4096 = 1024 probes: 1026 probes are two chunks, and the second one's probes keep
    the seeds of their places in the caller's array."""
    scene = scenes.single_triangle()
    gpu_ctx.upload_scene(scene)
    samples = api.PATH_MAX_SAMPLES
    chunk = api.QUERY_CHUNK // samples
    assert chunk == 1024
    rng = np.random.default_rng(8)
    probes = api.make_probes(rng.uniform(-1.5, 1.5, (chunk + 2, 3)).astype(F32) + np.array([0, 0, -0.5], F32))
    kw = dict(max_bounces=0)
    whole = gpu_ctx.radiance_sh(probes, samples, seed=7, **kw)
    st = gpu_ctx.stats()
    assert st["primary_rays"] == len(probes) * samples and st["rays"] == int(api.split_sh(whole)[1].astype(np.uint64).sum())
    tail = gpu_ctx.radiance_sh(np.ascontiguousarray(probes[1020:]), samples, seed=7 + 1020, **kw)
    assert whole[1020:].tobytes() == tail.tobytes()
    assert gpu_ctx.radiance_sh(np.ascontiguousarray(probes[1020:]), samples, seed=7, **kw).tobytes() != tail.tobytes()
    sh = api.split_sh(whole)[0]
    assert len(np.unique(_bits(sh[:, 1, 0]))) > 1000, "the probes see the triangle from different places"
    dev = gpu_ctx.radiance_sh(torch.from_numpy(probes).to("cuda:0"), samples, seed=7, **kw)
    assert dev.cpu().numpy().tobytes() == whole.tobytes()
    with api.Context((0, 0)) as two:
        two.upload_scene(scene)
        assert two.radiance_sh(probes, samples, seed=7, **kw).tobytes() == whole.tobytes()


# 3. the tree --------------------------------------------------------------------------------------------------------------------
def test_tree_and_updates(gpu_ctx, box):
    gpu_ctx.upload_scene(box)
    probes = _lattice()
    kw = dict(max_bounces=3, seed=SEED, first_sample=1)
    want = gpu_ctx.radiance_sh(probes, 65, **kw)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.stats()["tree_build"] == 0
    assert gpu_ctx.radiance_sh(probes, 65, **kw).tobytes() == want.tobytes()
    gpu_ctx.prepare()  # light grids on the device: never looked at
    assert gpu_ctx.radiance_sh(probes, 65, **kw).tobytes() == want.tobytes()
    # after a vertex update the call walks the refitted tree: the result of a fresh upload of the moved scene
    pos = box.vertices["position"].astype(F32)
    moved_pos = np.ascontiguousarray(pos + F32(0.2) * np.sin(pos[:, ::-1] * F32(3.0)), dtype=F32)
    v = box.vertices.copy()
    v["position"] = moved_pos
    assert gpu_ctx.update_geometry(vertices=moved_pos)["flags"] & (api.STAT_REFIT | api.STAT_REBUILT)
    after = gpu_ctx.radiance_sh(probes, 65, **kw)
    with api.Context() as fresh:
        fresh.upload_scene(dataclasses.replace(box, vertices=v))
        assert fresh.radiance_sh(probes, 65, **kw).tobytes() == after.tobytes()
    assert after.tobytes() != want.tobytes()


# 4. closed forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [64, 256, 1024, 4096])
def test_an_empty_scene_gives_the_sky(gpu_ctx, oracle_mod, samples):
    gpu_ctx.upload_scene(scenes.empty_scene())
    probes = _lattice()
    for seed in (0, 7, 12345, SEED):
        sh, segments = api.split_sh(gpu_ctx.radiance_sh(probes, samples, seed=seed))
        rc.check_constant_field(sh, samples, SKY, label=f"sky, seed {seed:#x}")
        assert np.all(segments == samples) and gpu_ctx.stats()["rays"] == N_PROBES * samples
        np.testing.assert_array_equal(_bits(sh), _bits(rc.constant_field(oracle_mod, N_PROBES, samples, seed, SKY)))


def test_inside_an_emissive_sphere(gpu_ctx):
    """A probe at the centre of a large sphere that only emits: every path is E, so the field is the constant E."""
    emission = np.array([0.5, 1.5, 0.25], F32)
    samples = 1024
    base = scenes.empty_scene()
    scene = dataclasses.replace(base, name="emissive sphere", spheres=np.array([((0.5, -0.25, 1.0), 50.0, 0)], dtype=T.SPHERE),
                                materials=np.array([HP.material_new((0, 0, 0), 0.0, 0.5, tuple(emission), 1.5, 0.0)], dtype=T.MATERIAL))
    gpu_ctx.upload_scene(scene)
    probes = api.make_probes(np.tile(np.array([[0.5, -0.25, 1.0]], F32), (N_PROBES, 1)))
    sh, segments = api.split_sh(gpu_ctx.radiance_sh(probes, samples, max_bounces=0, seed=SEED))
    rc.check_constant_field(sh, samples, emission, label="emissive sphere")
    assert np.all(segments == samples), "one segment per path: no light, no bounce"
    normals = np.concatenate([np.eye(3), -np.eye(3)]).astype(F32)
    tolerance = 6.0 * emission.astype(np.float64) * np.sqrt(4.0 * np.pi / samples) * np.pi * 0.2820948
    worst = 0.0
    for i in range(N_PROBES):
        e = api.sh9_irradiance(np.repeat(sh[i:i + 1], len(normals), 0), normals).astype(np.float64)
        off = np.abs(e - np.pi * emission.astype(np.float64)) / tolerance
        worst = max(worst, off.max())
    print(f"irradiance inside the emissive sphere: worst deviation from pi E is {worst:.3f} of the tolerance")
    assert worst <= 1.0


# 5. edges -----------------------------------------------------------------------------------------------------------------------
def test_edges(gpu_ctx, box):
    gpu_ctx.upload_scene(box)
    probes = _lattice()
    assert gpu_ctx.radiance_sh(np.zeros((0, 4), F32), 16).shape == (0, 28)
    whole = gpu_ctx.radiance_sh(probes, 3, seed=SEED)
    for n in (1, 21, 22, 63, 64, 65):  # 3 n around the wave's 64 lanes
        assert gpu_ctx.radiance_sh(np.ascontiguousarray(probes[:n]), 3, seed=SEED).tobytes() == whole[:n].tobytes()
    # the pad word is ignored
    padded = probes.copy()
    padded.view(U32)[:, 3] = 0xDEADBEEF
    assert gpu_ctx.radiance_sh(padded, 3, seed=SEED).tobytes() == whole.tobytes()
    # probes that are no probes: zeros, no segment, nothing traced; the others keep their bits (their seeds are their indices')
    kw = dict(max_bounces=2, seed=SEED)
    plain = gpu_ctx.radiance_sh(probes, 16, **kw)
    st_plain = gpu_ctx.stats()
    odd = probes.copy()
    bad = np.array([0, 13, 40, 66])
    odd[0, 0], odd[13, 1], odd[40, 2], odd[66, 0:3] = np.nan, np.inf, -np.inf, np.nan
    got = gpu_ctx.radiance_sh(odd, 16, **kw)
    st = gpu_ctx.stats()
    good = np.setdiff1d(np.arange(N_PROBES), bad)
    assert not _bits(got[bad]).any() and got[good].tobytes() == plain[good].tobytes()
    assert st["primary_rays"] == len(good) * 16 and st["rays"] == int(api.split_sh(got)[1].astype(np.uint64).sum()) < st_plain["rays"]
    # counters change no byte
    assert st["node_visits"] == 0 and st["tri_tests"] == 0
    counted = gpu_ctx.radiance_sh(probes, 16, counters=True, **kw)
    st = gpu_ctx.stats()
    assert st["node_visits"] > 0 and st["tri_tests"] > 0 and counted.tobytes() == plain.tobytes()
    # 33 lights: more than the extended mode's pipeline takes, and no limit here
    many = dataclasses.replace(box, lights=np.repeat(box.lights, 33))
    gpu_ctx.upload_scene(many)
    sh, segments = api.split_sh(gpu_ctx.radiance_sh(probes, 4, max_bounces=0, seed=SEED))
    assert gpu_ctx.stats()["shadow_rays"] > 33 and np.isfinite(sh).all()


def test_the_frame_and_a_running_accumulation_are_left_alone(gpu_ctx, box):
    gpu_ctx.upload_scene(box)
    probes = _lattice()
    gpu_ctx.render(W, H, box.camera, mode=1)
    rgb, comb, hits = gpu_ctx.read_rgb32f(), gpu_ctx.read_rgba8_combined(), gpu_ctx.read_hits()
    gpu_ctx.radiance_sh(probes, 8)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.read_rgba8_combined().tobytes() == comb.tobytes()
    again = gpu_ctx.read_hits()
    assert again[0].tobytes() == hits[0].tobytes() and again[1].tobytes() == hits[1].tobytes()
    gpu_ctx.render(W, H, box.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    gpu_ctx.radiance_sh(probes, 8, counters=True)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(W, H, box.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4


def test_the_librarys_own_checks(gpu_ctx, box):
    probes, out = _lattice()[:64].copy(), np.full((64, 28), 7, F32)
    pp = np.zeros((), T.PATH_PARAMS)
    pp["samples"], pp["max_bounces"] = 4, 2
    lib, h = gpu_ctx.lib, gpu_ctx._h
    call = lambda r, n, a, o: lib.rt_radiance_sh(h, C.c_void_p(r), C.c_size_t(n), C.c_void_p(a), C.c_void_p(o))
    assert call(probes.ctypes.data, 64, pp.ctypes.data, out.ctypes.data) == -4  # before any upload
    assert call(0, 0, 0, 0) == 0  # n == 0 (even then)
    gpu_ctx.upload_scene(box)
    gpu_ctx.render(W, H, box.camera, mode=1)
    before = gpu_ctx.stats()
    assert call(0, 0, 0, 0) == 0
    assert call(0, 64, pp.ctypes.data, out.ctypes.data) == -1 and "probes" in lib.rt_last_error(h).decode()
    assert call(probes.ctypes.data, 64, 0, out.ctypes.data) == -1 and "params" in lib.rt_last_error(h).decode()
    assert call(probes.ctypes.data, 64, pp.ctypes.data, 0) == -1 and "out" in lib.rt_last_error(h).decode()
    bad = [("samples", 0), ("samples", api.PATH_MAX_SAMPLES + 1), ("max_bounces", api.MAX_BOUNCES + 1), ("first_sample", 0xFFFFFFFF),
           ("flags", api.PATH_CAMERA_DRAWS), ("flags", api.PATH_CAMERA_DRAWS | api.PATH_NO_SHADOWS), ("flags", 2), ("flags", 4), ("flags", 16), ("flags", 128),
           ("flags", 1 << 31)]
    assert api.MAX_BOUNCES + 1 == 256 and api.PATH_MAX_SAMPLES + 1 == 4097
    for field, value in bad:
        p = pp.copy()
        p[field] = value
        if field == "first_sample":
            p["samples"] = 2  # 2^32 - 1 + 2
        assert call(probes.ctypes.data, 64, p.ctypes.data, out.ctypes.data) == -1, (field, value)
        assert field in lib.rt_last_error(h).decode() or field == "flags"
        if value == api.PATH_CAMERA_DRAWS:
            assert "RT_PATH_CAMERA_DRAWS" in lib.rt_last_error(h).decode()
    assert np.all(out == 7) and gpu_ctx.stats() == before, "a rejected call changes nothing"
    p = pp.copy()
    p["first_sample"], p["samples"] = (1 << 32) - 2, 2  # the last two samples there are
    assert call(probes.ctypes.data, 64, p.ctypes.data, out.ctypes.data) == 0
    assert gpu_ctx.stats()["primary_rays"] == 128 and np.all(_bits(out[:, 27]) >= 2)
    assert call(probes.ctypes.data, 64, pp.ctypes.data, out.ctypes.data) == 0
    # as rt_radiance: a misaligned device pointer and mixed kinds are rejected, device memory gives the host's bytes
    dev = torch.from_numpy(probes).to("cuda:0")
    skew = torch.zeros(64 * 4 + 4, device="cuda:0")[1:1 + 64 * 4].view(-1, 4)
    with pytest.raises(api.RtError) as e:
        gpu_ctx.radiance_sh(skew, 4)
    assert e.value.code == -1 and "aligned" in str(e.value)
    with pytest.raises(api.RtError) as e:
        gpu_ctx.radiance(torch.zeros(64 * 8 + 4, device="cuda:0")[1:1 + 64 * 8].view(-1, 8))
    assert e.value.code == -1 and "aligned" in str(e.value)
    host = np.full((64, 28), 7, F32)
    assert call(dev.data_ptr(), 64, pp.ctypes.data, host.ctypes.data) == -1 and np.all(host == 7)  # device probes, host out
    assert gpu_ctx.radiance_sh(dev, 4, max_bounces=2).cpu().numpy().tobytes() == out.tobytes()
