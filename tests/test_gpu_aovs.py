"""First-hit feature buffers (rt_aovs) and the frames' per-sample camera rays (rt_sample_rays) on the MI355X.

Every sample of mode 2 is recomputed with rt_sample_rays + rt_intersect (the frames' closest hit, bit for bit: test_gpu_ray_queries)
and reduced here in float32 in sample order, so albedo, depth and coverage must match bit for bit; the normal is recomputed from the
scene's vertices and spheres in numpy and must match within 1e-6."""
import ctypes as C

import numpy as np
import pytest

from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
MISS = 0xFFFFFFFF
SKY = np.array([0.1, 0.2, 0.3], F32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_bits(a, b, what):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _normalize(a):
    with np.errstate(all="ignore"):
        length = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]).astype(F32)
        return a * (F32(1.0) / length)[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2],
                     a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def _surface(scene, rays, t, prim):
    """Per ray: hit mask, albedo (the frame's colour of a miss left to the caller), face-forwarded geometric normal."""
    n = len(rays)
    hit = prim != MISS
    sphere = hit & (prim >= 0x80000000)
    tri = hit & ~sphere
    normal = np.zeros((n, 3), F32)
    mid = np.zeros(n, np.int64)
    pos = scene.vertices["position"].astype(F32)
    if tri.any():
        trs = scene.triangles[prim[tri].astype(np.int64)]
        v0 = pos[trs["v0_index"]]
        normal[tri] = _normalize(_cross(pos[trs["v1_index"]] - v0, pos[trs["v2_index"]] - v0))
        mid[tri] = trs["material_id"]
    if sphere.any():
        sp = scene.spheres[(prim[sphere] & 0x7FFFFFFF).astype(np.int64)]
        point = rays[sphere, 0:3] + rays[sphere, 4:7] * t[sphere, None]
        normal[sphere] = _normalize(point - sp["center"].astype(F32))
        mid[sphere] = sp["material_id"]
    d = rays[:, 4:7]
    front = ((d[:, 0] * normal[:, 0] + d[:, 1] * normal[:, 1]) + d[:, 2] * normal[:, 2]) < 0
    nf = np.where(front[:, None], normal, -normal)
    albedo = np.zeros((n, 3), F32)
    valid = mid < len(scene.materials)
    albedo[hit & valid] = scene.materials["albedo"][mid[hit & valid]].astype(F32)
    albedo[hit & ~valid] = [1, 0, 1]
    return hit, albedo, nf


def expected_aovs(ctx, scene, w, h, spp, **kw):
    """The mode-2 AOVs of a frame, recomputed sample by sample: rt_sample_rays + rt_intersect, float32 sums in sample order."""
    a_sum = np.zeros((w * h, 3), F32)
    n_sum = np.zeros((w * h, 3), F32)
    t_sum = np.zeros(w * h, F32)
    hits = np.zeros(w * h, F32)
    for s in range(spp):
        rays = ctx.sample_rays(w, h, scene.camera, s, spp=spp, **kw)
        t, _, _, prim = api.split_hits(ctx.intersect(rays))
        hit, albedo, nf = _surface(scene, rays, t, prim)
        albedo[~hit] = SKY
        a_sum = a_sum + albedo
        n_sum = n_sum + np.where(hit[:, None], nf, F32(0))
        t_sum = t_sum + np.where(hit, t, F32(0))
        hits = hits + hit.astype(F32)
    n = F32(spp)
    with np.errstate(all="ignore"):
        depth = np.where(hits > 0, t_sum / hits, F32(0)).astype(F32)
    return a_sum / n, depth, n_sum / n, hits / n


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(2000, n_spheres=3)


def _scene(name, soup):
    return soup if name == "soup" else scenes.SCENES[name]()


# modes 0 / 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["cornell12", "soup", "bad_material"])
def test_modes_0_1_against_the_frame(gpu_ctx, soup, name, mode):
    if name == "bad_material":  # a third of the triangles point past the material table: magenta, as the frame gives
        scene = scenes.random_soup(600, n_spheres=2, seed=4)
        scene.triangles["material_id"][::3] = 1000
    else:
        scene = _scene(name, soup)
    w, h = 96, 64
    gpu_ctx.upload_scene(scene)
    gpu_ctx.render(w, h, scene.camera, mode=mode)
    prim, t = gpu_ctx.read_hits()
    rgb = gpu_ctx.read_rgb32f()
    a = gpu_ctx.aovs(w, h, scene.camera, mode=mode, spp=7)  # spp is ignored in modes 0/1
    st = gpu_ctx.stats()
    assert st["pixels"] == w * h and st["rays"] == st["primary_rays"] == w * h and st["kernel_ms"] > 0
    s = api.split_aovs(a)
    hit = prim != MISS
    assert hit.any() and (~hit).any()
    _assert_bits(s["depth"][hit], t[hit], "depth == read_hits t")
    assert np.all(s["depth"][~hit] == 0)
    np.testing.assert_array_equal(s["coverage"], hit.astype(F32))
    rays = gpu_ctx.camera_rays(w, h, scene.camera, mode=mode)
    _, albedo, nf = _surface(scene, rays, t.reshape(-1), prim.reshape(-1))
    albedo[~hit.reshape(-1)] = SKY if mode == 1 else 0
    _assert_bits(s["albedo"].reshape(-1, 3), albedo, "albedo == material table")
    np.testing.assert_allclose(s["normal"].reshape(-1, 3), nf * hit.reshape(-1, 1), rtol=0, atol=1e-6)
    if name == "bad_material":
        assert np.any(np.all(s["albedo"] == [1, 0, 1], -1))
    _assert_bits(gpu_ctx.read_rgb32f(), rgb, "rt_aovs leaves the frame alone")


# mode 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [1, 5])
@pytest.mark.parametrize("name", ["cornell12", "soup"])
def test_mode_2_against_sample_rays_and_intersect(gpu_ctx, soup, name, spp):
    scene = _scene(name, soup)
    w, h = 80, 56
    gpu_ctx.upload_scene(scene)
    a = gpu_ctx.aovs(w, h, scene.camera, mode=2, spp=spp, frame_seed=17, max_bounces=3)
    st = gpu_ctx.stats()
    assert st["pixels"] == w * h and st["rays"] == st["primary_rays"] == w * h * spp
    assert st["continuation_rays"] == st["shadow_rays"] == 0
    albedo, depth, normal, coverage = expected_aovs(gpu_ctx, scene, w, h, spp, frame_seed=17)
    s = api.split_aovs(a.reshape(-1, 8))
    _assert_bits(s["albedo"], albedo, "albedo")
    _assert_bits(s["coverage"], coverage, "coverage")
    _assert_bits(s["depth"], depth, "depth")
    np.testing.assert_allclose(s["normal"], normal, rtol=0, atol=1e-6)
    assert coverage.mean() > 0


def test_many_samples_span_several_launches(gpu_ctx):
    """More samples than one launch traces: the partial sums carried between launches give the per-sample reduction."""
    scene = scenes.cornell12()
    w, h, spp = 24, 16, api.AOV_SAMPLES_PER_LAUNCH + 9
    gpu_ctx.upload_scene(scene)
    a = gpu_ctx.aovs(w, h, scene.camera, mode=2, spp=spp, frame_seed=3)
    albedo, depth, _, coverage = expected_aovs(gpu_ctx, scene, w, h, spp, frame_seed=3)
    s = api.split_aovs(a.reshape(-1, 8))
    _assert_bits(s["albedo"], albedo, "albedo")
    _assert_bits(s["depth"], depth, "depth")
    _assert_bits(s["coverage"], coverage, "coverage")


def test_sample_rays_closed_1spp_equal_camera_rays_mode_1(gpu_ctx):
    scene = scenes.cornell12()
    w, h = 64, 40
    r = gpu_ctx.sample_rays(w, h, scene.camera, 0, spp=1)
    _assert_bits(r, gpu_ctx.camera_rays(w, h, scene.camera, mode=1), "closed 1 spp == rt_camera_rays(mode 1)")
    rj = gpu_ctx.sample_rays(w, h, scene.camera, 0, spp=1, accumulate=True)
    assert np.all(rj[:, 3] == T.MIN_RAY_DISTANCE) and np.all(rj[:, 7] == np.finfo(F32).max)
    assert not np.array_equal(_bits(rj), _bits(r)), "an accumulation jitters every sample"
    _assert_bits(rj, gpu_ctx.sample_rays(w, h, scene.camera, 0, spp=2), "jitter: accumulate == spp > 1")
    assert not np.array_equal(_bits(rj), _bits(gpu_ctx.sample_rays(w, h, scene.camera, 1, spp=2)))


def test_sample_rays_argument_errors_and_no_scene(rt_api):
    with rt_api.Context() as ctx:  # no scene: rt_sample_rays needs none
        cam = scenes.cornell12().camera
        assert ctx.sample_rays(8, 4, cam, 3, spp=4).shape == (32, 8)
        for kw in (dict(mode=0), dict(mode=1), dict(spp=0), dict(max_bounces=256)):
            with pytest.raises(api.RtError) as e:
                ctx.sample_rays(8, 4, cam, 0, **kw)
            assert e.value.code == -1, kw
        assert ctx.sample_rays(8, 4, cam, 0, tile_rank=5, tile_world=2).shape == (32, 8)  # the tile fields are ignored


# invariance ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inv_scene():
    return scenes.random_soup(3000, n_spheres=3, seed=9)


INV = dict(mode=2, spp=3, frame_seed=5)
W, H = 150, 90


@pytest.fixture(scope="module")
def inv_ref(rt_api, inv_scene):
    with rt_api.Context() as ctx:
        ctx.upload_scene(inv_scene)
        return ctx.aovs(W, H, inv_scene.camera, **INV)


def test_tile_size_does_not_matter(gpu_ctx, inv_scene, inv_ref):
    gpu_ctx.upload_scene(inv_scene)
    for ts in (8, 128):
        _assert_bits(gpu_ctx.aovs(W, H, inv_scene.camera, tile_size=ts, **INV), inv_ref, f"tile_size {ts}")


def test_tile_shares_union(gpu_ctx, inv_scene, inv_ref):
    gpu_ctx.upload_scene(inv_scene)
    union = np.zeros_like(inv_ref)
    covered = np.zeros((H, W), bool)
    for rank in range(3):
        a = gpu_ctx.aovs(W, H, inv_scene.camera, tile_size=32, tile_rank=rank, tile_world=3, **INV)
        mine = np.zeros((H, W), bool)
        tiles_x = (W + 31) // 32
        for ty in range((H + 31) // 32):
            for tx in range(tiles_x):
                if (ty * tiles_x + tx) % 3 == rank:
                    mine[ty * 32:(ty + 1) * 32, tx * 32:(tx + 1) * 32] = True
        assert np.all(a[~mine] == 0), "zeros outside the share"
        assert not np.any(covered & mine)
        covered |= mine
        union[mine] = a[mine]
    assert covered.all()
    _assert_bits(union, inv_ref, "union of the shares")


def test_two_device_context(rt_api, inv_scene, inv_ref):
    with rt_api.Context((0, 0)) as ctx:
        ctx.upload_scene(inv_scene)
        _assert_bits(ctx.aovs(W, H, inv_scene.camera, tile_size=32, **INV), inv_ref, "devices (0, 0)")
        assert ctx.stats()["pixels"] == W * H


def test_quality_tree(gpu_ctx, inv_scene, inv_ref):
    gpu_ctx.upload_scene(inv_scene)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    _assert_bits(gpu_ctx.aovs(W, H, inv_scene.camera, **INV), inv_ref, "RT_PREPARE_QUALITY_TREE")


@pytest.mark.skipif(torch is None, reason="torch is not installed")
def test_host_and_torch_device_output(gpu_ctx, inv_scene, inv_ref):
    gpu_ctx.upload_scene(inv_scene)
    out = torch.full((H, W, 8), float("nan"), device="cuda:0")
    got = gpu_ctx.aovs(W, H, inv_scene.camera, out=out, **INV)
    assert got is out
    _assert_bits(out.cpu().numpy(), inv_ref, "torch device output")
    cpu = torch.empty((H, W, 8))
    _assert_bits(gpu_ctx.aovs(W, H, inv_scene.camera, out=cpu, **INV).numpy(), inv_ref, "torch CPU output")
    share = torch.full((H, W, 8), float("nan"), device="cuda:0")
    a = gpu_ctx.aovs(W, H, inv_scene.camera, out=share, tile_size=32, tile_rank=1, tile_world=2, **INV).cpu().numpy()
    _assert_bits(a, gpu_ctx.aovs(W, H, inv_scene.camera, tile_size=32, tile_rank=1, tile_world=2, **INV), "device share, zeros outside")


# accumulation ----------------------------------------------------------------------------------------------------------------
def test_accumulation_survives_and_aovs_match_its_samples(gpu_ctx):
    scene = scenes.cornell12()
    w, h = 64, 48
    kw = dict(mode=2, max_bounces=2, frame_seed=11)
    gpu_ctx.upload_scene(scene)
    gpu_ctx.render(w, h, scene.camera, spp=4, **kw)
    closed = gpu_ctx.read_rgb32f()
    gpu_ctx.render(w, h, scene.camera, spp=2, accumulate=True, restart=True, **kw)
    before = gpu_ctx.read_rgb32f()
    a2 = gpu_ctx.aovs(w, h, scene.camera, spp=gpu_ctx.accumulated_samples(), accumulate=True, **kw)
    _assert_bits(gpu_ctx.read_rgb32f(), before, "rt_read_rgb32f unchanged by rt_aovs")
    assert gpu_ctx.accumulated_samples() == 2
    gpu_ctx.render(w, h, scene.camera, spp=2, accumulate=True, **kw)
    assert gpu_ctx.accumulated_samples() == 4
    _assert_bits(gpu_ctx.read_rgb32f(), closed, "2 + 2 accumulated samples == a closed 4-spp frame")
    a4 = gpu_ctx.aovs(w, h, scene.camera, spp=4, accumulate=True, **kw)
    _assert_bits(a4, gpu_ctx.aovs(w, h, scene.camera, spp=4, **kw), "the AOVs of 4 accumulated samples == of a closed 4-spp frame")
    albedo, depth, _, coverage = expected_aovs(gpu_ctx, scene, w, h, 2, accumulate=True, frame_seed=11)
    _assert_bits(api.split_aovs(a2.reshape(-1, 8))["depth"], depth, "accumulated 2 samples: depth")
    _assert_bits(api.split_aovs(a2.reshape(-1, 8))["albedo"], albedo, "accumulated 2 samples: albedo")


# errors ----------------------------------------------------------------------------------------------------------------------
def _raw(ctx, fn, p, out):
    return getattr(ctx.lib, fn)(ctx._h, C.c_void_p(p.ctypes.data), C.c_void_p(out.ctypes.data))


def test_errors(rt_api):
    scene = scenes.cornell12()
    with rt_api.Context() as ctx:
        with pytest.raises(api.RtError) as e:
            ctx.aovs(8, 8, scene.camera)
        assert e.value.code == -4, "RT_ERR_NOT_UPLOADED before an upload"
        ctx.upload_scene(scene)
        out = np.full((64, 64, 8), 7.0, np.float32)
        bad = [dict(width=0), dict(height=0), dict(width=65535 * 8 + 1), dict(mode=3), dict(flags=api.FLAG_ACCUMULATE_RESTART),
               dict(flags=api.FLAG_ACCUMULATE, mode=0), dict(spp=0), dict(spp=65537), dict(max_bounces=256), dict(tile_rank=2, tile_world=2),
               dict(tile_size=4097)]
        for b in bad:
            p = api.render_params(64, 64, scene.camera, mode=2, spp=2)
            for k, v in b.items():
                p[k] = v
            rc_render = ctx.lib.rt_render(ctx._h, C.c_void_p(p.ctypes.data))
            rc = _raw(ctx, "rt_aovs", p, out)
            assert rc == rc_render == -1, (b, rc, rc_render)
            assert np.all(out == 7.0), f"{b}: a rejected call changes nothing"
            if "mode" not in b:  # the same rules, but the tile fields are ignored
                rays = np.zeros((64 * 64, 8), np.float32)
                rc_rays = ctx.lib.rt_sample_rays(ctx._h, C.c_void_p(p.ctypes.data), C.c_uint32(0), C.c_void_p(rays.ctypes.data))
                assert rc_rays == (0 if "tile_size" in b or "tile_rank" in b else -1), b
        p = api.render_params(64, 64, scene.camera, mode=2, spp=2)
        assert ctx.lib.rt_aovs(ctx._h, C.c_void_p(p.ctypes.data), C.c_void_p(0)) == -1
        assert ctx.lib.rt_aovs(ctx._h, C.c_void_p(0), C.c_void_p(out.ctypes.data)) == -1
        assert ctx.lib.rt_sample_rays(ctx._h, C.c_void_p(p.ctypes.data), C.c_uint32(0), C.c_void_p(0)) == -1
