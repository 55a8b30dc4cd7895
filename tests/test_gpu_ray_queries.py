"""Ray queries on the MI355X (rt_intersect / rt_occluded / rt_camera_rays), every comparison bit-exact.

The queries walk the frames' code with the ray's own range, so: camera rays give exactly the frame's closest hits (read_hits
and the oracle), arbitrary rays give what a brute-force float32 restatement of the device arithmetic gives, and occlusion is
exactly "the closest hit is not a miss"."""
import numpy as np
import pytest

from gpu_raytracer_amd import api, scenes

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
F32 = np.float32
MIN_T = F32(1e-5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_hits_equal(a, b):
    np.testing.assert_array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# Brute force: device_common.h's moller_trumbore and test_spheres in numpy float32, same operation order (the library is built
# with -ffp-contract=off: every operation is one IEEE f32 rounding, which numpy reproduces).
# ---------------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2],
                     a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _scene_tris(scene):
    p = scene.vertices["position"].astype(F32)
    tr = scene.triangles
    v0 = p[tr["v0_index"]]
    return v0, p[tr["v1_index"]] - v0, p[tr["v2_index"]] - v0  # e1, e2 in f32, as both builders store them in DevTri


def _moller_trumbore(v0, e1, e2, o, d):
    """rays (R, 1, 3) against triangles (1, T, 3) -> (ok, t, u, v), each (R, T)."""
    with np.errstate(all="ignore"):
        h = _cross(d, e2)
        a = _dot(e1, h)
        ok = ~(np.abs(a) < MIN_T)
        f = F32(1.0) / a
        s = o - v0
        u = f * _dot(s, h)
        ok &= ~((u < 0) | (u > 1))
        q = _cross(s, e1)
        v = f * _dot(d, q)
        ok &= ~((v < 0) | (u + v > 1))
        t = f * _dot(e2, q)
    return ok, t, u, v


def brute_force(scene, rays):
    """Expected (N, 4) hit records of rt_intersect for non-degenerate rays."""
    v0, e1, e2 = (x[None] for x in _scene_tris(scene))
    rays = rays.astype(F32)
    o_all, d_all = rays[:, 0:3], rays[:, 4:7]
    tmin_all = np.maximum(rays[:, 3], MIN_T)
    out = np.zeros((len(rays), 4), F32)
    out[:, 0] = rays[:, 7]
    out[:, 3] = np.full(len(rays), MISS, np.uint32).view(F32)
    for s0 in range(0, len(rays), 256):
        sl = slice(s0, s0 + 256)
        o, d, tmin = o_all[sl], d_all[sl], tmin_all[sl]
        best_t = rays[sl, 7].copy()
        best_p = np.full(len(o), MISS, np.uint64)
        with np.errstate(all="ignore"):
            for i, sp in enumerate(scene.spheres):  # spheres first, in index order, strict
                oc = o - sp["center"].astype(F32)
                a = _dot(d, d)
                b = F32(2.0) * _dot(oc, d)
                c = _dot(oc, oc) - F32(sp["radius"]) * F32(sp["radius"])
                disc = b * b - F32(4.0) * a * c
                sq = np.sqrt(disc)
                t1 = (-b - sq) / (F32(2.0) * a)
                t2 = (-b + sq) / (F32(2.0) * a)
                t = np.where(t1 > tmin, t1, t2)
                acc = ~(disc < 0) & (t > tmin) & (t < best_t)
                best_t = np.where(acc, t, best_t)
                best_p = np.where(acc, 0x80000000 | i, best_p)
        ok, t, u, v = _moller_trumbore(v0, e1, e2, o[:, None], d[:, None])
        ok &= t > tmin[:, None]
        tt = np.where(ok, t, np.inf).astype(F32)
        j = np.argmin(tt, 1)  # the first index among equal minima: the lower triangle index wins ties among triangles
        tj = tt[np.arange(len(o)), j]
        take = tj < best_t  # strict against a sphere and against tmax
        rows = np.arange(len(o))
        out[sl, 0] = np.where(take, tj, best_t)
        out[sl, 1] = np.where(take, u[rows, j], 0)
        out[sl, 2] = np.where(take, v[rows, j], 0)
        out[sl, 3] = np.where(take, j, best_p).astype(np.uint32).view(F32)
    return out


def _soup_rays(scene, n, seed):
    """Four kinds of rays, n // 4 each: aimed at interior points of random triangles, random directions, unnormalised
    directions, random tmin / tmax."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _scene_tris(scene)
    k = n // 4
    o = (rng.uniform(-4, 4, (n, 3)) + [0, 0, -2]).astype(F32)
    o[:k] = rng.uniform(-6, 6, (k, 3)).astype(F32) + F32(np.array([0, 0, 4], F32))
    ti = rng.integers(0, len(v0), k)
    w = rng.dirichlet([1, 1, 1], k).astype(F32)
    target = v0[ti] + e1[ti] * w[:, 1:2] + e2[ti] * w[:, 2:3]
    d = rng.standard_normal((n, 3)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:k] = target - o[:k]
    d[2 * k:3 * k] *= rng.uniform(0.01, 100, (k, 1)).astype(F32)
    tmin = np.full(n, MIN_T, F32)
    tmax = np.full(n, np.finfo(F32).max, F32)
    tmin[3 * k:] = rng.uniform(0, 4, n - 3 * k).astype(F32)
    tmax[3 * k:] = tmin[3 * k:] + rng.uniform(0, 6, n - 3 * k).astype(F32)
    return api.make_rays(o, d, tmin, tmax)


def _sponza_rays(scene, n, seed):
    """Incoherent rays from seeded surface points, random directions, tmax = distance to a light."""
    rng = np.random.default_rng(seed)
    v0, e1, e2 = _scene_tris(scene)
    ti = rng.integers(0, len(v0), n)
    w = rng.dirichlet([1, 1, 1], n).astype(F32)
    p = v0[ti] + e1[ti] * w[:, 1:2] + e2[ti] * w[:, 2:3]
    d = rng.standard_normal((n, 3)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lp = scene.lights["position"][1:].astype(F32)  # the point lights
    tmax = np.linalg.norm(lp[rng.integers(0, len(lp), n)] - p, axis=1).astype(F32)
    return api.make_rays(p, d, MIN_T, tmax)


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_rays(soup):
    return _soup_rays(soup, 4096, seed=11)


@pytest.fixture(scope="module")
def sponza():
    return scenes.sponza_like()


@pytest.fixture(scope="module")
def sponza_rays(sponza):
    return _sponza_rays(sponza, 1 << 20, seed=5)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("default", 0), ("default", 1), ("cornell12", 0), ("cornell12", 1), ("soup", 0), ("soup", 1)])
def test_camera_rays_give_the_frames_closest_hits(gpu_ctx, oracle_mod, name, mode):
    scene = scenes.random_soup(2000, n_spheres=3) if name == "soup" else scenes.SCENES[name]()
    w, h = 160, 96
    gpu_ctx.upload_scene(scene)
    gpu_ctx.render(w, h, scene.camera, mode=mode)
    prim, t = gpu_ctx.read_hits()
    rays = gpu_ctx.camera_rays(w, h, scene.camera, mode=mode)
    assert rays.shape == (w * h, 8)
    assert np.all(rays[:, 3] == MIN_T) and np.all(rays[:, 7] == np.finfo(F32).max)
    ht, hu, hv, hp = api.split_hits(gpu_ctx.intersect(rays))
    np.testing.assert_array_equal(hp, prim.reshape(-1))
    np.testing.assert_array_equal(_bits(ht), _bits(t.reshape(-1)))
    ref = oracle_mod.render_frame(oracle_mod.PackedScene(scene, use_bvh=False), w, h, mode=mode)
    np.testing.assert_array_equal(hp, ref["prim"].reshape(-1))
    np.testing.assert_array_equal(_bits(ht), _bits(ref["t"].reshape(-1)))
    np.testing.assert_array_equal(gpu_ctx.occluded(rays), hp != MISS)


def test_camera_rays_sponza_1080p_equal_read_hits(gpu_ctx, sponza):
    gpu_ctx.upload_scene(sponza)
    gpu_ctx.render(1920, 1080, sponza.camera, mode=0)
    prim, t = gpu_ctx.read_hits()
    ht, _, _, hp = api.split_hits(gpu_ctx.intersect(gpu_ctx.camera_rays(1920, 1080, sponza.camera)))
    np.testing.assert_array_equal(hp, prim.reshape(-1))
    np.testing.assert_array_equal(_bits(ht), _bits(t.reshape(-1)))


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_arbitrary_rays_equal_brute_force(gpu_ctx, soup, soup_rays):
    gpu_ctx.upload_scene(soup)
    got = gpu_ctx.intersect(soup_rays)
    want = brute_force(soup, soup_rays)
    _assert_hits_equal(got, want)
    _, _, _, p = api.split_hits(got)
    assert (p != MISS).mean() > 0.2 and (p < 0x80000000).sum() > 500 and ((p >= 0x80000000) & (p != MISS)).sum() > 5


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_range_boundaries(gpu_ctx, soup, soup_rays):
    gpu_ctx.upload_scene(soup)
    t, _, _, p = api.split_hits(gpu_ctx.intersect(soup_rays))
    hit = soup_rays[p != MISS].copy()
    th = t[p != MISS]
    at = hit.copy()
    at[:, 7] = th
    _, _, _, p2 = api.split_hits(gpu_ctx.intersect(at))
    assert np.all(p2 == MISS), "tmax = t_hit is exclusive"
    assert not gpu_ctx.occluded(at).any()
    past = hit.copy()
    past[:, 7] = np.nextafter(th, F32(np.inf))
    assert gpu_ctx.occluded(past).all()
    behind = hit.copy()
    behind[:, 3] = th
    behind[:, 7] = np.finfo(F32).max
    _assert_hits_equal(gpu_ctx.intersect(behind), brute_force(soup, behind))
    neg = soup_rays.copy()
    neg[:, 3] = np.where(np.arange(len(neg)) % 2 == 0, F32(-1.0), F32(-np.inf))
    floor = soup_rays.copy()
    floor[:, 3] = MIN_T
    _assert_hits_equal(gpu_ctx.intersect(neg), gpu_ctx.intersect(floor))


# 4 + 5 --------------------------------------------------------------------------------------------------------------------
def test_occlusion_equals_intersection_and_the_tree_does_not_matter(gpu_ctx, sponza, sponza_rays):
    gpu_ctx.upload_scene(sponza)
    assert gpu_ctx.stats()["tree_build"] == 2
    hits = gpu_ctx.intersect(sponza_rays)
    occ = gpu_ctx.occluded(sponza_rays)
    _, _, _, p = api.split_hits(hits)
    np.testing.assert_array_equal(occ, p != MISS)
    assert occ.any() and not occ.all()
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.stats()["tree_build"] == 0
    _assert_hits_equal(gpu_ctx.intersect(sponza_rays), hits)
    np.testing.assert_array_equal(gpu_ctx.occluded(sponza_rays), occ)


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_rays_are_misses(gpu_ctx, soup, soup_rays):
    gpu_ctx.upload_scene(soup)
    good = soup_rays[:64].copy()
    nan, inf = F32(np.nan), F32(np.inf)
    bad = np.tile(good[:1], (10, 1))
    bad[0, 0] = nan                    # origin NaN
    bad[1, 1] = inf                    # origin inf
    bad[2, 5] = -inf                   # direction inf
    bad[3, 6] = nan                    # direction NaN
    bad[4, 4:7] = 0                    # zero direction
    bad[5, 3] = nan                    # tmin NaN
    bad[6, 7] = nan                    # tmax NaN
    bad[7, 3], bad[7, 7] = 2.0, 2.0    # tmin == tmax
    bad[8, 3], bad[8, 7] = 3.0, 1.0    # tmin > tmax
    bad[9, 3], bad[9, 7] = -5.0, 0.0   # tmax below the floor
    mixed = np.concatenate([good[:30], bad, good[30:]])
    got = gpu_ctx.intersect(mixed)
    _assert_hits_equal(np.concatenate([got[:30], got[40:]]), gpu_ctx.intersect(good))
    g = got[30:40]
    np.testing.assert_array_equal(_bits(g[:, 0]), _bits(bad[:, 7]))  # t = tmax as given
    assert np.all(_bits(g[:, 1:3]) == 0) and np.all(_bits(g[:, 3]) == MISS)
    occ = gpu_ctx.occluded(mixed)
    assert not occ[30:40].any()
    np.testing.assert_array_equal(np.concatenate([occ[:30], occ[40:]]), gpu_ctx.occluded(good))


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_chunked_host_batch_equals_1m_calls(gpu_ctx, sponza, sponza_rays):
    gpu_ctx.upload_scene(sponza)
    n = 9_000_037
    assert n > 2 * api.QUERY_CHUNK and n % 64
    rays = np.resize(sponza_rays, (n, 8))
    rays[:, 4:7] *= np.linspace(0.5, 2.0, n, dtype=F32)[:, None]  # not nine copies of the same rays
    big = gpu_ctx.intersect(rays)
    assert gpu_ctx.stats()["rays"] == n
    for s in range(0, n, 1 << 20):
        _assert_hits_equal(big[s:s + (1 << 20)], gpu_ctx.intersect(rays[s:s + (1 << 20)]))
    _, _, _, p = api.split_hits(big)
    np.testing.assert_array_equal(gpu_ctx.occluded(rays), p != MISS)


@pytest.mark.parametrize("ids", [(0, 0), (0, 0, 0)])
def test_contexts_over_several_devices_give_the_same_bits(sponza, sponza_rays, ids):
    if torch is None:
        pytest.skip("torch is not installed")
    rays = sponza_rays[:300_001]
    with api.Context((0,)) as one:
        one.upload_scene(sponza)
        want_h, want_o = one.intersect(rays), one.occluded(rays)
    with api.Context(ids) as ctx:
        ctx.upload_scene(sponza)
        _assert_hits_equal(ctx.intersect(rays), want_h)
        np.testing.assert_array_equal(ctx.occluded(rays), want_o)
        dev = torch.from_numpy(rays).to("cuda:0")
        _assert_hits_equal(ctx.intersect(dev).cpu().numpy(), want_h)
        np.testing.assert_array_equal(ctx.occluded(dev).cpu().numpy(), want_o)


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_torch_tensors(gpu_ctx, soup, soup_rays):
    if torch is None:
        pytest.skip("torch is not installed")
    gpu_ctx.upload_scene(soup)
    want_h, want_o = gpu_ctx.intersect(soup_rays), gpu_ctx.occluded(soup_rays)
    dev = torch.from_numpy(soup_rays).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    h = gpu_ctx.intersect(dev)
    o = gpu_ctx.occluded(dev)
    assert h.device == dev.device and h.dtype == torch.float32 and o.dtype == torch.bool
    _assert_hits_equal(h.cpu().numpy(), want_h)
    np.testing.assert_array_equal(o.cpu().numpy(), want_o)
    out = torch.empty((len(soup_rays), 4), device="cuda:0")
    assert gpu_ctx.intersect(dev, out=out) is out
    _assert_hits_equal(out.cpu().numpy(), want_h)
    cpu = torch.from_numpy(soup_rays.copy())
    hc = gpu_ctx.intersect(cpu)
    assert hc.device.type == "cpu"
    _assert_hits_equal(hc.numpy(), want_h)
    np.testing.assert_array_equal(gpu_ctx.occluded(cpu).numpy(), want_o)
    _, _, _, p = api.split_hits(h)
    assert p.dtype == torch.int64 and int(p.max()) == MISS
    # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    buf = torch.zeros(len(soup_rays) * 8 + 4, device="cuda:0")
    skew = buf[1:1 + len(soup_rays) * 8].view(-1, 8)
    with pytest.raises(api.RtError) as e:
        gpu_ctx.intersect(skew)
    assert e.value.code == -1 and "aligned" in str(e.value)
    if torch.cuda.device_count() > 1:
        with api.Context((0, 1)) as two:
            two.upload_scene(soup)
            with pytest.raises(api.RtError) as e:
                two.intersect(dev, out=torch.empty((len(soup_rays), 4), device="cuda:1"))
            assert e.value.code == -1
    _assert_hits_equal(gpu_ctx.intersect(dev).cpu().numpy(), want_h)


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_queries_and_the_frame_path(gpu_ctx, oracle_mod, soup, soup_rays):
    with pytest.raises(api.RtError) as e:
        gpu_ctx.intersect(soup_rays)
    assert e.value.code == -4
    gpu_ctx.upload_scene(soup)
    assert gpu_ctx.intersect(np.zeros((0, 8), F32)).shape == (0, 4)
    assert gpu_ctx.occluded(np.zeros((0, 8), F32)).shape == (0,)
    gpu_ctx.render(200, 120, soup.camera, mode=1)
    rgb, prim, t = gpu_ctx.read_rgb32f(), *gpu_ctx.read_hits()
    gpu_ctx.intersect(soup_rays)
    gpu_ctx.occluded(soup_rays)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_rays) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["kernel_ms"] > 0
    np.testing.assert_array_equal(_bits(gpu_ctx.read_rgb32f()), _bits(rgb))
    p2, t2 = gpu_ctx.read_hits()
    np.testing.assert_array_equal(p2, prim)
    np.testing.assert_array_equal(_bits(t2), _bits(t))
    gpu_ctx.intersect(soup_rays, counters=True)
    st = gpu_ctx.stats()
    assert st["node_visits"] > 0 and st["tri_tests"] > 0 and st["rays"] == len(soup_rays)
    # empty scene: all misses
    gpu_ctx.upload_scene(scenes.empty_scene())
    _, _, _, p = api.split_hits(gpu_ctx.intersect(soup_rays))
    assert np.all(p == MISS) and not gpu_ctx.occluded(soup_rays).any()


def test_query_after_dispatch_tile_waits_for_it(oracle_mod, soup, soup_rays):
    packed = oracle_mod.PackedScene(soup)
    w, h = 256, 128
    pc = packed.push_constants(w, h, channel=0, tile_offset=(128, 0))
    with api.Context() as ref:
        ref.upload_scene_packed(packed.metadata, packed.offsets, packed.tri_bufs, packed.triangles_per_buffer, soup.materials)
        ref.dispatch_tile(pc)
        want = ref.read_rgba8_channels()
        want_h = ref.intersect(soup_rays)
    with api.Context() as ctx:
        ctx.upload_scene_packed(packed.metadata, packed.offsets, packed.tri_bufs, packed.triangles_per_buffer, soup.materials)
        ctx.dispatch_tile(pc)
        _assert_hits_equal(ctx.intersect(soup_rays), want_h)
        got = ctx.read_rgba8_channels()
    for c in range(3):
        np.testing.assert_array_equal(got[c], want[c])
    assert want[0][:, 128:, 3].min() == 255
