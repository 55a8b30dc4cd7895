"""Multi-hit ray queries on the MI355X (rt_intersect_all): the first K hits along each ray, every comparison of hit records bit for bit.

The expected lists come from a brute force in numpy float32 over all primitives (the library is built with -ffp-contract=off, so numpy
reproduces every rounding): all candidates of a ray in (tmin, tmax), sorted by t bits, spheres before triangles at equal t, each kind
by index.  The tests hold the call to that list, to rt_intersect (K = 1, and peeling with a raised tmin), to itself across K, trees,
devices and buffer kinds, and check that it leaves the frame path alone."""
import ctypes as C

import numpy as np
import pytest

from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import types as T

from test_gpu_ray_queries import _bits, _dot, _moller_trumbore, _scene_tris, _soup_rays, _sponza_rays

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
SPHERE = 0x80000000
F32 = np.float32
MIN_T = F32(1e-5)
LISTED = api.MULTI_HIT_MAX + 1  # candidates the brute force keeps per ray: one more than any K lists


def _assert_bits_equal(a, b):
    np.testing.assert_array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# Brute force.  Non-degenerate rays only.
# ---------------------------------------------------------------------------------------------------------------------------
def all_candidates(scene, rays):
    """-> (records (N, LISTED, 4) float32, totals (N,) uint32): each ray's first LISTED candidates in the order rule as (t, u, v,
    prim bits) records, miss records (tmax, 0, 0, MISS) behind them, and the number of all its candidates in (tmin, tmax)."""
    v0, e1, e2 = (x[None] for x in _scene_tris(scene))
    n_t, n_s = v0.shape[1], len(scene.spheres)
    rays = rays.astype(F32)
    o_all, d_all, tmax_all = rays[:, 0:3], rays[:, 4:7], rays[:, 7]
    tmin_all = np.maximum(rays[:, 3], MIN_T)
    rec = np.zeros((len(rays), LISTED, 4), F32)
    totals = np.zeros(len(rays), np.uint32)
    key = np.concatenate([np.arange(n_s, dtype=np.uint64), np.uint64(SPHERE) | np.arange(n_t, dtype=np.uint64)])  # spheres first, then by index
    prim = np.concatenate([SPHERE | np.arange(n_s, dtype=np.uint32), np.arange(n_t, dtype=np.uint32)])
    for s0 in range(0, len(rays), 256):
        sl = slice(s0, s0 + 256)
        o, d, tmin, tmax = o_all[sl], d_all[sl], tmin_all[sl], tmax_all[sl]
        r = len(o)
        t = np.zeros((r, n_s + n_t), F32)
        u, v = np.zeros_like(t), np.zeros_like(t)
        ok = np.zeros(t.shape, bool)
        with np.errstate(all="ignore"):
            for i, sp in enumerate(scene.spheres):  # test_spheres of device_common.h for one sphere, against the ray's own tmin
                oc = o - sp["center"].astype(F32)
                a = _dot(d, d)
                b = F32(2.0) * _dot(oc, d)
                c = _dot(oc, oc) - F32(sp["radius"]) * F32(sp["radius"])
                disc = b * b - F32(4.0) * a * c
                sq = np.sqrt(disc)
                t1 = (-b - sq) / (F32(2.0) * a)
                t2 = (-b + sq) / (F32(2.0) * a)
                t[:, i] = np.where(t1 > tmin, t1, t2)
                ok[:, i] = ~(disc < 0)
            ok[:, n_s:], t[:, n_s:], u[:, n_s:], v[:, n_s:] = _moller_trumbore(v0, e1, e2, o[:, None], d[:, None])
            ok &= (t > tmin[:, None]) & (t < tmax[:, None])
        totals[sl] = ok.sum(1)
        order_key = np.where(ok, (_bits(t).astype(np.uint64) << np.uint64(32)) | key[None], np.uint64(0xFFFFFFFFFFFFFFFF))
        first = np.argsort(order_key, axis=1, kind="stable")[:, :LISTED]
        rows = np.arange(r)[:, None]
        listed = ok[rows, first]
        rec[sl, :, 0] = np.where(listed, t[rows, first], tmax[:, None])
        rec[sl, :, 1] = np.where(listed, u[rows, first], 0)
        rec[sl, :, 2] = np.where(listed, v[rows, first], 0)
        rec[sl, :, 3] = np.where(listed, prim[first], np.uint32(MISS)).astype(np.uint32).view(F32)
    return rec, totals


def expected(cands, k):
    """What max_hits = k lists of all_candidates' result -> (hits (N, k, 4), counts (N,))."""
    rec, totals = cands
    hits = rec[:, :k].copy()
    return hits, np.minimum(totals, k).astype(np.uint32)


def _prims(hits):
    return _bits(hits[..., 3])


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_rays(soup):
    return _soup_rays(soup, 4096, seed=11)


@pytest.fixture(scope="module")
def soup_cands(soup, soup_rays):
    return all_candidates(soup, soup_rays)


@pytest.fixture(scope="module")
def sponza():
    return scenes.sponza_like()


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 8, 16])
def test_lists_equal_brute_force(gpu_ctx, soup, soup_rays, soup_cands, k):
    rec, totals = soup_cands
    # the batch exercises what it is meant to: truncated lists, spheres among the listed hits
    assert (totals > 8).sum() >= 100 and (totals > 4).sum() >= 500
    p = _prims(rec[:, :k])
    assert ((p >= SPHERE) & (p != MISS)).sum() > 5
    want_h, want_c = expected(soup_cands, k)
    gpu_ctx.upload_scene(soup)
    hits, counts = gpu_ctx.intersect_all(soup_rays, k)
    assert hits.shape == (len(soup_rays), k, 4) and hits.dtype == F32 and counts.shape == (len(soup_rays),) and counts.dtype == np.uint32
    _assert_bits_equal(hits, want_h)
    np.testing.assert_array_equal(counts, want_c)
    hits_all, counts_all = gpu_ctx.intersect_all(soup_rays, k, count_all=True)
    _assert_bits_equal(hits_all, want_h)
    np.testing.assert_array_equal(counts_all, totals)
    t, u, v, prim = api.split_hits(hits.reshape(-1, 4))
    np.testing.assert_array_equal(prim, _prims(want_h).reshape(-1))


# 2 ------------------------------------------------------------------------------------------------------------------------
def _degenerate_rays(good):
    """The degenerate rays of test_gpu_ray_queries.test_degenerate_rays_are_misses."""
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
    return bad


def test_one_hit_is_rt_intersect(gpu_ctx, soup, soup_rays):
    bad = _degenerate_rays(soup_rays)
    rays = np.concatenate([soup_rays[:1000], bad, soup_rays[1000:]])
    gpu_ctx.upload_scene(soup)
    want = gpu_ctx.intersect(rays)
    hits, counts = gpu_ctx.intersect_all(rays, 1)
    assert hits.tobytes() == want.tobytes()
    np.testing.assert_array_equal(counts, (_prims(want) != MISS).astype(np.uint32))
    assert not counts[1000:1010].any()
    # degenerate rays list nothing at any K and count nothing
    hits4, counts4 = gpu_ctx.intersect_all(bad, 4, count_all=True)
    assert not counts4.any() and np.all(_prims(hits4) == MISS) and np.all(_bits(hits4[:, :, 1:3]) == 0)
    _assert_bits_equal(hits4[:, :, 0], np.repeat(bad[:, 7:8], 4, 1))  # t = tmax as given
    # an empty scene: rt_intersect's bytes
    gpu_ctx.upload_scene(scenes.empty_scene())
    hits, counts = gpu_ctx.intersect_all(rays, 1)
    assert hits.tobytes() == gpu_ctx.intersect(rays).tobytes() and not counts.any() and np.all(_prims(hits) == MISS)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_shorter_lists_are_prefixes(gpu_ctx, soup, soup_rays):
    gpu_ctx.upload_scene(soup)
    h16, c16 = gpu_ctx.intersect_all(soup_rays, 16)
    h4, c4 = gpu_ctx.intersect_all(soup_rays, 4)
    _assert_bits_equal(h4, h16[:, :4])
    np.testing.assert_array_equal(c4, np.minimum(c16, 4))
    assert (c16 > 4).sum() >= 500


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_peeling_with_rt_intersect_gives_the_next_record(gpu_ctx):
    soup = scenes.random_soup(3000)  # triangles only: a sphere's hit changes with tmin (t1, then t2), a triangle's does not
    rays = _soup_rays(soup, 4096, seed=11)
    gpu_ctx.upload_scene(soup)
    hits, counts = gpu_ctx.intersect_all(rays, 16)
    t = hits[:, :, 0]
    ray, j = np.nonzero(np.arange(15)[None] + 1 < counts[:, None])  # hits j and j + 1 are both listed
    assert len(ray) > 3000 and j.max() >= 8
    # what makes peeling valid: t_j is at or above the floor, so it is the tmin the walk uses, and the next hit is strictly behind it
    assert np.all(t[ray, j] >= MIN_T) and np.all(t[ray, j + 1] > t[ray, j])
    peel = rays[ray].copy()
    peel[:, 3] = t[ray, j]
    _assert_bits_equal(gpu_ctx.intersect(peel), hits[ray, j + 1])


# 5 ------------------------------------------------------------------------------------------------------------------------
TIE_A, TIE_B, TIE_C, TIE_BACK = 5, 300, 900, 2


def _tie_scene():
    """1,024 triangles (enough for the device builder), all far away except: one triangle stored three times, at indices TIE_A <
    TIE_B < TIE_C, in the plane z = -3; one more behind it at z = -4 with the LOWEST index of the four; a sphere in front."""
    n = 1024
    k = np.arange(n, dtype=np.float64)
    base = np.stack([500.0 + (k % 32) * 1.5, -20.0 + (k // 32) * 1.5, 400.0 + (k % 7)], 1)  # as reference_cases.padded
    verts = np.stack([base, base + [1.0, 0.0, 0.0], base + [0.0, 1.0, 0.2]], 1)
    for i in (TIE_A, TIE_B, TIE_C):
        verts[i] = [(-1.0, -1.0, -3.0), (1.3, -0.9, -3.0), (-0.2, 1.1, -3.0)]
    verts[TIE_BACK] = [(-2.0, -2.0, -4.0), (2.0, -2.0, -4.0), (0.0, 2.5, -4.0)]
    va = np.zeros(3 * n, T.VERTEX)
    va["position"] = verts.reshape(-1, 3)
    ta = np.zeros(n, T.TRIANGLE)
    idx = np.arange(3 * n).reshape(-1, 3)
    ta["v0_index"], ta["v1_index"], ta["v2_index"] = idx[:, 0], idx[:, 1], idx[:, 2]
    spheres = np.array([((0.0, 0.0, -1.0), 0.3, 0)], dtype=T.SPHERE)
    lights = np.array([H.light_point((0.0, 0.0, 3.0), (1.0, 1.0, 1.0), 2.0)], dtype=T.LIGHT)
    materials = np.array([H.material_diffuse((0.5, 0.5, 0.5))], dtype=T.MATERIAL)
    return scenes.Scene("ties", spheres, lights, va, ta, materials, H.camera())


def _tie_rays():
    """128 rays from z = 2 toward -z: the first 64 through the sphere and the stack, the rest beside the sphere through the stack."""
    rng = np.random.default_rng(7)
    o = np.zeros((128, 3), F32)
    o[:64, :2] = rng.uniform(-0.15, 0.15, (64, 2))
    ang = rng.uniform(0, 2 * np.pi, 64)
    o[64:, 0], o[64:, 1] = 0.4 * np.cos(ang), 0.4 * np.sin(ang)
    o[:, 2] = 2.0
    d = np.tile(np.array([0.0, 0.0, -1.0], F32), (128, 1))
    d[:, :2] += rng.uniform(-0.01, 0.01, (128, 2)).astype(F32)
    return api.make_rays(o, d, MIN_T, np.finfo(F32).max)


def test_exact_ties_and_the_bound(gpu_ctx):
    scene, rays = _tie_scene(), _tie_rays()
    cands = all_candidates(scene, rays)
    rec, totals = cands
    stack = np.array([TIE_A, TIE_B, TIE_C, TIE_BACK], np.uint32)
    assert np.all(totals[:64] == 5) and np.all(totals[64:] == 4)
    assert np.all(_prims(rec[:64, :5]) == np.concatenate([[SPHERE], stack])) and np.all(_prims(rec[64:, :4]) == stack)
    for trees in ("device", "quality"):
        gpu_ctx.upload_scene(scene)
        assert gpu_ctx.stats()["tree_build"] == 2
        if trees == "quality":
            gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
            assert gpu_ctx.stats()["tree_build"] == 0
        for k in (1, 2, 3, 4, 5, 8):
            hits, counts = gpu_ctx.intersect_all(rays, k, count_all=True)
            want_h, _ = expected(cands, k)
            _assert_bits_equal(hits, want_h)
            np.testing.assert_array_equal(counts, totals)
        h5, _ = gpu_ctx.intersect_all(rays, 5)
        thru, beside = h5[:64], h5[64:]
        assert np.all(_prims(thru) == np.concatenate([[SPHERE], stack]))
        assert np.all(_prims(beside) == np.concatenate([stack, [MISS]]))
        for h, a in ((thru, 1), (beside, 0)):  # a, b and c: identical t, u, v bits
            _assert_bits_equal(h[:, a, :3], h[:, a + 1, :3])
            _assert_bits_equal(h[:, a, :3], h[:, a + 2, :3])
            assert np.all(h[:, a + 3, 0] > h[:, a, 0])
        h3, c3 = gpu_ctx.intersect_all(rays, 3)
        assert np.all(_prims(h3[:64]) == [SPHERE, TIE_A, TIE_B]) and np.all(_prims(h3[64:]) == [TIE_A, TIE_B, TIE_C]) and np.all(c3 == 3)
        h2, _ = gpu_ctx.intersect_all(rays, 2)
        assert np.all(_prims(h2[:64]) == [SPHERE, TIE_A]) and np.all(_prims(h2[64:]) == [TIE_A, TIE_B])
        _assert_bits_equal(h2, h5[:, :2])
        _assert_bits_equal(h3, h5[:, :3])


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_the_tree_does_not_matter(gpu_ctx, sponza):
    rays = _sponza_rays(sponza, 65536, seed=5)
    gpu_ctx.upload_scene(sponza)
    assert gpu_ctx.stats()["tree_build"] == 2
    hits, counts = gpu_ctx.intersect_all(rays, 8, count_all=True)
    assert (counts > 8).any() and (counts == 0).any() and ((counts > 1) & (counts < 8)).any()
    _assert_bits_equal(hits[:, 0], gpu_ctx.intersect(rays))
    st = gpu_ctx.update_geometry(vertices=np.ascontiguousarray(sponza.vertices["position"], dtype=F32))  # the same positions: a refitted tree
    assert st["flags"] & api.STAT_REFIT
    h, c = gpu_ctx.intersect_all(rays, 8, count_all=True)
    _assert_bits_equal(h, hits)
    np.testing.assert_array_equal(c, counts)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.stats()["tree_build"] == 0
    h, c = gpu_ctx.intersect_all(rays, 8, count_all=True)
    _assert_bits_equal(h, hits)
    np.testing.assert_array_equal(c, counts)


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_crossing_counts(gpu_ctx, soup, soup_rays, soup_cands):
    gpu_ctx.upload_scene(soup)
    hits, counts = gpu_ctx.intersect_all(soup_rays, 0, count_all=True)
    assert hits is None
    np.testing.assert_array_equal(counts, soup_cands[1])
    own = np.full(len(soup_rays), 77, np.uint32)
    assert gpu_ctx.intersect_all(soup_rays, 0, counts=own, count_all=True)[1] is own
    np.testing.assert_array_equal(own, soup_cands[1])
    with pytest.raises(ValueError, match="max_hits"):
        gpu_ctx.intersect_all(soup_rays, 0)
    # the library's own checks
    n = len(soup_rays)
    call = lambda k, h, c, flags: gpu_ctx.lib.rt_intersect_all(gpu_ctx._h, C.c_void_p(soup_rays.ctypes.data), C.c_size_t(n), C.c_uint32(k),
                                                                C.c_void_p(h), C.c_void_p(c), C.c_uint32(flags))
    buf = np.zeros((n, 17, 4), F32)
    assert call(0, buf.ctypes.data, own.ctypes.data, 0) == -1          # no RT_QUERY_COUNT_ALL
    assert call(0, buf.ctypes.data, 0, api.QUERY_COUNT_ALL) == -1      # no counts
    assert call(0, 0, own.ctypes.data, api.QUERY_COUNT_ALL) == 0       # hits is ignored
    assert call(17, buf.ctypes.data, own.ctypes.data, 0) == -1
    assert call(4, 0, own.ctypes.data, 0) == -1
    assert call(4, buf.ctypes.data, 0, 0) == 0                          # counts may be NULL
    assert call(4, buf.ctypes.data, own.ctypes.data, 4) == -1          # an unknown flag bit
    assert gpu_ctx.lib.rt_intersect_all(gpu_ctx._h, None, C.c_size_t(0), C.c_uint32(4), None, None, C.c_uint32(0)) == 0  # n == 0
    # the closest-hit and any-hit calls keep refusing the new flag bit
    with pytest.raises(api.RtError) as e:
        gpu_ctx._check(gpu_ctx.lib.rt_intersect(gpu_ctx._h, C.c_void_p(soup_rays.ctypes.data), C.c_size_t(n), C.c_void_p(buf.ctypes.data),
                                                C.c_uint32(api.QUERY_COUNT_ALL)))
    assert e.value.code == -1
    assert gpu_ctx.lib.rt_occluded(gpu_ctx._h, C.c_void_p(soup_rays.ctypes.data), C.c_size_t(n), C.c_void_p(buf.ctypes.data),
                                   C.c_uint32(api.QUERY_COUNT_ALL)) == -1
    with api.Context() as fresh:
        with pytest.raises(api.RtError) as e:
            fresh.intersect_all(soup_rays, 4)
        assert e.value.code == -4


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_torch_tensors(gpu_ctx, soup, soup_rays):
    if torch is None:
        pytest.skip("torch is not installed")
    gpu_ctx.upload_scene(soup)
    want_h, want_c = gpu_ctx.intersect_all(soup_rays, 8)
    want_a = gpu_ctx.intersect_all(soup_rays, 8, count_all=True)[1]
    dev = torch.from_numpy(soup_rays).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    h, c = gpu_ctx.intersect_all(dev, 8)
    assert h.device == dev.device and h.dtype == torch.float32 and tuple(h.shape) == (len(soup_rays), 8, 4)
    assert c.device == dev.device and c.dtype == torch.int32 and tuple(c.shape) == (len(soup_rays),)
    _assert_bits_equal(h.cpu().numpy(), want_h)
    np.testing.assert_array_equal(c.cpu().numpy(), want_c.astype(np.int32))
    out, cnt = torch.empty((len(soup_rays), 8, 4), device="cuda:0"), torch.empty(len(soup_rays), dtype=torch.int32, device="cuda:0")
    got = gpu_ctx.intersect_all(dev, 8, out=out, counts=cnt, count_all=True)
    assert got[0] is out and got[1] is cnt
    _assert_bits_equal(out.cpu().numpy(), want_h)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want_a.astype(np.int32))
    none, c0 = gpu_ctx.intersect_all(dev, 0, count_all=True)
    assert none is None
    np.testing.assert_array_equal(c0.cpu().numpy(), want_a.astype(np.int32))
    cpu = torch.from_numpy(soup_rays.copy())
    hc, cc = gpu_ctx.intersect_all(cpu, 8)
    assert hc.device.type == "cpu" and cc.device.type == "cpu"
    _assert_bits_equal(hc.numpy(), want_h)
    np.testing.assert_array_equal(cc.numpy(), want_c.astype(np.int32))
    _, _, _, p = api.split_hits(h.reshape(-1, 4))
    assert p.dtype == torch.int64 and int(p.max()) == MISS
    # device rays with host counts, and a counts tensor 4 bytes off: fine (4-byte alignment is enough); rays 4 bytes off: refused
    buf = torch.zeros(len(soup_rays) + 1, dtype=torch.int32, device="cuda:0")
    h1, c1 = gpu_ctx.intersect_all(dev, 8, counts=buf[1:])
    np.testing.assert_array_equal(c1.cpu().numpy(), want_c.astype(np.int32))
    skew = torch.zeros(len(soup_rays) * 8 + 4, device="cuda:0")[1:1 + len(soup_rays) * 8].view(-1, 8)
    with pytest.raises(api.RtError) as e:
        gpu_ctx.intersect_all(skew, 8)
    assert e.value.code == -1 and "aligned" in str(e.value)
    rc = gpu_ctx.lib.rt_intersect_all(gpu_ctx._h, C.c_void_p(dev.data_ptr()), C.c_size_t(len(soup_rays)), C.c_uint32(8), C.c_void_p(out.data_ptr()),
                                      C.c_void_p(want_c.ctypes.data), C.c_uint32(0))  # device rays and hits, host counts
    assert rc == -1
    _assert_bits_equal(gpu_ctx.intersect_all(dev, 8)[0].cpu().numpy(), want_h)


def test_chunked_host_batch_equals_its_halves(gpu_ctx, soup, soup_rays):
    n = 300_000
    assert n > api.QUERY_CHUNK // 16 and n % 64
    rays = np.resize(soup_rays, (n, 8))
    rays[:, 4:7] *= np.linspace(0.5, 2.0, n, dtype=F32)[:, None]  # not 73 copies of the same rays
    gpu_ctx.upload_scene(soup)
    hits, counts = gpu_ctx.intersect_all(rays, 16, count_all=True)
    assert gpu_ctx.stats()["rays"] == n
    for s in (slice(0, n // 2), slice(n // 2, n)):
        h, c = gpu_ctx.intersect_all(rays[s], 16, count_all=True)
        _assert_bits_equal(hits[s], h)
        np.testing.assert_array_equal(counts[s], c)
    _assert_bits_equal(hits[:, 0], gpu_ctx.intersect(rays))


def test_context_over_two_devices_gives_the_same_bits(gpu_ctx, soup, soup_rays):
    gpu_ctx.upload_scene(soup)
    want_h, want_c = gpu_ctx.intersect_all(soup_rays, 8, count_all=True)
    with api.Context((0, 0)) as two:
        two.upload_scene(soup)
        h, c = two.intersect_all(soup_rays, 8, count_all=True)
        assert two.stats()["rays"] == len(soup_rays)
    _assert_bits_equal(h, want_h)
    np.testing.assert_array_equal(c, want_c)


def test_counters_and_statistics(gpu_ctx, soup, soup_rays):
    gpu_ctx.upload_scene(soup)
    gpu_ctx.intersect_all(soup_rays, 4)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_rays) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["kernel_ms"] > 0
    assert st["node_visits"] == 0 and st["tri_tests"] == 0
    gpu_ctx.intersect_all(soup_rays, 4, counters=True)
    some = gpu_ctx.stats()
    assert some["node_visits"] > 0 and some["tri_tests"] > 0 and some["rays"] == len(soup_rays)
    gpu_ctx.intersect_all(soup_rays, 4, counters=True, count_all=True)
    every = gpu_ctx.stats()
    assert every["node_visits"] >= some["node_visits"] and every["tri_tests"] >= some["tri_tests"]
    gpu_ctx.intersect(soup_rays, counters=True)
    one = gpu_ctx.stats()
    gpu_ctx.intersect_all(soup_rays, 1, counters=True)
    st = gpu_ctx.stats()
    assert some["node_visits"] >= st["node_visits"] > 0 and st["tri_tests"] == one["tri_tests"] and st["node_visits"] == one["node_visits"]


def test_a_running_accumulation_is_left_alone(gpu_ctx, soup, soup_rays):
    gpu_ctx.upload_scene(soup)
    gpu_ctx.render(96, 64, soup.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    gpu_ctx.intersect_all(soup_rays, 8, count_all=True)
    _assert_bits_equal(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4
