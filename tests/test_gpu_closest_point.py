"""Closest-point queries on the MI355X (rt_closest_point).  Every comparison with the float32 statement (closest_point_cases.py's
numpy brute force over all triangles and spheres) is byte for byte: the tree only culls, so the answer is the statement's whatever
tree, memory, batch size or device count is in use."""
import dataclasses

import numpy as np
import pytest

import closest_point_cases as cc
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


def _same(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _miss_records(radius):
    rec = np.zeros(len(radius), T.NEAREST)
    rec["distance"] = radius
    rec["prim_id"] = cc.PRIM_MISS
    return rec.view(F32).reshape(-1, 8)


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_points(soup):
    """4096 points of the four kinds, then points inside each sphere and every sphere's centre."""
    rng = np.random.default_rng(21)
    c, r = soup.spheres["center"].astype(F32), soup.spheres["radius"].astype(F32)
    inside = (c[:, None, :] + rng.uniform(-0.5, 0.5, (len(c), 4, 3)) * r[:, None, None]).reshape(-1, 3).astype(F32)
    return api.make_points(np.concatenate([cc.four_kinds(soup, 4096, 11), inside, c]))


@pytest.fixture(scope="module")
def soup_want(soup, soup_points):
    """The statement's answers, computed once: (records, dist2)."""
    rec, dist2 = cc.brute_force(soup, soup_points, return_dist2=True)
    rec.setflags(write=False)
    dist2.setflags(write=False)
    return rec, dist2


@pytest.fixture(scope="module")
def sponza():
    return scenes.sponza_like()


@pytest.fixture(scope="module")
def sponza_points(sponza):
    return api.make_points(np.concatenate([cc.near_surface(sponza, 1024, 3), cc.scattered(sponza, 1024, 4)]))


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_soup_equals_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_points, soup_want):
    want, _ = soup_want
    prim = api.split_nearest(want)[4]
    assert (prim >= cc.SPHERE_FLAG).sum() >= 5 and (prim < cc.SPHERE_FLAG).sum() > 3000 and (prim != cc.PRIM_MISS).all()
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.closest_point(soup_points), want)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_points) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["kernel_ms"] > 0
    own = np.full((len(soup_points), 8), 7.0, F32)
    assert gpu_ctx.closest_point(soup_points, out=own) is own
    _same(own, want)
    if torch is None:
        pytest.skip("torch is not installed: device memory not exercised")
    dev = torch.from_numpy(soup_points).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    got = gpu_ctx.closest_point(dev)
    assert got.device == dev.device and got.dtype == torch.float32
    _same(got.cpu().numpy(), want)
    out = torch.empty((len(soup_points), 8), device="cuda:0")
    assert gpu_ctx.closest_point(dev, out=out) is out
    _same(out.cpu().numpy(), want)
    # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    buf = torch.zeros(len(soup_points) * 4 + 1, device="cuda:0")
    with pytest.raises(api.RtError) as e:
        gpu_ctx.closest_point(buf[1:].view(-1, 4))
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.closest_point(dev).cpu().numpy(), want)


def test_spheres_alone_from_outside_inside_and_the_centre(gpu_ctx, soup):
    """No triangles, so no tree: the spheres' own statement, the centre's +x rule and the index order among equal distances."""
    spheres = np.concatenate([soup.spheres, soup.spheres[:1]])  # sphere 3 coincides with sphere 0: the lower index wins
    scene = dataclasses.replace(soup, vertices=soup.vertices[:0], triangles=soup.triangles[:0], spheres=spheres)
    rng = np.random.default_rng(22)
    c, r = spheres["center"].astype(F32), spheres["radius"].astype(F32)
    inside = (c[:, None, :] + rng.uniform(-0.5, 0.5, (len(c), 8, 3)) * r[:, None, None]).reshape(-1, 3).astype(F32)
    outside = rng.uniform(-6.0, 4.0, (200, 3)).astype(F32)
    points = api.make_points(np.concatenate([c, inside, outside]))
    points[1::2, 3] = 0.3  # every other one within a finite radius: some misses
    want = cc.brute_force(scene, points)
    prim = api.split_nearest(want)[4]
    assert (prim == cc.PRIM_MISS).any() and prim[0] == cc.SPHERE_FLAG and set(prim[prim != cc.PRIM_MISS] & 3) == {0, 1, 2}
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.closest_point(points), want)


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_boundaries(gpu_ctx, soup, soup_points, soup_want, n):
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.closest_point(np.ascontiguousarray(soup_points[:n])), soup_want[0][:n])


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_between_walls_resolve_to_the_lower_index(gpu_ctx):
    """cornell12: the cube's centre, points on its diagonals and on its mid-planes are equally far from two or more triangles, bit
    for bit; the lower original index wins, as in the brute force."""
    scene = scenes.cornell12()
    rng = np.random.default_rng(8)
    t = np.linspace(-0.95, 0.95, 39).astype(F32)
    signs = np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1]], F32)
    diagonals = (t[None, :, None] * signs[:, None, :]).reshape(-1, 3)           # 156, the centre among them (t = 0)
    planes = rng.uniform(-0.9, 0.9, (600, 3)).astype(F32)
    planes[np.arange(600), np.arange(600) % 3] = 0.0                            # on x = 0, y = 0 or z = 0
    inside = rng.uniform(-1.0, 1.0, (1024 - 156 - 600, 3)).astype(F32)
    points = api.make_points(np.concatenate([diagonals, planes, inside]))
    assert len(points) == 1024 and (points[:, :3] == 0).all(1).any()
    want = cc.brute_force(scene, points)
    d2 = cc.triangle_candidates(*cc.records(scene)[:3], points[:, :3])[0]
    tied = (d2 == d2.min(1, keepdims=True)).sum(1) >= 2
    walls = np.array([np.flatnonzero(row == row.min())[[0, -1]] // 2 for row in d2])  # the first and the last of the tied: (quad, quad)
    assert tied.sum() >= 100 and (walls[:, 0] != walls[:, 1]).sum() >= 50, "exact ties, most of them between walls"
    np.testing.assert_array_equal(api.split_nearest(want)[4], (d2 == d2.min(1, keepdims=True)).argmax(1))
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.closest_point(points), want)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_the_radius_is_strict_on_both_sides(gpu_ctx, soup, soup_points, soup_want):
    """From each point's answer (dist2, record) at radius = inf: the smallest radius with r * r > dist2 gives the same bytes, the
    largest with r * r <= dist2 the miss record with that radius's bits in `distance`."""
    want, dist2 = soup_want
    gpu_ctx.upload_scene(soup)
    first = gpu_ctx.closest_point(soup_points)
    _same(first, want)
    with np.errstate(all="ignore"):
        above = np.maximum(np.sqrt(dist2), F32(3e-23))  # (3e-23)^2 is the smallest subnormal: above dist2 = 0
        for _ in range(4):
            above = np.where(above * above > dist2, above, np.nextafter(above, INF))
        below = np.sqrt(dist2)
        for _ in range(4):
            below = np.where(below * below <= dist2, below, np.nextafter(below, -INF))
        assert (above * above > dist2).all() and (below * below <= dist2).all()
        assert (np.nextafter(above, -INF) ** 2 <= dist2)[dist2 > 1e-30].all() and (np.nextafter(below, INF) ** 2 > dist2)[dist2 > 1e-30].all(), "adjacent"
    assert (dist2 == 0).any() and (dist2 > 0).any()
    q = soup_points.copy()
    q[:, 3] = above
    _same(gpu_ctx.closest_point(q), first)
    q[:, 3] = below
    _same(gpu_ctx.closest_point(q), _miss_records(below))


def test_degenerate_queries_are_misses_without_a_walk(gpu_ctx, soup):
    gpu_ctx.upload_scene(soup)
    nan = F32(np.nan)
    q = np.array([[nan, 0, -3, INF], [0, nan, -3, 1], [0, 0, nan, 1], [INF, 0, -3, INF], [0, -INF, -3, INF], [0, 0, INF, 2],
                  [0, 0, -3, nan], [0, 0, -3, 0.0], [0, 0, -3, -0.0], [0, 0, -3, -1.0], [0, 0, -3, -INF]], F32)
    got = gpu_ctx.closest_point(q, counters=True)
    _same(got, _miss_records(q[:, 3]))
    st = gpu_ctx.stats()
    assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(q)
    _same(got, cc.brute_force(soup, q))
    good = np.array([[0, 0, -3, INF]], F32)  # the same position with a radius walks
    gpu_ctx.closest_point(good, counters=True)
    assert gpu_ctx.stats()["node_visits"] > 0


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_sponza_answers_do_not_depend_on_the_tree(gpu_ctx, sponza, sponza_points):
    """The device-built tree and the host builder's quality tree give the same bytes; 256 of the points (near-surface and scattered)
    are held to the statement."""
    gpu_ctx.upload_scene(sponza)
    device_tree = gpu_ctx.closest_point(sponza_points)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    _same(gpu_ctx.closest_point(sponza_points), device_tree)
    pick = np.arange(0, len(sponza_points), 8)
    assert len(pick) == 256
    _same(device_tree[pick], cc.brute_force(sponza, sponza_points[pick], prefilter=True))
    assert (api.split_nearest(device_tree)[4] != cc.PRIM_MISS).all()


def test_sponza_refit_answers_are_a_fresh_uploads(gpu_ctx, sponza, sponza_points):
    """After rt_update_geometry (a refit of the quality tree, seeded displacement) the answers are those of a fresh upload of the
    moved scene, and not those of the scene before."""
    pos = np.ascontiguousarray(sponza.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.02, pos.shape)).astype(F32)
    v = sponza.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(sponza, vertices=v)
    gpu_ctx.upload_scene(sponza)
    before = gpu_ctx.closest_point(sponza_points)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.update_geometry(moved_pos)["flags"] == api.STAT_REFIT
    refitted = gpu_ctx.closest_point(sponza_points)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        _same(refitted, fresh.closest_point(sponza_points))
    assert (refitted.view(np.uint32) != before.view(np.uint32)).any(1).mean() > 0.9


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_the_walk_culls(gpu_ctx, soup):
    """A walk that skips nothing passes every equality above: against the brute force's n x n_tris triangle tests the walk makes
    fewer than a tenth."""
    points = api.make_points(cc.near_surface(soup, 2048, 31))
    gpu_ctx.upload_scene(soup)
    gpu_ctx.closest_point(points, counters=True)
    st = gpu_ctx.stats()
    n, n_tris = len(points), len(soup.triangles)
    print(f"soup, {n} near-surface points: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} triangle tests per query "
          f"(brute force: {n_tris})")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * n_tris / 10


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_side_effects_empty_scene_and_call_order(gpu_ctx, soup, soup_points, soup_want):
    with pytest.raises(api.RtError) as e:
        gpu_ctx.closest_point(soup_points)
    assert e.value.code == -4, "RT_ERR_NOT_UPLOADED before an upload"
    gpu_ctx.upload_scene(soup)
    assert gpu_ctx.closest_point(np.zeros((0, 4), F32)).shape == (0, 8)
    lib, one = gpu_ctx.lib, np.zeros((1, 8), F32)
    import ctypes as C
    assert lib.rt_closest_point(gpu_ctx._h, None, C.c_size_t(1), C.c_void_p(one.ctypes.data), C.c_uint32(0)) == -1
    assert lib.rt_closest_point(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), None, C.c_uint32(0)) == -1
    assert lib.rt_closest_point(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), C.c_void_p(one.ctypes.data), C.c_uint32(2)) == -1, "unknown flag"
    assert lib.rt_closest_point(gpu_ctx._h, None, C.c_size_t(0), None, C.c_uint32(0)) == 0
    # the last frame and a running accumulation are left alone
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    _same(gpu_ctx.closest_point(soup_points), soup_want[0])
    _same(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4, "the running image went on"
    # an empty scene: all misses
    gpu_ctx.upload_scene(scenes.empty_scene())
    _same(gpu_ctx.closest_point(soup_points), _miss_records(soup_points[:, 3]))


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_a_context_over_one_device_twice_gives_the_same_bytes(soup, soup_points, soup_want):
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.closest_point(soup_points), soup_want[0])
        ctx.closest_point(soup_points, counters=True)
        assert ctx.stats()["rays"] == len(soup_points) and ctx.stats()["tri_tests"] > 0


def test_two_devices_give_the_one_device_bytes(soup, soup_points, soup_want):
    if torch is None or torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.closest_point(soup_points), soup_want[0])
        dev = torch.from_numpy(soup_points).to("cuda:1")
        _same(ctx.closest_point(dev).cpu().numpy(), soup_want[0])
