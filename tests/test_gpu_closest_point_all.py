"""Nearest-K queries on the MI355X (rt_closest_point_all).  Every comparison with the float32 statement (closest_point_all_cases.py's
numpy sort over all triangles and spheres) is byte for byte, records and counts: the result is the K smallest elements of a totally
ordered set, so it is the statement's whatever tree, memory, batch size or device count is in use."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import closest_point_all_cases as ca
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
KS = (1, 2, 4, 16)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _same_counts(got, want):
    np.testing.assert_array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64))


def _miss_records(radius, k):
    rec = np.zeros((len(radius), k), T.NEAREST)
    rec["distance"] = np.asarray(radius, F32)[:, None]
    rec["prim_id"] = cc.PRIM_MISS
    return rec.view(F32).reshape(len(radius), k, 8)


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_points(soup):
    """2048 points of the four kinds with radius 0.1, 0.25, 0.5, inf by index."""
    p = api.make_points(cc.four_kinds(soup, 2048, 11))
    p[:, 3] = np.array([0.1, 0.25, 0.5, np.inf], F32)[np.arange(len(p)) % 4]
    p.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def soup_want(soup, soup_points):
    """The statement at K = 16, computed once: (records (N, 16, 8), total counts); ca.first_k gives every smaller K."""
    rec, _, total = ca.nearest_all(soup, soup_points)
    rec.setflags(write=False)
    total.setflags(write=False)
    return rec, total


@pytest.fixture(scope="module")
def finite(soup_points):
    return np.flatnonzero(np.isfinite(soup_points[:, 3]))


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_the_batch_fills_and_overflows_its_lists(soup_want):
    """A batch that never fills or never overflows a list proves nothing: at K = 4 and at K = 16 more than 5 % of the queries hold
    some but fewer than K candidates, and more than 5 % hold more than K."""
    _, total = soup_want
    for k in (4, 16):
        short, over = ((total > 0) & (total < k)).mean(), (total > k).mean()
        print(f"K = {k}: {short:.1%} of the queries with 1 .. {k - 1} candidates, {over:.1%} with more than {k}, {(total == 0).mean():.1%} with none")
        assert short > 0.05 and over > 0.05


@pytest.mark.parametrize("k", KS)
def test_soup_equals_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_points, soup_want, k):
    want, want_counts = ca.first_k(*soup_want, k)
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.closest_point_all(soup_points, k)
    assert out.shape == (len(soup_points), k, 8) and counts.dtype == np.uint32
    _same(out, want)
    _same_counts(counts, want_counts)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_points) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["kernel_ms"] > 0
    own, own_counts = np.full((len(soup_points), k, 8), 7.0, F32), np.full(len(soup_points), 77, np.uint32)
    got = gpu_ctx.closest_point_all(soup_points, k, out=own, counts=own_counts)
    assert got[0] is own and got[1] is own_counts
    _same(own, want)
    _same_counts(own_counts, want_counts)
    if torch is None:
        pytest.skip("torch is not installed: device memory not exercised")
    dev = torch.from_numpy(np.array(soup_points)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    out, counts = gpu_ctx.closest_point_all(dev, k)
    assert out.device == dev.device and out.dtype == torch.float32 and counts.dtype == torch.int32 and tuple(out.shape) == (len(soup_points), k, 8)
    _same(out.cpu().numpy(), want)
    _same_counts(counts.cpu().numpy(), want_counts)
    pre, pre_counts = torch.empty((len(soup_points), k, 8), device="cuda:0"), torch.empty(len(soup_points), dtype=torch.int32, device="cuda:0")
    got = gpu_ctx.closest_point_all(dev, k, out=pre, counts=pre_counts)
    assert got[0] is pre and got[1] is pre_counts
    _same(pre.cpu().numpy(), want)
    _same_counts(pre_counts.cpu().numpy(), want_counts)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_one_is_closest_point_and_record_zero_is_too(gpu_ctx, soup, soup_points):
    """K = 1: rt_closest_point's bytes, node visits and triangle tests.  K = 16: record 0 is that record."""
    gpu_ctx.upload_scene(soup)
    single = gpu_ctx.closest_point(soup_points, counters=True)
    st1 = gpu_ctx.stats()
    out, counts = gpu_ctx.closest_point_all(soup_points, 1, counters=True)
    st = gpu_ctx.stats()
    _same(out[:, 0], single)
    _same_counts(counts, api.split_nearest(single)[4] != cc.PRIM_MISS)
    assert st1["node_visits"] > 0 and st1["tri_tests"] > 0
    assert (st["node_visits"], st["tri_tests"], st["rays"]) == (st1["node_visits"], st1["tri_tests"], len(soup_points))
    out16, _ = gpu_ctx.closest_point_all(soup_points, 16)
    _same(out16[:, 0], single)


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_boundaries(gpu_ctx, soup, soup_points, soup_want, n):
    want, want_counts = ca.first_k(*soup_want, 4)
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.closest_point_all(np.ascontiguousarray(soup_points[:n]), 4)
    _same(out, want[:n])
    _same_counts(counts, want_counts[:n])


# 4 ------------------------------------------------------------------------------------------------------------------------
def _tie_cases():
    """(scene, points): the tripled triangle, the sphere and the triangle at equal dist2, and coplanar walls sharing edges, with points
    above shared edges, shared corners and the squares' diagonals."""
    rng = np.random.default_rng(5)
    over = np.concatenate([rng.uniform(-0.5, 1.5, (61, 2)), np.full((61, 1), 2.0)], 1)
    over = np.concatenate([over, [[0.25, 0.25, 2.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.5]]]).astype(F32)
    t = np.linspace(0.0, 1.0, 33).astype(F32)
    zero, one = np.zeros_like(t), np.ones_like(t)
    walls = np.concatenate([np.stack([one, t, 0.5 * one], 1),        # above the edge the two floor squares share: four triangles meet at its ends
                            np.stack([t, t, 0.25 * one], 1),         # above the first square's diagonal
                            np.stack([one + t, t, 0.75 * one], 1),   # above the second square's
                            np.stack([1.5 * one, t, 0.5 * one], 1),  # as far from the floor as from the wall
                            np.stack([2 * one, t, zero], 1),         # on the edge the wall stands on
                            [[1, 0, 0], [1, 1, 0], [2, 0, 0], [2, 1, 0], [1, 0, 1], [2, 1, 1]]]).astype(F32)
    return {"tripled": (ca.tripled_triangle(), over),
            "sphere_triangle": (ca.sphere_and_triangle_tie(), np.array([[0, 0, 0], [0, 0, 0.5], [0.5, 0.25, 0], [3, 3, 0], [0, 0, 2]], F32)),
            "walls": (ca.coplanar_walls(), walls)}


@pytest.mark.parametrize("quality_tree", [False, True], ids=["device_tree", "quality_tree"])
@pytest.mark.parametrize("case", ["tripled", "sphere_triangle", "walls"])
def test_exact_ties_across_the_k_boundary(gpu_ctx, case, quality_tree):
    """Candidates that are equal in dist2 bit for bit, more of them than the list holds: the lower key stays, whatever order the walk
    meets them in."""
    scene, pos = _tie_cases()[case]
    points = api.make_points(pos)
    rec, _, total = ca.nearest_all(scene, points)
    d2 = np.concatenate([cc.sphere_candidates(np.ascontiguousarray(scene.spheres["center"], F32).reshape(-1, 3), scene.spheres["radius"].astype(F32), points[:, :3])[0],
                         cc.triangle_candidates(*cc.records(scene)[:3], points[:, :3])[0]], 1)
    srt = np.sort(d2, 1)
    ks = [k for k in (1, 2, 3, 4) if k < d2.shape[1] and (srt[:, k - 1] == srt[:, k]).any()]  # the K with a tie across the boundary
    assert ks == {"tripled": [1, 2], "sphere_triangle": [1], "walls": [1, 2, 3, 4]}[case]
    gpu_ctx.upload_scene(scene)
    if quality_tree:
        gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    for k in (1, 2, 3, 4, 16):
        want, want_counts = ca.first_k(rec, total, k)
        out, counts = gpu_ctx.closest_point_all(points, k)
        _same(out, want)
        _same_counts(counts, want_counts)
    _same(gpu_ctx.closest_point(points), rec[:, 0])


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_the_radius_is_strict_on_both_sides(gpu_ctx, soup, soup_points, soup_want):
    """From the dist2 of each point's j-th candidate (j = 3, or its last where it has fewer): the smallest radius with r * r > dist2
    lists that candidate, the largest with r * r <= dist2 lists the candidates strictly nearer and not that one; in both cases the
    count is that of the candidates with dist2 < r * r."""
    rec, total = soup_want
    p = np.array(soup_points[total >= 1])
    j = np.minimum(total[total >= 1], 4) - 1
    rows = np.arange(len(p))
    p[:, 3] = INF
    gpu_ctx.upload_scene(soup)
    full, _ = gpu_ctx.closest_point_all(p, 16)
    prims = full[:, :, 6].copy().view(np.uint32)
    n_sph = len(soup.spheres)
    all_d2 = np.concatenate([cc.sphere_candidates(np.ascontiguousarray(soup.spheres["center"], F32), soup.spheres["radius"].astype(F32), p[:, :3])[0],
                             cc.triangle_candidates(*cc.records(soup)[:3], p[:, :3])[0]], 1)
    pj = prims[rows, j].astype(np.int64)
    dist2 = all_d2[rows, np.where(pj >= cc.SPHERE_FLAG, pj - cc.SPHERE_FLAG, pj + n_sph)]  # the statement's dist2 of candidate j, whose root the record carries
    assert (np.sqrt(dist2) == full[rows, j, 3]).all()
    with np.errstate(all="ignore"):
        above = np.maximum(np.sqrt(dist2), F32(3e-23))  # (3e-23)^2 is the smallest subnormal: above dist2 = 0
        for _ in range(4):
            above = np.where(above * above > dist2, above, np.nextafter(above, INF))
        below = np.sqrt(dist2)
        for _ in range(4):
            below = np.where(below * below <= dist2, below, np.nextafter(below, -INF))
        assert (above * above > dist2).all() and (below * below <= dist2).all()
        assert (np.nextafter(above, -INF) ** 2 <= dist2)[dist2 > 1e-30].all() and (np.nextafter(below, INF) ** 2 > dist2)[dist2 > 1e-30].all(), "adjacent"
        n_above, n_below = (all_d2 < (above * above)[:, None]).sum(1), (all_d2 < (below * below)[:, None]).sum(1)
    assert (n_above > j).all() and (n_below <= j).all() and (n_below > 0).any() and (n_below == 0).any()
    for radius, count in ((above, n_above), (below, n_below)):
        q = p.copy()
        q[:, 3] = radius
        out, counts = gpu_ctx.closest_point_all(q, 16, count_all=True)
        _same_counts(counts, count)
        _same(out, np.where((np.arange(16)[None] < count[:, None])[..., None], full, _miss_records(radius, 16)))


def test_degenerate_queries_are_misses_without_a_walk(gpu_ctx, soup):
    gpu_ctx.upload_scene(soup)
    nan = F32(np.nan)
    q = np.array([[nan, 0, -3, INF], [0, nan, -3, 1], [0, 0, nan, 1], [INF, 0, -3, INF], [0, -INF, -3, INF], [0, 0, INF, 2],
                  [0, 0, -3, nan], [0, 0, -3, 0.0], [0, 0, -3, -0.0], [0, 0, -3, -1.0], [0, 0, -3, -INF]], F32)
    for k, count_all in ((4, False), (16, True), (1, False)):
        out, counts = gpu_ctx.closest_point_all(q, k, count_all=count_all, counters=True)
        _same(out, _miss_records(q[:, 3], k))
        _same_counts(counts, np.zeros(len(q)))
        st = gpu_ctx.stats()
        assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(q)
    _same(out, ca.nearest_all(soup, q, 1)[0])
    good = np.array([[0, 0, -3, INF]], F32)  # the same position with a radius walks
    gpu_ctx.closest_point_all(good, 4, counters=True)
    assert gpu_ctx.stats()["node_visits"] > 0


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_count_all_counts_everything_in_range_and_lists_the_same(gpu_ctx, soup, soup_points, soup_want, finite):
    """Finite radii only: with an infinite one the flag tests the whole scene for every point."""
    rec, total = soup_want
    points = np.ascontiguousarray(soup_points[finite])
    gpu_ctx.upload_scene(soup)
    none, counts = gpu_ctx.closest_point_all(points, 0, count_all=True)
    assert none is None
    _same_counts(counts, total[finite])
    assert (total[finite] > 16).any()
    out, counts = gpu_ctx.closest_point_all(points, 4, count_all=True)
    _same(out, ca.first_k(rec, total, 4)[0][finite])
    _same_counts(counts, total[finite])
    plain, listed = gpu_ctx.closest_point_all(points, 4)
    _same(plain, out)
    _same_counts(listed, np.minimum(total[finite], 4))


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_tree(gpu_ctx, soup, soup_points, soup_want):
    want, want_counts = ca.first_k(*soup_want, 16)
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.closest_point_all(soup_points, 16)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    out_q, counts_q = gpu_ctx.closest_point_all(soup_points, 16)
    _same(out_q, out)
    _same_counts(counts_q, counts)
    _same(out_q, want)
    _same_counts(counts_q, want_counts)


def test_refit_results_are_a_fresh_uploads(gpu_ctx, soup, soup_points):
    """After rt_update_geometry (a refit, jittered vertices) the lists are those of a fresh upload of the moved scene, and not those of
    the scene before."""
    pos = np.ascontiguousarray(soup.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.02, pos.shape)).astype(F32)
    v = soup.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(soup, vertices=v)
    gpu_ctx.upload_scene(soup)
    before, _ = gpu_ctx.closest_point_all(soup_points, 16)
    assert gpu_ctx.update_geometry(moved_pos)["flags"] == api.STAT_REFIT
    refitted, refitted_counts = gpu_ctx.closest_point_all(soup_points, 16)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        out, counts = fresh.closest_point_all(soup_points, 16)
    _same(refitted, out)
    _same_counts(refitted_counts, counts)
    assert (refitted.view(np.uint32) != before.view(np.uint32)).any((1, 2)).mean() > 0.5


# 8 ------------------------------------------------------------------------------------------------------------------------
TESTS_PER_QUERY_BOUND = 400  # about three times the measurement in the docstring below


def test_the_walk_culls(gpu_ctx, soup):
    """A walk that skips nothing passes every equality above.  K = 16, radius = inf, 2048 near-surface points: the brute force makes
    3000 triangle tests per query.  Measured on the MI355X, device-built tree: 73.0 node visits and 135.2 triangle tests per query
    (rt_closest_point on the same points: see test_gpu_closest_point.py); the host check's soup of 20000 makes 66.2 at K = 16 over its
    mix of points.  The bound is about three times the measurement, to allow for another tree of the same scene."""
    points = api.make_points(cc.near_surface(soup, 2048, 31))
    gpu_ctx.upload_scene(soup)
    gpu_ctx.closest_point_all(points, 16, counters=True)
    st = gpu_ctx.stats()
    n, n_tris = len(points), len(soup.triangles)
    print(f"soup, {n} near-surface points, K = 16: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} triangle tests per query "
          f"(brute force: {n_tris})")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * TESTS_PER_QUERY_BOUND


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(gpu_ctx, soup, soup_points, soup_want):
    n = 8
    points = np.array(soup_points[:n])
    out, counts = np.full((n, 17, 8), 7.0, F32), np.full(n, 77, np.uint32)
    lib, h = gpu_ctx.lib, gpu_ctx._h

    def call(p, k, o, c, flags, m=n):
        return lib.rt_closest_point_all(h, C.c_void_p(p), C.c_size_t(m), C.c_uint32(k), C.c_void_p(o), C.c_void_p(c), C.c_uint32(flags))

    P, O, Cn = points.ctypes.data, out.ctypes.data, counts.ctypes.data
    assert call(P, 4, O, Cn, 0) == -4, "RT_ERR_NOT_UPLOADED before an upload"
    with pytest.raises(api.RtError) as e:
        gpu_ctx.closest_point_all(points, 4)
    assert e.value.code == -4
    gpu_ctx.upload_scene(soup)
    gpu_ctx.closest_point_all(points, 2)
    before = gpu_ctx.stats()
    assert call(P, 17, O, Cn, 0) == -1                              # max_nearest > RT_NEAREST_MAX
    assert call(P, 0, O, Cn, 0) == -1                               # max_nearest == 0 without RT_QUERY_COUNT_ALL
    assert call(P, 0, O, None, api.QUERY_COUNT_ALL) == -1           # ... without counts
    assert call(None, 4, O, Cn, 0) == -1 and call(P, 4, None, Cn, 0) == -1
    assert call(P, 4, O, Cn, 4) == -1 and call(P, 4, O, Cn, 0x80000000) == -1, "unknown flag bits"
    assert (out == 7.0).all() and (counts == 77).all()
    assert gpu_ctx.stats()["rays"] == before["rays"] == n
    assert call(None, 4, None, None, 0, m=0) == 0, "n == 0 is RT_OK"
    assert call(P, 4, O, None, 0) == 0, "counts may be NULL with max_nearest > 0"
    _same(out.reshape(-1)[:n * 4 * 8].reshape(n, 4, 8), ca.first_k(*soup_want, 4)[0][:n])
    assert gpu_ctx.closest_point_all(np.zeros((0, 4), F32), 4)[0].shape == (0, 4, 8)
    if torch is None:
        pytest.skip("torch is not installed: mixed memory kinds not exercised")
    dev = torch.from_numpy(points).to("cuda:0")
    dout, dcounts = torch.full((n, 4, 8), 7.0, device="cuda:0"), torch.full((n,), 77, dtype=torch.int32, device="cuda:0")
    assert call(dev.data_ptr(), 4, O, Cn, 0) == -1 and call(P, 4, dout.data_ptr(), Cn, 0) == -1 and call(dev.data_ptr(), 4, dout.data_ptr(), Cn, 0) == -1
    assert call(P, 4, O, dcounts.data_ptr(), 0) == -1, "mixed host and device buffers"
    assert (dout == 7.0).all() and (dcounts == 77).all()
    buf = torch.zeros(n * 4 + 1, device="cuda:0")  # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    with pytest.raises(api.RtError) as e:
        gpu_ctx.closest_point_all(buf[1:].view(-1, 4), 4)
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.closest_point_all(dev, 4)[0].cpu().numpy(), ca.first_k(*soup_want, 4)[0][:n])


def test_side_effects_and_an_empty_scene(gpu_ctx, soup, soup_points, soup_want):
    want, want_counts = ca.first_k(*soup_want, 4)
    gpu_ctx.upload_scene(soup)
    # the last frame and a running accumulation are left alone
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    out, counts = gpu_ctx.closest_point_all(soup_points, 4)
    _same(out, want)
    _same_counts(counts, want_counts)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_points) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["shadow_rays"] == 0
    _same(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4, "the running image went on"
    # an empty scene: all misses, counts of 0
    gpu_ctx.upload_scene(scenes.empty_scene())
    for k in (1, 16):
        out, counts = gpu_ctx.closest_point_all(soup_points, k, count_all=True)
        _same(out, _miss_records(soup_points[:, 3], k))
        _same_counts(counts, np.zeros(len(soup_points)))
    _same(gpu_ctx.closest_point_all(soup_points, 1)[0][:, 0], gpu_ctx.closest_point(soup_points))


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_a_context_over_one_device_twice_gives_the_same_bytes(soup, soup_points, soup_want):
    want, want_counts = ca.first_k(*soup_want, 16)
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(soup)
        out, counts = ctx.closest_point_all(soup_points, 16)
        _same(out, want)
        _same_counts(counts, want_counts)
        ctx.closest_point_all(soup_points, 16, counters=True)
        assert ctx.stats()["rays"] == len(soup_points) and ctx.stats()["tri_tests"] > 0


def test_two_devices_give_the_one_device_bytes(soup, soup_points, soup_want):
    if torch is None or torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    want, want_counts = ca.first_k(*soup_want, 16)
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        out, counts = ctx.closest_point_all(soup_points, 16)
        _same(out, want)
        _same_counts(counts, want_counts)
        dev = torch.from_numpy(np.array(soup_points)).to("cuda:1")
        out, counts = ctx.closest_point_all(dev, 16)
        _same(out.cpu().numpy(), want)
        _same_counts(counts.cpu().numpy(), want_counts)
