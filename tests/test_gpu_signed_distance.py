"""Inside tests and signed distance on the MI355X (rt_inside, rt_signed_distance).  Every comparison with the float32 statement
(signed_distance_cases.py: crossing counts over all triangles, the vote, closest_point_cases.brute_force's records with the sign) is
byte for byte - inside, votes, records and the number of rays traced: a vote is a count over all triangles of the scene, so the answer
is the statement's whatever tree, memory, batch size or device count is in use."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import closest_point_cases as cc
import signed_distance_cases as sd
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
NAN = F32(np.nan)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _same_bytes(got, want):
    np.testing.assert_array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64))


def _miss_records(radius):
    rec = np.zeros(len(radius), T.NEAREST)
    rec["distance"] = np.asarray(radius, F32)
    rec["prim_id"] = cc.PRIM_MISS
    return rec.view(F32).reshape(len(radius), 8)


def _without_spheres(scene):
    return dataclasses.replace(scene, spheres=np.zeros(0, T.SPHERE))


def _composed_parity(scene, positions, counters=False):
    """c_k & 1 of every point and direction, (N, 7), from rt_intersect_all(max_hits = 0, RT_QUERY_COUNT_ALL) over the statement's rays
    on the scene with its spheres removed; with `counters` also that call's (node visits, triangle tests) per direction."""
    rays = sd.inside_rays(positions)
    parity, walk = np.zeros((len(positions), 7), np.uint32), []
    with api.Context() as ctx:
        ctx.upload_scene(_without_spheres(scene))
        for k in range(7):
            parity[:, k] = ctx.intersect_all(np.ascontiguousarray(rays[k]), 0, count_all=True, counters=counters)[1] & 1
            walk.append((ctx.stats()["node_visits"], ctx.stats()["tri_tests"]))
    return (parity, walk) if counters else parity


# -- the closed scene: box + torus + two spheres ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def union():
    """(scene, points (N, 4) with radius inf, 0.25, 0.05, inf by index, the analytic truth, the statement's crossing counts)."""
    scene = sd.union_scene()
    pos, truth = sd.union_points()
    points = api.make_points(pos)
    points[:, 3] = np.array([np.inf, 0.25, 0.05, np.inf], F32)[np.arange(len(points)) % 4]
    counts = sd.crossings(scene, pos)
    for a in (points, truth, counts):
        a.setflags(write=False)
    return scene, points, truth, counts


@pytest.fixture(scope="module")
def union_records(union):
    scene, points, _, _ = union
    rec = cc.brute_force(scene, points)
    rec.setflags(write=False)
    return rec


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rays", [1, 3, 7])
def test_closed_shapes_equal_the_statement_and_the_analytic_truth(gpu_ctx, union, union_records, rays):
    scene, points, truth, counts = union
    assert truth.sum() > 400 and (~truth).sum() > 1000 and sd.sphere_inside(scene, points[:, :3]).sum() > 40
    gpu_ctx.upload_scene(scene)
    want_inside, want_votes, _ = sd.statement(scene, points, rays, True, counts=counts)
    inside, votes = gpu_ctx.inside(points, rays=rays, votes=True)
    assert inside.dtype == np.bool_ and votes.dtype == np.uint8 and inside.shape == votes.shape == (len(points),)
    _same_bytes(inside.view(np.uint8), want_inside)
    _same_bytes(votes, want_votes)
    _same_bytes(inside, truth)
    _same_bytes(gpu_ctx.inside(points, rays=rays).view(np.uint8), want_inside)
    want = sd.sign(union_records, want_inside)
    rec, votes = gpu_ctx.signed_distance(points, rays=rays, votes=True)
    _same(rec, want)
    _same_bytes(votes, want_votes)
    _same(gpu_ctx.signed_distance(points, rays=rays), want)
    d, prim = api.split_nearest(rec)[1], api.split_nearest(rec)[4]
    assert (np.signbit(d) == truth).all() and ((prim == cc.PRIM_MISS) & truth).any() and ((prim == cc.PRIM_MISS) & ~truth).any()
    assert (d[(prim == cc.PRIM_MISS)] == np.where(truth, -points[:, 3], points[:, 3])[prim == cc.PRIM_MISS]).all(), "-radius on an inside miss"
    st = gpu_ctx.stats()
    assert st["pixels"] == 0 and st["primary_rays"] == 0 and st["shadow_rays"] == 0 and st["node_visits"] == 0 and st["kernel_ms"] > 0


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_points(soup):
    p = api.make_points(cc.four_kinds(soup, 2048, 11))
    p[:, 3] = np.array([0.1, 0.25, 0.5, np.inf], F32)[np.arange(len(p)) % 4]
    p.setflags(write=False)
    return p


def test_the_soup_is_the_composition_of_the_existing_calls(gpu_ctx, soup, soup_points):
    """Not watertight, so the votes disagree: votes = the parities of rt_intersect_all's counts on the triangles alone, the records
    rt_closest_point's with the sign of `inside`, and the walk's counters the sum of the two calls'."""
    n = len(soup_points)
    parity, walk = _composed_parity(soup, soup_points[:, :3], counters=True)
    gpu_ctx.upload_scene(soup)
    in_sphere = sd.sphere_inside(soup, soup_points[:, :3])
    assert 0 < in_sphere.sum() < n
    unsigned = gpu_ctx.closest_point(soup_points, counters=True)
    st_cp = gpu_ctx.stats()
    for rays in (1, 3, 5, 7):
        inside, votes = gpu_ctx.inside(soup_points, rays=rays, votes=True)
        _same_bytes(votes, parity[:, :rays].sum(1))
        _same_bytes(inside, in_sphere | (votes.astype(np.int64) * 2 > rays))
        rec, votes_d = gpu_ctx.signed_distance(soup_points, rays=rays, votes=True, counters=True)
        st = gpu_ctx.stats()
        _same_bytes(votes_d, votes)
        want = unsigned.copy()
        want.view(np.uint32)[:, 3] ^= inside.astype(np.uint32) << np.uint32(31)
        _same(rec, want)
        assert st["rays"] == n * rays
        assert st["node_visits"] == st_cp["node_visits"] + sum(w[0] for w in walk[:rays]) and st_cp["node_visits"] > 0 and walk[0][0] > 0
        assert st["tri_tests"] == st_cp["tri_tests"] + sum(w[1] for w in walk[:rays])
    split = (votes > 0) & (votes < 7)
    print(f"soup: {split.mean():.1%} of the points with split votes at 7 rays")
    assert split.mean() > 0.2, "the case is about disagreeing votes"
    gpu_ctx.inside(soup_points, rays=7, votes=True, counters=True)
    st = gpu_ctx.stats()
    assert st["node_visits"] == sum(w[0] for w in walk) and st["tri_tests"] == sum(w[1] for w in walk), "rt_inside walks the rays only"


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_boundaries(gpu_ctx, union, union_records, n):
    scene, points, _, counts = union
    gpu_ctx.upload_scene(scene)
    p = np.ascontiguousarray(points[:n])
    want_inside, want_votes, _ = sd.statement(scene, p, 3, True, counts=counts[:n])
    rec, votes = gpu_ctx.signed_distance(p, rays=3, votes=True)
    _same(rec, sd.sign(union_records[:n], want_inside))
    _same_bytes(votes, want_votes)
    _same_bytes(gpu_ctx.inside(p, rays=3), want_inside)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_spheres_alone_and_an_empty_scene(gpu_ctx):
    scene = sd.make_scene("spheres", [], [((0.0, 0.0, 0.0), 1.0), ((3.0, 0.0, 0.0), 0.5)])
    p = api.make_points(np.array([[0, 0, 0], [0.5, 0.5, 0.5], [0.999, 0, 0], [1, 0, 0], [1.5, 0, 0], [3, 0, 0], [3.2, 0.1, 0], [3, 0.5, 0], [0, 5, 0]], F32))
    want = [True, True, True, False, False, True, True, False, False]
    assert sd.sphere_inside(scene, p[:, :3]).tolist() == want
    gpu_ctx.upload_scene(scene)
    for rays in (1, 7):
        inside, votes = gpu_ctx.inside(p, rays=rays, votes=True)
        assert inside.tolist() == want and votes.tolist() == [0] * len(p) and gpu_ctx.stats()["rays"] == len(p) * rays
        assert gpu_ctx.inside(p, rays=rays).tolist() == want
        assert gpu_ctx.stats()["rays"] == (len(p) - sum(want)) * (rays // 2 + 1), "nothing traced inside a sphere, the majority elsewhere"
        rec, votes = gpu_ctx.signed_distance(p, rays=rays, votes=True)
        _same(rec, sd.sign(cc.brute_force(scene, p), np.array(want)))
        assert votes.tolist() == [0] * len(p) and api.split_nearest(rec)[1][0] == F32(-1.0), "the centre: the radius away, inside"
    gpu_ctx.upload_scene(scenes.empty_scene())
    p = api.make_points(np.array([[0, 0, 0], [1, 2, 3], [-4, 0, 0.5]], F32), radius=2.0)
    for with_votes in (False, True):
        got = gpu_ctx.inside(p, rays=5, votes=with_votes)
        inside, votes = got if with_votes else (got, np.zeros(3, np.uint8))
        assert inside.tolist() == [False] * 3 and votes.tolist() == [0] * 3
        got = gpu_ctx.signed_distance(p, rays=5, votes=with_votes, counters=True)
        rec, votes = got if with_votes else (got, np.zeros(3, np.uint8))
        _same(rec, _miss_records(p[:, 3]))
        assert votes.tolist() == [0] * 3 and gpu_ctx.stats()["node_visits"] == 0


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_queries_trace_nothing(gpu_ctx):
    scene = sd.make_scene("box", [sd.box_mesh()])
    gpu_ctx.upload_scene(scene)
    centre = [0.125, 0.0, -0.125]
    bad = np.array([[NAN, 0, 0, INF], [0, NAN, 0, 1], [0, 0, NAN, 1], [INF, 0, 0, INF], [0, -INF, 0, INF], [0, 0, INF, 2]], F32)
    rad = np.array([centre + [NAN], centre + [0.0], centre + [-0.0], centre + [-1.0], centre + [-INF]], F32)
    for rays in (1, 5):
        for q in (bad, rad):
            rec, votes = gpu_ctx.signed_distance(q, rays=rays, votes=True, counters=True)
            _same(rec, _miss_records(q[:, 3]))
            st = gpu_ctx.stats()
            assert votes.tolist() == [0] * len(q) and (st["rays"], st["node_visits"], st["tri_tests"]) == (0, 0, 0)
            _same(gpu_ctx.signed_distance(q, rays=rays), _miss_records(q[:, 3]))
        inside, votes = gpu_ctx.inside(bad, rays=rays, votes=True, counters=True)
        assert inside.tolist() == [False] * len(bad) and votes.tolist() == [0] * len(bad) and gpu_ctx.stats()["rays"] == 0 and gpu_ctx.stats()["node_visits"] == 0
        inside, votes = gpu_ctx.inside(rad, rays=rays, votes=True)  # rt_inside reads the position only
        assert inside.tolist() == [True] * len(rad) and votes.tolist() == [rays] * len(rad) and gpu_ctx.stats()["rays"] == rays * len(rad)
    # finite radii: a miss inside the box is -radius, outside +radius
    q = np.array([centre + [0.1], centre + [0.4999], [5, 5, 5, 0.1], [0.125, 0.8, -0.125, 0.25], centre + [0.6]], F32)
    rec, votes = gpu_ctx.signed_distance(q, rays=3, votes=True)
    _same(rec, sd.signed_records(scene, q, 3, True)[0])
    pos, d, _, _, prim, _ = api.split_nearest(rec)
    assert prim[:4].tolist() == [cc.PRIM_MISS] * 4 and prim[4] != cc.PRIM_MISS and votes.tolist() == [3, 3, 0, 0, 3]
    assert d[:4].tolist() == [F32(-0.1), F32(-0.4999), F32(0.1), F32(0.25)] and abs(d[4] + 0.5) < 1e-6


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_the_stop_rule(gpu_ctx, union):
    """Without a votes array: the same answers, fewer rays - the statement's count of them, on the closed scene (unanimous votes) and on
    the box without its top (split votes)."""
    scene, points, _, counts = union
    open_box = sd.make_scene("open box and a sphere", [sd.box_mesh(open_top=True)], [((0.5, 0.0, 0.0), 0.3)])
    open_points = api.make_points(sd.closed_shape_points(5)[0][::4])
    open_counts = sd.crossings(open_box, open_points[:, :3])
    split = (open_counts[:, :3] & 1).sum(1) % 3 != 0
    assert split.mean() > 0.05, "the case is about disagreeing votes"
    for sc, p, c in ((scene, points, counts), (open_box, open_points, open_counts)):
        gpu_ctx.upload_scene(sc)
        for rays in (1, 3, 5, 7):
            want_inside, want_votes, all_traced = sd.statement(sc, p, rays, True, counts=c)
            inside, votes = gpu_ctx.inside(p, rays=rays, votes=True)
            assert gpu_ctx.stats()["rays"] == all_traced.sum() == len(p) * rays
            _same_bytes(inside, want_inside)
            _same_bytes(votes, want_votes)
            early_inside, _, traced = sd.statement(sc, p, rays, False, counts=c)
            assert (early_inside == want_inside).all()
            _same_bytes(gpu_ctx.inside(p, rays=rays), want_inside)
            assert gpu_ctx.stats()["rays"] == traced.sum() and (rays == 1 or traced.sum() < all_traced.sum())
            dist_inside, _, traced_d = sd.statement(sc, p, rays, False, distance=True, counts=c)
            rec = gpu_ctx.signed_distance(p, rays=rays)
            assert gpu_ctx.stats()["rays"] == traced_d.sum()
            assert (np.signbit(api.split_nearest(rec)[1]) == dist_inside).all()


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_the_tree_does_not_matter(gpu_ctx):
    """sponza-like at its default size: its structural geometry alone has 191944 triangles, so the generator builds nothing smaller."""
    scene = scenes.sponza_like()
    pos = np.concatenate([cc.near_surface(scene, 1536, 3), cc.scattered(scene, 512, 4)])
    points = api.make_points(pos)
    points[:, 3] = np.array([np.inf, 0.5], F32)[np.arange(len(points)) % 2]
    parity = _composed_parity(scene, pos)
    gpu_ctx.upload_scene(scene)
    assert gpu_ctx.stats()["tree_build"] == 2, "the device-built tree"

    def answers():
        inside, votes = gpu_ctx.inside(points, rays=7, votes=True)
        rec, votes_d = gpu_ctx.signed_distance(points, rays=7, votes=True)
        return inside.view(np.uint8), votes, rec.view(np.uint32), votes_d, gpu_ctx.inside(points, rays=3).view(np.uint8)

    first = answers()
    _same_bytes(first[1], parity.sum(1))
    _same_bytes(first[0], first[1] > 3)
    _same_bytes(first[4], parity[:, :3].sum(1) > 1)
    assert 0.02 < first[0].mean() < 0.98
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    for a, b in zip(answers(), first):
        np.testing.assert_array_equal(a, b)
    assert gpu_ctx.update_geometry(np.ascontiguousarray(scene.vertices["position"], F32))["flags"] == api.STAT_REFIT
    for a, b in zip(answers(), first):
        np.testing.assert_array_equal(a, b)


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_torch_device_tensors_in_and_out(gpu_ctx, union, union_records):
    if torch is None:
        pytest.skip("torch is not installed: device memory not exercised")
    scene, points, _, counts = union
    n = len(points)
    want_inside, want_votes, _ = sd.statement(scene, points, 3, True, counts=counts)
    want = sd.sign(union_records, want_inside)
    gpu_ctx.upload_scene(scene)
    dev = torch.from_numpy(np.array(points)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    inside, votes = gpu_ctx.inside(dev, rays=3, votes=True)
    assert inside.device == dev.device and inside.dtype == torch.bool and votes.dtype == torch.uint8 and tuple(inside.shape) == tuple(votes.shape) == (n,)
    _same_bytes(inside.cpu().numpy(), want_inside)
    _same_bytes(votes.cpu().numpy(), want_votes)
    rec = gpu_ctx.signed_distance(dev, rays=3)
    assert rec.device == dev.device and rec.dtype == torch.float32 and tuple(rec.shape) == (n, 8)
    _same(rec.cpu().numpy(), want)
    # preallocated, the votes at an odd byte offset
    pre, pre_inside, bytes_ = torch.full((n, 8), 7.0, device="cuda:0"), torch.zeros(n, dtype=torch.bool, device="cuda:0"), torch.full((n + 1,), 77, dtype=torch.uint8, device="cuda:0")
    odd = bytes_[1:]
    assert odd.data_ptr() % 2 == 1
    got = gpu_ctx.signed_distance(dev, rays=3, out=pre, votes=odd)
    assert got[0] is pre and got[1] is odd
    _same(pre.cpu().numpy(), want)
    _same_bytes(odd.cpu().numpy(), want_votes)
    assert bytes_[0].item() == 77
    got = gpu_ctx.inside(dev, rays=3, out=pre_inside, votes=odd)
    assert got[0] is pre_inside
    _same_bytes(pre_inside.cpu().numpy(), want_inside)
    # records 4 bytes off 16-byte alignment are refused, and the context keeps working
    buf = torch.zeros(n * 8 + 1, device="cuda:0")
    with pytest.raises(api.RtError) as e:
        gpu_ctx.signed_distance(dev, rays=3, out=buf[1:].view(-1, 8))
    assert e.value.code == -1 and "aligned" in str(e.value)
    params, host_inside, host_votes = np.array([3, 0, 0, 0], np.uint32), np.full(n, 7, np.uint8), np.full(n, 77, np.uint8)
    for o, v in ((host_inside.ctypes.data, None), (pre_inside.data_ptr(), host_votes.ctypes.data)):  # mixed host and device arrays
        assert gpu_ctx.lib.rt_inside(gpu_ctx._h, C.c_void_p(dev.data_ptr()), C.c_size_t(n), C.c_void_p(params.ctypes.data), C.c_void_p(o), C.c_void_p(v)) == -1
    assert (host_inside == 7).all() and (host_votes == 77).all()
    _same(gpu_ctx.signed_distance(dev, rays=3).cpu().numpy(), want)


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_a_host_batch_longer_than_a_chunk_equals_its_halves(gpu_ctx):
    """rays = 7: a chunk is RT_QUERY_CHUNK // 7 points."""
    scene = sd.make_scene("box", [sd.box_mesh()])
    n = api.QUERY_CHUNK // 7 + 100
    rng = np.random.default_rng(9)
    points = api.make_points(((sd.BOX_LO - 0.5) + rng.random((n, 3)) * (sd.BOX_HI - sd.BOX_LO + 1.0)).astype(F32), radius=0.3)
    gpu_ctx.upload_scene(scene)
    rec, votes = gpu_ctx.signed_distance(points, rays=7, votes=True)
    assert gpu_ctx.stats()["rays"] == 7 * n
    h = n // 2
    for sl in (slice(0, h), slice(h, n)):
        part, part_votes = gpu_ctx.signed_distance(np.ascontiguousarray(points[sl]), rays=7, votes=True)
        _same(rec[sl], part)
        _same_bytes(votes[sl], part_votes)
    tail = slice(api.QUERY_CHUNK // 7 - 50, n)  # across the chunk's end, held to the statement
    want_rec, want_votes, _ = sd.signed_records(scene, points[tail], 7, True)
    _same(rec[tail], want_rec)
    _same_bytes(votes[tail], want_votes)
    assert (votes == 0).any() and (votes == 7).any()
    inside = gpu_ctx.inside(points, rays=7)
    _same_bytes(inside, votes > 3)
    assert 4 * n <= gpu_ctx.stats()["rays"] < 7 * n, "a majority of seven takes four rays at least"


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_a_context_over_one_device_twice_gives_the_same_bytes(union, union_records):
    scene, points, _, counts = union
    want_inside, want_votes, traced = sd.statement(scene, points, 5, False, counts=counts)
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(scene)
        rec, votes = ctx.signed_distance(points, rays=5, votes=True, counters=True)
        _same(rec, sd.sign(union_records, want_inside))
        _same_bytes(votes, want_votes)
        assert ctx.stats()["rays"] == 5 * len(points) and ctx.stats()["tri_tests"] > 0
        _same_bytes(ctx.inside(points, rays=5), want_inside)
        assert ctx.stats()["rays"] == traced.sum()


def test_two_devices_give_the_one_device_bytes(union, union_records):
    if torch is None or torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    scene, points, _, counts = union
    want_inside, want_votes, _ = sd.statement(scene, points, 5, True, counts=counts)
    want = sd.sign(union_records, want_inside)
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(scene)
        rec, votes = ctx.signed_distance(points, rays=5, votes=True)
        _same(rec, want)
        _same_bytes(votes, want_votes)
        assert ctx.stats()["rays"] == 5 * len(points)
        dev = torch.from_numpy(np.array(points)).to("cuda:1")
        inside, votes = ctx.inside(dev, rays=5, votes=True)
        _same_bytes(inside.cpu().numpy(), want_inside)
        _same_bytes(votes.cpu().numpy(), want_votes)


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_a_running_accumulation_is_left_alone(gpu_ctx, soup, soup_points):
    gpu_ctx.upload_scene(soup)
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    inside, votes = gpu_ctx.inside(soup_points, rays=3, votes=True)
    rec = gpu_ctx.signed_distance(soup_points, rays=3)
    st = gpu_ctx.stats()
    assert 0 < st["rays"] <= 3 * len(soup_points) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["shadow_rays"] == 0
    assert (np.signbit(api.split_nearest(rec)[1]) == inside).all()
    _same(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4, "the running image went on"


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(gpu_ctx, union):
    scene, points, _, _ = union
    n = 8
    p = np.array(points[:n])
    inside, votes, out = np.full(n, 7, np.uint8), np.full(n, 77, np.uint8), np.full((n, 8), 7.0, F32)
    lib, h = gpu_ctx.lib, gpu_ctx._h

    def params(rays, flags=0):
        return np.array([rays, flags, 0, 0], np.uint32)

    def call(fn, pts, prm, o, v, m=n):
        return getattr(lib, fn)(h, C.c_void_p(pts), C.c_size_t(m), C.c_void_p(prm.ctypes.data if prm is not None else None), C.c_void_p(o), C.c_void_p(v))

    P, I, V, O = p.ctypes.data, inside.ctypes.data, votes.ctypes.data, out.ctypes.data
    assert call("rt_inside", P, params(3), I, V) == -4 and call("rt_signed_distance", P, params(3), O, V) == -4, "RT_ERR_NOT_UPLOADED before an upload"
    gpu_ctx.upload_scene(scene)
    gpu_ctx.inside(p, rays=1, votes=True)
    before = gpu_ctx.stats()
    for fn, o in (("rt_inside", I), ("rt_signed_distance", O)):
        for rays in (0, 2, 4, 6, 8, 9, 0xFFFFFFFF):
            assert call(fn, P, params(rays), o, V) == -1, rays
        assert call(fn, P, params(3, 2), o, V) == -1 and call(fn, P, params(3, 0x80000000), o, V) == -1, "flag bits other than RT_QUERY_COUNTERS"
        assert call(fn, None, params(3), o, V) == -1 and call(fn, P, None, o, V) == -1 and call(fn, P, params(3), None, V) == -1
        assert call(fn, None, None, None, None, m=0) == 0, "n == 0 is RT_OK"
    assert (inside == 7).all() and (votes == 77).all() and (out == 7.0).all()
    assert gpu_ctx.stats()["rays"] == before["rays"] == n
    assert call("rt_inside", P, params(3, api.QUERY_COUNTERS), I, None) == 0, "votes may be NULL"
    assert (votes == 77).all() and set(inside.tolist()) <= {0, 1}
    assert gpu_ctx.inside(np.zeros((0, 4), F32)).shape == (0,) and gpu_ctx.signed_distance(np.zeros((0, 4), F32)).shape == (0, 8)
