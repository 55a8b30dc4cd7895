"""Sphere sweeps on the MI355X (rt_sweep_sphere).  Every comparison with the float32 statement (sweep_cases.py's numpy brute force
over all triangles and spheres) is byte for byte: the tree only culls, so the answer is the statement's whatever tree, memory,
batch size or device count is in use."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import closest_point_cases as cc
import sweep_cases as sc
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first; these tests need it

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


def _same(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _miss_records(tmax):
    rec = np.zeros(len(tmax), T.SWEEP_HIT)
    rec["t"] = tmax
    rec["prim_id"] = sc.PRIM_MISS
    return rec.view(F32).reshape(-1, 8)


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_sweeps(soup):
    """4000 sweeps of the five kinds (tmax = inf), then sweeps toward each sphere, and from inside each sphere outward."""
    rng = np.random.default_rng(21)
    c, r = soup.spheres["center"].astype(np.float64), soup.spheres["radius"].astype(np.float64)
    n = 16 * len(c)
    centre, radius = np.repeat(c, 16, 0), np.repeat(r, 16)
    away = sc._unit(rng, n)
    outside = sc._pack(centre + away * (radius + rng.uniform(0.5, 2.0, n))[:, None], -away * rng.uniform(0.2, 5.0, (n, 1)), rng.uniform(0.01, 0.3, n))
    inside = sc._pack(centre + sc._unit(rng, n) * (radius * rng.uniform(0.0, 0.6, n))[:, None], sc._unit(rng, n), radius * rng.uniform(0.05, 0.3, n))
    sweeps = np.concatenate([sc.five_kinds(soup, 4000, 11), outside, inside])
    sweeps.setflags(write=False)
    return sweeps


@pytest.fixture(scope="module")
def soup_want(soup, soup_sweeps):
    """The statement's answers, computed once (the prefiltered brute force, which test_sweep_abi.py holds to the plain one)."""
    rec = sc.brute_force(soup, soup_sweeps, prefilter=True)
    rec.setflags(write=False)
    return rec


@pytest.fixture(scope="module")
def sponza():
    return scenes.sponza_like()


@pytest.fixture(scope="module")
def sponza_sweeps(sponza):
    return np.concatenate([sc.toward_surfaces(sponza, 1024, 3), sc.scattered(sponza, 1024, 4)])


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_soup_equals_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_sweeps, soup_want):
    face, edge, vertex, sphere, at_start, miss = sc.contact_kinds(soup_want)
    moving = ~at_start
    print("soup:", {k: int(v.sum()) for k, v in dict(face=face & moving, edge=edge & moving, vertex=vertex & moving, sphere=sphere & moving,
                                                     at_start=at_start, miss=miss).items()})
    assert (face & moving).sum() >= 100 and (edge & moving).sum() >= 100 and (vertex & moving).sum() >= 100 and (sphere & moving).sum() >= 20
    assert at_start.sum() >= 100 and miss.sum() >= 100
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_sphere(soup_sweeps), soup_want)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_sweeps) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["kernel_ms"] > 0
    own = np.full((len(soup_sweeps), 8), 7.0, F32)
    assert gpu_ctx.sweep_sphere(soup_sweeps, out=own) is own
    _same(own, soup_want)
    dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    got = gpu_ctx.sweep_sphere(dev)
    assert got.device == dev.device and got.dtype == torch.float32
    _same(got.cpu().numpy(), soup_want)
    out = torch.empty((len(soup_sweeps), 8), device="cuda:0")
    assert gpu_ctx.sweep_sphere(dev, out=out) is out
    _same(out.cpu().numpy(), soup_want)
    # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    buf = torch.zeros(len(soup_sweeps) * 8 + 1, device="cuda:0")
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_sphere(buf[1:].view(-1, 8))
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.sweep_sphere(dev).cpu().numpy(), soup_want)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_spheres_alone_from_outside_inside_and_in_contact(gpu_ctx, soup):
    """No triangles, so no tree: the spheres' own statement and the index order among equal times."""
    spheres = np.concatenate([soup.spheres, soup.spheres[:1]])  # sphere 3 coincides with sphere 0: the lower index wins
    scene = dataclasses.replace(soup, vertices=soup.vertices[:0], triangles=soup.triangles[:0], spheres=spheres)
    rng = np.random.default_rng(22)
    c, r = spheres["center"].astype(np.float64), spheres["radius"].astype(np.float64)
    n = 24 * len(c)
    centre, radius = np.repeat(c, 24, 0), np.repeat(r, 24)
    away = sc._unit(rng, n)
    outside = sc._pack(centre + away * (radius + rng.uniform(0.4, 2.0, n))[:, None], -away + 0.1 * sc._unit(rng, n), rng.uniform(0.01, 0.3, n))
    inside = sc._pack(centre + sc._unit(rng, n) * (radius * rng.uniform(0.0, 0.5, n))[:, None], sc._unit(rng, n), radius * rng.uniform(0.05, 0.3, n))
    touching = sc._pack(centre + sc._unit(rng, n) * (radius * rng.uniform(0.9, 1.1, n))[:, None], sc._unit(rng, n), radius * 0.2)
    astray = sc._pack(rng.uniform(-6.0, 4.0, (100, 3)), sc._unit(rng, 100), 0.1)
    sweeps = np.concatenate([outside, inside, touching, astray])
    sweeps[1::4, 7] = 0.3  # every fourth ends early: some misses more
    want = sc.brute_force(scene, sweeps)
    prim = api.split_sweep_hits(want)[4]
    t = want[:, 3]
    hit = prim != sc.PRIM_MISS
    assert (~hit).sum() >= 50 and set(prim[hit] & 3) == {0, 1, 2}, "sphere 3 never wins against its copy, sphere 0"
    assert (hit & (t == 0)).sum() >= 50 and (hit[:n] & (t[:n] > 0)).sum() >= 50 and (hit[n:2 * n] & (t[n:2 * n] > 0)).sum() >= 50
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.sweep_sphere(sweeps), want)


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_boundaries(gpu_ctx, soup, soup_sweeps, soup_want, n):
    gpu_ctx.upload_scene(soup)
    pick = np.arange(n) * 61 % len(soup_sweeps)  # of every kind
    _same(gpu_ctx.sweep_sphere(np.ascontiguousarray(soup_sweeps[pick])), soup_want[pick])


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_resolve_to_the_lower_index(gpu_ctx, soup, soup_sweeps, soup_want):
    """The soup's triangle array concatenated with itself: every candidate ties bit for bit with its copy 3000 indices on, so every
    answer is the single soup's - the same bytes, every prim_id below the original count."""
    doubled = dataclasses.replace(soup, triangles=np.concatenate([soup.triangles, soup.triangles]))
    assert len(doubled.triangles) == 6000
    prim = api.split_sweep_hits(soup_want)[4]
    assert ((prim < 3000) | (prim >= sc.SPHERE_FLAG)).all() and (prim < 3000).sum() > 3000
    gpu_ctx.upload_scene(doubled)
    _same(gpu_ctx.sweep_sphere(soup_sweeps), soup_want)


def test_cornell12_ties_between_neighbouring_triangles(gpu_ctx):
    """cornell12, the third shape: a cube whose walls share edges and corners, one node, axis-aligned faces.  Sweeps along an axis
    with two zero direction components (the 0 x inf of the slab test on a plane the centre lies in), toward walls, toward the cube's
    edges and corners from inside and outside, along its diagonals and starting within the radius of several walls.  Different
    triangles - the two of a wall, and those of different walls - reach the same t bit for bit, moving and at the start; the lower
    original index wins, as in the brute force."""
    scene = scenes.cornell12()
    sweeps = sc.cube_sweeps(9)
    assert len(sweeps) == 1024 and ((sweeps[:256, 4:7] == 0).sum(1) == 2).all() and np.signbit(sweeps[:256, 4:7]).any()
    want = sc.brute_force(scene, sweeps)
    v0, e1, e2, _ = sc.records(scene)
    t = sc.triangle_times(v0, e1, e2, np.ascontiguousarray(sweeps[:, 0:3]), np.ascontiguousarray(sweeps[:, 4:7]), np.ascontiguousarray(sweeps[:, 3]))
    best = t.min(1, keepdims=True)
    tied = (t == best) & np.isfinite(best)
    walls = np.array([np.flatnonzero(row)[[0, -1]] // 2 if row.any() else [0, 0] for row in tied])  # the first and the last of the tied: (quad, quad)
    several, moving, between = tied.sum(1) >= 2, best[:, 0] > 0, walls[:, 0] != walls[:, 1]
    face, edge, vertex, _, at_start, miss = sc.contact_kinds(want)
    print("cornell12:", dict(ties_moving=int((several & moving).sum()), between_walls=int((several & moving & between).sum()),
                             ties_at_start_between_walls=int((several & ~moving & between).sum()), face=int(face.sum()), edge=int(edge.sum()),
                             vertex=int(vertex.sum()), miss=int(miss.sum())))
    assert (several & moving).sum() >= 100 and (several & moving & between).sum() >= 100 and (several & ~moving & between).sum() >= 50
    assert face.sum() >= 100 and edge.sum() >= 50 and vertex.sum() >= 20 and miss.sum() >= 20 and at_start.sum() >= 100
    hit = ~miss
    np.testing.assert_array_equal(api.split_sweep_hits(want)[4][hit], tied.argmax(1)[hit])
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.sweep_sphere(sweeps), want)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_tmax_is_strict_on_both_sides(gpu_ctx, soup, soup_sweeps, soup_want):
    """From each sweep's answer at tmax = inf: nextafter(t, +inf) as tmax gives the same bytes - for a start in contact that is the
    smallest positive tmax - and t itself as tmax gives the miss record carrying that tmax."""
    gpu_ctx.upload_scene(soup)
    first = gpu_ctx.sweep_sphere(soup_sweeps)
    _same(first, soup_want)
    assert (soup_sweeps[:, 7] == INF).all()
    t = first[:, 3].copy()
    hit = api.split_sweep_hits(first)[4] != sc.PRIM_MISS
    assert (hit & (t == 0)).sum() >= 100 and (hit & (t > 0)).sum() >= 1000 and (~hit).sum() >= 100
    q = np.array(soup_sweeps)
    q[:, 7] = np.nextafter(t, INF)
    assert (q[hit & (t == 0), 7] == F32(1.4e-45)).all()
    _same(gpu_ctx.sweep_sphere(q), first)
    q[:, 7] = t
    _same(gpu_ctx.sweep_sphere(q), _miss_records(t))


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_queries_are_misses_without_a_walk(gpu_ctx, soup):
    gpu_ctx.upload_scene(soup)
    nan = F32(np.nan)
    o, d = [0, 0, 1], [0, 0, -1]
    q = np.array([[nan, 0, 1, 0.1, *d, INF], [0, nan, 1, 0.1, *d, 1], [0, 0, INF, 0.1, *d, INF], [0, -INF, 1, 0.1, *d, 2],
                  [*o, 0.1, nan, 0, -1, INF], [*o, 0.1, 0, INF, -1, INF], [*o, 0.1, 0, 0, -INF, 3], [*o, 0.1, 0, 0, 0, INF], [*o, 0.1, -0.0, 0, -0.0, 5],
                  [*o, nan, *d, INF], [*o, 0.0, *d, INF], [*o, -0.0, *d, INF], [*o, -1.0, *d, INF], [*o, INF, *d, INF], [*o, -INF, *d, INF],
                  [*o, 0.1, *d, nan], [*o, 0.1, *d, 0.0], [*o, 0.1, *d, -0.0], [*o, 0.1, *d, -1.0], [*o, 0.1, *d, -INF]], F32)
    got = gpu_ctx.sweep_sphere(q, counters=True)
    _same(got, _miss_records(q[:, 7]))
    st = gpu_ctx.stats()
    assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(q)
    _same(got, sc.brute_force(soup, q))
    good = np.array([[*o, 0.1, *d, INF]], F32)  # the same origin with a valid query walks
    gpu_ctx.sweep_sphere(good, counters=True)
    assert gpu_ctx.stats()["node_visits"] > 0


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_sponza_answers_do_not_depend_on_the_tree(gpu_ctx, sponza, sponza_sweeps):
    """The device-built tree and the host builder's quality tree give the same bytes; 256 of the sweeps (toward surfaces and
    scattered) are held to the statement."""
    gpu_ctx.upload_scene(sponza)
    device_tree = gpu_ctx.sweep_sphere(sponza_sweeps)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    _same(gpu_ctx.sweep_sphere(sponza_sweeps), device_tree)
    pick = np.arange(0, len(sponza_sweeps), 8)
    assert len(pick) == 256
    _same(device_tree[pick], sc.brute_force(sponza, sponza_sweeps[pick], prefilter=True))
    prim = api.split_sweep_hits(device_tree)[4]
    assert (prim[:1024] != sc.PRIM_MISS).all(), "a sweep aimed at a point of the surface touches something, that point at the latest"
    assert (prim[1024:] != sc.PRIM_MISS).any() and (prim[1024:] == sc.PRIM_MISS).any(), "scattered: some start outside the atrium and leave"


def test_sponza_refit_answers_are_a_fresh_uploads(gpu_ctx, sponza, sponza_sweeps):
    """After rt_update_geometry (a refit of the quality tree, seeded displacement) the answers are those of a fresh upload of the
    moved scene, and not those of the scene before."""
    pos = np.ascontiguousarray(sponza.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.02, pos.shape)).astype(F32)
    v = sponza.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(sponza, vertices=v)
    gpu_ctx.upload_scene(sponza)
    before = gpu_ctx.sweep_sphere(sponza_sweeps)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.update_geometry(moved_pos)["flags"] == api.STAT_REFIT
    refitted = gpu_ctx.sweep_sphere(sponza_sweeps)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        _same(refitted, fresh.sweep_sphere(sponza_sweeps))
    assert (refitted.view(np.uint32) != before.view(np.uint32)).any(1).mean() > 0.5


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_closest_point_agrees_at_the_time_of_contact(gpu_ctx, soup, soup_sweeps, soup_want):
    """The cross-check with a query that already exists, over every hit with t > 0, none left out: rt_closest_point at
    origin + direction * t (radius = inf) returns a distance within 2 eps + 2^-20 (max_a |origin_a| + |direction| t) of the sweep's
    radius, eps = the sandwich's measured k x the diagonal (sweep_cases.K_MEASURED).  The second term is not in the issue's bound of
    2 eps, which the sweeps from 20 to 100 diagonals away cannot meet: origin + direction * t is itself rounded at the size of the
    origin, and the statement's own error grows with it.  2^-20 of the magnitudes is what DESIGN.md's margin argument claims for the
    distance of the centre at the f32 time from r, so this is also the check of that claim.  For the sweeps that start within 1.5 times
    the box the term is below 1.1e-5.  For t = 0 the sweep's position, u and v are rt_closest_point's from the origin wherever that
    call names the same primitive, that is where the winner by index is also the nearest."""
    gpu_ctx.upload_scene(soup)
    got = gpu_ctx.sweep_sphere(soup_sweeps)
    _same(got, soup_want)
    pos, t, u, v, prim, _ = api.split_sweep_hits(got)
    o, r, d = soup_sweeps[:, 0:3], soup_sweeps[:, 3], soup_sweeps[:, 4:7]
    hit = prim != sc.PRIM_MISS
    moving = hit & (t > 0)
    travelled = np.where(hit, t, 0)
    centre = (o + d * travelled[:, None]).astype(F32)
    at_contact = gpu_ctx.closest_point(api.make_points(centre))
    eps = sc.K_MEASURED["soup"] * sc.diagonal(soup)
    reach = np.abs(o).max(1).astype(np.float64) + np.linalg.norm(d.astype(np.float64), axis=1) * travelled
    off = np.abs(at_contact[:, 3].astype(np.float64) - r)
    bound = 2 * eps + 2.0 ** -20 * reach
    groups = {"toward": slice(0, 800), "scattered": slice(800, 1600), "grazing": slice(1600, 2400), "in contact": slice(2400, 3200),
              "far outside": slice(3200, 4000), "spheres": slice(4000, None)}
    for name, sl in groups.items():
        m = moving[sl]
        if m.any():
            print(f"{name}: {m.sum()} contacts with t > 0, |distance - radius| at most {off[sl][m].max():.3g}, "
                  f"at most {(off[sl][m] / bound[sl][m]).max():.3g} of the bound (2 eps = {2 * eps:.3g}, reach up to {reach[sl][m].max():.4g})")
    assert moving.sum() >= 2000 and moving[3200:4000].sum() >= 700
    assert (off[moving] <= bound[moving]).all()
    start = hit & (t == 0)
    from_origin = gpu_ctx.closest_point(api.make_points(np.ascontiguousarray(o)))
    same_prim = start & (api.split_nearest(from_origin)[4] == prim)
    assert start.sum() >= 100 and same_prim.sum() >= 50
    _same(got[same_prim][:, [0, 1, 2, 4, 5, 6, 7]], from_origin[same_prim][:, [0, 1, 2, 4, 5, 6, 7]])
    assert (from_origin[start, 3] <= r[start]).all(), "in contact at the start: the nearest surface is within the radius"


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_the_walk_culls(gpu_ctx, soup):
    """A walk that skips nothing passes every equality above: against the brute force's n x n_tris triangle tests the walk makes
    fewer than a tenth."""
    sweeps = sc.toward_surfaces(soup, 2048, 31)
    gpu_ctx.upload_scene(soup)
    gpu_ctx.sweep_sphere(sweeps, counters=True)
    st = gpu_ctx.stats()
    n, n_tris = len(sweeps), len(soup.triangles)
    print(f"soup, {n} sweeps toward surfaces: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} triangle tests per sweep "
          f"(brute force: {n_tris})")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * n_tris / 10


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_side_effects_empty_scene_and_call_order(gpu_ctx, soup, soup_sweeps, soup_want):
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_sphere(soup_sweeps)
    assert e.value.code == -4, "RT_ERR_NOT_UPLOADED before an upload"
    gpu_ctx.upload_scene(soup)
    assert gpu_ctx.sweep_sphere(np.zeros((0, 8), F32)).shape == (0, 8)
    lib, one = gpu_ctx.lib, np.zeros((1, 8), F32)
    assert lib.rt_sweep_sphere(gpu_ctx._h, None, C.c_size_t(1), C.c_void_p(one.ctypes.data), C.c_uint32(0)) == -1
    assert lib.rt_sweep_sphere(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), None, C.c_uint32(0)) == -1
    assert lib.rt_sweep_sphere(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), C.c_void_p(one.ctypes.data), C.c_uint32(2)) == -1, "unknown flag"
    assert lib.rt_sweep_sphere(gpu_ctx._h, None, C.c_size_t(0), None, C.c_uint32(0)) == 0
    # the last frame and a running accumulation are left alone
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    _same(gpu_ctx.sweep_sphere(soup_sweeps), soup_want)
    _same(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4, "the running image went on"
    # an empty scene: all misses
    gpu_ctx.upload_scene(scenes.empty_scene())
    _same(gpu_ctx.sweep_sphere(soup_sweeps), _miss_records(soup_sweeps[:, 7]))


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_a_context_over_one_device_twice_gives_the_same_bytes(soup, soup_sweeps, soup_want):
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_sphere(soup_sweeps), soup_want)
        ctx.sweep_sphere(soup_sweeps, counters=True)
        assert ctx.stats()["rays"] == len(soup_sweeps) and ctx.stats()["tri_tests"] > 0


def test_two_devices_give_the_one_device_bytes(soup, soup_sweeps, soup_want):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_sphere(soup_sweeps), soup_want)
        dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:1")
        _same(ctx.sweep_sphere(dev).cpu().numpy(), soup_want)
