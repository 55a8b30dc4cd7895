"""Box sweeps on the MI355X (rt_sweep_box).  Every comparison with the float32 statement (sweep_box_cases.py's numpy brute force over
all triangles and spheres) is byte for byte: the tree only culls, so the answer is the statement's whatever tree, memory, batch size
or device count is in use."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import sweep_box_cases as sb
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
    rec = np.zeros(len(tmax), T.BOX_SWEEP_HIT)
    rec["t"] = tmax
    rec["axis"] = sb.AXIS_NONE
    rec["prim_id"] = sb.PRIM_MISS
    return rec.view(F32).reshape(-1, 8)


def _sphere_sweeps(spheres, rng, per_sphere):
    """Toward each sphere from outside and from inside each sphere outward, with boxes small against the sphere."""
    c, r = spheres["center"].astype(np.float64), spheres["radius"].astype(np.float64)
    n = per_sphere * len(c)
    centre, radius = np.repeat(c, per_sphere, 0), np.repeat(r, per_sphere)
    away = sc._unit(rng, n)
    outside = sb._pack(centre + away * (radius * 1.6 + rng.uniform(0.05, 0.4, n))[:, None], radius[:, None] * rng.uniform(0.02, 0.3, (n, 3)),
                       -away * rng.uniform(0.2, 5.0, (n, 1)))
    inside = sb._pack(centre + sc._unit(rng, n) * (radius * rng.uniform(0.0, 0.4, n))[:, None], radius[:, None] * rng.uniform(0.02, 0.15, (n, 3)),
                      sc._unit(rng, n))
    return outside, inside


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_sweeps(soup):
    """4000 sweeps of the five kinds (tmax = inf), then sweeps toward each sphere, and from inside each sphere outward."""
    outside, inside = _sphere_sweeps(soup.spheres, np.random.default_rng(21), 24)
    sweeps = np.concatenate([sb.five_kinds(soup, 4000, 11), outside, inside])
    sweeps.setflags(write=False)
    return sweeps


@pytest.fixture(scope="module")
def soup_want(soup, soup_sweeps):
    """The statement's answers, computed once (the prefiltered brute force, which test_sweep_box_abi.py holds to the plain one)."""
    rec = sb.brute_force(soup, soup_sweeps, prefilter=True)
    rec.setflags(write=False)
    return rec


@pytest.fixture(scope="module")
def sponza():
    return scenes.sponza_like()


@pytest.fixture(scope="module")
def sponza_sweeps(sponza):
    return np.concatenate([sb.toward_surfaces(sponza, 1024, 3), sb.scattered(sponza, 1024, 4)])


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_soup_equals_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_sweeps, soup_want):
    box_face, tri_face, edge_edge, sphere, at_start, miss = sb.contact_kinds(soup_want)
    print("soup:", {k: int(v.sum()) for k, v in dict(box_face=box_face, tri_face=tri_face, edge_edge=edge_edge, sphere=sphere, at_start=at_start,
                                                     miss=miss).items()})
    assert box_face.sum() >= 100 and tri_face.sum() >= 100 and edge_edge.sum() >= 100 and at_start.sum() >= 100 and miss.sum() >= 100
    assert sphere.sum() >= 20
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_box(soup_sweeps), soup_want)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_sweeps) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["kernel_ms"] > 0
    own = np.full((len(soup_sweeps), 8), 7.0, F32)
    assert gpu_ctx.sweep_box(soup_sweeps, out=own) is own
    _same(own, soup_want)
    dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    got = gpu_ctx.sweep_box(dev)
    assert got.device == dev.device and got.dtype == torch.float32
    _same(got.cpu().numpy(), soup_want)
    out = torch.empty((len(soup_sweeps), 8), device="cuda:0")
    assert gpu_ctx.sweep_box(dev, out=out) is out
    _same(out.cpu().numpy(), soup_want)
    # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    buf = torch.zeros(len(soup_sweeps) * 12 + 1, device="cuda:0")
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_box(buf[1:].view(-1, 12))
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.sweep_box(dev).cpu().numpy(), soup_want)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_spheres_alone_from_outside_inside_and_in_contact(gpu_ctx, soup):
    """No triangles, so no tree: the spheres' own statement and the index order among equal times."""
    spheres = np.concatenate([soup.spheres, soup.spheres[:1]])  # sphere 3 coincides with sphere 0: the lower index wins
    scene = dataclasses.replace(soup, vertices=soup.vertices[:0], triangles=soup.triangles[:0], spheres=spheres)
    rng = np.random.default_rng(22)
    outside, inside = _sphere_sweeps(spheres, rng, 24)
    n = len(outside)
    c, r = np.repeat(spheres["center"].astype(np.float64), 24, 0), np.repeat(spheres["radius"].astype(np.float64), 24)
    touching = sb._pack(c + sc._unit(rng, n) * (r * rng.uniform(0.9, 1.1, n))[:, None], r[:, None] * rng.uniform(0.1, 0.3, (n, 3)), sc._unit(rng, n))
    astray = sb._pack(rng.uniform(-6.0, 4.0, (100, 3)), rng.uniform(0.02, 0.2, (100, 3)), sc._unit(rng, 100))
    sweeps = np.concatenate([outside, inside, touching, astray])
    sweeps[1::4, 11] = 0.3  # every fourth ends early: some misses more
    want = sb.brute_force(scene, sweeps)
    _, t, axis, prim, _ = api.split_box_sweep_hits(want)
    hit = prim != sb.PRIM_MISS
    assert (~hit).sum() >= 50 and set(prim[hit] & 3) == {0, 1, 2}, "sphere 3 never wins against its copy, sphere 0"
    assert (hit & (t == 0)).sum() >= 50 and (hit[:n] & (t[:n] > 0)).sum() >= 50 and (hit[n:2 * n] & (t[n:2 * n] > 0)).sum() >= 50
    assert (axis[hit & (t > 0)] == sb.AXIS_SPHERE).all() and (axis[~hit | (t == 0)] == sb.AXIS_NONE).all()
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.sweep_box(sweeps), want)


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_boundaries(gpu_ctx, soup, soup_sweeps, soup_want, n):
    gpu_ctx.upload_scene(soup)
    pick = np.arange(n) * 61 % len(soup_sweeps)  # of every kind
    _same(gpu_ctx.sweep_box(np.ascontiguousarray(soup_sweeps[pick])), soup_want[pick])


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_resolve_to_the_lower_index(gpu_ctx, soup, soup_sweeps, soup_want):
    """The soup's triangle array concatenated with itself: every candidate ties bit for bit with its copy 3000 indices on, so every
    answer is the single soup's - the same bytes, every prim_id below the original count."""
    doubled = dataclasses.replace(soup, triangles=np.concatenate([soup.triangles, soup.triangles]))
    assert len(doubled.triangles) == 6000
    prim = api.split_box_sweep_hits(soup_want)[3]
    assert ((prim < 3000) | (prim >= sb.SPHERE_FLAG)).all() and (prim < 3000).sum() > 3000
    gpu_ctx.upload_scene(doubled)
    _same(gpu_ctx.sweep_box(soup_sweeps), soup_want)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_cornell12_ties_between_axes_and_between_neighbouring_triangles(gpu_ctx):
    """cornell12: a cube whose walls share edges and corners, one node, axis-aligned faces against axis-aligned boxes.  Sweeps along
    an axis with two zero direction components (the 0 x inf of the slab test on a plane the centre lies in), toward walls, toward the
    cube's edges and corners from inside and outside, cubes along the diagonals and boxes starting across several walls.  A wall's
    normal axis ties with a box axis on every face contact, and different triangles - the two of a wall, and those of different
    walls - reach the same t bit for bit, moving and at the start; the lower original index wins, as in the brute force."""
    scene = scenes.cornell12()
    sweeps = sb.cube_sweeps(9)
    assert len(sweeps) == 1024 and ((sweeps[:256, 8:11] == 0).sum(1) == 2).all() and np.signbit(sweeps[:256, 8:11]).any()
    want = sb.brute_force(scene, sweeps)
    t = sb.triangle_times_all(scene, sweeps)
    best = t.min(1, keepdims=True)
    tied = (t == best) & np.isfinite(best)
    v0, e1, e2, _ = sb.records(scene)
    n = np.cross(e1, e2)
    plane = np.abs(n).argmax(1)
    wall = plane * 1000 + np.round(v0[np.arange(len(v0)), plane] * 100).astype(int)  # the axis of the normal and the plane's coordinate
    first, last = tied.argmax(1), tied.shape[1] - 1 - tied[:, ::-1].argmax(1)
    several, moving, between = tied.sum(1) >= 2, best[:, 0] > 0, wall[first] != wall[last]
    box_face, tri_face, edge_edge, _, at_start, miss = sb.contact_kinds(want)
    print("cornell12:", dict(ties_moving=int((several & moving).sum()), between_walls=int((several & moving & between).sum()),
                             ties_at_start_between_walls=int((several & ~moving & between).sum()), box_face=int(box_face.sum()),
                             at_start=int(at_start.sum()), miss=int(miss.sum())))
    assert (several & moving).sum() >= 100 and (several & moving & between).sum() >= 100 and (several & ~moving & between).sum() >= 50
    assert box_face.sum() >= 100 and miss.sum() >= 20 and at_start.sum() >= 100
    hit = ~miss
    np.testing.assert_array_equal(api.split_box_sweep_hits(want)[3][hit], first[hit])
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.sweep_box(sweeps), want)


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_tmax_is_strict_on_both_sides(gpu_ctx, soup, soup_sweeps, soup_want):
    """From each sweep's answer at tmax = inf: nextafter(t, +inf) as tmax gives the same bytes - for a start in contact that is the
    smallest positive tmax - and t itself as tmax gives the miss record carrying that tmax."""
    gpu_ctx.upload_scene(soup)
    first = gpu_ctx.sweep_box(soup_sweeps)
    _same(first, soup_want)
    assert (soup_sweeps[:, 11] == INF).all()
    t = first[:, 3].copy()
    hit = api.split_box_sweep_hits(first)[3] != sb.PRIM_MISS
    assert (hit & (t == 0)).sum() >= 100 and (hit & (t > 0)).sum() >= 1000 and (~hit).sum() >= 100
    q = np.array(soup_sweeps)
    q[:, 11] = np.nextafter(t, INF)
    assert (q[hit & (t == 0), 11] == F32(1.4e-45)).all()
    _same(gpu_ctx.sweep_box(q), first)
    q[:, 11] = t
    _same(gpu_ctx.sweep_box(q), _miss_records(t))


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_queries_are_misses_without_a_walk(gpu_ctx, soup):
    gpu_ctx.upload_scene(soup)
    nan = F32(np.nan)
    c, h, d = [0, 0, 1], [0.1, 0.05, 0.2], [0, 0, -1]

    def q_(c=c, h=h, d=d, tmax=INF):
        return [*c, 0, *h, 0, *d, tmax]

    q = np.array([q_(c=[nan, 0, 1]), q_(c=[0, nan, 1], tmax=1), q_(c=[0, 0, INF]), q_(c=[0, -INF, 1], tmax=2),
                  q_(h=[nan, 0.1, 0.1]), q_(h=[0.1, INF, 0.1]), q_(h=[0.1, 0.1, -INF]), q_(h=[-0.1, 0.1, 0.1]), q_(h=[0.1, 0.1, -1e-30]),
                  q_(d=[nan, 0, -1]), q_(d=[0, INF, -1]), q_(d=[0, 0, -INF], tmax=3), q_(d=[0, 0, 0]), q_(d=[-0.0, 0, -0.0], tmax=5),
                  q_(tmax=nan), q_(tmax=0.0), q_(tmax=-0.0), q_(tmax=-1.0), q_(tmax=-INF)], F32)
    got = gpu_ctx.sweep_box(q, counters=True)
    _same(got, _miss_records(q[:, 11]))
    st = gpu_ctx.stats()
    assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(q)
    _same(got, sb.brute_force(soup, q))
    good = np.array([q_(), q_(h=[0, 0, 0]), q_(h=[-0.0, 0.1, 0.0])], F32)  # the same centre with a valid query walks; zero extents are valid
    _same(gpu_ctx.sweep_box(good, counters=True), sb.brute_force(soup, good))
    assert gpu_ctx.stats()["node_visits"] >= 3


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_sponza_answers_do_not_depend_on_the_tree(gpu_ctx, sponza, sponza_sweeps):
    """The device-built tree and the host builder's quality tree give the same bytes; 256 of the sweeps (toward surfaces and
    scattered) are held to the statement."""
    gpu_ctx.upload_scene(sponza)
    device_tree = gpu_ctx.sweep_box(sponza_sweeps)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    _same(gpu_ctx.sweep_box(sponza_sweeps), device_tree)
    pick = np.arange(0, len(sponza_sweeps), 8)
    assert len(pick) == 256
    _same(device_tree[pick], sb.brute_force(sponza, sponza_sweeps[pick], prefilter=True))
    prim = api.split_box_sweep_hits(device_tree)[3]
    assert (prim[:1024] != sb.PRIM_MISS).all(), "a sweep aimed at a point of the surface touches something, that point at the latest"
    assert (prim[1024:] != sb.PRIM_MISS).any() and (prim[1024:] == sb.PRIM_MISS).any(), "scattered: some start outside the atrium and leave"


def test_sponza_refit_answers_are_a_fresh_uploads(gpu_ctx, sponza, sponza_sweeps):
    """After rt_update_geometry (a refit of the quality tree, seeded displacement) the answers are those of a fresh upload of the
    moved scene, and not those of the scene before."""
    pos = np.ascontiguousarray(sponza.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.02, pos.shape)).astype(F32)
    v = sponza.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(sponza, vertices=v)
    gpu_ctx.upload_scene(sponza)
    before = gpu_ctx.sweep_box(sponza_sweeps)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.update_geometry(moved_pos)["flags"] == api.STAT_REFIT
    refitted = gpu_ctx.sweep_box(sponza_sweeps)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        _same(refitted, fresh.sweep_box(sponza_sweeps))
    assert (refitted.view(np.uint32) != before.view(np.uint32)).any(1).mean() > 0.5


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_overlap_box_agrees_at_the_time_of_contact(gpu_ctx, soup, soup_sweeps, soup_want):
    """The cross-check with a query that already exists, over every hit with t > 0 and all extents >= 1e-3 x the diagonal, none left
    out: rt_overlap_box(RT_OVERLAP_ANY) is 1 for the box at center + direction * t grown by eps on every axis, and 0 for the box
    shrunk by eps at 50, 90 and 99.9 % of t.  eps = 2 K_MEASURED x the diagonal + 2^-20 x (the largest |centre| component +
    |direction| t), the sphere sweep's bound: center + direction * t is itself rounded at the size of the centre.  The worst ratio per
    kind is how much of eps the box needs: the smallest growth (in units of eps, on a grid of eighths) at which the overlap holds."""
    gpu_ctx.upload_scene(soup)
    got = gpu_ctx.sweep_box(soup_sweeps)
    _same(got, soup_want)
    _, t, _, prim, _ = api.split_box_sweep_hits(got)
    c, h, d = soup_sweeps[:, 0:3], soup_sweeps[:, 4:7], soup_sweeps[:, 8:11]
    diag = sb.diagonal(soup)
    pick = (prim != sb.PRIM_MISS) & (t > 0) & sb.full_extents(soup, soup_sweeps)
    c, h, d, t = c[pick].astype(np.float64), h[pick].astype(np.float64), d[pick].astype(np.float64), t[pick].astype(np.float64)
    eps = 2 * sb.K_MEASURED["soup"] * diag + 2.0 ** -20 * (np.abs(c).max(1) + np.linalg.norm(d, axis=1) * t)
    assert (eps[:, None] < h).all()

    def any_touch(part, grow):
        boxes = api.make_boxes((c + d * (t * part)[:, None]).astype(F32), (h + (eps * grow)[:, None]).astype(F32))
        return gpu_ctx.overlap_box(boxes, 0, any_hit=True)[1].astype(bool)

    need = np.full(len(t), np.inf)
    for grow in np.arange(8, -1, -1) / 8.0:
        need = np.where(any_touch(np.ones(len(t)), np.full(len(t), grow)), grow, need)
    kind = np.searchsorted([800, 1600, 2400, 3200, 4000], np.flatnonzero(pick), side="right")
    for k, name in enumerate(("toward", "scattered", "grazing", "in contact", "far outside", "spheres")):
        m = kind == k
        if m.any():
            print(f"{name}: {m.sum()} contacts with t > 0, the box at the contact needs at most {need[m].max():.3g} eps to touch (eps up to {eps[m].max():.3g})")
    assert pick.sum() >= 1500 and (kind == 4).sum() >= 500
    assert (need <= 1.0).all(), "grown by eps the box touches at the time of contact"
    for part in (0.5, 0.9, 0.999):
        early = any_touch(np.full(len(t), part), np.full(len(t), -1.0))
        assert not early.any(), (part, int(early.sum()))


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_the_walk_culls(gpu_ctx, soup):
    """A walk that skips nothing passes every equality above: against the brute force's n x n_tris triangle tests the walk makes
    fewer than a tenth."""
    sweeps = sb.toward_surfaces(soup, 2048, 31)
    gpu_ctx.upload_scene(soup)
    gpu_ctx.sweep_box(sweeps, counters=True)
    st = gpu_ctx.stats()
    n, n_tris = len(sweeps), len(soup.triangles)
    print(f"soup, {n} sweeps toward surfaces: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} triangle tests per sweep "
          f"(brute force: {n_tris})")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * n_tris / 10


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_side_effects_empty_scene_and_call_order(gpu_ctx, soup, soup_sweeps, soup_want):
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_box(soup_sweeps)
    assert e.value.code == -4, "RT_ERR_NOT_UPLOADED before an upload"
    gpu_ctx.upload_scene(soup)
    assert gpu_ctx.sweep_box(np.zeros((0, 12), F32)).shape == (0, 8)
    lib, one, out = gpu_ctx.lib, np.zeros((1, 12), F32), np.zeros((1, 8), F32)
    assert lib.rt_sweep_box(gpu_ctx._h, None, C.c_size_t(1), C.c_void_p(out.ctypes.data), C.c_uint32(0)) == -1
    assert lib.rt_sweep_box(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), None, C.c_uint32(0)) == -1
    assert lib.rt_sweep_box(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), C.c_void_p(out.ctypes.data), C.c_uint32(2)) == -1, "unknown flag"
    assert lib.rt_sweep_box(gpu_ctx._h, None, C.c_size_t(0), None, C.c_uint32(0)) == 0
    # the last frame and a running accumulation are left alone
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    _same(gpu_ctx.sweep_box(soup_sweeps), soup_want)
    _same(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4, "the running image went on"
    # an empty scene: all misses
    gpu_ctx.upload_scene(scenes.empty_scene())
    _same(gpu_ctx.sweep_box(soup_sweeps), _miss_records(soup_sweeps[:, 11]))


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_a_context_over_one_device_twice_gives_the_same_bytes(soup, soup_sweeps, soup_want):
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_box(soup_sweeps), soup_want)
        ctx.sweep_box(soup_sweeps, counters=True)
        assert ctx.stats()["rays"] == len(soup_sweeps) and ctx.stats()["tri_tests"] > 0


def test_two_devices_give_the_one_device_bytes(soup, soup_sweeps, soup_want):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_box(soup_sweeps), soup_want)
        dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:1")
        _same(ctx.sweep_box(dev).cpu().numpy(), soup_want)
