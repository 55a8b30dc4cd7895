"""Capsule sweeps on the MI355X (rt_sweep_capsule).  Every comparison with the float32 statement (sweep_capsule_cases.py's numpy brute
force over all triangles and spheres) is byte for byte: the tree only culls, so the answer is the statement's whatever tree, memory,
batch size or device count is in use."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import sweep_capsule_cases as cap
import sweep_cases as sc
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first; these tests need it

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = np.float64
INF = F32(np.inf)


def _same(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _miss_records(tmax):
    rec = np.zeros(len(tmax), T.CAPSULE_SWEEP_HIT)
    rec["t"] = tmax
    rec["prim_id"] = cap.PRIM_MISS
    return rec.view(F32).reshape(-1, 8)


def _sphere_sweeps(spheres, rng, per_sphere):
    """Toward each sphere from outside and from inside each sphere outward, with capsules small against the sphere."""
    c, r = spheres["center"].astype(F64), spheres["radius"].astype(F64)
    n = per_sphere * len(c)
    centre, radius = np.repeat(c, per_sphere, 0), np.repeat(r, per_sphere)
    away = sc._unit(rng, n)
    axis = sc._unit(rng, n) * (radius * rng.uniform(0.0, 2.0, n))[:, None]
    axis[::6] = 0.0
    outside = cap._pack(centre + away * (radius * 1.8 + rng.uniform(0.05, 0.4, n))[:, None] - axis / 2, axis, -away * rng.uniform(0.2, 5.0, (n, 1)),
                        radius * rng.uniform(0.02, 0.3, n))
    inside = cap._pack(centre + sc._unit(rng, n) * (radius * rng.uniform(0.0, 0.3, n))[:, None] - axis * 0.1, axis * 0.2, sc._unit(rng, n),
                       radius * rng.uniform(0.02, 0.15, n))
    return outside, inside


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_sweeps(soup):
    """2048 sweeps: 1900 of the five kinds (tmax = inf), then sweeps toward each sphere, and from inside each sphere outward."""
    outside, inside = _sphere_sweeps(soup.spheres, np.random.default_rng(21), 24)
    sweeps = np.concatenate([cap.five_kinds(soup, 1900, 11), outside, inside, cap.scattered(soup, 4, 77)])
    assert len(sweeps) == 2048
    sweeps.setflags(write=False)
    return sweeps


@pytest.fixture(scope="module")
def soup_want(soup, soup_sweeps):
    """The statement's answers, computed once (the prefiltered brute force, which test_sweep_capsule_abi.py holds to the plain one)."""
    rec = cap.brute_force(soup, soup_sweeps, prefilter=True)
    rec.setflags(write=False)
    return rec


@pytest.fixture(scope="module")
def sponza():
    return scenes.sponza_like()


@pytest.fixture(scope="module")
def sponza_sweeps(sponza):
    return np.concatenate([cap.toward_surfaces(sponza, 1024, 3), cap.scattered(sponza, 1024, 4)])


def _fields(records):
    return np.ascontiguousarray(records, F32).view(T.CAPSULE_SWEEP_HIT).reshape(-1)


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_soup_equals_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_sweeps, soup_want):
    rec = _fields(soup_want)
    hit = rec["prim_id"] != cap.PRIM_MISS
    sphere = hit & (rec["prim_id"] >= cap.SPHERE_FLAG)
    counts = dict(hit=int(hit.sum()), miss=int((~hit).sum()), at_start=int((hit & (rec["t"] == 0)).sum()), sphere=int(sphere.sum()),
                  end_a=int((hit & (rec["s"] == 0)).sum()), end_b=int((hit & (rec["s"] == 1)).sum()), wall=int((hit & (rec["s"] > 0) & (rec["s"] < 1)).sum()))
    print("soup:", counts)
    assert counts["miss"] >= 100 and counts["at_start"] >= 100 and counts["sphere"] >= 20
    assert counts["end_a"] >= 100 and counts["end_b"] >= 100 and counts["wall"] >= 100
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_capsule(soup_sweeps), soup_want)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_sweeps) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["kernel_ms"] > 0
    own = np.full((len(soup_sweeps), 8), 7.0, F32)
    assert gpu_ctx.sweep_capsule(soup_sweeps, out=own) is own
    _same(own, soup_want)
    dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    got = gpu_ctx.sweep_capsule(dev)
    assert got.device == dev.device and got.dtype == torch.float32
    _same(got.cpu().numpy(), soup_want)
    out = torch.empty((len(soup_sweeps), 8), device="cuda:0")
    assert gpu_ctx.sweep_capsule(dev, out=out) is out
    _same(out.cpu().numpy(), soup_want)
    # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    buf = torch.zeros(len(soup_sweeps) * 12 + 1, device="cuda:0")
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_capsule(buf[1:].view(-1, 12))
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.sweep_capsule(dev).cpu().numpy(), soup_want)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_spheres_alone_from_outside_inside_and_in_contact(gpu_ctx, soup):
    """No triangles, so no tree: the spheres' own statement and the index order among equal times."""
    spheres = np.concatenate([soup.spheres, soup.spheres[:1]])  # sphere 3 coincides with sphere 0: the lower index wins
    scene = dataclasses.replace(soup, vertices=soup.vertices[:0], triangles=soup.triangles[:0], spheres=spheres)
    rng = np.random.default_rng(22)
    outside, inside = _sphere_sweeps(spheres, rng, 24)
    n = len(outside)
    c, r = np.repeat(spheres["center"].astype(F64), 24, 0), np.repeat(spheres["radius"].astype(F64), 24)
    axis = sc._unit(rng, n) * (r * rng.uniform(0.0, 3.0, n))[:, None]  # some longer than the sphere is wide: through it, both ends outside
    touching = cap._pack(c + sc._unit(rng, n) * (r * rng.uniform(0.9, 1.1, n))[:, None] - axis * rng.random((n, 1)), axis, sc._unit(rng, n),
                         r * rng.uniform(0.1, 0.3, n))
    astray = cap._pack(rng.uniform(-6.0, 4.0, (100, 3)), sc._unit(rng, 100) * 0.3, sc._unit(rng, 100), rng.uniform(0.02, 0.2, 100))
    sweeps = np.concatenate([outside, inside, touching, astray])
    sweeps[1::4, 11] = 0.3  # every fourth ends early: some misses more
    want = cap.brute_force(scene, sweeps)
    _, t, s, prim, _ = api.split_capsule_sweep_hits(want)
    hit = prim != cap.PRIM_MISS
    assert (~hit).sum() >= 50 and set(prim[hit] & 3) == {0, 1, 2}, "sphere 3 never wins against its copy, sphere 0"
    assert (hit & (t == 0)).sum() >= 50 and (hit[:n] & (t[:n] > 0)).sum() >= 50 and (hit[n:2 * n] & (t[n:2 * n] > 0)).sum() >= 50
    assert (hit & (s > 0) & (s < 1)).sum() >= 20 and (hit & (s == 1)).sum() >= 20
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.sweep_capsule(sweeps), want)


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_lane_boundaries(gpu_ctx, soup, soup_sweeps, soup_want, n):
    gpu_ctx.upload_scene(soup)
    pick = np.arange(n) * 61 % len(soup_sweeps)  # of every kind
    _same(gpu_ctx.sweep_capsule(np.ascontiguousarray(soup_sweeps[pick])), soup_want[pick])


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_cornell12_ties_between_neighbouring_triangles(gpu_ctx):
    """cornell12: a cube whose walls share edges and corners, one node.  Different triangles - the two of a wall, and those of
    different walls - reach the same t bit for bit, moving and at the start; the lower original index wins, as in the brute force."""
    scene = scenes.cornell12()
    sweeps = cap.cube_sweeps(9)
    assert len(sweeps) == 1024
    want = cap.brute_force(scene, sweeps)
    v0, e1, e2, _ = cap.records(scene)
    t = cap.triangle_times(v0, e1, e2, *(np.ascontiguousarray(sweeps[:, k:k + 3]) for k in (0, 4, 8)), sweeps[:, 3])
    best = t.min(1, keepdims=True)
    tied = (t == best) & np.isfinite(best)
    several, moving = tied.sum(1) >= 2, best[:, 0] > 0
    print("cornell12:", dict(ties_moving=int((several & moving).sum()), ties_at_start=int((several & ~moving).sum())))
    assert (several & moving).sum() >= 100 and (several & ~moving).sum() >= 50
    prim = api.split_capsule_sweep_hits(want)[3]
    hit = prim != cap.PRIM_MISS
    np.testing.assert_array_equal(prim[hit], tied.argmax(1)[hit])
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.sweep_capsule(sweeps), want)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_tmax_is_strict_on_both_sides(gpu_ctx, soup, soup_sweeps, soup_want):
    """From each sweep's answer at tmax = inf: nextafter(t, +inf) as tmax gives the same bytes - for a start in contact that is the
    smallest positive tmax - and t itself as tmax gives the miss record carrying that tmax."""
    gpu_ctx.upload_scene(soup)
    first = gpu_ctx.sweep_capsule(soup_sweeps)
    _same(first, soup_want)
    assert (soup_sweeps[:, 11] == INF).all()
    t = first[:, 3].copy()
    hit = api.split_capsule_sweep_hits(first)[3] != cap.PRIM_MISS
    assert (hit & (t == 0)).sum() >= 100 and (hit & (t > 0)).sum() >= 500 and (~hit).sum() >= 100
    q = np.array(soup_sweeps)
    q[:, 11] = np.nextafter(t, INF)
    assert (q[hit & (t == 0), 11] == F32(1.4e-45)).all()
    _same(gpu_ctx.sweep_capsule(q), first)
    q[:, 11] = t
    _same(gpu_ctx.sweep_capsule(q), _miss_records(t))


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_queries_are_misses_without_a_walk(gpu_ctx, soup):
    gpu_ctx.upload_scene(soup)
    nan = F32(np.nan)
    A, ax, d = [0, 0, 1], [0, 0.2, 0.1], [0, 0, -1]

    def q_(A=A, r=0.1, ax=ax, d=d, tmax=INF):
        return [*A, r, *ax, 0, *d, tmax]

    q = np.array([q_(A=[nan, 0, 1]), q_(A=[0, nan, 1], tmax=1), q_(A=[0, 0, INF]), q_(A=[0, -INF, 1], tmax=2),
                  q_(ax=[nan, 0.1, 0.1]), q_(ax=[0.1, INF, 0.1]), q_(ax=[0.1, 0.1, -INF]),
                  q_(r=nan), q_(r=0.0), q_(r=-0.0), q_(r=-0.1), q_(r=INF), q_(r=-INF),
                  q_(d=[nan, 0, -1]), q_(d=[0, INF, -1]), q_(d=[0, 0, -INF], tmax=3), q_(d=[0, 0, 0]), q_(d=[-0.0, 0, -0.0], tmax=5),
                  q_(tmax=nan), q_(tmax=0.0), q_(tmax=-0.0), q_(tmax=-1.0), q_(tmax=-INF)], F32)
    got = gpu_ctx.sweep_capsule(q, counters=True)
    _same(got, _miss_records(q[:, 11]))
    st = gpu_ctx.stats()
    assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(q)
    _same(got, cap.brute_force(soup, q))
    good = np.array([q_(), q_(ax=[0, 0, 0]), q_(ax=[-0.0, 0.1, 0.0])], F32)  # the same origin with a valid query walks; a zero axis is valid
    _same(gpu_ctx.sweep_capsule(good, counters=True), cap.brute_force(soup, good))
    assert gpu_ctx.stats()["node_visits"] >= 3


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_a_zero_axis_equals_the_sphere_sweep_field_by_field(gpu_ctx, soup):
    """axis == 0 exactly: rt_sweep_sphere's t, position, prim_id and material_id on the same device, bit for bit, and s = 0."""
    s8 = np.concatenate([sc.five_kinds(soup, 2000, 11), sc.toward_surfaces(soup, 48, 5, radius=(1e-3, 2e-3))])
    gpu_ctx.upload_scene(soup)
    sphere = np.ascontiguousarray(gpu_ctx.sweep_sphere(s8)).view(T.SWEEP_HIT).reshape(-1)
    got = _fields(gpu_ctx.sweep_capsule(cap.zero_axis(s8)))
    for f in ("t", "position", "prim_id", "material_id"):
        np.testing.assert_array_equal(got[f].view(np.uint32), sphere[f].view(np.uint32), err_msg=f)
    assert not got["s"].view(np.uint32).any() and not got["_reserved"].any()
    hit = sphere["prim_id"] != cap.PRIM_MISS
    assert hit.sum() > 1500 and (~hit).sum() > 50 and (sphere["t"][hit] == 0).sum() > 100 and (sphere["prim_id"][hit] >= cap.SPHERE_FLAG).sum() >= 5


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_closest_point_and_the_ends_sphere_sweeps_agree(gpu_ctx, soup, soup_sweeps, soup_want):
    """Two cross-checks with queries that already exist, over every contact with t > 0, none left out.
    rt_closest_point from the axis point A + axis s + d t: its distance from the surface is r to within 2 eps + 2^-20 (max_a |c_a| +
    |axis| + |d| t), eps = K_MEASURED x the diagonal: the statement's own error, and the rounding of the point, which is formed at the
    size of the origin, the axis and the path.
    Containment: the capsule contains the balls at both ends, so t <= the smaller of rt_sweep_sphere's times from A and from B, with
    a relative slack of 1e-5, over every sweep of the batch with its origin and axis rounded to multiples of 2^-12, so that A + axis
    is exact in f32 and the sphere sweep from B starts where the capsule's end B is.  With the batch as drawn, B = f32(A + axis) is
    off by up to an ulp of the coordinate, which moves a sphere's time by that over |d|: 2e-7 on a contact at t = 0.0147 of the
    batch, 1.4e-5 of it, with the float64 statements of both saying the same - the rounding of the input, not of either answer."""
    gpu_ctx.upload_scene(soup)
    got = gpu_ctx.sweep_capsule(soup_sweeps)
    _same(got, soup_want)
    _, t, s, prim, _ = api.split_capsule_sweep_hits(got)
    pick = (prim != cap.PRIM_MISS) & (t > 0)
    A, r, ax, d = (soup_sweeps[pick][:, c].astype(F64) for c in (slice(0, 3), 3, slice(4, 7), slice(8, 11)))
    tt, ss = t[pick].astype(F64), s[pick].astype(F64)
    point = A + ax * ss[:, None] + d * tt[:, None]
    eps = cap.K_MEASURED["soup"] * cap.diagonal(soup)
    bound = 2 * eps + 2.0 ** -20 * (np.abs(A).max(1) + np.linalg.norm(ax, axis=1) + np.linalg.norm(d, axis=1) * tt)
    near = gpu_ctx.closest_point(api.make_points(point.astype(F32)))
    dist = near[:, 3].astype(F64)
    err = np.abs(dist - r)
    print(f"{pick.sum()} contacts with t > 0: |distance - r| is at most {(err / bound).max():.3g} of the bound (bound up to {bound.max():.3g})")
    assert pick.sum() >= 800
    assert (err <= bound).all(), (int((err > bound).sum()), float((err / bound).max()))
    # containment, over every sweep
    exact = np.array(soup_sweeps)
    exact[:, 0:3], exact[:, 4:7] = np.round(exact[:, 0:3] * 4096) / 4096, np.round(exact[:, 4:7] * 4096) / 4096
    end_b = exact[:, 0:3] + exact[:, 4:7]
    assert (end_b.astype(F64) == exact[:, 0:3].astype(F64) + exact[:, 4:7].astype(F64)).all()
    from_a = np.ascontiguousarray(exact[:, [0, 1, 2, 3, 8, 9, 10, 11]])
    from_b = from_a.copy()
    from_b[:, 0:3] = end_b
    t = gpu_ctx.sweep_capsule(exact)[:, 3].astype(F64)
    ends = np.minimum(gpu_ctx.sweep_sphere(from_a)[:, 3], gpu_ctx.sweep_sphere(from_b)[:, 3]).astype(F64)
    assert (ends < np.inf).sum() >= 1000
    assert (t <= ends * (1 + 1e-5)).all(), np.flatnonzero(t > ends * (1 + 1e-5))[:8]
    assert (t < ends * (1 - 1e-3)).sum() >= 100, "the wall comes first for some"


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_sponza_answers_do_not_depend_on_the_tree(gpu_ctx, sponza, sponza_sweeps):
    """The device-built tree and the host builder's quality tree give the same bytes; 256 of the sweeps (toward surfaces and
    scattered) are held to the statement."""
    gpu_ctx.upload_scene(sponza)
    device_tree = gpu_ctx.sweep_capsule(sponza_sweeps)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    _same(gpu_ctx.sweep_capsule(sponza_sweeps), device_tree)
    pick = np.arange(0, len(sponza_sweeps), 8)
    assert len(pick) == 256
    _same(device_tree[pick], cap.brute_force(sponza, sponza_sweeps[pick], prefilter=True))
    prim = api.split_capsule_sweep_hits(device_tree)[3]
    assert (prim[:1024] != cap.PRIM_MISS).all(), "a body aimed at a point of the surface touches something, that point at the latest"
    assert (prim[1024:] != cap.PRIM_MISS).any() and (prim[1024:] == cap.PRIM_MISS).any(), "scattered: some start outside the atrium and leave"


def test_sponza_refit_answers_are_a_fresh_uploads(gpu_ctx, sponza, sponza_sweeps):
    """After rt_update_geometry (a refit of the quality tree, seeded displacement) the answers are those of a fresh upload of the
    moved scene, and not those of the scene before."""
    pos = np.ascontiguousarray(sponza.vertices["position"], F32)
    moved_pos = (pos.astype(F64) + np.random.default_rng(17).normal(0.0, 0.02, pos.shape)).astype(F32)
    v = sponza.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(sponza, vertices=v)
    gpu_ctx.upload_scene(sponza)
    before = gpu_ctx.sweep_capsule(sponza_sweeps)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.update_geometry(moved_pos)["flags"] == api.STAT_REFIT
    refitted = gpu_ctx.sweep_capsule(sponza_sweeps)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        _same(refitted, fresh.sweep_capsule(sponza_sweeps))
    assert (refitted.view(np.uint32) != before.view(np.uint32)).any(1).mean() > 0.5


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_the_walk_culls(gpu_ctx, soup):
    """A walk that skips nothing passes every equality above: the mean number of triangle tests per sweep stays below 300 of the
    soup's 3000."""
    sweeps = cap.toward_surfaces(soup, 2048, 31)
    gpu_ctx.upload_scene(soup)
    gpu_ctx.sweep_capsule(sweeps, counters=True)
    st = gpu_ctx.stats()
    n, n_tris = len(sweeps), len(soup.triangles)
    print(f"soup, {n} sweeps toward surfaces: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} triangle tests per sweep "
          f"(brute force: {n_tris})")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * 300


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_side_effects_empty_scene_and_call_order(gpu_ctx, soup, soup_sweeps, soup_want):
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_capsule(soup_sweeps)
    assert e.value.code == -4, "RT_ERR_NOT_UPLOADED before an upload"
    gpu_ctx.upload_scene(soup)
    assert gpu_ctx.sweep_capsule(np.zeros((0, 12), F32)).shape == (0, 8)
    lib, one, out = gpu_ctx.lib, np.zeros((1, 12), F32), np.zeros((1, 8), F32)
    assert lib.rt_sweep_capsule(gpu_ctx._h, None, C.c_size_t(1), C.c_void_p(out.ctypes.data), C.c_uint32(0)) == -1
    assert lib.rt_sweep_capsule(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), None, C.c_uint32(0)) == -1
    assert lib.rt_sweep_capsule(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), C.c_void_p(out.ctypes.data), C.c_uint32(2)) == -1, "unknown flag"
    assert lib.rt_sweep_capsule(gpu_ctx._h, None, C.c_size_t(0), None, C.c_uint32(0)) == 0
    # the last frame, the rt_read_* results and a running accumulation are left alone
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    _same(gpu_ctx.sweep_capsule(soup_sweeps), soup_want)
    _same(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4, "the running image went on"
    # an empty scene: all misses
    gpu_ctx.upload_scene(scenes.empty_scene())
    _same(gpu_ctx.sweep_capsule(soup_sweeps), _miss_records(soup_sweeps[:, 11]))


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_a_context_over_one_device_twice_gives_the_same_bytes(soup, soup_sweeps, soup_want):
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_capsule(soup_sweeps), soup_want)
        ctx.sweep_capsule(soup_sweeps, counters=True)
        assert ctx.stats()["rays"] == len(soup_sweeps) and ctx.stats()["tri_tests"] > 0


def test_two_devices_give_the_one_device_bytes(soup, soup_sweeps, soup_want):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_capsule(soup_sweeps), soup_want)
        dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:1")
        _same(ctx.sweep_capsule(dev).cpu().numpy(), soup_want)
