"""Triangle sweeps on the MI355X (rt_sweep_triangle).  Every comparison with the float32 statement (sweep_triangle_cases.py's numpy
brute force over all triangles and spheres) is byte for byte: the tree only culls, so the answer is the statement's whatever tree,
memory, batch size or device count is in use."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import sweep_triangle_cases as st
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first; these tests need it

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


def _same(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _miss_records(tmax):
    rec = np.zeros(len(tmax), T.TRIANGLE_SWEEP_HIT)
    rec["t"] = tmax
    rec["axis"] = st.AXIS_NONE
    rec["prim_id"] = st.PRIM_MISS
    return rec.view(F32).reshape(-1, 8)


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_sweeps(soup):
    """The soup's fixtures (tmax = inf): 3000 of the five kinds, then segments and points, then the sphere sets."""
    sweeps = np.concatenate(list(st.fixtures("soup", soup).values()))
    sweeps.setflags(write=False)
    return sweeps


@pytest.fixture(scope="module")
def soup_want(soup, soup_sweeps):
    """The statement's answers, computed once."""
    rec = st.brute_force(soup, soup_sweeps)
    rec.setflags(write=False)
    return rec


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_soup_equals_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_sweeps, soup_want):
    kinds = dict(zip(("coordinate", "normals", "edge_pairs", "coplanar", "segment", "sphere", "at_start", "miss"), st.contact_kinds(soup_want)))
    print("soup:", {k: int(v.sum()) for k, v in kinds.items()})
    assert all(kinds[k].sum() >= 100 for k in ("normals", "edge_pairs", "at_start", "miss")) and kinds["sphere"].sum() >= 20
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_triangle(soup_sweeps), soup_want)
    s = gpu_ctx.stats()
    assert s["rays"] == len(soup_sweeps) and s["pixels"] == 0 and s["primary_rays"] == 0 and s["node_visits"] == 0 and s["kernel_ms"] > 0
    own = np.full((len(soup_sweeps), 8), 7.0, F32)
    assert gpu_ctx.sweep_triangle(soup_sweeps, out=own) is own
    _same(own, soup_want)
    dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    got = gpu_ctx.sweep_triangle(dev)
    assert got.device == dev.device and got.dtype == torch.float32
    _same(got.cpu().numpy(), soup_want)
    out = torch.empty((len(soup_sweeps), 8), device="cuda:0")
    assert gpu_ctx.sweep_triangle(dev, out=out) is out
    _same(out.cpu().numpy(), soup_want)
    # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    buf = torch.zeros(len(soup_sweeps) * 16 + 1, device="cuda:0")
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_triangle(buf[1:].view(-1, 16))
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.sweep_triangle(dev).cpu().numpy(), soup_want)


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell12", "plane"])
def test_aimed_sets_equal_the_statement(gpu_ctx, name):
    """cornell12: axis-aligned triangles against the walls and triangles sliding in a wall's plane; the plane scene: coplanar triangles,
    segments and points moving inside z = 0.  These close on the coordinate axes and on the in-plane axes 14 .. 25, which no sweep in
    general position does."""
    scene = scenes.cornell12() if name == "cornell12" else st.plane_scene()
    sweeps = np.concatenate(list(st.fixtures(name, scene).values()))
    want = st.brute_force(scene, sweeps)
    coordinate, _, _, coplanar, segment, _, _, _ = st.contact_kinds(want)
    print(name, dict(coordinate=int(coordinate.sum()), coplanar=int(coplanar.sum()), segment=int(segment.sum())))
    assert coordinate.sum() >= 20 if name == "cornell12" else (coplanar.sum() >= 20 and segment.sum() >= 20)
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.sweep_triangle(sweeps), want)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_spheres_alone_and_a_duplicated_sphere(gpu_ctx, soup):
    """No triangles, so no tree: the spheres' own statement, and sphere 3 coincides with sphere 0: the lower index wins."""
    spheres = np.concatenate([soup.spheres, soup.spheres[:1]])
    scene = dataclasses.replace(soup, vertices=soup.vertices[:0], triangles=soup.triangles[:0], spheres=spheres)
    sweeps = np.concatenate([st.sphere_sweeps(scene, 384, 22), st.five_kinds(soup, 100, 23)])
    sweeps[1::4, 15] = 0.3  # every fourth ends early: some misses more
    want = st.brute_force(scene, sweeps)
    _, t, axis, prim, _ = api.split_triangle_sweep_hits(want)
    hit = prim != st.PRIM_MISS
    assert (~hit).sum() >= 50 and set(prim[hit] & 3) == {0, 1, 2}, "sphere 3 never wins against its copy, sphere 0"
    assert (hit & (t == 0)).sum() >= 50 and (hit & (t > 0)).sum() >= 100
    assert (axis[hit & (t > 0)] == st.AXIS_SPHERE).all() and (axis[~hit | (t == 0)] == st.AXIS_NONE).all()
    gpu_ctx.upload_scene(scene)
    _same(gpu_ctx.sweep_triangle(sweeps), want)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_a_duplicated_triangle_resolves_to_the_lower_index(gpu_ctx, soup, soup_sweeps, soup_want):
    """The soup's triangle array concatenated with itself: every candidate ties bit for bit with its copy 3000 indices on, so every
    answer is the single soup's."""
    doubled = dataclasses.replace(soup, triangles=np.concatenate([soup.triangles, soup.triangles]))
    prim = api.split_triangle_sweep_hits(soup_want)[3]
    assert ((prim < 3000) | (prim >= st.SPHERE_FLAG)).all() and (prim < 3000).sum() > 2000
    gpu_ctx.upload_scene(doubled)
    _same(gpu_ctx.sweep_triangle(soup_sweeps), soup_want)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_answers_do_not_depend_on_the_tree_or_on_a_refit(gpu_ctx, soup, soup_sweeps, soup_want):
    """The device-built tree and the host builder's quality tree give the statement's bytes, and after rt_update_geometry to a moved
    scene the answers are the statement's for that scene: those of a fresh upload."""
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_triangle(soup_sweeps), soup_want)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    _same(gpu_ctx.sweep_triangle(soup_sweeps), soup_want)
    pos = np.ascontiguousarray(soup.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.05, pos.shape)).astype(F32)
    v = soup.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(soup, vertices=v)
    gpu_ctx.update_geometry(moved_pos)
    refitted = gpu_ctx.sweep_triangle(soup_sweeps)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        _same(refitted, fresh.sweep_triangle(soup_sweeps))
    pick = np.arange(0, len(soup_sweeps), 4)
    _same(refitted[pick], st.brute_force(moved, soup_sweeps[pick]))
    assert (refitted.view(np.uint32) != soup_want.view(np.uint32)).any(1).mean() > 0.3


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_counters_change_no_byte_and_the_walk_culls(gpu_ctx, soup, soup_sweeps, soup_want):
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_triangle(soup_sweeps, counters=True), soup_want)
    s = gpu_ctx.stats()
    n, n_tris = len(soup_sweeps), len(soup.triangles)
    print(f"soup, {n} sweeps: {s['node_visits'] / n:.1f} node visits and {s['tri_tests'] / n:.1f} triangle tests per sweep (brute force: {n_tris})")
    assert s["rays"] == n and s["node_visits"] > 0 and 0 < s["tri_tests"] < n * n_tris / 10


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_a_start_in_contact_is_what_overlap_triangle_lists(gpu_ctx, soup):
    """On a scene without spheres, from the two kernels: t == 0 iff rt_overlap_triangle(RT_OVERLAP_ANY) answers 1 for the same
    triangle; then the sweep's prim_id is the lowest key the overlap lists."""
    scene = dataclasses.replace(soup, spheres=soup.spheres[:0])
    sweeps = np.concatenate([st.five_kinds(soup, 3000, 11), st.segments_and_points(soup, 600, 21)])
    gpu_ctx.upload_scene(scene)
    _, t, axis, prim, _ = api.split_triangle_sweep_hits(gpu_ctx.sweep_triangle(sweeps))
    tris = np.ascontiguousarray(sweeps[:, 0:12])
    touches = gpu_ctx.overlap_triangle(tris, 0, any_hit=True)[1].astype(bool)
    at_start = (prim != st.PRIM_MISS) & (t == 0)
    print(f"{at_start.sum()} of {len(sweeps)} start in contact")
    assert at_start.sum() >= 500 and (~at_start).sum() >= 500
    np.testing.assert_array_equal(at_start, touches)
    assert (axis[at_start] == st.AXIS_NONE).all()
    first = gpu_ctx.overlap_triangle(tris, 1)[0][:, 0]
    np.testing.assert_array_equal(prim[at_start], first[at_start])


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_tmax_is_strict_on_both_sides(gpu_ctx, soup, soup_sweeps, soup_want):
    """From each sweep's answer at tmax = inf: nextafter(t, +inf) as tmax gives the same bytes - for a start in contact that is the
    smallest positive tmax - and t itself as tmax gives the miss record carrying that tmax."""
    gpu_ctx.upload_scene(soup)
    first = gpu_ctx.sweep_triangle(soup_sweeps)
    _same(first, soup_want)
    assert (soup_sweeps[:, 15] == INF).all()
    t = first[:, 3].copy()
    hit = api.split_triangle_sweep_hits(first)[3] != st.PRIM_MISS
    assert (hit & (t == 0)).sum() >= 100 and (hit & (t > 0)).sum() >= 1000 and (~hit).sum() >= 100
    q = np.array(soup_sweeps)
    q[:, 15] = np.nextafter(t, INF)
    _same(gpu_ctx.sweep_triangle(q), first)
    q[:, 15] = t
    _same(gpu_ctx.sweep_triangle(q), _miss_records(t))


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_invalid_queries_bad_arguments_and_an_empty_batch(gpu_ctx, soup):
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_triangle(np.zeros((1, 16), F32))
    assert e.value.code == -4, "RT_ERR_NOT_UPLOADED before an upload"
    gpu_ctx.upload_scene(soup)
    nan = F32(np.nan)
    v, d = [[0, 0, 1], [0.3, 0, 1], [0, 0.3, 1.1]], [0, 0, -1]

    def q_(v0=v[0], v1=v[1], v2=v[2], d=d, tmax=INF):
        return [*v0, 0, *v1, 0, *v2, 0, *d, tmax]

    q = np.array([q_(v0=[nan, 0, 1]), q_(v1=[0, nan, 1], tmax=1), q_(v2=[0, 0, INF]), q_(v0=[0, -INF, 1], tmax=2), q_(v2=[nan, nan, nan]),
                  q_(d=[nan, 0, -1]), q_(d=[0, INF, -1]), q_(d=[0, 0, -INF], tmax=3), q_(d=[0, 0, 0]), q_(d=[-0.0, 0, -0.0], tmax=5),
                  q_(tmax=nan), q_(tmax=0.0), q_(tmax=-0.0), q_(tmax=-1.0), q_(tmax=-INF)], F32)
    got = gpu_ctx.sweep_triangle(q, counters=True)
    _same(got, _miss_records(q[:, 15]))
    s = gpu_ctx.stats()
    assert s["node_visits"] == 0 and s["tri_tests"] == 0 and s["rays"] == len(q)
    _same(got, st.brute_force(soup, q))
    good = np.array([q_(), q_(v1=v[0]), q_(v1=v[0], v2=v[0])], F32)  # the same start with a valid query walks; a segment and a point are valid
    _same(gpu_ctx.sweep_triangle(good, counters=True), st.brute_force(soup, good))
    assert gpu_ctx.stats()["node_visits"] >= 3
    assert gpu_ctx.sweep_triangle(np.zeros((0, 16), F32)).shape == (0, 8)
    lib, one, out = gpu_ctx.lib, np.array([q_()], F32), np.full((1, 8), 7.0, F32)
    assert lib.rt_sweep_triangle(gpu_ctx._h, None, C.c_size_t(1), C.c_void_p(out.ctypes.data), C.c_uint32(0)) == -1
    assert lib.rt_sweep_triangle(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), None, C.c_uint32(0)) == -1
    assert lib.rt_sweep_triangle(gpu_ctx._h, C.c_void_p(one.ctypes.data), C.c_size_t(1), C.c_void_p(out.ctypes.data), C.c_uint32(2)) == -1, "unknown flag"
    assert (out == 7.0).all(), "nothing written"
    assert lib.rt_sweep_triangle(gpu_ctx._h, None, C.c_size_t(0), None, C.c_uint32(0)) == 0


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_two_devices_give_the_one_device_bytes(soup, soup_sweeps, soup_want):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_triangle(soup_sweeps), soup_want)
        dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:1")
        _same(ctx.sweep_triangle(dev).cpu().numpy(), soup_want)
