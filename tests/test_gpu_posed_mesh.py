"""Posed meshes on the MI355X (rt_overlap_mesh, rt_sweep_mesh).  The expectation is always the reduction, in numpy
(posed_mesh_cases.reduce_overlap / reduce_sweep), of the EXISTING calls - ctx.overlap_triangle(..., count_all=True, max_prims=0) and
ctx.sweep_triangle - over api.pose_triangles(mesh, poses), compared as uint32 words; for one small set the numpy brute force of
posed_mesh_cases.py is the expectation as well, which ties the chain to the float64-pinned statements."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import posed_mesh_cases as pm
from gpu_raytracer_amd import api, scenes

import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first; these tests need it

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
MISS = 0xFFFFFFFF
MS = (1, 2, 3, 12, 63, 64, 65, 130)  # G = 1, 2, 4, 16, 64, 64 and two and three rounds of 64
NS = (1, 37, 129)                    # a partial last wave at every G (129 at G = 1 too)


def _same(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _mesh(m):
    return pm.box_hull(0.05) if m == 12 else pm.random_mesh(m, 100 + m)


def sweep_expect(ctx, mesh, sweeps):
    """The composition rt_sweep_mesh replaces, on the context's current tree."""
    sweeps = np.asarray(sweeps, F32)
    rec = ctx.sweep_triangle(pm.posed_sweeps(mesh, sweeps)).reshape(len(sweeps), len(mesh), 8)
    return pm.reduce_sweep(rec, sweeps[:, 11], api.pose_frames(sweeps)[1])


def overlap_expect(ctx, mesh, poses):
    tris = api.pose_triangles(mesh, poses)
    counts = ctx.overlap_triangle(tris.reshape(-1, 12), 0, count_all=True)[1].reshape(tris.shape[:2])
    return pm.reduce_overlap(counts, api.pose_frames(poses)[1])


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_sweeps(soup):
    sweeps = pm.soup_pose_sweeps(soup, max(NS), 7)
    sweeps.setflags(write=False)
    return sweeps


@pytest.fixture(scope="module")
def expected(soup, soup_sweeps):
    """m -> (mesh, sweep records, pairs, first) for the 129 poses, by the existing triangle calls, computed once; the sets of 1 and
    37 poses are prefixes of it.  Asserted per mesh of 12 triangles and more, on these 129 poses: at least 20 hit and 5 miss, 10
    start in contact, 10 touch two pairs or more and 10 touch nothing."""
    out = {}
    with api.Context() as ctx:
        ctx.upload_scene(soup)
        poses = np.ascontiguousarray(soup_sweeps[:, :8])
        for m in MS:
            mesh = _mesh(m)
            rec = sweep_expect(ctx, mesh, soup_sweeps)
            pairs, first = overlap_expect(ctx, mesh, poses)
            words = rec.view(np.uint32)
            hit = words[:, 6] != MISS
            print(f"m {m}: {hit.sum()} hit, {(~hit).sum()} miss, {(hit & (words[:, 3] == 0)).sum()} at the start, {(pairs >= 2).sum()} with pairs >= 2, "
                  f"{(pairs == 0).sum()} with none, most pairs {pairs.max()}")
            if m >= 12:
                assert hit.sum() >= 20 and (~hit).sum() >= 5 and (hit & (words[:, 3] == 0)).sum() >= 10
                assert (pairs >= 2).sum() >= 10 and (pairs == 0).sum() >= 10
                assert (words[hit, 5] < m).all() and len(set(words[hit, 5].tolist())) >= 4, "several mesh triangles are the first to touch"
            for a in (mesh, rec, pairs, first):
                a.setflags(write=False)
            out[m] = (mesh, rec, pairs, first)
    return out


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_shapes_equal_the_composition(gpu_ctx, soup, soup_sweeps, expected, m, n):
    """Group widths 1, 2, 4, 16 and 64, a partial group (3, 12, 63), a partial last wave and one, two and three rounds of the loop
    over the mesh."""
    mesh, rec, pairs, first = expected[m]
    gpu_ctx.upload_scene(soup)
    sweeps = np.ascontiguousarray(soup_sweeps[:n])
    _same(gpu_ctx.sweep_mesh(mesh, sweeps), rec[:n])
    s = gpu_ctx.stats()
    assert s["rays"] == n and s["pixels"] == 0 and s["node_visits"] == 0 and s["kernel_ms"] > 0
    got_pairs, got_first = gpu_ctx.overlap_mesh(mesh, np.ascontiguousarray(sweeps[:, :8]), first=True)
    _same(got_pairs, pairs[:n])
    _same(got_first, first[:n])
    _same(gpu_ctx.overlap_mesh(mesh, np.ascontiguousarray(sweeps[:, :8])), pairs[:n])


def test_a_small_set_equals_the_numpy_brute_force(gpu_ctx, soup, soup_sweeps, expected):
    mesh, rec, pairs, first = expected[12]
    sweeps = np.ascontiguousarray(soup_sweeps[:37])
    want = pm.sweep_want(soup, mesh, sweeps)
    _same(rec[:37], want)
    want_pairs, want_first = pm.overlap_want(soup, mesh, sweeps[:, :8])
    _same(pairs[:37], want_pairs)
    _same(first[:37], want_first)
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_mesh(mesh, sweeps), want)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_one_triangle_at_the_identity_is_the_triangle_call(gpu_ctx, soup):
    """m = 1, rotation (0, 0, 0, 1), position 0: sweep_triangle's bytes with triangle = 0 on a hit (PRIM_MISS on a miss), and
    overlap_triangle's counts."""
    import sweep_triangle_cases as st
    tri_sweeps = st.five_kinds(soup, 200, 31)
    gpu_ctx.upload_scene(soup)
    want = np.array(gpu_ctx.sweep_triangle(tri_sweeps)).view(np.uint32)
    counts = gpu_ctx.overlap_triangle(np.ascontiguousarray(tri_sweeps[:, :12]), 0, count_all=True)[1]
    hit = want[:, 6] != MISS
    assert hit.sum() >= 50 and (~hit).sum() >= 10 and (counts > 0).sum() >= 20
    want[:, 5] = np.where(hit, 0, MISS)
    got = np.zeros((len(tri_sweeps), 8), np.uint32)
    got_counts = np.zeros(len(tri_sweeps), np.uint32)
    for i, s in enumerate(tri_sweeps):  # a mesh per sweep: the pose is the identity, so the mesh is the query
        mesh = np.ascontiguousarray(s[None, :12])
        pose = api.make_pose_sweeps(np.zeros((1, 3), F32), np.array([[0, 0, 0, 1]], F32), s[None, 12:15], s[15])
        got[i] = gpu_ctx.sweep_mesh(mesh, pose).view(np.uint32)[0]
        got_counts[i] = gpu_ctx.overlap_mesh(mesh, np.ascontiguousarray(pose[:, :8]))[0]
    _same(got, want)
    _same(got_counts, counts)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_ties_resolve_to_the_lowest_scene_key_then_the_lowest_mesh_triangle(gpu_ctx, soup, soup_sweeps, expected):
    c12 = scenes.cornell12()
    gpu_ctx.upload_scene(c12)
    mesh, sweeps, t, prim, triangle = pm.cornell_drop()
    rec = gpu_ctx.sweep_mesh(mesh, sweeps)
    _same(rec, pm.sweep_want(c12, mesh, sweeps))
    _same(rec, sweep_expect(gpu_ctx, mesh, sweeps))
    w = rec.view(np.uint32)[0]
    assert w[3] == F32(t).view(np.uint32) and w[5] == triangle and w[6] == prim
    mesh, sweeps, triangle = pm.duplicated_triangle(c12)
    rec = gpu_ctx.sweep_mesh(mesh, sweeps)
    _same(rec, pm.sweep_want(c12, mesh, sweeps))
    assert rec.view(np.uint32)[0, 5] == triangle
    # the soup's triangle array concatenated with itself: every candidate ties with its copy 3000 indices on
    doubled = dataclasses.replace(soup, triangles=np.concatenate([soup.triangles, soup.triangles]))
    mesh, rec, pairs, first = expected[64]
    gpu_ctx.upload_scene(doubled)
    _same(gpu_ctx.sweep_mesh(mesh, soup_sweeps), rec)
    got_pairs, got_first = gpu_ctx.overlap_mesh(mesh, np.ascontiguousarray(soup_sweeps[:, :8]), first=True)
    spheres = overlap_expect(gpu_ctx, mesh, np.ascontiguousarray(soup_sweeps[:, :8]))[0]
    _same(got_pairs, spheres)
    assert (got_pairs >= pairs).all() and (got_pairs <= 2 * pairs.astype(np.uint64)).all() and (got_pairs > pairs).sum() >= 10
    _same(got_first, first)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_tmax_is_strict_on_both_sides(gpu_ctx, soup, soup_sweeps, expected):
    """Each pose's own expected t as tmax is a miss carrying that tmax; nextafter above it gives the bytes of tmax = inf."""
    mesh, rec, _, _ = expected[64]
    gpu_ctx.upload_scene(soup)
    words = rec.view(np.uint32)
    t = rec[:, 3].copy()
    q = np.array(soup_sweeps)
    q[:, 11] = np.nextafter(t, INF)
    _same(gpu_ctx.sweep_mesh(mesh, q), rec)
    q[:, 11] = t
    miss = np.zeros((len(q), 8), np.uint32)
    miss[:, 3], miss[:, 4], miss[:, 5], miss[:, 6] = t.view(np.uint32), MISS, MISS, MISS
    got = gpu_ctx.sweep_mesh(mesh, q)
    hit = words[:, 6] != MISS
    _same(got[hit & (t > 0)], miss[hit & (t > 0)])
    _same(got[~hit], miss[~hit])
    # tmax = 0 is an invalid query of every triangle: the miss record, as sweep_triangle gives it
    _same(got[hit & (t == 0)], miss[hit & (t == 0)])


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_any_hit_is_whether_the_count_is_positive(gpu_ctx, soup, soup_sweeps, expected):
    gpu_ctx.upload_scene(soup)
    poses = np.ascontiguousarray(soup_sweeps[:, :8])
    for m in (1, 12, 65, 130):
        mesh, _, pairs, _ = expected[m]
        _same(gpu_ctx.overlap_mesh(mesh, poses, any_hit=True), (pairs > 0).astype(np.uint32))
    mesh = pm.random_mesh(130, 230, edge=0.25, spread=0.2)  # a larger body: many touching pairs per pose
    pairs = overlap_expect(gpu_ctx, mesh, poses)[0]
    print(f"the larger body: most pairs {pairs.max()}, {(pairs >= 100).sum()} poses with a hundred and more")
    assert pairs.max() >= 100, "a pose with a hundred touching pairs and more exercises the early stop"
    _same(gpu_ctx.overlap_mesh(mesh, poses), pairs)
    _same(gpu_ctx.overlap_mesh(mesh, poses, any_hit=True), (pairs > 0).astype(np.uint32))
    with pytest.raises(ValueError):
        gpu_ctx.overlap_mesh(mesh, poses, first=True, any_hit=True)
    pairs_out, first_out = np.full(len(poses), 7, np.uint32), np.full(len(poses), 7, np.uint32)
    rc = gpu_ctx.lib.rt_overlap_mesh(gpu_ctx._h, C.c_void_p(mesh.ctypes.data), C.c_size_t(len(mesh)), C.c_void_p(poses.ctypes.data), C.c_size_t(len(poses)),
                                     C.c_void_p(pairs_out.ctypes.data), C.c_void_p(first_out.ctypes.data), C.c_uint32(api.OVERLAP_ANY))
    assert rc == -1 and (pairs_out == 7).all() and (first_out == 7).all()
    gpu_ctx.overlap_mesh(mesh, poses, any_hit=True, counters=True)
    stopped = gpu_ctx.stats()["tri_tests"]
    gpu_ctx.overlap_mesh(mesh, poses, counters=True)
    print(f"the larger body: {stopped} triangle tests with any_hit, {gpu_ctx.stats()['tri_tests']} counting")
    assert stopped < gpu_ctx.stats()["tri_tests"]


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_invalid_input_and_refusals(gpu_ctx, soup, soup_sweeps, expected):
    mesh, rec, pairs, first = expected[12]
    poses = np.ascontiguousarray(soup_sweeps[:, :8])
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_mesh(mesh, soup_sweeps)
    assert e.value.code == -4, "RT_ERR_NOT_UPLOADED before an upload"
    gpu_ctx.upload_scene(soup)

    def still_answers():
        _same(gpu_ctx.sweep_mesh(mesh, soup_sweeps), rec)
        _same(gpu_ctx.overlap_mesh(mesh, poses), pairs)

    # invalid poses among valid ones: answered without a walk
    names = sorted(pm.INVALID_POSES)
    bad = api.make_pose_sweeps(np.array([pm.INVALID_POSES[k][0] for k in names], F32), np.array([pm.INVALID_POSES[k][1] for k in names], F32),
                               np.array([0, 0, -1], F32), 2.5)
    got = gpu_ctx.sweep_mesh(mesh, bad, counters=True).view(np.uint32)
    assert (got == np.array([0, 0, 0, F32(2.5).view(np.uint32), MISS, MISS, MISS, 0], np.uint32)).all()
    assert gpu_ctx.stats()["node_visits"] == 0 and gpu_ctx.stats()["rays"] == len(bad)
    got_pairs, got_first = gpu_ctx.overlap_mesh(mesh, np.ascontiguousarray(bad[:, :8]), first=True, counters=True)
    assert not got_pairs.any() and (got_first == MISS).all() and gpu_ctx.stats()["node_visits"] == 0
    mixed = np.concatenate([soup_sweeps[:20], bad, soup_sweeps[20:40]])
    _same(gpu_ctx.sweep_mesh(mesh, mixed), np.concatenate([rec[:20], got.view(F32), rec[20:40]]))
    # a mesh triangle with a NaN vertex touches nothing; the others still answer
    holed = np.array(mesh)
    holed[5, 4] = np.nan
    _same(gpu_ctx.sweep_mesh(holed, soup_sweeps), sweep_expect(gpu_ctx, holed, soup_sweeps))
    hp, hf = gpu_ctx.overlap_mesh(holed, poses, first=True)
    wp, wf = overlap_expect(gpu_ctx, holed, poses)
    _same(hp, wp), _same(hf, wf)
    assert (hp <= pairs).all() and (hp < pairs).any() and not (hf == 5).any()
    # a zero direction and tmax <= 0 or NaN: every triangle is a miss
    q = np.array(soup_sweeps[:8])
    q[0:2, 8:11] = 0
    q[2, 11], q[3, 11], q[4, 11], q[5, 11] = 0.0, -1.0, np.nan, -INF
    got = gpu_ctx.sweep_mesh(mesh, q)
    _same(got, sweep_expect(gpu_ctx, mesh, q))
    assert (got.view(np.uint32)[:6, 6] == MISS).all() and (got.view(np.uint32)[:6, 3] == q[:6, 11].view(np.uint32)).all()
    # refused arguments
    with pytest.raises(ValueError):
        gpu_ctx.sweep_mesh(np.zeros((0, 12), F32), soup_sweeps)
    with pytest.raises(ValueError):
        gpu_ctx.overlap_mesh(np.zeros((api.POSED_MESH_MAX + 1, 12), F32), poses)
    lib, out = gpu_ctx.lib, np.full((len(soup_sweeps), 8), 7.0, F32)
    big = np.zeros((api.POSED_MESH_MAX + 1, 12), F32)
    for m_arg, buf in ((0, mesh), (api.POSED_MESH_MAX + 1, big)):
        rc = lib.rt_sweep_mesh(gpu_ctx._h, C.c_void_p(buf.ctypes.data), C.c_size_t(m_arg), C.c_void_p(soup_sweeps.ctypes.data), C.c_size_t(len(soup_sweeps)),
                               C.c_void_p(out.ctypes.data), C.c_uint32(0))
        assert rc == -1 and (out == 7.0).all(), m_arg
        still_answers()
    assert lib.rt_sweep_mesh(gpu_ctx._h, C.c_void_p(mesh.ctypes.data), C.c_size_t(12), C.c_void_p(soup_sweeps.ctypes.data), C.c_size_t(1),
                             C.c_void_p(out.ctypes.data), C.c_uint32(2)) == -1, "unknown flag"
    assert lib.rt_sweep_mesh(gpu_ctx._h, None, C.c_size_t(12), C.c_void_p(soup_sweeps.ctypes.data), C.c_size_t(1), C.c_void_p(out.ctypes.data), C.c_uint32(0)) == -1
    assert lib.rt_sweep_mesh(gpu_ctx._h, None, C.c_size_t(0), None, C.c_size_t(0), None, C.c_uint32(0)) == 0, "n = 0"
    assert (out == 7.0).all()
    assert gpu_ctx.sweep_mesh(mesh, np.zeros((0, 12), F32)).shape == (0, 8)
    # mixed host and device buffers, and a misaligned device tensor
    dev_sweeps, dev_mesh = torch.from_numpy(np.array(soup_sweeps)).to("cuda:0"), torch.from_numpy(np.array(mesh)).to("cuda:0")
    for a, b in ((mesh, dev_sweeps), (dev_mesh, np.array(soup_sweeps))):
        with pytest.raises(api.RtError) as e:
            gpu_ctx.sweep_mesh(a, b)
        assert e.value.code == -1
        still_answers()
    with pytest.raises(api.RtError) as e:
        gpu_ctx.overlap_mesh(mesh, dev_sweeps[:, :8].contiguous())
    assert e.value.code == -1
    buf = torch.zeros(len(mesh) * 12 + 1, device="cuda:0")
    buf[1:] = dev_mesh.reshape(-1)
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_mesh(buf[1:].view(-1, 12), dev_sweeps)
    assert e.value.code == -1 and "aligned" in str(e.value)
    still_answers()
    _same(gpu_ctx.sweep_mesh(dev_mesh, dev_sweeps).cpu().numpy(), rec)


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_host_device_and_preallocated_memory_give_the_same_bytes(gpu_ctx, soup, soup_sweeps, expected):
    mesh, rec, pairs, first = expected[65]
    gpu_ctx.upload_scene(soup)
    own = np.full((len(soup_sweeps), 8), 7.0, F32)
    assert gpu_ctx.sweep_mesh(mesh, soup_sweeps, out=own) is own
    _same(own, rec)
    dev_sweeps = torch.from_numpy(np.array(soup_sweeps)).to("cuda:0") * 1.0  # produced by kernels on torch's stream
    dev_mesh = torch.from_numpy(np.array(mesh)).to("cuda:0") * 1.0
    got = gpu_ctx.sweep_mesh(dev_mesh, dev_sweeps)
    assert got.device == dev_sweeps.device and got.dtype == torch.float32
    _same(got.cpu().numpy(), rec)
    out = torch.empty((len(soup_sweeps), 8), device="cuda:0")
    assert gpu_ctx.sweep_mesh(dev_mesh, dev_sweeps, out=out) is out
    _same(out.cpu().numpy(), rec)
    dev_poses = dev_sweeps[:, :8].contiguous()
    got_pairs, got_first = gpu_ctx.overlap_mesh(dev_mesh, dev_poses, first=True)
    assert got_pairs.device == dev_poses.device and got_pairs.dtype == torch.int32
    _same(got_pairs.cpu().numpy(), pairs)
    _same(got_first.cpu().numpy(), first)
    _same(gpu_ctx.overlap_mesh(dev_mesh, dev_poses, any_hit=True).cpu().numpy(), (pairs > 0).astype(np.uint32))


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_counters(gpu_ctx, soup, soup_sweeps, expected):
    mesh, rec, pairs, first = expected[64]
    gpu_ctx.upload_scene(soup)
    for _ in range(3):
        _same(gpu_ctx.sweep_mesh(mesh, soup_sweeps), rec)
    _same(gpu_ctx.sweep_mesh(mesh, soup_sweeps, counters=True), rec)
    s = gpu_ctx.stats()
    assert s["rays"] == len(soup_sweeps) and s["node_visits"] > 0 and s["tri_tests"] > 0
    shared = s["node_visits"]
    gpu_ctx.sweep_triangle(pm.posed_sweeps(mesh, soup_sweeps), counters=True)
    per_triangle = gpu_ctx.stats()["node_visits"]
    print(f"m 64, {len(soup_sweeps)} poses: {shared} node visits of sweep_mesh, {per_triangle} of sweep_triangle over the posed triangles: "
          f"ratio {shared / per_triangle:.3f}")
    assert shared <= per_triangle
    got_pairs, got_first = gpu_ctx.overlap_mesh(mesh, np.ascontiguousarray(soup_sweeps[:, :8]), first=True, counters=True)
    _same(got_pairs, pairs), _same(got_first, first)
    assert gpu_ctx.stats()["node_visits"] > 0


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_answers_do_not_depend_on_the_tree_or_on_a_refit(gpu_ctx, soup, soup_sweeps, expected):
    """The device tree, the host builder's quality tree and a refitted tree: the composition's bytes on the same tree state."""
    mesh, rec, pairs, first = expected[12]
    poses = np.ascontiguousarray(soup_sweeps[:, :8])
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_mesh(mesh, soup_sweeps), rec)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    _same(gpu_ctx.sweep_mesh(mesh, soup_sweeps), rec)
    _same(gpu_ctx.overlap_mesh(mesh, poses), pairs)
    pos = np.ascontiguousarray(soup.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.05, pos.shape)).astype(F32)
    gpu_ctx.update_geometry(moved_pos)
    refitted = gpu_ctx.sweep_mesh(mesh, soup_sweeps)
    _same(refitted, sweep_expect(gpu_ctx, mesh, soup_sweeps))
    got_pairs, got_first = gpu_ctx.overlap_mesh(mesh, poses, first=True)
    want_pairs, want_first = overlap_expect(gpu_ctx, mesh, poses)
    _same(got_pairs, want_pairs), _same(got_first, want_first)
    assert (refitted.view(np.uint32) != rec.view(np.uint32)).any(1).mean() > 0.2


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_two_devices_give_the_one_device_bytes(soup, soup_sweeps, expected):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    mesh, rec, pairs, first = expected[65]
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_mesh(mesh, soup_sweeps), rec)
        got_pairs, got_first = ctx.overlap_mesh(mesh, np.ascontiguousarray(soup_sweeps[:, :8]), first=True)
        _same(got_pairs, pairs), _same(got_first, first)
        dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:1")
        _same(ctx.sweep_mesh(torch.from_numpy(np.array(mesh)).to("cuda:1"), dev).cpu().numpy(), rec)
