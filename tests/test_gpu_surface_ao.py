"""Surface and ambient-occlusion queries on the MI355X (rt_surface, rt_ambient_occlusion), held to calls that already exist.

rt_surface: prim_id is rt_intersect's, position is numpy float32 o + d * t with rt_intersect's t, bit for bit (the library is built
with -ffp-contract=off, so numpy reproduces every rounding); the normal is rt_aovs' on camera rays, bit for bit, and the numpy normal of
the scene's own vertices within 1e-6; material_id is the scene's.
rt_ambient_occlusion: every one of the n * S rays of its definition is built here in numpy float32 (rng_for and the LCG in uint32, the
oracle's unit_vector, normalize, P + N * bias) and traced by rt_occluded; the counts must be equal as integers and the visibility the
bits of count / S, whatever the sample count, the buffers' kind, the chunking, the device count and the tree."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from gpu_raytracer_amd import api, scenes

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
MISS = 0xFFFFFFFF
MIN_T = F32(1e-5)
W, H = 96, 64


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_bits(a, b, what=""):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


# test_gpu_aovs' helpers, restated ----------------------------------------------------------------------------------------------
def _normalize(a):
    with np.errstate(all="ignore"):
        length = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]).astype(F32)
        return a * (F32(1.0) / length)[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2],
                     a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def _surface(scene, rays, t, prim):
    """Per ray: hit mask, face-forwarded geometric normal and material id from the scene's own arrays."""
    n = len(rays)
    hit = prim != MISS
    sphere = hit & (prim >= 0x80000000)
    tri = hit & ~sphere
    normal = np.zeros((n, 3), F32)
    mid = np.zeros(n, np.int64)
    pos = scene.vertices["position"].astype(F32)
    if tri.any():
        trs = scene.triangles[prim[tri].astype(np.int64)]
        v0 = pos[trs["v0_index"]]
        normal[tri] = _normalize(_cross(pos[trs["v1_index"]] - v0, pos[trs["v2_index"]] - v0))
        mid[tri] = trs["material_id"]
    if sphere.any():
        sp = scene.spheres[(prim[sphere] & 0x7FFFFFFF).astype(np.int64)]
        point = rays[sphere, 0:3] + rays[sphere, 4:7] * t[sphere, None]
        normal[sphere] = _normalize(point - sp["center"].astype(F32))
        mid[sphere] = sp["material_id"]
    d = rays[:, 4:7]
    front = ((d[:, 0] * normal[:, 0] + d[:, 1] * normal[:, 1]) + d[:, 2] * normal[:, 2]) < 0
    return hit, np.where(front[:, None], normal, -normal), mid


# scenes and rays ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_of():
    made = {"cornell12": scenes.cornell12(), "soup": scenes.random_soup(2000, n_spheres=3)}
    return made.__getitem__


def _incoherent_rays(scene, n, seed):
    """Origins in and around the scene's box, random directions (a quarter not normalised), finite tmax."""
    rng = np.random.default_rng(seed)
    p = scene.vertices["position"].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    size = float(np.linalg.norm(hi - lo))
    o = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (n, 3)).astype(F32)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: n // 4] *= rng.uniform(0.1, 10, (n // 4, 1))
    tmax = rng.uniform(0.1 * size, 1.5 * size, n).astype(F32)
    return api.make_rays(o, d.astype(F32), MIN_T, tmax)


def _degenerate_rays(good):
    nan = F32(np.nan)
    bad = np.tile(good[:1], (4, 1))
    bad[0, 0] = nan                    # origin NaN
    bad[1, 4:7] = 0                    # zero direction
    bad[2, 3], bad[2, 7] = 2.0, 2.0    # tmin == tmax
    bad[3, 3], bad[3, 7] = 3.0, 1.0    # tmin > tmax
    return bad


def _query_rays(ctx, scene):
    """The camera rays of a 96 x 64 mode-1 frame, then 4096 incoherent rays."""
    cam = ctx.camera_rays(W, H, scene.camera, mode=1)
    return np.concatenate([cam, _incoherent_rays(scene, 4096, seed=21)])


def _miss_records(n):
    rec = np.zeros((n, 8), F32)
    rec[:, 3] = np.full(n, MISS, U32).view(F32)
    return rec


# rt_surface --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell12", "soup"])
def test_surface_against_existing_calls(gpu_ctx, scene_of, name):
    scene = scene_of(name)
    gpu_ctx.upload_scene(scene)
    rays = _query_rays(gpu_ctx, scene)
    bad = _degenerate_rays(rays)
    rays = np.concatenate([rays, bad])
    n_cam = W * H
    t, _, _, prim = api.split_hits(gpu_ctx.intersect(rays))
    pts = gpu_ctx.surface(rays)
    st = gpu_ctx.stats()
    assert st["rays"] == len(rays) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["kernel_ms"] > 0
    assert st["node_visits"] == 0 and st["tri_tests"] == 0
    assert pts.shape == (len(rays), 8) and pts.dtype == F32
    position, prim_id, normal, material_id = api.split_surface(pts)
    hit = prim != MISS
    assert hit[:n_cam].any() and (~hit[:n_cam]).any() and hit[n_cam:].any() and (~hit[n_cam:-4]).any()
    np.testing.assert_array_equal(prim_id, prim)
    with np.errstate(all="ignore"):
        want_pos = rays[:, 0:3] + rays[:, 4:7] * t[:, None]
    _assert_bits(position[hit], want_pos[hit], "position == o + d * t")
    # rt_aovs' normal of a one-sample pixel is its reduction (0 + nf) / 1 of the same nf: the bits of nf, but for a zero's sign
    aov = api.split_aovs(gpu_ctx.aovs(W, H, scene.camera, mode=1).reshape(-1, 8))
    _assert_bits((F32(0) + normal[:n_cam]) / F32(1), aov["normal"], "normal == rt_aovs' normal")
    np.testing.assert_array_equal(normal[:n_cam] == 0, aov["normal"] == 0)
    np.testing.assert_array_equal(hit[:n_cam].astype(F32), aov["coverage"])
    want_hit, want_nf, want_mid = _surface(scene, rays, t, prim)
    np.testing.assert_allclose(normal[hit], want_nf[hit], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(material_id[hit], want_mid[hit].astype(U32))
    if name == "soup":
        assert ((prim >= 0x80000000) & hit).any(), "spheres among the hits"
    # misses and degenerate rays: the all-zero record but for prim_id
    assert not hit[-4:].any()
    assert pts[~hit].tobytes() == _miss_records(int((~hit).sum())).tobytes()
    # counters: the walk is rt_intersect's
    gpu_ctx.intersect(rays, counters=True)
    one = gpu_ctx.stats()
    assert gpu_ctx.surface(rays, counters=True).tobytes() == pts.tobytes()
    st = gpu_ctx.stats()
    assert st["node_visits"] == one["node_visits"] > 0 and st["tri_tests"] == one["tri_tests"] > 0 and st["rays"] == len(rays)
    # the tree does not matter
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.stats()["tree_build"] == 0
    assert gpu_ctx.surface(rays).tobytes() == pts.tobytes()
    # own output array; torch tensors on the host and on the device
    own = np.full((len(rays), 8), 7, F32)
    assert gpu_ctx.surface(rays, out=own) is own and own.tobytes() == pts.tobytes()
    if torch is not None:
        dev = torch.from_numpy(rays).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
        got = gpu_ctx.surface(dev)
        assert got.device == dev.device and got.dtype == torch.float32 and tuple(got.shape) == (len(rays), 8)
        assert got.cpu().numpy().tobytes() == pts.tobytes()
        assert gpu_ctx.surface(torch.from_numpy(rays.copy())).numpy().tobytes() == pts.tobytes()
        _, tprim, _, tmat = api.split_surface(got)
        np.testing.assert_array_equal(tprim.cpu().numpy(), prim.astype(np.int64))
        np.testing.assert_array_equal(tmat.cpu().numpy(), material_id.astype(np.int64))


def test_surface_of_an_empty_scene_and_after_a_geometry_update(gpu_ctx, scene_of):
    soup = scene_of("soup")
    gpu_ctx.upload_scene(soup)
    rays = _query_rays(gpu_ctx, soup)
    before = gpu_ctx.surface(rays)
    pos = soup.vertices["position"].astype(F32)
    moved_pos = np.ascontiguousarray(pos + F32(0.2) * np.sin(pos[:, ::-1] * F32(3.0)), dtype=F32)
    v = soup.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(soup, vertices=v)
    assert gpu_ctx.update_geometry(vertices=moved_pos)["flags"] & (api.STAT_REFIT | api.STAT_REBUILT)
    after = gpu_ctx.surface(rays)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        want = fresh.surface(rays)
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()
    t, _, _, prim = api.split_hits(gpu_ctx.intersect(rays))
    hit, want_nf, want_mid = _surface(moved, rays, t, prim)
    np.testing.assert_allclose(after[hit, 4:7], want_nf[hit], rtol=0, atol=1e-6)  # the moved triangles' normals, not the uploaded ones'
    gpu_ctx.upload_scene(scenes.empty_scene())
    assert gpu_ctx.surface(rays).tobytes() == _miss_records(len(rays)).tobytes()
    vis, cnt = gpu_ctx.ambient_occlusion(before[:100], 5)
    assert np.all(cnt == 5) and np.all(vis == 1)


# rt_ambient_occlusion against its definition -----------------------------------------------------------------------------------
def _rng_for(pixel_seed, sample):
    h = pixel_seed + sample * U32(0x9E3779B9)
    h = h ^ (h >> U32(16))
    h = h * U32(0x7FEB352D)
    h = h ^ (h >> U32(15))
    h = h * U32(0x846CA68B)
    return h ^ (h >> U32(16))


def _next(state):
    state = state * U32(1664525) + U32(1013904223)
    return state, (state >> U32(8)).astype(F32) / F32(16777216.0)


def compose_rays(oracle_mod, points, index, samples, seed, max_distance, bias):
    """The rays of the definition for the points `points` whose indices in the caller's array are `index` -> (len * samples, 8), point-major."""
    index = np.asarray(index, np.uint64)
    pixel_seed = ((np.uint64(seed) + index) & np.uint64(0xFFFFFFFF)).astype(U32)
    state = _rng_for(pixel_seed[:, None], np.arange(samples, dtype=U32)[None, :])
    state, u1 = _next(state)
    state, u2 = _next(state)
    unit = oracle_mod.unit_vectors(u1, u2)[0].reshape(len(index), samples, 3)
    P, N = points[:, None, 0:3], points[:, None, 4:7]
    with np.errstate(all="ignore"):
        d = _normalize(N + unit)
        o = np.broadcast_to(P + N * F32(bias), d.shape)
    return api.make_rays(o.reshape(-1, 3), d.reshape(-1, 3), MIN_T, F32(max_distance))


def _is_point(points):
    with np.errstate(all="ignore"):
        return np.isfinite(points[:, 0:3]).all(1) & np.isfinite(points[:, 4:7]).all(1) & (points[:, 4:7] != 0).any(1)


def reference(ctx, oracle_mod, points, index, samples, seed, max_distance, bias, counters=False):
    """unoccluded = samples - the sum of rt_occluded over the composed rays; a record that is no point: samples.  -> (counts, occluded fraction)"""
    occ = ctx.occluded(compose_rays(oracle_mod, points, index, samples, seed, max_distance, bias), counters=counters).reshape(len(points), samples)
    real = _is_point(points)
    counts = np.where(real, samples - occ.sum(1), samples).astype(U32)
    return counts, float(occ[real].mean()) if real.any() else 0.0


def _ao_points(ctx, scene):
    """257 records: 254 hits of rt_surface (camera rays and incoherent rays), then a NaN position, a zero normal and an inf normal."""
    pts = ctx.surface(_query_rays(ctx, scene))
    rows = np.flatnonzero(_bits(pts[:, 3]) != MISS)
    pts = pts[rows[np.linspace(0, len(rows) - 1, 254).astype(np.int64)]]
    odd = np.tile(pts[:1], (3, 1))
    odd[0, 1] = np.nan
    odd[1, 4:7] = 0
    odd[2, 5] = np.inf
    return np.ascontiguousarray(np.concatenate([pts, odd]))


MAIN = dict(samples=64, seed=0xFFFFFF80, bias=1e-3)  # seed + i wraps at i = 128


def _finite_distance(ctx, oracle_mod, points):
    """A max_distance picked from the reference alone: the median distance at which the main case's rays, unbounded, first hit something."""
    rays = compose_rays(oracle_mod, points, np.arange(len(points)), MAIN["samples"], MAIN["seed"], np.inf, MAIN["bias"])
    t, _, _, prim = api.split_hits(ctx.intersect(rays))
    return float(np.median(t[prim != MISS]))


def _check_ao(ctx, oracle_mod, points, samples, seed, max_distance, bias, index=None, occluded_between=None):
    n = len(points)
    want, fraction = reference(ctx, oracle_mod, points, np.arange(n) if index is None else index, samples, seed, max_distance, bias)
    if occluded_between:
        assert occluded_between[0] <= fraction <= occluded_between[1], f"the reference has {fraction:.3f} of its samples occluded"
    if index is not None:
        return want
    vis, cnt = ctx.ambient_occlusion(points, samples, seed=seed, max_distance=max_distance, bias=bias)
    st = ctx.stats()
    assert st["rays"] == n * samples and st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["tri_tests"] == 0
    assert cnt.dtype == U32 and cnt.shape == (n,) and vis.dtype == F32 and vis.shape == (n,)
    np.testing.assert_array_equal(cnt, want)
    _assert_bits(vis, want.astype(F32) / F32(samples), "visibility == count / samples")
    if torch is not None:  # device-resident buffers: the same result
        dev = torch.from_numpy(points).to("cuda:0") * 1.0
        tv, tc = ctx.ambient_occlusion(dev, samples, seed=seed, max_distance=max_distance, bias=bias)
        assert tv.device == dev.device and tc.device == dev.device and tv.dtype == torch.float32 and tc.dtype == torch.int32
        np.testing.assert_array_equal(tc.cpu().numpy().astype(U32), want)
        _assert_bits(tv.cpu().numpy(), vis)
    return want


# (samples, n, seed, bias, finite max_distance)
CASES = [(1, 257, 0, 0.0, False), (3, 257, 12345, 1e-3, True), (64, 257, MAIN["seed"], MAIN["bias"], True), (65, 257, 0xFFFFFFFF, 0.0, True),
         (100, 257, 7, 1e-3, False), (4096, 3, 99, 1e-3, True), (7, 1, 5, 0.0, False)]


@pytest.mark.parametrize("samples,n,seed,bias,finite", CASES, ids=[f"S{c[0]}-n{c[1]}" for c in CASES])
@pytest.mark.parametrize("name", ["cornell12", "soup"])
def test_ao_equals_its_definition(gpu_ctx, oracle_mod, scene_of, name, samples, n, seed, bias, finite):
    scene = scene_of(name)
    gpu_ctx.upload_scene(scene)
    pts = _ao_points(gpu_ctx, scene)
    dist = _finite_distance(gpu_ctx, oracle_mod, pts) if finite else np.inf
    main = samples == MAIN["samples"]
    rows = {257: slice(None), 3: [5, 130, 255], 1: [17]}[n]  # 255: the zero normal
    want = _check_ao(gpu_ctx, oracle_mod, np.ascontiguousarray(pts[rows]), samples, seed, dist, bias, occluded_between=(0.1, 0.9) if main else None)
    if n == 257:
        assert np.all(want[-3:] == samples), "records that are no points trace nothing"
    if main:
        assert want[:-3].min() < want[:-3].max() <= samples


def test_ao_does_not_depend_on_devices_tree_or_outputs(gpu_ctx, oracle_mod, scene_of):
    scene = scene_of("soup")
    gpu_ctx.upload_scene(scene)
    pts = _ao_points(gpu_ctx, scene)
    kw = dict(seed=3, max_distance=_finite_distance(gpu_ctx, oracle_mod, pts), bias=1e-3)
    vis, cnt = gpu_ctx.ambient_occlusion(pts, 100, **kw)
    np.testing.assert_array_equal(cnt, reference(gpu_ctx, oracle_mod, pts, np.arange(len(pts)), 100, kw["seed"], kw["max_distance"], kw["bias"])[0])
    with api.Context((0, 0)) as two:  # each device gets a contiguous range of the points, the indices stay the caller's
        two.upload_scene(scene)
        v2, c2 = two.ambient_occlusion(pts, 100, **kw)
        assert two.stats()["rays"] == len(pts) * 100
    np.testing.assert_array_equal(c2, cnt)
    _assert_bits(v2, vis)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.stats()["tree_build"] == 0
    own_v, own_c = np.full(len(pts), 7, F32), np.full(len(pts), 7, U32)
    got = gpu_ctx.ambient_occlusion(pts, 100, out=own_v, counts=own_c, **kw)
    assert got[0] is own_v and got[1] is own_c
    np.testing.assert_array_equal(own_c, cnt)
    _assert_bits(own_v, vis)
    # either output alone
    ap = np.zeros((), api.T.AO_PARAMS)
    ap["samples"], ap["seed"], ap["max_distance"], ap["bias"] = 100, kw["seed"], kw["max_distance"], kw["bias"]
    call = lambda v, c: gpu_ctx.lib.rt_ambient_occlusion(gpu_ctx._h, C.c_void_p(pts.ctypes.data), C.c_size_t(len(pts)), C.c_void_p(ap.ctypes.data),
                                                          C.c_void_p(v), C.c_void_p(c))
    only_v, only_c = np.zeros(len(pts), F32), np.zeros(len(pts), U32)
    assert call(only_v.ctypes.data, 0) == 0 and call(0, only_c.ctypes.data) == 0
    _assert_bits(only_v, vis)
    np.testing.assert_array_equal(only_c, cnt)
    if torch is not None:
        dev = torch.from_numpy(pts).to("cuda:0")
        tv = torch.empty(len(pts), device="cuda:0")
        buf = torch.zeros(len(pts) + 1, dtype=torch.int32, device="cuda:0")  # counts 4 bytes off 16-byte alignment: fine
        got = gpu_ctx.ambient_occlusion(dev, 100, out=tv, counts=buf[1:], **kw)
        assert got[0] is tv
        np.testing.assert_array_equal(buf[1:].cpu().numpy().astype(U32), cnt)
        _assert_bits(tv.cpu().numpy(), vis)
        skew = torch.zeros(len(pts) * 8 + 4, device="cuda:0")[1:1 + len(pts) * 8].view(-1, 8)
        with pytest.raises(api.RtError) as e:
            gpu_ctx.ambient_occlusion(skew, 100, **kw)
        assert e.value.code == -1 and "aligned" in str(e.value)
        rc = gpu_ctx.lib.rt_ambient_occlusion(gpu_ctx._h, C.c_void_p(dev.data_ptr()), C.c_size_t(len(pts)), C.c_void_p(ap.ctypes.data),
                                              C.c_void_p(tv.data_ptr()), C.c_void_p(only_c.ctypes.data))  # device points, host counts
        assert rc == -1


def _many_points(ctx, scene, n):
    pts = ctx.surface(ctx.camera_rays(W, H, scene.camera, mode=1))
    pts = pts[_bits(pts[:, 3]) != MISS]
    assert len(pts) >= 1024
    return np.ascontiguousarray(np.resize(pts, (n, 8)))  # the same point at another index is another point: its seed differs


def test_ao_host_batch_across_a_chunk_boundary(gpu_ctx, oracle_mod, scene_of):
    scene = scene_of("cornell12")
    gpu_ctx.upload_scene(scene)
    samples = api.AO_MAX_SAMPLES
    n = api.QUERY_CHUNK // samples + 5
    assert n == 1029
    pts = _many_points(gpu_ctx, scene, n)
    kw = dict(seed=0xFFFFFC00, max_distance=1.0, bias=1e-3)
    vis, cnt = gpu_ctx.ambient_occlusion(pts, samples, **kw)  # two chunks: 1024 points and 5
    assert gpu_ctx.stats()["rays"] == n * samples
    if torch is not None:
        tv, tc = gpu_ctx.ambient_occlusion(torch.from_numpy(pts).to("cuda:0"), samples, **kw)  # one device-resident call
        np.testing.assert_array_equal(tc.cpu().numpy().astype(U32), cnt)
        _assert_bits(tv.cpu().numpy(), vis)
    index = np.array([0, 1023, 1024, n - 1])
    want = _check_ao(gpu_ctx, oracle_mod, np.ascontiguousarray(pts[index]), samples, kw["seed"], kw["max_distance"], kw["bias"], index=index)
    np.testing.assert_array_equal(cnt[index], want)
    _assert_bits(vis[index], want.astype(F32) / F32(samples))
    assert len(np.unique(cnt)) > 16


def test_ao_samples_that_straddle_kernel_launches(gpu_ctx, oracle_mod, scene_of):
    """A device-resident batch of more lanes than one launch takes (RT_AO_LAUNCH_LANES = 2^26 in csrc/surface_query.h), with a sample
    count that does not divide it: the point at the cut has samples in both launches, and every point behind it is traced by the second.
    Without torch there is no device-resident batch; the host-chunked call is then still held to the definition."""
    launch = 1 << 26
    scene = scene_of("cornell12")
    gpu_ctx.upload_scene(scene)
    samples, n = 4095, 16400
    cut = launch // samples  # the point with samples on both sides of the cut
    assert n * samples > launch and 0 < launch % samples and cut + 1 < n
    pts = _many_points(gpu_ctx, scene, n)
    kw = dict(seed=11, max_distance=1.0, bias=1e-3)
    vis, cnt = gpu_ctx.ambient_occlusion(pts, samples, **kw)  # chunks of 1024 points: other cuts, no launch of more than 2^22 lanes
    index = np.array([0, cut - 1, cut, cut + 1, n - 1])
    want = _check_ao(gpu_ctx, oracle_mod, np.ascontiguousarray(pts[index]), samples, kw["seed"], kw["max_distance"], kw["bias"], index=index)
    np.testing.assert_array_equal(cnt[index], want)
    assert len(np.unique(cnt[cut:])) > 1  # the points of the second launch are not all alike
    if torch is not None:
        tv, tc = gpu_ctx.ambient_occlusion(torch.from_numpy(pts).to("cuda:0"), samples, **kw)  # one chunk, two launches
        assert gpu_ctx.stats()["rays"] == n * samples
        np.testing.assert_array_equal(tc.cpu().numpy().astype(U32)[index], want)
        np.testing.assert_array_equal(tc.cpu().numpy().astype(U32), cnt)
        _assert_bits(tv.cpu().numpy(), vis)


def test_ao_counters_are_those_of_the_composed_rays(gpu_ctx, oracle_mod, scene_of):
    scene = scene_of("soup")
    gpu_ctx.upload_scene(scene)
    pts = np.ascontiguousarray(_ao_points(gpu_ctx, scene)[:200])
    samples, seed, bias = 24, 8, 1e-3
    dist = _finite_distance(gpu_ctx, oracle_mod, pts)
    want, _ = reference(gpu_ctx, oracle_mod, pts, np.arange(len(pts)), samples, seed, dist, bias, counters=True)
    composed = gpu_ctx.stats()
    assert composed["node_visits"] > 0 and composed["tri_tests"] > 0 and composed["rays"] == len(pts) * samples
    _, cnt = gpu_ctx.ambient_occlusion(pts, samples, seed=seed, max_distance=dist, bias=bias, counters=True)
    st = gpu_ctx.stats()
    np.testing.assert_array_equal(cnt, want)
    assert st["rays"] == len(pts) * samples and st["kernel_ms"] > 0
    assert st["node_visits"] == composed["node_visits"] and st["tri_tests"] == composed["tri_tests"]
    gpu_ctx.ambient_occlusion(pts, samples, seed=seed, max_distance=dist, bias=bias)
    st = gpu_ctx.stats()
    assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(pts) * samples


# side effects and errors -------------------------------------------------------------------------------------------------------
def test_the_frame_and_a_running_accumulation_are_left_alone(gpu_ctx, scene_of):
    scene = scene_of("soup")
    gpu_ctx.upload_scene(scene)
    gpu_ctx.render(W, H, scene.camera, mode=1)
    rgb, comb, hits = gpu_ctx.read_rgb32f(), gpu_ctx.read_rgba8_combined(), gpu_ctx.read_hits()
    pts = gpu_ctx.surface(_query_rays(gpu_ctx, scene))
    gpu_ctx.ambient_occlusion(pts, 16)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.read_rgba8_combined().tobytes() == comb.tobytes()
    again = gpu_ctx.read_hits()
    assert again[0].tobytes() == hits[0].tobytes() and again[1].tobytes() == hits[1].tobytes()
    gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    gpu_ctx.surface(_query_rays(gpu_ctx, scene))
    gpu_ctx.ambient_occlusion(pts, 16, counters=True)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4


def test_the_librarys_own_checks(gpu_ctx, scene_of):
    scene = scene_of("cornell12")
    rays = np.ascontiguousarray(_incoherent_rays(scene, 64, seed=2))
    pts, vis, cnt = np.full((64, 8), 7, F32), np.full(64, 7, F32), np.full(64, 7, U32)
    ap = np.zeros((), api.T.AO_PARAMS)
    ap["samples"], ap["max_distance"], ap["bias"] = 8, np.inf, 1e-3
    lib, h = gpu_ctx.lib, gpu_ctx._h
    surface = lambda r, n, o, flags=0: lib.rt_surface(h, C.c_void_p(r), C.c_size_t(n), C.c_void_p(o), C.c_uint32(flags))
    ao = lambda p, n, a, v, c: lib.rt_ambient_occlusion(h, C.c_void_p(p), C.c_size_t(n), C.c_void_p(a), C.c_void_p(v), C.c_void_p(c))
    assert surface(rays.ctypes.data, 64, pts.ctypes.data) == -4  # before any upload
    assert ao(pts.ctypes.data, 64, ap.ctypes.data, vis.ctypes.data, cnt.ctypes.data) == -4
    gpu_ctx.upload_scene(scene)
    assert surface(0, 0, 0) == 0 and ao(0, 0, 0, 0, 0) == 0  # n == 0
    assert surface(0, 64, pts.ctypes.data) == -1 and surface(rays.ctypes.data, 64, 0) == -1
    assert surface(rays.ctypes.data, 64, pts.ctypes.data, 2) == -1  # RT_QUERY_COUNT_ALL is not a flag of rt_surface
    assert ao(0, 64, ap.ctypes.data, vis.ctypes.data, cnt.ctypes.data) == -1
    assert ao(pts.ctypes.data, 64, 0, vis.ctypes.data, cnt.ctypes.data) == -1
    assert ao(pts.ctypes.data, 64, ap.ctypes.data, 0, 0) == -1
    for field, bad in (("samples", 0), ("samples", 4097), ("max_distance", 0.0), ("max_distance", -1.0), ("max_distance", np.nan),
                       ("bias", -1e-3), ("bias", np.inf), ("bias", np.nan), ("flags", 2)):
        p = ap.copy()
        p[field] = bad
        assert ao(pts.ctypes.data, 64, p.ctypes.data, vis.ctypes.data, cnt.ctypes.data) == -1, (field, bad)
        assert field.split("_")[0] in gpu_ctx.lib.rt_last_error(h).decode() or field == "flags"
    assert np.all(pts == 7) and np.all(vis == 7) and np.all(cnt == 7), "a rejected call changes nothing"
    assert surface(rays.ctypes.data, 64, pts.ctypes.data) == 0
    assert ao(pts.ctypes.data, 64, ap.ctypes.data, vis.ctypes.data, cnt.ctypes.data) == 0
    assert np.all(cnt <= 8) and np.all(vis == cnt.astype(F32) / F32(8))
