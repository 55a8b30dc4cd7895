"""Geometry updates on the MI355X (rt_update_geometry): refit, rebuild, and what follows them, every comparison bit-exact.

Closest hits do not depend on the tree, so the reference for every check is a second context that uploads the moved scene fresh:
after an update, queries, hit records, rgba8 frames and extended-mode float images must be exactly that context's."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 96, 64


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _positions(scene):
    return np.ascontiguousarray(scene.vertices["position"], dtype=F32)


def _moved(scene, pos, spheres=None):
    v = scene.vertices.copy()
    v["position"] = pos
    return dataclasses.replace(scene, vertices=v, spheres=scene.spheres if spheres is None else spheres)


def _motion(scene, kind, seed=0):
    """New positions: 'jitter' per vertex, 'rigid' rotation + translation of a third of the vertices, 'large' half the vertices
    carried across the scene's box."""
    p = _positions(scene).astype(np.float64)
    rng = np.random.default_rng(seed)
    lo, hi = p.min(0), p.max(0)
    ext = float((hi - lo).max())
    if kind == "jitter":
        p = p + rng.normal(0.0, 0.003 * ext, p.shape)
    elif kind == "rigid":
        sub = np.arange(len(p)) < len(p) // 3
        a = 0.4
        rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c = p[sub].mean(0)
        p[sub] = (p[sub] - c) @ rot.T + c + np.array([0.05, 0.02, -0.03]) * ext
    elif kind == "large":
        sub = np.arange(len(p)) % 2 == 0
        p[sub] = p[sub] + np.array([0.6, 0.0, 0.3]) * (hi - lo)
    return np.ascontiguousarray(p.astype(F32))


def _rays(scene, n=4096, seed=7):
    """Rays from around the scene's box toward random points inside it, plus the camera's own pixel rays."""
    p = _positions(scene)
    rng = np.random.default_rng(seed)
    lo, hi = p.min(0), p.max(0)
    c, ext = (lo + hi) / 2, (hi - lo).max() + 1e-3
    o = (c + rng.normal(0, 1, (n, 3)) * ext).astype(F32)
    t = (lo + rng.random((n, 3)) * (hi - lo)).astype(F32)
    return api.make_rays(o, t - o, tmax=np.float32(3.0e38))


def _upload(scene, devices=(0,)):
    ctx = api.Context(devices)
    ctx.upload_scene(scene)
    return ctx


def _assert_same(ctx, ref, scene, extended=True, rays=None):
    rays = _rays(scene) if rays is None else rays
    cam = ref.camera_rays(W, H, scene.camera)
    for r in (rays, cam):
        np.testing.assert_array_equal(_bits(ctx.intersect(r)), _bits(ref.intersect(r)))
        np.testing.assert_array_equal(ctx.occluded(r), ref.occluded(r))
    for mode in (0, 1):
        ctx.render(W, H, scene.camera, mode=mode)
        ref.render(W, H, scene.camera, mode=mode)
        for a, b in zip(ctx.read_hits(), ref.read_hits()):
            np.testing.assert_array_equal(_bits(a), _bits(b))
        np.testing.assert_array_equal(ctx.read_rgba8_combined(), ref.read_rgba8_combined())
    if extended:  # shadows and bounces: stale light grids would show here
        ctx.render(W, H, scene.camera, mode=2, spp=2, max_bounces=2, frame_seed=3)
        ref.render(W, H, scene.camera, mode=2, spp=2, max_bounces=2, frame_seed=3)
        np.testing.assert_array_equal(_bits(ctx.read_rgb32f()), _bits(ref.read_rgb32f()))


def _clean(ctx):
    c = ctx.debug_check_bvh()
    assert c["failures"] == 0, c
    return c


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, seed=5, size=0.4, n_spheres=3, n_lights=2)


@pytest.fixture(scope="module")
def sponza():
    return scenes.sponza_like()


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["soup", "sponza"])
def test_unchanged_positions_reproduce_the_upload(name, soup, sponza):
    """A refit with the uploaded positions rewrites every record and node with the same bits: this also pins refit.hip's
    quantisation to k_db_emit's (the device build's node hash)."""
    scene = soup if name == "soup" else sponza
    with _upload(scene) as ctx, _upload(scene) as ref:
        before = _clean(ctx)
        assert before["method"] == 2
        st = ctx.update_geometry(_positions(scene))
        assert st["flags"] == api.STAT_REFIT and st["kernel_ms"] > 0 and st["tree_build"] == 2
        after = _clean(ctx)
        assert after["nodes_hash"] == before["nodes_hash"] and after["tris_hash"] == before["tris_hash"]
        assert after["nodes"] == before["nodes"] and after["placed_once"] == before["placed_once"]
        _assert_same(ctx, ref, scene, extended=name == "soup")


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["jitter", "rigid", "large"])
@pytest.mark.parametrize("name", ["cornell12", "soup", "sponza"])
def test_moved_geometry_matches_a_fresh_upload(name, kind, soup, sponza):
    scene = {"soup": soup, "sponza": sponza}.get(name) or scenes.cornell12()
    moved = _moved(scene, _motion(scene, kind))
    with _upload(scene) as ctx:
        ctx.render(W, H, scene.camera, mode=2, spp=1, max_bounces=1)  # the light grids of the old triangles exist now
        st = ctx.update_geometry(_positions(moved))
        assert st["flags"] == api.STAT_REFIT and st["grid_bytes"] == 0
        _clean(ctx)
        with _upload(moved) as ref:
            _assert_same(ctx, ref, moved)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_animation_of_twenty_steps(soup):
    base = _positions(soup).astype(np.float64)
    with _upload(soup) as ctx:
        for step in range(20):
            a = 0.05 * step
            p = base.copy()
            p[:, 0] += 0.3 * np.sin(a + base[:, 1])
            p[:, 2] += 0.2 * np.cos(2 * a + base[:, 0])
            moved = _moved(soup, p.astype(F32))
            assert ctx.update_geometry(_positions(moved))["flags"] == api.STAT_REFIT
            _clean(ctx)
            with _upload(moved) as ref:
                _assert_same(ctx, ref, moved, extended=step % 5 == 4)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_device_resident_input_equals_host_input(soup):
    if torch is None:
        pytest.skip("torch is not installed")
    moved = _moved(soup, _motion(soup, "rigid", seed=2))
    spheres = soup.spheres.copy()
    spheres["radius"] *= 1.5
    with _upload(soup) as a, _upload(soup) as b:
        a.update_geometry(_positions(moved), spheres=spheres)
        dev = torch.from_numpy(_positions(moved)).to("cuda:0")
        st = b.update_geometry(dev)
        assert st["flags"] == api.STAT_REFIT
        b.update_geometry(spheres=spheres)
        _assert_same(b, a, moved)
        # rt_prepare and the light grids read the positions back when they need them
        b.prepare(api.PREPARE_QUALITY_TREE)
        with _upload(_moved(moved, _positions(moved), spheres)) as ref:
            _assert_same(b, ref, moved)
        # a device buffer 4 bytes off 16-byte alignment is accepted (4-byte alignment is enough)
        buf = torch.zeros(dev.numel() + 1, device="cuda:0")
        buf[1:] = dev.reshape(-1)
        b.update_geometry(buf[1:].view(-1, 3))
        _assert_same(b, a, moved, extended=False)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_quality_tree_refit_prepare_and_rebuild(soup):
    moved = _moved(soup, _motion(soup, "large", seed=3))
    with _upload(moved) as ref:
        with _upload(soup) as ctx:  # a refit of the host builder's tree
            ctx.prepare(api.PREPARE_QUALITY_TREE)
            st = ctx.update_geometry(_positions(moved))
            assert st["flags"] == api.STAT_REFIT and st["tree_build"] == 0
            _clean(ctx)
            _assert_same(ctx, ref, moved)
        with _upload(soup) as ctx:  # rt_prepare after an update builds from the new positions
            ctx.update_geometry(_positions(moved))
            ctx.prepare(api.PREPARE_QUALITY_TREE)
            assert ctx.stats()["tree_build"] == 0
            c = _clean(ctx)
            with _upload(moved) as q:
                q.prepare(api.PREPARE_QUALITY_TREE)
                assert c["nodes_hash"] == q.debug_check_bvh()["nodes_hash"]
            _assert_same(ctx, ref, moved)
        with _upload(soup) as ctx:  # RT_UPDATE_REBUILD: the device build's tree of the new positions
            st = ctx.update_geometry(_positions(moved), rebuild=True)
            assert st["flags"] == api.STAT_REBUILT and st["tree_build"] == 2
            c = _clean(ctx)
            r = ref.debug_check_bvh()
            assert (c["nodes_hash"], c["tris_hash"]) == (r["nodes_hash"], r["tris_hash"])
            assert st["bvh_nodes"] == ref.stats()["bvh_nodes"] and st["scene_bytes"] == ref.stats()["scene_bytes"]
            _assert_same(ctx, ref, moved)
            # a refit after a rebuild uses the new tree's view
            assert ctx.update_geometry(_positions(soup))["flags"] == api.STAT_REFIT
            with _upload(soup) as back:
                _assert_same(ctx, back, soup, extended=False)


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_non_finite_vertices(soup):
    p = _positions(soup).copy()
    tr = soup.triangles
    p[tr["v0_index"][10]] = np.nan
    p[tr["v1_index"][20]] = np.inf
    for k in range(40, 44):  # whole leaves likely empty: consecutive triangles of the soup lie apart, but several go together
        p[tr["v2_index"][k]] = np.nan
    nan_scene = _moved(soup, p)
    with _upload(soup) as ctx, _upload(nan_scene) as ref:
        assert ctx.update_geometry(p)["flags"] == api.STAT_REFIT
        _clean(ctx)
        _assert_same(ctx, ref, nan_scene)
    # every vertex of a small scene non-finite: every leaf and the root are empty
    cb = scenes.cornell12()
    allnan = np.full_like(_positions(cb), np.nan)
    with _upload(cb) as ctx, _upload(_moved(cb, allnan)) as ref:
        assert ctx.update_geometry(allnan)["flags"] == api.STAT_REFIT
        _clean(ctx)
        _assert_same(ctx, ref, _moved(cb, allnan))
    # a triangle left out at upload that is finite now: only a new tree can place it
    with _upload(nan_scene) as ctx, _upload(soup) as ref:
        st = ctx.update_geometry(_positions(soup))
        assert st["flags"] == api.STAT_REBUILT
        assert _clean(ctx)["placed_once"] == len(soup.triangles)
        _assert_same(ctx, ref, soup)


# 7 ------------------------------------------------------------------------------------------------------------------------
def _packed(oracle_mod, scene, counts, tpb):
    """The scene's triangles in three buffers of `counts` triangles each (prim id = buffer * tpb + position: not the index)."""
    pk = oracle_mod.PackedScene(scene, use_bvh=False, triangles_per_buffer=max(len(scene.triangles), 1))
    tris = np.ascontiguousarray(scene.triangles)
    bufs, at = [], 0
    for c in counts:
        bufs.append(np.ascontiguousarray(tris[at:at + c]))
        at += c
    return pk.metadata, pk.offsets, bufs, tpb


def test_packed_upload_then_update(oracle_mod, soup):
    moved = _moved(soup, _motion(soup, "rigid", seed=4))
    counts, tpb = (700, 1400, 900), 1500
    with api.Context() as ctx, api.Context() as ref:
        md, off, bufs, _ = _packed(oracle_mod, soup, counts, tpb)
        ctx.upload_scene_packed(md, off, bufs, tpb, soup.materials)
        md2, off2, bufs2, _ = _packed(oracle_mod, moved, counts, tpb)
        ref.upload_scene_packed(md2, off2, bufs2, tpb, moved.materials)
        assert ctx.update_geometry(_positions(moved))["flags"] == api.STAT_REFIT
        # rt_debug_check_bvh counts prim ids against the number of triangles, so it reports every prim id of the third buffer
        # (>= 2 * tpb) as out of range for any packed upload with gaps: the refit must add nothing to what a fresh upload reports
        got, want = ctx.debug_check_bvh(), ref.debug_check_bvh()
        assert got["failures"] == want["failures"] == counts[2]
        _assert_same(ctx, ref, moved)
        prim = api.split_hits(ctx.intersect(_rays(moved)))[3]
        assert prim[prim != api.PRIM_MISS].max() >= 2 * tpb  # the prim ids of the third buffer came through


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_spheres_only_keeps_the_light_grids(soup):
    spheres = soup.spheres.copy()
    spheres["center"] += np.array([0.3, -0.2, 0.1], F32)
    spheres["radius"] *= 0.7
    spheres["material_id"] = (spheres["material_id"] + 1) % len(soup.materials)
    moved = _moved(soup, _positions(soup), spheres)
    with _upload(soup) as ctx, _upload(moved) as ref:
        ctx.prepare(api.PREPARE_SHADOW_GRIDS)
        g = ctx.stats()
        assert g["grid_bytes"] > 0
        st = ctx.update_geometry(spheres=spheres)
        assert st["flags"] == 0 and st["grid_build_ms"] == g["grid_build_ms"] and st["grid_bytes"] == g["grid_bytes"]
        _assert_same(ctx, ref, moved)
        assert ctx.stats()["grid_build_ms"] == g["grid_build_ms"]


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_scene_intact(soup, oracle_mod):
    lib = api.load()
    with api.Context() as ctx:
        v = _positions(soup)
        rc = lib.rt_update_geometry(ctx._h, C.c_void_p(v.ctypes.data), C.c_uint32(len(v)), None, C.c_uint32(0), C.c_uint32(0))
        assert rc == -4  # before any upload
        ctx.upload_scene(soup)
        with _upload(soup) as ref:
            moved = _positions(_moved(soup, _motion(soup, "large")))
            for nv, ns, flags in ((len(v) - 1, 0, 0), (len(v) + 1, 0, 0), (len(v), 0, 2), (len(v), 0, 0x80000000)):
                rc = lib.rt_update_geometry(ctx._h, C.c_void_p(moved.ctypes.data), C.c_uint32(nv), None, C.c_uint32(ns), C.c_uint32(flags))
                assert rc == -1, (nv, ns, flags)
            sp = np.zeros(len(soup.spheres) + 1, T.SPHERE)
            assert lib.rt_update_geometry(ctx._h, None, C.c_uint32(0), C.c_void_p(sp.ctypes.data), C.c_uint32(len(sp)), C.c_uint32(0)) == -1
            assert lib.rt_update_geometry(ctx._h, None, C.c_uint32(5), None, C.c_uint32(0), C.c_uint32(0)) == -1
            _assert_same(ctx, ref, soup, extended=False)
        # an rt_dispatch_tile still in flight renders the old positions: the update waits for it
        packed = oracle_mod.PackedScene(soup, use_bvh=False)
        pc = packed.push_constants(W, H, channel=0, tile_offset=(0, 0))
        with _upload(soup) as old:
            old.dispatch_tile(pc)
            want = old.read_rgba8_channels()[0]
        ctx.dispatch_tile(pc)
        ctx.update_geometry(moved)
        np.testing.assert_array_equal(ctx.read_rgba8_channels()[0], want)


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_context_with_several_devices(soup):
    if torch is None or torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    moved = _moved(soup, _motion(soup, "jitter", seed=9))
    with api.Context((0, 1)) as ctx, api.Context((0, 1)) as ref:
        ctx.upload_scene(soup)
        ref.upload_scene(moved)
        assert ctx.update_geometry(_positions(moved))["flags"] == api.STAT_REFIT
        _assert_same(ctx, ref, moved)
        dev = torch.from_numpy(_positions(_moved(soup, _motion(soup, "rigid", seed=9)))).to("cuda:1")
        ctx.update_geometry(dev)
        with api.Context((0, 1)) as ref2:
            ref2.upload_scene(_moved(soup, dev.cpu().numpy()))
            _assert_same(ctx, ref2, _moved(soup, dev.cpu().numpy()))


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_tree_stats_are_those_of_an_upload_of_that_tree(soup, monkeypatch):
    """rt_prepare(RT_PREPARE_QUALITY_TREE) reports the tree it put in place as an upload that builds the same tree reports it
    (scene_bytes included), and a fresh upload of the scene afterwards reports what the first upload did."""
    keys = ("scene_bytes", "bvh_nodes", "bvh_depth", "tree_build", "grid_bytes", "grid_build_ms")
    monkeypatch.setenv("RT_BUILD_METHOD", "0")  # the host builder's tree: the one rt_prepare builds
    with _upload(soup) as host:
        want = {k: host.stats()[k] for k in keys}
        want_hash = _clean(host)["nodes_hash"]
    monkeypatch.delenv("RT_BUILD_METHOD")
    with _upload(soup) as ctx:
        first = {k: ctx.stats()[k] for k in keys}
        assert first["tree_build"] == 2
        ctx.prepare(api.PREPARE_SHADOW_GRIDS)  # light grids, which go with the device-built tree
        assert ctx.stats()["grid_bytes"] > 0
        ctx.prepare(api.PREPARE_QUALITY_TREE)
        assert {k: ctx.stats()[k] for k in keys} == want and _clean(ctx)["nodes_hash"] == want_hash
        ctx.upload_scene(soup)
        assert {k: ctx.stats()[k] for k in keys} == first
