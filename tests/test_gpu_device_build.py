"""The acceleration structure built ON the GPU (gpu_raytracer_amd/csrc/device_build.hip: Morton sort, PLOC, the 8-slot collapse
program, emission) - the default for scenes of 1,024 triangles and more.

  * structure: the tree a context holds is downloaded and validated the way the kernels decode it (csrc/bvh_check.h, the checker
    the host builders run under ASan/UBSan): slots and masks, every finite triangle in exactly one leaf, conservative boxes, depth;
  * the host's PLOC build (bvh_builder.cpp, RT_BUILD_METHOD=1) calls the same rules (csrc/bvh_rules.h: Morton codes, neighbour rule,
    collapse program, slots, quantisation) and appends in the depth-first layout the device computes - so the node and triangle
    arrays are BYTE-IDENTICAL (compared by hash);
  * images: hits and colours are identical to those from a host-built (binned SAH) tree - closest hits do not depend on topology;
  * degenerate input (coincident triangles, a chain of growing triangles, non-finite vertices) stays logarithmic and shallow.
"""
import time

import numpy as np
import pytest

from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

pytestmark = pytest.mark.gpu


def _upload(rt_api, monkeypatch, scene, method):
    monkeypatch.setenv("RT_BUILD_METHOD", str(method))
    ctx = rt_api.Context()
    t0 = time.perf_counter()
    ctx.upload_scene(scene)
    return ctx, (time.perf_counter() - t0) * 1e3


def _finite_triangles(scene):
    v = scene.vertices["position"]
    t = scene.triangles
    ok = np.isfinite(v[t["v0_index"]]).all(-1) & np.isfinite(v[t["v1_index"]]).all(-1) & np.isfinite(v[t["v2_index"]]).all(-1)
    return int(ok.sum())


@pytest.mark.parametrize("name", ["sponza_like", "soup60k"])
def test_device_build_structure_and_host_statement(rt_api, monkeypatch, name):
    scene = scenes.sponza_like() if name == "sponza_like" else scenes.random_soup(60000, seed=5, size=0.12, n_lights=3)
    dev, ms_dev = _upload(rt_api, monkeypatch, scene, 2)
    host, ms_host = _upload(rt_api, monkeypatch, scene, 1)
    try:
        a, b = dev.debug_check_bvh(), host.debug_check_bvh()
        assert a["method"] == 2 and b["method"] == 1
        assert a["failures"] == 0 and b["failures"] == 0
        assert a["placed_once"] == b["placed_once"] == _finite_triangles(scene)
        assert (a["nodes"], a["leaves"], a["depth"]) == (b["nodes"], b["leaves"], b["depth"])
        assert (a["nodes_hash"], a["tris_hash"]) == (b["nodes_hash"], b["tris_hash"])
        assert a["real_depth"] <= a["depth"] <= 32
        # same hits and colours as with the host's binned-SAH tree
        w, h = 320, 180
        sah, _ = _upload(rt_api, monkeypatch, scene, 0)
        try:
            out = []
            for ctx in (dev, sah):
                ctx.render(w, h, scene.camera, mode=1)
                prim, t = ctx.read_hits()
                out.append((prim, t, ctx.read_rgb32f()))
                ctx.render(w // 2, h // 2, scene.camera, mode=2, spp=3, max_bounces=3)
                out[-1] += (ctx.read_rgb32f(),)
            for x, y in zip(out[0], out[1]):
                np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
        finally:
            sah.close()
        print(f"{name}: upload with device build {ms_dev:.1f} ms, host PLOC {ms_host:.1f} ms")
    finally:
        dev.close()
        host.close()


def _degenerate(kind, n):
    rng = np.random.default_rng(len(kind) * 7 + 1)
    tri = np.zeros((n, 3, 3), np.float32)
    if kind == "coincident":
        tri[:] = np.float32(1.25)
    elif kind == "chain":  # every triangle's nearest neighbour along the curve is its predecessor
        c = (np.float32(1.0005) ** np.arange(n, dtype=np.float32))[:, None, None]
        tri[:] = c * np.array([1, 0, 0], np.float32) + rng.uniform(-1e-3, 1e-3, (n, 3, 3)).astype(np.float32)
    elif kind == "nonfinite":
        tri[:] = rng.uniform(-3, 3, (n, 1, 3)).astype(np.float32) + rng.uniform(-0.2, 0.2, (n, 3, 3)).astype(np.float32)
        tri[::7, 1, 0] = np.nan
        tri[3::14, 2, 2] = np.inf
    vertices = np.zeros(n * 3, dtype=T.VERTEX)
    vertices["position"] = tri.reshape(-1, 3)
    triangles = np.zeros(n, dtype=T.TRIANGLE)
    idx = np.arange(n * 3, dtype=np.uint32).reshape(-1, 3)
    triangles["v0_index"], triangles["v1_index"], triangles["v2_index"] = idx[:, 0], idx[:, 1], idx[:, 2]
    base = scenes.random_soup(8, seed=3)
    return scenes.Scene(kind, base.spheres[:0], base.lights, vertices, triangles, base.materials, base.camera)


@pytest.mark.parametrize("kind", ["coincident", "chain", "nonfinite"])
def test_device_build_on_degenerate_input(rt_api, monkeypatch, kind):
    scene = _degenerate(kind, 20000)
    dev, ms = _upload(rt_api, monkeypatch, scene, 2)
    host, _ = _upload(rt_api, monkeypatch, scene, 1)
    try:
        a, b = dev.debug_check_bvh(), host.debug_check_bvh()
        assert a["failures"] == 0 and a["placed_once"] == _finite_triangles(scene)
        if a["method"] == 2:  # (a tree deeper than the kernels' stacks would have fallen back to the host build: method 0)
            assert (a["nodes"], a["leaves"], a["depth"]) == (b["nodes"], b["leaves"], b["depth"])
            assert (a["nodes_hash"], a["tris_hash"]) == (b["nodes_hash"], b["tris_hash"])
        assert a["depth"] <= 32 and ms < 5000
        st = dev.render(96, 64, scene.camera, mode=1)
        prim, t = dev.read_hits()
        host.render(96, 64, scene.camera, mode=1)
        prim2, t2 = host.read_hits()
        np.testing.assert_array_equal(prim, prim2)
        np.testing.assert_array_equal(t.view(np.uint32), t2.view(np.uint32))
        assert st["rays"] == 96 * 64
    finally:
        dev.close()
        host.close()


# Small trees: a wide node has fewer than eight children, a whole subtree becomes one leaf, the root's program is nearly a leaf.
# An explicit RT_BUILD_METHOD=2 still leaves scenes under 1,024 triangles to the host builder (tree_method, rt_scene.cpp), so of
# the sizes 9 / 37 / 300 / 1000 and the 1,000 coincident triangles none reaches the device build: they stay as the declined cases,
# and the smallest sizes the device build accepts (1,024, one more, an odd one) and 1,024 coincident triangles are added to them.
SMALL = [("soup", 9), ("soup", 37), ("soup", 300), ("soup", 1000), ("coincident", 1000),
         ("soup", 1024), ("soup", 1025), ("soup", 1531), ("coincident", 1024)]


def _small_scene(kind, n):
    return scenes.random_soup(n, seed=11) if kind == "soup" else _degenerate(kind, n)


@pytest.fixture(scope="module")
def small_builds(rt_api):
    """Every small case built once with RT_BUILD_METHOD=2 and once with =1: (device's check, host's check) per case."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for kind, n in SMALL:
            scene = _small_scene(kind, n)
            dev, _ = _upload(rt_api, mp, scene, 2)
            host, _ = _upload(rt_api, mp, scene, 1)
            try:
                out[(kind, n)] = (dev.debug_check_bvh(), host.debug_check_bvh())
            finally:
                dev.close()
                host.close()
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("kind,n", SMALL, ids=[f"{k}{n}" for k, n in SMALL])
def test_small_device_builds_match_the_host(small_builds, kind, n):
    a, b = small_builds[(kind, n)]
    assert b["method"] == 1
    assert a["failures"] == 0 and b["failures"] == 0
    assert a["placed_once"] == b["placed_once"] == _finite_triangles(_small_scene(kind, n))
    if a["method"] == 2:  # (declined: a host tree, checked above; a one-leaf root is the host's business)
        assert (a["nodes"], a["leaves"], a["depth"]) == (b["nodes"], b["leaves"], b["depth"])
        assert (a["nodes_hash"], a["tris_hash"]) == (b["nodes_hash"], b["tris_hash"])


def test_small_device_builds_reach_the_device(small_builds):
    """Enough of the small cases must have been built on the device for them to say anything about it."""
    methods = {c: small_builds[c][0]["method"] for c in SMALL}
    assert sum(m == 2 for m in methods.values()) >= 3, methods
    assert all(methods[("soup", n)] == 2 for n in (1024, 1025, 1531)), methods


def test_small_scenes_use_the_host_build(rt_api, monkeypatch):
    monkeypatch.delenv("RT_BUILD_METHOD", raising=False)
    with rt_api.Context() as ctx:
        ctx.upload_scene(scenes.cornell12())
        assert ctx.debug_check_bvh()["method"] == 0
        ctx.upload_scene(scenes.random_soup(5000, seed=4, size=0.3))
        c = ctx.debug_check_bvh()
        assert c["method"] == 2 and c["failures"] == 0 and c["placed_once"] == 5000


def test_headline_frame_is_the_same_with_every_builder(rt_api, monkeypatch):
    """The whole sponza-like 1920x1080 64-spp frame from a host binned-SAH tree, a host PLOC tree and a device-built tree: one CRC,
    and at the pixel where the reference's BVH walk and its brute-force path disagree (tests/test_oracle_extended.py) the
    brute-force value - the box filter is conservative, results do not depend on the tree."""
    scene = scenes.sponza_like()
    frames = {}
    for method in (0, 1, 2):
        ctx, _ = _upload(rt_api, monkeypatch, scene, method)
        try:
            ctx.render(1920, 1080, scene.camera, mode=2, spp=64, max_bounces=4, tile_size=32)
            frames[method] = ctx.read_rgb32f()
        finally:
            ctx.close()
    for method in (1, 2):
        np.testing.assert_array_equal(frames[method].view(np.uint32), frames[0].view(np.uint32))
    assert frames[2][563, 844].view(np.uint32).tolist() == [1066366301, 1057316370, 1044521191]
