"""The light grids' one property - every cell's list holds every triangle that a segment looking up that cell can be stopped by, under a
key that does not exceed the triangle's distance (csrc/shadow_grid.hip) - tested where it can break: rt_direct_light at the points of
shadow_grid_edge_cases.py, whose segments are aimed within an ulp of silhouettes, cube seams and corners, cell borders, the near-list
threshold, a key's own limit and every boundary of the list bookkeeping, on coarse grids (16 - 64 cells per side) and on the
resolutions the benchmark runs on (1024 / 2048: a ground of 300 000 triangles sets them).

Per case: the lists' answer equals the tree's on whole byte strings (no tolerance, no exclusion); the tree's answer equals the float64
brute force of the case module wherever that is clear; the counters say that the lists ran and, for the stacks, exactly how far every
walk went; and a small frame that looks at the occluders carries equal bits with and without the lists (k_wf_shadow_grid's parked
walks see the same lists).  test_shadow_grid_edge_cases.py checks the cases themselves on the CPU."""
import numpy as np
import pytest

import shadow_grid_edge_cases as ec
from gpu_raytracer_amd import api
from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import types as T
from test_gpu_adversarial import _grid, _scene
from test_gpu_shadow_grid_occluders import BOUNCES, HGT, SPP, W, _assert_same_bits, _env, _frames

pytestmark = pytest.mark.gpu

U32 = np.uint32
CASES = [(name, level) for name in ec.BUILDERS for level in ("coarse", "production")]


def _light(light):
    if light["kind"] == "point":
        return H.light_point(tuple(light["position"]), (1.0, 1.0, 1.0), 30.0)
    if light["kind"] == "spot":
        return H.light_spot(tuple(light["position"]), tuple(light["direction"]), (1.0, 1.0, 1.0), 30.0, np.inf, 0.3, 0.6)
    return H.light_directional(tuple(light["direction"]), (1.0, 1.0, 1.0), 0.8)


_GROUND = {}


def _to_scene(case, level):
    if level not in _GROUND:  # (the one ground all builders of a resolution share)
        n = ec.GROUND_N[level]
        _GROUND[level] = _grid(n, n, z=ec.GROUND["z"], size=ec.GROUND["size"])[0]
    ground = _GROUND[level]
    tris = np.concatenate([case.occluders, ground])
    cam = H.camera(position=case.camera[0], direction=case.camera[1], up=(0.0, 0.0, 1.0) if abs(case.camera[1][2]) < 0.9 else (0.0, 1.0, 0.0), fov=50.0)
    return _scene(f"{case.name} ({level})", tris, [0] * len(tris), lights=np.array([_light(l) for l in case.lights], dtype=T.LIGHT), camera=cam)


def _expected_res(ctx, scene, level):
    """The restated resolution rule: from the tree's leaves (coarse), or from the bounds n / 4 <= leaves <= n where both give the same."""
    n = len(scene.triangles)
    if level == "production":
        lo, hi = -(-n // 4), n
        assert ec.resolution("point", lo) == ec.resolution("point", hi) == 1024 and ec.resolution("directional", lo) == ec.resolution("directional", hi) == 2048
        return 1024, 2048
    check = ctx.debug_check_bvh()
    assert check["failures"] == 0
    return ec.resolution("point", check["leaves"]), ec.resolution("directional", check["leaves"])


@pytest.fixture(scope="module", params=CASES, ids=[f"{name}-{level}" for name, level in CASES])
def prepared(request, rt_api):
    """One upload, one query on the tree, one prepare per (builder, resolution).  A case's geometry is laid out in the grid's cells, so
    it is built for the resolution the restated rule gives for the uploaded tree (at most one rebuild: the assumed coarse resolution)."""
    name, level = request.param
    res = ec.ASSUMED_RES[level]
    ctx = rt_api.Context()
    try:
        for attempt in range(2):
            case = ec.BUILDERS[name](*res)
            scene = _to_scene(case, level)
            assert level == "production" or len(scene.triangles) <= 600
            ctx.upload_scene(scene)
            want = _expected_res(ctx, scene, level)
            if want == res:
                break
            res = want
        assert want == res, "the case's own triangles changed the resolution it was built for"
        points = case.points
        assert len(points) <= 1 << 18
        tree = ctx.direct_light(points, counters=True)                      # 1. before prepare(): the tree
        tree_stats, tree_use = ctx.stats(), ctx.debug_shadow_grid()
        with _env(RT_SHADOW_GRID_MEAN="1e9"):
            ctx.prepare()
        yield dict(name=name, level=level, res=res, case=case, scene=scene, ctx=ctx, tree=tree, tree_stats=tree_stats, tree_use=tree_use)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def reference_of():
    cache = {}

    def get(p):
        key = (p["name"], p["level"])
        if key not in cache:
            cache.clear()
            cache[key] = ec.reference(p["case"])
        return cache[key]
    return get


def _mask_bits(got, n_lights):
    _, mask = api.split_lighting(got)
    return ((mask[:, None] >> np.arange(n_lights, dtype=U32)[None, :]) & U32(1)).astype(bool)


def test_lists_equal_the_tree_bit_for_bit(prepared):
    p, ctx, case = prepared, prepared["ctx"], prepared["case"]
    assert p["tree_use"]["segments_answered"] == 0 and p["tree_use"]["lights_with_grid"] == 0 and p["tree_stats"]["grid_bytes"] == 0
    # 2. after prepare(): every light has a grid of the restated resolution
    assert ctx.debug_shadow_grid()["lights_with_grid"] == len(case.lights) and ctx.stats()["grid_bytes"] > 0
    for i, light in enumerate(case.lights):
        g = ctx.debug_shadow_grid(i)
        print(p["name"], p["level"], light["kind"], g)
        assert g["kind"] == (2 if light["kind"] == "directional" else 1)
        assert g["res"] == (p["res"][1] if light["kind"] == "directional" else p["res"][0])
        if p["level"] == "production":
            assert g["res"] == (2048 if light["kind"] == "directional" else 1024)
    with_lists = ctx.direct_light(case.points, counters=True)
    st, use = ctx.stats(), ctx.debug_shadow_grid()
    without = ctx.direct_light(case.points, use_grids=False)
    plain = ctx.direct_light(case.points)  # the kernel that does not count
    print(f"{p['name']} {p['level']}: {len(case.points)} points, {st['rays']} segments, {use['segments_answered']} answered by the lists, {use['entries_read']} entries read")
    assert with_lists.tobytes() == p["tree"].tobytes(), "the lists' answer differs from the tree's"
    assert without.tobytes() == p["tree"].tobytes() and plain.tobytes() == p["tree"].tobytes()
    assert st["rays"] == p["tree_stats"]["rays"] > 0
    assert 0 < use["segments_answered"] <= st["rays"]                       # 4. the lists ran


def test_tree_equals_the_float64_reference_where_clear(prepared, reference_of):
    p, case = prepared, prepared["case"]
    ref = reference_of(p)
    got = _mask_bits(p["tree"], len(case.lights))
    clear = ref["clear"]
    not_clear = 1.0 - clear.mean()
    print(f"{p['name']} {p['level']}: pairs not clear {not_clear:.4f} (cap {ec.MAX_NOT_CLEAR}), lit {ref['lit'][clear].mean():.3f} of the clear ones")
    assert not_clear <= ec.MAX_NOT_CLEAR
    wrong = np.argwhere(clear & (got != ref["lit"]))
    assert len(wrong) == 0, [(int(i), int(li), case.tags["features"][case.tags["feature"][i]], float(case.tags["delta"][i]), bool(got[i, li])) for i, li in wrong[:8]]
    # the segment count: every clear pair with positive facing terms has one, every pair that is not clear may have one
    sure, maybe = int((ref["segment"] & clear).sum()), int((~clear).sum())
    assert sure <= p["tree_stats"]["rays"] <= sure + maybe


def test_counters_say_what_the_restatement_says(prepared, reference_of):
    """Every builder: a light's near list holds the occluders the restated rule puts below r_near (0.8 and 1.25 r_near leave room for
    the key's 1e-4 shrink; the ground lies 26 under the lights).  The stacks: per K, how many segments the lists answer and how many
    entries they read - strips behind one another with nothing else in the cell's list, so the walk's length is determined."""
    p, ctx, case = prepared, prepared["ctx"], prepared["case"]
    for i, light in enumerate(case.lights):
        if light["kind"] != "directional":
            assert ctx.debug_shadow_grid(i)["near"] == int(ec.in_near_list(light["position"], case.occluders, p["res"][0]).sum()), (p["name"], i)
    if p["name"] == "near threshold":
        assert [ctx.debug_shadow_grid(i)["near"] for i in range(2)] == case.tags["expect_near"] == [6, 1]
    if not p["name"].startswith("stacks"):
        return
    ref = reference_of(p)
    g = ctx.debug_shadow_grid(0)
    assert g["heavy_cells"] >= 1 and g["longest"] >= max(ec.STACK_KS)
    for si, K in enumerate(ec.STACK_KS):
        rows = np.flatnonzero(case.tags["stack"] == si)
        segments, answered, reads, _ = ec.stack_expectation(case, ref, si)
        got = ctx.direct_light(np.ascontiguousarray(case.points[rows]), counters=True)
        st, use = ctx.stats(), ctx.debug_shadow_grid()
        print(f"{p['name']} {p['level']} K = {K}: {st['rays']} segments, answered {use['segments_answered']} (restated {answered}), entries read {use['entries_read']} (restated {reads})")
        assert got.tobytes() == p["tree"][rows].tobytes()
        assert st["rays"] == segments
        if K <= ec.WALK:
            assert use["segments_answered"] == st["rays"]                   # every segment of the stack's cell is answered by the lists
        if K > ec.HEAVY:
            assert use["segments_answered"] == 0 and use["entries_read"] == 0  # a cell over `heavy`: nothing is looked at
        assert st["rays"] - use["segments_answered"] == segments - answered  # exactly the segments that need entry 31 or later are handed on
        assert use["entries_read"] == reads


def test_the_frames_kernel_sees_the_same_lists(prepared):
    """k_wf_shadow_grid runs the parked walks in LDS, k_dl_direct does not: one 64 x 64 frame, 4 spp, 2 bounces, looking at the
    occluders from the points' side, with the lists and with no_shadow_grid: equal bits and equal segment totals."""
    p, ctx = prepared, prepared["ctx"]
    ref, got, counted, st, use = _frames(ctx, p["scene"])
    _assert_same_bits(p["scene"], ref, got, counted)
    assert (W, HGT, SPP, BOUNCES) == (64, 64, 4, 2)
    assert use["segments_answered"] <= st["shadow_rays"]
    print(p["name"], p["level"], "frame: shadow segments", st["shadow_rays"], "lists", use)
