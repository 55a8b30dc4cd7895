"""What the float64 reference of shadow_grid_edge_cases.py says about its own cases: the conditions under which
test_gpu_shadow_grid_edges.py means something.  Nothing here touches the HIP library.

Per builder and resolution: every rung of 3e-4 and more is clear, both outcomes occur on every targeted feature, at most half of the
(point, light) pairs are not clear (a condition the geometry is chosen to meet - the ladder alone gives 5 rungs of 11 - not a
measurement), no segment comes near the filler ground, every point lies inside the widened box of direct_light_box and every occluder
inside the box the restated rules assume; the seam and border cases hit their features exactly, the stacks' points look up one cell
and no key comes near a limit, the near-list cases have the occluders on both sides of r_near that they claim."""
import numpy as np
import pytest

import shadow_grid_edge_cases as ec

CASES = [(name, level) for name in ec.BUILDERS for level in ("coarse", "production")]


@pytest.fixture(scope="module")
def made():
    cache = {}

    def get(name, level):
        if (name, level) not in cache:
            cache.clear()  # (one case at a time: a reference holds a margin per point, light and occluder)
            case = ec.BUILDERS[name](*ec.ASSUMED_RES[level])
            cache[(name, level)] = (case, ec.reference(case))
        return cache[(name, level)]
    return get


@pytest.mark.parametrize("name,level", CASES)
def test_conditions(made, name, level):
    case, ref = made(name, level)
    tags = case.tags
    n = len(case.points)
    assert 0 < n <= 1 << 18 and len(case.occluders) <= 600 - 2 * ec.GROUND_N["coarse"] ** 2
    # the boxes
    lo, hi = ec.widened_box()
    P = case.points[:, 0:3].astype(np.float64)
    assert ((P >= lo) & (P <= hi)).all(), "a point outside the widened box would walk the tree"
    V = case.occluders.reshape(-1, 3).astype(np.float64)
    assert ((V >= ec.BOX_LO) & (V <= ec.BOX_HI)).all(), "the pins and the ground span the triangle box"
    for k in range(3):
        assert V[:, k].min() == ec.BOX_LO[k] or k == 2 and ec.GROUND["z"] == ec.BOX_LO[2]
        assert V[:, k].max() == ec.BOX_HI[k]
    assert np.abs((case.points[:, 4:7].astype(np.float64) ** 2).sum(1) - 1.0).max() < 1e-6  # unit normals: eligible for the lists
    assert ec.ground_clearance(case) >= 1e-2
    # the rungs
    clear, lit, delta = ec.aimed(case, ref, "clear"), ec.aimed(case, ref, "lit"), tags["delta"]
    rung = ~np.isnan(delta)
    big = rung & (np.abs(delta) >= 3e-4)
    never = np.isin(tags["feature"], [f for f, nm in enumerate(tags["features"]) if nm in tags.get("never_clear", [])])
    assert clear[big].all(), sorted({tags["features"][f] for f in tags["feature"][big & ~clear]})
    assert clear[~rung & ~never].all(), "points that are not rungs are decided clearly"
    one_sided, dark = ec.one_sided_features(case, ref)
    assert len(dark) <= 0.15 * len(tags["features"]), dark
    for f, feature in enumerate(tags["features"]):
        mine = (tags["feature"] == f) & (big | ~rung)
        assert mine.any()
        if feature in one_sided:
            assert feature in tags.get("never_clear", []) or len(np.unique(lit[mine])) == 1, feature
        else:
            assert lit[mine].any() and (~lit[mine]).any(), f"{feature}: one outcome only"
    not_clear = 1.0 - ref["clear"].mean()
    print(f"{case.name}: {n} points x {len(case.lights)} lights, {len(case.occluders)} occluders, pairs not clear {not_clear:.4f}, "
          f"lit {ref['lit'].mean():.3f}, rungs under 3e-4 that came out clear {int((rung & ~big & clear).sum())}")
    assert not_clear <= ec.MAX_NOT_CLEAR


@pytest.mark.parametrize("level", ["coarse", "production"])
def test_seams_and_borders_hit_their_features(made, level):
    rc, ro = ec.ASSUMED_RES[level]
    case, ref = made("seams and borders", level)   # (the builder asserts the cube's features itself, exactly)
    assert {what.split()[0] for what, _ in case.tags["exact"]} == {"seam", "cell", "corner"}
    sun = case.lights[1]
    fr = ec.ortho_frame(sun, ro)
    b = case.tags["ortho_borders"]
    fu, _, _ = ec.ortho_cell(fr, np.array([[0.0, b["yb"], 0.0]]))
    _, fv, _ = ec.ortho_cell(fr, np.array([[b["xb"], 0.0, 0.0]]))
    ulp = 2.0 ** -23 * 32.0 * fr["scale"]  # an ulp of a coordinate below 32, in cells
    assert abs(fu[0] - b["ku"]) <= ulp and abs(fv[0] - b["kv"]) <= ulp
    # rung 0 of an orthographic border: the origin the device composes lies within two ulps of it; outer edges: on both sides
    o, _, _ = ec.segment32(sun, case.points)
    fu, fv, inside = ec.ortho_cell(fr, o)
    for f, feature in enumerate(case.tags["features"]):
        mine = (case.tags["feature"] == f) & (case.tags["delta"] == 0.0)
        if feature.startswith("ortho border in u"):
            assert np.abs(fu[mine] - b["ku"]).max() <= 2 * ulp
        if feature.startswith("ortho border in v"):
            assert np.abs(fv[mine] - b["kv"]).max() <= 2 * ulp
        if feature.startswith("ortho outer edge"):
            every = case.tags["feature"] == f
            assert inside[every].any() and (~inside[every]).any()
            assert ec.aimed(case, ref, "lit")[every].all(), "nothing projects there: visible"
    # the cube's rung 0: the direction the device composes looks up a cell next to the feature
    point = case.lights[0]
    _, d, _ = ec.segment32(point, case.points)
    face, ix, iy, fu, fv = ec.cube_cell(-d.astype(np.float64), rc)
    zero = (case.tags["light"] == 0) & (case.tags["delta"] == 0.0)
    near = np.minimum(np.abs(fu - np.round(fu)), np.abs(fv - np.round(fv)))
    assert near[zero].max() < 0.5 and len(np.unique(face[zero])) >= 5, "seams of five faces at least"


@pytest.mark.parametrize("kind", ["point", "spot", "directional"])
@pytest.mark.parametrize("level", ["coarse", "production"])
def test_stacks_look_up_one_cell_each(made, kind, level):
    rc, ro = ec.ASSUMED_RES[level]
    case, ref = made(f"stacks {kind}", level)
    light = case.lights[0]
    o, d, _ = ec.segment32(light, case.points)
    assert ec.aimed(case, ref, "segment").all()
    if kind == "directional":
        fr = ec.ortho_frame(light, ro)
        fu, fv, inside = ec.ortho_cell(fr, o)
        assert inside.all()
        cell = np.stack([np.zeros(len(o), np.int64), np.floor(fu).astype(np.int64), np.floor(fv).astype(np.int64)], 1)
        # the filler ground's footprint, dilated by the build's margin and two cells more, does not reach a stack's cell
        half = ec.GROUND["size"] / 2
        g = np.array([(x, y, ec.GROUND["z"]) for x in (-half, half) for y in (-half, half)])
        gu, gv, _ = ec.ortho_cell(fr, g)
        reach = fr["margin_cells"] + 2.0
        for _, cu, cv in case.tags["cells"]:
            assert cv + 1 < gv.min() - reach or cv > gv.max() + reach or cu + 1 < gu.min() - reach or cu > gu.max() + reach
        frac = np.stack([fu - np.floor(fu), fv - np.floor(fv)], 1)
    else:
        face, ix, iy, fu, fv = ec.cube_cell(-d.astype(np.float64), rc)
        cell = np.stack([face, ix, iy], 1)
        # the ground and the pins lie under the light's height or far from the faces' middles: nothing of them in a stack's cell
        others = np.concatenate([case.occluders[-len(ec.PINS):].reshape(-1, 3).astype(np.float64),
                                 [(x, y, ec.GROUND["z"]) for x in np.linspace(-30, 30, 61) for y in np.linspace(-30, 30, 61)]])
        of, ox, oy, _, _ = ec.cube_cell(others - ec.POINT_L, rc)
        for f_, x_, y_ in case.tags["cells"]:
            assert not ((of == f_) & (np.abs(ox - x_) <= 1) & (np.abs(oy - y_) <= 1)).any()  # (the dilation stays under a cell: 0.5 + 0.25 + the cone's 0.01)
        frac = np.stack([fu - np.floor(fu), fv - np.floor(fv)], 1)
    assert frac.min() > 0.1 and frac.max() < 0.9, "well inside the cell"
    cells = case.tags["cells"]  # a strip reaches its cell's neighbours (the dilation: up to a cell), not the next stack's cell
    assert all(a[0] != b[0] or abs(a[1] - b[1]) >= 3 for i, a in enumerate(cells) for b in cells[:i])
    for si, K in enumerate(ec.STACK_KS):
        mine = case.tags["stack"] == si
        assert (cell[mine] == np.array(case.tags["cells"][si])).all(), f"K = {K}"
        tri = case.tags["tri_stack"] == si
        assert tri.sum() == K
        # role 0: occluded by exactly its strip; role 1: lit
        hits = ref["margin"][mine][:, 0, :len(tri)][:, tri] >= 0
        role, strip = case.tags["role"][mine], case.tags["strip"][mine]
        straight = np.arange(mine.sum()) % ec.N_NORMALS == 0  # the normal that points at the light: the line passes through the light
        own = hits[np.arange(mine.sum()), np.where(role == 3, strip - 1, strip)]  # (role 3 carries m, its strip is m - 1)
        assert own[(role == 0) | (role == 3)].all(), "aimed at a strip's middle from behind it"
        assert (hits[(role == 0) & straight].sum(1) == 1).all() and not hits[(role == 1) & straight].any()
        assert not hits[role == 2][:, :].any() or kind != "directional"
        unclear = int((~ref["clear"][mine]).sum())
        segments, answered, reads, tight = ec.stack_expectation(case, ref, si)
        print(f"{case.name} K = {K}: {segments} segments, {answered} answered by the lists, {reads} entries read, tightest key {tight:.2e}, points not clear {unclear}")
        # (the device's keys, limits and distances are f32 results of a few operations on numbers below 64: within 1e-5 of these)
        assert K > ec.HEAVY or tight > 1e-4, "keys well apart from each other and from every limit: the walk's length is determined"
        assert segments == mine.sum()
        if K <= ec.WALK:
            assert answered == segments
        elif K <= ec.HEAVY:
            assert 0 < answered < segments
        else:
            assert answered == 0 and reads == 0


@pytest.mark.parametrize("level", ["coarse", "production"])
def test_near_threshold_occluders_lie_on_both_sides(made, level):
    rc, _ = ec.ASSUMED_RES[level]
    case, ref = made("near threshold", level)
    rn = ec.r_near(ec.POINT_L, rc)
    keys = ec.cube_key(ec.POINT_L, case.occluders[:12])
    np.testing.assert_allclose(keys[:6] / rn, 0.8, rtol=2e-3)
    np.testing.assert_allclose(keys[6:] / rn, 1.25, rtol=2e-3)
    for li, light in enumerate(case.lights):
        assert int(ec.in_near_list(light["position"], case.occluders, rc).sum()) == case.tags["expect_near"][li]
    assert ec.tri_dist(case.lights[1]["position"], case.occluders[12:13])[0] == 0.0
    # no triangle of this case is too small for the triangle test
    v0, e1, e2 = ec.device_triangles(case.occluders)
    assert (np.linalg.norm(np.cross(e1, e2), axis=1) > 3e-5).all()
    apart = ec.displaced_cells(case, rc)
    print(f"{case.name}: sideways normals look up a cell {np.mean(apart >= 1):.2f} one or more / {np.mean(apart >= 2):.2f} two or more cells from the target's")
    assert np.mean(apart >= 2) >= 0.25


def test_restated_rules():
    assert [ec.resolution("point", n) for n in (1, 64, 65, 65536, 65537, 10 ** 7)] == [16, 16, 32, 512, 1024, 1024]
    assert [ec.resolution("directional", n) for n in (1, 64, 65, 65536, 65537, 10 ** 7)] == [32, 32, 64, 1024, 2048, 2048]
    n_production = 2 * ec.GROUND_N["production"] ** 2
    assert n_production // 4 > 65536, "a leaf holds four triangles at most: the production ground alone makes more than 65 536 leaves"
    assert ec.walk([1.0, 2.0, 3.0], 2.5, [False, False, True]) == (True, 2)
    assert ec.walk(list(range(40)), 100.0, [False] * 40) == (False, 31) and ec.walk(list(range(31)), 100.0, [False] * 31) == (True, 31)
    assert ec.walk(list(range(40)), 100.0, [False] * 30 + [True] + [False] * 9) == (True, 31)
    assert ec.walk(list(range(129)), 100.0, [True] * 129) == (False, 0)
    n8 = ec.normals8(np.array([[0.3, -0.2, 0.9]]))
    l = ec._unit(np.array([0.3, -0.2, 0.9]))
    np.testing.assert_allclose(n8[0] @ l, [1.0] + [ec.TILT] * 7, atol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(n8[0], axis=1), 1.0, atol=1e-12)
