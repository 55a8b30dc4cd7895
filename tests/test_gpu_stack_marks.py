"""Every traversal stack driven to its high-water mark on the deck (tests/stack_cases.py; run with -m gpu), against brute force.

k_wf_trace keeps RT_WF8_LDS_STACK entries per lane in LDS and everything deeper in an HBM overflow area sized from the tree's depth; the
pop with the clamped LDS read and the HBM override, the two overflow pushes, the (sp - 8) * 64 indexing, the per-wave base, the second
lane's own area and the reuse test of a live context exist only for a stack top in HBM.  The deck reaches it with 8194 triangles: the
counting kernel's mark (WF_TOTAL_STACK_MAX, read below) exceeds the LDS part with every builder, and the frames, bit for bit and
segment for segment, are the oracle's brute force (PackedScene(use_bvh=False)).  The per-lane walks of the other kernels (traverse /
occluded, traverse_all, cp_walk, cp_walk_all, the sweep and the parity walks) get depth + 2 LDS entries with a hit list or K-nearest list
right behind the stack; every batch call runs on the deck and is compared as its own GPU test compares it, with that test's statement.

Marks measured on the MI355X (8192 cards, LDS part 8; printed by test_the_mark / test_refit, tabulated in DESIGN.md "Traversal
stacks"): RT_BUILD_METHOD=0 depth 7, mark 10; =1 depth 8, mark 12; =2 (device build) depth 8, mark 12; quality tree depth 7, mark 10;
the device-built tree refitted to the sheared deck 12 before and 12 after; a 600-triangle soup frame 5."""
import dataclasses

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
import signed_distance_cases as sd
import stack_cases as sc
import sweep_cases as sw
from gpu_raytracer_amd import api, scenes
from test_gpu_adversarial import _check as check_reference_modes
from test_gpu_closest_point_all import _same as same_lists, _same_counts
from test_gpu_direct_light import _check_definition, _geometric_facing
from test_gpu_multi_hit import all_candidates, expected as expected_lists
from test_gpu_ray_queries import _bits, brute_force
from test_gpu_signed_distance import _same_bytes
from test_gpu_surface_ao import _check_ao, _surface
from test_stack_cases import lds_stack_entries

pytestmark = pytest.mark.gpu

F32 = np.float32
MISS = 0xFFFFFFFF
W, H = sc.FRAME
SPP, BOUNCES, SEED = 4, 3, 11
BUILDERS = ("0", "1", "2", "quality")  # RT_BUILD_METHOD 0 binned SAH, 1 host PLOC, 2 device build; the default tree after rt_prepare(PREPARE_QUALITY_TREE)
TREES = ("device", "0")                # the batch calls: once on the device-built tree, once on method 0
LDS = lds_stack_entries()


@pytest.fixture(scope="module")
def deck():
    scene = sc.deck_scene()
    rays = {k: sc.ray_set(k) for k in ("through", "corner", "mixed")}
    for r in rays.values():
        r.setflags(write=False)
    return scene, rays


@pytest.fixture(scope="module")
def truth(oracle_mod, deck):
    """The brute-force frame of the deck, computed once: rgb bits and segment counts."""
    scene, _ = deck
    ext = oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), W, H, SPP, BOUNCES, camera=scene.camera, frame_seed=SEED)
    ext["rgb"].setflags(write=False)
    seg = ext["segments"]
    assert seg["continuation"] > W * H and seg["shadow"] > W * H, "bounced and shadow segments: the ones that reach the overflow"
    return ext


def _upload(ctx, monkeypatch, scene, builder):
    """Uploads `scene` with the tree of `builder` and checks it is that tree -> rt_debug_check_bvh's record."""
    if builder in ("quality", "device"):
        monkeypatch.delenv("RT_BUILD_METHOD", raising=False)
    else:
        monkeypatch.setenv("RT_BUILD_METHOD", builder)
    ctx.upload_scene(scene)
    if builder == "quality":
        ctx.prepare(api.PREPARE_QUALITY_TREE)
    b = ctx.debug_check_bvh()
    assert b["failures"] == 0 and b["placed_once"] == scene.n_triangles and b["real_depth"] <= b["depth"], b
    assert b["method"] == {"0": 0, "1": 1, "2": 2, "quality": 0, "device": 2}[builder], b
    return b


def _frame(ctx, scene, **kw):
    st = ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=SPP, max_bounces=BOUNCES, frame_seed=SEED, **kw)
    return ctx.read_rgb32f(), st


def _assert_frame(rgb, st, ext, label):
    seg = ext["segments"]
    assert (st["primary_rays"], st["continuation_rays"], st["shadow_rays"]) == (seg["camera"], seg["continuation"], seg["shadow"]), label
    np.testing.assert_array_equal(_bits(rgb), _bits(ext["rgb"]), err_msg=label)


def _assert_mark(m, depth, label):
    """The counted pipeline frame's mark: above the LDS part - the case does its job; that is no tolerance - and within what the host
    sizes the overflow area for (ensure_wavefront: stack_entries = 2 * depth + 2)."""
    assert LDS < m <= 2 * depth + 2, f"{label}: mark {m}, LDS part {LDS}, depth {depth}"


# 1 ------------------------------------------------------------------------------------------------------------------------
VARIANTS = [("pipeline", {}, dict(kernel_pipeline=True)),
            ("pipeline counted", {}, dict(kernel_pipeline=True, counters=True)),
            ("no_shadow_grid", {}, dict(kernel_pipeline=True, no_shadow_grid=True)),
            ("no_shadow_grid counted", {}, dict(kernel_pipeline=True, no_shadow_grid=True, counters=True)),
            ("no_beams", {}, dict(kernel_pipeline=True, no_beams=True)),
            # A context keeps the batch size of its last pipeline frame while the frame's shape, samples and use of the lanes stay the
            # same (setup_pipeline, rt_frame.cpp), and reads RT_WF_BATCH only when one of them changes.  So every variant from here on
            # switches the lanes against the one before it: its RT_WF_BATCH is the batch it runs with.
            ("two lanes", {"RT_WF_LANES": "2", "RT_WF_BATCH": "2"}, dict(kernel_pipeline=True)),
            ("two lanes counted", {"RT_WF_LANES": "2", "RT_WF_BATCH": "2"}, dict(kernel_pipeline=True, counters=True)),  # (same lanes: keeps the batch of 2)
            ("one lane, two batches", {"RT_WF_LANES": "1", "RT_WF_BATCH": "2"}, dict(kernel_pipeline=True)),
            ("two lanes, batch 1", {"RT_WF_LANES": "2", "RT_WF_BATCH": "1"}, dict(kernel_pipeline=True)),
            ("one lane, batch 1", {"RT_WF_LANES": "1", "RT_WF_BATCH": "1"}, dict(kernel_pipeline=True)),
            ("kernel_sm", {}, dict(kernel_sm=True)),
            ("kernel_v1", {}, dict(kernel_v1=True))]


@pytest.mark.parametrize("builder", BUILDERS)
def test_frames_equal_brute_force_with_every_builder(gpu_ctx, monkeypatch, deck, truth, builder):
    """The pipeline in both instantiations (counting and not), with the light grids asked for and not (the build refuses the deck's
    long lists, so the shadow segments walk the tree either way: k_wf_trace<any hit>, far child first; forced grids are in
    test_direct_light_and_radiance), with and without camera beams, in two batches and in batches of one sample on two lanes (the second
    lane's own overflow area) and on one, and the two megakernels (depth + 2 entries in LDS): the oracle's bits and segment counts."""
    scene, _ = deck
    for var in ("RT_WF_LANES", "RT_WF_BATCH"):
        monkeypatch.delenv(var, raising=False)
    b = _upload(gpu_ctx, monkeypatch, scene, builder)
    for label, env, kw in VARIANTS:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            rgb, st = _frame(gpu_ctx, scene, **kw)
        assert st["flags"] & api.STAT_MEGAKERNEL_FALLBACK == 0
        _assert_frame(rgb, st, truth, f"builder {builder}, {label}")
        if kw.get("counters") and kw.get("kernel_pipeline"):
            m = gpu_ctx.debug_stack_mark()  # WF_TOTAL_STACK_MAX of this frame
            print(f"builder {builder} ({label}): mark {m}, depth {b['depth']}, LDS part {LDS}")
            assert m <= 2 * b["depth"] + 2


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
def test_the_mark(gpu_ctx, monkeypatch, deck, builder):
    """m = debug_counters()["transition_passes"] after a counted pipeline frame is the pipeline's WF_TOTAL_STACK_MAX (rt_frame.cpp folds
    the totals into the diagnostics slots; api.Context.debug_stack_mark names it): RT_WF8_LDS_STACK < m <= 2 * depth + 2 with every
    builder.  m >= RT_WF8_LDS_STACK + 2 means overflow index 1, not only index 0, was written and read back."""
    scene, _ = deck
    for var in ("RT_WF_LANES", "RT_WF_BATCH"):
        monkeypatch.delenv(var, raising=False)
    b = _upload(gpu_ctx, monkeypatch, scene, builder)
    st = gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=SPP, max_bounces=BOUNCES, frame_seed=SEED, kernel_pipeline=True, counters=True)
    m = gpu_ctx.debug_counters()["transition_passes"]
    assert m == gpu_ctx.debug_stack_mark()
    print(f"deck: builder {builder}, n {scene.meta['cards']} cards, depth {st['bvh_depth']} (real {b['real_depth']}), mark {m}, "
          f"LDS part {LDS}, overflow index {'>= 1' if m >= LDS + 2 else '0 only'} used")
    assert st["bvh_depth"] == b["depth"]
    _assert_mark(m, st["bvh_depth"], f"builder {builder}")


def test_the_mark_of_a_soup_is_recorded(gpu_ctx):
    """Recorded, not asserted: a 600-triangle soup of the kind the pipeline tests use stays inside the LDS part."""
    scene = scenes.random_soup(600, seed=5, size=0.6, n_spheres=3, n_lights=3)
    gpu_ctx.upload_scene(scene)
    st = gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=SPP, max_bounces=BOUNCES, frame_seed=SEED, kernel_pipeline=True, counters=True)
    print(f"soup600: depth {st['bvh_depth']}, mark {gpu_ctx.debug_stack_mark()}, LDS part {LDS}")


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_one_context_shallow_then_deep_then_shallow(rt_api, monkeypatch, deck, truth, lanes):
    """cornell12 (depth 1: one overflow entry per lane), then the deck, then cornell12 again, in one context at the same frame size,
    samples, batch and lanes - and with the deck's two lights on the Cornell box, so that only `ovf_entries >= needed` of
    ensure_wavefront's reuse test differs between the calls.  Every frame holds the bits of a fresh context's."""
    scene, _ = deck
    shallow = dataclasses.replace(scenes.cornell12(), lights=scene.lights, camera=scenes.cornell12().camera)
    monkeypatch.delenv("RT_BUILD_METHOD", raising=False)
    monkeypatch.setenv("RT_WF_LANES", lanes)
    monkeypatch.setenv("RT_WF_BATCH", "2")
    fresh = {}
    for s in (shallow, scene):
        with rt_api.Context() as ctx:
            ctx.upload_scene(s)
            fresh[s.name] = _frame(ctx, s, kernel_pipeline=True)
    _assert_frame(*fresh[scene.name], truth, f"fresh context, {lanes} lane(s)")
    with rt_api.Context() as ctx:
        for step, s in enumerate((shallow, scene, shallow, scene)):
            ctx.upload_scene(s)
            rgb, st = _frame(ctx, s, kernel_pipeline=True)
            want, want_st = fresh[s.name]
            np.testing.assert_array_equal(_bits(rgb), _bits(want), err_msg=f"step {step}: {s.name}, {lanes} lane(s)")
            assert st["rays"] == want_st["rays"]
        # (the counting instantiation through the same reallocated lanes)
        rgb, st = _frame(ctx, scene, kernel_pipeline=True, counters=True)
        _assert_frame(rgb, st, truth, f"reused context, {lanes} lane(s)")
        _assert_mark(ctx.debug_stack_mark(), st["bvh_depth"], f"reused context, {lanes} lane(s)")


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_refit(rt_api, oracle_mod, monkeypatch, deck):
    """update_geometry with the sheared positions: the topology of the unsheared deck, boxes that overlap far more.  Frames and
    intersect / occluded equal a fresh upload of the sheared scene and brute force; the refitted tree validates; the counted mark stays
    within 2 * depth + 2 of the unchanged topology."""
    scene, rays = deck
    moved = sc.sheared(scene)
    for var in ("RT_WF_LANES", "RT_WF_BATCH", "RT_BUILD_METHOD"):
        monkeypatch.delenv(var, raising=False)
    ext = oracle_mod.render_extended(oracle_mod.PackedScene(moved, use_bvh=False), W, H, SPP, BOUNCES, camera=moved.camera, frame_seed=SEED)
    batch = np.ascontiguousarray(np.concatenate([rays["mixed"], rays["through"], rays["corner"]]))
    want_hits = brute_force(moved, batch)
    with rt_api.Context() as ctx:
        ctx.upload_scene(moved)
        fresh_rgb, fresh_st = _frame(ctx, moved, kernel_pipeline=True, counters=True)
        fresh_mark = ctx.debug_stack_mark()
        fresh_hits, fresh_occ = ctx.intersect(batch), ctx.occluded(batch)
    _assert_frame(fresh_rgb, fresh_st, ext, "fresh upload of the sheared deck")
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        _, st0 = _frame(ctx, scene, kernel_pipeline=True, counters=True)
        mark0, depth = ctx.debug_stack_mark(), st0["bvh_depth"]
        assert ctx.update_geometry(moved.vertices["position"].astype(F32))["flags"] == api.STAT_REFIT
        b = ctx.debug_check_bvh()
        assert b["failures"] == 0 and b["placed_once"] == moved.n_triangles and b["depth"] == depth, b
        for label, kw in (("pipeline", dict(kernel_pipeline=True)), ("pipeline counted", dict(kernel_pipeline=True, counters=True)), ("kernel_sm", dict(kernel_sm=True))):
            rgb, st = _frame(ctx, moved, **kw)
            _assert_frame(rgb, st, ext, f"refit, {label}")
            np.testing.assert_array_equal(_bits(rgb), _bits(fresh_rgb), err_msg=f"refit, {label}")
            if kw.get("counters"):
                mark = ctx.debug_stack_mark()
        hits, occ = ctx.intersect(batch), ctx.occluded(batch)
    print(f"refit: depth {depth}, mark {mark0} before the shear, {mark} after it (a fresh build of the sheared deck: depth {fresh_st['bvh_depth']}, mark {fresh_mark})")
    _assert_mark(mark0, depth, "before the shear")
    assert mark <= 2 * depth + 2
    np.testing.assert_array_equal(_bits(hits), _bits(want_hits))
    np.testing.assert_array_equal(_bits(hits), _bits(fresh_hits))
    np.testing.assert_array_equal(occ, _bits(want_hits[:, 3]) != MISS)
    np.testing.assert_array_equal(occ, fresh_occ)


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", TREES)
def test_reference_modes(gpu_ctx, oracle_mod, monkeypatch, deck, tree):
    """Modes 0 and 1 (k_render_reference: `traverse` with depth + 2 entries) against render_frame: prim, t, rgb and rgba8."""
    scene, _ = deck
    if tree == "device":
        monkeypatch.delenv("RT_BUILD_METHOD", raising=False)
    else:
        monkeypatch.setenv("RT_BUILD_METHOD", tree)
    ref = check_reference_modes(gpu_ctx, oracle_mod, scene, W, H, extended=None)
    n = scene.meta["cards"]
    assert (ref["prim"] == 0).mean() >= 0.25 and (ref["prim"] >= n).mean() >= 0.25  # card 0; the wall behind the empty half (and beside the deck)
    assert gpu_ctx.debug_check_bvh()["method"] == (2 if tree == "device" else 0)


# 6 ------------------------------------------------------------------------------------------------------------------------
def _between(rays):
    """The rays with a range that ends between the deck and the wall (origins in front) or leaves the wall out (origins behind):
    "through" rays then have exactly n candidates and "corner" rays none."""
    r = np.array(rays, F32)
    front = r[:, 6] < 0
    r[front, 7] = ((r[front, 2] - F32(sc.Z_WALL + 0.25)) / -r[front, 6]).astype(F32)
    return r


@pytest.fixture(scope="module")
def ray_statements(deck):
    """Per ray set: (rays, brute-force closest hits, all candidates); for "through" and "corner" also with the wall cut off."""
    scene, rays = deck
    out = {}
    for name, r in list(rays.items()) + [("through_cut", _between(rays["through"])), ("corner_cut", _between(rays["corner"]))]:
        r = np.ascontiguousarray(r)
        out[name] = (r, brute_force(scene, r), all_candidates(scene, r))
    return out


@pytest.mark.parametrize("tree", TREES)
def test_intersect_occluded_and_intersect_all(gpu_ctx, monkeypatch, deck, ray_statements, tree):
    scene, _ = deck
    n = scene.meta["cards"]
    _upload(gpu_ctx, monkeypatch, scene, tree)
    for name, (rays, want, cands) in ray_statements.items():
        np.testing.assert_array_equal(_bits(gpu_ctx.intersect(rays)), _bits(want), err_msg=name)
        np.testing.assert_array_equal(gpu_ctx.occluded(rays), _bits(want[:, 3]) != MISS, err_msg=name)
        totals = cands[1]
        for k in (1, 4, 16):
            want_h, want_c = expected_lists(cands, k)
            hits, counts = gpu_ctx.intersect_all(rays, k)
            np.testing.assert_array_equal(_bits(hits), _bits(want_h), err_msg=f"{name} K={k}")
            np.testing.assert_array_equal(counts, want_c, err_msg=f"{name} K={k}")
            hits, counts = gpu_ctx.intersect_all(rays, k, count_all=True)
            np.testing.assert_array_equal(_bits(hits), _bits(want_h), err_msg=f"{name} K={k} COUNT_ALL")
            np.testing.assert_array_equal(counts, totals, err_msg=f"{name} K={k} COUNT_ALL")
        np.testing.assert_array_equal(gpu_ctx.intersect_all(rays, 0, count_all=True)[1], totals, err_msg=name)
        if name == "through_cut":
            assert (totals == n).all(), "a ray through the covered half crosses every card"
        if name == "corner_cut":
            assert (totals == 0).all(), "a ray through the empty corner crosses none"
        if name == "mixed":
            assert (totals >= n).sum() * 2 == len(rays)


@pytest.mark.parametrize("tree", TREES)
def test_surface_and_ambient_occlusion(gpu_ctx, oracle_mod, monkeypatch, deck, ray_statements, tree):
    """rt_surface as test_gpu_surface_ao compares it (position == o + d * t of the brute-force hit, prim, normal, material from the
    scene's arrays); rt_ambient_occlusion against its definition over rt_occluded, which the test above holds to brute force."""
    scene, _ = deck
    _upload(gpu_ctx, monkeypatch, scene, tree)
    rays = np.ascontiguousarray(np.concatenate([ray_statements[k][0] for k in ("mixed", "through", "corner")]))
    want = np.concatenate([ray_statements[k][1] for k in ("mixed", "through", "corner")])
    t, prim = want[:, 0], _bits(want[:, 3])
    pts = gpu_ctx.surface(rays)
    position, prim_id, normal, material_id = api.split_surface(pts)
    hit = prim != MISS
    assert hit.sum() > 500 and (~hit).sum() > 20
    np.testing.assert_array_equal(prim_id, prim)
    np.testing.assert_array_equal(_bits(position[hit]), _bits((rays[:, 0:3] + rays[:, 4:7] * t[:, None])[hit]))
    _, want_nf, want_mid = _surface(scene, rays, t, prim)
    np.testing.assert_allclose(normal[hit], want_nf[hit], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(material_id[hit], want_mid[hit].astype(np.uint32))
    assert not _bits(pts[~hit][:, [0, 1, 2, 4, 5, 6, 7]]).any()
    points = np.ascontiguousarray(pts[hit][:sc.RECORDS])
    for samples, max_distance in ((16, np.inf), (5, 1.5)):
        got = _check_ao(gpu_ctx, oracle_mod, points, samples, 77, max_distance, 1e-3)
        assert got.min() < got.max()


@pytest.mark.parametrize("tree", TREES)
def test_direct_light_and_radiance(gpu_ctx, oracle_mod, monkeypatch, deck, ray_statements, tree):
    """rt_direct_light against its definition with the segments on the tree and on the light grids (same bytes); rt_radiance of the
    camera rays is the one-sample frame, which is the oracle's; without bounces it is rt_direct_light at the surface hit."""
    scene, _ = deck
    _upload(gpu_ctx, monkeypatch, scene, tree)
    rays = np.ascontiguousarray(np.concatenate([ray_statements[k][0] for k in ("mixed", "corner")]))
    pts = gpu_ctx.surface(rays)
    position, prim, _, _ = api.split_surface(pts)
    hit = prim != MISS
    cosang = np.zeros(len(rays))
    cosang[hit] = _geometric_facing(scene, rays[hit], prim[hit], position[hit])
    use = hit & (np.abs(cosang) >= 1e-4)
    assert use.sum() >= sc.RECORDS
    geo = pts.copy()
    geo[cosang > 0, 4:7] = -geo[cosang > 0, 4:7]  # the geometric normal, as the frames' vertices use it
    points = np.ascontiguousarray(pts[hit])
    before = gpu_ctx.direct_light(points)
    assert gpu_ctx.debug_shadow_grid()["lights_with_grid"] == 0
    lit, _, segments = _check_definition(gpu_ctx, scene, points, before, max_excluded=0.02)
    assert 0 < lit.sum() < segments, "some segments are occluded and some are not"
    for shadows in (True, False):
        light, _ = api.split_lighting(gpu_ctx.direct_light(geo, bias=1e-3, ambient=True, shadows=shadows))
        got, _ = api.split_radiance(gpu_ctx.radiance(rays, max_bounces=0, seed=SEED, shadows=shadows))
        np.testing.assert_array_equal(_bits(got[use]), _bits((F32(0) + light[use]) / F32(1)), err_msg=f"shadows={shadows}")
    cam = gpu_ctx.camera_rays(W, H, scene.camera, mode=1)
    one = oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), W, H, 1, BOUNCES, camera=scene.camera, frame_seed=SEED)
    # The deck's lists are long by construction (every card lies behind the next as the lights see them), so the grid build refuses
    # them and every segment walks the tree.  RT_SHADOW_GRID_MEAN lifts the refusal, as test_gpu_direct_light does for its cluttered
    # scenes, on a coarse grid: cells with short lists answer their segments, the others hand theirs on to the tree walk.
    monkeypatch.setenv("RT_SHADOW_GRID_MEAN", "1e9")
    monkeypatch.setenv("RT_SHADOW_GRID_RES", "16")
    for grids in (False, True):
        if grids:
            gpu_ctx.prepare()
            assert gpu_ctx.debug_shadow_grid()["lights_with_grid"] > 0
            with_grids = gpu_ctx.direct_light(points, counters=True)
            answered = gpu_ctx.debug_shadow_grid()["segments_answered"]
            print(f"grids: {[gpu_ctx.debug_shadow_grid(i) for i in range(len(scene.lights))]}, segments answered by the lists {answered} of {gpu_ctx.stats()['rays']}")
            assert with_grids.tobytes() == before.tobytes()
            assert gpu_ctx.direct_light(points, use_grids=False).tobytes() == before.tobytes()
        st_f = gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=1, max_bounces=BOUNCES, frame_seed=SEED, kernel_pipeline=True, no_shadow_grid=not grids)
        frame = gpu_ctx.read_rgb32f()
        _assert_frame(frame, st_f, one, f"one-sample frame, grids={grids}")
        radiance, seg = api.split_radiance(gpu_ctx.radiance(cam, max_bounces=BOUNCES, seed=SEED))
        np.testing.assert_array_equal(_bits(radiance), _bits(frame.reshape(-1, 3)))
        assert int(seg.astype(np.uint64).sum()) == st_f["rays"] == gpu_ctx.stats()["rays"]


@pytest.fixture(scope="module")
def point_statements(deck):
    """(points with radius inf, 0.5, 0.05, inf by index; closest_point's records; the same points with a radius that covers the
    deck and their K = 16 lists and totals; the parity rays' crossing counts; nearest_all of the points with their own radii)."""
    scene, _ = deck
    pos = sc.points()
    points = api.make_points(pos)
    points[:, 3] = np.array([np.inf, 0.5, 0.05, np.inf], F32)[np.arange(len(points)) % 4]
    wide = api.make_points(pos, radius=20.0)
    rec, _, total = ca.nearest_all(scene, wide)
    return points, cc.brute_force(scene, points), wide, rec, total, sd.crossings(scene, pos), ca.nearest_all(scene, points)


@pytest.mark.parametrize("tree", TREES)
def test_closest_point_and_closest_point_all(gpu_ctx, monkeypatch, deck, point_statements, tree):
    scene, _ = deck
    points, want, wide, rec, total, _, (rec_own, _, total_own) = point_statements
    _upload(gpu_ctx, monkeypatch, scene, tree)
    prim = api.split_nearest(want)[4]
    assert (prim == cc.PRIM_MISS).any() and (prim < scene.meta["cards"]).sum() > 100
    same_lists(gpu_ctx.closest_point(points), want)
    assert (total == scene.n_triangles + len(scene.spheres)).all(), "the radius covers the deck: every primitive is a candidate"
    for k in (1, 16):
        want_k, want_c = ca.first_k(rec, total, k)
        out, counts = gpu_ctx.closest_point_all(wide, k)
        same_lists(out, want_k)
        _same_counts(counts, want_c)
        out, counts = gpu_ctx.closest_point_all(wide, k, count_all=True)
        same_lists(out, want_k)
        _same_counts(counts, total)
    _same_counts(gpu_ctx.closest_point_all(wide, 0, count_all=True)[1], total)
    # the points' own radii (inf, 0.5, 0.05): walks that end early on the deep tree, with counts of nothing, of a part and of everything
    everything = scene.n_triangles + len(scene.spheres)
    assert (total_own == 0).sum() >= 16 and ((total_own > 16) & (total_own < everything)).sum() >= 64 and (total_own == everything).sum() >= 64
    for k in (1, 16):
        want_k, want_c = ca.first_k(rec_own, total_own, k)
        out, counts = gpu_ctx.closest_point_all(points, k)
        same_lists(out, want_k)
        _same_counts(counts, want_c)
        out, counts = gpu_ctx.closest_point_all(points, k, count_all=True)
        same_lists(out, want_k)
        _same_counts(counts, total_own)
    _same_counts(gpu_ctx.closest_point_all(points, 0, count_all=True)[1], total_own)
    same_lists(gpu_ctx.closest_point_all(points, 1)[0][:, 0], want)


@pytest.mark.parametrize("tree", TREES)
def test_inside_and_signed_distance(gpu_ctx, monkeypatch, deck, point_statements, tree):
    """The parity walks: a parity ray from a point in the covered half crosses thousands of cards."""
    scene, _ = deck
    points, want, _, _, _, counts, _ = point_statements
    assert counts.max() >= 2000 and (counts == 0).any()
    _upload(gpu_ctx, monkeypatch, scene, tree)
    for rays in (1, 7):
        want_inside, want_votes, _ = sd.statement(scene, points, rays, True, counts=counts)
        inside, votes = gpu_ctx.inside(points, rays=rays, votes=True)
        _same_bytes(inside.view(np.uint8), want_inside)
        _same_bytes(votes, want_votes)
        _same_bytes(gpu_ctx.inside(points, rays=rays).view(np.uint8), want_inside)
        signed_inside, signed_votes, _ = sd.statement(scene, points, rays, True, distance=True, counts=counts)
        rec, votes = gpu_ctx.signed_distance(points, rays=rays, votes=True)
        same_lists(rec, sd.sign(want, signed_inside))
        _same_bytes(votes, signed_votes)
        same_lists(gpu_ctx.signed_distance(points, rays=rays), sd.sign(want, signed_inside))
    assert 0 < want_votes.astype(np.int64).sum() and (want_votes < 7).any()


@pytest.fixture(scope="module")
def sweep_statements(deck):
    scene, rays = deck
    r = np.concatenate([rays["mixed"][:128], rays["corner"][:64], rays["through"][:64]])
    sweeps = sw._pack(r[:, 0:3], r[:, 4:7], np.array([0.02, 0.1, 0.3, 0.6], F32)[np.arange(len(r)) % 4])
    return sweeps, sw.brute_force(scene, sweeps)


@pytest.mark.parametrize("tree", TREES)
def test_sweep_sphere(gpu_ctx, monkeypatch, deck, sweep_statements, tree):
    scene, _ = deck
    sweeps, want = sweep_statements
    face, edge, vertex, sphere, at_start, miss = sw.contact_kinds(want)
    print({k: int(v.sum()) for k, v in dict(face=face, edge=edge, vertex=vertex, sphere=sphere, at_start=at_start, miss=miss).items()})
    assert face.sum() > 20 and (edge | vertex).sum() > 20
    _upload(gpu_ctx, monkeypatch, scene, tree)
    same_lists(gpu_ctx.sweep_sphere(sweeps), want)
