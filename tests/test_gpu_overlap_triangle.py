"""Triangle queries on the MI355X (rt_overlap_triangle).  Every comparison with the float32 statement (overlap_triangle_cases.py's numpy
evaluation of every query triangle against every triangle and sphere) is byte for byte, ids and counts: the result is a set picked by
one f32 statement and listed by key, so it is the statement's whatever tree, memory, batch size or device count is in use."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
import overlap_triangle_cases as tc
import stack_cases as sc
from gpu_raytracer_amd import api, scenes

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
MISS = cc.PRIM_MISS
KS = (1, 4, 16, 32)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _same_counts(got, want):
    np.testing.assert_array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64))


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_tris(soup):
    t = tc.soup_triangles(soup, 2048, 11)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def soup_want(soup, soup_tris):
    """The statement at K = 32, computed once: (ids (N, 32), total counts); tc.first_k gives every smaller K."""
    ids, _, total = tc.overlap_all(soup, soup_tris)
    ids.setflags(write=False)
    total.setflags(write=False)
    return ids, total


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_the_batch_fills_and_overflows_its_lists(soup_want, soup, soup_tris):
    """A batch that never fills or never overflows a list proves nothing: at K = 4 and at K = 16 more than 5 % of the queries hold some
    but fewer than K primitives, and more than 5 % hold more than K; some hold more than 32, and a sphere is listed.  On the CPU:
    28.6 % / 22.1 % at K = 4, 45.0 % / 7.9 % at K = 16, 1.9 % above 32, 46.3 % empty."""
    ids, total = soup_want
    for k in (4, 16):
        short, over = ((total > 0) & (total < k)).mean(), (total > k).mean()
        print(f"K = {k}: {short:.1%} of the queries with 1 .. {k - 1} primitives, {over:.1%} with more than {k}, {(total == 0).mean():.1%} with none")
        assert short > 0.05 and over > 0.05
    assert (total > 32).any() and (ids[total > 0, 0] >= cc.SPHERE_FLAG).any()


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_soup_equals_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_tris, soup_want, k):
    want, want_counts = tc.first_k(*soup_want, k)
    n = len(soup_tris)
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.overlap_triangle(soup_tris, k)
    assert out.shape == (n, k) and out.dtype == np.uint32 and counts.dtype == np.uint32
    _same(out, want)
    _same_counts(counts, want_counts)
    st = gpu_ctx.stats()
    assert st["rays"] == n and st["pixels"] == 0 and st["primary_rays"] == 0 and st["shadow_rays"] == 0 and st["continuation_rays"] == 0
    assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["kernel_ms"] > 0
    own, own_counts = np.full((n, k), 7, np.uint32), np.full(n, 77, np.uint32)
    got = gpu_ctx.overlap_triangle(soup_tris, k, out=own, counts=own_counts, counters=True)
    assert got[0] is own and got[1] is own_counts
    _same(own, want)
    _same_counts(own_counts, want_counts)
    st = gpu_ctx.stats()
    assert st["node_visits"] > 0 and st["tri_tests"] > 0 and st["rays"] == n
    if torch is None:
        pytest.skip("torch is not installed: device memory not exercised")
    dev = torch.from_numpy(np.array(soup_tris)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    out, counts = gpu_ctx.overlap_triangle(dev, k)
    assert out.device == dev.device and out.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(out.shape) == (n, k)
    _same(out.cpu().numpy(), want)
    _same_counts(counts.cpu().numpy(), want_counts)
    pre, pre_counts = torch.empty((n, k), dtype=torch.int32, device="cuda:0"), torch.empty(n, dtype=torch.int32, device="cuda:0")
    got = gpu_ctx.overlap_triangle(dev, k, out=pre, counts=pre_counts)
    assert got[0] is pre and got[1] is pre_counts
    _same(pre.cpu().numpy(), want)
    _same_counts(pre_counts.cpu().numpy(), want_counts)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_count_all_counts_everything_and_lists_the_same(gpu_ctx, soup, soup_tris, soup_want):
    ids, total = soup_want
    assert (total > 32).any()
    gpu_ctx.upload_scene(soup)
    none, counts = gpu_ctx.overlap_triangle(soup_tris, 0, count_all=True)
    assert none is None
    _same_counts(counts, total)
    for k in (4, 32):
        out, counts = gpu_ctx.overlap_triangle(soup_tris, k, count_all=True)
        _same(out, tc.first_k(ids, total, k)[0])
        _same_counts(counts, total)
        plain, listed = gpu_ctx.overlap_triangle(soup_tris, k)
        _same(plain, out)
        _same_counts(listed, np.minimum(total, k))


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_any_is_total_above_zero_on_both_trees_and_stops_early(gpu_ctx, soup, soup_tris, soup_want):
    _, total = soup_want
    gpu_ctx.upload_scene(soup)
    for quality_tree in (False, True):
        if quality_tree:
            gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
        none, hit = gpu_ctx.overlap_triangle(soup_tris, 0, any_hit=True, counters=True)
        st_any = gpu_ctx.stats()
        assert none is None and hit.dtype == np.uint32
        _same_counts(hit, total > 0)
        _, counts = gpu_ctx.overlap_triangle(soup_tris, 0, count_all=True, counters=True)
        st_all = gpu_ctx.stats()
        _same_counts(counts, total)
        print(f"quality tree {quality_tree}: ANY {st_any['node_visits'] / len(total):.1f} node visits and {st_any['tri_tests'] / len(total):.1f} records "
              f"per query, count only {st_all['node_visits'] / len(total):.1f} and {st_all['tri_tests'] / len(total):.1f}")
        assert 0 < st_any["tri_tests"] < st_all["tri_tests"] and 0 < st_any["node_visits"] <= st_all["node_visits"]


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_boundaries(gpu_ctx, soup, soup_tris, soup_want, n):
    want, want_counts = tc.first_k(*soup_want, 4)
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.overlap_triangle(np.ascontiguousarray(soup_tris[:n]), 4)
    _same(out, want[:n])
    _same_counts(counts, want_counts[:n])
    _, total = gpu_ctx.overlap_triangle(np.ascontiguousarray(soup_tris[:n]), 0, count_all=True)
    _same_counts(total, soup_want[1][:n])


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality_tree", [False, True], ids=["device_tree", "quality_tree"])
def test_lattice_triangles_on_coplanar_walls(gpu_ctx, quality_tree):
    """Vertices, edges and whole queries lie exactly in the walls' planes, on their shared edges and corners: touching is listed, bit
    for bit the statement's, whatever order the walk meets the triangles in and wherever the list ends."""
    scene, tris = ca.coplanar_walls(), tc.lattice_triangles()
    ids, _, total = tc.overlap_all(scene, tris)
    assert total.max() == 8 and all((total == t).any() for t in range(9)), "from nothing to all eight triangles"
    gpu_ctx.upload_scene(scene)
    if quality_tree:
        gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    for k in (1, 2, 3, 4, 32):
        want, want_counts = tc.first_k(ids, total, k)
        out, counts = gpu_ctx.overlap_triangle(tris, k)
        _same(out, want)
        _same_counts(counts, want_counts)
        out, counts = gpu_ctx.overlap_triangle(tris, k, count_all=True)
        _same(out, want)
        _same_counts(counts, total)
    _same_counts(gpu_ctx.overlap_triangle(tris, 0, any_hit=True)[1], total > 0)


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_tree(gpu_ctx, soup, soup_tris, soup_want):
    want, want_counts = tc.first_k(*soup_want, 32)
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.overlap_triangle(soup_tris, 32, count_all=True)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    out_q, counts_q = gpu_ctx.overlap_triangle(soup_tris, 32, count_all=True)
    _same(out_q, out)
    _same_counts(counts_q, counts)
    _same(out_q, want)
    _same_counts(counts_q, soup_want[1])


def test_refit_results_are_a_fresh_uploads(gpu_ctx, soup, soup_tris, soup_want):
    """After rt_update_geometry (a refit; vertices jittered by sigma = 0.05) the ids and totals are those of a fresh upload of the
    moved scene, and for more than half of the queries that had hits not those of the scene before."""
    pos = np.ascontiguousarray(soup.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.05, pos.shape)).astype(F32)
    v = soup.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(soup, vertices=v)
    gpu_ctx.upload_scene(soup)
    before, before_counts = gpu_ctx.overlap_triangle(soup_tris, 32, count_all=True)
    _same(before, soup_want[0])
    assert gpu_ctx.update_geometry(moved_pos)["flags"] == api.STAT_REFIT
    refitted, refitted_counts = gpu_ctx.overlap_triangle(soup_tris, 32, count_all=True)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        out, counts = fresh.overlap_triangle(soup_tris, 32, count_all=True)
    _same(refitted, out)
    _same_counts(refitted_counts, counts)
    had = before_counts > 0
    print(f"{had.sum()} queries had hits; the refit changed the list of {(refitted != before).any(1)[had].mean():.1%} of them")
    assert had.sum() > 1000 and (refitted != before).any(1)[had].mean() > 0.5


# 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality_tree", [False, True], ids=["device_tree", "quality_tree"])
def test_the_deck_at_the_stacks_high_water_mark(gpu_ctx, quality_tree):
    """The deck's boxes overlap completely in x and y, so a sliver along z enters every node that holds a card, whether it touches a
    card (the covered half: all N_CARDS of them) or none (the empty corner): the deepest stack a walk can build.  A node refers to at
    most 8 leaves of at most 4 records, so a query that enters every card's box visits at least N_CARDS / 32 nodes and reads at least
    N_CARDS records."""
    scene = sc.deck_scene()
    n_cards = sc.N_CARDS
    gpu_ctx.upload_scene(scene)
    if quality_tree:
        gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    corner, covered, mixed = tc.deck_triangles("corner"), tc.deck_triangles("covered"), tc.deck_triangles("mixed")
    none, counts = gpu_ctx.overlap_triangle(corner, 0, count_all=True, counters=True)
    st = gpu_ctx.stats()
    _same_counts(counts, np.zeros(len(corner)))
    print(f"deck, quality tree {quality_tree}: {st['node_visits'] / len(corner):.1f} node visits and {st['tri_tests'] / len(corner):.1f} records per corner "
          f"sliver, {st['bvh_nodes']} nodes, depth {st['bvh_depth']}")
    assert st["node_visits"] >= len(corner) * (n_cards // 32) > 0 and st["tri_tests"] >= len(corner) * n_cards
    _same_counts(gpu_ctx.overlap_triangle(corner, 0, any_hit=True)[1], np.zeros(len(corner)))
    out, counts = gpu_ctx.overlap_triangle(covered, 32, count_all=True)
    _same_counts(counts, np.full(len(covered), n_cards))
    _same(out, np.tile(np.arange(32, dtype=np.uint32), (len(covered), 1)))
    out, counts = gpu_ctx.overlap_triangle(covered, 32)
    _same_counts(counts, np.full(len(covered), 32))
    _same(out, np.tile(np.arange(32, dtype=np.uint32), (len(covered), 1)))
    # lanes that finish at once beside lanes that visit everything, against the statement
    ids, _, total = tc.overlap_all(scene, mixed)
    is_covered = sc.mixed_covered(len(mixed))
    assert (total == np.where(is_covered, n_cards, 0)).all() and is_covered.any() and not is_covered.all()
    out, counts = gpu_ctx.overlap_triangle(mixed, 32, count_all=True)
    _same(out, ids)
    _same_counts(counts, total)
    _same_counts(gpu_ctx.overlap_triangle(mixed, 0, any_hit=True)[1], is_covered)


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_non_finite_queries_touch_nothing_without_a_walk(gpu_ctx, soup):
    gpu_ctx.upload_scene(soup)
    a, b, c = (-1, -1, -3), (1, -1, -3), (0, 1, -2)
    q = tc.make_triangles([(NAN, -1, -3), (-1, NAN, -3), (-1, -1, INF), a, a, a, a, a, a],
                          [b, b, b, (NAN, -1, -3), (1, -INF, -3), (1, -1, NAN), b, b, b],
                          [c, c, c, c, c, c, (INF, 1, -2), (0, NAN, -2), (0, 1, -INF)])
    assert not tc.valid(q).any()
    for k, kw in ((4, {}), (32, {"count_all": True}), (0, {"count_all": True}), (0, {"any_hit": True})):
        out, counts = gpu_ctx.overlap_triangle(q, k, counters=True, **kw)
        if k:
            _same(out, np.full((len(q), k), MISS, np.uint32))
        _same_counts(counts, np.zeros(len(q)))
        st = gpu_ctx.stats()
        assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(q)
    # finite degenerate queries walk: the same corner as a point, as a segment and as the triangle
    good = tc.make_triangles([a, a, a], [a, b, b], [a, b, c])
    _, counts = gpu_ctx.overlap_triangle(good, 0, count_all=True, counters=True)
    assert gpu_ctx.stats()["node_visits"] > 0
    _same_counts(counts, tc.overlap_all(soup, good)[2])


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_the_walk_culls(gpu_ctx, soup):
    """A walk that skips nothing passes every equality above.  2048 triangles with their vertices within 0.08 per axis of a point
    near a surface, counting every touching primitive: the brute force reads 3000 records per query, and the bound is a tenth of
    that."""
    centres = cc.near_surface(soup, 2048, 31).astype(np.float64)
    v = (centres[:, None, :] + np.random.default_rng(31).uniform(-0.08, 0.08, (2048, 3, 3))).astype(F32)
    tris = tc.make_triangles(v[:, 0], v[:, 1], v[:, 2])
    gpu_ctx.upload_scene(soup)
    _, counts = gpu_ctx.overlap_triangle(tris, 0, count_all=True, counters=True)
    st = gpu_ctx.stats()
    n, n_tris = len(tris), len(soup.triangles)
    print(f"soup, {n} small triangles near surfaces, count only: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} records per query "
          f"(brute force: {n_tris}); {np.asarray(counts).mean():.2f} primitives touched per query")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * n_tris / 10
    _same_counts(counts, tc.overlap_all(soup, tris)[2])


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(gpu_ctx, soup, soup_tris, soup_want):
    n = 8
    tris = np.array(soup_tris[:n])
    out, counts = np.full((n, 33), 7, np.uint32), np.full(n, 77, np.uint32)
    lib, h = gpu_ctx.lib, gpu_ctx._h
    ALL, ANY = api.QUERY_COUNT_ALL, api.OVERLAP_ANY

    def call(b, k, o, c, flags, m=n):
        return lib.rt_overlap_triangle(h, C.c_void_p(b), C.c_size_t(m), C.c_uint32(k), C.c_void_p(o), C.c_void_p(c), C.c_uint32(flags))

    B, O, Cn = tris.ctypes.data, out.ctypes.data, counts.ctypes.data
    assert call(B, 4, O, Cn, 0) == -4, "RT_ERR_NOT_UPLOADED before an upload"
    with pytest.raises(api.RtError) as e:
        gpu_ctx.overlap_triangle(tris, 4)
    assert e.value.code == -4
    gpu_ctx.upload_scene(soup)
    gpu_ctx.overlap_triangle(tris, 2)
    before = gpu_ctx.stats()
    assert call(B, 33, O, Cn, 0) == -1                                    # max_prims > RT_OVERLAP_MAX
    assert call(B, 0, O, Cn, 0) == -1                                     # max_prims == 0 without RT_QUERY_COUNT_ALL or RT_OVERLAP_ANY
    assert call(B, 0, O, None, ALL) == -1 and call(B, 0, O, None, ANY) == -1  # ... without counts
    assert call(B, 4, O, Cn, ANY) == -1 and call(B, 0, O, Cn, ANY | ALL) == -1  # RT_OVERLAP_ANY lists nothing and counts to one
    assert call(None, 4, O, Cn, 0) == -1
    assert "triangles is NULL" in lib.rt_last_error(h).decode(), "the message names the call's own input"
    assert call(B, 4, None, Cn, 0) == -1
    assert call(B, 4, O, Cn, 8) == -1 and call(B, 4, O, Cn, 0x80000000) == -1, "unknown flag bits"
    assert (out == 7).all() and (counts == 77).all()
    assert gpu_ctx.stats()["rays"] == before["rays"] == n
    assert call(None, 4, None, None, 0, m=0) == 0, "n == 0 is RT_OK"
    assert call(B, 4, O, None, 0) == 0, "counts may be NULL with max_prims > 0"
    _same(out.reshape(-1)[:n * 4].reshape(n, 4), tc.first_k(*soup_want, 4)[0][:n])
    assert (out.reshape(-1)[n * 4:] == 7).all()
    empty = gpu_ctx.overlap_triangle(np.zeros((0, 12), F32), 4)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0,)
    if torch is None:
        pytest.skip("torch is not installed: mixed memory kinds not exercised")
    dev = torch.from_numpy(tris).to("cuda:0")
    dout, dcounts = torch.full((n, 4), 7, dtype=torch.int32, device="cuda:0"), torch.full((n,), 77, dtype=torch.int32, device="cuda:0")
    assert call(dev.data_ptr(), 4, O, Cn, 0) == -1 and call(B, 4, dout.data_ptr(), Cn, 0) == -1 and call(dev.data_ptr(), 4, dout.data_ptr(), Cn, 0) == -1
    assert call(B, 4, O, dcounts.data_ptr(), 0) == -1, "mixed host and device buffers"
    assert (dout == 7).all() and (dcounts == 77).all()
    buf = torch.zeros(n * 12 + 1, device="cuda:0")  # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    with pytest.raises(api.RtError) as e:
        gpu_ctx.overlap_triangle(buf[1:].view(-1, 12), 4)
    assert e.value.code == -1 and "aligned" in str(e.value) and "triangles" in str(e.value)
    _same(gpu_ctx.overlap_triangle(dev, 4)[0].cpu().numpy(), tc.first_k(*soup_want, 4)[0][:n])


def test_side_effects_an_empty_scene_and_spheres_alone(gpu_ctx, soup, soup_tris, soup_want):
    want, want_counts = tc.first_k(*soup_want, 4)
    gpu_ctx.upload_scene(soup)
    # the last frame and a running accumulation are left alone
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    out, counts = gpu_ctx.overlap_triangle(soup_tris, 4)
    _same(out, want)
    _same_counts(counts, want_counts)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_tris) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["shadow_rays"] == 0
    _same(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4, "the running image went on"
    # an empty scene: nothing
    gpu_ctx.upload_scene(scenes.empty_scene())
    for k in (1, 32):
        out, counts = gpu_ctx.overlap_triangle(soup_tris, k, count_all=True)
        _same(out, np.full((len(soup_tris), k), MISS, np.uint32))
        _same_counts(counts, np.zeros(len(soup_tris)))
    _same_counts(gpu_ctx.overlap_triangle(soup_tris, 0, any_hit=True)[1], np.zeros(len(soup_tris)))
    # spheres alone: no tree to walk
    balls = dataclasses.replace(soup, vertices=soup.vertices[:0], triangles=soup.triangles[:0])
    assert len(balls.triangles) == 0 and len(balls.spheres) == 3
    ids, _, total = tc.overlap_all(balls, soup_tris, 4)
    assert (total > 0).any() and (ids[total > 0, 0] >= cc.SPHERE_FLAG).all()
    gpu_ctx.upload_scene(balls)
    out, counts = gpu_ctx.overlap_triangle(soup_tris, 4, count_all=True)
    _same(out, ids)
    _same_counts(counts, total)
    _same_counts(gpu_ctx.overlap_triangle(soup_tris, 0, any_hit=True)[1], total > 0)


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_a_context_over_one_device_twice_gives_the_same_bytes(soup, soup_tris, soup_want):
    want, want_counts = tc.first_k(*soup_want, 32)
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(soup)
        out, counts = ctx.overlap_triangle(soup_tris, 32)
        _same(out, want)
        _same_counts(counts, want_counts)
        _, total = ctx.overlap_triangle(soup_tris, 0, count_all=True, counters=True)
        _same_counts(total, soup_want[1])
        assert ctx.stats()["rays"] == len(soup_tris) and ctx.stats()["tri_tests"] > 0


def test_two_devices_give_the_one_device_bytes(soup, soup_tris, soup_want):
    if torch is None or torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    want, want_counts = tc.first_k(*soup_want, 32)
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        out, counts = ctx.overlap_triangle(soup_tris, 32)
        _same(out, want)
        _same_counts(counts, want_counts)
        dev = torch.from_numpy(np.array(soup_tris)).to("cuda:1")
        out, counts = ctx.overlap_triangle(dev, 32)
        _same(out.cpu().numpy(), want)
        _same_counts(counts.cpu().numpy(), want_counts)
