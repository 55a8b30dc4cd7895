"""Triangle contacts on the MI355X (rt_contact_triangle).  Every comparison with the float32 statement (contact_triangle_cases.py's
numpy evaluation of every query triangle against every triangle and sphere) is byte for byte, records and counts: the result is a
set picked and ordered by one f32 statement, so it is the statement's whatever tree, memory, batch size or device count is in use.
For a point (three equal vertices) the yardstick is the library itself: rt_closest_point_all in the same context."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
import contact_triangle_cases as kt
import stack_cases as sk
from gpu_raytracer_amd import api, scenes

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
MISS = cc.PRIM_MISS
KS = (1, 4, 16)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _same_counts(got, want):
    np.testing.assert_array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64))


def _misses(tris, k):
    out = np.zeros((len(tris), k, 8), F32)
    out[..., 3] = np.asarray(tris)[:, 3, None]
    out.view(np.uint32)[..., 6] = MISS
    return out


@pytest.fixture(scope="module")
def soup():
    return kt.soup()


@pytest.fixture(scope="module")
def soup_tris():
    return kt.soup_reference()[0]


@pytest.fixture(scope="module")
def soup_want():
    """The statement at K = 16, computed once and read-only: (records (N, 16, 8), total counts); kt.first_k gives every smaller K."""
    _, _, recs, total = kt.soup_reference()
    return recs, total


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_the_batch_fills_and_overflows_its_lists(soup_want):
    """A batch that never fills or never overflows a list proves nothing: at K = 4 and at K = 16 more than 5 % of the queries hold
    some but fewer than K contacts, more than 5 % hold more than K, and some hold none.  On the CPU: 21.6 % / 46.5 % at K = 4,
    45.5 % / 25.1 % at K = 16, 28.3 % empty."""
    _, total = soup_want
    for k in (4, 16):
        short, over, none = kt.batch_condition(total, k)
        print(f"K = {k}: {short:.1%} of the queries with 1 .. {k - 1} contacts, {over:.1%} with more than {k}, {none:.1%} with none")
        assert short > 0.05 and over > 0.05 and none > 0


@pytest.mark.parametrize("k", KS)
def test_soup_equals_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_tris, soup_want, k):
    want, want_counts = kt.first_k(*soup_want, k)
    n = len(soup_tris)
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.contact_triangle(soup_tris, k)
    assert out.shape == (n, k, 8) and out.dtype == np.float32 and counts.dtype == np.uint32
    _same(out, want)
    _same_counts(counts, want_counts)
    st = gpu_ctx.stats()
    assert st["rays"] == n and st["pixels"] == 0 and st["primary_rays"] == 0 and st["shadow_rays"] == 0 and st["continuation_rays"] == 0
    assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["kernel_ms"] > 0
    own, own_counts = np.full((n, k, 8), 7, F32), np.full(n, 77, np.uint32)
    got = gpu_ctx.contact_triangle(soup_tris, k, out=own, counts=own_counts, counters=True)
    assert got[0] is own and got[1] is own_counts
    _same(own, want)
    _same_counts(own_counts, want_counts)
    st = gpu_ctx.stats()
    assert st["node_visits"] > 0 and st["tri_tests"] > 0 and st["rays"] == n
    if torch is None:
        pytest.skip("torch is not installed: device memory not exercised")
    dev = torch.from_numpy(np.array(soup_tris)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    out, counts = gpu_ctx.contact_triangle(dev, k)
    assert out.device == dev.device and out.dtype == torch.float32 and counts.dtype == torch.int32 and tuple(out.shape) == (n, k, 8)
    _same(out.cpu().numpy(), want)
    _same_counts(counts.cpu().numpy(), want_counts)
    pre, pre_counts = torch.empty((n, k, 8), dtype=torch.float32, device="cuda:0"), torch.empty(n, dtype=torch.int32, device="cuda:0")
    got = gpu_ctx.contact_triangle(dev, k, out=pre, counts=pre_counts)
    assert got[0] is pre and got[1] is pre_counts
    _same(pre.cpu().numpy(), want)
    _same_counts(pre_counts.cpu().numpy(), want_counts)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_count_all_counts_everything_and_lists_the_same(gpu_ctx, soup, soup_tris, soup_want):
    recs, total = soup_want
    assert (total > 16).any()
    gpu_ctx.upload_scene(soup)
    none, counts = gpu_ctx.contact_triangle(soup_tris, 0, count_all=True)
    assert none is None
    _same_counts(counts, total)
    for k in (4, 16):
        out, counts = gpu_ctx.contact_triangle(soup_tris, k, count_all=True)
        _same(out, kt.first_k(recs, total, k)[0])
        _same_counts(counts, total)
        plain, listed = gpu_ctx.contact_triangle(soup_tris, k)
        _same(plain, out)
        _same_counts(listed, np.minimum(total, k))


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_any_is_total_above_zero_on_both_trees_and_stops_early(gpu_ctx, soup, soup_tris, soup_want):
    _, total = soup_want
    gpu_ctx.upload_scene(soup)
    for quality_tree in (False, True):
        if quality_tree:
            gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
        none, hit = gpu_ctx.contact_triangle(soup_tris, 0, any_hit=True, counters=True)
        st_any = gpu_ctx.stats()
        assert none is None and hit.dtype == np.uint32
        _same_counts(hit, total > 0)
        _, counts = gpu_ctx.contact_triangle(soup_tris, 0, count_all=True, counters=True)
        st_all = gpu_ctx.stats()
        _same_counts(counts, total)
        print(f"quality tree {quality_tree}: ANY {st_any['node_visits'] / len(total):.1f} node visits and {st_any['tri_tests'] / len(total):.1f} triangle tests "
              f"per query, count only {st_all['node_visits'] / len(total):.1f} and {st_all['tri_tests'] / len(total):.1f}")
        assert 0 < st_any["tri_tests"] < st_all["tri_tests"] and 0 < st_any["node_visits"] <= st_all["node_visits"]


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_a_point_is_closest_point_all_in_the_same_context(gpu_ctx, soup, soup_tris):
    """The queries collapsed to v0, some with no margin at all: words 0 - 3 and 6 - 7 of every record are rt_closest_point_all's, qu
    and qv are 0, the counts are equal, and at K = 1 so are the node visits and the triangle tests."""
    tris = np.array(soup_tris)
    tris[:, 4:7] = tris[:, 8:11] = tris[:, 0:3]
    tris[::7, 3] = INF
    points = np.ascontiguousarray(tris[:, :4])
    gpu_ctx.upload_scene(soup)
    for k in KS:
        want, want_counts = gpu_ctx.closest_point_all(points, k, counters=True)
        st_points = gpu_ctx.stats()
        got, counts = gpu_ctx.contact_triangle(tris, k, counters=True)
        st = gpu_ctx.stats()
        _same(got[..., [0, 1, 2, 3, 6, 7]], want[..., [0, 1, 2, 3, 6, 7]])
        assert not got.view(np.uint32)[..., 4:6].any()
        _same_counts(counts, want_counts)
        if k == 1:
            assert st["node_visits"] == st_points["node_visits"] > 0 and st["tri_tests"] == st_points["tri_tests"] > 0
    finite = np.array(soup_tris)
    finite[:, 4:7] = finite[:, 8:11] = finite[:, 0:3]
    _, want_total = gpu_ctx.closest_point_all(np.ascontiguousarray(finite[:, :4]), 0, count_all=True)
    _, total = gpu_ctx.contact_triangle(finite, 0, count_all=True)
    _same_counts(total, want_total)
    assert (np.asarray(total) > 16).any() and (np.asarray(total) == 0).any()


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_what_overlaps_is_in_contact(gpu_ctx, soup, soup_tris):
    """Every margin at 0.05: where rt_overlap_triangle finds something, so does this query, element by element in the same context
    (a touching pair's f32 distance is at most K_TOUCH x the diagonal, far below the margin)."""
    assert kt.K_TOUCH["soup"] * kt.diagonal(soup) < 0.05
    tris = kt.with_margin(soup_tris, 0.05)
    gpu_ctx.upload_scene(soup)
    _, near = gpu_ctx.contact_triangle(tris, 0, any_hit=True)
    _, touch = gpu_ctx.overlap_triangle(tris, 0, any_hit=True)
    near, touch = np.asarray(near), np.asarray(touch)
    assert touch.sum() > 200 and (near >= touch).all() and (near > touch).any()


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_boundaries(gpu_ctx, soup, soup_tris, soup_want, n):
    want, want_counts = kt.first_k(*soup_want, 4)
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.contact_triangle(np.ascontiguousarray(soup_tris[:n]), 4)
    _same(out, want[:n])
    _same_counts(counts, want_counts[:n])
    _, total = gpu_ctx.contact_triangle(np.ascontiguousarray(soup_tris[:n]), 0, count_all=True)
    _same_counts(total, soup_want[1][:n])


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality_tree", [False, True], ids=["device_tree", "quality_tree"])
def test_lattice_triangles_on_coplanar_walls(gpu_ctx, quality_tree):
    """Vertices on the half-integer lattice over walls that share edges, corners and diagonals: the contacts tie bit for bit and are
    ordered by key, whatever order the walk meets the triangles in and wherever the list ends."""
    scene, tris = ca.coplanar_walls(), kt.lattice_triangles()
    recs, _, total = kt.contacts_all(scene, tris)
    d = recs[..., 3]
    listed = np.ascontiguousarray(recs[..., 6]).view(np.uint32) != MISS
    assert (total == 0).any() and total.max() >= 8 and (listed[:, 1] & (d[:, 0] == d[:, 1])).mean() > 0.5, "ties decide most lists"
    assert (listed[:, 0] & (d[:, 0] == 0)).any() and (listed[:, 0] & (d[:, 0] > 0)).any()
    gpu_ctx.upload_scene(scene)
    if quality_tree:
        gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    for k in (1, 2, 3, 4, 16):
        want, want_counts = kt.first_k(recs, total, k)
        out, counts = gpu_ctx.contact_triangle(tris, k)
        _same(out, want)
        _same_counts(counts, want_counts)
        out, counts = gpu_ctx.contact_triangle(tris, k, count_all=True)
        _same(out, want)
        _same_counts(counts, total)
    _same_counts(gpu_ctx.contact_triangle(tris, 0, any_hit=True)[1], total > 0)


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_tree(gpu_ctx, soup, soup_tris, soup_want):
    gpu_ctx.upload_scene(soup)
    out, counts = gpu_ctx.contact_triangle(soup_tris, 16, count_all=True)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    out_q, counts_q = gpu_ctx.contact_triangle(soup_tris, 16, count_all=True)
    _same(out_q, out)
    _same_counts(counts_q, counts)
    _same(out_q, soup_want[0])
    _same_counts(counts_q, soup_want[1])


def test_refit_results_are_a_fresh_uploads(gpu_ctx, soup, soup_tris, soup_want):
    """After rt_update_geometry (a refit; vertices jittered by sigma = 0.05) the records and totals are those of a fresh upload of the
    moved scene, and not those of the scene before."""
    pos = np.ascontiguousarray(soup.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.05, pos.shape)).astype(F32)
    v = soup.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(soup, vertices=v)
    gpu_ctx.upload_scene(soup)
    before, before_counts = gpu_ctx.contact_triangle(soup_tris, 16, count_all=True)
    _same(before, soup_want[0])
    assert gpu_ctx.update_geometry(moved_pos)["flags"] == api.STAT_REFIT
    refitted, refitted_counts = gpu_ctx.contact_triangle(soup_tris, 16, count_all=True)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        out, counts = fresh.contact_triangle(soup_tris, 16, count_all=True)
    _same(refitted, out)
    _same_counts(refitted_counts, counts)
    had = before_counts > 0
    assert had.sum() > 1000 and (refitted.view(np.uint32) != before.view(np.uint32)).any((1, 2))[had].mean() > 0.5


# 9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality_tree", [False, True], ids=["device_tree", "quality_tree"])
def test_the_deck_at_the_stacks_high_water_mark(gpu_ctx, quality_tree):
    """The deck's boxes overlap completely in x and y, so a long thin sliver along z enters every node that holds a card, whether it
    passes through every card (the covered half: all N_CARDS of them at distance 0) or is near none (the empty corner): the deepest
    stack a walk can build.  A node refers to at most 8 leaves of at most 4 records, so a sliver that enters every card's box visits
    at least N_CARDS / 32 nodes and reads at least N_CARDS records."""
    scene = sk.deck_scene()
    n_cards = sk.N_CARDS
    gpu_ctx.upload_scene(scene)
    if quality_tree:
        gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    corner, covered, mixed = kt.deck_triangles("corner"), kt.deck_triangles("covered"), kt.deck_triangles("mixed")
    none, counts = gpu_ctx.contact_triangle(corner, 0, count_all=True, counters=True)
    st = gpu_ctx.stats()
    _same_counts(counts, np.zeros(len(corner)))
    print(f"deck, quality tree {quality_tree}: {st['node_visits'] / len(corner):.1f} node visits and {st['tri_tests'] / len(corner):.1f} records per corner "
          f"sliver, {st['bvh_nodes']} nodes, depth {st['bvh_depth']}")
    assert st["node_visits"] >= len(corner) * (n_cards // 32) > 0 and st["tri_tests"] >= len(corner) * n_cards
    _same_counts(gpu_ctx.contact_triangle(corner, 0, any_hit=True)[1], np.zeros(len(corner)))
    _same(gpu_ctx.contact_triangle(corner, 16)[0], _misses(corner, 16))
    recs, _, total = kt.contacts_all(scene, covered)
    assert (total == n_cards).all() and (np.ascontiguousarray(recs[..., 6]).view(np.uint32) == np.arange(16)[None]).all() and not recs[..., 3].any()
    out, counts = gpu_ctx.contact_triangle(covered, 16, count_all=True)
    _same(out, recs)
    _same_counts(counts, total)
    out, counts = gpu_ctx.contact_triangle(covered, 16)
    _same(out, recs)
    _same_counts(counts, np.full(len(covered), 16))
    # lanes that list every card beside lanes that list none, against the statement
    recs, _, total = kt.contacts_all(scene, mixed)
    is_covered = sk.mixed_covered(len(mixed))
    assert (total == np.where(is_covered, n_cards, 0)).all() and is_covered.any() and not is_covered.all()
    out, counts = gpu_ctx.contact_triangle(mixed, 16, count_all=True)
    _same(out, recs)
    _same_counts(counts, total)
    _same_counts(gpu_ctx.contact_triangle(mixed, 0, any_hit=True)[1], is_covered)


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_degenerate_queries_list_nothing_without_a_walk(gpu_ctx, soup):
    gpu_ctx.upload_scene(soup)
    a, b, c = (0, 0, -3), (0, 0.5, -3), (0.5, 0, -3)
    bad = [NAN, INF, -INF]
    v0 = [(x, 0, -3) for x in bad] + [a] * 6 + [a] * 4
    v1 = [b] * 3 + [(0, x, -3) for x in bad] + [b] * 3 + [b] * 4
    v2 = [c] * 6 + [(0.5, 0, x) for x in bad] + [c] * 4
    q = kt.make_contact_triangles(np.array(v0, F32), np.array(v1, F32), np.array(v2, F32), [1] * 9 + [NAN, 0, -1, -INF])
    assert not kt.valid(q).any()
    for k, kw in ((4, {}), (16, {"count_all": True}), (0, {"count_all": True}), (0, {"any_hit": True})):
        out, counts = gpu_ctx.contact_triangle(q, k, counters=True, **kw)
        if k:
            _same(out, _misses(q, k))
        _same_counts(counts, np.zeros(len(q)))
        st = gpu_ctx.stats()
        assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(q)
    good = kt.make_contact_triangles([a], [b], [c], 1.0)  # the same pose with a valid margin walks
    _, counts = gpu_ctx.contact_triangle(good, 0, count_all=True, counters=True)
    assert gpu_ctx.stats()["node_visits"] > 0
    _same_counts(counts, kt.contacts_all(soup, good)[2])
    wide = kt.make_contact_triangles([a], [b], [c], INF)  # an infinite margin is allowed: the 16 nearest of the whole scene
    out, counts = gpu_ctx.contact_triangle(wide, 16, count_all=True)
    recs, _, total = kt.contacts_all(soup, wide)
    _same(out, recs)
    _same_counts(counts, total)
    assert total[0] == len(soup.triangles) + len(soup.spheres)


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(gpu_ctx, soup, soup_tris, soup_want):
    n = 8
    tris = np.array(soup_tris[:n])
    out, counts = np.full((n, 17, 8), 7, F32), np.full(n, 77, np.uint32)
    lib, h = gpu_ctx.lib, gpu_ctx._h
    ALL, ANY = api.QUERY_COUNT_ALL, api.CONTACT_ANY

    def call(b, k, o, c, flags, m=n):
        return lib.rt_contact_triangle(h, C.c_void_p(b), C.c_size_t(m), C.c_uint32(k), C.c_void_p(o), C.c_void_p(c), C.c_uint32(flags))

    B, O, Cn = tris.ctypes.data, out.ctypes.data, counts.ctypes.data
    assert call(B, 4, O, Cn, 0) == -4, "RT_ERR_NOT_UPLOADED before an upload"
    with pytest.raises(api.RtError) as e:
        gpu_ctx.contact_triangle(tris, 4)
    assert e.value.code == -4
    gpu_ctx.upload_scene(soup)
    gpu_ctx.contact_triangle(tris, 2)
    before = gpu_ctx.stats()
    assert call(B, 17, O, Cn, 0) == -1                                    # max_contacts > RT_CONTACT_MAX
    assert call(B, 0, O, Cn, 0) == -1                                     # max_contacts == 0 without RT_QUERY_COUNT_ALL or RT_CONTACT_ANY
    assert call(B, 0, O, None, ALL) == -1 and call(B, 0, O, None, ANY) == -1  # ... without counts
    assert call(B, 4, O, Cn, ANY) == -1 and call(B, 0, O, Cn, ANY | ALL) == -1  # RT_CONTACT_ANY lists nothing and counts to one
    assert call(None, 4, O, Cn, 0) == -1 and call(B, 4, None, Cn, 0) == -1
    assert call(B, 4, O, Cn, 8) == -1 and call(B, 4, O, Cn, 0x80000000) == -1, "unknown flag bits"
    assert (out == 7).all() and (counts == 77).all()
    assert gpu_ctx.stats()["rays"] == before["rays"] == n
    assert call(None, 4, None, None, 0, m=0) == 0, "n == 0 is RT_OK"
    assert call(B, 4, O, None, 0) == 0, "counts may be NULL with max_contacts > 0"
    _same(out.reshape(-1)[:n * 4 * 8].reshape(n, 4, 8), kt.first_k(*soup_want, 4)[0][:n])
    assert (out.reshape(-1)[n * 4 * 8:] == 7).all()
    empty = gpu_ctx.contact_triangle(np.zeros((0, 12), F32), 4)
    assert empty[0].shape == (0, 4, 8) and empty[1].shape == (0,)
    if torch is None:
        pytest.skip("torch is not installed: mixed memory kinds not exercised")
    dev = torch.from_numpy(tris).to("cuda:0")
    dout, dcounts = torch.full((n, 4, 8), 7.0, dtype=torch.float32, device="cuda:0"), torch.full((n,), 77, dtype=torch.int32, device="cuda:0")
    assert call(dev.data_ptr(), 4, O, Cn, 0) == -1 and call(B, 4, dout.data_ptr(), Cn, 0) == -1 and call(dev.data_ptr(), 4, dout.data_ptr(), Cn, 0) == -1
    assert call(B, 4, O, dcounts.data_ptr(), 0) == -1, "mixed host and device buffers"
    assert (dout == 7).all() and (dcounts == 77).all()
    buf = torch.zeros(n * 12 + 1, device="cuda:0")  # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    with pytest.raises(api.RtError) as e:
        gpu_ctx.contact_triangle(buf[1:].view(-1, 12), 4)
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.contact_triangle(dev, 4)[0].cpu().numpy(), kt.first_k(*soup_want, 4)[0][:n])


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_side_effects_an_empty_scene_and_spheres_alone(gpu_ctx, soup, soup_tris, soup_want):
    want, want_counts = kt.first_k(*soup_want, 4)
    gpu_ctx.upload_scene(soup)
    # the last frame and a running accumulation are left alone
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    out, counts = gpu_ctx.contact_triangle(soup_tris, 4)
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
    for k in (1, 16):
        out, counts = gpu_ctx.contact_triangle(soup_tris, k, count_all=True)
        _same(out, _misses(soup_tris, k))
        _same_counts(counts, np.zeros(len(soup_tris)))
    _same_counts(gpu_ctx.contact_triangle(soup_tris, 0, any_hit=True)[1], np.zeros(len(soup_tris)))
    # spheres alone: no tree to walk; wider margins, so that the three spheres are met from outside, across and from inside
    balls = dataclasses.replace(soup, vertices=soup.vertices[:0], triangles=soup.triangles[:0])
    assert len(balls.triangles) == 0 and len(balls.spheres) == 3
    wide = np.array(soup_tris)
    wide[:, 3] *= 4
    wide[::5, 4:7] = wide[::5, 0:3]  # every fifth a segment given as v1 == v0
    recs, _, total = kt.contacts_all(balls, wide, 4)
    prim = np.ascontiguousarray(recs[..., 6]).view(np.uint32)
    assert (total > 0).sum() > 50 and (prim[total > 0, 0] >= cc.SPHERE_FLAG).all() and (recs[..., 3][total > 0, 0] == 0).any()
    gpu_ctx.upload_scene(balls)
    out, counts = gpu_ctx.contact_triangle(wide, 4, count_all=True)
    _same(out, recs)
    _same_counts(counts, total)
    _same_counts(gpu_ctx.contact_triangle(wide, 0, any_hit=True)[1], total > 0)


def test_a_context_over_one_device_twice_gives_the_same_bytes(soup, soup_tris, soup_want):
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(soup)
        out, counts = ctx.contact_triangle(soup_tris, 16)
        _same(out, soup_want[0])
        _same_counts(counts, np.minimum(soup_want[1], 16))
        _, total = ctx.contact_triangle(soup_tris, 0, count_all=True, counters=True)
        _same_counts(total, soup_want[1])
        assert ctx.stats()["rays"] == len(soup_tris) and ctx.stats()["tri_tests"] > 0


# 13 -----------------------------------------------------------------------------------------------------------------------
def test_the_walk_culls(gpu_ctx, soup):
    """A walk that skips nothing passes every equality above.  1024 small triangles near surfaces (edges of about 0.1, margin 0.03),
    counting every contact: the brute force makes 3000 triangle tests per query, and the bound is a tenth of that."""
    tris = kt.small_triangles(soup, 1024, 31)
    gpu_ctx.upload_scene(soup)
    _, counts = gpu_ctx.contact_triangle(tris, 0, count_all=True, counters=True)
    st = gpu_ctx.stats()
    n, n_tris = len(tris), len(soup.triangles)
    print(f"soup, {n} small triangles near surfaces, count only: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} triangle tests per "
          f"query (brute force: {n_tris}); {np.asarray(counts).mean():.2f} contacts per query")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * n_tris / 10
    _same_counts(counts, kt.contacts_all(soup, tris, 1)[2])
