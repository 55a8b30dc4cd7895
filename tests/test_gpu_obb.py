"""Oriented boxes on the MI355X (rt_overlap_obb, rt_sweep_obb).  Every comparison with the float32 statement (obb_cases.py's numpy brute
force over all triangles and spheres) is byte for byte: the trees only cull, in world space, so the answer is the statement's whatever
tree, memory, batch size or device count is in use.  The identity, start-in-contact and contact-time tests hold the two calls to each
other and to rt_overlap_box / rt_sweep_box, which a kernel that is self-consistent but wrong would not pass."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import obb_cases as ob
import overlap_cases as oc
import sweep_box_cases as sb
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first; these tests need it

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


def _same(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _miss_records(tmax):
    rec = np.zeros(len(tmax), T.BOX_SWEEP_HIT)
    rec["t"] = tmax
    rec["axis"] = ob.AXIS_NONE
    rec["prim_id"] = ob.PRIM_MISS
    return rec.view(F32).reshape(-1, 8)


def _boxes(sweeps):
    return np.ascontiguousarray(sweeps[:, 0:12])


@pytest.fixture(scope="module")
def soup():
    return scenes.random_soup(3000, n_spheres=3)


@pytest.fixture(scope="module")
def soup_sweeps(soup):
    """4000 sweeps of the five kinds and 288 at the spheres (tmax = inf); every eighth rotation the exact identity, every
    eighth within 1e-3 rad of it, the others uniform and of lengths 0.5 .. 2."""
    sweeps = np.concatenate([ob.five_kinds(soup, 4000, 11), ob.sphere_directed(soup, 288, 21)])
    sweeps.setflags(write=False)
    return sweeps


@pytest.fixture(scope="module")
def soup_want(soup, soup_sweeps):
    """The sweep statement's answers, computed once (the prefiltered brute force, which test_obb_abi.py holds to the plain one)."""
    rec = ob.brute_force(soup, soup_sweeps, prefilter=True)
    rec.setflags(write=False)
    return rec


@pytest.fixture(scope="module")
def soup_touch(soup, soup_sweeps):
    """The overlap statement for the start poses, computed once: (N, 3 + 3000) bool in key order."""
    touch = ob.touching(soup, _boxes(soup_sweeps))
    touch.setflags(write=False)
    return touch


@pytest.fixture(scope="module")
def sponza():
    return scenes.sponza_like()


@pytest.fixture(scope="module")
def sponza_sweeps(sponza):
    return ob.with_rotation(np.concatenate([sb.toward_surfaces(sponza, 1024, 3), sb.scattered(sponza, 1024, 4)]), ob.rotations(2048, 5))


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_soup_sweeps_equal_the_statement_from_host_device_and_preallocated_memory(gpu_ctx, soup, soup_sweeps, soup_want):
    box_face, tri_face, edge_edge, sphere, at_start, miss = sb.contact_kinds(soup_want)
    print("soup:", {k: int(v.sum()) for k, v in dict(box_face=box_face, tri_face=tri_face, edge_edge=edge_edge, sphere=sphere, at_start=at_start,
                                                     miss=miss).items()})
    assert box_face.sum() >= 100 and tri_face.sum() >= 100 and edge_edge.sum() >= 100 and at_start.sum() >= 100 and miss.sum() >= 100
    assert sphere.sum() >= 20
    gpu_ctx.upload_scene(soup)
    _same(gpu_ctx.sweep_obb(soup_sweeps), soup_want)
    st = gpu_ctx.stats()
    assert st["rays"] == len(soup_sweeps) and st["pixels"] == 0 and st["primary_rays"] == 0 and st["node_visits"] == 0 and st["kernel_ms"] > 0
    own = np.full((len(soup_sweeps), 8), 7.0, F32)
    assert gpu_ctx.sweep_obb(soup_sweeps, out=own) is own
    _same(own, soup_want)
    dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
    got = gpu_ctx.sweep_obb(dev)
    assert got.device == dev.device and got.dtype == torch.float32
    _same(got.cpu().numpy(), soup_want)
    out = torch.empty((len(soup_sweeps), 8), device="cuda:0")
    assert gpu_ctx.sweep_obb(dev, out=out) is out
    _same(out.cpu().numpy(), soup_want)
    # a device tensor 4 bytes off 16-byte alignment is refused, and the context keeps working
    buf = torch.zeros(len(soup_sweeps) * 16 + 1, device="cuda:0")
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_obb(buf[1:].view(-1, 16))
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.sweep_obb(dev).cpu().numpy(), soup_want)


def test_soup_overlaps_equal_the_statement_in_every_mode(gpu_ctx, soup, soup_sweeps, soup_touch):
    """The start poses of the soup's sweeps as boxes: the list at K = 32 and K = 4, COUNT_ALL at K = 0, 4 and 32, and ANY; from host
    and device memory and into preallocated outputs."""
    boxes = _boxes(soup_sweeps)
    ids, listed, total = ob.overlap_all(soup, boxes, touch=soup_touch)
    print(f"soup: {int((total > 0).sum())} of {len(boxes)} boxes touch something, {int((total > 4).sum())} more than 4, {int((total > 32).sum())} more than 32, "
          f"{int(soup_touch[:, :3].any(1).sum())} a sphere")
    assert (total > 0).sum() >= 500 and (total == 0).sum() >= 500 and (total > 4).sum() >= 100 and soup_touch[:, :3].any(1).sum() >= 10
    gpu_ctx.upload_scene(soup)
    # lists that overflow K = 32: 64 of the boxes with every half extent 0.15 diagonals
    big = api.make_obbs(boxes[::61][:64, 0:3], F32(0.15 * ob.diagonal(soup)), boxes[::61][:64, 8:12])
    big_ids, big_listed, big_total = ob.overlap_all(soup, big)
    assert (big_total > 32).sum() >= 32
    got_ids, got_counts = gpu_ctx.overlap_obb(big, 32)
    _same(got_ids, big_ids), _same(got_counts, big_listed)
    _same(gpu_ctx.overlap_obb(big, 32, count_all=True)[1], big_total)
    got_ids, got_counts = gpu_ctx.overlap_obb(boxes, 32)
    _same(got_ids, ids), _same(got_counts, listed)
    ids4, listed4 = oc.first_k(ids, total, 4)
    got_ids, got_counts = gpu_ctx.overlap_obb(boxes, 4)
    _same(got_ids, ids4), _same(got_counts, listed4)
    for k, want_ids in ((4, ids4), (32, ids)):
        got_ids, got_counts = gpu_ctx.overlap_obb(boxes, k, count_all=True)
        _same(got_ids, want_ids), _same(got_counts, total)
    none, got_counts = gpu_ctx.overlap_obb(boxes, 0, count_all=True)
    assert none is None
    _same(got_counts, total)
    _same(gpu_ctx.overlap_obb(boxes, 0, any_hit=True)[1], (total > 0).astype(np.uint32))
    st = gpu_ctx.stats()
    assert st["rays"] == len(boxes) and st["node_visits"] == 0 and st["kernel_ms"] > 0
    dev = torch.from_numpy(boxes).to("cuda:0") * 1.0
    got_ids, got_counts = gpu_ctx.overlap_obb(dev, 32, count_all=True)
    assert got_ids.device == dev.device and got_ids.dtype == torch.int32 and got_counts.dtype == torch.int32
    _same(got_ids.cpu().numpy().view(np.uint32), ids), _same(got_counts.cpu().numpy().view(np.uint32), total)
    out, counts = torch.empty((len(boxes), 4), dtype=torch.int32, device="cuda:0"), torch.empty(len(boxes), dtype=torch.int32, device="cuda:0")
    got = gpu_ctx.overlap_obb(dev, 4, out=out, counts=counts)
    assert got[0] is out and got[1] is counts
    _same(out.cpu().numpy().view(np.uint32), ids4), _same(counts.cpu().numpy().view(np.uint32), listed4)
    buf = torch.zeros(len(boxes) * 12 + 1, device="cuda:0")
    with pytest.raises(api.RtError) as e:
        gpu_ctx.overlap_obb(buf[1:].view(-1, 12), 4)
    assert e.value.code == -1 and "aligned" in str(e.value)
    _same(gpu_ctx.overlap_obb(dev, 0, any_hit=True)[1].cpu().numpy().view(np.uint32), (total > 0).astype(np.uint32))


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_identity_rotations_give_the_axis_aligned_calls_bytes(gpu_ctx, soup, soup_sweeps):
    """rotation = (0, 0, 0, 1), (0, 0, 0, -3) and (-0, 0, -0, 2) in turn: R is the identity (in the third case with some -0 off the
    diagonal), so sweep_obb and overlap_obb return what sweep_box and overlap_box return for the same boxes, in the same context."""
    box_sweeps = ob.as_box_sweeps(soup_sweeps)
    rot = np.array([[0, 0, 0, 1], [0, 0, 0, -3], [-0.0, 0, -0.0, 2]], F32)[np.arange(len(box_sweeps)) % 3]
    sweeps = ob.with_rotation(box_sweeps, rot)
    gpu_ctx.upload_scene(soup)
    aligned = gpu_ctx.sweep_box(box_sweeps)
    _same(gpu_ctx.sweep_obb(sweeps), aligned)
    kinds = sb.contact_kinds(aligned)
    assert all(k.sum() >= 20 for k in kinds), [int(k.sum()) for k in kinds]
    boxes = np.ascontiguousarray(box_sweeps[:, 0:8])
    for kwargs in (dict(max_prims=32), dict(max_prims=4, count_all=True), dict(max_prims=0, any_hit=True)):
        want_ids, want_counts = gpu_ctx.overlap_box(boxes, **kwargs)
        got_ids, got_counts = gpu_ctx.overlap_obb(_boxes(sweeps), **kwargs)
        _same(got_counts, want_counts)
        if want_ids is not None:
            _same(got_ids, want_ids)
    assert want_counts.sum() >= 500


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_boundaries(gpu_ctx, soup, soup_sweeps, soup_want, soup_touch, n):
    gpu_ctx.upload_scene(soup)
    pick = np.arange(n) * 61 % len(soup_sweeps)  # of every kind
    sweeps = np.ascontiguousarray(soup_sweeps[pick])
    _same(gpu_ctx.sweep_obb(sweeps), soup_want[pick])
    ids, listed, total = ob.overlap_all(soup, _boxes(sweeps), 4, touch=soup_touch[pick])
    got_ids, got_counts = gpu_ctx.overlap_obb(_boxes(sweeps), 4, count_all=True)
    _same(got_ids, ids), _same(got_counts, total)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_exact_ties_resolve_to_the_lower_index(gpu_ctx, soup, soup_sweeps, soup_want, soup_touch):
    """The soup's triangle array concatenated with itself: every candidate ties bit for bit with its copy 3000 indices on, so every
    sweep's answer is the single soup's, and every box lists each touching triangle and then, K permitting, its copy."""
    doubled = dataclasses.replace(soup, triangles=np.concatenate([soup.triangles, soup.triangles]))
    prim = api.split_box_sweep_hits(soup_want)[3]
    assert ((prim < 3000) | (prim >= ob.SPHERE_FLAG)).all() and (prim < 3000).sum() > 2500
    gpu_ctx.upload_scene(doubled)
    _same(gpu_ctx.sweep_obb(soup_sweeps), soup_want)
    touch2 = np.concatenate([soup_touch, soup_touch[:, 3:]], 1)
    ids, listed, total = ob.overlap_all(doubled, _boxes(soup_sweeps), 4, touch=touch2)
    got_ids, got_counts = gpu_ctx.overlap_obb(_boxes(soup_sweeps), 4, count_all=True)
    _same(got_ids, ids), _same(got_counts, total)
    _same(total, (soup_touch[:, :3].sum(1) + 2 * soup_touch[:, 3:].sum(1)).astype(np.uint32))


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_tmax_is_strict_on_both_sides(gpu_ctx, soup, soup_sweeps, soup_want):
    """From each sweep's answer at tmax = inf: nextafter(t, +inf) as tmax gives the same bytes - for a start in contact that is the
    smallest positive tmax - and t itself as tmax gives the miss record carrying that tmax."""
    gpu_ctx.upload_scene(soup)
    first = gpu_ctx.sweep_obb(soup_sweeps)
    _same(first, soup_want)
    assert (soup_sweeps[:, 15] == INF).all()
    t = first[:, 3].copy()
    hit = api.split_box_sweep_hits(first)[3] != ob.PRIM_MISS
    assert (hit & (t == 0)).sum() >= 100 and (hit & (t > 0)).sum() >= 1000 and (~hit).sum() >= 100
    q = np.array(soup_sweeps)
    q[:, 15] = np.nextafter(t, INF)
    assert (q[hit & (t == 0), 15] == F32(1.4e-45)).all()
    _same(gpu_ctx.sweep_obb(q), first)
    q[:, 15] = t
    _same(gpu_ctx.sweep_obb(q), _miss_records(t))


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_queries_are_misses_and_empty_lists_without_a_walk(gpu_ctx, soup):
    gpu_ctx.upload_scene(soup)
    nan = F32(np.nan)
    c, h, r, d = [0, 0, 1], [0.1, 0.05, 0.2], [0.1, 0.2, 0.3, 0.9], [0, 0, -1]

    def q_(c=c, h=h, r=r, d=d, tmax=INF):
        return [*c, 0, *h, 0, *r, *d, tmax]

    box_bad = [q_(c=[nan, 0, 1]), q_(c=[0, nan, 1], tmax=1), q_(c=[0, 0, INF]), q_(c=[0, -INF, 1], tmax=2),
               q_(h=[nan, 0.1, 0.1]), q_(h=[0.1, INF, 0.1]), q_(h=[0.1, 0.1, -INF]), q_(h=[-0.1, 0.1, 0.1]), q_(h=[0.1, 0.1, -1e-30]),
               q_(r=[nan, 0, 0, 1]), q_(r=[0, nan, 0, 1], tmax=4), q_(r=[0, 0, nan, 1]), q_(r=[0, 0, 0, nan]), q_(r=[INF, 0, 0, 1]), q_(r=[0, 0, 0, -INF]),
               q_(r=[0, 0, 0, 0]), q_(r=[0, -0.0, 0, 0], tmax=6),
               q_(r=[0, 0, 2e19, 2e19]),       # n overflows
               q_(r=[1e-30, 0, 0, 1e-30])]     # n underflows to 0
    sweep_bad = [q_(d=[nan, 0, -1]), q_(d=[0, INF, -1]), q_(d=[0, 0, -INF], tmax=3), q_(d=[0, 0, 0]), q_(d=[-0.0, 0, -0.0], tmax=5),
                 q_(tmax=nan), q_(tmax=0.0), q_(tmax=-0.0), q_(tmax=-1.0), q_(tmax=-INF)]
    q = np.array(box_bad + sweep_bad, F32)
    assert not ob.valid(q).any() and not ob.valid_boxes(q[:len(box_bad)]).any() and ob.valid_boxes(q[len(box_bad):]).all()
    got = gpu_ctx.sweep_obb(q, counters=True)
    _same(got, _miss_records(q[:, 15]))
    st = gpu_ctx.stats()
    assert st["node_visits"] == 0 and st["tri_tests"] == 0 and st["rays"] == len(q)
    _same(got, ob.brute_force(soup, q))
    boxes = _boxes(q[:len(box_bad)])
    ids, counts = gpu_ctx.overlap_obb(boxes, 4, count_all=True, counters=True)
    assert (ids == ob.PRIM_MISS).all() and not counts.any()
    assert gpu_ctx.stats()["node_visits"] == 0 and gpu_ctx.stats()["tri_tests"] == 0
    assert not gpu_ctx.overlap_obb(boxes, 0, any_hit=True, counters=True)[1].any() and gpu_ctx.stats()["node_visits"] == 0
    # the same centre with a valid query walks; zero extents are valid, and so is a tiny quaternion whose n does not underflow
    on = soup.vertices["position"][soup.triangles["v0_index"][:3]].astype(F32)
    good = np.array([q_(), q_(h=[0, 0, 0]), q_(h=[-0.0, 0.1, 0.0]), q_(r=[0, 0, 1e-10, 1e-10]), q_(c=on[0], r=[0, 0, 1e-10, 1e-10]),
                     q_(c=on[1], r=[3e-12, 0, 1e-10, -2e-11]), q_(c=on[2], h=[0.3, 0.2, 0.4], r=[0, 0, 1e-10, 1e-10]),
                     q_(h=[3e38, 3e38, 3e38]), q_(h=[3e38, 1.0, 0.0])], F32)  # the world box's half extents overflow: every node is followed
    assert ob.valid(good).all()
    want = ob.brute_force(soup, good)
    assert (want[3:, 3] == 0).sum() >= 3, "the boxes on vertices start in contact"
    _same(gpu_ctx.sweep_obb(good, counters=True), want)
    assert gpu_ctx.stats()["node_visits"] >= len(good)
    ids, listed, total = ob.overlap_all(soup, _boxes(good), 4)
    got_ids, got_counts = gpu_ctx.overlap_obb(_boxes(good), 4, count_all=True, counters=True)
    _same(got_ids, ids), _same(got_counts, total)
    assert total[4:7].all() and gpu_ctx.stats()["node_visits"] >= len(good)


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_a_start_in_contact_is_the_overlap_of_the_start_pose(gpu_ctx, soup, soup_sweeps):
    """Exactly, with no eps: a sweep that answers (t = 0, NONE) with a triangle has that triangle in overlap_obb's list for the start
    pose - it is the lowest touching triangle, so with the three spheres ahead of it K = 4 always holds it - and a sweep whose start
    pose overlap_obb(ANY) reports empty answers t > 0 or a miss."""
    gpu_ctx.upload_scene(soup)
    _, t, axis, prim, _ = api.split_box_sweep_hits(gpu_ctx.sweep_obb(soup_sweeps))
    ids, _ = gpu_ctx.overlap_obb(_boxes(soup_sweeps), 4)
    occupied = gpu_ctx.overlap_obb(_boxes(soup_sweeps), 0, any_hit=True)[1].astype(bool)
    at_start = (t == 0) & (axis == ob.AXIS_NONE) & (prim < ob.SPHERE_FLAG)
    assert at_start.sum() >= 500 and (~occupied).sum() >= 1000
    assert (ids[at_start] == prim[at_start, None]).any(1).all()
    free = ~occupied
    assert ((prim[free] == ob.PRIM_MISS) | (t[free] > 0)).all()
    assert occupied[(t == 0) & (prim != ob.PRIM_MISS)].all(), "and every start in contact is an occupied pose"


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_overlap_obb_agrees_at_the_time_of_contact(gpu_ctx, soup, soup_sweeps, soup_want):
    """Over every hit with t > 0 and all extents >= 1e-3 x the diagonal, none left out: rt_overlap_obb(RT_OVERLAP_ANY) is 1 for the box
    at center + direction * t grown by eps on every axis, and 0 for the box shrunk by eps at 50, 90 and 99.9 % of t.  eps = 2
    K_MEASURED x the diagonal + 2^-20 x (the largest |centre| component + |direction| t), test_gpu_sweep_box.py's form."""
    gpu_ctx.upload_scene(soup)
    got = gpu_ctx.sweep_obb(soup_sweeps)
    _same(got, soup_want)
    _, t, _, prim, _ = api.split_box_sweep_hits(got)
    c, h, rot, d = soup_sweeps[:, 0:3], soup_sweeps[:, 4:7], soup_sweeps[:, 8:12], soup_sweeps[:, 12:15]
    pick = (prim != ob.PRIM_MISS) & (t > 0) & ob.full_extents(soup, soup_sweeps)
    c, h, rot, d, t = c[pick].astype(np.float64), h[pick].astype(np.float64), rot[pick], d[pick].astype(np.float64), t[pick].astype(np.float64)
    eps = 2 * ob.K_MEASURED["soup"] * ob.diagonal(soup) + 2.0 ** -20 * (np.abs(c).max(1) + np.linalg.norm(d, axis=1) * t)
    assert (eps[:, None] < h).all()

    def any_touch(part, grow):
        boxes = api.make_obbs((c + d * (t * part)[:, None]).astype(F32), (h + (eps * grow)[:, None]).astype(F32), rot)
        return gpu_ctx.overlap_obb(boxes, 0, any_hit=True)[1].astype(bool)

    need = np.full(len(t), np.inf)
    for grow in np.arange(8, -1, -1) / 8.0:
        need = np.where(any_touch(np.ones(len(t)), np.full(len(t), grow)), grow, need)
    print(f"{pick.sum()} contacts with t > 0: the box at the contact needs at most {need.max():.3g} eps to touch (eps up to {eps.max():.3g})")
    assert pick.sum() >= 1500
    assert (need <= 1.0).all(), "grown by eps the box touches at the time of contact"
    for part in (0.5, 0.9, 0.999):
        early = any_touch(np.full(len(t), part), np.full(len(t), -1.0))
        assert not early.any(), (part, int(early.sum()))


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_sponza_answers_do_not_depend_on_the_tree(gpu_ctx, sponza, sponza_sweeps):
    """The device-built tree and the host builder's quality tree give the same bytes, for both calls; 256 of the queries (toward
    surfaces and scattered) are held to the statement."""
    boxes = _boxes(sponza_sweeps)
    gpu_ctx.upload_scene(sponza)
    device_tree = gpu_ctx.sweep_obb(sponza_sweeps)
    device_ids, device_counts = gpu_ctx.overlap_obb(boxes, 8, count_all=True)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    _same(gpu_ctx.sweep_obb(sponza_sweeps), device_tree)
    ids, counts = gpu_ctx.overlap_obb(boxes, 8, count_all=True)
    _same(ids, device_ids), _same(counts, device_counts)
    pick = np.arange(0, len(sponza_sweeps), 8)
    assert len(pick) == 256
    _same(device_tree[pick], ob.brute_force(sponza, sponza_sweeps[pick], prefilter=True))
    want_ids, _, want_total = ob.overlap_all(sponza, boxes[pick], 8, touch=ob.touching(sponza, boxes[pick], prefilter=True))
    _same(device_ids[pick], want_ids), _same(device_counts[pick], want_total)
    prim = api.split_box_sweep_hits(device_tree)[3]
    assert (prim[:1024] != ob.PRIM_MISS).all(), "a sweep aimed at a point of the surface touches something, that point at the latest"
    assert (prim[1024:] != ob.PRIM_MISS).any() and (prim[1024:] == ob.PRIM_MISS).any() and device_counts.any() and not device_counts.all()


def test_sponza_refit_answers_are_a_fresh_uploads(gpu_ctx, sponza, sponza_sweeps):
    """After rt_update_geometry (a refit of the quality tree, seeded displacement) the answers are those of a fresh upload of the
    moved scene, and not those of the scene before."""
    pos = np.ascontiguousarray(sponza.vertices["position"], F32)
    moved_pos = (pos.astype(np.float64) + np.random.default_rng(17).normal(0.0, 0.02, pos.shape)).astype(F32)
    v = sponza.vertices.copy()
    v["position"] = moved_pos
    moved = dataclasses.replace(sponza, vertices=v)
    boxes = _boxes(sponza_sweeps)
    gpu_ctx.upload_scene(sponza)
    before = gpu_ctx.sweep_obb(sponza_sweeps)
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.update_geometry(moved_pos)["flags"] == api.STAT_REFIT
    refitted = gpu_ctx.sweep_obb(sponza_sweeps)
    ids, counts = gpu_ctx.overlap_obb(boxes, 8, count_all=True)
    with api.Context() as fresh:
        fresh.upload_scene(moved)
        _same(refitted, fresh.sweep_obb(sponza_sweeps))
        fresh_ids, fresh_counts = fresh.overlap_obb(boxes, 8, count_all=True)
        _same(ids, fresh_ids), _same(counts, fresh_counts)
    assert (refitted.view(np.uint32) != before.view(np.uint32)).any(1).mean() > 0.5


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_the_walks_cull(gpu_ctx, soup):
    """A walk that skips nothing passes every equality above: against the brute force's n x n_tris triangle tests each walk makes
    fewer than a tenth."""
    sweeps = ob.with_rotation(sb.toward_surfaces(soup, 2048, 31), ob.rotations(2048, 32))
    gpu_ctx.upload_scene(soup)
    n, n_tris = len(sweeps), len(soup.triangles)
    gpu_ctx.sweep_obb(sweeps, counters=True)
    st = gpu_ctx.stats()
    print(f"soup, {n} sweeps toward surfaces: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} triangle tests per sweep "
          f"(brute force: {n_tris})")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * n_tris / 10
    gpu_ctx.overlap_obb(_boxes(sweeps), 0, count_all=True, counters=True)
    st = gpu_ctx.stats()
    print(f"soup, {n} boxes: {st['node_visits'] / n:.1f} node visits and {st['tri_tests'] / n:.1f} triangle tests per box")
    assert st["node_visits"] > 0 and 0 < st["tri_tests"] < n * n_tris / 10


# 11 -----------------------------------------------------------------------------------------------------------------------
def test_side_effects_empty_scene_and_call_order(gpu_ctx, soup, soup_sweeps, soup_want, soup_touch):
    boxes = _boxes(soup_sweeps)
    total = soup_touch.sum(1).astype(np.uint32)
    with pytest.raises(api.RtError) as e:
        gpu_ctx.sweep_obb(soup_sweeps)
    assert e.value.code == -4, "RT_ERR_NOT_UPLOADED before an upload"
    with pytest.raises(api.RtError) as e:
        gpu_ctx.overlap_obb(boxes, 4)
    assert e.value.code == -4
    gpu_ctx.upload_scene(soup)
    assert gpu_ctx.sweep_obb(np.zeros((0, 16), F32)).shape == (0, 8)
    lib, one, out, cnt = gpu_ctx.lib, np.zeros((1, 16), F32), np.zeros((1, 8), F32), np.zeros(1, np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.rt_sweep_obb(gpu_ctx._h, None, C.c_size_t(1), p(out), C.c_uint32(0)) == -1
    assert lib.rt_sweep_obb(gpu_ctx._h, p(one), C.c_size_t(1), None, C.c_uint32(0)) == -1
    assert lib.rt_sweep_obb(gpu_ctx._h, p(one), C.c_size_t(1), p(out), C.c_uint32(2)) == -1, "unknown flag"
    assert lib.rt_sweep_obb(gpu_ctx._h, None, C.c_size_t(0), None, C.c_uint32(0)) == 0
    assert lib.rt_overlap_obb(gpu_ctx._h, None, C.c_size_t(1), C.c_uint32(4), p(out), p(cnt), C.c_uint32(0)) == -1
    assert lib.rt_overlap_obb(gpu_ctx._h, p(one), C.c_size_t(1), C.c_uint32(4), None, p(cnt), C.c_uint32(0)) == -1
    assert lib.rt_overlap_obb(gpu_ctx._h, p(one), C.c_size_t(1), C.c_uint32(33), p(out), p(cnt), C.c_uint32(0)) == -1, "max_prims > RT_OVERLAP_MAX"
    assert lib.rt_overlap_obb(gpu_ctx._h, p(one), C.c_size_t(1), C.c_uint32(0), None, p(cnt), C.c_uint32(0)) == -1, "max_prims 0 without a mode"
    assert lib.rt_overlap_obb(gpu_ctx._h, p(one), C.c_size_t(1), C.c_uint32(4), p(out), p(cnt), C.c_uint32(4)) == -1, "ANY with max_prims > 0"
    assert lib.rt_overlap_obb(gpu_ctx._h, p(one), C.c_size_t(1), C.c_uint32(4), p(out), p(cnt), C.c_uint32(8)) == -1, "unknown flag"
    assert lib.rt_overlap_obb(gpu_ctx._h, None, C.c_size_t(0), C.c_uint32(4), None, None, C.c_uint32(0)) == 0
    assert not out.any() and not cnt.any()
    # the last frame and a running accumulation are left alone
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    _same(gpu_ctx.sweep_obb(soup_sweeps), soup_want)
    _same(gpu_ctx.overlap_obb(boxes, 0, count_all=True)[1], total)
    _same(gpu_ctx.read_rgb32f(), rgb)
    assert gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(96, 64, soup.camera, mode=2, spp=2, max_bounces=2, frame_seed=3, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4, "the running image went on"
    # an empty scene: all misses, nothing touched
    gpu_ctx.upload_scene(scenes.empty_scene())
    _same(gpu_ctx.sweep_obb(soup_sweeps), _miss_records(soup_sweeps[:, 15]))
    ids, counts = gpu_ctx.overlap_obb(boxes, 4, count_all=True)
    assert (ids == ob.PRIM_MISS).all() and not counts.any()


# 12 -----------------------------------------------------------------------------------------------------------------------
def test_a_context_over_one_device_twice_gives_the_same_bytes(soup, soup_sweeps, soup_want, soup_touch):
    with api.Context((0, 0)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_obb(soup_sweeps), soup_want)
        ctx.sweep_obb(soup_sweeps, counters=True)
        assert ctx.stats()["rays"] == len(soup_sweeps) and ctx.stats()["tri_tests"] > 0
        _same(ctx.overlap_obb(_boxes(soup_sweeps), 0, count_all=True, counters=True)[1], soup_touch.sum(1).astype(np.uint32))
        assert ctx.stats()["rays"] == len(soup_sweeps) and ctx.stats()["tri_tests"] > 0


def test_two_devices_give_the_one_device_bytes(soup, soup_sweeps, soup_want, soup_touch):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    with api.Context((0, 1)) as ctx:
        ctx.upload_scene(soup)
        _same(ctx.sweep_obb(soup_sweeps), soup_want)
        dev = torch.from_numpy(np.array(soup_sweeps)).to("cuda:1")
        _same(ctx.sweep_obb(dev).cpu().numpy(), soup_want)
        _same(ctx.overlap_obb(_boxes(soup_sweeps), 0, count_all=True)[1], soup_touch.sum(1).astype(np.uint32))
