"""The cases of beam_edge_cases.py say what they aim at; this module checks, in float64 and without the library, that they do: the
margins and totals under which the cap and fallback families' list lengths are exact, what the order family's lists look like, how
often every border sliver is hit from each side, how much of its region every pyramid case sees - and that a builder broken on purpose
fails its statement.  test_gpu_beam_edges.py means something only while these hold."""
import dataclasses

import numpy as np
import pytest

import beam_edge_cases as ec


def _assert_materials(case, neighbours=True):
    """At least 64 materials exist, neighbours in index differ, and so do neighbours in space (the nearest other triangle on the screen
    that is not the same triangle twice)."""
    assert len(ec.materials()) >= 64 and case.mats.min() >= 0 and case.mats.max() < ec.MATERIALS
    assert (np.diff(case.mats) != 0).all(), case.name
    if not neighbours:
        return
    near = ec.nearest_on_screen(case)
    assert (case.mats[near] != case.mats).all(), case.name


# cap ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.CAP_NS)
def test_cap_lists_are_exact(n):
    case = ec.cap(n)
    want = ec.expected_lists(case)  # (asserts the margins of one pixel, the flat triangles and the backdrop's cover)
    assert len(want) == 9 and len(case.tris) == n + 2 < ec.LEAVES  # every leaf holds a triangle: fewer leaves than RT_BEAM_LEAVES in all
    assert want == [2] * 4 + [n + 2 if n + 2 <= ec.CAP else ec.NO_LIST] + [2] * 4
    assert (want[4] is ec.NO_LIST) == (n >= 127)
    lo, hi = ec.screen_boxes(case, slice(2, None))
    assert (hi - lo).max() < 0.2 and lo.min() >= 10.0 and hi.max() <= 14.0  # the inner 4x4 pixels of block (8, 8)
    _, _, depth = ec.project(case.camera, case.w, case.h, case.tris[2:, 0])
    assert 2.0 - 1e-6 <= depth.min() and depth.max() <= 6.0 + 1e-6
    if n > 8:
        assert abs(np.corrcoef(np.arange(n), depth)[0, 1]) < 0.3  # index order is shuffled against depth
    _assert_materials(case)
    win, _ = ec.first_hits(case)
    assert (win >= 0).all() and (win >= 2).sum() >= (8 if n >= 63 else 1)  # the backdrop fills the frame; pixel centres see the pile


def test_a_broken_cap_case_fails_its_statement():
    case = ec.cap(126)
    bad = case.tris.copy()
    bad[5] = ec.back_project(case.camera, 24, 24, np.array([15.95, 16.1, 15.95]), np.array([12.0, 12.0, 12.15]), np.full(3, 3.0))  # across the border x = 16
    with pytest.raises(AssertionError):
        want = ec.expected_lists(dataclasses.replace(case, tris=bad))
        assert want[4] == 128
    tilted = case.tris.copy()
    tilted[7, 0, 2] -= np.float32(0.5)
    with pytest.raises(AssertionError):
        ec.expected_lists(dataclasses.replace(case, tris=tilted))


# fallback -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ec.FALLBACK_PATTERNS)
@pytest.mark.parametrize("frame", list(ec.FALLBACK_FRAMES))
def test_fallback_lists_are_exact(frame, pattern):
    case = ec.fallback(frame, pattern)
    blocks = ec.case_blocks(case)
    want = ec.expected_lists(case)
    over = case.info["over"]
    assert want == [ec.NO_LIST if b in over else ec.SPARSE + 2 for b in range(len(blocks))]
    assert sum(w is ec.NO_LIST for w in want) == len(over) == {"none": 0, "first": 1, "last": 1, "alternate": (len(blocks) + 1) // 2, "every": len(blocks)}[pattern]
    assert len(case.tris) == 2 + len(over) * ec.OVER_FULL + (len(blocks) - len(over)) * ec.SPARSE
    if len(over) < len(blocks):
        assert len(case.tris) <= ec.LEAVES  # a block that has a list cannot have met more leaves than there are triangles
    if frame == "20x12 tile 12":
        assert len(blocks) == 8 and (blocks[:, 2] == 0).sum() == 2 and ((blocks[:, 2] > 0) & (blocks[:, 2] < 8)).sum() >= 2  # blocks without a pixel, blocks cut by the tile edge
        assert int((blocks[:, 2] * blocks[:, 3]).sum()) == 20 * 12
    if frame == "32x16 rank 1 of 3":
        assert [tuple(b[:2]) for b in blocks] == [(8, 0), (0, 8), (24, 8)]
    _assert_materials(case)


def test_fallback_sample_counts_straddle_the_chunk():
    assert ec.CHUNK == 8 and set(ec.FALLBACK_SPP) >= {1, ec.CHUNK - 1, ec.CHUNK, ec.CHUNK + 1, 2 * ec.CHUNK + 1}


def test_block_table_against_the_pixels():
    for w, h, tile, rank, world in ((20, 12, 12, 0, 1), (32, 16, 8, 1, 3), (33, 33, 33, 0, 1), (64, 1080, 1080, 0, 1)):
        t = ec.block_table(w, h, tile, rank, world)
        seen = np.zeros((h, w), int)
        for x0, y0, nx, ny in t:
            seen[y0:y0 + ny, x0:x0 + nx] += 1
        tx = (w + tile - 1) // tile
        owner = (np.arange(h)[:, None] // tile) * tx + np.arange(w)[None, :] // tile
        assert (seen == (owner % world == rank)).all()


# order --------------------------------------------------------------------------------------------------------------------------
def test_order_inside_boxes():
    case = ec.order_inside_boxes()
    tr, o = case.tris.astype(np.float64), np.asarray(case.camera["position"], np.float64)
    assert len(tr) == 40 and ((tr.min(1) < o) & (o < tr.max(1))).all() and (ec.box_distance(case) == 0).all()
    win, _ = ec.first_hits(case)
    assert (win >= 0).all() and len(np.unique(win)) >= 6
    mixed = [len(np.unique(win[:, y0:y0 + 8, x0:x0 + 8])) >= 2 for x0, y0, _, _ in ec.case_blocks(case)]
    assert sum(mixed) >= len(mixed) // 2  # planes cross inside half the blocks and more
    _assert_materials(case, neighbours=False)


def test_order_slanted_first():
    case = ec.order_slanted_first()
    dist = ec.box_distance(case)
    assert len(case.tris) == 31 and dist[0] < 0.99 * dist[1:].min()  # first in every list
    alone = dataclasses.replace(case, tris=case.tris[:1], mats=case.mats[:1])
    w0, t0 = ec.first_hits(alone)
    assert (w0 == 0).all()  # every sample hits it ...
    win, t = ec.first_hits(case)
    small = win > 0
    assert (t[small] < t0[small]).all() and small.mean() > 0.1 and (~small).mean() > 0.3 and len(np.unique(win)) >= 25  # ... behind every small one
    # a bound 0.1 % too large (and the padding's 4e-6 smaller) ends every block's list after entry 0
    assert t0.max() < 1.001 * (1.0 - 2 * ec.BOX_PAD) * dist[1:].min()
    _assert_materials(case, neighbours=False)


def test_order_coincident_pairs():
    case = ec.order_coincident_pairs()
    n = len(case.tris)
    assert n == 40
    for i, j in case.info["pairs"]:
        assert i < j == n - 1 - i and (case.tris[i] == case.tris[j]).all() and case.mats[i] != case.mats[j]
    win, _ = ec.first_hits(case)
    assert win.max() < 20 and len(np.unique(win[win >= 0])) >= 10
    _assert_materials(case, neighbours=False)


@pytest.mark.parametrize("D,gap", ec.ORDER_D)
def test_order_plates(D, gap):
    case = ec.order_plates(D, gap)
    win, t = ec.first_hits(case)
    assert np.isin(win, case.info["near"]).all() and min(case.info["near"]) > max(case.info["far"])
    far_only = dataclasses.replace(case, tris=case.tris[:2], mats=case.mats[:2])
    _, t_far = ec.first_hits(far_only)
    assert (t < t_far).all()
    rel = t_far / t - 1.0
    assert 0.5 * gap < rel.min() and rel.max() < 1.5 * gap  # (f32 vertices: the gap is what the case says, within the rounding of D)
    # the far plate's bound against the nearest hit on the axis: under it for 5e-6 (the far plate is tested), over it for 2e-5
    dist = ec.box_distance(case)
    assert (dist[0] * ec.DIST_SCALE < dist[2]) == (gap < 1e-5)


def test_order_spheres():
    case = ec.order_spheres()
    win, t = ec.first_hits(case)
    assert case.w % 2 == 1 and win[0, 16, 16] == -4 and t[0, 16, 16] == 4.0   # the sphere that touches the plate's plane ...
    plates = dataclasses.replace(case, spheres=())
    w1, t1 = ec.first_hits(plates)
    assert w1[0, 16, 16] in (4, 5) and t1[0, 16, 16] == 4.0                    # ... at exactly the plate's t
    px = lambda c: tuple(int(v) for v in ec.project(case.camera, case.w, case.h, np.array(c))[:2])
    x, y = px(case.spheres[0][0])
    assert win[0, y, x] == -2 and w1[0, y, x] in (0, 1)                         # in front of its plate
    x, y = px(case.spheres[1][0])
    assert win[0, y, x] in (2, 3) and (win == -3).sum() >= 4                   # behind its plate, and seen around it
    for x0, y0, nx, ny in ec.case_blocks(case):
        assert nx * ny > 0


# edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [64, 1])
def test_every_border_sliver_is_hit_from_every_side_it_reaches(spp):
    case = ec.edges(spp)
    n_sl = len(case.info["slivers"])
    assert n_sl == 2 * 5 * len(ec.EDGE_OFFSETS) and len(case.tris) == 2 + 2 * n_sl
    lo, hi = ec.screen_boxes(case, slice(2, None))
    size = np.sort((hi - lo)[::2], axis=1)
    assert np.allclose(size, [ec.SLIVER_W, ec.SLIVER_L], atol=1e-4)
    win, _ = ec.first_hits(case)
    hits = ec.sliver_hits(case, win)
    two_sided = 0
    for sl, sides in zip(case.info["slivers"], hits):
        reached = [s for s, (width, n) in sides.items() if width >= ec.MIN_SIDE_PX]
        assert reached or (sl[1] in (0, case.w) and spp > 1), sl  # (a sliver outside the image's border reaches no pixel: it may only do no harm)
        for s in reached:
            assert sides[s][1] >= 1, (sl, sides)
        two_sided += len(reached) == 2
        if spp == 1:
            assert abs((sl[4] % 1.0) - 0.5) <= 0.03 + 1e-9  # centred on a pixel centre
    if spp > 1:
        assert two_sided == 2 * 3 * 3  # the interior borders' slivers at 0 and +-0.05 straddle their border
    _assert_materials(case, neighbours=False)


def test_a_broken_edge_case_fails_its_statement():
    case = ec.edges(64)
    bad = case.tris.copy()
    first = case.info["slivers"][6][3]
    bad[first:first + 2, :, 2] -= np.float32(9.0)  # behind the backdrop
    hits = ec.sliver_hits(case, ec.first_hits(dataclasses.replace(case, tris=bad))[0])
    assert all(n == 0 for _, n in hits[6].values())


# pyramids -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.PYRAMIDS))
def test_pyramid_cases_see_their_carpet(name):
    case = ec.pyramid(name)
    fov, w, h, variant = ec.PYRAMIDS[name]
    n_blocks = min(w // 8, ec.FRINGE_BLOCKS[0]) * min(h // 8, ec.FRINGE_BLOCKS[1])
    assert case.info["n_carpet"] == 1024 and case.info["n_fringe"] == 4 * n_blocks and len(case.tris) == 1024 + 4 * n_blocks and (case.w, case.h) == (w, h) and float(case.camera["fov"]) == np.float32(fov)
    lo, hi = ec.screen_boxes(case, slice(0, 1024))
    size = hi - lo
    assert 0.9 <= size.min() and size.max() <= 3.1, (size.min(), size.max())  # 1 to 3 px each (f32 vertices)
    assert case.region[0] % 8 == 0 and case.region[1] % 8 == 0 and case.spp == ec.PYRAMID_SPP and case.region[0] >= 0 and case.region[0] + case.region[2] <= w
    win, _ = ec.first_hits(dataclasses.replace(case, tris=case.tris[:1024], mats=case.mats[:1024]), samples=range(4))
    win = win[:, 8:8 + ec.CARPET_PX, 8:8 + ec.CARPET_PX]
    cover = (win >= 0).mean()
    strip = aimed_samples(case)
    assert fringe_samples(case) >= 400  # (64 blocks, four strips of 4 x 0.03 px each, 16 samples a pixel: 490 expected)
    assert strip >= 60, strip  # (four strips of 48 x 0.03 px and 16 samples a pixel: 92 expected, 10 their deviation)  # samples that fall into the strips of 0.03 px along the block borders the carpet's quads end behind
    print(f"{case.name}: {strip} samples in the strips, depth {case.info['depth']:.1f}, coverage of the region {cover:.3f}, {len(np.unique(win[win >= 0]))} triangles seen")
    assert cover >= ec.MIN_COVERAGE and len(np.unique(win[win >= 0])) >= 900
    if fov >= 1.0:
        assert case.info["depth"] == pytest.approx(np.linalg.norm(ec.PYRAMID_POS))  # around the origin
    _assert_materials(case)


def aimed_samples(case):
    """How many of the case's samples fall into the strips between a block border and the carpet edge 0.03 px behind it."""
    jx, jy = ec.sample_positions(case)
    x0, y0, rw, rh = case.region
    assert (x0 + 8, y0 + 8) == case.info["carpet"]
    sx = (np.arange(case.w) + jx)[:, y0:y0 + rh, x0:x0 + rw] - x0 - 8
    sy = (np.arange(case.h)[:, None] + jy)[:, y0:y0 + rh, x0:x0 + rw] - y0 - 8
    on = (sx > 0) & (sx < ec.CARPET_PX) & (sy > 0) & (sy < ec.CARPET_PX)
    in_x = ((sx % 24.0) < ec.CARPET_SHIFT[0]) & (sx >= 24.0) & (sy > 0) & (sy < ec.CARPET_PX - 0.03)
    in_y = ((sy % 24.0) > 24.0 + ec.CARPET_SHIFT[1]) & (sy < 24.0) & (sx > 0.03) & (sx < ec.CARPET_PX)
    return int(in_x.sum() + in_y.sum())


def fringe_samples(case):
    """How many of the region's samples fall into the fringe's strips: within FRINGE_REACH of a block border, on the half of the side
    whose triangle belongs to the sample's own block."""
    jx, jy = ec.sample_positions(case)
    x0, y0, rw, rh = case.region
    sx = ((np.arange(case.w) + jx)[:, y0:y0 + rh, x0:x0 + rw]) % 8.0
    sy = ((np.arange(case.h)[:, None] + jy)[:, y0:y0 + rh, x0:x0 + rw]) % 8.0
    r = ec.FRINGE_REACH
    return int(((sx < r) & (sy < 4)).sum() + ((sx > 8 - r) & (sy > 4)).sum() + ((sy < r) & (sx < 4)).sum() + ((sy > 8 - r) & (sx > 4)).sum())


def test_a_pyramid_carpet_at_the_origin_is_invisible_below_a_degree():
    """Why the narrow cases' carpets lie beyond the origin: at the origin's distance a triangle of 3 x 1.5 px has |a| < 1e-5."""
    case = ec.pyramid("0.3")
    pos = np.asarray(case.camera["position"], np.float64)
    shrunk = (pos + (case.tris.astype(np.float64) - pos) * (np.linalg.norm(pos) / case.info["depth"])).astype(np.float32)
    win, _ = ec.first_hits(dataclasses.replace(case, tris=shrunk), samples=range(2))
    assert (win == -1).all()
