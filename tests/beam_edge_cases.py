"""Camera samples aimed at the places where the camera beams (csrc/wavefront.hip, "Camera beams": k_wf_beams / k_wf_trace_camera) can
go wrong: a block's list at, one under and one over RT_BEAM_CAP; blocks without a list at the first, the last, alternate or all
places of the walk queue, with sample counts on both sides of the 8-sample chunk; lists whose order by box distance is not the order
of the hits; geometry within a fraction of a pixel of a block, tile or image border; and pyramids down to 0.003 degrees, whose
widening of an eighth of a pixel approaches the rounding of a corner direction.

Nothing here loads the library or the oracle: the sampler and the camera are estimator_cases' float64 restatements, the block order
is restated from rt_hip.h / DESIGN.md below.  test_beam_edge_cases.py checks, from float64 alone, the statement every case makes about
itself; test_gpu_beam_edges.py runs the cases.

Placement.  Geometry is given in SCREEN positions (pixels, float64: x right, y down, pixel i covers [i, i + 1)) and a depth along the
view axis, and back-projected (back_project); project() is the inverse.  What a case says about pixels it says about the f32
vertices the scene really holds.

Materials.  MATERIALS emissive materials, no lights, max_bounces = 0: a sample's value is 0.1 albedo + emission of the triangle it
hit, so a pixel's bits name the triangle (at spp 1) or the multiset of triangles (above)."""
import dataclasses
import math

import numpy as np

from estimator_cases import camera_rays, jitter
from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import types as T
from gpu_raytracer_amd.scenes import Scene

F32 = np.float32
CAP = 128             # RT_BEAM_CAP (wavefront.h)
LEAVES = 1024         # RT_BEAM_LEAVES
MARGIN_PX = 0.125     # RT_BEAM_MARGIN_PX
CHUNK = 8             # RT_BEAM_SAMPLES_PER_WAVE
DIST_SCALE = 0.99999  # RT_BEAM_DIST_SCALE
BOX_PAD = 2.0e-6      # the relative padding of a box, per coordinate, of |lo| + |hi|
MIN_T = 1e-5          # RT_MIN_RAY_DISTANCE: a hit needs t > MIN_T ...
MIN_A = 1e-5          # ... and a triangle |e1 . (d x e2)| >= MIN_A (device_common.h moller_trumbore): twice its area as the ray sees it
NO_LIST = None
MATERIALS = 64
CLEAR_PX = 1.0        # the cap / fallback statements: every triangle lies this far inside a block's square or outside the widened one


@dataclasses.dataclass
class Case:
    name: str
    tris: np.ndarray           # (n, 3, 3) f32
    mats: np.ndarray           # (n,) material index
    camera: np.ndarray         # types.CAMERA record
    w: int
    h: int
    tile: int
    spp: int = 1
    rank: int = 0
    world: int = 1
    frame_seed: int = 0
    spheres: tuple = ()        # (centre, radius, material)
    region: tuple = None       # (x0, y0, w, h): the part of the frame the statement looks at and the oracle renders (None: all of it)
    info: dict = dataclasses.field(default_factory=dict)

    def scene(self):
        return make_scene(self.name, self.tris, self.mats, self.camera, self.spheres)

    def render_kw(self, spp=None):
        return dict(mode=2, spp=self.spp if spp is None else spp, max_bounces=0, frame_seed=self.frame_seed, tile_size=self.tile,
                    tile_rank=self.rank, tile_world=self.world, kernel_pipeline=True)


def materials():
    out = []
    for k in range(MATERIALS):
        out.append(H.material_emissive((0.5, 0.5, 0.5), ((k % 4 + 1) / 4.0, ((k // 4) % 4 + 1) / 4.0, (k // 16 + 1) / 4.0)))
    return np.array(out, dtype=T.MATERIAL)


def make_scene(name, tris, mats, camera, spheres=()):
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    n = len(tris)
    vertices = np.zeros(n * 3, dtype=T.VERTEX)
    vertices["position"] = tris.reshape(-1, 3)
    triangles = np.zeros(n, dtype=T.TRIANGLE)
    idx = np.arange(n * 3, dtype=np.uint32).reshape(-1, 3)
    triangles["v0_index"], triangles["v1_index"], triangles["v2_index"] = idx[:, 0], idx[:, 1], idx[:, 2]
    triangles["material_id"] = np.asarray(mats, np.uint32)
    sph = np.zeros(len(spheres), dtype=T.SPHERE)
    for i, (c, r, m) in enumerate(spheres):
        sph[i]["center"], sph[i]["radius"], sph[i]["material_id"] = c, r, m
    return Scene(name, sph, np.zeros(0, T.LIGHT), vertices, triangles, materials(), camera)


# ---------------------------------------------------------------------------------------------------------------------------------
# the camera, restated in float64 from the f32 record (camera_rays has the forward direction; these add the inverse)
def _basis(cam):
    f, u = np.asarray(cam["direction"], np.float64), np.asarray(cam["up"], np.float64)
    r = np.cross(f, u)
    return np.asarray(cam["position"], np.float64), f, r, np.cross(r, f), math.tan(float(cam["fov"]) * 0.5 * math.pi / 180.0)


def screen_dir(cam, w, h, sx, sy):
    """The unnormalised direction through the screen position (sx, sy): forward + right cx + true_up cy."""
    _, f, r, t, fs = _basis(cam)
    cx = (np.asarray(sx, np.float64) / w * 2.0 - 1.0) * (w / h) * fs
    cy = (1.0 - np.asarray(sy, np.float64) / h * 2.0) * fs
    return f + cx[..., None] * r + cy[..., None] * t


def back_project(cam, w, h, sx, sy, depth):
    """World points that the screen positions see at `depth` (world units along the view axis)."""
    pos, f = _basis(cam)[:2]
    return pos + screen_dir(cam, w, h, sx, sy) * (np.asarray(depth, np.float64) / np.linalg.norm(f))[..., None]


def project(cam, w, h, points):
    """Screen positions (sx, sy) of world points in front of the camera, and their depth along the view axis."""
    pos, f, r, t, fs = _basis(cam)
    q = np.asarray(points, np.float64) - pos
    a, b, c = q @ f / (f @ f), q @ r / (r @ r), q @ t / (t @ t)
    assert (a > 0).all()
    return (b / a / ((w / h) * fs) + 1.0) * 0.5 * w, (1.0 - c / a / fs) * 0.5 * h, a * np.linalg.norm(f)


def sample_positions(case, samples=None):
    """(jx, jy) of the case's samples, (n, h, w): the sampler's two draws when the frame jitters (spp > 1), the pixel centre otherwise."""
    samples = np.arange(case.spp) if samples is None else np.asarray(samples)
    if case.spp > 1:
        return jitter(case.frame_seed, case.w, case.h, samples)
    half = np.full((len(samples), case.h, case.w), 0.5)
    return half, half


# ---------------------------------------------------------------------------------------------------------------------------------
# the blocks: a context owns the tiles whose row-major index % world == rank, in that order; one 8x8 block per wave,
# ceil(tile / 8)^2 per tile whether inside the image or not, row by row within the tile (tests/test_gpu_adaptive.py _block_table)
def block_table(w, h, tile, rank=0, world=1):
    """(n, 4) per owned block in the library's order: its first pixel (x0, y0) and how many columns and rows of it (nx, ny) lie inside
    its tile and the image (0: the block has no pixel and still takes its place)."""
    tx, ty, per_side = (w + tile - 1) // tile, (h + tile - 1) // tile, (tile + 7) // 8
    rows = []
    for t in range(rank, tx * ty, world):
        oy, ox = (t // tx) * tile, (t % tx) * tile
        for by in range(per_side):
            for bx in range(per_side):
                y0, x0 = oy + 8 * by, ox + 8 * bx
                nx, ny = max(0, min(x0 + 8, ox + tile, w) - x0), max(0, min(y0 + 8, oy + tile, h) - y0)
                rows.append((x0, y0, nx if ny else 0, ny if nx else 0))
    return np.array(rows, np.int64)


def owned_mask(w, h, tile, rank=0, world=1):
    m = np.zeros((h, w), bool)
    for x0, y0, nx, ny in block_table(w, h, tile, rank, world):
        m[y0:y0 + ny, x0:x0 + nx] = True
    return m


def block_of_pixel(case, x, y):
    """Index of the owned block that holds pixel (x, y), or -1."""
    for b, (x0, y0, nx, ny) in enumerate(block_table(case.w, case.h, case.tile, case.rank, case.world)):
        if x0 <= x < x0 + nx and y0 <= y < y0 + ny:
            return b
    return -1


def case_blocks(case):
    return block_table(case.w, case.h, case.tile, case.rank, case.world)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 statement of a first hit: Moeller-Trumbore on the records' (v0, e1, e2) (f32 differences), the rules of
# device_common.h: |a| >= 1e-5, 0 <= u, 0 <= v, u + v <= 1, t > 1e-5, the nearest wins, the lowest index among equal t, a sphere
# (tested first) keeps an equal t
def first_hits(case, samples=None, region=None):
    """-> (winner (n, rh, rw) int64: triangle index, -1 sky, -2 - i sphere i; t (n, rh, rw)) over the case's region."""
    jx, jy = sample_positions(case, samples)
    o, d = camera_rays(case.camera, case.w, case.h, jx, jy)
    x0, y0, rw, rh = region or case.region or (0, 0, case.w, case.h)
    d = d[:, y0:y0 + rh, x0:x0 + rw]
    best = np.full(d.shape[:-1], np.inf)
    win = np.full(d.shape[:-1], -1, np.int64)
    for i, (c, r, _) in enumerate(case.spheres):
        oc = o - np.asarray(c, np.float64)
        b = 2.0 * (d @ oc)
        disc = b * b - 4.0 * (oc @ oc - r * r)
        with np.errstate(invalid="ignore"):
            sq = np.sqrt(disc)
            t1, t2 = (-b - sq) / 2.0, (-b + sq) / 2.0
            t = np.where(t1 > MIN_T, t1, t2)
            ok = (disc >= 0) & (t > MIN_T) & (t < best)
        best, win = np.where(ok, t, best), np.where(ok, -2 - i, win)
    tr = np.asarray(case.tris, F32)
    v0, e1, e2 = tr[:, 0].astype(np.float64), (tr[:, 1] - tr[:, 0]).astype(np.float64), (tr[:, 2] - tr[:, 0]).astype(np.float64)
    for k in range(len(tr)):
        hv = np.cross(d, e2[k])
        a = hv @ e1[k]
        with np.errstate(all="ignore"):
            f = 1.0 / a
            s = o - v0[k]
            u = f * (hv @ s)
            q = np.cross(s, e1[k])
            v = f * (d @ q)
            t = f * (q @ e2[k])
            ok = (np.abs(a) >= MIN_A) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > MIN_T) & (t < best)
        best, win = np.where(ok, t, best), np.where(ok, k, win)
    return win, best


def box_distance(case):
    """Per triangle the distance from the camera to its (unpadded) box: what k_wf_beams orders a list by, before its 0.99999."""
    tr = np.asarray(case.tris, np.float64)
    lo, hi, o = tr.min(1), tr.max(1), np.asarray(case.camera["position"], np.float64)
    return np.linalg.norm(np.maximum(np.maximum(lo - o, o - hi), 0.0), axis=1)


def screen_boxes(case, idx=None):
    """Per triangle the bounding rectangle of its projected f32 vertices, in pixels: (lo (n, 2), hi (n, 2))."""
    tr = np.asarray(case.tris, F32)[slice(None) if idx is None else idx]
    sx, sy, _ = project(case.camera, case.w, case.h, tr.reshape(-1, 3))
    p = np.stack([sx, sy], -1).reshape(-1, 3, 2)
    return p.min(1), p.max(1)


def mix_material(*ks):
    """A material index from small integers such that a step of 1 in any of them changes it."""
    return int(sum(k * m for k, m in zip(ks, (5, 11, 23, 37)))) % MATERIALS


def nearest_on_screen(case):
    """Per triangle the index of the nearest other triangle on the screen (by the middles of their rectangles; coincident twins do not count)."""
    lo, hi = screen_boxes(case)
    c = 0.5 * (lo + hi)
    d = np.linalg.norm(c[:, None, :] - c[None, :, :], axis=-1)
    tr = np.asarray(case.tris)
    d[(tr[:, None] == tr[None, :]).all((2, 3))] = np.inf
    return d.argmin(1)


def separate_materials(case):
    """Changes materials until no triangle shares one with its neighbours in index or with its nearest neighbour on the screen."""
    near = nearest_on_screen(case)
    mats = case.mats
    n = len(mats)
    for _ in range(8):
        clash = [k for k in range(n) if mats[k] == mats[near[k]] or (k > 0 and mats[k] == mats[k - 1])]
        if not clash:
            return
        for k in clash:
            taken = {int(mats[near[k]]), int(mats[max(k - 1, 0)]), int(mats[min(k + 1, n - 1)])} | {int(mats[j]) for j in np.flatnonzero(near == k)}
            mats[k] = next(m for m in range((int(mats[k]) + 17) % MATERIALS, 2 * MATERIALS) if m % MATERIALS not in taken) % MATERIALS
    raise AssertionError(f"{case.name}: materials still clash")


# ---------------------------------------------------------------------------------------------------------------------------------
# cap / fallback: stacks of micro-triangles over single blocks
_FRONT = dict(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=45.0)
MICRO_PX = 0.15     # the legs of a micro-triangle (its box is under 0.2 px)
OVER_FULL = 200
SPARSE = 3


CELL = 0.25         # admissible places are found on a grid of quarter pixels


def admissible_cells(blocks, b):
    """The quarter-pixel cells (x, y of their first corner) of block b that lie CLEAR_PX inside b's own square and, for every other owned
    block, CLEAR_PX outside its widened square in x or in y: a micro-triangle inside such a cell is in b's list and in no other (tiles
    that are no multiple of 8 make blocks overlap, and leave a block only a strip of its own)."""
    x0, y0 = blocks[b, :2]
    far = CLEAR_PX + MARGIN_PX
    out = []
    for j in np.arange(y0 + CLEAR_PX, y0 + 8 - CLEAR_PX, CELL):
        for i in np.arange(x0 + CLEAR_PX, x0 + 8 - CLEAR_PX, CELL):
            ok = True
            for o, (ox, oy, _, _) in enumerate(blocks):
                if o != b:
                    ok &= bool(i + CELL <= ox - far or i >= ox + 8 + far or j + CELL <= oy - far or j >= oy + 8 + far)
            if ok:
                out.append((float(i), float(j)))
    inner = [(x, y) for x, y in out if x >= x0 + 2 and x + CELL <= x0 + 6 and y >= y0 + 2 and y + CELL <= y0 + 6]
    return inner or out  # (the block's inner 4x4 pixels where the other blocks leave them)


def _backdrop(cam, w, h, blocks, depth=8.0):
    """Two triangles behind everything whose rectangle covers every owned block's widened square by two pixels and more."""
    x_lo, y_lo = blocks[:, 0].min() - 4.0, blocks[:, 1].min() - 5.3  # (uneven: the shared edge passes through no pixel centre)
    x_hi, y_hi = blocks[:, 0].max() + 13.7, blocks[:, 1].max() + 12.0
    c = back_project(cam, w, h, np.array([x_lo, x_hi, x_hi, x_lo]), np.array([y_lo, y_lo, y_hi, y_hi]), np.full(4, depth))
    return np.array([[c[0], c[1], c[2]], [c[0], c[2], c[3]]])


def _stack(cam, w, h, cells, n, rng):
    """n right-angled micro-triangles with legs MICRO_PX, each inside admissible cells; every second one covers a pixel's centre where
    the four cells around one are admissible (so that pixel centres see a pile of them).  Depths 2 .. 6, shuffled against the index."""
    depths = np.linspace(2.0, 6.0, n) if n > 1 else np.array([4.0])
    depths = depths[rng.permutation(n)]
    have = set(cells)
    centres = [(x + CELL, y + CELL) for x, y in cells if (x + CELL) % 1.0 == 0.5 and (y + CELL) % 1.0 == 0.5
               and {(x + CELL, y), (x, y + CELL), (x + CELL, y + CELL)} <= have]
    tris = []
    for k in range(n):
        if k % 2 == 0 and centres:
            x, y = centres[rng.integers(len(centres))]
            cx, cy = x - MICRO_PX * rng.uniform(0.2, 0.4), y - MICRO_PX * rng.uniform(0.2, 0.4)
        else:
            x, y = cells[rng.integers(len(cells))]
            cx, cy = x + rng.uniform(0.02, CELL - MICRO_PX - 0.02), y + rng.uniform(0.02, CELL - MICRO_PX - 0.02)
        sx, sy = np.array([cx, cx + MICRO_PX, cx]), np.array([cy, cy, cy + MICRO_PX])
        tris.append(back_project(cam, w, h, sx, sy, np.full(3, depths[k])))
    return np.array(tris).reshape(-1, 3, 3)


def _stacked_case(name, w, h, tile, counts, spp, rank=0, world=1, seed=1):
    """counts: micro-triangles per owned block (in block order)."""
    cam = H.camera(**_FRONT)
    blocks = block_table(w, h, tile, rank, world)
    assert len(counts) == len(blocks)
    rng = np.random.default_rng(seed)
    tris, mats, owner = [_backdrop(cam, w, h, blocks)], [mix_material(0, 0, 1), mix_material(0, 0, 2)], [-1, -1]
    for b, n in enumerate(counts):
        if n == 0:
            continue
        pix = admissible_cells(blocks, b)
        assert pix, f"{name}: block {b} has no place of its own"
        tris.append(_stack(cam, w, h, pix, n, rng))
        mats += [mix_material(k, b) for k in range(n)]
        owner += [b] * n
    case = Case(name, np.concatenate(tris).astype(F32), np.array(mats), cam, w, h, tile, spp=spp, rank=rank, world=world,
                info=dict(backdrop=[0, 1], owner=np.array(owner), counts=list(counts)))
    separate_materials(case)
    return case


def expected_lists(case):
    """The statement of the cap and fallback families, from the f32 vertices alone: per owned block the exact length of its list, or
    NO_LIST.  Holds because (asserted here) the camera looks along -z with an upright screen and every triangle is flat in z, so a
    triangle's box projects to its screen rectangle; the backdrop's rectangle covers every block's widened square; and every other
    triangle's rectangle lies CLEAR_PX inside a block's own square (it is in that list: an eighth of a pixel, the padding and every
    rounding are far smaller) or CLEAR_PX outside the widened one in x or in y (it is outside one of the pyramid's planes).
    Raises AssertionError when a triangle is neither: the case does not aim."""
    cam = case.camera
    assert tuple(cam["direction"]) == (0.0, 0.0, -1.0) and tuple(cam["up"]) == (0.0, 1.0, 0.0)
    tr = np.asarray(case.tris, F32)
    assert (tr[:, :, 2].max(1) == tr[:, :, 2].min(1)).all()
    lo, hi = screen_boxes(case)
    blocks = case_blocks(case)
    back = np.zeros(len(tr), bool)
    back[case.info["backdrop"]] = True
    far = CLEAR_PX + MARGIN_PX
    assert (lo[back, 0] <= blocks[:, 0].min() - far).all() and (hi[back, 0] >= blocks[:, 0].max() + 8 + far).all()
    assert (lo[back, 1] <= blocks[:, 1].min() - far).all() and (hi[back, 1] >= blocks[:, 1].max() + 8 + far).all()
    out = []
    for x0, y0, _, _ in blocks:
        inside = (lo[:, 0] >= x0 + CLEAR_PX) & (hi[:, 0] <= x0 + 8 - CLEAR_PX) & (lo[:, 1] >= y0 + CLEAR_PX) & (hi[:, 1] <= y0 + 8 - CLEAR_PX)
        outside = (hi[:, 0] <= x0 - far) | (lo[:, 0] >= x0 + 8 + far) | (hi[:, 1] <= y0 - far) | (lo[:, 1] >= y0 + 8 + far)
        assert (inside | outside | back).all(), f"{case.name}: triangles {np.flatnonzero(~(inside | outside | back))[:5]} lie on the border of block ({x0}, {y0})"
        n = int((inside & ~back).sum()) + int(back.sum())
        out.append(n if n <= CAP else NO_LIST)
    return out


CAP_NS = (1, 63, 64, 65, 126, 127, 128, 198)


def cap(n, spp=1):
    """A 24x24 frame, nine blocks; the middle one (block 4) holds n micro-triangles in its inner 4x4 pixels: its list is n + 2.
    spp 1: the pixel centres see the piles."""
    counts = [0] * 9
    counts[4] = n
    case = _stacked_case(f"cap {n}", 24, 24, 24, counts, spp, seed=100 + n)
    case.info["target"] = 4
    return case


FALLBACK_FRAMES = {           # name: (w, h, tile, rank, world)
    "16x16": (16, 16, 16, 0, 1),            # four blocks
    "20x12 tile 12": (20, 12, 12, 0, 1),    # eight blocks that overlap; two of them have no pixel inside the image
    "32x16 rank 1 of 3": (32, 16, 8, 1, 3), # eight tiles of one block: this share owns tiles 1, 4 and 7
}
FALLBACK_PATTERNS = ("none", "first", "last", "alternate", "every")
FALLBACK_SPP = (1, 7, 8, 9, 17)


def fallback(frame, pattern, spp=1):
    w, h, tile, rank, world = FALLBACK_FRAMES[frame]
    n = len(block_table(w, h, tile, rank, world))
    over = {"none": [], "first": [0], "last": [n - 1], "alternate": list(range(0, n, 2)), "every": list(range(n))}[pattern]
    counts = [OVER_FULL if b in over else SPARSE for b in range(n)]
    case = _stacked_case(f"fallback {frame} {pattern}", w, h, tile, counts, spp, rank, world, seed=7)
    case.info["over"] = over
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
# order: lists whose order by box distance says little or nothing about the order of the hits
def _slanted(cam, w, h, depth, slope, reach):
    """A triangle over the whole view whose plane passes the view axis at `depth` and comes nearer by `slope` per unit to the right:
    two of its vertices lie `reach` away, so its box starts far in front of what the view sees of it."""
    pos = np.asarray(cam["position"], np.float64)
    z = lambda x: pos[2] - depth + slope * x
    return np.array([[pos[0] + reach, pos[1] - reach, z(reach)], [pos[0] + reach, pos[1] + reach, z(reach)], [pos[0] - 2 * reach, pos[1], z(-2 * reach)]])


def order_inside_boxes():
    """(a) 40 large slanted triangles in front of the camera, each with the camera inside its box: every bound is 0, the list's order is
    the order of the records, and the planes cross one another, so every block sees several winners."""
    rng = np.random.default_rng(11)
    cam = H.camera(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fov=60.0)
    tris, R = [], 10.0
    for k in range(40):
        d0 = 1.0 + 0.5 * rng.random()
        a, b = rng.choice([-1, 1]) * rng.uniform(0.3, 0.5), rng.choice([-1, 1]) * rng.uniform(0.3, 0.5)
        z = lambda x, y: -d0 + a * x + b * y
        tris.append([(-R, -R, z(-R, -R)), (R, -R, z(R, -R)), (0.0, R, z(0.0, R))])
    return Case("order inside boxes", np.array(tris, F32), np.array([mix_material(k) for k in range(40)]), cam, 32, 32, 32, spp=4)


ORDER_B = dict(depth=4.0, behind=3e-4, slope=5e-3, reach=40.0, fov=2.0)


def order_slanted_first():
    """(b) Triangle 0 covers the view 3e-4 of the depth BEHIND thirty small triangles and its box starts far in front of them: it is
    first in every list, every sample hits it, and every small triangle must still be tested after it.  The view is 2 degrees wide, so
    a hit's distance and a box's differ by 1.0003 at most: a bound that is 0.1 % too large ends the list after entry 0."""
    p = ORDER_B
    cam = H.camera(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fov=p["fov"])
    w = h = 32
    tris, mats = [_slanted(cam, w, h, p["depth"] * (1.0 + p["behind"]), p["slope"], p["reach"])], [mix_material(0, 1)]
    rng = np.random.default_rng(5)
    for k in range(30):
        cx, cy = 2.0 + 28.0 * rng.random(), 2.0 + 28.0 * rng.random()
        s = rng.uniform(4.0, 6.0)
        depth = p["depth"] * (1.0 - 1e-5 * (k % 5))
        tris.append(back_project(cam, w, h, np.array([cx - s / 2, cx + s / 2, cx]), np.array([cy - s / 2, cy - s / 2, cy + s / 2]), np.full(3, depth)))
        mats.append(mix_material(k + 1))
    return Case("order slanted first", np.array(tris, F32), np.array(mats), cam, w, h, 32, spp=4, info=dict(slanted=0))


def order_coincident_pairs():
    """(c) Twenty triangles, each twice: records i and n - 1 - i hold the same vertices and different materials.  Equal t: the lower
    index wins wherever the pair sits in the list."""
    rng = np.random.default_rng(3)
    cam = H.camera(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fov=50.0)
    w = h = 32
    half = []
    for k in range(20):
        cx, cy, s = 3.0 + 26.0 * rng.random(), 3.0 + 26.0 * rng.random(), rng.uniform(4.0, 9.0)
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
        depth = 3.0 + 2.0 * rng.random() + 0.3 * np.cos(ang)  # (tilted: the pairs' boxes overlap in depth)
        half.append(back_project(cam, w, h, cx + s * np.cos(ang), cy + s * np.sin(ang), depth))
    half = np.array(half, F32)
    tris = np.concatenate([half, half[::-1]])
    n = len(tris)
    mats = np.array([mix_material(k, int(k >= 20)) for k in range(n)])
    return Case("order coincident pairs", tris, mats, cam, w, h, 32, spp=4, info=dict(pairs=[(i, n - 1 - i) for i in range(20)]))


ORDER_D = [(D, gap) for D in (1.0, 1e3, 1e5) for gap in (5e-6, 2e-5)]


def order_plates(D, gap):
    """(d) Two plates across the view at distances D (1 + gap) (records 0, 1) and D (records 2, 3): the nearer plate has the higher
    index.  gap = 5e-6 lies under what RT_BEAM_DIST_SCALE takes off a bound (1e-5), 2e-5 over it."""
    cam = H.camera(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fov=2.0)
    w = h = 16
    tris = []
    for depth in (D * (1.0 + gap), D):
        c = back_project(cam, w, h, np.array([-8.0, 24.0, 24.0, -8.0]), np.array([-8.0, -8.0, 24.0, 24.0]), np.full(4, depth))
        tris += [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
    return Case(f"order plates D={D:g} gap={gap:g}", np.array(tris, F32), np.array([mix_material(k) for k in range(4)]), cam, w, h, 16, spp=4,
                info=dict(near=[2, 3], far=[0, 1]))


def order_spheres():
    """(e) Three spheres and three plates at z = -4, on a 33x33 frame whose middle pixel looks exactly along the axis: sphere 0 in front
    of its plate, sphere 1 behind its (smaller) plate, sphere 2 (centre (0, 0, -5), radius 1) touching the middle plate's plane on the
    axis: t = 4 for both, and the sphere, tested first, keeps it."""
    cam = H.camera(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fov=60.0)
    plate = lambda x0, x1, y: [[(x0, -y, -4.0), (x1, -y, -4.0), (x1, y, -4.0)], [(x0, -y, -4.0), (x1, y, -4.0), (x0, y, -4.0)]]
    tris = np.array(plate(-2.2, -1.0, 0.8) + plate(1.2, 2.0, 0.5) + plate(-0.8, 0.8, 0.8), F32)
    spheres = (((-1.6, 0.0, -3.0), 0.4, mix_material(0, 0, 0, 1)), ((2.4, 0.0, -6.0), 1.4, mix_material(1, 0, 0, 1)), ((0.0, 0.0, -5.0), 1.0, mix_material(2, 0, 0, 1)))
    return Case("order spheres", tris, np.array([mix_material(k) for k in range(6)]), cam, 33, 33, 33, spp=1, spheres=spheres)


# ---------------------------------------------------------------------------------------------------------------------------------
# edges: slivers on and next to block, tile and image borders
EDGE_OFFSETS = (0.0, 0.05, -0.05, 0.3, -0.3)
SLIVER_W, SLIVER_L = 0.6, 3.0
EDGE_FRAME = dict(w=32, h=32, tile=16)   # block borders at 8 and 24, a tile border at 16, the image's at 0 and 32
MIN_SIDE_PX = 0.2                        # a side of a border on which a sliver is at least this wide must be hit from that side


def edges(spp):
    """Slivers SLIVER_W x SLIVER_L px (two triangles each) along every border x = 8k and y = 8k of a 32x32 frame with 16-pixel tiles, at
    the offsets EDGE_OFFSETS from it, in front of a backdrop.  spp = 64: jittered samples.  spp = 1: pixel centres; the slivers are
    centred on the pixel centres next to the border instead (border -+ 0.5 + offset / 10)."""
    cam = H.camera(**_FRONT)
    w, h, tile = EDGE_FRAME["w"], EDGE_FRAME["h"], EDGE_FRAME["tile"]
    blocks = block_table(w, h, tile)
    tris, mats = [_backdrop(cam, w, h, blocks)], [mix_material(0, 0, 1), mix_material(0, 0, 2)]
    slivers = []  # (axis, border, offset, first triangle, centre across, centre along)
    for axis in (0, 1):
        for bi, border in enumerate(range(0, w + 1, 8)):
            for oi, off in enumerate(EDGE_OFFSETS):
                slot = (oi + 2 * bi + 3 * axis) % 8
                along = 8 * (slot // 2) + (2.5 if slot % 2 == 0 else 5.5)
                if spp > 1:
                    across = border + off
                else:
                    side = 1 if border == 0 else -1 if border == w else 1 if (oi + bi) % 2 == 0 else -1  # (inward at the image's border)
                    across = border + 0.5 * side + off / 10.0
                a0, a1, l0, l1 = across - SLIVER_W / 2, across + SLIVER_W / 2, along - SLIVER_L / 2, along + SLIVER_L / 2
                qa, ql = np.array([a0, a1, a1, a0]), np.array([l0, l0, l1, l1])
                sx, sy = (qa, ql) if axis == 0 else (ql, qa)
                c = back_project(cam, w, h, sx, sy, np.full(4, 3.0 - 0.5 * axis))  # (the horizontal ones pass in front of the vertical ones)
                slivers.append((axis, border, off, len(np.concatenate(tris)), across, along))
                tris.append(np.array([[c[0], c[1], c[2]], [c[0], c[2], c[3]]]))
                mats += [mix_material(len(slivers), 0), mix_material(len(slivers), 1)]
    return Case(f"edges spp {spp}", np.concatenate(tris).astype(F32), np.array(mats), cam, w, h, tile, spp=spp, frame_seed=3,
                info=dict(slivers=slivers, backdrop=[0, 1]))


def sliver_hits(case, win):
    """Per sliver: {side: (width of the sliver on that side of its border inside the image, samples of that side's pixels whose first hit
    it is)} for side -1 (left / above) and +1.  win: first_hits(case)[0]."""
    out = []
    size = (case.w, case.h)
    for axis, border, off, first, across, along in case.info["slivers"]:
        mine = (win == first) | (win == first + 1)
        per_pixel = mine.sum(0)  # (h, w)
        sides = {}
        for side in (-1, 1):
            lo, hi = (across - SLIVER_W / 2, min(across + SLIVER_W / 2, border)) if side < 0 else (max(across - SLIVER_W / 2, border), across + SLIVER_W / 2)
            lo, hi = max(lo, 0.0), min(hi, float(size[axis]))
            width = max(0.0, hi - lo)
            px = slice(0, border) if side < 0 else slice(border, size[axis])
            n = int(per_pixel[:, px].sum() if axis == 0 else per_pixel[px, :].sum())
            sides[side] = (width, n)
        out.append(sides)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# pyramids: narrow and wide fields of view
PYRAMIDS = {                 # name: (fov, w, h, camera variant)
    "0.3": (0.3, 64, 1080, "aimed"), "0.1": (0.1, 64, 1080, "aimed"), "0.03": (0.03, 64, 1080, "aimed"),
    "0.02": (0.02, 256, 256, "aimed"), "0.01": (0.01, 64, 64, "aimed"), "0.003": (0.003, 64, 64, "aimed"),
    "120": (120.0, 64, 64, "aimed"), "170": (170.0, 64, 64, "aimed"),
    "0.1 unnormalised": (0.1, 64, 1080, "unnormalised"), "0.1 tilted up": (0.1, 64, 1080, "tilted up"),
    "0.003 unnormalised": (0.003, 64, 64, "unnormalised"),
}
PYRAMID_POS = (0.3, 0.2, 5.0)
CARPET = (32, 16)            # quads across and down, two triangles each: 1 024 triangles
CARPET_PX = 48               # ... over 48 x 48 pixels that start on a block border: a quad is 1.5 x 3 px
CARPET_SHIFT = (0.03, -0.03) # the carpet's offset from that border: every 24 px a quad ENDS 0.03 px inside the next block in x, the previous in y
FRINGE_REACH = 0.03          # the fringe: per block and side a triangle that lies in the neighbouring block and ends this far inside
FRINGE_BLOCKS = (8, 48)      # ... for the blocks of at most this many columns and rows around the frame's middle
PYRAMID_SPP = 16             # jittered: a pixel centre is half a pixel from every border, a pyramid that is 0.2 px too narrow loses none
MIN_COVERAGE = 0.9
VISIBLE_A = 4e-5             # the smallest |a| a carpet triangle is built with: four times the test's threshold


def pyramid(name):
    """A carpet of 1 024 triangles (right-angled, legs 1.5 and 3 px) over 48 x 48 pixels in the frame's middle, in the plane normal to
    the view, quads alternately 1e-3 of the depth nearer and farther.  It is shifted by CARPET_SHIFT against the block borders: along
    the borders at 24 and 48 px the triangles of one block reach three hundredths of a pixel into the next, so the samples that fall
    into that strip need a triangle whose box lies almost wholly outside their own block's pyramid.  In front of the carpet, a fringe
    (below) does the same on every side of every block of the frame's middle.  The camera sits at PYRAMID_POS and looks at the origin (`aimed`), along
    (0, 0, -3) (`unnormalised`: right and true_up are 3 and 9 long), or at the origin with an `up` 30 degrees off the screen's.
    DEPTH: the carpet lies around the view axis at the origin's distance or, at the narrow fields of view, as far beyond it as a
    triangle of 1.5 by 3 pixels needs to have |a| = VISIBLE_A: nearer, Moeller-Trumbore's |a| >= 1e-5 rejects every carpet triangle
    for every ray and the frame is sky whatever the lists hold."""
    fov, w, h, variant = PYRAMIDS[name]
    pos = np.array(PYRAMID_POS)
    if variant == "unnormalised":
        direction, up = (0.0, 0.0, -3.0), (0.0, 1.0, 0.0)
    else:
        direction = tuple(-pos / np.linalg.norm(pos))
        up = (0.0, 1.0, 0.0) if variant == "aimed" else (math.sin(math.radians(30.0)), math.cos(math.radians(30.0)), 0.0)
    cam = H.camera(position=tuple(pos), direction=direction, up=up, fov=fov)
    x0, y0 = (w - CARPET_PX) // 16 * 8, (h - CARPET_PX) // 16 * 8
    nx, ny = CARPET
    gx, gy = np.meshgrid(x0 + CARPET_SHIFT[0] + float(CARPET_PX) / nx * np.arange(nx + 1), y0 + CARPET_SHIFT[1] + float(CARPET_PX) / ny * np.arange(ny + 1))

    def build(depth):
        tris, mats = [], []
        for j in range(ny):
            for i in range(nx):
                dq = depth * (1.0 + 1e-3 * ((i + j) % 2 * 2 - 1))
                sx = np.array([gx[j, i], gx[j, i + 1], gx[j + 1, i + 1], gx[j + 1, i]])
                sy = np.array([gy[j, i], gy[j, i + 1], gy[j + 1, i + 1], gy[j + 1, i]])
                c = back_project(cam, w, h, sx, sy, np.full(4, dq))
                tris += [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
                mats += [mix_material(i, j, 0), mix_material(i, j, 1)]
        return np.array(tris), np.array(mats)
    def fringe(depth):
        """Per block of the middle FRINGE_BLOCKS and per side one triangle along half of that side: its base FRINGE_REACH inside the
        block, its apex a pixel outside.  A sample in the strip between border and base needs a triangle whose box lies, but for
        three hundredths of a pixel, outside its own block's pyramid.  (Left and top: the first half of the side; right and bottom: the
        second - the neighbour's triangle along the same border takes the other half.)"""
        bx0, by0 = max(0, (w // 8 - FRINGE_BLOCKS[0]) // 2), max(0, (h // 8 - FRINGE_BLOCKS[1]) // 2)
        tris, mats = [], []
        r = FRINGE_REACH
        for by in range(by0, min(h // 8, by0 + FRINGE_BLOCKS[1])):
            for bx in range(bx0, min(w // 8, bx0 + FRINGE_BLOCKS[0])):
                X, Y = 8.0 * bx, 8.0 * by
                sides = [((X + r, Y), (X + r, Y + 4), (X - 1, Y + 2)), ((X + 8 - r, Y + 4), (X + 8 - r, Y + 8), (X + 9, Y + 6)),
                         ((X, Y + r), (X + 4, Y + r), (X + 2, Y - 1)), ((X + 4, Y + 8 - r), (X + 8, Y + 8 - r), (X + 6, Y + 9))]
                for k, tri in enumerate(sides):
                    sxy = np.array(tri)
                    tris.append(back_project(cam, w, h, sxy[:, 0], sxy[:, 1], np.full(3, depth * (0.990 + 0.001 * k))))
                    mats.append(mix_material(bx, by, k, 1))
        return np.array(tris), np.array(mats)
    depth = float(np.linalg.norm(pos))
    tris, mats = build(depth)
    view = screen_dir(cam, w, h, np.array(w / 2.0), np.array(h / 2.0))
    view /= np.linalg.norm(view)
    a_min = np.abs(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]) @ view).min()
    if a_min < VISIBLE_A:
        depth *= math.sqrt(VISIBLE_A / a_min) * 1.05
        tris, mats = build(depth)
    ftris, fmats = fringe(depth)
    n_carpet = len(tris)
    tris, mats = np.concatenate([tris, ftris]), np.concatenate([mats, fmats])
    case = Case(f"pyramid {name}", tris.astype(F32), mats, cam, w, h, 64, spp=PYRAMID_SPP, region=(x0 - 8, y0 - 8, CARPET_PX + 16, CARPET_PX + 16),
                info=dict(depth=depth, fov=fov, carpet=(x0, y0), n_carpet=n_carpet, n_fringe=len(ftris)))  # (the region: the carpet and the blocks around it)
    separate_materials(case)
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
ORDER = {"inside boxes": order_inside_boxes, "slanted first": order_slanted_first, "coincident pairs": order_coincident_pairs, "spheres": order_spheres}
ORDER.update({f"plates D={D:g} gap={gap:g}": (lambda D=D, gap=gap: order_plates(D, gap)) for D, gap in ORDER_D})


def single_triangle(w, h):
    """Step 4 of the work's plan: one far triangle, 60 degrees: only the pyramid's own `bad` test can leave a block without a list."""
    cam = H.camera(position=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fov=60.0)
    return Case(f"single triangle {w}x{h}", np.array([[(-50.0, -40.0, -100.0), (60.0, -30.0, -100.0), (0.0, 55.0, -100.0)]], F32), np.array([5]), cam, w, h, 64)
