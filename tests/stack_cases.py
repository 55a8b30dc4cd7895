"""The deck: a small scene whose 8-wide tree is deep for its size and whose rays enter every box without hitting anything, so that
every traversal stack is driven to its high-water mark on a scene brute force can still check (DESIGN.md "Traversal stacks").

Geometry.  n right triangles ("cards") with corners (-1,-1), (1,-1), (-1,1) in the planes z = -3 - 4 i / n, each shifted in x and y
by a seeded jitter of at most JITTER so that Morton codes differ.  Every card's box is (nearly) the whole square [-1,1]^2 in its plane,
so the boxes of the tree overlap completely in x and y and are told apart along z only: a ray through the EMPTY half of the square
(x + y > 0) that runs roughly along z enters every node and every leaf and hits no card; a ray through the COVERED half (x + y < 0)
crosses all n cards.  Behind the deck stands a diffuse wall, beside it one sphere; a point light on the camera's side is placed so that
the segments from the wall behind the empty half reach it through the empty half, and a directional light shines along the deck.
Every eighth card is metallic.  The camera is far away with a narrow lens, so that its rays stay inside the cards' boxes over the
deck's whole length.

Ray sets, RECORDS each, as (N, 8) float32 batches (ox oy oz tmin dx dy dz tmax):
  through   x + y <= -MARGIN at both ends of the deck: crosses all n cards, the closest hit is card 0 (from the front)
  corner    x + y >= +MARGIN at both ends, inside the square: enters every box, crosses no card, ends on the wall
  mixed     oblique, from in front of and from behind the deck, through both regions in turn (the waves the overflow needs: lanes
            that finish at once beside lanes that visit everything, in two different child orders)
  crossing  (for the model of tests/check_stack_marks.cpp only) MIXED_CORNER_LANES of every 64 rays enter through the empty corner and
            leave through the covered half, so that they find a card in mid-deck behind boxes they entered in vain; the others are
            "through" rays.  These are the rays whose answer depends on what the deepest stack entries hold.
MARGIN is more than twice the jitter of both coordinates together, which is what makes the two statements above closed forms
(tests/test_stack_cases.py holds them against reference_cases.closest_hit in float64).

Nothing here needs a GPU or the library."""
import dataclasses

import numpy as np

from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

N_CARDS = 8192
JITTER = 0.02
MARGIN = 0.1          # > 2 * (2 * JITTER): |x + y| of a card's hypotenuse stays below 2 * JITTER
Z_FRONT, Z_LENGTH = -3.0, 4.0
Z_WALL = -8.0
INSIDE = 0.95         # |x|, |y| <= INSIDE lies inside every card's box (1 - JITTER = 0.98)
RECORDS = 256
SHEAR = 0.5
SEED = 0x5EC4
FRAME = (64, 48)      # the GPU tests' frame size
MAT_CARD, MAT_METAL, MAT_WALL, MAT_BALL = 0, 1, 2, 3
LIGHT_POS = (0.7, 0.7, 4.0)
MIXED_CORNER_LANES = 22  # of every 64 consecutive "mixed" rays in the first half of the set (mixed_covered)


def camera():
    return H.camera(position=(0.0, 0.0, 20.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=4.5)


def card_corners(n=N_CARDS, shear=0.0, seed=SEED):
    """(n, 3, 3) float32 corners of the cards.  shear: card i moves in x by shear * i / n (same topology, boxes that overlap far more
    once a tree built for shear 0 is refitted)."""
    rng = np.random.default_rng(seed)
    jit = rng.uniform(-JITTER, JITTER, (n, 2))
    i = np.arange(n, dtype=np.float64)
    base = np.array([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0]])
    c = np.zeros((n, 3, 3))
    c[:, :, :2] = base[None] + jit[:, None, :]
    c[:, :, 0] += (shear * i / n)[:, None]
    c[:, :, 2] = (Z_FRONT - Z_LENGTH * i / n)[:, None]
    return c.astype(np.float32)


def _wall():
    a, b, c, d = (-3.0, -3.0, Z_WALL), (3.0, -3.0, Z_WALL), (3.0, 3.0, Z_WALL), (-3.0, 3.0, Z_WALL)
    return np.array([[a, b, c], [a, c, d]], np.float32)


def deck_positions(n=N_CARDS, shear=0.0, seed=SEED):
    """((n + 2) * 3, 3) float32 vertex positions of the deck scene: the cards, then the wall's two triangles."""
    return np.concatenate([card_corners(n, shear, seed), _wall()]).reshape(-1, 3)


def deck_scene(n=N_CARDS, shear=0.0, seed=SEED):
    """The scene: triangles 0 .. n-1 are the cards (card 0 in front), n and n + 1 the wall."""
    pos = deck_positions(n, shear, seed)
    nt = n + 2
    vertices = np.zeros(nt * 3, dtype=T.VERTEX)
    vertices["position"] = pos
    triangles = np.zeros(nt, dtype=T.TRIANGLE)
    idx = np.arange(nt * 3, dtype=np.uint32).reshape(-1, 3)
    triangles["v0_index"], triangles["v1_index"], triangles["v2_index"] = idx[:, 0], idx[:, 1], idx[:, 2]
    mats = np.where(np.arange(n) % 8 == 7, MAT_METAL, MAT_CARD).astype(np.uint32)
    triangles["material_id"] = np.concatenate([mats, np.array([MAT_WALL, MAT_WALL], np.uint32)])
    materials = np.array([H.material_diffuse((0.7, 0.6, 0.5)), H.material_metallic((0.8, 0.8, 0.3), 0.2), H.material_diffuse((0.6, 0.7, 0.8)),
                          H.material_diffuse((0.8, 0.3, 0.3))], dtype=T.MATERIAL)
    spheres = np.array([((2.0, 0.3, -5.0), 0.6, MAT_BALL)], dtype=T.SPHERE)
    lights = np.array([H.light_point(LIGHT_POS, (1.0, 0.95, 0.9), 3.0), H.light_directional((-0.05, -0.08, -1.0), (0.6, 0.7, 1.0), 0.8)], dtype=T.LIGHT)
    name = f"deck{n}" + ("_sheared" if shear else "")
    return scenes.Scene(name, spheres, lights, vertices, triangles, materials, camera(), meta={"cards": n, "shear": shear})


def sheared(scene):
    """The deck scene with the sheared copy of its vertex positions (what the refit test uploads afresh)."""
    n = scene.meta["cards"]
    v = scene.vertices.copy()
    v["position"] = deck_positions(n, SHEAR)
    return dataclasses.replace(scene, vertices=v, name=scene.name + "_sheared", meta={"cards": n, "shear": SHEAR})


# ------------------------------------------------------------------------------------------------------------------------
# Ray sets
# ------------------------------------------------------------------------------------------------------------------------
def _region_points(rng, count, covered):
    """(count, 2) points of the square with |x|, |y| <= INSIDE and x + y <= -MARGIN (covered) or >= +MARGIN (the empty corner)."""
    out = np.zeros((0, 2))
    while len(out) < count:
        p = rng.uniform(-INSIDE, INSIDE, (4 * count, 2))
        s = p.sum(1)
        out = np.concatenate([out, p[(s <= -MARGIN) if covered else (s >= MARGIN)]])
    return out[:count]


def _batch(o, d):
    n = len(o)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = o, d
    rays[:, 3], rays[:, 7] = 1e-5, np.inf
    return rays


def _rays_between(p_front, p_back, from_back, lateral=1.0):
    """Unit rays through p_front (in the plane of card 0) and p_back (in the plane behind the last card); from_back (N,) bool: the
    origin lies behind the deck (between it and the wall) instead of in front.  lateral < 1 pulls p_back toward p_front (less oblique)."""
    a = np.concatenate([p_front, np.full((len(p_front), 1), Z_FRONT)], 1)
    b = np.concatenate([p_front + (p_back - p_front) * lateral, np.full((len(p_back), 1), Z_FRONT - Z_LENGTH)], 1)
    d = b - a
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o_front = a - d * (2.0 / -d[:, 2:3])                     # z = -1: two units in front of card 0
    o_back = b + d * (0.5 / -d[:, 2:3])                      # z = -7.5: between the deck and the wall
    fb = np.asarray(from_back, bool)[:, None]
    return _batch(np.where(fb, o_back, o_front), np.where(fb, -d, d))


def ray_set(kind, n=RECORDS, seed=SEED):
    rng = np.random.default_rng(seed + {"through": 1, "corner": 2, "mixed": 3, "crossing": 5}[kind])
    i = np.arange(n)
    if kind in ("through", "corner"):
        covered = kind == "through"
        return _rays_between(_region_points(rng, n, covered), _region_points(rng, n, covered), np.zeros(n, bool), lateral=0.25)
    if kind == "crossing":
        from_back = (i // 2) % 2 == 1
        cross = (i % 64) < MIXED_CORNER_LANES
        enters_covered, leaves_covered = ~cross, np.ones(n, bool)  # as the ray travels; p0 lies at the front, p1 at the back
        p0_covered, p1_covered = np.where(from_back, leaves_covered, enters_covered), np.where(from_back, enters_covered, leaves_covered)
        p0 = np.where(p0_covered[:, None], _region_points(rng, n, True), _region_points(rng, n, False))
        p1 = np.where(p1_covered[:, None], _region_points(rng, n, True), _region_points(rng, n, False))
        return _rays_between(p0, p1, from_back)
    covered = mixed_covered(n)
    p0 = np.where(covered[:, None], _region_points(rng, n, True), _region_points(rng, n, False))
    p1 = np.where(covered[:, None], _region_points(rng, n, True), _region_points(rng, n, False))
    return _rays_between(p0, p1, (i // 2) % 2 == 1)


def mixed_covered(n=RECORDS):
    """(n,) bool: which rays of "mixed" run through the covered half.  Half of the set through each region, but not half of each
    wave: of every 64 consecutive rays MIXED_CORNER_LANES (or 64 minus that many, in the second half of the set) run through the empty
    corner.  While fewer lanes than k_wf_trace's leaf threshold (24) hold a postponed leaf group the wave keeps taking node steps, so
    those lanes descend to the deepest level with a leaf group parked at every level on the way: the most a stack can hold."""
    i = np.arange(n)
    corner_lanes = np.where(i < n // 2, MIXED_CORNER_LANES, 64 - MIXED_CORNER_LANES)
    return (i % 64) >= corner_lanes



def camera_block_rays(bx, by, w=FRAME[0], h=FRAME[1]):
    """The 64 camera rays (pixel centres) of the 8x8 pixel block (bx, by) of the GPU tests' frame: one coherent wave."""
    import reference_cases as rc
    o, d = rc.camera_rays(camera(), w, h)
    blk = d[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].reshape(-1, 3)
    return _batch(np.broadcast_to(o, blk.shape), blk)


def points(n=RECORDS, n_cards=N_CARDS, seed=SEED):
    """(n, 3) float32 positions for the point queries, in turn: on a card, between two cards, in the empty corner, outside the deck."""
    rng = np.random.default_rng(seed + 4)
    i = np.arange(n)
    card = rng.integers(0, n_cards, n)
    z_card = Z_FRONT - Z_LENGTH * card / n_cards
    cov, emp = _region_points(rng, n, True), _region_points(rng, n, False)
    out = np.zeros((n, 3))
    out[:, :2] = np.where((i % 4 < 2)[:, None], cov, emp)
    out[:, 2] = np.where(i % 4 == 0, z_card, z_card - 0.5 * Z_LENGTH / n_cards)
    far = i % 4 == 3
    side = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([0.8, 0.8, 2.5]) + np.array([-2.0, 1.8, -5.0])
    out[far] = side[far]
    return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# The closed form's other half: how many cards a ray crosses (Moeller-Trumbore in float64, no range but t > tmin)
# ------------------------------------------------------------------------------------------------------------------------
def crossings(corners, rays, chunk=32):
    """Number of triangles of `corners` (n, 3, 3) each ray of the (N, 8) batch crosses at tmin < t < tmax."""
    c = np.asarray(corners, np.float64)
    v0, e1, e2 = c[:, 0][None], (c[:, 1] - c[:, 0])[None], (c[:, 2] - c[:, 0])[None]
    rays = np.asarray(rays, np.float64)
    out = np.zeros(len(rays), np.int64)
    for s0 in range(0, len(rays), chunk):
        r = rays[s0:s0 + chunk]
        o, d = r[:, None, 0:3], r[:, None, 4:7]
        hh = np.cross(d, e2)
        a = (e1 * hh).sum(-1)
        with np.errstate(all="ignore"):
            f = 1.0 / a
            s = o - v0
            u = f * (s * hh).sum(-1)
            q = np.cross(s, e1)
            v = f * (d * q).sum(-1)
            t = f * (e2 * q).sum(-1)
        hit = (np.abs(a) >= 1e-5) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > r[:, 3:4]) & (t < r[:, 7:8])
        out[s0:s0 + chunk] = hit.sum(1)
    return out
