"""Scenes whose extended-mode (mode 2) radiance has a closed form, and those closed forms in float64.

Every expectation here is derived from the prose of DESIGN.md section 5 (the numbered steps cited below), never from
oracle/rt_oracle.cpp or the library: neither is imported.  The tests run the CPU statement (test_estimator_oracle.py) and the
HIP kernels (test_gpu_estimator.py) through these scenes and compare with what this module computes.

Conventions.  sky = (0.1, 0.2, 0.3) (step 1).  Continuation and shadow segments start at P +- Nf * 1e-3 (steps 2, 4).  A frame
jitters its samples when spp > 1 or when it accumulates.  All images are (h, w, 3), y down, as the library stores them.

Bands.  `hoeffding_eps` / `bernstein_eps` give the half-width at a stated failure probability for a mean of independent samples
bounded in [0, M] (Hoeffding) or with a known variance (Bernstein); `f32_mean_slack` bounds what the f32 sample sum and the
division of step "Pixel = sum / spp" add.  None of them looks at the image under test.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from gpu_raytracer_amd import hostpack as H
from gpu_raytracer_amd import types as T
from gpu_raytracer_amd.scenes import Scene, _box, _Mesh

SKY = np.array([0.1, 0.2, 0.3])
ORIGIN_EPS = 1e-3          # WavefrontRay::t_min, the origin offset of steps 2 and 4
U32 = 2.0 ** -24           # unit roundoff of f32
GOLDEN = 0x9E3779B9        # sample stride of the seed rule
FAIL_P = 1e-9              # failure probability every statistical band is sized for


# ------------------------------------------------------------------------------------------------------------------------
# The sampler, restated from DESIGN section 5: seed = hash(frame_seed + x + y*W + s*0x9E3779B9), the hash one integer scramble
# (xor-shift 16, * 0x7FEB352D, xor-shift 15, * 0x846CA68B, xor-shift 16); SimpleRng: state = state * 1664525 + 1013904223,
# next_f32 = (state >> 8) / 2^24.
# ------------------------------------------------------------------------------------------------------------------------
def hash_u32(x):
    x = np.array(x, dtype=np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def seed_inputs(frame_seed, w, h, samples, mult=GOLDEN):
    """frame_seed + x + y*W + s*mult (mod 2^32) as uint32 of shape (len(samples), h, w)."""
    pix = np.arange(w * h, dtype=np.uint32).reshape(1, h, w)
    s = (np.asarray(samples, dtype=np.uint64) * np.uint64(mult) + np.uint64(frame_seed)) & np.uint64(0xFFFFFFFF)
    return s.astype(np.uint32).reshape(-1, 1, 1) + pix


class SimpleRng:
    def __init__(self, state):
        self.state = np.array(state, dtype=np.uint32, copy=True)

    def next_u32(self):
        self.state = self.state * np.uint32(1664525) + np.uint32(1013904223)
        return self.state

    def next_f32(self):
        return (self.next_u32() >> np.uint32(8)).astype(np.float64) / 16777216.0


def sample_rng(frame_seed, w, h, samples):
    return SimpleRng(hash_u32(seed_inputs(frame_seed, w, h, samples)))


def jitter(frame_seed, w, h, samples):
    """(jx, jy) of the global samples `samples`: the first two next_f32 of each (pixel, sample) stream; shape (n, h, w)."""
    rng = sample_rng(frame_seed, w, h, samples)
    jx = rng.next_f32()
    return jx, rng.next_f32()


def camera_rays(cam, w, h, jx, jy):
    """generate_camera_ray in float64 through the positions (x + jx, y + jy): origin (3,), unit directions (..., h, w, 3)."""
    px = np.arange(w, dtype=np.float64).reshape(1, w)
    py = np.arange(h, dtype=np.float64).reshape(h, 1)
    u = (px + jx) / w
    v = (py + jy) / h
    fov_scale = math.tan(float(cam["fov"]) * 0.5 * math.pi / 180.0)
    cx = (u * 2.0 - 1.0) * (w / h) * fov_scale
    cy = (1.0 - v * 2.0) * fov_scale
    fwd = np.asarray(cam["direction"], np.float64)
    up = np.asarray(cam["up"], np.float64)
    right = np.cross(fwd, up)
    true_up = np.cross(right, fwd)
    d = fwd + cx[..., None] * right + cy[..., None] * true_up
    return np.asarray(cam["position"], np.float64), d / np.linalg.norm(d, axis=-1, keepdims=True)


# f32 error of a camera direction against camera_rays: the pixel position (one add at magnitude <= W, one divide), cx / cy (three
# multiplies and an add), the two scaled basis vectors and two adds per component, the dot (five operations), sqrt, reciprocal and
# the final multiply are 16 roundings of at most 2^-24 relative on magnitudes <= 2 (fov <= 90 degrees, aspect 1, unit basis), and
# tanf is within 2 ulp: 32 * 2^-24 absolute per component.
CAMERA_DIR_F32_BOUND = 32 * U32


# ------------------------------------------------------------------------------------------------------------------------
# Bands
# ------------------------------------------------------------------------------------------------------------------------
def hoeffding_eps(m, n, p=FAIL_P):
    """Half-width t with P(|mean - mu| >= t) <= p for n independent samples in [0, m]."""
    return np.asarray(m, np.float64) * math.sqrt(math.log(2.0 / p) / (2.0 * n))


def bernstein_eps(var_sum, m, n, p=FAIL_P):
    """Half-width t of the mean with P(|mean - mu| >= t) <= p (Bernstein): n independent samples, sum of variances var_sum,
    |sample - its mean| <= m.  t solves t^2 n^2 / (2 (var_sum + m n t / 3)) = ln(2 / p)."""
    var_sum, m = np.asarray(var_sum, np.float64), np.asarray(m, np.float64)
    L = math.log(2.0 / p)
    b = m * L / 3.0
    return (b + np.sqrt(b * b + 2.0 * var_sum * L)) / n


def f32_mean_slack(m, spp):
    """What the f32 chain 'sum of spp samples in order, then / spp' can differ from the real mean by, samples in [0, m]:
    (spp - 1) additions and one division, each within 2^-24 of a partial sum <= spp * m; first-order bound with 1 % headroom."""
    return 1.01 * spp * U32 * np.asarray(m, np.float64)


def chi2_critical(dof, z=4.753424):
    """Upper critical value of chi-square with `dof` degrees of freedom by Wilson-Hilferty; z = 4.753424 is the standard normal
    quantile of 1 - 1e-6."""
    a = 2.0 / (9.0 * dof)
    return dof * (1.0 - a + z * math.sqrt(a)) ** 3


# ------------------------------------------------------------------------------------------------------------------------
# Segments that escape.  Step 1 accepts a hit only for t > 1e-5 (MIN_RAY_DISTANCE), so a continuation that starts within 1e-5
# (along its direction) of a second surface passes through it: in a closed box a vertex within s of an adjacent wall escapes when
# s < 1e-5 * w_n, w_n the direction's component toward that wall.  For vertices spread evenly over the unit box (24 face-edge
# adjacencies of length 1 over an area of 6) and a cosine lobe (E[max(w_n, 0)] = 2 / (3 pi)) that is 4 * 1e-5 * 0.21 = 8.5e-6 of
# the continuation segments.  SHARED EDGES: the triangle test is not watertight either; a ray within a few 2^-24 (relative to the
# triangle) of an edge two triangles share can miss both, about 3e-6 of the box's segments.  ESCAPE_CAP is twice the sum, rounded.
# The scenes below keep shared edges out of the camera's footprint where their geometry allows it.
# ------------------------------------------------------------------------------------------------------------------------
ESCAPE_CAP = 2e-5


def escapes_allowed(segments):
    return int(math.ceil(ESCAPE_CAP * segments))


# ------------------------------------------------------------------------------------------------------------------------
# Scene helpers
# ------------------------------------------------------------------------------------------------------------------------
def _quad(mesh, a, b, c, d, mat, normal):
    """Two triangles over the corners a-b-c-d (in order around the quad), wound so that normalize(cross(e1, e2)) = `normal`."""
    a, b, c, d = (np.asarray(p, np.float64) for p in (a, b, c, d))
    if np.dot(np.cross(b - a, c - a), normal) < 0:
        b, d = d, b
    mesh.add([a, b, c, d], [(0, 1, 2), (0, 2, 3)], mat)


def _scene(name, mesh, materials, cam, lights=()):
    vertices, triangles = mesh.finish()
    lights = np.array(list(lights), dtype=T.LIGHT) if len(lights) else np.zeros(0, T.LIGHT)
    return Scene(name, np.zeros(0, T.SPHERE), lights, vertices, triangles, np.array(materials, dtype=T.MATERIAL), cam)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


@dataclass
class Case:
    name: str
    scene: Scene
    w: int
    h: int
    bounces: int
    frame_seed: int = 0
    info: dict = field(default_factory=dict)

    def rays(self, samples):
        """Float64 camera rays of the jittered global samples `samples`: origin, directions (n, h, w, 3)."""
        jx, jy = jitter(self.frame_seed, self.w, self.h, samples)
        return camera_rays(self.scene.camera, self.w, self.h, jx, jy)


# ------------------------------------------------------------------------------------------------------------------------
# 1. Furnace
# ------------------------------------------------------------------------------------------------------------------------
FURNACE_RHO = np.array([0.5, 0.25, 0.8])
FURNACE_E = np.array([0.3, 0.6, 0.2])


def furnace(bounces, w=64, h=64):
    """Camera inside a closed unit box of one emissive-diffuse material (albedo rho, emission E), no lights.

    Every segment hits the box.  Step 2 gives a non-terminal vertex the direct light E (no lights, no ambient) and the terminal
    one E + 0.1 rho; step 3 adds it times the throughput; step 4 multiplies the throughput by rho; step 5 divides it by the
    survival probability, which leaves its expectation alone.  So E[sample] = sum_{k<B} E rho^k + rho^B (E + 0.1 rho), and for
    B <= 2 (roulette starts at the third vertex, and only a non-terminal vertex continues) every sample IS that value.

    Rejects: roulette without the division (vertices 3.. lose the factor p), roulette from the second vertex (B = 2 stops being
    deterministic), emission or ambient at the wrong vertices, an albedo applied twice, and for B > 8 a path that ends where the
    queue pipeline first reads back its live paths (furnace_ends_at_first_poll: blue misses about 0.13 (1 - 0.8^(B-8))).

    Per-sample bound: after step 5 the throughput's largest channel is at most 1 (it is t / clamp(max t, 0.05, 1)), before it the
    throughput is rho^k <= 1, so a sample is at most (B + 1) E + 0.1 rho per channel."""
    mesh = _Mesh()
    mesh.add(*_box((0, 0, 0), (1, 1, 1)), 0)
    mat = H.material_new(tuple(FURNACE_RHO), 0.0, 1.0, tuple(FURNACE_E), 1.5, 0.0)
    cam = H.camera((0.37, 0.45, 0.81), tuple(_unit((0.2, -0.1, -1.0))), (0.0, 1.0, 0.0), 70.0)
    return Case(f"furnace_b{bounces}", _scene("furnace", mesh, [mat], cam), w, h, bounces)


def furnace_expected(bounces):
    rho, e = FURNACE_RHO, FURNACE_E
    return sum(e * rho ** k for k in range(bounces)) + rho ** bounces * (e + 0.1 * rho)


def furnace_sample_max(bounces):
    return (bounces + 1) * FURNACE_E + 0.1 * FURNACE_RHO


def furnace_no_reweight(bounces):
    """The same estimator with step 5's division left out: vertex k >= 3 is reached with the product of the survival
    probabilities p_j = clamp(max(rho^(j+1)), 0.05, 1) of vertices j = 2 .. k-1 and nothing makes up for it."""
    rho, e = FURNACE_RHO, FURNACE_E
    total, reach = np.zeros(3), 1.0
    for k in range(bounces + 1):
        term = e + 0.1 * rho if k == bounces else e
        total = total + reach * rho ** k * term
        if k >= 2:
            reach *= min(max(float((rho ** (k + 1)).max()), 0.05), 1.0)
    return total


def furnace_ends_at_first_poll(bounces):
    """The same estimator on a pipeline that loses every path still alive when it first reads back its live paths, after the
    bounce iteration that shades vertex 7 and hands on to vertex 8 (B > 8): vertices 0 .. 8 are as they should be - vertex 8 has its
    record written before the read - and a path that reaches vertex 8 contributes nothing further: sum_{k<=8} E rho^k."""
    rho, e = FURNACE_RHO, FURNACE_E
    return sum(e * rho ** k for k in range(min(bounces, 8) + 1))


def furnace_f32_rel_bound(bounces, spp):
    """Relative f32 error of a deterministic furnace pixel: a sample is B + 1 products 'light * throughput' (k - 1 roundings in
    the throughput rho^k, two in E + 0.1 rho, one in the product: at most B + 2 each) added in B + 1 additions; the pixel adds
    spp samples and divides.  All terms are positive, so the relative errors add: ((B + 1)(B + 3) + spp + 1) * 2^-24, and the
    f32 representation of rho and E themselves (0.5 and 0.25 are exact, the others within 2^-24, entering up to B + 1 times)."""
    return ((bounces + 1) * (bounces + 3) + spp + 1 + (bounces + 2)) * U32


# ------------------------------------------------------------------------------------------------------------------------
# 2. Sky visibility past a wall
# ------------------------------------------------------------------------------------------------------------------------
WALL_RHO = np.array([0.6, 0.9, 0.3])
WALL_HEIGHT = 1.0
WALL_HALF_LENGTH = 1.0e4
# name: (side the camera is on, direction away from the wall, wall's long axis, geometric normal of the floor)
WALL_LAYOUTS = {
    "wall_along_z": ((0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0)),
    "wall_along_x_backface": ((0, 1, 0), (0, 0, 1), (1, 0, 0), (0, -1, 0)),   # floor seen from behind: Nf = -N
    "from_below": ((0, -1, 0), (-1, 0, 0), (0, 0, 1), (0, -1, 0)),           # floor facing -y, camera under it
}


def sky_wall(layout, w=128, h=128):
    """A diffuse floor (albedo rho) in the plane y = 0 and a black wall of height 1 standing on it along a line, +-1e4 long;
    no lights, B = 1; the camera looks straight at the floor from the wall's side.

    Step 3 adds nothing at the floor (no light, no emission, no ambient at a non-terminal vertex); step 4 continues from
    O = P + Nf 1e-3 along normalize(Nf + unit vector), whose density is cos(theta) / pi about Nf; the segment either reaches the sky
    (step 1: rho * sky) or the wall, whose terminal shading 0.1 * 0 + 0 is black.  With x the floor point's distance from the wall,
    the wall covers the wedge between the horizontal plane through O and the plane through O and the wall's top edge, of dihedral
    angle beta = atan((1 - 1e-3) / x).  Projected on the base disc (Nusselt) that wedge is the half disc minus half an ellipse of
    semi-axis cos(beta): the blocked cosine-weighted share is F = (1 - cos beta) / 2 and E[sample] = rho sky (1 - F).
    The wall's finite length leaves out directions within x / D of its axis and below elevation 1 / D, D > 9990: a share below
    (2 / pi)(1 / D)^2 (x / D) < 1e-11, inside WALL_FORM_SLACK.

    Rejects: a lobe that is not cosine-weighted (a uniform hemisphere blocks beta / pi), a unit vector that is not uniform (the
    three layouts put the wall along z, along x and under the floor, so no axis of the sampler is hidden by symmetry), a normal
    that is not face-forwarded (the second layout's floor is seen from behind)."""
    side, away, axis, normal = (np.array(v, np.float64) for v in WALL_LAYOUTS[layout])
    mesh = _Mesh()
    c = lambda x, z: away * x + axis * z  # noqa: E731  floor coordinates -> world
    _quad(mesh, c(0.25, -40), c(8, -40), c(8, 4), c(0.25, 4), 0, normal)  # diagonal a-c clear of the footprint (SHARED EDGES)
    L = WALL_HALF_LENGTH
    _quad(mesh, c(0, -L), c(0, L), c(0, L) + side * WALL_HEIGHT, c(0, -L) + side * WALL_HEIGHT, 1, away)
    mats = [H.material_diffuse(tuple(WALL_RHO)), H.material_diffuse((0.0, 0.0, 0.0))]
    cam = H.camera(tuple(c(2.5, 0.3) + side * 6.0), tuple(-side), tuple(_unit(away * 0.8 + axis * 0.6)), 30.0)
    return Case(f"sky_{layout}", _scene("sky_wall", mesh, mats, cam), w, h, 1, info={"layout": layout})


WALL_FORM_SLACK = 1e-9


def sky_wall_distance(case, samples):
    """Distance x of every sample's floor point from the wall, float64, (n, h, w)."""
    side, away, _, _ = (np.array(v, np.float64) for v in WALL_LAYOUTS[case.info["layout"]])
    o, d = case.rays(samples)
    t = -np.dot(o, side) / (d @ side)
    return (o + d * t[..., None]) @ away


def sky_wall_blocked(case, samples):
    """Blocked share of every sample's lobe, (n, h, w): (cosine-weighted: the estimator of step 4, uniform hemisphere: the wrong
    alternative)."""
    x = sky_wall_distance(case, samples)
    beta = np.arctan((WALL_HEIGHT - ORIGIN_EPS) / x)
    return 0.5 * (1.0 - np.cos(beta)), beta / math.pi


# ------------------------------------------------------------------------------------------------------------------------
# 3. Transmission branch and hero channel
# ------------------------------------------------------------------------------------------------------------------------
GLASS_A = np.array([0.9, 0.6, 0.7])
GLASS_E = np.array([0.2, 0.1, 0.4])
FLOOR_RHO = np.array([0.4, 0.7, 0.5])
FLOOR_E = np.array([0.5, 0.3, 0.9])
_DOWN_CAM = dict(position=(0.1, 5.0, -0.2), direction=(0.0, -1.0, 0.0), up=(0.0, 0.0, -1.0), fov=20.0)


def _glass_quad_and_floor(mesh):
    # both diagonals (a-c) pass far from the camera's footprint around (0.1, -0.2): see SHARED EDGES
    _quad(mesh, (-2, 1, -2), (2, 1, -2), (2, 1, 10), (-2, 1, 10), 0, (0, 1, 0))
    _quad(mesh, (-50, 0, -30), (50, 0, -30), (50, 0, 70), (-50, 0, 70), 1, (0, 1, 0))


def glass_over_black_floor(transmission, w=128, h=128):
    """A glass quad (transmission T, albedo a, emission Eg, not metallic) at y = 1 over a black diffuse floor, under the sky;
    camera above, looking down, B = 2.

    At the quad step 3 adds Eg (1 - T).  Step 4 transmits with probability T: the segment reaches the black floor, whose albedo 0
    ends all further contribution.  Otherwise (probability 1 - T) it leaves diffusely into the upper half space, throughput a,
    where nothing but the sky is: a sky.  E[sample] = (1 - T)(Eg + a sky); at T = 1 every sample is exactly 0.

    Rejects: an inverted branch (`u >= T` transmits: (1 - T) Eg + T a sky), a missing (1 - T) on the reflective share
    (Eg + (1 - T) a sky)."""
    mesh = _Mesh()
    _glass_quad_and_floor(mesh)
    mats = [H.material_new(tuple(GLASS_A), 0.0, 0.0, tuple(GLASS_E), 1.5, transmission), H.material_diffuse((0.0, 0.0, 0.0))]
    return Case(f"glass_T{transmission}", _scene("glass_black", mesh, mats, H.camera(**_DOWN_CAM)), w, h, 2, info={"T": transmission})


def glass_black_expected(t, variant="right"):
    """-> (mean, per-sample variance, per-sample maximum)."""
    a_sky = GLASS_A * SKY
    if variant == "inverted_branch":
        return (1 - t) * GLASS_E + t * a_sky, None, None
    if variant == "no_one_minus_t":
        return GLASS_E + (1 - t) * a_sky, None, None
    return (1 - t) * (GLASS_E + a_sky), a_sky ** 2 * t * (1 - t), (1 - t) * GLASS_E + a_sky


def glass_over_emissive_floor(w=128, h=128):
    """The same quad with T = 1 (no emission) over an emissive diffuse floor (albedo rf, emission Ef), B = 1: step 4 always
    transmits, picks the hero channel c uniformly and sets throughput = 3 a_c e_c; the floor is the terminal vertex, shaded
    Ef + 0.1 rf.  A sample is 3 a_c (Ef + 0.1 rf)_c in channel c (probability 1/3) and 0 in the others: E = a (Ef + 0.1 rf).

    Rejects: a hero factor other than 3 (factor 2: two thirds of it), a channel pick that is not uniform over {0, 1, 2}
    (`u * 2`: 1.5 x red and green, no blue)."""
    mesh = _Mesh()
    _glass_quad_and_floor(mesh)
    mats = [H.material_new(tuple(GLASS_A), 0.0, 0.0, (0, 0, 0), 1.5, 1.0), H.material_emissive(tuple(FLOOR_RHO), tuple(FLOOR_E))]
    return Case("glass_hero", _scene("glass_emissive", mesh, mats, H.camera(**_DOWN_CAM)), w, h, 1)


def hero_expected(full, variant="right"):
    """Mean, per-sample variance and maximum of '3 * full_c with probability 1/3' per channel; the wrong alternatives' means."""
    if variant == "factor2":
        return full * 2.0 / 3.0, None, None
    if variant == "two_channels":
        return full * np.array([1.5, 1.5, 0.0]), None, None
    return full, (3.0 * full) ** 2 * (1.0 / 3.0) * (2.0 / 3.0), 3.0 * full


GLASS_HERO_FULL = GLASS_A * (FLOOR_E + 0.1 * FLOOR_RHO)
SLAB_FULL = GLASS_A ** 2 * SKY


def glass_slab(w=128, h=128):
    """A closed slab (box, 0.2 thick) of the T = 1 glass under the sky, nothing below it, B = 2: two transmissions, each
    multiplying the throughput by a, the hero channel chosen at the first only; the third segment meets the sky.
    E = a^2 sky per channel.  The camera's rays are within 10 degrees of the slab's normal: far from total internal reflection
    (sin^2 = 1.535^2 * 0.03 < 1) and from the slab's sides."""
    mesh = _Mesh()
    lo, hi = np.array([-2.0, 1.0, -2.0]), np.array([2.0, 1.2, 10.0])
    for axis in range(3):  # six quads; the large faces' diagonals clear of the footprint (SHARED EDGES)
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        for side, val in ((-1.0, lo[axis]), (1.0, hi[axis])):
            corners = []
            for c1, c2 in ((lo[a1], lo[a2]), (hi[a1], lo[a2]), (hi[a1], hi[a2]), (lo[a1], hi[a2])):
                p = np.zeros(3)
                p[axis], p[a1], p[a2] = val, c1, c2
                corners.append(p)
            n = np.zeros(3)
            n[axis] = side
            _quad(mesh, *corners, 0, n)
    mats = [H.material_new(tuple(GLASS_A), 0.0, 0.0, (0, 0, 0), 1.5, 1.0)]
    return Case("glass_slab", _scene("glass_slab", mesh, mats, H.camera(**_DOWN_CAM)), w, h, 2)


# ------------------------------------------------------------------------------------------------------------------------
# 4. Mirror
# ------------------------------------------------------------------------------------------------------------------------
MIRROR_A = np.array([0.9, 0.7, 0.5])
MIRROR_WALL = dict(z=-3.0, half_width=1.5, height=7.0)
MIRROR_MARGIN = 1e-4   # a sample whose reflected segment passes this close to the wall's outline is not classified (f32 error ~1e-6)


def mirror(roughness=0.0, w=128, h=128):
    """A metallic floor (albedo a, roughness 0) in front of a black wall under the sky, B = 1.  Step 4's metallic branch
    continues along the mirror direction r = d - 2 (d . Nf) Nf from P + Nf 1e-3 with throughput a; the segment meets the black
    wall (0) or the sky (a sky).  Each sample is classified in float64 by reflecting its camera ray."""
    mesh = _Mesh()
    _quad(mesh, (-10, 0, -10), (10, 0, -10), (10, 0, 50), (-10, 0, 50), 0, (0, 1, 0))
    z, hw, ht = MIRROR_WALL["z"], MIRROR_WALL["half_width"], MIRROR_WALL["height"]
    _quad(mesh, (-hw, 0, z), (hw, 0, z), (hw, ht, z), (-hw, ht, z), 1, (0, 0, 1))
    mats = [H.material_metallic(tuple(MIRROR_A), roughness), H.material_diffuse((0.0, 0.0, 0.0))]
    cam = H.camera((0.2, 3.0, 3.0), tuple(_unit((0.0, -1.0, -0.6))), (0.0, 1.0, 0.0), 40.0)
    return Case("mirror", _scene("mirror", mesh, mats, cam), w, h, 1)


def mirror_classify(case, samples):
    """-> (sees_sky, unsure), bool (n, h, w): whether the reflected segment of each sample reaches the sky, and whether it passes
    within MIRROR_MARGIN of the wall's outline."""
    o, d = case.rays(samples)
    n = np.array([0.0, 1.0, 0.0])
    t = -o[1] / d[..., 1]
    p = o + d * t[..., None]
    r = d - 2.0 * (d @ n)[..., None] * n
    org = p + n * ORIGIN_EPS
    s = (MIRROR_WALL["z"] - org[..., 2]) / r[..., 2]
    q = org + r * s[..., None]
    dx = MIRROR_WALL["half_width"] - np.abs(q[..., 0])
    dy = np.minimum(q[..., 1], MIRROR_WALL["height"] - q[..., 1])
    inside = (dx > 0) & (dy > 0) & (s > 0)
    unsure = (np.minimum(np.abs(dx), np.abs(dy)) < MIRROR_MARGIN) & (np.minimum(dx, dy) > -MIRROR_MARGIN)
    return ~inside, unsure


def mirror_f32_rel_bound(spp):
    """a * sky: one rounding in the throughput 1 * a, one in the product, spp additions, one division, and the f32
    representation of a and sky (two more)."""
    return (spp + 5) * U32


# ------------------------------------------------------------------------------------------------------------------------
# 5. Direct light and hard shadow
# ------------------------------------------------------------------------------------------------------------------------
LIT_RHO = np.array([0.7, 0.5, 0.3])
LIGHT_COLOR = np.array([1.0, 0.9, 0.8])
LIGHT_INTENSITY = 2.0
POINT_LIGHT_POS = np.array([0.3, 3.0, -0.2])
DIRECTIONAL_DIR = np.array([0.3, -1.0, 0.2])   # the way the light travels
OCCLUDER = dict(y=1.0, half=0.5)
SHADOW_MARGIN = 1e-4


def direct_light(kind, w=64, h=64):
    """A diffuse floor (albedo rho, geometric normal +y) under one light, a black square occluder at y = 1 between them, B = 0.
    kind = "point": a point light at y = 3 and a black ceiling at y = 5 ABOVE the light, which a shadow segment longer than the
    distance to the light would meet.  kind = "directional": a light travelling along DIRECTIONAL_DIR, no ceiling.

    Step 2, restated in float64 in `direct_light_expected`: l = direction to the light; point: d = |L - P|,
    att = f16(1 / (1 + 0.01 d^2)); intensity = max(N . l, 0) * I * att (directional: no att, l = -normalize(direction));
    BRDF of a dielectric = albedo / pi * intensity; times the light's colour; visible unless the segment from P + N 1e-3 along l
    meets something before the light (directional: at all).  The vertex is terminal: + 0.1 rho."""
    mesh = _Mesh()
    _quad(mesh, (-6, 0, -6), (6, 0, -6), (6, 0, 30), (-6, 0, 30), 0, (0, 1, 0))
    y, hf = OCCLUDER["y"], OCCLUDER["half"]
    _quad(mesh, (-hf, y, -hf), (hf, y, -hf), (hf, y, hf), (-hf, y, hf), 1, (0, 1, 0))
    if kind == "point":
        _quad(mesh, (-6, 5, -6), (6, 5, -6), (6, 5, 6), (-6, 5, 6), 1, (0, -1, 0))
        light = H.light_point(tuple(POINT_LIGHT_POS), tuple(LIGHT_COLOR), LIGHT_INTENSITY)
    else:
        light = H.light_directional(tuple(DIRECTIONAL_DIR), tuple(LIGHT_COLOR), LIGHT_INTENSITY)
    mats = [H.material_diffuse(tuple(LIT_RHO)), H.material_diffuse((0.0, 0.0, 0.0))]
    cam = H.camera((0.1, 4.5, 0.05), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0), 50.0)
    return Case(f"direct_{kind}", _scene("direct_light", mesh, mats, cam, [light]), w, h, 0, info={"kind": kind})


def _in_square(q, half):
    d = half - np.maximum(np.abs(q[..., 0]), np.abs(q[..., 2]))
    return d > 0, np.abs(d) < SHADOW_MARGIN


def direct_light_expected(case, samples, variant="right"):
    """-> (per-sample radiance (n, h, w, 3), unsure (n, h, w)).  variant "shadow_below": the shadow segment starts at P - N 1e-3
    (the floor itself occludes everything); "not_negated": the directional light's direction used as it is (N . l < 0: no light)."""
    o, d = case.rays(samples)
    n = np.array([0.0, 1.0, 0.0])
    # what the camera ray meets first: the occluder's top (black: 0) or the floor
    tq = (OCCLUDER["y"] - o[1]) / d[..., 1]
    on_occluder, unsure = _in_square(o + d * tq[..., None], OCCLUDER["half"])
    p = o + d * (-o[1] / d[..., 1])[..., None]
    if case.info["kind"] == "point":
        to_light = POINT_LIGHT_POS - p
        dist = np.linalg.norm(to_light, axis=-1)
        l = to_light / dist[..., None]
        with np.errstate(over="ignore"):
            att = (1.0 / (1.0 + dist * dist * 0.01)).astype(np.float16).astype(np.float64)
    else:
        l = np.broadcast_to(-_unit(DIRECTIONAL_DIR), p.shape)
        att = 1.0
        if variant == "not_negated":
            l = -l
    intensity = np.maximum(l @ n, 0.0) * LIGHT_INTENSITY * att
    lit = LIT_RHO / math.pi * intensity[..., None] * LIGHT_COLOR
    # shadow segment from P + N eps along l: where it crosses the occluder's plane (always before the light, which is at y = 3)
    org = p + n * ORIGIN_EPS
    s = (OCCLUDER["y"] - org[..., 1]) / l[..., 1]
    shadowed, edge = _in_square(org + l * s[..., None], OCCLUDER["half"])
    if variant == "shadow_below":
        shadowed = np.ones_like(shadowed)
    rad = 0.1 * LIT_RHO + np.where(shadowed[..., None], 0.0, lit)
    rad = np.where(on_occluder[..., None], 0.0, rad)
    return rad, unsure | (edge & ~on_occluder)


# ------------------------------------------------------------------------------------------------------------------------
# 6. Seed collisions
# ------------------------------------------------------------------------------------------------------------------------
def seed_collisions(w, h, spp, mult=GOLDEN):
    """Pairs of (pixel, sample) that share a seed, in closed form: inputs p + s * mult collide when the pixel offset equals
    ds * mult (mod 2^32, as a signed residue) and is smaller than the frame; the hash is a bijection of u32.
    -> (pairs, [(ds, |offset|, pixel pairs, samples shared by each), ...])."""
    ds = np.arange(1, spp, dtype=np.uint64)
    off = (ds * np.uint64(mult)) & np.uint64(0xFFFFFFFF)
    mag = np.minimum(off, np.uint64(1 << 32) - off).astype(np.int64)
    hit = mag < w * h
    rows = [(int(d), int(m), w * h - int(m), spp - int(d)) for d, m in zip(ds[hit], mag[hit])]
    return sum(r[2] * r[3] for r in rows), rows


def seed_collisions_brute_force(w, h, spp, mult=GOLDEN, frame_seed=0):
    """The same count by hashing every (pixel, sample) and sorting the seeds."""
    seeds = np.sort(hash_u32(seed_inputs(frame_seed, w, h, np.arange(spp), mult)).ravel())
    _, counts = np.unique(seeds, return_counts=True)
    counts = counts.astype(np.int64)
    return int((counts * (counts - 1) // 2).sum())


# ------------------------------------------------------------------------------------------------------------------------
# The assertions, shared by the CPU and the GPU file: each takes the (h, w, 3) float32 image of whatever rendered the case, prints
# its figures, then asserts.  Nothing here takes a variance, a bound or an expectation from the image.
# ------------------------------------------------------------------------------------------------------------------------
def _image_mean(rgb):
    return np.asarray(rgb, np.float64).reshape(-1, 3).mean(0)


def _assert_mean(label, rgb, mu, eps, alternatives):
    """|image mean - mu| <= eps per channel, and eps at most half the distance to every named wrong alternative in the channel
    that separates it best."""
    mean = _image_mean(rgb)
    print(f"{label}: mean {mean}, expected {mu}, band {eps}")
    for name, alt in alternatives.items():
        gap = np.abs(np.asarray(alt) - mu)
        ch = int(np.argmax(gap / eps))
        print(f"  alternative {name}: {alt}, distance {gap}, separating channel {ch}")
        assert eps[ch] <= 0.5 * gap[ch], f"{label}: band {eps[ch]} too wide to reject '{name}' (distance {gap[ch]})"
    assert (np.abs(mean - mu) <= eps).all(), f"{label}: mean {mean}, expected {mu}, band {eps}"


def check_furnace(rgb, case, spp, continuation=None):
    """B <= 2: every pixel is the closed form within furnace_f32_rel_bound, except at most escapes_allowed pixels (a path that
    escaped; `continuation`, the frame's continuation-segment count, may not miss more segments than that).  B >= 3: the image mean."""
    b, n = case.bounces, case.w * case.h * spp
    mu = furnace_expected(b)
    if b <= 2:
        rel = np.abs(np.asarray(rgb, np.float64) / mu - 1.0).max(-1)
        bound, allowed = furnace_f32_rel_bound(b, spp), escapes_allowed(n * b)
        off = int((rel > bound).sum())
        print(f"{case.name}: largest relative error {np.sort(rel.ravel())[-1 - off:][0]:.3e} outside {off} pixels, bound {bound:.3e}, "
              f"pixels off {off}, allowed {allowed}")
        assert off <= allowed
        if continuation is not None:
            escaped = n * b - continuation
            print(f"{case.name}: paths that escaped before their last segment {escaped}")
            assert 0 <= escaped <= off  # each of them shows as a pixel that is off (an escape at the last segment only shows there)
        return
    m = furnace_sample_max(b)
    eps = hoeffding_eps(m, n) + f32_mean_slack(m, spp) + ESCAPE_CAP * b * m
    alternatives = {"no division by p": furnace_no_reweight(b)}
    if b > 8:
        alternatives["paths end at the first poll"] = furnace_ends_at_first_poll(b)
    _assert_mean(case.name, rgb, mu, eps, alternatives)


_SKY_WALL_CACHE = {}


def sky_wall_moments(case, spp, chunk=32):
    """(expected image mean, the uniform-hemisphere alternative's, sum of the per-sample variances) per channel for samples 0..spp-1."""
    key = (case.name, case.w, case.h, spp)
    if key not in _SKY_WALL_CACHE:
        vis = alt = var = 0.0
        for s0 in range(0, spp, chunk):
            f_cos, f_uni = sky_wall_blocked(case, np.arange(s0, min(s0 + chunk, spp)))
            vis += (1.0 - f_cos).sum()
            alt += (1.0 - f_uni).sum()
            var += (f_cos * (1.0 - f_cos)).sum()
        full, n = WALL_RHO * SKY, case.w * case.h * spp
        _SKY_WALL_CACHE[key] = (full * vis / n, full * alt / n, full ** 2 * var)
    return _SKY_WALL_CACHE[key]


def check_sky_wall(rgb, case, spp):
    mu, alt, var_sum = sky_wall_moments(case, spp)
    full, n = WALL_RHO * SKY, case.w * case.h * spp
    eps = bernstein_eps(var_sum, full, n) + f32_mean_slack(full, spp) + (ESCAPE_CAP + WALL_FORM_SLACK) * full
    _assert_mean(case.name, rgb, mu, eps, {"uniform hemisphere": alt})


def check_glass_black(rgb, case, spp):
    t, n = case.info["T"], case.w * case.h * spp
    mu, var, m = glass_black_expected(t)
    if t >= 1.0:
        print(f"{case.name}: largest pixel {np.abs(rgb).max()}, expected exactly 0")
        assert not np.asarray(rgb).any()
        return
    eps = bernstein_eps(var * n, GLASS_A * SKY, n) + f32_mean_slack(m, spp) + ESCAPE_CAP * 2 * m
    _assert_mean(case.name, rgb, mu, eps, {"inverted branch": glass_black_expected(t, "inverted_branch")[0],
                                           "no (1 - T)": glass_black_expected(t, "no_one_minus_t")[0]})


def check_hero(rgb, case, spp):
    full = GLASS_HERO_FULL if case.name == "glass_hero" else SLAB_FULL
    n = case.w * case.h * spp
    mu, var, m = hero_expected(full)
    eps = bernstein_eps(var * n, m, n) + f32_mean_slack(m, spp) + ESCAPE_CAP * case.bounces * m
    _assert_mean(case.name, rgb, mu, eps, {"hero factor 2": hero_expected(full, "factor2")[0],
                                           "two channels": hero_expected(full, "two_channels")[0]})


EDGE_SHARE_CAP = 0.02


def check_mirror(rgb, case, spp):
    """Pure pixels (every sample's reflection on one side of the wall's outline) are a * sky or 0 within the f32 bound; the pixels
    left out (mixed or unsure) are at most 2 % of the frame.  Then the mixed pixels too: k of spp samples see the sky, so the pixel
    is a sky k / spp - which only holds if the jitter is the restated one (the sampler's tie to the statement)."""
    sees_sky, unsure = mirror_classify(case, np.arange(spp))
    k, unsure = sees_sky.sum(0), unsure.any(0)
    pure = ((k == 0) | (k == spp)) & ~unsure
    left_out = 1.0 - pure.mean()
    full = MIRROR_A * SKY
    tol = mirror_f32_rel_bound(spp) * full
    err = np.abs(np.asarray(rgb, np.float64) - (k / spp)[..., None] * full)
    print(f"{case.name}: left out {left_out:.4f} of the frame (cap {EDGE_SHARE_CAP}), sky pixels {(k == spp).mean():.3f}, wall pixels "
          f"{(k == 0).mean():.3f}, mixed {((k > 0) & (k < spp)).sum()}, unsure {unsure.sum()}, largest error pure {err[pure].max(0)}, "
          f"mixed {err[~unsure].max(0)}, tolerance {tol}")
    assert left_out <= EDGE_SHARE_CAP
    assert (k == 0).mean() > 0.1 and (k == spp).mean() > 0.1   # both sides are in the frame
    assert (err[pure] <= tol).all()
    assert ((k > 0) & (k < spp) & ~unsure).sum() >= 16 and (err[~unsure] <= tol).all()


def check_direct_light(rgb, case, spp):
    """Every classified pixel within 2^-10 relative of the float64 restatement (f16 attenuation: 2^-11, the f32 chain a few 2^-24);
    pixels with a sample within SHADOW_MARGIN of the occluder's outline or its shadow's are left out, at most 2 % of the frame."""
    rad, unsure = direct_light_expected(case, np.arange(spp))
    want, unsure = rad.mean(0), unsure.any(0)
    got = np.asarray(rgb, np.float64)
    tol = 2.0 ** -10 * want
    err = np.abs(got - want)
    lit = want[..., 0] > 0.1 * LIT_RHO[0] * (1 + 1e-9)
    print(f"{case.name}: left out {unsure.mean():.4f} (cap {EDGE_SHARE_CAP}), lit pixels {(lit & ~unsure).sum()}, shadowed "
          f"{((want[..., 0] > 0) & ~lit & ~unsure).sum()}, occluder {(want[..., 0] == 0).sum()}, "
          f"largest relative error on lit pixels {(err[lit & ~unsure] / want[lit & ~unsure]).max():.3e}, tolerance {2.0 ** -10:.3e}")
    assert unsure.mean() <= EDGE_SHARE_CAP
    assert (lit & ~unsure).mean() > 0.5 and ((want[..., 0] > 0) & ~lit & ~unsure).sum() > 50
    assert (err[~unsure] <= tol[~unsure]).all()
    # the wrong alternatives this rejects, each further from `want` than the tolerance on most of the frame
    for variant in ("shadow_below",) + (("not_negated",) if case.info["kind"] == "directional" else ()):
        alt = direct_light_expected(case, np.arange(spp), variant)[0].mean(0)
        share = (np.abs(alt - want) > 2 * tol)[~unsure].all(-1).mean()
        print(f"  alternative {variant}: differs by more than twice the tolerance on {share:.3f} of the frame")
        assert share > 0.5
