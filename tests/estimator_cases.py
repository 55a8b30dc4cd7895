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

    def centre_rays(self):
        """Float64 camera rays through the pixel centres, which a closed frame with spp = 1 uses: origin, directions (h, w, 3)."""
        return camera_rays(self.scene.camera, self.w, self.h, 0.5, 0.5)


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
    meets something before the light (directional: at all).  The vertex is terminal: + 0.1 rho.

    The kinds with two lights put that scene under a spot light at the point light's place, aimed along SPOT_DIR, and a second point
    light at POINT2_LIGHT_POS with a colour and an intensity of its own; the occluder's two shadows (around (-0.15, 0.1) and
    (1.0, -0.67), each about 1.5 wide) overlap in a corner only, so most shadowed pixels keep one of the two lights.  A spot light
    is the point light times max(dot(-normalize(direction), l), 0); its range and cone angles are never read (the scene gives them
    values that would darken the floor if they were).  The lights are summed in their order, each gated on its own.
    "spot_and_point": the diffuse floor.  "metallic_two_lights": a metallic floor, whose BRDF is albedo * intensity * 0.5.
    "backface": the diffuse floor with the geometric normal -y: N . l < 0 for both lights, step 2 uses the unflipped normal, so every
    floor pixel is the ambient term alone and no light has a contribution to gate."""
    mesh = _Mesh()
    _quad(mesh, (-6, 0, -6), (6, 0, -6), (6, 0, 30), (-6, 0, 30), 0, (0, -1, 0) if kind == "backface" else (0, 1, 0))
    y, hf = OCCLUDER["y"], OCCLUDER["half"]
    _quad(mesh, (-hf, y, -hf), (hf, y, -hf), (hf, y, hf), (-hf, y, hf), 1, (0, 1, 0))
    if kind != "directional":
        _quad(mesh, (-6, 5, -6), (6, 5, -6), (6, 5, 6), (-6, 5, 6), 1, (0, -1, 0))
    if kind == "point":
        lights = [H.light_point(tuple(POINT_LIGHT_POS), tuple(LIGHT_COLOR), LIGHT_INTENSITY)]
    elif kind == "directional":
        lights = [H.light_directional(tuple(DIRECTIONAL_DIR), tuple(LIGHT_COLOR), LIGHT_INTENSITY)]
    else:
        assert kind in TWO_LIGHT_KINDS, kind
        lights = [H.light_spot(tuple(POINT_LIGHT_POS), tuple(SPOT_DIR), tuple(LIGHT_COLOR), LIGHT_INTENSITY, 0.5, 0.01, 0.02),
                  H.light_point(tuple(POINT2_LIGHT_POS), tuple(LIGHT2_COLOR), LIGHT2_INTENSITY, rng=0.5)]
    floor = H.material_metallic(tuple(LIT_RHO), 1.0) if kind == "metallic_two_lights" else H.material_diffuse(tuple(LIT_RHO))
    mats = [floor, H.material_diffuse((0.0, 0.0, 0.0))]
    cam = H.camera((0.1, 4.5, 0.05), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0), 50.0)
    return Case(f"direct_{kind}", _scene("direct_light", mesh, mats, cam, lights), w, h, 0, info={"kind": kind})


TWO_LIGHT_KINDS = ("spot_and_point", "metallic_two_lights", "backface")
SPOT_DIR = np.array([0.2, -1.0, 0.1])          # the way the spot light points
POINT2_LIGHT_POS = np.array([-1.5, 2.5, 1.0])
LIGHT2_COLOR = np.array([0.6, 1.0, 0.7])
LIGHT2_INTENSITY = 3.0
DIRECT_VARIANTS = {"point": ("shadow_below",), "directional": ("shadow_below", "not_negated"),
                   "spot_and_point": ("shadow_below", "spot_plus_direction", "one_occluded_removes_both"),
                   "metallic_two_lights": ("dielectric_on_metal", "spot_plus_direction", "one_occluded_removes_both"),
                   "backface": ("flipped_normal",)}


def _in_square(q, half):
    d = half - np.maximum(np.abs(q[..., 0]), np.abs(q[..., 2]))
    return d > 0, np.abs(d) < SHADOW_MARGIN


def _direct_lights(kind):
    """(type, position, direction, colour, intensity) of the case's lights, in the scene's order."""
    if kind == "point":
        return [("point", POINT_LIGHT_POS, None, LIGHT_COLOR, LIGHT_INTENSITY)]
    if kind == "directional":
        return [("directional", None, DIRECTIONAL_DIR, LIGHT_COLOR, LIGHT_INTENSITY)]
    return [("spot", POINT_LIGHT_POS, SPOT_DIR, LIGHT_COLOR, LIGHT_INTENSITY), ("point", POINT2_LIGHT_POS, None, LIGHT2_COLOR, LIGHT2_INTENSITY)]


def direct_light_eval(case, samples, variant="right", lights=None):
    """-> (per-sample radiance (n, h, w, 3), unsure (n, h, w), shadow segments): step 2 at the floor point of every sample, and the
    number of (sample, light) pairs whose contribution is not zero - the pairs a shadow segment is traced for.  `lights`: the indices
    of the lights that are summed (all of them by default).  Variants:
    "shadow_below": the shadow segment starts at P - N 1e-3 (the floor itself occludes everything); "not_negated": the directional
    light's direction used as it is (N . l < 0: no light); "spot_plus_direction": the spot factor max(dot(+normalize(direction), l), 0)
    (the spot light goes dark); "dielectric_on_metal": albedo / pi on the metallic floor; "one_occluded_removes_both": a sample
    loses all its lights where any one of them is occluded; "flipped_normal": step 2 with the face-forwarded normal (the back face
    is lit like a front face)."""
    kind = case.info["kind"]
    o, d = case.rays(samples)
    n = np.array([0.0, -1.0, 0.0]) if kind == "backface" else np.array([0.0, 1.0, 0.0])
    if variant == "flipped_normal":
        n = -n
    # what the camera ray meets first: the occluder's top (black: 0) or the floor
    tq = (OCCLUDER["y"] - o[1]) / d[..., 1]
    on_occluder, unsure = _in_square(o + d * tq[..., None], OCCLUDER["half"])
    p = o + d * (-o[1] / d[..., 1])[..., None]
    metallic = kind == "metallic_two_lights" and variant != "dielectric_on_metal"
    total = np.zeros(p.shape)
    any_shadowed = np.zeros(p.shape[:-1], bool)
    edge_any = np.zeros(p.shape[:-1], bool)
    segments = 0
    terms = []
    for index, (ltype, pos, direction, colour, power) in enumerate(_direct_lights(kind)):
        if lights is not None and index not in lights:
            continue
        if ltype == "directional":
            l = np.broadcast_to(-_unit(direction), p.shape)
            att = 1.0
            if variant == "not_negated":
                l = -l
        else:
            to_light = pos - p
            dist = np.linalg.norm(to_light, axis=-1)
            l = to_light / dist[..., None]
            with np.errstate(over="ignore"):
                att = (1.0 / (1.0 + dist * dist * 0.01)).astype(np.float16).astype(np.float64)
        intensity = np.maximum(l @ n, 0.0) * power * att
        if ltype == "spot":
            axis = _unit(direction) if variant == "spot_plus_direction" else -_unit(direction)
            intensity = intensity * np.maximum(l @ axis, 0.0)
        brdf = LIT_RHO * 0.5 if metallic else LIT_RHO / math.pi
        lit = brdf * intensity[..., None] * colour
        # shadow segment from P + N eps along l: where it crosses the occluder's plane (always before the light: both are above y = 1)
        org = p + n * ORIGIN_EPS
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (OCCLUDER["y"] - org[..., 1]) / l[..., 1]
            shadowed, edge = _in_square(org + l * s[..., None], OCCLUDER["half"])
        shadowed = shadowed & (s > 0)
        if variant == "shadow_below":
            shadowed = np.ones_like(shadowed)
        gated = (intensity > 0) & ~on_occluder
        segments += int(gated.sum())
        any_shadowed |= shadowed & gated
        edge_any |= edge & gated
        terms.append(np.where(shadowed[..., None], 0.0, lit))
    for term in terms:   # in the lights' order
        total = total + (np.where(any_shadowed[..., None], 0.0, term) if variant == "one_occluded_removes_both" else term)
    rad = 0.1 * LIT_RHO + total
    rad = np.where(on_occluder[..., None], 0.0, rad)
    return rad, unsure | edge_any, segments


def direct_light_expected(case, samples, variant="right"):
    """-> (per-sample radiance (n, h, w, 3), unsure (n, h, w)) of direct_light_eval."""
    return direct_light_eval(case, samples, variant)[:2]


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
# 7. Refraction through the front face, total reflection at the back face
# ------------------------------------------------------------------------------------------------------------------------
GLASS_IOR = 1.5                                   # f16 holds it exactly
DISPERSION = (-0.018, 0.0, 0.035)                 # step 4: ior_c = ior + {-0.018, 0, +0.035}[c]
# ior_c as f32 forms it: f32(1.5) + f32(offset), rounded to f32
IOR_C = np.array([float(np.float32(GLASS_IOR) + np.float32(o)) for o in DISPERSION])
GLASS_Y = 1.0
REFRACT_X0 = 0.65625                              # where the floor's emissive half ends (exact in f32)
REFRACT_MARGIN = 1e-4                             # a segment that lands this close to X0 is not classified (f32 error ~1e-6)
TIR_MARGIN = 1e-5                                 # |ior_c^2 sin^2 - 1| below which the branch is not classified (tir_back)
# the terminal shading of a T = 1 vertex (step 3, the reference's per-channel transmission mix): (0.2, 0.2, 0.3) * (ior_c - 1) / (ior - 1)
GLASS_TERMINAL_MIX = np.array([0.2, 0.2, 0.3]) * (IOR_C - 1.0) / (GLASS_IOR - 1.0)
HERO_F32_REL_BOUND = 6 * U32
"""A path of one transmission that ends on an emitter or the sky is 3 a_c V_c in its hero channel: the throughput 1 * 3 and
(3) * a_c are two roundings, V * throughput one, the sum 0 + x and the division by spp = 1 are exact, and a_c and V_c are each
within 2^-24 of their float64 values as f32: five; six leaves one over."""


def _big_glass_quad(mesh, mat=0):
    # the diagonal a-c passes x = -10 at z = 0, far from both cameras' footprints near the origin: see SHARED EDGES
    _quad(mesh, (-20, GLASS_Y, -20), (20, GLASS_Y, -20), (20, GLASS_Y, 60), (-20, GLASS_Y, 60), mat, (0, 1, 0))


def _glass_t1():
    return H.material_new(tuple(GLASS_A), 0.0, 0.0, (0, 0, 0), GLASS_IOR, 1.0)


def _tilted_camera(position, theta_deg, roll_deg, fov, upward=False):
    """A camera at `position` looking along (sin theta, -+cos theta, 0) - theta from the vertical, down unless `upward` - with an
    up vector perpendicular to that direction, turned by `roll_deg` about it."""
    th, ro = math.radians(theta_deg), math.radians(roll_deg)
    sign = 1.0 if upward else -1.0
    fwd = np.array([math.sin(th), sign * math.cos(th), 0.0])
    up0 = np.array([-sign * math.cos(th), math.sin(th), 0.0])          # perpendicular to fwd, in the plane of incidence
    up = math.cos(ro) * up0 + math.sin(ro) * np.cross(fwd, up0)
    return H.camera(tuple(position), tuple(fwd), tuple(up), fov)


def snell(d, nf, eta):
    """Step 4's transmission direction for an incoming direction d (..., 3) (used as it is, unit or not, as the step does),
    the face-forwarded normal nf and eta (..., ) or scalar: cos i = -nf . d, sin^2 t = eta^2 (1 - cos^2 i);
    sin^2 t > 1: the mirror direction d - 2 (d . nf) nf; else normalize(eta d + (eta cos i - cos t) nf).
    -> (direction (..., 3), total reflection (...,), sin^2 t (...,))."""
    d = np.asarray(d, np.float64)
    eta = np.asarray(eta, np.float64)
    cos_i = -(d @ nf)
    sin2_t = eta * eta * (1.0 - cos_i * cos_i)
    tir = sin2_t > 1.0
    cos_t = np.sqrt(np.where(tir, 0.0, 1.0 - sin2_t))
    refr = d * eta[..., None] + nf * (eta * cos_i - cos_t)[..., None]
    refl = d - 2.0 * (d @ nf)[..., None] * nf
    out = np.where(tir[..., None], refl, refr)
    return out / np.linalg.norm(out, axis=-1, keepdims=True), tir, sin2_t


def refract_front(w=96, h=96):
    """The T = 1 glass quad (albedo a, ior 1.5, no emission) at y = 1 over a floor at y = 0 whose half x < X0 is emissive (albedo 0,
    emission Ef) and whose other half is black; no lights, B = 1; a 2-degree camera looks down at 55 degrees from the vertical,
    toward +x, rolled by 12 degrees about its axis so that the boundary crosses the pixel rows.

    A closed 1-spp frame sends one path through each pixel centre.  The quad adds nothing (no emission, no light).  Step 4 transmits
    (T = 1), picks the hero channel c and leaves throughput 3 a_c e_c; it enters through the front face, so eta = 1 / ior_c, and the
    segment runs from P - N 1e-3 along normalize(eta d + (eta cos i - cos t) N).  The floor is the terminal vertex: Ef + 0.1 * 0 on
    the emissive half, 0 on the black one.  So the pixel is 3 a_c Ef_c in channel c alone if channel c's segment lands at x < X0,
    and 0 otherwise.  At 55 degrees and depth 1 the three channels land 0.0107 (red to green) and 0.0201 (green to blue) apart, the
    frame spans about 0.24 in x on the quad, and the camera is aimed so that the straddling band lies inside the frame.

    Rejects (refract_front_values' variants): no dispersion, eta inverted (ior_c from the front: total reflection, the sky),
    no bending, an origin at P + N 1e-3 (the segment meets the quad again, whose terminal shading is the transmission mix)."""
    mesh = _Mesh()
    _big_glass_quad(mesh)
    z0, z1 = -30.0, 70.0   # the halves' diagonals pass x = -34.5 and x = 15.5 at z = 0
    _quad(mesh, (-50, 0, z0), (REFRACT_X0, 0, z0), (REFRACT_X0, 0, z1), (-50, 0, z1), 1, (0, 1, 0))
    _quad(mesh, (REFRACT_X0, 0, z0), (50, 0, z0), (50, 0, z1), (REFRACT_X0, 0, z1), 2, (0, 1, 0))
    mats = [_glass_t1(), H.material_emissive((0.0, 0.0, 0.0), tuple(FLOOR_E)), H.material_diffuse((0.0, 0.0, 0.0))]
    th = math.radians(55.0)
    aim = np.array([0.01, GLASS_Y, 0.0])   # green lands 0.651 further: the frame's centre is on the straddling band
    pos = aim - 4.0 * np.array([math.sin(th), -math.cos(th), 0.0])
    return Case("refract_front", _scene("refract_front", mesh, mats, _tilted_camera(pos, 55.0, 12.0, 2.0)), w, h, 1)


def refract_front_values(o, d, variant="right"):
    """For rays (origin o (3,) or (..., 3), directions d (..., 3)) that meet the quad of refract_front from above:
    -> (V (..., 3), unsure (..., 3), landing x (..., 3)), V_c the radiance the terminal vertex of a path with hero channel c
    returns (the path's value is 3 a_c V_c in channel c), unsure_c whether channel c's segment lands within REFRACT_MARGIN of X0."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = np.array([0.0, 1.0, 0.0])
    p = o + d * ((GLASS_Y - o[..., 1]) / d[..., 1])[..., None]
    ior = np.full(3, GLASS_IOR) if variant == "no_dispersion" else IOR_C
    v, unsure, land = [], [], []
    for c in range(3):
        eta = ior[c] if variant == "eta_inverted" else 1.0 / ior[c]
        t, tir, _ = snell(d, n, eta)
        if variant == "straight":
            t, tir = d / np.linalg.norm(d, axis=-1, keepdims=True), np.zeros(d.shape[:-1], bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = p[..., 0] + t[..., 0] * (GLASS_Y - ORIGIN_EPS) / -t[..., 1]
        x = np.where(tir, np.inf, x)
        val = np.where(tir, SKY[c], np.where(x < REFRACT_X0, FLOOR_E[c], 0.0))   # a reflected segment leaves for the sky
        if variant == "origin_above":
            val = np.full(x.shape, GLASS_TERMINAL_MIX[c])
        v.append(val)
        unsure.append(np.abs(x - REFRACT_X0) < REFRACT_MARGIN)
        land.append(x)
    return np.stack(v, -1), np.stack(unsure, -1), np.stack(land, -1)


REFRACT_VARIANTS = ("no_dispersion", "eta_inverted", "straight", "origin_above")


def tir_back(w=128, h=64):
    """The same quad seen from below: a camera at y = 0.5 looks up at 41.6 degrees from the vertical with 4 degrees of (vertical)
    field, the plane of incidence vertical in the image, rolled by 10 degrees; an emissive floor (albedo 0, emission Ef) at y = 0, the
    sky above; B = 1.  The frame's incidence angles run from about 38.9 to 44.3 degrees, across the three critical angles
    asin(1 / ior_c) = 42.436, 41.810, 40.652 degrees.

    The quad is met from behind: Nf = -N, eta = ior_c.  With x_c = ior_c^2 sin^2(theta) the hero channel c refracts when x_c <= 1 -
    from P - Nf 1e-3, above the quad, to the sky: 3 a_c sky_c - and is totally reflected when x_c > 1 - from P + Nf 1e-3, below the
    quad, down to the floor, the terminal vertex: 3 a_c Ef_c.  Ef and the sky differ in every channel, so a pixel's value names its
    hero channel and its branch.

    TIR_MARGIN.  f32 forms x_c as eta * eta * (1 - cos_i * cos_i) from the camera direction's y component.  That component is within
    32 * 2^-24 of float64's (CAMERA_DIR_F32_BOUND); cos_i <= 0.78, so cos_i^2 is within 2 * 0.78 * 32 + 1 = 51 units of 2^-24, the
    difference 1 - cos_i^2 (about 0.44) within 52, eta^2 <= 2.36 (ior_c one rounding, the square another: 3 relative, on a product
    of about 1: 3 absolute) and the last product one more: 2.36 * 52 + 4 = 127 units = 7.6e-6 < 1e-5.  With caller-supplied rays
    (rt_radiance) the direction is taken as it is and only the 4 + 2.36 * 2 units of the arithmetic remain.  The margin is a
    condition on what is classified, not a measurement of the code under test.

    Rejects (tir_back_values' variants): no total-reflection branch (the sky everywhere), one critical angle for all channels, a
    reflection that starts on the far side (P - Nf 1e-3: it meets the quad again, whose terminal shading is the transmission mix)."""
    mesh = _Mesh()
    _big_glass_quad(mesh)
    _quad(mesh, (-50, 0, -30), (50, 0, -30), (50, 0, 70), (-50, 0, 70), 1, (0, 1, 0))   # diagonal: x = -20 at z = 0
    mats = [_glass_t1(), H.material_emissive((0.0, 0.0, 0.0), tuple(FLOOR_E))]
    return Case("tir_back", _scene("tir_back", mesh, mats, _tilted_camera((0.0, 0.5, 0.0), 41.6, 10.0, 4.0, upward=True)), w, h, 1)


def tir_back_values(d, variant="right"):
    """For directions d (..., 3) that meet the quad of tir_back from below: -> (V (..., 3), unsure (..., 3), x (..., 3)) as
    refract_front_values, x_c = ior_c^2 (1 - d_y^2)."""
    d = np.asarray(d, np.float64)
    ior = np.full(3, GLASS_IOR) if variant == "one_critical_angle" else IOR_C
    x = ior ** 2 * (1.0 - d[..., 1:2] ** 2)
    reflects = x > 1.0
    if variant == "no_tir_branch":
        reflects = np.zeros_like(reflects)
    below = GLASS_TERMINAL_MIX if variant == "reflect_from_far_side" else FLOOR_E
    return np.where(reflects, below, SKY), np.abs(x - 1.0) < TIR_MARGIN, x


TIR_VARIANTS = ("no_tir_branch", "one_critical_angle", "reflect_from_far_side")


# ------------------------------------------------------------------------------------------------------------------------
# 8. The rough metallic lobe's absorbed cap
# ------------------------------------------------------------------------------------------------------------------------
ROUGH_LAYOUTS = {"front": (0, 1, 0), "backface": (0, -1, 0)}   # the floor's geometric normal; the camera is above it in both
ROUGH_EMPTY_CAP_MARGIN = 1e-5   # the cap counts as empty for c > roughness + this (the f32 lobe's c and |unit vector| are within 1e-6)


def rough_metal(roughness, layout="front", w=64, h=64):
    """A metallic floor (albedo a = MIRROR_A, roughness rho) in the plane y = 0 under the sky, nothing else, B = 1; the camera looks
    down at 65 degrees from the vertical with 40 degrees of field, so c = r . Nf = -d . Nf runs from 0.08 to 0.71 over the frame.
    The floor is ONE triangle, so that no shared edge lies in the footprint (SHARED EDGES).  layout "backface": its geometric normal
    is -y and the camera sees it from behind, so Nf = -N.

    Step 4, metallic: ndir = normalize(r + rho * u), u uniform on the sphere, absorbed if ndir . Nf <= 0.  ndir . Nf has the sign of
    c + rho z with z = u . Nf uniform on [-1, 1] (Archimedes), so the path is absorbed with probability max(0, (1 - c / rho) / 2) -
    the cap - and then traces no continuation segment and returns 0; otherwise its segment leaves upward from P + Nf 1e-3, meets
    nothing and returns a sky.  Every pixel is a sky k / spp with k the number of its samples that continue, the sum of k is the
    frame's continuation-segment count, and k = spp where c > rho for all the pixel's samples (rho = 0.5: the nearer part of the
    frame).

    Rejects: nothing absorbed, the roughness ignored (the cap of rho = 1 at rho = 0.5), a normal that is not face-forwarded (on the
    back face ndir . N > 0 exactly where the lobe should be absorbed)."""
    normal = np.array(ROUGH_LAYOUTS[layout], np.float64)
    a, b, c = np.array([-100.0, 0, -1000.0]), np.array([-100.0, 0, 1000.0]), np.array([2000.0, 0, 0.0])
    if np.dot(np.cross(b - a, c - a), normal) < 0:
        b, c = c, b
    mesh = _Mesh()
    mesh.add([a, b, c], [(0, 1, 2)], 0)
    mats = [H.material_metallic(tuple(MIRROR_A), roughness)]
    cam = _tilted_camera((0.0, 2.0, 0.0), 65.0, 0.0, 40.0)
    return Case(f"rough_metal_{roughness}_{layout}", _scene("rough_metal", mesh, mats, cam), w, h, 1,
                info={"roughness": roughness, "layout": layout})


def rough_cap(c, roughness):
    """The absorbed share of the lobe at c = r . Nf: max(0, (1 - c / roughness) / 2)."""
    return np.maximum(0.0, 0.5 * (1.0 - np.asarray(c, np.float64) / roughness))


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


def check_direct_light(rgb, case, spp, segments=None):
    """Every classified pixel within 2^-10 relative of the float64 restatement (f16 attenuation: 2^-11 on each light's term, so on
    their sum; the f32 chain a few 2^-24); pixels with a sample within SHADOW_MARGIN of the occluder's outline or of one of its
    shadows' are left out, at most 2 % of the frame.  `segments` (the frame's segment counts): the shadow segments are the
    (sample, light) pairs whose contribution is not zero in float64 - one per light and floor sample, none on the black occluder,
    none on a floor that faces away.

    Each named alternative differs from the restatement by more than twice the tolerance on a share of the frame that follows from
    the scene: most of it where the alternative changes every lit pixel, the shadows' area where it changes only those."""
    kind = case.info["kind"]
    rad, unsure, shadow_segments = direct_light_eval(case, np.arange(spp))
    want, unsure = rad.mean(0), unsure.any(0)
    got = np.asarray(rgb, np.float64)
    tol = 2.0 ** -10 * want
    err = np.abs(got - want)
    lit = want[..., 0] > 0.1 * LIT_RHO[0] * (1 + 1e-9)
    floor = want[..., 0] > 0
    print(f"{case.name}: left out {unsure.mean():.4f} (cap {EDGE_SHARE_CAP}), lit pixels {(lit & ~unsure).sum()}, shadowed "
          f"{(floor & ~lit & ~unsure).sum()}, occluder {(~floor).sum()}, "
          f"largest relative error on floor pixels {(err[floor & ~unsure] / want[floor & ~unsure]).max():.3e}, tolerance {2.0 ** -10:.3e}")
    assert unsure.mean() <= EDGE_SHARE_CAP
    if kind == "backface":
        # the ambient term alone: f32(rho) * f32(0.1) summed spp times and divided, (spp + 2) roundings - far below 2^-10
        ambient = 0.1 * LIT_RHO
        exact = (spp + 2) * U32 * ambient
        pure = (np.abs(want - ambient) <= 1e-12).all(-1)   # every sample of the pixel is on the floor
        print(f"  backface: largest |pixel - 0.1 rho| on the {pure.sum()} pixels that are all floor {np.abs(got[pure] - ambient).max(0)}, bound {exact}; "
              f"shadow segments expected {shadow_segments}")
        assert shadow_segments == 0 and pure.mean() > 0.85 and not lit.any()
        assert (np.abs(got[pure] - ambient) <= exact).all() and not got[~floor & ~unsure].any()
    elif len(_direct_lights(kind)) == 1:
        assert (lit & ~unsure).mean() > 0.5 and (floor & ~lit & ~unsure).sum() > 50
    else:   # (the two shadows hardly overlap: what is asserted below is that each light has pixels it lights alone)
        assert (lit & ~unsure).mean() > 0.5
    assert (err[~unsure] <= tol[~unsure]).all()
    if segments is not None:
        print(f"  shadow segments {segments['shadow']}, (sample, light) pairs with a contribution in float64 {shadow_segments}")
        assert segments["shadow"] == shadow_segments
    if len(_direct_lights(kind)) == 2 and kind != "backface":
        # the ordered sum: pixels that keep exactly one of their two lights are in the frame, for either light
        one = [direct_light_eval(case, np.arange(spp), lights=(k,))[0].mean(0) for k in (0, 1)]
        dark = [(np.abs(one[k] - 0.1 * LIT_RHO) <= 1e-12).all(-1) for k in (0, 1)]   # every sample of the pixel lost light k
        only = [dark[1 - k] & ~dark[k] & ~unsure & floor for k in (0, 1)]
        print(f"  pixels lit by the spot light alone {only[0].sum()}, by the second point light alone {only[1].sum()}")
        assert only[0].sum() > 50 and only[1].sum() > 50
    # the wrong alternatives this rejects, each further from `want` than the tolerance on the stated share of the frame
    for variant in DIRECT_VARIANTS[kind]:
        alt = direct_light_eval(case, np.arange(spp), variant)[0].mean(0)
        share = (np.abs(alt - want) > 2 * tol)[~unsure].all(-1).mean()
        least = 0.02 if variant == "one_occluded_removes_both" else 0.5
        print(f"  alternative {variant}: differs by more than twice the tolerance on {share:.3f} of the frame (at least {least})")
        assert share > least


def check_hero_candidates(label, rgb, values, unsure, alternatives, min_differs=200):
    """The shared pixel rule of refract_front and tir_back, for an image or a batch of rays (..., 3): `values[..., c]` is what the
    terminal vertex returns to a path whose hero channel is c, so the path is 3 a_c values_c in channel c alone - one of three
    candidates, the hero pick deciding which.  Asserts, over the pixels none of whose channels is unsure: at most one channel is
    non-zero, and the pixel is one of its candidates within HERO_F32_REL_BOUND (a non-zero channel c needs values_c > 0 and names
    its value; a pixel whose candidates are all non-zero is non-zero; one whose candidates are all 0 is 0).  The share left out is
    at most EDGE_SHARE_CAP.

    `alternatives` (name -> values of a wrong rule): `differs` counts the classified pixels at which the alternative changes at least
    one candidate - it follows from the scene alone and must be at least `min_differs` - and `violations` the pixels of THIS image
    that are none of the alternative's candidates: every pixel of `differs` whose hero channel is a changed one, so about a third
    of `differs` at the least; asserted above a sixth.  -> dict(left_out, violations per alternative)."""
    got = np.asarray(rgb, np.float64)
    sure = ~unsure.any(-1)
    left_out = 1.0 - sure.mean()

    def matches(vals):
        cand = 3.0 * GLASS_A * vals
        ok = np.zeros(got.shape[:-1], bool)
        for c in range(3):
            others = [k for k in range(3) if k != c]
            ok |= (np.abs(got[..., c] - cand[..., c]) <= HERO_F32_REL_BOUND * cand[..., c]) & ~got[..., others].any(-1)
        return ok

    nonzero = (got != 0).sum(-1)
    ok = matches(values)
    lit = (values > 0).sum(-1)
    print(f"{label}: {sure.sum()} of {sure.size} classified, left out {left_out:.4f} (cap {EDGE_SHARE_CAP}); candidates non-zero in "
          f"3 / some / 0 channels: {(sure & (lit == 3)).sum()} / {(sure & (lit > 0) & (lit < 3)).sum()} / {(sure & (lit == 0)).sum()}; "
          f"pixels with more than one channel {(nonzero > 1).sum()}, violations {(sure & ~ok).sum()}")
    assert left_out <= EDGE_SHARE_CAP
    assert (nonzero <= 1).all()
    assert not (sure & ~ok).any()
    score = {}
    for name, alt in alternatives.items():
        differs = int((sure & (np.abs(alt - values) > 1e-3 * np.maximum(values, alt)).any(-1)).sum())
        wrong = int((sure & ~matches(alt)).sum())
        print(f"  alternative {name}: changes a candidate at {differs} classified pixels, {wrong} pixels of this image are none of its candidates")
        assert differs >= min_differs and wrong * 6 >= differs
        score[name] = wrong
    return {"left_out": left_out, "violations": score}


def check_refract_front(rgb, case, spp, segments=None):
    """refract_front's closed form on a closed 1-spp frame (pixel centres); all three classes of pixel are in the frame."""
    assert spp == 1
    o, d = case.centre_rays()
    values, unsure, land = refract_front_values(o, d)
    lit = (values > 0).sum(-1)
    sure = ~unsure.any(-1)
    print(f"{case.name}: landing x red {land[..., 0].min():.4f} .. {land[..., 0].max():.4f}, blue {land[..., 2].min():.4f} .. {land[..., 2].max():.4f}, "
          f"X0 {REFRACT_X0}; mean separation red-green {np.mean(land[..., 0] - land[..., 1]):.5f}, green-blue {np.mean(land[..., 1] - land[..., 2]):.5f}")
    assert min((sure & (lit == 3)).sum(), (sure & (lit == 0)).sum(), (sure & (lit > 0) & (lit < 3)).sum()) >= 500
    if segments is not None:
        assert segments["continuation"] == segments["camera"] == case.w * case.h and segments["shadow"] == 0
    return check_hero_candidates(case.name, rgb, values, unsure, {v: refract_front_values(o, d, v)[0] for v in REFRACT_VARIANTS})


def check_hero_uniform(images, case):
    """Frames of refract_front whose seeds are at least w * h apart (disjoint streams): over the pixels whose three channels all
    land on the emitter, the hero counts are uniform - chi-square with 2 degrees of freedom below chi2_critical(2) (p = 1e-6)."""
    o, d = case.centre_rays()
    values, unsure, _ = refract_front_values(o, d)
    full = (values > 0).all(-1) & ~unsure.any(-1)
    counts = np.zeros(3)
    for rgb in images:
        nz = np.asarray(rgb)[full] != 0
        assert (nz.sum(-1) == 1).all()
        counts += nz.sum(0)
    e = counts.sum() / 3.0
    chi2 = float(((counts - e) ** 2 / e).sum())
    print(f"{case.name}: hero counts {counts.astype(int)} over {len(images)} frames x {full.sum()} fully lit pixels, chi2 {chi2:.2f} "
          f"(critical {chi2_critical(2):.2f})")
    assert counts.sum() >= 10000 and chi2 < chi2_critical(2)


def check_tir_back(rgb, case, spp, segments=None):
    """tir_back's closed form on a closed 1-spp frame; every channel has both branches in the frame."""
    assert spp == 1
    _, d = case.centre_rays()
    values, unsure, x = tir_back_values(d)
    share = (x > 1.0).reshape(-1, 3).mean(0)
    theta = np.degrees(np.arccos(d[..., 1]))
    print(f"{case.name}: incidence {theta.min():.2f} .. {theta.max():.2f} degrees, critical angles {np.degrees(np.arcsin(1.0 / IOR_C))}, "
          f"total-reflection share per channel {share}, pixels inside the margin {unsure.any(-1).sum()}")
    assert (share > 0.1).all() and (share < 0.9).all()
    assert ((np.asarray(rgb) != 0).sum(-1) == 1).all()   # the sky and Ef are positive in every channel: exactly one, the hero
    if segments is not None:
        assert segments["continuation"] == segments["camera"] == case.w * case.h and segments["shadow"] == 0
    return check_hero_candidates(case.name, rgb, values, unsure, {v: tir_back_values(d, v)[0] for v in TIR_VARIANTS})


_ROUGH_CACHE = {}


def rough_metal_moments(case, spp, chunk=64):
    """-> (mean continuing share of the frame's samples, the same with the cap of roughness 1, per-pixel smallest c) for samples
    0 .. spp - 1, c = -d . Nf from each sample's own jittered ray."""
    key = (case.name, case.w, case.h, spp, case.frame_seed)
    if key not in _ROUGH_CACHE:
        rho = case.info["roughness"]
        keep = keep1 = 0.0
        c_min = np.full((case.h, case.w), np.inf)
        for s0 in range(0, spp, chunk):
            _, d = case.rays(np.arange(s0, min(s0 + chunk, spp)))
            c = -d[..., 1]      # the camera is above the floor in both layouts: Nf = +y
            keep += (1.0 - rough_cap(c, rho)).sum()
            keep1 += (1.0 - rough_cap(c, 1.0)).sum()
            c_min = np.minimum(c_min, c.min(0))
        n = case.w * case.h * spp
        _ROUGH_CACHE[key] = (keep / n, keep1 / n, c_min)
    return _ROUGH_CACHE[key]


def check_rough_metal(rgb, case, spp, segments=None):
    """The image mean a sky (1 - cap) within Hoeffding's band (samples in [0, a sky]) plus the f32 slack, the named alternatives at
    least two bands away; and, where the f32 sum still tells k from k + 1 (spp <= 1024): every pixel a sky k / spp for one integer k,
    k = spp where the cap is empty for all the pixel's samples, and sum k = the frame's continuation segments."""
    rho, n = case.info["roughness"], case.w * case.h * spp
    full = MIRROR_A * SKY
    keep, keep_rho1, c_min = rough_metal_moments(case, spp)
    eps = hoeffding_eps(full, n) + f32_mean_slack(full, spp)
    alternatives = {"nothing absorbed": full}
    if rho < 1.0:
        alternatives["roughness ignored (the cap of roughness 1)"] = full * keep_rho1
    if case.info["layout"] == "backface":
        alternatives["normal not face-forwarded"] = full * (1.0 - keep)
    print(f"{case.name}: expected continuing share {keep:.4f}" + (f", measured {segments['continuation'] / n:.4f}" if segments else "")
          + f"; c from {c_min.min():.3f}; pixels with an empty cap {(c_min > rho + ROUGH_EMPTY_CAP_MARGIN).sum()}")
    _assert_mean(case.name, rgb, full * keep, eps, alternatives)
    if spp > 1024:
        return
    got = np.asarray(rgb, np.float64)
    k = np.rint(got[..., 0] * spp / full[0])
    err = np.abs(got - (k / spp)[..., None] * full)
    tol = mirror_f32_rel_bound(spp) * full
    empty = c_min > rho + ROUGH_EMPTY_CAP_MARGIN
    print(f"  largest |pixel - a sky k / spp| {err.max((0, 1))}, tolerance {tol}; sum k {int(k.sum())}; k from {int(k.min())} to {int(k.max())}")
    assert (err <= tol).all()
    assert (k[empty] == spp).all()
    if rho >= 1.0:
        assert not empty.any()
    else:
        assert empty.mean() > 0.2 and (~empty).mean() > 0.2
    if segments is not None:
        assert segments["camera"] == n and segments["shadow"] == 0
        assert int(k.sum()) == segments["continuation"]
