"""The extended mode's estimator against closed-form expectations, on the CPU statement.

Every other test of mode 2 compares the HIP kernels with oracle/rt_oracle.cpp bit for bit; this file asks whether that statement
converges to the right image.  The scenes, their float64 expectations (derived from DESIGN.md section 5, not from the statement),
the bands and the assertions are in estimator_cases.py; test_gpu_estimator.py runs the same assertions on the HIP output.
Seeds are fixed, so nothing here is random from run to run; the bands are nevertheless sized for a failure probability of 1e-9
from bounds that never look at the image.
"""
import numpy as np
import pytest

import estimator_cases as ec


def _render(oracle_mod, case, spp):
    return oracle_mod.render_extended(oracle_mod.PackedScene(case.scene, use_bvh=False), case.w, case.h, spp, case.bounces,
                                      frame_seed=case.frame_seed)


FURNACE_SPP = {b: (64, 64, 4) if b <= 2 else (128, 128, 128) for b in range(9)}
# past the queue pipeline's first read-back of its live paths (after 8 bounce iterations) and its second: the Hoeffding band of
# 128 x 128 x 64 samples bounded by (B + 1) E + 0.1 rho is 0.0067 (B = 9) to 0.019 (B = 24) in blue, ambient and escapes included,
# against a distance of 0.038 to 0.131 to 'paths end at the first poll'; check_furnace asserts the factor of two
FURNACE_SPP.update({b: (128, 128, 64) for b in (9, 12, 16, 17, 24)})


@pytest.mark.parametrize("bounces", list(FURNACE_SPP))
def test_furnace(oracle_mod, bounces):
    """Closed box of one emissive-diffuse material: sum_{k<B} E rho^k + rho^B (E + 0.1 rho).  B <= 2 pixel by pixel, B >= 3
    (russian roulette) as an image mean that the estimator without the division by p misses by at least twice the band, and so
    does, for B > 8, one whose paths end after their ninth vertex.

    The path the B = 2 frame 'loses' (one continuation segment fewer than two per path): a camera ray of pixel (0, 50) meets the
    wall z = 0 at 4.8e-6 from the wall x = 0; its continuation starts 1e-3 off the first wall and reaches the second after less
    than 1e-5, which step 1 does not accept as a hit (MIN_RAY_DISTANCE), so it leaves the box and takes the sky.  That is the
    specified rule, not a defect; estimator_cases.ESCAPE_CAP bounds the share of such segments and the test allows that many
    pixels to be off, and no more missing segments than pixels that are off."""
    w, h, spp = FURNACE_SPP[bounces]
    case = ec.furnace(bounces, w, h)
    out = _render(oracle_mod, case, spp)
    assert out["segments"]["camera"] == w * h * spp
    assert (out["segments"]["roulette"] == 0) == (bounces <= 2)   # roulette acts from the third vertex on, and only there
    ec.check_furnace(out["rgb"], case, spp, out["segments"]["continuation"])


SKY_WALL_SPP = 256


@pytest.mark.parametrize("layout", list(ec.WALL_LAYOUTS))
def test_sky_visibility_past_a_wall(oracle_mod, layout):
    """rho sky (1 - (1 - cos beta) / 2) per sample, beta from the sample's own floor point; a uniform hemisphere is rejected."""
    case = ec.sky_wall(layout)
    ec.check_sky_wall(_render(oracle_mod, case, SKY_WALL_SPP)["rgb"], case, SKY_WALL_SPP)


GLASS_SPP = 256


@pytest.mark.parametrize("transmission", [0.25, 1.0])
def test_transmission_branch(oracle_mod, transmission):
    """(1 - T)(Eg + a sky); exactly 0 at T = 1.  Rejects the inverted branch and a missing (1 - T)."""
    case = ec.glass_over_black_floor(transmission)
    ec.check_glass_black(_render(oracle_mod, case, GLASS_SPP)["rgb"], case, GLASS_SPP)


@pytest.mark.parametrize("which", ["glass_over_emissive_floor", "glass_slab"])
def test_hero_channel(oracle_mod, which):
    """a (Ef + 0.1 rf) through one T = 1 interface, a^2 sky through a closed slab.  Rejects a hero factor of 2 and a pick
    among two channels."""
    case = getattr(ec, which)()
    ec.check_hero(_render(oracle_mod, case, GLASS_SPP)["rgb"], case, GLASS_SPP)


MIRROR_SPP = 4


def test_mirror_and_sampler_tie(oracle_mod):
    """Roughness 0: a sky or 0 per pixel by reflecting each sample's float64 camera ray, at most 2 % of the frame left out.
    The mixed pixels tie the restated sampler (seed rule, SimpleRng, jitter) to the statement: a sky k / spp holds only if the
    statement jitters each sample exactly where the restatement says."""
    case = ec.mirror()
    ec.check_mirror(_render(oracle_mod, case, MIRROR_SPP)["rgb"], case, MIRROR_SPP)


def test_rough_mirror_absorbs_nothing_at_roughness_below_one(oracle_mod):
    """normalize(r + roughness * unit vector) . Nf = (r . Nf + roughness * z) / |..| with |z| <= 1: for roughness 0.3 and the camera's
    r . Nf > 0.7 the absorbed cap (z <= -(r . Nf) / roughness) is empty, so every path continues: one continuation segment per
    path.  (The closed-form cap (1 - c / roughness) / 2 is not empty only for roughness > r . Nf.)"""
    case = ec.mirror(roughness=0.3, w=64, h=64)
    _, d = case.rays(np.arange(4))
    assert (-d[..., 1]).min() > 0.7
    out = _render(oracle_mod, case, 4)
    assert out["segments"]["continuation"] == out["segments"]["camera"] == 64 * 64 * 4


DIRECT_SPP = 4
DIRECT_KINDS = ("point", "directional") + ec.TWO_LIGHT_KINDS


@pytest.mark.parametrize("kind", DIRECT_KINDS)
def test_direct_light_and_hard_shadow(oracle_mod, kind):
    """Step 2 restated in float64 (f16 attenuation included): 2^-10 relative on every classified pixel, at most 2 % left out; one
    shadow segment per (sample, light) pair with a contribution.  Two lights: the spot factor, the metallic BRDF, the ordered sum
    where the occluder hides one light and not the other, and a floor that faces away from both (the ambient term, no segment)."""
    case = ec.direct_light(kind)
    out = _render(oracle_mod, case, DIRECT_SPP)
    ec.check_direct_light(out["rgb"], case, DIRECT_SPP, out["segments"])


HERO_FRAMES = 4


def test_refraction_through_the_front_face(oracle_mod):
    """Snell's direction with eta = 1 / ior_c and the three channels' own indices, from P - N 1e-3: each pixel of a closed 1-spp
    frame is 3 a_c Ef_c or 0 by where ITS channel's segment lands; the hero pick is uniform over frames with disjoint streams."""
    case = ec.refract_front()
    out = _render(oracle_mod, case, 1)
    ec.check_refract_front(out["rgb"], case, 1, out["segments"])
    images = [out["rgb"]]
    for k in range(1, HERO_FRAMES):
        case.frame_seed = k * case.w * case.h
        images.append(_render(oracle_mod, case, 1)["rgb"])
        ec.check_refract_front(images[-1], case, 1)
    ec.check_hero_uniform(images, case)


def test_total_reflection_at_the_back_face(oracle_mod):
    """eta = ior_c from behind: each channel refracts to the sky below its own critical angle and reflects to the floor above it."""
    case = ec.tir_back()
    out = _render(oracle_mod, case, 1)
    ec.check_tir_back(out["rgb"], case, 1, out["segments"])


ROUGH_SPP = 64
ROUGH_CASES = [(1.0, "front"), (0.5, "front"), (1.0, "backface"), (0.5, "backface")]


@pytest.mark.parametrize("roughness,layout", ROUGH_CASES)
def test_rough_metal_absorbs_its_cap(oracle_mod, roughness, layout):
    """a sky (1 - max(0, (1 - c / roughness) / 2)) as an image mean, a sky k / spp pixel by pixel with sum k = the continuation
    segments, k = spp where the cap is empty."""
    case = ec.rough_metal(roughness, layout)
    out = _render(oracle_mod, case, ROUGH_SPP)
    ec.check_rough_metal(out["rgb"], case, ROUGH_SPP, out["segments"])


# ---- the sampler ---------------------------------------------------------------------------------------------------------
SINCOS_MAX_MEASURED = 1.8773e-7       # max |sincos_2pi - float64 sin / cos(2 pi u)| over all 2^24 u
UNIT_NORM_MAX_MEASURED = 2.3129e-7    # max ||unit_vector(u1, u2)| - 1| over the 2^24 pairs below


def test_sincos_2pi_and_unit_vector_over_all_u(oracle_mod):
    """Every u = k / 2^24: the statement's polynomial sin / cos against float64 libm, and the length of unit_vector(u1, u2) with
    u1 a fixed permutation of the same values (k * 2654435761 mod 2^24).  Measured: 1.8773e-7 and 2.3129e-7; asserted at twice
    that (the factor only guards against another libm).  A swap of two quadrants is an error of up to 2."""
    k = np.arange(1 << 24, dtype=np.uint64)
    u2 = (k.astype(np.float64) / (1 << 24)).astype(np.float32)
    u1 = (((k * np.uint64(2654435761)) & np.uint64((1 << 24) - 1)).astype(np.float64) / (1 << 24)).astype(np.float32)
    xyz, sc = oracle_mod.unit_vectors(u1, u2)
    ang = 2.0 * np.pi * u2.astype(np.float64)
    e_sin, e_cos = np.abs(sc[:, 0] - np.sin(ang)).max(), np.abs(sc[:, 1] - np.cos(ang)).max()
    e_norm = np.abs(np.sqrt((xyz.astype(np.float64) ** 2).sum(1)) - 1.0).max()
    e_z = np.abs(xyz[:, 2].astype(np.float64) - (1.0 - 2.0 * u1.astype(np.float64))).max()
    print(f"max error sin {e_sin:.4e}, cos {e_cos:.4e}, |v| - 1 {e_norm:.4e}, z - (1 - 2 u1) {e_z:.4e}")
    assert max(e_sin, e_cos) <= 2 * SINCOS_MAX_MEASURED
    assert e_norm <= 2 * UNIT_NORM_MAX_MEASURED
    assert e_z <= 2.0 ** -23   # z = 1 - 2 u1: one rounding at magnitude <= 1 (uniform in z: Archimedes)


def _chi2(counts):
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


def test_restated_sampler_properties():
    """The restated streams of a 64 x 64 frame, samples 0..255 (2^20 streams; deterministic): range, sub-pixel histogram,
    consecutive-draw pairs, correlation between neighbours.  chi-square critical values at p = 1e-6 by Wilson-Hilferty
    (255 degrees of freedom: 377.2; 1023: 1252.7); correlations against 5 / sqrt(n) (p < 1e-6 for a normal)."""
    w = h = 64
    rng = ec.sample_rng(0, w, h, np.arange(256))
    draws = [rng.next_f32() for _ in range(4)]
    for d in draws:
        assert d.min() >= 0.0 and d.max() < 1.0
    jx, jy, u1, u2 = draws
    c16 = np.histogram2d(jx.ravel(), jy.ravel(), bins=16, range=[[0, 1], [0, 1]])[0]
    c32 = np.histogram2d(u1.ravel(), u2.ravel(), bins=32, range=[[0, 1], [0, 1]])[0]
    crit16, crit32 = ec.chi2_critical(255), ec.chi2_critical(1023)
    print(f"chi2 16x16 jitter {_chi2(c16):.1f} (critical {crit16:.1f}), 32x32 consecutive draws {_chi2(c32):.1f} (critical {crit32:.1f})")
    assert _chi2(c16) < crit16 and _chi2(c32) < crit32

    def corr(a, b):
        return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    pairs = {"horizontal": (jx[:, :, :-1], jx[:, :, 1:]), "vertical": (jy[:, :-1], jy[:, 1:]), "samples s, s+1": (jx[:-1], jx[1:]),
             "jx, jy": (jx, jy)}
    for name, (a, b) in pairs.items():
        r, lim = corr(a, b), 5.0 / np.sqrt(a.size)
        print(f"correlation {name}: {r:+.5f} (limit {lim:.5f})")
        assert abs(r) < lim


BASELINE_FRAMES = {"C0": (256, 256, 1), "C1": (1920, 1080, 64), "C2": (1920, 1080, 16), "headline": (1920, 1080, 64),
                   "C3": (3840, 2160, 256), "C4": (3840, 2160, 64)}


def test_seed_collisions_closed_form_against_brute_force():
    """The closed-form counter against 'hash every (pixel, sample), sort, count equal seeds'.  With the rule's own stride the first
    collision of ANY frame needs W*H*spp of about 2^32 / sqrt(5) = 1.9e9 seeds (0x9E3779B9 / 2^32 is the golden ratio's
    fraction, whose multiples stay 1 / (sqrt(5) ds) away from integers), which cannot be enumerated here: the frames with the real
    stride are collision-free, and the counter's colliding branch is validated with strides that collide early, multiple
    collisions per seed included."""
    for w, h, spp in ((64, 64, 64), (256, 256, 256), (97, 31, 300)):
        assert ec.seed_collisions(w, h, spp)[0] == 0 == ec.seed_collisions_brute_force(w, h, spp, frame_seed=0xDEADBEEF)
    for mult in (0x80000001, 0x55555556, 0xFFFFFF00, 0x00000100, 3):
        for w, h, spp in ((64, 64, 48), (61, 17, 33)):
            want = ec.seed_collisions_brute_force(w, h, spp, mult)
            got, rows = ec.seed_collisions(w, h, spp, mult)
            print(f"stride {mult:#x} {w}x{h} {spp} spp: {got} colliding pairs")
            assert got == want and got > 0


def test_seed_collisions_of_the_baseline_frames():
    """DESIGN section 5, 'Seed collisions': every BASELINE frame but C3 is collision-free; C3 (3840 x 2160, 256 spp) has the 50,847
    pixel pairs at offset 8,243,553 that share the 23 sample pairs 233 apart, and nothing else."""
    for name, (w, h, spp) in BASELINE_FRAMES.items():
        pairs, rows = ec.seed_collisions(w, h, spp)
        if name == "C3":
            assert rows == [(233, 8243553, 50847, 23)] and pairs == 50847 * 23
        else:
            assert pairs == 0, name
    assert ec.seed_collisions(1920, 1080, 1024)[1] == [(987, 1946557, 1920 * 1080 - 1946557, 37)]
    # the smallest offsets below 64 spp, which the envelope W*H < 34,920,769 rests on
    ds = np.arange(1, 64, dtype=np.uint64)
    off = (ds * np.uint64(ec.GOLDEN)) & np.uint64(0xFFFFFFFF)
    mag = np.minimum(off, np.uint64(1 << 32) - off)
    assert int(mag.min()) == 34920769 and int(ds[np.argmin(mag)]) == 55


def test_frame_seed_plus_one_shifts_the_streams_by_one_pixel():
    a = ec.hash_u32(ec.seed_inputs(7, 32, 8, np.arange(4))).reshape(4, -1)
    b = ec.hash_u32(ec.seed_inputs(8, 32, 8, np.arange(4))).reshape(4, -1)
    np.testing.assert_array_equal(b[:, :-1], a[:, 1:])
